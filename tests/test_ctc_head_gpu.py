"""GPU tests of the logit-free CTC loss on the head: the VASR_EPI_LSE GEMM epilogue + combine
(ops.gemm_lse), the target logits without the logits (ops.ctc_head_emissions), the in-place logit
gradient from saved statistics (ops.ctc_grad_logits_stats) and their users CTCOutputHead.ctc_emissions
/ align, training.CTCHeadLoss and VELOCITYASR.ctc_loss.  Inputs and fp64 references: ctc_head_cases.py.

Tolerances ("The loss on the head" has the derivations and the measured uses):
  lse       |lse - lse64(device logits)| <= 4 max(e_unfused, 2^-23 max(1, |lse|)), e_unfused the
            existing ops.ctc_emissions path's error against the same fp64 value, measured here;
  emission  per row against fp64 of the inputs: 2 delta_row + 8 * 2^-23 max |logit|,
            delta_row = 2^-20 max_j (|a| . |w_j| + |b_j|) (the tile GEMM's own rule); the unfused
            device path must meet the same bound;
  nll       per utterance: frames_b * (emission bound) + 1.63e-6 |nll|; the two device paths agree with
            each other within twice its first, emission-derived term (they share the lattice kernel);
  gradient  e = max |got - fp64| / max |fp64| for each of dX, dW, db: e_hip <= max(FACTOR e_ref, 1e-6),
            e_ref the same quantity of torch CPU fp32 autograd of F.linear -> F.log_softmax ->
            nn.CTCLoss, computed here; FACTOR = 4 (test_ctc_grad_gpu.py's convention).
"""

import functools

import numpy as np
import pytest
import torch

import ctc_head_cases as H
from conftest import record_metric
from velocity_asr import _lib, ops
from velocity_asr.decode import ctc_forced_align
from velocity_asr.model import CTCOutputHead
from velocity_asr.training import CTCHeadLoss, CTCLoss

pytestmark = pytest.mark.gpu
DEV = "cuda"
EPS = H.EPS
FACTOR = 4.0

LOSS_CASES = ["l1_s0", "l1_s1", "l7_repeat", "l33_v29", "l129_v1001", "s63", "s64", "s130", "ragged", "infeasible",
              "flat_targets", "pm80", "v50000", "l501_v1000"]
GRAD_CASES = [n for n in LOSS_CASES if n not in ("v50000", "l501_v1000")] + ["s280"]


# ------------------------------------------------------------------ the epilogue alone

def _lse_inputs(M, V, K, seed):
    g = torch.Generator().manual_seed(seed)
    a = torch.nn.functional.layer_norm(torch.randn(M, K, generator=g), (K,))
    w = 0.3 * torch.randn(V, K, generator=g)
    b = 0.5 * torch.randn(V, generator=g)
    if V > 1:
        b[V - 1] = float("-inf")  # a masked token
    r = M // 2  # one row with |logit| about 80
    a[r] *= 80.0 / float((a[r].double() @ w.double().T).abs().max())
    return a.to(DEV), w.to(DEV), b.to(DEV)


def _check_lse(M, V, K, seed=0):
    a, w, b = _lse_inputs(M, V, K, seed)
    slots = (V + 31) // 32
    logits = ops.gemm(a, w, b)
    pairs = torch.full((M, slots + 2, 2), float("nan"), device=DEV)
    stats = ops.gemm_lse(a, w, b, pairs=pairs)
    assert tuple(stats.shape) == (M, 2) and torch.equal(stats, ops.gemm_lse(a, w, b))
    # the write footprint: every used slot finite or the neutral pair, the spare columns untouched
    used, spare = pairs[:, :slots], pairs[:, slots:]
    neutral = torch.isinf(used[..., 0]) & (used[..., 0] < 0) & (used[..., 1] == 0)
    assert bool((torch.isfinite(used).all(-1) | neutral).all()) and bool(torch.isnan(spare).all())
    # the accumulator does not depend on the epilogue: the maximum is the logits' own
    assert torch.equal(stats[:, 0], logits.max(-1).values)
    x = logits.double()
    Ms, lse = stats[:, 0].double(), stats[:, 1]
    lse64 = torch.log(torch.exp(x - Ms[:, None]).sum(-1))
    # the unfused path's log-sum-exp as its blank emission carries it: e0 = (x0 - Ms) - lse
    emis, *_ = ops.ctc_emissions(logits.view(1, M, V), torch.zeros((1, 0), dtype=torch.int32, device=DEV))
    e_unfused = (((x[:, 0] - Ms) - emis[0, :, 0].double()) - lse64).abs()
    e_fused = (lse.double() - lse64).abs()
    bound = 4.0 * torch.maximum(e_unfused, EPS * lse64.abs().clamp(min=1.0))
    use = float((e_fused / bound).max())
    record_metric("ctc_head_lse", M=M, V=V, K=K, use=use, e_fused=float(e_fused.max()), e_unfused=float(e_unfused.max()))
    print(f"lse M={M} V={V} K={K}: e_fused {float(e_fused.max()):.3e} e_unfused {float(e_unfused.max()):.3e} use {use:.3f}")
    assert bool((e_fused <= bound).all()), (M, V, K, use)


@pytest.mark.parametrize("K", [36, 192])
@pytest.mark.parametrize("V", [1, 5, 31, 32, 33, 65, 1000, 1025])
def test_lse_epilogue(V, K):
    for M in (1, 33, 130, 300):
        assert ops.gemm_tile(M, V, K, epilogue=_lib.EPI_LSE) == 64064
        _check_lse(M, V, K, seed=1000 * K + V + M)


@pytest.mark.parametrize("M,V,K,tile", [(2881, 1000, 192, 128064), (7777, 1000, 100, 128128)])
def test_lse_epilogue_on_the_large_tiles(M, V, K, tile):
    assert ops.gemm_tile(M, V, K, epilogue=_lib.EPI_LSE) == tile
    assert ops.gemm_tile(M, V, K) == tile  # the comparison GEMM runs the same accumulation
    _check_lse(M, V, K, seed=M)


@pytest.mark.parametrize("M,V,K,engine", [(4100, 1000, 192, 0), (4224, 544, 192, 0), (130, 65, 192, 2), (33, 1025, 128, 2)])
def test_lse_epilogue_on_the_rows_engine(M, V, K, engine):
    """Where the plain head GEMM runs on the rows engine (automatically from 4096 rows and 512
    columns at K = 192; anywhere at K <= 192 when the engine option forces it) the log-sum-exp GEMM
    does too: a ragged last row block, a ragged last 32-column chunk, one chunk per group, Kp = 128."""
    with ops.option(_lib.OPT_GEMM_ENGINE, engine):
        assert ops.gemm_tile(M, V, K, epilogue=_lib.EPI_LSE) == 1 and ops.gemm_tile(M, V, K) == 1
        _check_lse(M, V, K, seed=M + V)


def test_lse_of_a_row_of_minus_infinity():
    a, w, _ = _lse_inputs(33, 5, 36, 7)
    b = torch.full((5,), float("-inf"), device=DEV)
    stats = ops.gemm_lse(a, w, b)
    assert not stats.isnan().any() and not stats[:, 0].any() and bool((stats[:, 1] == float("-inf")).all())


def test_lse_refuses_bf16_weights():
    a, w, b = _lse_inputs(33, 65, 36, 8)
    with pytest.raises(TypeError, match="float32"):
        ops.gemm_lse(a, w.bfloat16(), b)


# ------------------------------------------------------------------ emissions and loss

@functools.lru_cache(maxsize=None)
def _dev(name):
    """A case on the device, made once (nothing below changes it in place)."""
    c, xn, W, b, tg, ilen, tlen = H.head_case(name)
    return c, xn.to(DEV), W.to(DEV), b.to(DEV), tg.to(DEV), ilen.to(DEV), tlen.to(DEV)


@functools.lru_cache(maxsize=None)
def _head(name, dropout=0.0):
    c, xn, W, b, *_ = _dev(name)
    head = CTCOutputHead(d_model=xn.shape[-1], vocab_size=c["V"], dropout=dropout)
    with torch.no_grad():
        head.proj[2].weight.copy_(W)
        head.proj[2].bias.copy_(b)
    return head.to(DEV).eval()


def _emission_use(name, emis):
    """max over the specified entries of |emis - fp64| / the row's bound."""
    want, rb = H.emissions_f64(name), H.row_bounds(name)
    got = emis.double().cpu().numpy()
    spec = ~np.isnan(want)
    assert np.isfinite(got[spec]).all()
    return float((np.abs(got - np.where(spec, want, 0.0)) / rb[..., None])[spec].max())


@pytest.mark.parametrize("name", LOSS_CASES)
def test_emissions_and_nll_match_fp64(name):
    c, xn, W, b, tg, ilen, tlen = _dev(name)
    B, Lq, K = xn.shape
    emis, stats, tg32, fr, tl = ops.ctc_head_emissions(xn.view(B * Lq, K), W, b, tg, ilen, tlen, B=B)
    assert tuple(emis.shape) == (B, Lq, c["S"] + 1) and tuple(stats.shape) == (B * Lq, 2)
    logits = ops.gemm(xn.view(B * Lq, K), W, b).view(B, Lq, c["V"])
    emis_u, *_ = ops.ctc_emissions(logits, tg, ilen, tlen)
    use_f, use_u = _emission_use(name, emis), _emission_use(name, emis_u)
    record_metric("ctc_head_emission_use", case=name, fused=use_f, unfused=use_u)
    print(f"{name}: emission bound use fused {use_f:.3f} unfused {use_u:.3f}")
    assert use_u <= 1.0 and use_f <= 1.0, (name, use_f, use_u)
    want, nb = H.nll_f64(name), H.nll_bounds(name)
    for tag, e in (("fused", emis), ("unfused", emis_u)):
        nll = ops.ctc_loss(e, tg32, fr, tl).double().cpu().numpy()
        fin = np.isfinite(want)
        assert np.array_equal(np.isposinf(nll), ~fin), (name, tag)
        use = float((np.abs(nll - want)[fin] / nb[fin]).max(initial=0.0))
        record_metric("ctc_head_nll_use", case=name, path=tag, use=use)
        print(f"{name}: nll bound use {tag} {use:.3f}")
        assert use <= 1.0, (name, tag, use)


def test_emission_of_a_token_outside_the_vocabulary_and_padding_rows():
    c, xn, W, b, tg, ilen, tlen = _dev("ragged")
    B, Lq, K = xn.shape
    clean, *_ = ops.ctc_head_emissions(xn.view(-1, K), W, b, tg, ilen, tlen, B=B)
    bad_x, bad_tg = xn.clone(), tg.clone()
    for i in range(B):
        bad_x[i, int(ilen[i]):] = float("nan")
    bad_tg[0, 2], bad_tg[2, 0] = c["V"], -1
    got, *_ = ops.ctc_head_emissions(bad_x.view(-1, K), W, b, bad_tg, ilen, tlen, B=B)
    for i in range(B):
        T, n = int(ilen[i]), int(tlen[i])
        keep = torch.ones(n + 1, dtype=torch.bool, device=DEV)
        if i == 0:
            keep[3] = False
            assert bool((got[0, :T, 3] == float("-inf")).all())
        if i == 2:
            keep[1] = False
            assert bool((got[2, :T, 1] == float("-inf")).all())
        assert torch.equal(got[i, :T, :n + 1][:, keep], clean[i, :T, :n + 1][:, keep])


def _reduced_bound(name, reduction):
    """The emission-derived nll bound (no lattice term: both paths run the same lattice), reduced."""
    c, *_, tlen = H.head_case(name)
    nb = H.nll_bounds(name, lattice=False)
    if reduction == "none":
        return nb
    return nb.sum() if reduction == "sum" else (nb / np.maximum(tlen.numpy(), 1)).mean()


@pytest.mark.parametrize("name", ["l33_v29", "ragged", "infeasible", "flat_targets"])
def test_head_loss_fused_and_unfused_agree(name):
    c, xn, W, b, tg, ilen, tlen = _dev(name)
    head = _head(name)
    if c.get("flat"):
        tg = torch.from_numpy(H.G.flat_targets(c, tg.cpu().numpy(), tlen.cpu().numpy())).to(DEV)
    for reduction in ("none", "sum", "mean"):
        for zi in (True, False):
            f = CTCHeadLoss(head, reduction=reduction, zero_infinity=zi, fused=True)(xn, tg, ilen, tlen, normalized=True)
            u = CTCHeadLoss(head, reduction=reduction, zero_infinity=zi, fused=False)(xn, tg, ilen, tlen, normalized=True)
            f, u = f.double().cpu().numpy(), u.double().cpu().numpy()
            if name == "infeasible":
                first = f[0] if reduction == "none" else f
                assert first == 0.0 if zi and reduction == "none" else np.isfinite(first) if zi else np.isposinf(first)
            assert np.array_equal(np.isfinite(f), np.isfinite(u))
            fin = np.isfinite(f)
            bound = np.broadcast_to(2.0 * _reduced_bound(name, reduction), f.shape)
            assert (np.abs(f - u)[fin] <= bound[fin]).all(), (name, reduction, zi)


@pytest.mark.parametrize("name", ["l33_v29", "ragged"])
def test_align_is_the_forced_alignment_of_the_logits(name):
    c, xn, W, b, tg, ilen, tlen = _dev(name)
    head = _head(name)
    got = head.align(xn, tg, ilen, tlen, normalized=True)
    want = ctc_forced_align(head(xn, normalized=True), tg, ilen, tlen)
    nb = H.nll_bounds(name)
    for i, ((s0, spans0, st0), (s1, spans1, st1)) in enumerate(zip(got, want)):
        assert spans0 == spans1 and st0 == st1
        assert abs(s0 - s1) <= nb[i]


@pytest.mark.parametrize("ragged", [False, True])
@pytest.mark.parametrize("tail", ["1", "0"])
def test_model_ctc_loss(default_weights, monkeypatch, tail, ragged):
    """VELOCITYASR.ctc_loss = CTCLoss()(model(mel)) on the synthetic default model, B = 3 short clips,
    with the logit-free path forced (the default rule would send V = 1000 through the logits)."""
    import velocity_asr as va
    from velocity_asr import synthetic as S
    monkeypatch.setenv("VASR_FUSION_TAIL", tail)
    m = va.VELOCITYASR()
    m.load_state_dict({k: torch.from_numpy(v) for k, v in default_weights.items()}, strict=True)
    m = m.to(DEV).eval()
    mel = va.compute_mel_spectrogram(torch.from_numpy(S.make_audio(3, 16000, seed=21)).to(DEV))
    frames = [mel.shape[1], 61, 80] if ragged else None
    if ragged:
        for i, f in enumerate(frames):
            mel[i, f:] = 0
    Lq = m.get_output_length(mel.shape[1])
    ilen = torch.tensor([m.get_output_length(f) for f in frames] if ragged else [Lq] * 3)
    V = m.config.vocab_size
    tg = torch.from_numpy(np.random.RandomState(4).randint(1, V, size=(3, 6)))
    tlen = torch.tensor([6, 3, 5])
    logits = m(mel, frames=frames)
    # the emission bound from the logits' own scale: |a| . |w_j| + |b_j| <= sqrt(K) ||w_j|| max|xn| + |b_j|
    w, b = m.ctc_head.proj[2].weight.detach().double(), m.ctc_head.proj[2].bias.detach().double()
    with torch.no_grad():
        _, x, normalized = m._local_global(mel, m._token_lengths(frames, mel.shape[1]))
        xn = (x if normalized else m.ctc_head.proj[0](x)).double()
    mag = (xn.abs().reshape(-1, xn.shape[-1]) @ w.abs().T + b.abs()).max(-1).values.view(3, Lq)
    rb = 2.0 * 2.0 ** -20 * mag + 8.0 * EPS * logits.double().abs().max(-1).values
    for reduction in ("none", "mean"):
        want = CTCLoss(reduction=reduction)(logits, tg, ilen, tlen).double().cpu()
        for min_vocab in (0, 1 << 30):  # fused, then the default rule's choice at V = 1000
            monkeypatch.setattr(CTCHeadLoss, "FUSED_MIN_VOCAB", min_vocab)
            got = m.ctc_loss(mel, tg, ilen, tlen, reduction=reduction, frames=frames).double().cpu()
            nb = torch.stack([int(ilen[i]) * rb[i, :int(ilen[i])].max() for i in range(3)]).cpu()
            bound = 2.0 * (nb if reduction == "none" else (nb / tlen.clamp(min=1)).mean())
            assert bool(((got - want).abs() <= bound).all()), (reduction, min_vocab, got, want, bound)
            if min_vocab:
                assert torch.equal(got, want)


# ------------------------------------------------------------------ gradient

@functools.lru_cache(maxsize=None)
def _e_ref(name, reduction, zi=True):
    want = H.grads_f64(name, reduction, zi)
    ref = H.reference_grads(name, torch.float32, reduction, zi)[1:]
    return tuple(H.rel_err(np.nan_to_num(r), np.nan_to_num(w)) for r, w in zip(ref, want))


def _backward(name, reduction="none", zi=True, fused=True, chunk_bytes=256 << 20, xn=None):
    """(loss, dX, dW, db) through CTCHeadLoss(differentiable=True) on the case's head."""
    c, x0, W, b, tg, ilen, tlen = _dev(name)
    head = _head(name)
    x = (x0 if xn is None else xn).detach().clone().requires_grad_(True)
    for p in head.parameters():
        p.grad = None
    loss = CTCHeadLoss(head, reduction=reduction, zero_infinity=zi, differentiable=True, fused=fused,
                       chunk_bytes=chunk_bytes)(x, tg, ilen, tlen, normalized=True)
    loss.backward(torch.ones_like(loss))
    lin = head.proj[2]
    return loss.detach(), x.grad, lin.weight.grad.clone(), lin.bias.grad.clone()


def _errs(name, reduction, got, zi=True):
    want = H.grads_f64(name, reduction, zi)
    return tuple(H.rel_err(g.double().cpu().numpy().reshape(w.shape), w) for g, w in zip(got, want))


@pytest.mark.parametrize("reduction", ["none", "mean"])
@pytest.mark.parametrize("name", GRAD_CASES)
def test_gradient_matches_fp64(name, reduction):
    c, xn, W, b, tg, ilen, tlen = _dev(name)
    loss, *grads = _backward(name, reduction)
    # the value is the forward-only fused path's, bitwise
    assert torch.equal(loss, CTCHeadLoss(_head(name), reduction=reduction, fused=True)(xn, tg, ilen, tlen, normalized=True))
    assert all(bool(torch.isfinite(g).all()) for g in grads)
    e_ref, e_hip = _e_ref(name, reduction), _errs(name, reduction, grads)
    e_unf = _errs(name, reduction, _backward(name, reduction, fused=False)[1:])
    for what, r, h, u in zip(("dX", "dW", "db"), e_ref, e_hip, e_unf):
        bound = max(FACTOR * r, 1e-6)
        record_metric("ctc_head_grad", case=name, reduction=reduction, what=what, e_ref=r, e_hip=h, e_unfused=u, bound=bound)
        print(f"{name} {reduction} {what}: e_ref {r:.3e} e_hip {h:.3e} e_unfused {u:.3e} bound {bound:.3e}")
    for what, r, h in zip(("dX", "dW", "db"), e_ref, e_hip):
        assert h <= max(FACTOR * r, 1e-6), (name, reduction, what, h, r)
    for i in range(c["B"]):  # padding rows: exact zeros
        assert not grads[0][i, int(ilen[i]):].any()


@pytest.mark.parametrize("name", ["ragged", "l33_v29"])
def test_chunked_backward(name):
    """One utterance per chunk against one chunk for the batch: same loss bitwise, and every gradient
    within the tolerance of the fp64 one (the chunk GEMMs of dX = G W are torch.mm calls whose kernel
    may change with the row count, so bitwise equality of dX is recorded, not required)."""
    c, xn, *_ = _dev(name)
    whole = _backward(name, "mean")
    parts = _backward(name, "mean", chunk_bytes=c["L"] * c["V"] * 4)
    assert torch.equal(whole[0], parts[0])
    record_metric("ctc_head_chunk_bitwise", case=name, dX=bool(torch.equal(whole[1], parts[1])),
                  dW=bool(torch.equal(whole[2], parts[2])), db=bool(torch.equal(whole[3], parts[3])))
    print(f"{name}: chunked bitwise dX {torch.equal(whole[1], parts[1])} dW {torch.equal(whole[2], parts[2])}")
    for r, h in zip(_e_ref(name, "mean"), _errs(name, "mean", parts[1:])):
        assert h <= max(FACTOR * r, 1e-6)
    tiny = _backward(name, "mean", chunk_bytes=1)  # below one utterance: still one utterance per chunk
    assert all(torch.equal(a, b) for a, b in zip(parts, tiny))


def test_padding_rows_never_reach_the_gradient():
    c, xn, W, b, tg, ilen, tlen = _dev("ragged")
    bad = xn.clone()
    for i in range(c["B"]):
        bad[i, int(ilen[i]):] = float("nan")
    for chunk in (256 << 20, c["L"] * c["V"] * 4):
        clean = _backward("ragged", "mean", chunk_bytes=chunk)
        got = _backward("ragged", "mean", chunk_bytes=chunk, xn=bad)
        assert all(bool(torch.isfinite(g).all()) for g in got)
        assert all(torch.equal(a, b) for a, b in zip(got, clean))
        for i in range(c["B"]):
            assert not got[1][i, int(ilen[i]):].any() and got[1][i, :int(ilen[i])].any()


def test_infeasible_utterance():
    c, xn, W, b, tg, ilen, tlen = _dev("infeasible")
    loss, dx, dw, db = _backward("infeasible", "none", zi=True)
    assert bool(torch.isfinite(loss).all()) and not dx[0].any() and dx[1].any()
    for r, h in zip(_e_ref("infeasible", "none"), _errs("infeasible", "none", (dx, dw, db))):
        assert h <= max(FACTOR * r, 1e-6)
    loss, rx, rw, rb = _backward("infeasible", "none", zi=False)
    assert bool(torch.isinf(loss[0])) and bool(torch.isnan(rx[0, :int(ilen[0])]).all())
    assert torch.equal(rx[1], dx[1])  # the neighbour's rows are unaffected
    assert not rx[0, int(ilen[0]):].any()


def test_gradients_through_the_modules():
    """features -> LayerNorm -> Dropout(0) -> fused loss in train(): gradients reach the features, both
    LayerNorm parameters, W and b, and match the unfused module path (torch Linear + CTCLoss)."""
    name = "l33_v29"
    c, xn, W, b, tg, ilen, tlen = _dev(name)
    head = CTCOutputHead(d_model=192, vocab_size=c["V"], dropout=0.0).to(DEV)
    with torch.no_grad():
        head.proj[2].weight.copy_(W)
        head.proj[2].bias.copy_(b)
        head.proj[0].weight.copy_(1 + 0.2 * torch.randn(192, device=DEV, generator=torch.Generator(DEV).manual_seed(1)))
        head.proj[0].bias.copy_(0.2 * torch.randn(192, device=DEV, generator=torch.Generator(DEV).manual_seed(2)))
    head.train()
    rows = 2.0 * torch.randn(xn.shape, device=DEV, generator=torch.Generator(DEV).manual_seed(3)) + 0.5

    def run(fused):
        x = rows.clone().requires_grad_(True)
        head.zero_grad(set_to_none=True)
        loss = CTCHeadLoss(head, differentiable=True, fused=fused)(x, tg, ilen, tlen)
        loss.backward()
        ps = [head.proj[0].weight, head.proj[0].bias, head.proj[2].weight, head.proj[2].bias]
        assert all(p.grad is not None for p in ps)
        return [loss.detach(), x.grad] + [p.grad.clone() for p in ps]

    def compose(dtype):
        """torch CPU autograd of LayerNorm -> Linear -> log_softmax -> nn.CTCLoss (mean) in dtype."""
        leaves = [t.detach().to(device="cpu", dtype=dtype).requires_grad_(True) for t in
                  (rows, head.proj[0].weight, head.proj[0].bias, head.proj[2].weight, head.proj[2].bias)]
        xr, ln_w, ln_b, w_, b_ = leaves
        lp = torch.nn.functional.log_softmax(torch.nn.functional.linear(
            torch.nn.functional.layer_norm(xr, (192,), ln_w, ln_b, head.proj[0].eps), w_, b_), -1)
        nll = torch.nn.CTCLoss(reduction="none", zero_infinity=True)(lp.transpose(0, 1), tg.cpu(), ilen.cpu(), tlen.cpu())
        (nll / tlen.cpu().clamp(min=1).to(dtype)).mean().backward()
        return [t.grad.double().numpy() for t in leaves]

    f, u = run(True), run(False)
    want, ref = compose(torch.float64), compose(torch.float32)
    for what, a, b_, w_, r_ in zip(("dfeatures", "dln_w", "dln_b", "dW", "db"), f[1:], u[1:], want, ref):
        ef, eu = H.rel_err(a.double().cpu().numpy(), w_), H.rel_err(b_.double().cpu().numpy(), w_)
        e_ref = H.rel_err(r_, w_)
        record_metric("ctc_head_module_grad", what=what, e_fused=ef, e_unfused=eu, e_ref=e_ref)
        print(f"modules {what}: e_ref {e_ref:.3e} e_fused {ef:.3e} e_unfused {eu:.3e}")
        assert ef <= max(FACTOR * e_ref, 1e-6), (what, ef, e_ref)


def test_dropout_runs_and_repeats_under_a_seed():
    c, xn, W, b, tg, ilen, tlen = _dev("l33_v29")
    head = CTCOutputHead(d_model=192, vocab_size=c["V"], dropout=0.1).to(DEV).train()
    outs = []
    for _ in range(2):
        torch.manual_seed(11)
        x = xn.clone().requires_grad_(True)
        head.zero_grad(set_to_none=True)
        loss = CTCHeadLoss(head, differentiable=True)(x, tg, ilen, tlen)
        loss.backward()
        outs.append((loss.detach(), x.grad, head.proj[2].weight.grad.clone()))
    assert all(torch.equal(a, b) for a, b in zip(*outs)) and bool(torch.isfinite(outs[0][1]).all())


# ------------------------------------------------------------------ memory (conditions, not measurements)

def _peak_over(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out = fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    del out
    return peak


def test_forward_memory_does_not_grow_with_the_logits():
    c, xn, W, b, tg, ilen, tlen = _dev("v50000")
    head = _head("v50000")
    full = c["B"] * c["L"] * c["V"] * 4
    fused = CTCHeadLoss(head, fused=True)
    unfused = CTCHeadLoss(head, fused=False)
    for loss in (fused, unfused):  # warm-up: the split weight planes are cached per parameter version
        loss(xn, tg, ilen, tlen, normalized=True)
    pf = _peak_over(lambda: fused(xn, tg, ilen, tlen, normalized=True))
    pu = _peak_over(lambda: unfused(xn, tg, ilen, tlen, normalized=True))
    record_metric("ctc_head_forward_memory", logits_bytes=full, fused=pf, unfused=pu)
    print(f"forward peak: fused {pf} unfused {pu} logits {full}")
    assert pu >= full, "the measurement does not see the logits"
    assert pf < full // 4, (pf, full)


def test_backward_memory_is_bounded_by_the_chunk():
    B, Lq, V, S, K = 16, 128, 4096, 16, 192
    g = torch.Generator().manual_seed(5)
    xn = torch.nn.functional.layer_norm(torch.randn(B, Lq, K, generator=g), (K,)).to(DEV)
    head = CTCOutputHead(d_model=K, vocab_size=V, dropout=0.0).to(DEV).eval()
    with torch.no_grad():
        head.proj[2].weight.copy_(0.3 * torch.randn(V, K, generator=g))
        head.proj[2].bias.copy_(0.5 * torch.randn(V, generator=g))
    tg = torch.from_numpy(np.random.RandomState(6).randint(1, V, size=(B, S))).to(DEV)
    ilen, tlen = torch.full((B,), Lq, device=DEV), torch.full((B,), S, device=DEV)
    full = B * Lq * V * 4
    loss = CTCHeadLoss(head, differentiable=True, fused=True, chunk_bytes=full // 8)

    def step():
        x = xn.clone().requires_grad_(True)
        head.zero_grad(set_to_none=True)
        loss(x, tg, ilen, tlen, normalized=True).backward()
        return x.grad

    step()  # warm-up: weight planes, the BLAS library's workspace
    head.zero_grad(set_to_none=True)
    peak = _peak_over(step)
    record_metric("ctc_head_backward_memory", logits_bytes=full, peak=peak)
    print(f"backward peak {peak} of logits {full}")
    assert peak < full // 2, (peak, full)
