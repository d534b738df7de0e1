"""GPU tests of the greedy decode with confidences: the VASR_EPI_ARGMAX_LSE GEMM epilogue, the frame
log-probability from it and from logits (vasr_argmax_logp_f32), the scored collapses
(vasr_ctc_collapse_conf, vasr_ctc_collapse_keys_conf) and their users CTCOutputHead / VELOCITYASR
.greedy_scored, decode.ctc_greedy_decode_with_confidence and transcribe_files(confidence=True).
Host references: greedy_conf_cases.py.

Tolerances:
  keys, pairs  bitwise the VASR_EPI_ARGMAX / VASR_EPI_LSE GEMM's on the same kernel;
  frame lp     per row against fp64 log_softmax(a W^T + b) at the kernel's own argmax:
               2 delta_row + 8 * 2^-23 max |logit|, delta_row = 2^-20 max_j (|a| . |w_j| + |b_j|)
               (ctc_head_cases.row_bounds' rule);
  logp_min     exact (a selection); tokens, lengths, spans bitwise ops.ctc_collapse's;
  sums         |sum - fp64 sum| <= n * 2^-23 * sum |lp| over the n terms (the fp32 summation bound of any
               association), against fp64 sums of the same fp32 lp;
  path_logp    at model level: frames_b * (the largest row bound) against fp64 from the head's fp32 input.
"""

import functools

import numpy as np
import pytest
import torch

import greedy_conf_cases as C
from conftest import record_error
from velocity_asr import _lib, ops
from velocity_asr import synthetic as S

pytestmark = pytest.mark.gpu
DEV = "cuda"
EPS = C.EPS
NAN = float("nan")


# ------------------------------------------------------------------ the epilogue

SHAPES = [(1, 5, 36), (33, 64, 128), (300, 1000, 192), (129, 1001, 192), (2881, 1000, 192)]


@functools.lru_cache(maxsize=None)
def _operands(M, N, K, variant):
    """Host float32 (a, w, b or None).  variant: bias, nobias, inf (-inf bias on a quarter of the
    columns), tie (every odd W row and bias entry repeats the one before: exact ties of two columns)."""
    g = torch.Generator().manual_seed(1000 * M + 10 * N + K)
    a = torch.nn.functional.layer_norm(torch.randn(M, K, generator=g), (K,))
    w = 0.3 * torch.randn(N, K, generator=g)
    b = 0.5 * torch.randn(N, generator=g)
    if variant == "inf":
        b[torch.arange(N) % 4 == 1] = float("-inf")
    if variant == "tie":
        w[1::2] = w[0:N - 1:2][:w[1::2].shape[0]]
        b[1::2] = b[0:N - 1:2][:b[1::2].shape[0]]
    return a, w, (None if variant == "nobias" else b)


@functools.lru_cache(maxsize=None)
def _reference(M, N, K, variant):
    """(row bound (M,), fp64 logits (M, N)), computed once per case."""
    return C.row_bounds(*_operands(M, N, K, variant))


def _dev(M, N, K, variant):
    a, w, b = _operands(M, N, K, variant)
    return a.to(DEV), w.to(DEV), None if b is None else b.to(DEV)


def _slots(a, w, b, spare=3):
    """The new epilogue into a nan-filled buffer with spare slots per row -> (buffer, used slots)."""
    n = 2 * ((w.shape[0] + 31) // 32)
    buf = torch.full((a.shape[0], n + spare), NAN, device=DEV, dtype=torch.float64).view(torch.int64)
    out = ops.gemm_argmax_lse(a, w, b, out=buf)
    assert out.data_ptr() == buf.data_ptr()
    return buf, n


def _dense(view):
    """A densely laid out copy (contiguous() keeps the strides of a view with size-1 dimensions)."""
    return torch.empty(view.shape, device=view.device, dtype=view.dtype).copy_(view)


def _bits(pairs):
    return pairs.contiguous().view(torch.int64).reshape(pairs.shape[0], -1)


def _check_epilogue(M, N, K, variant, engine, kernel=None):
    a, w, b = _dev(M, N, K, variant)
    G = (N + 31) // 32
    with ops.option(_lib.OPT_GEMM_ENGINE, engine):
        tiles = {e: ops.gemm_tile(M, N, K, epilogue=e) for e in (_lib.EPI_ARGMAX_LSE, _lib.EPI_ARGMAX, _lib.EPI_LSE)}
        assert len(set(tiles.values())) == 1 and (kernel is None or tiles[_lib.EPI_LSE] == kernel), tiles
        buf, n = _slots(a, w, b)
        keys, kslots, _ = ops._gemm_argmax_keys(a, w, b, None, None, "test")
        a2, dims, wdims = ops._head_operands("test", a, w, b, None)
        pairs, pslots = ops._gemm_lse_pairs(a2, w, b, dims, wdims)
        want_idx = ops.gemm_argmax(a, w, b)
        want_stats = ops.gemm_lse(a, w, b)
    assert n == 2 * G and kslots == pslots == G
    got_keys, got_pairs = _dense(buf[:, 0:n:2]), _dense(buf[:, 1:n:2])
    assert torch.equal(got_keys, keys), "keys differ from the ARGMAX epilogue's"
    assert torch.equal(got_pairs, _bits(pairs)), "pairs differ from the LSE epilogue's"
    # the spare slots of the nan-filled buffer are untouched
    assert bool(torch.isnan(buf[:, n:].view(torch.float64)).all())
    # decoded by the existing kernels
    idx = torch.empty(M, device=DEV, dtype=torch.int32)
    _lib.check(_lib.lib().vasr_argmax_keys(got_keys.data_ptr(), G, G, M, idx.data_ptr(), _lib.stream_of(idx)),
               "vasr_argmax_keys")
    assert torch.equal(idx, want_idx)
    stats = ops.lse_combine(got_pairs.view(torch.float32).view(M, G, 2), G)
    assert torch.equal(_bits(stats), _bits(want_stats))
    return idx


@pytest.mark.parametrize("variant", ["bias", "nobias"])
@pytest.mark.parametrize("M,N,K", SHAPES)
def test_epilogue_is_both_epilogues_bitwise(M, N, K, variant):
    kernel = {2881: 128064}.get(M, 64064)
    _check_epilogue(M, N, K, variant, 1, kernel)


def test_epilogue_on_the_largest_tile():
    """The head's own kernel (128 x 128 tiles) at the smallest row count that selects it."""
    M, N, K = 7777, 1000, 100
    _check_epilogue(M, N, K, "bias", 1, 128128)


def test_epilogue_with_minus_infinity_bias():
    idx = _check_epilogue(129, 1001, 192, "inf", 1)
    assert bool((idx % 4 != 1).all())  # never a masked column


def test_epilogue_ties_take_the_first_column():
    M, N, K = 300, 1000, 192
    idx = _check_epilogue(M, N, K, "tie", 1)
    assert bool((idx % 2 == 0).all())  # column 2j + 1 repeats column 2j exactly: the first of the two wins


@pytest.mark.parametrize("M,N,K", [(130, 65, 192), (33, 1025, 128), (300, 1000, 192)])
def test_epilogue_on_the_rows_engine(M, N, K):
    """Where the engine option sends ARGMAX to the rows engine the new epilogue goes too: a ragged last
    row block, a ragged last 32-column chunk, Kp = 128."""
    _check_epilogue(M, N, K, "bias", 2, 1)


# ------------------------------------------------------------------ the frame log-probability

def _check_logp(got_lp, got_idx, M, N, K, variant, what):
    bound, x = _reference(M, N, K, variant)
    idx = got_idx.cpu().numpy().astype(np.int64)
    want = C.log_softmax_at(x, idx)
    got = got_lp.double().cpu().numpy()
    err = np.abs(got - want)
    print(f"{what} {M}x{N}x{K} {variant}: max err {err.max():.3e}, worst use of the bound {(err / bound).max():.3f}")
    record_error(got, want, dict(atol=float(bound.min()), rtol=0.0))
    assert np.isfinite(got).all() and (err <= bound).all(), (what, float((err / bound).max()))


@pytest.mark.parametrize("variant", ["bias", "nobias", "inf", "tie"])
@pytest.mark.parametrize("M,N,K", SHAPES)
def test_frame_logp_without_logits(M, N, K, variant):
    a, w, b = _dev(M, N, K, variant)
    with ops.option(_lib.OPT_GEMM_ENGINE, 1):
        want_idx = ops.gemm_argmax(a, w, b)
        res = ops.gemm_ctc_greedy_conf(a, w, b, 1, blank=0, per_frame=True)
    pred, lp = res[7].view(-1), res[8].view(-1)
    assert torch.equal(pred, want_idx)
    _check_logp(lp, pred, M, N, K, variant, "logit-free")


@pytest.mark.parametrize("variant", ["bias", "inf", "tie"])
@pytest.mark.parametrize("M,N,K", SHAPES)
def test_frame_logp_from_logits(M, N, K, variant):
    a, w, b = _dev(M, N, K, variant)
    logits = ops.gemm(a, w, b)
    idx, lp = ops.argmax_logp(logits)
    assert idx.dtype == torch.int32 and torch.equal(idx, ops.argmax(logits))
    _check_logp(lp, idx, M, N, K, variant, "from logits")


def test_argmax_logp_takes_any_width_and_alignment():
    g = torch.Generator().manual_seed(5)
    base = torch.randn(7, 131, generator=g).to(DEV)
    for V, off in ((1, 0), (3, 1), (63, 2), (64, 0), (65, 3), (129, 1)):
        x = base[:, off:off + V]  # a strided view: row stride 131, start off a 16-byte boundary
        idx, lp = ops.argmax_logp(x)
        assert torch.equal(idx, ops.argmax(x))
        want = torch.log_softmax(x.double(), -1).gather(-1, idx.long()[:, None])[:, 0]
        assert float((lp.double() - want).abs().max()) <= 8 * EPS * max(1.0, float(want.abs().max()))


# ------------------------------------------------------------------ the collapse

def _sticky(rng, B, L, V, stay=0.6):
    pred = rng.integers(0, V, size=(B, L))
    keep = rng.random((B, L)) < stay
    for t in range(1, L):
        pred[:, t] = np.where(keep[:, t], pred[:, t - 1], pred[:, t])
    return pred.astype(np.int32)


@functools.lru_cache(maxsize=None)
def _collapse_case(name):
    """(pred (B, L) int32, logp (B, L) float32, frames list or None), made once and left unchanged."""
    rng = np.random.default_rng(sum(map(ord, name)))
    frames = None
    if name == "l1":
        pred = np.array([[0], [5], [5]], np.int32)
    elif name == "l8192":
        pred = _sticky(rng, 1, 8192, 6)
    elif name == "all_blank":
        pred = _sticky(rng, 2, 70, 4)
        pred[0] = 0
    elif name == "run130":
        pred = np.zeros((2, 200), np.int32)
        pred[0, 30:160] = 7  # one 130-frame run over the 64-frame window boundaries at 64 and 128
        pred[1, 0:130] = 3   # the same from frame 0
    elif name == "alternating":
        pred = (1 + np.arange(131) % 2).astype(np.int32)[None].repeat(2, 0)
        pred[1] = 3 - pred[1]
    elif name == "run_ends_at_frames":
        pred = _sticky(rng, 2, 100, 5)
        pred[0, 73:90] = 4  # the run goes on past frames[0] = 77: it is cut there
        pred[0, 72] = 0
        pred[1, 60:64] = 2  # ends exactly at frames[1] = 64, a window boundary
        pred[1, 59] = 0
        frames = [77, 64]
    elif name == "frames_edge":
        pred = _sticky(rng, 5, 66, 5)
        pred[:, 0] = 2
        frames = [0, 1, 66, -4, 99]
    elif name == "mixed4":
        pred = _sticky(rng, 4, 300, 6)
        frames = [300, 123, 64, 257]
    else:
        raise KeyError(name)
    logp = (-6.0 * rng.random(pred.shape) ** 3).astype(np.float32)
    pred.setflags(write=False)
    logp.setflags(write=False)
    return pred, logp, frames


COLLAPSE_CASES = ["l1", "l8192", "all_blank", "run130", "alternating", "run_ends_at_frames", "frames_edge", "mixed4"]


def _frames_dev(frames):
    return None if frames is None else torch.tensor(frames, dtype=torch.int32, device=DEV)


def _raw_collapse_conf(pred, logp, frames, blank=0):
    """vasr_ctc_collapse_conf into sentinel-filled outputs (ints -1, floats nan)."""
    B, L = pred.shape
    ints = [torch.full((B, L), -1, device=DEV, dtype=torch.int32) for _ in range(3)]
    lens = torch.full((B,), -1, device=DEV, dtype=torch.int32)
    lsum, lmin = (torch.full((B, L), NAN, device=DEV) for _ in range(2))
    path = torch.full((B,), NAN, device=DEV)
    fr = _frames_dev(frames)
    _lib.check(_lib.lib().vasr_ctc_collapse_conf(pred.data_ptr(), logp.data_ptr(), B, L, _lib.ptr(fr), blank,
                                                 ints[0].data_ptr(), lens.data_ptr(), ints[1].data_ptr(),
                                                 ints[2].data_ptr(), lsum.data_ptr(), lmin.data_ptr(), path.data_ptr(),
                                                 _lib.stream_of(pred)), "vasr_ctc_collapse_conf")
    return ints[0], lens, ints[1], ints[2], lsum, lmin, path


def _check_against_reference(res, pred_np, logp_np, frames, blank=0):
    """Tokens / spans against ops.ctc_collapse (bitwise) and the host reference; min exact; sums within the
    fp32 summation bound; everything past the used counts still the sentinel."""
    toks, lens, st, en, lsum, lmin, path = (t.cpu().numpy() for t in res)
    B, L = pred_np.shape
    pred = torch.from_numpy(np.array(pred_np)).to(DEV)
    t2, l2, s2, e2 = (t.cpu().numpy() for t in ops.ctc_collapse(pred, blank, True, True, frames=_frames_dev(frames)))
    ref = C.collapse_conf_ref(pred_np, logp_np, blank, frames)
    assert np.array_equal(lens, l2)
    worst = 0.0
    for b in range(B):
        n, r = int(lens[b]), ref[b]
        assert n == len(r["tokens"]) and toks[b, :n].tolist() == r["tokens"]
        assert np.array_equal(toks[b, :n], t2[b, :n]) and np.array_equal(st[b, :n], s2[b, :n])
        assert np.array_equal(en[b, :n], e2[b, :n]) and list(zip(st[b, :n], en[b, :n])) == r["spans"]
        assert (toks[b, n:] == -1).all() and (st[b, n:] == -1).all() and (en[b, n:] == -1).all()
        assert np.isnan(lsum[b, n:]).all() and np.isnan(lmin[b, n:]).all()
        assert np.array_equal(lmin[b, :n], r["min"].astype(np.float32))  # a selection: exact
        terms = np.array([e - s for s, e in r["spans"]], np.float64)
        err = np.abs(lsum[b, :n].astype(np.float64) - r["sum"])
        bound = terms * EPS * r["abs"]
        assert (err <= bound).all(), (b, float((err / np.maximum(bound, 1e-300)).max()))
        nfr = C.clamp_frames(frames, B, L)[b]
        perr, pbound = abs(float(path[b]) - r["path"]), nfr * EPS * r["abs_path"]
        assert perr <= pbound, (b, perr, pbound)
        if nfr == 0:
            assert path[b] == 0.0 and n == 0
        worst = max([worst, perr / pbound if pbound else 0.0] + (err[bound > 0] / bound[bound > 0]).tolist())
    return worst


@pytest.mark.parametrize("name", COLLAPSE_CASES)
def test_collapse_conf(name):
    pred_np, logp_np, frames = _collapse_case(name)
    pred, logp = torch.from_numpy(np.array(pred_np)).to(DEV), torch.from_numpy(np.array(logp_np)).to(DEV)
    res = _raw_collapse_conf(pred, logp, frames)
    worst = _check_against_reference(res, pred_np, logp_np, frames)
    print(f"collapse {name}: worst use of the summation bound {worst:.3f}")
    # repeatable bit for bit, and through ops
    again = _raw_collapse_conf(pred, logp, frames)
    assert all(torch.equal(_bits2(x), _bits2(y)) for x, y in zip(res, again))
    via_ops = ops.ctc_collapse_conf(pred, logp, 0, frames=_frames_dev(frames))
    lens = res[1].cpu().numpy()
    for x, y in zip(res, via_ops):
        if x.dim() == 2:
            assert all(torch.equal(x[b, :lens[b]], y[b, :lens[b]]) for b in range(len(lens)))
        else:
            assert torch.equal(x, y)
    # an utterance alone is bitwise the utterance in its batch
    if pred.shape[0] > 1:
        for b in range(pred.shape[0]):
            alone = _raw_collapse_conf(pred[b:b + 1].contiguous(), logp[b:b + 1].contiguous(),
                                       None if frames is None else frames[b:b + 1])
            assert all(torch.equal(_bits2(x[b:b + 1]), _bits2(y)) for x, y in zip(res, alone)), (name, b)


def _bits2(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def test_collapse_conf_reads_no_row_past_frames():
    """nan log-probabilities and out-of-range tokens past each utterance's count change nothing."""
    pred_np, logp_np, frames = _collapse_case("mixed4")
    pred, logp = torch.from_numpy(np.array(pred_np)).to(DEV), torch.from_numpy(np.array(logp_np)).to(DEV)
    want = _raw_collapse_conf(pred, logp, frames)
    p2, l2 = pred.clone(), logp.clone()
    for b, n in enumerate(frames):
        p2[b, n:] = 2 ** 30
        l2[b, n:] = NAN
    got = _raw_collapse_conf(p2, l2, frames)
    assert all(torch.equal(_bits2(x), _bits2(y)) for x, y in zip(want, got))


# ------------------------------------------------------------------ the fused path

def _decode_max(keys, pred):
    """The float the winning key carries (host side of what the kernel does), float32 on the device."""
    # the row's largest key as unsigned (a wave's key sits in the first slot of its columns, not
    # always the winning column's own): flip the sign bit, take the signed maximum, flip it back
    k = (keys ^ -2 ** 63).max(1).values ^ -2 ** 63
    assert torch.equal((0xFFFFFFFF - (k & 0xFFFFFFFF)).to(torch.int32), pred)
    ord_ = (k >> 32) & 0xFFFFFFFF
    u = torch.where((ord_ & 0x80000000) != 0, ord_ & 0x7FFFFFFF, ~ord_ & 0xFFFFFFFF)
    return torch.where(u >= 2 ** 31, u - 2 ** 32, u).to(torch.int32).view(torch.float32)


@pytest.mark.parametrize("B,L", [(2, 37), (3, 501)])
def test_fused_path_is_the_composed_path_bitwise(B, L):
    V, K = 1000, 192
    rng = np.random.default_rng(B * L)
    g = torch.Generator().manual_seed(B * L)
    w = 0.3 * torch.randn(V, K, generator=g)
    b = 0.5 * torch.randn(V, generator=g)
    base = torch.nn.functional.layer_norm(torch.randn(24, K, generator=g), (K,))
    base[:6] = 4.0 * w[0] / w[0].norm() * K ** 0.5 / 4  # six rows that decode to the blank
    a = base[torch.from_numpy(_sticky(rng, B, L, 24).astype(np.int64)).view(-1)].contiguous()  # runs of equal rows
    a, w, b = a.to(DEV), w.to(DEV), b.to(DEV)
    frames = [L, L - 5, 1][:B]
    G = (V + 31) // 32
    slots, n = _slots(a, w, b, spare=1)
    # composed: the existing decode kernels, the key's float in torch, then the collapse from pred / logp
    keys, pairs = _dense(slots[:, 0:n:2]), _dense(slots[:, 1:n:2])
    pred = torch.empty(B * L, device=DEV, dtype=torch.int32)
    _lib.check(_lib.lib().vasr_argmax_keys(keys.data_ptr(), G, G, B * L, pred.data_ptr(), _lib.stream_of(pred)),
               "vasr_argmax_keys")
    stats = ops.lse_combine(pairs.view(torch.float32).view(B * L, G, 2), G)
    logp = (_decode_max(keys, pred) - stats[:, 0]) - stats[:, 1]
    assert torch.equal(pred, ops.gemm_argmax(a, w, b)) and int((pred == 0).sum()) > 0
    want = _raw_collapse_conf(pred.view(B, L), logp.view(B, L), frames)
    # fused: one launch from the slots, sentinel-filled per-frame outputs
    fr = _frames_dev(frames)
    ints = [torch.full((B, L), -1, device=DEV, dtype=torch.int32) for _ in range(4)]
    lens = torch.full((B,), -1, device=DEV, dtype=torch.int32)
    f32 = [torch.full((B, L), NAN, device=DEV) for _ in range(3)]
    path = torch.full((B,), NAN, device=DEV)
    _lib.check(_lib.lib().vasr_ctc_collapse_keys_conf(slots.data_ptr(), slots.shape[1], n, B, L, fr.data_ptr(), 0,
                                                      ints[3].data_ptr(), f32[2].data_ptr(), ints[0].data_ptr(),
                                                      lens.data_ptr(), ints[1].data_ptr(), ints[2].data_ptr(),
                                                      f32[0].data_ptr(), f32[1].data_ptr(), path.data_ptr(),
                                                      _lib.stream_of(slots)), "vasr_ctc_collapse_keys_conf")
    got = (ints[0], lens, ints[1], ints[2], f32[0], f32[1], path)
    assert all(torch.equal(_bits2(x), _bits2(y)) for x, y in zip(want, got))
    assert int(lens.min()) >= 1 and int(lens.max()) < L  # runs were collapsed and blanks dropped
    for bb, nfr in enumerate(frames):  # the per-frame outputs: written up to the count, untouched past it
        assert torch.equal(ints[3][bb, :nfr], pred.view(B, L)[bb, :nfr]) and bool((ints[3][bb, nfr:] == -1).all())
        assert torch.equal(f32[2][bb, :nfr], logp.view(B, L)[bb, :nfr]) and bool(torch.isnan(f32[2][bb, nfr:]).all())
    # and through ops, without frames
    res = ops.gemm_ctc_greedy_conf(a, w, b, B)
    full = ops.ctc_collapse_conf(pred.view(B, L), logp.view(B, L))
    for x, y in zip(res, full):
        if x.dim() == 2:
            assert all(torch.equal(x[i, :int(res[1][i])], y[i, :int(res[1][i])]) for i in range(B))
        else:
            assert torch.equal(x, y)


# ------------------------------------------------------------------ model level

SMALL_CFG = dict(d_model=96, ssm_layers=2, ssm_state_dim=32, global_ssm_state_dim=16, attention_heads=2,
                 attention_dim=24, vocab_size=50)
SAMPLES = [48000, 38400]  # the fwd_b2_3s clips, the second cut to 2.4 s: a padded batch


@functools.lru_cache(maxsize=None)
def _model(kind):
    import velocity_asr as va
    cfg, seed = (SMALL_CFG, 3) if kind == "small" else (None, 0)
    m = va.VELOCITYASR(va.VelocityASRConfig(**(cfg or {})))
    m.load_state_dict({k: torch.from_numpy(v) for k, v in S.make_weights(cfg, seed=seed).items()}, strict=True)
    if kind == "qat":
        from velocity_asr import quantize as Q
        import velocity_asr as va
        m = Q.prepare_model_for_qat(m).to(DEV).eval()
        Q.calibrate_from_activations(m, va.compute_mel_spectrogram(torch.from_numpy(S.make_audio(2, 48000, seed=21)).to(DEV)))
        return m
    m = m.to(DEV).eval()
    return m.to(torch.bfloat16) if kind == "bf16" else m


def _mel(m):
    from velocity_asr.audio import HOP_LENGTH, mel_on_device
    audio = torch.from_numpy(S.make_audio(2, 48000, seed=21)).to(DEV)
    audio[1, SAMPLES[1]:] = 0
    mel = mel_on_device(audio, n_mels=m.config.mel_bins, lengths=SAMPLES, frame_pad=m.temporal_binding.conv_padding())
    return mel, [n // HOP_LENGTH + 1 for n in SAMPLES]


def _used(res):
    """The written part of a scored result per utterance, as host arrays."""
    toks, lens, st, en, lsum, lmin, path = (t.cpu().numpy() for t in res)
    return [tuple(x[b, :lens[b]] for x in (toks, st, en, lsum, lmin)) + (path[b:b + 1],) for b in range(len(lens))]


@pytest.mark.parametrize("kind", ["small", "default"])
def test_model_greedy_scored_without_logits(kind):
    from velocity_asr import decode
    m = _model(kind)
    assert m.ctc_head.fusable()
    mel, frames = _mel(m)
    rows = [m.get_output_length(f) for f in frames]
    rows_dev = torch.tensor(rows, dtype=torch.int32, device=DEV)
    res = m.greedy_scored(mel, frames=frames)
    toks, lens = m.greedy_token_ids(mel, frames=frames, rows=rows_dev)
    assert torch.equal(res[1], lens)
    assert all(torch.equal(res[0][b, :int(lens[b])], toks[b, :int(lens[b])]) for b in range(2))
    t2, l2, s2, e2 = ops.ctc_collapse(m.token_ids(mel, frames=frames), 0, True, True, frames=rows_dev)
    assert all(torch.equal(res[2][b, :int(lens[b])], s2[b, :int(lens[b])]) and
               torch.equal(res[3][b, :int(lens[b])], e2[b, :int(lens[b])]) for b in range(2))
    # fp64 from the model's own fp32 rows at the head's input
    with torch.no_grad():
        _, x, normalized = m._local_global(mel.to(torch.float32), rows)
        B, L, D = x.shape
        ln = m.ctc_head.proj[0]
        a = x if normalized else ops.layer_norm(x, ln.weight, ln.bias, ln.eps)
        lin = m.ctc_head.proj[2]
        per = ops.gemm_ctc_greedy_conf(a.reshape(B * L, D), lin.weight, lin.bias, B, frames=rows_dev, per_frame=True)
    for p, q in zip(_used(per[:7]), _used(res)):  # the same launches: bitwise
        assert all(np.array_equal(u.view(np.int32), v.view(np.int32)) for u, v in zip(p, q))
    bound, x64 = C.row_bounds(a.reshape(B * L, D).cpu(), lin.weight.detach().cpu(), lin.bias.detach().cpu())
    bound, x64 = bound.reshape(B, L), x64.reshape(B, L, -1)
    scored = decode._scored_from_device(res, "mean")
    from_logits = decode.ctc_greedy_decode_with_confidence(m(mel, frames=frames), input_lengths=rows_dev)
    for b in range(B):
        n = rows[b]
        pred = per[7][b, :n].cpu().numpy().astype(np.int64)
        lp64 = C.log_softmax_at(x64[b, :n], pred)
        err = abs(float(res[6][b]) - lp64.sum())
        tol = n * bound[b, :n].max()
        print(f"{kind} utterance {b}: path_logp {float(res[6][b]):.4f}, |err| {err:.3e}, bound {tol:.3e}")
        record_error(float(res[6][b]), lp64.sum(), dict(atol=tol, rtol=0.0))
        assert err <= tol
        r, f = scored[b], from_logits[b]
        assert len(r.tokens) == int(lens[b]) > 0 and all(0.0 < c <= 1.0 for c in r.confidences)
        assert r.score == float(res[6][b]) and r.score <= 0.0
        # through the logits: same tokens and spans, per-token values within the frame tolerance
        assert f.tokens == r.tokens and f.timestamps == r.timestamps
        for (s, e), cr, cf in zip(r.timestamps, r.confidences, f.confidences):
            assert abs(np.log(cr) - np.log(cf)) <= 2.0 * bound[b, s:e].max() + 4 * EPS
        assert abs(f.score - r.score) <= 2.0 * tol
    for agg in ("min", "prod"):
        for r in decode._scored_from_device(res, agg):
            assert all(0.0 < c <= 1.0 for c in r.confidences)


@pytest.mark.parametrize("kind", ["bf16", "qat"])
def test_model_greedy_scored_through_logits(kind):
    """A bf16 or a QAT head is not fusable(): forward() then vasr_argmax_logp_f32 and the collapse."""
    from velocity_asr import decode
    m = _model(kind)
    assert not m.ctc_head.fusable()
    mel, frames = _mel(m)
    rows_dev = torch.tensor([m.get_output_length(f) for f in frames], dtype=torch.int32, device=DEV)
    res = m.greedy_scored(mel, frames=frames)
    toks, lens = m.greedy_token_ids(mel, frames=frames, rows=rows_dev)
    assert torch.equal(res[1], lens)
    assert all(torch.equal(res[0][b, :int(lens[b])], toks[b, :int(lens[b])]) for b in range(2))
    want = decode.ctc_greedy_decode_with_confidence(m(mel, frames=frames), input_lengths=rows_dev)
    got = decode._scored_from_device(res, "mean")
    for r, f in zip(got, want):
        assert r == f and all(0.0 < c <= 1.0 for c in r.confidences) and r.score <= 0.0


def test_decoder_greedy_scored():
    import velocity_asr as va
    from velocity_asr import decode
    m = _model("small")
    mel, frames = _mel(m)
    rows_dev = torch.tensor([m.get_output_length(f) for f in frames], dtype=torch.int32, device=DEV)
    logits = m(mel, frames=frames)
    dec = va.CTCDecoder(va.create_default_vocabulary(50))
    got = dec.decode_greedy_scored(logits, input_lengths=rows_dev)
    want = decode.ctc_greedy_decode_with_confidence(logits, input_lengths=rows_dev)
    for r, w in zip(got, want):
        assert isinstance(r, decode.DecodingResult) and r.tokens == w.tokens and r.timestamps == w.timestamps
        assert r.score == w.score and r.text == dec._tokens_to_text(w.tokens)
    with pytest.raises(ValueError, match="aggregation"):
        decode.ctc_greedy_decode_with_confidence(logits, aggregation="median")


def test_transcribe_files_with_confidence(tmp_path):
    import velocity_asr as va
    from velocity_asr import decode
    from velocity_asr.audio import write_wav
    from velocity_asr.transcription import group_words, transcribe_files
    m = _model("small")
    dec = va.CTCDecoder(va.create_default_vocabulary(50))
    audio = S.make_audio(2, 48000, seed=21)
    paths = [tmp_path / "a.wav", tmp_path / "b.wav"]
    write_wav(str(paths[0]), audio[0][:SAMPLES[1]])  # sorted by length: the batch is (b cut, a) -> (a.wav, b.wav)
    write_wav(str(paths[1]), audio[1])
    plain = transcribe_files(m, paths, dec, "cuda", timestamps=True)
    got = transcribe_files(m, paths, dec, "cuda", confidence=True)
    assert all("error" not in r for r in plain + got), (plain, got)
    assert transcribe_files(m, paths, dec, "cuda") == [{k: v for k, v in r.items() if k != "words"} for r in plain]
    with pytest.raises(ValueError, match="greedy"):
        transcribe_files(m, paths, dec, "cuda", confidence=True, beam_width=4)
    # the same batch by hand
    from velocity_asr.audio import HOP_LENGTH, mel_on_device
    batch = torch.zeros(2, 48000)
    batch[0, :SAMPLES[1]] = torch.from_numpy(audio[0][:SAMPLES[1]])
    batch[1] = torch.from_numpy(audio[1])
    ns = [SAMPLES[1], 48000]
    mel = mel_on_device(batch.to(DEV), n_mels=m.config.mel_bins, lengths=ns, frame_pad=m.temporal_binding.conv_padding())
    scored = decode._scored_from_device(m.greedy_scored(mel, frames=[n // HOP_LENGTH + 1 for n in ns]), "mean")
    for r, p, s in zip(got, plain, scored):
        assert r["transcription"] == p["transcription"] and r["file"] == p["file"] and r["duration"] == p["duration"]
        assert [{k: v for k, v in w.items() if k != "confidence"} for w in r["words"]] == p["words"]
        assert r["score"] == s.score and set(r) == set(p) | {"score"}
        words = group_words(s.tokens, s.timestamps, dec.vocabulary)
        assert [w["word"] for w in words] == [w["word"] for w in r["words"]] and len(words) >= 1
        # each word's confidence is the minimum over its own tokens' values (separators split and do not count)
        want, own = [], []
        for tok, c in zip(s.tokens, s.confidences):
            if dec.vocabulary[tok] in (" ", "▁"):
                want, own = want + ([min(own)] if own else []), []
            else:
                own.append(c)
        want += [min(own)] if own else []
        assert [w["confidence"] for w in r["words"]] == want and all(0.0 < c <= 1.0 for c in want)
