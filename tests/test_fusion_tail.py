"""The gated fusion + CTC-head LayerNorm as one launch (vasr_fusion_tail_f32, ops.fusion_tail).

The kernel repeats the float operations of the four launches it replaces -- the two paired GEMMs
(EPI_NONE, then EPI_PAIR_FUSION with aux = the first's output), the out_proj GEMM and
vasr_layer_norm_f32 -- so every comparison here is torch.equal against those launches in the same
process (VASR_FUSION_TAIL=0 at model level), never a tolerance."""

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
D, A = 192, 48


@pytest.fixture(scope="module")
def params():
    """Random weights, biases and LayerNorm parameters (the seeded model's biases are 0 and its
    LayerNorm weights 1, which would hide a dropped term)."""
    g = torch.Generator().manual_seed(11)
    r = lambda *s, sc=1.0: (torch.randn(*s, generator=g) * sc).to(DEV)  # noqa: E731
    return dict(w_local=r(2 * D, D, sc=D ** -0.5), w_glob=r(2 * D, A, sc=A ** -0.5), b_glob=r(2 * D, sc=0.3),
                b_local=r(D, sc=0.3), w_out=r(D, D, sc=D ** -0.5), b_out=r(D, sc=0.3),
                ln_w=1 + r(D, sc=0.2), ln_b=r(D, sc=0.2))


def _inputs(M):
    g = torch.Generator().manual_seed(1000 + M)
    return torch.randn(M, D, generator=g).to(DEV), torch.randn(M, A, generator=g).to(DEV)


def _four_launches(local, o, P, eps=1e-5):
    from velocity_asr import _lib, ops
    t1 = ops.gemm(local, P["w_local"])
    fused = ops.gemm(o, P["w_glob"], P["b_glob"], epilogue=_lib.EPI_PAIR_FUSION, aux=t1, aux2=P["b_local"], n_out=D)
    out = ops.gemm(fused, P["w_out"], P["b_out"])
    return ops.layer_norm(out, P["ln_w"], P["ln_b"], eps), out


def _fused(local, o, P, eps=1e-5, **kw):
    from velocity_asr import ops
    return ops.fusion_tail(local, o, P["w_local"], P["w_glob"], P["b_glob"], P["b_local"], P["w_out"], P["b_out"],
                           P["ln_w"], P["ln_b"], eps, **kw)


@pytest.mark.parametrize("M", [1, 31, 32, 33, 65, 750, 1002])
def test_kernel_bitwise_the_four_launches(M, params):
    """Row counts below, at and past one and two 32-row tiles, B = 3 x L = 250 and 1002; the 32- and
    64-row workgroups and the automatic choice; both outputs, and the normalised rows alone."""
    local, o = _inputs(M)
    y_ref, out_ref = _four_launches(local, o, params)
    for rows in (0, 32, 64):
        y, out = _fused(local, o, params, want_out=True, rows=rows)
        assert torch.equal(out, out_ref), f"out, rows {rows}: {(out != out_ref).sum().item()} differ"
        assert torch.equal(y, y_ref), f"y, rows {rows}: {(y != y_ref).sum().item()} differ"
        y1, none = _fused(local, o, params, rows=rows)
        assert none is None and torch.equal(y1, y_ref), f"y alone, rows {rows}"


def test_kernel_strided_rows(params):
    """local and o as column slices of wider buffers (row strides 256 and 64)."""
    local, o = _inputs(77)
    bl, bo = torch.zeros(77, 256, device=DEV), torch.zeros(77, 64, device=DEV)
    bl[:, :D], bo[:, :A] = local, o
    y_ref, out_ref = _four_launches(local, o, params)
    y, out = _fused(bl[:, :D], bo[:, :A], params, want_out=True)
    assert torch.equal(y, y_ref) and torch.equal(out, out_ref)


def test_argument_checks(params):
    from velocity_asr import ops
    local, o = _inputs(8)
    with pytest.raises(RuntimeError, match="rows must be"):
        _fused(local, o, params, rows=16)
    with pytest.raises(ValueError, match="inconsistent"):
        ops.fusion_tail(local, o[:, :32], params["w_local"], params["w_glob"], params["b_glob"], params["b_local"],
                        params["w_out"], params["b_out"], params["ln_w"], params["ln_b"], 1e-5)


def _model(default_weights, randomise=True):
    import velocity_asr as va
    m = va.VELOCITYASR()
    m.load_state_dict({k: torch.from_numpy(v) for k, v in default_weights.items()}, strict=True)
    if randomise:  # biases and LayerNorm parameters of the fused chain away from 0 and 1
        g = torch.Generator().manual_seed(5)
        f = m.global_context.fusion
        with torch.no_grad():
            for t in (f.gate_proj[0].bias, f.local_proj.bias, f.global_proj.bias, f.out_proj.bias,
                      m.global_context.cross_attention.out_proj.bias, m.ctc_head.proj[0].bias):
                t.copy_(torch.randn(t.shape, generator=g) * 0.2)
            m.ctc_head.proj[0].weight.copy_(1 + torch.randn(D, generator=g) * 0.2)
    return m.to(DEV).eval()


class _Calls:
    """Counts ops.fusion_tail launches (the wrapped op still runs)."""

    def __init__(self, monkeypatch):
        from velocity_asr import ops
        self.n = 0
        real = ops.fusion_tail

        def counted(*a, **k):
            self.n += 1
            return real(*a, **k)
        monkeypatch.setattr(ops, "fusion_tail", counted)


def _mel(B, seconds, seed):
    import velocity_asr as va
    from velocity_asr import synthetic as S
    return va.compute_mel_spectrogram(torch.from_numpy(S.make_audio(B, int(16000 * seconds), seed=seed)).to(DEV))


def _same_tokens(a, b):
    """(tokens (B, L), lengths (B,)) pairs agree: the lengths, and each row up to its length (the
    rest of a row is never written)."""
    (ta, la), (tb, lb) = a, b
    return torch.equal(la, lb) and all(torch.equal(ta[i, :n], tb[i, :n]) for i, n in enumerate(la.tolist()))


def _both(monkeypatch, calls, fn):
    monkeypatch.setenv("VASR_FUSION_TAIL", "1")
    n0 = calls.n
    new = fn()
    assert calls.n == n0 + 1, "the fused launch did not run"
    monkeypatch.setenv("VASR_FUSION_TAIL", "0")
    old = fn()
    assert calls.n == n0 + 1, "VASR_FUSION_TAIL=0 still took the fused launch"
    return new, old


def test_model_logits_and_tokens_bitwise(default_weights, monkeypatch):
    """Logits of 2 x 10 s clips and the greedy tokens of B = 3: the fused launch (default) against
    VASR_FUSION_TAIL=0; return_features=True keeps the separate launches and its logits agree too."""
    m, calls = _model(default_weights), _Calls(monkeypatch)
    mel = _mel(2, 10.0, 21)
    new, old = _both(monkeypatch, calls, lambda: m(mel))
    assert torch.equal(new, old), f"{(new != old).sum().item()} logits differ"
    monkeypatch.setenv("VASR_FUSION_TAIL", "1")
    n0 = calls.n
    feat_logits, feats = m(mel, return_features=True)
    assert calls.n == n0 and torch.equal(feat_logits, old) and feats["fused_features"].shape == (2, 501, D)
    del new, old, feat_logits
    mel3 = _mel(3, 5.0, 22)
    assert _same_tokens(*_both(monkeypatch, calls, lambda: m.greedy_token_ids(mel3)))
    an, ao = _both(monkeypatch, calls, lambda: m.token_ids(mel3))
    assert torch.equal(an, ao)


def test_model_ragged_batch_bitwise(default_weights, monkeypatch):
    """A zero-padded batch with frames= given: logits and greedy tokens, the two settings."""
    m, calls = _model(default_weights), _Calls(monkeypatch)
    mel = _mel(3, 4.0, 23)
    frames = [mel.shape[1], 251, 117]
    for b, f in enumerate(frames):
        mel[b, f:] = 0
    new, old = _both(monkeypatch, calls, lambda: m(mel, frames=frames))
    assert torch.equal(new, old)
    rows = torch.tensor([m.get_output_length(f) for f in frames], dtype=torch.int32, device=DEV)
    assert _same_tokens(*_both(monkeypatch, calls, lambda: m.greedy_token_ids(mel, frames=frames, rows=rows)))


def test_bf16_and_qat_models_keep_the_separate_launches(default_weights, monkeypatch):
    """The kernel is the fp32 model's: a bf16 model and a QAT model run the GEMMs + LayerNorm."""
    from velocity_asr import quantize as Q
    calls = _Calls(monkeypatch)
    monkeypatch.setenv("VASR_FUSION_TAIL", "1")
    mel = _mel(1, 1.5, 24)
    bf = _model(default_weights, randomise=False).to(torch.bfloat16).eval()
    assert torch.isfinite(bf(mel)).all() and calls.n == 0
    q = Q.prepare_model_for_qat(_model(default_weights, randomise=False).cpu()).to(DEV).eval()
    Q.calibrate_from_activations(q, mel)
    assert torch.isfinite(q(mel)).all() and calls.n == 0
    fp = _model(default_weights, randomise=False)
    fp(mel)
    assert calls.n == 1
