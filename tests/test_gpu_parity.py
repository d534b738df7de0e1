"""HIP path vs the oracle / reference goldens, on an MI355X (pytest -m gpu).

Tolerances (float32 path):
  * kernels vs numpy/torch fp32:             max-abs <= 2e-5 * scale (GEMM K-order, exp ULPs)
  * mel vs reference golden:                  atol 2e-4, rtol 1e-4
  * scan (tree / recurrence) vs golden:       atol 1e-4, rtol 1e-4
  * logits vs reference golden:               atol 1e-4, rtol 1e-5 (measured max 8.2e-6)
  * CTC argmax tokens and greedy token lists: bit-exact (integer output)
"""

import json

import numpy as np
import pytest
import torch

from conftest import golden, golden_json, record_error
from oracle import velocity_ref as R
from velocity_asr import synthetic as S

pytestmark = pytest.mark.gpu

DEV = "cuda"
LOGIT_TOL = dict(atol=1e-4, rtol=1e-5)  # SURVEY §8(d); measured max |diff| 8.2e-6


def assert_logits(got, want, tol=LOGIT_TOL):
    """assert_allclose(got, want, **tol), recording max |diff| and the worst |diff| / (atol + rtol |want|)
    per test in $VASR_PARITY_LOG (JSON lines) when set, so the measured margins can be reported."""
    got = np.asarray(got, dtype=np.float64)
    want = np.asarray(want, dtype=np.float64)
    record_error(got, want, tol)
    np.testing.assert_allclose(got, want, **tol)


@pytest.fixture(scope="module")
def va():
    import velocity_asr
    from velocity_asr import _lib
    _lib.require_device()
    _lib.load()
    return velocity_asr


def make_model(va, config=None, seed=0):
    cfg = va.VelocityASRConfig(**(config or {}))
    m = va.VELOCITYASR(cfg)
    W = S.make_weights(config, seed=seed)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in W.items()}, strict=True)
    return m.to(DEV).eval()


@pytest.fixture(scope="module")
def model(va):
    return make_model(va)


def t(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


# ----------------------------------------------------------------------------- kernels
@pytest.mark.parametrize("M,N,K", [(1, 64, 32), (33, 192, 192), (257, 768, 192), (300, 512, 384),
                                   (130, 1000, 192), (64, 48, 48), (5, 96, 240)])
@pytest.mark.parametrize("epi", ["none", "gelu", "softplus", "residual"])
def test_gemm_epilogues(va, M, N, K, epi):
    from velocity_asr import _lib, ops
    g = torch.Generator().manual_seed(M * 7 + N)
    a = torch.randn(M, K, generator=g)
    w = torch.randn(N, K, generator=g) / K ** 0.5
    b = torch.randn(N, generator=g) * 0.1
    res = torch.randn(M, N, generator=g)
    ref = a.double() @ w.double().T + b.double()
    kw = {}
    if epi == "none":
        e = _lib.EPI_NONE
    elif epi == "gelu":
        e = _lib.EPI_GELU
        ref = torch.nn.functional.gelu(ref)
    elif epi == "softplus":
        e = _lib.EPI_SOFTPLUS_FROM
        kw["n_out"] = N // 3
        ref = torch.cat([ref[:, : N // 3], torch.nn.functional.softplus(ref[:, N // 3:])], 1)
    else:
        e = _lib.EPI_RESIDUAL
        kw["aux"] = res.to(DEV)
        ref = ref + res.double()
    out = ops.gemm(a.to(DEV), w.to(DEV), b.to(DEV), epilogue=e, **kw).cpu().double()
    assert out.shape == ref.shape
    assert (out - ref).abs().max().item() < 2e-5 * max(1.0, ref.abs().max().item())


def test_gemm_strided_views_and_batches(va):
    from velocity_asr import ops
    g = torch.Generator().manual_seed(3)
    big = torch.randn(50, 100, generator=g).to(DEV)
    w = torch.randn(64, 40, generator=g).to(DEV)
    out = ops.gemm(big[:, 8:48], w)
    ref = big[:, 8:48].double() @ w.double().T
    assert (out.double() - ref).abs().max().item() < 1e-4
    # overlapping strided rows (the temporal-conv / STFT im2col trick)
    base = torch.randn(3, 1000, generator=g)
    wb = torch.randn(64, 120, generator=g)
    res = torch.empty(3, 20, 64, device=DEV)
    ops.gemm_batched(base.to(DEV), 40, 1000, 20, 3, 120, wb.to(DEV), None, res, 64, 20 * 64)
    rows = torch.stack([torch.stack([base[b, 40 * m: 40 * m + 120] for m in range(20)]) for b in range(3)])
    ref = rows.double() @ wb.double().T
    assert (res.cpu().double() - ref).abs().max().item() < 1e-4


def test_gemm_x3_accuracy_matches_f32(va):
    """Split-bf16 GEMM error vs fp64 stays at an fp32 GEMM's level (torch's fp32 matmul on the
    same device, the plain PyTorch fp32 reference), also for operands spanning 2^-20..2^20
    (the split keeps all 24 bits of every value)."""
    from velocity_asr import ops
    g = torch.Generator().manual_seed(11)
    M, N, K = 512, 384, 768
    for scale in (False, True):
        a = torch.randn(M, K, generator=g)
        w = torch.randn(N, K, generator=g) / K ** 0.5
        if scale:
            a = a * torch.exp2(torch.randint(-20, 21, (M, K), generator=g).float())
            w = w * torch.exp2(torch.randint(-20, 21, (N, K), generator=g).float())
        ref = a.double() @ w.double().T
        bound = (a.double().abs() @ w.double().abs().T)  # condition-aware error scale
        errs = {"x3": ops.gemm(a.to(DEV), w.to(DEV)).cpu().double(),
                "torch_f32": (a.to(DEV) @ w.to(DEV).T).cpu().double()}
        errs = {k: ((v - ref).abs() / bound).max().item() for k, v in errs.items()}
        assert errs["torch_f32"] < 2 ** -16
        assert errs["x3"] < max(2.0 * errs["torch_f32"], 2 ** -20), errs


def test_split_weights_planes(va):
    """hi + mid + lo reproduces every fp32 weight exactly in the fragment-native layout
    [N/32][Kp/16][3][64][8]; rows >= N and k >= K are zero."""
    from velocity_asr import ops
    g = torch.Generator().manual_seed(5)
    N, K = 70, 100
    w = (torch.randn(N, K, generator=g) * torch.exp2(torch.randint(-30, 31, (N, K), generator=g).float()))
    NT, KS = 3, 8
    planes = ops.split_weights(w.to(DEV)).cpu().view(NT, KS, 3, 2, 32, 8)  # [nt][ks][pl][h][r][j]
    f = ((planes.to(torch.int32) & 0xFFFF) << 16).view(torch.float32).double()
    # (nt, r) -> n ; (ks, h, j) -> k
    dense = f.permute(2, 0, 4, 1, 3, 5).reshape(3, NT * 32, KS * 16)
    np.testing.assert_array_equal(dense.sum(0)[:N, :K].float().numpy(), w.numpy())
    assert (dense[:, N:, :] == 0).all() and (dense[:, :, K:] == 0).all()


@pytest.mark.parametrize("L,C,Kc", [(37, 192, 4), (501, 192, 4), (16, 192, 4), (1, 192, 4), (3, 192, 4),
                                    (37, 192, 3), (40, 96, 2), (33, 256, 7), (20, 64, 1)])
def test_layer_norm_and_dwconv(va, L, C, Kc):
    """LayerNorm and the fused LN + causal depthwise conv (Kc = 4 is the compile-time path,
    other widths the generic one; full 16-row tiles, ragged last tiles, L < Kc)."""
    from velocity_asr import ops
    rng = np.random.default_rng(L * 10 + Kc)
    x = rng.standard_normal((2, L, C)).astype(np.float32) * 3 + 1
    w = (1 + 0.1 * rng.standard_normal(C)).astype(np.float32)
    b = (0.1 * rng.standard_normal(C)).astype(np.float32)
    cw = rng.standard_normal((C, 1, Kc)).astype(np.float32) * 0.3
    cb = rng.standard_normal(C).astype(np.float32) * 0.1
    ln = ops.layer_norm(t(x), t(w), t(b)).cpu().numpy()
    np.testing.assert_allclose(ln, R.layer_norm(x, w, b), atol=2e-5, rtol=1e-5)
    y = ops.ln_dwconv(t(x), t(w), t(b), t(cw.reshape(C, Kc)), t(cb)).cpu().numpy()
    np.testing.assert_allclose(y, R.causal_dwconv(R.layer_norm(x, w, b), cw, cb), atol=3e-5, rtol=1e-5)


@pytest.mark.gpu
@pytest.mark.parametrize("B,L,C,Kc", [(1, 501, 192, 4), (3, 64, 192, 4), (2, 37, 192, 4), (2, 3, 192, 4),
                                      (1, 40, 96, 2), (2, 33, 256, 7)])
def test_ln_dwconv_tile_heights_bitwise(va, B, L, C, Kc):
    """vasr_ln_dwconv_f32's workgroup tile heights (VASR_OPT_DW_ROWS 4 / 8 / 16; auto picks 8
    below 512 workgroups of 16) give bitwise the same outputs."""
    import torch
    from velocity_asr import _lib, ops
    rng = np.random.default_rng(B * 1000 + L + Kc)
    x = t(rng.standard_normal((B, L, C)).astype(np.float32) * 2 + 0.5)
    w, b = t((1 + 0.1 * rng.standard_normal(C)).astype(np.float32)), t((0.1 * rng.standard_normal(C)).astype(np.float32))
    cw, cb = t((0.3 * rng.standard_normal((C, Kc))).astype(np.float32)), t((0.1 * rng.standard_normal(C)).astype(np.float32))
    ys = []
    for rows in (0, 4, 8, 16):
        with ops.option(_lib.OPT_DW_ROWS, rows):
            ys.append(ops.ln_dwconv(x, w, b, cw, cb))
    for y in ys[1:]:
        assert torch.equal(y, ys[0])


@pytest.mark.gpu
@pytest.mark.parametrize("lengths", [None, (16000, 9000, 12345)])
def test_mel_batch_invariant_bitwise(va, lengths):
    """An utterance's log-mel (per-utterance statistics from fp64 chunk partials summed in a fixed
    order) is bitwise the same alone, in a pair and in a batch of three, with and without
    per-utterance lengths, and in the zero-framed layout the temporal conv reads."""
    import torch
    from velocity_asr import audio as A, ops
    rng = np.random.default_rng(5)
    audio = t((0.1 * rng.standard_normal((3, 16000))).astype(np.float32))
    lens = None if lengths is None else torch.tensor(lengths, dtype=torch.int32)
    full = A.compute_mel_spectrogram(audio, lengths=lens)
    for i in range(3):
        one = A.compute_mel_spectrogram(audio[i:i + 1].contiguous(), lengths=None if lens is None else lens[i:i + 1])
        assert torch.equal(one[0], full[i])
    two = A.compute_mel_spectrogram(audio[:2].contiguous(), lengths=None if lens is None else lens[:2])
    assert torch.equal(two, full[:2])
    if lens is None:  # the zero-framed layout the temporal conv reads (frame_pad = 1)
        tb = A._tables(audio.device, 400, 80, 16000)
        power = ops.stft_power_400(audio, tb.window)
        F = power.shape[1]
        z3 = ops.mel_log_norm(power, tb.n_bins, F * tb.n_bins, tb.fb_csr, 3, F, 80, True, frame_pad=1)
        z1 = ops.mel_log_norm(power[:1].contiguous(), tb.n_bins, F * tb.n_bins, tb.fb_csr, 1, F, 80, True, frame_pad=1)
        assert torch.equal(z1._vasr_zero_framed[0][0], z3._vasr_zero_framed[0][0])


@pytest.mark.gpu
@pytest.mark.parametrize("L,K", [(501, 64), (64, 16), (501, 16), (37, 5), (9, 9), (300, 7)])
def test_adaptive_pool_sums_rows_in_order(va, L, K):
    """vasr_adaptive_pool_f32 adds each window's rows in row order (fp32, one rounding per add;
    windows of 1 to 72 rows, loaded 8 at a time): bitwise equal to that sum done on the host."""
    from velocity_asr import ops
    rng = np.random.default_rng(L * 100 + K)
    B, C = 2, 192
    x = rng.standard_normal((B, L, C)).astype(np.float32)
    got = ops.adaptive_pool(t(x), K).cpu().numpy()
    want = np.empty((B, K, C), np.float32)
    for i in range(K):
        s, e = (i * L) // K, ((i + 1) * L + K - 1) // K
        acc = np.zeros((B, C), np.float32)
        for r in range(s, e):
            acc = (acc + x[:, r]).astype(np.float32)
        want[:, i] = acc / np.float32(e - s)
    assert np.array_equal(got, want)


def _scan_cases():
    meta = json.loads(str(golden("scan.npz")["meta"]))
    return [tuple(c) for c in meta["cases"]]


def _scan_inputs(seed, B, L, Di, N):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((B, L, Di)).astype(np.float32)
    dt = np.log1p(np.exp(rng.standard_normal((B, L, Di)) * 0.7 - 1.0)).astype(np.float32)
    Bm = rng.standard_normal((B, L, N)).astype(np.float32)
    Cm = rng.standard_normal((B, L, N)).astype(np.float32)
    A_log = (np.log(np.arange(1, N + 1)) + 0.01 * rng.standard_normal(N)).astype(np.float32)
    D = (1.0 + 0.1 * rng.standard_normal(Di)).astype(np.float32)
    return x, dt, Bm, Cm, A_log, D


def _run_scan(x, dt, Bm, Cm, A_log, D, mode, z=None):
    """Drive vasr_ssm_scan_f32 with padded channels (kernel needs Di % 16 == 0)."""
    from velocity_asr import ops
    B, L, Di = x.shape
    N = Bm.shape[-1]
    Dp = max(64, (Di + 63) // 64 * 64)
    xz = np.zeros((B * L, 2 * Dp), np.float32)
    xz[:, :Di] = x.reshape(B * L, Di)
    zz = np.full((B * L, Dp), 30.0, np.float32) if z is None else z  # silu(30) == 30 -> divide out
    xz[:, Dp:] = zz
    dtp = np.ones((B * L, Dp), np.float32) * 0.1
    dtp[:, :Di] = dt.reshape(B * L, Di)
    bc = np.concatenate([Bm.reshape(B * L, N), Cm.reshape(B * L, N)], 1)
    A = -np.exp(A_log.astype(np.float32))
    A2 = (A * np.float32(1.4426950408889634)).astype(np.float32)
    Dv = np.ones(Dp, np.float32)
    Dv[:Di] = D
    out = ops.ssm_scan(t(xz), t(dtp), t(bc), t(A2), t(Dv), B, L, mode).cpu().numpy()
    return (out[:, :Di] / np.float32(30.0)).reshape(B, L, Di)


@pytest.mark.parametrize("case", _scan_cases(), ids=lambda c: c[0])
def test_scan_matches_reference_golden(va, case):
    name, seed, B, L, Di, N = case
    g = golden("scan.npz")
    x, dt, Bm, Cm, A_log, D = _scan_inputs(seed, B, L, Di, N)
    yp = _run_scan(x, dt, Bm, Cm, A_log, D, 0)
    ys = _run_scan(x, dt, Bm, Cm, A_log, D, 1)
    yf = _run_scan(x, dt, Bm, Cm, A_log, D, 2)
    np.testing.assert_allclose(yp, g[name + "__parallel"], atol=1e-4, rtol=1e-4)
    np.testing.assert_allclose(yf, g[name + "__parallel"], atol=1e-4, rtol=1e-4)
    np.testing.assert_allclose(ys, g[name + "__sequential"], atol=1e-4, rtol=1e-4)


@pytest.mark.parametrize("mode", [0, 2])
@pytest.mark.parametrize("L", [1, 2, 15, 16, 17, 33, 255, 256, 257, 511, 512, 513, 1024, 2049])
def test_scan_tree_vs_oracle_lengths(va, L, mode):
    """The tree scan op for op (mode 0) and with fused multiply-adds (mode 2) vs the oracle."""
    x, dt, Bm, Cm, A_log, D = _scan_inputs(1000 + L, 1, L, 16, 64)
    A = (-np.exp(A_log)).astype(np.float32)
    ref = R.parallel_scan(x, dt, A, Bm, Cm, D)
    got = _run_scan(x, dt, Bm, Cm, A_log, D, mode)
    np.testing.assert_allclose(got, ref, atol=1e-4, rtol=1e-4)


@pytest.mark.parametrize("npl", [2, 4])
@pytest.mark.parametrize("N,L", [(16, 70), (32, 300), (64, 513)])
@pytest.mark.parametrize("mode", [0, 1, 2])
def test_scan_lane_layouts(va, npl, N, L, mode):
    """Both lane layouts of the scan kernel (2 or 4 state indices per lane, VASR_OPT_SCAN_LANES)
    against the oracle, tree (mode 0) and recurrence (mode 1); they differ only in the
    order of the y = sum_n h C partial sums."""
    from velocity_asr import _lib, ops
    x, dt, Bm, Cm, A_log, D = _scan_inputs(5 * N + L, 3, L, 64, N)
    A = (-np.exp(A_log)).astype(np.float32)
    ref = (R.sequential_scan if mode == 1 else R.parallel_scan)(x, dt, A, Bm, Cm, D)
    with ops.option(_lib.OPT_SCAN_LANES, npl):
        got = _run_scan(x, dt, Bm, Cm, A_log, D, mode)
    np.testing.assert_allclose(got, ref, atol=1e-4, rtol=1e-4)


@pytest.mark.parametrize("L", [1, 17, 501])
def test_mamba_mode_vs_selective_scan_ref(va, L):
    """scan_mode="mamba" runs the recurrence kernel (mode 1); checked against the oracle's
    restatement of mamba-ssm's selective_scan_ref in the package's documented layout (the
    package is absent: parity with it is unpinned)."""
    x, dt, Bm, Cm, A_log, D = _scan_inputs(300 + L, 2, L, 32, 64)
    A = (-np.exp(A_log)).astype(np.float32)
    np.testing.assert_allclose(_run_scan(x, dt, Bm, Cm, A_log, D, 1), R.mamba_scan(x, dt, A, Bm, Cm, D),
                               atol=1e-4, rtol=1e-4)


@pytest.mark.parametrize("N", [16, 32, 64])
def test_scan_state_dims(va, N):
    x, dt, Bm, Cm, A_log, D = _scan_inputs(77 + N, 2, 70, 64, N)
    A = (-np.exp(A_log)).astype(np.float32)
    np.testing.assert_allclose(_run_scan(x, dt, Bm, Cm, A_log, D, 0), R.parallel_scan(x, dt, A, Bm, Cm, D),
                               atol=1e-4, rtol=1e-4)
    np.testing.assert_allclose(_run_scan(x, dt, Bm, Cm, A_log, D, 1), R.sequential_scan(x, dt, A, Bm, Cm, D),
                               atol=1e-4, rtol=1e-4)


def test_scan_gate_and_skip(va):
    """z gate and D skip: out = (y + x D) * silu(z)."""
    from velocity_asr import ops
    x, dt, Bm, Cm, A_log, D = _scan_inputs(5, 1, 40, 64, 64)
    rng = np.random.default_rng(9)
    z = rng.standard_normal((40, 64)).astype(np.float32) * 2
    A = (-np.exp(A_log)).astype(np.float32)
    y = R.parallel_scan(x, dt, A, Bm, Cm, D)[0]
    ref = y * R.silu(z)
    xz = np.concatenate([x[0], z], 1)
    bc = np.concatenate([Bm[0], Cm[0]], 1)
    A2 = (A * np.float32(1.4426950408889634)).astype(np.float32)
    out = ops.ssm_scan(t(xz), t(dt[0]), t(bc), t(A2), t(D), 1, 40, 0).cpu().numpy()
    np.testing.assert_allclose(out, ref, atol=1e-4, rtol=1e-4)


# ----------------------------------------------------------------------------- mel
@pytest.mark.parametrize("name,make", [
    ("rand_b2_1s", lambda: S.make_audio(2, 16000, seed=11)),
    ("rand_b2_10s", lambda: S.make_audio(2, 160000, seed=1234)),
    ("odd_16333", lambda: S.make_audio(3, 16333, seed=8)),
    ("chirp_3s", lambda: S.make_chirp(48000)[None]),
    ("zero_1s", lambda: np.zeros((1, 16000), np.float32)),
    ("short_201", lambda: S.make_audio(1, 201, seed=5)),
    ("short_400", lambda: S.make_audio(1, 400, seed=6)),
    ("oned_8000", lambda: S.make_audio(1, 8000, seed=9)[0]),
])
@pytest.mark.parametrize("stft", ["fft", "gemm"])
def test_mel_matches_reference(va, name, make, stft, monkeypatch):
    from velocity_asr import audio as A
    monkeypatch.setattr(A, "_STFT_FFT", stft != "gemm")
    monkeypatch.setattr(A, "_STFT_MODE", stft)
    g = golden("mel.npz")
    audio = torch.from_numpy(make())
    mel = va.compute_mel_spectrogram(audio.to(DEV))
    assert mel.device.type == "cuda"
    np.testing.assert_allclose(mel.cpu().numpy(), g[name], atol=2e-4, rtol=1e-4)
    if name == "zero_1s":
        assert torch.count_nonzero(mel).item() == 0
    # CPU input comes back on the CPU, same values
    mel_cpu = va.compute_mel_spectrogram(audio)
    assert mel_cpu.device.type == "cpu"
    np.testing.assert_array_equal(mel_cpu.numpy(), mel.cpu().numpy())


# 800 .. 5120: F = 6, 7, 10, 12, 16, 32, 33 (6 frames per workgroup, 16 per mel chunk)
@pytest.mark.parametrize("S_", [201, 400, 1601, 16000, 16333, 160000, 800, 960, 1440, 1760, 2400, 4960, 5120])
def test_stft_power_fft_vs_fp64(va, S_):
    """Real-FFT power spectrogram vs torch.stft in fp64 (reference audio.py:97-115 in double):
    |P - P64| <= 1e-5 * max(P64) per frame + 1e-6 relative (fp32 FFT rounding)."""
    from velocity_asr import ops
    x = S.make_audio(3, S_, seed=S_)
    win = torch.hann_window(400)
    p = ops.stft_power_400(t(x), win.to(DEV)).cpu().double()
    xd = torch.from_numpy(x).double()
    xp = torch.nn.functional.pad(xd.unsqueeze(1), (200, 200), mode="reflect").squeeze(1)
    ref = torch.stft(xp, 400, 160, window=win.double(), center=False, return_complex=True).abs().pow(2).transpose(1, 2)
    assert p.shape == ref.shape == (3, S_ // 160 + 1, 201)
    frame_max = ref.amax(dim=2, keepdim=True)
    err = (p - ref).abs() - 1e-6 * ref.abs()
    assert (err <= 1e-5 * frame_max + 1e-12).all(), float((err / frame_max.clamp_min(1e-30)).max())


@pytest.mark.parametrize("S_", [160000, 201, 16333, 2559])
def test_stft_power_fft_matches_dft_gemm(va, monkeypatch, S_):
    """The real-FFT front end agrees with the windowed-DFT GEMM (VASR_STFT=gemm) on the mel."""
    from velocity_asr import audio as A
    x = t(S.make_audio(4, S_, seed=77))
    out = {}
    for mode in ("fft", "gemm"):
        monkeypatch.setattr(A, "_STFT_FFT", mode != "gemm")
        monkeypatch.setattr(A, "_STFT_MODE", mode)
        out[mode] = A.mel_on_device(x).cpu()
    np.testing.assert_allclose(out["fft"].numpy(), out["gemm"].numpy(), atol=2e-4, rtol=1e-4)


# ----------------------------------------------------------------------------- global context
def test_adaptive_pool_and_attention(va):
    from velocity_asr import ops
    rng = np.random.default_rng(4)
    for L, K in ((501, 64), (64, 16), (187, 46), (6, 6), (1501, 187)):
        x = rng.standard_normal((2, L, 192)).astype(np.float32)
        np.testing.assert_allclose(ops.adaptive_pool(t(x), K).cpu().numpy(), R.adaptive_avg_pool(x, K),
                                   atol=1e-5, rtol=1e-5)
    B, L, Kp, H, hd = 2, 77, 16, 4, 12
    q = rng.standard_normal((B * L, H * hd)).astype(np.float32)
    kv = rng.standard_normal((B * Kp, 2 * H * hd)).astype(np.float32)
    out = ops.pooled_attention(t(q), t(kv), B, L, Kp, H).cpu().numpy()
    qh = q.reshape(B, L, H, hd).transpose(0, 2, 1, 3)
    kh = kv[:, : H * hd].reshape(B, Kp, H, hd).transpose(0, 2, 1, 3)
    vh = kv[:, H * hd:].reshape(B, Kp, H, hd).transpose(0, 2, 1, 3)
    s = qh @ kh.transpose(0, 1, 3, 2) / np.sqrt(hd)
    p = np.exp(s - s.max(-1, keepdims=True))
    p /= p.sum(-1, keepdims=True)
    ref = (p @ vh).transpose(0, 2, 1, 3).reshape(B * L, H * hd)
    np.testing.assert_allclose(out, ref, atol=2e-5, rtol=1e-5)


# ----------------------------------------------------------------------------- decode
def test_decode_kernels_match_reference(va):
    d = golden_json("decode.json")
    for name, c in d["cases"].items():
        lg = torch.tensor(c["logits"], dtype=torch.float32, device=DEV)
        assert va.ctc_greedy_decode(lg) == c["greedy"], name
        assert va.ctc_greedy_decode(lg, collapse_repeated=False) == c["greedy_nocollapse"], name
        ts = va.ctc_greedy_decode_with_timestamps(lg)
        assert [[tk, [list(x) for x in s]] for tk, s in ts] == c["timestamps"], name
    vocab = va.create_default_vocabulary(1000)
    dec = va.CTCDecoder(vocab)
    lg = torch.tensor(d["cases"]["c3"]["logits"], dtype=torch.float32, device=DEV)
    assert dec.decode_greedy(lg) == d["texts_c3"]


def test_argmax_ties_first_index(va):
    from velocity_asr import ops
    x = torch.zeros(3, 1000, device=DEV)
    x[0, 5] = x[0, 700] = 1.0
    x[2, 999] = 2.0
    assert ops.argmax(x).cpu().tolist() == [5, 0, 999]


# ----------------------------------------------------------------------------- model
def test_forward_stages_b2_3s(va, model):
    g = golden("fwd_b2_3s.npz")
    logits, f = model(t(g["mel"]), return_features=True)
    np.testing.assert_allclose(f["temporal_binding"].cpu().numpy(), g["temporal_binding"], atol=1e-4, rtol=1e-4)
    np.testing.assert_allclose(f["local_features"].cpu().numpy(), g["local_features"], atol=3e-4, rtol=1e-4)
    np.testing.assert_allclose(f["fused_features"].cpu().numpy(), g["fused_features"], atol=3e-4, rtol=1e-4)
    assert_logits(logits.cpu().numpy(), g["logits"])
    np.testing.assert_array_equal(logits.argmax(-1).cpu().numpy(), g["tokens"])


def test_audio_to_tokens_b2_3s(va, model):
    g = golden("fwd_b2_3s.npz")
    mel = va.compute_mel_spectrogram(t(S.make_audio(2, 48000, seed=21)))
    logits = model(mel)
    assert_logits(logits.cpu().numpy(), g["logits"])
    dec = golden_json("decode_fwd.json")["results"]
    assert va.ctc_greedy_decode(logits) == dec["b2_3s"]
    ts = va.ctc_greedy_decode_with_timestamps(logits)
    assert [[tk, [list(x) for x in s]] for tk, s in ts] == dec["b2_3s_ts"]


def test_headline_shape_b2_10s(va, model):
    g = golden("fwd_b2_10s.npz")
    mel = va.compute_mel_spectrogram(t(S.make_audio(2, 160000, seed=1234)))
    logits = model(mel)
    assert logits.shape == (2, 501, 1000)
    np.testing.assert_array_equal(logits.argmax(-1).cpu().numpy(), g["tokens"])
    assert_logits(logits[:, g["frames"]].cpu().numpy(), g["logits_sub"])
    assert va.ctc_greedy_decode(logits) == golden_json("decode_fwd.json")["results"]["b2_10s"]


def test_long_utterance_30s(va, model):
    g = golden("fwd_b1_30s.npz")
    mel = va.compute_mel_spectrogram(t(S.make_audio(1, 480000, seed=4321)))
    logits = model(mel)
    assert logits.shape == (1, 1501, 1000)
    np.testing.assert_array_equal(logits.argmax(-1).cpu().numpy(), g["tokens"])
    assert_logits(logits[:, g["frames"]].cpu().numpy(), g["logits_sub"])


def test_edge_lengths(va, model):
    g = golden("fwd_edge.npz")
    for S_, seed in ((201, 31), (400, 32), (1600, 33), (8000, 34), (16333, 35)):
        mel = va.compute_mel_spectrogram(t(S.make_audio(1, S_, seed=seed)))
        logits = model(mel)
        assert_logits(logits.cpu().numpy(), g[f"S{S_}__logits"])
        np.testing.assert_array_equal(logits.argmax(-1).cpu().numpy(), g[f"S{S_}__tokens"])


def test_mel_input_and_chirp(va, model):
    g = golden("fwd_melin_500.npz")
    mel = np.random.default_rng(41).standard_normal((2, 500, 80)).astype(np.float32)
    logits = model(t(mel))
    assert_logits(logits.cpu().numpy(), g["logits"])
    np.testing.assert_array_equal(logits.argmax(-1).cpu().numpy(), g["tokens"])
    g = golden("fwd_chirp_3s.npz")
    logits = model(va.compute_mel_spectrogram(t(S.make_chirp(48000)[None])))
    assert_logits(logits.cpu().numpy(), g["logits"])
    np.testing.assert_array_equal(logits.argmax(-1).cpu().numpy(), g["tokens"])


def test_sequential_scan_mode(va):
    g = golden("fwd_seq_b2_3s.npz")
    m = make_model(va, dict(scan_mode="sequential"))
    logits = m(va.compute_mel_spectrogram(t(S.make_audio(2, 48000, seed=21))))
    assert_logits(logits.cpu().numpy(), g["logits"])
    np.testing.assert_array_equal(logits.argmax(-1).cpu().numpy(), g["tokens"])


def test_small_config(va):
    g = golden("fwd_smallcfg.npz")
    cfg = json.loads(str(g["meta"]))["config"]
    m = make_model(va, cfg, seed=3)
    logits = m(va.compute_mel_spectrogram(t(S.make_audio(2, 32000, seed=51))))
    assert_logits(logits.cpu().numpy(), g["logits"])
    np.testing.assert_array_equal(logits.argmax(-1).cpu().numpy(), g["tokens"])


def _statedims():
    return golden("fwd_statedims.npz"), json.loads(str(golden("fwd_statedims.npz")["meta"]))


@pytest.mark.parametrize("name", ["sd8", "sd48", "sd128"])
def test_state_dims_model_vs_reference(va, name):
    """any ssm_state_dim / global_ssm_state_dim (model.py:23-68).  N = 8 and
    48 run as 16 / 64 with zero-padded states (SelectiveSSM._prepared), N = 128 natively;
    logits and tokens vs the reference at N = 8, 48, 128 (global 8, 24, 128)."""
    g, meta = _statedims()
    m = make_model(va, meta["configs"][name], seed=5)
    logits = m(va.compute_mel_spectrogram(t(S.make_audio(2, 32000, seed=52)))).cpu().numpy()
    assert_logits(logits[:, ::4], g[name + "__logits_sub4"])
    np.testing.assert_array_equal(logits.argmax(-1), g[name + "__tokens"])


@pytest.mark.parametrize("case", [tuple(c) for c in json.loads(str(golden("fwd_statedims.npz")["meta"]))["scans"]],
                         ids=lambda c: c[0])
@pytest.mark.parametrize("mode", [0, 1, 2])
def test_scan_state_dims_vs_reference(va, case, mode):
    """The scan op at N = 8, 48 (zero-padded to 16 / 64 by ops.ssm_scan) and 128 vs the reference."""
    name, seed, B, L, Di, N = case
    g, _ = _statedims()
    x, dt, Bm, Cm, A_log, D = _scan_inputs(seed, B, L, Di, N)
    got = _run_scan(x, dt, Bm, Cm, A_log, D, mode)
    want = g[name + ("__sequential" if mode == 1 else "__parallel")]
    np.testing.assert_allclose(got, want, atol=1e-4, rtol=1e-4)


@pytest.mark.parametrize("L", [1, 33, 513, 1501])
def test_scan_n128_chunked_bitwise_and_oracle(va, L):
    """N = 128 (32 lanes per channel): streaming and chunk-parallel forms bitwise equal, and vs
    the oracle."""
    from velocity_asr import ops
    x, dt, Bm, Cm, A_log, D = _scan_inputs(500 + L, 1, L, 16, 128)
    prev = ops.scan_form("streaming")
    try:
        a = _run_scan(x, dt, Bm, Cm, A_log, D, 2)
        ops.scan_form("chunked")
        b = _run_scan(x, dt, Bm, Cm, A_log, D, 2)
    finally:
        ops.scan_form(prev)
    np.testing.assert_array_equal(a, b)
    ref = R.parallel_scan(x, dt, (-np.exp(A_log)).astype(np.float32), Bm, Cm, D)
    np.testing.assert_allclose(a, ref, atol=1e-4, rtol=1e-4)


# ----------------------------------------------------------------------------- full-size properties
def _assert_tokens_pinned(got_argmax, got_lists, g, prefix, what):
    """Argmax tokens and greedy lists equal to the reference's, with the frames that differ
    (and their reference top-2 margins) named on failure."""
    exp = g[prefix + "tokens"].astype(np.int32)
    diff = np.argwhere(got_argmax != exp)
    assert diff.size == 0, (f"{what}: {len(diff)} argmax frames differ from the reference, e.g. "
                            f"{[(int(b), int(f), float(g[prefix + 'margin'][b, f])) for b, f in diff[:8]]} "
                            "(clip, frame, reference top-2 margin)")
    assert got_lists == json.loads(str(g["greedy"]))[prefix.rstrip("_")]


def test_full_batch_32x10s_properties(va, model):
    """BASELINE config 2, the bench's exact batch (make_audio(32, 160000, seed=1234), one
    forward of 32 clips): all 32 clips' argmax tokens and greedy lists equal the reference's
    (tests/golden/fwd_fullbatch.npz, reference run in chunks of 8; min top-2 margin 1.1e-5),
    plus determinism and batch invariance."""
    from velocity_asr.pipeline import audio_to_token_ids, token_lists
    audio = t(S.make_audio(32, 160000, seed=1234))
    mel = va.compute_mel_spectrogram(audio)
    l1 = model(mel)
    l2 = model(mel)
    assert torch.equal(l1, l2), "forward must be deterministic"
    assert torch.isfinite(l1).all()
    g = golden("fwd_fullbatch.npz")
    am = l1.argmax(-1).cpu().numpy()
    _assert_tokens_pinned(am, va.ctc_greedy_decode(l1), g, "c2_", "C2 32 x 10 s")
    # the token pipeline (fused CTC-head argmax + device collapse) as the bench runs it
    toks, lens = audio_to_token_ids(model, audio)
    assert token_lists(toks, lens) == json.loads(str(g["greedy"]))["c2"]
    single = model(mel[5:6])
    np.testing.assert_array_equal(single.argmax(-1).cpu().numpy(), am[5:6])
    np.testing.assert_allclose(single.cpu().numpy(), l1[5:6].cpu().numpy(), atol=1e-4, rtol=1e-4)


def test_full_batch_30s_pinned(va, model):
    """BASELINE config 4 as the bench launches it (make_audio(32, 480000, seed=1234), one B = 32
    forward, L = 1501): argmax tokens and greedy lists equal the reference's for all 32 clips
    (tests/golden/fwd_fullbatch.npz, the reference run in chunks of 4), and the token pipeline
    (fused CTC-head argmax + device collapse) gives the same lists."""
    from velocity_asr.pipeline import audio_to_token_ids, token_lists
    audio = t(S.make_audio(32, 480000, seed=1234))
    logits = model(va.compute_mel_spectrogram(audio))
    g = golden("fwd_fullbatch.npz")
    _assert_tokens_pinned(logits.argmax(-1).cpu().numpy(), va.ctc_greedy_decode(logits), g, "c4_",
                          "C4 32 x 30 s")
    del logits
    assert token_lists(*audio_to_token_ids(model, audio)) == json.loads(str(g["greedy"]))["c4"]


HEADLINE_TOL = dict(atol=1e-4, rtol=1e-5)  # the fp tolerance of SURVEY §8 d, at the headline shapes


@pytest.mark.parametrize("fma", ["1", "0"], ids=["mode2", "mode0"])
@pytest.mark.parametrize("cfg,secs", [("c2", 10), ("c4", 30)])
def test_headline_logits_pinned(va, model, monkeypatch, cfg, secs, fma):
    """logits, not only tokens, pinned at C2 (32 x 10 s) and C4 (32 x 30 s),
    each as ONE B = 32 forward: every clip's frames 0::every (all 1000 classes) within atol 1e-4
    / rtol 1e-5 of the reference's (tests/golden/fwd_headline_logits.npz, the reference run in
    chunks of 8 / 4), in both scan modes (2: the default fused multiply-adds; 0: the reference
    tree op for op).  Every near-tie frame (reference top-2 margin < 2e-5, > 2x the largest
    |dlogit| measured) is compared in full and its top-1 must be the reference's."""
    monkeypatch.setenv("VASR_SCAN_FMA", fma)
    g = golden("fwd_headline_logits.npz")
    audio = t(S.make_audio(32, secs * 16000, seed=1234))
    with torch.no_grad():
        logits = model(va.compute_mel_spectrogram(audio))
    every = int(g[cfg + "_every"])
    got = logits[:, ::every].cpu().numpy()
    want = g[cfg + "_logits_sub"]
    assert got.shape == want.shape
    assert_logits(got, want, HEADLINE_TOL)
    ties = g[cfg + "_tie_idx"]
    if len(ties):
        rows = logits[torch.from_numpy(ties[:, 0]).long().to(DEV), torch.from_numpy(ties[:, 1]).long().to(DEV)]
        rows = rows.cpu().numpy()
        ref_rows = g[cfg + "_tie_logits"]
        assert_logits(rows, ref_rows, HEADLINE_TOL)
        top = rows.argmax(-1)
        ref_top = ref_rows.argmax(-1)
        bad = [(int(b), int(f)) for (b, f), x, y in zip(ties, top, ref_top) if x != y]
        assert not bad, f"{cfg}: near-tie frames whose top-1 differs from the reference: {bad}"
        d = np.abs(rows - ref_rows).max(-1)
        srt = np.sort(ref_rows, -1)
        margins = srt[:, -1] - srt[:, -2]
        from conftest import record_metric
        record_metric(f"{cfg}_near_ties", mode=fma, count=int(len(ties)), min_margin=float(margins.min()),
                      max_abs_dlogit_at_ties=float(d.max()), max_abs_dlogit_sub=float(np.abs(got - want).max()),
                      ties_below_max_dlogit=int((margins < float(np.abs(got - want).max())).sum()))


@pytest.mark.parametrize("M,N,K", [(1, 64, 192), (33, 1280, 192), (501, 1280, 192), (8016, 1280, 192), (16032, 1280, 192),
                                   (300, 1000, 192), (129, 96, 128), (77, 200, 100), (1024, 192, 192)])
@pytest.mark.parametrize("epi", ["none", "gelu", "softplus", "residual", "argmax"])
def test_gemm_rows_engine_bitwise_equals_tiles(va, M, N, K, epi):
    """The A-rows-stationary split GEMM (gemm_rows.hip, K = 128 / 192 after padding to 32)
    performs the tile kernel's MFMA sequence per output element: bitwise equal outputs, for
    every unpaired epilogue, ragged M and N, and K below the padded width."""
    from velocity_asr import _lib, ops
    g = torch.Generator().manual_seed(M + 3 * N + K)
    a = torch.randn(M, K, generator=g).to(DEV)
    w = (torch.randn(N, K, generator=g) / K ** 0.5).to(DEV)
    b = (torch.randn(N, generator=g) * 0.1).to(DEV)
    res = torch.randn(M, N, generator=g).to(DEV)
    kw = {"none": dict(epilogue=_lib.EPI_NONE), "gelu": dict(epilogue=_lib.EPI_GELU),
          "softplus": dict(epilogue=_lib.EPI_SOFTPLUS_FROM, n_out=N // 3),
          "residual": dict(epilogue=_lib.EPI_RESIDUAL, aux=res)}.get(epi)
    out = {}
    for eng in (1, 2):
        with ops.option(_lib.OPT_GEMM_ENGINE, eng):
            out[eng] = ops.gemm_argmax(a, w, b) if epi == "argmax" else ops.gemm(a, w, b, **kw)
    assert torch.equal(out[1], out[2])


def test_probe_clock_reports_clock_and_xcd_dispatch(va):
    """vasr_probe_clock (bench.py's machine record): a plausible shader clock and all 8 XCDs seen;
    the round-robin fraction is reported, not asserted (it is what the probe measures)."""
    from velocity_asr import ops
    m = ops.probe_clock(torch.device(DEV), blocks=512, iters=4000)
    assert 0.5 < m["clock_ghz"] < 3.5, m
    assert m["xcds_seen"] == 8 and 0.0 <= m["xcd_round_robin_frac"] <= 1.0, m
