"""Kernel-level tests of the gated and the bf16 SSM block tails (csrc/ssm_tail.hip:
vasr_ssm_block_tail_gated_f32, vasr_ssm_block_tail_bf16, vasr_ssm_block_tail_gated_bf16) against the
host references of ssm_tail_cases.py, at grids of 1 ... 18 row tiles -- the sizes the model never
launches the gated kernels at (it needs B L >= 4097), where a ragged last tile, the row clamp of the u
loads, the row guards of the yd loads and the XCD tile-order map at nblk < 8 and nblk % 8 != 0 run.

Every launch writes into an out pre-filled with NaN, so a row no workgroup wrote fails the comparison
whatever the allocator left there.

fp32 gated kernel: the fp32 bar against ref_f64(staged=False), gate saturation, bitwise equality with
the scan + tail composition it replaces, strides and write discipline.  bf16 kernels: the three row
conditions of ssm_tail_cases.conditions against ref_f64(staged=True) (measured figures: DESIGN.md §4),
row forms, strides."""

import functools

import numpy as np
import pytest
import torch

import ssm_tail_cases as C
from conftest import record_error, record_metric

pytestmark = pytest.mark.gpu
DEV = "cuda"
STRIDE_M = 77


def _t(a):
    return torch.from_numpy(np.array(a, dtype=np.float32)).to(DEV)


@functools.lru_cache(maxsize=None)
def _params(bf16):
    """The case parameters on the device, made once (ops caches weight planes by tensor identity); bf16:
    the four weight matrices as the bf16 parameters."""
    P = {k: _t(v) for k, v in C.params().items()}
    if bf16:
        for k in C.WEIGHTS:
            P[k] = P[k].to(torch.bfloat16)
    return P


@functools.lru_cache(maxsize=None)
def _inputs(M, seed=0):
    return tuple(_t(a) for a in C.inputs(M, seed))


def _nan(*shape):
    return torch.full(shape, float("nan"), device=DEV)


def _gated(yd, u, x, P, mode, out=None):
    from velocity_asr import ops
    out = _nan(yd.shape[0], C.D) if out is None else out
    return ops.ssm_block_tail_gated(yd, u, P["wz"], mode, x, P["wo"], P["ln_w"], P["ln_b"], C.EPS, P["w1"], P["b1"],
                                    P["w2"], P["b2"], out=out)


def _ungated(g, x, P, out=None):
    from velocity_asr import ops
    out = _nan(g.shape[0], C.D) if out is None else out
    return ops.ssm_block_tail(g, x, P["wo"], P["ln_w"], P["ln_b"], C.EPS, P["w1"], P["b1"], P["w2"], P["b2"], out=out)


def _run(kind, mode, yd, u, x, P, out=None):
    return _ungated(yd, x, P, out) if kind == "ungated" else _gated(yd, u, x, P, mode, out)


def _assert_fp32_bar(got, ref):
    tol = dict(atol=C.ATOL * max(1.0, float(np.abs(ref).max())), rtol=C.RTOL)
    record_error(got, ref, tol)
    np.testing.assert_allclose(got, ref, **tol)


# ------------------------------------------------------------------------------------------------
# vasr_ssm_block_tail_gated_f32
# ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", [0, 2], ids=["mode0", "mode2"])
@pytest.mark.parametrize("M", C.MS)
def test_gated_f32_matches_fp64(M, mode):
    """1 ... 18 row tiles (nblk < 8, nblk % 8 in {0, 1, 2}, ragged last tiles of 1, 31 and 1 rows)
    against the float64 gated tail: test_tail_matches_fp64's bar."""
    yd, u, x = _inputs(M)
    got = _gated(yd, u, x, _params(False), mode).cpu().numpy()
    _assert_fp32_bar(got, C.case_ref(M, 0, True, False))


@pytest.mark.parametrize("mode", [0, 2], ids=["mode0", "mode2"])
def test_gated_f32_gate_saturation(mode):
    """u scaled by 40: |z| passes 88.7 (fp32 exp overflows; 128 / log2 e, where exp2 does, is the same
    point) on both sides.  gate.h: for large negative z mode 2 forms z * rcp(inf) = -0 and mode 0
    z / inf = -0; for large positive z both form z / 1.  Neither has an inf * 0 or inf / inf, so the
    output is finite, and it is within the fp32 bar of the float64 gate."""
    yd, u, x = C.inputs(65, 3)
    u = (u * np.float32(40.0)).astype(np.float32)
    z = u.astype(np.float64) @ C.params()["wz"].astype(np.float64).T
    assert z.max() > 89.0 and z.min() < -89.0
    got = _gated(_t(yd), _t(u), _t(x), _params(False), mode).cpu().numpy()
    assert np.isfinite(got).all()
    _assert_fp32_bar(got, C.ref_f64(yd, u, x, C.params(), False))


@pytest.mark.parametrize("mode", [0, 2], ids=["mode0", "mode2"])
def test_gated_f32_zero_rows_of_u(mode):
    """A row of u at exactly 0 (and one at -0): z = 0, g = 0, the row's output is the tail of x alone."""
    yd, u, x = C.inputs(65, 4)
    u = u.copy()
    u[17] = 0.0
    u[64] = -0.0
    got = _gated(_t(yd), _t(u), _t(x), _params(False), mode).cpu().numpy()
    assert np.isfinite(got).all()
    ref = C.ref_f64(yd, u, x, C.params(), False)
    _assert_fp32_bar(got, ref)
    np.testing.assert_allclose(got[[17, 64]], C.ref_f64(np.zeros_like(yd), None, x, C.params(), False)[[17, 64]],
                               atol=C.ATOL * max(1.0, float(np.abs(ref).max())), rtol=C.RTOL)


@pytest.mark.parametrize("mode", [0, 2], ids=["mode0", "mode2"])
@pytest.mark.parametrize("B,L", [(1, 1), (1, 31), (3, 11), (1, 257), (5, 109)])
def test_gated_f32_bitwise_scan_then_tail(B, L, mode):
    """ssm_tail.hip's claim below the model's 4097 rows: z = gemm(u, wz) (vasr_linear_x3_f32, no bias),
    g = the streamed gated scan of [x | z], yd = the ungated scan of the same operands; then
    ssm_block_tail(g) and ssm_block_tail_gated(yd, u, wz) are bitwise equal.  (The ungated tail runs
    its default form, 16 rows here; its row forms are bitwise equal, test_tail_row_forms_bitwise_equal.)"""
    from velocity_asr import ops
    M, Di, N = B * L, C.E, 64
    gen = torch.Generator().manual_seed(1000 * B + L)
    r = lambda *s: torch.randn(*s, generator=gen).to(DEV)  # noqa: E731
    u, xs, x = r(M, C.D), r(M, Di), r(M, C.D)
    dt = torch.nn.functional.softplus(r(M, Di))
    bc = r(M, 2 * N)
    A2 = (-torch.exp(0.5 * r(N)) * ops.LOG2E).contiguous()
    Dv = r(Di)
    P = _params(False)
    z = ops.gemm(u, P["wz"])
    prev = ops.scan_form("streaming")
    try:
        g = ops.ssm_scan(torch.cat([xs, z], 1), dt, bc, A2, Dv, B, L, mode)
        yd = ops.ssm_scan_ungated(xs, dt, bc, A2, Dv, B, L, mode)
    finally:
        ops.scan_form(prev)
    a = _ungated(g, x, P)
    b = _gated(yd, u, x, P, mode)
    assert torch.isfinite(a).all()
    assert torch.equal(a, b), (a - b).abs().max().item()


def _strided(kind, mode, bf16):
    """M = 77 with yd, u and x as column slices of wider buffers (strides 896, 256 and 320, the
    neighbouring columns filled with other numbers) and out a window of a NaN buffer 64 columns and 32
    rows larger: bitwise the contiguous run, nothing written outside the window."""
    M = STRIDE_M
    P = _params(bf16)
    yd, u, x = _inputs(M, 5)
    want = _run(kind, mode, yd, u, x, P)
    assert torch.isfinite(want).all()
    gen = torch.Generator().manual_seed(11)
    wide = lambda n: torch.randn(M, n, generator=gen).to(DEV)  # noqa: E731
    by, bu, bx = wide(896), wide(256), wide(320)
    by[:, 128:128 + C.E] = yd
    bu[:, 64:64 + C.D] = u
    bx[:, 101:101 + C.D] = x
    frame = _nan(M + 32, C.D + 64)
    out = frame[16:16 + M, 31:31 + C.D]
    got = _run(kind, mode, by[:, 128:128 + C.E], bu[:, 64:64 + C.D], bx[:, 101:101 + C.D], P, out=out)
    assert got.data_ptr() == out.data_ptr()
    assert torch.equal(out, want), (out - want).abs().max().item()
    outside = torch.ones_like(frame, dtype=torch.bool)
    outside[16:16 + M, 31:31 + C.D] = False
    assert torch.isnan(frame[outside]).all()


@pytest.mark.parametrize("mode", [0, 2], ids=["mode0", "mode2"])
def test_gated_f32_strides_and_nan_frame(mode):
    _strided("gated", mode, False)


@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
def test_gated_refuses_bad_u(bf16):
    """A u that is not 16-byte aligned, or whose row stride is not a multiple of 4 floats, cannot be
    read by the kernel's float4 loads: refused with -1 and a message that names u."""
    M = STRIDE_M
    P = _params(bf16)
    yd, u, x = _inputs(M, 5)
    off = torch.zeros((M, 260), device=DEV)[:, 1:1 + C.D]      # ldu = 260, first element 4 bytes in
    odd = torch.zeros((M, 194), device=DEV)[:, :C.D]           # aligned, ldu = 194
    for bad in (off, odd):
        with pytest.raises(RuntimeError, match=r"code -1\).*: u \("):
            _gated(yd, bad, x, P, 2)


@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
def test_gated_m0_launches_nothing(bf16):
    """M = 0 returns VASR_OK before any launch (an empty torch tensor has a null data pointer, which
    the entry point refuses, so this goes to the library with real pointers): out stays as it was."""
    from velocity_asr import _lib, ops
    lib = _lib.lib()
    P = _params(bf16)
    yd, u, x = _inputs(STRIDE_M, 5)
    zprep, prep = (ops.pack_bf16, ops.pack_weights16) if bf16 else (ops.split_weights, ops.split_weights16)
    fn = lib.vasr_ssm_block_tail_gated_bf16 if bf16 else lib.vasr_ssm_block_tail_gated_f32
    out = _nan(32, C.D)
    rc = fn(yd.data_ptr(), C.E, u.data_ptr(), C.D, zprep(P["wz"]).data_ptr(), 2, x.data_ptr(), C.D,
            prep(P["wo"]).data_ptr(), P["ln_w"].data_ptr(), P["ln_b"].data_ptr(), C.EPS, prep(P["w1"]).data_ptr(),
            P["b1"].data_ptr(), prep(P["w2"]).data_ptr(), P["b2"].data_ptr(), out.data_ptr(), C.D, 0, C.D, C.E, None)
    assert rc == 0
    torch.cuda.synchronize()
    assert torch.isnan(out).all()


# ------------------------------------------------------------------------------------------------
# vasr_ssm_block_tail_bf16, vasr_ssm_block_tail_gated_bf16
# ------------------------------------------------------------------------------------------------

BF16_KERNELS = [("ungated", None), ("gated", 0), ("gated", 2)]
BF16_IDS = ["ungated", "gated-mode0", "gated-mode2"]


@pytest.mark.parametrize("kind,mode", BF16_KERNELS, ids=BF16_IDS)
def test_bf16_tail_rows_against_staged_fp64(kind, mode):
    """Every M of the fp32 test x three input seeds against ref_f64(staged=True), per output row
    (ssm_tail_cases.conditions): (a) every row within 4 E_ref, (b) the pooled share of rows outside the
    fp32 bar at most 4 s_ref, (c) no row position outside it under all three seeds -- E_ref and s_ref
    being ref_f32's own figures against ref_f64 over the same cases, computed here."""
    gated = kind == "gated"
    P = _params(True)
    pair = C.pair_stats(gated)
    per = {}
    for M in C.MS:
        for s in C.SEEDS:
            yd, u, x = _inputs(M, s)
            got = _run(kind, mode, yd, u, x, P).cpu().numpy()
            per[(M, s)] = C.row_errors(got, C.case_ref(M, s, gated, True))
    fails, st = C.conditions(per, pair)
    figures = dict(E_ref=pair["E_ref"], s_ref=pair["s_ref"], tight_ref=pair["tight"], e_max=st["E_ref"],
                   loose_share=st["s_ref"], loose_rows=st["loose_rows"], rows=st["rows"], tight=st["tight"])
    record_metric("ssm_tail_bf16_rows", kernel=kind, mode=mode, **figures)
    print(kind, mode, figures)
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("M", [17, 501])
def test_bf16_tail_row_forms_bitwise_equal(M):
    """The bf16 tail's 16- and 32-row workgroups of 4, 6 or 12 waves (weight prefetch depths 6 and 8,
    pd_of<1, ...>) against its 16 x 4 form: bitwise equal, as test_tail_row_forms_bitwise_equal asserts
    for the fp32 planes."""
    from velocity_asr import _lib, ops
    P = _params(True)
    g, _, x = _inputs(M, 6)
    with ops.option(_lib.OPT_TAIL_ROWS, 16), ops.option(_lib.OPT_TAIL_WAVES, 4):
        a = _ungated(g, x, P)
    assert torch.isfinite(a).all()
    for rows in (16, 32):
        for waves in (4, 6, 12):
            with ops.option(_lib.OPT_TAIL_ROWS, rows), ops.option(_lib.OPT_TAIL_WAVES, waves):
                b = _ungated(g, x, P)
            assert torch.equal(a, b), f"rows {rows} waves {waves}: {(a - b).abs().max().item()}"


@pytest.mark.parametrize("kind,mode", BF16_KERNELS, ids=BF16_IDS)
def test_bf16_tail_strides_and_nan_frame(kind, mode):
    _strided(kind, mode, True)
