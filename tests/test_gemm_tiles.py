"""The tile GEMM (csrc/gemm_x3.hip) on every tile shape, in both operand modes, under every epilogue,
against fp64 restatements written here (pytest -m gpu).  No golden file.

Every case first asks the library which kernel its call launches (ops.gemm_tile, the launchers' own
rule) and asserts the tile it is meant for, so a retune of the picker breaks the case instead of
silently moving it to another kernel.

Bounds.  The pre-activation acc + bias of element (m, n) is held to
    delta = c * (|a| @ |w|^T + |bias|)[m, n],
c = max(2 * r32, 2^-20), r32 = the worst ratio of torch's fp32 matmul on the same device against the same
per-element scale (the rule of test_gemm_x3_accuracy_matches_f32, per element instead of per matrix).  In
bf16 mode the reference is the fp64 product of A rounded to bf16 (RNE) and the bf16 W; products of two
bf16 numbers are exact in fp32, so the same scale and the same c hold, and the torch comparator gets the
rounded operands as fp32.  An activated epilogue f gets |f'(pre)| * delta (first order, fp64) plus f's
own envelope from test_fast_activation_* plus the fp32 roundings of its last operations.  No asserted
bound exceeds the old per-matrix rule 2e-5 * max(1, |ref|max): every tolerance is min(derived, that).
"""

import pytest
import torch

from conftest import record_metric

pytestmark = pytest.mark.gpu

DEV = "cuda"
T128, T12864, T64 = 128128, 128064, 64064
U = 2.0 ** -24  # unit roundoff of fp32
FLUSH = 2.0 ** -126  # smallest normal: what a flushed denormal result or operand may cost
E_ERF = 1.5e-7  # documented |erf error| of gelu_fast's Abramowitz & Stegun 7.1.26 form
Q_ROUND = 22 * U  # fp32 roundings of gelu_fast's q, counted in _gelu_env
# Worst error of softplus20_fast / sigmoid_fast on the sweeps of test_fast_activation_*, measured on an
# MI355X in units of their shapes (_softplus_shape, _sigmoid_shape); the tests assert twice these.
KAPPA_SOFTPLUS = 3.35  # measured 3.346
KAPPA_SIGMOID = 1.69  # measured 1.682


@pytest.fixture(scope="module")
def lib():
    import velocity_asr  # noqa: F401
    from velocity_asr import _lib
    _lib.require_device()
    _lib.load()
    return _lib


def _ops():
    from velocity_asr import ops
    return ops


def _assert_tile(want, M, N, K, batch=1, epi=0, bf16=False):
    got = _ops().gemm_tile(M, N, K, batch=batch, epilogue=epi, bf16=bf16)
    assert got == want, f"({M}, {N}, {K}) batch {batch} epilogue {epi} bf16 {bf16} launches {got}; this case is for {want}"
    return got


def _operands(M, N, K, seed, bf16, wide=False):
    """a (M, K) fp32 and w (N, K) fp32 or bf16 on the device, bias (N,), and the fp64 operands the kernel
    multiplies exactly (a rounded to bf16 in bf16 mode)."""
    g = torch.Generator().manual_seed(seed)
    a = torch.randn(M, K, generator=g)
    w = torch.randn(N, K, generator=g) / K ** 0.5
    if wide:  # operands over 2^-20 .. 2^20, as test_gemm_x3_accuracy_matches_f32
        a = a * torch.exp2(torch.randint(-20, 21, (M, K), generator=g).float())
        w = w * torch.exp2(torch.randint(-20, 21, (N, K), generator=g).float())
    b = torch.randn(N, generator=g) * 0.1
    a, w, b = a.to(DEV), w.to(DEV), b.to(DEV)
    if bf16:
        w = w.bfloat16()
        return a, w, b, a.bfloat16().double(), w.double()
    return a, w, b, a.double(), w.double()


def _preact(a64, w64, b):
    """fp64 reference of acc + bias, its per-element error bound delta, c and torch's fp32 ratio."""
    ref = a64 @ w64.T
    scale = a64.abs() @ w64.abs().T
    r32 = (((a64.float() @ w64.float().T).double() - ref).abs() / scale).max().item()
    assert r32 < 2 ** -16, r32  # the comparator itself is an fp32 GEMM
    c = max(2.0 * r32, 2.0 ** -20)
    if b is not None:
        ref = ref + b.double()
        scale = scale + b.double().abs()
    return ref, c * scale, c, r32


def _cap(ref):
    """The old rule of test_gemm_epilogues at the same shape: one scale per matrix."""
    fin = ref[torch.isfinite(ref)]
    return 2e-5 * max(1.0, fin.abs().max().item() if fin.numel() else 0.0)


def _check(got, ref, tol, what):
    """|got - ref| <= min(tol, old rule) per element; records the worst ratio to the bound."""
    cap = _cap(ref)
    tol = tol.clamp(max=cap)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    assert torch.isfinite(got).all(), what
    err = (got.double() - ref).abs()
    ratio = torch.where(err > 0, err / tol, torch.zeros_like(err)).max().item()
    capped = (tol >= cap).double().mean().item()
    record_metric(what, worst_ratio=ratio, max_abs=err.max().item(), cap=cap, at_cap=capped)
    print(f"{what}: worst |err| / bound {ratio:.3f}, max |err| {err.max().item():.3e}, old rule {cap:.3e}")
    assert ratio <= 1.0, (what, ratio, err.max().item())
    return ratio


# ----------------------------------------------------------------------------- fp64 activations
def _gelu(x):
    """x Phi(x) with Phi = erfc(-x / sqrt 2) / 2: 1 + erf(x / sqrt 2) without its cancellation in the negative tail."""
    return 0.5 * x * torch.special.erfc(-x * 0.7071067811865476)


def _gelu_d(x):
    return 0.5 * torch.special.erfc(-x * 0.7071067811865476) + x * torch.exp(-0.5 * x * x) * 0.3989422804014327


def _gelu_env(x, ref):
    """gelu_fast(x) = x (1 - q/2) for x >= 0 and x q/2 below, q ~ erfc(a), a = |x| / sqrt 2.  |q - erfc(a)| <=
    E_ERF (the formula, as documented) + Q_ROUND, the fp32 roundings of q, each relative to a value <= 1:
    a = |x| * const 1 (through erfc' a <= 0.5); t = rcp(fma) 3 ulp of t, through d(poly(t) t)/dt <= 3.5: 10;
    four Horner fmas at <= 1.5 each: 6; * t: 1; * exp: 1; v_exp_f32 itself: 2; its argument -a a log2 e,
    three roundings relative to a^2, through erfc(a) a^2 <= 0.16: 0.5; 21.5 in all, 22 asserted.  Both q and
    erfc(a) are below exp(-a^2) (poly(t) t <= 1 on (0, 1]), which bounds the difference in the tails.  Then
    x * fma(-0.5, q, 1) or 0.5 * x * q: two more roundings of the result."""
    eq = torch.minimum(torch.full_like(x, E_ERF + Q_ROUND), 2.0 * torch.exp(-0.5 * x * x))
    return 0.5 * x.abs() * eq + 2 * U * ref.abs() + FLUSH


def _softplus(x):
    return x.clamp(min=0) + torch.log1p(torch.exp(-x.abs()))


def _softplus_shape(x, ref):
    """softplus20_fast = max(x, 0) + l, l = log1p(e), e = exp2(-|x| log2 e): the rounding of the exponent is
    relative to |x| and reaches l through e / (1 + e) = sigmoid(-|x|); everything else is relative to the
    result.  Unit: one fp32 roundoff."""
    return U * (ref.abs() + x.abs() * torch.sigmoid(-x.abs())) + FLUSH


def _sigmoid_shape(x, ref):
    """sigmoid_fast = rcp(1 + exp2(-x log2 e)): the exponent's rounding is relative to |x| and reaches the
    result through 1 - sigmoid(x); rcp and the add are relative to the result."""
    return U * ref * (1.0 + x.abs() * (1.0 - ref)) + FLUSH


# ----------------------------------------------------------------------------- shapes
# The smallest shapes that reach each tile through the picker (486 tiles for 128 x 128, 358 for 128 x 64).
BIG = [  # (tile, M, N, K)
    (T128, 7681, 1024, 416),   # 488 tiles, one live row in the last M tile
    (T128, 7777, 1000, 36),    # 488, ragged M and N
    (T128, 12417, 640, 100),   # 490
    (T12864, 9217, 320, 240),  # 365
    (T12864, 5697, 512, 4),    # 360
    (T12864, 2881, 1000, 416),  # 368
]
SMALL = [(T64, 63, 33, 4), (T64, 64, 64, 36), (T64, 65, 65, 100), (T64, 300, 192, 240), (T64, 130, 1000, 416),
         (T64, 257, 768, 100), (T64, 1, 64, 36)]
WIDE = [(T128, 7777, 1000, 100), (T12864, 2881, 1000, 100), (T64, 65, 192, 100)]
# one ragged shape per tile for the epilogue cases
EPI_SHAPES = [(T128, 7777, 1000, 100), (T12864, 2881, 1000, 36), (T12864, 9217, 320, 100), (T64, 257, 200, 240)]
MODES = [pytest.param(False, id="x3"), pytest.param(True, id="bf16")]


def _id(c):
    return f"{c[0]}-{c[1]}x{c[2]}x{c[3]}"


# ----------------------------------------------------------------------------- a. accuracy
@pytest.mark.parametrize("bf16", MODES)
@pytest.mark.parametrize("case,wide", [(c, False) for c in BIG + SMALL] + [(c, True) for c in WIDE],
                         ids=[_id(c) for c in BIG + SMALL] + [_id(c) + "-wide" for c in WIDE])
def test_accuracy_per_element(lib, case, wide, bf16):
    """EPI_NONE with bias: |got - ref| <= c (|a| @ |w|^T + |bias|) per element, so a lost low-order plane
    (1.5e-5 relative) or one wrong row in a ragged tail cannot hide under a per-matrix scale."""
    tile, M, N, K = case
    _assert_tile(tile, M, N, K, bf16=bf16)
    a, w, b, a64, w64 = _operands(M, N, K, 100 + M + N + K, bf16, wide)
    ref, delta, c, r32 = _preact(a64, w64, b)
    got = _ops().gemm(a, w, b)
    record_metric("c", tile=tile, bf16=bf16, M=M, N=N, K=K, wide=wide, c=c, r32=r32)
    _check(got, ref, delta, f"none tile {tile} bf16 {bf16} ({M}, {N}, {K}) wide {wide} c {c:.3e}")


# ----------------------------------------------------------------------------- b. tile-independent bits
@pytest.mark.parametrize("bf16", MODES)
@pytest.mark.parametrize("case", BIG, ids=_id)
def test_large_tiles_bitwise_equal_64x64(lib, case, bf16):
    """An element's MFMA sequence depends on k alone, so its bits must not depend on the tile: 300-row
    slices (first, last, one straddling an M-tile edge), which the picker sends to 64 x 64, computed on
    their own are torch.equal to those rows of the large product.  NONE, GELU and RESIDUAL."""
    tile, M, N, K = case
    ops = _ops()
    a, w, b, _, _ = _operands(M, N, K, 200 + M + N + K, bf16)
    res = torch.randn(M, N, generator=torch.Generator().manual_seed(M)).to(DEV)
    edge = 128 * (M // 256)
    for epi in (lib.EPI_NONE, lib.EPI_GELU, lib.EPI_RESIDUAL):
        _assert_tile(tile, M, N, K, epi=epi, bf16=bf16)
        _assert_tile(T64, 300, N, K, epi=epi, bf16=bf16)
        kw = lambda lo, hi: dict(aux=res[lo:hi]) if epi == lib.EPI_RESIDUAL else {}
        big = ops.gemm(a, w, b, epilogue=epi, **kw(0, M))
        for lo in (0, M - 300, edge - 150):
            part = ops.gemm(a[lo:lo + 300], w, b, epilogue=epi, **kw(lo, lo + 300))
            assert torch.equal(part, big[lo:lo + 300]), (epi, lo, (part - big[lo:lo + 300]).abs().max().item())


# ----------------------------------------------------------------------------- f. batched tile order
@pytest.mark.parametrize("bf16", MODES)
@pytest.mark.parametrize("tile,M,N,K", [(T128, 1000, 640, 100), (T12864, 1000, 320, 36)])
def test_batched_tile_order(lib, tile, M, N, K, bf16):
    """Batch 13 x 40 tiles = 520 (520 % 8 != 0: the XCD runs are of unequal length): every batch's
    output is torch.equal to the same product as a batch-1 call (a 64 x 64 launch)."""
    ops = _ops()
    _assert_tile(tile, M, N, K, batch=13, bf16=bf16)
    _assert_tile(T64, M, N, K, bf16=bf16)
    g = torch.Generator().manual_seed(M + N)
    a = torch.randn(13, M, K, generator=g).to(DEV)
    w = (torch.randn(N, K, generator=g) / K ** 0.5).to(DEV)
    b = torch.randn(N, generator=g).to(DEV)
    if bf16:
        w = w.bfloat16()
    out = torch.full((13, M, N), float("nan"), device=DEV)
    ops.gemm_batched(a, K, M * K, M, 13, K, w, b, out, N, M * N)
    for z in range(13):
        assert torch.equal(out[z], ops.gemm(a[z], w, b)), z
    # against fp64 too (one batch: the others are bitwise its kind)
    a64 = (a[12].bfloat16() if bf16 else a[12]).double()
    ref, delta, c, _ = _preact(a64, w.double(), b)
    _check(out[12], ref, delta, f"batched none tile {tile} bf16 {bf16}")


# ----------------------------------------------------------------------------- c. epilogues against fp64
@pytest.mark.parametrize("bf16", MODES)
@pytest.mark.parametrize("case", EPI_SHAPES, ids=_id)
def test_unpaired_epilogues_vs_fp64(lib, case, bf16):
    """GELU, RESIDUAL with ld_aux > N, and SOFTPLUS_FROM at n_out in {0, 1, 31, 32, 33, BN - 1, BN, N - 1, N}
    (the per-32-column all / none / mixed decisions of the epilogue)."""
    tile, M, N, K = case
    ops = _ops()
    a, w, b, a64, w64 = _operands(M, N, K, 300 + M + N + K, bf16)
    pre, delta, c, _ = _preact(a64, w64, b)
    tag = f"tile {tile} bf16 {bf16} ({M}, {N}, {K})"

    _assert_tile(tile, M, N, K, epi=lib.EPI_GELU, bf16=bf16)
    ref = _gelu(pre)
    _check(ops.gemm(a, w, b, epilogue=lib.EPI_GELU), ref, _gelu_d(pre).abs() * delta + _gelu_env(pre, ref), "gelu " + tag)

    _assert_tile(tile, M, N, K, epi=lib.EPI_RESIDUAL, bf16=bf16)
    auxbuf = torch.randn(M, N + 12, generator=torch.Generator().manual_seed(N)).to(DEV)
    ref = pre + auxbuf[:, 4:4 + N].double()
    _check(ops.gemm(a, w, b, epilogue=lib.EPI_RESIDUAL, aux=auxbuf[:, 4:4 + N]), ref, delta + 2 * U * ref.abs(),
           "residual " + tag)

    _assert_tile(tile, M, N, K, epi=lib.EPI_SOFTPLUS_FROM, bf16=bf16)
    bn = tile % 1000
    sp = _softplus(pre)
    sp_tol = torch.sigmoid(pre) * delta + 2 * KAPPA_SOFTPLUS * _softplus_shape(pre, sp)
    cols = torch.arange(N, device=DEV)
    for n_out in sorted({0, 1, 31, 32, 33, bn - 1, bn, N - 1, N}):
        got = ops.gemm(a, w, b, epilogue=lib.EPI_SOFTPLUS_FROM, n_out=n_out)
        on = cols >= n_out
        _check(got, torch.where(on, sp, pre), torch.where(on, sp_tol, delta), f"softplus_from {n_out} " + tag)


@pytest.mark.parametrize("bf16", MODES)
@pytest.mark.parametrize("tile,M,N,K,lda", [(T128, 1000, 640, 240, 80), (T12864, 1000, 320, 240, 80),
                                            (T64, 65, 192, 240, 80)])
def test_gelu_pe_batched_overlapping_rows(lib, tile, M, N, K, lda, bf16):
    """GELU_PE as the temporal binding uses it: gemm_batched, batch 13, the positional table shared by
    every batch (stride_aux = 0) and overlapping A rows (lda < K)."""
    ops = _ops()
    B = 13
    _assert_tile(tile, M, N, K, batch=B, epi=lib.EPI_GELU_PE, bf16=bf16)
    g = torch.Generator().manual_seed(M + N + 1)
    span = ((M - 1) * lda + K + 3) // 4 * 4
    sig = torch.randn(B, span, generator=g).to(DEV)
    w = (torch.randn(N, K, generator=g) / K ** 0.5).to(DEV)
    b = (torch.randn(N, generator=g) * 0.1).to(DEV)
    pe = torch.randn(M, N, generator=g).to(DEV)
    if bf16:
        w = w.bfloat16()
    out = torch.full((B, M, N), float("nan"), device=DEV)
    ops.gemm_batched(sig, lda, span, M, B, K, w, b, out, N, M * N, epilogue=lib.EPI_GELU_PE, aux=pe, ld_aux=N,
                     stride_aux=0)
    for z in (0, 7, 12):
        rows = sig[z].unfold(0, K, lda)[:M]
        pre, delta, c, _ = _preact((rows.bfloat16() if bf16 else rows).double(), w.double(), b)
        ref = _gelu(pre) + pe.double()
        tol = _gelu_d(pre).abs() * delta + _gelu_env(pre, _gelu(pre)) + 2 * U * ref.abs()
        _check(out[z], ref, tol, f"gelu_pe tile {tile} bf16 {bf16} batch {z}")


def _pair_columns(n_out):
    """Paired layout: output column c = 32 j + r reads W rows 64 j + r (half 0) and 64 j + 32 + r (half 1)."""
    c = torch.arange(n_out, device=DEV)
    pc = 64 * (c // 32) + c % 32
    return pc, pc + 32


@pytest.mark.parametrize("bf16", MODES)
@pytest.mark.parametrize("tile,M,B,N,n_out", [(T12864, 98, 4, 448, 201), (T12864, 1001, 32, 448, 201),
                                              (T128, 1001, 13, 640, 201), (T128, 1001, 13, 640, 320)])
def test_pair_power_stft_geometry(lib, tile, M, B, N, n_out, bf16):
    """PAIR_POWER through gemm_batched at the STFT's geometry (K = 400, lda = 160 = the hop): out[m, c] =
    re^2 + im^2 of the paired W rows; columns >= n_out are not written."""
    ops = _ops()
    K, lda = 400, 160
    _assert_tile(tile, M, N, K, batch=B, epi=lib.EPI_PAIR_POWER, bf16=bf16)
    g = torch.Generator().manual_seed(M + N + n_out)
    span = ((M - 1) * lda + K + 3) // 4 * 4
    sig = torch.randn(B, span, generator=g).to(DEV)
    w = (torch.randn(N, K, generator=g) / K ** 0.5).to(DEV)
    if bf16:
        w = w.bfloat16()
    ldc = n_out + 3
    out = torch.full((B, M, ldc), -7.25e10, device=DEV)
    ops.gemm_batched(sig, lda, span, M, B, K, w, None, out, ldc, M * ldc, epilogue=lib.EPI_PAIR_POWER, n_out=n_out)
    assert (out[:, :, n_out:] == -7.25e10).all()
    p0, p1 = _pair_columns(n_out)
    for z in sorted({0, B // 2, B - 1}):
        rows = sig[z].unfold(0, K, lda)[:M]
        pre, delta, c, _ = _preact((rows.bfloat16() if bf16 else rows).double(), w.double(), None)
        v0, v1, d0, d1 = pre[:, p0], pre[:, p1], delta[:, p0], delta[:, p1]
        ref = v0 * v0 + v1 * v1
        tol = 2 * v0.abs() * d0 + 2 * v1.abs() * d1 + d0 * d0 + d1 * d1 + 4 * U * ref
        _check(out[z, :, :n_out], ref, tol, f"pair_power tile {tile} bf16 {bf16} n_out {n_out} batch {z}")


def _fq64(x, q):
    """fake_quant in fp64: q rows {scale, zero point, qmin, qmax}; scale 0 = not quantized."""
    s, zp, lo, hi = (q[:, i].double() for i in range(4))
    safe = torch.where(s == 0, torch.ones_like(s), s)
    xdq = (torch.minimum(torch.maximum(torch.round(x / safe + zp), lo), hi) - zp) * safe
    return torch.where(s == 0, x, xdq)


@pytest.mark.parametrize("bf16", MODES)
@pytest.mark.parametrize("quant", [False, True], ids=["plain", "qparams"])
@pytest.mark.parametrize("tile,M,N,n_out", [(T12864, 300, 448, 224), (T12864, 300, 448, 201), (T12864, 6500, 448, 201),
                                            (T128, 12417, 640, 320), (T128, 12417, 640, 201)])
def test_pair_fusion_vs_fp64(lib, tile, M, N, n_out, quant, bf16):
    """PAIR_FUSION against gemm_common.h's formula in fp64: gate = sigmoid((aux[pc] + v0) + bias[pc]),
    lt = aux[pc + 32] + aux2[c], gt = v1 + bias[pc + 32], out = gate lt + (1 - gate) gt, with n_out = N / 2
    (the model) and n_out < N / 2.  qparams: N entries in the paired layout, then n_out for the local
    projection (include/vasr.h).  Quantized columns get one level (qmin = qmax, a different value per
    column) or scale 0 (not quantized), so a column that reads another column's entry is off by the
    distance between levels while no result depends on which side of a rounding edge a value falls."""
    ops = _ops()
    K = 100
    _assert_tile(tile, M, N, K, epi=lib.EPI_PAIR_FUSION, bf16=bf16)
    a, w, b, a64, w64 = _operands(M, N, K, 400 + M + N + n_out, bf16)
    g = torch.Generator().manual_seed(n_out)
    aux = torch.randn(M, N + 8, generator=g).to(DEV)[:, :N]  # ld_aux > N
    aux2 = torch.randn(n_out, generator=g).to(DEV)
    qp = None
    if quant:
        qp = torch.zeros(N + n_out, 4)
        lvl = torch.arange(N + n_out).float()
        on = torch.rand(N + n_out, generator=g) < 0.6
        qp[:, 0] = torch.where(on, torch.full_like(lvl, 0.03125), torch.zeros_like(lvl))  # scale 2^-5
        qp[:, 1] = 3.0
        qp[:, 2] = qp[:, 3] = (lvl % 97) - 48  # the single level: (q - 3) / 32 in [-1.6, 1.5], period 97
        qp = qp.to(DEV)
    out = ops.gemm(a, w, b, epilogue=lib.EPI_PAIR_FUSION, aux=aux, aux2=aux2, n_out=n_out, qparams=qp)
    assert out.shape == (M, n_out)
    v, dv, c, _ = _preact(a64, w64, None)
    p0, p1 = _pair_columns(n_out)
    b64, x64 = b.double(), aux.double()
    gp = x64[:, p0] + v[:, p0] + b64[p0]
    lt = x64[:, p1] + aux2.double()
    gt = v[:, p1] + b64[p1]
    d_gp = dv[:, p0] + 2 * U * (x64[:, p0].abs() + v[:, p0].abs() + b64[p0].abs())
    d_lt = U * lt.abs()
    d_gt = dv[:, p1] + U * gt.abs()
    if quant:
        loc = torch.arange(N, N + n_out, device=DEV)
        for x, d, idx in ((gp, d_gp, p0), (lt, d_lt, loc), (gt, d_gt, p1)):
            qi = qp[idx]
            xq = _fq64(x, qi)
            fixed = (qi[:, 0] != 0).expand_as(x)
            d.copy_(torch.where(fixed, 4 * U * (x.abs() + xq.abs()), d))  # x + (xdq - x) in fp32
            x.copy_(xq)
    gate = torch.sigmoid(gp)
    ref = gate * lt + (1 - gate) * gt
    d_gate = gate * (1 - gate) * d_gp + 2 * KAPPA_SIGMOID * _sigmoid_shape(gp, gate)
    tol = (lt - gt).abs() * d_gate + gate * d_lt + (1 - gate) * d_gt + 4 * U * ((gate * lt).abs() + ((1 - gate) * gt).abs())
    _check(out, ref, tol, f"pair_fusion tile {tile} bf16 {bf16} ({M}, {N}) n_out {n_out} quant {quant}")


def _first_argmax(x):
    idx = torch.arange(x.shape[1], device=x.device).expand_as(x)
    return torch.where(x == x.max(1, keepdim=True).values, idx, torch.full_like(idx, x.shape[1])).min(1).values


@pytest.mark.parametrize("bf16", MODES)
@pytest.mark.parametrize("tile,M,N,K", [(T128, 7777, 1000, 100), (T12864, 2881, 1000, 36), (T64, 130, 1000, 240),
                                        (T64, 130, 33, 36), (T64, 65, 5, 4)])
def test_argmax_first_index_of_the_same_product(lib, tile, M, N, K, bf16):
    """ARGMAX against the first-index argmax of the same call's EPI_NONE output (bitwise consistent by
    construction), with exact ties planted by duplicated W rows.  64 x 64 in bf16 mode takes the DPP row
    reduction (its stage is under 16.5 KiB), every other kernel the LDS transpose."""
    ops = _ops()
    _assert_tile(tile, M, N, K, epi=lib.EPI_ARGMAX, bf16=bf16)
    _assert_tile(tile, M, N, K, bf16=bf16)
    a, w, b, _, _ = _operands(M, N, K, 500 + M + N + K, bf16)
    w, b = w.clone(), b.clone()
    for src, dst in ((0, N - 1), (1, 3), (N // 2, N // 2 - 1)):  # tied columns: equal rows and biases
        w[dst], b[dst] = w[src], b[src]
    b[[0, N - 1]] += 2.0  # and make one tied pair win often
    none = ops.gemm(a, w, b)
    want = _first_argmax(none)
    got = ops.gemm_argmax(a, w, b)
    assert got.dtype == torch.int32 and torch.equal(got.long(), want)
    hits = (want == 0).sum().item()
    assert hits > 0 and not (want == N - 1).any(), hits  # the planted tie was decided, and for the first index


# ----------------------------------------------------------------------------- d. nothing outside is touched
def _raw(lib, a, w, C, ldc, M, N, K, epi, bias=None):
    """One launch with a caller-owned C (ops.gemm without the output conveniences)."""
    ops = _ops()
    args = lib.GemmArgs()
    args.A, args.lda, args.stride_a = a.data_ptr(), a.stride(0), 0
    args.W, args.ldw = w.data_ptr(), w.stride(0)
    args.bias = lib.ptr(bias)
    args.C, args.ldc, args.stride_c = C.data_ptr(), ldc, 0
    args.batch, args.M, args.N, args.K = 1, M, N, K
    args.epilogue = epi
    ops._linear(args, w, lib.stream_of(a))


@pytest.mark.parametrize("bf16", MODES)
@pytest.mark.parametrize("tile,M,N,K", [(T128, 7777, 1000, 100), (T12864, 2881, 1000, 36), (T64, 65, 33, 100)])
def test_nothing_outside_is_written_or_read(lib, tile, M, N, K, bf16):
    """C is a view into a sentinel-filled buffer (ldc > N, rows past M) and A a view into a NaN-filled one
    (lda > K, NaN rows after row M - 1, NaN columns right of K; ragged M, N, K): the sentinels stay bitwise
    intact and the output is finite and within bound, so the clamped re-reads of row M - 1 and chunk 0
    are all the kernel substitutes.  The argmax keys likewise: every slot < ceil(N / 32) written, none
    beyond."""
    ops = _ops()
    _assert_tile(tile, M, N, K, bf16=bf16)
    a, w, b, a64, w64 = _operands(M, N, K, 600 + M + N + K, bf16)
    abuf = torch.full((M + 5, K + 8), float("nan"), device=DEV)
    abuf[:M, :K] = a
    SENT = -7.25e10
    cbuf = torch.full((M + 3, N + 5), SENT, device=DEV)
    ops.gemm(abuf[:M, :K], w, b, out=cbuf[:M, :N])
    assert (cbuf[M:] == SENT).all() and (cbuf[:, N:] == SENT).all()
    ref, delta, c, _ = _preact(a64, w64, b)
    _check(cbuf[:M, :N], ref, delta, f"sentinel tile {tile} bf16 {bf16}")

    _assert_tile(tile, M, N, K, epi=lib.EPI_ARGMAX, bf16=bf16)
    slots = (N + 31) // 32
    KSENT = -0x0123456789ABCDEF
    keys = torch.full((M + 3, slots + 2), KSENT, device=DEV, dtype=torch.int64)
    _raw(lib, abuf[:M, :K], w, keys, slots + 2, M, N, K, lib.EPI_ARGMAX, b)
    assert (keys[M:] == KSENT).all() and (keys[:, slots:] == KSENT).all()
    assert (keys[:M, :slots] != KSENT).all()
    # the keys decode to the first-index argmax of the product above: (ordered value << 32) | ~column
    hi = (keys[:M, :slots] >> 32) & 0xFFFFFFFF
    col = 0xFFFFFFFF - (keys[:M, :slots] & 0xFFFFFFFF)
    top = hi.max(1, keepdim=True).values
    got = torch.where(hi == top, col, torch.full_like(col, 1 << 40)).min(1).values
    assert torch.equal(got, _first_argmax(cbuf[:M, :N]))


# ----------------------------------------------------------------------------- e. the fast activations
def _sweep_points():
    """Pre-activations x_m (through A[m, 0] with W[n, 0] = 1: the split of a finite fp32 is exact) and
    b_n (through the bias: what cannot pass the MFMA -- infinities, NaN, denormals)."""
    ulp20 = float(torch.nextafter(torch.tensor(20.0), torch.tensor(30.0)) - 20.0)
    xs = torch.cat([torch.linspace(-12, 12, 4801), torch.linspace(-100, 100, 2001),
                    torch.tensor([0.0, 1e-30, -1e-30, 88.0, -88.0, 1e30, -1e30, 20.0, 20.0 + ulp20, 20.0 - ulp20,
                                  16.7, -16.7, 16.635532, -16.635532, -104.0, 87.3, -87.3, 0.75, -0.75])])
    bs = torch.tensor([0.0, -0.0, 1e-40, -1e-40, 2.0 ** -149, -2.0 ** -149, float("inf"), float("-inf"),
                       float("nan"), 0.3, -7.1, 3e-39])
    return xs, bs


def _sweep(lib, epi, **kw):
    ops = _ops()
    xs, bs = _sweep_points()
    M, N, K = xs.numel(), 64, 4
    _assert_tile(T64, M, N, K, epi=epi)
    a = torch.zeros(M, K)
    a[:, 0] = xs
    w = torch.zeros(N, K)
    w[:, 0] = 1.0
    b = torch.zeros(N)
    b[:bs.numel()] = bs
    pre = (xs[:, None] + b[None, :]).double().to(DEV)  # the kernel's fp32 add, restated in fp32
    return ops.gemm(a.to(DEV), w.to(DEV), b.to(DEV), epilogue=epi, **kw).double(), pre


def _compare_special(got, ref, pre, gelu=False):
    """NaN in, NaN out; infinities equal; returns the mask of finite points."""
    nan_ok = torch.isnan(got) == torch.isnan(ref)
    if gelu:  # x = -inf: the erf formula is -inf * 0 = NaN (nn.GELU too); the limit -0 is accepted as well
        nan_ok |= (pre == float("-inf")) & (got == 0)
    assert nan_ok.all()
    inf = torch.isinf(ref)
    assert torch.equal(got[inf], ref[inf])
    fin = torch.isfinite(ref)
    assert torch.isfinite(got[fin]).all()
    edge = fin & torch.isinf(pre)  # a finite limit at an infinite point (softplus(-inf) = 0): exact
    assert torch.equal(got[edge], ref[edge])
    return fin & torch.isfinite(pre)


def test_fast_activation_gelu(lib):
    """gelu_fast value by value against fp64 erf, inside the derived envelope of _gelu_env: a dense grid on
    [-12, 12], [-100, 100], +-0, denormals, +-1e-30, +-88, +-1e30, +-inf, NaN."""
    got, pre = _sweep(lib, lib.EPI_GELU)
    ref = _gelu(pre)
    fin = _compare_special(got, ref, pre, gelu=True)
    tol = _gelu_env(pre, ref)
    assert (tol[fin] <= 2e-5 * ref[fin].abs().clamp(min=1.0)).all()  # under the old rule, per element
    err = (got - ref).abs()[fin]
    ratio = (err / tol[fin]).max().item()
    bulk = (pre.abs() <= 12) & fin
    record_metric("gelu_fast", worst_ratio=ratio, max_abs_bulk=(got - ref).abs()[bulk].max().item())
    print(f"gelu_fast: worst |err| / envelope {ratio:.3f}, max |err| on [-12, 12] {(got - ref).abs()[bulk].max().item():.3e}")
    assert ratio <= 1.0


def test_fast_activation_softplus(lib):
    """softplus20_fast value by value against fp64 log1p(exp): the same points, the threshold (20 - ulp, 20,
    20 + ulp), +-16.7 and +-16.6355 (where 1 + e rounds to 1: d == 0), -104, -1e30.  The hardware exp / log
    / rcp carry no stated bound, so the envelope is twice the worst error measured on this sweep, in
    units of _softplus_shape."""
    got, pre = _sweep(lib, lib.EPI_SOFTPLUS_FROM, n_out=0)
    ref = _softplus(pre)
    fin = _compare_special(got, ref, pre)
    shape = _softplus_shape(pre, ref)
    assert (2 * KAPPA_SOFTPLUS * shape[fin] <= 2e-5 * ref[fin].abs().clamp(min=1.0)).all()
    kappa = ((got - ref).abs()[fin] / shape[fin]).max().item()
    record_metric("softplus20_fast", kappa=kappa, max_abs_bulk=(got - ref).abs()[(pre.abs() <= 12) & fin].max().item())
    print(f"softplus20_fast: measured kappa {kappa:.3f} (asserted {2 * KAPPA_SOFTPLUS})")
    assert kappa <= 2 * KAPPA_SOFTPLUS


def test_fast_activation_sigmoid(lib):
    """sigmoid_fast through PAIR_FUSION with lt = 1 and gt = 0, so out = gate exactly: gate pre-activations
    over [-100, 100] and +-inf.  Envelope: twice the worst measured error in units of _sigmoid_shape."""
    ops = _ops()
    xs, bs = _sweep_points()
    keep = ~torch.isnan(bs)
    M, N, K, n_out = xs.numel(), 64, 4, 32
    _assert_tile(T12864, M, N, K, epi=lib.EPI_PAIR_FUSION)
    a = torch.zeros(M, K)
    a[:, 0] = xs
    w = torch.zeros(N, K)
    w[:32, 0] = 1.0  # half 0: the gate; half 1 (global_proj) stays 0
    b = torch.zeros(N)
    b[:bs.numel()] = torch.where(keep, bs, torch.zeros_like(bs))
    aux = torch.zeros(M, N)
    aux[:, 32:] = 1.0  # lt = 1 + aux2 (0)
    out = ops.gemm(a.to(DEV), w.to(DEV), b.to(DEV), epilogue=lib.EPI_PAIR_FUSION, aux=aux.to(DEV),
                   aux2=torch.zeros(n_out, device=DEV), n_out=n_out).double()
    pre = (xs[:, None] + b[None, :32]).double().to(DEV)
    ref = torch.sigmoid(pre)
    assert torch.isfinite(out).all()
    assert (out[pre == float("inf")] == 1).all() and (out[pre == float("-inf")] == 0).all()
    fin = torch.isfinite(pre)
    out, pre, ref = out[fin], pre[fin], ref[fin]
    shape = _sigmoid_shape(pre, ref)
    assert (2 * KAPPA_SIGMOID * shape <= 2e-5).all()
    kappa = ((out - ref).abs() / shape).max().item()
    record_metric("sigmoid_fast", kappa=kappa, max_abs=(out - ref).abs().max().item())
    print(f"sigmoid_fast: measured kappa {kappa:.3f} (asserted {2 * KAPPA_SIGMOID})")
    assert kappa <= 2 * KAPPA_SIGMOID
