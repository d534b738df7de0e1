"""pooled_attention_kernel (csrc/attn.hip) at every instantiation, key count, block edge and
limit, against a plain fp64 numpy softmax(q k^T / sqrt(hd)) v per utterance and head.

Tolerance, derived per case and never from the kernel's output: with
    e32 = max |fp32 numpy restatement - fp64|   (same two-pass max-then-exp order, on the host)
an output element may differ from the fp64 reference by
    max(2e-5 + 1e-5 |ref|,  4 * e32).
The first term is the project's bound for fp32 kernels on unit-scale data (header of
test_gpu_parity.py).  The second is for the large-score cases, where an fp32 score of magnitude
~100 already carries ~1e-5 of absolute error in the exponent whatever computes it; the factor 4
covers another accumulation order over hd and Kp and the device's expf (the convention of the CTC
loss and gradient tests; test_gemm_x3_accuracy_matches_f32 allows 2x torch fp32).

What reaches which instantiation (uniform = vasr_pooled_attention_f32, ragged = ..._var_f32):
    pooled_attention_kernel<8>   inst-h4x8, inst-h1x8, L*-h8x8, all uniform; inv-h8x8 ragged
    pooled_attention_kernel<12>  inst-h4x12, inst-h3x12 (heads straddle the block edge), kp*, L*-h4x12,
                                 ldq-h4x12, the score edges; ragged: ragged-kp20, ragged-kp64
    pooled_attention_kernel<16>  inst-h4x16, lds-kp64-a128
    pooled_attention_kernel<0>   inst-h4x1, h4x4, h4x5, h1x20, h2x32, lds-kp32-a256 (64 KiB), ldq-h4x5;
                                 ragged: ragged-h4x5

Measured on an MI355X, worst over the 40 compared launches: |kernel - fp64| is 0.25 of
the tolerance (edge-q30-h4x12: e32 1.06e-5, kernel 1.07e-5, the 4 x e32 term governs) and at most 0.024
of it on unit-scale data (lds-kp32-a256, 5.6e-7).  Against e32 itself the kernel's error is at most
2.5 x (inst-h4x1: 5.6e-7 against 2.3e-7, 0.017 of the tolerance) and 0.97-1.01 x in the large-score
and wide-value cases (q30, widev), whose errors are the largest (up to 0.18 on outputs near 1e6).
"""

import zlib

import numpy as np
import pytest
import torch

from conftest import record_error, record_metric

DEV = "cuda"
TOL = dict(atol=2e-5, rtol=1e-5)  # header of test_gpu_parity.py
FACTOR = 4.0


def C(name, L=65, Kp=20, heads=4, hd=12, B=3, flavor="unit", kps=None):
    return dict(name=name, B=B, L=L, Kp=Kp, heads=heads, hd=hd, flavor=flavor, kps=kps)


INSTANCES = [C(f"inst-h{h}x{d}", heads=h, hd=d)
             for h, d in ((4, 8), (4, 12), (4, 16), (4, 1), (4, 4), (4, 5), (1, 20), (2, 32), (1, 8))]
INSTANCES.append(C("inst-h3x12", L=129, heads=3, hd=12))  # 387 threads: token 85's heads sit in two blocks
KEYS = [C(f"kp{k}", Kp=k) for k in (1, 2, 63, 64)]
# L * heads: 4, 252, 256, 260, 516 with 4 heads; 8, 504, 512, 520, 1032 with 8
TOKENS = [C(f"L{L}-h{h}x{d}", L=L, heads=h, hd=d) for h, d in ((4, 12), (8, 8)) for L in (1, 63, 64, 65, 129)]
LDS = [C("lds-kp32-a256", L=33, Kp=32, heads=8, hd=32), C("lds-kp64-a128", L=33, Kp=64, heads=8, hd=16)]
EDGES = [C(f"edge-{f}-h{h}x{d}", flavor=f, heads=h, hd=d)
         for f in ("q30", "samekeys", "dominant", "widev") for h, d in ((4, 12), (4, 5))]
RAGGED = [C("ragged-kp20", Kp=20, kps=[20, 1, 11]), C("ragged-kp64", Kp=64, kps=[64, 1, 37]),
          C("ragged-h4x5", Kp=20, heads=4, hd=5, kps=[20, 1, 7])]
UNIFORM = INSTANCES + KEYS + TOKENS + LDS + EDGES
ALL = UNIFORM + RAGGED
ids = lambda c: c["name"]  # noqa: E731


def make_inputs(c):
    """q (B*L, A), kv (B*Kp, 2A) float32: row b*Kp + k holds key k then value k of utterance b."""
    rng = np.random.default_rng(zlib.crc32(c["name"].encode()))
    B, L, Kp, H, hd = c["B"], c["L"], c["Kp"], c["heads"], c["hd"]
    A = H * hd
    q = rng.standard_normal((B * L, A)).astype(np.float32)
    kv = rng.standard_normal((B * Kp, 2 * A)).astype(np.float32)
    f = c["flavor"]
    if f == "q30":  # nearly one-hot softmax, scores up to ~150
        q *= np.float32(30)
    elif f == "samekeys":  # p = 1 / Kp: the output is the mean of the value rows
        kv.reshape(B, Kp, 2 * A)[:, :, :A] = kv.reshape(B, Kp, 2 * A)[:, :1, :A]
    elif f == "dominant":  # key 3 scores 80 above the others for every query
        q.reshape(B * L, H, hd)[:, :, 0] = 1.0
        kv.reshape(B, Kp, 2, H, hd)[:, :, 0, :, 0] = 0.0
        kv.reshape(B, Kp, 2, H, hd)[:, 3, 0, :, 0] = np.float32(80 * np.sqrt(hd))
    elif f == "widev":  # values over 2^-20 .. 2^20
        kv[:, A:] *= np.exp2(rng.integers(-20, 21, (B * Kp, A))).astype(np.float32)
    else:
        assert f == "unit"
    if c["kps"] is not None:  # rows past an utterance's own keys must never be read
        for b, n in enumerate(c["kps"]):
            kv[b * Kp + n:(b + 1) * Kp] = np.nan
    return q, kv


def attention_ref(q, kv, c, dtype):
    """softmax(q k^T / sqrt(hd)) v per utterance and head over the utterance's own keys, all in
    `dtype`: scores, their row maximum, exp of the difference, then the weighted values over the sum."""
    B, L, Kp, H, hd = c["B"], c["L"], c["Kp"], c["heads"], c["hd"]
    A = H * hd
    q, kv = q.astype(dtype), kv.astype(dtype)
    out = np.empty((B * L, A), dtype)
    for b in range(B):
        n = Kp if c["kps"] is None else c["kps"][b]
        rows = kv[b * Kp:b * Kp + n]
        for h in range(H):
            cols = slice(h * hd, (h + 1) * hd)
            s = (q[b * L:(b + 1) * L, cols] @ rows[:, cols].T) / np.sqrt(dtype(hd))
            p = np.exp(s - s.max(axis=1, keepdims=True))
            out[b * L:(b + 1) * L, cols] = (p @ rows[:, A:][:, cols]) / p.sum(axis=1, keepdims=True)
    assert out.dtype == dtype
    return out


_refs = {}


def refs(c):
    """(q, kv, fp64 reference, e32, elementwise tolerance) of a case; computed once and shared."""
    if c["name"] not in _refs:
        q, kv = make_inputs(c)
        r64 = attention_ref(q, kv, c, np.float64)
        e32 = float(np.abs(attention_ref(q, kv, c, np.float32).astype(np.float64) - r64).max())
        tol = np.maximum(TOL["atol"] + TOL["rtol"] * np.abs(r64), FACTOR * e32)
        for a in (q, kv, r64, tol):
            a.setflags(write=False)
        _refs[c["name"]] = (q, kv, r64, e32, tol)
    return _refs[c["name"]]


# ----------------------------------------------------------------------------- host
def test_fp64_reference_against_a_scalar_loop():
    """The vectorised fp64 reference equals a per-(token, head, key) loop in Python floats."""
    c = C("loop", B=2, L=3, Kp=5, heads=2, hd=6, kps=[5, 2])
    q, kv, r64, _, _ = refs(c)
    A = 12
    for b in range(2):
        for t in range(3):
            for h in range(2):
                qr = q[b * 3 + t, h * 6:(h + 1) * 6].astype(np.float64)
                s = [float(qr @ kv[b * 5 + k, h * 6:(h + 1) * 6].astype(np.float64)) / 6 ** 0.5
                     for k in range(c["kps"][b])]
                p = [np.exp(x - max(s)) for x in s]
                want = sum(pk * kv[b * 5 + k, A + h * 6:A + (h + 1) * 6].astype(np.float64)
                           for k, pk in enumerate(p)) / sum(p)
                np.testing.assert_allclose(r64[b * 3 + t, h * 6:(h + 1) * 6], want, rtol=1e-13, atol=1e-15)


@pytest.mark.parametrize("c", ALL, ids=ids)
def test_references_agree(c):
    """fp32 restatement vs fp64: finite, within the project's bound on unit-scale data, and never so
    far off that 4 x its error would stop being a check (fp32 eps 6e-8 x scores up to ~200 x a few
    roundings is below 1e-4 of the largest output)."""
    q, kv, r64, e32, tol = refs(c)
    assert np.isfinite(r64).all() and np.isfinite(e32)
    scale = max(1.0, float(np.abs(r64).max()))
    if c["flavor"] == "unit":
        assert e32 <= TOL["atol"] + TOL["rtol"] * scale
    assert FACTOR * e32 <= 1e-4 * scale, (e32, scale)


def test_reference_closed_forms():
    """Identical keys give the mean of the value rows; one key gives its value row; the dominant
    key's weight is 1 to within exp(-60)."""
    for c in EDGES:
        q, kv, r64, _, _ = refs(c)
        B, L, Kp, A = c["B"], c["L"], c["Kp"], c["heads"] * c["hd"]
        v = kv.reshape(B, Kp, 2 * A)[:, :, A:].astype(np.float64)
        if c["flavor"] == "samekeys":
            np.testing.assert_allclose(r64.reshape(B, L, A), np.repeat(v.mean(1)[:, None], L, 1), rtol=1e-12, atol=1e-14)
        if c["flavor"] == "dominant":
            np.testing.assert_allclose(r64.reshape(B, L, A), np.repeat(v[:, 3][:, None], L, 1), rtol=0, atol=1e-20)
    c = KEYS[0]
    q, kv, r64, _, _ = refs(c)
    A = c["heads"] * c["hd"]
    np.testing.assert_array_equal(r64.reshape(c["B"], c["L"], A), np.repeat(kv[:, None, A:].astype(np.float64), c["L"], 1))


# ----------------------------------------------------------------------------- device
@pytest.fixture(scope="module")
def ops():
    from velocity_asr import _lib, ops
    _lib.require_device()
    _lib.load()
    return ops


def t(x):
    return torch.tensor(np.ascontiguousarray(x), device=DEV)  # copies: the shared inputs are read-only


def run(ops, c, q, kv, kps="case"):
    kps = c["kps"] if kps == "case" else kps
    k = None if kps is None else torch.tensor(kps, dtype=torch.int32, device=DEV)
    q = q if isinstance(q, torch.Tensor) else t(q)
    return ops.pooled_attention(q, t(kv), q.shape[0] // c["L"], c["L"], c["Kp"], c["heads"], kps=k)


def check(c, got):
    """|got - fp64| <= max(project bound, 4 e32) elementwise; the margins go to the parity log."""
    _, _, r64, e32, tol = refs(c)
    got = got.cpu().numpy().astype(np.float64)
    assert got.shape == r64.shape
    assert not np.isnan(got).any()
    err = np.abs(got - r64)
    record_error(got, r64, TOL)
    record_metric("pooled_attention", case=c["name"], e32=e32, e_hip=float(err.max()),
                  of_tolerance=float((err / tol).max()), of_e32=float(err.max() / e32) if e32 else 0.0)
    print(f"{c['name']}: e32 {e32:.3e} e_hip {err.max():.3e} worst err/tol {(err / tol).max():.3f}")
    bad = err > tol
    assert not bad.any(), f"{c['name']}: {bad.sum()} elements, worst err/tol {(err / tol).max():.2f} (e32 {e32:.3e})"


@pytest.mark.gpu
@pytest.mark.parametrize("c", ALL, ids=ids)
def test_against_fp64(ops, c):
    q, kv, _, _, _ = refs(c)
    got = run(ops, c, q, kv)
    check(c, got)
    A = c["heads"] * c["hd"]
    for b in range(c["B"]):  # one key: p = exp(0) = 1 and the sum is 1, so the value row comes back as it is
        if (c["Kp"] if c["kps"] is None else c["kps"][b]) == 1:
            want = t(kv[b * c["Kp"], A:]).expand(c["L"], A)
            assert torch.equal(got[b * c["L"]:(b + 1) * c["L"]], want)


@pytest.mark.gpu
@pytest.mark.parametrize("c", [C("ldq-h4x12"), C("ldq-h4x5", hd=5), C("ldq-ragged", kps=[20, 1, 9])], ids=ids)
def test_row_stride(ops, c):
    """q as a column slice of a wider buffer (ld_q = A + 10, not 16-byte aligned) whose other
    columns hold 1e30: same bits as the contiguous q, and within tolerance of fp64."""
    q, kv, _, _, _ = refs(c)
    A = q.shape[1]
    wide = torch.full((q.shape[0], A + 10), 1e30, device=DEV)
    wide[:, 3:3 + A] = t(q)
    view = wide[:, 3:3 + A]
    assert view.stride(0) == A + 10 and not view.is_contiguous()
    got = run(ops, c, view, kv)
    check(c, got)
    assert torch.equal(got, run(ops, c, q, kv))


@pytest.mark.gpu
@pytest.mark.parametrize("c", [INSTANCES[1], INSTANCES[5], TOKENS[4], C("inv-h8x8", heads=8, hd=8, kps=[20, 20, 20])]
                         + RAGGED, ids=ids)
def test_batch_invariance(ops, c):
    """Each utterance's rows of the B = 3 launch are bitwise those of the utterance launched alone."""
    q, kv, _, _, _ = refs(c)
    L, Kp = c["L"], c["Kp"]
    got = run(ops, c, q, kv)
    for b in range(c["B"]):
        alone = run(ops, c, q[b * L:(b + 1) * L], kv[b * Kp:(b + 1) * Kp],
                    kps=None if c["kps"] is None else [c["kps"][b]])
        assert torch.equal(got[b * L:(b + 1) * L], alone), f"utterance {b}"


@pytest.mark.gpu
@pytest.mark.parametrize("Kp,heads,hd,msg", [
    (65, 4, 12, "unsupported shape"),
    (16, 4, 33, "unsupported shape"),
    (16, 20, 13, "unsupported shape"),     # heads * head_dim = 260
    (16, 3, 5, "multiple of 4"),           # A = 15
    (64, 8, 32, "exceeds 64 KiB"),         # 128 KiB of keys and values
])
def test_refused_shapes(ops, Kp, heads, hd, msg):
    """Refused by the launcher before any launch; the output buffer of a refused call is not the test's."""
    A = heads * hd
    q = torch.zeros((2 * 5, A), device=DEV)
    kv = torch.zeros((2 * Kp, 2 * A), device=DEV)
    with pytest.raises(RuntimeError, match=msg):
        ops.pooled_attention(q, kv, 2, 5, Kp, heads)
    with pytest.raises(RuntimeError, match=msg):
        ops.pooled_attention(q, kv, 2, 5, Kp, heads, kps=torch.tensor([1, 1], dtype=torch.int32, device=DEV))


@pytest.mark.gpu
def test_var_entry_refuses_null_kps(ops):
    from velocity_asr import _lib
    q = torch.zeros((5, 48), device=DEV)
    kv = torch.zeros((16, 96), device=DEV)
    out = torch.full((5, 48), 7.0, device=DEV)
    rc = _lib.lib().vasr_pooled_attention_var_f32(q.data_ptr(), 48, kv.data_ptr(), out.data_ptr(), 1, 5, 16, 4, 12,
                                                  None, _lib.stream_of(q))
    with pytest.raises(RuntimeError, match="null kps"):
        _lib.check(rc, "vasr_pooled_attention_var_f32")
    assert bool((out == 7.0).all())
