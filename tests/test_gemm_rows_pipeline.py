"""The wave-specialised rows GEMM's A prologue and accumulator hand-off (gemm_rows.hip,
gemm_rows_roles_kernel) against the LDS-ring tile engine: VASR_OPT_GEMM_ENGINE 1 / 2, outputs bitwise
equal.  tests/test_gemm_rows_roles.py covers the kernel's shapes in general; this file aims at the two
parts that have more than one form.

The prologue brings a compute wave's 32 rows in through its LDS staging tiles in passes of 64
K-columns (three at K = 192 / 180, two at 128 / 100), 4 rows per load instruction: ragged row counts
around the 32-row wave and the 128-row block, K below the padded width (zero fill inside the last
pass, and a whole zero k-step), a row stride wider than K, and an A that does not start its
allocation.

The hand-off has two barrier protocols, nc + 1 or nc + 2 barriers for a block of nc chunks: one
accumulator, and two, which the softplus epilogue without qparams runs (its arithmetic sits in the
compute waves, between the next chunk's MFMAs), the 8-byte-slot epilogues ARGMAX, LSE and ARGMAX_LSE
in a -DVASR_ROWS_ACC2=1 build and every epilogue in a -DVASR_ROWS_ACC2=2 build; the cases below hold
for either.  nc = 1 .. 5 come from one column group, which the launcher
takes when the row blocks alone fill more than one round of 256 blocks: groups() below is its rule,
and the cases assert the nc they mean to run.  M = 4100, N = 896 runs groups of 4 chunks, so both
staging tiles of every compute wave are written twice.

The tile engine's LSE pair sums its exponentials in another order than the rows engine, so for the
slot epilogues the reference is the tile engine's logits: a slot's key and maximum are exact
functions of the chunk's 32 logits (bitwise), and its sum of exponentials is checked against fp64
to 1e-5 relative (fast_exp: the argument's rounding after the log2(e) multiply, at most |x| 2^-24
with |x| < 32 here, about 2e-6, plus 32 positive terms added in fp32, 32 x 6e-8).
"""

import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
SIGN = -(1 << 63)


@pytest.fixture(scope="module")
def va():
    import velocity_asr
    from velocity_asr import _lib
    _lib.require_device()
    _lib.load()
    return velocity_asr


def groups(M, N, cus=256, max_group=16):
    """gemm_rows.hip's pick_groups for 128-row blocks -> (column groups, chunks per group)."""
    rb, NT = (M + 127) // 128, (N + 31) // 32
    best = None
    for g in range(1, NT + 1):
        pg = (NT + g - 1) // g
        if pg > max_group:
            continue
        gg = (NT + pg - 1) // pg
        cost = ((rb * gg + cus - 1) // cus) * (pg + 1)
        if best is None or cost < best[0]:
            best = (cost, gg, pg)
    return best[1], best[2]


@functools.lru_cache(maxsize=4)
def operands(M, N, K):
    g = torch.Generator(device=DEV).manual_seed(5 * M + 3 * N + K)
    a = torch.randn(M, K, device=DEV, generator=g)
    w = torch.randn(N, K, device=DEV, generator=g) / K ** 0.5
    b = torch.randn(N, device=DEV, generator=g) * 0.1
    return a, w, b


def engine(e):
    from velocity_asr import _lib, ops
    return ops.option(_lib.OPT_GEMM_ENGINE, e)


def both(fn):
    out = {}
    for e in (1, 2):
        with engine(e):
            out[e] = fn()
    return out[1], out[2]


# ------------------------------------------------------------------ the A prologue

MS = [1, 31, 33, 127, 128, 129, 257]


def a_view(M, K, form, gen):
    if form == "dense":
        return torch.randn(M, K, device=DEV, generator=gen)
    if form == "lda256":
        a = torch.randn(M, 256, device=DEV, generator=gen)[:, :K]
        assert a.stride(0) == 256
        return a
    # 12 floats into the allocation: 48 bytes, 16-byte aligned and no more
    flat = torch.randn(M * K + 12, device=DEV, generator=gen)
    a = flat[12:].view(M, K)
    assert a.storage_offset() == 12 and a.data_ptr() % 16 == 0 and a.data_ptr() % 64 != 0
    return a


@pytest.mark.parametrize("form", ["dense", "lda256", "offset"])
@pytest.mark.parametrize("K", [192, 180, 128, 100])
def test_prologue(va, K, form):
    from velocity_asr import ops
    gen = torch.Generator(device=DEV).manual_seed(K)
    w = torch.randn(96, K, device=DEV, generator=gen) / K ** 0.5
    b = torch.randn(96, device=DEV, generator=gen) * 0.1
    for M in MS:
        a = a_view(M, K, form, gen)
        t, r = both(lambda: ops.gemm(a, w, b))
        assert torch.equal(t, r), (M, K, form)


def test_prologue_then_recycled_tiles(va):
    """The prologue's staging image is overwritten by the first tiles: 4 chunks per block, strided A."""
    from velocity_asr import _lib, ops
    gen = torch.Generator(device=DEV).manual_seed(11)
    a = a_view(4100, 180, "lda256", gen)
    w = torch.randn(896, 180, device=DEV, generator=gen) / 180 ** 0.5
    b = torch.randn(896, device=DEV, generator=gen) * 0.1
    t, r = both(lambda: ops.gemm(a, w, b, epilogue=_lib.EPI_SOFTPLUS_FROM, n_out=512))
    assert torch.equal(t, r)


# ------------------------------------------------------------------ the barrier protocols

def ordered(keys):
    """uint64 keys held as int64 -> int64 in the same order."""
    return keys ^ SIGN


def expected_slots(logits):
    """Per 32-column chunk of the logits: the ARGMAX key (order-preserving bits of the maximum in the
    high word, 0xFFFFFFFF - first column of it in the low word), and the maximum itself."""
    M, N = logits.shape
    G = (N + 31) // 32
    u = logits.contiguous().view(torch.int32).to(torch.int64) & 0xFFFFFFFF
    ordb = torch.where((u & 0x80000000) != 0, ~u & 0xFFFFFFFF, u | 0x80000000)
    col = torch.arange(N, device=logits.device, dtype=torch.int64)
    key = (ordb << 32) | (0xFFFFFFFF - col)
    pad = torch.zeros((M, G * 32), device=logits.device, dtype=torch.int64)  # a column past N: key 0
    pad[:, :N] = key
    keys = ordered(ordered(pad).view(M, G, 32).max(-1).values)
    mx = torch.full((M, G * 32), float("-inf"), device=logits.device)
    mx[:, :N] = logits
    return keys, mx.view(M, G, 32).max(-1).values


def check_pairs(pairs, logits):
    M, N = logits.shape
    G = (N + 31) // 32
    _, mx = expected_slots(logits)
    assert torch.equal(pairs[..., 0], mx), "slot maxima differ from the logits'"
    x = torch.full((M, G * 32), float("-inf"), device=logits.device, dtype=torch.float64)
    x[:, :N] = logits.double()
    s64 = torch.exp(x.view(M, G, 32) - mx.double()[..., None]).sum(-1)
    rel = ((pairs[..., 1].double() - s64).abs() / s64).max().item()
    print(f"lse sums M={M} N={N}: max relative error {rel:.3e}")
    assert rel <= 1e-5, rel


EPIS = ["none", "softplus", "argmax", "lse", "argmax_lse"]


def run_epilogue(epi, M, N):
    """Engine 2's output for `epi` against what engine 1 says it must be."""
    from velocity_asr import _lib, ops
    a, w, b = operands(M, N, 192)
    G = (N + 31) // 32
    if epi in ("none", "softplus"):
        kw = dict(epilogue=_lib.EPI_SOFTPLUS_FROM, n_out=N // 2 + 8) if epi == "softplus" else {}
        t, r = both(lambda: ops.gemm(a, w, b, **kw))
        assert torch.equal(t, r)
        return r
    with engine(1):
        logits = ops.gemm(a, w, b)
        idx = ops.gemm_argmax(a, w, b)
    want_keys, _ = expected_slots(logits)
    with engine(2):
        if epi == "argmax":
            keys, slots, _ = ops._gemm_argmax_keys(a, w, b, None, None, "test")
            assert slots == G and torch.equal(keys, want_keys), "keys differ from the logits'"
            assert torch.equal(ops.gemm_argmax(a, w, b), idx)
            return keys
        if epi == "lse":
            a2, dims, wdims = ops._head_operands("test", a, w, b, None)
            pairs, slots = ops._gemm_lse_pairs(a2, w, b, dims, wdims)
            assert slots == G
            check_pairs(pairs, logits)
            return pairs
        buf = ops.gemm_argmax_lse(a, w, b)
    assert tuple(buf.shape) == (M, 2 * G)
    assert torch.equal(buf[:, 0::2], want_keys), "keys differ from the logits'"
    check_pairs(buf[:, 1::2].contiguous().view(torch.float32).view(M, G, 2), logits)
    return buf


@pytest.mark.parametrize("epi", EPIS)
@pytest.mark.parametrize("M,N,nc", [(33000, 32, 1), (33000, 64, 2), (33000, 96, 3), (49200, 128, 4), (33000, 160, 5)])
def test_chunks_per_block(va, M, N, nc, epi):
    """One column group of nc chunks (more row blocks than one round of 256 CUs): nc below, at and
    above the ring's depth and the two staging tiles, odd and even."""
    assert groups(M, N) == (1, nc)
    run_epilogue(epi, M, N)


@pytest.mark.parametrize("epi", EPIS)
def test_groups_of_four(va, epi):
    """M = 4100, N = 896: 33 row blocks x 7 interleaved groups of 4 chunks, a ragged last block."""
    assert groups(4100, 896) == (7, 4)
    run_epilogue(epi, 4100, 896)


@pytest.mark.parametrize("epi", ["softplus", "argmax_lse"])
def test_repeatable(va, epi):
    """The same inputs launched 10 times under each protocol: a hand-off that races shows as a difference."""
    outs = [run_epilogue(epi, 4100, 896) for _ in range(10)]
    assert all(torch.equal(o, outs[0]) for o in outs[1:])


# ------------------------------------------------------------------ the head

@pytest.mark.parametrize("M", [4100, 8016])
def test_head_argmax_under_auto(va, M):
    """The CTC head's argmax GEMM as the model launches it (engine 0): indices and row keys equal
    the tile engine's, whichever engine the rule names; the engine named is the one the shape's
    forced launch agrees with.  The rule was left as it was (the tiles): the host tests pin
    vasr_gemm_tile's answer at this shape, so this records the engine and checks both."""
    from velocity_asr import _lib, ops
    N, K = 1000, 192
    a, w, b = operands(M, N, K)
    named = ops.gemm_tile(M, N, K, epilogue=_lib.EPI_ARGMAX)
    with engine(2):
        assert ops.gemm_tile(M, N, K, epilogue=_lib.EPI_ARGMAX) == 1
    with engine(1):
        tiles = ops.gemm_tile(M, N, K, epilogue=_lib.EPI_ARGMAX)
        assert tiles != 1
        k1, slots, _ = ops._gemm_argmax_keys(a, w, b, None, None, "test")
        i1 = ops.gemm_argmax(a, w, b)
        logits = ops.gemm(a, w, b)
    print(f"argmax head M={M}: auto names engine {named} (tiles: {tiles}, rows: 1)")
    assert named in (1, tiles)
    k0, _, _ = ops._gemm_argmax_keys(a, w, b, None, None, "test")
    i0 = ops.gemm_argmax(a, w, b)
    assert torch.equal(i0, i1)
    # engines may spread a row's key over its slots differently: the row's key is their maximum
    assert torch.equal(ordered(k0).max(1).values, ordered(k1).max(1).values)
    if named == 1:  # the rows engine: one key per 32-column chunk
        assert torch.equal(k0, expected_slots(logits)[0])
    else:
        assert torch.equal(k0, k1)


@pytest.mark.parametrize("form", ["nobias", "qparams", "aligned"])
def test_softplus_forms(va, form):
    """The softplus epilogue's arithmetic runs in the compute waves unless the launch has qparams: without a
    bias, with qparams (the memory waves' form), and from a column on a chunk edge (512: chunks all below,
    all above; test_groups_of_four's 456 adds the mixed chunk)."""
    from velocity_asr import _lib, ops
    M, N = 4100, 896
    a, w, b = operands(M, N, 192)
    kw = dict(epilogue=_lib.EPI_SOFTPLUS_FROM, n_out=512)
    if form == "qparams":
        g = torch.Generator(device=DEV).manual_seed(7)
        scale = torch.rand(N, device=DEV, generator=g) * 0.05 + 0.01
        zp = torch.randint(-8, 8, (N,), device=DEV, generator=g).float()
        kw["qparams"] = torch.stack([scale, zp, torch.full_like(scale, -128.0), torch.full_like(scale, 127.0)], 1).contiguous()
    t, r = both(lambda: ops.gemm(a, w, None if form == "nobias" else b, **kw))
    assert torch.equal(t, r)
