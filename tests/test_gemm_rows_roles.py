"""The wave-specialised A-rows-stationary GEMM (gemm_rows.hip: compute waves hand each 32 x 32
accumulator to memory waves through LDS) against the LDS-ring tile engine: one launch per engine
(VASR_OPT_GEMM_ENGINE 1 / 2), outputs bitwise equal.  Forced engine 2 runs at any M, so the
shapes are the smallest that reach each path of the kernel.

A block is 128 rows x a run of nc 32-column chunks; the launcher takes as many column groups as
fit one round of 256 blocks, so nc = 1 until row blocks x chunks exceeds 256: the cases that
need nc = 2, 3 or a short last group use M = 33000 (258 row blocks, which is also a second
round), where N = 64 / 96 run as one group of 2 / 3 chunks and N = 900 (29 chunks, the last of
4 columns) as groups of 6, 6, 6, 6 and 5.  M = 4100 (33 row blocks) runs N = 896 as 7 groups of
4 chunks, so both staging tiles of every compute wave are used by every epilogue there.
"""

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"


@pytest.fixture(scope="module")
def va():
    import velocity_asr
    from velocity_asr import _lib
    _lib.require_device()
    _lib.load()
    return velocity_asr


def operands(M, N, K, lda=None):
    g = torch.Generator(device=DEV).manual_seed(M + 3 * N + K)
    a = torch.randn(M, lda or K, device=DEV, generator=g)[:, :K]
    w = torch.randn(N, K, device=DEV, generator=g) / K ** 0.5
    b = torch.randn(N, device=DEV, generator=g) * 0.1
    return a, w, b


def both(fn):
    from velocity_asr import _lib, ops
    out = {}
    for eng in (1, 2):
        with ops.option(_lib.OPT_GEMM_ENGINE, eng):
            out[eng] = fn()
    return out[1], out[2]


@pytest.mark.parametrize("M", [1, 31, 33, 127, 128, 129, 257])
def test_rows(va, M):
    """One compute wave partly filled, a block with idle compute waves, two blocks with a ragged
    second (and a third with one row)."""
    from velocity_asr import ops
    a, w, b = operands(M, 96, 192)
    t, r = both(lambda: ops.gemm(a, w, b))
    assert torch.equal(t, r)


@pytest.mark.parametrize("M,N", [(129, 32), (33000, 32), (33000, 64), (33000, 96), (33000, 900)])
def test_chunks_per_group(va, M, N):
    """nc = 1, 2, 3 (fewer chunks than the ring is deep, odd and even), and groups of 6 and 5
    with a ragged last chunk; M = 33000 also runs a second round of blocks."""
    from velocity_asr import _lib, ops
    a, w, b = operands(M, N, 192)
    t, r = both(lambda: ops.gemm(a, w, b, epilogue=_lib.EPI_SOFTPLUS_FROM, n_out=N // 2))
    assert torch.equal(t, r)


@pytest.mark.parametrize("K", [192, 180, 128, 100])
def test_k_below_the_padded_width(va, K):
    from velocity_asr import ops
    a, w, b = operands(129, 96, K)
    t, r = both(lambda: ops.gemm(a, w, b))
    assert torch.equal(t, r)


@pytest.mark.parametrize("epi", ["none", "nobias", "gelu", "softplus520", "softplus512", "residual", "argmax",
                                 "qparams"])
def test_epilogues(va, epi):
    """M = 4100, N = 896: 7 groups of 4 chunks (softplus from a column inside a chunk, 520, and
    on a chunk edge, 512)."""
    from velocity_asr import _lib, ops
    M, N = 4100, 896
    a, w, b = operands(M, N, 192)
    g = torch.Generator(device=DEV).manual_seed(7)
    if epi == "argmax":
        t, r = both(lambda: ops.gemm_argmax(a, w, b))
    else:
        kw = dict(epilogue=_lib.EPI_NONE)
        if epi == "gelu":
            kw = dict(epilogue=_lib.EPI_GELU)
        elif epi.startswith("softplus"):
            kw = dict(epilogue=_lib.EPI_SOFTPLUS_FROM, n_out=int(epi[8:]))
        elif epi == "residual":
            kw = dict(epilogue=_lib.EPI_RESIDUAL, aux=torch.randn(M, N, device=DEV, generator=g))
        elif epi == "qparams":
            scale = torch.rand(N, device=DEV, generator=g) * 0.05 + 0.01
            zp = torch.randint(-8, 8, (N,), device=DEV, generator=g).float()
            qp = torch.stack([scale, zp, torch.full_like(scale, -128.0), torch.full_like(scale, 127.0)], 1).contiguous()
            kw = dict(epilogue=_lib.EPI_GELU, qparams=qp)
        t, r = both(lambda: ops.gemm(a, w, None if epi == "nobias" else b, **kw))
    assert torch.equal(t, r)


@pytest.mark.parametrize("first", [100, 1], ids=["aligned", "unaligned"])
def test_ldc_wider_than_n(va, first):
    """C as columns first .. first + 896 of a 1280-wide buffer, as the block writes [x|B|C|dt]; a
    first column that is no multiple of 4 takes the dword stores.  Nothing outside is written."""
    from velocity_asr import _lib, ops
    M, N = 257, 896
    a, w, b = operands(M, N, 192)

    def run():
        buf = torch.full((M, 1280), -7.0, device=DEV)
        ops.gemm(a, w, b, epilogue=_lib.EPI_SOFTPLUS_FROM, n_out=512, out=buf[:, first:first + N])
        return buf
    t, r = both(run)
    assert torch.equal(t, r)
    assert (r[:, :first] == -7.0).all() and (r[:, first + N:] == -7.0).all()


def test_n_not_a_multiple_of_four(va):
    """N = 50: a lane's four columns straddle N, so the dword stores run."""
    from velocity_asr import _lib, ops
    a, w, b = operands(129, 50, 192)
    t, r = both(lambda: ops.gemm(a, w, b, epilogue=_lib.EPI_GELU))
    assert torch.equal(t, r)


def test_strided_a(va):
    from velocity_asr import ops
    a, w, b = operands(257, 96, 192, lda=256)
    assert a.stride(0) == 256
    t, r = both(lambda: ops.gemm(a, w, b))
    assert torch.equal(t, r)


def test_second_round(va):
    """M = 40000, N = 896: 313 row blocks x 4 groups of 7 chunks, five rounds of blocks."""
    from velocity_asr import _lib, ops
    a, w, b = operands(40000, 896, 192)
    t, r = both(lambda: ops.gemm(a, w, b, epilogue=_lib.EPI_SOFTPLUS_FROM, n_out=512))
    assert torch.equal(t, r)


def test_repeatable(va):
    """The same inputs launched 10 times: a hand-off that races shows as a difference."""
    from velocity_asr import _lib, ops
    a, w, b = operands(4100, 896, 192)
    with ops.option(_lib.OPT_GEMM_ENGINE, 2):
        outs = [ops.gemm(a, w, b, epilogue=_lib.EPI_SOFTPLUS_FROM, n_out=512) for _ in range(10)]
    with ops.option(_lib.OPT_GEMM_ENGINE, 1):
        ref = ops.gemm(a, w, b, epilogue=_lib.EPI_SOFTPLUS_FROM, n_out=512)
    assert all(torch.equal(o, ref) for o in outs)
