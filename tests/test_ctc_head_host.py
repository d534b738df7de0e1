"""Host tests of the logit-free CTC head loss (no GPU): the shared fp64 helper of
ctc_head_cases.py against torch CPU fp64 autograd of the reference's composition, the C ABI of the
new symbols (declared, exported, typed, ABI 21), their argument checks (all return before any
launch), the dispatch of the new GEMM epilogue, and CTCHeadLoss's argument errors."""

import ctypes

import numpy as np
import pytest
import torch

import ctc_head_cases as H
from velocity_asr import _lib, ops
from velocity_asr.model import CTCOutputHead
from velocity_asr.training import CTCHeadLoss

NEW = ("vasr_lse_combine_f32", "vasr_ctc_head_emissions_f32", "vasr_ctc_grad_logits_stats_f32")
FAKE = 256  # an aligned non-null pointer value: the checks return before any dereference


@pytest.mark.parametrize("name", ["l7_repeat", "l33_v29", "ragged", "infeasible", "flat_targets"])
def test_fp64_helper_is_the_reference_composition(name):
    """nll, dX, dW, db of the helper = torch CPU fp64 autograd of F.linear -> F.log_softmax ->
    nn.CTCLoss, to 1e-10 relative."""
    for reduction in ("sum", "mean"):
        nll, dx, dw, db = H.reference_grads(name, torch.float64, reduction)
        want = H.nll_f64(name)
        fin = np.isfinite(want)
        assert np.array_equal(np.isfinite(nll) | (nll == 0), fin | (nll == 0))
        assert np.allclose(nll[fin], want[fin], rtol=1e-10, atol=0)
        for got, ref in zip(H.grads_f64(name, reduction), (dx, dw, db)):
            assert got.shape == ref.shape and H.rel_err(got, ref) <= 1e-10, (name, reduction)


def test_new_symbols_are_declared_exported_and_typed():
    lib = _lib.load()
    assert lib.vasr_version() == _lib.ABI_VERSION == 21
    with open(_lib.HEADER_PATH) as f:
        header = f.read()
    for n in NEW:
        assert n in _lib.header_functions() and n in _lib._SIGNATURES and hasattr(lib, n) and f" {n}(" in header, n
    assert "VASR_EPI_LSE = 9" in header and _lib.EPI_LSE == 9


def test_lse_epilogue_dispatch():
    """The new epilogue runs where the plain epilogue runs, under every engine option: on the same
    tile kernel, and on the rows engine at the shapes the plain head GEMM is sent there (the issue
    proposed the tile kernels only; with the logits' GEMM on the rows engine and the log-sum-exp
    GEMM on the tiles the logit-free forward lost at V = 5000, which the issue rules out, so the
    rows engine learnt the epilogue).  Every answer test_host.py pins for the existing epilogues
    is unchanged; 8 stays unknown."""
    lib = _lib.load()
    T128, T12864, T64, ROWS = 128128, 128064, 64064, 1
    shapes = ((16032, 1000, 192), (16032, 896, 192), (16032, 5000, 192), (33, 64, 128), (2881, 1000, 192),
              (7777, 1000, 100), (300, 1000, 192), (4008, 50000, 192), (1, 5, 36), (16032, 1000, 384))
    for engine in (0, 1, 2):
        with ops.option(_lib.OPT_GEMM_ENGINE, engine):
            for shape in shapes:
                assert ops.gemm_tile(*shape, epilogue=_lib.EPI_LSE) == ops.gemm_tile(*shape), (engine, shape)
    assert ops.gemm_tile(16032, 1000, 192, epilogue=_lib.EPI_LSE) == ROWS
    assert ops.gemm_tile(16032, 5000, 192, epilogue=_lib.EPI_LSE) == ROWS
    assert ops.gemm_tile(4096, 512, 192, epilogue=_lib.EPI_LSE) == ROWS
    assert ops.gemm_tile(4095, 512, 192, epilogue=_lib.EPI_LSE) != ROWS
    assert ops.gemm_tile(4096, 511, 192, epilogue=_lib.EPI_LSE) != ROWS
    assert ops.gemm_tile(2881, 1000, 192, epilogue=_lib.EPI_LSE) == T12864
    assert ops.gemm_tile(7777, 1000, 100, epilogue=_lib.EPI_LSE) == T128
    assert ops.gemm_tile(300, 1000, 192, epilogue=_lib.EPI_LSE) == T64
    assert ops.gemm_tile(4008, 50000, 192, epilogue=_lib.EPI_LSE) == T128
    with ops.option(_lib.OPT_GEMM_ENGINE, 1):
        assert ops.gemm_tile(16032, 1000, 192, epilogue=_lib.EPI_LSE) == T128
    with ops.option(_lib.OPT_GEMM_ENGINE, 2):
        assert ops.gemm_tile(33, 64, 128, epilogue=_lib.EPI_LSE) == ROWS
        assert ops.gemm_tile(16032, 1000, 384, epilogue=_lib.EPI_LSE) == T128  # K > 192: never the rows engine
    assert lib.vasr_gemm_tile(4, 64, 32, 1, _lib.EPI_LSE, 1) == -1 and b"fp32 only" in lib.vasr_last_error()
    assert lib.vasr_gemm_tile(4, 64, 32, 1, 8, 0) == -1 and b"unknown epilogue" in lib.vasr_last_error()
    assert lib.vasr_gemm_tile(4, 64, 32, 1, 10, 0) == -1 and b"unknown epilogue" in lib.vasr_last_error()
    # the existing epilogues at the shapes test_host.py lists
    K = 384
    assert ops.gemm_tile(7680, 1024, K) == T12864 and ops.gemm_tile(7681, 1024, K) == T128
    assert ops.gemm_tile(9088, 320, K) == T64 and ops.gemm_tile(12417, 640, K) == T128
    assert ops.gemm_tile(16032, 896, 192) == ROWS and ops.gemm_tile(16032, 384, 192) == T12864
    assert ops.gemm_tile(16032, 1000, 192, epilogue=_lib.EPI_ARGMAX) == T128
    assert ops.gemm_tile(16032, 896, 192, epilogue=_lib.EPI_RESIDUAL) == T128
    assert ops.gemm_tile(300, 448, 192, epilogue=_lib.EPI_PAIR_FUSION) == T12864


def _gemm_args(epi, ldc=2, qparams=None):
    a = _lib.GemmArgs()
    a.A = a.C = a.W = FAKE
    a.batch, a.M, a.N, a.K, a.lda, a.ldw, a.ldc = 1, 4, 64, 32, 32, 32, ldc
    a.epilogue = epi
    a.qparams = qparams
    return a


def test_lse_gemm_refuses_bad_arguments_before_any_launch():
    lib = _lib.load()
    err = lib.vasr_last_error
    assert lib.vasr_linear_x3_f32(ctypes.byref(_gemm_args(_lib.EPI_LSE, ldc=1)), FAKE, None) == -1
    assert b"lse pairs" in err() and b"slots" in err()  # N = 64 needs two slots
    a = _gemm_args(_lib.EPI_LSE)
    a.C = FAKE + 4
    assert lib.vasr_linear_x3_f32(ctypes.byref(a), FAKE, None) == -1 and b"8-byte aligned" in err()
    assert lib.vasr_linear_x3_f32(ctypes.byref(_gemm_args(_lib.EPI_LSE, qparams=FAKE)), FAKE, None) == -1
    assert b"qparams" in err()
    for epi in (8, 10, -1):
        assert lib.vasr_linear_x3_f32(ctypes.byref(_gemm_args(epi)), FAKE, None) == -1 and b"unknown epilogue" in err()


def test_lse_combine_refuses_bad_arguments_before_any_launch():
    lib = _lib.load()
    err = lib.vasr_last_error
    f = lib.vasr_lse_combine_f32
    assert f(None, 4, 4, 1, FAKE, None) == -1 and b"null" in err()
    assert f(FAKE, 4, 4, 1, None, None) == -1 and b"null" in err()
    assert f(FAKE + 4, 4, 4, 1, FAKE, None) == -1 and b"aligned" in err()
    assert f(FAKE, 3, 4, 1, FAKE, None) == -1 and b"ld=3" in err()  # leading dimension below the slots
    assert f(FAKE, 4, 0, 1, FAKE, None) == -1 and f(FAKE, 4, 4, -1, FAKE, None) == -1
    assert f(FAKE, 4, 4, 0, FAKE, None) == 0  # no rows: nothing to do


def _emis(**kw):
    a = dict(xn=FAKE, ld_x=192, W=FAKE, ldw=192, bias=FAKE, stats=FAKE, B=2, L=8, V=29, K=192, targets=FAKE, Smax=4,
             frames=FAKE, tlen=FAKE, blank=0, emis=FAKE, stream=None)
    a.update(kw)
    return _lib.load().vasr_ctc_head_emissions_f32(*a.values())


def test_head_emissions_refuses_bad_arguments_before_any_launch():
    err = _lib.load().vasr_last_error
    for k in ("xn", "W", "stats", "targets", "frames", "tlen", "emis"):
        assert _emis(**{k: None}) == -1 and b"null" in err(), k
    assert _emis(V=0) == -1 and b"bad shape" in err()
    assert _emis(L=8193) == -1 and b"bad shape" in err()
    assert _emis(L=0) == -1 and _emis(K=0) == -1 and _emis(B=-1) == -1
    assert _emis(ld_x=191) == -1 and b"ld_x=191" in err()
    assert _emis(ldw=100) == -1 and b"ldw=100" in err()
    assert _emis(blank=29) == -1 and b"blank" in err()
    assert _emis(Smax=2049) == -2 and b"Smax=2049" in err()
    # 65 rows x K floats of LDS: K = 252 is the last that fits 64 KiB
    assert _emis(K=256, ld_x=256, ldw=256) == -2 and b"LDS" in err() and b"K=256" in err()
    assert _emis(B=0) == 0 and _emis(B=0, K=252, ld_x=252, ldw=252) == 0
    assert _emis(B=0, bias=None) == 0 and _emis(B=0, targets=None, Smax=0) == 0


def _grad(**kw):
    a = dict(logits=FAKE, ld_row=29, ld_utt=8 * 29, B=2, L=8, V=29, stats=FAKE, targets=FAKE, Smax=4, frames=FAKE,
             tlen=FAKE, blank=0, occ=FAKE, scale=FAKE, workspace=FAKE, workspace_elems=10, stream=None)
    a.update(kw)
    return _lib.load().vasr_ctc_grad_logits_stats_f32(*a.values())


def test_grad_logits_stats_refuses_bad_arguments_before_any_launch():
    err = _lib.load().vasr_last_error
    for k in ("logits", "stats", "targets", "frames", "tlen", "occ", "scale", "workspace"):
        assert _grad(**{k: None}) == -1 and b"null" in err(), k
    assert _grad(V=0) == -1 and b"bad shape" in err()
    assert _grad(L=8193) == -1 and b"bad shape" in err()
    assert _grad(ld_row=28) == -1 and b"ld_row=28" in err()
    assert _grad(blank=-1) == -1 and b"blank" in err()
    assert _grad(Smax=2049) == -2 and b"Smax=2049" in err()
    assert _grad(workspace_elems=9) == -1 and b"workspace" in err()
    assert _grad(B=0) == 0


def test_head_loss_argument_errors():
    head = CTCOutputHead(d_model=16, vocab_size=9, dropout=0.0)
    with pytest.raises(ValueError, match="reduction"):
        CTCHeadLoss(head, reduction="avg")
    with pytest.raises(ValueError, match="fused"):
        CTCHeadLoss(head, fused="yes")
    with pytest.raises(ValueError, match="chunk_bytes"):
        CTCHeadLoss(head, chunk_bytes=0)
    with pytest.raises(TypeError, match="CTCOutputHead"):
        CTCHeadLoss(torch.nn.Linear(16, 9))
    x = torch.zeros(1, 4, 16, requires_grad=True)
    tg, il, tl = torch.tensor([[1, 2]]), torch.tensor([4]), torch.tensor([2])
    with pytest.raises(RuntimeError, match="forward-only"):
        CTCHeadLoss(head)(x, tg, il, tl)
    with pytest.raises(ValueError, match="features must be"):
        CTCHeadLoss(head)(torch.zeros(4, 16), tg, il, tl)
    # the loss does not adopt the head: the model owns its parameters
    assert not list(CTCHeadLoss(head).parameters()) and "head" not in dict(CTCHeadLoss(head).named_children())

    half = CTCOutputHead(d_model=16, vocab_size=9).to(torch.bfloat16)
    assert head.fusable() and not half.fusable()
    for kw in (dict(differentiable=True), dict(fused=True)):
        with pytest.raises(TypeError, match="float32 head"):
            CTCHeadLoss(half, **kw)
    CTCHeadLoss(half)  # forward-only: goes through its logits

    from velocity_asr import quantize as Q
    qat = CTCOutputHead(d_model=16, vocab_size=9)
    qat.proj[2] = Q.QuantizedLinear(16, 9)
    assert not qat.fusable()
    for kw in (dict(differentiable=True), dict(fused=True)):
        with pytest.raises(TypeError, match="float32 head"):
            CTCHeadLoss(qat, **kw)
    with pytest.raises(TypeError, match="float32 head"):
        qat.ctc_emissions(torch.zeros(1, 4, 16), tg, fused=True)


def test_only_training_exports_the_head_loss():
    import velocity_asr
    assert "CTCHeadLoss" not in velocity_asr.__all__ and not hasattr(velocity_asr, "CTCHeadLoss")
