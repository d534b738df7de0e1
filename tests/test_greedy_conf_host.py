"""Host tests of the scored greedy decode (no GPU): the C ABI of the new symbols (declared, exported,
typed, ABI 21), the dispatch of VASR_EPI_ARGMAX_LSE, every argument check (all return before any
launch), the host references of greedy_conf_cases.py against each other, decode.token_confidences,
transcription.group_words with and without confidences, and the --confidence flag."""

import ctypes
import importlib.util
import os

import numpy as np
import pytest

import greedy_conf_cases as C
from conftest import PKG_ROOT
from velocity_asr import _lib, decode, ops
from velocity_asr.transcription import frames_to_seconds, group_words

NEW = ("vasr_argmax_logp_f32", "vasr_ctc_collapse_conf", "vasr_ctc_collapse_keys_conf")
FAKE = 256  # an aligned non-null pointer value: the checks return before any dereference
EPI = 11


def test_new_symbols_are_declared_exported_and_typed():
    lib = _lib.load()
    assert lib.vasr_version() == _lib.ABI_VERSION == 21
    with open(_lib.HEADER_PATH) as f:
        header = f.read()
    for n in NEW:
        assert n in _lib.header_functions() and n in _lib._SIGNATURES and hasattr(lib, n) and f" {n}(" in header, n
        assert getattr(lib, n).argtypes == _lib._SIGNATURES[n][0] and getattr(lib, n).restype is ctypes.c_int
    assert "VASR_EPI_ARGMAX_LSE = 11" in header and _lib.EPI_ARGMAX_LSE == EPI
    assert "8 and 10 are unassigned" in header
    for n in ("ScoredDecoding", "ctc_greedy_decode_with_confidence"):
        assert n in decode.__all__ and hasattr(decode, n)
    import velocity_asr
    assert "ScoredDecoding" not in velocity_asr.__all__


def test_argmax_lse_epilogue_dispatch():
    """The new epilogue runs wherever ARGMAX runs at that shape under every engine option (on the rows
    engine too when the option forces it); 8, 10 and 12 stay unknown; bf16 is refused."""
    lib = _lib.load()
    shapes = ((16032, 1000, 192), (16032, 896, 192), (16032, 5000, 192), (33, 64, 128), (2881, 1000, 192),
              (7777, 1000, 100), (300, 1000, 192), (4008, 50000, 192), (1, 5, 36), (16032, 1000, 384))
    for engine in (0, 1, 2):
        with ops.option(_lib.OPT_GEMM_ENGINE, engine):
            for shape in shapes:
                assert ops.gemm_tile(*shape, epilogue=EPI) == ops.gemm_tile(*shape, epilogue=_lib.EPI_ARGMAX), \
                    (engine, shape)
    assert ops.gemm_tile(16032, 1000, 192, epilogue=EPI) == 128128  # the head's shape: the 128 x 128 tile kernel
    assert ops.gemm_tile(16032, 5000, 192, epilogue=EPI) == 128128
    assert ops.gemm_tile(2881, 1000, 192, epilogue=EPI) == 128064 and ops.gemm_tile(300, 1000, 192, epilogue=EPI) == 64064
    with ops.option(_lib.OPT_GEMM_ENGINE, 2):
        assert ops.gemm_tile(33, 64, 128, epilogue=EPI) == 1
        assert ops.gemm_tile(16032, 1000, 384, epilogue=EPI) == 128128
    for epi in (8, 10, 12):
        assert lib.vasr_gemm_tile(4, 64, 32, 1, epi, 0) == -1 and b"unknown epilogue" in lib.vasr_last_error(), epi
    assert lib.vasr_gemm_tile(4, 64, 32, 1, EPI, 1) == -1 and b"fp32 only" in lib.vasr_last_error()
    # answers pinned for the existing epilogues
    assert ops.gemm_tile(16032, 1000, 192, epilogue=_lib.EPI_ARGMAX) == 128128
    assert ops.gemm_tile(16032, 1000, 192, epilogue=_lib.EPI_LSE) == 1 and ops.gemm_tile(16032, 896, 192) == 1


def _gemm_args(epi, ldc=4, qparams=None):
    a = _lib.GemmArgs()
    a.A = a.C = a.W = FAKE
    a.batch, a.M, a.N, a.K, a.lda, a.ldw, a.ldc = 1, 4, 64, 32, 32, 32, ldc
    a.epilogue = epi
    a.qparams = qparams
    return a


def test_argmax_lse_gemm_refuses_bad_arguments_before_any_launch():
    lib = _lib.load()
    err = lib.vasr_last_error
    assert lib.vasr_linear_x3_f32(ctypes.byref(_gemm_args(EPI, ldc=3)), FAKE, None) == -1  # N = 64 needs four slots
    assert b"argmax+lse" in err() and b"slots" in err()
    a = _gemm_args(EPI)
    a.C = FAKE + 4
    assert lib.vasr_linear_x3_f32(ctypes.byref(a), FAKE, None) == -1 and b"8-byte aligned" in err()
    assert lib.vasr_linear_x3_f32(ctypes.byref(_gemm_args(EPI, qparams=FAKE)), FAKE, None) == -1
    assert b"qparams" in err()
    assert lib.vasr_linear_bf16(ctypes.byref(_gemm_args(EPI)), FAKE, None) == -1 and b"fp32 only" in err()
    for epi in (8, 10, 12, -1):
        assert lib.vasr_linear_x3_f32(ctypes.byref(_gemm_args(epi)), FAKE, None) == -1 and b"unknown epilogue" in err()


def test_argmax_logp_refuses_bad_arguments_before_any_launch():
    lib = _lib.load()
    err = lib.vasr_last_error
    f = lib.vasr_argmax_logp_f32
    for k in range(3):
        ptrs = [FAKE, FAKE, FAKE]
        ptrs[k] = None
        assert f(ptrs[0], 8, 2, 8, ptrs[1], ptrs[2], None) == -1 and b"null" in err()
    assert f(FAKE, 8, 2, 0, FAKE, FAKE, None) == -1 and b"bad shape" in err()
    assert f(FAKE, 7, 2, 8, FAKE, FAKE, None) == -1 and b"ld=7" in err()
    assert f(FAKE, 8, -1, 8, FAKE, FAKE, None) == -1
    assert f(FAKE, 8, 0, 8, FAKE, FAKE, None) == 0  # no rows: nothing to do


def _conf(**kw):
    a = dict(pred=FAKE, logp=FAKE, B=2, L=8, frames=FAKE, blank=0, tokens=FAKE, len=FAKE, start=FAKE, end=FAKE,
             logp_sum=FAKE, logp_min=FAKE, path=FAKE, stream=None)
    a.update(kw)
    return _lib.load().vasr_ctc_collapse_conf(*a.values())


def _keys_conf(**kw):
    a = dict(slots=FAKE, ld=4, nslots=4, B=2, L=8, frames=FAKE, blank=0, pred=None, logp=None, tokens=FAKE, len=FAKE,
             start=FAKE, end=FAKE, logp_sum=FAKE, logp_min=FAKE, path=FAKE, stream=None)
    a.update(kw)
    return _lib.load().vasr_ctc_collapse_keys_conf(*a.values())


@pytest.mark.parametrize("call,inputs", [(_conf, ("pred", "logp")), (_keys_conf, ("slots",))])
def test_collapse_conf_refuses_bad_arguments_before_any_launch(call, inputs):
    err = _lib.load().vasr_last_error
    for k in inputs + ("tokens", "len", "start", "end", "logp_sum", "logp_min", "path"):
        assert call(**{k: None}) == -1 and b"null" in err(), k
    assert call(L=0) == -1 and b"bad shape" in err() and b"L=0" in err()
    assert call(L=8193) == -1 and b"bad shape" in err() and b"L=8193" in err()
    assert call(B=-1) == -1 and b"bad shape" in err()
    assert call(B=0) == 0 and call(B=0, frames=None) == 0  # no utterances: nothing to do


def test_collapse_keys_conf_refuses_bad_slots_before_any_launch():
    err = _lib.load().vasr_last_error
    assert _keys_conf(slots=FAKE + 4) == -1 and b"8-byte aligned" in err()
    assert _keys_conf(ld=3) == -1 and b"ld=3" in err()  # leading dimension below the used slots
    assert _keys_conf(nslots=3) == -1 and b"even" in err()  # a key and a pair per group
    assert _keys_conf(nslots=0) == -1


@pytest.mark.parametrize("seed", range(6))
def test_collapse_restatement_is_the_brute_force(seed):
    """The vectorised float64 restatement the GPU tests compare against = the oracle's timestamped greedy
    decode plus plain loops, on random small predictions with long runs, blanks and ragged lengths."""
    rng = np.random.default_rng(seed)
    B, L, V = 5, int(rng.integers(1, 40)), 4
    pred = np.repeat(rng.integers(0, V, size=(B, L)), 3, axis=1)[:, :L]  # runs of up to three
    pred[0] = 0  # an all-blank utterance
    if L > 2:
        pred[1] = 2  # one run over the whole utterance
    logp = -rng.random((B, L)) * 5
    frames = [L, L, 0, L + 7, -3][:B] if seed % 2 else None
    if frames is not None and L > 1:
        frames[0] = L - 1
    a, b = C.collapse_conf_ref(pred, logp, 0, frames), C.collapse_conf_brute(pred, logp, 0, frames)
    for x, y in zip(a, b):
        assert x["tokens"] == y["tokens"] and x["spans"] == y["spans"]
        assert np.array_equal(x["min"], y["min"])
        assert np.allclose(x["sum"], y["sum"], rtol=1e-13, atol=0) and abs(x["path"] - y["path"]) <= 1e-12
    if frames is not None:
        assert a[2]["tokens"] == [] and a[2]["path"] == 0.0 and a[4]["tokens"] == []


def test_token_confidences():
    lsum, lmin, n = np.float32([-0.6, -0.1, -3.0]), np.float32([-0.4, -0.1, -2.0]), [3, 1, 2]
    assert np.allclose(decode.token_confidences(lsum, lmin, n), np.exp([-0.2, -0.1, -1.5]), rtol=1e-6)
    assert np.allclose(decode.token_confidences(lsum, lmin, n, "mean"), decode.token_confidences(lsum, lmin, n))
    assert np.allclose(decode.token_confidences(lsum, lmin, n, "min"), np.exp([-0.4, -0.1, -2.0]), rtol=1e-6)
    assert np.allclose(decode.token_confidences(lsum, lmin, n, "prod"), np.exp([-0.6, -0.1, -3.0]), rtol=1e-6)
    assert decode.token_confidences([], [], []) == []
    with pytest.raises(ValueError, match="aggregation"):
        decode.token_confidences(lsum, lmin, n, "median")
    r = decode.ScoredDecoding([3], [(0, 2)], [0.5], -1.0)
    assert (r.tokens, r.timestamps, r.confidences, r.score) == ([3], [(0, 2)], [0.5], -1.0)


def test_group_words_with_and_without_confidences():
    vocab = decode.create_default_vocabulary(64)
    ids = [vocab.index(c) for c in "hi yo"] + [vocab.index(" ")] + [vocab.index("a")]
    spans = [(2 * k, 2 * k + 1) for k in range(len(ids))]
    conf = [0.9, 0.5, 0.01, 0.8, 0.7, 0.02, 0.6]  # the separators' values never count
    plain = group_words(ids, spans, vocab)
    assert plain == [{"word": "hi", "start": frames_to_seconds(0), "end": frames_to_seconds(5)},
                     {"word": "yo", "start": frames_to_seconds(6), "end": frames_to_seconds(11)},
                     {"word": "a", "start": frames_to_seconds(12), "end": frames_to_seconds(13)}]
    scored = group_words(ids, spans, vocab, conf)
    assert [w["confidence"] for w in scored] == [0.5, 0.7, 0.6]
    assert [{k: v for k, v in w.items() if k != "confidence"} for w in scored] == plain
    assert group_words(ids, spans, vocab, None) == plain and group_words([], [], vocab, []) == []
    with pytest.raises(ValueError, match="confidences"):
        group_words(ids, spans, vocab, conf[:-1])


def test_confidence_flag_parses():
    spec = importlib.util.spec_from_file_location("transcribe_cli", os.path.join(PKG_ROOT, "scripts", "transcribe.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert mod.parse_args(["a.wav", "--checkpoint", "m.pt"]).confidence is False
    args = mod.parse_args(["a.wav", "--checkpoint", "m.pt", "--confidence", "--format", "json"])
    assert args.confidence is True and args.timestamps is False
