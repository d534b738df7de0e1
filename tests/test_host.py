"""CPU-side tests: C ABI exports, module/state_dict contract, checkpoint format, host logic.

No kernel is launched here (there is no GPU in the build container); the GPU parity
tests are in test_gpu_parity.py (pytest -m gpu).
"""

import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import REPO, golden_json
from velocity_asr import synthetic as S


def test_c_abi_library_exports_every_header_symbol():
    from velocity_asr import _lib
    names = _lib.header_functions()
    assert "vasr_ssm_scan_f32" in names and "vasr_linear_x3_f32" in names
    lib = ctypes.CDLL(_lib.LIB_PATH)
    missing = [n for n in names if not hasattr(lib, n)]
    assert not missing, missing
    assert lib.vasr_version() == _lib.ABI_VERSION
    # every declared symbol has a typed binding
    assert set(names) <= set(_lib._SIGNATURES)


def test_abi_rejects_bad_arguments_without_gpu():
    """Argument validation happens before any launch, so it is testable on the host."""
    from velocity_asr import _lib
    L = _lib.load()
    rc = L.vasr_ssm_scan_f32(None, 0, None, 0, None, 0, None, None, None, 0, 1, 1, 384, 64, 0, None)
    assert rc == -1 and b"null" in L.vasr_last_error()
    # modes 0 (tree), 1 (recurrence), 2 (tree with fused multiply-adds); anything else is refused
    fake = 256  # aligned non-null pointer values: the checks return before any dereference
    rc = L.vasr_ssm_scan_f32(fake, 768, fake, 384, fake, 128, fake, fake, fake, 384, 1, 1, 384, 64, 3, None)
    assert rc == -1 and b"mode" in L.vasr_last_error()
    rc = L.vasr_ctc_collapse(None, 1, 1, 0, 1, None, None, None, None, None)
    assert rc == -1
    args = _lib.GemmArgs()
    assert L.vasr_linear_x3_f32(ctypes.byref(args), None, None) == -1
    assert L.vasr_linear_bf16(ctypes.byref(args), None, None) == -1
    assert L.vasr_split_weights_bf16x3(None, 4, 4, 4, None, None) == -1
    assert L.vasr_split_weights_elems(70, 100) == 3 * 96 * 128
    # front end: null pointers and too-short audio are rejected before any launch
    assert L.vasr_stft_power_400_f32(None, 0, 1, 1000, None, None, 201, 201, None) == -1
    # GEMM shape rules: K a multiple of 4
    args = _lib.GemmArgs()
    args.A = args.C = args.W = 16
    args.batch, args.M, args.N, args.K, args.lda, args.ldw, args.ldc = 1, 4, 4, 34, 36, 36, 4
    assert L.vasr_linear_x3_f32(ctypes.byref(args), 16, None) == -1
    assert b"multiples of 4" in L.vasr_last_error()


def test_tuning_options():
    """vasr_set_option: launcher decomposition knobs (never numerics), query with value < 0,
    unknown keys / values refused."""
    from velocity_asr import _lib, ops
    L = _lib.load()
    for key, allowed in ((_lib.OPT_SCAN_LANES, (2, 4)), (_lib.OPT_SCAN_CHUNK, (16, 32)), (_lib.OPT_TAIL_ROWS, (16, 32)),
                         (_lib.OPT_GEMM_ENGINE, (1, 2)), (_lib.OPT_TAIL_WAVES, (4, 6, 12)),
                         (_lib.OPT_SCAN_SPLIT, (1, 2)), (_lib.OPT_DW_ROWS, (4, 8, 16))):
        base = L.vasr_set_option(key, -1)
        assert base in (0,) + allowed
        for v in allowed:
            with ops.option(key, v):
                assert L.vasr_set_option(key, -1) == v
            assert L.vasr_set_option(key, -1) == base
        assert L.vasr_set_option(key, 3) == -1 and b"not allowed" in L.vasr_last_error()
    assert L.vasr_set_option(7, 0) == -1 and b"unknown option" in L.vasr_last_error()


def test_public_api_matches_reference_all():
    import velocity_asr as v
    expected = {"VELOCITYASR", "VelocityASRConfig", "from_pretrained", "TemporalBindingLayer", "CTCOutputHead",
                "SelectiveSSM", "SSMBlock", "LocalSSMProcessor", "GlobalSSM", "ScanMode", "MAMBA_AVAILABLE",
                "HierarchicalGlobalContext", "AdaptivePool", "MultiHeadAttention", "GatedFusion", "load_audio",
                "compute_mel_spectrogram", "MelSpectrogramTransform", "audio_to_frames", "frames_to_audio",
                "pad_or_trim", "SAMPLE_RATE", "N_FFT", "HOP_LENGTH", "N_MELS", "ctc_greedy_decode",
                "ctc_greedy_decode_with_timestamps", "ctc_beam_search", "CTCDecoder", "DecodingResult",
                "create_default_vocabulary", "ASRDataset", "ASRCollator", "LibriSpeechDataset",
                "create_dataloader", "create_librispeech_dataloaders", "__version__", "__author__"}
    assert expected == set(v.__all__)
    for n in expected:
        assert hasattr(v, n), n
    from velocity_asr.audio import SAMPLE_RATE, HOP_LENGTH  # scripts/transcribe.py:33
    from velocity_asr.training import compute_wer, compute_cer  # scripts/evaluate.py:31
    assert (SAMPLE_RATE, HOP_LENGTH) == (16000, 160)


@pytest.mark.parametrize("cfg", [None, dict(d_model=96, ssm_layers=2, ssm_state_dim=32, global_ssm_state_dim=16,
                                            attention_heads=2, attention_dim=24, vocab_size=50)])
def test_state_dict_contract(cfg):
    import velocity_asr as v
    m = v.VELOCITYASR(v.VelocityASRConfig(**(cfg or {})))
    spec = S.state_dict_spec(cfg)
    sd = m.state_dict()
    assert [k for k, _, _ in spec] == list(sd.keys())
    assert all(tuple(sd[k].shape) == s for k, s, _ in spec)
    if cfg is None:
        assert len(sd) == 208 and m.count_parameters() == 6_172_696


def test_checkpoint_roundtrip_and_strict_load(tmp_path):
    import velocity_asr as v
    m = v.VELOCITYASR()
    W = S.make_weights(None, seed=0)
    m.load_state_dict({k: torch.from_numpy(a) for k, a in W.items()}, strict=True)
    path = str(tmp_path / "ck" / "model.pt")
    m.save_pretrained(path)
    ck = torch.load(path, map_location="cpu", weights_only=True)
    assert set(ck) == {"config", "model_state_dict"} and len(ck["config"]) == 15
    m2 = v.from_pretrained(path)
    for k, a in m2.state_dict().items():
        assert torch.equal(a, m.state_dict()[k]), k
    # Trainer-style checkpoint: 'config' holds the training config -> default model config
    torch.save({"model_state_dict": m.state_dict(), "config": {"learning_rate": 1e-3}}, str(tmp_path / "t.pt"))
    assert v.VELOCITYASR.from_pretrained(str(tmp_path / "t.pt")).config == v.VelocityASRConfig()
    with pytest.raises(NotImplementedError):
        v.VELOCITYASR.from_pretrained("velocity-asr-v2")


def test_config_from_dict_filters_unknown_keys():
    import velocity_asr as v
    c = v.VelocityASRConfig.from_dict({"d_model": 96, "bogus": 1, "scan_mode": "sequential"})
    assert c.d_model == 96 and c.scan_mode == "sequential"


def test_seeded_init_is_the_reference_init():
    """torch.manual_seed(s); VELOCITYASR() draws the same numbers as the reference
    (same module order and initialisers, model.py:305-318)."""
    import velocity_asr as v
    torch.manual_seed(0)
    a = v.VELOCITYASR().state_dict()
    torch.manual_seed(0)
    b = v.VELOCITYASR().state_dict()
    assert all(torch.equal(a[k], b[k]) for k in a)
    # init statistics of the reference initialiser
    assert torch.all(a["local_ssm.layers.0.ssm.D"] == 1)
    assert torch.allclose(a["local_ssm.layers.0.ssm.A_log"], torch.log(torch.arange(1, 65.0)))
    assert torch.all(a["ctc_head.proj.2.bias"] == 0)


def test_vocabulary_and_text():
    import velocity_asr as v
    d = golden_json("decode.json")
    vocab = v.create_default_vocabulary(1000)
    assert len(vocab) == d["vocab_len"] and vocab[:80] == d["vocab_head"] and vocab[-3:] == d["vocab_tail"]
    assert v.create_default_vocabulary(10) == d["vocab_small"]
    dec = v.CTCDecoder(vocab)
    assert dec._tokens_to_text([30, 4, 3, 5, 9999]) == "Aa b<unk>"
    assert dec.text_to_tokens("ab") == [4, 5]


def test_wer_cer_match_reference():
    from velocity_asr.training import compute_cer, compute_wer
    for c in golden_json("decode.json")["wer"]:
        assert compute_wer(c["pred"], c["ref"]) == pytest.approx(c["wer"], abs=0)
        assert compute_cer(c["pred"], c["ref"]) == pytest.approx(c["cer"], abs=0)


def test_audio_helpers_and_wav_reader(tmp_path):
    import wave
    import velocity_asr as v
    assert v.audio_to_frames(160000) == 1002  # reference off-by-one kept (audio.py:280)
    assert v.frames_to_audio(10) == 1600
    x = torch.arange(10.0)
    assert v.pad_or_trim(x, 4).tolist() == [0, 1, 2, 3]
    assert v.pad_or_trim(x, 12)[-2:].tolist() == [0, 0]
    sig = (np.sin(np.arange(1600) / 7.0) * 12000).astype("<i2")
    p = str(tmp_path / "a.wav")
    with wave.open(p, "wb") as w:
        w.setnchannels(2)
        w.setsampwidth(2)
        w.setframerate(16000)
        w.writeframes(np.stack([sig, sig // 2], 1).tobytes())
    a = v.load_audio(p)
    assert a.shape == (1600,) and a.dtype == torch.float32
    np.testing.assert_allclose(a.numpy(), (sig.astype(np.float32) + (sig // 2).astype(np.float32)) / 2 / 32768, atol=1e-6)
    assert v.load_audio(p, mono=False).shape == (2, 1600)


@pytest.mark.skipif(torch.cuda.is_available(), reason="checks the no-GPU error path")
def test_no_cpu_fallback():
    import velocity_asr as v
    m = v.VELOCITYASR().eval()
    with pytest.raises(RuntimeError, match="HIP device"):
        m(torch.randn(1, 50, 80))
    with pytest.raises(RuntimeError, match="HIP device"):
        v.compute_mel_spectrogram(torch.randn(16000))
    with pytest.raises(RuntimeError, match="HIP device"):
        v.ctc_greedy_decode(torch.randn(1, 5, 10))


def test_mamba_mode_and_bad_mode():
    import velocity_asr as v
    v.SelectiveSSM(scan_mode="mamba")  # served by the HIP recurrence kernel
    with pytest.raises(ValueError):
        v.SelectiveSSM(scan_mode="bogus")


def test_tree_scan_kernel_mode_selection(monkeypatch):
    """scan_mode="parallel" runs kernel mode 2 (fused multiply-adds) unless VASR_SCAN_FMA=0
    selects mode 0 (the reference tree op for op); the other modes map to the recurrence."""
    from velocity_asr import ssm
    monkeypatch.delenv("VASR_SCAN_FMA", raising=False)
    assert ssm._tree_mode() == 2
    monkeypatch.setenv("VASR_SCAN_FMA", "0")
    assert ssm._tree_mode() == 0
    monkeypatch.setenv("VASR_SCAN_FMA", "1")
    assert ssm._tree_mode() == 2
    assert ssm._SCAN_MODE_ID == {"parallel": 0, "sequential": 1, "mamba": 1}


def test_scan_form_follows_the_library_rule():
    """ops._use_chunked takes the library's own one-launch rule (vasr_ssm_scan_split_selected,
    ABI 15) instead of a Python copy of scan.hip's condition; options change it."""
    from velocity_asr import _lib, ops
    lib = _lib.load()
    sel = lib.vasr_ssm_scan_split_selected
    assert sel(1, 501, 384, 64) == 1 and sel(1, 64, 384, 32) == 1  # one utterance: one launch
    assert sel(1, 513, 384, 64) == 0 and sel(2, 501, 384, 64) == 0 and sel(1, 501, 384, 128) == 0
    assert ops._use_chunked(1, 64, 384, 32, 2)  # short L, but the one-launch form
    assert not ops._use_chunked(32, 501, 384, 64, 2)
    with ops.option(_lib.OPT_SCAN_SPLIT, 1):  # three launches forced: short L stays streaming
        assert sel(1, 64, 384, 32) == 0 and not ops._use_chunked(1, 64, 384, 32, 2)
    with ops.option(_lib.OPT_SCAN_SPLIT, 2):
        assert sel(2, 1000, 384, 64) == 1
    with ops.option(_lib.OPT_SCAN_LANES, 4):
        assert sel(1, 501, 384, 64) == 0


def test_gemm_tile_query_pins_the_dispatch_rule():
    """vasr_gemm_tile (ABI 21) is the launchers' own rule (gemm_x3.hip select_kernel): pinned at the
    picker's edges (128 x 128 from 486 tiles, 128 x 64 from 358) and at the model's shapes, so a retune
    shows up here and in tests/test_gemm_tiles.py, whose cases assert the tile they run on."""
    from velocity_asr import _lib, ops
    lib = _lib.load()
    T128, T12864, T64, ROWS = 128128, 128064, 64064, 1
    K = 384  # not 128 / 192: off the rows engine
    for bf16 in (False, True):
        assert ops.gemm_tile(7680, 1024, K, bf16=bf16) == T12864  # 480 tiles of 128 x 128: below 486
        assert ops.gemm_tile(7681, 1024, K, bf16=bf16) == T128  # 488
        for M in (1, 300, 16032, 1 << 20):  # N <= 192: 64 x 64 at any M
            assert ops.gemm_tile(M, 192, K, bf16=bf16) == T64
        assert ops.gemm_tile(9217, 320, K, bf16=bf16) == T12864  # N % 128 != 0 and N <= 512; 365 tiles
        assert ops.gemm_tile(9089, 320, K, bf16=bf16) == T12864  # 360 tiles
        assert ops.gemm_tile(9088, 320, K, bf16=bf16) == T64  # 355 tiles of 128 x 64: below 358
        assert ops.gemm_tile(12417, 640, K, bf16=bf16) == T128
        assert ops.gemm_tile(1001, 448, 400, batch=32, epilogue=_lib.EPI_PAIR_POWER, bf16=bf16) == T12864
        for epi in (_lib.EPI_PAIR_POWER, _lib.EPI_PAIR_FUSION):  # pairs never take 64 x 64
            assert ops.gemm_tile(300, 448, K, epilogue=epi, bf16=bf16) == T12864
            assert ops.gemm_tile(1, 64, K, epilogue=epi, bf16=bf16) == T12864
        assert ops.gemm_tile(300, 448, K, bf16=bf16) == T64
        # the bf16 GEMM has no rows engine: the CTC head's argmax at K = 192 stays on the tiles
        for engine in (0, 1, 2):
            with ops.option(_lib.OPT_GEMM_ENGINE, engine):
                assert ops.gemm_tile(16032, 1000, 192, epilogue=_lib.EPI_ARGMAX, bf16=True) == T128
                assert ops.gemm_tile(16032, 896, 192, bf16=True) == T128
    # fp32 at K = 192: engine 0 (auto) / 1 (tiles) / 2 (rows)
    for engine, want in ((0, ROWS), (1, T128), (2, ROWS)):
        with ops.option(_lib.OPT_GEMM_ENGINE, engine):
            assert ops.gemm_tile(16032, 896, 192) == want
    # auto keeps the tiles for N < 512, M < 4096, the argmax / residual epilogues, batches, other K
    assert ops.gemm_tile(16032, 384, 192) == T12864 and ops.gemm_tile(4095, 896, 192) == T12864
    assert ops.gemm_tile(16032, 1000, 192, epilogue=_lib.EPI_ARGMAX) == T128
    assert ops.gemm_tile(16032, 896, 192, epilogue=_lib.EPI_RESIDUAL) == T128
    assert ops.gemm_tile(8016, 896, 192, batch=2) == T128 and ops.gemm_tile(16032, 896, 164) == ROWS
    assert ops.gemm_tile(16032, 896, 224) == T128 and ops.gemm_tile(16032, 896, 128) == T128
    assert ops.gemm_tile(16032, 896, 160) == T128  # Kp = 160
    assert ops.gemm_tile(1 << 20, 896, 192) == T128  # C past the rows engine's 31-bit offsets
    with ops.option(_lib.OPT_GEMM_ENGINE, 2):  # forced: K = 128 too, never pairs or batches
        assert ops.gemm_tile(33, 64, 128) == ROWS and ops.gemm_tile(33, 64, 100) == ROWS
        assert ops.gemm_tile(33, 64, 96) == T64 and ops.gemm_tile(33, 64, 128, batch=2) == T64
        assert ops.gemm_tile(300, 448, 192, epilogue=_lib.EPI_PAIR_FUSION) == T12864
    # bad arguments: refused as the launchers refuse them, nothing launched
    for bad in ((0, 64, 32, 1, 0, 0), (4, 0, 32, 1, 0, 0), (4, 64, 34, 1, 0, 0), (4, 64, 32, 0, 0, 0),
                (4, 64, 32, 1, 8, 0), (4, 64, 32, 1, -1, 0), (4, 64, 32, 1, 0, 2), (4, 96, 32, 1, _lib.EPI_PAIR_POWER, 0)):
        assert lib.vasr_gemm_tile(*bad) == -1, bad
    assert b"vasr_gemm_tile" in lib.vasr_last_error()
    with pytest.raises(RuntimeError, match="vasr_gemm_tile"):
        ops.gemm_tile(4, 64, 34)


def _isa_scan():
    sys.path.insert(0, os.path.join(REPO, "tools", "isa"))
    import isa_scan
    try:
        isa_scan.objdump()
    except FileNotFoundError:
        pytest.skip("llvm-objdump absent")
    return isa_scan


@pytest.fixture(scope="module")
def shipped_kernels():
    from velocity_asr import _lib
    return _isa_scan().library_kernels(_lib.LIB_PATH)


def test_no_kernel_has_a_packed_fp32_op_with_swapped_source(shipped_kernels):
    """Library-wide guard: no kernel in the shipped gfx950 code has a packed-fp32
    VOP3P instruction (v_pk_{add,mul,fma}_f32) reading a source with its dwords swapped (op_sel 1,
    op_sel_hi 0).  That form -- 12 instructions of stft.hip's SLP-vectorised build, the re/im swaps
    of its complex products -- returned wrong |STFT|^2 values for a half-wave beside MFMA kernels of
    another stream: 18/400 launches, 0/400 with only those 12 rewritten as scalar pairs, 18-19/400
    with every other packed form rewritten instead (profiles/r05e/, r05f/)."""
    isa = _isa_scan()
    assert len(shipped_kernels) > 200
    hits = {k: isa.pk_swapped(v) for k, v in shipped_kernels.items()}
    hits = {k: h for k, h in hits.items() if h}
    assert not hits, [(k[:80], h[0][1]) for k, h in list(hits.items())[:4]]


def test_stft_kernel_has_no_packed_fp32_valu(shipped_kernels):
    """stft.hip is built without SLP vectorisation (velocity-asr_amd/Makefile), so its kernel holds
    no packed-fp32 VALU at all."""
    body = [v for k, v in shipped_kernels.items() if "stft_power_400_kernel" in k]
    assert body and len(body[0]) > 100, "stft_power_400_kernel not found in the library"
    packed = [ln for ln in body[0] if ln.startswith(("v_pk_fma_f32", "v_pk_mul_f32", "v_pk_add_f32"))]
    assert not packed, packed[:4]


def test_isa_guard_detects_the_slp_stft_sequence(tmp_path):
    """Positive control of the guard: stft.hip compiled WITH SLP vectorisation (the build that
    failed) has the form (12 instructions); the shipped flags (-fno-slp-vectorize) do not."""
    isa = _isa_scan()
    hipcc = "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc absent")
    pkg = os.path.join(REPO, "velocity-asr_amd")
    found = {}
    for tag, extra in (("slp", []), ("noslp", ["-fno-slp-vectorize"])):
        asm = tmp_path / f"{tag}.s"
        subprocess.run([hipcc, "-O3", "-std=c++17", "--offload-arch=gfx950", "-I../include", "-munsafe-fp-atomics",
                        "--cuda-device-only", "-S", "csrc/stft.hip", "-o", str(asm)] + extra,
                       cwd=pkg, check=True, capture_output=True)
        ins = [ln.strip() for ln in open(asm) if ln.startswith("\t") and not ln.strip().startswith((".", ";"))]
        found[tag] = isa.pk_swapped(ins)
    assert len(found["slp"]) >= 10, found["slp"]
    assert found["noslp"] == []


_TEARDOWN_SCRIPT = r"""
import sys
sys.path[:0] = [{pkg!r}]
import torch
from velocity_asr import ops
seen = []
sys.unraisablehook = lambda u: seen.append(repr(u.exc_value))
t = torch.zeros(8, 8, device={dev!r}, dtype={dtype})
if {real!r}:  # the split planes of a weight, as the model builds them
    ops.split_weights(t); ops.split_weights16(t)
    torch.cuda.synchronize()
else:  # an fp32 copy of a bf16 parameter: the same cache registration, no kernel
    ops.f32(t)
# what interpreter teardown did in the driver's runs (profiles/r05j/step_course.txt): the module's
# _-prefixed globals are None (_PyModule_ClearDict's first pass) while a cache entry and its
# weakref are still alive, and then the weight dies
alive = {{k: v for k, v in vars(ops).items() if k.startswith("_") and not k.startswith("__")}}
for k in alive:
    setattr(ops, k, None)
del t
import gc; gc.collect()
print("ok" if not seen else seen)
"""


def _teardown_stdout(dev, real, dtype):
    code = _TEARDOWN_SCRIPT.format(pkg=os.path.join(REPO, "velocity-asr_amd"), dev=dev, real=real, dtype=dtype)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    return r.stdout.strip()


def test_weight_caches_exit_quietly():
    """the weight caches' weakref callbacks looked their dict up as a module
    global, which is None once interpreter teardown has cleared the module, and printed
    AttributeError tracebacks at exit.  They now hold the dict itself (ops._dropper)."""
    assert _teardown_stdout("cpu", False, "torch.bfloat16") == "ok"


@pytest.mark.gpu
def test_split_planes_exit_quietly():
    assert _teardown_stdout("cuda", True, "torch.float32") == "ok"
