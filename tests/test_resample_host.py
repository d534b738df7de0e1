"""Host side of the device resampler: the exported geometry and tap table are the ones
vasr_resample_f32 applies, argument errors are refused before any device call, and load_audio
without a device is what it was.  No GPU needed."""

import ctypes

import numpy as np
import pytest
import torch

import resample_cases as rc


def _lib():
    from velocity_asr import _lib
    return _lib


def _plan(lib, orig_sr, new_sr):
    g = [ctypes.c_int() for _ in range(4)]
    rc_ = lib.vasr_resample_plan(orig_sr, new_sr, *[ctypes.addressof(v) for v in g])
    return rc_, tuple(v.value for v in g)


def _taps(lib, orig_sr, new_sr):
    _, nw, _, klen = rc.geometry(orig_sr, new_sr)
    t = np.empty((nw, klen), np.float32)
    assert lib.vasr_resample_taps_f32(orig_sr, new_sr, t.ctypes.data, t.size) == 0
    return t


def test_abi_version_stays_and_symbols_bind():
    L = _lib()
    lib = L.lib()
    assert lib.vasr_version() == L.ABI_VERSION == 21
    for name in ("vasr_resample_plan", "vasr_resample_taps_f32", "vasr_resample_mix_f32", "vasr_resample_tile_outputs"):
        assert name in L._SIGNATURES and name in L.header_functions()
        assert getattr(lib, name).argtypes is not None


@pytest.mark.parametrize("orig_sr,new_sr", [(r, rc.TARGET) for r in rc.RATES] + [(16000, 8000)])
def test_plan_is_the_restatements_geometry(orig_sr, new_sr):
    code, got = _plan(_lib().lib(), orig_sr, new_sr)
    assert code == 0
    assert got == rc.geometry(orig_sr, new_sr)


def test_plan_and_taps_refuse_a_huge_table():
    lib = _lib().lib()
    code, _ = _plan(lib, 44101, 16000)
    assert code == -1
    assert b"tap kernel" in lib.vasr_last_error() and b"44101 -> 16000" in lib.vasr_last_error()
    buf = np.empty(16, np.float32)
    assert lib.vasr_resample_taps_f32(44101, 16000, buf.ctypes.data, buf.size) == -1
    assert b"tap kernel" in lib.vasr_last_error()
    assert _plan(lib, 0, 16000)[0] == -1 and _plan(lib, 16000, -1)[0] == -1
    # a table that does not fit the caller's buffer is refused, not truncated
    assert lib.vasr_resample_taps_f32(48000, 16000, buf.ctypes.data, 40) == -1


@pytest.mark.parametrize("orig_sr,new_sr", rc.PAIRS)
def test_exported_table_is_the_one_the_host_resampler_applies(orig_sr, new_sr):
    """vasr_resample_f32 on 300 samples == the ascending float64 chain over the exported table,
    bit for bit; the table itself is the restatement's to a float32 rounding."""
    from velocity_asr.audio import resample
    lib = _lib().lib()
    orig, nw, width, klen = rc.geometry(orig_sr, new_sr)
    taps = _taps(lib, orig_sr, new_sr)
    # float32 values of magnitude <= 1 built by two float64 libms: at most an ulp (1.2e-7) apart
    np.testing.assert_allclose(taps, rc.taps_ref(orig_sr, new_sr), rtol=0, atol=1.2e-7)
    x = rc.signal(300, seed=orig_sr + new_sr)
    want = rc.chain(x, taps, orig, nw, width)
    got = resample(torch.from_numpy(x), orig_sr, new_sr).numpy()
    assert got.shape == want.shape == (rc.out_length(300, orig_sr, new_sr),)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))


def test_tile_outputs_are_whole_frames():
    lib = _lib().lib()
    for orig_sr, new_sr in rc.PAIRS:
        orig, nw, _, _ = rc.geometry(orig_sr, new_sr)
        T = lib.vasr_resample_tile_outputs(orig, nw)
        assert T > 0 and T % nw == 0, (orig_sr, new_sr, T)
    assert lib.vasr_resample_tile_outputs(1, 1) > 0
    assert lib.vasr_resample_tile_outputs(0, 1) == 0
    # an input span no workgroup can hold is refused (and the callers resample on the host)
    assert lib.vasr_resample_tile_outputs(16000, 44101) == 0


def test_mix_refuses_bad_arguments_before_any_device_call():
    lib = _lib().lib()
    x = np.zeros(64, np.float32)
    y = np.zeros(64, np.float32)
    t = np.zeros(64, np.float32)
    px, py, pt = x.ctypes.data, y.ctypes.data, t.ctypes.data

    def call(x=px, ld_clip=30, ld_chan=30, B=1, C=1, S_in=30, taps=pt, y=py, ld_y=10, S_out=10):
        # 48 -> 16 kHz: orig 3, nw 1, width 19; 30 samples give 10 outputs
        return lib.vasr_resample_mix_f32(x, ld_clip, ld_chan, B, C, S_in, None, taps, 3, 1, 19, y, ld_y, S_out, None)

    assert call(x=None) == -1 and b"null" in lib.vasr_last_error()
    assert call(y=None) == -1
    assert call(taps=None) == -1
    assert call(C=0) == -1 and b"channels" in lib.vasr_last_error()
    assert call(C=9) == -1 and b"channels" in lib.vasr_last_error()
    assert call(ld_y=9) == -1 and b"ld_y" in lib.vasr_last_error()
    assert call(S_out=9, ld_y=9) == -1 and b"S_out" in lib.vasr_last_error()
    assert lib.vasr_resample_mix_f32(None, 0, 0, 1, 1, 1, None, None, 1, 1, 0, None, 0, 0, None) == -1
    # a geometry whose span does not fit in LDS says so
    assert lib.vasr_resample_mix_f32(px, 30, 30, 1, 1, 30, None, pt, 16000, 44101, 7, py, 83, 83, None) == -1
    assert b"LDS" in lib.vasr_last_error()


def test_load_audio_without_device_is_unchanged(tmp_path):
    """load_audio(path) == read_audio + the steps it always took (mean over channels, host
    resampler, squeeze), bit for bit, on a 44.1 kHz stereo FLAC."""
    try:
        import torchaudio  # noqa: F401
        pytest.skip("load_audio goes through torchaudio when it is installed")
    except ImportError:
        pass
    import flac_writer as fw
    from velocity_asr import audio
    rng = np.random.default_rng(5)
    pcm = [rng.integers(-20000, 20000, 3000) for _ in range(2)]
    p = str(tmp_path / "s.flac")
    with open(p, "wb") as f:
        f.write(fw.encode(pcm, 44100, 16, block=1152))
    w, sr = audio.read_audio(p)
    assert sr == 44100 and tuple(w.shape) == (2, 3000) and w.dtype == torch.float32 and w.device.type == "cpu"
    np.testing.assert_array_equal(w.numpy(), np.stack(pcm).astype(np.float32) / 32768.0)
    want = audio.resample(w.mean(dim=0, keepdim=True), 44100, 16000).squeeze(0)
    got = audio.load_audio(p)
    assert got.device.type == "cpu" and torch.equal(got, want)
    assert np.array_equal(got.numpy().view(np.uint32), want.numpy().view(np.uint32))
    both = audio.load_audio(p, mono=False)
    assert torch.equal(both, audio.resample(w, 44100, 16000))
    with pytest.raises(ImportError):
        audio.read_audio(str(tmp_path / "s.mp3"))
