"""GPU tests of the device resampler (vasr_resample_mix_f32, ops.resample_mix, audio.resample on a
HIP tensor, audio.resample_on_device, load_audio(device=), transcribe_files).

Every comparison is torch.equal against the host path (audio.resample on a host tensor, after the
specified downmix where there are channels): the kernel walks the host resampler's float32 taps in
its order with one float64 chain per output, and a float32 x float32 product is exact in float64,
so there is no tolerance to choose.  Cases: resample_cases.py."""

import functools

import numpy as np
import pytest
import torch

import resample_cases as rc
from velocity_asr import synthetic as S

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module")
def A():
    from velocity_asr import _lib, audio
    _lib.load()
    return audio


@functools.lru_cache(maxsize=None)
def _clip(n, seed, channels=None):
    return rc.signal(n, seed, channels)


@functools.lru_cache(maxsize=None)
def _host(n, seed, channels, orig_sr, new_sr):
    """The host path on clip (n, seed): the specified downmix, then audio.resample on the host."""
    from velocity_asr import audio
    x = _clip(n, seed, channels)
    if channels is not None:
        x = rc.downmix(x)
    return audio.resample(torch.from_numpy(x), orig_sr, new_sr)


def _tile(orig_sr, new_sr):
    from velocity_asr import _lib
    orig, nw, _, _ = rc.geometry(orig_sr, new_sr)
    T = int(_lib.lib().vasr_resample_tile_outputs(orig, nw))
    assert T > 0
    return T


def _edge_lengths(orig_sr, new_sr):
    """Input lengths with T-1, T, T+1 and 2T+1 outputs, and the longest one still short of T."""
    T = _tile(orig_sr, new_sr)
    ns = rc.lengths_for_outputs([T - 1, T, T + 1, 2 * T + 1], orig_sr, new_sr)
    below = rc.lengths_for_outputs([T], orig_sr, new_sr)[0] - 1
    return sorted(set(ns + ([below] if below >= 1 else [])))


def _table(A, orig_sr, new_sr):
    return A._resample_table(orig_sr, new_sr, torch.device(DEV, torch.cuda.current_device()))


@pytest.mark.parametrize("orig_sr,new_sr", rc.PAIRS)
def test_single_clips_equal_the_host_resampler(A, orig_sr, new_sr):
    T = _tile(orig_sr, new_sr)
    edges = _edge_lengths(orig_sr, new_sr)
    outs = [rc.out_length(n, orig_sr, new_sr) for n in edges]
    assert min(outs) < T and T in outs and max(outs) > 2 * T  # both sides of a tile edge, and past a second one
    for n in rc.LENGTHS + edges:
        want = _host(n, n, None, orig_sr, new_sr)
        got = A.resample(torch.from_numpy(_clip(n, n)).to(DEV), orig_sr, new_sr)
        assert got.device.type == "cuda" and got.dtype == torch.float32
        assert got.shape == want.shape == (rc.out_length(n, orig_sr, new_sr),), n
        assert torch.equal(got.cpu(), want), (orig_sr, new_sr, n)


def test_equal_rates_copy(A):
    x = torch.from_numpy(_clip(3001, 1))
    got = A.resample(x.to(DEV), 16000, 16000)
    assert torch.equal(got.cpu(), x) and torch.equal(A.resample(x, 16000, 16000), x)
    # with channels: the downmix alone, and zeros past each clip
    xc = torch.from_numpy(_clip(1500, 2, 3))
    y, outs = A.resample_on_device(xc[None].to(DEV).repeat(2, 1, 1), 16000, 16000, lengths=[1500, 40])
    assert outs == [1500, 40] and tuple(y.shape) == (2, 1500)
    m = torch.from_numpy(rc.downmix(xc.numpy()))
    assert torch.equal(y[0].cpu(), m) and torch.equal(y[1, :40].cpu(), m[:40]) and not y[1, 40:].any()


@pytest.mark.parametrize("C", [1, 2, 3, 4])
@pytest.mark.parametrize("orig_sr", [44100, 48000, 8000])
def test_ragged_batch_rows_are_the_clips_alone(A, orig_sr, C):
    T = _tile(orig_sr, 16000)
    S_in = rc.lengths_for_outputs([T + 37], orig_sr, 16000)[0]  # more than one workgroup per clip
    samples = [S_in, 1, 777, S_in - 1, 2]
    x = torch.zeros((5, C, S_in))
    for b, n in enumerate(samples):
        x[b, :, :n] = torch.from_numpy(_clip(n, 10 + b, C))
    y, outs = A.resample_on_device(x.to(DEV), orig_sr, 16000, lengths=samples)
    S_out = rc.out_length(S_in, orig_sr, 16000)
    assert tuple(y.shape) == (5, S_out) and outs == [rc.out_length(n, orig_sr, 16000) for n in samples]
    y = y.cpu()
    for b, n in enumerate(samples):
        want = _host(n, 10 + b, C, orig_sr, 16000)
        assert torch.equal(y[b, :outs[b]], want), (b, n)
        assert not y[b, outs[b]:].any(), (b, n)
    if C == 1:  # (B, S) input is the one-channel batch
        y2, _ = A.resample_on_device(x[:, 0].to(DEV), orig_sr, 16000, lengths=samples)
        assert torch.equal(y2.cpu(), y)
    # load_audio's fused downmix relies on this: for C <= 4 the specified mean is torch's
    assert torch.equal(torch.from_numpy(rc.downmix(x[0].numpy())), x[0].mean(dim=0))


def _raw_launch(A, x, ld_clip, ld_chan, B, C, S_in, samples, orig_sr, new_sr, y, ld_y, S_out):
    from velocity_asr import _lib
    tb = _table(A, orig_sr, new_sr)
    _lib.check(_lib.lib().vasr_resample_mix_f32(x.data_ptr(), ld_clip, ld_chan, B, C, S_in, _lib.ptr(samples),
                                                _lib.ptr(tb.taps), tb.orig, tb.nw, tb.width, y.data_ptr(), ld_y, S_out,
                                                _lib.stream_of(x)), "vasr_resample_mix_f32")


@pytest.mark.parametrize("orig_sr", [44100, 48000, 8000])
def test_poisoned_output_and_strided_input(A, orig_sr):
    """y pre-filled with NaN and five spare columns per row: every column below S_out is written
    (values, then zeros), the spare ones are untouched; x with clip and channel strides larger than
    the packed sizes, NaN in the gaps and after each clip's own samples."""
    B, C, S_in = 3, 2, 1200
    samples = [1200, 5, 731]
    ld_chan, ld_clip = S_in + 7, 2 * (S_in + 7) + 11
    x = torch.full((B * ld_clip,), float("nan"))
    for b, n in enumerate(samples):
        for c in range(C):
            x[b * ld_clip + c * ld_chan: b * ld_clip + c * ld_chan + n] = torch.from_numpy(_clip(n, 20 + b, C)[c])
    S_out = rc.out_length(S_in, orig_sr, 16000)
    y = torch.full((B, S_out + 5), float("nan"), device=DEV)
    _raw_launch(A, x.to(DEV), ld_clip, ld_chan, B, C, S_in, torch.tensor(samples, dtype=torch.int32).to(DEV), orig_sr,
                16000, y, S_out + 5, S_out)
    y = y.cpu()
    assert not torch.isnan(y[:, :S_out]).any() and torch.isnan(y[:, S_out:]).all()
    for b, n in enumerate(samples):
        m = rc.out_length(n, orig_sr, 16000)
        assert torch.equal(y[b, :m], _host(n, 20 + b, C, orig_sr, 16000)) and not y[b, m:S_out].any()


def test_side_stream(A):
    x = torch.from_numpy(_clip(3001, 3001)).to(DEV)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        got = A.resample(x, 44100, 16000)
    s.synchronize()
    assert torch.equal(got.cpu(), _host(3001, 3001, None, 44100, 16000))


def test_graph_capture_replays_with_new_input(A):
    from velocity_asr import ops
    tb = _table(A, 44100, 16000)
    a, b = (torch.from_numpy(_clip(3001, s))[None] for s in (3001, 4))
    buf = a.to(DEV)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):  # warm-up outside the capture
        ops.resample_mix(buf, tb.taps, tb.orig, tb.nw, tb.width)
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = ops.resample_mix(buf, tb.taps, tb.orig, tb.nw, tb.width)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out.cpu()[0], _host(3001, 3001, None, 44100, 16000))
    buf.copy_(b.to(DEV))
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out.cpu()[0], A.resample(b[0], 44100, 16000))


def _write_flac(path, pcm, sample_rate):
    import flac_writer as fw
    with open(path, "wb") as f:
        f.write(fw.encode(list(pcm), sample_rate, 16, block=1152))


def test_load_audio_on_the_device(A, tmp_path):
    rng = np.random.default_rng(8)
    stereo = str(tmp_path / "stereo.flac")
    _write_flac(stereo, rng.integers(-20000, 20000, (2, 5000)), 44100)
    mono = str(tmp_path / "mono.wav")
    A.write_wav(mono, _clip(4000, 48), 48000)
    six = str(tmp_path / "six.flac")
    _write_flac(six, rng.integers(-20000, 20000, (6, 3000)), 22050)
    same = str(tmp_path / "same.wav")
    A.write_wav(same, _clip(2000, 16, 2), 16000)
    for p in (stereo, mono, six, same):
        want = A.load_audio(p)
        got = A.load_audio(p, device=DEV)
        assert got.device.type == "cuda" and got.dim() == 1
        assert torch.equal(got.cpu(), want), p
    both = A.load_audio(stereo, mono=False, device=DEV)
    assert torch.equal(both.cpu(), A.load_audio(stereo, mono=False))
    # the six-channel file took the host downmix: one channel reached the kernel
    w, sr = A.read_audio(six)
    assert w.size(0) == 6 > A._FUSED_DOWNMIX_CHANNELS
    assert torch.equal(A.load_audio(six), A.resample(w.mean(dim=0, keepdim=True), sr, 16000).squeeze(0))


@pytest.fixture(scope="module")
def small_model():
    import velocity_asr as v
    cfg = dict(mel_bins=80, d_model=96, ssm_layers=2, ssm_state_dim=32, global_ssm_state_dim=16,
               attention_heads=2, attention_dim=24, vocab_size=50)
    W = S.make_weights(cfg, seed=5)
    m = v.VELOCITYASR(v.VelocityASRConfig(**cfg))
    m.load_state_dict({k: torch.from_numpy(w) for k, w in W.items()}, strict=True)
    return m.to(DEV).eval(), v.CTCDecoder(v.create_default_vocabulary(50))


@pytest.fixture(scope="module")
def five_files(tmp_path_factory):
    """44.1 kHz stereo 1.3 s, 48 kHz mono 0.9 s, 8 kHz mono 1.1 s, 16 kHz mono 1.0 s and a 44.1 kHz
    clip too short to frame (400 samples -> 146 at 16 kHz <= 200)."""
    from velocity_asr.audio import write_wav
    d = tmp_path_factory.mktemp("rs")
    spec = [(44100, 2, 1.3), (48000, 1, 0.9), (8000, 1, 1.1), (16000, 1, 1.0), (44100, 1, 400 / 44100)]
    paths = []
    for i, (sr, ch, sec) in enumerate(spec):
        n = int(round(sr * sec))
        a16 = S.make_audio(ch, max(n, 400), seed=60 + i)[:, :n]
        p = d / f"f{i}_{sr}.wav"
        write_wav(str(p), torch.from_numpy(np.ascontiguousarray(a16)), sr)
        paths.append(p)
    return paths


@pytest.mark.parametrize("kw", [dict(), dict(timestamps=True, beam_width=4)], ids=["greedy", "beam4_timestamps"])
def test_transcribe_files_same_dicts_either_way(small_model, five_files, monkeypatch, kw):
    from velocity_asr import transcription as T
    model, dec = small_model
    calls = []
    real = T.resample_on_device
    monkeypatch.setattr(T, "resample_on_device", lambda *a, **k: calls.append(a[1]) or real(*a, **k))
    monkeypatch.setenv("VASR_DEVICE_RESAMPLE", "0")
    host = T.transcribe_files(model, five_files, dec, DEV, batch_size=4, **kw)
    assert calls == []
    monkeypatch.delenv("VASR_DEVICE_RESAMPLE")
    dev = T.transcribe_files(model, five_files, dec, DEV, batch_size=4, **kw)
    assert sorted(calls) == [8000, 44100, 48000]  # one launch per (rate, channels) group; 16 kHz untouched
    assert dev == host
    assert [("error" in r) for r in host] == [False, False, False, False, True]
    assert "reflect padding of 200 needs more than 200 samples, got 146" in host[4]["error"]
    assert all(r["transcription"] == r["transcription"].strip() and r["duration"] > 0.8 for r in host[:4])
    if kw.get("timestamps"):
        assert all("words" in r for r in host[:4])
