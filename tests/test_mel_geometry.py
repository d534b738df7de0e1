"""The log-mel front end off its default geometry, on an MI355X (pytest -m gpu).

The default geometry (16 kHz, n_fft 400, hop 160, 80 bins, normalised) is covered by
test_gpu_parity.py.  Here: every row of mel_geometry_cases.CASES against the reference's own
output (tests/golden/mel_geometry.npz), the windowed-DFT GEMM at other K and N against fp64,
ragged batches whose clips end on chunk (16-frame) and FFT-group (6-frame) boundaries against
the oracle run on each clip alone, the global-CSR branch of the chunked pass against fp64, and
what each kernel writes and leaves alone in NaN-filled buffers.

Tolerance: the mel tolerance of test_gpu_parity.py (atol 2e-4, rtol 1e-4); the power bound is
test_stft_power_fft_vs_fp64's.
"""

import numpy as np
import pytest
import torch

import mel_geometry_cases as G
from conftest import golden, record_error
from oracle import velocity_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda"
MEL_TOL = dict(atol=2e-4, rtol=1e-4)


@pytest.fixture(scope="module")
def va():
    import velocity_asr
    from velocity_asr import _lib
    _lib.require_device()
    _lib.load()
    return velocity_asr


@pytest.fixture(scope="module")
def gold():
    g = golden("mel_geometry.npz")
    return {k: g[k] for k in g.files}


def t(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def bits(x):
    """float32 tensor -> its bit patterns (equality that also holds for nan)."""
    return x.contiguous().view(torch.int32)


def assert_mel(got, want):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    record_error(got, want, MEL_TOL)
    np.testing.assert_allclose(got, want, **MEL_TOL)


# ----------------------------------------------------------------------------- a. every table row
@pytest.mark.parametrize("normalize", [True, False], ids=["norm", "raw"])
@pytest.mark.parametrize("case", G.CASES, ids=lambda c: G.name(*c))
def test_geometry_matches_reference(va, gold, case, normalize):
    """compute_mel_spectrogram, MelSpectrogramTransform on the device and the zero-framed layout
    (frame_pad = 1) against the reference's output at this geometry.

    Empty filters (fb.sum(1) == 0, from the filterbank): the row is the constant log(1e-10), so
    the normalised output is exactly 0 (fp64 statistics: exact mean of a constant row); the
    reference's fp32 mean is inexact there and its output noise, so those bins are left out of
    the normalised comparison.  One frame normalises to nan, like the reference."""
    from velocity_asr import audio as A, ops
    sr, n_fft, hop, n_mels, S_ = case
    name = G.name(*case)
    F_ = G.frames(S_, n_fft, hop)
    want = gold[f"{name}__{'norm' if normalize else 'raw'}"]
    fb = gold[f"fb_{n_fft}_{n_mels}_{sr}"]
    empty = fb.sum(1) == 0
    assert int(empty.sum()) == {"sr16000_fft400_hop160_mel128_S2560": 4, "sr16000_fft256_hop64_mel80_S1100": 2}.get(name, 0)
    x = t(G.audio(name, S_))
    kw = dict(sample_rate=sr, n_fft=n_fft, hop_length=hop, n_mels=n_mels, normalize=normalize)

    mel = va.compute_mel_spectrogram(x, **kw)
    assert mel.device.type == "cuda" and mel.dtype == torch.float32
    assert tuple(mel.shape) == want.shape == (2, F_, n_mels)
    got = mel.cpu().numpy()
    if F_ == 1 and normalize:
        assert np.isnan(want).all() and np.isnan(got).all()
    else:
        assert np.isfinite(got).all()
        keep = ~empty if normalize else np.ones(n_mels, bool)
        assert_mel(got[..., keep], want[..., keep])
        if normalize:
            assert not got[..., empty].any()

    tr = va.MelSpectrogramTransform(sr, n_fft, hop, n_mels, normalize).to(DEV)
    assert tr.window.device.type == "cuda" and tr.mel_filters.device.type == "cuda"
    np.testing.assert_array_equal(tr.mel_filters.cpu().numpy(), fb)
    assert torch.equal(bits(tr(x)), bits(mel))

    view = A.mel_on_device(x, sr, n_fft, hop, n_mels, normalize, frame_pad=1)
    assert tuple(view.shape) == (2, F_, n_mels)
    assert torch.equal(bits(view), bits(mel))
    buf = ops.zero_framed(view, 1)
    assert buf is not None and tuple(buf.shape) == (2, F_ + 2, n_mels)
    assert buf.data_ptr() + 4 * n_mels == view.data_ptr()
    assert torch.count_nonzero(bits(buf[:, 0])).item() == 0
    assert torch.count_nonzero(bits(buf[:, -1])).item() == 0


# ----------------------------------------------------------------------------- b. power at other sizes
GEMM_CASES = [c for c in G.CASES if (c[1], c[2]) != (400, 160)]


@pytest.mark.parametrize("case", GEMM_CASES, ids=lambda c: G.name(*c))
def test_stft_power_gemm_vs_fp64(va, case):
    """reflect_pad + the windowed-DFT GEMM with the |X|^2 epilogue (K = n_fft, lda = hop,
    N = 64 ceil(bins / 32)) vs torch.stft in fp64, with test_stft_power_fft_vs_fp64's bound:
    |P - P64| <= 1e-5 * max(P64) per frame + 1e-6 relative."""
    from velocity_asr import _lib, audio as A, ops
    sr, n_fft, hop, n_mels, S_ = case
    name = G.name(*case)
    x = G.audio(name, S_)
    B, pad, F_ = x.shape[0], n_fft // 2, G.frames(S_, n_fft, hop)
    tb = A._tables(torch.device(DEV, torch.cuda.current_device()), n_fft, n_mels, sr)
    assert tb.n_bins == n_fft // 2 + 1 and tuple(tb.dft.shape) == (64 * ((tb.n_bins + 31) // 32), n_fft)
    ld = (S_ + 2 * pad + 3) // 4 * 4
    xp = ops.reflect_pad(t(x), pad, ld)
    power = torch.full((B, F_, tb.n_bins), float("nan"), device=DEV)
    ops.gemm_batched(xp, hop, ld, F_, B, n_fft, tb.dft, None, power, tb.n_bins, F_ * tb.n_bins,
                     epilogue=_lib.EPI_PAIR_POWER, n_out=tb.n_bins)
    p = power.cpu().double()
    xd = torch.from_numpy(x).double()
    xpd = torch.nn.functional.pad(xd.unsqueeze(1), (pad, pad), mode="reflect").squeeze(1)
    np.testing.assert_array_equal(xp[:, :S_ + 2 * pad].cpu().numpy(), xpd.float().numpy())
    ref = torch.stft(xpd, n_fft, hop, window=torch.hann_window(n_fft).double(), center=False,
                     return_complex=True).abs().pow(2).transpose(1, 2)
    assert p.shape == ref.shape == (B, F_, n_fft // 2 + 1)
    frame_max = ref.amax(dim=2, keepdim=True)
    err = (p - ref).abs() - 1e-6 * ref.abs()
    print(name, "worst |P - P64| / frame max:", float((err / frame_max.clamp_min(1e-30)).max()))
    assert (err <= 1e-5 * frame_max + 1e-12).all(), float((err / frame_max.clamp_min(1e-30)).max())


# ----------------------------------------------------------------------------- c. ragged edges
RAGGED_LENGTHS = [2560, 201, 5279, 800, 4960, 2400]  # own frames 17, 2, 33, 6, 32, 16


@pytest.fixture(scope="module")
def ragged():
    """One zero-padded batch whose clips end on and next to the 16-frame chunk and the 6-frame
    FFT-group boundaries, and the oracle's log-mel of each clip alone."""
    S_ = max(RAGGED_LENGTHS)
    rng = np.random.default_rng(20)
    batch = np.zeros((len(RAGGED_LENGTHS), S_), np.float32)
    alone = []
    for i, n in enumerate(RAGGED_LENGTHS):
        batch[i, :n] = (0.1 * rng.standard_normal(n)).astype(np.float32)
        alone.append(R.compute_mel_spectrogram(batch[i, :n]))
    assert [a.shape[0] for a in alone] == [17, 2, 33, 6, 32, 16]
    return batch, alone


def test_ragged_edges_vs_oracle(va, ragged):
    """Each clip's own frames match the oracle run on the clip alone and its later frames are
    exactly 0; with the padding samples set to nan instead of 0 the result is bitwise the same
    (reflection is resolved inside the clip; statistics and normalisation select, not multiply)."""
    batch, alone = ragged
    lens = torch.tensor(RAGGED_LENGTHS, dtype=torch.int32)
    mel = va.compute_mel_spectrogram(t(batch), lengths=lens)
    assert tuple(mel.shape) == (len(RAGGED_LENGTHS), batch.shape[1] // 160 + 1, 80)
    got = mel.cpu().numpy()
    for i, want in enumerate(alone):
        f = want.shape[0]
        assert_mel(got[i, :f], want)
        assert not got[i, f:].any(), (i, f)
    poisoned = batch.copy()
    for i, n in enumerate(RAGGED_LENGTHS):
        poisoned[i, n:] = np.nan
    mel_nan = va.compute_mel_spectrogram(t(poisoned), lengths=lens)
    assert torch.equal(bits(mel_nan), bits(mel))


# ----------------------------------------------------------------------------- d. the global-CSR branch
@pytest.mark.parametrize("normalize", [True, False], ids=["norm", "raw"])
def test_mel_log_norm_global_csr_vs_fp64(va, normalize):
    """A dense 8 x 201 filterbank has 1608 non-zeros, more than the 1024 the chunked pass keeps
    in LDS, so it reads the CSR from global memory.  Against fp64 log(fb @ P + 1e-10) and its
    per-bin normalisation over each utterance's own frames; frames past them are 0.

    Tolerance: a float32 sum of 201 non-negative products is within 201 * 2^-24 = 1.2e-5
    relative of the exact one, so its log is within 1.2e-5 absolute (+ an ulp of log, < 1e-6);
    the frames' power spans e^+-3, so the per-bin std is > 1 and the normalised error no
    larger: inside the mel tolerance."""
    from velocity_asr import ops
    rng = np.random.default_rng(33)
    B, F_, n_mels, n_bins = 2, 17, 8, 201
    fb = rng.random((n_mels, n_bins)).astype(np.float32) + np.float32(0.01)
    P = (rng.random((B, F_, n_bins)) * np.exp(rng.uniform(-3, 3, (B, F_, 1)))).astype(np.float32) + np.float32(1e-3)
    own = [17, 9]
    rowptr = torch.arange(0, n_mels * n_bins + 1, n_bins, dtype=torch.int32)
    col = torch.arange(n_bins, dtype=torch.int32).repeat(n_mels)
    assert int(rowptr[-1]) == 1608 > 1024
    csr = (rowptr.to(DEV), col.to(DEV), t(fb.reshape(-1)))
    frames = torch.tensor(own, dtype=torch.int32, device=DEV)
    out = ops.mel_log_norm(t(P), n_bins, F_ * n_bins, csr, B, F_, n_mels, normalize, frames=frames).cpu().numpy()
    full = ops.mel_log_norm(t(P), n_bins, F_ * n_bins, csr, B, F_, n_mels, normalize).cpu().numpy()
    ref = np.log(np.einsum("mk,bfk->bfm", fb.astype(np.float64), P.astype(np.float64)) + 1e-10)
    for b, f in enumerate(own):
        want = ref[b, :f]
        if normalize:
            assert want.std(axis=0, ddof=1).min() > 1.0
            want = (want - want.mean(axis=0)) / (want.std(axis=0, ddof=1) + 1e-10)
        assert_mel(out[b, :f], want)
        assert not out[b, f:].any()
    want = ref[0]
    if normalize:
        want = (want - want.mean(axis=0)) / (want.std(axis=0, ddof=1) + 1e-10)
    np.testing.assert_array_equal(full[0], out[0])  # the same utterance with and without frame counts
    assert_mel(full[0], want)


# ----------------------------------------------------------------------------- e. unwritten / over-written memory
GUARD = 64


def _poisoned(n):
    return torch.full((n,), float("nan"), device=DEV, dtype=torch.float32)


@pytest.mark.parametrize("n_mels", [80, 96], ids=["chunked", "unchunked"])
@pytest.mark.parametrize("normalize", [True, False], ids=["norm", "raw"])
def test_mel_log_norm_writes_exactly_its_frames(va, n_mels, normalize):
    """vasr_mel_log_norm_f32 / _var_f32 through the C ABI into nan-filled output and workspace,
    frame_off = 1, out_stride = (F + 3) n_mels + 5: every element of [0, (F + 3) n_mels) is
    written (the mel where the frames are, zeros around them), and the 5-float tail of each
    utterance and the guard after the buffer keep their nan."""
    from velocity_asr import _lib, audio as A, ops
    lib = _lib.lib()
    B, F_, n_bins, off = 2, 17, 201, 1
    tb = A._tables(torch.device(DEV, torch.cuda.current_device()), 400, n_mels, 16000)
    rowptr, col, val = tb.fb_csr
    rng = np.random.default_rng(44 + n_mels)
    P = t((rng.random((B, F_, n_bins)) * np.exp(rng.uniform(-3, 3, (B, F_, 1)))).astype(np.float32))
    Fo = F_ + 3
    stride = Fo * n_mels + 5
    nws = int(lib.vasr_mel_workspace_floats(B, F_, n_mels))
    stream = _lib.stream_of(P)

    def run(frames):
        out, ws = _poisoned(B * stride + GUARD), _poisoned(nws)
        if frames is None:
            rc = lib.vasr_mel_log_norm_f32(P.data_ptr(), n_bins, F_ * n_bins, rowptr.data_ptr(), col.data_ptr(),
                                           val.data_ptr(), out.data_ptr(), stride, off, B, F_, n_mels, int(normalize),
                                           ws.data_ptr(), stream)
        else:
            rc = lib.vasr_mel_log_norm_var_f32(P.data_ptr(), n_bins, F_ * n_bins, rowptr.data_ptr(), col.data_ptr(),
                                               val.data_ptr(), out.data_ptr(), stride, off, B, F_, n_mels,
                                               int(normalize), frames.data_ptr(), ws.data_ptr(), stream)
        torch.cuda.synchronize()
        return rc, out

    def check(out, plain):
        assert torch.isnan(out[B * stride:]).all()
        rows = out[:B * stride].view(B, stride)
        assert torch.isnan(rows[:, Fo * n_mels:]).all()
        body = rows[:, :Fo * n_mels].reshape(B, Fo, n_mels)
        want = torch.zeros_like(body)
        want[:, off:off + F_] = plain
        assert torch.equal(bits(body), bits(want))

    plain = ops.mel_log_norm(P, n_bins, F_ * n_bins, tb.fb_csr, B, F_, n_mels, normalize)
    assert torch.isfinite(plain).all()
    rc, out = run(None)
    assert rc == 0
    check(out, plain)

    frames = torch.tensor([F_, 9], dtype=torch.int32, device=DEV)
    rc, out = run(frames)
    if n_mels > 85:  # per-utterance frame counts need the chunked pass: refused, nothing written
        assert rc != 0 and "per-utterance frame counts" in lib.vasr_last_error().decode()
        assert torch.isnan(out).all()
        return
    assert rc == 0
    plain_var = ops.mel_log_norm(P, n_bins, F_ * n_bins, tb.fb_csr, B, F_, n_mels, normalize, frames=frames)
    assert torch.equal(plain_var[0], plain[0]) and torch.count_nonzero(plain_var[1, 9:]).item() == 0
    check(out, plain_var)


@pytest.mark.parametrize("off", [0, 2])
def test_pad_frames_vs_torch_pad(va, off):
    """ops.pad_frames and vasr_pad_frames_f32 against F.pad with out_frames > F + off: zeros
    before and after, nothing past the buffer (nan guard kept)."""
    from velocity_asr import _lib, ops
    B, F_, C = 2, 5, 80
    out_frames = F_ + off + 3
    x = t(np.random.default_rng(50 + off).standard_normal((B, F_, C)).astype(np.float32))
    want = torch.nn.functional.pad(x, (0, 0, off, out_frames - F_ - off))
    assert torch.equal(ops.pad_frames(x, out_frames, off), want)
    out = _poisoned(B * out_frames * C + GUARD)
    rc = _lib.lib().vasr_pad_frames_f32(x.data_ptr(), out.data_ptr(), out_frames, off, B, F_, C, _lib.stream_of(x))
    torch.cuda.synchronize()
    assert rc == 0
    assert torch.equal(out[:B * out_frames * C].view(B, out_frames, C), want)
    assert torch.isnan(out[B * out_frames * C:]).all()


def test_reflect_pad_vs_torch_pad(va):
    """ops.reflect_pad and vasr_reflect_pad_f32 against F.pad(mode="reflect") at the shortest
    legal input (S = pad + 1) with ld_out > S + 2 pad: the row tail is 0, the guard kept."""
    from velocity_asr import _lib, ops
    B, pad = 3, 200
    S_ = pad + 1
    ld = S_ + 2 * pad + 7
    x = t(np.random.default_rng(60).standard_normal((B, S_)).astype(np.float32))
    want = torch.zeros((B, ld), device=DEV)
    want[:, :S_ + 2 * pad] = torch.nn.functional.pad(x.unsqueeze(1), (pad, pad), mode="reflect").squeeze(1)
    assert torch.equal(ops.reflect_pad(x, pad, ld), want)
    out = _poisoned(B * ld + GUARD)
    rc = _lib.lib().vasr_reflect_pad_f32(x.data_ptr(), S_, out.data_ptr(), ld, B, S_, pad, _lib.stream_of(x))
    torch.cuda.synchronize()
    assert rc == 0
    assert torch.equal(out[:B * ld].view(B, ld), want)
    assert torch.isnan(out[B * ld:]).all()


# ----------------------------------------------------------------------------- f. argument errors
def test_argument_errors(va):
    x = torch.zeros((2, 2000), device=DEV)
    with pytest.raises(NotImplementedError):
        va.compute_mel_spectrogram(x, n_fft=402)
    for kw, S_ in ((dict(), 200), (dict(n_fft=512, hop_length=128), 256)):  # S <= n_fft // 2
        with pytest.raises(RuntimeError) as e:
            va.compute_mel_spectrogram(x[:, :S_].contiguous(), **kw)
        assert e.type is RuntimeError  # not its subclass NotImplementedError
    lens = torch.tensor([2000, 1500], dtype=torch.int32)
    with pytest.raises(NotImplementedError):
        va.compute_mel_spectrogram(x, n_mels=128, lengths=lens)
    with pytest.raises(NotImplementedError):
        va.compute_mel_spectrogram(x, n_fft=512, lengths=lens)
