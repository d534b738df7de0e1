"""Long-form segmentation on the device: the three kernels against the host rule, bit for bit, and
transcribe_files over recordings cut into segments against each planned segment decoded alone.
Every comparison is exact (torch.equal / array_equal / list equality)."""

import numpy as np
import pytest
import torch

import longform_cases as lc
from velocity_asr import synthetic as S

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module")
def A():
    from velocity_asr import _lib, audio
    _lib.load()
    return audio


@pytest.fixture(scope="module")
def ops(A):
    from velocity_asr import ops
    return ops


@pytest.fixture(scope="module")
def tile(A):
    from velocity_asr import _lib
    return int(_lib.lib().vasr_segment_tile_blocks())


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _edge_lengths(T):
    return [319, 320, 321, 320 * T - 1, 320 * T, 320 * T + 1, 2 * 320 * T + 17]


def test_block_energy_alone_is_the_host_chain(A, ops, tile):
    for n in _edge_lengths(tile):
        x = lc.signal(n, seed=n)
        E = ops.block_energy(torch.from_numpy(x)[None].to(DEV))
        assert E.dtype == torch.float64 and tuple(E.shape) == (1, n // 320)
        assert np.array_equal(_bits(E.cpu().numpy()[0]), _bits(A.block_energy_host(x))), n


@pytest.mark.parametrize("extra", [4, 7], ids=["rows16B", "rows_unaligned"])
def test_block_energy_of_a_padded_batch_honours_the_lengths(A, ops, tile, extra):
    """Five recordings in one batch, the padding filled with 1e3: each row's full blocks are the
    recording's alone, the other blocks 0.  extra 7 makes the row stride odd (the scalar loads)."""
    ns = [2 * 320 * tile + 17, 320 * tile - 1, 321, 320 * tile + 1, 319]
    Smax = max(ns) + 320 + extra
    x = np.full((len(ns), Smax), 1e3, np.float32)
    for b, n in enumerate(ns):
        x[b, :n] = lc.signal(n, seed=100 + n)
    samples = torch.tensor(ns, dtype=torch.int32).to(DEV)
    E = ops.block_energy(torch.from_numpy(x).to(DEV), samples).cpu().numpy()
    assert E.shape == (len(ns), Smax // 320)
    for b, n in enumerate(ns):
        alone = A.block_energy_host(x[b, :n])
        assert np.array_equal(_bits(E[b, :n // 320]), _bits(alone)), b
        assert not E[b, n // 320:].any(), b
    # without lengths the padding counts
    full = ops.block_energy(torch.from_numpy(x).to(DEV)).cpu().numpy()
    assert np.array_equal(_bits(full[4]), _bits(A.block_energy_host(x[4])))


def _plan_recordings(M):
    z = lc.signal(9 * M + 55, seed=5, zero_stretches=0)
    for a in (M // 2, 3 * M, 5 * M + 321):  # several all-zero stretches, longer than a window: exact ties
        z[a:a + M] = 0.0
    return [lc.signal(M - 640, seed=1), lc.signal(M, seed=2), lc.signal(M + 1, seed=3), lc.signal(40 * M + 123, seed=4),
            z, np.zeros(6 * M + 9, np.float32)]


# m 4000 needs 13 blocks and M 8000 holds 25, one short of the rule's MB >= 2 mB; 3840 is the most it takes
@pytest.mark.parametrize("m,M", [(3840, 8000), (4000, 12000)])
def test_plan_equals_the_host_alone_and_in_a_batch(A, ops, m, M):
    W = 4
    recs = _plan_recordings(M)
    want = [A.plan_segments_host(x, M, m, W) for x in recs]
    assert want[0] == [] and want[1] == [] and len(want[2]) == 1 and len(want[3]) >= 40
    mB = -(-m // 320)
    assert want[5] == [k * mB * 320 for k in range(1, len(want[5]) + 1)]  # all ties: the lowest candidate
    for x, w in zip(recs, want):
        lc.check_plan(w, len(x), m, M)
        got = A.plan_segments(torch.from_numpy(x).to(DEV), max_samples=M, min_samples=m, window_blocks=W)
        assert got == [w], len(x)
    ns = [len(x) for x in recs]
    batch = np.full((len(recs), max(ns) + 5), 1e3, np.float32)  # the padding is not silence
    for b, x in enumerate(recs):
        batch[b, :ns[b]] = x
    got = A.plan_segments(torch.from_numpy(batch).to(DEV), ns, max_samples=M, min_samples=m, window_blocks=W)
    assert got == want


def test_plan_refuses_a_table_one_column_too_narrow(A, ops):
    from velocity_asr import _lib
    m, M, W = 4000, 12000, 4
    x = lc.signal(40 * M + 123, seed=4)
    E = ops.block_energy(torch.from_numpy(x)[None].to(DEV))
    need = int(_lib.lib().vasr_segment_max_cuts(len(x), m))
    assert need == (len(x) // 320) // 13
    with pytest.raises(ValueError, match="too narrow"):
        ops.segment_plan(E, len(x), M, m, W, max_cuts=need - 1)
    cuts, n_cuts = ops.segment_plan(E, len(x), M, m, W, max_cuts=need)
    k = int(n_cuts.cpu()[0])
    assert tuple(cuts.shape) == (1, need) and cuts.cpu()[0, :k].tolist() == A.plan_segments_host(x, M, m, W)
    assert not cuts.cpu()[0, k:].any()  # nothing written past the count
    with pytest.raises(ValueError):
        ops.segment_plan(E.to(torch.float32), len(x), M, m, W)
    with pytest.raises(ValueError):
        ops.segment_plan(E[:, :-1], len(x), M, m, W)


def test_gather_rows_are_the_slices_followed_by_zeros(A, ops):
    m, M, W = 4000, 12000, 4
    xs = [lc.signal(3 * M + 1234, seed=11), lc.signal(2 * M + 77, seed=12)]
    ns = [len(x) for x in xs]
    rec = np.full((2, max(ns) + 3), 1e3, np.float32)
    for b, x in enumerate(xs):
        rec[b, :ns[b]] = x
    dev = torch.from_numpy(rec).to(DEV)
    cuts = A.plan_segments(dev, ns, max_samples=M, min_samples=m, window_blocks=W)
    assert cuts == [A.plan_segments_host(x, M, m, W) for x in xs] and all(cuts)
    batch, seg_lengths, table = A.segment_on_device(dev, ns, cuts)
    want = [(b, s, n) for b in range(2) for s, n in lc.segments_of(ns[b], cuts[b])]
    assert table == want and seg_lengths == [n for _, _, n in want]
    assert tuple(batch.shape) == (len(want), max(seg_lengths)) and batch.dtype == torch.float32
    got = batch.cpu().numpy()
    for g, (b, s, n) in enumerate(want):
        assert np.array_equal(got[g, :n].view(np.uint32), xs[b][s:s + n].view(np.uint32)), g
        assert not got[g, n:].any() and not np.signbit(got[g, n:]).any(), g
    # a wider output row, unaligned starts, and rows that do not lie in their recording (zeros, no fault)
    tb = torch.tensor([[1, 3, 1001], [0, ns[0] - 5, 5], [2, 0, 10], [0, -1, 10], [0, ns[0], rec.shape[1]], [1, 0, 2001]],
                      dtype=torch.int64).to(DEV)
    y = ops.segment_gather(dev, tb, 2000).cpu().numpy()
    assert np.array_equal(y[0, :1001], rec[1, 3:1004]) and not y[0, 1001:].any()
    assert np.array_equal(y[1, :5], rec[0, ns[0] - 5:ns[0]]) and not y[1, 5:].any()
    assert not y[2:].any()
    with pytest.raises(ValueError):
        ops.segment_gather(dev, tb.to(torch.int32), 2000)
    with pytest.raises(ValueError):
        ops.segment_gather(dev.to(torch.float64), tb, 2000)


# ---------------------------------------------------------------- tokens end to end

M_E2E, m_E2E = 16000, 6400


@pytest.fixture(scope="module")
def model():
    import velocity_asr as va
    W = S.make_weights(None, seed=0)
    mdl = va.VELOCITYASR()
    mdl.load_state_dict({k: torch.from_numpy(v) for k, v in W.items()}, strict=True)
    return mdl.to(DEV).eval(), va.CTCDecoder(va.create_default_vocabulary(mdl.config.vocab_size))


@pytest.fixture(scope="module")
def recordings():
    return [S.make_audio(1, 3 * 16000 + 123, seed=71)[0], S.make_audio(1, 2 * 16000 + 4567, seed=72)[0]]


@pytest.fixture(scope="module")
def alone(A, model, recordings):
    """Per recording: its planned cuts and, for each planned segment decoded alone at B = 1, the
    greedy_scored arrays with the spans shifted by start // 320, concatenated by hand."""
    mdl, dec = model
    out = []
    for x in recordings:
        cuts = A.plan_segments_host(x, M_E2E, m_E2E)
        keys = ("tokens", "start", "end", "logp_sum", "logp_min")
        cat = {k: [] for k in keys}
        score = 0.0
        for s, n in lc.segments_of(len(x), cuts):
            mel = A.mel_on_device(torch.from_numpy(x[s:s + n])[None].to(DEV), n_mels=mdl.config.mel_bins,
                                  frame_pad=mdl.temporal_binding.conv_padding())
            toks, lens, st, en, lsum, lmin, path = (t.cpu().numpy() for t in mdl.greedy_scored(mel, blank=dec.blank_token))
            k = int(lens[0])
            cat["tokens"] += toks[0, :k].tolist()
            cat["start"] += (st[0, :k].astype(np.int64) + s // 320).tolist()
            cat["end"] += (en[0, :k].astype(np.int64) + s // 320).tolist()
            cat["logp_sum"] += lsum[0, :k].tolist()
            cat["logp_min"] += lmin[0, :k].tolist()
            score = score + float(path[0])
        cat["path_logp"] = score
        out.append((cuts, cat))
    return out


def test_longform_arrays_equal_each_segment_alone(A, model, recordings, alone):
    """Both recordings in one call: plan on the device, gather, one padded batch through the scored
    greedy decode, stitch: the integer arrays and log-probabilities of every segment decoded alone."""
    from velocity_asr import transcription as T
    mdl, dec = model
    ns = [len(x) for x in recordings]
    rec = np.zeros((2, max(ns)), np.float32)
    for b, x in enumerate(recordings):
        rec[b, :ns[b]] = x
    dev = torch.from_numpy(rec).to(DEV)
    cuts = A.plan_segments(dev, ns, max_samples=M_E2E, min_samples=m_E2E)
    assert cuts == [c for c, _ in alone] and len(cuts[0]) >= 3 and len(cuts[1]) >= 2
    batch, seg_lengths, table = A.segment_on_device(dev, ns, cuts)
    raw = T._decode_batch(mdl, batch, dec, True, lengths=seg_lengths, confidence=True, raw=True)
    for b in range(2):
        rows = [g for g, r in enumerate(table) if r[0] == b]
        got = T.stitch_segments([raw[g] for g in rows], [table[g][1] for g in rows])
        want = alone[b][1]
        assert len(want["tokens"]) > 0
        for k in ("tokens", "start", "end", "logp_sum", "logp_min"):
            assert got[k] == want[k], (b, k)
        assert got["run_lengths"] == [e - s for s, e in zip(want["start"], want["end"])]
        assert got["path_logp"] == want["path_logp"]


@pytest.fixture(scope="module")
def wavs(A, recordings, tmp_path_factory):
    d = tmp_path_factory.mktemp("longform")
    paths = []
    for i, x in enumerate(recordings):
        p = d / f"rec{i}.wav"
        A.write_wav(str(p), torch.from_numpy(x))
        paths.append(str(p))
    return paths


SEG = dict(segment_seconds=1.0, min_segment_seconds=0.4)


def test_transcribe_files_stitches_words_confidences_and_score(A, model, wavs, alone):
    from velocity_asr import transcription as T
    from velocity_asr.decode import token_confidences
    mdl, dec = model
    got = T.transcribe_files(mdl, wavs, dec, DEV, confidence=True, **SEG)
    plain = T.transcribe_files(mdl, wavs, dec, DEV, **SEG)
    timed = T.transcribe_files(mdl, wavs, dec, DEV, timestamps=True, **SEG)
    for b, (cuts, w) in enumerate(alone):
        spans = list(zip(w["start"], w["end"]))
        conf = token_confidences(w["logp_sum"], w["logp_min"], [e - s for s, e in spans], "mean")
        words = T.group_words(w["tokens"], spans, dec.vocabulary, conf)
        n = 3 * 16000 + 123 if b == 0 else 2 * 16000 + 4567
        assert got[b] == {"file": wavs[b], "duration": n / 16000, "transcription": " ".join(x["word"] for x in words),
                          "words": words, "score": w["path_logp"]}
        assert plain[b] == {"file": wavs[b], "duration": n / 16000, "transcription": dec._tokens_to_text(w["tokens"])}
        bare = T.group_words(w["tokens"], spans, dec.vocabulary)
        assert timed[b] == {"file": wavs[b], "duration": n / 16000, "transcription": " ".join(x["word"] for x in bare),
                            "words": bare}


def test_transcribe_files_beam_joins_each_segments_best_hypothesis(A, model, recordings, wavs, alone):
    from velocity_asr import transcription as T
    mdl, dec = model
    got = T.transcribe_files(mdl, wavs, dec, DEV, beam_width=4, **SEG)
    for b, x in enumerate(recordings):
        tokens = []
        for s, n in lc.segments_of(len(x), alone[b][0]):  # each segment searched alone
            seg = torch.from_numpy(x[s:s + n])[None].to(DEV)
            tokens += T._decode_batch(mdl, seg, dec, False, beam_width=4, raw=True)[0]["tokens"]
        assert tokens and got[b]["transcription"] == dec._tokens_to_text(tokens)
        assert set(got[b]) == {"file", "duration", "transcription"}


def test_a_44k_stereo_file_gives_the_host_resampled_result(A, model, tmp_path, monkeypatch):
    """44.1 kHz stereo files: resampled on the device, planned and gathered there, against the route
    that resamples on the host (VASR_DEVICE_RESAMPLE=0) and uploads 16 kHz samples."""
    from velocity_asr import transcription as T
    mdl, dec = model
    paths = []
    for i, sec in enumerate((3.01, 2.2)):
        p = str(tmp_path / f"s{i}.wav")
        A.write_wav(p, torch.from_numpy(S.make_audio(2, int(44100 * sec), seed=80 + i)), 44100)
        paths.append(p)
    calls = []
    real = T.resample_on_device
    monkeypatch.setattr(T, "resample_on_device", lambda *a, **k: calls.append(a[1]) or real(*a, **k))
    dev = T.transcribe_files(mdl, paths, dec, DEV, confidence=True, **SEG)
    assert calls == [44100]
    monkeypatch.setenv("VASR_DEVICE_RESAMPLE", "0")
    host = T.transcribe_files(mdl, paths, dec, DEV, confidence=True, **SEG)
    assert calls == [44100] and dev == host
    assert all("error" not in r and r["transcription"] for r in dev)
    # and the host-resampled samples planned by the host rule give the segments the device planned
    a16 = A.load_audio(paths[0])
    cuts = A.plan_segments(a16, max_samples=16000, min_samples=6400)[0]
    assert len(cuts) >= 3 and cuts == A.plan_segments(a16.to(DEV), max_samples=16000, min_samples=6400)[0]


def test_a_recording_over_the_limit(A, model, tmp_path, monkeypatch):
    """101 s: an error by default, as before; with segment_seconds=30 a transcription whose duration
    is the recording's, from segments of at most 30 s; a short file in the same call is untouched."""
    from velocity_asr import transcription as T
    mdl, dec = model
    n = 101 * 16000
    long = str(tmp_path / "long.wav")
    A.write_wav(long, torch.from_numpy(S.make_audio(1, n, seed=90)[0]))
    short = str(tmp_path / "short.wav")
    A.write_wav(short, torch.from_numpy(S.make_audio(1, 20000, seed=91)[0]))
    r = T.transcribe_files(mdl, [long], dec, DEV, timestamps=True)[0]
    assert set(r) == {"file", "error"} and "positional table" in r["error"]
    base = T.transcribe_files(mdl, [short], dec, DEV, timestamps=True)[0]
    seen = []
    real = T.segment_on_device
    monkeypatch.setattr(T, "segment_on_device", lambda *a, **k: seen.append(real(*a, **k)) or seen[-1])
    got = T.transcribe_files(mdl, [long, short], dec, DEV, timestamps=True, segment_seconds=30)
    assert got[1] == base
    assert set(got[0]) == {"file", "duration", "transcription", "words"} and got[0]["duration"] == 101.0
    assert got[0]["transcription"] and got[0]["words"][-1]["end"] > 90.0
    (_, seg_lengths, table), = seen
    assert sum(seg_lengths) == n and 4 <= len(seg_lengths) <= 10
    assert all(160000 <= v <= 480000 for v in seg_lengths)  # min_segment_seconds: a third of 30 s
    assert all(s % 320 == 0 for _, s, _ in table)
