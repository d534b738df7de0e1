"""Pin the CPU oracle (oracle/velocity_ref.py) to the reference's golden outputs.

The goldens were produced by the real reference (tests/golden/gen_goldens.py), so
these tests are what makes the oracle trustworthy as the checker for the HIP path.
"""

import json

import numpy as np
import pytest

import mel_geometry_cases as G
from conftest import golden, golden_json
from oracle import velocity_ref as R
from velocity_asr import synthetic as S

FWD_TOL = dict(atol=1e-4, rtol=1e-4)


def test_window_and_filterbank_match_reference():
    g = golden("mel.npz")
    np.testing.assert_allclose(R.hann_window(), g["hann"], atol=5e-7, rtol=0)
    fb = R.mel_filterbank()
    assert fb.shape == (80, 201)
    np.testing.assert_array_equal(fb, g["filterbank"])  # bit-exact restatement
    # 393 non-zeros, 1-14 per row
    assert int((g["filterbank"] > 0).sum()) == 393


@pytest.mark.parametrize("name,make", [
    ("rand_b2_1s", lambda: S.make_audio(2, 16000, seed=11)),
    ("rand_b2_10s", lambda: S.make_audio(2, 160000, seed=1234)),
    ("odd_16333", lambda: S.make_audio(3, 16333, seed=8)),
    ("chirp_3s", lambda: S.make_chirp(48000)[None]),
    ("zero_1s", lambda: np.zeros((1, 16000), np.float32)),
    ("short_201", lambda: S.make_audio(1, 201, seed=5)),
    ("short_400", lambda: S.make_audio(1, 400, seed=6)),
    ("oned_8000", lambda: S.make_audio(1, 8000, seed=9)[0]),
])
def test_mel_matches_reference(name, make):
    g = golden("mel.npz")
    audio = make()
    if name + "__audio" in g.files:
        np.testing.assert_array_equal(audio.reshape(g[name + "__audio"].shape), g[name + "__audio"])
    mel = R.compute_mel_spectrogram(audio)
    assert mel.shape == g[name].shape
    np.testing.assert_allclose(mel, g[name], atol=2e-4, rtol=1e-4)


def test_geometry_golden_holds_the_case_table():
    meta = json.loads(str(golden("mel_geometry.npz")["meta"]))
    assert [tuple(c) for c in meta["cases"]] == G.CASES
    assert set(meta["own_fp32_vs_fp64"]) == {G.name(*c) for c in G.CASES}


@pytest.mark.parametrize("normalize", [True, False], ids=["norm", "raw"])
@pytest.mark.parametrize("case", G.CASES, ids=lambda c: G.name(*c))
def test_mel_geometry_matches_reference(case, normalize):
    """The oracle with the reference's parameters (sample_rate, n_fft, hop_length, n_mels,
    normalize) against the reference's output off the default geometry.  Bins of empty filters
    (taken from the filterbank) are left out of the normalised comparison: their row is the
    constant log(1e-10), which the oracle's fp64 mean maps to 0 and the reference's fp32 mean to
    noise; a single frame normalises to nan in both."""
    sr, n_fft, hop, n_mels, S_ = case
    g = golden("mel_geometry.npz")
    name = G.name(*case)
    want = g[f"{name}__{'norm' if normalize else 'raw'}"]
    mel = R.compute_mel_spectrogram(G.audio(name, S_), sample_rate=sr, n_fft=n_fft, hop_length=hop,
                                    n_mels=n_mels, normalize=normalize)
    assert mel.shape == want.shape == (2, S_ // hop + 1, n_mels)
    empty = g[f"fb_{n_fft}_{n_mels}_{sr}"].sum(1) == 0
    if S_ // hop + 1 == 1 and normalize:
        assert np.isnan(want).all() and np.isnan(mel).all()
        return
    assert np.isfinite(mel).all()
    keep = ~empty if normalize else np.ones(n_mels, bool)
    np.testing.assert_allclose(mel[..., keep], want[..., keep], atol=2e-4, rtol=1e-4)
    if normalize:
        assert not mel[..., empty].any()


@pytest.mark.parametrize("case", sorted({(c[1], c[3], c[0]) for c in G.CASES}),
                         ids=lambda c: "fft%d_mel%d_sr%d" % c)
def test_filterbanks_match_reference(case):
    """The package's filterbank is the reference's, bit for bit, at every geometry (the same
    torch ops in the same order).  The oracle's numpy restatement has the same support and
    weights within 5e-5: numpy's float32 log10 / pow can differ from torch's vectorised ones by
    an ulp.  An ulp of mel_max (2^-12 mel near 3800) moves the top band edges by
    2^-12 * (700 + hz) ln10 / 2595 = 2.5e-3 Hz at 11 kHz, plus an ulp of the edge itself
    (2^-10 Hz), and a slope divides that by a band half-width of >= 100 Hz there: <= 3.5e-5
    (measured 1.8e-5 at 22.05 kHz / 128 bins; bit-exact at the default geometry,
    test_window_and_filterbank_match_reference).  The mel tests above bound its effect."""
    import torch
    from velocity_asr import audio as A
    n_fft, n_mels, sr = case
    want = golden("mel_geometry.npz")["fb_%d_%d_%d" % case]
    assert want.shape == (n_mels, n_fft // 2 + 1)
    np.testing.assert_array_equal(A._create_mel_filterbank(n_fft, n_mels, sr, torch.device("cpu")).numpy(), want)
    fb = R.mel_filterbank(n_fft, n_mels, sr)
    np.testing.assert_allclose(fb, want, atol=5e-5, rtol=0)
    np.testing.assert_array_equal(fb.sum(1) == 0, want.sum(1) == 0)


def test_geometry_goldens_empty_filters():
    """The empty filters (fb.sum(1) == 0) the GPU tests exclude: 4 and 2 bins, on two rows."""
    g = golden("mel_geometry.npz")
    got = {G.name(*c): int((g["fb_%d_%d_%d" % (c[1], c[3], c[0])].sum(1) == 0).sum())
           for c in G.CASES}
    assert {k: v for k, v in got.items() if v} == {"sr16000_fft400_hop160_mel128_S2560": 4,
                                                   "sr16000_fft256_hop64_mel80_S1100": 2}


@pytest.mark.parametrize("L", [1, 2, 3, 5, 8, 16, 17, 31, 64, 100, 257])
def test_stream_equals_tree_bitwise(L):
    rng = np.random.default_rng(L)
    dA = np.exp(-rng.random((2, L, 3, 4)) * 3).astype(np.float32)
    xdB = rng.standard_normal((2, L, 3, 4)).astype(np.float32)
    tree = R.associative_scan_tree(dA, xdB)
    stream = R.associative_scan_stream(dA, xdB)
    np.testing.assert_array_equal(stream, tree)
    assert np.all(tree[:, 0] == 0)  # exclusive prefix: h[0] = 0


def _scan_cases():
    meta = json.loads(str(golden("scan.npz")["meta"]))
    return [tuple(c) for c in meta["cases"]]


@pytest.mark.parametrize("case", _scan_cases(), ids=lambda c: c[0])
def test_scan_matches_reference(case):
    import sys
    sys.path.insert(0, __import__("os").path.dirname(__file__) + "/golden")
    name, seed, B, L, Di, N = case
    g = golden("scan.npz")
    x, dt, Bm, Cm, A_log, D = scan_inputs(seed, B, L, Di, N)
    A = (-np.exp(A_log)).astype(np.float32)
    yp = R.parallel_scan(x, dt, A, Bm, Cm, D)
    ys = R.sequential_scan(x, dt, A, Bm, Cm, D)
    np.testing.assert_allclose(yp, g[name + "__parallel"], atol=5e-5, rtol=5e-5)
    np.testing.assert_allclose(ys, g[name + "__sequential"], atol=5e-5, rtol=5e-5)
    if L > 8:  # the reference's tree scan is NOT the recurrence
        assert np.abs(g[name + "__parallel"] - g[name + "__sequential"]).max() > 1e-2


@pytest.mark.parametrize("case", _scan_cases(), ids=lambda c: c[0])
def test_mamba_restatement_is_the_sequential_golden(case):
    """scan_mode="mamba" (ssm.py:297-337) calls mamba-ssm's selective_scan_fn, absent here
    (parity unpinned against the package itself): its published reference algorithm,
    restated in the oracle with the documented (B, G, N, L) layout, is the recurrence whose
    reference outputs are the `__sequential` goldens."""
    name, seed, B, L, Di, N = case
    g = golden("scan.npz")
    x, dt, Bm, Cm, A_log, D = scan_inputs(seed, B, L, Di, N)
    A = (-np.exp(A_log)).astype(np.float32)
    ym = R.mamba_scan(x, dt, A, Bm, Cm, D)
    np.testing.assert_allclose(ym, g[name + "__sequential"], atol=5e-5, rtol=5e-5)


def test_selective_scan_ref_groups_gate_bias():
    """selective_scan_ref restatement beyond the reference's call: B/C groups, the z gate,
    delta bias + softplus, against a direct per-channel loop."""
    rng = np.random.default_rng(7)
    Bsz, Dd, L, N, G = 2, 8, 13, 4, 2
    u = rng.standard_normal((Bsz, Dd, L)).astype(np.float32)
    delta = rng.standard_normal((Bsz, Dd, L)).astype(np.float32)
    A = -np.exp(rng.standard_normal((Dd, N))).astype(np.float32)
    Bv = rng.standard_normal((Bsz, G, N, L)).astype(np.float32)
    Cv = rng.standard_normal((Bsz, G, N, L)).astype(np.float32)
    D = rng.standard_normal(Dd).astype(np.float32)
    z = rng.standard_normal((Bsz, Dd, L)).astype(np.float32)
    bias = rng.standard_normal(Dd).astype(np.float32)
    got = R.selective_scan_ref(u, delta, A, Bv, Cv, D, z=z, delta_bias=bias, delta_softplus=True)
    dl = np.log1p(np.exp((delta + bias[None, :, None]).astype(np.float64)))
    want = np.zeros((Bsz, Dd, L))
    for b in range(Bsz):
        for d in range(Dd):
            gi = d // (Dd // G)
            h = np.zeros(N)
            for t in range(L):
                h = np.exp(dl[b, d, t] * A[d]) * h + dl[b, d, t] * Bv[b, gi, :, t] * u[b, d, t]
                want[b, d, t] = h @ Cv[b, gi, :, t] + u[b, d, t] * D[d]
    want *= z / (1.0 + np.exp(-z.astype(np.float64)))
    np.testing.assert_allclose(got, want, atol=1e-4, rtol=1e-4)


def scan_inputs(seed, B, L, Di, N):
    """Same draws as tests/golden/gen_goldens.py:scan_inputs."""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((B, L, Di)).astype(np.float32)
    dt = np.log1p(np.exp(rng.standard_normal((B, L, Di)) * 0.7 - 1.0)).astype(np.float32)
    Bm = rng.standard_normal((B, L, N)).astype(np.float32)
    Cm = rng.standard_normal((B, L, N)).astype(np.float32)
    A_log = (np.log(np.arange(1, N + 1)) + 0.01 * rng.standard_normal(N)).astype(np.float32)
    D = (1.0 + 0.1 * rng.standard_normal(Di)).astype(np.float32)
    return x, dt, Bm, Cm, A_log, D


def test_forward_stages_b2_3s(default_weights):
    g = golden("fwd_b2_3s.npz")
    cfg = dict(S.DEFAULT_CONFIG)
    mel = R.compute_mel_spectrogram(S.make_audio(2, 48000, seed=21))
    np.testing.assert_allclose(mel, g["mel"], atol=2e-4, rtol=1e-4)
    logits, f = R.forward(default_weights, g["mel"], cfg, return_features=True)
    np.testing.assert_allclose(f["temporal_binding"], g["temporal_binding"], **FWD_TOL)
    np.testing.assert_allclose(f["local_features"], g["local_features"], **FWD_TOL)
    np.testing.assert_allclose(f["fused_features"], g["fused_features"], **FWD_TOL)
    np.testing.assert_allclose(logits, g["logits"], **FWD_TOL)
    np.testing.assert_array_equal(logits.argmax(-1), g["tokens"])


def test_forward_from_audio_b2_3s(default_weights):
    g = golden("fwd_b2_3s.npz")
    mel = R.compute_mel_spectrogram(S.make_audio(2, 48000, seed=21))
    logits = R.forward(default_weights, mel, dict(S.DEFAULT_CONFIG))
    np.testing.assert_allclose(logits, g["logits"], atol=5e-4, rtol=1e-4)
    np.testing.assert_array_equal(logits.argmax(-1), g["tokens"])
    dec = golden_json("decode_fwd.json")["results"]
    assert R.ctc_greedy_decode(logits) == dec["b2_3s"]
    ts = R.ctc_greedy_decode_with_timestamps(logits)
    assert [[t, [list(x) for x in s]] for t, s in ts] == dec["b2_3s_ts"]


def test_forward_edge_lengths(default_weights):
    g = golden("fwd_edge.npz")
    for S_, seed in ((201, 31), (400, 32), (1600, 33), (8000, 34), (16333, 35)):
        mel = R.compute_mel_spectrogram(S.make_audio(1, S_, seed=seed))
        logits = R.forward(default_weights, mel, dict(S.DEFAULT_CONFIG))
        np.testing.assert_allclose(logits, g[f"S{S_}__logits"], atol=5e-4, rtol=1e-4)
        np.testing.assert_array_equal(logits.argmax(-1), g[f"S{S_}__tokens"])


def test_forward_mel_input_500(default_weights):
    g = golden("fwd_melin_500.npz")
    mel = np.random.default_rng(41).standard_normal((2, 500, 80)).astype(np.float32)
    logits = R.forward(default_weights, mel, dict(S.DEFAULT_CONFIG))
    assert logits.shape == (2, 250, 1000)
    np.testing.assert_allclose(logits, g["logits"], **FWD_TOL)
    np.testing.assert_array_equal(logits.argmax(-1), g["tokens"])


def test_forward_sequential_mode():
    g = golden("fwd_seq_b2_3s.npz")
    cfg = dict(S.DEFAULT_CONFIG, scan_mode="sequential")
    W = S.make_weights(cfg, seed=0)
    mel = R.compute_mel_spectrogram(S.make_audio(2, 48000, seed=21))
    logits = R.forward(W, mel, cfg)
    np.testing.assert_allclose(logits, g["logits"], atol=5e-4, rtol=1e-4)
    np.testing.assert_array_equal(logits.argmax(-1), g["tokens"])


def test_forward_small_config():
    g = golden("fwd_smallcfg.npz")
    cfg = dict(S.DEFAULT_CONFIG, **json.loads(str(g["meta"]))["config"])
    W = S.make_weights(cfg, seed=3)
    mel = R.compute_mel_spectrogram(S.make_audio(2, 32000, seed=51))
    logits = R.forward(W, mel, cfg)
    np.testing.assert_allclose(logits, g["logits"], atol=5e-4, rtol=1e-4)
    np.testing.assert_array_equal(logits.argmax(-1), g["tokens"])


@pytest.mark.slow
def test_forward_10s_tokens(default_weights):
    g = golden("fwd_b2_10s.npz")
    mel = R.compute_mel_spectrogram(S.make_audio(2, 160000, seed=1234))
    logits = R.forward(default_weights, mel, dict(S.DEFAULT_CONFIG))
    np.testing.assert_array_equal(logits.argmax(-1), g["tokens"])
    np.testing.assert_allclose(logits[:, g["frames"]], g["logits_sub"], atol=5e-4, rtol=1e-4)
    assert R.ctc_greedy_decode(logits) == golden_json("decode_fwd.json")["results"]["b2_10s"]


def test_decode_cases():
    d = golden_json("decode.json")
    for name, c in d["cases"].items():
        lg = np.array(c["logits"], np.float32)
        assert R.ctc_greedy_decode(lg) == c["greedy"], name
        assert R.ctc_greedy_decode(lg, collapse_repeated=False) == c["greedy_nocollapse"], name
        ts = R.ctc_greedy_decode_with_timestamps(lg)
        assert [[t, [list(x) for x in s]] for t, s in ts] == c["timestamps"], name


def _statedim_meta():
    return json.loads(str(golden("fwd_statedims.npz")["meta"]))


@pytest.mark.parametrize("name", ["sd8", "sd48", "sd128"])
def test_forward_state_dims(name):
    """Any ssm_state_dim / global_ssm_state_dim (model.py:23-68): the oracle
    at N = 8, 48, 128 vs the reference (tests/golden/fwd_statedims.npz)."""
    g = golden("fwd_statedims.npz")
    cfg = dict(S.DEFAULT_CONFIG, **_statedim_meta()["configs"][name])
    W = S.make_weights(cfg, seed=5)
    logits = R.forward(W, R.compute_mel_spectrogram(S.make_audio(2, 32000, seed=52)), cfg)
    np.testing.assert_allclose(logits[:, ::4], g[name + "__logits_sub4"], atol=5e-4, rtol=1e-4)
    np.testing.assert_array_equal(logits.argmax(-1), g[name + "__tokens"])


@pytest.mark.parametrize("case", [tuple(c) for c in _statedim_meta()["scans"]], ids=lambda c: c[0])
def test_scan_state_dims(case):
    name, seed, B, L, Di, N = case
    g = golden("fwd_statedims.npz")
    x, dt, Bm, Cm, A_log, D = scan_inputs(seed, B, L, Di, N)
    A = (-np.exp(A_log)).astype(np.float32)
    np.testing.assert_allclose(R.parallel_scan(x, dt, A, Bm, Cm, D), g[name + "__parallel"], atol=5e-5, rtol=5e-5)
    np.testing.assert_allclose(R.sequential_scan(x, dt, A, Bm, Cm, D), g[name + "__sequential"], atol=5e-5, rtol=5e-5)


def test_headline_logits_fixture_is_consistent():
    """fwd_headline_logits.npz (the reference's logits at C2 / C4) agrees with
    the tokens-only golden of the same reference runs: the argmax of every stored frame is the
    stored token, every near-tie row's margin is below the recorded threshold, and each near-tie
    frame is one of fwd_fullbatch.npz's frames with that margin."""
    g = golden("fwd_headline_logits.npz")
    full = golden("fwd_fullbatch.npz")
    thr = json.loads(str(g["meta"]))["tie_margin"]
    for cfg in ("c2", "c4"):
        every = int(g[cfg + "_every"])
        sub = g[cfg + "_logits_sub"]
        np.testing.assert_array_equal(sub.argmax(-1), full[cfg + "_tokens"][:, ::every].astype(np.int64))
        ties, rows = g[cfg + "_tie_idx"], g[cfg + "_tie_logits"]
        s = np.sort(rows, -1)
        assert ((s[:, -1] - s[:, -2]) < thr).all()
        np.testing.assert_array_equal(rows.argmax(-1), full[cfg + "_tokens"][ties[:, 0], ties[:, 1]])
        np.testing.assert_allclose(s[:, -1] - s[:, -2], full[cfg + "_margin"][ties[:, 0], ties[:, 1]], rtol=0, atol=1e-9)
        assert len(ties) == int((full[cfg + "_margin"] < thr).sum())
