"""Long-form segmentation, host side: the rule (velocity_asr.audio.plan_segments on host tensors),
its validation, stitch_segments and the argument checks of the three device entry points.  No GPU
needed; every comparison is exact."""

import inspect
import math
import sys

import numpy as np
import pytest
import torch

import longform_cases as lc
from conftest import REPO
from velocity_asr import audio as A
from velocity_asr import transcription as T


def _plan(x, m, M, W):
    return A.plan_segments(torch.from_numpy(np.asarray(x, np.float32)), max_samples=M, min_samples=m, window_blocks=W)[0]


def test_worked_example():
    """BLK 320, W 2, m 640, M 1600; 2560 samples of 0.5 with 960..1279 zeroed: energies 80 except
    block 3, candidates 2..5 score 160, 80, 80, 160, the tie goes to c = 3: one cut at 960."""
    x = np.full(2560, 0.5, np.float32)
    x[960:1280] = 0.0
    E = A.block_energy_host(x)
    assert E.dtype == np.float64 and E.tolist() == [80.0, 80.0, 80.0, 0.0, 80.0, 80.0, 80.0, 80.0]
    assert lc.energy_ref(x) == E.tolist()
    scores = [E[c - 1] + E[c] for c in range(2, 6)]
    assert scores == [160.0, 80.0, 80.0, 160.0]
    cuts = _plan(x, 640, 1600, 2)
    assert cuts == [960] == A.plan_segments_host(x, 1600, 640, 2) == lc.plan_ref(E.tolist(), 2560, 640, 1600, 2)
    assert lc.segments_of(2560, cuts) == [(0, 960), (960, 1600)]
    assert A.segment_table([2560], [cuts]) == [(0, 0, 960), (0, 960, 1600)]


def test_defaults_are_30_10_and_a_fifth_of_a_second():
    p = inspect.signature(A.plan_segments).parameters
    assert (p["max_samples"].default, p["min_samples"].default, p["window_blocks"].default) == (480000, 160000, 10)
    assert all(p[k].kind is inspect.Parameter.KEYWORD_ONLY for k in ("max_samples", "min_samples", "window_blocks"))
    assert A.SEGMENT_BLOCK == 320 == 2 * A.HOP_LENGTH
    assert A.check_segment_params(480000, 160000, 10, max_rows=5000) == (1500, 500, 10)


def test_properties_over_random_parameters():
    """300 seeded (n, m, M, W) draws on noise with zeroed stretches: the partition, cuts on multiples
    of 320, the segment bounds (the last one included), the cut-count bound; the numpy rule equals
    the scalar restatement, energies bit for bit."""
    rng = np.random.default_rng(2024)
    made_cuts = 0
    for t in range(300):
        n, m, M, W = lc.draw_params(rng)
        x = lc.signal(n, seed=t)
        cuts = _plan(x, m, M, W)
        lc.check_plan(cuts, n, m, M)
        made_cuts += bool(cuts)
        if t % 6 == 0:  # the scalar restatement is slow: every sixth draw
            E = A.block_energy_host(x)
            ref = lc.energy_ref(x)
            assert np.array_equal(E.view(np.uint64), np.asarray(ref, np.float64).view(np.uint64))
            assert cuts == lc.plan_ref(ref, n, m, M, W), (n, m, M, W)
    assert made_cuts > 200


@pytest.mark.parametrize("m,M,W", [(640, 1600, 2), (3840, 8000, 4), (4000, 12000, 4), (6400, 16000, 10)])
def test_edges_of_the_loop(m, M, W):
    """n <= M: no cut.  n = M + 1: exactly one.  The cut of n = M + 1 leaves both parts in [m, M]."""
    for n in (1, 319, m, M - 1, M):
        assert _plan(lc.signal(n, seed=n), m, M, W) == []
    x = lc.signal(M + 1, seed=M)
    cuts = _plan(x, m, M, W)
    assert len(cuts) == 1
    lc.check_plan(cuts, M + 1, m, M)
    many = _plan(lc.signal(40 * M + 123, seed=3), m, M, W)
    lc.check_plan(many, 40 * M + 123, m, M)
    assert len(many) >= 40


def test_all_zero_recording_takes_the_lowest_candidate_every_time():
    m, M, W = 3840, 8000, 4
    n = 5 * M + 77
    cuts = _plan(np.zeros(n, np.float32), m, M, W)
    mB = -(-m // 320)
    # every score ties at 0: each cut is p + mB, until the rest fits
    want, p = [], 0
    while n - p * 320 > M:
        p += mB
        want.append(p * 320)
    assert cuts == want


def test_a_nan_block_never_wins_over_a_finite_one():
    m, M, W = 640, 1600, 2
    x = np.full(2560, 0.5, np.float32)
    x[960:1280] = np.nan  # block 3: candidates 3 and 4 score NaN -> +inf
    # c = 2 (160 ties with c = 5, the lowest wins); then from p = 2 candidates 4..6 score inf, 160, 160
    assert _plan(x, m, M, W) == [640, 1600]
    # every candidate NaN: all +inf, ties to the lowest candidate (2, then 2 + 2)
    assert _plan(np.full(2560, np.nan, np.float32), m, M, W) == [640, 1280]
    E = [80.0, 80.0, math.nan, 1e9, 80.0, 80.0, 80.0, 80.0]
    assert A.plan_cuts_host(np.asarray(E), 2560, 1600, 640, 2) == lc.plan_ref(E, 2560, 640, 1600, 2) == [1600]


@pytest.mark.parametrize("kw,word", [
    (dict(max_samples=1600, min_samples=640, window_blocks=3), "even"),
    (dict(max_samples=1600, min_samples=640, window_blocks=0), "even"),
    (dict(max_samples=3200, min_samples=640, window_blocks=6), "half the window"),
    (dict(max_samples=1279, min_samples=640, window_blocks=2), "twice"),
    # 8000 samples hold 25 blocks, 4000 need 13: one block short of twice (3840 is the most M = 8000 takes)
    (dict(max_samples=8000, min_samples=4000, window_blocks=4), "twice"),
    (dict(max_samples=1600, min_samples=200, window_blocks=2), "reflect padding"),
])
def test_validation_raises_value_error_with_the_reason(kw, word):
    x = torch.zeros(4000)
    with pytest.raises(ValueError, match=word):
        A.plan_segments(x, **kw)
    with pytest.raises(ValueError, match=word):
        A.check_segment_params(kw["max_samples"], kw["min_samples"], kw["window_blocks"])


def test_validation_against_the_models_positional_table():
    # 5000 rows: M // 160 + 1 frames, (frames + 1) // 2 rows
    assert A.check_segment_params(1599680, 160000, 10, max_rows=5000)[0] == 4999
    with pytest.raises(ValueError, match="positional table"):
        A.check_segment_params(1600000, 160000, 10, max_rows=5000)
    with pytest.raises(ValueError, match="lengths"):
        A.plan_segments(torch.zeros(2, 4000), [4000, 4001], max_samples=1600, min_samples=640, window_blocks=2)
    with pytest.raises(ValueError, match="partition"):
        A.segment_table([2560], [[960, 960]])


VOCAB = ["<blank>", "<unk>", "<pad>", "▁", "a", "b", "c", "d"]


def test_stitch_shifts_spans_and_joins_words_across_a_cut():
    """Two segments and an empty one between them.  The second decoded segment starts with "c",
    no separator: it continues the word the first one left open."""
    s0 = dict(tokens=[4, 5, 3, 4], start=[0, 2, 5, 7], end=[2, 4, 6, 9], logp_sum=[-0.5, -0.25, -1.0, -0.125],
              logp_min=[-0.5, -0.25, -0.75, -0.125], run_lengths=[2, 2, 1, 2], path_logp=-3.0)
    s1 = dict(tokens=[], start=[], end=[], logp_sum=[], logp_min=[], run_lengths=[], path_logp=-0.1)
    s2 = dict(tokens=[6, 3, 7], start=[1, 3, 4], end=[3, 4, 8], logp_sum=[-2.0, -0.5, -0.75],
              logp_min=[-1.5, -0.5, -0.5], run_lengths=[2, 1, 4], path_logp=-4.2)
    starts = [0, 10 * 320, 25 * 320]
    out = T.stitch_segments([s0, s1, s2], starts)
    assert out["tokens"] == [4, 5, 3, 4, 6, 3, 7]
    assert out["start"] == [0, 2, 5, 7, 26, 28, 29] and out["end"] == [2, 4, 6, 9, 28, 29, 33]
    assert all(isinstance(v, int) for v in out["start"] + out["end"])
    assert out["logp_sum"] == s0["logp_sum"] + s2["logp_sum"] and out["logp_min"] == s0["logp_min"] + s2["logp_min"]
    assert out["run_lengths"] == [2, 2, 1, 2, 2, 1, 4]
    assert out["path_logp"] == (0.0 + -3.0 + -0.1) + -4.2 and isinstance(out["path_logp"], float)
    spans = list(zip(out["start"], out["end"]))
    words = T.group_words(out["tokens"], spans, VOCAB)
    assert [w["word"] for w in words] == ["ab", "ac", "d"]
    # "ac" runs from row 7 of segment 0 to the separator that closes it in segment 2 (row 25 + 4)
    assert words[1]["start"] == T.frames_to_seconds(7) and words[1]["end"] == T.frames_to_seconds(29)
    assert words[2] == {"word": "d", "start": T.frames_to_seconds(29), "end": T.frames_to_seconds(33)}


def test_stitch_score_is_the_float64_sum_in_segment_order():
    vals = [float(np.float32(v)) for v in (-1234.5678, -1e-3, -77.125, -3.3e-5)]
    segs = [dict(tokens=[], path_logp=v) for v in vals]
    acc = np.float64(0.0)
    for v in vals:
        acc = acc + np.float64(v)
    assert T.stitch_segments(segs, [0, 320, 640, 960])["path_logp"] == float(acc)
    assert T.stitch_segments(segs, [0, 320, 640, 960])["path_logp"] != float(np.float32(sum(np.float32(v) for v in vals)))
    # tokens alone (beam search, greedy without time spans)
    out = T.stitch_segments([dict(tokens=[4, 5]), dict(tokens=[]), dict(tokens=[6])], [0, 3200, 6400])
    assert out == {"tokens": [4, 5, 6]}
    with pytest.raises(ValueError, match="multiple of 320"):
        T.stitch_segments([dict(tokens=[4])], [100])
    with pytest.raises(ValueError, match="segments"):
        T.stitch_segments([dict(tokens=[4])], [0, 320])
    with pytest.raises(ValueError, match="values of 'start'"):
        T.stitch_segments([dict(tokens=[4], start=[], end=[1])], [0])


def test_render_of_one_segment_is_the_unsegmented_result():
    """_render of a raw decoding builds what _decode_batch builds for a clip."""
    from velocity_asr.decode import CTCDecoder, token_confidences
    dec = CTCDecoder(VOCAB)
    r = dict(tokens=[4, 5, 3, 6], start=[0, 2, 5, 7], end=[2, 4, 6, 9], logp_sum=[-0.5, -0.25, -1.0, -0.125],
             logp_min=[-0.5, -0.25, -0.75, -0.125], run_lengths=[2, 2, 1, 2], path_logp=-3.0)
    spans = list(zip(r["start"], r["end"]))
    assert T._render(dict(tokens=r["tokens"]), dec, False, False) == ("ab c", None)
    words = T.group_words(r["tokens"], spans, VOCAB)
    assert T._render(r, dec, True, False) == ("ab c", words)
    conf = token_confidences(r["logp_sum"], r["logp_min"], r["run_lengths"], "mean")
    assert T._render(r, dec, True, True) == ("ab c", T.group_words(r["tokens"], spans, VOCAB, conf), -3.0)


def _L():
    from velocity_asr import _lib
    return _lib


def test_abi_symbols_and_max_cuts():
    L = _L()
    lib = L.lib()
    assert lib.vasr_version() == L.ABI_VERSION
    for name in ("vasr_block_energy_f64", "vasr_segment_plan", "vasr_segment_gather_f32", "vasr_segment_max_cuts",
                 "vasr_segment_tile_blocks", "vasr_segment_block"):
        assert name in L._SIGNATURES and name in L.header_functions()
    assert lib.vasr_segment_block() == 320 and lib.vasr_segment_tile_blocks() > 0
    assert lib.vasr_segment_max_cuts(2560, 640) == 4       # nB 8, mB 2
    assert lib.vasr_segment_max_cuts(2559, 640) == 3       # full blocks only
    assert lib.vasr_segment_max_cuts(2560, 641) == 2       # mB = ceil(m / 320)
    assert lib.vasr_segment_max_cuts(8 * 57600000, 160000) == 8 * 360   # 64-bit sample counts
    assert lib.vasr_segment_max_cuts(-1, 640) == -1 and lib.vasr_segment_max_cuts(100, 0) == -1
    rng = np.random.default_rng(7)
    for _ in range(50):  # the bound holds for every plan
        n, m, M, W = lc.draw_params(rng)
        assert len(_plan(lc.signal(n, seed=n), m, M, W)) <= lib.vasr_segment_max_cuts(n, m)


def test_entry_points_refuse_bad_arguments_before_any_device_call():
    lib = _L().lib()
    fake = 256  # aligned non-null pointer values: the checks return before any dereference

    def energy(x=fake, ld_x=3200, B=1, S=3200, E=fake, ld_e=10):
        return lib.vasr_block_energy_f64(x, ld_x, B, S, None, E, ld_e, None)

    assert energy(x=None) == -1 and b"null" in lib.vasr_last_error()
    assert energy(E=None) == -1
    assert energy(B=0) == -1 and energy(S=0) == -1
    assert energy(B=65536) == -1 and b"65535" in lib.vasr_last_error()
    assert energy(ld_x=3199) == -1 and b"ld_x" in lib.vasr_last_error()
    assert energy(ld_e=9) == -1 and b"ld_e" in lib.vasr_last_error()
    assert energy(S=319, ld_x=319, ld_e=0) == 0  # no full block: nothing to launch

    def plan(E=fake, ld_e=10, B=1, S=3200, M=1600, m=640, W=2, cuts=fake, ld_cuts=5, max_cuts=5, n_cuts=fake):
        return lib.vasr_segment_plan(E, ld_e, B, S, None, M, m, W, cuts, ld_cuts, max_cuts, n_cuts, None)

    assert plan(E=None) == -1 and b"null" in lib.vasr_last_error()
    assert plan(cuts=None) == -1 and plan(n_cuts=None) == -1
    assert plan(B=65536) == -1 and b"65535" in lib.vasr_last_error()
    assert plan(W=3) == -1 and b"even" in lib.vasr_last_error()
    assert plan(W=0) == -1 and b"even" in lib.vasr_last_error()
    assert plan(W=6) == -1 and b"half the window" in lib.vasr_last_error()
    assert plan(M=1279) == -1 and b"twice" in lib.vasr_last_error()
    assert plan(m=0) == -1
    assert plan(ld_e=9) == -1 and b"ld_e" in lib.vasr_last_error()
    # 3200 samples, mB 2: up to 5 cuts; a table of 4 columns is refused, not overrun
    assert plan(max_cuts=4, ld_cuts=4) == -1 and b"too narrow" in lib.vasr_last_error()
    assert plan(ld_cuts=4) == -1

    def gather(x=fake, ld_x=3200, B=1, S=3200, table=fake, n_seg=2, y=fake, ld_y=1600, S_seg=1600):
        return lib.vasr_segment_gather_f32(x, ld_x, B, S, table, n_seg, y, ld_y, S_seg, None)

    assert gather(x=None) == -1 and b"null" in lib.vasr_last_error()
    assert gather(table=None) == -1 and gather(y=None) == -1
    assert gather(n_seg=0) == -1 and gather(S_seg=0) == -1
    assert gather(B=65536) == -1 and gather(n_seg=65536) == -1
    assert gather(ld_x=3199) == -1 and b"ld_x" in lib.vasr_last_error()
    assert gather(ld_y=1599) == -1 and b"ld_y" in lib.vasr_last_error()


def test_ops_wrappers_check_before_the_library():
    from velocity_asr import ops
    with pytest.raises(RuntimeError, match="HIP"):
        ops.block_energy(torch.zeros(1, 640))
    with pytest.raises(RuntimeError, match="HIP"):
        ops.segment_gather(torch.zeros(1, 640), torch.zeros(1, 3, dtype=torch.int64), 320)
    with pytest.raises(RuntimeError, match="HIP"):
        ops.segment_plan(torch.zeros(1, 2, dtype=torch.float64), 640, 1600, 640)
    with pytest.raises(RuntimeError, match="HIP"):
        A.segment_on_device(torch.zeros(1, 640), [640], [[]])


def test_transcribe_files_and_scripts_take_the_new_arguments():
    p = inspect.signature(T.transcribe_files).parameters
    assert p["segment_seconds"].default is None and p["min_segment_seconds"].default is None
    sys.path.insert(0, f"{REPO}/velocity-asr_amd/scripts")
    import evaluate
    import transcribe
    a = evaluate.parse_args(["--checkpoint", "m.pt", "--audio-dir", "d"])
    assert a.segment_seconds is None and a.min_segment_seconds is None
    a = evaluate.parse_args(["--checkpoint", "m.pt", "--audio-dir", "d", "--segment-seconds", "30",
                             "--min-segment-seconds", "8.5"])
    assert (a.segment_seconds, a.min_segment_seconds) == (30.0, 8.5)
    src = inspect.getsource(transcribe)
    assert "--segment-seconds" in src and "--min-segment-seconds" in src
    # parameters are checked before any file is read
    with pytest.raises(ValueError, match="twice"):
        T.transcribe_files(None, [], None, "cpu", segment_seconds=0.3, min_segment_seconds=0.2)
    with pytest.raises(ValueError, match="needs segment_seconds"):
        T.transcribe_files(None, [], None, "cpu", min_segment_seconds=1.0)
