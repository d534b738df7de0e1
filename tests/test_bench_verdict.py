"""bench.py's validity checks on the host (no GPU): the reference-token check of the timed graphs
(golden_check / golden_summary) and the exit path (run_verdict) on a forced mismatch, and the
schedule description.  VERDICT r04 weak 8: a failed reference check must fail the run."""

import argparse
import json
import os

import numpy as np
import torch

import bench

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _args(**kw):
    a = argparse.Namespace(bf16=False, int8=False, seconds=10.0, batch=32)
    a.__dict__.update(kw)
    return a


def _c2_reference():
    full = json.loads(str(np.load(os.path.join(GOLD, "fwd_fullbatch.npz"), allow_pickle=False)["greedy"]))
    return full["c2"]


def _as_tensors(lists):
    L = max(1, max(len(x) for x in lists))
    toks = torch.zeros((len(lists), L), dtype=torch.int32)
    for b, x in enumerate(lists):
        toks[b, :len(x)] = torch.tensor(x, dtype=torch.int32)
    lens = torch.tensor([len(x) for x in lists], dtype=torch.int32)
    return toks, lens


def test_golden_check_passes_reference_tokens():
    ref = _c2_reference()
    toks, lens = _as_tensors(ref)
    c = bench.golden_check(toks, lens, _args(), rank=0)
    g = bench.golden_summary(c, _args())
    assert g["clips"] == 32 and g["clips_identical"] == 32 and g["all_ranks_pass"]
    assert bench.run_verdict(True, g, g, g) == (0, [])


def test_forced_mismatch_fails_the_run():
    ref = [list(x) for x in _c2_reference()]
    ref[5] = ref[5][:-1] + [ref[5][-1] % 999 + 1]  # one token of one clip changed
    toks, lens = _as_tensors(ref)
    g = bench.golden_summary(bench.golden_check(toks, lens, _args(), rank=0), _args())
    assert g["clips_identical"] == 31 and not g["all_ranks_pass"]
    ok = bench.golden_summary(bench.golden_check(*_as_tensors(_c2_reference()), _args(), rank=0), _args())
    # any one failing check fails the run: timed, warm-up, or eager
    for combo in ((g, ok, ok), (ok, g, ok), (ok, ok, g)):
        rc, why = bench.run_verdict(True, *combo)
        assert rc == 1 and len(why) == 1 and "all_ranks_pass is false" in why[0]
    rc, why = bench.run_verdict(False, ok, ok, ok)
    assert rc == 1 and "graph_tokens_match_eager" in why[0]
    # no golden for this workload (None) is not a failure
    assert bench.run_verdict(True, None, None, None) == (0, [])


def test_dump_outputs_writes_float32_arrays(tmp_path):
    toks, lens = _as_tensors([[3, 7, 7], [], [999]])
    toks[1, :] = 55  # past a clip's length: no result, written as -1
    out = tmp_path / "dump"
    bench.dump_outputs(str(out), toks, lens, rank=0, world=1)
    assert sorted(os.listdir(out)) == ["lengths.npy", "tokens.npy"]
    t, n = np.load(out / "tokens.npy"), np.load(out / "lengths.npy")
    assert t.dtype == np.float32 and n.dtype == np.float32
    assert t.tolist() == [[3, 7, 7], [-1, -1, -1], [999, -1, -1]] and n.tolist() == [3, 0, 1]
    bench.dump_outputs(str(out), toks, lens, rank=1, world=2)
    assert (out / "tokens_rank1.npy").exists() and (out / "lengths_rank1.npy").exists()


def test_plain_run_is_the_default():
    a = bench.parse_args(["--gpus", "1", "--steps", "7", "--warmup", "2"])
    assert a.full is False and a.dump_outputs is None and a.steps == 7 and a.warmup == 2
    a = bench.parse_args(["--full", "--dump-outputs", "d"])
    assert a.full is True and a.dump_outputs == "d"
    step_ms = [2.0] * 7 + [dict(host_step_ms=[0.04] * 7, issue_ms=0.3)]
    line = bench.headline(bench.parse_args(["--steps", "7"]), 1, False, 32, 160000, 1, None, 0.014, step_ms)
    assert line["steps"] == 7 and line["ms_per_step"] == 2.0 and line["full"] is False
    assert line["value"] == round(32 * 10.0 * 7 / 0.014, 2) and line["higher_is_better"] is True
    assert line["unit"] == "audio-sec/sec (RTFx)" and line["dtype"] == "f32" and line["metric"] == bench.METRIC
    for k in ("roofline", "cpu_baseline", "with_scatter", "tokens_vs_reference", "machine"):
        assert k not in line


def test_schedule_how_reflects_candidates():
    assert "single candidate" in bench.schedule_how({}, 1)
    h = bench.schedule_how({1: 2.1, 2: 2.2}, 1)
    assert "2 schedules" in h and "own audio" in h
    assert "max over ranks" in bench.schedule_how({1: 2.1, 2: 2.2}, 8)
