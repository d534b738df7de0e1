"""WER / CER scoring on the device: vasr_edit_counts_i32 against the specification
training.edit_counts_host, exact equality of the (P, 3) integers everywhere.  Ids come from an alphabet
of 3, so cost ties are everywhere; seeds are fixed.  The pure-Python oracle costs about half a
microsecond per cell, which sets the sizes."""

import importlib.util
import os
import random

import numpy as np
import pytest
import torch

import score_cases as sc
from conftest import PKG_ROOT, golden_json
from velocity_asr import synthetic as S
from velocity_asr import training as T

pytestmark = pytest.mark.gpu


def _geometry():
    from velocity_asr import _lib
    lib = _lib.lib()
    return lib.vasr_edit_wave_cols(), lib.vasr_edit_tile_cols()


def _spec(pairs):
    return [list(T.edit_counts_host(h, r)) for h, r in pairs]


def _device(pairs, fill=-1, extra_ld=0, width_h=None, width_r=None):
    """One batched call on `pairs`; the matrices are views of wider ones when extra_ld > 0."""
    from velocity_asr import ops
    wh = max([len(h) for h, _ in pairs] + [0]) if width_h is None else width_h
    wr = max([len(r) for _, r in pairs] + [0]) if width_r is None else width_r
    H, hl = sc.pad_batch([h for h, _ in pairs], wh, max(wh, 1) + extra_ld, fill)
    R, rl = sc.pad_batch([r for _, r in pairs], wr, max(wr, 1) + extra_ld, fill)
    dev = lambda a: torch.from_numpy(a).cuda()  # noqa: E731
    got = ops.edit_counts(dev(H)[:, :wh], dev(R)[:, :wr], dev(hl), dev(rl))
    assert got.dtype == torch.int32 and got.shape == (len(pairs), 3) and got.is_cuda
    return got.cpu().tolist()


@pytest.mark.parametrize("long_side", ["ref", "hyp"])
def test_boundary_lengths_in_one_batched_call(long_side):
    """Strip, wave, one-wave-limit and tile boundaries (and three passes) against 0, 1, 5 and 70 items
    on the other side; both orientations."""
    w, t = _geometry()
    pairs = sc.boundary_pairs(w, t)
    assert {len(a) for a, _ in pairs} >= {0, 1, 2, 63, 64, 65, w - 1, w, w + 1, t - 1, t, t + 1, 2 * t + 3}
    if long_side == "ref":
        pairs = [(b, a) for a, b in pairs]
    assert _device(pairs) == _spec(pairs)


def test_tall_and_wide_pair_fills_and_drains_several_waves():
    rng = random.Random(3)
    ref = sc.seq(rng, 1300)
    hyp = sc.edited(rng, ref, 0.3) + sc.seq(rng, 200)
    hyp = hyp[:1500]
    assert len(hyp) > 1300
    pairs = [(hyp, ref)]
    assert _device(pairs) == _spec(pairs)


@pytest.mark.parametrize("n", [7, "w+1"])
def test_structured_contents(n):
    n = _geometry()[0] + 1 if n == "w+1" else n
    pairs = sc.content_pairs(n)
    want = _spec(pairs)
    assert want[0] == [0, 0, 0]
    assert want[1][0] == n and want[1][1] == 2 and want[2][0] == n and want[2][2] == 2   # disjoint: all substitutions
    assert want[4] == [0, 3, 0] and want[5] == [0, 0, 3]
    assert _device(pairs) == want


def test_padding_content_and_leading_dimension_do_not_matter():
    pairs = sc.random_pairs(300, 200, seed=9)
    want = _spec(pairs)
    a = _device(pairs, fill=1, extra_ld=37)   # a symbol of the alphabet
    b = _device(pairs, fill=-1, extra_ld=37)
    assert a == b == want
    # matrices narrower than some stored lengths: the lengths clamp
    cut = [(h[:150], r[:120]) for h, r in pairs]
    assert any(len(h) > 150 for h, _ in pairs) and any(len(r) > 120 for _, r in pairs)
    assert _device(pairs, fill=1, extra_ld=5, width_h=150, width_r=120) == _spec(cut)


def test_mixed_regimes_in_one_call_and_run_to_run():
    w, t = _geometry()
    rng = random.Random(21)
    pairs = sc.random_pairs(200, 90, seed=22)
    wide = [(sc.seq(rng, 40), sc.seq(rng, t + 9)), (sc.seq(rng, 33), sc.seq(rng, t + w + 1))]
    pairs = pairs[:50] + wide[:1] + pairs[50:] + wide[1:]
    first = _device(pairs)
    assert first == _spec(pairs)
    assert _device(pairs) == first


def test_more_pairs_than_one_launch_takes():
    """65535 + 7 pairs of 0..4 items: ops.edit_counts splits them into two launches."""
    pairs = sc.random_pairs(65535 + 7, 4, seed=29)
    got = _device(pairs, fill=2)
    want = _spec(pairs)
    assert got[:10] == want[:10] and got[65530:] == want[65530:]
    assert got == want


def test_non_default_stream_and_poisoned_workspace():
    """The C entry point on a side stream with a workspace full of NaN bit patterns: the boundary
    column is written before it is read."""
    from velocity_asr import _lib
    lib = _lib.lib()
    w, t = _geometry()
    rng = random.Random(31)
    pairs = [(sc.seq(rng, 50), sc.seq(rng, 2 * t + 5)), (sc.seq(rng, 9), sc.seq(rng, 12)), (sc.seq(rng, 64), sc.seq(rng, t + 1))]
    H, hl = sc.pad_batch([h for h, _ in pairs])
    R, rl = sc.pad_batch([r for _, r in pairs])
    need = lib.vasr_edit_workspace_bytes(len(pairs), H.shape[1], R.shape[1])
    assert need > 0
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        Hd, Rd, hld, rld = (torch.from_numpy(a).cuda() for a in (H, R, hl, rl))
        ws = torch.full((need // 8,), float("nan"), device="cuda", dtype=torch.float64)
        out = torch.full((len(pairs), 3), -7, device="cuda", dtype=torch.int32)
        rc = lib.vasr_edit_counts_i32(Hd.data_ptr(), H.shape[1], hld.data_ptr(), H.shape[1], Rd.data_ptr(), R.shape[1],
                                      rld.data_ptr(), R.shape[1], len(pairs), out.data_ptr(), ws.data_ptr(), need,
                                      stream.cuda_stream)
        assert rc == 0, lib.vasr_last_error()
    stream.synchronize()
    assert out.cpu().tolist() == _spec(pairs)


# --------------------------------------------------------------------------- the public path
@pytest.fixture
def always_on_device(monkeypatch):
    """Score every batch with the kernel, however small."""
    monkeypatch.setattr(T, "MIN_DEVICE_CELLS", 0)


def test_rates_on_the_device_equal_the_host_floats(always_on_device):
    g = golden_json("score.json")
    preds, refs = [e["prediction"] for e in g["pairs"]], [e["reference"] for e in g["pairs"]]
    assert T.compute_wer(preds, refs, device="cuda") == g["corpus"]["wer"] == T.compute_wer(preds, refs)
    assert T.compute_cer(preds, refs, device="cuda") == g["corpus"]["cer"] == T.compute_cer(preds, refs)
    for e in g["pairs"][:8]:
        assert T.compute_wer([e["prediction"]], [e["reference"]], device="cuda") == e["wer"]
        assert T.compute_cer([e["prediction"]], [e["reference"]], device="cuda") == e["cer"]
    pairs = sc.sentence_pairs(50, 60, seed=13)
    preds, refs = [p for p, _ in pairs], [r for _, r in pairs]
    assert T.compute_wer(preds, refs, device=torch.device("cuda", 0)) == T.compute_wer(preds, refs)
    assert T.compute_cer(preds, refs, device="cuda") == T.compute_cer(preds, refs)
    for unit in ("word", "char"):
        assert T.error_counts(preds, refs, unit, device="cuda") == T.error_counts(preds, refs, unit)


def test_token_error_counts_on_device_tensors():
    pairs = sc.random_pairs(40, 120, seed=17, alphabet=5)
    H, hl = sc.pad_batch([h for h, _ in pairs], fill=0)
    R, rl = sc.pad_batch([r for _, r in pairs], fill=0)
    got = T.token_error_counts(torch.from_numpy(H).cuda().long(), torch.from_numpy(hl).cuda().long(),
                               torch.from_numpy(R).cuda(), torch.from_numpy(rl).cuda())
    assert got.is_cuda and got.dtype == torch.int32
    assert got.cpu().tolist() == _spec(pairs)


def test_a_pair_over_the_device_limit_is_scored_on_the_host_inside_a_device_batch(monkeypatch):
    calls = []
    from velocity_asr import ops
    real = ops.edit_counts
    monkeypatch.setattr(ops, "edit_counts", lambda *a: calls.append(a[0].shape) or real(*a))
    rng = random.Random(41)
    chars = "abc"
    long_ref = "".join(rng.choice(chars) for _ in range(65540))
    short = ["".join(rng.choice(chars) for _ in range(rng.randint(100, 200))) for _ in range(8)]
    preds = ["abc"] + ["".join(chars[i] for i in sc.edited(rng, [chars.index(c) for c in s], 0.2)) for s in short]
    refs = [long_ref] + short
    got = T.error_counts(preds, refs, "char", device="cuda")
    assert got == T.error_counts(preds, refs, "char")
    assert got[0].ref_length == 65540 and got[0].errors == T._edit_distance("abc", long_ref)
    assert len(calls) == 1 and calls[0][0] == 8          # the eight short pairs went to the kernel in one call
    with pytest.raises(ValueError, match="65535"):
        z = torch.zeros((1, 65536), dtype=torch.int32, device="cuda")
        real(z, z[:, :4], torch.ones(1, dtype=torch.int32, device="cuda"), torch.ones(1, dtype=torch.int32, device="cuda"))


# --------------------------------------------------------------------------- evaluate.py end to end
def test_evaluate_scores_on_the_device(tmp_path, capsys, always_on_device):
    import velocity_asr as v
    from velocity_asr.audio import write_wav
    spec = importlib.util.spec_from_file_location("vasr_script_evaluate_score_gpu", os.path.join(PKG_ROOT, "scripts", "evaluate.py"))
    ev = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ev)
    m = v.VELOCITYASR()
    m.load_state_dict({k: torch.from_numpy(x) for k, x in S.make_weights(None, seed=0).items()})
    m.save_pretrained(str(tmp_path / "model.pt"))
    a = S.make_audio(2, 32000, seed=21)
    clips = [("c0.wav", a[0]), ("c1.wav", a[1]), ("e.wav", S.make_audio(1, 16333, seed=35)[0])]
    for name, x in clips:
        write_wav(str(tmp_path / name), x)
    # what the model says, then references that differ from it in known ways
    dec = v.CTCDecoder(v.create_default_vocabulary(m.config.vocab_size))
    from velocity_asr.transcription import transcribe_files
    texts = [r["transcription"] for r in transcribe_files(m.cuda().eval(), [tmp_path / n for n, _ in clips], dec, "cuda")]
    refs = [texts[0], "zz " + texts[1] + " q", "one two three"]
    man = tmp_path / "m.tsv"
    man.write_text("".join(f"{tmp_path / n}\t{r}\n" for (n, _), r in zip(clips, refs)), encoding="utf-8")
    out, per = tmp_path / "report.txt", tmp_path / "per.tsv"
    assert ev.main(["--checkpoint", str(tmp_path / "model.pt"), "--test-set", str(man), "--output", str(out),
                    "--error-breakdown", "--per-utterance", str(per)]) == 0
    lines = out.read_text().splitlines()
    wer, cer = T.compute_wer(texts, refs), T.compute_cer(texts, refs)   # host scoring
    assert lines[:4] == [f"Test Set: {man}", "Samples: 3", f"WER: {wer * 100:.2f}%", f"CER: {cer * 100:.2f}%"]
    totals = {}
    for line in lines[4:]:
        name, nums = line.split(" S/D/I/N: ")
        totals[name] = tuple(map(int, nums.split("/")))
    assert set(totals) == {"Word", "Char"}
    assert sum(totals["Word"][:3]) == round(wer * totals["Word"][3])
    assert sum(totals["Char"][:3]) == round(cer * totals["Char"][3])
    rows = [r.split("\t") for r in per.read_text(encoding="utf-8").splitlines()]
    assert [os.path.basename(r[0]) for r in rows] == [n for n, _ in clips]
    assert tuple(sum(int(r[k]) for r in rows) for k in (2, 3, 4, 1)) == totals["Word"]
    host = T.error_counts(texts, refs, "word")
    assert [tuple(map(int, r[1:5])) for r in rows] == [(c.ref_length, c.substitutions, c.deletions, c.insertions) for c in host]
