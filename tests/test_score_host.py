"""WER / CER scoring, host side: the specification edit_counts_host, the public API around it, the
reference's recorded values, the argument checks of the device entry point and evaluate.py's new
options with the transcription stubbed out.  No GPU needed; every comparison is exact."""

import importlib.util
import inspect
import os
import random

import pytest
import torch

import score_cases as sc
from conftest import PKG_ROOT, golden_json
from velocity_asr import training as T


def _L():
    from velocity_asr import _lib
    return _lib


# --------------------------------------------------------------------------- the specification
@pytest.mark.parametrize("hyp,ref,want", [
    ("a b c", "a x c", (1, 0, 0)),
    ("a c", "a b c", (0, 1, 0)),
    ("a b b c", "a b c", (0, 0, 1)),
])
def test_hand_cases_one_edit_each(hyp, ref, want):
    assert T.edit_counts_host(hyp.split(), ref.split()) == want


def test_pinned_tie_and_empty_sides():
    assert T.edit_counts_host("ab", "ba") == (2, 0, 0)  # two substitutions, not an insertion and a deletion
    assert T.edit_counts_host("", "") == (0, 0, 0)
    assert T.edit_counts_host("", "abc") == (0, 3, 0)
    assert T.edit_counts_host("abcd", "") == (0, 0, 4)
    assert T.edit_counts_host([], ("x",)) == (0, 1, 0)


def test_counts_sum_to_the_distance_and_hits_agree():
    pairs = sc.random_pairs(300, 40, seed=1)
    assert any(not h for h, _ in pairs) and any(len(r) == 40 for _, r in pairs)
    for hyp, ref in pairs:
        s, d, i = T.edit_counts_host(hyp, ref)
        assert min(s, d, i) >= 0
        assert s + d + i == T._edit_distance(hyp, ref)
        assert len(ref) - s - d == len(hyp) - s - i >= 0


# --------------------------------------------------------------------------- the public API
MIXED = (["The  CAT sat", "a  B", "", "x y z", "Über   naïve 𝄞"], ["the cat  SAT on", "a b c", "one", "", "über naive 𝄞 𝄞"])


def test_error_counts_totals_reproduce_the_rates():
    preds, refs = MIXED
    for unit, rate in (("word", T.compute_wer), ("char", T.compute_cer)):
        cs = T.error_counts(preds, refs, unit)
        assert len(cs) == len(preds) and all(isinstance(c, T.ErrorCounts) for c in cs)
        assert sum(c.errors for c in cs) / sum(c.ref_length for c in cs) == rate(preds, refs) == T.error_rate(cs)
        for c, p, r in zip(cs, preds, refs):
            items = (lambda s: s.lower().split()) if unit == "word" else (lambda s: list(s.lower()))
            assert (c.hyp_length, c.ref_length) == (len(items(p)), len(items(r)))
            assert c.hits == c.ref_length - c.substitutions - c.deletions == c.hyp_length - c.substitutions - c.insertions
            assert c.errors == T._edit_distance(items(p), items(r))
    with pytest.raises(ValueError, match="unit"):
        T.error_counts(preds, refs, "phone")


def test_rate_of_an_empty_reference_is_zero():
    c = T.error_counts(["some words"], [""])[0]
    assert (c.substitutions, c.deletions, c.insertions, c.ref_length, c.hyp_length) == (0, 0, 2, 0, 2)
    assert c.rate == 0.0 and c.errors == 2 and c.hits == 0
    assert T.error_rate([c]) == 0.0 and T.error_rate([]) == 0.0


def test_default_path_of_the_rates_is_unchanged():
    for f in (T.compute_wer, T.compute_cer):
        p = list(inspect.signature(f).parameters.values())
        assert [q.name for q in p] == ["predictions", "references", "device"] and p[2].default is None
    assert T.compute_wer(["a b c d"], ["a x c"]) == 2 / 3
    assert T.compute_cer(["abc"], ["abd"]) == 1 / 3
    assert T.compute_wer([], []) == 0.0 and T.compute_cer(["x"], [""]) == 0.0
    preds, refs = MIXED
    # a non-HIP device scores on the host
    assert T.compute_wer(preds, refs, device="cpu") == T.compute_wer(preds, refs)
    assert T.compute_cer(preds, refs, device=torch.device("cpu")) == T.compute_cer(preds, refs)


def test_reference_recorded_values():
    g = golden_json("score.json")
    assert len(g["pairs"]) >= 30
    assert [(e["prediction"], e["reference"]) for e in g["pairs"]] == sc.GOLDEN_PAIRS
    for e in g["pairs"]:
        assert T.compute_wer([e["prediction"]], [e["reference"]]) == e["wer"], e
        assert T.compute_cer([e["prediction"]], [e["reference"]]) == e["cer"], e
        assert T.error_counts([e["prediction"]], [e["reference"]], "word")[0].rate == e["wer"]
    preds, refs = [e["prediction"] for e in g["pairs"]], [e["reference"] for e in g["pairs"]]
    assert T.compute_wer(preds, refs) == g["corpus"]["wer"] and T.compute_cer(preds, refs) == g["corpus"]["cer"]


# --------------------------------------------------------------------------- the C ABI
NAMES = ("vasr_edit_counts_i32", "vasr_edit_workspace_bytes", "vasr_edit_wave_cols", "vasr_edit_tile_cols")


def test_abi_symbols_and_geometry():
    L = _L()
    lib = L.lib()
    assert lib.vasr_version() == L.ABI_VERSION == 21
    for name in NAMES:
        assert name in L._SIGNATURES and name in L.header_functions() and hasattr(lib, name)
    w, t = lib.vasr_edit_wave_cols(), lib.vasr_edit_tile_cols()
    assert w > 0 and t >= w and w % 64 == 0
    assert lib.vasr_edit_workspace_bytes(1, 100, t) == 0           # one pass: no boundary column kept
    one = lib.vasr_edit_workspace_bytes(1, 100, t + 1)
    assert one >= 8 * 101                                          # a packed cell per row
    assert lib.vasr_edit_workspace_bytes(1, 65535, 65535) >= 8 * 65536
    assert lib.vasr_edit_workspace_bytes(65535, 65535, 65535) < 2 ** 31   # bounded by the grid, not by P
    for bad in ((0, 1, 1), (-1, 1, 1), (65536, 1, 1), (1, -1, 1), (1, 1, -1), (1, 65536, 1), (1, 1, 65536)):
        assert lib.vasr_edit_workspace_bytes(*bad) == -1, bad


def test_entry_point_refuses_bad_arguments_before_any_device_call():
    lib = _L().lib()
    t = lib.vasr_edit_tile_cols()
    fake = 256  # aligned non-null pointer values: the checks return before any dereference

    def call(hyp=fake, ld_hyp=100, hyp_len=fake, max_hyp=100, ref=fake, ld_ref=100, ref_len=fake, max_ref=100, P=4,
             counts=fake, ws=None, ws_bytes=0):
        return lib.vasr_edit_counts_i32(hyp, ld_hyp, hyp_len, max_hyp, ref, ld_ref, ref_len, max_ref, P, counts, ws,
                                        ws_bytes, None)

    for k in ("hyp", "hyp_len", "ref", "ref_len", "counts"):
        assert call(**{k: None}) == -1 and b"null" in lib.vasr_last_error(), k
    assert call(P=0) == -1 and b"pairs" in lib.vasr_last_error()
    assert call(P=-3) == -1
    assert call(P=65536) == -1 and b"65535" in lib.vasr_last_error()
    assert call(max_hyp=-1) == -1 and call(max_ref=-1) == -1
    assert call(max_hyp=65536, ld_hyp=65536) == -1 and b"65535" in lib.vasr_last_error()
    assert call(max_ref=65536, ld_ref=65536) == -1 and b"65535" in lib.vasr_last_error()
    assert call(ld_hyp=99) == -1 and b"ld_hyp" in lib.vasr_last_error()
    assert call(ld_ref=99) == -1 and b"ld_ref" in lib.vasr_last_error()
    need = lib.vasr_edit_workspace_bytes(4, 100, t + 1)
    assert need > 0
    assert call(max_ref=t + 1, ld_ref=t + 1) == -1 and b"workspace" in lib.vasr_last_error()          # none given
    assert call(max_ref=t + 1, ld_ref=t + 1, ws=fake, ws_bytes=need - 1) == -1 and b"workspace" in lib.vasr_last_error()
    assert call(max_ref=t + 1, ld_ref=t + 1, ws=None, ws_bytes=need) == -1 and b"workspace" in lib.vasr_last_error()


def test_ops_wrapper_checks_before_the_library():
    from velocity_asr import ops
    z = torch.zeros((2, 5), dtype=torch.int32)
    n = torch.zeros((2,), dtype=torch.int32)
    with pytest.raises(RuntimeError, match="HIP"):
        ops.edit_counts(z, z, n, n)
    with pytest.raises(RuntimeError, match="HIP"):
        T.token_error_counts(z, n, z, n)
    assert ops.EDIT_MAX_ITEMS == 65535 == T.MAX_DEVICE_ITEMS and T.MIN_DEVICE_CELLS >= 0


# --------------------------------------------------------------------------- evaluate.py
def _evaluate():
    spec = importlib.util.spec_from_file_location("vasr_script_evaluate_score",
                                                  os.path.join(PKG_ROOT, "scripts", "evaluate.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_evaluate_parses_the_new_options():
    ev = _evaluate()
    a = ev.parse_args(["--checkpoint", "m.pt", "--test-set", "m.tsv"])
    assert a.error_breakdown is False and a.per_utterance is None
    a = ev.parse_args(["--checkpoint", "m.pt", "--test-set", "m.tsv", "--error-breakdown", "--per-utterance", "u.tsv"])
    assert a.error_breakdown is True and a.per_utterance == "u.tsv"


class _FakeModel:
    class config:
        vocab_size = 100

    @classmethod
    def from_pretrained(cls, path):
        return cls()

    def to(self, device):
        return self

    def eval(self):
        return self

    def count_parameters(self):
        return 0


def test_evaluate_report_with_and_without_the_breakdown(tmp_path, monkeypatch, capsys):
    """The model and the transcription are stubbed (they need the device); scoring, the report and
    the two new outputs are the script's own."""
    ev = _evaluate()
    rng = random.Random(4)
    refs = [sc.sentence(rng, n).strip() for n in (6, 1, 9, 4)]  # mixed case, runs of spaces inside
    hyps = [refs[0], "", refs[2].replace("a", "the"), refs[3] + " extra"]
    man = tmp_path / "m.tsv"
    man.write_text("".join(f"f{i}.wav\t{r}\n" for i, r in enumerate(refs)), encoding="utf-8")
    monkeypatch.setattr(ev, "VELOCITYASR", _FakeModel)
    monkeypatch.setattr(ev, "transcribe_files", lambda model, files, *a, **k: [dict(transcription=h) for h in hyps])
    base = ["--checkpoint", "m.pt", "--test-set", str(man), "--device", "cpu"]
    out0, out1, per = tmp_path / "r0.txt", tmp_path / "r1.txt", tmp_path / "u.tsv"
    assert ev.main(base + ["--output", str(out0)]) == 0
    plain_stdout = capsys.readouterr().out
    assert ev.main(base + ["--output", str(out1), "--error-breakdown", "--per-utterance", str(per)]) == 0
    full_stdout = capsys.readouterr().out
    r0, r1 = out0.read_text().splitlines(), out1.read_text().splitlines()
    wer, cer = T.compute_wer(hyps, refs), T.compute_cer(hyps, refs)
    assert r0 == [f"Test Set: {man}", "Samples: 4", f"WER: {wer * 100:.2f}%", f"CER: {cer * 100:.2f}%"]
    assert r1[:4] == r0 and len(r1) == 6                       # the standard lines, byte for byte, then two more
    assert "S/D/I/N" not in plain_stdout and all(line in plain_stdout for line in r0)
    assert all(line in full_stdout for line in r1)
    for line, unit in zip(r1[4:], ("word", "char")):
        name, nums = line.split(" S/D/I/N: ")
        assert name == unit.capitalize()
        s, d, i, n = map(int, nums.split("/"))
        cs = T.error_counts(hyps, refs, unit)
        assert (s, d, i, n) == (sum(c.substitutions for c in cs), sum(c.deletions for c in cs),
                                sum(c.insertions for c in cs), sum(c.ref_length for c in cs))
        assert s + d + i == round((wer if unit == "word" else cer) * n)
    rows = [line.split("\t") for line in per.read_text(encoding="utf-8").splitlines()]
    assert len(rows) == 4 and all(len(r) == 6 for r in rows)
    assert [os.path.basename(r[0]) for r in rows] == [f"f{i}.wav" for i in range(4)]
    ws = T.error_counts(hyps, refs, "word")
    assert [tuple(map(int, r[1:5])) for r in rows] == [(c.ref_length, c.substitutions, c.deletions, c.insertions) for c in ws]
    assert [float(r[5]) for r in rows] == [round(c.rate, 6) for c in ws]
