"""Alignments, host side: the specification edit_alignment_host against an independent statement of the
rule (align_cases.reference_path), the identities of a path, the public API around it, the argument checks
of the device entry point and evaluate.py's --alignments / --confusions with the transcription stubbed out.
No GPU needed; every comparison is exact."""

import importlib.util
import os
import random

import pytest
import torch

import align_cases as ac
import score_cases as sc
from conftest import PKG_ROOT
from velocity_asr import training as T


def _L():
    from velocity_asr import _lib
    return _lib


def _check(hyp, ref):
    path = T.edit_alignment_host(hyp, ref)
    assert path == ac.reference_path(hyp, ref)
    s, d, i = ac.replay(path, hyp, ref)                      # consumes both sides, hits on equal items
    assert (s, d, i) == T.edit_counts_host(hyp, ref)         # the path's counts are the scorer's
    assert s + d + i == T._edit_distance(hyp, ref)
    assert len(path) == len(ref) + i
    return path


# --------------------------------------------------------------------------- the specification
@pytest.mark.parametrize("hyp,ref,want", ac.HAND)
def test_hand_cases_and_empty_sides(hyp, ref, want):
    assert _check(hyp, ref) == want


def test_pinned_examples_of_the_rule():
    assert T.edit_alignment_host("ab", "ba") == [1, 1]
    assert T.edit_alignment_host("a c".split(), "a b c".split()) == [0, 2, 0]
    assert (T.HIT, T.SUBSTITUTION, T.DELETION, T.INSERTION) == (0, 1, 2, 3) == (ac.HIT, ac.SUB, ac.DEL, ac.INS)


def test_random_pairs_equal_the_independent_statement_and_keep_the_identities():
    pairs = sc.random_pairs(300, 40, seed=3)
    assert any(not h for h, _ in pairs) and any(not r for _, r in pairs)
    kinds = set()
    for hyp, ref in pairs:
        kinds |= set(_check(hyp, ref))
    assert kinds == {0, 1, 2, 3}
    for hyp, ref in sc.content_pairs(33):
        _check(hyp, ref)


# --------------------------------------------------------------------------- the public API
PREDS = ["The  cat sat on mat", "a 𝄞clef  ran", "", "Dog ran fast", "über"]
REFS = ["the cat SAT on a mat", "a naïve ran", "it's ok", "", "über"]


def test_error_alignments_on_the_host():
    for unit in ("word", "char"):
        als = T.error_alignments(PREDS, REFS, unit)
        counts = T.error_counts(PREDS, REFS, unit)
        assert len(als) == len(PREDS) and [a.counts for a in als] == counts
        assert als == T.error_alignments(PREDS, REFS, unit, device="cpu")    # a non-HIP device: the host
        for a, p, r in zip(als, PREDS, REFS):
            items = (lambda s: s.lower().split()) if unit == "word" else (lambda s: list(s.lower()))
            assert (a.hyp, a.ref) == (items(p), items(r)) and a.ops == T.edit_alignment_host(a.hyp, a.ref)
            got = list(a.pairs())
            assert [g[0] for g in got] == a.ops
            assert [g[1] for g in got if g[1] is not None] == a.hyp and [g[2] for g in got if g[2] is not None] == a.ref
            for op, h, r_, i, j in got:
                assert (h is None) == (op == T.DELETION) and (r_ is None) == (op == T.INSERTION)
                assert h is None or a.hyp[i] == h
                assert r_ is None or a.ref[j] == r_
    with pytest.raises(ValueError, match="unit"):
        T.error_alignments(PREDS, REFS, "phone")


def test_format_alignment_on_fixed_sentences():
    a, b, c, d, e = T.error_alignments(PREDS, REFS, "word")
    assert T.format_alignment(a) == ("REF: the cat sat on a   mat\n"
                                     "HYP: the cat sat on *** mat\n"
                                     "                    D")
    assert T.format_alignment(b) == ("REF: a naïve ran\n"          # a non-BMP word is one column wide per code point
                                     "HYP: a 𝄞clef ran\n"
                                     "       S")
    assert T.format_alignment(c) == "REF: it's ok\nHYP: ***  ***\n     D    D"
    assert T.format_alignment(d) == "REF: *** *** ***\nHYP: dog ran fast\n     I   I   I"
    assert T.format_alignment(e) == "REF: über\nHYP: über\n"
    # wrapping: no line longer than the width, the columns in order, three lines per block
    wrapped = T.format_alignment(a, width=18).split("\n")
    assert len(wrapped) == 6 and all(len(x) <= 18 for x in wrapped)
    assert wrapped[0] == "REF: the cat sat" and wrapped[3] == "REF: on a   mat" and wrapped[5] == "        D"
    # characters: a space is shown as an underscore
    ch = T.error_alignments(["a b"], ["ab"], "char")[0]
    assert T.format_alignment(ch) == "REF: a *** b\nHYP: a _   b\n       I"


def test_confusions_on_fixed_sentences():
    preds = ["the cat sat", "the 𝄞clef sat on", "cat", "a cat"]
    refs = ["the mat sat", "the mat sat", "the cat", "a mat"]
    sub, dele, ins = T.confusions(T.error_alignments(preds, refs, "word"))
    assert dict(sub) == {("mat", "cat"): 2, ("mat", "𝄞clef"): 1}
    assert dict(dele) == {"the": 1} and dict(ins) == {"on": 1}
    assert sub.most_common(1) == [(("mat", "cat"), 2)]
    assert T.confusions([]) == ({}, {}, {})


# --------------------------------------------------------------------------- the C ABI
NAMES = ("vasr_edit_align_i32", "vasr_edit_align_table_bytes")


def test_abi_symbols_and_table_extent():
    L = _L()
    lib = L.lib()
    assert lib.vasr_version() == L.ABI_VERSION == 21
    for name in NAMES:
        assert name in L._SIGNATURES and name in L.header_functions() and hasattr(lib, name)
    ext = lib.vasr_edit_align_table_bytes
    assert ext(400, 400) == 40000 and ext(9000, 9000) == 9000 * 1125 * 2 and ext(65535, 65535) == 65535 * 8192 * 2
    assert ext(0, 7) == 0 and ext(7, 0) == 0 and ext(1, 1) == 2 and ext(3, 8) == 6 and ext(3, 9) == 12
    for bad in ((-1, 1), (1, -1), (65536, 1), (1, 65536)):
        assert ext(*bad) == -1, bad


def test_entry_point_refuses_bad_arguments_before_any_device_call():
    lib = _L().lib()
    t = lib.vasr_edit_tile_cols()
    fake = 256  # aligned non-null pointer values: the checks return before any dereference

    def call(hyp=fake, ld_hyp=100, hyp_len=fake, max_hyp=100, ref=fake, ld_ref=100, ref_len=fake, max_ref=100, P=4,
             counts=fake, ops=fake, ld_ops=200, ops_len=fake, offset=fake, table=fake, table_bytes=1 << 20, ws=None,
             ws_bytes=0):
        return lib.vasr_edit_align_i32(hyp, ld_hyp, hyp_len, max_hyp, ref, ld_ref, ref_len, max_ref, P, counts, ops, ld_ops,
                                       ops_len, offset, table, table_bytes, ws, ws_bytes, None)

    for k in ("hyp", "hyp_len", "ref", "ref_len", "counts", "ops", "ops_len", "offset"):
        assert call(**{k: None}) == -1 and b"null" in lib.vasr_last_error(), k
    assert call(P=0) == -1 and b"pairs" in lib.vasr_last_error()
    assert call(P=65536) == -1 and b"65535" in lib.vasr_last_error()
    assert call(max_hyp=-1) == -1 and call(max_ref=-1) == -1
    assert call(max_hyp=65536, ld_hyp=65536, ld_ops=1 << 20) == -1 and b"65535" in lib.vasr_last_error()
    assert call(max_ref=65536, ld_ref=65536, ld_ops=1 << 20) == -1 and b"65535" in lib.vasr_last_error()
    assert call(ld_hyp=99) == -1 and b"ld_hyp" in lib.vasr_last_error()
    assert call(ld_ref=99) == -1 and b"ld_ref" in lib.vasr_last_error()
    assert call(ld_ops=199) == -1 and b"ld_ops" in lib.vasr_last_error()
    assert call(table=None) == -1 and b"table" in lib.vasr_last_error()
    assert call(table_bytes=-1) == -1 and b"table" in lib.vasr_last_error()
    assert call(table=257) == -1 and b"aligned" in lib.vasr_last_error()
    need = lib.vasr_edit_workspace_bytes(4, 100, t + 1)
    big = dict(max_ref=t + 1, ld_ref=t + 1, ld_ops=t + 101)
    assert call(**big) == -1 and b"workspace" in lib.vasr_last_error()
    assert call(**big, ws=fake, ws_bytes=need - 1) == -1 and b"workspace" in lib.vasr_last_error()
    assert call(**big, ws=260, ws_bytes=need) == -1 and b"aligned" in lib.vasr_last_error()


def test_ops_wrapper_checks_before_the_library():
    from velocity_asr import ops
    z = torch.zeros((2, 5), dtype=torch.int32)
    with pytest.raises(RuntimeError, match="HIP"):
        ops.edit_alignment(z, z, [1, 2], [3, 4])
    with pytest.raises(ValueError, match="tensor"):
        ops.edit_alignment([[1]], z, [1], [1])
    assert ops.EDIT_ALIGN_TABLE_BYTES == 1 << 30 == T.ALIGN_TABLE_BYTES and T.ALIGN_MIN_DEVICE_CELLS >= 0


# --------------------------------------------------------------------------- evaluate.py
def _evaluate():
    spec = importlib.util.spec_from_file_location("vasr_script_evaluate_align",
                                                  os.path.join(PKG_ROOT, "scripts", "evaluate.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


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


def test_evaluate_alignments_and_confusions(tmp_path, monkeypatch, capsys):
    """The model and the transcription are stubbed (they need the device); scoring, the report and the two
    new outputs are the script's own."""
    ev = _evaluate()
    a = ev.parse_args(["--checkpoint", "m.pt", "--test-set", "m.tsv"])
    assert a.alignments is None and a.confusions == 0
    rng = random.Random(4)
    refs = [sc.sentence(rng, n).strip() for n in (6, 1, 9, 4)]
    hyps = [refs[0], "", refs[2].replace("a", "the"), refs[3] + " extra"]
    man = tmp_path / "m.tsv"
    man.write_text("".join(f"f{i}.wav\t{r}\n" for i, r in enumerate(refs)), encoding="utf-8")
    monkeypatch.setattr(ev, "VELOCITYASR", _FakeModel)
    monkeypatch.setattr(ev, "transcribe_files", lambda model, files, *a, **k: [dict(transcription=h) for h in hyps])
    base = ["--checkpoint", "m.pt", "--test-set", str(man), "--device", "cpu"]
    out0, out1, al = tmp_path / "r0.txt", tmp_path / "r1.txt", tmp_path / "al.txt"
    assert ev.main(base + ["--output", str(out0)]) == 0
    plain = capsys.readouterr().out
    assert ev.main(base + ["--output", str(out1), "--alignments", str(al), "--confusions", "2"]) == 0
    full = capsys.readouterr().out
    r0, r1 = out0.read_text().splitlines(), out1.read_text().splitlines()
    wer, cer = T.compute_wer(hyps, refs), T.compute_cer(hyps, refs)
    # without the flags the report is what it was
    assert r0 == [f"Test Set: {man}", "Samples: 4", f"WER: {wer * 100:.2f}%", f"CER: {cer * 100:.2f}%"]
    assert "Top word" not in plain and not os.path.exists(tmp_path / "none")
    assert r1[:4] == r0 and all(line in full for line in r1)
    aligned = T.error_alignments(hyps, refs, "word")
    want = []
    for name, counter, show in zip(("substitutions", "deletions", "insertions"), T.confusions(aligned),
                                   (lambda k: f"{k[0]} -> {k[1]}", str, str)):
        want.append(f"Top word {name}:")
        want += [f"  {n:6d}  {show(k)}" for k, n in counter.most_common(2)]
    assert r1[4:] == want and "  extra" in r1[-1]
    text = ""
    for i, a_ in enumerate(aligned):
        c = a_.counts
        text += f"{tmp_path / f'f{i}.wav'}\tN={c.ref_length} S={c.substitutions} D={c.deletions} I={c.insertions}\n"
        text += T.format_alignment(a_) + "\n\n"
    assert al.read_text(encoding="utf-8") == text and text.count("REF: ") == 4
