"""Host tests of the ragged / bigram-LM beam search (vasr_ctc_beam_search_lm): the
yardstick of the GPU tests -- beam_lm_cases.search -- against the reference's own results in
tests/golden/beam_lm.json, decode.BigramLM, the new C entry point's declaration and argument
checks, the host search with lengths, and the near-tie cap of the GPU case list.  No GPU is needed.

The restatement is pinned to the reference at 1e-12 on the reference's own float32
log-probabilities (stored in the fixture: torch's and numpy's log-softmax differ in the last ulp,
which is the 1e-4 of the device bar, not part of this one); prefixes and beam counts are identical.
"""

import sys

import numpy as np
import pytest
import torch

from conftest import GOLDEN, REPO, golden_json
from oracle import velocity_ref as R

sys.path.insert(0, GOLDEN)
import beam_lm_cases as C  # noqa: E402
import gen_beam_lm_goldens as G  # noqa: E402

SCORE_TOL = 1e-12


@pytest.fixture(scope="module")
def gold():
    return golden_json("beam_lm.json")["cases"]


def _same(got, want, tol=SCORE_TOL):
    assert len(got) == len(want)
    for gb, wb in zip(got, want):
        assert [list(p) for p, _ in gb] == [list(p) for p, _ in wb]
        for (_, a), (_, b) in zip(gb, wb):
            assert abs(a - b) <= tol, (a, b)


def test_fixture_lists_every_case_and_regenerates_its_inputs(gold):
    assert sorted(gold) == sorted(C.GOLD)
    for name, c in C.GOLD.items():
        lg, table = C.gold_inputs(name)
        g = gold[name]
        assert g["shape"] == [c["B"], c["L"], c["V"]] and c["V"] <= 12 and c["L"] <= 20
        assert np.array_equal(lg, G.unpack(g["logits"], lg.shape))
        assert np.array_equal(table, G.unpack(g["table"], table.shape))
        assert sorted(g["full"]) == sorted(G.key(w, x) for w in C.GOLD_WIDTHS for x in C.GOLD_WEIGHTS)
        # the reference's log-softmax and numpy's agree to float32 rounding
        assert np.abs(G.unpack(g["log_probs"], lg.shape) - C.log_softmax(lg)).max() <= 2e-6


@pytest.mark.parametrize("name", sorted(C.GOLD))
def test_restatement_equals_the_reference_with_a_language_model(name, gold):
    c, g = C.GOLD[name], gold[name]
    shape = tuple(g["shape"])
    lg, table, lp = (G.unpack(g[k], s) for k, s in (("logits", shape), ("table", (shape[2] + 1, shape[2])),
                                                    ("log_probs", shape)))
    for w in C.GOLD_WIDTHS:
        for x in C.GOLD_WEIGHTS:
            _same(C.search(lg, w, c["blank"], table=table, lm_weight=x, log_probs=lp), g["full"][G.key(w, x)])
            _same(C.search(lg, w, c["blank"], table=table, lm_weight=x, log_probs=lp, lengths=c["lengths"]),
                  g["cut"][G.key(w, x)])
    if 0 in c["lengths"]:  # the reference on seq_len = 0: the empty beam, score 0.0
        assert g["cut"]["w3_x0.5"][c["lengths"].index(0)] == [[[], 0.0]]


def test_the_language_model_changes_the_golden_results(gold):
    """Otherwise the fixture would pin nothing about the LM term."""
    differ = 0
    for name, c in C.GOLD.items():
        lg, _ = C.gold_inputs(name)
        plain = R.ctc_beam_search(lg, 3, c["blank"])
        differ += C.prefixes(plain) != [[p for p, _ in ub] for ub in gold[name]["full"]["w3_x2.0"]]
    assert differ >= 2


@pytest.mark.parametrize("name", sorted(C.GOLD))
def test_restatement_without_a_table_is_the_oracle(name):
    c = C.GOLD[name]
    lg, table = C.gold_inputs(name)
    for w in C.GOLD_WIDTHS:
        want = R.ctc_beam_search(lg, w, c["blank"])
        assert C.search(lg, w, c["blank"]) == want
        assert C.search(lg, w, c["blank"], table=table, lm_weight=0.0) == want  # the reference's own test: weight > 0
        cut = [R.ctc_beam_search(lg[b:b + 1, :n], w, c["blank"])[0] for b, n in enumerate(c["lengths"])]
        assert C.search(lg, w, c["blank"], lengths=c["lengths"]) == cut


# ----------------------------------------------------------------------------- BigramLM
def test_bigram_score_is_bitwise_the_generators_scorer():
    from velocity_asr.decode import BigramLM
    rng = np.random.default_rng(1)
    for name, c in C.GOLD.items():
        _, table = C.gold_inputs(name)
        lm, scorer = BigramLM(table), G.TableScorer(table)
        toks = [t for t in range(c["V"]) if t != c["blank"]]
        assert lm.score([]) == 0.0 and isinstance(lm.score([]), float)
        for n in (1, 2, 5, 17):
            seq = rng.choice(toks, size=n).tolist()
            got = lm.score(seq)
            assert isinstance(got, float) and got == scorer.score(seq) == C.table_score(table, seq)
    assert lm.table.dtype == np.float32 and lm.table.shape == (c["V"] + 1, c["V"]) and lm.vocab_size == c["V"]
    with pytest.raises(ValueError, match=r"\(V \+ 1, V\)"):
        BigramLM(np.zeros((5, 5), np.float32))


@pytest.mark.parametrize("V,blank,alpha", [(6, 0, 1.0), (9, 8, 0.5), (1000, 999, 1.0)])
def test_from_token_sequences_rows_are_distributions_over_the_non_blank_tokens(V, blank, alpha):
    from velocity_asr.decode import BigramLM
    rng = np.random.default_rng(V)
    toks = [t for t in range(V) if t != blank]
    seqs = [rng.choice(toks, size=int(rng.integers(0, 9))).tolist() for _ in range(30)]
    lm = BigramLM.from_token_sequences(seqs, V, blank=blank, alpha=alpha)
    t = lm.table.astype(np.float64)
    assert t.shape == (V + 1, V) and np.isneginf(t[:, blank]).all()
    keep = np.arange(V) != blank
    assert np.isfinite(t[:, keep]).all()
    assert np.abs(np.log(np.exp(t[:, keep]).sum(axis=1))).max() <= 1e-5  # float32 entries
    # add-alpha counts: start -> a twice, a -> b once, nothing else seen
    a, b, c = toks[0], toks[1], toks[2]
    t = BigramLM.from_token_sequences([[a, b], [a]], V, blank=blank, alpha=alpha).table.astype(np.float64)
    n = V - 1
    assert abs(t[0, a] - np.log((2 + alpha) / (2 + alpha * n))) <= 1e-6
    assert abs(t[0, b] - np.log(alpha / (2 + alpha * n))) <= 1e-6
    assert abs(t[1 + a, b] - np.log((1 + alpha) / (1 + alpha * n))) <= 1e-6
    assert abs(t[1 + c, a] - np.log(1.0 / n)) <= 1e-6 and abs(t[1 + blank, a] - np.log(1.0 / n)) <= 1e-6
    for bad in ([[blank]], [[V]], [[-1]]):
        with pytest.raises(ValueError, match="BigramLM"):
            BigramLM.from_token_sequences(bad, V, blank=blank)


def test_save_load_round_trip(tmp_path):
    from velocity_asr.decode import BigramLM
    _, table = C.gold_inputs("v12_l20_b11")
    path = tmp_path / "lm.npz"
    BigramLM(table).save(path)
    with np.load(path) as z:
        assert list(z) == ["table"] and z["table"].dtype == np.float32
    back = BigramLM.load(path)
    assert np.array_equal(back.table, table) and back.score([3, 4, 4]) == C.table_score(table, [3, 4, 4])
    import velocity_asr.decode as D
    assert "BigramLM" in D.__all__


# ----------------------------------------------------------------------------- C ABI
def test_abi_declares_and_exports_the_entry_point():
    from velocity_asr import _lib
    L = _lib.load()
    header = open(f"{REPO}/include/vasr.h").read()
    n = "vasr_ctc_beam_search_lm"
    assert n in _lib.header_functions() and n in _lib._SIGNATURES and hasattr(L, n) and f" {n}(" in header
    assert len(_lib._SIGNATURES[n][0]) == 18
    assert L.vasr_version() == _lib.ABI_VERSION == 21 and "#define VASR_ABI_VERSION 21\n" in header


def test_abi_refuses_bad_arguments_before_any_launch():
    from velocity_asr import _lib
    L = _lib.load()
    fake = 256  # non-null pointer values: the checks return before any dereference or launch

    def run(logits=fake, B=1, Lq=8, V=10, W=4, blank=0, frames=None, table=None, ld_lm=0, weight=0.0, trie=fake,
            toks=fake, lens=fake, score=fake, nb=fake):
        return L.vasr_ctc_beam_search_lm(logits, V, Lq * V, B, Lq, V, W, blank, frames, table, ld_lm, weight, trie,
                                         toks, lens, score, nb, None)

    for null in ("logits", "trie", "toks", "lens", "score", "nb"):
        assert run(**{null: None}) == -1 and b"vasr_ctc_beam_search_lm: null pointer" in L.vasr_last_error(), null
    for bad in (dict(W=0), dict(W=33), dict(blank=10), dict(blank=-1), dict(V=0), dict(B=-1), dict(Lq=-1)):
        assert run(**bad) == -1 and b"vasr_ctc_beam_search_lm: bad shape" in L.vasr_last_error(), bad
    assert run(table=fake, ld_lm=9, weight=1.0) == -1 and b"ld_lm" in L.vasr_last_error()
    assert run(table=fake, ld_lm=0) == -1 and b"ld_lm" in L.vasr_last_error()  # also with the LM switched off
    assert run(weight=float("nan")) == -1 and b"NaN" in L.vasr_last_error()
    assert run(table=fake, ld_lm=10, weight=float("nan")) == -1 and b"NaN" in L.vasr_last_error()
    assert run(B=0) == 0 and run(B=0, frames=fake, table=fake, ld_lm=10, weight=1.0) == 0  # nothing to do: no launch
    # the old entry keeps its own name in its messages
    assert L.vasr_ctc_beam_search(fake, 10, 80, 1, 8, 10, 33, 0, fake, fake, fake, fake, fake, None) == -1
    assert b"vasr_ctc_beam_search: bad shape" in L.vasr_last_error()


def test_ops_refuses_host_frames_outside_the_logits_and_misshaped_tables():
    import inspect
    from velocity_asr import ops
    sig = inspect.signature(ops.ctc_beam_search)
    for k in ("frames", "lm_table", "lm_weight"):
        assert sig.parameters[k].kind is inspect.Parameter.KEYWORD_ONLY
    with pytest.raises(RuntimeError, match="HIP devices only"):  # a host tensor never reaches the kernel
        ops.ctc_beam_search(torch.zeros(1, 4, 6), 3, frames=[4])


# ----------------------------------------------------------------------------- host search
@pytest.mark.parametrize("name", ["v5_l12_b0", "v7_l9_b3"])
def test_host_search_with_a_bigram_and_lengths_equals_the_restatement(name):
    from velocity_asr.decode import BigramLM, _ctc_beam_search_host
    c = C.GOLD[name]
    lg, table = C.gold_inputs(name)
    lm = BigramLM(table)
    # the host search normalises with torch: compare on torch's log-probabilities, and exactly
    lp = torch.log_softmax(torch.from_numpy(lg), dim=-1).numpy()
    for lengths in (None, c["lengths"], torch.tensor(c["lengths"])):
        got = _ctc_beam_search_host(torch.from_numpy(lg), 3, c["blank"], 0.5, lm, lengths)
        want = C.search(lg, 3, c["blank"], table=table, lm_weight=0.5, log_probs=lp,
                        lengths=None if lengths is None else c["lengths"])
        _same([[(r.tokens, r.score) for r in ub] for ub in got], want)
    with pytest.raises(ValueError, match="input_lengths"):
        _ctc_beam_search_host(torch.from_numpy(lg), 3, c["blank"], 0.5, lm, [c["L"] + 1] * c["B"])


def test_decoder_and_transcription_take_the_new_arguments():
    import inspect
    from velocity_asr import transcription
    from velocity_asr.decode import CTCDecoder, ctc_beam_search
    assert "input_lengths" in inspect.signature(ctc_beam_search).parameters
    p = inspect.signature(CTCDecoder.decode_beam_search).parameters
    assert all(p[k].kind is inspect.Parameter.KEYWORD_ONLY for k in ("input_lengths", "lm_scorer", "lm_weight"))
    for fn in (transcription.transcribe_files, transcription._decode_batch):
        p = inspect.signature(fn).parameters
        assert p["lm"].default is None and p["lm_weight"].default == 0.0
    sys.path.insert(0, f"{REPO}/velocity-asr_amd/scripts")
    import evaluate
    a = evaluate.parse_args(["--checkpoint", "m.pt", "--audio-dir", "d"])
    assert a.lm is None and a.lm_weight == 0.0
    a = evaluate.parse_args(["--checkpoint", "m.pt", "--audio-dir", "d", "--beam-width", "5", "--lm", "lm.npz",
                             "--lm-weight", "0.5"])
    assert (a.beam_width, a.lm, a.lm_weight) == (5, "lm.npz", 0.5)


# ----------------------------------------------------------------------------- the GPU case list
def test_case_list_stays_within_the_stated_shapes():
    cases = C.continuous_cases() + C.tie_cases()
    assert len({c["name"] for c in cases}) == len(cases)
    for c in cases:
        _, L, V = c["logits"].shape
        assert (V <= 257 and L <= 65 or (V, L, c["W"]) == (1000, 40, 17)) and 1 <= c["W"] <= 32
        assert c["table"].shape == (V + 1, V) and c["table"].dtype == np.float32
    cont = C.continuous_cases()
    assert {c["lm_weight"] for c in cont} == {0.3, 1.0, 4.0} and {c["W"] for c in cont} >= {1, 32}
    assert {c["blank"] == 0 for c in cont} == {True, False}
    for c in C.tie_cases():
        assert set(np.unique(c["table"]).tolist()) <= set(C.TIE_ENTRIES) and c["lm_weight"] in C.TIE_WEIGHTS


def test_tie_cases_are_decided_and_tie():
    """No allowance for the tie families: every one is decided.  The ties are real (final scores
    repeat in most cases; with one non-blank token the table separates them), and the table
    changes the outcome of most cases (the LM term takes part in the ties)."""
    changed = tied = 0
    for c in C.tie_cases():
        want, decided = C.expected(c)
        assert decided, c["name"]
        assert all(len(np.unique(row)) <= 2 for row in C.log_softmax(c["logits"])[0])
        scores = [s for _, s in want[0]]
        tied += len(set(scores)) < len(scores)
        changed += C.prefixes(want) != C.prefixes(R.ctc_beam_search(c["logits"], c["W"], c["blank"]))
    assert tied * 2 >= len(C.tie_cases()) and changed * 2 >= len(C.tie_cases())


def test_at_most_one_in_ten_continuous_cases_is_undecided():
    cont = C.continuous_cases()
    undecided = [c["name"] for c in cont if not C.expected(c)[1]]
    print(f"undecided: {len(undecided)} of {len(cont)}: {undecided}")
    assert len(undecided) * 10 <= len(cont), undecided


def test_few_candidates_give_fewer_beams_than_the_width():
    by = {c["name"]: c for c in C.continuous_cases()}
    assert len(C.expected(by["lm-v7-l1-w32-b6-x0.3-s0"])[0][0]) == 7
    assert len(C.expected(by["lm-v7-l2-w32-b0-x4.0-s0"])[0][0]) == 32
