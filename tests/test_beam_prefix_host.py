"""Host tests of the standard CTC prefix beam search's specification (beam_prefix_cases, DESIGN.md
§3.6h), the yardstick of tests/test_beam_prefix_gpu.py, and of decode's host form of it.

The specification is pinned from outside: with every prefix kept (W = 32 at the exhaustive shapes)
a beam's logp is the log of the total probability of its prefix's alignments, which is what
torch's CPU float64 ctc_loss computes by the forward recursion.  Bar 1e-12: both are float64 sums
of the same float32 values in different orders, over at most 20 frames (measured: 4e-15).
"""

import itertools
import math

import numpy as np
import pytest
import torch

import beam_lm_cases as F
import beam_prefix_cases as P

ids = lambda c: c["name"]  # noqa: E731
SCORE_ATOL = 1e-4  # tests/test_beam_sweep.py


def ctc_logp(lp, tokens, blank):
    """log p(tokens | frames) of (L, V) float32 log-probabilities by torch's float64 ctc_loss; the
    empty prefix is the all-blank path."""
    if not tokens:
        return float(lp[:, blank].astype(np.float64).sum())
    nll = torch.nn.functional.ctc_loss(torch.tensor(lp, dtype=torch.float64)[:, None, :], torch.tensor([tokens]),
                                       torch.tensor([lp.shape[0]]), torch.tensor([len(tokens)]), blank=blank,
                                       reduction="none", zero_infinity=False)
    return -float(nll[0])


@pytest.mark.parametrize("c", P.exhaustive_cases(), ids=ids)
@pytest.mark.parametrize("alpha,beta", [(0.0, 0.0), (0.7, 0.3)])
def test_specification_vs_ctc_loss(c, alpha, beta):
    lp = P.log_softmax(c["logits"])
    V, L, blank = c["V"], lp.shape[1], c["blank"]
    beams = P.search(lp, P.EXHAUSTIVE_W, blank, c["table"], alpha, beta)[0]
    feasible = [p for n in range(L + 1) for p in itertools.product([t for t in range(V) if t != blank], repeat=n)
                if n + sum(a == b for a, b in zip(p, p[1:])) <= L]
    assert len(feasible) <= P.EXHAUSTIVE_W
    assert sorted(tuple(p) for p, _, _ in beams) == sorted(feasible)  # every prefix with an alignment, once
    worst, total = 0.0, -math.inf
    for tokens, logp, score in beams:
        ref = ctc_logp(lp[0], tokens, blank)
        rank = (ref + alpha * F.table_score(c["table"], tokens)) + beta * len(tokens)
        worst = max(worst, abs(logp - ref), abs(score - rank))
        total = P.logaddexp(total, logp)
    print(f"{c['name']} alpha {alpha} beta {beta}: worst |logp + ctc_loss| {worst:.2e}, log-sum of all beams {total:.2e}")
    assert worst <= 1e-12
    assert abs(total) <= 1e-6  # complete up to the float32 softmax's rounding
    scores = [s for _, _, s in beams]
    assert scores == sorted(scores, reverse=True)


def test_fast_specification_is_the_plain_one():
    """search (vectorised over a beam's single-contribution extensions) against search_plain (every
    candidate through a dict): equal values, -inf columns, a -inf blank and lengths included."""
    for c in P.exhaustive_cases() + P.blank_inf_cases() + [c for c in P.device_cases() if c["V"] <= 64]:
        lp = P.log_softmax(c["logits"])
        args = (lp, c["W"], c["blank"], c["table"], c["alpha"], c["beta"])
        assert P.search(*args) == P.search_plain(*args), c["name"]
    lp = np.array(P.log_softmax(np.random.default_rng(1).standard_normal((2, 9, 12)).astype(np.float32)))
    lp[:, :, 5] = -np.inf
    lp[0, 3:6, 0] = -np.inf
    assert P.search(lp, 6, 0, lengths=[9, 4]) == P.search_plain(lp, 6, 0, lengths=[9, 4])


def test_blank_inf_cases_share_a_position_and_are_decided():
    """What the device test of these cases relies on: each is decided, and in each some frame has two
    surviving keys with one position (a prefix whose first contribution is its repeat, and its
    extension by the same token), which an implementation that names keys by position confuses."""
    for c in P.blank_inf_cases():
        lp = P.log_softmax(c["logits"])
        shared = []
        want = P.search_plain(lp, c["W"], c["blank"], beta=c["beta"], shared=shared)
        assert shared[0] > 0, c["name"]
        assert P.expected(c) == (want, True), c["name"]


@pytest.mark.parametrize("c", P.uniform_cases(), ids=ids)
def test_uniform_rows_order_by_position(c):
    """L = 1, every candidate ties: the blank extension (the empty prefix), then tokens ascending."""
    want, decided = P.expected(c)
    tokens = [t for t in range(c["V"]) if t != c["blank"]]
    assert P.prefixes(want)[0] == ([[]] + [[t] for t in tokens])[:c["W"]]
    assert decided and len({s for _, _, s in want[0]}) == 1


def test_most_device_cases_are_decided():
    """The project's rule: at most 1 undecided case in 10, for the specification alone."""
    cases = P.device_cases() + P.exhaustive_cases()
    undecided = [c["name"] for c in cases if not P.expected(c)[1]]
    print(f"undecided: {len(undecided)} of {len(cases)}: {undecided}")
    assert len(undecided) * 10 <= len(cases), undecided


def test_pruned_and_full_search_can_differ():
    """Token pruning is an approximation: over small cases the best prefix mostly agrees, not always
    (measured: recorded in the print), and K = V - 1 prunes nothing."""
    rng = np.random.default_rng(99)
    same = 0
    for n in range(16):
        lp = P.log_softmax((rng.standard_normal((1, 12, 12)) * 1.0).astype(np.float32))
        full = P.search(lp, 4, 0)
        assert P.search(P.pruned_rows(lp, 11, 0), 4, 0) == full
        same += P.prefixes(P.search(P.pruned_rows(lp, 2, 0), 4, 0))[0][0] == P.prefixes(full)[0][0]
    print(f"best prefix equal in {same} of 16")
    assert same == 7  # the figure DESIGN.md §3.6h quotes


class _Wrapped:
    """A scorer the device cannot run: BigramLM's table behind a plain score()."""

    def __init__(self, table):
        self.table = table

    def score(self, tokens):
        return F.table_score(self.table, tokens)


def _compare(got, want, decided, what):
    assert len(got) == len(want)
    worst = 0.0
    for gb, wb in zip(got, want):
        assert len(gb) == len(wb), what
        if decided:
            assert [r.tokens for r in gb] == [p for p, _, _ in wb], what
            for r, (_, logp, score) in zip(gb, wb):
                worst = max(worst, abs(r.logp - logp), abs(r.score - score))
    assert worst <= SCORE_ATOL, (what, worst)
    return worst


HOST_CASES = P.exhaustive_cases() + P.blank_inf_cases() + [
    c for c in P.device_cases() if c["V"] <= 64 or (c["V"] == 257 and c["W"] == 5 and c["alpha"] == 0.5)]


@pytest.mark.parametrize("c", HOST_CASES, ids=ids)
def test_host_search_is_the_specification(c):
    """decode's host form (CPU logits, or a scorer that is not a BigramLM) against the specification:
    identical prefixes where decided, logp and score within 1e-4 (its log-probabilities are torch's
    float32 log_softmax, not numpy's)."""
    from velocity_asr import decode
    want, decided = P.expected(c)
    lg = torch.from_numpy(np.array(c["logits"]))
    lm = None if c["table"] is None else decode.BigramLM(c["table"])
    kw = dict(beam_width=c["W"], blank_token=c["blank"], lm_weight=c["alpha"], length_bonus=c["beta"])
    worst = _compare(decode.ctc_prefix_beam_search(lg, lm_scorer=lm, **kw), want, decided, c["name"])
    if c["alpha"] > 0:
        _compare(decode.ctc_prefix_beam_search(lg, lm_scorer=_Wrapped(c["table"]), **kw), want, decided, c["name"])
    else:
        assert decode.ctc_prefix_beam_search(lg, **kw) == decode.ctc_prefix_beam_search(lg, lm_scorer=lm, **kw)
    print(f"{c['name']}: decided {decided}, worst |d| {worst:.2e}")


def test_host_search_lengths_and_pruning():
    from velocity_asr import decode
    lg, lengths = F.ragged_case(V=12, L=9, blank=3, seed=8)
    x = torch.from_numpy(lg)
    lp = P.log_softmax(lg)
    got = decode.ctc_prefix_beam_search(x, beam_width=4, blank_token=3, length_bonus=0.25, input_lengths=lengths)
    _compare(got, P.search(lp, 4, 3, beta=0.25, lengths=lengths), True, "ragged")
    assert [(r.tokens, r.logp, r.score) for r in got[2]] == [([], 0.0, 0.0)]  # no frames
    for b, n in enumerate(lengths):
        alone = decode.ctc_prefix_beam_search(x[b:b + 1, :n], beam_width=4, blank_token=3, length_bonus=0.25)
        assert alone[0] == got[b]
    pruned = decode.ctc_prefix_beam_search(x, beam_width=4, blank_token=3, input_lengths=lengths, token_topk=3)
    _compare(pruned, P.search(P.pruned_rows(lp, 3, 3), 4, 3, lengths=lengths), True, "pruned")
    auto = decode.ctc_prefix_beam_search(x, beam_width=4, blank_token=3, token_topk="auto")  # 16 >= V - 1: nothing pruned
    assert auto == decode.ctc_prefix_beam_search(x, beam_width=4, blank_token=3)
    with pytest.raises(ValueError, match="input_lengths"):
        decode.ctc_prefix_beam_search(x, input_lengths=[1, 2])
    dec = decode.CTCDecoder(decode.create_default_vocabulary(12), blank_token=3)
    texts = dec.decode_prefix_beam_search(x, beam_width=4, input_lengths=lengths, length_bonus=0.25)
    beams = dec.decode_prefix_beam_search(x, beam_width=4, input_lengths=lengths, length_bonus=0.25, return_all_beams=True)
    assert texts == [ub[0].text for ub in beams] and [[r.tokens for r in ub] for ub in beams] == [[r.tokens for r in ub]
                                                                                                   for ub in got]
    assert decode.DecodingResult("", [], 0.0).logp is None
