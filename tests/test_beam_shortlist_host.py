"""Host tests of the shortlisted beam search's specification (beam_shortlist_cases, DESIGN.md
§3.6f), the yardstick of tests/test_beam_shortlist_gpu.py, against beam_lm_cases.search, the
restatement of the reference's full search that test_beam_lm_host.py pins to the reference's own
results.  No GPU is needed.

The claim under test is exactness: on the same float32 log-probabilities, an utterance for which
the specification reports no uncertified frame has the full search's beams -- the same prefixes
in the same order and the same float64 scores, bit for bit (both sides add the same Python floats
in the same order) -- and anything else is reported, never silently different.  At most 1 in 10
continuous utterances may be uncertified (the project's rule for undecided cases).
"""

import numpy as np
import pytest

import beam_lm_cases as F
import beam_shortlist_cases as C

ids = lambda c: c["name"]  # noqa: E731

_full = {}


def full(c):
    """The full search of a host case, computed once for all its K."""
    if c["name"] not in _full:
        _full[c["name"]] = F.search(None, c["W"], c["blank"], lengths=c["lengths"], log_probs=c["lp"])
    return _full[c["name"]]


def pruned(c, K):
    return C.search(*C.shortlist(c["lp"], K, c["blank"]), c["W"], c["blank"], c["V"], c["lengths"])


def test_shortlist_orders_by_log_probability_then_token():
    lp = np.array([[-1.0, -3.0, -1.0, -0.5, -3.0, -np.inf, -2.0]], np.float32)
    tok, val, bl = C.shortlist(lp, 4, 3)
    assert tok.tolist() == [[0, 2, 6, 1]] and val.tolist() == [[-1.0, -1.0, -2.0, -3.0]] and bl.tolist() == [-0.5]
    tok, val, bl = C.shortlist(lp, 64, 0)  # clamped to V - 1; -inf stays a value, the blank is left out
    assert tok.tolist() == [[3, 2, 6, 1, 4, 5]] and bl.tolist() == [-1.0]
    assert C.shortlist(np.array([[0.0, -0.0, 0.0]], np.float32), 2, 0)[0].tolist() == [[1, 2]]  # -0.0 == 0.0


@pytest.mark.parametrize("c", C.host_cases(), ids=ids)
def test_certified_utterances_equal_the_full_search(c):
    want = full(c)
    assert [len(ub) for ub in want][1:3] == [min(c["W"], c["V"]), 1] and want[2] == [([], 0.0)]
    for K in C.widths_and_sizes(c["W"], c["V"]):
        got, unc = pruned(c, K)
        for b, n in enumerate(unc):
            assert 0 <= n <= c["lengths"][b]
            if n == 0:
                assert got[b] == want[b], (c["name"], K, b)  # prefixes, order and float64 scores
        if K == c["V"] - 1:
            assert unc == [0] * len(unc), (c["name"], K)


def test_at_most_one_in_ten_continuous_utterances_is_uncertified():
    total, bad = 0, []
    for c in C.host_cases():
        for K in C.widths_and_sizes(c["W"], c["V"]):
            unc = pruned(c, K)[1]
            total += len(unc)
            bad += [(c["name"], K, b, n) for b, n in enumerate(unc) if n]
    print(f"uncertified: {len(bad)} of {total}: {bad}")
    assert len(bad) * 10 <= total, bad


def test_the_complete_shortlist_certifies_every_frame():
    for c in C.host_cases():
        got, unc = pruned(c, c["V"] - 1)
        assert unc == [0] * 5 and got == full(c), c["name"]


@pytest.mark.parametrize("c", C.tie_cases(), ids=ids)
def test_tie_families_certify_and_are_equal_or_say_so(c):
    lp = F.log_softmax(c["logits"])
    want = F.search(None, c["W"], c["blank"], log_probs=lp)
    got, unc = C.search(*C.shortlist(lp, c["K"], c["blank"]), c["W"], c["blank"], c["V"])
    assert unc[0] > 0 or got == want, c["name"]
    # with every non-blank token shortlisted the ties are the full search's own, insertion order and all
    got, unc = C.search(*C.shortlist(lp, c["V"] - 1, c["blank"]), c["W"], c["blank"], c["V"])
    assert unc == [0] and got == want, c["name"]


def test_a_tail_token_outside_the_shortlist_keeps_its_keys_position():
    """The structural position decides a certified frame.  After frame 0 the beams are (), (7), (1)
    with () and (7) tied.  In frame 1 token 7 is far outside the shortlist {9, 3, 4}, and (), (7) (by
    its blank extension) and (9) tie at -0.75.  The full search inserted the key (7) when beam ()
    was extended by 7, at position 0 * 13 + 8, ahead of (9) at 0 * 13 + 10; (7)'s own blank
    extension comes only at 1 * 13.  A pruned step that places (7) by its scored candidates alone
    returns (), (9), (7) -- certified and wrong."""
    V, W, blank, K = 12, 3, 0, 3
    lp = np.full((1, 2, V), -30.0, np.float32)
    lp[0, 0, [0, 7, 1, 2]] = [-0.5, -0.5, -20.0, -25.0]
    lp[0, 1, [0, 9, 3, 4]] = [-0.25, -0.25, -5.0, -6.0]
    want = F.search(None, W, blank, log_probs=lp)
    assert want == [[([], -0.75), ([7], -0.75), ([9], -0.75)]]
    tok, val, bl = C.shortlist(lp, K, blank)
    assert tok[0].tolist() == [[7, 1, 2], [9, 3, 4]]
    got, unc = C.search(tok, val, bl, W, blank, V)
    assert unc == [0] and got == want


def test_abi_declares_exports_and_types_both_entry_points():
    from conftest import REPO
    from velocity_asr import _lib
    L = _lib.load()
    header = open(f"{REPO}/include/vasr.h").read()
    for n, nargs in (("vasr_ctc_beam_shortlist_f32", 13), ("vasr_ctc_beam_search_shortlist", 17)):
        assert n in _lib.header_functions() and n in _lib._SIGNATURES and hasattr(L, n) and f" {n}(" in header
        assert len(_lib._SIGNATURES[n][0]) == nargs
    assert L.vasr_version() == _lib.ABI_VERSION == 21 and "#define VASR_ABI_VERSION 21\n" in header


def test_abi_refuses_bad_arguments_before_any_launch():
    from velocity_asr import _lib
    L = _lib.load()
    fake = 256  # non-null pointer values: the checks return before any dereference or launch

    def short(logits=fake, B=1, Lq=8, V=10, K=4, blank=0, frames=None, tok=fake, lp=fake, bl=fake, ld_row=None):
        return L.vasr_ctc_beam_shortlist_f32(logits, V if ld_row is None else ld_row, Lq * V, B, Lq, V, K, blank, frames,
                                             tok, lp, bl, None)

    for null in ("logits", "tok", "lp", "bl"):
        assert short(**{null: None}) == -1 and b"vasr_ctc_beam_shortlist_f32: null pointer" in L.vasr_last_error(), null
    assert short(K=0, lp=None) == -1  # complete mode needs its rows, but neither tok nor the blank column
    for bad in (dict(K=65), dict(K=-1), dict(blank=10), dict(blank=-1), dict(V=0), dict(B=-1), dict(Lq=-1),
                dict(V=(1 << 20) + 1)):
        assert short(**bad) == -1 and b"vasr_ctc_beam_shortlist_f32: bad shape" in L.vasr_last_error(), bad
    assert short(V=1, K=1) == -1 and b"non-blank" in L.vasr_last_error()
    assert short(ld_row=9) == -1 and b"strides" in L.vasr_last_error()
    assert short(B=0) == 0 and short(Lq=0, logits=None) == 0  # nothing to do: no launch

    def search(tok=fake, lp=fake, bl=fake, B=1, Lq=8, K=4, V=10, W=4, blank=0, trie=fake, toks=fake, lens=fake,
               score=fake, nb=fake, unc=fake):
        return L.vasr_ctc_beam_search_shortlist(tok, lp, bl, B, Lq, K, V, W, blank, None, trie, toks, lens, score, nb,
                                                unc, None)

    for null in ("lp", "trie", "toks", "lens", "score", "nb", "unc"):
        assert search(**{null: None}) == -1 and b"vasr_ctc_beam_search_shortlist: null pointer" in L.vasr_last_error()
    assert search(bl=None) == -1 and b"blank column" in L.vasr_last_error()
    for bad in (dict(W=0), dict(W=33), dict(blank=10), dict(blank=-1), dict(V=0), dict(B=-1), dict(Lq=-1)):
        assert search(**bad) == -1 and b"vasr_ctc_beam_search_shortlist: bad shape" in L.vasr_last_error(), bad
    for bad in (dict(K=0), dict(K=65, V=100), dict(K=10)):  # K = 10 > V - 1
        assert search(**bad) == -1 and b"K=" in L.vasr_last_error(), bad
    assert search(B=0) == 0 and search(tok=None, bl=None, K=0, B=0) == 0


def test_public_arguments():
    import torch
    from velocity_asr import decode, ops
    assert decode.beam_shortlist_size("auto", 1000, 10) == 20 and decode.beam_shortlist_size("auto", 1000, 4) == 16
    assert decode.beam_shortlist_size("auto", 50000, 32) == 64 and decode.beam_shortlist_size(12, 5, 3) == 4
    for bad in (0, 65, "all"):
        with pytest.raises(ValueError, match="shortlist"):
            decode.beam_shortlist_size(bad, 100, 4)
    with pytest.raises(RuntimeError, match="HIP devices only"):  # a host tensor never reaches the kernels
        ops.ctc_beam_shortlist(torch.zeros(1, 4, 6), 3)
    with pytest.raises(RuntimeError, match="HIP devices only"):
        ops.ctc_beam_search_shortlist(None, torch.zeros(1, 4, 6), None, 6, 3)
    with pytest.raises(ValueError, match="language model"):
        decode._check_shortlist("ctc_beam_search", "auto", 4, True)
    with pytest.raises(ValueError, match="width"):
        decode._check_shortlist("ctc_beam_search", "auto", 33, False)
