"""Cases shared by test_align_host.py and test_align_gpu.py: a second statement of the alignment rule,
written as a full cost table with an explicit backward walk (no code shared with velocity_asr.training),
the identities every path must satisfy, and the generators of score_cases."""

import score_cases as sc  # noqa: F401  (the generators, re-exported)

HIT, SUB, DEL, INS = 0, 1, 2, 3


def reference_path(hyp, ref):
    """The edit path in forward order.  cost[i][j] is the Levenshtein distance of hyp[:i] and ref[:j]; the
    walk starts at (len(hyp), len(ref)) and looks at its cell's neighbours each time: on row 0 only deletions
    are left, on column 0 only insertions, equal items are a hit, otherwise the cheapest neighbour in the
    order diagonal (substitution), left (deletion), up (insertion), the first one on a tie."""
    m, n = len(hyp), len(ref)
    cost = [[0] * (n + 1) for _ in range(m + 1)]
    for j in range(n + 1):
        cost[0][j] = j
    for i in range(1, m + 1):
        cost[i][0] = i
        for j in range(1, n + 1):
            if hyp[i - 1] == ref[j - 1]:
                cost[i][j] = cost[i - 1][j - 1]
            else:
                cost[i][j] = 1 + min(cost[i - 1][j - 1], cost[i][j - 1], cost[i - 1][j])
    back = []
    i, j = m, n
    while (i, j) != (0, 0):
        if i == 0:
            op = DEL
        elif j == 0:
            op = INS
        elif hyp[i - 1] == ref[j - 1]:
            op = HIT
        else:
            around = [(cost[i - 1][j - 1], SUB), (cost[i][j - 1], DEL), (cost[i - 1][j], INS)]
            op = min(around, key=lambda cv: cv[0])[1]  # min keeps the first of equal keys
        back.append(op)
        if op in (HIT, SUB):
            i, j = i - 1, j - 1
        elif op == DEL:
            j -= 1
        else:
            i -= 1
    return back[::-1]


def replay(path, hyp, ref):
    """Walks the path over both sequences and checks that it consumes them exactly, with hits on equal items
    and substitutions on unequal ones.  -> (S, D, I)."""
    i = j = 0
    n = [0, 0, 0, 0]
    for op in path:
        assert op in (HIT, SUB, DEL, INS), op
        n[op] += 1
        if op in (HIT, SUB):
            assert i < len(hyp) and j < len(ref)
            assert (hyp[i] == ref[j]) == (op == HIT), (i, j, op)
            i, j = i + 1, j + 1
        elif op == DEL:
            assert j < len(ref)
            j += 1
        else:
            assert i < len(hyp)
            i += 1
    assert (i, j) == (len(hyp), len(ref))
    return n[SUB], n[DEL], n[INS]


HAND = [
    ("ab", "ba", [SUB, SUB]),
    ("a c".split(), "a b c".split(), [HIT, DEL, HIT]),
    ("a b b c".split(), "a b c".split(), [HIT, INS, HIT, HIT]),   # walking back, the later b is the hit
    ("a b c".split(), "a x c".split(), [HIT, SUB, HIT]),
    ("", "", []),
    ("", "abc", [DEL, DEL, DEL]),
    ("abcd", "", [INS, INS, INS, INS]),
]
