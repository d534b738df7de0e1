"""Cases shared by test_score_host.py, test_score_gpu.py and tests/golden/gen_score_goldens.py:
seeded id sequences over a tiny alphabet (so ties are everywhere), sentence pairs, the boundary
lengths of the edit-distance kernel and the padded batches it reads."""

import random

import numpy as np

ALPHABET = 3
WORDS = ["the", "cat", "sat", "on", "a", "mat", "Dog", "ran", "fast", "über", "naïve", "𝄞clef", "it's", "ok"]


def seq(rng, n, alphabet=ALPHABET):
    return [rng.randrange(alphabet) for _ in range(n)]


def random_pairs(count, max_len, seed, alphabet=ALPHABET):
    """`count` (hyp, ref) pairs of ids with lengths 0..max_len, both ends included."""
    rng = random.Random(seed)
    return [(seq(rng, rng.randint(0, max_len), alphabet), seq(rng, rng.randint(0, max_len), alphabet))
            for _ in range(count)]


def edited(rng, ref, rate=0.1, alphabet=ALPHABET):
    """`ref` with about `rate` of its items substituted, dropped or preceded by a new one."""
    out = []
    for x in ref:
        u = rng.random()
        if u < rate / 3:
            out.append(rng.randrange(alphabet))
        elif u < 2 * rate / 3:
            continue
        elif u < rate:
            out.extend((rng.randrange(alphabet), x))
        else:
            out.append(x)
    return out


def boundary_lengths(w, t, strips=range(1, 10)):
    """Lengths of the long side: around the strip widths, the wave, the one-wave limit w, the tile t,
    and 2t + 3 (three passes)."""
    s = set(strips) | {0, 1, 2, 63, 64, 65, w - 1, w, w + 1, t - 1, t, t + 1, 2 * t + 3}
    return sorted(x for x in s if x >= 0)


SHORT_SIDE = (0, 1, 5, 70)


def boundary_pairs(w, t, seed=11):
    """(long, short) id sequences: every boundary length against every short-side length."""
    rng = random.Random(seed)
    return [(seq(rng, a), seq(rng, b)) for a in boundary_lengths(w, t) for b in SHORT_SIDE]


def content_pairs(n, seed=5):
    """Structured (hyp, ref) pairs at length n: identical, disjoint alphabets (with a length
    difference), ref = hyp rotated by one, and one repeated symbol at (n, n + 3) and (n + 3, n)."""
    rng = random.Random(seed)
    a = seq(rng, n)
    return [
        (a, list(a)),
        (a, [x + ALPHABET for x in seq(rng, n + 2)]),
        ([x + ALPHABET for x in seq(rng, n + 2)], a),
        (a, a[1:] + a[:1]),
        ([1] * n, [1] * (n + 3)),
        ([1] * (n + 3), [1] * n),
    ]


def pad_batch(seqs, width=None, ld=None, fill=-1):
    """(P, ld) int32 matrix filled with `fill`, row p starting with seqs[p] cut to `width` items, and the
    stored (uncut) lengths.  The kernel's matrix is the first `width` columns."""
    width = max([len(s) for s in seqs] + [0]) if width is None else width
    ld = max(width, 1) if ld is None else ld
    m = np.full((len(seqs), ld), fill, np.int32)
    for row, s in zip(m, seqs):
        k = min(len(s), ld)
        row[:k] = s[:k]
    return m, np.asarray([len(s) for s in seqs], np.int32)


def sentence(rng, n):
    """n words joined by one to three spaces, in mixed case."""
    parts = []
    for _ in range(n):
        w = rng.choice(WORDS)
        parts.append(w.upper() if rng.random() < 0.2 else w)
        parts.append(" " * rng.randint(1, 3))
    return "".join(parts)


def sentence_pairs(count, max_words, seed):
    """(prediction, reference) strings of 0..max_words words; the prediction is the reference with a
    few words changed, dropped or added."""
    rng = random.Random(seed)
    out = []
    for _ in range(count):
        ref = [rng.choice(WORDS) for _ in range(rng.randint(0, max_words))]
        hyp = [WORDS[i] for i in edited(rng, [WORDS.index(w) for w in ref], 0.3, len(WORDS))]
        if rng.random() < 0.1:
            hyp = []
        join = lambda ws: "".join(w + " " * rng.randint(1, 3) for w in ws)  # noqa: E731
        out.append((join(hyp).title() if rng.random() < 0.3 else join(hyp), join(ref)))
    return out


GOLDEN_PAIRS = [
    ("", ""), ("", "hello world"), ("hello world", ""), ("a b c", "a x c"), ("a c", "a b c"), ("a b b c", "a b c"),
    ("ab", "ba"), ("The  Cat SAT", "the cat sat"), ("  leading and trailing  ", "leading and trailing"),
    ("über naïve", "uber naive"), ("𝄞clef 𝄞", "𝄞 clef"), ("tab\tseparated\nwords", "tab separated words"),
] + sentence_pairs(18, 12, seed=77)
