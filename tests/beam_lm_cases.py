"""Shared by tests/test_beam_lm_host.py, tests/test_beam_lm_gpu.py and
tests/golden/gen_beam_lm_goldens.py: the case lists of the ragged / bigram-LM beam search
(vasr_ctc_beam_search_lm) and `search`, a numpy restatement of the reference's
prefix beam search (decode.py:128-217) -- oracle.velocity_ref.ctc_beam_search's loop extended by
the lm_scorer term of decode.py:187-190 for a bigram table, and by per-utterance lengths (the
reference run on logits[b:b+1, :lengths[b]]).

Importing this module imports neither velocity_asr nor the reference, so the golden generator can
use it with the reference's package on the path; the helpers that need the project's BigramLM or
test_beam_sweep's tie families import them when called.
"""

import numpy as np

f32 = np.float32

# ------------------------------------------------------------------------------- restatement


def log_softmax(x):
    """oracle.velocity_ref.log_softmax: (x - max) - log(sum(exp(x - max))) in float32."""
    x = np.asarray(x, f32)
    d = (x - x.max(axis=-1, keepdims=True)).astype(f32)
    return (d - np.log(np.exp(d).sum(axis=-1, keepdims=True, dtype=f32))).astype(f32)


def table_score(table, tokens):
    """Score of a whole prefix: the left-to-right Python-float sum of its table entries, row 0
    after the sentence start and row 1 + p after token p; 0.0 for the empty prefix."""
    s, row = 0.0, 0
    for tok in tokens:
        s += float(table[row, tok])
        row = 1 + tok
    return s


def search(logits, beam_width, blank=0, table=None, lm_weight=0.0, lengths=None, log_probs=None):
    """Per utterance a list of (tokens, score), as oracle.velocity_ref.ctc_beam_search returns.
    table / lm_weight: the reference's lm_scorer hook with a bigram table behind it -- every
    non-blank candidate adds lm_weight * table_score(key), in every frame, the blank extension
    nothing.  lengths: utterance b walks its first lengths[b] rows only.  log_probs: use these
    float32 log-probabilities in place of log_softmax(logits)."""
    lp_all = log_softmax(logits) if log_probs is None else np.asarray(log_probs, f32)
    lm = table is not None and lm_weight > 0
    memo = {}

    def S(key):
        if key not in memo:
            memo[key] = table_score(table, key)
        return memo[key]

    out = []
    for b in range(lp_all.shape[0]):
        beams = {(): (0.0, None)}
        for t in range(lp_all.shape[1] if lengths is None else int(lengths[b])):
            lp = lp_all[b, t].tolist()  # float32 values as Python floats
            new = {}
            for prefix, (score, last) in beams.items():
                s = score + lp[blank]
                if prefix not in new or new[prefix][0] < s:
                    new[prefix] = (s, blank)
                for tok in range(len(lp)):
                    if tok == blank:
                        continue
                    s = score + lp[tok]
                    key = prefix if last == tok else prefix + (tok,)
                    if lm:
                        s += lm_weight * S(key)
                    if key not in new or new[key][0] < s:
                        new[key] = (s, tok)
            beams = dict(sorted(new.items(), key=lambda kv: kv[1][0], reverse=True)[:beam_width])
        out.append([(list(p), sc) for p, (sc, _) in sorted(beams.items(), key=lambda kv: kv[1][0], reverse=True)])
    return out


def variants(lg):
    """test_beam_sweep._variants: the float32 log-probabilities a correct implementation may
    produce besides log_softmax's own -- fp64 rounded to fp32, and each row's normaliser one fp32
    ulp up and down."""
    x = np.asarray(lg, np.float64)
    d64 = x - x.max(-1, keepdims=True)
    yield (d64 - np.log(np.exp(d64).sum(-1, keepdims=True))).astype(f32)
    lg = np.asarray(lg, f32)
    d = (lg - lg.max(-1, keepdims=True)).astype(f32)
    lse = np.log(np.exp(d).sum(-1, keepdims=True, dtype=f32)).astype(f32)
    for to in (f32(np.inf), f32(-np.inf)):
        yield (d - np.nextafter(lse, to)).astype(f32)


def prefixes(beams):
    return [[p for p, _ in ub] for ub in beams]


_expected = {}


def expected(c):
    """(the restatement's beams, decided) for a case dict, computed once.  Decided (the sweep's
    rule): the same prefixes under log_softmax's own values and under the three of variants()."""
    if c["name"] not in _expected:
        kw = dict(table=c.get("table"), lm_weight=c.get("lm_weight", 0.0), lengths=c.get("lengths"))
        want = search(c["logits"], c["W"], c["blank"], **kw)
        decided = all(prefixes(search(c["logits"], c["W"], c["blank"], log_probs=lp, **kw)) == prefixes(want)
                      for lp in variants(c["logits"]))
        _expected[c["name"]] = (want, decided)
    return _expected[c["name"]]


# ------------------------------------------------------------------------------- golden cases
# Searched by the reference itself (tests/golden/gen_beam_lm_goldens.py -> beam_lm.json) at
# every width and weight below, whole and cut to `lengths` by slicing.
GOLD_WIDTHS = (1, 3, 10)
GOLD_WEIGHTS = (0.5, 2.0)
GOLD = {  # name: B, L, V, blank, logit scale, seed, lengths
    "v5_l12_b0": dict(B=2, L=12, V=5, blank=0, scale=1.5, seed=11, lengths=[7, 12]),
    "v12_l20_b11": dict(B=2, L=20, V=12, blank=11, scale=2.0, seed=12, lengths=[20, 1]),
    "v7_l9_b3": dict(B=2, L=9, V=7, blank=3, scale=1.0, seed=13, lengths=[0, 5]),
    "v3_l16_b1": dict(B=1, L=16, V=3, blank=1, scale=3.0, seed=14, lengths=[9]),
}


def random_table(rng, V, blank, spread=2.0):
    """A (V + 1, V) float32 table of log-probabilities over the non-blank tokens of each row; the
    blank column is -inf, as BigramLM.from_token_sequences leaves it."""
    w = np.exp(rng.standard_normal((V + 1, V)) * spread)
    w[:, blank] = 0.0
    with np.errstate(divide="ignore"):
        return (np.log(w) - np.log(w.sum(axis=1, keepdims=True))).astype(f32)


def gold_inputs(name):
    """(logits (B, L, V) float32, table (V + 1, V) float32) of a golden case, from its seed."""
    c = GOLD[name]
    rng = np.random.default_rng(c["seed"])
    lg = (rng.standard_normal((c["B"], c["L"], c["V"])) * c["scale"]).astype(f32)
    return lg, random_table(rng, c["V"], c["blank"])


# ------------------------------------------------------------------------------- device cases
# V, L, W, blank, logit scale, lm_weight: three seeds each.  Blank 0 and V - 1, width 1, and width
# 32 above the number of candidates (v7-l1, v7-l2); the sweep's larger shapes.
CONTINUOUS = [(2, 12, 3, 0, 1.0, 1.0), (5, 33, 1, 4, 1.5, 0.3), (6, 30, 32, 0, 1.5, 4.0), (40, 25, 32, 39, 2.0, 1.0),
              (257, 65, 32, 256, 2.0, 0.3), (257, 65, 5, 0, 4.0, 4.0), (64, 64, 2, 0, 1.0, 1.0), (7, 1, 32, 6, 1.0, 0.3),
              (7, 2, 32, 0, 1.0, 4.0)]
MODEL_SIZED = (1000, 40, 17, 999, 3.0, 1.0)  # one seed: the model's vocabulary
TIE_WEIGHTS = (0.5, 0.25)
# V, L, W, blank: test_beam_sweep.TIE_SHAPES within V <= 257, and width 16 for the first.  In the
# two-level family the two log-probabilities differ by 3 up to one rounding, a multiple of every
# lm_weight * entry, so candidates with other counts of the two values can come within an ulp of
# each other; at V = 5 and width 32 nearly every prefix survives and such a pair always reaches
# the cut (undecided for every table tried), at width 16 it does not.
TIE_SHAPES = [(5, 10, 16, 0), (5, 10, 7, 2), (33, 6, 32, 32), (257, 5, 32, 0), (2, 40, 4, 1)]
TIE_TABLE_SEED = 2  # chosen on the CPU: all ten cases are decided (test_beam_lm_host.py asserts it)
TIE_ENTRIES = (0.0, -0.5, -1.0, -2.0)


def trained_table(rng, V, blank, count=40, length=12):
    """BigramLM.from_token_sequences on random non-blank sequences (add-one smoothing)."""
    from velocity_asr.decode import BigramLM
    toks = [t for t in range(V) if t != blank]
    seqs = [rng.choice(toks, size=int(rng.integers(1, length + 1))).tolist() for _ in range(count)]
    return BigramLM.from_token_sequences(seqs, V, blank=blank)


def _freeze(cases):
    for c in cases:
        for k in ("logits", "table"):
            if isinstance(c.get(k), np.ndarray):
                c[k].setflags(write=False)
    return cases


_built = {}


def continuous_cases():
    if "cont" not in _built:
        out = []
        rng = np.random.default_rng(3030)
        for V, L, W, blank, scale, w in CONTINUOUS + [MODEL_SIZED]:
            for s in range(1 if V == 1000 else 3):
                lg = (rng.standard_normal((1, L, V)) * scale).astype(f32)
                lm = trained_table(rng, V, blank)
                out.append(dict(name=f"lm-v{V}-l{L}-w{W}-b{blank}-x{w}-s{s}", kind="continuous", W=W, blank=blank,
                                logits=lg, lm=lm, table=lm.table, lm_weight=w))
        _built["cont"] = _freeze(out)
    return _built["cont"]


def tie_cases():
    """test_beam_sweep's two tie families with a table of entries from TIE_ENTRIES: log-probability
    sums are exact in float64 (see that module), and so is every lm_weight * S, so tied candidates
    tie bit for bit on the device and in the restatement alike."""
    if "tie" not in _built:
        from test_beam_sweep import two_level_rows, uniform_rows
        out = []
        for n, (V, L, W, blank) in enumerate(TIE_SHAPES):
            w = TIE_WEIGHTS[n % 2]
            for fam, rows in (("uniform", uniform_rows), ("twolevel", two_level_rows)):
                rng = np.random.default_rng(TIE_TABLE_SEED)
                table = rng.choice(np.array(TIE_ENTRIES, f32), size=(V + 1, V)).astype(f32)
                out.append(dict(name=f"lm-{fam}-v{V}-l{L}-w{W}-b{blank}-x{w}", kind="tie", W=W, blank=blank,
                                logits=rows(V, L).astype(f32), table=table, lm_weight=w))
        _built["tie"] = _freeze(out)
    return _built["tie"]


def ragged_case(V=40, L=25, blank=7, seed=5, B=5):
    """B utterances of random logits with frame counts [L, 1, 0, L - 1, 7][:B]."""
    rng = np.random.default_rng(seed)
    lg = (rng.standard_normal((B, L, V)) * 1.5).astype(f32)
    return lg, [L, 1, 0, L - 1, 7][:B]
