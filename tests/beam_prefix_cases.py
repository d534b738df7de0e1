"""Shared by tests/test_beam_prefix_host.py and tests/test_beam_prefix_gpu.py: the specification of
the standard CTC prefix beam search (csrc/beam_prefix.hip) in plain Python floats,
and the case lists.  Importing this module imports neither velocity_asr nor the reference.

The search.  Log domain, float64 over float32 log-probabilities.  A live beam is (prefix, pb, pnb):
the summed log-probability of the alignments of `prefix` that end in the blank and of those that
end in its last token; the start is ((), 0.0, -inf).  A frame turns the sorted live beams into
contributions, each with a position, beam i at i * (V + 1) onwards:
    position i (V + 1)            pb[prefix]          += tot + lp[blank]          tot = pb (+) pnb
    position i (V + 1) + tok + 1  tok == tail:  pnb[prefix]          += pnb + lp[tok]
                                                pnb[prefix + (tok,)] += pb  + lp[tok]
                                  otherwise:    pnb[prefix + (tok,)] += tot + lp[tok]
where += is logaddexp in the order of the positions and a contribution of -inf is not made (it
creates no key and lends no position).  A key's position is that of its first contribution; at
the one position a repeated tail shares, the prefix's own key comes before prefix + (tok,) (they
share it as first position only when the blank's contribution is missing, i.e. -inf).  The W
keys of largest rank = ((pb (+) pnb) + alpha * S(key)) + beta * len(key) survive, the smaller
position first among equal ranks; S is beam_lm_cases.table_score, in effect with a table and
alpha > 0.  Results per beam: (tokens, logp = pb (+) pnb, score = rank).
"""

import math

import numpy as np

import beam_lm_cases as F
import beam_shortlist_cases as SC

f32 = np.float32
NEG = -math.inf
log_softmax = F.log_softmax


def logaddexp(a, b):
    """log(exp(a) + exp(b)); x (+) -inf = x exactly."""
    if a == NEG:
        return b
    if b == NEG:
        return a
    hi, lo = (a, b) if a >= b else (b, a)
    return hi + math.log1p(math.exp(lo - hi))


def search_plain(log_probs, W, blank=0, table=None, alpha=0.0, beta=0.0, lengths=None, shared=None):
    """The text above, word for word: log_probs (B, L, V) float32 -> per utterance
    [(tokens, logp, score)], best first.  Every candidate goes through a dict; for small cases.
    shared: a list that receives, per utterance, the number of frames in which two surviving keys
    have the same position."""
    lp_all = np.asarray(log_probs, f32)
    B, L, V = lp_all.shape
    lm = table is not None and alpha > 0

    def rank(key, pb, pnb):
        s = logaddexp(pb, pnb)
        if lm:
            s = s + alpha * F.table_score(table, key)
        return s + beta * len(key)

    out = []
    for b in range(B):
        live = [((), 0.0, NEG)]
        twice = 0
        for t in range(L if lengths is None else int(lengths[b])):
            lp = lp_all[b, t].tolist()
            new = {}  # key -> [pb, pnb, position]; insertion order breaks a tie in rank and position

            def give(key, which, value, pos):
                if value == NEG:
                    return
                e = new.get(key)
                if e is None:
                    e = new[key] = [NEG, NEG, pos]
                e[which] = logaddexp(e[which], value)

            for i, (prefix, pb, pnb) in enumerate(live):
                at = i * (V + 1)
                tot = logaddexp(pb, pnb)
                give(prefix, 0, tot + lp[blank], at)
                tail = prefix[-1] if prefix else None
                for tok in range(V):
                    if tok == blank:
                        continue
                    if tok == tail:
                        give(prefix, 1, pnb + lp[tok], at + tok + 1)
                        give(prefix + (tok,), 1, pb + lp[tok], at + tok + 1)
                    else:
                        give(prefix + (tok,), 1, tot + lp[tok], at + tok + 1)
            ranked = sorted(((-rank(k, e[0], e[1]), e[2], n, k) for n, (k, e) in enumerate(new.items())))[:W]
            twice += len({pos for _, pos, _, _ in ranked}) < len(ranked)
            live = [(k, new[k][0], new[k][1]) for _, _, _, k in ranked]
        if shared is not None:
            shared.append(twice)
        out.append([(list(k), logaddexp(pb, pnb), rank(k, pb, pnb)) for k, pb, pnb in live])
    return out


def search(log_probs, W, blank=0, table=None, alpha=0.0, beta=0.0, lengths=None, margins=None):
    """search_plain's results, value for value (test_beam_prefix_host.py compares them), for the
    larger cases.  Only the keys of live prefixes can receive more than one contribution, so those
    are merged one by one as above; every other extension is a key of a single contribution, whose
    rank is formed for all tokens of a beam at once in float64 -- the same operations in the same
    order -- and only each beam's W + 1 best (rank descending, token ascending) enter the sort.
    margins: a list that receives, per utterance, the smallest difference between neighbouring ranks
    among any frame's W + 1 best keys (inf with a single key): what an implementation whose float64
    values differ by less than that cannot reorder."""
    lp_all = np.asarray(log_probs, f32)
    B, L, V = lp_all.shape
    lm = table is not None and alpha > 0
    tab = None if not lm else np.asarray(table, np.float64)

    def rank(tot, S, n):
        s = tot
        if lm:
            s = s + alpha * S
        return s + beta * n

    out = []
    for b in range(B):
        live = [((), 0.0, NEG, 0.0)]  # prefix, pb, pnb, S(prefix)
        margin = math.inf
        for t in range(L if lengths is None else int(lengths[b])):
            row = lp_all[b, t].astype(np.float64)
            lp = row.tolist()
            index = {beam[0]: j for j, beam in enumerate(live)}
            cands = []  # (-rank, position, prefix, pb, pnb, S)
            single = np.ones((len(live), V), bool)  # extensions that reach no live prefix
            single[:, blank] = False
            for j, (prefix, pb, pnb, S) in enumerate(live):
                tot = logaddexp(pb, pnb)
                given = []  # (which, value, position) in the order of the positions
                given.append((0, tot + lp[blank], j * (V + 1)))
                if prefix:
                    tail = prefix[-1]
                    given.append((1, pnb + lp[tail], j * (V + 1) + tail + 1))
                    i = index.get(prefix[:-1])
                    if i is not None:
                        ip, ipb, ipnb, _ = live[i]
                        base = ipb if (ip and ip[-1] == tail) else logaddexp(ipb, ipnb)
                        given.append((1, base + lp[tail], i * (V + 1) + tail + 1))
                        single[i, tail] = False
                e = [NEG, NEG]
                pos = None
                for which, value, at in sorted(given, key=lambda g: g[2]):
                    if value == NEG:
                        continue
                    e[which] = logaddexp(e[which], value)
                    pos = at if pos is None else min(pos, at)
                if pos is not None:
                    cands.append((-rank(logaddexp(e[0], e[1]), S, len(prefix)), pos, prefix, e[0], e[1], S))
            for i, (prefix, pb, pnb, S) in enumerate(live):
                a = np.full(V, logaddexp(pb, pnb)) + row
                if prefix:
                    a[prefix[-1]] = pb + lp[prefix[-1]]
                r = a
                Sx = None
                if lm:
                    Sx = S + tab[1 + prefix[-1] if prefix else 0]
                    with np.errstate(invalid="ignore"):
                        r = r + alpha * Sx
                r = r + beta * (len(prefix) + 1)
                ok = single[i] & (a != NEG)
                toks = np.flatnonzero(ok)
                toks = toks[np.argsort(-r[toks], kind="stable")[:W + 1]]
                for tok in toks.tolist():
                    cands.append((-float(r[tok]), i * (V + 1) + tok + 1, prefix + (tok,), NEG, float(a[tok]),
                                  float(Sx[tok]) if lm else 0.0))
            cands.sort(key=lambda c: (c[0], c[1], len(c[2])))  # at a shared position the prefix's own key first
            margin = min([margin] + [y[0] - x[0] for x, y in zip(cands[:W], cands[1:W + 1])])
            live = [c[2:] for c in cands[:W]]
        if margins is not None:
            margins.append(margin)
        out.append([(list(k), logaddexp(pb, pnb), rank(logaddexp(pb, pnb), S, len(k))) for k, pb, pnb, S in live])
    return out


def pruned_rows(log_probs, K, blank):
    """The rows the pruned mode searches: every non-blank token outside the frame's K best
    (beam_shortlist_cases.shortlist: log-probability descending, token ascending) at -inf."""
    lp = np.asarray(log_probs, f32)
    tok, val, bl = SC.shortlist(lp, K, blank)
    return rows_of_shortlist(tok, val, bl, lp.shape[-1], blank)


def rows_of_shortlist(tok, val, blank_lp, V, blank):
    """(B, L, V) rows holding a shortlist's entries and the blank, -inf elsewhere."""
    tok, val, blank_lp = np.asarray(tok), np.asarray(val, f32), np.asarray(blank_lp, f32)
    rows = np.full(tok.shape[:2] + (V,), -np.inf, f32)
    np.put_along_axis(rows, np.where(tok >= 0, tok, blank).astype(np.int64), val, axis=-1)  # a -1 fill: overwritten below
    rows[..., blank] = blank_lp
    return rows


def prefixes(beams):
    return [[p for p, _, _ in ub] for ub in beams]


# ------------------------------------------------------------------------------------- cases
EXHAUSTIVE = [(3, 4, 0), (3, 4, 1), (3, 4, 2), (2, 20, 0), (5, 2, 4)]  # V, L, blank: W = 32 holds every prefix
EXHAUSTIVE_W = 32
ALPHAS, BETAS = (0.0, 0.5, 1.0), (0.0, 0.5)
SEED = 7070  # chosen on the CPU: at most 1 device case in 10 is undecided (test_beam_prefix_host.py asserts it)
UNIFORM = [(7, 4, 3), (7, 32, 3), (257, 4, 100), (257, 32, 100)]  # V, W, blank: L = 1, every candidate ties

_built = {}
_expected = {}


def exhaustive_cases():
    if "ex" not in _built:
        rng = np.random.default_rng(SEED + 1)
        out = []
        for V, L, blank in EXHAUSTIVE:
            lg = (rng.standard_normal((1, L, V)) * 2.0).astype(f32)
            tb = F.random_table(rng, V, blank)
            for a in (lg, tb):
                a.setflags(write=False)
            out.append(dict(name=f"all-v{V}-l{L}-b{blank}", V=V, W=EXHAUSTIVE_W, blank=blank, logits=lg, table=tb,
                            alpha=0.0, beta=0.0))
        _built["ex"] = out
    return _built["ex"]


def device_cases():
    """beam_lm_cases.CONTINUOUS's shapes and MODEL_SIZED, one utterance of random logits and one
    random table per shape, at every (alpha, beta) of ALPHAS x BETAS."""
    if "dev" not in _built:
        rng = np.random.default_rng(SEED)
        out = []
        for V, L, W, blank, scale, _ in F.CONTINUOUS + [F.MODEL_SIZED]:
            lg = (rng.standard_normal((1, L, V)) * scale).astype(f32)
            tb = F.random_table(rng, V, blank)
            for a in (lg, tb):
                a.setflags(write=False)
            for alpha in ALPHAS:
                for beta in BETAS:
                    out.append(dict(name=f"v{V}-l{L}-w{W}-b{blank}-a{alpha}-b{beta}", V=V, W=W, blank=blank, logits=lg,
                                    table=tb, alpha=alpha, beta=beta))
        _built["dev"] = out
    return _built["dev"]


# V 5, L 8, W 6, blank 0 at -inf in three frames: without its blank contribution a prefix's first
# position is its repeat's, which the extension by the same token shares, and at this width the two
# keys compete.  Seeds chosen on the CPU (test_beam_prefix_host.py asserts both properties): every
# case is decided, and in every case two surviving keys of some frame share a position.
BLANK_INF = dict(V=5, L=8, W=6, blank=0, frames=3, beta=0.3)
BLANK_INF_SEEDS = (26, 30, 44, 54, 68, 80, 83, 87)


def blank_inf_cases():
    if "binf" not in _built:
        out = []
        q = BLANK_INF
        for seed in BLANK_INF_SEEDS:
            rng = np.random.default_rng(seed)
            lg = (rng.standard_normal((1, q["L"], q["V"])) * 1.5).astype(f32)
            lg[0, rng.choice(q["L"], q["frames"], replace=False), q["blank"]] = -np.inf
            lg.setflags(write=False)
            out.append(dict(name=f"blank-inf-s{seed}", V=q["V"], W=q["W"], blank=q["blank"], logits=lg, table=None, alpha=0.0,
                            beta=q["beta"]))
        _built["binf"] = out
    return _built["binf"]


def uniform_cases():
    return [dict(name=f"uniform-v{V}-w{W}-b{blank}", V=V, W=W, blank=blank, logits=np.full((1, 1, V), 0.25, f32),
                 table=None, alpha=0.0, beta=0.0) for V, W, blank in UNIFORM]


def expected(c):
    """(the specification's beams on log_softmax(logits), decided) for a case, computed once.
    Decided (test_beam_sweep's rule): the same prefixes in the same order under the three other
    float32 log-probabilities of beam_lm_cases.variants()."""
    if c["name"] not in _expected:
        kw = dict(table=c["table"], alpha=c["alpha"], beta=c["beta"])
        want = search(log_softmax(c["logits"]), c["W"], c["blank"], **kw)
        decided = all(prefixes(search(lp, c["W"], c["blank"], **kw)) == prefixes(want) for lp in F.variants(c["logits"]))
        _expected[c["name"]] = (want, decided)
    return _expected[c["name"]]
