"""Shared by tests/test_beam_shortlist_host.py and tests/test_beam_shortlist_gpu.py: a numpy
specification of the shortlisted prefix beam search (csrc/beam_shortlist.hip) and
the case lists.  Importing this module imports neither velocity_asr nor the reference.

shortlist(lp, K, blank): each frame's K non-blank tokens of largest log-probability, ordered by
(log-probability descending, token ascending), their log-probabilities, and the blank's.

search(tok, lp, blank_lp, W, blank, V, lengths): the frame step of the reference's prefix beam
search (decode.py:128-217, restated in beam_lm_cases.search) with only the blank and the frame's
shortlisted tokens as candidates, and the certificate that says when that step equals the full
one.  The reference finds a key's place in the stable sort from its dict's insertion order; here
every candidate carries its insertion position i * (V + 1) + (0 for the blank, tok + 1 otherwise)
explicitly, a key merges to its best score (the earliest position among equals, the reference's
strict `<`), and a key's own position is the smallest over all its candidates -- the structural
one included: live beam j's key is also reached by its parent beam `src` extended with j's tail
token, at src * (V + 1) + tail + 1, which the full search always offers, whether or not the tail
token is in the frame's shortlist.
"""

import numpy as np

f32 = np.float32


def log_softmax(x):
    """(x - max) - log(sum(exp(x - max))) in float32 (beam_lm_cases.log_softmax)."""
    x = np.asarray(x, f32)
    d = (x - x.max(axis=-1, keepdims=True)).astype(f32)
    return (d - np.log(np.exp(d).sum(axis=-1, keepdims=True, dtype=f32))).astype(f32)


def keys(lp):
    """Order-preserving uint64 keys of (log-probability, ~token) along the last axis: a larger key
    is a larger log-probability, or an equal one at a smaller token; -0.0 orders as +0.0."""
    lp = np.ascontiguousarray(np.asarray(lp, f32) + f32(0.0))
    u = lp.view(np.uint32)
    u = np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000)).astype(np.uint64)
    tok = np.arange(lp.shape[-1], dtype=np.uint64)
    return (u << np.uint64(32)) | (~tok & np.uint64(0xFFFFFFFF))


def shortlist(lp, K, blank):
    """lp (..., V) float32 -> (tok (..., K) int32, lp (..., K) float32, blank_lp (...) float32), K
    clamped to V - 1."""
    lp = np.asarray(lp, f32)
    V = lp.shape[-1]
    K = min(int(K), V - 1)
    k = keys(lp)
    k[..., blank] = 0  # below every key
    order = np.argsort(k, axis=-1)[..., ::-1][..., :K]
    return order.astype(np.int32), np.take_along_axis(lp, order, -1), lp[..., blank].copy()


def search(tok, lp, blank_lp, W, blank, V, lengths=None):
    """(beams, uncertified): per utterance [(tokens, score)] as beam_lm_cases.search returns them,
    and per utterance the number of frames whose step is not certified equal to the full search's.
    tok, lp (B, L, K) and blank_lp (B, L) as shortlist() gives them."""
    tok, lp, blank_lp = np.asarray(tok), np.asarray(lp, f32), np.asarray(blank_lp, f32)
    B, L, K = tok.shape
    VP = V + 1
    out, unc = [], []
    for b in range(B):
        beams = [((), 0.0, None)]  # (prefix, score, last), in sorted order
        bad = 0
        for t in range(L if lengths is None else int(lengths[b])):
            T, lpT, lpb = tok[b, t].tolist(), lp[b, t].tolist(), float(blank_lp[b, t])
            new = {}  # key -> [score, last, position of the score, position of the key]

            def offer(key, s, lt, pos):
                e = new.get(key)
                if e is None:
                    new[key] = [s, lt, pos, pos]
                    return
                e[3] = min(e[3], pos)
                if s is not None and (e[0] is None or s > e[0] or (s == e[0] and pos < e[2])):
                    e[0], e[1], e[2] = s, lt, pos

            for i, (prefix, score, last) in enumerate(beams):
                offer(prefix, score + lpb, blank, i * VP)
                for tk, v in zip(T, lpT):
                    offer(prefix if tk == last else prefix + (tk,), score + v, tk, i * VP + tk + 1)
            for j, (prefix, _, _) in enumerate(beams):  # structural positions
                if not prefix:
                    continue
                for i, (p, _, last) in enumerate(beams):
                    if p == prefix[:-1] and last != prefix[-1]:
                        offer(prefix, None, None, i * VP + prefix[-1] + 1)
            ranked = sorted(new.items(), key=lambda kv: (-kv[1][0], kv[1][3]))[:W]
            if K < V - 1:
                ok = len(ranked) == W
                if ok:
                    sigma, theta = ranked[-1][1][0], lpT[-1]
                    ok = all(sigma > s + theta for _, s, _ in beams)  # False with a NaN
                bad += not ok
            beams = [(key, e[0], e[1]) for key, e in ranked]
        out.append([(list(p), s) for p, s, _ in beams])
        unc.append(bad)
    return out, unc


# ------------------------------------------------------------------------------------- cases
def widths_and_sizes(W, V):
    """The K of a width's cases: W + 2, 2 W and 64, within 1..min(64, V - 1), without repeats."""
    out = []
    for K in (W + 2, 2 * W, 64):
        K = min(K, 64, V - 1)
        if K not in out:
            out.append(K)
    return out


HOST_SHAPES = [(5, 30), (40, 30), (200, 24)]  # V, L
HOST_WIDTHS = (1, 4, 8, 32)
HOST_SCALES = (1.0, 3.0, 6.0)

_built = {}


def host_cases():
    """Continuous cases of the host test: per (V, L, W, blank) a batch of five utterances of random
    logits (scales 1, 3, 6 in turn) with lengths [L, 1, 0, L - 1, 7], as float32 log-probabilities."""
    if "host" not in _built:
        out = []
        rng = np.random.default_rng(4242)
        for V, L in HOST_SHAPES:
            for W in HOST_WIDTHS:
                for blank in (0, V - 1):
                    scale = np.array([HOST_SCALES[n % 3] for n in range(5)], f32)[:, None, None]
                    lp = log_softmax(rng.standard_normal((5, L, V)).astype(f32) * scale)
                    lp.setflags(write=False)
                    out.append(dict(name=f"v{V}-l{L}-w{W}-b{blank}", V=V, L=L, W=W, blank=blank, lp=lp,
                                    lengths=[L, 1, 0, L - 1, 7]))
        _built["host"] = out
    return _built["host"]


# The device cases of the search: every (V, L, W) below, K from widths_and_sizes (W + 2 and 2 W), the
# blank first, last and inside in turn, logit scales 1..6 in turn.
DEVICE_V, DEVICE_L, DEVICE_W = (5, 64, 257, 1000), (1, 12, 64), (1, 2, 10, 32)
DEVICE_SEARCH = [(V, L, W, (0, V - 1, V // 2)[n % 3], (1.0, 2.0, 3.0, 6.0)[n % 4])
                 for n, (V, L, W) in enumerate((V, L, W) for V in DEVICE_V for L in DEVICE_L for W in DEVICE_W)]


def device_cases():
    if "dev" not in _built:
        out = []
        rng = np.random.default_rng(5151)
        for V, L, W, blank, scale in DEVICE_SEARCH:
            lg = (rng.standard_normal((1, L, V)) * scale).astype(f32)
            lg.setflags(write=False)
            for K in widths_and_sizes(W, V)[:2]:
                out.append(dict(name=f"v{V}-l{L}-w{W}-b{blank}-k{K}", kind="continuous", V=V, W=W, K=K, blank=blank,
                                logits=lg))
        _built["dev"] = out
    return _built["dev"]


TIE_EXTRA = [(33, 6, 7, 32), (257, 5, 10, 0)]  # V, L, W, blank: shortlists well below V - 1


def tie_cases():
    """test_beam_sweep's two tie families at its shapes and at TIE_EXTRA's, K = W + 2 and 2 W.  Where
    K < V - 1, frames whose candidates tie at the shortlist's tail cannot pass the strict
    certificate, so the exact search must take over."""
    if "tie" not in _built:
        from test_beam_sweep import TIE_SHAPES, two_level_rows, uniform_rows
        out = []
        for V, L, W, blank in TIE_SHAPES + TIE_EXTRA:
            for fam, rows in (("uniform", uniform_rows), ("twolevel", two_level_rows)):
                lg = rows(V, L).astype(f32)
                lg.setflags(write=False)
                for K in widths_and_sizes(W, V)[:2]:
                    out.append(dict(name=f"{fam}-v{V}-l{L}-w{W}-b{blank}-k{K}", kind="tie", V=V, W=W, K=K, blank=blank,
                                    logits=lg))
        _built["tie"] = out
    return _built["tie"]
