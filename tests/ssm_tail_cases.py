"""Shared inputs, host references and row statistics of the kernel-level SSM block tail tests
(test_ssm_tail_host.py, test_ssm_tail_kernels_gpu.py).

The gated tail (csrc/ssm_tail.hip, vasr_ssm_block_tail_gated_f32 / _bf16) for D = 192, E = 384:

    z   = u Wz^T                    g  = yd * z / (1 + e^-z)
    x1  = g Wo^T + x                h  = LayerNorm(x1) * ln_w + ln_b
    f   = gelu_erf(h W1^T + b1)     out = f W2^T + b2 + x1

and the ungated tail (vasr_ssm_block_tail_f32 / _bf16) is the same from g on.  Parameters follow
test_ssm_tail.py's _params (weights / sqrt(fan-in), LayerNorm weight 1 + 0.1 n, biases 0.1 n) with wz
(E, D) added; inputs yd (M, E), u (M, D), x (M, D) are standard normal from a seed per case.

staged=True is the bf16 kernels' arithmetic: the four weights are the bf16 parameters, and u, g, h and
f -- the A operands of the Wz, Wo, W1 and W2 products -- are rounded to bf16 (nearest even, from their
float32 value) where the kernel rounds them: the MFMA operand at read_u, gate_split_store<., 1> (the
ungated kernel: split_store8<1> of the g it is given), split_store<1> of h and split_store<1> of f.
Everything else (accumulation, LayerNorm, biases, residuals) the kernels keep in float32.

Two evaluations of that algorithm: ref_f64 in float64 numpy, ref_f32 in float32 on the CPU with torch's
own matmul, layer_norm, gelu and sigmoid (another summation order).  Unstaged they agree to fp32
rounding.  Staged they agree to fp32 rounding on most rows; on a few per cent of rows an h, f or g
value within float32 error of a bf16 tie rounds the other way in one of them and the change (one bf16
ulp of one operand) spreads over the output row.  The bf16 kernels are a third evaluation of the same
algorithm, so they are held to the pair's own figures (pair_stats, conditions): what a correct
reordering of the float32 operations does, measured, times this project's factor 4.
"""

import functools
import math

import numpy as np
import torch

D, E = 192, 384
EPS = 1e-5
ATOL, RTOL = 2e-5, 2e-5  # the project's fp32 bar (test_tail_matches_fp64): atol * max(1, max |ref|), rtol
FACTOR = 4.0             # same algorithm, another operation order (test_scan_grad_gpu.py, test_ctc_grad_gpu.py)

# 1, 1, 1, 2, 2, 3, 4, 9, 16 and 18 tiles of 32 rows: grids below 8 tiles, nblk % 8 in {0, 1, 2}, ragged
# last tiles of 1, 31 and 1 rows
MS = (1, 31, 32, 33, 63, 65, 100, 257, 481, 545)
SEEDS = (0, 1, 2)        # input seeds per M of the bf16 tests
PARAM_SEED = 7
WEIGHTS = ("wz", "wo", "w1", "w2")


def gelu_f64(x):
    from scipy.special import erf
    return 0.5 * x * (1.0 + erf(x / math.sqrt(2.0)))


def bf16_round(a):
    """float64 / float32 array -> its float32 value rounded to bf16 (nearest even), as float64."""
    return torch.from_numpy(np.array(a, dtype=np.float32)).to(torch.bfloat16).double().numpy()


@functools.lru_cache(maxsize=None)
def params(seed=PARAM_SEED):
    """test_ssm_tail.py's _params (the same draws in the same order) plus wz; read-only float32."""
    rng = np.random.default_rng(seed)
    f = lambda *s, sc=1.0: (rng.standard_normal(s) * sc).astype(np.float32)  # noqa: E731
    P = dict(wo=f(D, E, sc=1 / math.sqrt(E)), ln_w=(1 + 0.1 * rng.standard_normal(D)).astype(np.float32),
             ln_b=f(D, sc=0.1), w1=f(E, D, sc=1 / math.sqrt(D)), b1=f(E, sc=0.1),
             w2=f(D, E, sc=1 / math.sqrt(E)), b2=f(D, sc=0.1))
    P["wz"] = f(E, D, sc=1 / math.sqrt(D))
    for v in P.values():
        v.setflags(write=False)
    return P


@functools.lru_cache(maxsize=None)
def inputs(M, seed=0):
    """(yd (M, E), u (M, D), x (M, D)) float32, read-only; the ungated tail takes yd as its g."""
    rng = np.random.default_rng([M, seed, 20])
    out = tuple(rng.standard_normal((M, n)).astype(np.float32) for n in (E, D, D))
    for a in out:
        a.setflags(write=False)
    return out


def ref_f64(yd, u, x, P, staged):
    """The gated tail in float64 (u None: the ungated tail of g = yd)."""
    r = bf16_round if staged else (lambda a: np.asarray(a, np.float64))
    W = {k: r(P[k]) for k in WEIGHTS}
    g = np.asarray(yd, np.float64)
    if u is not None:
        z = r(u) @ W["wz"].T
        g = g * z / (1.0 + np.exp(-z))
    x1 = r(g) @ W["wo"].T + np.asarray(x, np.float64)
    mu = x1.mean(-1, keepdims=True)
    var = ((x1 - mu) ** 2).mean(-1, keepdims=True)
    h = (x1 - mu) / np.sqrt(var + EPS) * P["ln_w"].astype(np.float64) + P["ln_b"].astype(np.float64)
    f = gelu_f64(r(h) @ W["w1"].T + P["b1"].astype(np.float64))
    return r(f) @ W["w2"].T + P["b2"].astype(np.float64) + x1


def ref_f32(yd, u, x, P, staged):
    """The same algorithm in float32 with torch's CPU kernels; float64 numpy of the float32 result."""
    F = torch.nn.functional
    t = lambda a: torch.from_numpy(np.array(a, dtype=np.float32))  # noqa: E731
    r = (lambda a: a.to(torch.bfloat16).float()) if staged else (lambda a: a)
    W = {k: r(t(P[k])) for k in WEIGHTS}
    g = t(yd)
    if u is not None:
        z = r(t(u)) @ W["wz"].T
        g = g * (z * torch.sigmoid(z))
    x1 = r(g) @ W["wo"].T + t(x)
    h = F.layer_norm(x1, (D,), t(P["ln_w"]), t(P["ln_b"]), EPS)
    f = F.gelu(F.linear(r(h), W["w1"], t(P["b1"])))
    return (F.linear(r(f), W["w2"], t(P["b2"])) + x1).double().numpy()


@functools.lru_cache(maxsize=None)
def case_ref(M, seed, gated, staged, f32=False):
    """ref_f64 (f32: ref_f32) of inputs(M, seed) under params(); computed once, read-only."""
    yd, u, x = inputs(M, seed)
    out = (ref_f32 if f32 else ref_f64)(yd, u if gated else None, x, params(), staged)
    out.setflags(write=False)
    return out


def fp32_bar(ref):
    """Elementwise |got - ref| allowed by the fp32 bar: assert_allclose(atol = ATOL max(1, max |ref|), rtol)."""
    a = np.abs(np.asarray(ref, np.float64))
    return ATOL * max(1.0, float(a.max(initial=0.0))) + RTOL * a


def row_errors(got, ref):
    """(e_row, loose): max_j |got - ref| per row and whether the row misses the fp32 bar.  A value that
    is not finite counts as an infinite error."""
    got = np.asarray(got, np.float64)
    d = np.where(np.isfinite(got), np.abs(got - ref), np.inf)
    return d.max(-1), (d > fp32_bar(ref)).any(-1)


@functools.lru_cache(maxsize=None)
def pair_stats(gated):
    """The reference pair's own staged figures over MS x SEEDS: dict(E_ref = largest row error of
    ref_f32 against ref_f64, s_ref = share of loose rows, tight = largest error on the other rows,
    rows, per = {(M, seed): (e_row, loose)})."""
    per = {(M, s): row_errors(case_ref(M, s, gated, True, True), case_ref(M, s, gated, True)) for M in MS for s in SEEDS}
    return summarise(per)


def summarise(per):
    e = np.concatenate([v[0] for v in per.values()])
    loose = np.concatenate([v[1] for v in per.values()])
    return dict(E_ref=float(e.max()), s_ref=float(loose.mean()), rows=int(e.size), loose_rows=int(loose.sum()),
                tight=float(e[~loose].max(initial=0.0)), per=per)


def conditions(per, pair):
    """The three row conditions a bf16 kernel's outputs meet, for per = {(M, seed): (e_row, loose)} over
    MS x SEEDS against ref_f64(staged=True) and pair = pair_stats(gated).  Returns (failures, stats): a
    list of messages that name the condition, the case, the row and its 32-row tile -- empty when all
    hold -- and summarise(per).

    (a) every row: e_row <= 4 E_ref;
    (b) the pooled share of loose rows <= 4 s_ref;
    (c) no row position of a case is loose under all of its seeds (a rounding flip depends on the
        values, an indexing error on the position)."""
    st = summarise(per)
    fails = []
    cap = FACTOR * pair["E_ref"]
    for (M, s), (e, _) in per.items():
        bad = np.flatnonzero(~(e <= cap))
        if bad.size:
            w = bad[np.argmax(e[bad])]
            fails.append(f"(a) M={M} seed={s}: {bad.size} rows over 4 E_ref = {cap:.3g}; worst row {w} "
                         f"(tile {w // 32}, row {w % 32} of it) e_row = {e[w]:.3g}; rows {bad[:8].tolist()}")
    if st["s_ref"] > FACTOR * pair["s_ref"]:
        fails.append(f"(b) loose share {st['s_ref']:.4f} ({st['loose_rows']} of {st['rows']} rows) over "
                     f"4 s_ref = {FACTOR * pair['s_ref']:.4f}")
    for M in sorted({k[0] for k in per}):
        always = np.logical_and.reduce([v[1] for k, v in per.items() if k[0] == M])
        if always.any():
            rows = np.flatnonzero(always)
            fails.append(f"(c) M={M}: rows {rows[:8].tolist()} (tiles {sorted(set((rows // 32).tolist()))[:8]}) "
                         f"loose under every seed")
    return fails, st
