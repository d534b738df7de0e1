"""Cases shared by test_longform_host.py and test_longform_gpu.py: signals with silent stretches,
seeded parameter draws that satisfy the segmentation rule's validation, a scalar restatement of the
rule (plain Python floats, one loop per sum) and the properties every plan must have."""

import math

import numpy as np

BLK = 320
N_FFT = 400


def signal(n, seed, zero_stretches=3, scale=0.1):
    """float32 noise with a few stretches set to exact zeros (so block energies and scores tie)."""
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal(n) * scale).astype(np.float32)
    for _ in range(zero_stretches):
        if n < 2:
            break
        a = int(rng.integers(0, n))
        x[a:a + int(rng.integers(1, max(2, n // 4)))] = 0.0
    return x


def draw_params(rng):
    """(n, m, M, W) satisfying the validation: W even >= 2, mB >= W/2, MB >= 2 mB, m > N_FFT // 2."""
    W = 2 * int(rng.integers(1, 5))
    m = int(rng.integers(max(N_FFT // 2 + 1, (W // 2 - 1) * BLK + 1), 6 * BLK))
    mB = -(-m // BLK)
    M = int(rng.integers(2 * mB * BLK, 5 * mB * BLK))
    n = int(rng.integers(1, 12 * M))
    return n, m, M, W


def energy_ref(x):
    """E[k] with a Python float (float64) accumulator per block, samples ascending."""
    out = []
    for k in range(len(x) // BLK):
        acc = 0.0
        for v in x[k * BLK:(k + 1) * BLK].tolist():  # float32 -> float64 exactly
            acc += v * v
        out.append(acc)
    return out


def plan_ref(E, n, m, M, W):
    """The greedy loop of the rule on energies E, every sum written out."""
    MB, mB, nB = M // BLK, -(-m // BLK), n // BLK
    cuts, p = [], 0
    while n - p * BLK > M:
        best, best_c = math.inf, None
        for c in range(p + mB, min(p + MB, nB - mB) + 1):
            s = 0.0
            for k in range(c - W // 2, c + W // 2):
                s += E[k]
            if s != s:
                s = math.inf
            if best_c is None or s < best:
                best, best_c = s, c
        cuts.append(best_c * BLK)
        p = best_c
    return cuts


def check_plan(cuts, n, m, M):
    """The consequences of the rule that callers rely on."""
    edges = [0] + list(cuts) + [n]
    assert all(c % BLK == 0 for c in cuts), cuts
    assert all(a < b for a, b in zip(edges, edges[1:])), (cuts, n)  # a partition of [0, n)
    lens = [b - a for a, b in zip(edges, edges[1:])]
    if cuts:
        assert all(m <= v <= M for v in lens), (lens, m, M)  # the last segment included
    else:
        assert n <= M and lens == [n]
    assert len(cuts) <= (n // BLK) // (-(-m // BLK))
    if n == M + 1:
        assert len(cuts) == 1


def segments_of(n, cuts):
    edges = [0] + list(cuts) + [n]
    return [(a, b - a) for a, b in zip(edges, edges[1:])]
