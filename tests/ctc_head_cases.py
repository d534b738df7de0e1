"""Shared inputs and fp64 references of the logit-free CTC head loss tests (test_ctc_head_host.py,
test_ctc_head_gpu.py).

A case is a shape row of tests/golden/gen_ctc_goldens.py's CASES (plus v50000 and the gradient
tests' s280 as they stand there) with the logits replaced by a head: xn (B, L, K) the LayerNorm of
seeded normal rows, W ~ 0.3 N(0, 1) (V, K), b ~ 0.5 N(0, 1) (V,), all float32; targets and lengths
are the case's own (make_targets applies its ilen / tlen overrides).  pm80 scales W and b so that
the largest |logit| is 80.  Everything the references compute is float64 of these float32 inputs:
logits = xn W^T + b, then gen_ctc_goldens.ctc_nll_f64 / gen_ctc_grad_goldens.case_grad_f64, and
dX = G W, dW = G^T xn, db = sum G for the head's three gradients.
"""

import functools
import sys

import numpy as np
import torch

from conftest import GOLDEN

sys.path.insert(0, GOLDEN)
import gen_ctc_goldens as G  # noqa: E402
import gen_ctc_grad_goldens as GG  # noqa: E402

CASES = dict(G.CASES)
CASES["v50000"] = dict(B=4, L=64, V=50000, S=20, seed=201)

EPS = 2.0 ** -23


@functools.lru_cache(maxsize=None)
def head_case(name, K=192):
    """(c, xn (B, L, K), W (V, K), b (V,), targets (B, S) int64, ilen, tlen) as host tensors."""
    c = CASES[name]
    g = torch.Generator().manual_seed(int(c["seed"]) + 1000)
    rows = torch.randn(c["B"], c["L"], K, generator=g, dtype=torch.float32)
    xn = torch.nn.functional.layer_norm(rows, (K,))
    W = 0.3 * torch.randn(c["V"], K, generator=g, dtype=torch.float32)
    b = 0.5 * torch.randn(c["V"], generator=g, dtype=torch.float32)
    if c.get("scale"):
        top = float((xn.double() @ W.double().T + b.double()).abs().max())
        W, b = W * (float(c["scale"]) / top), b * (float(c["scale"]) / top)
    tg, ilen, tlen = G.make_targets(c)
    return c, xn, W, b, torch.from_numpy(tg), torch.from_numpy(ilen), torch.from_numpy(tlen)


@functools.lru_cache(maxsize=None)
def logits_f64(name, K=192):
    c, xn, W, b, *_ = head_case(name, K)
    x = xn.double().numpy() @ W.double().numpy().T + b.double().numpy()
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def nll_f64(name, K=192):
    c, _, _, _, tg, ilen, tlen = head_case(name, K)
    x = logits_f64(name, K)
    return np.array([G.ctc_nll_f64(x[b], tg[b, :int(tlen[b])].numpy(), int(ilen[b])) for b in range(c["B"])])


@functools.lru_cache(maxsize=None)
def emissions_f64(name, K=192):
    """(B, L, S + 1) log-softmax of the blank and the target tokens; NaN where unspecified."""
    c, _, _, _, tg, ilen, tlen = head_case(name, K)
    x = logits_f64(name, K)
    out = np.full((c["B"], c["L"], c["S"] + 1), np.nan)
    for b in range(c["B"]):
        T, n = int(ilen[b]), int(tlen[b])
        lp = G.log_softmax_f64(x[b, :T])
        out[b, :T, 0] = lp[:, G.BLANK]
        out[b, :T, 1:n + 1] = lp[:, tg[b, :n].numpy()]
    return out


@functools.lru_cache(maxsize=None)
def grads_f64(name, reduction="sum", zero_infinity=True, K=192):
    """(dX (B, L, K), dW (V, K), db (V,)) of the reduced loss (none = sum: all-ones upstream)."""
    c, xn, W, _, tg, ilen, tlen = head_case(name, K)
    g = GG.case_grad_f64(c, logits_f64(name, K), tg.numpy(), ilen.numpy(), tlen.numpy(),
                         "sum" if reduction == "none" else reduction, zero_infinity)
    g2 = g.reshape(-1, c["V"])
    x2 = xn.double().numpy().reshape(-1, K)
    return (g2 @ W.double().numpy()).reshape(c["B"], c["L"], K), g2.T @ x2, g2.sum(0)


def reference_grads(name, dtype, reduction="sum", zero_infinity=True, K=192):
    """torch CPU autograd of the reference's composition F.linear -> F.log_softmax -> nn.CTCLoss in
    `dtype` -> (nll (B,), dX, dW, db) as float64 numpy."""
    c, xn, W, b, tg, ilen, tlen = head_case(name, K)
    x, w, bb = (t.to(dtype).clone().requires_grad_(True) for t in (xn, W, b))
    lp = torch.nn.functional.log_softmax(torch.nn.functional.linear(x, w, bb), dim=-1)
    nll = torch.nn.CTCLoss(blank=G.BLANK, reduction="none", zero_infinity=zero_infinity)(
        lp.transpose(0, 1), tg, ilen, tlen)
    loss = (nll / tlen.clamp(min=1).to(dtype)).mean() if reduction == "mean" else nll.sum()
    loss.backward()
    return tuple(t.detach().double().numpy() for t in (nll, x.grad, w.grad, bb.grad))


def row_bounds(name, K=192):
    """The emission tolerance per (b, t): 2 delta_row + 8 * 2^-23 * max |logit| of the row, with
    delta_row = 2^-20 max_j (|a| . |w_j| + |b_j|), the tile GEMM's own rule (test_gemm_tiles.py)."""
    c, xn, W, b, *_ = head_case(name, K)
    mag = xn.double().abs().numpy() @ W.double().abs().numpy().T + b.double().abs().numpy()
    return 2.0 * 2.0 ** -20 * mag.max(-1) + 8.0 * EPS * np.abs(logits_f64(name, K)).max(-1)


def nll_bounds(name, K=192, lattice=True):
    """Per utterance: frames_b * (its largest emission bound) + 1.63e-6 |nll| (the lattice's measured
    bound of test_ctc_loss_gpu.py); lattice=False: the emission-derived term alone, for two device
    paths that run the same lattice kernel."""
    c, *_, ilen, _ = head_case(name, K)
    rb, nll = row_bounds(name, K), nll_f64(name, K)
    lat = 1.63e-6 if lattice else 0.0
    return np.array([int(ilen[b]) * rb[b, :max(int(ilen[b]), 1)].max() + lat * abs(nll[b]) if np.isfinite(nll[b])
                     else 0.0 for b in range(c["B"])])


def rel_err(got, want):
    """max |got - want| / max |want| (0 when both are all zero)."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    top = np.abs(want).max(initial=0.0)
    return float(np.abs(got - want).max(initial=0.0) / top) if top > 0 else float(np.abs(got).max(initial=0.0))
