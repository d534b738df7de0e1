#!/usr/bin/env python
"""Generate tests/golden/ctc_grad.npz: the gradient of the reference's CTCLoss on the seeded cases
of gen_ctc_goldens.py (CASES, make_logits, make_targets are imported from there; ctc_loss.npz is
not touched).

Build-machine tool, run with the REFERENCE package first on the path,

    PYTHONDONTWRITEBYTECODE=1 PYTHONPATH=<reference checkout> python tests/golden/gen_ctc_grad_goldens.py

Per case it runs the reference's velocity_asr.training.CTCLoss (F.log_softmax + nn.CTCLoss) on the
CPU with logits.requires_grad_(), in float32 and in float64, with reduction none (all-ones
upstream) / mean / sum and both zero_infinity settings, and stores

  <case>/e_ref            max |fp32 reference - fp64 reference| over the finite entries, sum reduction
                          (none gives the same gradient); <case>/e_ref_mean the same for mean
  <case>/nonfinite_zi{0,1} the number of non-finite entries of the fp64 reference, and for the
                          small cases the mask itself (<case>/mask_zi0)
  <case>/grad_{sum,mean}  the fp64 reference gradient (zero_infinity set), in full where
                          B L V <= FULL_LIMIT;
  for the larger cases, of the sum-reduction gradient: <case>/frames (B, NFRAMES) a seeded sample
  of frames of each utterance (the first and the last valid one among them), <case>/slots the
  blank-and-target columns by slot (B, NFRAMES, S + 1) at those frames, <case>/cols + <case>/other
  a seeded sample of up to 64 other columns at those frames, and <case>/rowsum (B, L) the sum of
  every row.

Random float64 values do not compress: the full gradients of all cases are about 11 MB, the
blank-and-target columns of l501_v1000 alone 0.97 MB.  FULL_LIMIT = 5000 and NFRAMES = 24 keep the
file near 0.4 MB.  The fixture only pins ctc_grad_f64 below to the reference; the GPU tests compare
the device gradient with ctc_grad_f64 over every entry of every case.

The helpers (ctc_grad_f64, case_grad_f64) are our own numpy and import nothing of the reference.
Only main() imports the reference, and asserts that it did.
"""

import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from gen_ctc_goldens import BLANK, CASES, flat_targets, log_softmax_f64, make_logits, make_targets  # noqa: E402

OUT = os.path.join(HERE, "ctc_grad.npz")
FULL_LIMIT = 5000
NFRAMES = 24
NCOLS = 64


def _lse(*xs):
    """Elementwise log(sum(exp(x))) of equally shaped arrays; -inf where every argument is."""
    x = np.stack(xs)
    m = x.max(axis=0)
    ms = np.where(np.isfinite(m), m, 0.0)
    with np.errstate(divide="ignore"):
        return np.where(np.isfinite(m), ms + np.log(np.exp(x - ms).sum(axis=0)), -np.inf)


def ctc_grad_f64(logits, target, T, blank=BLANK):
    """ONE utterance in float64 -> (nll, grad (L, V), occ (L, n + 1)).

    alpha and beta over the extended label sequence (both include the emission at t),
    gamma = exp(alpha + beta - e + nll); occ[t][0] sums gamma over the blank states and
    occ[t][1 + j] is label j's; grad[t] = softmax(logits[t]) - occ gathered per token for t < T and
    0 for t >= T: the gradient of nll with respect to the logits.  An infeasible target gives
    nll = inf, occ = 0 and NaN in the rows t < T of grad."""
    x = np.asarray(logits, np.float64)
    L, V = x.shape
    target = np.asarray(target, np.int64)
    n = len(target)
    S = 2 * n + 1
    grad = np.zeros((L, V))
    occ = np.zeros((L, n + 1))
    if T == 0:
        return (0.0 if n == 0 else np.inf), grad, occ
    lp = log_softmax_f64(x[:T])
    ext = np.full(S, blank, np.int64)
    ext[1::2] = target
    e = lp[:, ext]  # (T, S)
    fwd = np.zeros(S, bool)  # s may be entered from s - 2
    fwd[3::2] = ext[3::2] != ext[1:-2:2]
    bwd = np.zeros(S, bool)  # s may be left for s + 2
    bwd[:-2] = fwd[2:]
    ninf = -np.inf
    with np.errstate(invalid="ignore"):
        alpha = np.full((T, S), ninf)
        alpha[0, :2] = e[0, :2]
        for t in range(1, T):
            a = alpha[t - 1]
            a1 = np.concatenate(([ninf], a))[:S]
            a2 = np.where(fwd, np.concatenate(([ninf, ninf], a))[:S], ninf)
            alpha[t] = _lse(a, a1, a2) + e[t]
        beta = np.full((T, S), ninf)
        beta[T - 1, max(S - 2, 0):] = e[T - 1, max(S - 2, 0):]
        for t in range(T - 2, -1, -1):
            b = beta[t + 1]
            b1 = np.concatenate((b, [ninf]))[1:]
            b2 = np.where(bwd, np.concatenate((b, [ninf, ninf]))[2:], ninf)
            beta[t] = _lse(b, b1, b2) + e[t]
        ll = _lse(*alpha[T - 1, max(S - 2, 0):])
    if not np.isfinite(ll):
        grad[:T] = np.nan
        return np.inf, grad, occ
    nll = -float(ll)
    with np.errstate(invalid="ignore"):
        gamma = np.where(np.isfinite(alpha) & np.isfinite(beta), np.exp(alpha + beta - e + nll), 0.0)
    occ[:T, 0] = gamma[:, 0::2].sum(axis=1)
    occ[:T, 1:] = gamma[:, 1::2]
    grad[:T] = np.exp(lp)
    grad[:T, blank] -= occ[:T, 0]
    for j in range(n):  # repeated tokens share a column
        grad[:T, target[j]] -= occ[:T, 1 + j]
    return nll, grad, occ


def case_grad_f64(c, logits, tg, ilen, tlen, reduction="sum", zero_infinity=True):
    """(B, L, V) float64 gradient of a whole case's reduced loss, by ctc_grad_f64 per utterance:
    none (all-ones upstream) and sum scale every utterance by 1, mean by 1 / (B max(tlen, 1)); an
    infeasible utterance's gradient is 0 with zero_infinity and NaN (rows t < T) without."""
    x = np.asarray(logits, np.float64)
    out = np.zeros(x.shape)
    for b in range(c["B"]):
        nll, g, _ = ctc_grad_f64(x[b], tg[b, : tlen[b]], int(ilen[b]))
        if np.isinf(nll):
            g = np.zeros_like(g) if zero_infinity else g
        elif reduction == "mean":
            g = g / (c["B"] * max(int(tlen[b]), 1))
        out[b] = g
    return out


def sample_frames(c, ilen, seed):
    """(B, NFRAMES) frames of each utterance: its first and last valid frame and a seeded draw of
    the others (with repetition where it has fewer than NFRAMES)."""
    rng = np.random.RandomState(seed + 23)
    out = np.zeros((c["B"], NFRAMES), np.int64)
    for b in range(c["B"]):
        T = max(int(ilen[b]), 1)
        out[b] = np.sort(np.concatenate(([0, T - 1], rng.randint(0, T, size=NFRAMES - 2))))
    return out


def sample_columns(c, tg, seed):
    """Up to NCOLS vocabulary columns that are neither the blank nor any target of the case."""
    free = np.setdiff1d(np.arange(c["V"]), np.concatenate(([BLANK], np.asarray(tg).ravel())))
    rng = np.random.RandomState(seed + 29)
    return np.sort(rng.permutation(free)[:NCOLS]).astype(np.int64)


def by_slot(grad, tg, frames):
    """grad (B, L, V) at the sampled frames, gathered by slot: (B, NFRAMES, S + 1), slot 0 the blank."""
    B, S = tg.shape
    tok = np.concatenate((np.full((B, 1), BLANK, np.int64), tg), axis=1)
    return np.stack([grad[b][frames[b]][:, tok[b]] for b in range(B)])


def main():
    import velocity_asr
    from velocity_asr import training as ref_training

    ours = os.path.realpath(os.path.join(HERE, "..", "..", "velocity-asr_amd"))
    assert not os.path.realpath(velocity_asr.__file__).startswith(ours) and hasattr(ref_training, "Trainer"), \
        f"{velocity_asr.__file__} is not the reference package: put the reference first on PYTHONPATH"

    def reference(c, logits, targets, ilen, tlen, red, zi, dtype):
        x = logits.to(dtype).clone().requires_grad_()
        loss = ref_training.CTCLoss(blank_token=BLANK, reduction=red, zero_infinity=bool(zi))
        val = loss(x, targets, torch.from_numpy(ilen), torch.from_numpy(tlen))
        val.backward(torch.ones_like(val))
        return x.grad.numpy().astype(np.float64)

    out = {"names": np.array(sorted(CASES))}
    for name, c in CASES.items():
        logits = make_logits(c)
        tg, ilen, tlen = make_targets(c)
        targets = torch.from_numpy(flat_targets(c, tg, tlen) if c.get("flat") else tg)
        small = c["B"] * c["L"] * c["V"] <= FULL_LIMIT
        worst_own, none = 0.0, {}
        for red in ("none", "mean", "sum"):
            for zi in (0, 1):
                g32 = reference(c, logits, targets, ilen, tlen, red, zi, torch.float32)
                g64 = reference(c, logits, targets, ilen, tlen, red, zi, torch.float64)
                assert np.array_equal(np.isfinite(g32), np.isfinite(g64)), (name, red, zi)
                ok = np.isfinite(g64)
                e_ref = float(np.abs(g32 - g64)[ok].max()) if ok.any() else 0.0
                own = case_grad_f64(c, logits.numpy(), tg, ilen, tlen, "sum" if red == "none" else red, bool(zi))
                assert np.array_equal(np.isfinite(own), ok), (name, red, zi)
                worst_own = max(worst_own, float(np.abs(own - g64)[ok].max()) if ok.any() else 0.0)
                for b in range(c["B"]):  # padding rows are exact zeros in the reference too
                    assert not g64[b, int(ilen[b]):].any(), (name, red, zi, b)
                if red == "none":
                    none[zi] = g64
                    continue
                if red == "sum":
                    # all-ones upstream = sum: the same finite values and the same non-finite pattern
                    assert np.array_equal(np.isfinite(none[zi]), ok), (name, zi)
                    assert np.array_equal(g64[ok], none[zi][ok]), (name, zi)
                    out[f"{name}/nonfinite_zi{zi}"] = np.array(int((~ok).sum()), np.int64)
                    if zi == 0 and small:
                        out[f"{name}/mask_zi0"] = ~ok
                if zi == 0:
                    continue
                out[f"{name}/e_ref" + ("_mean" if red == "mean" else "")] = np.array(e_ref, np.float64)
                if small:
                    out[f"{name}/grad_{red}"] = g64
                elif red == "sum":
                    frames = sample_frames(c, ilen, c["seed"])
                    cols = sample_columns(c, tg, c["seed"])
                    out[f"{name}/frames"] = frames
                    out[f"{name}/slots"] = by_slot(g64, tg, frames)
                    out[f"{name}/cols"] = cols
                    out[f"{name}/other"] = np.stack([g64[b][frames[b]][:, cols] for b in range(c["B"])])
                    out[f"{name}/rowsum"] = g64.sum(axis=2)
        print(f"{name:14s} e_ref sum {float(out[f'{name}/e_ref']):.3e}  mean {float(out[f'{name}/e_ref_mean']):.3e}  "
              f"non-finite zi0 {int(out[f'{name}/nonfinite_zi0'])} zi1 {int(out[f'{name}/nonfinite_zi1'])}  "
              f"ctc_grad_f64 vs fp64 reference {worst_own:.3e}")
    np.savez_compressed(OUT, **out)
    print(f"wrote {OUT} ({os.path.getsize(OUT)} bytes)")


if __name__ == "__main__":
    sys.exit(main())
