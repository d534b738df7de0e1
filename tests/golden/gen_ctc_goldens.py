#!/usr/bin/env python
"""Generate tests/golden/ctc_loss.npz: the reference's CTCLoss on seeded cases.

Build-machine tool, like gen_goldens.py: run it with the REFERENCE package first on the path,

    PYTHONDONTWRITEBYTECODE=1 PYTHONPATH=<reference checkout> python tests/golden/gen_ctc_goldens.py

It runs the reference's velocity_asr.training.CTCLoss (F.log_softmax + nn.CTCLoss) on the CPU
with reduction none / mean / sum and both zero_infinity settings, and stores beside each result
an fp64 evaluation of the same lattice by the plain numpy loop below (ctc_nll_f64).  Logits are
not stored: every case regenerates them from its seed with torch.randn on the CPU (make_logits),
so the file stays a few kilobytes.  It also picks, per alignment case, the first seed whose fp64
Viterbi decisions all have a margin above ALIGN_MARGIN (viterbi_f64).

The helpers here (CASES, make_logits, ctc_nll_f64, viterbi_f64) are our own code and import
nothing of the reference; the tests import them to rebuild the inputs.  Only main() imports the
reference, and asserts that it did.
"""

import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "ctc_loss.npz")
BLANK = 0
ALIGN_MARGIN = 1e-3

# name: B, L, V, S (Smax), seed, and optionally
#   scale:   logits rescaled so that max |logit| = scale
#   gain:    logits multiplied by this
#   targets: explicit rows (else seeded, non-blank); ilen / tlen: per-utterance lengths
#   flat:    pass the targets 1-D, concatenated, with this many blanks embedded
CASES = {
    "l1_s0": dict(B=1, L=1, V=5, S=0, seed=101),
    "l1_s1": dict(B=1, L=1, V=5, S=1, seed=102),
    "l7_repeat": dict(B=3, L=7, V=5, S=3, seed=103, targets=[[2, 2, 3], [1, 4, 4], [3, 3, 3]]),
    "l33_v29": dict(B=4, L=33, V=29, S=12, seed=104),
    "l129_v1001": dict(B=2, L=129, V=1001, S=40, seed=105),
    "l501_v1000": dict(B=2, L=501, V=1000, S=120, seed=106),
    "s31": dict(B=2, L=140, V=50, S=31, seed=107),
    "s32": dict(B=2, L=140, V=50, S=32, seed=108),
    "s63": dict(B=2, L=140, V=50, S=63, seed=109),
    "s64": dict(B=2, L=140, V=50, S=64, seed=110),
    "s130": dict(B=2, L=140, V=50, S=130, seed=115, tlen=[130, 128]),
    "s280": dict(B=2, L=300, V=20, S=280, seed=116, tlen=[280, 257]),
    "pm80": dict(B=3, L=33, V=29, S=12, seed=111, scale=80.0),
    "ragged": dict(B=4, L=40, V=29, S=9, seed=112, ilen=[40, 17, 31, 5], tlen=[9, 0, 6, 2]),
    "infeasible": dict(B=2, L=4, V=5, S=4, seed=113, targets=[[1, 1, 1, 2], [1, 2, 0, 0]], tlen=[4, 2]),
    "flat_targets": dict(B=3, L=21, V=11, S=5, seed=114, tlen=[5, 3, 4], flat=3),
}
# forced-alignment cases: the seed is chosen by main() and stored as align/<name>/seed.
# l140_v50 has about 10^4 decisions between finite candidates; with unit-variance logits their
# smallest gap stayed below 1.1e-3 over 5000 seeds, so its logits are randn * 4 (gaps scale with it).
ALIGN_CASES = {
    "l33_v29": dict(B=1, L=33, V=29, S=12),
    "l140_v50": dict(B=1, L=140, V=50, S=64, gain=4.0),
}


def make_logits(c, seed=None):
    """(B, L, V) float32 logits of a case, from its seed."""
    g = torch.Generator().manual_seed(int(c["seed"] if seed is None else seed))
    x = torch.randn(c["B"], c["L"], c["V"], generator=g, dtype=torch.float32)
    if c.get("scale"):
        x = x * (float(c["scale"]) / float(x.abs().max()))
    if c.get("gain"):
        x = x * float(c["gain"])
    return x


def make_targets(c, seed=None):
    """(targets (B, S) int64 non-blank, input_lengths (B,), target_lengths (B,))."""
    B, S = c["B"], c["S"]
    if "targets" in c:
        tg = np.asarray(c["targets"], np.int64).reshape(B, S)
    else:
        rng = np.random.RandomState(int(c["seed"] if seed is None else seed) + 7)
        tg = rng.randint(1, c["V"], size=(B, S)).astype(np.int64)
    ilen = np.asarray(c.get("ilen", [c["L"]] * B), np.int64)
    tlen = np.asarray(c.get("tlen", [S] * B), np.int64)
    return tg, ilen, tlen


def flat_targets(c, tg, tlen):
    """The 1-D form of a `flat` case: rows concatenated up to their lengths, with c['flat'] blanks
    embedded at seeded positions (the reference drops them, training.py:95)."""
    cat = np.concatenate([tg[b, : tlen[b]] for b in range(c["B"])])
    pos = np.random.RandomState(c["seed"] + 11).randint(0, len(cat) + 1, size=c["flat"])
    return np.insert(cat, np.sort(pos), BLANK)


def log_softmax_f64(x):
    x = np.asarray(x, np.float64)
    m = x.max(-1, keepdims=True)
    return x - m - np.log(np.exp(x - m).sum(-1, keepdims=True))


def _extended(target, blank):
    ext = np.full(2 * len(target) + 1, blank, np.int64)
    ext[1::2] = target
    skip = np.zeros(len(ext), bool)  # s may be entered from s - 2
    skip[3::2] = ext[3::2] != ext[1:-2:2]
    return ext, skip


def ctc_nll_f64(logits, target, T, blank=BLANK):
    """-log p(target | logits[:T]) of ONE utterance in float64: plain alpha recursion over the
    extended label sequence (from s, s - 1, and s - 2 for a non-blank differing from s - 2)."""
    lp = log_softmax_f64(np.asarray(logits)[:T])
    ext, skip = _extended(np.asarray(target, np.int64), blank)
    S = len(ext)
    alpha = np.full(S, -np.inf)
    alpha[0] = lp[0, blank]
    if S > 1:
        alpha[1] = lp[0, ext[1]]
    with np.errstate(invalid="ignore", divide="ignore"):
        for t in range(1, T):
            a1 = np.concatenate(([-np.inf], alpha))[:S]
            a2 = np.where(skip, np.concatenate(([-np.inf, -np.inf], alpha))[:S], -np.inf)
            m = np.maximum(alpha, np.maximum(a1, a2))
            ms = np.where(np.isfinite(m), m, 0.0)
            alpha = np.where(np.isfinite(m), ms + np.log(np.exp(alpha - ms) + np.exp(a1 - ms) + np.exp(a2 - ms)), -np.inf)
            alpha = alpha + lp[t, ext]
    tail = alpha[-2:] if S > 1 else alpha[-1:]
    m = tail.max()
    if not np.isfinite(m):
        return np.inf
    return -(m + np.log(np.exp(tail - m).sum()))


def viterbi_f64(logits, target, T, blank=BLANK):
    """Best path of ONE utterance in float64 -> (score, frame_state (T,) target index or -1,
    margin): ties to the smaller source state; margin = the smallest gap between the best and the
    second-best finite candidate over every decision of the lattice (and the final one)."""
    lp = log_softmax_f64(np.asarray(logits)[:T])
    ext, skip = _extended(np.asarray(target, np.int64), blank)
    S = len(ext)
    v = np.full(S, -np.inf)
    v[0] = 0.0  # frame -1: frame 0 then follows from the same recursion
    back = np.zeros((T, S), np.int64)
    margin = np.inf
    for t in range(T):
        c = np.stack([v, np.concatenate(([-np.inf], v))[:S],
                      np.where(skip, np.concatenate(([-np.inf, -np.inf], v))[:S], -np.inf)])
        back[t] = np.argmax(c, axis=0)  # first maximum = smaller source state
        srt = np.sort(c, axis=0)
        both = np.isfinite(srt[1])
        if both.any():
            margin = min(margin, float((srt[2][both] - srt[1][both]).min()))
        v = c.max(axis=0) + lp[t, ext]
    tail = v[-2:] if S > 1 else v[-1:]
    if not np.isfinite(tail.max()):
        return -np.inf, np.full(T, -1, np.int64), margin
    if S > 1 and np.isfinite(tail).all():
        margin = min(margin, float(abs(tail[1] - tail[0])))
    s = S - 2 if (S > 1 and tail[0] >= tail[1]) else S - 1
    score = float(v[s])
    state = np.full(T, -1, np.int64)
    for t in range(T - 1, -1, -1):
        state[t] = s // 2 if s % 2 else -1
        s -= back[t, s]
    return score, state, margin


def case_f64(c, logits, tg, ilen, tlen):
    x = logits.numpy()
    return np.array([ctc_nll_f64(x[b], tg[b, : tlen[b]], int(ilen[b])) for b in range(c["B"])], np.float64)


def reduce_f64(nll, tlen, reduction, zero_infinity):
    nll = np.where(np.isinf(nll), 0.0, nll) if zero_infinity else nll
    if reduction == "none":
        return nll
    if reduction == "sum":
        return np.array(nll.sum())
    return np.array((nll / np.maximum(tlen, 1)).mean())


def main():
    import velocity_asr
    from velocity_asr import training as ref_training

    ours = os.path.realpath(os.path.join(HERE, "..", "..", "velocity-asr_amd"))
    assert not os.path.realpath(velocity_asr.__file__).startswith(ours) and hasattr(ref_training, "Trainer"), \
        f"{velocity_asr.__file__} is not the reference package: put the reference first on PYTHONPATH"

    out = {"names": np.array(sorted(CASES)), "align_names": np.array(sorted(ALIGN_CASES))}
    worst = 0.0
    for name, c in CASES.items():
        logits = make_logits(c)
        tg, ilen, tlen = make_targets(c)
        f64 = case_f64(c, logits, tg, ilen, tlen)
        targets = torch.from_numpy(flat_targets(c, tg, tlen) if c.get("flat") else tg)
        out[f"{name}/targets"] = tg.astype(np.int32)
        out[f"{name}/ilen"] = ilen.astype(np.int32)
        out[f"{name}/tlen"] = tlen.astype(np.int32)
        out[f"{name}/f64"] = f64
        for zi in (0, 1):
            for red in ("none", "mean", "sum"):
                loss = ref_training.CTCLoss(blank_token=BLANK, reduction=red, zero_infinity=bool(zi))
                with torch.no_grad():
                    got = loss(logits, targets, torch.from_numpy(ilen), torch.from_numpy(tlen))
                out[f"{name}/ref_{red}_zi{zi}"] = got.numpy().astype(np.float32)
                out[f"{name}/f64_{red}_zi{zi}"] = reduce_f64(f64, tlen, red, bool(zi))
        ref = out[f"{name}/ref_none_zi0"].astype(np.float64)
        ok = np.isfinite(f64)
        assert np.array_equal(np.isfinite(ref), ok), (name, ref, f64)
        rel = np.abs(ref[ok] - f64[ok]) / np.abs(f64[ok])
        worst = max(worst, float(rel.max()) if rel.size else 0.0)
        print(f"{name:14s} nll {np.array2string(f64, precision=4)}  ref-vs-f64 rel {rel.max() if rel.size else 0:.2e}")
    print(f"largest reference fp32 vs fp64 relative error over the fixture: {worst:.3e}")

    for name, c in ALIGN_CASES.items():
        for seed in range(1000, 6000):
            cc = dict(c, seed=seed)
            tg, ilen, tlen = make_targets(cc)
            score, state, margin = viterbi_f64(make_logits(cc).numpy()[0], tg[0], c["L"])
            if margin > 2 * ALIGN_MARGIN:  # twice the tested margin: no seed sits on the edge
                break
        else:
            raise AssertionError(f"{name}: no seed with every decision margin above {2 * ALIGN_MARGIN}")
        out[f"align/{name}/seed"] = np.array(seed, np.int64)
        out[f"align/{name}/score"] = np.array(score, np.float64)
        out[f"align/{name}/state"] = state.astype(np.int32)
        print(f"align {name}: seed {seed}, margin {margin:.3e}, score {score:.4f}")
    np.savez_compressed(OUT, **out)
    print(f"wrote {OUT} ({os.path.getsize(OUT)} bytes)")


if __name__ == "__main__":
    sys.exit(main())
