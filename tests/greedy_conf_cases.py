"""Shared host references of the scored greedy decode tests (test_greedy_conf_host.py,
test_greedy_conf_gpu.py).

collapse_conf_ref restates what vasr_ctc_collapse_conf computes, in float64: for each utterance the
kept tokens of the collapse with their [start, end) runs, the sum and the minimum of the frame
log-probabilities over each run, and the sum over the utterance's frames.  collapse_conf_brute gets
the same from the CPU oracle's ctc_greedy_decode_with_timestamps (one-hot logits of the predictions)
and a loop over its spans: the two are written independently and test_greedy_conf_host.py compares them.
"""

import numpy as np

from oracle import velocity_ref as R

EPS = 2.0 ** -23


def clamp_frames(frames, B, L):
    return [L] * B if frames is None else [min(max(int(f), 0), L) for f in frames]


def collapse_conf_ref(pred, logp, blank=0, frames=None):
    """pred (B, L) ints, logp (B, L) floats -> per utterance a dict(tokens, spans, sum, min, path,
    abs): sum / min / path float64, abs = the sum of |lp| over the same terms as sum (per token)
    and abs_path over the path's (the fp32 summation bounds scale with them)."""
    pred = np.asarray(pred)
    logp = np.asarray(logp, dtype=np.float64)
    B, L = pred.shape
    out = []
    for b, n in enumerate(clamp_frames(frames, B, L)):
        p, lp = pred[b, :n], logp[b, :n]
        # a run starts where the value changes; a kept token is a run of a non-blank value
        starts = np.flatnonzero(np.r_[True, p[1:] != p[:-1]]) if n else np.zeros(0, np.int64)
        ends = np.r_[starts[1:], n] if n else starts
        keep = p[starts] != blank if n else np.zeros(0, bool)
        spans = [(int(s), int(e)) for s, e in zip(starts[keep], ends[keep])]
        out.append(dict(tokens=[int(t) for t in p[starts[keep]]] if n else [], spans=spans,
                        sum=np.array([lp[s:e].sum() for s, e in spans]),
                        min=np.array([lp[s:e].min() for s, e in spans]),
                        abs=np.array([np.abs(lp[s:e]).sum() for s, e in spans]),
                        path=float(lp.sum()), abs_path=float(np.abs(lp).sum())))
    return out


def collapse_conf_brute(pred, logp, blank=0, frames=None):
    """The same values by the oracle's timestamped greedy decode and plain loops."""
    pred = np.asarray(pred)
    B, L = pred.shape
    V = int(max(pred.max(initial=0), blank)) + 1
    out = []
    for b, n in enumerate(clamp_frames(frames, B, L)):
        onehot = np.zeros((1, n, V), dtype=np.float32)
        onehot[0, np.arange(n), pred[b, :n]] = 1.0
        tokens, spans = R.ctc_greedy_decode_with_timestamps(onehot, blank)[0] if n else ([], [])
        sums, mins = [], []
        for s, e in spans:
            tot, low = 0.0, float("inf")
            for t in range(s, e):
                tot += float(logp[b][t])
                low = min(low, float(logp[b][t]))
            sums.append(tot)
            mins.append(low)
        path = 0.0
        for t in range(n):
            path += float(logp[b][t])
        out.append(dict(tokens=list(tokens), spans=[(int(s), int(e)) for s, e in spans], sum=np.array(sums),
                        min=np.array(mins), path=path))
    return out


def row_bounds(a, w, b):
    """ctc_head_cases.row_bounds' rule on explicit operands (float32 host tensors a (M, K), w (V, K), b (V,)
    or None) -> (bound (M,), logits float64 (M, V)): 2 delta_row + 8 * 2^-23 * max |logit|,
    delta_row = 2^-20 max_j (|a| . |w_j| + |b_j|)."""
    a64, w64 = a.double().numpy(), w.double().numpy()
    b64 = np.zeros(w64.shape[0]) if b is None else b.double().numpy()
    x = a64 @ w64.T + b64
    with np.errstate(invalid="ignore"):
        mag = np.abs(a64) @ np.abs(w64).T + np.where(np.isfinite(b64), np.abs(b64), 0.0)
        top = np.where(np.isfinite(x), np.abs(x), 0.0).max(-1)
    return 2.0 * 2.0 ** -20 * mag.max(-1) + 8.0 * EPS * top, x


def log_softmax_at(x64, idx):
    """float64 log-softmax of rows x64 (M, V) at column idx[m] of each row."""
    m = x64.max(-1, keepdims=True)
    lse = np.log(np.exp(x64 - m).sum(-1)) + m[:, 0]
    return x64[np.arange(x64.shape[0]), idx] - lse
