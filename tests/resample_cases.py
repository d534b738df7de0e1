"""Cases shared by test_resample_host.py and test_resample_gpu.py: the rate pairs the device
resampler must serve, the clip lengths, and a sequential float64 restatement of the resampler
(taps built as tests/test_audio_io.py::_resample_ref builds them, then one ascending chain per
output over the zero-padded signal)."""

import math

import numpy as np

RATES = [8000, 11025, 12000, 16000, 22050, 24000, 32000, 44100, 48000, 88200, 96000, 176400, 192000]
TARGET = 16000
# every pair with a filter: the rates above -> 16 kHz except 16 kHz itself, and 16 -> 8 kHz
PAIRS = [(r, TARGET) for r in RATES if r != TARGET] + [(16000, 8000)]
LENGTHS = [1, 2, 37, 440, 441, 442, 3001, 20011]


def geometry(orig_sr, new_sr):
    """(orig, nw, width, klen) after the gcd reduction (torchaudio's Resample defaults)."""
    g = math.gcd(orig_sr, new_sr)
    o, nw = orig_sr // g, new_sr // g
    base = min(o, nw) * 0.99
    width = math.ceil(6 * o / base)
    return o, nw, width, 2 * width + o


def taps_ref(orig_sr, new_sr):
    """The (nw, klen) table in float64, rounded to float32 (as _resample_ref)."""
    o, nw, width, _ = geometry(orig_sr, new_sr)
    base = min(o, nw) * 0.99
    idx = np.arange(-width, width + o, dtype=np.float64)[None] / o
    t = (np.arange(0, -nw, -1, dtype=np.float64)[:, None] / nw + idx) * base
    t = np.clip(t, -6, 6)
    win = np.cos(t * math.pi / 6 / 2) ** 2
    t = t * math.pi
    with np.errstate(invalid="ignore", divide="ignore"):
        k = np.where(t == 0, 1.0, np.sin(t) / t)
    return (k * (win * (base / o))).astype(np.float32)


def out_length(n, orig_sr, new_sr):
    o, nw, _, _ = geometry(orig_sr, new_sr)
    return (nw * n + o - 1) // o


def chain(x, taps, orig, nw, width):
    """y[o] = float32(sum_k float64(taps[o % nw][k]) * float64(xp[(o // nw) * orig + k])), k ascending,
    xp the signal padded by `width` zeros in front and enough behind.  One float64 accumulator per
    output, updated once per tap: the loop over k is the order; numpy only runs the outputs side by
    side."""
    x = np.asarray(x, np.float32)
    klen = taps.shape[1]
    m = (nw * len(x) + orig - 1) // orig
    frames = (m + nw - 1) // nw
    xp = np.zeros(width + frames * orig + klen, np.float64)
    xp[width:width + len(x)] = x
    o = np.arange(m)
    start, row = (o // nw) * orig, o % nw
    t64 = taps.astype(np.float64)
    acc = np.zeros(m, np.float64)
    for k in range(klen):
        acc = acc + t64[row, k] * xp[start + k]
    return acc.astype(np.float32)


def downmix(x):
    """(C, n) float32 -> (n,): ascending float32 sum of the channels, then a true division by C."""
    x = np.asarray(x, np.float32)
    s = x[0].copy()
    for c in range(1, x.shape[0]):
        s = (s + x[c]).astype(np.float32)
    return (s / np.float32(x.shape[0])).astype(np.float32)


def signal(n, seed, channels=None):
    rng = np.random.default_rng(seed)
    shape = (n,) if channels is None else (channels, n)
    return (rng.standard_normal(shape) * 0.3).astype(np.float32)


def lengths_for_outputs(wants, orig_sr, new_sr):
    """Smallest input lengths that give `wants` outputs each; where no length gives a count (an odd
    one when the rate doubles) the next count up stands in, so both sides of an edge stay covered."""
    o, nw, _, _ = geometry(orig_sr, new_sr)
    ns = []
    for m in wants:
        n = max(1, (m * o) // nw - 1)
        while out_length(n, orig_sr, new_sr) < m:
            n += 1
        if n not in ns:
            ns.append(n)
    return ns
