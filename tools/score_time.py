"""Times WER / CER scoring on one machine, device kernel against the host loop:
  (a) 2620 pairs, reference 20-400 characters, the hypothesis the reference with 10 % random edits;
  (b) 8 pairs of 9000 characters, same edit rate;
  (c) (a) plus one pair of (b),
each at character and at word level.  Per row: the kernel (ops.edit_counts on ids already on the
device) by device events, median of 20 after 3 warm-ups; cells per second; the wall time of
compute_cer / compute_wer(..., device=) with interning, upload, download and a final synchronise, median
of 20; the wall time of the host compute_cer / compute_wer (the default path), median of 3 -- for the
9000-character pairs at character level one pair is scored once and the figure scaled, as stated in the
table; whether the rates are equal as floats, and whether the (S, D, I) of a sample of the pairs equal
edit_counts_host.  Then the crossover: small batches of 30-character pairs, device wall against host
wall, which sets training.MIN_DEVICE_CELLS.
    python tools/score_time.py [--out profiles/score] [--quick]
writes <out>.json and <out>.md."""
import argparse
import json
import os
import random
import statistics
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "velocity-asr_amd"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from velocity_asr import _lib as L, ops, training as T  # noqa: E402

LETTERS = "etaoinshrdlucmfwyp"


def text(rng, n_chars):
    """Words of 1-9 letters separated by single spaces, n_chars characters in all."""
    out = []
    while len(out) < n_chars:
        out.extend(rng.choice(LETTERS) for _ in range(rng.randint(1, 9)))
        out.append(" ")
    return "".join(out[:n_chars]).rstrip() or "a"


def edit(rng, s, rate=0.1):
    out = []
    for ch in s:
        u = rng.random()
        if u < rate / 3:
            out.append(rng.choice(LETTERS))
        elif u < 2 * rate / 3:
            continue
        elif u < rate:
            out.extend((rng.choice(LETTERS + " "), ch))
        else:
            out.append(ch)
    return "".join(out)


def workload(name, quick):
    rng = random.Random(2620)
    short = [text(rng, rng.randint(20, 400)) for _ in range(262 if quick else 2620)]
    long_ = [text(rng, 900 if quick else 9000) for _ in range(8)]
    refs = dict(a=short, b=long_, c=short + long_[:1])[name]
    return [edit(rng, r) for r in refs], refs


def events(fn, reps=20, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b) * 1e3)
    return ts


def wall(fn, reps, warm):
    for _ in range(warm):
        fn()
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return ts


def spread(ts, nd=1):
    return dict(median=round(statistics.median(ts), nd), min=round(min(ts), nd), max=round(max(ts), nd))


def id_matrices(seqs_h, seqs_r, dev):
    ids = {}
    P = len(seqs_h)
    mh, mr = max(map(len, seqs_h)), max(map(len, seqs_r))
    H, R = np.zeros((P, mh), np.int32), np.zeros((P, mr), np.int32)
    for p, (h, r) in enumerate(zip(seqs_h, seqs_r)):
        H[p, :len(h)] = [ids.setdefault(x, len(ids)) for x in h]
        R[p, :len(r)] = [ids.setdefault(x, len(ids)) for x in r]
    t = lambda a: torch.from_numpy(np.asarray(a, np.int32)).to(dev)  # noqa: E731
    return t(H), t(R), t([len(h) for h in seqs_h]), t([len(r) for r in seqs_r])


def row(name, unit, dev, quick):
    preds, refs = workload(name, quick)
    split = (lambda s: s.lower().split()) if unit == "word" else (lambda s: list(s.lower()))
    rate = T.compute_wer if unit == "word" else T.compute_cer
    sh, sr = [split(p) for p in preds], [split(r) for r in refs]
    cells = sum(len(h) * len(r) for h, r in zip(sh, sr))
    H, R, hl, rl = id_matrices(sh, sr, dev)
    k = events(lambda: ops.edit_counts(H, R, hl, rl))
    host_val, dev_val = [], []
    w_dev = wall(lambda: dev_val.append(rate(preds, refs, device=dev)), 20, 3)
    note = ""
    if name == "b" and unit == "char" and not quick:
        t0 = time.perf_counter()
        one = rate(preds[:1], refs[:1])
        t1 = (time.perf_counter() - t0) * 1e3
        w_host = [t1 * len(refs)]
        same = one == rate(preds[:1], refs[:1], device=dev)
        note = f"host: one pair scored once ({t1 / 1e3:.1f} s) x {len(refs)}"
    else:
        w_host = wall(lambda: host_val.append(rate(preds, refs)), 1 if quick else 3, 0)
        same = host_val[-1] == dev_val[-1]
    sample = [p for p in range(0, len(refs), 20) if len(sh[p]) * len(sr[p]) <= 200000]
    dev_counts = T.error_counts([preds[p] for p in sample], [refs[p] for p in sample], unit, dev)
    host_counts = T.error_counts([preds[p] for p in sample], [refs[p] for p in sample], unit)
    return dict(workload=name, unit=unit, pairs=len(refs), cells=cells, longest=[max(map(len, sh)), max(map(len, sr))],
                kernel_us=spread(k), gcells_per_s=round(cells / statistics.median(k) / 1e3, 2),
                device_wall_ms=spread(w_dev, 2), host_wall_ms=spread(w_host, 1), note=note,
                host_over_device=round(statistics.median(w_host) / statistics.median(w_dev), 1),
                rates_equal=bool(same), sampled_pairs=len(sample), sampled_counts_equal=dev_counts == host_counts)


def crossover(dev):
    """Batches of P pairs of ~30 characters: where the device wall drops under the host wall."""
    rng = random.Random(7)
    refs = [text(rng, 30) for _ in range(256)]
    preds = [edit(rng, r) for r in refs]
    out = []
    for P in (1, 2, 4, 8, 16, 32, 64, 128, 256):
        p, r = preds[:P], refs[:P]
        cells = sum(len(a) * len(b) for a, b in zip(p, r))
        d = statistics.median(wall(lambda: T.compute_cer(p, r, device=dev), 20, 3))
        h = statistics.median(wall(lambda: T.compute_cer(p, r), 20, 1))
        out.append(dict(pairs=P, cells=cells, device_wall_ms=round(d, 3), host_wall_ms=round(h, 3)))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/score")
    ap.add_argument("--quick", action="store_true", help="a tenth of the sizes (a rehearsal, not a measurement)")
    a = ap.parse_args()
    L.require_device()
    dev = torch.device("cuda", 0)
    threshold = T.MIN_DEVICE_CELLS
    T.MIN_DEVICE_CELLS = 0  # time the device path itself, whatever the size
    rows = [row(n, u, dev, a.quick) for n in "abc" for u in ("char", "word")]
    cross = crossover(dev)
    first = next((c["cells"] for c in cross if c["device_wall_ms"] < c["host_wall_ms"]), None)
    lib = L.lib()
    out = dict(device=torch.cuda.get_device_name(0), quick=a.quick, wave_cols=lib.vasr_edit_wave_cols(),
               tile_cols=lib.vasr_edit_tile_cols(), rows=rows, crossover=cross, first_batch_cells_device_wins=first,
               min_device_cells=threshold)
    with open(a.out + ".json", "w") as f:
        json.dump(out, f, indent=1)

    def cell(s):
        return f"{s['median']} ({s['min']} - {s['max']})"

    md = ["# WER / CER scoring: the edit-distance kernel against the host loop", "",
          f"tools/score_time.py on {out['device']}" + (" (--quick: a rehearsal at a tenth of the sizes)" if a.quick else "")
          + ".  Workloads: (a) 2620 pairs, reference 20-400 characters, hypothesis = reference with 10 % random edits; "
          "(b) 8 pairs of 9000 characters; (c) (a) plus one pair of (b); each at character and word level.  Kernel: "
          "ops.edit_counts on ids already on the device, device events, median of 20 after 3 warm-ups (min - max).  Device "
          "wall: compute_cer / compute_wer(..., device=) with interning, upload, download and a final synchronise, median of "
          "20.  Host wall: the default compute_cer / compute_wer, median of 3 unless the note says otherwise.  Rates equal: "
          "the two floats compare equal; sampled counts: every 20th pair's (S, D, I) against edit_counts_host.", "",
          "| workload | unit | pairs | DP cells | kernel us | Gcells/s | device wall ms | host wall ms | host / device | "
          "rates equal | sampled counts equal | note |", "|---|---|---|---|---|---|---|---|---|---|---|---|"]
    for r in rows:
        md.append(f"| ({r['workload']}) | {r['unit']} | {r['pairs']} | {r['cells']} | {cell(r['kernel_us'])} | {r['gcells_per_s']} | "
                  f"{cell(r['device_wall_ms'])} | {cell(r['host_wall_ms'])} | {r['host_over_device']} | {r['rates_equal']} | "
                  f"{r['sampled_counts_equal']} ({r['sampled_pairs']}) | {r['note']} |")
    wins = all(r["host_over_device"] > 1.0 for r in rows)
    md += ["", "The device wall is " + ("lower than the host wall on every row." if wins else "NOT lower than the host wall "
           "on every row."), "", "## Crossover", "",
           "Batches of P pairs of about 30 characters, compute_cer wall with and without device=, median of 20:", "",
           "| pairs | DP cells | device wall ms | host wall ms |", "|---|---|---|---|"]
    md += [f"| {c['pairs']} | {c['cells']} | {c['device_wall_ms']} | {c['host_wall_ms']} |" for c in cross]
    md += ["", f"The smallest batch here at which the device wins has {first} cells; training.MIN_DEVICE_CELLS is "
           f"{threshold}: error_counts keeps a batch of fewer cells on the host."]
    with open(a.out + ".md", "w") as f:
        f.write("\n".join(md) + "\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
