"""Times the device alignment (vasr_edit_align_i32) on tools/score_time.py's workloads:
  (a) 2620 pairs, reference 20-400 characters, the hypothesis the reference with 10 % random edits;
  (b) 8 pairs of 9000 characters, same edit rate;
  (c) (a) plus one pair of (b),
each at character and at word level.  Per row, by device events, median of 20 after 3 warm-ups, on ids, lengths
and buffers already on the device: the sweeps that keep the choice table (VASR_EDIT_ALIGN_STAGE=1), the walk
(=2, over the table the call before left), and the counts-only entry; the counts-only entry again from
--parent-lib (the library of the parent commit) in processes of its own, alternating with this tree's, two
rounds.  Then the wall time of error_alignments(..., device=) with interning, upload, download and building
the Alignment objects, median of 5, and of the host path: median of 1 (it is seconds to minutes long), and
for the 9000-character pairs at character level one pair aligned once and the figure scaled, as the table
says; whether every path equals the host's.  Then the crossover: small batches of 30-character pairs,
device wall against host wall, which sets training.ALIGN_MIN_DEVICE_CELLS.
    python tools/align_time.py [--out profiles/align] [--parent-lib FILE] [--quick]
writes <out>.json and <out>.md.  A library built with -DVASR_EDIT_BACK_ROWS=1 -DVASR_EDIT_BACK_STRIPS=1
(VASR_LIB=...) times the other form of the walk, one dependent load per operation: --walk-only prints it."""
import argparse
import ctypes
import json
import os
import statistics
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "velocity-asr_amd"))
sys.path.insert(0, HERE)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from score_time import events, id_matrices, spread, wall, workload, text, edit  # noqa: E402

ROWS = [(n, u) for n in "abc" for u in ("char", "word")]


def items(name, unit, quick):
    preds, refs = workload(name, quick)
    split = (lambda s: s.lower().split()) if unit == "word" else (lambda s: list(s.lower()))
    return preds, refs, [split(p) for p in preds], [split(r) for r in refs]


def counts_worker(lib_path, quick):
    """Counts-only kernel times of the library at lib_path, by its C entry alone (the parent's has no more)."""
    lib = ctypes.CDLL(lib_path)
    c_p, c_i64, c_int = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int
    lib.vasr_edit_counts_i32.argtypes = [c_p, c_i64, c_p, c_int, c_p, c_i64, c_p, c_int, c_int, c_p, c_p, c_i64, c_p]
    lib.vasr_edit_workspace_bytes.argtypes = [c_int] * 3
    lib.vasr_edit_workspace_bytes.restype = c_i64
    dev = torch.device("cuda", 0)
    out = {}
    for name, unit in ROWS:
        _, _, sh, sr = items(name, unit, quick)
        H, R, hl, rl = id_matrices(sh, sr, dev)
        P, mh, mr = H.shape[0], H.shape[1], R.shape[1]
        need = lib.vasr_edit_workspace_bytes(P, mh, mr)
        ws = torch.empty((max(need, 8) // 8,), device=dev, dtype=torch.int64)
        counts = torch.empty((P, 3), device=dev, dtype=torch.int32)
        stream = torch.cuda.current_stream().cuda_stream

        def run():
            rc = lib.vasr_edit_counts_i32(H.data_ptr(), mh, hl.data_ptr(), mh, R.data_ptr(), mr, rl.data_ptr(), mr, P,
                                          counts.data_ptr(), ws.data_ptr() if need else None, need, stream)
            assert rc == 0
        out[f"{name}/{unit}"] = spread(events(run))
    return out


def stages(sh, sr, dev):
    """Sweeps-with-table, walk and counts-only times of one workload through the C entry, on persistent buffers."""
    from velocity_asr import _lib as L
    lib = L.lib()
    H, R, hl, rl = id_matrices(sh, sr, dev)
    P, mh, mr = H.shape[0], H.shape[1], R.shape[1]
    offs, used = [], 0
    for h, r in zip(sh, sr):
        offs.append(used)
        used += -(-lib.vasr_edit_align_table_bytes(len(h), len(r)) // 16) * 16
    need = lib.vasr_edit_workspace_bytes(P, mh, mr)
    ws = torch.empty((max(need, 8) // 8,), device=dev, dtype=torch.int64)
    table = torch.empty((max(used, 16),), device=dev, dtype=torch.uint8)
    counts = torch.empty((P, 3), device=dev, dtype=torch.int32)
    ops = torch.empty((P, mh + mr), device=dev, dtype=torch.uint8)
    ops_len = torch.empty((P,), device=dev, dtype=torch.int32)
    offd = torch.tensor(offs, dtype=torch.int64).to(dev)
    stream = torch.cuda.current_stream().cuda_stream

    def align():
        L.check(lib.vasr_edit_align_i32(H.data_ptr(), mh, hl.data_ptr(), mh, R.data_ptr(), mr, rl.data_ptr(), mr, P,
                                        counts.data_ptr(), ops.data_ptr(), mh + mr, ops_len.data_ptr(), offd.data_ptr(),
                                        table.data_ptr(), used, ws.data_ptr() if need else None, need, stream), "align")

    def count():
        L.check(lib.vasr_edit_counts_i32(H.data_ptr(), mh, hl.data_ptr(), mh, R.data_ptr(), mr, rl.data_ptr(), mr, P,
                                         counts.data_ptr(), ws.data_ptr() if need else None, need, stream), "counts")
    out = {}
    os.environ.pop("VASR_EDIT_ALIGN_STAGE", None)
    out["both_us"] = spread(events(align))
    for key, stage in (("sweep_us", "1"), ("walk_us", "2")):   # the walk reads what the full calls above left
        os.environ["VASR_EDIT_ALIGN_STAGE"] = stage
        out[key] = spread(events(align))
    os.environ.pop("VASR_EDIT_ALIGN_STAGE", None)
    out["counts_us"] = spread(events(count))
    out["table_bytes"] = used
    return out


def row(name, unit, dev, quick, walk_only):
    from velocity_asr import training as T
    preds, refs, sh, sr = items(name, unit, quick)
    cells = sum(len(h) * len(r) for h, r in zip(sh, sr))
    r = dict(workload=name, unit=unit, pairs=len(refs), cells=cells, **stages(sh, sr, dev))
    if walk_only:
        return r
    got = []
    w_dev = wall(lambda: got.append(T.error_alignments(preds, refs, unit, device=dev)), 5, 1)
    note = ""
    if name == "b" and unit == "char" and not quick:
        t0 = time.perf_counter()
        one = T.edit_alignment_host(sh[0], sr[0])
        t1 = (time.perf_counter() - t0) * 1e3
        w_host = [t1 * len(refs)]
        same = one == got[-1][0].ops
        note = f"host: one pair aligned once ({t1 / 1e3:.1f} s) x {len(refs)}; that pair's path compared"
    else:
        t0 = time.perf_counter()
        host = T.error_alignments(preds, refs, unit)
        w_host = [(time.perf_counter() - t0) * 1e3]
        same = host == got[-1]
    k = statistics.median
    r.update(device_wall_ms=spread(w_dev, 2), host_wall_ms=spread(w_host, 1), note=note,
             host_over_device=round(k(w_host) / k(w_dev), 1), paths_equal=bool(same),
             align_over_counts=round((r["sweep_us"]["median"] + r["walk_us"]["median"]) / r["counts_us"]["median"], 2))
    return r


def crossover(dev):
    from velocity_asr import training as T
    import random
    rng = random.Random(7)
    refs = [text(rng, 30) for _ in range(256)]
    preds = [edit(rng, r) for r in refs]
    out = []
    for P in (1, 2, 4, 8, 16, 32, 64, 128, 256):
        p, r = preds[:P], refs[:P]
        cells = sum(len(a) * len(b) for a, b in zip(p, r))
        d = statistics.median(wall(lambda: T.error_alignments(p, r, "char", device=dev), 20, 3))
        h = statistics.median(wall(lambda: T.error_alignments(p, r, "char"), 20, 1))
        out.append(dict(pairs=P, cells=cells, device_wall_ms=round(d, 3), host_wall_ms=round(h, 3)))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/align")
    ap.add_argument("--parent-lib", default=None, help="libvasr_hip.so of the parent commit, for the counts-only comparison")
    ap.add_argument("--quick", action="store_true", help="a tenth of the sizes (a rehearsal, not a measurement)")
    ap.add_argument("--walk-only", action="store_true", help="kernel times only, printed, nothing written")
    ap.add_argument("--counts-worker", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.counts_worker:
        print(json.dumps(counts_worker(a.counts_worker, a.quick)))
        return
    from velocity_asr import _lib as L, training as T
    L.require_device()
    dev = torch.device("cuda", 0)
    threshold = T.ALIGN_MIN_DEVICE_CELLS
    T.ALIGN_MIN_DEVICE_CELLS = 0  # time the device path itself, whatever the size
    rows = []
    for n, u in ROWS:
        rows.append(row(n, u, dev, a.quick, a.walk_only))
        print(f"({n}) {u} done", file=sys.stderr, flush=True)
    if a.walk_only:
        print(json.dumps(dict(lib=L.LIB_PATH, rows=rows)))
        return
    cross = crossover(dev)
    first = next((c["cells"] for c in cross if c["device_wall_ms"] < c["host_wall_ms"]), None)
    rounds = []
    if a.parent_lib:
        for _ in range(2):
            for which, path in (("tree", L.LIB_PATH), ("parent", a.parent_lib)):
                cmd = [sys.executable, os.path.abspath(__file__), "--counts-worker", path] + (["--quick"] if a.quick else [])
                res = subprocess.run(cmd, check=True, capture_output=True, text=True, timeout=600)
                rounds.append(dict(lib=which, kernel_us=json.loads(res.stdout.strip().splitlines()[-1])))
    out = dict(device=torch.cuda.get_device_name(0), quick=a.quick, rows=rows, crossover=cross,
               first_batch_cells_device_wins=first, align_min_device_cells=threshold, counts_rounds=rounds)
    with open(a.out + ".json", "w") as f:
        json.dump(out, f, indent=1)

    def cell(s):
        return f"{s['median']} ({s['min']} - {s['max']})"

    md = ["# Alignment on the device: sweeps with the choice table, the walk, and the host path", "",
          f"tools/align_time.py on {out['device']}" + (" (--quick: a rehearsal at a tenth of the sizes)" if a.quick else "")
          + ".  Workloads as in profiles/score.md.  Kernel columns: the C entries on ids and buffers already on the device, "
          "device events, median of 20 after 3 warm-ups (min - max), in microseconds: the two sweeps that keep the choice "
          "table, the walk, both in one call, and the counts-only entry of this tree.  (sweeps + walk) / counts is what the "
          "alignment costs over the counts.  Device wall: error_alignments(..., device=) with interning, upload, download "
          "and building the Alignment objects, median of 5.  Host wall: the same call without a device, once, unless the "
          "note says otherwise.", "",
          "| workload | unit | pairs | DP cells | table MB | sweeps us | walk us | one call us | counts-only us | "
          "(sweeps + walk) / counts | device wall ms | host wall ms | host / device | paths equal | note |",
          "|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|"]
    for r in rows:
        md.append(f"| ({r['workload']}) | {r['unit']} | {r['pairs']} | {r['cells']} | {r['table_bytes'] / 1e6:.1f} | "
                  f"{cell(r['sweep_us'])} | {cell(r['walk_us'])} | {cell(r['both_us'])} | {cell(r['counts_us'])} | "
                  f"{r['align_over_counts']} | {cell(r['device_wall_ms'])} | {cell(r['host_wall_ms'])} | "
                  f"{r['host_over_device']} | {r['paths_equal']} | {r['note']} |")
    md += ["", "Paths are " + ("equal on every row." if all(r["paths_equal"] for r in rows) else "NOT equal on every row."),
           "The device wall is " + ("lower than the host wall on every row." if all(r["host_over_device"] > 1 for r in rows)
                                    else "NOT lower than the host wall on every row.")]
    if rounds:
        md += ["", "## The counts-only kernel, this tree against the parent commit", "",
               "vasr_edit_counts_i32 of each library in a process of its own, alternating, median of 20 (min - max), us:", "",
               "| round | library | " + " | ".join(f"({n}) {u}" for n, u in ROWS) + " |", "|---|---|" + "---|" * len(ROWS)]
        for k, rd in enumerate(rounds):
            md.append(f"| {k // 2 + 1} | {rd['lib']} | " + " | ".join(cell(rd["kernel_us"][f"{n}/{u}"]) for n, u in ROWS) + " |")
    md += ["", "## Crossover", "",
           "Batches of P pairs of about 30 characters, error_alignments wall with and without device=, median of 20:", "",
           "| pairs | DP cells | device wall ms | host wall ms |", "|---|---|---|---|"]
    md += [f"| {c['pairs']} | {c['cells']} | {c['device_wall_ms']} | {c['host_wall_ms']} |" for c in cross]
    md += ["", f"The smallest batch here at which the device wins has {first} cells; training.ALIGN_MIN_DEVICE_CELLS was "
           f"{threshold} during this run (the tool sets it to 0 while it times)."]
    with open(a.out + ".md", "w") as f:
        f.write("\n".join(md) + "\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
