#!/usr/bin/env python3
"""Per-launch times of a rocprofv3 --kernel-trace run grouped by (kernel, grid size, workgroup size):
kernel_stats.csv averages a kernel over all its shapes, this keeps the shapes apart (the one-graph
schedule's launches at M = 16032 from the same kernel's small launches).
    python tools/trace_groups.py <directory holding *kernel_trace.csv>   (the 60 largest groups)"""
import collections
import csv
import glob
import sys

path = glob.glob(sys.argv[1] + "/**/*kernel_trace.csv", recursive=True)[0]
g = collections.defaultdict(list)
for r in csv.DictReader(open(path)):
    key = (r["Kernel_Name"][:110], r.get("Grid_Size_X", r.get("Grid_Size", "?")), r.get("Workgroup_Size_X", "?"))
    g[key].append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
for (n, gs, ws), v in sorted(g.items(), key=lambda kv: -sum(kv[1]))[:60]:
    v2 = sorted(v)
    print(f"{sum(v):10.1f} us total  n={len(v):5d}  med {v2[len(v2) // 2]:8.2f}  min {v2[0]:8.2f}  "
          f"grid {gs:>8s} wg {ws:>4s}  {n}")
