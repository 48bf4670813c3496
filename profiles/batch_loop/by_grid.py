"""Launches of spmv_vs_kernel and aug_tail_kernel in a rocprofv3 kernel trace (`--kernel-trace`, csv) by instantiation
and grid: calls, total and average duration.  usage: by_grid.py <kernel_trace.csv> <out.csv>"""
import collections
import csv
import sys

acc = collections.defaultdict(lambda: [0, 0])
with open(sys.argv[1]) as f:
    for r in csv.DictReader(f):
        n = r["Kernel_Name"]
        if "spmv_vs_kernel" not in n and "aug_tail_kernel" not in n:
            continue
        n = n[n.index("alfd::") + 6:] if "alfd::" in n else n
        n = n.split("(")[0]
        k = (n, int(r["Grid_Size_X"]) // max(int(r["Workgroup_Size_X"]), 1))
        acc[k][0] += 1
        acc[k][1] += int(r["End_Timestamp"]) - int(r["Start_Timestamp"])
with open(sys.argv[2], "w") as f:
    w = csv.writer(f)
    w.writerow(["kernel", "workgroups", "calls", "total_ns", "avg_ns"])
    for (n, g), (c, t) in sorted(acc.items(), key=lambda kv: -kv[1][1]):
        w.writerow([n, g, c, t, t // c])
