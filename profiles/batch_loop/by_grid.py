"""Launches in a rocprofv3 kernel trace (`--kernel-trace`, csv) by instantiation and grid: calls, total, average, shortest
and longest duration.  Counted are the kernels whose name holds one of the given family names, by default spmv_vs_kernel
and aug_tail_kernel.  usage: by_grid.py <kernel_trace.csv> <out.csv> [<family> ...]"""
import collections
import csv
import sys

families = sys.argv[3:] or ["spmv_vs_kernel", "aug_tail_kernel"]
acc = collections.defaultdict(lambda: [0, 0, 1 << 62, 0])
with open(sys.argv[1]) as f:
    for r in csv.DictReader(f):
        n = r["Kernel_Name"]
        if not any(s + "<" in n for s in families):
            continue
        n = n[n.index("alfd::") + 6:] if "alfd::" in n else n
        n = n.split("(")[0]
        k = (n, int(r["Grid_Size_X"]) // max(int(r["Workgroup_Size_X"]), 1))
        t = int(r["End_Timestamp"]) - int(r["Start_Timestamp"])
        a = acc[k]
        a[0] += 1
        a[1] += t
        a[2] = min(a[2], t)
        a[3] = max(a[3], t)
with open(sys.argv[2], "w") as f:
    w = csv.writer(f)
    w.writerow(["kernel", "workgroups", "calls", "total_ns", "avg_ns", "min_ns", "max_ns"])
    for (n, g), (c, t, lo, hi) in sorted(acc.items(), key=lambda kv: -kv[1][1]):
        w.writerow([n, g, c, t, t // c, lo, hi])
