"""Per-kernel-family table (launches and ms per solve, average µs) out of the rocprofv3 kernel statistics of this folder.
`bench.py --steps 1 --warmup 1` is two solves after the setup.  usage: families.py [arm ...]"""
import csv
import re
import sys

ARMS = sys.argv[1:] or ["parent", "change"]
FAMILIES = [
    ("spmv_vs_kernel<0,0,4,0,false> (fine A)", r"spmv_vs_kernel<0, 0, 4, 0, false>"),
    ("spmv_vs_kernel<0,1,4,0,true> (levels 1-2, patch)", r"spmv_vs_kernel<0, 1, 4, 0, true>"),
    ("aug_tail_kernel<*,*>", r"aug_tail_kernel<"),
] + [(f"aug_tail_kernel<{l}, {m}>", rf"aug_tail_kernel<{l}, {m}>") for l in (16, 32, 64) for m in range(5)]

print("| family | " + " | ".join(f"{a}: launches, ms, avg µs" for a in ARMS) + " |")
print("|---|" + "---|" * len(ARMS))
data = {}
for a in ARMS:
    with open(f"{a}_kernel_stats.csv") as f:
        data[a] = [(r["Name"], int(r["Calls"]), int(r["TotalDurationNs"])) for r in csv.DictReader(f)]
for label, pat in FAMILIES:
    cells = []
    for a in ARMS:
        rows = [(c, ns) for n, c, ns in data[a] if re.search(pat, n)]
        calls, ns = sum(c for c, _ in rows), sum(t for _, t in rows)
        cells.append(f"{calls / 2:.0f}, {ns / 2e6:.1f}, {ns / calls * 1e-3:.2f}" if calls else "0")
    print(f"| `{label}` | " + " | ".join(cells) + " |")
