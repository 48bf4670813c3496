"""Per-kernel-family table (calls and ms per solve) out of the rocprofv3 kernel statistics of this folder.
`bench.py --steps 1 --warmup 1` is two solves after the setup; kernels of the setup alone are left out."""
import csv
import re
import sys

ARMS = ["parent", "fuse1", "fuse2", "fuse3"]
FAMILIES = [
    ("spmv_vs_kernel<0,0,4,0> (fine A)", r"spmv_vs_kernel<0, 0, 4, 0(, false)?>"),
    ("spmv_vs_kernel<0,0,4,0,true> (fine A + C)", r"spmv_vs_kernel<0, 0, 4, 0, true>"),
    ("spmv_vs_kernel<0,1,4,0> (patch, levels 1-2)", r"spmv_vs_kernel<0, 1, 4, 0(, false)?>"),
    ("spmv_vs_kernel<0,1,4,0,true> (the same + C)", r"spmv_vs_kernel<0, 1, 4, 0, true>"),
    ("spmv_stream_kernel<2,8,0> (levels 3-4)", r"spmv_stream_kernel<2, 8, 0, false(, false)?>"),
    ("spmv_stream_kernel<2,8,0,.,true> (the same + C)", r"spmv_stream_kernel<2, 8, 0, false, true>"),
    ("spmv_stream_kernel<2,8,2> (C, 64 lanes)", r"spmv_stream_kernel<2, 8, 2, false(, false)?>"),
    ("spmv_kernel<16,2> (C)", r"spmv_kernel<16, 2, false>"),
    ("spmv_kernel<32,2> (C)", r"spmv_kernel<32, 2, false>"),
    ("aug_tail_kernel<*,*>", r"aug_tail_kernel<"),
]


def load(arm):
    with open(f"{arm}_kernel_stats.csv") as f:
        return [(r["Name"], int(r["Calls"]), int(r["TotalDurationNs"])) for r in csv.DictReader(f)]


def main():
    data = {a: load(a) for a in ARMS}
    solves = 2.0
    print("| family | " + " | ".join(f"{a} calls | ms | avg µs" for a in ARMS) + " |")
    print("|---|" + "---|" * (3 * len(ARMS)))
    for label, pat in FAMILIES:
        cells = []
        for a in ARMS:
            rows = [(c, ns) for n, c, ns in data[a] if re.search(pat, n)]
            calls, ns = sum(c for c, _ in rows), sum(t for _, t in rows)
            cells.append(f"{calls / solves:.0f} | {ns / solves * 1e-6:.1f} | {ns / calls * 1e-3:.1f}" if calls else "0 | 0 | –")
        print(f"| `{label}` | " + " | ".join(cells) + " |")
    for a in ARMS:
        calls = sum(c for _, c, _ in data[a])
        print(f"{a}: {calls} kernel launches in the whole run", file=sys.stderr)


if __name__ == "__main__":
    main()
