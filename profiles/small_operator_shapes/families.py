"""The long-row batch-major level / patch family (spmv_vs_kernel<*, 1, ...>) of a rocprofv3 kernel trace, split by grid.

    python profiles/small_operator_shapes/families.py <..._kernel_trace.csv> <out.csv> [solves]

`bench.py --steps 1 --warmup 1` is two solves after the setup.  One line per (instantiation, workgroups of the launch):
calls and ms per solve, average microseconds per call.  The workgroup count tells the operators apart: the patch
operators, level 1 and level 2 have different block counts (a pair launch adds the workgroups of C)."""
import collections
import csv
import re
import sys

src, dst = sys.argv[1], sys.argv[2]
solves = float(sys.argv[3]) if len(sys.argv) > 3 else 2.0
acc = collections.defaultdict(lambda: [0, 0])
with open(src) as f:
    for r in csv.DictReader(f):
        name = r["Kernel_Name"]
        m = re.search(r"spmv_vs_kernel<[^>]*>", name)
        if not m or not re.match(r"spmv_vs_kernel<\d+, 1,", m.group(0)):
            continue
        wg = int(r["Grid_Size_X"]) // max(int(r["Workgroup_Size_X"]), 1)
        a = acc[(m.group(0), int(r["Workgroup_Size_X"]), wg)]
        a[0] += 1
        a[1] += int(r["End_Timestamp"]) - int(r["Start_Timestamp"])
with open(dst, "w") as f:
    w = csv.writer(f)
    w.writerow(["kernel", "workgroup_size", "workgroups", "calls_per_solve", "ms_per_solve", "avg_us"])
    for (name, wgs, wg), (calls, ns) in sorted(acc.items()):
        w.writerow([name, wgs, wg, f"{calls / solves:.1f}", f"{ns / solves * 1e-6:.3f}", f"{ns / calls * 1e-3:.2f}"])
print(open(dst).read())
