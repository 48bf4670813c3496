#!/usr/bin/env python3
"""Compare the kernels of two gfx950 code objects by name: compare_kernels.py PARENT.elf CHANGE.elf [--lists DIR]

Reads, with llvm-readelf, the symbol table (-sW), the section headers (-SW) and the AMDGPU metadata note (--notes) of
each file, and the bytes of every kernel (FUNC symbol) out of the file at the offset the symbol table gives.  Reports
  * the two sets of kernel names (they must be equal),
  * per kernel: symbol size, VGPRs, SGPRs, private segment, group segment, wavefront size (they must be equal),
  * per kernel: whether the bytes are equal, and in how many bytes they differ where they are not.
Kernels are matched by name, not by position: the order of instantiation moves them around in the file.  Nothing is
disassembled.  --lists DIR writes the sorted kernel names of the two files to DIR/parent_kernels.txt and
DIR/change_kernels.txt.  Exit status 0: same names, same sizes and metadata; 1 otherwise."""
import os
import re
import shutil
import subprocess
import sys

META = ("vgpr_count", "sgpr_count", "private_segment_fixed_size", "group_segment_fixed_size", "wavefront_size")


def readelf():
    for cand in (shutil.which("llvm-readelf"), os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib/llvm/bin/llvm-readelf")):
        if cand and os.path.exists(cand):
            return cand
    sys.exit("llvm-readelf not found")


def run(*args):
    return subprocess.run(args, check=True, capture_output=True, text=True).stdout


def kernels(path):
    """name -> dict(size, bytes, the META fields)"""
    tool = readelf()
    sections = {}                                                     # index -> (address, file offset)
    for m in re.finditer(r"^\s*\[\s*(\d+)\]\s+\S*\s+\S+\s+([0-9a-f]+)\s+([0-9a-f]+)\s+[0-9a-f]+", run(tool, "-SW", path), re.M):
        sections[int(m.group(1))] = (int(m.group(2), 16), int(m.group(3), 16))
    with open(path, "rb") as f:
        blob = f.read()
    out = {}
    for line in run(tool, "-sW", path).splitlines():
        f = line.split()
        if len(f) == 8 and f[3] == "FUNC" and f[6].isdigit():
            addr, size, (sec_addr, sec_off) = int(f[1], 16), int(f[2]), sections[int(f[6])]
            out[f[7]] = dict(size=size, bytes=blob[sec_off + addr - sec_addr:sec_off + addr - sec_addr + size])
    entries = []
    for line in run(tool, "--notes", path).splitlines():
        m = re.match(r"\s*(-\s+)?\.(\w+):\s+(\S+)\s*$", line)
        if not m:
            continue
        if line.startswith("  - "):                                   # a new entry of amdhsa.kernels
            entries.append({})
        if entries and m.group(2) in META:
            entries[-1][m.group(2)] = int(m.group(3))
        elif entries and line.startswith("    .name:"):               # the kernel's own name (arguments are deeper)
            entries[-1]["name"] = m.group(3).strip("'\"")
    for e in entries:
        out[e["name"]].update({k: e[k] for k in META if k in e})
    missing = [k for k, v in out.items() if any(key not in v for key in META)]
    if missing:
        sys.exit(f"{path}: no metadata for {len(missing)} kernels, e.g. {missing[0]}")
    return out


def main(argv):
    lists = None
    if "--lists" in argv:
        at = argv.index("--lists")
        lists = argv[at + 1]
        del argv[at:at + 2]
    if len(argv) != 3:
        sys.exit(__doc__)
    parent, change = kernels(argv[1]), kernels(argv[2])
    if lists:
        for name, ks in (("parent_kernels.txt", parent), ("change_kernels.txt", change)):
            with open(os.path.join(lists, name), "w") as f:
                f.write("".join(k + "\n" for k in sorted(ks)))
    ok = True
    for label, ks in (("parent", parent), ("change", change)):
        print(f"{label}: {len(ks)} kernels, {sum('spmv_' in k for k in ks)} with spmv_ in the name")
    for label, names in (("only in parent", sorted(set(parent) - set(change))), ("only in change", sorted(set(change) - set(parent)))):
        print(f"{label}: {len(names)}")
        for k in names:
            print("   ", k)
        ok = ok and not names
    common = sorted(set(parent) & set(change))
    unequal = [k for k in common if any(parent[k][key] != change[k][key] for key in ("size",) + META)]
    print(f"symbol size or metadata ({', '.join(META)}) differ: {len(unequal)} of {len(common)}")
    for k in unequal:
        print("   ", k, {key: (parent[k][key], change[k][key]) for key in ("size",) + META if parent[k][key] != change[k][key]})
    ok = ok and not unequal
    differ = [k for k in common if k not in unequal and parent[k]["bytes"] != change[k]["bytes"]]
    print(f"bytes differ at equal size: {len(differ)} of {len(common)}")
    for k in differ:
        n = sum(a != b for a, b in zip(parent[k]["bytes"], change[k]["bytes"]))
        print(f"    {k}: {n} of {parent[k]['size']} bytes")
    print("RESULT:", "same kernels, sizes and metadata" + ("; same bytes" if not differ else "") if ok else "DIFFERENT")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main(sys.argv))
