#!/usr/bin/env python3
"""Regenerates tests/golden/refined_q1_solves.json from the CPU oracle: iteration counts and residual history of the
refined stokes3d_sphere(6, 1) solve with the multilevel inner preconditioner on the hierarchy WITH the Q1 level of the
refined mesh (problems.refined_prolongators(q1_level=True), tests/refined_q1_cases.py).  A regression pin like
refined_solves.json (make_refined_golden.py), whose entry stokes3d_sphere/multilevel is the same solve without that
level; floats are stored as hex strings (exact)."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import refined_q1_cases as qc  # noqa: E402


def main():
    pb, lv = qc.mesh(qc.SOLVE), qc.levels(qc.SOLVE)
    res, hist = qc.oracle_solve(pb, lv)
    out = {f"{qc.SOLVE}/multilevel_q1_level": qc.record(pb, lv, res, hist)}
    print(qc.SOLVE, pb.block_sizes, [n for _, n in lv], "outer", res.outer_iterations, "inner", res.inner_iterations)
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "refined_q1_solves.json"), "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
