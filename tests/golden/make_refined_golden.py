#!/usr/bin/env python3
"""Regenerates tests/golden/refined_solves.json from the CPU oracle: iteration counts and residual histories of the
locally refined solve cases of tests/refined_cases.py (Chebyshev and multilevel inner preconditioner).  A regression
pin like solves.json (make_golden.py); floats are stored as hex strings (exact)."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import refined_cases as rc  # noqa: E402
from oracle import oracle  # noqa: E402


def solve(name, prec):
    pb, cfg = rc.problem(name), rc.config(name, prec)
    osys = oracle.system_from_problem(pb, aggregates=rc.levels(name, prec))
    code, rhs = osys.augment_rhs(cfg, rc.rhs_of(pb))
    assert code == 0
    code, x, res, hist = osys.solve(cfg, rhs)
    assert code == 0, (name, prec, code)
    return pb, res, hist


def record(pb, res, hist):
    return {"block_sizes": pb.block_sizes,
            "hanging_rows": int(pb.vecs["u_hanging"].sum()) * pb.params["ncomp"],
            "outer_iterations": res.outer_iterations, "inner_iterations": res.inner_iterations,
            "mp_iterations": res.mp_iterations, "last_residual": float(res.last_residual).hex(),
            "history": [float(h).hex() for h in hist]}


def main():
    out = {}
    for name in rc.SOLVE_CASES:
        for prec in rc.PRECONDITIONERS:
            pb, res, hist = solve(name, prec)
            out[f"{name}/{prec}"] = record(pb, res, hist)
            print(name, prec, pb.block_sizes, "outer", res.outer_iterations, "inner", res.inner_iterations)
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "refined_solves.json"), "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
