"""The numbering of block 0 below the C ABI (alfd_set_numbering, alfd_set_numbering_from_points): a context that was
told the caller's numbering once against the hand-permuted route -- a second context without numbering, operators
permuted with solver.permute_csr, level-0 transfers, row blocks and vectors permuted in numpy.  Everything compares as
bits (np.array_equal on the uint64 view), iteration counts and residual histories included: the feature is a pure
relabelling, so there is no tolerance.

The checks live in tests/numbering_worker.py and run ONCE, in a process of their own that imports torch before the
library is loaded, so that the tensors of the *_device calls and the library share one HIP runtime; the tests here read
its report, one entry each.  A check that did not run (the worker stops at the first failed HIP call) fails as
"not run".

One case the contract names cannot be reached from outside: a numbering whose size differs from block 0 AT A SOLVE.
alfd_set_matrix refuses every operator with a block-0 side of another size, so no context with such a numbering is ever
set up; the vector calls and alfd_setup still check.  The refusal check covers the reachable part: the uploads are
refused, no solve runs, and the context works once the numbering is cleared."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EDGE_SHAPES = ["laplace2d_81", "laplace2d_5329", "stokes2d_8"]
PERMUTATIONS = ["identity", "reversal", "random", "points_of_cuthill_mckee"]
OTHERS = ["operators", "transfers", "whole_path[stokes3d]", "whole_path[elliptic]", "setup_coupling", "refusals"]


@pytest.fixture(scope="module")
def report(built, tmp_path_factory):
    path = str(tmp_path_factory.mktemp("numbering") / "report.json")
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "numbering_worker.py"), path],
                       capture_output=True, text=True, timeout=900, cwd=ROOT)
    out = json.load(open(path)) if os.path.exists(path) else {}
    out["__process__"] = f"exit status {p.returncode}\n{p.stdout[-3000:]}\n{p.stderr[-3000:]}"
    return out


def _passed(report, name):
    assert report.get(name, "not run\n" + report["__process__"]) == "ok"


@pytest.mark.parametrize("kind", PERMUTATIONS)
@pytest.mark.parametrize("shape", EDGE_SHAPES)
def test_pack_and_unpack_at_the_chunk_edges(report, shape, kind):
    """system_apply and system_apply_device (views with guards, in place, both unpack forms): block 0 of 81 rows (one
    partial chunk, odd), 5 329 rows (two chunks, a pair straddles the end), and three blocks."""
    _passed(report, f"kernel_edges[{shape}-{kind}]")


def test_operators_are_stored_in_the_new_numbering(report):
    """alfd_spmv on A, BT, B, CT, C against the hand-permuted context; alfd_get_numbering round-trips."""
    _passed(report, "operators")


def test_level_0_transfers_come_back_in_the_callers_order(report):
    """alfd_get_prolongator / alfd_get_aggregates at level 0; solves with both kinds of hierarchy."""
    _passed(report, "transfers")


def test_whole_path_reference_shaped_stokes(report):
    """N = 16, cell-wise, Cuthill-McKee, multilevel, set_numbering_from_points: solve, solve_device,
    precond_apply[_device], augment_rhs[_device], constraint_residual; matrix_info(A) as the hand-built route's."""
    _passed(report, "whole_path[stokes3d]")


def test_whole_path_elliptic_interface_with_a_block_1_hierarchy(report):
    _passed(report, "whole_path[elliptic]")


def test_setup_coupling_takes_the_new_ct_in_the_callers_order(report):
    _passed(report, "setup_coupling")


def test_refusals_leave_the_context_usable(report):
    """A numbering after set_matrix(A), a wrong n, a duplicate entry, non-finite points, a 2-rank group in either call
    order, clearing with operators present: each refused, each context solves correctly afterwards."""
    _passed(report, "refusals")


def test_worker_ran_every_check(report):
    names = [f"kernel_edges[{s}-{k}]" for s in EDGE_SHAPES for k in PERMUTATIONS] + OTHERS
    assert sorted(k for k in report if k != "__process__") == sorted(names), report["__process__"]
