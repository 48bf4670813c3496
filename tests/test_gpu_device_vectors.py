"""Device-resident vectors: Context.solve_device / precond_apply_device / system_apply_device / augment_rhs_device /
upload_rhs_device / download_solution_device on torch tensors against the host-pointer calls of the same context.
All comparisons are np.array_equal -- the device calls run the same code behind one pack and one unpack launch.

The checks themselves live in tests/device_vectors_worker.py and run ONCE, in a process of their own that imports
torch before the library is loaded, so that the tensors and the library share one HIP runtime (that module's
docstring has the reason); the tests here read its report, one entry each.  A check that did not run (the worker
stops at the first failed HIP call) fails as "not run"."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOLVE_CASES = ["laplace2d_circle", "stokes3d_sphere", "elliptic_modified", "rational_minres"]
CHUNK_CASES = ["exact_and_short", "multiple_plus_1", "multiple_minus_1", "two_exact_chunks"]


@pytest.fixture(scope="module")
def report(built, tmp_path_factory):
    path = str(tmp_path_factory.mktemp("device_vectors") / "report.json")
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "device_vectors_worker.py"), path],
                       capture_output=True, text=True, timeout=900, cwd=ROOT)
    out = json.load(open(path)) if os.path.exists(path) else {}
    out["__process__"] = f"exit status {p.returncode}\n{p.stdout[-3000:]}\n{p.stderr[-3000:]}"
    return out


def _passed(report, name):
    assert report.get(name, "not run\n" + report["__process__"]) == "ok"


@pytest.mark.parametrize("name", SOLVE_CASES)
def test_solve_device_equals_host_solve(report, name):
    """From a non-zero x0, after a solve of other data on the same context: solution, history, counts, status."""
    _passed(report, f"solve_parity[{name}]")


def test_augment_rhs_and_resident_solve_from_device_blocks(report):
    _passed(report, "augment_and_resident")


@pytest.mark.parametrize("key", CHUNK_CASES)
def test_apply_device_at_chunk_edges(report, key):
    """system_apply_device / precond_apply_device with block sizes 4096, 4096 +- 1, 8192, 40: three chunks in all."""
    _passed(report, f"chunk_edges[{key}]")


def test_blocks_as_odd_offset_views_and_in_place(report):
    _passed(report, "views")


def test_inputs_are_awaited_on_the_callers_stream(report):
    _passed(report, "stream")


def test_warm_start_from_the_returned_solution(report):
    _passed(report, "warm_start")


def test_refusals_leave_the_context_usable(report):
    """Host and null pointers, a block that runs past its allocation (ALFD_E_INVALID), ValueError in Python,
    ALFD_E_NOT_SETUP, ALFD_E_UNSUPPORTED."""
    _passed(report, "validation")


@pytest.mark.parametrize("variant", ["multigrid", "empty_rank_multigrid", "empty_rank"])
def test_two_in_process_ranks(report, variant):
    _passed(report, f"two_ranks[{variant}]")


def test_worker_ran_every_check(report):
    names = [f"solve_parity[{n}]" for n in SOLVE_CASES] + ["augment_and_resident"] + \
            [f"chunk_edges[{k}]" for k in CHUNK_CASES] + ["views", "stream", "warm_start", "validation"] + \
            [f"two_ranks[{v}]" for v in ("multigrid", "empty_rank_multigrid", "empty_rank")]
    assert sorted(k for k in report if k != "__process__") == sorted(names), report["__process__"]
