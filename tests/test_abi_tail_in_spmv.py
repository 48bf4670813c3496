"""The ABI of the tails inside the A launch (tunable "ml_tail_in_spmv"): alfd_spmv_tail_step, alfd_get_fused_tail_launches
and their Python mirror exist and refuse a null context; the header says what the tunable does with values outside 0 / 1.
No GPU here: a context cannot be created without one, so the tunable's refusal of other values and the environment
variable are checked in tests/test_gpu_tail_in_spmv.py."""
import ctypes as C
import os
import re

import pytest

from fictitious_domain_al_preconditioners_amd import _abi, solver

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module", autouse=True)
def _built(built):
    return built


def test_symbols_and_mirror():
    lib = solver.load_library()
    for name in ("alfd_spmv_tail_step", "alfd_get_fused_tail_launches"):
        assert hasattr(lib, name) and name in solver.ABI_SYMBOLS
    assert lib.alfd_spmv_tail_step.argtypes == [C.c_void_p, C.c_int, C.c_int, C.POINTER(_abi.TailStep)]
    assert lib.alfd_get_fused_tail_launches.argtypes == [C.c_void_p, C.POINTER(C.c_int64)]
    assert hasattr(solver.Context, "spmv_tail_step") and hasattr(solver.Context, "fused_tail_launches")


def test_null_context_is_refused():
    lib = solver.load_library()
    s, n = _abi.TailStep(), C.c_int64(7)
    assert lib.alfd_spmv_tail_step(None, _abi.A, 0, C.byref(s)) == _abi.E_INVALID
    assert lib.alfd_spmv_tail_step(None, _abi.A, 1, None) == _abi.E_INVALID
    assert lib.alfd_get_fused_tail_launches(None, C.byref(n)) == _abi.E_INVALID and n.value == 7


def test_struct_mirrors_the_header():
    hdr = open(os.path.join(ROOT, "include", "alfd", "alfd.h")).read()
    body = re.search(r"typedef struct alfd_tail_step \{(.*?)\} alfd_tail_step;", hdr, re.S).group(1)
    names = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            names += [w.strip(" *") for w in re.sub(r"^(const\s+)?\w+\s", "", decl).split(",")]
    assert names == [k for k, _ in _abi.TailStep._fields_]
    assert C.sizeof(_abi.TailStep) == 4 * 4 + 3 * 8 + 2 * 8 + 15 * 8
    assert (_abi.TAIL_STEP, _abi.TAIL_LAST, _abi.TAIL_LAST_ADD, _abi.TAIL_RES, _abi.TAIL_RES_INIT,
            _abi.TAIL_RES_INIT_ADD) == tuple(range(6))


def test_header_documents_the_tunable():
    hdr = open(os.path.join(ROOT, "include", "alfd", "alfd.h")).read()
    at = hdr.index('"ml_tail_in_spmv"')
    doc = hdr[at:hdr.index('"ml_gpu_galerkin"', at)]
    assert "ALFD_ML_TAIL_IN_SPMV" in doc and "default 1" in doc
    assert "refused with ALFD_E_INVALID" in doc          # values outside 0 / 1: refused, not clamped
