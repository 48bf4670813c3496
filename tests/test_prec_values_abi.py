"""The C ABI of the single-precision preconditioner values (alfd_set_preconditioner_values and its three companions):
new symbols only, nothing existing moves.  No compute calls; null x / y / out on a live context need a GPU
(tests/test_gpu_prec_values.py)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from fictitious_domain_al_preconditioners_amd import _abi, solver

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("alfd_set_preconditioner_values", "alfd_get_preconditioner_values", "alfd_spmv_preconditioner",
       "alfd_bench_spmv_preconditioner")


@pytest.fixture(scope="module", autouse=True)
def _built(built):
    return built


def test_new_symbols_and_nothing_else_moves():
    lib = solver.load_library()
    hdr = open(os.path.join(ROOT, "include", "alfd", "alfd.h")).read()
    for name in NEW:
        assert hasattr(lib, name) and name in solver.ABI_SYMBOLS, name
        assert re.search(r"\bint " + name + r"\(alfd_ctx_t ctx", hdr), name
    assert "typedef struct alfd_prec_values_info {" in hdr
    assert lib.alfd_abi_version() == 12 and "#define ALFD_ABI_VERSION 12" in hdr
    assert C.sizeof(_abi.Config) == 264 and C.sizeof(_abi.Result) == 80
    assert C.sizeof(_abi.MatrixInfo) == 120
    # 6 x int32, 3 x int64, 2 x double, no padding
    assert C.sizeof(_abi.PrecValuesInfo) == 64
    assert [f for f, _ in _abi.PrecValuesInfo._fields_] == [
        "requested", "stored", "used", "reason", "family", "reserved", "nnz", "flushed_to_zero", "copy_bytes",
        "streamed_bytes_fp64", "streamed_bytes_fp32"]


def test_enums_mirror_the_header():
    hdr = open(os.path.join(ROOT, "include", "alfd", "alfd.h")).read()
    assert "enum alfd_prec_values { ALFD_PREC_VALUES_FP64 = 0, ALFD_PREC_VALUES_FP32 = 1 };" in hdr
    assert (_abi.PREC_VALUES_FP64, _abi.PREC_VALUES_FP32) == (0, 1)
    names = ("NONE", "NOT_REQUESTED", "NO_MATRIX", "SHORT_ROWS", "SPARSE_ROWS", "DICTIONARY_FORM", "PARTITIONED",
             "OUT_OF_RANGE", "NOT_APPLIED")
    for value, name in enumerate(names):
        assert re.search(r"ALFD_PREC_VALUES_" + name + r" = " + str(value) + r"\b", hdr), name
        assert getattr(_abi, "PV_" + name) == value
        assert _abi.PREC_VALUES_REASON_NAMES[value] == name.lower()
    assert _abi.PREC_VALUES_FAMILY_NAMES == ("plain", "stream", "window")


def test_null_pointers_without_gpu():
    lib = solver.load_library()
    z = np.zeros(4)
    p = z.ctypes.data
    info = _abi.PrecValuesInfo()
    for kind in (_abi.PREC_VALUES_FP64, _abi.PREC_VALUES_FP32, 7):
        assert lib.alfd_set_preconditioner_values(None, kind) == _abi.E_INVALID
    assert lib.alfd_get_preconditioner_values(None, C.byref(info)) == _abi.E_INVALID
    assert lib.alfd_get_preconditioner_values(None, None) == _abi.E_INVALID
    for x, y in ((p, p), (None, p), (p, None), (None, None)):
        assert lib.alfd_spmv_preconditioner(None, x, y, 0, 0.0) == _abi.E_INVALID
    ms = C.c_double(-1.0)
    assert lib.alfd_bench_spmv_preconditioner(None, 5, C.byref(ms), None) == _abi.E_INVALID
    assert ms.value == -1.0 and not np.any(z)
