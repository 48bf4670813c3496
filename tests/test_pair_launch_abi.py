"""alfd_spmv_pair without a GPU: declared, exported, mirrored, and refused on a null context."""
import ctypes as C
import os
import re

import numpy as np

from fictitious_domain_al_preconditioners_amd import _abi, solver

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "alfd", "alfd.h")


def test_spmv_pair_is_declared_exported_and_mirrored(built):
    lib = solver.load_library()
    assert "alfd_spmv_pair" in solver.ABI_SYMBOLS and hasattr(lib, "alfd_spmv_pair")
    with open(HEADER) as f:
        text = f.read()
    assert re.search(r"int alfd_spmv_pair\(alfd_ctx_t ctx, int slot_a, int slot_c, const double \*x, const double \*d, "
                     r"double \*y, double \*t\);", text)
    assert lib.alfd_spmv_pair.argtypes == [C.c_void_p, C.c_int, C.c_int] + [C.c_void_p] * 4
    assert hasattr(solver.Context, "spmv_pair")


def test_spmv_pair_refuses_a_null_context(built):
    """A null context answers ALFD_E_INVALID before any device call and writes nothing.  (The checks of the other
    arguments need a live context: tests/test_gpu_pair_launch.py.)"""
    lib = solver.load_library()
    v, y, t = np.ones(3), np.full(3, np.nan), np.full(3, np.nan)
    assert lib.alfd_spmv_pair(None, _abi.A, _abi.C_, v.ctypes.data, v.ctypes.data, y.ctypes.data, t.ctypes.data) == _abi.E_INVALID
    assert np.isnan(y).all() and np.isnan(t).all()
