"""The numbering of block 0 at the C ABI, as far as no GPU is needed: the four declarations, the host-only check of a
permutation (alfd_host_check_numbering) and the null-context answers of the calls that take a context."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from fictitious_domain_al_preconditioners_amd import _abi, solver

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = ["alfd_host_check_numbering", "alfd_set_numbering", "alfd_set_numbering_from_points", "alfd_get_numbering"]


def _permutations(n):
    rng = np.random.default_rng(1000 + n)
    return {"identity": np.arange(n, dtype=np.int64), "reversal": np.arange(n, dtype=np.int64)[::-1].copy(),
            "random": rng.permutation(n).astype(np.int64)}


def test_the_four_calls_are_declared_and_the_version_stays(built):
    header = open(os.path.join(ROOT, "include", "alfd", "alfd.h")).read()
    lib = solver.load_library()
    for name in CALLS:
        assert re.search(r"^int " + name + r"\(", header, re.M), name
        assert name in solver.ABI_SYMBOLS
        assert getattr(lib, name).argtypes is not None and getattr(lib, name).restype is C.c_int
    assert lib.alfd_abi_version() == 12
    assert re.search(r"^#define ALFD_ABI_VERSION 12$", header, re.M)


@pytest.mark.parametrize("n", [1, 2, 5329])
@pytest.mark.parametrize("kind", ["identity", "reversal", "random"])
def test_check_numbering_accepts_permutations_and_inverts_them(built, n, kind):
    p = _permutations(n)[kind]
    inv = solver.check_numbering(p)
    assert inv.dtype == np.int64 and inv.shape == (n,)
    assert np.array_equal(inv[p], np.arange(n)) and np.array_equal(p[inv], np.arange(n))
    # the inverse is optional
    assert solver.load_library().alfd_host_check_numbering(n, p.ctypes.data, None) == _abi.OK


def test_check_numbering_refuses_what_is_no_bijection(built):
    lib = solver.load_library()
    for n in (2, 5329):
        base = _permutations(n)["random"]
        for bad_value in (-1, n):
            p = base.copy()
            p[n // 2] = bad_value
            inv = np.full(n, -7, np.int64)
            assert lib.alfd_host_check_numbering(n, p.ctypes.data, inv.ctypes.data) == _abi.E_INVALID, (n, bad_value)
        p = base.copy()
        p[0] = p[n - 1]                                          # a duplicate (and so a missing entry)
        assert lib.alfd_host_check_numbering(n, p.ctypes.data, None) == _abi.E_INVALID
        with pytest.raises(solver.AlfdError) as e:
            solver.check_numbering(p)
        assert e.value.status == _abi.E_INVALID
    one = np.zeros(1, np.int64)
    assert lib.alfd_host_check_numbering(1, None, None) == _abi.E_INVALID      # null pointer with n > 0
    assert lib.alfd_host_check_numbering(-1, one.ctypes.data, None) == _abi.E_INVALID
    assert lib.alfd_host_check_numbering(0, None, None) == _abi.OK             # the empty permutation


def test_a_null_context_is_invalid(built):
    lib = solver.load_library()
    p = np.arange(4, dtype=np.int64)
    pts = np.zeros((4, 2))
    n = C.c_int64(-1)
    assert lib.alfd_set_numbering(None, 4, p.ctypes.data) == _abi.E_INVALID
    assert lib.alfd_set_numbering(None, 0, None) == _abi.E_INVALID
    assert lib.alfd_set_numbering_from_points(None, 4, 2, pts.ctypes.data, None) == _abi.E_INVALID
    assert lib.alfd_get_numbering(None, None, 0, C.byref(n)) == _abi.E_INVALID
