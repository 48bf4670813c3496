"""alfd_host_sparse_product -- the host routine behind every Galerkin product of the setup, whose bits DESIGN.md
section 4 promises to the device kernel as well -- against the independent reference of
tests/sparse_product_reference.py, on the cases of tests/sparse_product_cases.py (no GPU).  The same cases run through
the device calls in tests/test_gpu_setup_kernels.py.  The prolongator cases are checked here too, through
alfd_host_smoothed_prolongator and alfd_host_truncate_prolongator: the host side of the device test."""
import ctypes as C

import numpy as np
import pytest

from fictitious_domain_al_preconditioners_amd import _abi, problems, solver

import sparse_product_cases as sc
import sparse_product_reference as ref
import truncation_reference as tr


@pytest.fixture(scope="module", autouse=True)
def _built(built):
    return built


def lib_csr(M):
    return problems.Csr(M.nrows, M.ncols, M.row_ptr, M.col, M.val)


def check_product(case, got, tag):
    """The bits of the reference; on the general-valued case also the derived row-wise bound against longdouble."""
    print(f"{case.name} [{tag}]: rows {case.A.nrows}, row under test {case.row} with {case.width} columns, widest "
          f"{int(case.widths.max()) if case.widths.size else 0}, nnz {int(case.ref.row_ptr[-1])}")
    assert ref.same_bits(got, case.ref) is None, (case.name, tag, ref.same_bits(got, case.ref))
    if not case.exact:
        rp, col, want, bound = ref.rowwise_bound(case.A, case.P)
        assert np.array_equal(rp, got.row_ptr) and np.array_equal(col, got.col)
        err = np.abs(np.asarray(got.val).astype(np.longdouble) - want)
        assert np.all(err <= bound), (case.name, tag, "longdouble bound", int(np.argmax(err - bound)))


@pytest.mark.parametrize("name", sc.PRODUCT_NAMES)
def test_host_product_equals_the_reference(name):
    case = sc.product_case(name)
    check_product(case, solver.host_sparse_product(lib_csr(case.A), lib_csr(case.P)), "host")


def test_chain_restatement_agrees_with_the_exact_reference():
    """The two references against each other where both apply: the Fraction chain on exact operands."""
    for name in ("values_and_pattern", "width_65", "width_129"):
        case = sc.product_case(name)
        assert ref.same_bits(ref.chain_product(case.A, case.P), case.ref) is None, name


def test_host_product_refuses_bad_arguments():
    lib = solver.load_library()
    rp = np.array([0, 1], np.int64)
    col = np.array([0], np.int32)
    val = np.array([1.0])
    nnz = C.c_int64(-1)
    orp = np.zeros(2, np.int64)

    def call(a_nrows=1, a_ncols=1, arp=rp, acol=col, p_ncols=1, prp=rp, pcol=col, out=(None, None, 0), n=nnz):
        return lib.alfd_host_sparse_product(a_nrows, a_ncols, arp.ctypes.data, acol.ctypes.data, val.ctypes.data, p_ncols,
                                            prp.ctypes.data, pcol.ctypes.data, val.ctypes.data, orp.ctypes.data, *out,
                                            C.byref(n) if n is not None else None)
    assert call() == _abi.OK and nnz.value == 1 and orp.tolist() == [0, 1]
    assert call(a_nrows=-1) == _abi.E_INVALID
    assert call(p_ncols=-1) == _abi.E_INVALID
    assert call(acol=np.array([1], np.int32)) == _abi.E_INVALID           # a column of A beyond the rows of P
    assert call(acol=np.array([-1], np.int32)) == _abi.E_INVALID
    assert call(pcol=np.array([1], np.int32)) == _abi.E_INVALID           # a column of P beyond p_ncols
    assert call(arp=np.array([1, 1], np.int64)) == _abi.E_INVALID         # a row pointer that does not start at 0
    assert call(prp=np.array([0, -1], np.int64)) == _abi.E_INVALID        # a row pointer that decreases
    assert call(n=None) == _abi.E_INVALID
    oc, ov = np.zeros(1, np.int32), np.zeros(1)
    assert call(out=(oc.ctypes.data, ov.ctypes.data, 0)) == _abi.E_INVALID      # capacity below nnz
    assert call(out=(oc.ctypes.data, ov.ctypes.data, 1)) == _abi.OK and ov[0] == 1.0 and oc[0] == 0


def test_bucket_restatement():
    """The hash of the kernels, restated: a multiplicative hash by 2654435761 whose top 12 (11) bits are the slot."""
    assert ref.bucket(0) == 0 and ref.bucket(1) == 2654435761 >> 20 and ref.bucket(1, 11) == 2654435761 >> 21
    assert ref.bucket(3) == ((3 * 2654435761) & 0xffffffff) >> 20
    for b, bits in ((4095, 12), (4000, 12), (2040, 11)):
        ids = ref.bucket_members(b, bits, 2 ** 23, 1024)
        assert ids.size >= (1024 if bits == 12 else 300) and all(ref.bucket(j, bits) == b for j in ids)


# ---- the prolongator cases on the host routines

@pytest.mark.parametrize("name", sc.PROLONGATOR_NAMES)
def test_host_prolongator_rows_equal_the_reference(name):
    case = sc.prolongator_case(name)
    got = solver.host_smoothed_prolongator(lib_csr(case.A), case.agg, case.n_coarse, case.omega,
                                           None if case.Ct is None else lib_csr(case.Ct), case.w, case.gamma)
    print(f"{name}: rows {case.A.nrows}, row under test {case.row}, widest row {int(case.widths.max())} candidates, "
          f"longest row of A {int(np.diff(case.A.row_ptr).max())}")
    assert ref.same_bits(got, case.ref) is None, (name, ref.same_bits(got, case.ref))


@pytest.mark.parametrize("bs,tau,cap", sc.TRUNCATIONS)
def test_host_truncation_equals_the_restated_rule(bs, tau, cap):
    case = sc.truncation_case()
    want = tr.truncate_rows(lib_csr(case.ref), case.agg, bs, tau, cap)
    got = solver.host_truncate_prolongator(lib_csr(case.ref), case.agg, bs, tau, cap)
    kept = int(want.row_ptr[1] - want.row_ptr[0])
    print(f"truncation bs={bs} tau={tau} cap={cap}: row 0 keeps {kept} of {int(case.widths[0])}")
    sc.check_truncation_properties(case, want, bs, tau, cap)
    assert ref.same_bits(got, want) is None, ref.same_bits(got, want)
