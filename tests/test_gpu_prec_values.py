"""Single-precision operator values inside the inner preconditioner (alfd_set_preconditioner_values) on the GPU.

  * A~ x of the three float kernel families bit for bit against the oracle's canonical sums on the rounded values;
  * operators that keep their 8-byte values: the reason, the refusal of the primitive, solves bit-equal to option off;
  * M^-1 against tests/prec_values_reference.py -- and NOT against the restatement on the exact values;
  * representable values: option on is option off, bit for bit, down to the window kernel inside the real cycle;
  * a solve on general values, the lifecycle of the copy, and the bytes the timer reports.

Every case first asserts the storage form it means to test (alfd_get_matrix_info, alfd_get_preconditioner_values)."""
import numpy as np
import pytest
import scipy.sparse as sp

import cases
import prec_values_reference as pv
import precond_reference as pr
import test_inner_preconditioner as base
import test_prec_values_reference as cpu
from fictitious_domain_al_preconditioners_amd import _abi, partition, problems, solver
from oracle import oracle

pytestmark = pytest.mark.gpu
LONG_GEN = dict(dim=3, degree=2, ncomp=3, stokes=False, grad_div=True, gamma_grad_div=10.0, radius=0.1, immersed_refine=0)


# ---------------------------------------------------------------------------------------------------- helpers
def _form(info, **want):
    got = {k: info[k] for k in want}
    assert got == want, info


def _fp32_context():
    ctx = solver.Context(0)
    ctx.set_preconditioner_values("fp32")
    return ctx


def _context(cf, values, fuse=None, dictionaries=True):
    """cf (base.Config) on a fresh context with the option set BEFORE the upload.  dictionaries = False: the context plans
    no dictionary-coded form at all (ALFD_SPMV_VALUE_INDEX = 0 at alfd_create), as for values that never repeat."""
    with pytest.MonkeyPatch.context() as mp:
        if not dictionaries:
            mp.setenv("ALFD_SPMV_VALUE_INDEX", "0")
        ctx = solver.Context(0)
    if values == "fp32":
        ctx.set_preconditioner_values("fp32")
    if fuse is not None:
        ctx.set_tunable("ml_fuse", fuse)
    return solver.upload_problem(ctx, cf.pb, _abi.Config.from_buffer_copy(cf.cfg), cf.levels)


def _solve(ctx, pb):
    rhs = ctx.augment_rhs(cases.rhs_of(pb))
    x, res = ctx.solve(rhs, raise_on_failure=False)
    return dict(status=res.status, outer=res.outer_iterations, inner=res.inner_iterations, mp=res.mp_iterations,
                lambda_max=res.lambda_max, papp=res.precond_applications, history=ctx.history(), x=np.concatenate(x), rhs=rhs,
                last_residual=res.last_residual)


def _assert_same_solve(a, b, tag):
    for k in ("status", "outer", "inner", "mp", "lambda_max"):
        assert a[k] == b[k], (tag, k, a[k], b[k])
    assert np.array_equal(a["history"], b["history"]), (tag, "history")
    assert np.array_equal(a["x"], b["x"]), (tag, "solution")


def _unsupported_and_untouched(ctx, n_cols, n_rows):
    x, y = np.ones(max(n_cols, 1)), np.full(max(n_rows, 1), np.nan)
    for mode in (0, 1):
        assert ctx._lib.alfd_spmv_preconditioner(ctx._h, x.ctypes.data, y.ctypes.data, mode, 1.0) == _abi.E_UNSUPPORTED
    assert np.isnan(y).all()
    ms = solver.C.c_double(-1.0)
    assert ctx._lib.alfd_bench_spmv_preconditioner(ctx._h, 3, solver.C.byref(ms), None) == _abi.E_UNSUPPORTED
    assert ms.value == -1.0


def edge_content(m, seed):
    """m with: structurally empty rows (r = 5 mod 97), single-entry rows (r = 50 mod 1013), a pair of 700-entry rows on a
    contiguous column range (200, 201) and a pair of 2400-entry rows on columns scattered over the whole matrix
    (1000, 1001: no x window holds them) -- each pair longer than 64 * 16 entries --, stored zeros, values whose
    binary32 image is subnormal, values near FLT_MAX."""
    rng = np.random.default_rng(seed)
    rp = np.asarray(m.row_ptr, np.int64)
    row = np.repeat(np.arange(m.nrows, dtype=np.int64), np.diff(rp))
    col, val = np.asarray(m.col, np.int64), np.array(m.val, np.float64)
    first = np.zeros(row.size, bool)
    first[rp[:-1][np.diff(rp) > 0]] = True
    long_rows = np.isin(row, (200, 201, 1000, 1001))
    keep = ~(row % 97 == 5) & (~(row % 1013 == 50) | first) & ~long_rows
    row, col, val = row[keep], col[keep], val[keep]
    extra_r, extra_c = [], []
    for r in (200, 201):
        extra_r.append(np.full(700, r)), extra_c.append(np.arange(700) + max(0, min(r - 350, m.ncols - 700)))
    n_far = min(2400, m.ncols - 100)               # two such rows: more than the 4096 slots of an x window
    for r in (1000, 1001):
        extra_r.append(np.full(n_far, r)), extra_c.append(np.sort(rng.choice(m.ncols, n_far, replace=False)))
    row = np.concatenate([row] + extra_r)
    col = np.concatenate([col] + extra_c)
    val = np.concatenate([val, rng.uniform(-1, 1, 1400 + 2 * n_far) * (1.0 + 2.0 ** -30)])
    k = rng.permutation(val.size)
    val[k[:300]] = 0.0
    val[k[300:400]] = rng.choice([1e-40, -7e-42, 1.17e-38, -2e-39, 3e-45], 100)
    val[k[400:420]] = rng.choice([1e-60, -1e-50], 20)                      # image zero, not subnormal
    val[k[420:520]] = rng.choice([3.4e38, -3.3e38, 3.0e38, -(2.0 - 2.0 ** -24) * 2.0 ** 127 * (1 - 2.0 ** -50)], 100)
    a = sp.coo_matrix((val, (row, col)), shape=(m.nrows, m.ncols)).tocsr()
    a.sort_indices()
    out = problems.Csr(m.nrows, m.ncols, a.indptr.astype(np.int64), a.indices.astype(np.int32), a.data.astype(np.float64))
    ln = np.diff(out.row_ptr)
    assert (ln == 0).sum() > 20 and (ln == 1).sum() >= 2 and ln[200] + ln[201] > 1024 and ln[1000] + ln[1001] > 1024
    assert (out.val == 0).sum() >= 300
    return out


class SpmvCase:
    """One matrix, the oracle's canonical sums on its rounded values (the reference) and on the exact ones."""

    def __init__(self, m, seed):
        rng = np.random.default_rng(seed)
        self.m = m
        f, self.flushed = pv.round_values(m.val)
        assert np.all(np.isfinite(f)) and self.flushed > 0
        self.rounded = problems.Csr(m.nrows, m.ncols, m.row_ptr, m.col, f.astype(np.float64))
        self.x = rng.uniform(-1.0, 1.0, m.ncols)
        self.y0 = rng.uniform(-1.0, 1.0, m.nrows)
        self.s32, self.lanes = oracle.spmv(self.rounded, self.x, None, mode=0)
        self.s64, _ = oracle.spmv(m, self.x, None, mode=0)
        self.m32, _ = oracle.spmv(self.rounded, self.x, self.y0, mode=1, alpha=-0.75)
        self.m64, _ = oracle.spmv(m, self.x, self.y0, mode=1, alpha=-0.75)
        assert self.lanes == 64 and not np.array_equal(self.s32, self.s64)

    def check(self, ctx, tag, family):
        info = ctx.preconditioner_values()
        _form(info, requested=1, stored=1, used=0, reason=_abi.PV_NOT_APPLIED, family=family, nnz=self.m.nnz,
              flushed_to_zero=self.flushed, copy_bytes=4 * self.m.nnz)
        assert info["streamed_bytes_fp64"] - info["streamed_bytes_fp32"] == 4.0 * self.m.nnz, info
        assert info["streamed_bytes_fp64"] == ctx.matrix_info(_abi.A)["streamed_bytes"]
        nan = np.full(self.m.nrows, np.nan)
        y = ctx.spmv_preconditioner(self.x, nan, mode=0)
        assert np.array_equal(y, self.s32), (tag, "mode 0", _first_bad(y, self.s32))
        assert not np.array_equal(y, self.s64), (tag, "mode 0 equals the product with the exact values")
        assert np.array_equal(np.signbit(y), np.signbit(self.s32)), (tag, "signed zeros")
        y = ctx.spmv_preconditioner(self.x, self.y0, mode=1, alpha=-0.75)
        assert np.array_equal(y, self.m32), (tag, "mode 1", _first_bad(y, self.m32))
        assert not np.array_equal(y, self.m64), tag
        # the 8-byte values are still what everything else sees
        y, _ = ctx.spmv(_abi.A, self.x, nan, mode=0)
        assert np.array_equal(y, self.s64), (tag, "alfd_spmv")


def _first_bad(got, want):
    bad = np.flatnonzero(~(got == want))
    return (int(bad.size), int(bad[0]), float(got[bad[0]]), float(want[bad[0]])) if bad.size else None


def _random_matrix(avg):
    a = sp.random(3001, 2500, density=avg / 2500.0, random_state=int(avg), format="csr")
    a.data[:] = np.random.default_rng(5).uniform(-1, 1, a.nnz)
    return problems.Csr.from_scipy(a)


@pytest.fixture(scope="module")
def long_operator():
    """The N = 10 vector-Q2 operator of tests/test_gpu_spmv_epilogues.py (27 783 rows: 290 row blocks of 96)."""
    pb = problems.generate(n_cells=10, **LONG_GEN)
    assert pb.mats["A"].nrows == 27783
    return pb.mats["A"]


@pytest.fixture(scope="module")
def window_case(long_operator):
    return SpmvCase(edge_content(pv.general_values(long_operator), 61), 62)


# ------------------------------------------------------------------------------------- A~ x, bit for bit
def test_window_kernel_both_branches_bitwise(built, window_case):
    """spmv_window_kernel<.., float>: the LDS-window branch and, in the row block of the two scattered 2400-entry rows,
    the blk_W < 0 branch that gathers from global memory; 27 783 = 289 * 96 + 39 rows, so the last block is partial."""
    ctx = _fp32_context()
    try:
        ctx.set_matrix(_abi.A, window_case.m)
        info = ctx.matrix_info(_abi.A)
        _form(info, lanes=64, windowed=1, value_indexed=0, batch_major=0)
        assert 0 < info["window_fallback_blocks"] < info["window_blocks"] and window_case.m.nrows % 96 != 0, info
        window_case.check(ctx, "window", family=2)
    finally:
        ctx.close()


@pytest.mark.parametrize("shape", [(2, 8), (4, 8), (2, 16)])
def test_window_kernel_result_does_not_depend_on_the_launch_shape(built, window_case, shape, monkeypatch):
    """The candidate shapes of profiles/prec_values/ beside the default (4, 16): ALFD_SPMV_PREC32_R / _U at alfd_create."""
    monkeypatch.setenv("ALFD_SPMV_PREC32_R", str(shape[0]))
    monkeypatch.setenv("ALFD_SPMV_PREC32_U", str(shape[1]))
    ctx = _fp32_context()
    try:
        ctx.set_matrix(_abi.A, window_case.m)
        window_case.check(ctx, f"window {shape}", family=2)
    finally:
        ctx.close()


@pytest.mark.parametrize("avg", [70, 200])
@pytest.mark.parametrize("family", ["stream", "plain"])
def test_stream_and_plain_kernels_bitwise(built, avg, family, monkeypatch):
    """spmv_stream_kernel<2, 8, .., float> and, with the streaming kernel switched off at alfd_create,
    spmv_kernel<64, ., false, float>: 3001 rows (odd: the last wave holds a partially filled set of row groups)."""
    if family == "plain":
        monkeypatch.setenv("ALFD_SPMV_STREAM_R", "0")
    case = SpmvCase(edge_content(_random_matrix(avg), 63 + avg), 64 + avg)
    ctx = _fp32_context()
    try:
        ctx.set_matrix(_abi.A, case.m)
        _form(ctx.matrix_info(_abi.A), lanes=64, windowed=0, batch_major=0, value_indexed=0)
        case.check(ctx, f"{family} {avg}", family=1 if family == "stream" else 0)
    finally:
        ctx.close()


def test_null_pointers_and_unknown_kind_on_a_live_context(built):
    ctx = _fp32_context()
    try:
        m = _random_matrix(70)
        ctx.set_matrix(_abi.A, m)
        x, y = np.ones(m.ncols), np.full(m.nrows, np.nan)
        lib, h = ctx._lib, ctx._h
        assert lib.alfd_spmv_preconditioner(h, None, y.ctypes.data, 0, 0.0) == _abi.E_INVALID
        assert lib.alfd_spmv_preconditioner(h, x.ctypes.data, None, 0, 0.0) == _abi.E_INVALID
        assert lib.alfd_spmv_preconditioner(h, x.ctypes.data, y.ctypes.data, 2, 0.0) == _abi.E_INVALID
        assert np.isnan(y).all()
        assert lib.alfd_get_preconditioner_values(h, None) == _abi.E_INVALID
        assert lib.alfd_bench_spmv_preconditioner(h, 0, None, None) == _abi.E_INVALID
        for kind in (2, -1, 99):
            assert lib.alfd_set_preconditioner_values(h, kind) == _abi.E_INVALID
        assert ctx.preconditioner_values()["stored"] == 1
        with pytest.raises(ValueError):
            ctx.set_preconditioner_values("fp16")
        ms, nbytes = ctx.bench_spmv_preconditioner(3)
        assert ms > 0 and nbytes == ctx.preconditioner_values()["streamed_bytes_fp32"]
    finally:
        ctx.close()


# ------------------------------------------------------------------------------------- ineligible operators
def _ineligible(pb, cfg, levels, reason, tag):
    """Reason reported, primitive refused, and the solve bit-equal to option off."""
    out = {}
    for values in ("fp64", "fp32"):
        ctx = solver.Context(0)
        try:
            ctx.set_preconditioner_values(values)
            solver.upload_problem(ctx, pb, _abi.Config.from_buffer_copy(cfg), levels)
            info = ctx.preconditioner_values()
            if values == "fp32":
                _form(info, requested=1, stored=0, used=0, reason=reason, copy_bytes=0, nnz=pb.mats["A"].nnz)
                _unsupported_and_untouched(ctx, pb.mats["A"].ncols, pb.mats["A"].nrows)
            else:
                _form(info, requested=0, stored=0, used=0, reason=_abi.PV_NOT_REQUESTED)
            out[values] = _solve(ctx, pb)
        finally:
            ctx.close()
    print(f"{tag}: status {out['fp32']['status']}, outer {out['fp32']['outer']}, inner {out['fp32']['inner']}")
    _assert_same_solve(out["fp64"], out["fp32"], tag)
    return out["fp32"]


def test_dictionary_form_keeps_its_values(built):
    """The unperturbed N = 10 Taylor-Hood operator: batch-major, dictionary-coded."""
    pb = problems.stokes3d_sphere(10, 1)
    cfg = _abi.default_config(_abi.AL_STOKES)
    cfg.inner.max_steps = 1000
    ctx = solver.Context(0)
    try:
        ctx.set_matrix(_abi.A, pb.mats["A"])
        assert ctx.matrix_info(_abi.A)["batch_major"] >= 1 and pb.mats["A"].nrows == 27783
    finally:
        ctx.close()
    res = _ineligible(pb, cfg, None, _abi.PV_DICTIONARY_FORM, "dictionary form")
    assert res["status"] == _abi.OK


def test_short_rows_keep_their_values(built):
    """A 2-D Q1 Laplacian: 8 lanes per row."""
    pb, cfg = problems.laplace2d_circle(32, 3), _abi.default_config(_abi.AL2)
    ctx = solver.Context(0)
    try:
        ctx.set_matrix(_abi.A, pb.mats["A"])
        assert ctx.matrix_info(_abi.A)["lanes"] < 64
    finally:
        ctx.close()
    res = _ineligible(pb, cfg, None, _abi.PV_SHORT_ROWS, "short rows")
    assert res["status"] == _abi.OK


def test_an_entry_out_of_range_keeps_the_values(built):
    """One entry 1e39 (the diagonal of a Dirichlet row, so the operator stays definite): no finite image."""
    cf = cpu.general_config("cheb4_stokes")
    A = cf.pb.mats["A"]
    lone = np.flatnonzero(np.diff(A.row_ptr) == 1)
    val = np.array(A.val)
    val[A.row_ptr[lone[lone.size // 2]]] = 1e39
    pb = pv.with_A(cf.pb, problems.Csr(A.nrows, A.ncols, A.row_ptr, A.col, val))
    _ineligible(pb, cf.cfg, None, _abi.PV_OUT_OF_RANGE, "out of range")
    ctx = _fp32_context()
    try:                                             # ... and the next upload without it is taken
        ctx.set_matrix(_abi.A, pb.mats["A"])
        assert ctx.preconditioner_values()["reason"] == _abi.PV_OUT_OF_RANGE
        ctx.set_matrix(_abi.A, A)
        assert ctx.preconditioner_values()["stored"] == 1
    finally:
        ctx.close()


def test_sparse_rows_and_no_matrix(built):
    ctx = _fp32_context()
    try:
        _form(ctx.preconditioner_values(), requested=1, stored=0, reason=_abi.PV_NO_MATRIX, nnz=0)
        _unsupported_and_untouched(ctx, 4, 4)
        a = sp.random(5000, 400, density=0.3, random_state=1, format="lil")
        a[10:4900, :] = 0
        m = problems.Csr.from_scipy(a.tocsr())
        ctx.set_matrix(_abi.A, m)
        _form(ctx.preconditioner_values(), requested=1, stored=0, reason=_abi.PV_SPARSE_ROWS, nnz=m.nnz)
        _unsupported_and_untouched(ctx, m.ncols, m.nrows)
    finally:
        ctx.close()


def test_partitioned_context_keeps_its_values(built):
    """Two in-process ranks as in tests/test_gpu_multirank.py, upload and query only: the request is accepted and stays
    ineligible, the same answer on both ranks."""
    import threading
    n, refine = 8, 1
    plan = partition.slab_partition_stokes3d(n, refine, 2)
    group = solver.LocalGroup(2)
    out, errs = [None, None], []

    def work(rank):
        try:
            pb = problems.stokes3d_sphere(n, refine, row_ranges=plan.generator_ranges(rank))
            ctx = solver.Context(0)
            try:
                ctx.comm_init_local(group.handle, rank)
                ctx.set_partition(plan.offsets)
                ctx.set_preconditioner_values("fp32")
                before = ctx.preconditioner_values()
                ctx.set_matrix(_abi.A, pb.mats["A"])
                info = ctx.preconditioner_values()
                _unsupported_and_untouched(ctx, 8, 8)
                out[rank] = (before["reason"], info["requested"], info["stored"], info["used"], info["reason"])
            finally:
                ctx.close()
        except Exception as e:   # noqa: BLE001
            errs.append((rank, e))

    th = [threading.Thread(target=work, args=(r,)) for r in range(2)]
    for t in th:
        t.start()
    for t in th:
        t.join(timeout=300)
    group.close()
    assert not errs, errs
    assert out[0] == out[1] == (_abi.PV_PARTITIONED, 1, 0, 0, _abi.PV_PARTITIONED), out


# ------------------------------------------------------------------------------------- M^-1 against the restatement
def _lambda_max(ctx, pb):
    ctx.set_controls(inner=_abi.Control(_abi.CTRL_FIXED_ITERS, 1, 0.0, 0.0))
    return ctx.precond_apply(cases.rng_blocks(pb, 3))[1].lambda_max


@pytest.mark.parametrize("name", pv.CONFIGS)
def test_inner_preconditioner_against_the_restatement(built, name):
    """alfd_inner_prec_apply with the option on agrees with the subclass within its measured tolerance and does NOT agree
    with the restatement on the exact values; lambda_max is bit-equal to option off.  ml_gmg_patch: every column, with
    base.check_operator (symmetry, definiteness) against the subclass."""
    cf = cpu.general_config(name)
    sub, par = cpu.subclass_reference(cf), cf.reference()
    off = _context(cf, "fp64")
    try:
        lam_off = _lambda_max(off, cf.pb)
        z_off = {what: off.inner_prec_apply(r) for what, r in base.inputs(cf).items()}
    finally:
        off.close()
    ctx = _context(cf, "fp32")
    try:
        _form(ctx.matrix_info(_abi.A), lanes=64, windowed=0, batch_major=0, value_indexed=0)
        _form(ctx.preconditioner_values(), requested=1, stored=1, used=1, reason=_abi.PV_NONE, family=1)
        for what, r in base.inputs(cf).items():
            z = ctx.inner_prec_apply(r)
            err, err_exact = base.rel(z, sub.apply(r)), base.rel(z, par.apply(r))
            print(f"{cf.name}, {what}: against the subclass {err:.2e}, against the restatement on A {err_exact:.2e}, "
                  f"option off against the restatement on A {base.rel(z_off[what], par.apply(r)):.2e}")
            assert err <= pv.TOL, (name, what, err)
            assert err_exact > pv.TOL, (name, what, err_exact)
            assert base.rel(z_off[what], par.apply(r)) <= pr.TOL
        if name == "ml_gmg_patch":
            m = base.dense_operator(lambda e: ctx.inner_prec_apply(e), sub.n)
            base.check_operator("library, fp32 values", cf.name, m, sub)
        assert _lambda_max(ctx, cf.pb) == lam_off
    finally:
        ctx.close()


# ------------------------------------------------------------------------------------- representable values
def test_representable_values_small_option_on_is_option_off(built):
    """n_0 = 2187 (the streaming kernel): alfd_inner_prec_apply, residual history, every count and the solution."""
    for name in ("cheb4_stokes", "ml_gmg_patch"):
        cf = cpu.general_config(name, representable=True)
        got = {}
        for values in ("fp64", "fp32"):
            ctx = _context(cf, values)
            try:
                if values == "fp32":
                    _form(ctx.preconditioner_values(), stored=1, used=1, family=1, flushed_to_zero=0)
                got[values] = ({k: ctx.inner_prec_apply(r) for k, r in base.inputs(cf).items()}, _solve(ctx, cf.pb))
            finally:
                ctx.close()
        for k in got["fp64"][0]:
            assert np.array_equal(got["fp64"][0][k], got["fp32"][0][k]), (name, k)
        assert got["fp32"][1]["status"] == _abi.OK
        _assert_same_solve(got["fp64"][1], got["fp32"][1], name)


@pytest.fixture(scope="module")
def window_problem():
    """Taylor-Hood at N = 10 with general values in A: the window kernel inside the real cycle (tensor prolongators,
    interface patch).  The batch-major planner halves row blocks until their dictionaries fit and still codes this
    operator, so its contexts are created with dictionary forms off (_context(..., dictionaries=False)): A, and the level
    and patch operators with it, then take the forms of a matrix whose values never repeat."""
    pb = problems.stokes3d_sphere(10, 1)
    general = pv.general_values(pb.mats["A"])
    cfg = _abi.Config.from_buffer_copy(base.config("ml_gmg_patch").cfg)
    levels = problems.tensor_prolongators(pb.params, min_coarse=100)
    return {False: base.Config("N = 10, general values", pv.with_A(pb, general), cfg, levels),
            True: base.Config("N = 10, representable values", pv.with_A(pb, pv.representable(general)), cfg, levels)}


@pytest.fixture(scope="module")
def window_reference(built, window_problem):
    """Option off on the representable values: one inner application and one solve."""
    cf = window_problem[True]
    ctx = _context(cf, "fp64", dictionaries=False)
    try:
        _form(ctx.matrix_info(_abi.A), lanes=64, windowed=1, batch_major=0, value_indexed=0)
        r = np.random.default_rng(71).uniform(-1, 1, cf.pb.block_sizes[0])
        return r, ctx.inner_prec_apply(r), _solve(ctx, cf.pb)
    finally:
        ctx.close()


@pytest.mark.parametrize("fuse", [0, 1, 2, 3])
def test_representable_values_window_kernel_in_the_cycle(built, window_problem, window_reference, fuse):
    cf = window_problem[True]
    r, z_off, solve_off = window_reference
    ctx = _context(cf, "fp32", fuse=fuse, dictionaries=False)
    try:
        _form(ctx.matrix_info(_abi.A), lanes=64, windowed=1, batch_major=0, value_indexed=0)
        _form(ctx.preconditioner_values(), stored=1, used=1, reason=_abi.PV_NONE, family=2, flushed_to_zero=0)
        assert np.array_equal(ctx.inner_prec_apply(r), z_off), fuse
        got = _solve(ctx, cf.pb)
        assert got["status"] == _abi.OK
        _assert_same_solve(solve_off, got, f"ml_fuse {fuse}")
    finally:
        ctx.close()


# ------------------------------------------------------------------------------------- a solve on general values
RESIDUAL_MARGIN = 2.0 * 1.0    # 2 x the measured ratio 1.0000, see test_solve_on_general_values


def _true_residual(pb, cfg, sol):
    """|| b - AA x || from the 8-byte operators in NumPy: AA = [[A + gamma Ct W C, Bt, Ct], [B, 0, 0], [C, 0, 0]]."""
    m = {k: v.to_scipy() for k, v in pb.mats.items() if k in ("A", "B", "Bt", "C", "Ct")}
    n = pb.block_sizes
    x0, x1, x2 = np.split(sol["x"], np.cumsum(n)[:-1])
    w = pb.inv_w_diag_squared()
    y0 = m["A"] @ x0 + cfg.gamma * (m["Ct"] @ (w * (m["C"] @ x0))) + m["Bt"] @ x1 + m["Ct"] @ x2
    r = np.concatenate(sol["rhs"]) - np.concatenate([y0, m["B"] @ x0, m["C"] @ x0])
    return float(np.linalg.norm(r)), float(np.linalg.norm(np.concatenate(sol["rhs"])))


@pytest.mark.parametrize("size", ["n0_2187", "n10_window"])
def test_solve_on_general_values(built, window_problem, size):
    """Option on, general values: status OK and the residual || b - AA x || recomputed in NumPy from the 8-byte operators
    meets the outer stop rule: at most RESIDUAL_MARGIN times the larger of the stop tolerance
    max(tol, reduce * || b ||) and the recomputed residual of the option-off solve.  RESIDUAL_MARGIN = 2 x the ratio
    (recomputed residual) / (FGMRES's own last residual) measured with the option off on an MI355X:
    1.0000 at n_0 = 2187 (5.153e-09 against 5.153e-09) and at N = 10 (4.859e-09 against 4.859e-09).
    Iteration counts against option off: one outer iteration and one inner iteration per inner solve of slack (a stop
    rule passed a step earlier or later).  Recorded on an MI355X (outer / inner / Mp), off and on:
    n_0 = 2187: 16 / 100 / 225 and 16 / 100 / 225;  N = 10: 10 / 54 / 262 and 10 / 54 / 262."""
    cf = cpu.general_config("ml_gmg_patch") if size == "n0_2187" else window_problem[False]
    got = {}
    for values in ("fp64", "fp32"):
        ctx = _context(cf, values, dictionaries=size == "n0_2187")
        try:
            if values == "fp32":
                _form(ctx.preconditioner_values(), stored=1, used=1, family=1 if size == "n0_2187" else 2)
            got[values] = _solve(ctx, cf.pb)
        finally:
            ctx.close()
    off, on = got["fp64"], got["fp32"]
    res_off, nb = _true_residual(cf.pb, cf.cfg, off)
    res_on, _ = _true_residual(cf.pb, cf.cfg, on)
    stop = max(cf.cfg.outer.tol, cf.cfg.outer.reduce * nb)
    print(f"{cf.name}: |b| = {nb:.3e}, stop {stop:.3e}; off: recomputed {res_off:.3e}, FGMRES {off['last_residual']:.3e}, "
          f"ratio {res_off / off['last_residual']:.4f}; on: recomputed {res_on:.3e}, FGMRES {on['last_residual']:.3e}, "
          f"ratio {res_on / on['last_residual']:.4f}")
    print(f"{cf.name}: outer / inner / Mp  off {off['outer']} / {off['inner']} / {off['mp']}   "
          f"on {on['outer']} / {on['inner']} / {on['mp']}")
    assert on["status"] == _abi.OK and off["status"] == _abi.OK
    assert on["lambda_max"] == off["lambda_max"]
    assert res_on <= RESIDUAL_MARGIN * max(stop, res_off), (res_on, res_off, stop)
    assert abs(on["outer"] - off["outer"]) <= 1, (on["outer"], off["outer"])
    inner_solves = max(on["papp"], off["papp"])                  # one solve on Aug per preconditioner application
    assert abs(on["inner"] - off["inner"]) <= inner_solves, (on["inner"], off["inner"])


# ------------------------------------------------------------------------------------- lifecycle, accounting
def test_setter_after_setup_unsets_the_context(built):
    cf = cpu.general_config("ml_gmg_patch")
    ctx = _context(cf, "fp64")
    try:
        rhs = ctx.augment_rhs(cases.rhs_of(cf.pb))
        ctx.set_preconditioner_values("fp64")                       # changes nothing: the setup stays
        assert ctx.solve(rhs)[1].status == _abi.OK
        ctx.set_preconditioner_values("fp32")
        _form(ctx.preconditioner_values(), requested=1, stored=1, used=0, reason=_abi.PV_NOT_APPLIED)
        with pytest.raises(solver.AlfdError) as e:
            ctx.solve(rhs)
        assert e.value.status == _abi.E_NOT_SETUP
        with pytest.raises(solver.AlfdError) as e:
            ctx.setup_coupling()
        assert e.value.status == _abi.E_INVALID and "needs alfd_setup" in str(e.value)
        ctx.setup(cf.pb.block_sizes)
        _form(ctx.preconditioner_values(), requested=1, stored=1, used=1, reason=_abi.PV_NONE)
        on = ctx.inner_prec_apply(np.ones(cf.pb.block_sizes[0]))
        ctx.set_preconditioner_values("fp32")                       # again nothing changes
        assert np.array_equal(ctx.inner_prec_apply(np.ones(cf.pb.block_sizes[0])), on)
        ctx.set_preconditioner_values("fp64")
        _form(ctx.preconditioner_values(), requested=0, stored=0, used=0, reason=_abi.PV_NOT_REQUESTED, copy_bytes=0)
        with pytest.raises(solver.AlfdError) as e:
            ctx.inner_prec_apply(np.ones(cf.pb.block_sizes[0]))
        assert e.value.status == _abi.E_NOT_SETUP
    finally:
        ctx.close()
    fresh = _context(cf, "fp32")
    try:                                                            # set before or after the upload: the same operator
        assert np.array_equal(fresh.inner_prec_apply(np.ones(cf.pb.block_sizes[0])), on)
    finally:
        fresh.close()


def test_setup_coupling_keeps_the_copy_and_equals_a_fresh_setup(built):
    cf = cpu.general_config("ml_gmg_patch")
    r = np.random.default_rng(81).uniform(-1, 1, cf.pb.block_sizes[0])
    ctx = _context(cf, "fp32")
    try:
        before = ctx.inner_prec_apply(r)
        solver.update_coupling(ctx, None, gamma=25.0)
        _form(ctx.preconditioner_values(), requested=1, stored=1, used=1, reason=_abi.PV_NONE)
        z, sol = ctx.inner_prec_apply(r), _solve(ctx, cf.pb)
        assert not np.array_equal(z, before)
    finally:
        ctx.close()
    cfg = _abi.Config.from_buffer_copy(cf.cfg)
    cfg.gamma = 25.0
    fresh = _context(base.Config(cf.name, cf.pb, cfg, cf.levels), "fp32")
    try:
        assert np.array_equal(fresh.inner_prec_apply(r), z)
        _assert_same_solve(_solve(fresh, cf.pb), sol, "setup_coupling against a fresh setup")
    finally:
        fresh.close()


def test_reupload_is_reflected_and_memory_does_not_grow(built):
    a, b = edge_content(_random_matrix(70), 91), edge_content(_random_matrix(200), 92)
    ca, cb = SpmvCase(a, 93), SpmvCase(b, 94)
    nan = np.full(a.nrows, np.nan)
    ctx = _fp32_context()
    try:
        ctx.set_matrix(_abi.A, a)
        assert np.array_equal(ctx.spmv_preconditioner(ca.x, nan), ca.s32)
        ctx.set_matrix(_abi.A, b)
        assert np.array_equal(ctx.spmv_preconditioner(cb.x, nan), cb.s32)
        assert ctx.preconditioner_values()["copy_bytes"] == 4 * b.nnz
        free = {}
        for k in range(1, 11):
            ctx.set_preconditioner_values("fp64")
            assert ctx.preconditioner_values()["stored"] == 0
            ctx.set_preconditioner_values("fp32")
            ctx.set_matrix(_abi.A, a if k % 2 else b)
            assert ctx.preconditioner_values()["stored"] == 1
            free[k] = ctx.device_memory()[0]
        print("free device bytes after each toggle and re-upload:", free)
        assert [free[k] for k in (4, 6, 8, 10)] == [free[2]] * 4, free
        assert [free[k] for k in (3, 5, 7, 9)] == [free[1]] * 4, free
        assert np.array_equal(ctx.spmv_preconditioner(cb.x, nan), cb.s32)
    finally:
        ctx.close()


def test_timer_reports_the_smaller_stream(built, window_problem):
    """With timing on, one alfd_inner_prec_apply streams exactly 4 nnz bytes fewer per level-0 A launch."""
    for cf in (cpu.general_config("ml_gmg_patch"), cpu.general_config("cheb4_stokes"), window_problem[False]):
        r = np.ones(cf.pb.block_sizes[0])
        seen = {}
        for values in ("fp64", "fp32"):
            ctx = _context(cf, values, dictionaries=cf is not window_problem[False])
            try:
                ctx.enable_timing(1)
                t0 = ctx.timing()["spmv_A"]
                ctx.inner_prec_apply(r)
                t1 = ctx.timing()["spmv_A"]
                seen[values] = (t1["launches"] - t0["launches"], t1["format_bytes"] - t0["format_bytes"],
                                t1["bytes"] - t0["bytes"])
            finally:
                ctx.close()
        launches, nnz = seen["fp64"][0], cf.pb.mats["A"].nnz
        print(f"{cf.name}: {launches} level-0 A launches, format bytes off {seen['fp64'][1]:.0f} on {seen['fp32'][1]:.0f}")
        assert launches > 0 and seen["fp32"][0] == launches
        assert seen["fp64"][1] - seen["fp32"][1] == 4.0 * nnz * launches, seen
        assert seen["fp64"][2] == seen["fp32"][2]                 # the algorithmic bytes are those of the operator
