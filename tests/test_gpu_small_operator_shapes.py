"""Per-operator row-block shapes of the long-row batch-major form (tunable "batch_major_small").

The level and patch operators the library builds get smaller row blocks when their default plan (96 rows, 4 waves)
leaves the chip under-filled.  Blocks only change the order in which rows are visited and what a block stages, so
every result must stay bit for bit what it was:

  kernel level   a long-row operator of 1 922 rows (Q2 vector Laplacian with grad-div, rows 9 000.. of the N = 10
                 operator: template-shared and plain batches) planned at every shape the rule can give -- rows per
                 block 16, 32, .. 96, every wave count that is instantiated (1, 2, 4) -- through "batch_major_rows" /
                 "batch_major_waves": all four epilogues out of NaN-prefilled outputs against the default shape and
                 against the oracle's canonical sums.  1 922 = 2 (mod 16 .. 96): every shape ends in a block of two
                 rows, less than one batch.  16 (CUs - 1) + 2 and 16 CUs + 2 rows at 16 rows per block give exactly
                 as many blocks as the device has compute units, and one more; 1 922 rows give fewer.
  pair launch    the same operator at 1, 2 and 4 waves with C at 16 / 32 / 64 lanes per row and a one-row C
                 (_check_pair of test_gpu_pair_launch.py).
  solve level    stokes3d_gmg_patch at N = 12 with the window threshold lowered (patch and level operators batch-major
                 with few blocks): batch_major_small 1, 0, 1 on one context solve bit for bit alike, and the patch
                 operator does carry another shape with the switch on.
  determinism    two setups report the same rows / waves / blocks for every operator.
  plan (no GPU)  alfd_host_stream_plan at the small row blocks decodes back and covers every row once; the rule as a
                 function (alfd_host_small_shape) leaves filled operators alone, stops at one batch per wave and at 16
                 rows, and never grows a block."""
import ctypes as C

import numpy as np
import pytest

from fictitious_domain_al_preconditioners_amd import _abi, problems, solver

ROWS = (16, 32, 48, 64, 80, 96)
WAVES = (1, 2, 4)
LONG_GEN = dict(dim=3, degree=2, ncomp=3, stokes=False, grad_div=True, gamma_grad_div=10.0, radius=0.1, immersed_refine=0)
FIRST_ROW = 9000


@pytest.fixture(scope="module")
def long_rows():
    """The N = 10 operator of test_gpu_spmv_epilogues.long_problem (27 783 rows, up to 375 entries per row)."""
    return problems.generate(n_cells=10, **LONG_GEN).mats["A"]


def _subset(a, nrows):
    m = a.slice_rows(FIRST_ROW, FIRST_ROW + nrows)
    assert m.nrows == nrows and m.ncols == a.ncols
    return m


@pytest.fixture
def ctx(built, monkeypatch):
    monkeypatch.setenv("ALFD_SPMV_WINDOW_MIN_BLOCKS", "1")     # read at alfd_create: a few thousand rows take the window forms
    c = solver.Context(0)
    yield c
    c.close()


def _plan(ctx, m, rows, waves):
    ctx.set_tunable("batch_major_rows", rows)
    ctx.set_tunable("batch_major_waves", waves)
    ctx.set_matrix(_abi.A, m)
    info = ctx.matrix_info(_abi.A)
    assert info["batch_major"] == 1 and info["lanes"] == 64 and info["batch_major_wide"] == 0, info
    assert (info["batch_major_rows"], info["batch_major_waves"], info["batch_major_small"]) == (rows, waves, 0), info
    assert 0 < info["shared_nnz"] < m.nnz, info                 # template-shared AND plain batches
    return info


def _all_epilogues(ctx, case):
    nan = np.full(case.m.nrows, np.nan)
    y0, _ = ctx.spmv(_abi.A, case.x, nan, mode=0)
    y1, _ = ctx.spmv(_abi.A, case.x, case.y0, mode=1, alpha=-0.75)
    y2 = ctx.spmv_scaled(_abi.A, case.x, case.d, nan)
    y3, y3s = ctx.spmv_scaled(_abi.A, case.x, case.d, nan, nan)
    return [y0, y1, y2, y3, y3s]


@pytest.mark.gpu
def test_every_shape_gives_the_bits_of_the_default_shape(ctx, long_rows):
    from oracle import oracle
    from spmv_reference import Case
    ctx.set_matrix(_abi.A, _subset(long_rows, 1922))
    cus = ctx.matrix_info(_abi.A)["batch_major_compute_units"]
    assert cus >= 8
    sizes = {"fewer blocks than CUs": 1922, "as many": 16 * (cus - 1) + 2, "one more": 16 * cus + 2}
    seen = set()
    for name, nrows in sizes.items():
        assert nrows % 16 == 2 and FIRST_ROW + nrows <= long_rows.nrows
        case = Case(_subset(long_rows, nrows), 41)
        want = [case.s, oracle.spmv(case.m, case.x, case.y0, mode=1, alpha=-0.75)[0], case.ds, case.s, case.ds]
        info = _plan(ctx, case.m, 96, 4)
        default = _all_epilogues(ctx, case)
        for got, ref in zip(default, want):
            assert not np.isnan(got).any() and np.array_equal(got, ref), (name, "default shape")
        for rows in (ROWS if nrows == 1922 else (16,)):
            assert nrows % rows == 2                            # the last block: two rows, less than one batch
            for waves in WAVES:
                info = _plan(ctx, case.m, rows, waves)
                assert info["batch_major_blocks"] == -(-nrows // rows), (name, rows, info)
                seen.add(np.sign(info["batch_major_blocks"] - cus))
                for k, (got, dflt, ref) in enumerate(zip(_all_epilogues(ctx, case), default, want)):
                    assert np.array_equal(got, dflt), (name, rows, waves, "epilogue output", k, "default shape")
                    assert np.array_equal(got, ref), (name, rows, waves, "epilogue output", k, "oracle")
    assert seen == {-1, 0, 1}, seen


@pytest.mark.gpu
@pytest.mark.parametrize("waves", WAVES)
def test_pair_launch_at_every_wave_count(built, monkeypatch, long_rows, waves):
    from test_gpu_pair_launch import _check_pair, _random_c
    # 96 x 20 rows take the window forms: the 1 922 rows of A do, no C below does (the second party reads plain CSR rows)
    monkeypatch.setenv("ALFD_SPMV_WINDOW_MIN_BLOCKS", "20")
    ctx = solver.Context(0)
    try:
        _pair_cases(ctx, long_rows, waves, _check_pair, _random_c)
    finally:
        ctx.close()


def _pair_cases(ctx, long_rows, waves, _check_pair, _random_c):
    m = _subset(long_rows, 1922)
    info = _plan(ctx, m, 32, waves)
    x = np.random.default_rng(3).uniform(-1.0, 1.0, m.ncols)
    for lanes in (16, 32, 64):
        rpb = 64 * waves // lanes                               # rows of C per workgroup of the pair grid
        sizes = {"one row": 1, "fewer": 7 * max(rpb, 1) + 3, "more": (info["batch_major_blocks"] + 9) * max(rpb, 1) + 3}
        for name, nrows in sizes.items():
            c = _random_c(nrows, m.ncols, lanes, 100 + lanes) if nrows > 1 else \
                problems.Csr(1, m.ncols, np.array([0, lanes + 3], np.int64), np.arange(0, 5 * (lanes + 3), 5, dtype=np.int32),
                             np.linspace(-1.0, 1.0, lanes + 3))
            ctx.set_matrix(_abi.C_, c)
            ci = ctx.matrix_info(_abi.C_)
            assert (ci["windowed"], ci["batch_major"]) == (0, 0), ci
            if nrows > 1:
                assert ci["lanes"] == lanes, ci
            _check_pair(ctx, m.nrows, nrows, x, (waves, lanes, name))


def _operators(ctx):
    out = {"A[S,S]": ctx.operator_info(_abi.OPERATOR_PATCH_SS), "A[S,:]": ctx.operator_info(_abi.OPERATOR_PATCH_S)}
    for level in range(1, 8):
        try:
            out[f"level {level}"] = ctx.operator_info(_abi.OPERATOR_LEVEL, level)
        except solver.AlfdError:
            break
    return {k: {f: v[f] for f in ("batch_major", "batch_major_rows", "batch_major_waves", "batch_major_small",
                                  "batch_major_blocks", "batch_major_batches", "nrows")} for k, v in out.items()}


@pytest.fixture(scope="module")
def patch_case():
    import cases
    _, cfg = cases.case("stokes3d_gmg_patch")
    pb = problems.stokes3d_sphere(12, 1)
    levels = problems.tensor_prolongators(pb.params, min_coarse=100)
    rhs = cases.rhs_of(pb)
    return pb, cfg, levels, rhs


def _setup(pb, cfg, levels):
    return solver.context_from_problem(pb, cfg, aggregates=levels)


@pytest.mark.gpu
def test_switch_on_off_on_solves_bit_for_bit(built, monkeypatch, patch_case):
    monkeypatch.setenv("ALFD_SPMV_WINDOW_MIN_BLOCKS", "8")
    pb, cfg, levels, rhs = patch_case
    ctx = _setup(pb, cfg, levels)
    try:
        rhs = ctx.augment_rhs(rhs)
        runs, shapes = [], []
        for small in (1, 0, 1):
            if runs:
                ctx.set_tunable("batch_major_small", small)
                ctx.setup(ctx.block_sizes)                      # the switch takes effect at the next alfd_setup
            shapes.append(_operators(ctx))
            x, res = ctx.solve(rhs, raise_on_failure=False)
            runs.append((x, res, ctx.history().copy()))
    finally:
        ctx.close()
    print("switch on :", shapes[0])
    print("switch off:", shapes[1])
    on, off = shapes[0], shapes[1]
    assert shapes[2] == on
    assert off["A[S,S]"]["batch_major"] == 1 and (off["A[S,S]"]["batch_major_rows"], off["A[S,S]"]["batch_major_waves"]) == (96, 4)
    assert all(not v["batch_major_small"] for v in off.values()), off
    assert on["A[S,S]"]["batch_major_small"] == 1, on
    assert (on["A[S,S]"]["batch_major_rows"], on["A[S,S]"]["batch_major_waves"]) != (96, 4), on
    assert on["A[S,S]"]["batch_major_blocks"] > off["A[S,S]"]["batch_major_blocks"], (on, off)
    x0, r0, h0 = runs[0]
    print("outer", r0.outer_iterations, "inner", r0.inner_iterations, "mp", r0.mp_iterations)
    assert r0.status == 0 and r0.outer_iterations > 0 and r0.inner_iterations > 0
    for xa, ra, ha in runs[1:]:
        assert (ra.status, ra.outer_iterations, ra.inner_iterations, ra.mp_iterations, ra.inner_failures) == \
               (r0.status, r0.outer_iterations, r0.inner_iterations, r0.mp_iterations, r0.inner_failures)
        assert np.array_equal(ha, h0)
        assert len(xa) == len(x0)
        for a, b in zip(xa, x0):
            assert np.array_equal(a, b)


@pytest.mark.gpu
def test_two_setups_plan_the_same_shapes(built, monkeypatch, patch_case):
    monkeypatch.setenv("ALFD_SPMV_WINDOW_MIN_BLOCKS", "8")
    pb, cfg, levels, _ = patch_case
    shapes = []
    for _ in range(2):
        ctx = _setup(pb, cfg, levels)
        try:
            shapes.append(_operators(ctx))
        finally:
            ctx.close()
    assert shapes[0] == shapes[1], shapes
    assert any(v["batch_major_small"] for v in shapes[0].values()), shapes[0]


def _rule(nrows, blocks, batches, rows=96, waves=4, cus=256):
    r, w = C.c_int32(-1), C.c_int32(-1)
    rc = solver.load_library().alfd_host_small_shape(nrows, blocks, batches, rows, waves, cus, C.byref(r), C.byref(w))
    assert rc == _abi.OK
    return r.value, w.value


def test_small_row_blocks_decode_back_and_the_rule_is_a_function(built, long_rows):
    """No GPU: the plan at every row block the rule can give, on the partition-free path that replicated level and patch
    operators of a partitioned context take as well (they are planned like the operators of one rank)."""
    m = _subset(long_rows, 1922)
    blocks = {}
    for rows in ROWS:
        info = solver.host_stream_plan(m, row_block=rows)
        assert info["ok"] and info["decode_mismatches"] == 0 and info["rows_covered"] == m.nrows, (rows, info)
        assert info["max_rows"] <= rows and info["blocks"] == -(-m.nrows // rows), (rows, info)
        blocks[rows] = info
    d = blocks[96]
    # 21 blocks x 4 waves against 4 096 waves (half the slots of 256 CUs): under-filled.  The rule stops at one batch per
    # wave (rounded up to whole 16-row batches) ...
    rows, waves = _rule(m.nrows, d["blocks"], d["batches"])
    per_batch = m.nrows / d["batches"]
    assert waves == 4 and rows % 16 == 0 and 16 <= rows < 96
    assert rows >= 4 * per_batch and rows - 16 < max(4 * per_batch, 16), (rows, per_batch)
    assert _rule(m.nrows, d["blocks"], d["batches"]) == (rows, waves)              # a function of its arguments
    # ... leaves an operator alone whose default plan reaches 16 waves per compute unit, on a device of whatever size ...
    assert _rule(96 * 1024, 1024, 96 * 1024 // 16) == (96, 4)
    assert _rule(96 * 256, 256, 96 * 256 // 16, cus=64) == (96, 4)
    assert _rule(96 * 256, 256, 96 * 256 // 16, cus=65) != (96, 4)
    # ... 500 blocks of 96 rows: 4 096 waves take blocks of 46 rows, whole batches 32; with 16-row batches one batch per
    # wave is 64 rows and the rule stops there, with 4-row batches it goes down to the 32
    assert _rule(96 * 500, 500, 96 * 500 // 16) == (64, 4)
    assert _rule(96 * 500, 500, 96 * 500 // 4) == (32, 4)
    # ... never below 16 rows, never above the default
    assert _rule(400, 5, 100) == (16, 4)
    assert _rule(4000, 84, 42 * 6, rows=48) == (48, 4)
