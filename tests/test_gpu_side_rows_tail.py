"""The tails of side rows behind the launch with the block-end tail (tunable "ml_tail_side_rows",
spmv_side_rows_tail_kernel): an operator with side rows ("batch_major_side_rows") has rows without a block end; their
row sums and tails come from a launch of one wave per side row that follows the batch-major launch.

The kernel through alfd_spmv_tail_step on launch_shape_cases.long_rows(3365, "few"), whose six planted rows of
1025 .. 511 entries are one 64 x 8-entry pass of the side kernel and less, exactly two passes, and two passes and one
entry: form 0 (A launch with the epilogue + side-row tails, then the rows party of the tail) against form 1 (y = A x,
then the whole tail launch), bit for bit, with the helpers and the conventions of tests/test_gpu_tail_in_spmv.py.  Ct
lists the 1025- and the 512-entry row, so both branches of the kernel's lane 0 run on long rows: y stored and the tail
left to the rows party, or the tail applied and y left alone.

Solver level: one inner-preconditioner application on the refined stokes3d_sphere(6, 1) with the Q1-level hierarchy."""
import re

import numpy as np
import pytest

import launch_shape_cases as lc
import refined_cases as rc
import refined_q1_cases as qc
from fictitious_domain_al_preconditioners_amd import _abi, solver
from test_gpu_tail_in_spmv import MODES, NT, Step, _compare, _ct, _run

pytestmark = pytest.mark.gpu
N = 3365
ROWS = 96                                                             # rows per block
LONG = dict(zip((1025, 1024, 1023, 513, 512, 511), lc.long_structure(N)[2]))       # entries -> row
# rows of Ct: two of the six long rows, and rows where a block begins and ends (0 and N - 1 are empty rows of A)
LISTED = sorted({LONG[1025], LONG[512], 0, 95, 96, 191, 192, 1727, 1728, N - 1})


@pytest.fixture
def ctx(built, monkeypatch):
    monkeypatch.setenv("ALFD_SPMV_WINDOW_MIN_BLOCKS", "1")
    c = solver.Context(0)
    c.set_tunable("batch_major", 1)
    c.set_tunable("batch_major_side_rows", 1)
    c.set_tunable("batch_major_waves", 4)
    c.set_tunable("batch_major_rows", ROWS)
    c.set_tunable("ml_tail_side_rows", 1)
    c.set_matrix(_abi.A, lc.long_rows(N, "few"))
    info, sr = c.matrix_info(_abi.A), c.side_rows(_abi.A)
    assert info["batch_major"] == 1 and info["batch_major_waves"] == 4 and info["batch_major_wide"] == 0, info
    assert sr["rows"] == 6 and sr["longest"] == 1025, sr
    yield c
    c.close()


def test_the_planted_ct():
    A = lc.long_rows(N, "few")
    ln = np.diff(np.asarray(A.row_ptr))
    assert sorted(LONG.values()) == list(np.flatnonzero(ln > 384)) and all(ln[r] == k for k, r in LONG.items())
    assert len(LISTED) == 10 and 2 * len(LISTED) < N
    assert sum(r in LISTED for r in LONG.values()) == 2
    assert all(r % ROWS in (0, ROWS - 1) or r == N - 1 for r in LISTED if r not in LONG.values())


def test_form_0_equals_form_1_in_every_mode(ctx):
    """_compare: res, d, z, zout bit-equal; y = A x on the rows of Ct, its fill on all others (the four unlisted long
    rows included); the counter of fused launches grows by one per form-0 call, by none per form-1 call."""
    st, ct = Step(N, 71), _ct(N, LISTED)
    _compare(ctx, st, ct, "side rows", modes=MODES)
    # the sums themselves, on the two long rows that store them, against the plain product
    y, _ = ctx.spmv(_abi.A, st.x, np.full(N, np.nan), mode=0)
    a = _run(ctx, 0, _abi.TAIL_RES, st, ct)
    listed = np.asarray(LISTED)
    assert np.array_equal(a["y"][listed], y[listed])
    unlisted = [r for r in LONG.values() if r not in LISTED]
    assert len(unlisted) == 4 and np.array_equal(a["y"][unlisted], st.fill[unlisted])
    assert np.array_equal(a["res"][unlisted], st.rin[unlisted] - y[unlisted])        # Ct has no entry there: res = rin - A x


def test_form_0_equals_form_1_beside_the_pair_launch(ctx):
    from test_gpu_pair_launch import _random_c
    ctx.set_matrix(_abi.C_, _random_c(NT, N, 32, 9))
    assert ctx.matrix_info(_abi.C_)["batch_major"] == 0
    w = np.random.default_rng(3).uniform(0.5, 2.0, NT)
    for fuse in (3, 1):                     # slot A is a fine-level operator: the pair launch takes it from ml_fuse 3 on
        ctx.set_tunable("ml_fuse", fuse)
        _compare(ctx, Step(N, 72), _ct(N, LISTED), ("side rows, pair", fuse), slot_c=_abi.C_, w=w)


def test_refusals(ctx):
    st, ct = Step(N, 73), _ct(N, LISTED)
    # the tunable 0: an operator with side rows has no launch with the block-end tail
    ctx.set_tunable("ml_tail_side_rows", 0)
    before = ctx.fused_tail_launches()
    for mode in MODES:
        with pytest.raises(solver.AlfdError) as e:
            _run(ctx, 0, mode, st, ct)
        assert e.value.status == _abi.E_UNSUPPORTED, mode
    ref = _run(ctx, 1, _abi.TAIL_STEP, st, ct)
    assert ctx.fused_tail_launches() == before
    ctx.set_tunable("ml_tail_side_rows", 1)
    got = _run(ctx, 0, _abi.TAIL_STEP, st, ct)
    assert ctx.fused_tail_launches() == before + 1
    for k in ("res", "d", "z"):
        assert np.array_equal(got[k], ref[k]), k
    # an output at the address of x: refused before any launch
    for mode, name in ((_abi.TAIL_STEP, "z"), (_abi.TAIL_STEP, "d"), (_abi.TAIL_STEP, "res"), (_abi.TAIL_LAST, "z"),
                       (_abi.TAIL_LAST_ADD, "zout"), (_abi.TAIL_RES, "res"), (_abi.TAIL_RES_INIT, "z"), (_abi.TAIL_RES, "y")):
        before = ctx.fused_tail_launches()
        with pytest.raises(solver.AlfdError) as e:
            _run(ctx, 0, mode, st, ct, **{name: "x"})
        assert e.value.status == _abi.E_INVALID, (mode, name)
        assert ctx.fused_tail_launches() == before
    # mode 5 has no epilogue, with side rows or without
    before = ctx.fused_tail_launches()
    with pytest.raises(solver.AlfdError) as e:
        _run(ctx, 0, _abi.TAIL_RES_INIT_ADD, st, ct)
    assert e.value.status in (_abi.E_INVALID, _abi.E_UNSUPPORTED)
    assert ctx.fused_tail_launches() == before
    _run(ctx, 1, _abi.TAIL_RES_INIT_ADD, st, ct)


def test_inner_preconditioner_application_with_and_without(built, monkeypatch, capfd):
    """One application of the multilevel inner preconditioner on the refined (6, 1) sphere, side rows on, Q1-level
    hierarchy: the bits of "ml_tail_side_rows" = 0 with 1.  The setup's log line says whether the fine level qualifies
    for the tails inside the A launch; where it does, the counter of fused launches must grow."""
    monkeypatch.setenv("ALFD_SPMV_WINDOW_MIN_BLOCKS", "1")
    monkeypatch.setenv("ALFD_LOG_UPLOAD", "1")
    pb = qc.mesh(qc.SOLVE)
    r = np.random.default_rng(41).uniform(-1.0, 1.0, pb.block_sizes[0])
    out, fused, fine = {}, {}, {}
    for on in (0, 1):
        ctx = solver.Context(0)
        try:
            ctx.set_tunable("batch_major_side_rows", 1)
            ctx.set_tunable("ml_tail_side_rows", on)
            capfd.readouterr()
            solver.upload_problem(ctx, pb, qc.config(), qc.levels(qc.SOLVE))
            log = capfd.readouterr().err
            assert ctx.side_rows(_abi.A)["rows"] == 294
            m = re.findall(r"hierarchy 0 level 0 \((\d+) rows, (\d+) in Ct\): tails inside the A launch (possible|not possible)", log)
            assert m, log[-2000:]
            fine[on] = m[-1][2] == "possible"
            before = ctx.fused_tail_launches()
            out[on] = ctx.inner_prec_apply(r)
            fused[on] = ctx.fused_tail_launches() - before
        finally:
            ctx.close()
    print("fine level qualifies at ml_tail_side_rows 0 / 1:", fine[0], fine[1], "fused launches", fused[0], fused[1])
    assert np.array_equal(out[0], out[1])
    assert not fine[0]                      # side rows, tunable 0: the two-launch tail
    assert fine[1]                          # nothing but the side rows kept this level from the form
    assert fused[1] > fused[0]
