"""Whole solves on the hierarchy with the Q1 level of the refined mesh (problems.refined_prolongators(q1_level=True)):
the refined stokes3d_sphere(6, 1) with the multilevel inner preconditioner reproduces the oracle's run pinned in
tests/golden/refined_q1_solves.json -- counts and residual history bit for bit -- with A in the form the library selects
and on the batch-major kernel with its 294 long rows in the side list ("batch_major_side_rows"); there also with the
side rows' tails behind the launch with the block-end tail ("ml_tail_side_rows") switched 1 / 0 / 1 on one context.
The new levels go through alfd_set_prolongator and the Galerkin products like any caller's.

ALFD_SPMV_WINDOW_MIN_BLOCKS = 1 lets operators of a few thousand rows take the long-row forms."""
import json
import os

import numpy as np
import pytest

import refined_cases as rc
import refined_q1_cases as qc
from fictitious_domain_al_preconditioners_amd import _abi, solver

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(autouse=True)
def _small_matrices_take_the_long_row_forms(built, monkeypatch):
    monkeypatch.setenv("ALFD_SPMV_WINDOW_MIN_BLOCKS", "1")          # read when a context is created


@pytest.fixture(scope="module")
def gold():
    return json.load(open(os.path.join(GOLDEN, "refined_q1_solves.json")))[f"{qc.SOLVE}/multilevel_q1_level"]


def _check(res, hist, gold):
    assert res.status == 0
    assert (res.outer_iterations, res.inner_iterations, res.mp_iterations) == \
        (gold["outer_iterations"], gold["inner_iterations"], gold["mp_iterations"])
    assert [float(h).hex() for h in hist] == gold["history"]


def test_solve_in_the_selected_form_reproduces_the_golden_run(gold):
    pb, lv = qc.mesh(qc.SOLVE), qc.levels(qc.SOLVE)
    assert [n for _, n in lv] == gold["level_sizes"] == [759, 375, 24]
    ctx = solver.Context(0)
    try:
        ctx.set_tunable("batch_major_side_rows", 0)
        solver.upload_problem(ctx, pb, qc.config(), lv)
        info = ctx.matrix_info(_abi.A)
        x, res = ctx.solve(ctx.augment_rhs(rc.rhs_of(pb)))
        hist = ctx.history()
    finally:
        ctx.close()
    print("Q1 level, selected form: batch_major", info["batch_major"], "outer", res.outer_iterations, "inner",
          res.inner_iterations)
    assert info["batch_major"] == 0                                   # rows of up to 807 entries refuse the form
    _check(res, hist, gold)


def test_solves_with_side_rows_and_their_tails_switched_on_one_context(gold):
    pb, lv = qc.mesh(qc.SOLVE), qc.levels(qc.SOLVE)
    ctx = solver.Context(0)
    runs = []
    try:
        ctx.set_tunable("batch_major_side_rows", 1)
        ctx.set_tunable("ml_tail_side_rows", 1)                       # a level qualifies at the setup
        solver.upload_problem(ctx, pb, qc.config(), lv)
        info, sr = ctx.matrix_info(_abi.A), ctx.side_rows(_abi.A)
        rhs = ctx.augment_rhs(rc.rhs_of(pb))
        for on in (1, 0, 1):                                          # and back: the switch leaves no state behind
            ctx.set_tunable("ml_tail_side_rows", on)
            before = ctx.fused_tail_launches()
            x, res = ctx.solve(rhs)
            runs.append((on, x, res, ctx.history().copy(), ctx.fused_tail_launches() - before))
    finally:
        ctx.close()
    print("Q1 level with side rows:", sr, "outer", runs[0][2].outer_iterations, "inner", runs[0][2].inner_iterations,
          "fused launches at ml_tail_side_rows 1 / 0 / 1:", [r[4] for r in runs])
    assert info["batch_major"] == 1 and sr["rows"] == 294
    for on, x, res, hist, fused in runs:
        _check(res, hist, gold)
        for a, b in zip(x, runs[1][1]):
            assert np.array_equal(a, b)
    assert runs[0][4] == runs[2][4]
    assert runs[1][4] < runs[0][4]                                    # 0: the fine level keeps the two-launch tail


def test_the_tunable_takes_0_and_1_only():
    ctx = solver.Context(0)
    try:
        for v in (0, 1):
            ctx.set_tunable("ml_tail_side_rows", v)
        for v in (-1, 2):
            with pytest.raises(solver.AlfdError) as e:
                ctx.set_tunable("ml_tail_side_rows", v)
            assert e.value.status == _abi.E_INVALID
    finally:
        ctx.close()
