"""The library on the operators of a locally refined background mesh (generate(local_refine=1)): two families of
cell matrices (h and h / 2), condensed rows next to the refinement edge (Q2 weights 3/8, 3/4 and -1/8), lone-diagonal
hanging rows inside the lattice, empty hanging rows in Bt / B / Ct, and a velocity space without tensor-product
transfers.  Case: refined stokes3d_sphere(6, 1), 13 335 + 687 + 78 unknowns, 2 592 hanging velocity rows.

SpMV of A, Bt, B, Ct in the storage form the library selects and in every form the ALFD_SPMV_* variables and the
batch_major tunable can force on it (the switches of tests/test_gpu_launch_shapes.py; the launch record of each is
printed), all four epilogues through spmv_reference.Case (oracle's canonical sums bit for bit, np.longdouble bound).
Seen on the MI355X: A takes the stream kernel as selected and the general window kernel under every window switch
-- its 14 472 distinct values in 13 335 rows leave no block dictionary and its rows of up to 807 entries are beyond
the 384 the batch-major form takes, so the value-indexed and batch-major switches fall through to those two; B
stream / window, Bt plain<16> / window_group<16>, Ct (0.6 entries per row) the sparse-row kernel under every switch;
alfd_system_apply and alfd_precond_apply bit for bit; whole solves with three inner preconditioners like
tests/test_gpu_parity.py (same outer / inner / pressure-mass counts, residual history bit for bit), also on the
refined laplace2d_circle(16, 3)."""
import json
import os

import numpy as np
import pytest

import refined_cases as rc
from fictitious_domain_al_preconditioners_amd import _abi, problems, solver
from oracle import oracle
from spmv_reference import Case

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
WINDOW_ON = {"ALFD_SPMV_WINDOW_MIN_BLOCKS": 1, "ALFD_SPMV_WINDOW_SHORT_MIN_BLOCKS": 1}
# name -> (environment before alfd_create, batch_major tunable or None = as the context defaults)
FORMS = {
    "selected": ({}, None),
    "no_window": ({"ALFD_SPMV_WINDOW": 0}, 0),
    "window": (WINDOW_ON, 0),
    "window_xcd_order": (dict(WINDOW_ON, ALFD_SPMV_WINDOW_XCD=1, ALFD_SPMV_VI_XCD=1), 0),
    "window_no_dictionary": (dict(WINDOW_ON, ALFD_SPMV_VALUE_INDEX=0), 0),
    "window_in_order_value_indexed": (dict(WINDOW_ON, ALFD_SPMV_VI_BATCHED=0), 0),
    "window_general_on_coded": (dict(WINDOW_ON, ALFD_SPMV_VI_BATCHED=0, ALFD_SPMV_VI_R=0), 0),
    "window_short_scale_1": (dict(WINDOW_ON, ALFD_SPMV_WINDOW_SHORT=1), 0),
    "window_short_off": (dict(WINDOW_ON, ALFD_SPMV_WINDOW_SHORT=0), 0),
    "batch_major": (WINDOW_ON, 1),
    "batch_major_default_thresholds": ({}, 1),
}
OPERATORS = ("A", "Bt", "B", "Ct")


@pytest.fixture(scope="module")
def stokes(built):
    return rc.problem("stokes3d_sphere")


@pytest.fixture(scope="module")
def spmv_cases(stokes):
    """One spmv_reference.Case per operator: inputs and both references computed once, read-only."""
    return {name: Case(stokes.mats[name], 900 + k) for k, name in enumerate(OPERATORS)}


def test_the_case_is_what_the_library_has_not_seen(stokes):
    assert stokes.block_sizes == [13335, 687, 78]
    A = stokes.mats["A"]
    ln = np.diff(A.row_ptr)
    hanging = np.repeat(stokes.vecs["u_hanging"], 3) != 0
    assert hanging.sum() == 2592 and np.all(ln[hanging] == 1)
    assert np.all(np.diff(stokes.mats["Bt"].row_ptr)[hanging] == 0) and np.all(np.diff(stokes.mats["Ct"].row_ptr)[hanging] == 0)
    assert np.unique(ln).size > 30                                  # 41 different row lengths
    assert ln.max() == 807                                          # a base-cell corner with hanging neighbours: beyond
    #                                                                 the 384 entries the long-row batch-major form takes


@pytest.mark.parametrize("form", sorted(FORMS))
@pytest.mark.parametrize("name", OPERATORS)
def test_spmv_bitwise_in_every_form(stokes, spmv_cases, monkeypatch, name, form):
    env, batch_major = FORMS[form]
    for k, v in env.items():
        monkeypatch.setenv(k, str(v))
    slot = _abi.SLOT_BY_NAME[name]
    ctx = solver.Context(0)
    try:
        if batch_major is not None:
            ctx.set_tunable("batch_major", batch_major)
        ctx.set_matrix(slot, stokes.mats[name])
        info = ctx.matrix_info(slot)
        spmv_cases[name].check(ctx, (name, form), slot=slot, mode1=True)
        rec = ctx.last_spmv_launch()
        print("refined", name, form, {k: info[k] for k in ("lanes", "windowed", "value_indexed", "batch_major")},
              {k: rec[k] for k in ("family_name", "lanes", "R", "U", "xcd_order", "grid")})
    finally:
        ctx.close()


@pytest.mark.parametrize("blocks", ["bricks_from_points", "rcb_from_points"])
def test_spmv_bitwise_on_row_blocks_from_the_support_points(stokes, spmv_cases, blocks):
    """What the front end does with a mesh it knows only through support points: row blocks for A from bricks /
    recursive bisection of the refined lattice's points.  Rows of up to 807 entries are more than the batch-major
    form takes (384), so the library may keep another form; whichever it keeps gives the oracle's bits."""
    pts = problems.row_support_points(stokes)
    ctx = solver.Context(0)
    try:
        ctx.set_tunable("batch_major", 1)
        if blocks == "bricks_from_points":
            ctx.set_row_blocks(_abi.A, *solver.brick_blocks_from_points(pts, (16, 4, 1)))
        else:
            ctx.set_row_blocks(_abi.A, *solver.row_blocks_from_points(pts, 192))
        ctx.set_matrix(_abi.A, stokes.mats["A"])
        info = ctx.matrix_info(_abi.A)
        spmv_cases["A"].check(ctx, blocks, mode1=True)
        print("refined A", blocks, {k: info[k] for k in ("lanes", "windowed", "value_indexed", "batch_major")},
              ctx.last_spmv_launch()["family_name"])
    finally:
        ctx.close()


def _blocks(pb, seed):
    rng = np.random.default_rng(seed)
    return [rng.uniform(-1.0, 1.0, n) for n in pb.block_sizes]


def test_system_and_preconditioner_apply_bitwise(stokes):
    cfg = rc.config("stokes3d_sphere", "chebyshev")
    ctx = solver.context_from_problem(stokes, cfg)
    try:
        osys = oracle.system_from_problem(stokes)
        src = _blocks(stokes, 10)
        code, ref = osys.system_apply(cfg, src)
        assert code == 0
        for g, r in zip(ctx.system_apply(src), ref):
            assert np.array_equal(g, r)
        code, oref = osys.augment_rhs(cfg, rc.rhs_of(stokes))
        for g, r in zip(ctx.augment_rhs(rc.rhs_of(stokes)), oref):
            assert np.array_equal(g, r)
        src = _blocks(stokes, 20)
        got, res = ctx.precond_apply(src)
        code, ref, ores = osys.precond_apply(cfg, src)
        assert code == 0
        assert (res.inner_iterations, res.mp_iterations) == (ores.inner_iterations, ores.mp_iterations)
        assert res.lambda_max == ores.lambda_max
        for g, r in zip(got, ref):
            assert np.array_equal(g, r)
    finally:
        ctx.close()


def _sa_build_args(pb):
    return dict(block_size=pb.params["ncomp"], threshold=0.02, max_aggregate_nodes=8, damping=4.0 / 3.0,
                min_coarse=300 if pb.params["ncomp"] > 1 else 50, max_row_entries=4)


@pytest.mark.parametrize("prec", rc.PRECONDITIONERS + ("truncated_sa",))
@pytest.mark.parametrize("name", rc.SOLVE_CASES)
def test_solve_matches_the_oracle(built, name, prec):
    pb, cfg = rc.problem(name), rc.config(name, prec)
    ctx = solver.Context(0)
    try:
        if prec == "truncated_sa":
            # alfd_build_smoothed_aggregation_truncated from the uploaded operators; the oracle gets the same CSR levels
            ctx.set_matrix(_abi.A, pb.mats["A"])
            ctx.set_matrix(_abi.C_, pb.mats["C"])
            ctx.set_matrix(_abi.CT, pb.mats["Ct"])
            ctx.set_diag(_abi.INVW, pb.inv_w_diag_squared())
            ctx.configure(cfg)
            levels = ctx.build_smoothed_aggregation(**_sa_build_args(pb))
            assert len(levels) >= 1 and int(np.diff(levels[0][0].row_ptr).max()) <= 4
            hanging = np.repeat(pb.vecs["u_hanging"], pb.params["ncomp"]) != 0
            assert not np.diff(levels[0][0].row_ptr)[hanging].any()       # lone diagonals are left out of the aggregates
            solver.upload_problem(ctx, pb, cfg, None)                     # keeps the hierarchy built above
        else:
            levels = rc.levels(name, prec)
            solver.upload_problem(ctx, pb, cfg, levels)
        rhs = ctx.augment_rhs(rc.rhs_of(pb))
        x, res = ctx.solve(rhs)
        hist = ctx.history()
        ax = ctx.system_apply(x)
    finally:
        ctx.close()
    osys = oracle.system_from_problem(pb, aggregates=levels)
    code, orhs = osys.augment_rhs(cfg, rc.rhs_of(pb))
    assert code == 0 and all(np.array_equal(a, b) for a, b in zip(rhs, orhs))
    code, ox, ores, ohist = osys.solve(cfg, orhs)
    assert code == 0 and res.status == 0
    print("refined solve", name, prec, "outer", res.outer_iterations, "inner", res.inner_iterations,
          "mp", res.mp_iterations, "levels", [lv[1] for lv in levels or []])
    assert (res.outer_iterations, res.inner_iterations, res.mp_iterations) == \
        (ores.outer_iterations, ores.inner_iterations, ores.mp_iterations)
    assert len(hist) == len(ohist) and np.array_equal(hist, ohist)
    for g, r in zip(x, ox):
        assert np.allclose(g, r, rtol=1e-9, atol=1e-10 * max(np.abs(r).max(), 1e-30))
    if prec != "truncated_sa":                                            # the committed pin of the oracle's run
        gold = json.load(open(os.path.join(GOLDEN, "refined_solves.json")))[f"{name}/{prec}"]
        assert (res.outer_iterations, res.inner_iterations, res.mp_iterations) == \
            (gold["outer_iterations"], gold["inner_iterations"], gold["mp_iterations"])
        assert [float(h).hex() for h in hist] == gold["history"]
    # the GPU solution really solves the condensed system, hanging and Dirichlet rows included
    r = np.concatenate([a - b for a, b in zip(rhs, ax)])
    assert np.linalg.norm(r) <= 10 * max(cfg.outer.tol, cfg.outer.reduce * res.initial_residual)
