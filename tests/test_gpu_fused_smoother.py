"""The fused smoother steps of the multigrid inner preconditioner (tunable "ml_fuse": aug_tail_kernel) against the
separate launches, on ONE context: the same solve with ml_fuse 1 and 0 must give the same bits -- solution blocks,
residual history, outer / inner / mp counts.

Coverage of the paths (asserted below from the host copies of the operators, by the rule the library uses for
the row-list form: fewer than half of the rows non-empty):
  * Ct in row-list form: the fine Ct of every Stokes case (the immersed body touches few velocity rows);
  * Ct NOT in row-list form: the patch operator Ct[S, :] (every row non-empty by construction) and the coarsest
    levels of the prolongator hierarchies;
  * smoother degree 1 (cheb_init without the residual copy, TAIL_RES_INIT_ADD): the *_deg1 variants;
  * patch degree 0: stokes3d_gmg and the aggregation cases; patch degree 1: stokes3d_gmg_patch_deg1."""
import numpy as np
import pytest

import cases
from fictitious_domain_al_preconditioners_amd import solver

pytestmark = pytest.mark.gpu

CASES = ["stokes3d_gmg", "stokes3d_gmg_patch", "elliptic_modified_gmg_patch", "stokes3d_multilevel",
         "stokes3d_bench_settings", "stokes3d_multilevel_deg1", "stokes3d_gmg_patch_deg1"]


def _case(name):
    if name.endswith("_deg1"):
        pb, cfg = cases.case(name[:-len("_deg1")])
        cfg.ml_smooth_degree = 1
        cfg.ml_smooth_degree_coarse = 0
        if cfg.ml_patch_degree > 0:
            cfg.ml_patch_degree = 1
        return pb, cfg
    return cases.case(name)


def _row_list_form(m):
    """DevCsr::sparse as upload_matrix decides it."""
    nonempty = int(np.count_nonzero(np.diff(m.row_ptr)))
    return nonempty * 2 < m.nrows


def _ct_forms(pb, levels):
    """Row-list form (True / False) of Ct on every level of a CSR-prolongator hierarchy, level 0 first."""
    forms = [_row_list_form(pb.mats["Ct"])]
    ct = pb.mats["Ct"].to_scipy()
    for entry in levels:
        if not hasattr(entry[0], "row_ptr"):
            break
        ct = (entry[0].to_scipy().T @ ct).tocsr()
        forms.append(int(np.count_nonzero(np.diff(ct.indptr))) * 2 < ct.shape[0])
    return forms


def _solve(ctx, rhs, fuse):
    ctx.set_tunable("ml_fuse", fuse)
    x, res = ctx.solve(rhs, raise_on_failure=False)
    return x, res, ctx.history().copy()


@pytest.mark.parametrize("name", CASES)
def test_fused_equals_unfused_bit_for_bit(built, name):
    pb, cfg = _case(name)
    levels = cases.aggregates_of(pb, cfg)
    osys = cases.oracle_system(pb, cfg)
    rhs = cases.prepared_rhs(osys, pb, cfg)
    ctx = solver.context_from_problem(pb, cfg, aggregates=levels)
    try:
        x1, r1, h1 = _solve(ctx, rhs, 1)
        x0, r0, h0 = _solve(ctx, rhs, 0)
        x2, r2, h2 = _solve(ctx, rhs, 1)      # and back: the switch leaves no state behind
    finally:
        ctx.close()
    print(name, "outer", r1.outer_iterations, "inner", r1.inner_iterations, "mp", r1.mp_iterations,
          "status", r1.status, "history", h1.size)
    assert r1.outer_iterations > 0 and r1.inner_iterations > 0
    for xa, ra, ha in ((x1, r1, h1), (x2, r2, h2)):
        assert (ra.status, ra.outer_iterations, ra.inner_iterations, ra.mp_iterations, ra.inner_failures) == \
               (r0.status, r0.outer_iterations, r0.inner_iterations, r0.mp_iterations, r0.inner_failures)
        assert np.array_equal(ha, h0)
        assert len(xa) == len(x0)
        for a, b in zip(xa, x0):
            assert np.array_equal(a, b)


def test_cases_cover_both_ct_forms(built):
    """The cases above reach aug_tail_kernel with Ct in row-list form and in plain form."""
    pb, cfg = cases.case("stokes3d_gmg")
    forms = _ct_forms(pb, cases.aggregates_of(pb, cfg))
    print("stokes3d_gmg: Ct in row-list form per level:", forms)
    assert forms[0]
    assert not all(forms), forms
    pb, cfg = cases.case("stokes3d_gmg_patch")
    assert cfg.ml_patch_degree > 0 and _row_list_form(pb.mats["Ct"])    # the patch rows: all non-empty, plain form
    pb, cfg = cases.case("stokes3d_gmg")
    assert cfg.ml_patch_degree == 0


def test_env_knob_and_tunable(built):
    """ALFD_ML_FUSE is read at alfd_create; an unknown tunable name is still refused."""
    import os
    import subprocess
    import sys
    ctx = solver.Context(0)
    try:
        ctx.set_tunable("ml_fuse", 0)
        ctx.set_tunable("ml_fuse", 1)
        with pytest.raises(Exception):
            ctx.set_tunable("ml_fuse_not_a_name", 1)
    finally:
        ctx.close()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = ("import sys; sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
            "import cases\n"
            "from fictitious_domain_al_preconditioners_amd import solver\n"
            "pb, cfg = cases.case('stokes3d_gmg_patch')\n"
            "osys = cases.oracle_system(pb, cfg)\n"
            "rhs = cases.prepared_rhs(osys, pb, cfg)\n"
            "ctx = solver.context_from_problem(pb, cfg, aggregates=cases.aggregates_of(pb, cfg))\n"
            "ctx.enable_timing(2)\n"
            "x, res = ctx.solve(rhs)\n"
            "t = ctx.timing()\n"
            "print('LAUNCHES', sum(v['launches'] for v in t.values()), res.inner_iterations)\n"
            % (root, os.path.join(root, "tests")))
    counts = {}
    for fuse in ("0", "1"):
        out = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, ALFD_ML_FUSE=fuse), check=True,
                             capture_output=True, text=True, timeout=600).stdout
        line = [ln for ln in out.splitlines() if ln.startswith("LAUNCHES")][-1].split()
        counts[fuse] = (int(line[1]), int(line[2]))
    print("timed launches, inner iterations per solve: unfused", counts["0"], "fused", counts["1"])
    assert counts["0"][1] == counts["1"][1]
    assert counts["1"][0] < counts["0"][0]
