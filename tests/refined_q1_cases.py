"""The Q1 level of the refined-mesh hierarchies (problems.refined_prolongators(q1_level=True)): the meshes and the
solve case shared by tests/test_refined_q1_level.py, tests/test_gpu_refined_q1_level.py, tests/test_gpu_side_rows_tail.py
and tests/golden/make_refined_q1_golden.py."""
import functools

import refined_cases as rc
from fictitious_domain_al_preconditioners_amd import problems

MESHES = ("stokes2d", "stokes3d_grad_div", "stokes3d_sphere", "stokes3d_sphere_cuthill_mckee")
MIN_COARSE = {"stokes2d": 20, "stokes3d_grad_div": 20, "stokes3d_sphere": 100, "stokes3d_sphere_cuthill_mckee": 100}
SOLVE = "stokes3d_sphere"                     # refined (6, 1) sphere, the settings of rc.config(SOLVE, "multilevel")


@functools.lru_cache(maxsize=None)
def mesh(name):
    if name in rc.PARTLY_REFINED:
        return problems.generate(local_refine=1, assembly="cellwise", **rc.PARTLY_REFINED[name])
    if name == "stokes3d_sphere":
        return rc.problem(name)
    pb = problems.stokes3d_sphere(6, 1, assembly="cellwise", local_refine=1)      # renumbered in place: a problem of its own
    return problems.permute_background_nodes(pb, problems.cuthill_mckee_nodes(pb))


@functools.lru_cache(maxsize=None)
def levels(name, q1_level=True):
    return problems.refined_prolongators(mesh(name), min_coarse=MIN_COARSE[name], q1_level=q1_level)


def config():
    return rc.config(SOLVE, "multilevel")


def oracle_solve(pb, lv, cfg=None):
    from oracle import oracle
    cfg = cfg or config()
    osys = oracle.system_from_problem(pb, aggregates=lv)
    code, rhs = osys.augment_rhs(cfg, rc.rhs_of(pb))
    assert code == 0
    code, x, res, hist = osys.solve(cfg, rhs)
    assert code == 0
    return res, hist


def record(pb, lv, res, hist):
    return {"block_sizes": pb.block_sizes, "level_sizes": [int(n) for _, n in lv],
            "outer_iterations": res.outer_iterations, "inner_iterations": res.inner_iterations,
            "mp_iterations": res.mp_iterations, "last_residual": float(res.last_residual).hex(),
            "history": [float(h).hex() for h in hist]}
