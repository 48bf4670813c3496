"""Locally refined problems (generate(local_refine=1)) shared by tests/test_refined_generator.py,
tests/test_gpu_refined.py and tests/golden/make_refined_golden.py: the generator arguments of the partly refined
meshes that are compared with refined_reference.py, and the two solve cases with their three inner preconditioners."""
import functools

from fictitious_domain_al_preconditioners_amd import _abi, problems

# generate() arguments without local_refine / assembly.  The 2-D Laplace body is a square of FOUR segments, each
# longer than two base cells: its quadrature points also fall into unrefined cells and next to hanging nodes.
PARTLY_REFINED = {
    "laplace2d_q1": dict(dim=2, degree=1, ncomp=1, n_cells=8, center=(0.4, 0.4, 0.0), radius=0.2, immersed_refine=0,
                         coupling_nq=3, body_force=(1.0,), embedded_value=(1.0,)),
    "stokes2d": dict(dim=2, degree=2, ncomp=2, n_cells=8, stokes=True, grad_div=True, gamma_grad_div=10.0,
                     center=(0.5, 0.5, 0.0), radius=0.2, immersed_refine=2, coupling_nq=3, body_force=(1.0, 0.0),
                     embedded_value=(-1.0, 1.0)),
    "stokes3d_grad_div": dict(dim=3, degree=2, ncomp=3, n_cells=4, stokes=True, grad_div=True, gamma_grad_div=10.0,
                              center=(0.5, 0.5, 0.5), radius=0.1, immersed_refine=1, coupling_nq=4,
                              body_force=(1.0, 0.0, 0.0), embedded_value=(-1.0, 1.0, 0.0)),
}

SOLVE_CASES = ("stokes3d_sphere", "laplace2d_circle")
PRECONDITIONERS = ("chebyshev", "multilevel")            # + "truncated_sa", built on the device (GPU tests only)


@functools.lru_cache(maxsize=None)
def problem(name):
    """stokes3d_sphere: 6^3 base cells, 32 refined, 13 335 + 687 + 78 unknowns, 864 x 3 hanging velocity rows;
    laplace2d_circle: 16^2 base cells, 60 refined, 493 + 32 unknowns, 48 hanging rows."""
    if name == "stokes3d_sphere":
        return problems.stokes3d_sphere(6, 1, assembly="cellwise", local_refine=1)
    return problems.laplace2d_circle(16, 3, local_refine=1)


def config(name, prec):
    """Solver settings of tests/cases.py: the reference prms, Chebyshev with the raised inner cap, the multilevel
    cases with the settings of "stokes3d_gmg_patch" (patch corrections, explicit inverse on the coarsest level)."""
    if name == "stokes3d_sphere":
        cfg = _abi.default_config(_abi.AL_STOKES)
    else:
        cfg = _abi.default_config(_abi.AL2)
        cfg.outer = _abi.Control(_abi.CTRL_REDUCTION, 1000, 1e-10, 1e-12)
    if prec == "chebyshev":
        cfg.inner.max_steps = 1000
    elif prec == "multilevel":
        cfg.inner_prec = _abi.PREC_MULTILEVEL
        cfg.ml_smooth_degree, cfg.ml_smooth_ratio = 4, 30.0
        cfg.ml_patch_degree, cfg.ml_patch_ratio, cfg.ml_coarse_direct = 5, 30.0, 1024
        cfg.inner.max_steps = 100
    else:                                               # truncated smoothed aggregation: tests/test_gpu_truncated_aggregation.py
        cfg.inner_prec = _abi.PREC_MULTILEVEL
        cfg.ml_smooth_degree, cfg.ml_smooth_ratio, cfg.ml_coarse_degree = 4, 256.0, 10
        cfg.inner.max_steps = 100
    return cfg


def levels(name, prec):
    if prec != "multilevel":
        return None
    return problems.refined_prolongators(problem(name), min_coarse=100 if name == "stokes3d_sphere" else 20)


def rhs_of(pb):
    blocks = [pb.vecs["f"].copy()]
    if "B" in pb.mats:
        blocks.append(pb.vecs["rhs_p"].copy())
    return blocks + [pb.vecs["g"].copy()]
