"""The Krylov-layer configurations shared by test_krylov_edges.py (oracle against SciPy) and
test_gpu_krylov_edges.py (library against oracle): warm starts, a full 63-vector basis, restart 1 and 2,
an outer failure in the middle of a cycle.  Everything builds on cases.case(); the start vector is
cases.rng_blocks(pb, 1) and the right-hand side cases.prepared_rhs throughout.

A configuration is named by a key: an entry of X0_CASES, "long_basis:<mgs|cgs|cgs2>", "stagnating:<restart>",
"stagnating:2:dealii95" or "mid_cycle_failure".  oracle_run(key) solves it once on the oracle from the random
start and keeps the result for every test of the process; callers must not write into what it returns."""
import functools
from types import SimpleNamespace

import numpy as np
import scipy.sparse as sp

import cases
from fictitious_domain_al_preconditioners_amd import _abi

# warm starts: every outer loop (FGMRES 9.6 with CGS2 / MGS / CGS, with restarts, FGMRES 9.5, MinRes with both SPD
# preconditioners), every system operator (AL2, Stokes, elliptic interface, rational) and one multigrid case
X0_CASES = ["laplace2d_circle", "laplace2d_jacobi", "laplace3d_sphere", "stokes3d_sphere", "stokes3d_restart",
            "stokes3d_fgmres95", "stokes_minres_diag", "rational_minres", "elliptic_modified", "stokes3d_gmg_patch"]

ORTH = {"mgs": _abi.ORTH_MGS, "cgs": _abi.ORTH_CGS, "cgs2": _abi.ORTH_CGS2}
LONG_RESTART = 63                       # kMaxBasis - 1: the longest basis setup() admits
LONG_BASIS = ["long_basis:mgs", "long_basis:cgs", "long_basis:cgs2"]
STAGNATING = ["stagnating:1", "stagnating:2", "stagnating:2:dealii95"]
FAILING = STAGNATING + ["mid_cycle_failure"]


def _weak_inner(restart, max_steps):
    """stokes3d_restart with three CG steps per application: a preconditioner weak enough for long outer runs."""
    pb, cfg = cases.case("stokes3d_restart")
    cfg.restart = restart
    cfg.inner = _abi.Control(_abi.CTRL_FIXED_ITERS, 3, 0.0, 0.0)
    cfg.outer.max_steps = max_steps
    return pb, cfg


def long_basis(orth):
    """Converges in 185 outer iterations on the oracle: two full 63-vector cycles and one of 59."""
    pb, cfg = _weak_inner(LONG_RESTART, 400)
    cfg.orthogonalization = orth
    return pb, cfg


def stagnating(restart, flavour=_abi.FGMRES_DEALII_96):
    """restart 1 and 2 stagnate (residual 0.17-0.29 of the start after 400 steps): outer failure after 40."""
    pb, cfg = _weak_inner(restart, 40)
    cfg.fgmres_flavour = flavour
    return pb, cfg


def mid_cycle_failure():
    """long_basis(CGS2) cut at 100 steps: column 37 of the second cycle."""
    pb, cfg = long_basis(_abi.ORTH_CGS2)
    cfg.outer.max_steps = 100
    return pb, cfg


def config(key):
    """key -> (problem, config), fresh objects on every call."""
    if key in X0_CASES:
        return cases.case(key)
    kind, _, arg = key.partition(":")
    if kind == "long_basis":
        return long_basis(ORTH[arg])
    if kind == "stagnating":
        restart, _, flavour = arg.partition(":")
        return stagnating(int(restart), _abi.FGMRES_DEALII_95 if flavour == "dealii95" else _abi.FGMRES_DEALII_96)
    if key == "mid_cycle_failure":
        return mid_cycle_failure()
    raise KeyError(key)


def x0_of(pb):
    return cases.rng_blocks(pb, 1)


def copy_config(cfg, **changes):
    out = _abi.Config.from_buffer_copy(cfg)
    for k, v in changes.items():
        setattr(out, k, v)
    return out


@functools.lru_cache(maxsize=None)
def system(key):
    """(problem, config, oracle system, prepared rhs, x0) of a key; the stagnating / long-basis keys share one."""
    pb, cfg = config(key)
    osys = cases.oracle_system(pb, cfg)
    return SimpleNamespace(pb=pb, cfg=cfg, osys=osys, rhs=cases.prepared_rhs(osys, pb, cfg), x0=x0_of(pb))


@functools.lru_cache(maxsize=None)
def oracle_run(key):
    """The oracle's solve of `key` from the random start, computed once: the fields of system(key) plus
    rc, x, res, hist."""
    s = system(key)
    rc, x, res, hist = s.osys.solve(s.cfg, s.rhs, x0=s.x0)
    return SimpleNamespace(**vars(s), rc=rc, x=x, res=res, hist=hist)


def control_met_at_the_solution(cfg, res, hist):
    """The outer control under which the solution of a finished solve (its config, result and history) is already
    converged.  A solve that stopped on the absolute tolerance keeps its control.  One that stopped on the reduction
    alone (elliptic_modified: 1.8e-8 against tol 1e-10) would iterate again, because ReductionControl takes the
    reduction from the new start; it gets the absolute form of the rule that stopped it,
    SolverControl(reduce * hist[0])."""
    if res.last_residual <= cfg.outer.tol:
        return _abi.Control(cfg.outer.kind, cfg.outer.max_steps, cfg.outer.tol, cfg.outer.reduce)
    return _abi.Control(_abi.CTRL_ABS, cfg.outer.max_steps, cfg.outer.reduce * hist[0], 0.0)


# ---- independent assembly of the block system (SciPy), as tests/test_oracle.py does
def assemble(pb, cfg):
    """The block system K of a case as a SciPy CSR matrix, from pb.mats alone."""
    if cfg.variant == _abi.RATIONAL:                 # immersed_laplace.cc:596-597: no augmentation
        A, Ct, C = (pb.mats[k].to_scipy() for k in ("A", "Ct", "C"))
        return sp.bmat([[A, Ct], [C, None]]).tocsr()
    if "A2" in pb.mats:                              # elliptic_interface.cc:805-819
        A, Ct, C, A2, M = (pb.mats[k].to_scipy() for k in ("A", "Ct", "C", "A2", "M"))
        W = sp.diags(pb.inv_w_diag_of_mass_squared())
        a11 = A + cfg.gamma * (Ct @ W @ C)
        a22 = A2 + cfg.gamma2 * (M @ W @ M)
        a12 = -cfg.gamma * (Ct @ W @ M)
        a21 = -cfg.gamma2 * (M @ W @ C)
        return sp.bmat([[a11, a12, Ct], [a21, a22, -M], [C, -M, None]]).tocsr()
    A, Ct, C = (pb.mats[k].to_scipy() for k in ("A", "Ct", "C"))
    aug = A + cfg.gamma * (Ct @ sp.diags(pb.inv_w_diag_squared()) @ C)
    if "B" in pb.mats:
        B, Bt = pb.mats["B"].to_scipy(), pb.mats["Bt"].to_scipy()
        return sp.bmat([[aug, Bt, Ct], [B, None, None], [C, None, None]]).tocsr()
    return sp.bmat([[aug, Ct], [C, None]]).tocsr()


def matvec_ld(K, x):
    """K @ x accumulated in np.longdouble (SciPy's own product has no longdouble kernel)."""
    K = K.tocsr()
    prod = K.data.astype(np.longdouble) * np.asarray(x, np.longdouble)[K.indices]
    out = np.zeros(K.shape[0], np.longdouble)
    rows = np.repeat(np.arange(K.shape[0]), np.diff(K.indptr))
    np.add.at(out, rows, prod)
    return out


def residual_ld(K, b, x):
    """b - K x in longdouble; b, x as block lists or flat arrays."""
    b = np.concatenate(b) if isinstance(b, (list, tuple)) else b
    x = np.concatenate(x) if isinstance(x, (list, tuple)) else x
    return np.asarray(b, np.longdouble) - matvec_ld(K, x)


def norm_ld(v):
    v = np.asarray(v, np.longdouble)
    return float(np.sqrt(np.sum(v * v)))
