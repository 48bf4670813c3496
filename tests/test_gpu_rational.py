"""RationalPreconditioner on the GPU beyond one 4096-entry chunk per system.

The rational variant has a device path of its own: 21 CG solves on the immersed matrices run in lock step through the
batched kernels (b_replicate / b_jacobi_dot / b_final / b_p_update / b_xr_update_dot / b_combine) on a block-diagonal
matrix [S_1 .. S_20, M] that setup builds for this variant alone, every system padded to whole 4096-entry chunks
(cps = chunks per system).  The rational_minres case of the parity suite has 32 immersed unknowns: cps = 1, one
workgroup in the combine, and so few non-empty rows that only the row-list SpMV runs.  The shapes below are the
smallest at which each index computation, either storage form and lane widths 4 and 8 can go wrong.

Reference: the CPU oracle, bit for bit (the same fma for the shifted values, the same 1/diag, the same
v = v + c * x accumulation order, canonical dots), which tests/test_rational_reference.py pins to a SciPy sparse-LU
evaluation of the rational sum at these very shapes; block 1 of the GPU result is also held against that sum directly,
at the bound the CPU module records.  Problems, inputs and oracle results are those of that module, computed once."""
import numpy as np
import pytest

import test_rational_reference as ref
from fictitious_domain_al_preconditioners_amd import _abi, solver

pytestmark = pytest.mark.gpu

CHUNK = 4096

# name          n1    cps   what it reaches
SHAPES = [
    # laplace2d_circle(16, 3, immersed_segments=n1): K has 3 entries per row, lane width L = 4
    ("circle1500", 1500, 1),    # row-list form (2 * 1500 < 4096)
    ("circle2100", 2100, 1),    # full-row form with 1996 empty padding rows per system
    ("circle4096", 4096, 1),    # no padding row at all
    ("circle4097", 4097, 2),    # the second chunk of every system holds one real entry
    ("circle8200", 8200, 3),    # cps odd: / cps and % cps differ from shifts
    # laplace3d_sphere(8, r): 9 entries per row, L = 8
    ("sphere386", 386, 1),      # row-list form
    ("sphere6146", 6146, 2),    # full-row form, two chunks
]
NAMES = [s[0] for s in SHAPES]
CAPPED = ["circle2100", "circle4097", "circle8200"]      # the accepted-failure runs
STATE = ["circle4097", "sphere6146"]


def test_the_table_is_the_cpu_modules(built):
    assert NAMES == ref.NAMES
    for name, n1, cps in SHAPES:
        assert ref.SHAPES[name][1] == n1 and -(-n1 // CHUNK) == cps


def _context(c, cfg=None):
    return solver.context_from_problem(c.pb, cfg or ref.converging_config(c.pb))


def _reconfigure(ctx, c, cfg):
    ctx.configure(cfg)
    ctx.setup(c.pb.block_sizes)


def _same_bits(got, want):
    return all(np.array_equal(g, w) for g, w in zip(got, want))


def _assert_equals_oracle(got, res, want, ores):
    assert (res.rational_iterations, res.inner_iterations, res.inner_failures) == \
           (ores.rational_iterations, ores.inner_iterations, ores.inner_failures)
    assert np.array_equal(got[0], want[0])
    assert np.array_equal(got[1], want[1])


@pytest.mark.parametrize("name", NAMES)
def test_vmult_and_system_equal_the_oracle_bit_for_bit(built, name):
    c = ref.case(name)
    cfg = ref.converging_config(c.pb)
    ctx = _context(c, cfg)
    got, res = ctx.precond_apply(c.src)
    ax = ctx.system_apply(c.src)
    ctx.close()
    assert c.rc == 0 and res.status == 0
    assert res.rational_iterations > 21 and res.inner_failures == 0
    _assert_equals_oracle(got, res, c.v, c.res)
    # the GPU result itself against the SciPy sum (not only through the oracle)
    err = ref.rel_err(got[1], ref.scipy_sum(name)[1])
    print(f"{name}: GPU vs SciPy {err:.2e} (bound {ref.BOUND:.1e}), {res.rational_iterations} rational iterations")
    assert err <= ref.BOUND
    rc, oax = c.osys.system_apply(cfg, c.src)
    assert rc == 0 and _same_bits(ax, oax)


@pytest.mark.parametrize("name", CAPPED)
def test_accepted_failures_freeze_each_system_where_it_stopped(built, name):
    """600 steps: the 21 systems stop anywhere between a few dozen steps (the mass system) and the cap, which 4 of
    them hit.  A system that has met its stop rule, or the cap, is never touched again, so the result is the
    oracle's, whose 21 solves run one after the other."""
    c = ref.case(name)
    orc, ov, ores = ref.accepted_failure_case(name)
    assert orc == 0 and 0 < ores.inner_failures < 21
    ctx = _context(c, ref.failing_config(c.pb, _abi.INNER_ACCEPT))
    got, res = ctx.precond_apply(c.src)
    _assert_equals_oracle(got, res, ov, ores)
    # the same cap under INNER_THROW is an error ...
    _reconfigure(ctx, c, ref.failing_config(c.pb, _abi.INNER_THROW))
    with pytest.raises(solver.AlfdError) as e:
        ctx.precond_apply(c.src)
    assert e.value.status == _abi.E_NO_CONVERGENCE_INNER
    # ... after which the context still works, and nothing of the systems that the failure froze is left
    _reconfigure(ctx, c, ref.converging_config(c.pb))
    got, res = ctx.precond_apply(c.src)
    ctx.close()
    _assert_equals_oracle(got, res, c.v, c.res)


@pytest.mark.parametrize("name", STATE)
def test_no_state_survives_an_application(built, name):
    """rt_p and rt_z are not cleared between applications: a, b, a must give the same bits for a twice, and for b
    those of a context that never saw a."""
    c = ref.case(name)
    a, b = c.src, ref.rng_blocks(c.pb, ref.SEED + 2)
    ctx = _context(c)
    va1, ra1 = ctx.precond_apply(a)
    vb, rb = ctx.precond_apply(b)
    va2, ra2 = ctx.precond_apply(a)
    ctx.close()
    fresh = _context(c)
    vf, rf = fresh.precond_apply(b)
    fresh.close()
    assert _same_bits(va1, c.v) and _same_bits(va2, va1)
    assert ra1.rational_iterations == ra2.rational_iterations == c.res.rational_iterations
    assert _same_bits(vb, vf) and rb.rational_iterations == rf.rational_iterations
    assert not np.array_equal(vb[1], va1[1])


@pytest.mark.parametrize("name", STATE)
def test_no_state_survives_accepted_failures(built, name):
    """Systems frozen by the step cap keep their x, r, p: neither the next application with the same cap nor, after
    alfd_configure / alfd_setup, the converging one may see them."""
    c = ref.case(name)
    a, b = c.src, ref.rng_blocks(c.pb, ref.SEED + 2)
    capped = ref.failing_config(c.pb, _abi.INNER_ACCEPT)
    if name == "sphere6146":      # its systems need a few hundred steps at most: at 100 a third of them hit the cap
        capped.rational.max_steps = 100
    rc, ova, ores = c.osys.precond_apply(capped, a)
    assert rc == 0 and 0 < ores.inner_failures < 21
    ctx = _context(c, capped)
    va1, ra1 = ctx.precond_apply(a)
    vb, rb = ctx.precond_apply(b)
    va2, ra2 = ctx.precond_apply(a)
    assert rb.inner_failures > 0
    _assert_equals_oracle(va1, ra1, ova, ores)
    _assert_equals_oracle(va2, ra2, ova, ores)
    _reconfigure(ctx, c, ref.converging_config(c.pb))
    got, res = ctx.precond_apply(a)
    ctx.close()
    _assert_equals_oracle(got, res, c.v, c.res)


def test_zero_immersed_input(built):
    """u1 = 0: every system meets its stop rule at step 0; v1 is exactly zero (no 0/0 of the scalar kernel turns
    into a NaN), block 0 is the oracle's, and the application after it is unaffected."""
    c = ref.case("circle4097")
    cfg = ref.converging_config(c.pb)
    src = [c.src[0], np.zeros(c.pb.block_sizes[1])]
    ctx = _context(c, cfg)
    got, res = ctx.precond_apply(src)
    after, res_after = ctx.precond_apply(c.src)
    ctx.close()
    rc, want, ores = c.osys.precond_apply(cfg, src)
    assert rc == 0 and ores.rational_iterations == 0
    assert res.rational_iterations == 0 and res.inner_failures == 0
    assert np.array_equal(got[1], np.zeros_like(got[1]))
    assert np.array_equal(got[0], want[0]) and res.inner_iterations == ores.inner_iterations
    _assert_equals_oracle(after, res_after, c.v, c.res)


def test_one_entry_in_the_last_real_row_of_the_second_chunk(built):
    """circle4097, u1 = e_4096: the only nonzero of the right-hand side is the single real entry of every system's
    second chunk, the first chunk starts from an all-zero residual."""
    name = "circle4097"
    c = ref.case(name)
    cfg = ref.converging_config(c.pb)
    u1 = np.zeros(c.pb.block_sizes[1])
    u1[CHUNK] = 1.0
    src = [np.zeros(c.pb.block_sizes[0]), u1]
    ctx = _context(c, cfg)
    got, res = ctx.precond_apply(src)
    ctx.close()
    rc, want, ores = c.osys.precond_apply(cfg, src)
    assert rc == 0 and ores.rational_iterations > 21
    _assert_equals_oracle(got, res, want, ores)
    assert np.array_equal(got[0], np.zeros_like(got[0]))
    # (the oracle is 4.8e-12 from the SciPy sum for this input: its absolute stop rule is looser on a unit vector)
    assert ref.rel_err(got[1], np.sum(ref.scipy_terms(c.pb, u1), axis=0)) <= ref.BOUND


def test_symmetric_positive_definite_at_circle8200(built):
    """Block 1 of the preconditioner is SPD (MinRes needs it): the symmetry defect of two applications within the
    bound the CPU module takes from the oracle's own value, positive Rayleigh quotients."""
    c = ref.case("circle8200")
    ctx = _context(c)
    defect, upu, wpw = ref.symmetry_defect(lambda src: ctx.precond_apply(src)[0], *c.pb.block_sizes)
    ctx.close()
    print(f"circle8200: symmetry defect {defect:.2e} (bound {ref.SYM_BOUND:.1e})")
    assert upu > 0 and wpw > 0
    assert defect <= ref.SYM_BOUND
