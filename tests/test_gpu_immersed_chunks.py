"""The immersed-side solves on the GPU beyond one 4096-entry chunk: library against oracle.

The keys of tests/immersed_chunk_cases.py put 4096, 4097, 4225 and 8281 unknowns into the immersed and multiplier
blocks, so that the paths the parity suite only runs with one chunk take several: mass_solve (Jacobi CG on M for the
exact W^-1, on the swapped-in n_* work set, nested inside Aug p, A22 p, Aug2 p and system_apply), the inner CG on
OP_A22 with its Chebyshev sweep and dinv_a22, the 2-block OP_AUG2 (x + off[1], pmul_scale_kernel on nlp, dinv_aug2 =
[dinv_aug | dinv_a22]), the 3-block system operator and block preconditioner with blocks at off[1], off[2] of several
chunks each, and the row-partitioned immersed blocks (a rank that owns the second chunk's entries only; a rank without
an immersed row).

Reference: the CPU oracle (canonical arithmetic), which tests/test_immersed_chunks_reference.py pins
to SciPy at these sizes.  One context and one oracle handle per key, both kept for the module."""
import threading

import numpy as np
import pytest

import cases
import immersed_chunk_cases as icc
from fictitious_domain_al_preconditioners_amd import _abi, solver

pytestmark = pytest.mark.gpu
HIST_RTOL = 1e-10          # tests/test_gpu_parity.py


@pytest.fixture(scope="module")
def ctxs(built):
    cache = {}

    def get(key):
        if key not in cache:
            s = icc.system(key)
            cache[key] = solver.context_from_problem(s.pb, icc.copy_config(s.cfg))
        return cache[key]
    yield get
    for c in cache.values():
        c.close()


def _same_bits(got, want):
    return all(np.array_equal(g, w) for g, w in zip(got, want))


def _first_bad(got, want):
    for b, (g, w) in enumerate(zip(got, want)):
        bad = np.flatnonzero(~(g == w))
        if bad.size:
            return b, int(bad.size), int(bad[0]), float(g[bad[0]]), float(w[bad[0]])
    return None


def test_the_keys_have_the_sizes_they_are_named_for(built):
    for key in icc.KEYS:
        n = icc.BLOCKS[key][1]
        chunks = -(-n // icc.CHUNK)
        assert chunks == {4096: 1, 4097: 2, 4225: 2, 8281: 3}[n]
        assert icc.system(key).pb.block_sizes == icc.BLOCKS[key]
        assert set(icc.system(key).inputs) == set(icc.INPUT_NAMES if chunks > 1 else ["rng", "e_last", "constant"])


@pytest.mark.parametrize("key", icc.KEYS)
def test_system_apply_bitwise(ctxs, key):
    """AA x for every input, into fresh arrays: bit-equal to the oracle (the yardstick of
    test_gpu_parity.py::test_system_and_rhs_bitwise)."""
    s, ctx = icc.system(key), ctxs(key)
    for name, src in s.inputs.items():
        got = ctx.system_apply(src)
        want = icc.oracle_system_apply(key, name)
        assert _same_bits(got, want), (key, name, _first_bad(got, want))


def _check_vmult(key, name, got, res, counts, tag):
    o = icc.oracle_vmult(key, name)
    assert (res.inner_iterations, res.mass_iterations, res.mp_iterations, res.inner_failures) == \
        (o.res.inner_iterations, o.res.mass_iterations, o.res.mp_iterations, o.res.inner_failures), (key, name, tag)
    assert res.lambda_max == o.res.lambda_max, (key, name, tag)
    assert counts == o.counts, (key, name, tag)
    for g, r in zip(got, o.v):
        assert np.allclose(g, r, rtol=HIST_RTOL, atol=HIST_RTOL * np.abs(r).max()), (key, name, tag)
    bitwise = _same_bits(got, o.v)
    print(f"{key} {name} ({tag}): inner {counts}, mass {res.mass_iterations}, "
          f"{'bit-identical to' if bitwise else 'NOT bit-identical to'} the oracle")
    assert bitwise, (key, name, tag, _first_bad(got, o.v))      # DESIGN section 4, one rank


@pytest.mark.parametrize("key", icc.KEYS)
def test_precond_apply_matches_the_oracle_in_two_orders(ctxs, key):
    """<Preconditioner>::vmult for every input, then for every input again in the reverse order, on one context: equal
    counts (total, per inner operator, mass), equal lambda_max, vectors within HIST_RTOL and bit-identical.  The second
    pass meets the work vectors and the padding that another input left behind -- after the indicator of the second
    chunk, after a unit vector -- and must reproduce the bits of a first application.
    (The two elliptic exact_w keys spend most of their time in the oracle: 1.4 - 2.9 s per input, 14 000 - 24 000 nested
    mass iterations each; the ten applications on the GPU take under 3 s.)"""
    s, ctx = icc.system(key), ctxs(key)
    names = list(s.inputs)
    for tag, order in (("first pass", names), ("reverse pass", names[::-1])):
        for name in order:
            got, res = ctx.precond_apply(s.inputs[name])
            _check_vmult(key, name, got, res, ctx.inner_iterations(), tag)
    o = icc.oracle_vmult(key, "rng")
    if key in icc.EXACT_W_KEYS:
        assert o.res.mass_iterations > 0
    variant = s.cfg.variant
    if variant == _abi.AL_ELL_MODIFIED:
        assert o.counts["aug"] > 0 and o.counts["a22"] > 0 and o.counts["aug2"] == 0
    elif variant == _abi.AL_ELL_IDEAL:
        assert o.counts["aug2"] == o.res.inner_iterations > 0


@pytest.mark.parametrize("key", icc.SOLVE_KEYS)
def test_solve_matches_the_oracle(ctxs, key):
    """The yardstick of test_gpu_parity.py::test_solve_matches_oracle_and_golden without the golden part, and the
    true residual of the returned solution through system_apply against the stop rule."""
    s, ctx = icc.system(key), ctxs(key)
    o = icc.oracle_solve(key)
    x, res = ctx.solve(s.rhs)
    hist = ctx.history()
    counts = ctx.inner_iterations()
    print(f"{key}: outer {res.outer_iterations}, inner {res.inner_iterations} {counts}, mass {res.mass_iterations}, "
          f"GPU solve {res.solve_seconds:.2f} s, oracle {o.seconds:.1f} s")
    assert o.rc == 0 and res.status == 0
    assert res.outer_iterations == o.res.outer_iterations
    assert res.inner_iterations == o.res.inner_iterations
    assert res.mp_iterations == o.res.mp_iterations
    assert res.rational_iterations == o.res.rational_iterations
    assert res.mass_iterations == o.res.mass_iterations
    assert counts == o.counts
    assert len(hist) == len(o.hist)
    assert np.max(np.abs(hist - o.hist) / np.abs(o.hist)) <= HIST_RTOL
    for g, r in zip(x, o.x):
        assert np.allclose(g, r, rtol=1e-9, atol=1e-10 * max(np.abs(r).max(), 1e-30))
    ax = ctx.system_apply(x)
    r = np.concatenate([a - b for a, b in zip(s.rhs, ax)])
    assert np.linalg.norm(r) <= 10 * max(s.cfg.outer.tol, s.cfg.outer.reduce * res.initial_residual)


def test_mass_solve_failure_leaves_no_state_behind(ctxs):
    """ell_mod_4225_exact_w with 3 mass CG steps (every mass solve of the oracle needs more): the preconditioner
    answers ALFD_E_NO_CONVERGENCE_INNER from inside the nested solve, as the oracle does; with the cap restored through
    configure / setup the same context gives the unchanged bits."""
    key = "ell_mod_4225_exact_w"
    s, ctx = icc.system(key), ctxs(key)
    src = s.inputs["rng"]
    capped = icc.copy_config(s.cfg)
    capped.mass = _abi.Control(s.cfg.mass.kind, 3, s.cfg.mass.tol, s.cfg.mass.reduce)
    rc, _, _ = s.osys.precond_apply(capped, src)
    assert rc == _abi.E_NO_CONVERGENCE_INNER
    before, res = ctx.precond_apply(src)
    _check_vmult(key, "rng", before, res, ctx.inner_iterations(), "before the failure")
    try:
        ctx.configure(capped)
        ctx.setup(s.pb.block_sizes)
        with pytest.raises(solver.NoConvergence) as e:
            ctx.precond_apply(src)
        assert e.value.status == _abi.E_NO_CONVERGENCE_INNER
        with pytest.raises(solver.NoConvergence) as e:       # the nested solve of the outer operator fails alike
            ctx.system_apply(src)
        assert e.value.status == _abi.E_NO_CONVERGENCE_INNER
    finally:
        ctx.configure(icc.copy_config(s.cfg))
        ctx.setup(s.pb.block_sizes)
    after, res = ctx.precond_apply(src)
    _check_vmult(key, "rng", after, res, ctx.inner_iterations(), "after the failure")
    assert _same_bits(after, before)
    assert _same_bits(ctx.system_apply(src), icc.oracle_system_apply(key, "rng"))


# ------------------------------------------------------------------------------------------------ two and three ranks
def _run_ranks(key, plan, cfg):
    """tests/test_gpu_multirank.py::_run_interface_ranks with the problem and the plan of a key."""
    world = plan.world
    group = solver.LocalGroup(world)
    out = [None] * world
    errs = []

    def work(rank):
        try:
            pb = icc.problem(key, row_ranges=plan.generator_ranges(rank))
            ctx = solver.Context(0)
            ctx.comm_init_local(group.handle, rank)
            ctx.set_partition(plan.offsets)
            solver.upload_problem(ctx, pb, cfg)
            x, res = ctx.solve(cases.rhs_of(pb))
            out[rank] = dict(x=x, res=res.as_dict(), hist=ctx.history(), sizes=pb.block_sizes)
            ctx.close()
        except Exception as e:   # noqa: BLE001
            errs.append((rank, repr(e)))

    th = [threading.Thread(target=work, args=(r,)) for r in range(world)]
    for t in th:
        t.start()
    for t in th:
        t.join(timeout=600)
    group.close()
    assert not errs, errs
    return out


@pytest.mark.parametrize("split", list(icc.SPLITS))
@pytest.mark.parametrize("key", ["ell_mod_4225", "ell_ideal_4225_exact_w"])
def test_partitioned_immersed_blocks_match_the_oracle_emulation(built, key, split):
    """The immersed and multiplier rows cut at 4096 / 129 (one rank owns the second chunk's entries only), at
    2112 / 2113, and over three ranks of which the first owns no immersed row: the yardstick of
    test_gpu_multirank.py::test_partitioned_interface_problems_match_oracle_emulation."""
    s = icc.system(key)
    o = icc.oracle_partitioned_solve(key, split)
    plan, world = o.plan, o.plan.world
    cuts = icc.SPLITS[split]
    out = _run_ranks(key, plan, icc.copy_config(o.cfg))
    bounds = [0, *cuts, s.pb.block_sizes[1]]
    assert [out[r]["sizes"][1] for r in range(world)] == [b - a for a, b in zip(bounds, bounds[1:])]
    print(f"{key} {split}: outer {o.res.outer_iterations}, inner {o.res.inner_iterations}, mass "
          f"{o.res.mass_iterations}, oracle {o.seconds:.1f} s")
    assert o.rc == 0 and o.res.outer_iterations > 0
    for r in range(world):
        res = out[r]["res"]
        assert res["status"] == 0
        assert (res["outer_iterations"], res["inner_iterations"], res["mass_iterations"]) == \
            (o.res.outer_iterations, o.res.inner_iterations, o.res.mass_iterations)
        assert np.array_equal(out[r]["hist"], out[0]["hist"])
        assert np.max(np.abs(out[r]["hist"] - o.hist) / np.abs(o.hist)) <= 1e-10
    for b in range(3):
        xs = np.concatenate([out[r]["x"][b] for r in range(world)])
        assert np.allclose(xs, o.x[b], rtol=1e-8, atol=1e-9 * max(np.abs(o.x[b]).max(), 1e-30))
