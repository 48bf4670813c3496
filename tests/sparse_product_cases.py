"""The cases of tests/test_sparse_product_host.py and tests/test_gpu_setup_kernels.py: operands aimed at the capacity
edges of spgemm_rows_kernel (hash set of 4096 slots, at most 1024 distinct columns per product row, 64-column tiles, a
grid of at most 16 384 blocks) and of the prolongator row kernels (hash set of 2048, at most 512 candidates, rows of A
staged 512 entries at a time).  Every case is built once, carries its reference (tests/sparse_product_reference.py)
and asserts, from the reference alone, the property it was built for."""
import functools

import numpy as np

import sparse_product_reference as ref

GRID = 16384           # blocks of the row kernels' launches: rows b and b + GRID share a block
MAX_COLS = 1024        # distinct columns of a product row on the device
MAX_CAND = 512         # candidates of a prolongator row on the device


def dyadic(rng, n, zeros=False):
    """Integers |k| <= 16 times 2^-3, without zeros unless asked for."""
    k = rng.integers(1, 17, n) * rng.choice([-1, 1], n)
    if zeros:
        k[rng.random(n) < 0.1] = 0
    return k / 8.0


class ProductCase:
    def __init__(self, name, A, P, row, width, on_device, exact=True):
        self.name, self.A, self.P, self.row, self.width, self.on_device = name, A, P, row, width, on_device
        self.ref = ref.exact_product(A, P) if exact else ref.chain_product(A, P)
        self.exact = exact
        self.widths = np.diff(self.ref.row_ptr)
        if row is not None:
            assert self.widths[row] == width, (name, int(self.widths[row]), width)
            assert (self.widths.max() <= MAX_COLS) == bool(on_device), name
            if not on_device:                       # exactly one row does not fit, all others are ordinary
                assert int((self.widths > MAX_COLS).sum()) == 1 and np.sort(self.widths)[-2] <= 64, name
        for a in (A.row_ptr, A.col, A.val, P.row_ptr, P.col, P.val, self.ref.row_ptr, self.ref.col, self.ref.val):
            a.setflags(write=False)

    def row_cols(self, i):
        return self.ref.col[self.ref.row_ptr[i]:self.ref.row_ptr[i + 1]]


def _blocks_P(rng, ncols, sets, extra_rows=0):
    """P whose row k holds the columns sets[k] (in the given order), then `extra_rows` rows of three columns."""
    rows = [list(zip(s, dyadic(rng, len(s)))) for s in sets]
    for _ in range(extra_rows):
        c = rng.choice(ncols, 3, replace=False)
        rows.append(list(zip(c.tolist(), dyadic(rng, 3))))
    return ref.csr(len(rows), ncols, rows)


def _width_case(n):
    """Row 1 of the product has exactly n distinct columns (P rows of 8 columns, the last one shorter); the other rows
    are ordinary (three entries meeting rows of three columns)."""
    rng = np.random.default_rng(1000 + n)
    ncols = 2048
    cols = rng.permutation(ncols)[:n]
    sets = [cols[s:s + 8].tolist() for s in range(0, n, 8)] or [[]]
    extra = 12
    P = _blocks_P(rng, ncols, sets, extra)
    m = len(sets)
    rows = []
    for i in range(6):
        if i == 1:
            rows.append(list(zip(range(m), dyadic(rng, m))))
        else:
            k = rng.choice(extra, 3, replace=False) + m
            rows.append(list(zip(k.tolist(), dyadic(rng, 3))))
    A = ref.csr(6, P.nrows, rows)
    return ProductCase(f"width_{n}", A, P, 1, n, n <= MAX_COLS)


def _overlap_case():
    """200 entries of A (the lane-strided insertion runs four times), each meeting a P row of 8 consecutive columns
    that overlap to exactly 1024: every column is reached through one to several k."""
    rng = np.random.default_rng(7)
    starts = [round(k * 1016 / 199) for k in range(200)]
    assert starts[0] == 0 and starts[-1] == 1016 and max(np.diff(starts)) <= 8
    P = _blocks_P(rng, 1024, [list(range(s, s + 8)) for s in starts], 4)
    A = ref.csr(3, P.nrows, [list(zip(range(200, 203), dyadic(rng, 3))), list(zip(range(200), dyadic(rng, 200))),
                             list(zip(range(201, 204), dyadic(rng, 3)))])
    c = ProductCase("overlap_200x8", A, P, 1, 1024, True)
    assert A.row_ptr[2] - A.row_ptr[1] == 200 > 64
    return c


def _collide_case(b):
    """1024 columns that share the home slot b of the 4096-slot table: the probe run b .. b + 1023 wraps the end of the
    table.  ncols = 2^23, so about 2048 ids share a slot; nrows stays small (the host product keeps ncols-long vectors)."""
    rng = np.random.default_rng(b)
    ncols = 2 ** 23
    ids = ref.bucket_members(b, 12, ncols, 1024)
    assert ids.size >= 1024 and {ref.bucket(j) for j in ids} == {b} and b + 1024 > 4096
    ids = ids[rng.permutation(1024)]
    P = _blocks_P(rng, ncols, [ids[s:s + 8].tolist() for s in range(0, 1024, 8)])
    A = ref.csr(2, 128, [list(zip(range(128), dyadic(rng, 128))), list(zip([5, 77], dyadic(rng, 2)))])
    return ProductCase(f"collide_{b}", A, P, 0, 1024, True)


PAIRS = ("heavy_light", "light_heavy", "empty_heavy", "heavy_empty", "full_65")


def _stride_case():
    """16 384 + 257 rows: blocks 0 .. 256 take a second row.  Pair b (rows b and b + 16 384) is of kind PAIRS[b % 5];
    every other row is light.  A table, key list or count left over from a block's first row shows in its second."""
    rng = np.random.default_rng(11)
    n = GRID + 257
    P = _blocks_P(rng, 2048, [list(range(8 * r, 8 * r + 8)) for r in range(256)] + [[2047]])
    def light():
        return [(int(rng.integers(256)), float(dyadic(rng, 1)[0]))]
    def heavy():
        return list(zip(rng.choice(256, 40, replace=False).tolist(), dyadic(rng, 40)))      # 320 columns
    def full():
        return list(zip(rng.permutation(256)[:128].tolist(), dyadic(rng, 128)))              # 1024 columns
    def c65():
        k = rng.choice(255, 8, replace=False).tolist() + [256]                               # 64 + column 2047
        return list(zip(k, dyadic(rng, 9)))
    kinds = dict(heavy_light=(heavy, light), light_heavy=(light, heavy), empty_heavy=(list, heavy),
                 heavy_empty=(heavy, list), full_65=(full, c65))
    rows = [None] * n
    for b in range(n):
        if rows[b] is None:
            rows[b] = light()
        if b < 257:
            first, second = kinds[PAIRS[b % 5]]
            rows[b], rows[b + GRID] = first(), second()
    A = ref.csr(n, P.nrows, rows)
    c = ProductCase("grid_stride", A, P, None, None, True)
    want = dict(heavy_light=(320, 8), light_heavy=(8, 320), empty_heavy=(0, 320), heavy_empty=(320, 0), full_65=(1024, 65))
    for b in range(257):
        assert (c.widths[b], c.widths[b + GRID]) == want[PAIRS[b % 5]], b
    assert n > GRID and c.widths.max() == MAX_COLS
    return c


def _values_case():
    """Stored zeros in both operands, a chain that cancels exactly, the same J through many k, empty rows and empty
    columns of P, an empty row of A, a row of A that meets only empty rows of P."""
    P = ref.csr(8, 10, [
        [(1, 0.5), (4, 1.0), (7, -2.0)],            # 0
        [(1, 0.5), (4, 0.0), (8, 0.25)],            # 1: a stored zero
        [],                                         # 2: empty
        [(7, 1.5), (1, -0.5)],                      # 3: unsorted
        [(4, 1.0)],                                 # 4
        [],                                         # 5: empty
        [(4, 1.0)],                                 # 6
        [(0, 2.0), (9, -2.0)]])                     # 7         columns 2, 3, 5, 6 are never reached
    A = ref.csr(7, 8, [
        [(0, 1.0), (1, -1.0)],                      # column 1: 0.5 - 0.5 cancels and stays, as +0.0
        [(0, 0.0), (7, 1.0)],                       # a stored zero of A reaches columns 1, 4, 7
        [(2, 1.0), (5, -1.5)],                      # only empty rows of P: no columns
        [],                                         # empty
        [(4, 0.5), (6, 0.5), (0, 1.0), (1, 2.0), (3, 0.125)],      # column 4 through four k, one of them a zero
        [(4, 1.0), (6, -1.0)],                      # cancels
        [(3, -1.0), (0, -1.0)]])
    c = ProductCase("values_and_pattern", A, P, 2, 0, True)
    assert c.widths.tolist() == [4, 5, 0, 0, 4, 1, 3]
    r0 = dict(zip(c.row_cols(0).tolist(), c.ref.val[c.ref.row_ptr[0]:c.ref.row_ptr[1]].tolist()))
    assert r0[1] == 0.0 and not np.signbit(r0[1]) and r0[4] == 1.0          # cancelled: +0.0; 1 * 1 + (-1) * 0
    assert c.ref.val[c.ref.row_ptr[5]] == 0.0 and 4 in c.row_cols(1) and not np.isin([2, 3, 5, 6], c.ref.col).any()
    return c


def _degenerate_cases():
    e = lambda n, m: ref.csr(n, m, [[] for _ in range(n)])
    P = ref.csr(5, 7, [[(1, 1.0)], [], [(6, 0.5), (0, 1.0)], [], [(3, 2.0)]])
    a = ProductCase("no_rows", e(0, 5), P, None, None, True)
    b = ProductCase("no_entries", e(3, 4), e(4, 5), None, None, True)
    assert a.ref.row_ptr.tolist() == [0] and b.ref.row_ptr.tolist() == [0, 0, 0, 0]
    return [a, b]


def _general_case():
    """Uniform values, 300 rows of 1 .. 200 columns (beyond two 64-column tiles), checked against the Fraction chain."""
    rng = np.random.default_rng(5)
    nP, ncols = 300, 256
    prow = []
    for _ in range(nP):
        c = rng.choice(ncols, int(rng.integers(1, 7)), replace=False)
        prow.append(list(zip(c.tolist(), rng.uniform(-1.0, 1.0, c.size))))
    P = ref.csr(nP, ncols, prow)
    arow = []
    for r in range(300):
        k = rng.choice(nP, 1 + r % 60, replace=False)
        arow.append(list(zip(k.tolist(), rng.uniform(-1.0, 1.0, k.size))))
    A = ref.csr(300, nP, arow)
    assert ref.chain_terms(A, P) <= 300000
    c = ProductCase("general_values", A, P, None, None, True, exact=False)
    assert c.widths.min() == 1 and 128 < c.widths.max() <= 200, (c.widths.min(), c.widths.max())
    return c


WIDTHS = (0, 1, 63, 64, 65, 128, 129, 1023, 1024, 1025, 1500)
PRODUCT_NAMES = ([f"width_{n}" for n in WIDTHS] +
                 ["overlap_200x8", "collide_4095", "collide_4000", "grid_stride", "values_and_pattern", "no_rows",
                  "no_entries", "general_values"])


@functools.lru_cache(maxsize=None)
def product_case(name):
    if name.startswith("width_"):
        return _width_case(int(name[6:]))
    if name.startswith("collide_"):
        return _collide_case(int(name[8:]))
    if name in ("no_rows", "no_entries"):
        return {c.name: c for c in _degenerate_cases()}[name]
    return {"overlap_200x8": _overlap_case, "grid_stride": _stride_case, "values_and_pattern": _values_case,
            "general_values": _general_case}[name]()


# ---------------------------------------------------------------------------------------------------------------------
# prolongator rows

class ProlongatorCase:
    """A square A with its aggregates; row `row` is the one under test.  ref = the untruncated rows."""

    def __init__(self, name, A, agg, n_coarse, row, candidates, on_device, omega=0.5, Ct=None, w=None, gamma=0.0):
        self.name, self.A, self.agg, self.n_coarse, self.row = name, A, np.asarray(agg, np.int32), n_coarse, row
        self.omega, self.Ct, self.w, self.gamma, self.on_device = omega, Ct, w, gamma, on_device
        self.ref = ref.prolongator_rows(A, self.agg, n_coarse, omega, Ct, w, gamma)
        self.widths = np.diff(self.ref.row_ptr)
        if row is not None:
            assert self.widths[row] == candidates, (name, int(self.widths[row]), candidates)
        assert (self.widths.max() <= MAX_CAND) == bool(on_device), name
        assert np.all(self.widths[self.agg < 0] == 0)

    def row_of(self, M, i):
        s = slice(M.row_ptr[i], M.row_ptr[i + 1])
        return M.col[s], M.val[s]


def _square(rng, n, special, diag=None):
    """n x n: every row its diagonal (a power of two, so f_i is exact) and two neighbours, the rows in `special`
    (row -> list of (col, val), which must hold the diagonal) as given."""
    rows = []
    for i in range(n):
        if i in special:
            rows.append(special[i])
            assert any(c == i and v != 0.0 for c, v in special[i])
            continue
        d = float(2 ** int(rng.integers(1, 4))) if diag is None else diag
        r = [((i - 1) % n, float(dyadic(rng, 1)[0])), (i, d), ((i + 1) % n, float(dyadic(rng, 1)[0]))]
        rows.append(sorted(set((c, v) for c, v in r), key=lambda t: t[0]) if n > 2 else [(i, d)])
    return ref.csr(n, n, rows)


def _cand_case(c):
    """Row 0 has exactly c candidates: agg is the identity on the unknowns it reaches, except a few with agg < 0 (their
    columns are skipped and their rows come out empty)."""
    rng = np.random.default_rng(2000 + c)
    n = 640
    agg = np.arange(n, dtype=np.int32)
    off = np.array([3, 70, 200, 639]) if c > 3 else np.array([639])
    agg[off] = -1
    reach = np.flatnonzero(agg >= 0)[:c]                    # row 0 itself first
    cols = np.sort(np.concatenate([reach, off]))
    row0 = [(int(j), 4.0 if j == 0 else float(dyadic(rng, 1)[0])) for j in cols]
    A = _square(rng, n, {0: row0})
    return ProlongatorCase(f"cand_{c}", A, agg, n, 0, c, c <= MAX_CAND)


def _long_case(L):
    """Row 0 of A has L entries that map to 400 aggregates (agg[j] = j mod 400): the 512-entry stage loop runs once,
    twice or three times while the row stays on the device; every aggregate sums several entries."""
    rng = np.random.default_rng(3000 + L)
    n = 1200
    agg = (np.arange(n) % 400).astype(np.int32)
    row0 = [(j, 8.0 if j == 0 else float(dyadic(rng, 1)[0])) for j in range(L)]
    A = _square(rng, n, {0: row0})
    c = ProlongatorCase(f"long_{L}", A, agg, 400, 0, 400, True)
    assert A.row_ptr[1] - A.row_ptr[0] == L
    return c


def _penalty_case():
    """A penalty term whose rows add columns outside the pattern of A: unknown 0 shares multipliers with unknowns 300
    .. 339, which row 0 of A does not reach.  Row 0: 129 candidates from A, 40 more from the penalty."""
    rng = np.random.default_rng(17)
    n, m = 400, 5
    agg = np.arange(n, dtype=np.int32)
    agg[[50, 310]] = -1
    row0 = [(j, 4.0 if j == 0 else float(dyadic(rng, 1)[0])) for j in range(130)]
    A = _square(rng, n, {0: row0})
    ct = [[] for _ in range(n)]
    ct[0] = [(k, float(dyadic(rng, 1)[0])) for k in range(m)]
    for j in range(300, 340):
        ct[j] = [(int(j % m), float(dyadic(rng, 1)[0]))]
    ct[120] = [(2, 0.5)]
    Ct = ref.csr(n, m, ct)
    w = np.array([0.5, 1.0, 2.0, 0.25, 4.0])
    c = ProlongatorCase("penalty", A, agg, n, 0, 129 + 39, True, Ct=Ct, w=w, gamma=2.0)
    mine = set(c.row_of(c.ref, 0)[0].tolist())
    from_A = {int(agg[j]) for j in range(130) if agg[j] >= 0}
    assert len(from_A) == 129 and len(mine - from_A) == 39 and 305 in mine and 310 not in mine
    return c


def _sa_collide_case():
    """Aggregate ids that share the home slot 2040 of the 2048-slot table: 300 of them, so the probe run wraps."""
    rng = np.random.default_rng(19)
    nc = 2 ** 23
    ids = ref.bucket_members(2040, 11, nc, 300)
    assert ids.size == 300 and {ref.bucket(j, 11) for j in ids} == {2040} and 2040 + 300 > 2048
    n = 320
    agg = np.full(n, -1, np.int32)
    agg[:300] = ids[rng.permutation(300)]
    row0 = [(j, 4.0 if j == 0 else float(dyadic(rng, 1)[0])) for j in range(n)]
    A = _square(rng, n, {0: row0})
    return ProlongatorCase("collide_2040", A, agg, nc, 0, 300, True)


def _sa_stride_case():
    """16 384 + 257 rows; pair b (rows b, b + 16 384) of kind PAIRS[b % 5]: heavy = 300 candidates, light = the
    diagonal alone, empty = a row without an aggregate, full = 512 candidates then 65.  agg[j] = j mod 600; row i with
    c candidates reaches itself and c - 1 consecutive unknowns from 1200 + (i mod 600) + 1 on, whose aggregates are
    distinct and differ from its own; no row without an aggregate lies there."""
    rng = np.random.default_rng(23)
    n = GRID + 257
    agg = (np.arange(n) % 600).astype(np.int32)
    sizes = dict(heavy_light=(300, 1), light_heavy=(1, 300), empty_heavy=(0, 300), heavy_empty=(300, 0), full_65=(512, 65))
    special, want = {}, {}
    for b in range(257):
        for i, c in zip((b, b + GRID), sizes[PAIRS[b % 5]]):
            want[i] = c
            if c == 0:
                agg[i] = -1
            s = 1200 + i % 600 + 1
            cols = sorted([i] + list(range(s, s + max(c, 1) - 1)))
            special[i] = [(j, 4.0 if j == i else float(dyadic(rng, 1)[0])) for j in cols]
    A = _square(rng, n, special, diag=4.0)
    c = ProlongatorCase("grid_stride", A, agg, 600, None, None, True)
    for i, k in want.items():
        assert c.widths[i] == k, (i, k, int(c.widths[i]))
    assert n > GRID and c.widths.max() == MAX_CAND
    return c


CANDIDATES = (1, 64, 65, 128, 129, 256, 257, 511, 512, 513)
LONG_ROWS = (512, 513, 1024, 1100)
PROLONGATOR_NAMES = ([f"cand_{c}" for c in CANDIDATES] + [f"long_{L}" for L in LONG_ROWS] +
                     ["penalty", "collide_2040", "grid_stride"])


@functools.lru_cache(maxsize=None)
def prolongator_case(name):
    if name.startswith("cand_"):
        return _cand_case(int(name[5:]))
    if name.startswith("long_"):
        return _long_case(int(name[5:]))
    return {"penalty": _penalty_case, "collide_2040": _sa_collide_case, "grid_stride": _sa_stride_case}[name]()


@functools.lru_cache(maxsize=None)
def truncation_case():
    """Row 0 with 300 candidates whose values are built for the truncation rule: f_0 = -1/8, so p_J = -a_0J / 8 exactly
    (and 1 - a_00 / 8 for its own column).  |p| takes the values m = 2, m / 4 (exactly tau m for tau = 1/4: kept), m / 8
    (dropped) and ties of opposite signs; the aggregates run over all three components."""
    rng = np.random.default_rng(29)
    n = 640
    agg = np.arange(n, dtype=np.int32)
    vals = np.empty(300)
    mags = np.array([16.0, 4.0, 2.0, 4.0, 1.0, 2.0, 8.0, 4.0])               # |a|: |p| = 2, .5, .25, .5, .125, .25, 1, .5
    for j in range(300):
        vals[j] = mags[j % 8] * (1 if (j // 8) % 2 == 0 else -1)             # the same |p| with both signs
    row0 = [(j, 4.0 if j == 0 else float(vals[j])) for j in range(300)]
    A = _square(rng, n, {0: row0})
    c = ProlongatorCase("truncation", A, agg, n, 0, 300, True)
    J, p = c.row_of(c.ref, 0)
    m = np.abs(p).max()
    assert m == 2.0 and p[0] == 0.5 and (np.abs(p) == 0.25 * m).sum() > 50 and (np.abs(p) < 0.25 * m).sum() > 50
    assert np.any((p == 0.5)[1:]) and np.any(p == -0.5)                     # ties in |p| with opposite signs
    return c


# (block_size, drop_tolerance, max_row_entries): what each is for
TRUNCATIONS = (
    (3, 0.0, 1),       # only the row's own column stays: two components keep nothing
    (3, 0.0, 4),       # the cap cuts inside a run of equal |p|
    (1, 0.0, 65),      # a cap beyond one 64-lane pass
    (3, 0.0, 200),     # a cap beyond three passes, ties of opposite signs at the cut
    (1, 0.25, 0),      # |p| == tau m exactly: kept
    (3, 0.25, 0),
    (3, 0.25, 65),     # the cap bites only after the tolerance has dropped some
    (1, 0.5, 200),     # the tolerance leaves fewer than the cap: the cap does not bite
)


def check_truncation_properties(case, T, bs, tau, cap):
    """What each entry of TRUNCATIONS was chosen for, asserted on the restated rule's row 0 (T) and the untruncated one."""
    J, p = case.row_of(case.ref, 0)
    g = int(case.agg[0])
    m = np.abs(p).max()
    K0 = (np.abs(p) >= tau * m) | (J == g)
    n0 = int(K0.sum())
    kept = T.col[T.row_ptr[0]:T.row_ptr[1]]
    assert g in kept
    if cap > 0 and n0 > cap:
        assert kept.size == cap
        rest = sorted(np.flatnonzero(K0 & (J != g)).tolist(), key=lambda t: (-abs(p[t]), J[t]))
        if cap > 1:                                  # the cut falls inside a run of equal |p| that holds both signs
            cut = abs(p[rest[cap - 2]])
            assert cut == abs(p[rest[cap - 1]]) and {np.sign(p[t]) for t in rest if abs(p[t]) == cut} == {-1.0, 1.0}
    else:
        assert kept.size == n0
    if tau > 0.0:
        edge = J[np.abs(p) == tau * m]
        assert edge.size > 0 and n0 < p.size         # |p| == tau m exactly exists; the tolerance drops some
        if cap == 0:
            assert np.isin(edge, kept).all()         # ... and is kept
    if cap == 1:
        assert bs == 3 and set((kept % bs).tolist()) == {g % bs}           # two components keep nothing
    if (bs, tau, cap) == (3, 0.25, 65):
        assert 65 < n0 < p.size                      # the cap bites only after the tolerance has dropped some
    if (bs, tau, cap) == (1, 0.5, 200):
        assert n0 <= 200
