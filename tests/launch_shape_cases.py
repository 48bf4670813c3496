"""Matrices for the SpMV launch-shape tests (tests/test_gpu_launch_shapes.py) and the storage forms on partitions
(tests/test_gpu_partitioned_forms.py).  NumPy and the project's generator only: nothing here calls libalfd.  Every
generator is deterministic (fixed seeds), cached, and returns read-only arrays; case(...) wraps a matrix into a
spmv_reference.Case, whose bitwise reference is the oracle's canonical sum and whose independent reference is the
np.longdouble row sum with the bound (len_r + 2) 2^-53 |d_r| (|A||x|)_r.

A few thousand rows reach every window form once ALFD_SPMV_WINDOW_MIN_BLOCKS = 1 (and _SHORT_MIN_BLOCKS = 1) is set, so
each case costs a fraction of a second on the device.

long_rows(n): square, 64 lanes (mean over the non-empty rows above 48, asserted).  Rows hold uniform(40, 160) distinct
sorted columns, rows < n / 2 from [i - 100, i + 100], the others from [i - 700, i + 700], clipped to the matrix: with
ALFD_SPMV_WINDOW_MAXW = 512 the narrow half stages its x window and the wide half gathers from global memory.  Planted in
the wide half, no two in one 8-row batch, longest first (nearest n / 2, where the band is not yet clipped): rows of 1025,
1024, 1023, 513, 512, 511, 257, 256, 255, 129, 128, 127, 65, 64, 63 and 1 entries -- they straddle the 64-entry chunk,
every 64 U pass for U <= 16 and the class limit 6 (384 entries) of the class-batched kernel.  A planted length that the
clipped band cannot hold is cut to what fits (n = 480 has 480 columns: 1025 .. 511 come out as the full clipped band).
Row 0, the last row and one aligned run of 8 rows are empty; about 100 entries sit in far columns (c + n / 2 mod n).
`longest` caps the planted lengths: the long-row batch-major form takes rows of at most 384 entries, so its cases use
long_rows(n, longest=384), planted 384, 383 and 257 .. 1.

Row counts: 3365 = 35 blocks of 96 and one of 5 (36 mod 8 = 4: an uneven XCD remap), 3072 = 32 full blocks, 480 = 5
blocks (fewer than one per XCD)."""
import functools
import zlib

import numpy as np

from fictitious_domain_al_preconditioners_amd import problems
from oracle import oracle
from spmv_reference import Case

LONG_SIZES = (3365, 3072, 480)
PLANTED_LONG = (1025, 1024, 1023, 513, 512, 511, 257, 256, 255, 129, 128, 127, 65, 64, 63, 1)
SHORT_SIZES = {32: 6 * 384 + 37, 16: 5 * 512 + 37, 8: 5 * 512 + 37}
# mean row length of short_rows(L): inside the lane rule's interval (24, 48], (12, 24], (6, 12]
SHORT_LENGTHS = {32: (20, 52), 16: (8, 28), 8: (3, 15)}


def _freeze(m):
    for a in (m.row_ptr, m.col, m.val):
        a.setflags(write=False)
    return m


def _csr(n, rows_cols, val_of):
    """rows_cols: one sorted array of distinct columns per row."""
    ln = np.array([c.size for c in rows_cols], np.int64)
    rp = np.concatenate([[0], np.cumsum(ln)]).astype(np.int64)
    col = (np.concatenate(rows_cols) if rp[-1] else np.zeros(0)).astype(np.int32)
    for r in range(n):
        c = col[rp[r]:rp[r + 1]]
        assert np.all(np.diff(c) > 0) and (c.size == 0 or (c[0] >= 0 and c[-1] < n)), r
    return problems.Csr(n, n, rp, col, val_of(rp, col))


def _band(rng, n, i, w, k):
    lo, hi = max(0, i - w), min(n - 1, i + w)
    k = min(k, hi - lo + 1)
    return np.sort(lo + rng.choice(hi - lo + 1, k, replace=False))


def _far(rng, n, cols, protect, count):
    """Move one entry of `count` rows to the column half a matrix away."""
    pick = [r for r in rng.permutation(n) if r not in protect and cols[r].size > 1][:count]
    for r in pick:
        c = cols[r].copy()
        far = (int(c[c.size // 2]) + n // 2) % n
        if far not in c:
            c[c.size // 2] = far
            cols[r] = np.sort(c)
    return len(pick)


@functools.lru_cache(maxsize=None)
def long_structure(n, longest=1025):
    """(row_ptr, col, planted rows) of long_rows(n)."""
    rng = np.random.default_rng(1000 + n)
    planted = [k for k in PLANTED_LONG if k <= longest]
    if longest < PLANTED_LONG[0]:
        planted = [longest, longest - 1] + planted
    half = n // 2
    stride = max(8, (n - half - 16) // len(planted) // 8 * 8)
    at = {half + 11 + stride * j: k for j, k in enumerate(planted)}
    assert max(at) < n - 1 and len({r // 8 for r in at}) == len(at)
    empty = {0, n - 1} | set(range(n // 4 // 8 * 8, n // 4 // 8 * 8 + 8))
    cols = []
    for i in range(n):
        if i in empty:
            cols.append(np.zeros(0, np.int64))
        elif i in at:
            cols.append(_band(rng, n, i, 700, at[i]))
        else:
            cols.append(_band(rng, n, i, 100 if i < half else 700, int(rng.integers(40, 161))))
    if n >= 3000:                                     # the band holds every planted length
        assert [cols[r].size for r in sorted(at)] == planted
    assert _far(rng, n, cols, empty | set(at), 100) == 100
    m = _csr(n, cols, lambda rp, col: np.zeros(col.size))
    ln = np.diff(m.row_ptr)
    assert ln[ln > 0].mean() > 48 and (ln == 0).sum() == 10
    m.row_ptr.setflags(write=False)
    m.col.setflags(write=False)
    return m.row_ptr, m.col, tuple(sorted(at))


def _values(kind, n, rp, col):
    rng = np.random.default_rng({"random": 21, "coded": 22, "few": 23}[kind] + n)
    nnz = col.size
    v = rng.uniform(-1.0, 1.0, nnz)
    if kind == "few":                                 # 40 distinct values
        v = rng.uniform(-1.0, 1.0, 40)[rng.integers(0, 40, nnz)]
    elif kind == "coded":                             # 100 distinct / 400 distinct / random, by thirds of the rows
        k1, k2 = int(rp[n // 3]), int(rp[2 * n // 3])
        v[:k1] = rng.uniform(-1.0, 1.0, 100)[rng.integers(0, 100, k1)]
        v[k1:k2] = rng.uniform(-1.0, 1.0, 400)[rng.integers(0, 400, k2 - k1)]
    return v


@functools.lru_cache(maxsize=None)
def long_rows(n, values="random", longest=1025):
    """long_rows(n) with one of the three value fields: `random` (no dictionary), `coded` (rows < n / 3 from 100
    distinct values, the middle third from 400, the rest random: 8-bit, 16-bit and raw blocks in one matrix whatever
    the row block) and `few` (40 distinct values)."""
    rp, col, _ = long_structure(n, longest)
    return _freeze(problems.Csr(n, n, rp, col, _values(values, n, rp, col)))


@functools.lru_cache(maxsize=None)
def short_rows(L, n=None):
    """Ragged bands for the L-lane kernels (L = 32, 16, 8): row lengths uniform over SHORT_LENGTHS[L], columns from
    [i - 100, i + 100]; planted rows of 0, 1, L - 1, L, L + 1, 2L - 1, 2L, 2L + 1, 4L and 4L + 1 entries; empty first
    and last rows; 40 entries in far columns.  n = 6 * 384 + 37 (L = 32) and 5 * 512 + 37 (L = 16, 8): the last row
    block is partial."""
    n = SHORT_SIZES[L] if n is None else n
    rng = np.random.default_rng(2000 + L)
    planted = (0, 1, L - 1, L, L + 1, 2 * L - 1, 2 * L, 2 * L + 1, 4 * L, 4 * L + 1)
    at = {300 + 173 * j: k for j, k in enumerate(planted)}
    lo, hi = SHORT_LENGTHS[L]
    cols = []
    for i in range(n):
        if i in (0, n - 1):
            cols.append(np.zeros(0, np.int64))
        else:
            cols.append(_band(rng, n, i, 100, at[i] if i in at else int(rng.integers(lo, hi + 1))))
    assert [cols[r].size for r in sorted(at)] == list(planted)
    assert _far(rng, n, cols, {0, n - 1} | set(at), 40) == 40
    m = _csr(n, cols, lambda rp, col: rng.uniform(-1.0, 1.0, col.size))
    ln = np.diff(m.row_ptr)
    assert L * 0.75 < ln[ln > 0].mean() <= L * 1.5     # the lane rule's interval for L
    return _freeze(m)


@functools.lru_cache(maxsize=None)
def random_rows(n, avg, empty_share=0):
    """Rows of avg / 2 .. 3 avg / 2 distinct columns anywhere in the matrix (no window form takes them); with
    empty_share = k only every k-th row holds entries (k >= 3: the sparse-row form)."""
    rng = np.random.default_rng(3000 + 7 * avg + empty_share)
    cols = []
    for i in range(n):
        if empty_share and i % empty_share:
            cols.append(np.zeros(0, np.int64))
        else:
            cols.append(np.sort(rng.choice(n, int(rng.integers(max(1, avg // 2), 3 * avg // 2 + 1)), replace=False)))
    return _freeze(_csr(n, cols, lambda rp, col: rng.uniform(-1.0, 1.0, col.size)))


@functools.lru_cache(maxsize=None)
def stencil():
    """The 9-point Q1 stencil on 57 x 57 cells (3364 rows, 8 lanes): with one row block of 512 rows as the threshold
    (ALFD_SPMV_WINDOW_SHORT_MIN_BLOCKS = 1) it is the batch-major short-row form that takes it."""
    return _freeze(problems.generate(dim=2, degree=1, ncomp=1, n_cells=57, radius=0.1).mats["A"])


def row_slice(m, r0, r1):
    """Rows r0 .. r1 - 1 with their global columns: what the rank owning them uploads."""
    return m.slice_rows(r0, r1)


def references_every_other_rank(m, offsets):
    """Does every rank's row slice hold a column of every other rank's range?"""
    world = len(offsets) - 1
    for p in range(world):
        c = np.asarray(m.col[int(m.row_ptr[offsets[p]]):int(m.row_ptr[offsets[p + 1]])])
        for q in range(world):
            if q != p and not np.any((c >= offsets[q]) & (c < offsets[q + 1])):
                return False
    return True


@functools.lru_cache(maxsize=None)
def case(kind, *args):
    """The spmv_reference.Case of a generator's matrix (inputs and both references, computed once, read-only)."""
    m = {"long": long_rows, "short": short_rows, "random": random_rows, "stencil": stencil}[kind](*args)
    return Case(m, 500 + zlib.crc32(repr((kind,) + args).encode()) % 400)


@functools.lru_cache(maxsize=None)
def mode1_reference(kind, *args):
    """The oracle's y0 - 0.75 A x for case(kind, *args): what Case.check(mode1=True) compares epilogue 1 with."""
    c = case(kind, *args)
    y, _ = oracle.spmv(c.m, c.x, c.y0, mode=1, alpha=-0.75)
    y.setflags(write=False)
    return y
