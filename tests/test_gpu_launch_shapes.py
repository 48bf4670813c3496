"""Every SpMV launch shape the ALFD_SPMV_* variables select at alfd_create, bit for bit against the oracle.

The suite pins each storage form at the shape a context defaults to; the (R, U) instantiations of the stream, window,
group and value-indexed kernels, the in-order paths, the XCD block orders, the grid cap and the planner inputs behind
the other variables stay selectable "for re-measuring" and are reached here, on the matrices of launch_shape_cases.py
(a few thousand rows: ALFD_SPMV_WINDOW_MIN_BLOCKS = 1 and ALFD_SPMV_WINDOW_SHORT_MIN_BLOCKS = 1 let them take the window
forms).  Every case runs epilogues 2, 3, 0 and 1 out of NaN-prefilled outputs through spmv_reference.Case.check
(canonical sums of the oracle bit for bit, np.longdouble row sums within the derived bound) and then asks
alfd_get_last_spmv_launch which kernel ran: family, lanes, R, U, non-temporal loads, block order.  A shape no dispatch
list names falls through to another family without a word; the record is what tells.

The tables below are compared with the dispatch lists in alfd.hip by a test that needs no GPU, so a shape added to the
source cannot go untested.  Each case prints its record; the distinct (family, lanes, R, U, NT, xcd) records of a full
run number the entries of the tables."""
import os
import re

import numpy as np
import pytest

import launch_shape_cases as lc
import prec_values_reference as pv
from fictitious_domain_al_preconditioners_amd import _abi, problems, solver
from oracle import oracle

STREAM_SHAPES = [(2, 2), (2, 4), (4, 2), (4, 4), (4, 8), (8, 4), (8, 8), (1, 4), (2, 8), (8, 2)]
WINDOW_SHAPES = [(1, 4), (2, 4), (2, 8), (4, 2), (4, 4), (4, 8), (8, 4), (1, 8), (1, 16), (2, 16)]
GROUP_SHAPES = [(4, 4), (2, 4), (4, 2), (8, 4), (8, 2)]
VI_SHAPES = [(4, 3), (2, 4), (4, 4), (4, 2)]            # (4, 2) is the launcher's default, the last of its chain
WINDOW_ON = {"ALFD_SPMV_WINDOW_MIN_BLOCKS": "1", "ALFD_SPMV_WINDOW_SHORT_MIN_BLOCKS": "1"}
SOURCE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                      "fictitious_domain_al_preconditioners_amd", "csrc", "alfd.hip")
ids = lambda v: "-".join(map(str, v)) if isinstance(v, tuple) else str(v)   # noqa: E731


def run(monkeypatch, env, case, want, info=None, batch_major=0, tag=""):
    """One context with `env` set before alfd_create: upload, matrix_info against `info` (values, or predicates of the
    whole dict), the four epilogues against both references, then the record of the last launch (epilogue 1) against
    `want`.  Returns (info, record)."""
    for k, v in env.items():
        monkeypatch.setenv(k, str(v))
    ctx = solver.Context(0)
    try:
        with pytest.raises(solver.AlfdError) as e:                    # nothing launched yet
            ctx.last_spmv_launch()
        assert e.value.status == _abi.E_NOT_SETUP
        if batch_major is not None:
            ctx.set_tunable("batch_major", batch_major)
        ctx.set_matrix(_abi.A, case.m)
        got = ctx.matrix_info(_abi.A)
        for k, v in (info or {}).items():
            assert v(got) if callable(v) else got[k] == v, (tag, k, got)
        case.check(ctx, tag, mode1=True)
        rec = ctx.last_spmv_launch()
        print("launch record", tag, {k: rec[k] for k in ("family_name", "lanes", "R", "U", "nontemporal", "xcd_order",
                                                         "grid", "lds_bytes")})
        want = dict(dict(nontemporal=0, xcd_order=0, epilogue=1), **want)
        assert {k: rec[k] for k in want} == want, (tag, rec)
        return got, rec
    finally:
        ctx.close()


gpu = pytest.mark.gpu


# ------------------------------------------------------------------------------------------------ 1. stream kernel
@gpu
@pytest.mark.parametrize("nt", [0, 1])
@pytest.mark.parametrize("shape", STREAM_SHAPES, ids=ids)
def test_stream_kernel_shapes_bitwise(built, monkeypatch, shape, nt):
    """spmv_stream_kernel<R, U, EPI, NT> for every pair of launch_stream_RU, with and without non-temporal loads, on
    3365 long rows with the window forms off."""
    R, U = shape
    env = {"ALFD_SPMV_WINDOW": 0, "ALFD_SPMV_STREAM_R": R, "ALFD_SPMV_STREAM_U": U, "ALFD_SPMV_NT": nt}
    case = lc.case("long", 3365, "random")
    _, rec = run(monkeypatch, env, case, dict(family=_abi.SPMV_STREAM, lanes=64, R=R, U=U, nontemporal=nt),
                 info=dict(lanes=64, windowed=0, batch_major=0), tag=f"stream {shape} nt {nt}")
    assert rec["grid"] == (-(-3365 // R) + 3) // 4 and rec["lds_bytes"] == 0


@gpu
@pytest.mark.parametrize("shape", [s for s in STREAM_SHAPES if s[0] in (1, 2, 8)], ids=ids)
def test_stream_kernel_under_the_smallest_grid_cap_bitwise(built, monkeypatch, shape):
    """ALFD_SPMV_GRID = 1 caps the grid at 256 workgroups of 4 waves, one batch of R rows per wave and pass: with R = 1
    and R = 2 the 3365 rows are more than 1024 batches and the grid-stride loop wraps (asserted from the batch count).
    With R = 8 there are 421 batches, 106 workgroups: below the cap at any size this suite allows (wrapping takes more
    than 8192 rows), so that shape is pinned at the grid it gets."""
    R, U = shape
    env = {"ALFD_SPMV_WINDOW": 0, "ALFD_SPMV_STREAM_R": R, "ALFD_SPMV_STREAM_U": U, "ALFD_SPMV_GRID": 1}
    batches = -(-3365 // R)
    _, rec = run(monkeypatch, env, lc.case("long", 3365, "random"), dict(family=_abi.SPMV_STREAM, lanes=64, R=R, U=U),
                 info=dict(windowed=0), tag=f"stream {shape} grid 1")
    assert rec["grid"] == min(256, (batches + 3) // 4)
    if R < 8:
        assert rec["grid"] == 256 and batches > 4 * rec["grid"]       # a wave takes a second batch: the loop wraps
    else:
        assert rec["grid"] == 106 and batches == 421


# ---------------------------------------------------------------------------------------- 2. general window kernel
def _window_env(**more):
    return dict(WINDOW_ON, **{"ALFD_SPMV_" + k: v for k, v in more.items()})


@gpu
@pytest.mark.parametrize("shape", WINDOW_SHAPES, ids=ids)
def test_window_kernel_shapes_bitwise(built, monkeypatch, shape):
    """spmv_window_kernel<R, U> for every pair of launch_window_RU: random values (no dictionary), 36 row blocks, the
    last of 5 rows."""
    R, U = shape
    got, rec = run(monkeypatch, _window_env(STREAM_R=R, STREAM_U=U), lc.case("long", 3365, "random"),
                   dict(family=_abi.SPMV_WINDOW, lanes=64, R=R, U=U),
                   info=dict(lanes=64, windowed=1, value_indexed=0, batch_major=0, window_blocks=36,
                             window_fallback_blocks=0), tag=f"window {shape}")
    assert rec["grid"] == 36 and 0 < rec["lds_bytes"] <= 8 * 4096


@gpu
@pytest.mark.parametrize("n", lc.LONG_SIZES)
def test_window_kernel_xcd_block_order_bitwise(built, monkeypatch, n):
    """ALFD_SPMV_WINDOW_XCD = 1: the remap of blockIdx to row blocks on 36 (36 mod 8 = 4), 32 and 5 workgroups."""
    blocks = -(-n // 96)
    _, rec = run(monkeypatch, _window_env(WINDOW_XCD=1), lc.case("long", n, "random"),
                 dict(family=_abi.SPMV_WINDOW, lanes=64, R=2, U=8, xcd_order=1),
                 info=dict(windowed=1, value_indexed=0, window_blocks=blocks), tag=f"window xcd {n}")
    assert rec["grid"] == blocks


@gpu
@pytest.mark.parametrize("var,value", [("WINDOW_RB", 4), ("WINDOW_RB", 100), ("WINDOW_RB", 250), ("WINDOW_GAP", 1),
                                       ("WINDOW_GAP", 64)])
def test_window_planner_inputs_bitwise(built, monkeypatch, var, value):
    """Row blocks of 4 (two of the four waves idle at R = 2), 100 and 250 rows; window segments that bridge no gap and
    gaps of up to 63 columns.  Four rows hold some 400 entries: fewer than the 512 distinct values a block dictionary
    takes, whatever the values.  The planner's sample therefore takes even random values for dictionary-codable and plans
    with ALFD_SPMV_WINDOW_RB_VI rows per block instead of 4 (and with that variable at 0 it codes every 4-row block),
    so the 4-row case also sets ALFD_SPMV_VALUE_INDEX = 0: no dictionaries, the general kernel on the blocks asked
    for."""
    blocks = -(-3365 // value) if var == "WINDOW_RB" else 36
    env = _window_env(**{var: value})
    if (var, value) == ("WINDOW_RB", 4):
        env["ALFD_SPMV_VALUE_INDEX"] = 0
    run(monkeypatch, env, lc.case("long", 3365, "random"),
        dict(family=_abi.SPMV_WINDOW, lanes=64, R=2, U=8),
        info=dict(windowed=1, value_indexed=0, window_blocks=blocks, window_fallback_blocks=0), tag=f"{var}={value}")


@gpu
def test_window_kernel_fallback_blocks_bitwise(built, monkeypatch):
    """ALFD_SPMV_WINDOW_MAXW = 512 on 32 full blocks: the 16 blocks of the narrow half stage their window, the 16 of the
    wide half gather from global memory (a plan with more than half of its blocks falling back is dropped, which is
    why this case runs on 3072 rows: at 3365 the block across the middle tips the balance)."""
    got, _ = run(monkeypatch, _window_env(WINDOW_MAXW=512), lc.case("long", 3072, "random"),
                 dict(family=_abi.SPMV_WINDOW, lanes=64, R=2, U=8),
                 info=dict(windowed=1, window_blocks=32, fallback=lambda i: 0 < i["window_fallback_blocks"] < i["window_blocks"]),
                 tag="maxw 512")
    assert got["window_fallback_blocks"] == 16


@gpu
def test_window_plan_with_every_block_falling_back_is_dropped_bitwise(built, monkeypatch):
    """ALFD_SPMV_WINDOW_MAXW = 256: no block's window fits, the planner keeps no window form and the stream kernel
    runs."""
    run(monkeypatch, _window_env(WINDOW_MAXW=256), lc.case("long", 3365, "random"),
        dict(family=_abi.SPMV_STREAM, lanes=64, R=2, U=8), info=dict(windowed=0, window_blocks=0), tag="maxw 256")


# ----------------------------------------------------------------------------------------- 3. value-indexed kernels
def _three_block_kinds(i):
    """8-bit, 16-bit and raw blocks in one matrix."""
    return 0 < i["value_wide_nnz"] < i["value_indexed_nnz"] and 0 < i["value_indexed_blocks"] < i["window_blocks"]


def _vi_info(values):
    if values == "coded":
        return dict(lanes=64, windowed=1, value_indexed=1, batch_major=0, kinds=_three_block_kinds)
    return dict(lanes=64, windowed=1, value_indexed=1, batch_major=0, value_wide_nnz=0, value_indexed_blocks=36)


@gpu
@pytest.mark.parametrize("xcd", [0, 1])
@pytest.mark.parametrize("values", ["coded", "few"])
def test_class_batched_value_indexed_kernel_bitwise(built, monkeypatch, values, xcd):
    """spmv_window_vib_kernel in both block orders; rows of 1 .. 1025 entries cover its classes 0 .. 6 and the generic
    path beyond 384 entries."""
    run(monkeypatch, _window_env(VI_XCD=xcd), lc.case("long", 3365, values),
        dict(family=_abi.SPMV_WINDOW_VIB, lanes=64, R=0, U=0, xcd_order=xcd), info=_vi_info(values),
        tag=f"vib {values} xcd {xcd}")


@gpu
@pytest.mark.parametrize("shape", VI_SHAPES, ids=ids)
@pytest.mark.parametrize("values", ["coded", "few"])
def test_in_order_value_indexed_kernel_shapes_bitwise(built, monkeypatch, values, shape):
    """ALFD_SPMV_VI_BATCHED = 0: spmv_window_vi_kernel<R, J> for each pair of launch_window."""
    R, J = shape
    run(monkeypatch, _window_env(VI_BATCHED=0, VI_R=R, VI_J=J), lc.case("long", 3365, values),
        dict(family=_abi.SPMV_WINDOW_VI, lanes=64, R=R, U=J), info=_vi_info(values), tag=f"vi {values} {shape}")


@gpu
@pytest.mark.parametrize("values", ["coded", "few"])
def test_general_kernel_on_a_dictionary_coded_matrix_bitwise(built, monkeypatch, values):
    """ALFD_SPMV_VI_BATCHED = 0 and ALFD_SPMV_VI_R = 0: the general window kernel reads the 8-byte values of a matrix
    that also holds dictionaries."""
    run(monkeypatch, _window_env(VI_BATCHED=0, VI_R=0), lc.case("long", 3365, values),
        dict(family=_abi.SPMV_WINDOW, lanes=64, R=2, U=8), info=_vi_info(values), tag=f"vi off {values}")


@gpu
@pytest.mark.parametrize("rb", [32, 96, 200])
@pytest.mark.parametrize("values", ["coded", "few"])
def test_value_indexed_row_block_bitwise(built, monkeypatch, values, rb):
    """ALFD_SPMV_WINDOW_RB_VI: `few` is codable everywhere and takes the row block asked for; of `coded` a third of the
    sampled blocks is not (random values), fewer than the three quarters the planner asks for, so it keeps 96 rows."""
    blocks = -(-3365 // rb) if values == "few" else 36
    info = dict(_vi_info(values), window_blocks=blocks)
    if values == "few":
        info["value_indexed_blocks"] = blocks
    run(monkeypatch, _window_env(WINDOW_RB_VI=rb), lc.case("long", 3365, values),
        dict(family=_abi.SPMV_WINDOW_VIB, lanes=64, R=0, U=0), info=info, tag=f"rb_vi {rb} {values}")


# -------------------------------------------------------------------------------------------------- 4. group kernel
def _short_block(L, scale):
    return min(512, 96 * scale * 64 // L)


@gpu
@pytest.mark.parametrize("shape", GROUP_SHAPES, ids=ids)
@pytest.mark.parametrize("L", [32, 16, 8])
def test_group_kernel_shapes_bitwise(built, monkeypatch, L, shape):
    """spmv_window_group_kernel<L, R, U> for every pair of launch_window_group_RU on the ragged bands: rows of 0 ..
    4 L + 1 entries, a partial last block."""
    R, U = shape
    n = lc.SHORT_SIZES[L]
    _, rec = run(monkeypatch, _window_env(GROUP_R=R, GROUP_U=U), lc.case("short", L),
                 dict(family=_abi.SPMV_WINDOW_GROUP, lanes=L, R=R, U=U),
                 info=dict(lanes=L, windowed=1, batch_major=0, window_blocks=-(-n // _short_block(L, 2)),
                           window_fallback_blocks=0), tag=f"group L{L} {shape}")
    assert rec["grid"] == -(-n // _short_block(L, 2))


@gpu
@pytest.mark.parametrize("scale", [0, 1])
@pytest.mark.parametrize("L", [32, 16, 8])
def test_short_row_block_scale_bitwise(built, monkeypatch, L, scale):
    """ALFD_SPMV_WINDOW_SHORT = 1: row blocks of min(512, 96 * 64 / L) rows (2, the default, runs above); 0: no window
    form for short rows, spmv_kernel<L>."""
    n = lc.SHORT_SIZES[L]
    if scale:
        want = dict(family=_abi.SPMV_WINDOW_GROUP, lanes=L, R=4, U=4)
        info = dict(lanes=L, windowed=1, window_blocks=-(-n // _short_block(L, 1)))
    else:
        want, info = dict(family=_abi.SPMV_PLAIN, lanes=L, R=0, U=0), dict(lanes=L, windowed=0)
    run(monkeypatch, _window_env(WINDOW_SHORT=scale), lc.case("short", L), want, info=info, tag=f"short scale {scale} L{L}")


# ------------------------------------------------------------------------------- 5. unlisted and cross-family pairs
@gpu
@pytest.mark.parametrize("name", ["3-8 windowed", "2-2 windowed", "1-16 unwindowed", "group 3-4", "vi 3-3"])
def test_unlisted_shapes_fall_through_to_a_correct_kernel(built, monkeypatch, name):
    """A pair no dispatch list names does not fail: (3, 8) is in neither list and a windowed matrix runs on spmv_kernel<64>;
    (2, 2) is a stream shape the window list lacks, and the windowed matrix runs on the stream kernel; (1, 16) is a window
    shape the stream list lacks, and an unwindowed matrix runs on spmv_kernel<64>; an unlisted group pair runs spmv_kernel<L>
    and an unlisted (R, J) the value-indexed default (4, 2).  Same bits every time, and the record says which."""
    long_random, windowed = lc.case("long", 3365, "random"), dict(lanes=64, windowed=1, value_indexed=0)
    env, case, want, info = {
        "3-8 windowed": (_window_env(STREAM_R=3, STREAM_U=8), long_random,
                         dict(family=_abi.SPMV_PLAIN, lanes=64, R=0, U=0), windowed),
        "2-2 windowed": (_window_env(STREAM_R=2, STREAM_U=2), long_random,
                         dict(family=_abi.SPMV_STREAM, lanes=64, R=2, U=2), windowed),
        "1-16 unwindowed": ({"ALFD_SPMV_WINDOW": 0, "ALFD_SPMV_STREAM_R": 1, "ALFD_SPMV_STREAM_U": 16}, long_random,
                            dict(family=_abi.SPMV_PLAIN, lanes=64, R=0, U=0), dict(lanes=64, windowed=0)),
        "group 3-4": (_window_env(GROUP_R=3, GROUP_U=4), lc.case("short", 16),
                      dict(family=_abi.SPMV_PLAIN, lanes=16, R=0, U=0), dict(lanes=16, windowed=1)),
        "vi 3-3": (_window_env(VI_BATCHED=0, VI_R=3, VI_J=3), lc.case("long", 3365, "few"),
                   dict(family=_abi.SPMV_WINDOW_VI, lanes=64, R=4, U=2), dict(lanes=64, windowed=1, value_indexed=1)),
    }[name]
    run(monkeypatch, env, case, want, info=info, tag=name)


# --------------------------------------------------------------------------------------------- 6. related checks
@gpu
def test_pair_launch_is_refused_on_another_stream_shape(built, monkeypatch):
    """The pair launch has one stream instantiation, (2, 8): under ALFD_SPMV_STREAM_R = 4, _U = 4 alfd_spmv_pair on a
    stream-kernel A answers ALFD_E_UNSUPPORTED and writes neither output; under the default shape the same pair goes
    through with the bits of the two launches."""
    case, c = lc.case("long", 3365, "random"), lc.case("random", 3365, 14)
    x, d = case.x, c.d
    for shape, ok in (((4, 4), False), ((2, 8), True)):
        monkeypatch.setenv("ALFD_SPMV_WINDOW", "0")
        monkeypatch.setenv("ALFD_SPMV_STREAM_R", str(shape[0]))
        monkeypatch.setenv("ALFD_SPMV_STREAM_U", str(shape[1]))
        ctx = solver.Context(0)
        try:
            ctx.set_matrix(_abi.A, case.m)
            ctx.set_matrix(_abi.C_, c.m)
            assert ctx.matrix_info(_abi.A)["windowed"] == 0 and ctx.matrix_info(_abi.C_)["lanes"] == 16
            y, t = np.full(3365, np.nan), np.full(3365, np.nan)
            rc = ctx._lib.alfd_spmv_pair(ctx._h, _abi.A, _abi.C_, x.ctypes.data, d.ctypes.data, y.ctypes.data, t.ctypes.data)
            if ok:
                assert rc == _abi.OK
                assert np.array_equal(y, case.s) and np.array_equal(t, d * oracle.spmv(c.m, x, None, mode=0)[0])
                rec = ctx.last_spmv_launch()
                assert (rec["family"], rec["R"], rec["U"]) == (_abi.SPMV_STREAM, 2, 8) and rec["grid"] > 421
            else:
                assert rc == _abi.E_UNSUPPORTED, rc
                assert np.isnan(y).all() and np.isnan(t).all()
                with pytest.raises(solver.AlfdError):
                    ctx.last_spmv_launch()                         # and nothing was launched
        finally:
            ctx.close()


@gpu
def test_single_precision_copy_keeps_its_shape_under_another_stream_shape(built, monkeypatch):
    """Under ALFD_SPMV_STREAM_R = 4, _U = 4 the single-precision copy of slot A still runs its one stream instantiation,
    (2, 8) on float, and gives the bits of the 8-byte kernel on the rounded values; alfd_spmv beside it runs (4, 4)."""
    case = lc.case("long", 3365, "random")
    f, _ = pv.round_values(case.m.val)
    rounded = problems.Csr(3365, 3365, case.m.row_ptr, case.m.col, f.astype(np.float64))
    want0, _ = oracle.spmv(rounded, case.x, None, mode=0)
    want1, _ = oracle.spmv(rounded, case.x, case.y0, mode=1, alpha=-0.75)
    assert not np.array_equal(want0, case.s)
    for k, v in {"ALFD_SPMV_WINDOW": 0, "ALFD_SPMV_STREAM_R": 4, "ALFD_SPMV_STREAM_U": 4}.items():
        monkeypatch.setenv(k, str(v))
    ctx = solver.Context(0)
    try:
        ctx.set_preconditioner_values("fp32")
        ctx.set_matrix(_abi.A, case.m)
        assert ctx.preconditioner_values()["stored"] == 1
        y = ctx.spmv_preconditioner(case.x, np.full(3365, np.nan), mode=0)
        assert np.array_equal(y, want0)
        rec = ctx.last_spmv_launch()
        assert (rec["family"], rec["R"], rec["U"], rec["epilogue"]) == (_abi.SPMV_STREAM_F32, 2, 8, 0), rec
        assert np.array_equal(ctx.spmv_preconditioner(case.x, case.y0, mode=1, alpha=-0.75), want1)
        assert ctx.last_spmv_launch()["epilogue"] == 1
        y, _ = ctx.spmv(_abi.A, case.x, np.full(3365, np.nan), mode=0)
        assert np.array_equal(y, case.s)
        rec = ctx.last_spmv_launch()
        assert (rec["family"], rec["R"], rec["U"]) == (_abi.SPMV_STREAM, 4, 4), rec
    finally:
        ctx.close()


# ------------------------------------------------------------------------------------ 7. table guard (no GPU)
def _function_body(text, head):
    at = text.index(head)
    return text[at:text.index("\n}\n", at)]


def _table(text, name):
    """The pairs of `constexpr Shape name[] = {...};`, which the source must define exactly once."""
    found = re.findall(r"^constexpr Shape " + name + r"\[\] = \{(.*?)\};", text, re.M | re.S)
    assert len(found) == 1, (name, found)
    pairs = re.findall(r"\{(\d+), (\d+)\}", found[0])
    assert "{" + "}, {".join(f"{a}, {b}" for a, b in pairs) + "}" == found[0], (name, found[0])   # nothing but pairs
    return [(int(a), int(b)) for a, b in pairs]


def test_tables_match_the_dispatch_lists_of_the_source():
    """The (R, U) / (R, J) lists that launch_stream_RU, launch_window_RU, launch_window_group_RU and launch_window look
    their shape up in, read out of alfd.hip: a shape added there (or dropped) shows here.  Each launcher must name its
    own list, the value-indexed one with its last entry as the default."""
    with open(SOURCE) as f:
        text = f.read()
    assert _table(text, "kStreamShapes") == STREAM_SHAPES
    assert _table(text, "kWindowShapes") == WINDOW_SHAPES
    assert _table(text, "kGroupShapes") == GROUP_SHAPES
    assert _table(text, "kViShapes") == VI_SHAPES                      # default last
    for head, lookup in (("static bool launch_stream_RU(", "with_shape<kStreamShapes>(ctx->spmv_stream_R, ctx->spmv_stream_U, false,"),
                         ("static bool launch_window_RU(", "with_shape<kWindowShapes>(ctx->spmv_stream_R, ctx->spmv_stream_U, false,"),
                         ("static bool launch_window_group_RU(", "with_shape<kGroupShapes>(ctx->spmv_group_R, ctx->spmv_group_U, false,"),
                         ("static void launch_window(", "with_shape<kViShapes>(ctx->vi_rows_R, ctx->vi_rows_J, true,")):
        body = _function_body(text, head)
        assert re.findall(r"with_shape<\w+>\([^\[]*", body) == [lookup + " "], (head, body)
    for shapes in (STREAM_SHAPES, WINDOW_SHAPES, GROUP_SHAPES, VI_SHAPES):
        assert len(set(shapes)) == len(shapes)
    # the group launcher is reached for exactly these lane counts, in this order, and from nowhere else
    reached = re.findall(r"with_const<([\d, ]+)>\(m\.L, \[&\]\(auto l\) \{ ok = launch_window_group_RU<decltype\(l\)::value>\(", text)
    assert [[int(v) for v in r.split(", ")] for r in reached] == [[32, 16, 8]]
    assert text.count("launch_window_group_RU<") == 1
