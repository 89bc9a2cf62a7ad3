"""ORDER BY col [DESC] LIMIT k on the GPU (GpuContext.scan_topn) and the
SELECT-list gather (GpuContext.gather) against the top-n matrix
(tests/topn_matrix.py; tests/test_topn_matrix.py proves its reference and the
facts about the order columns on the CPU). Every comparison is exact: rows and
int64 values equal, float32 values as bit patterns (widened to f64 through
agg_matrix.f32_bits_to_f64_bits), isnull equal; the returned order is then
re-checked from the returned arrays alone.

Per geometry a FoR table and an all-raw one, with the planes of `m`, the
poisoned `key` and `fx` attached and a string slot made of kmod. A case runs
over the FoR columns of the FoR table, the raw columns of the FoR table and
the raw table (one 65536-row tiling: odd_t33 is a single row group there).
"""

import ctypes as C

import numpy as np
import pytest

import agg_matrix as amx
import col_matrix as cmx
import nullkey_matrix as nkx
import serenedb_amd as sa
import topn_matrix as tnx

pytestmark = pytest.mark.gpu

COL = {"m_raw": 0, "m_for": 1, "m2": 2, "keyp_raw": 3, "keyp_for": 4,
       "key_raw": 5, "key_for": 6, "f": 7, "fx": 8, "c7_raw": 9,
       "c7_for": 10}
CODECS = {"for": ["raw", "for", "for", "raw", "for", "raw", "for", "raw",
                  "raw", "raw", "for"],
          "raw": ["raw"] * 11}
NCOLS = 11
PLANE_COLS = {"m_raw": "m", "m_for": "m", "keyp_raw": "keyp",
              "keyp_for": "keyp", "fx": "fx"}
VARIANTS = (("for", "for"), ("for", "raw"), ("raw", "raw"))  # table, codec
STR_SLOT = 0
STRMASK = 7
HOOK = "SDB_TOPN_CAND_CAP"
ERR_INVALID = "rc=-1$"

M2_BAND = ("m2", cmx.BETWEEN, -5, 1 << 41)   # int64_min / int64_max base
                                             # groups are zonemap-dead
THIN = ("f", cmx.GE, 1000.0, 0.0)            # about 1.2 % of the rows
STR_K1 = ("kstr", nkx.PREFIX, b"k1", 0)
NONE = ("f", cmx.GE, 2000.0, 0.0)


@pytest.fixture(scope="module")
def ctx():
    c = sa.GpuContext(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def tabs(ctx):
    out = {}
    for name in tnx.GEOMS:
        t = tnx.matrix(name)
        arrays = [t.vals["m"], t.vals["m"], t.mx.m2.vals,
                  t.stored("keyp", "raw"), t.stored("keyp", "for"),
                  t.vals["key"], t.vals["key"], t.vals["f"], t.vals["fx"],
                  t.c7, t.c7]
        offsets, blob = sa.encode_col_str_raw(t.am.kmod_strings()[1])
        for kind, codecs in CODECS.items():
            tab = ctx.load_table(arrays, codecs, group_rows=t.group_rows)
            for col, plane in PLANE_COLS.items():
                ctx.attach_validity(tab, COL[col], t.validity_words(plane))
            ctx.attach_strcol(tab, STR_SLOT, offsets, blob)
            out[name, kind] = tab
    yield out
    for tab in out.values():
        ctx.free_table(tab)


@pytest.fixture(autouse=True)
def no_hook(monkeypatch):
    monkeypatch.delenv(HOOK, raising=False)


geoms = pytest.mark.parametrize("geom", tnx.GEOMS)


def col_of(name, codec):
    return COL[name] if name in COL else COL[f"{name}_{codec}"]


def gpu_preds(ctx, tab, codec, preds):
    gp = []
    for c, op, lo, hi in preds:
        if c == "kstr":
            ctx.strpred_mask(tab, STR_SLOT, "prefix", lo)
            gp.append((STR_SLOT, STRMASK, 0, 0))
        else:
            gp.append((col_of(c, codec), op, lo, hi))
    return gp


def f64_bits_of_f32_bits(bits):
    return np.array([amx.f32_bits_to_f64_bits(int(b)) for b in bits],
                    dtype=np.uint64)


def assert_vals(order, got, want, what):
    if order in tnx.F32_COLS:
        assert got.dtype == np.float32, what
        g = got.astype(np.float64).view(np.uint64)
        w = f64_bits_of_f32_bits(want)
        assert (got.view(np.uint32) == want).all(), what + ": f32 bits"
    else:
        assert got.dtype == np.int64, what
        g, w = got, want
    bad = np.flatnonzero(g != w)
    assert not len(bad), (
        f"{what}: {len(bad)} values differ; first at {bad[0]}: got "
        f"{got[bad[0]]!r} want {want[bad[0]]!r}")


def assert_ordered(t, order, codec, preds, rows, vals, isnull, desc,
                   nulls_first, what):
    """the order rule on the returned arrays alone: every row passes, holds
    the value returned, and (NULL class, value, row) strictly ascends"""
    r = rows.astype(np.int64)
    assert t.pred_mask(tuple(preds))[r].all(), what + ": a row does not pass"
    assert (isnull == ~t.valid(order)[r]).all(), what + ": NULL flags"
    assert not np.asarray(vals)[isnull].any(), what + ": a NULL is not 0"
    if order in tnx.F32_COLS:
        bits = vals.view(np.uint32).tolist()
        keys = [amx.f32_key_py(b) for b in bits]
        stored = amx.f32_key(t.bits(order)[r]).tolist()
        assert [k for k, n in zip(keys, isnull) if not n] == \
            [k for k, n in zip(stored, isnull) if not n], what
    else:
        keys = vals.tolist()
        assert (vals[~isnull] == t.stored(order, codec)[r][~isnull]).all(), \
            what + ": value is not the row's"
    tuples = [(bool(n) != nulls_first, 0 if n else (-v if desc else v), row)
              for n, v, row in zip(isnull.tolist(), keys, r.tolist())]
    for a, b in zip(tuples, tuples[1:]):
        assert a < b, f"{what}: {a} before {b}"


def run(ctx, tabs, t, order, preds, k, desc=False, nulls_first=False,
        variants=VARIANTS, label=""):
    """one query on every table / codec == the reference, exactly, and
    ordered by its own rule. Returns ({variant: stats}, reference)."""
    want = t.ref(order, tuple(preds), k, desc, nulls_first)
    wrows, wvals, wnull, wpassed = want
    stats = {}
    for kind, codec in variants:
        tab = tabs[t.name, kind]
        what = (f"{t.name} {label} {order} k={k} desc={desc} "
                f"nulls_first={nulls_first} {kind} table, {codec}")
        rows, vals, isnull, passed, st = ctx.scan_topn(
            tab, col_of(order, codec), k, gpu_preds(ctx, tab, codec, preds),
            desc=desc, nulls_first=nulls_first, stats=True)
        assert passed == wpassed, what + ": rows_passed"
        assert rows.dtype == np.uint64 and isnull.dtype == np.bool_
        assert len(rows) == len(vals) == len(isnull) == len(wrows), \
            f"{what}: n = {len(rows)}, want {len(wrows)}"
        bad = np.flatnonzero(rows != wrows)
        assert not len(bad), (
            f"{what}: {len(bad)} rows differ; first at {bad[0]}: got "
            f"{rows[bad[0]]} want {wrows[bad[0]]}")
        assert (isnull == wnull).all(), what + ": isnull"
        assert_vals(order, vals, wvals, what)
        assert_ordered(t, order, codec, preds, rows, vals, isnull, desc,
                       nulls_first, what)
        assert st["candidates"] <= st["cand_cap"], what
        assert st["cand_cap"] >= k + 1, what
        assert st["hist_passes"] >= 1
        stats[kind, codec] = st
    return stats, want


# ---- directions and NULL placement ---------------------------------------
@geoms
@pytest.mark.parametrize("order", tnx.ORDER_COLS)
def test_directions_and_null_placement(ctx, tabs, geom, order):
    t = tnx.matrix(geom)
    for desc in (False, True):
        for nulls_first in (False, True):
            run(ctx, tabs, t, order, (), 300, desc, nulls_first)


# ---- k edges ----------------------------------------------------------------
@geoms
@pytest.mark.parametrize("k", (1, 2, 63, 64, 65, 1000, 65536))
def test_k_edges(ctx, tabs, geom, k):
    t = tnx.matrix(geom)
    run(ctx, tabs, t, "m", (), k, desc=True)
    run(ctx, tabs, t, "f", (M2_BAND,), k, desc=False,
        variants=VARIANTS[:1])


@geoms
@pytest.mark.parametrize("delta", (-1, 0, 1))
def test_k_around_rows_passing(ctx, tabs, geom, delta):
    t = tnx.matrix(geom)
    passing = int(t.pred_mask((THIN,)).sum())
    assert 2 < passing < tnx.MAX_K
    for order in ("m", "fx"):
        for nulls_first in (False, True):
            _, (rows, _, _, passed) = run(
                ctx, tabs, t, order, (THIN,), passing + delta, True,
                nulls_first)
            assert passed == passing
            assert len(rows) == min(passing + delta, passing)


def test_k_above_table_rows(ctx, tabs):
    t = tnx.matrix("odd_t33")
    k = 40000
    assert t.rows < k <= tnx.MAX_K
    for order in ("m", "keyp", "c7", "fx"):
        _, (rows, _, _, _) = run(ctx, tabs, t, order, (), k, desc=True)
        assert len(rows) == t.rows


# ---- predicates -------------------------------------------------------------
def one_row_preds(t):
    r = t.mx.minus_one_row
    return (("m2", cmx.EQ, int(t.mx.m2.vals[r]), 0),
            ("f", cmx.EQ, float(t.vals["f"][r]), 0.0))


PRED_CASES = {
    "m2_band": lambda t: ("m", (M2_BAND,)),
    "own_ge": lambda t: ("m", (("m", cmx.GE, 0, 0),)),
    "own_lt_f32": lambda t: ("fx", (("fx", cmx.LT, 1.5, 0.0),)),
    "isnull": lambda t: ("m", (("m", cmx.ISNULL, 0, 0),)),
    "isnull_keyp": lambda t: ("keyp", (("keyp", cmx.ISNULL, 0, 0),)),
    "notnull": lambda t: ("m", (("m", cmx.NOTNULL, 0, 0), M2_BAND)),
    "f32_pred": lambda t: ("key", (("fx", cmx.GE, 0.0, 0.0),)),
    "strmask": lambda t: ("m", (STR_K1,)),
    "strmask_f32_order": lambda t: ("fx", (STR_K1, M2_BAND)),
    "four_preds": lambda t: ("c7", (M2_BAND, STR_K1,
                                    ("fx", cmx.NOTNULL, 0, 0),
                                    ("f", cmx.LT, 512.0, 0.0))),
    "one_row": lambda t: ("m", one_row_preds(t)),
    "none": lambda t: ("m", (NONE,)),
    "none_empty_range": lambda t: ("f", (("m2", cmx.BETWEEN, 5, 4),)),
}


@geoms
@pytest.mark.parametrize("case", sorted(PRED_CASES))
def test_predicates(ctx, tabs, geom, case):
    t = tnx.matrix(geom)
    order, preds = PRED_CASES[case](t)
    for desc in (False, True):
        _, (rows, vals, isnull, passed) = run(
            ctx, tabs, t, order, preds, 500, desc, label=case)
        if case.startswith("isnull"):
            # only NULL rows, in row order, whatever they store
            assert isnull.all() and passed == int((~t.valid(order)).sum())
            assert (rows == np.flatnonzero(~t.valid(order))[:500]).all()
        if case == "notnull":
            assert not isnull.any()
        if case == "one_row":
            assert passed == 1 and len(rows) == 1
        if case.startswith("none"):
            assert passed == 0 and len(rows) == 0
    if case == "m2_band":       # the predicate's zonemap has dead groups
        kinds = t.mx.m2.kinds
        assert "int64_min" in kinds and "int64_max" in kinds


# ---- stored values of NULL rows never rank --------------------------------
@geoms
@pytest.mark.parametrize("desc", (False, True))
def test_poisoned_null_rows_never_rank(ctx, tabs, geom, desc):
    t = tnx.matrix(geom)
    nonnull = int(t.valid("keyp").sum())
    for nulls_first in (False, True):
        k = min(tnx.MAX_K, t.rows)
        _, (rows, vals, isnull, _) = run(ctx, tabs, t, "keyp", (), k, desc,
                                         nulls_first)
        live = vals[~isnull]       # empty when k NULL rows come first
        assert ((0 <= live) & (live < t.mx.ngroups)).all()
        assert len(live) == min(k, nonnull) if not nulls_first else \
            len(live) == max(0, min(k - (t.rows - nonnull), nonnull))
        # NULL rows only after (or before) every value
        flips = int(np.count_nonzero(isnull[1:] != isnull[:-1]))
        assert flips <= 1
        if nulls_first:
            assert isnull[0]
        elif k <= nonnull:
            assert not isnull.any()
        else:
            assert not isnull[:nonnull].any() and isnull[nonnull:].all()


# ---- ties and the row-order arm --------------------------------------------
@pytest.mark.parametrize("case", tnx.TIE_CASES, ids=lambda c: "-".join(
    str(x) for x in c))
def test_tie_arm(ctx, tabs, monkeypatch, case):
    geom, order, desc, nulls_first, k, kind = case
    t = tnx.matrix(geom)
    variants = VARIANTS[:1]     # the FoR table: cap floor = k + group_rows
    free, want = run(ctx, tabs, t, order, (), k, desc, nulls_first, variants)
    monkeypatch.setenv(HOOK, "1")
    hooked, want2 = run(ctx, tabs, t, order, (), k, desc, nulls_first,
                        variants, label="hook")
    st = hooked["for", "for"]
    assert st["tie_arm"] == 1
    assert st["cand_cap"] == k + t.group_rows
    assert st["candidates"] <= st["cand_cap"]
    # identical results with and without the hook: both equal one reference
    assert all((a == b).all() for a, b in zip(want[:3], want2[:3]))
    if kind == "ties":
        assert free["for", "for"]["tie_arm"] == 0
        assert free["for", "for"]["cand_cap"] == 1 << 20
        if order != "c7":       # 6 digits of an i64 code, all needed
            assert st["hist_passes"] == 6
    if order == "c7":           # ordered purely by row
        assert (want[0] == np.arange(k, dtype=np.uint64)).all()


def test_tie_arm_on_every_variant(ctx, tabs, monkeypatch):
    """the hooked c7 / NULLS FIRST queries on the raw paths too (the raw
    table tiles at 65536 rows, so its floor is k + 65536)"""
    monkeypatch.setenv(HOOK, "1")
    t = tnx.matrix("chunk")
    stats, _ = run(ctx, tabs, t, "c7", (), 100, label="hook")
    assert all(st["tie_arm"] == 1 for st in stats.values())
    stats, _ = run(ctx, tabs, t, "fx", (), 100, True, True, label="hook")
    assert all(st["tie_arm"] == 1 for st in stats.values())
    stats, _ = run(ctx, tabs, t, "m", (M2_BAND,), 70, False, False,
                   label="hook")


# ---- refinement -------------------------------------------------------------
@geoms
def test_refinement_runs_several_passes(ctx, tabs, monkeypatch, geom):
    t = tnx.matrix(geom)
    free, want = run(ctx, tabs, t, "key", (), 1000, desc=True)
    monkeypatch.setenv(HOOK, "1")
    hooked, want2 = run(ctx, tabs, t, "key", (), 1000, desc=True,
                        label="hook")
    for (kind, _), st in hooked.items():
        # the raw table tiles at 65536 rows: odd_t33 fits its floor whole
        tiling = t.group_rows if kind == "for" else 65536
        assert st["cand_cap"] == 1000 + tiling
        if t.rows > st["cand_cap"]:
            assert st["hist_passes"] > 1
    assert hooked["for", "for"]["hist_passes"] > 1
    assert all((a == b).all() for a, b in zip(want[:3], want2[:3]))
    assert all(st["hist_passes"] == 1 for st in free.values())


# ---- fx -----------------------------------------------------------------------
@geoms
def test_fx_total_order(ctx, tabs, geom):
    t = tnx.matrix(geom)
    bits, valid = t.bits("fx"), t.valid("fx")
    nan_rows = np.flatnonzero(((bits & 0x7FFFFFFF) > 0x7F800000) & valid)
    k = len(nan_rows) + 5
    # DESC starts with every NaN, by row, canonical; then +inf
    _, (rows, vals, isnull, _) = run(ctx, tabs, t, "fx", (), k, desc=True)
    assert (rows[:len(nan_rows)] == nan_rows).all()
    assert (vals[:len(nan_rows)] == amx.CANON_NAN).all()
    assert (vals[len(nan_rows):] == amx.POS_INF).all()
    # ASC starts with -inf
    _, (rows, vals, _, _) = run(ctx, tabs, t, "fx", (), 5, desc=False)
    assert (vals == amx.NEG_INF).all()
    # -0.0 before +0.0 ascending, after it descending; each by row
    zeros = (("fx", cmx.BETWEEN, -0.0, 0.0),)
    nz = int(((bits == 0x80000000) & valid).sum())
    pz = int(((bits == 0) & valid).sum())
    assert nz and pz
    _, (rows, vals, _, passed) = run(ctx, tabs, t, "fx", zeros, nz + pz,
                                     desc=False)
    assert passed == nz + pz
    assert (vals[:nz] == 0x80000000).all() and (vals[nz:] == 0).all()
    _, (rows, vals, _, _) = run(ctx, tabs, t, "fx", zeros, nz + pz,
                                desc=True)
    assert (vals[:pz] == 0).all() and (vals[pz:] == 0x80000000).all()


# ---- the order column's zonemap ---------------------------------------------
@geoms
def test_order_zonemap_skip(ctx, tabs, geom):
    t = tnx.matrix(geom)
    stats, _ = run(ctx, tabs, t, "m", (), 10, desc=True)
    assert stats["for", "for"]["rowgroups_skipped"] > 0
    assert stats["for", "raw"]["rowgroups_skipped"] == 0
    stats, _ = run(ctx, tabs, t, "m", (), 10, desc=False)
    assert stats["for", "for"]["rowgroups_skipped"] > 0
    # a NULL-class pass does not skip on it: NULLS FIRST needs NULL rows of
    # every row group, whatever range the group stores
    stats, _ = run(ctx, tabs, t, "m", (), 10, desc=True, nulls_first=True)


# ---- stats and determinism ---------------------------------------------------
@geoms
def test_same_call_twice_is_identical(ctx, tabs, monkeypatch, geom):
    t = tnx.matrix(geom)
    tab = tabs[geom, "for"]
    for hook in (None, "1"):
        if hook:
            monkeypatch.setenv(HOOK, hook)
        for order, desc, nf in (("m", True, False), ("fx", True, True),
                                ("c7", False, False)):
            a = ctx.scan_topn(tab, col_of(order, "for"), 777, [], desc=desc,
                              nulls_first=nf, stats=True)
            b = ctx.scan_topn(tab, col_of(order, "for"), 777, [], desc=desc,
                              nulls_first=nf, stats=True)
            for x, y in zip(a[:3], b[:3]):
                assert x.tobytes() == y.tobytes()
            assert a[3:] == b[3:]
            assert a[4]["candidates"] <= a[4]["cand_cap"]


# ---- errors -------------------------------------------------------------------
def raw_topn(ctx, tab, order_col, flags, k, preds, npreds=None):
    """the C entry with sentinel-filled outputs: (rc, outputs untouched)"""
    cap = 16
    rows = np.full(cap, 0xA5A5A5A5A5A5A5A5, dtype=np.uint64)
    nulls = np.full(cap, 0xA5, dtype=np.uint8)
    out = (ctx._AggResult * cap)()
    for i in range(cap):
        out[i].i64, out[i].f64 = -77, -77.5
    n, passed = C.c_uint64(12345), C.c_uint64(54321)
    st = ctx._TopnStats(9, 9, 9, 9, 9)
    rc = ctx._lib.sdb_gpu_scan_topn(
        ctx._ctx, tab, C.c_uint32(order_col), C.c_uint32(flags),
        C.c_uint32(k), ctx._pred_specs(preds),
        C.c_uint32(len(preds) if npreds is None else npreds),
        rows.ctypes.data_as(C.POINTER(C.c_uint64)), out,
        nulls.ctypes.data_as(C.POINTER(C.c_uint8)), C.byref(n),
        C.byref(passed), C.byref(st))
    untouched = ((rows == 0xA5A5A5A5A5A5A5A5).all() and
                 (nulls == 0xA5).all() and
                 all(out[i].i64 == -77 and out[i].f64 == -77.5
                     for i in range(cap)) and
                 n.value == 12345 and passed.value == 54321 and
                 (st.hist_passes, st.tie_arm, st.candidates, st.cand_cap,
                  st.rowgroups_skipped) == (9, 9, 9, 9, 9))
    return rc, untouched


ERROR_CASES = {
    "k_zero": dict(k=0),
    "k_above_max": dict(k=tnx.MAX_K + 1),
    "order_col_out_of_range": dict(order_col=NCOLS),
    "unknown_flag": dict(flags=4),
    "unknown_flag_high": dict(flags=1 | (1 << 31)),
    "pred_col_out_of_range": dict(preds=[(NCOLS, cmx.GE, 0, 0)]),
    "pred_op_none": dict(preds=[(COL["m2"], 0, 0, 0)]),
    "pred_op_prefix": dict(preds=[(COL["m2"], 8, 0, 0)]),
    "pred_op_unknown": dict(preds=[(COL["m2"], 9, 0, 0)]),
    "strmask_slot_out_of_range": dict(preds=[(4, STRMASK, 0, 0)]),
    "strmask_without_mask": dict(preds=[(1, STRMASK, 0, 0)]),
    "five_preds": dict(preds=[(COL["m2"], cmx.GE, 0, 0)] * 5),
}


@pytest.mark.parametrize("case", sorted(ERROR_CASES))
def test_errors_leave_outputs_untouched(ctx, tabs, case):
    args = dict(order_col=COL["m_for"], flags=0, k=10, preds=[])
    args.update(ERROR_CASES[case])
    for kind in CODECS:
        rc, untouched = raw_topn(ctx, tabs["odd_t33", kind], **args)
        assert rc == -1, case
        assert untouched, case
    # and the wrapper raises
    if "flags" not in ERROR_CASES[case]:
        with pytest.raises(RuntimeError, match=ERR_INVALID):
            ctx.scan_topn(tabs["odd_t33", "for"], args["order_col"],
                          args["k"], args["preds"])
    else:
        with pytest.raises(RuntimeError, match=ERR_INVALID):
            ctx.scan_topn(tabs["odd_t33", "for"], args["order_col"],
                          args["k"], args["preds"], flags=args["flags"])


def test_valid_call_after_errors(ctx, tabs):
    rc, untouched = raw_topn(ctx, tabs["odd_t33", "for"], COL["m_for"], 3,
                             10, [])
    assert rc == 0 and not untouched


def test_empty_table(ctx):
    tab = ctx.load_table([np.zeros(0, dtype=np.int64),
                          np.zeros(0, dtype=np.float32)])
    for col in (0, 1):
        rows, vals, isnull, passed, st = ctx.scan_topn(tab, col, 5, [],
                                                       stats=True)
        assert len(rows) == len(vals) == len(isnull) == 0 and passed == 0
        assert st["hist_passes"] == 0
    ctx.free_table(tab)


# ---- gather ---------------------------------------------------------------------
@geoms
def test_gather_rows_of_a_topn(ctx, tabs, geom):
    t = tnx.matrix(geom)
    for kind, codec in VARIANTS:
        tab = tabs[geom, kind]
        rows, vals, isnull, _ = ctx.scan_topn(
            tab, col_of("m", codec), 2000, [], desc=True, nulls_first=True)
        r = rows.astype(np.int64)
        gv, gn = ctx.gather(tab, col_of("m", codec), rows)
        assert gv.dtype == np.int64 and gn.dtype == np.bool_
        assert (gv == vals).all() and (gn == isnull).all()
        # the rest of the SELECT list: another i64 column, an f32 one
        gv, gn = ctx.gather(tab, COL["m2"], rows)
        assert (gv == t.mx.m2.vals[r]).all() and not gn.any()
        gv, gn = ctx.gather(tab, COL["fx"], rows)
        assert gv.dtype == np.float32
        want = t.ref("fx", (), 1)[1].dtype  # uint32 bit patterns
        assert want == np.uint32
        wb = t.bits("fx")[r].copy()
        wb[(wb & 0x7FFFFFFF) > 0x7F800000] = amx.CANON_NAN
        wb[~t.valid("fx")[r]] = 0
        assert (gn == ~t.valid("fx")[r]).all()
        assert (gv.view(np.uint32) == wb).all()
        assert (gv.astype(np.float64).view(np.uint64) ==
                f64_bits_of_f32_bits(wb)).all()


@geoms
def test_gather_row_group_edges(ctx, tabs, geom):
    """first and last row of every row group of `m`: FoR widths 0..32 with
    both int64 extremes as bases, and the tail group"""
    t = tnx.matrix(geom)
    edges = np.array([r for r0, r1 in t.mx.bounds for r in (r0, r1 - 1)],
                     dtype=np.uint64)
    assert sorted(set(t.mx.m.widths[:33])) == list(range(33))
    e = edges.astype(np.int64)
    for kind, codec in VARIANTS:
        tab = tabs[geom, kind]
        gv, gn = ctx.gather(tab, col_of("m", codec), edges)
        valid = t.valid("m")[e]
        assert (gn == ~valid).all()
        assert (gv == np.where(valid, t.vals["m"][e], 0)).all()
        gv, gn = ctx.gather(tab, col_of("keyp", codec), edges[::-1])
        valid = t.valid("keyp")[e[::-1]]
        assert (gn == ~valid).all()
        assert (gv == np.where(valid, t.vals["key"][e[::-1]], 0)).all()
        # unplaned columns: no NULLs; a repeated row is fine
        twice = np.concatenate([edges, edges])
        gv, gn = ctx.gather(tab, col_of("key", codec), twice)
        assert not gn.any()
        assert (gv == t.vals["key"][twice.astype(np.int64)]).all()
    vals = t.vals["m"][e]
    assert (vals == tnx.I64_MAX).any() and (vals == tnx.I64_MIN).any()


def test_gather_empty_and_out_of_range(ctx, tabs):
    t = tnx.matrix("odd_t33")
    for kind in CODECS:
        tab = tabs["odd_t33", kind]
        gv, gn = ctx.gather(tab, COL["m_for"], np.zeros(0, dtype=np.uint64))
        assert len(gv) == 0 and len(gn) == 0
        gv, gn = ctx.gather(tab, COL["f"], [t.rows - 1])
        assert gv.view(np.uint32)[0] == t.bits("f")[t.rows - 1]
        for bad in ([t.rows], [0, 1, t.rows + 5], [2 ** 63]):
            with pytest.raises(RuntimeError, match=ERR_INVALID):
                ctx.gather(tab, COL["m_for"], bad)
        with pytest.raises(RuntimeError, match=ERR_INVALID):
            ctx.gather(tab, NCOLS, [0])
