"""GROUP BY several nullable key columns (GpuContext.scan_agg_hash_multi)
against the composite-group-key matrix (tests/multikey_matrix.py;
tests/test_multikey_matrix.py proves its reference, its tuple counts and the
collision facts of the restated hash on the CPU). One pytest case per
(geometry, arm). Every comparison is exact: integers equal, f64 as bit
patterns (SUM_F64 runs over `f`, whose sums are exact in any order).

The tables are those of tests/test_gpu_nullkey_matrix.py: per geometry a FoR
table and an all-raw one, whose key columns are the POISONED arrays with their
planes attached — a NULL row stores -1, an int64 extreme, a value no valid row
holds or a live key, so a kernel that hashed or witnessed a NULL position's
stored value returns phantom tuples here, or fails its own proof. Each case
runs over the FoR columns of the FoR table, the raw columns of the FoR table
and the raw table; the raw table tiles at 65536 rows, so odd_t33 is a single
row group there and one workgroup meets every tuple of a query.
"""

import numpy as np
import pytest

import agg_matrix as amx
import col_matrix as cmx
import multikey_matrix as mkx
import nullkey_matrix as nkx
import serenedb_amd as sa

pytestmark = pytest.mark.gpu

COL = {"key_raw": 0, "key_for": 1, "m": 2, "m2": 3, "f": 4, "kmod_raw": 5,
       "kmod_for": 6, "fx": 7, "ksparse": 8, "keyclean_raw": 9,
       "keyclean_for": 10}
CODECS = {"for": ["raw", "for", "for", "for", "raw", "raw", "for", "raw",
                  "raw", "raw", "for"],
          "raw": ["raw"] * 11}
KEY_PLANES = {"key_raw": "key", "key_for": "key", "kmod_raw": "kmod",
              "kmod_for": "kmod", "ksparse": "ksparse"}
VARIANTS = (("for", "for"), ("for", "raw"), ("raw", "raw"))  # table, codec
STR_SLOT = 0
STRMASK = 7
ERR_INVALID, ERR_OOM, ERR_COLLISION = "rc=-1$", "rc=-4$", "rc=-6$"
HOOK = "SDB_MK_HASH_BITS"


@pytest.fixture(scope="module")
def ctx():
    c = sa.GpuContext(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def tabs(ctx):
    out = {}
    for name in mkx.GEOMS:
        nk = nkx.matrix(name)
        mx, am = nk.mx, nk.am
        arrays = [nk.poisoned["key", "raw"], nk.poisoned["key", "for"],
                  mx.m.vals, mx.m2.vals, mx.f, nk.poisoned["kmod", "raw"],
                  nk.poisoned["kmod", "for"], am.fx,
                  nk.poisoned["ksparse", "raw"], mx.key, mx.key]
        offsets, blob = sa.encode_col_str_raw(am.kmod_strings()[1])
        for kind, codecs in CODECS.items():
            tab = ctx.load_table(arrays, codecs, group_rows=mx.group_rows)
            for col, plane in KEY_PLANES.items():
                ctx.attach_validity(tab, COL[col], nk.validity_words(plane))
            ctx.attach_strcol(tab, STR_SLOT, offsets, blob)
            out[name, kind] = tab
    yield out
    for tab in out.values():
        ctx.free_table(tab)


@pytest.fixture(autouse=True)
def no_hook(monkeypatch):
    monkeypatch.delenv(HOOK, raising=False)


geoms = pytest.mark.parametrize("geom", mkx.GEOMS)


def col_of(name, codec):
    if name in ("key", "kmod"):
        return COL[f"{name}_{codec}"]
    return COL[name]


def gpu_specs(ctx, tab, codec, preds, aggs):
    gp = []
    for c, op, lo, hi in preds:
        if c == "kstr":
            ctx.strpred_mask(tab, STR_SLOT, "prefix", lo)
            gp.append((STR_SLOT, STRMASK, 0, 0))
        else:
            gp.append((col_of(c, codec), op, lo, hi))
    return gp, [(col_of(c, codec) if c else 0, op) for c, op in aggs]


def assert_exact(got, want, what, as_bits=False):
    g = np.ascontiguousarray(got)
    w = np.ascontiguousarray(want)
    assert g.shape == w.shape, f"{what}: shape {g.shape} want {w.shape}"
    if as_bits:
        g, w = g.view(np.uint64), w.view(np.uint64)
    bad = np.argwhere(g != w)
    if len(bad):
        k, q = (int(v) for v in bad[0])
        raise AssertionError(
            f"{what}: {len(bad)} slots differ; first row {k} column {q} "
            f"got {got[k, q]!r} want {want[k, q]!r}")


def assert_ordered(keys, keynull, what):
    """the order rule on the returned arrays: tuples strictly ascending,
    column by column as signed int64, NULL last in its column; 0 stored in
    a NULL position"""
    assert not keys[keynull].any(), what + ": a NULL position is not 0"
    tuples = [tuple((n, k) for k, n in zip(kr, nr))
              for kr, nr in zip(keys.tolist(), keynull.tolist())]
    for a, b in zip(tuples, tuples[1:]):
        assert a < b, f"{what}: {a} before {b}"


def run(ctx, tabs, mk, case, label, variants=VARIANTS):
    """one query on every table / codec == the reference, exactly. Returns
    the reference."""
    group_cols, max_groups, preds, aggs, nulls = case
    want = mk.ref(tuple(group_cols), tuple(preds), tuple(aggs), tuple(nulls))
    rk, rn, ri, rf, rpassed = want
    for kind, codec in variants:
        tab = tabs[mk.name, kind]
        gp, ga = gpu_specs(ctx, tab, codec, preds, aggs)
        gcols = [col_of(g, codec) for g in group_cols]
        what = f"{mk.name} {label} {kind} table, {codec} keys {group_cols}"
        keys, keynull, i64, f64, passed = ctx.scan_agg_hash_multi(
            tab, gcols, max_groups, gp, ga)
        assert passed == rpassed, what + ": rows_passed"
        assert len(keys) == len(rk), (
            f"{what}: {len(keys)} groups, want {len(rk)}")
        assert keys.shape == keynull.shape == (len(rk), len(group_cols))
        assert keynull.dtype == np.bool_ and keys.dtype == np.int64
        assert_exact(keynull, rn, what + " keynull")
        assert_exact(keys, rk, what + " keys")
        assert_exact(i64, ri, what + " i64")
        assert_exact(f64, rf, what + " f64", as_bits=True)
        assert_ordered(keys, keynull, what)
    return want


# ---- 1. one key: the existing entry --------------------------------------
@geoms
def test_one_key_agrees_with_the_nullable_key_entry(ctx, tabs, geom):
    """nkeys == 1 returns scan_agg_hash_nullkey's key groups with its NULL
    group appended last, and both equal the reference"""
    mk = mkx.matrix(geom)
    for group in nkx.KEYCOLS:
        case = ((group,), 2048, mkx.ALL, mkx.AGGS_ALL, ())
        rk, rn, ri, rf, rpassed = run(ctx, tabs, mk, case, "one key")
        assert rn[-1, 0] and not rn[:-1].any()
        for kind, codec in VARIANTS:
            tab = tabs[geom, kind]
            gp, ga = gpu_specs(ctx, tab, codec, mkx.ALL, mkx.AGGS_ALL)
            gcol = col_of(group, codec)
            okeys, oi, of, opassed, ni, nf, null_rows = \
                ctx.scan_agg_hash_nullkey(tab, gcol, 2048, gp, ga)
            keys, keynull, i64, f64, passed = ctx.scan_agg_hash_multi(
                tab, [gcol], 2048, gp, ga)
            assert null_rows > 0 and passed == opassed == rpassed
            what = f"{geom} {group}_{codec} vs nullkey entry"
            np.testing.assert_array_equal(
                keys[:, 0], np.append(okeys, 0), err_msg=what)
            np.testing.assert_array_equal(
                keynull[:, 0], np.arange(len(keys)) == len(okeys))
            assert_exact(i64, np.vstack([oi, ni[None]]), what + " i64")
            assert_exact(f64, np.vstack([of, nf[None]]), what + " f64",
                         as_bits=True)
            assert i64[-1, 0] == null_rows


# ---- 2. the LDS table -----------------------------------------------------
@geoms
def test_lds_arm(ctx, tabs, geom):
    """(kmod, ksparse), max_groups 256, all eight aggregates: 182 tuples in
    four null-ness classes, staged in a 1024-slot LDS table"""
    mk = mkx.matrix(geom)
    rk, rn, ri, _, _ = run(ctx, tabs, mk, mkx.ARMS["lds"], "lds")
    assert len(rk) == 182
    assert {tuple(r) for r in rn.tolist()} == {
        (False, False), (False, True), (True, False), (True, True)}
    assert (rk[~rn[:, 1], 1] == -1).any()           # key -1 live in ksparse
    assert nkx.NULL_KMOD not in rk[~rn[:, 0], 0]    # never a valid kmod
    assert rn[-1].all() and ri[-1, 0] > 0           # (NULL, NULL) is last


# ---- 3. the global table --------------------------------------------------
@pytest.mark.parametrize("arm", ("global_2", "global_3", "global_4_repeat"))
@geoms
def test_global_arm(ctx, tabs, geom, arm):
    """max_groups = 65536 is past twice any LDS table: every row upserts
    into the global table. FoR `key` and raw `key`; the 4-key case repeats
    a column and has the tuples of the 3-key one."""
    mk = mkx.matrix(geom)
    rk, rn, _, _, _ = run(ctx, tabs, mk, mkx.ARMS[arm], arm)
    groups = mkx.ARMS[arm][0]
    assert len(rk) == mkx.DISTINCT[tuple(dict.fromkeys(groups))][geom]
    if arm == "global_4_repeat":
        np.testing.assert_array_equal(rk[:, 0], rk[:, 2])
        np.testing.assert_array_equal(rn[:, 0], rn[:, 2])


# ---- 4. LDS staging at its limit ------------------------------------------
@geoms
def test_lds_spill_arm(ctx, tabs, geom):
    """naggs = 1, nkeys = 2: 2048 LDS slots, staging still on at max_groups
    = 4096, and more than 2048 tuples pass (test_lds_spill_case). The LDS
    tables flush into a global table that also takes rows directly; on the
    raw table of odd_t33, one row group and so one workgroup, the tuples
    outnumber the slots and rows must fall through the probe bound."""
    mk = mkx.matrix(geom)
    rk, _, ri, _, rpassed = run(ctx, tabs, mk, mkx.SPILL, "lds_spill")
    assert 2048 < len(rk) <= 4096 and int(ri[:, 0].sum()) == rpassed
    # one more tuple allowed: LDS staging is off, same answer
    group_cols, max_groups, preds, aggs, nulls = mkx.SPILL
    run(ctx, tabs, mk, (group_cols, max_groups + 1, preds, aggs, nulls),
        "lds_spill, staging off")


# ---- 5. predicates --------------------------------------------------------
@pytest.mark.parametrize("name", ("between_key", "isnull_notnull",
                                  "notnull_isnull", "m_plane", "strmask",
                                  "nothing"))
@geoms
def test_predicates(ctx, tabs, geom, name):
    mk = mkx.matrix(geom)
    nk = mk.nk
    case = mkx.pred_cases(geom)[name]
    planes = case[4]
    try:
        for kind in CODECS:
            for c in planes:
                ctx.attach_validity(tabs[geom, kind], COL[c],
                                    nk.validity_words(c))
        rk, rn, ri, _, rpassed = run(ctx, tabs, mk, case, name)
    finally:
        for kind in CODECS:
            for c in planes:
                ctx.attach_validity(tabs[geom, kind], COL[c], None)
    if name == "between_key":       # the compare dropped key's NULL rows
        assert not rn[:, 0].any() and rn[:, 1].any()
        assert rk[:, 0].min() >= 40 and rk[:, 0].max() <= 400
    elif name == "isnull_notnull":  # (NULL, ksparse) tuples only
        assert rn[:, 0].all() and not rn[:, 1].any() and len(rk) == 61
    elif name == "notnull_isnull":
        assert rn[:, 1].all() and not rn[:, 0].any() and len(rk) > 0
    elif name == "m_plane":         # NULL m rows fail the compare on m
        assert 0 < rpassed < nk.rows
        assert np.array_equal(ri[:, 0], ri[:, 1])   # COUNT(*) == COUNT(m)
    elif name == "strmask":         # kmod 10 .. 19, valid or NULL
        assert set(rk[~rn[:, 0], 0].tolist()) == set(range(10, 20))
        assert 0 < rpassed < nk.rows
    else:
        assert len(rk) == 0 and rpassed == 0


# ---- 6. aggregates over the key columns -----------------------------------
@geoms
def test_aggregates_over_key_columns(ctx, tabs, geom):
    """SUM / COUNT_COL / MIN / MAX over a key column skip its NULL rows: in
    a group where that key is NULL they return 0, 0 and the identities, in
    every other group the key itself"""
    mk = mkx.matrix(geom)
    groups = ("kmod", "ksparse")
    for j, g in enumerate(groups):
        case = (groups, 256, mkx.ALL, mkx.aggs_on_key(g), ())
        rk, rn, ri, _, _ = run(ctx, tabs, mk, case, f"aggs on {g}")
        null = rn[:, j]
        assert null.any() and (~null).any() and (ri[:, 0] > 0).all()
        assert (ri[null, 1:] == [0, 0, cmx.I64_MAX, cmx.I64_MIN]).all()
        live = ~null
        assert np.array_equal(ri[live, 2], ri[live, 0])
        assert np.array_equal(ri[live, 3], rk[live, j])
        assert np.array_equal(ri[live, 4], rk[live, j])


# ---- 7. errors ------------------------------------------------------------
@geoms
def test_errors(ctx, tabs, geom):
    mk = mkx.matrix(geom)
    group_cols, max_groups, preds, aggs, nulls = mkx.ARMS["lds"]
    for kind, codec in VARIANTS:
        tab = tabs[geom, kind]
        gp, ga = gpu_specs(ctx, tab, codec, preds, aggs)
        good = [col_of(g, codec) for g in group_cols]
        with pytest.raises(RuntimeError, match=ERR_OOM):    # 182 tuples
            ctx.scan_agg_hash_multi(tab, good, 181, gp, ga)
        keys = ctx.scan_agg_hash_multi(tab, good, 182, gp, ga)[0]
        assert len(keys) == 182
        bad_lists = ([], good + good + good[:1],            # 0 and 5 keys
                     [good[0], COL["f"]], [COL["fx"]],      # an f32 column
                     [good[0], len(COL)], [1 << 20])        # out of range
        for bad in bad_lists:
            with pytest.raises(RuntimeError, match=ERR_INVALID):
                ctx.scan_agg_hash_multi(tab, bad, max_groups, gp, ga)
        # the existing bad aggregate / predicate cases, before launch
        for bad_gp, bad_ga in ((gp, [(COL["f"], amx.SUM_I64)]),
                               (gp, [(len(COL), amx.MIN_I64)]),
                               (gp, [(0, 99)]), (gp, []),
                               ([(len(COL), cmx.GE, 0, 0)], ga)):
            with pytest.raises(RuntimeError, match=ERR_INVALID):
                ctx.scan_agg_hash_multi(tab, good, max_groups, bad_gp,
                                        bad_ga)
    # and the table still answers
    run(ctx, tabs, mk, mkx.ARMS["lds"], "after the errors")


# ---- 8. the witness and the retry -----------------------------------------
@geoms
def test_hash_bits_hook(ctx, tabs, geom, monkeypatch):
    """SDB_MK_HASH_BITS cuts the hash so that tuples share a slot
    (test_hook_facts proves which widths collide under which seed). 13
    bits: seed 0 merges two of the 182 tuples, the witness words show it,
    and the scan under seed 1 — which does not collide — is the one that
    returns, exact. 12 bits and 2 bits: every seed collides, and the call
    ends in SDB_ERR_COLLISION, never in an answer. 17 bits: no collision."""
    mk = mkx.matrix(geom)
    case = mkx.ARMS["lds"]
    group_cols, max_groups, preds, aggs, nulls = case
    for bits, exact in (("13", True), ("12", False), ("2", False),
                        ("17", True), ("64", True)):
        monkeypatch.setenv(HOOK, bits)
        if exact:
            assert len(run(ctx, tabs, mk, case, f"{bits} bits")[0]) == 182
        else:
            for kind, codec in VARIANTS:
                tab = tabs[geom, kind]
                gp, ga = gpu_specs(ctx, tab, codec, preds, aggs)
                with pytest.raises(RuntimeError, match=ERR_COLLISION):
                    ctx.scan_agg_hash_multi(
                        tab, [col_of(g, codec) for g in group_cols],
                        max_groups, gp, ga)
        monkeypatch.delenv(HOOK)
    run(ctx, tabs, mk, case, "hook removed")
