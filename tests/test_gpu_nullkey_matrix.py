"""GROUP BY a nullable key on every GPU scan path, against the NULL-group-key
matrix (tests/nullkey_matrix.py; tests/test_nullkey_matrix.py proves its
planes, poison and references on the CPU). One pytest case per (geometry,
path), the six paths of tests/test_gpu_agg_matrix.py with the same
environment switches. Every comparison is exact: integers equal, f64 as bit
patterns (SUM_F64 runs over `f`, whose sums are exact in any order).

The key columns of the tables are the POISONED arrays: a NULL row stores a
value outside [0, ngroups), an int64 extreme, -1 or a live key, so a kernel
that indexed, hashed or summed a NULL row's key gives a wrong slot, a
phantom group or a wrong sum here. A hash result is compared as returned:
its key groups against the reference rows of the keys it names, its NULL
group always, nothing filled in.
"""

import numpy as np
import pytest

import agg_matrix as amx
import col_matrix as cmx
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
STR_SLOT = 0
STRMASK = 7
ENV_SWITCHES = ("SDB_SCAN_NOSTAGE", "SDB_SCAN_NOSHAPE", "SDB_SCAN_NOF32STAGE")
PATHS = {   # name: (environment, entry, table, max_groups)
    "raw": ({}, "dense", "raw", None),
    "staged": ({}, "dense", "for", None),
    "nof32stage": ({"SDB_SCAN_NOF32STAGE": "1"}, "dense", "for", None),
    "nostage": ({"SDB_SCAN_NOSTAGE": "1"}, "dense", "for", None),
    "hash_lds": ({}, "hash", "for", 2048),
    "hash_global": ({}, "hash", "for", 1 << 14),
}
HASH_PATHS = ("hash_lds", "hash_global")

C, CC = amx.COUNT, amx.COUNT_COL
AGGS_ALL = ((None, C), ("m", CC), ("m", amx.SUM_I64), ("f", amx.SUM_F64),
            ("m", amx.MIN_I64), ("m2", amx.MAX_I64), ("fx", amx.MIN_F32),
            ("fx", amx.MAX_F32))
AGGS_OLD3 = ((None, C), ("m", amx.SUM_I64), ("f", amx.SUM_F64))


def aggs_on_key(group):
    return ((None, C), (group, amx.SUM_I64), (group, CC),
            (group, amx.MIN_I64), (group, amx.MAX_I64))


@pytest.fixture(scope="module")
def ctx():
    c = sa.GpuContext(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def tabs(ctx):
    """per geometry a FoR table and an all-raw one: poisoned key columns
    with their planes attached, a clean `key` without one, and kmod as a
    string slot"""
    out = {}
    for name in nkx.GEOMS:
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


@pytest.fixture
def path(request, monkeypatch):
    for k in ENV_SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in PATHS[request.param][0].items():
        monkeypatch.setenv(k, v)
    return request.param


def cases(paths):
    return pytest.mark.parametrize(
        "geom,path", [(g, p) for g in nkx.GEOMS for p in paths],
        indirect=["path"], ids=lambda v: v)


def codecs_of(path):
    return ("raw",) if PATHS[path][2] == "raw" else ("raw", "for")


def group_col(group, codec):
    return COL["ksparse" if group == "ksparse" else f"{group}_{codec}"]


def gpu_specs(ctx, tab, group, codec, preds, aggs):
    """column names -> indices; the group's name as a predicate or aggregate
    column means the group column in the codec under test. A ("kstr",
    PREFIX, literal, 0) predicate evaluates its string mask now and becomes
    the STRMASK predicate that consumes it."""
    def col(c):
        return group_col(c, codec) if c in nkx.KEYCOLS else COL[c]
    gp = []
    for c, op, lo, hi in preds:
        if c == "kstr":
            ctx.strpred_mask(tab, STR_SLOT, "prefix", lo)
            gp.append((STR_SLOT, STRMASK, 0, 0))
        else:
            gp.append((col(c), op, lo, hi))
    return gp, [(col(c) if c else 0, op) for c, op in aggs]


def assert_exact(got, want, what, aggs, as_bits=False):
    g = np.ascontiguousarray(got)
    w = np.ascontiguousarray(want)
    assert g.shape == w.shape, f"{what}: shape {g.shape} want {w.shape}"
    if as_bits:
        g, w = g.view(np.uint64), w.view(np.uint64)
    bad = np.argwhere(g != w)
    if len(bad):
        k, q = (int(v) for v in bad[0])
        raise AssertionError(
            f"{what}: {len(bad)} slots differ; first group row {k} agg {q} "
            f"{aggs[q]} got {got[k, q]!r} want {want[k, q]!r}")


def check(ctx, tabs, nk, path, group, codec, preds, aggs, nulls=(),
          label=""):
    """one nullable-key query on the active path == the numpy reference,
    exactly. Returns (i64 [ng+1, naggs], f64, rows_passed, null_rows,
    present [ng+1]) of the reference, which the result equals."""
    preds, aggs, nulls = tuple(preds), tuple(aggs), tuple(nulls)
    _, entry, kind, max_groups = PATHS[path]
    tab = tabs[nk.name, kind]
    gp, ga = gpu_specs(ctx, tab, group, codec, preds, aggs)
    gcol = group_col(group, codec)
    what = f"{nk.name} {path} {label} group={group}_{codec} preds={preds}"
    if entry == "hash":
        rk, ri, rf, rpassed, rni, rnf, rnull = nk.ref_hash(
            group, preds, aggs, nulls)
        keys, hi, hf, passed, ni, nf, null_rows = ctx.scan_agg_hash_nullkey(
            tab, gcol, max_groups, gp, ga)
        np.testing.assert_array_equal(keys, rk, err_msg=what + ": keys")
        assert_exact(hi, ri, what + " i64", aggs)
        assert_exact(hf, rf, what + " f64", aggs, as_bits=True)
        assert_exact(ni[None], rni[None], what + " NULL group i64", aggs)
        assert_exact(nf[None], rnf[None], what + " NULL group f64", aggs,
                     as_bits=True)
        assert passed == rpassed, what + ": rows_passed"
        assert null_rows == rnull, what + ": null_rows"
        if group == "ksparse":
            return None
    ri, rf, rpassed, rnull, present = nk.ref_dense(group, preds, aggs, nulls)
    if entry == "dense":
        ng = nk.groups[group][1]
        i64, f64, passed, null_rows = ctx.scan_agg_nullkey(tab, gcol, ng,
                                                           gp, ga)
        assert passed == rpassed, what + ": rows_passed"
        assert null_rows == rnull, what + ": null_rows"
        assert_exact(i64, ri, what + " i64", aggs)
        assert_exact(f64, rf, what + " f64", aggs, as_bits=True)
    return ri, rf, rpassed, rnull, present


@cases(PATHS)
def test_all_aggregates(ctx, tabs, geom, path):
    """all eight ops at once, by `key` and by `kmod` with poisoned keys: every
    row passing, a predicate that splits a row group, two staged predicates;
    then once more with planes on m and fx, so that a NULL-key row can hold
    a NULL value too"""
    nk = nkx.matrix(geom)
    tab = tabs[geom, PATHS[path][2]]
    for group in ("key", "kmod"):
        lists = nkx.pred_lists(nk, group)
        for codec in codecs_of(path):
            for name in ("all", "split", "two_staged"):
                preds, nulls, _ = lists[name]
                _, _, _, rnull, present = check(
                    ctx, tabs, nk, path, group, codec, preds, AGGS_ALL,
                    nulls, label=name)
                assert rnull > 0 and present[-1]
    try:
        ctx.attach_validity(tab, COL["m"], nk.validity_words("m"))
        ctx.attach_validity(tab, COL["fx"], nk.validity_words("fx"))
        for group in ("key", "kmod"):
            lists = nkx.pred_lists(nk, group)
            for codec in codecs_of(path):
                for name in ("all_nulls", "split_nulls", "two_staged_nulls"):
                    preds, nulls, _ = lists[name]
                    ri, _, _, rnull, _ = check(
                        ctx, tabs, nk, path, group, codec, preds, AGGS_ALL,
                        nulls, label=name)
                    # NULL-key rows with a NULL m: counted, not summed —
                    # unless a compare on m has dropped them already
                    assert 0 < ri[-1, 1] <= ri[-1, 0] == rnull
                    assert (ri[-1, 1] == rnull) == any(
                        p[0] == "m" for p in preds)
    finally:
        ctx.attach_validity(tab, COL["m"], None)
        ctx.attach_validity(tab, COL["fx"], None)


@cases(PATHS)
def test_old_three_op_shape(ctx, tabs, geom, path):
    """[COUNT, SUM_I64, SUM_F64] alone — the list the ASHAPE bodies serve
    without a key plane — gives the same answers under one"""
    nk = nkx.matrix(geom)
    for group in ("key", "kmod"):
        lists = nkx.pred_lists(nk, group)
        for codec in codecs_of(path):
            for name in ("all", "split"):
                preds, nulls, _ = lists[name]
                check(ctx, tabs, nk, path, group, codec, preds, AGGS_OLD3,
                      nulls, label="old3 " + name)
                # the reused-key-value source (agg_src 9) in the same shape
                check(ctx, tabs, nk, path, group, codec, preds,
                      ((None, C), (group, amx.SUM_I64), ("f", amx.SUM_F64)),
                      nulls, label="old3 sum(key) " + name)


@cases(PATHS)
def test_key_as_predicate_and_aggregate(ctx, tabs, geom, path):
    nk = nkx.matrix(geom)
    for group in ("key", "kmod"):
        ng = nk.groups[group][1]
        lists = nkx.pred_lists(nk, group)
        aggs = aggs_on_key(group)
        nvalid = int(nk.valid[group].sum())
        for codec in codecs_of(path):
            ri, _, passed, rnull, _ = check(
                ctx, tabs, nk, path, group, codec, lists["all"][0], aggs,
                label="aggs on key")
            assert passed == nk.rows and rnull == nk.rows - nvalid
            assert ri[ng].tolist() == [rnull, 0, 0, cmx.I64_MAX, cmx.I64_MIN]
            live = ri[:ng, 0] > 0
            assert np.array_equal(ri[:ng, 2], ri[:ng, 0])   # valid rows only
            assert np.array_equal(ri[:ng][live, 3], np.flatnonzero(live))
            assert np.array_equal(ri[:ng][live, 4], np.flatnonzero(live))
            ri, _, passed, rnull, _ = check(
                ctx, tabs, nk, path, group, codec, lists["key_ge_0"][0],
                aggs, label="key GE 0")
            assert rnull == 0 and passed == nvalid and ri[ng, 0] == 0
            ri, _, passed, rnull, _ = check(
                ctx, tabs, nk, path, group, codec, lists["key_isnull"][0],
                aggs, label="ISNULL(key)")
            assert passed == rnull == nk.rows - nvalid == ri[ng, 0]
            assert not ri[:ng, 0].any()
            _, _, passed, rnull, _ = check(
                ctx, tabs, nk, path, group, codec, lists["key_notnull"][0],
                aggs, label="NOTNULL(key)")
            assert rnull == 0 and passed == nvalid


@cases(HASH_PATHS)
def test_hash_isolation_of_poison(ctx, tabs, geom, path):
    """ksparse: keys from both ends of int64 with a live key -1, NULL rows
    that store -1, a live key or a key no valid row holds"""
    nk = nkx.matrix(geom)
    tab = tabs[geom, "for"]
    lists = nkx.pred_lists(nk, "ksparse")
    for name in ("all", "split"):
        preds, nulls, _ = lists[name]
        check(ctx, tabs, nk, path, "ksparse", "raw", preds, AGGS_ALL, nulls,
              label="ksparse " + name)
        rk, ri, rf, rpassed, rni, rnf, rnull = nk.ref_hash(
            "ksparse", preds, AGGS_ALL, nulls)
        assert -1 in rk and rnull > 0
        n = len(rk)
        gp, ga = gpu_specs(ctx, tab, "ksparse", "raw", preds, AGGS_ALL)
        # exactly as many slots as distinct valid passing keys: the NULL
        # group takes none and poison inserted no key
        keys, hi, hf, passed, ni, nf, null_rows = ctx.scan_agg_hash_nullkey(
            tab, COL["ksparse"], n, gp, ga)
        assert len(keys) == n and passed == rpassed and null_rows == rnull
        np.testing.assert_array_equal(keys, rk)
        assert_exact(hi, ri, "exact max_groups i64", AGGS_ALL)
        assert_exact(ni[None], rni[None], "exact max_groups NULL", AGGS_ALL)
        at = int(np.flatnonzero(keys == -1)[0])
        assert hi[at, 0] == ri[at, 0] > 0 and ni[0] == rnull
        dead = set(nk.poison_values["ksparse", "raw"]) - set(
            nkx.KSPARSE.tolist())
        assert dead and not dead & set(keys.tolist())


@cases(PATHS)
def test_range_proof(ctx, tabs, geom, path):
    nk = nkx.matrix(geom)
    _, entry, kind, max_groups = PATHS[path]
    tab = tabs[geom, kind]
    aggs = AGGS_ALL
    preds = (nkx.ALL_M,)
    for codec in codecs_of(path):
        for group in ("key", "kmod"):
            ng = nk.groups[group][1]
            gcol = group_col(group, codec)
            gp, ga = gpu_specs(ctx, tab, group, codec, preds, aggs)
            words = nk.validity_words(group)
            try:
                if entry == "dense":
                    # NULL rows hold out-of-range values: accepted
                    a = nk.poisoned[group, codec]
                    assert a.min() < 0 and a.max() >= ng
                    ctx.scan_agg_nullkey(tab, gcol, ng, gp, ga)
                    # the same column without its plane: every row binds
                    ctx.attach_validity(tab, gcol, None)
                    with pytest.raises(RuntimeError, match="rc=-1"):
                        ctx.scan_agg_nullkey(tab, gcol, ng, gp, ga)
                # an all-NULL key: no key group, the NULL group holds all
                ctx.attach_validity(
                    tab, gcol, nk.validity_words(
                        group, plane=np.zeros(nk.rows, bool)))
                ui, uf, upassed = nk.ref_ungrouped(preds, aggs)
                if entry == "dense":
                    i64, f64, passed, null_rows = ctx.scan_agg_nullkey(
                        tab, gcol, ng, gp, ga)
                    ei, ef, _, _, _ = nk.ref_dense(group, (
                        (group, cmx.ISNULL, 0, 0),), aggs, plane=False)
                    assert not ei[:, 0].any()       # every group empty
                    assert_exact(i64[:ng], ei[:ng], "all-NULL keys", aggs)
                    assert_exact(f64[:ng], ef[:ng], "all-NULL keys", aggs,
                                 as_bits=True)
                    ni, nf = i64[ng], f64[ng]
                else:
                    keys, _, _, passed, ni, nf, null_rows = \
                        ctx.scan_agg_hash_nullkey(tab, gcol, max_groups, gp,
                                                  ga)
                    assert len(keys) == 0
                assert passed == null_rows == upassed == nk.rows
                assert_exact(ni[None], ui[None], "all-NULL NULL group", aggs)
                assert_exact(nf[None], uf[None], "all-NULL NULL group", aggs,
                             as_bits=True)
            finally:
                ctx.attach_validity(tab, gcol, words)
            # the real plane is back and proved afresh
            check(ctx, tabs, nk, path, group, codec, preds, aggs,
                  label="plane re-attached")
    if entry != "dense":
        return
    # a second, small table: one VALID key equal to ngroups is refused before
    # launch; once that row is NULL the scan runs
    rows, ng = 1000, 8
    key = np.arange(rows, dtype=np.int64) % ng
    valid = np.arange(rows) % 5 != 0
    key[~valid] = -3
    bad = 501
    assert valid[bad]
    key[bad] = ng
    for codec in codecs_of(path):
        small = ctx.load_table([key], [codec], group_rows=128)
        try:
            def words(v):
                b = np.zeros((rows + 63) // 64 * 64, dtype=np.uint8)
                b[:rows] = v
                return np.packbits(b, bitorder="little").view(np.uint64)
            ctx.attach_validity(small, 0, words(valid))
            with pytest.raises(RuntimeError, match="rc=-1"):
                ctx.scan_agg_nullkey(small, 0, ng, [], [(0, C)])
            fixed = valid.copy()
            fixed[bad] = False
            ctx.attach_validity(small, 0, words(fixed))
            i64, _, passed, null_rows = ctx.scan_agg_nullkey(
                small, 0, ng, [], [(0, C)])
            assert passed == rows and null_rows == (~fixed).sum()
            want = np.bincount(np.where(fixed, key, ng), minlength=ng + 1)
            assert i64[:, 0].tolist() == want.tolist()
        finally:
            ctx.free_table(small)


@cases(PATHS)
def test_no_plane_attached(ctx, tabs, geom, path):
    """a key column without a plane: the new entries return the old entries'
    answers slot for slot and no NULL group; a key column with one is still
    refused by the old entries"""
    nk = nkx.matrix(geom)
    _, entry, kind, max_groups = PATHS[path]
    tab = tabs[geom, kind]
    ng = nk.mx.ngroups
    for codec in codecs_of(path):
        gcol = COL[f"keyclean_{codec}"]
        for aggs in (AGGS_ALL, AGGS_OLD3):
            for preds in ((nkx.ALL_M,), (nkx.split(nk, "m"),)):
                gp, ga = gpu_specs(ctx, tab, "key", codec, preds, aggs)
                ri, rf, rpassed, rnull, _ = nk.ref_dense(
                    "key", preds, aggs, plane=False)
                assert rnull == 0
                if entry == "dense":
                    oi, of, opassed = ctx.scan_agg(tab, gcol, ng, gp, ga)
                    i64, f64, passed, null_rows = ctx.scan_agg_nullkey(
                        tab, gcol, ng, gp, ga)
                    assert_exact(i64, ri, "no plane i64", aggs)
                    assert_exact(f64, rf, "no plane f64", aggs, as_bits=True)
                    ki, kf, ni, nf = i64[:ng], f64[:ng], i64[ng], f64[ng]
                else:
                    okeys, oi, of, opassed = ctx.scan_agg_hash(
                        tab, gcol, max_groups, gp, ga)
                    keys, ki, kf, passed, ni, nf, null_rows = \
                        ctx.scan_agg_hash_nullkey(tab, gcol, max_groups, gp,
                                                  ga)
                    np.testing.assert_array_equal(keys, okeys)
                    assert_exact(ki, ri[keys], "no plane i64", aggs)
                    assert_exact(ni[None], ri[ng:], "no plane NULL", aggs)
                    assert_exact(nf[None], rf[ng:], "no plane NULL", aggs,
                                 as_bits=True)
                assert_exact(ki, oi, "new vs old i64", aggs)
                assert_exact(kf, of, "new vs old f64", aggs, as_bits=True)
                assert passed == opassed == rpassed and null_rows == 0
        planed = COL[f"key_{codec}"]
        gp, ga = gpu_specs(ctx, tab, "key", codec, (), AGGS_OLD3)
        with pytest.raises(RuntimeError, match="rc=-1"):
            if entry == "dense":
                ctx.scan_agg(tab, planed, ng, gp, ga)
            else:
                ctx.scan_agg_hash(tab, planed, max_groups, gp, ga)


@cases(PATHS)
def test_strmask_with_a_nullable_key(ctx, tabs, geom, path):
    """a PREFIX mask over the kmod strings consumed as SDB_PRED_STRMASK: it
    rides the key column as its value column with the mask as its plane,
    while the key's own plane still decides nothing but the group"""
    nk = nkx.matrix(geom)
    for group in ("key", "kmod"):
        preds, nulls, _ = nkx.pred_lists(nk, group)["strmask"]
        for codec in codecs_of(path):
            ri, _, passed, rnull, present = check(
                ctx, tabs, nk, path, group, codec, preds, AGGS_ALL, nulls,
                label="strmask")
            assert 0 < rnull < passed < nk.rows
            if group == "kmod":     # k10 .. k19 only, and the NULL group
                assert set(np.flatnonzero(present)) == set(range(10, 20)) | {
                    amx.NKMOD}
    # the mask alone, no other predicate
    check(ctx, tabs, nk, path, "kmod", "raw", (nkx.STR_K1,), AGGS_OLD3,
          label="strmask alone")
