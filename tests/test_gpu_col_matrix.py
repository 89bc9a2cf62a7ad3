"""Every GPU scan path on the column-codec matrix (tests/col_matrix.py):
every FoR width 0..32 in every extraction role, bases at both ends of
int64, row-group tilings that are odd / no multiple of 32 or 64, zonemap
literals exactly at and one off each bound, NULLs across group boundaries,
the chunk-shrink loop up to the largest dynamic-LDS launch, and the hash
aggregate over FoR keys. One pytest case per (geometry, path) so a failure
names the path; the assertion message names the row groups (and so the
widths) behind the wrong slots.

Expected values are numpy over the raw arrays (tests/test_col_matrix.py
proves the references sound): counts, rows_passed and wrap-around SUM_I64
exact, SUM_F64 bit-equal (the f column is dyadic, so its f64 sums are exact
in any order).

Paths — five kernel bodies of sdb_scan.hip and their host-side arms:
  staged_shape        scan_agg_staged_kernel<1>, f32 agg column staged
  staged_generic      scan_agg_staged_kernel<0>, f32 agg column staged
  nof32stage_shape    <1> with SDB_SCAN_NOF32STAGE (f32 read from global)
  nof32stage_generic  <0> with SDB_SCAN_NOF32STAGE
  noshape             <0> on the 3-agg shape (SDB_SCAN_NOSHAPE)
  nostage_shape       scan_agg_kernel<0,1> (SDB_SCAN_NOSTAGE)
  nostage_generic     scan_agg_kernel<0,0> (SDB_SCAN_NOSTAGE)
  hash                scan_agg_hash_kernel, grouped by the dense key
"""

import numpy as np
import pytest

import col_matrix as cmx
import serenedb_amd as sa

pytestmark = pytest.mark.gpu

GEOMS = tuple(cmx.GEOMETRIES)
COL = {"key_raw": 0, "key_for": 1, "m": 2, "m2": 3, "f": 4}
KEY_CODECS = ("key_raw", "key_for")
PATHS = {   # name: (environment switches, aggregate list kind)
    "staged_shape": ({}, "shape"),
    "staged_generic": ({}, "generic"),
    "nof32stage_shape": ({"SDB_SCAN_NOF32STAGE": "1"}, "shape"),
    "nof32stage_generic": ({"SDB_SCAN_NOF32STAGE": "1"}, "generic"),
    "noshape": ({"SDB_SCAN_NOSHAPE": "1"}, "shape"),
    "nostage_shape": ({"SDB_SCAN_NOSTAGE": "1"}, "shape"),
    "nostage_generic": ({"SDB_SCAN_NOSTAGE": "1"}, "generic"),
    "hash": ({}, "hash"),
}
ALL_M = ("m", cmx.GE, cmx.I64_MIN, 0)       # passes every row
ALL_M2 = ("m2", cmx.GE, cmx.I64_MIN, 0)
ALL_F = ("f", cmx.GE, -2048.0, 0.0)


def agg_list(kind, sum_col):
    """shape: exactly [COUNT, SUM_I64, SUM_F64] (the straight-lined ASHAPE 1
    bodies unless SDB_SCAN_NOSHAPE); generic / hash: another order plus
    SUM(key) (the runtime aggregate loop, agg_src 9 in every query)"""
    if kind == "shape":
        return ((None, cmx.COUNT), (sum_col, cmx.SUM_I64),
                ("f", cmx.SUM_F64))
    return ((sum_col, cmx.SUM_I64), ("f", cmx.SUM_F64), (None, cmx.COUNT),
            ("key", cmx.SUM_I64))


@pytest.fixture(scope="module")
def ctx():
    c = sa.GpuContext(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def tabs(ctx):
    """every geometry's table, loaded once for the module"""
    out = {}
    for name in GEOMS:
        mx = cmx.matrix(name)
        out[name] = ctx.load_table(
            [mx.key, mx.key, mx.m.vals, mx.m2.vals, mx.f],
            ["raw", "for", "for", "for", "raw"], group_rows=mx.group_rows)
    yield out
    for tab in out.values():
        ctx.free_table(tab)


@pytest.fixture
def path(request, monkeypatch):
    env, kind = PATHS[request.param]
    for k in ("SDB_SCAN_NOSTAGE", "SDB_SCAN_NOSHAPE", "SDB_SCAN_NOF32STAGE"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    return kind


matrix_case = pytest.mark.parametrize(
    "geom,path", [(g, p) for g in GEOMS for p in PATHS],
    indirect=["path"], ids=lambda v: v)


def _gpu_specs(key, preds, aggs):
    return ([(COL[key if c == "key" else c], op, lo, hi)
             for c, op, lo, hi in preds],
            [(COL[key if c == "key" else c] if c else 0, op)
             for c, op in aggs])


def _assert_slots(mx, got, exp, aggs, what, as_bits=False):
    g = np.ascontiguousarray(got)
    e = np.ascontiguousarray(exp)
    if as_bits:
        g, e = g.view(np.uint64), e.view(np.uint64)
    bad = np.argwhere(g != e)
    if len(bad):
        k, q = (int(v) for v in bad[0])
        raise AssertionError(
            f"{what}: {len(bad)} slots differ; first key {k} agg {q} "
            f"{aggs[q]} got {got[k, q]!r} want {exp[k, q]!r}; "
            f"row groups: {mx.describe_keys(bad[:, 0])}")


def check(ctx, tab, mx, kind, key, preds, aggs, nulls=(), label="",
          ngroups=None):
    """one query on the active path == the numpy reference, exactly"""
    preds, aggs = tuple(preds), tuple(aggs)
    ng = ngroups or mx.ngroups
    ri, rf, rpassed = mx.ref_scan(preds, aggs, tuple(nulls), ngroups)
    gp, ga = _gpu_specs(key, preds, aggs)
    what = f"{mx.name} {label} key={key} preds={preds}"
    if kind == "hash":
        keys, hi, hf, passed = ctx.scan_agg_hash(tab, COL[key], 2048, gp, ga)
        qc = [q for q, (_, op) in enumerate(aggs) if op == cmx.COUNT][0]
        np.testing.assert_array_equal(
            keys, np.flatnonzero(ri[:, qc]),
            err_msg=f"{what}: group keys")
        i64 = np.zeros((ng, len(aggs)), dtype=np.int64)
        f64 = np.zeros((ng, len(aggs)), dtype=np.float64)
        i64[keys] = hi
        f64[keys] = hf
    else:
        i64, f64, passed = ctx.scan_agg(tab, COL[key], ng, gp, ga)
    assert passed == rpassed, f"{what}: rows_passed"
    _assert_slots(mx, i64, ri, aggs, what + " i64")
    _assert_slots(mx, f64, rf, aggs, what + " f64", as_bits=True)
    return rpassed


@matrix_case
def test_extraction_every_width_every_role(ctx, tabs, geom, path):
    """all-pass predicates, so every row of every width goes through the
    role's extraction and lands in a slot that names its row group"""
    mx = cmx.matrix(geom)
    roles = {
        # staged: LDS extraction of pred 0, SUM reuses it (agg_src 1)
        "pred0+sum": ([ALL_M], "m"),
        # staged: LDS extraction of pred 1, SUM reuses it (agg_src 2)
        "pred1+sum": ([ALL_M, ALL_M2], "m2"),
        # third predicate and its SUM: global col_read inside every kernel
        "pred2+sum": ([ALL_M2, ALL_F, ALL_M], "m"),
        # SUM of a column no predicate reads (agg_src 0)
        "independent_sum": ([ALL_M], "m2"),
        # SUM of the group key itself (agg_src 9)
        "key_sum": ([ALL_M], "key"),
    }
    for key in KEY_CODECS:
        for role, (preds, sum_col) in roles.items():
            passed = check(ctx, tabs[geom], mx, path, key, preds,
                           agg_list(path, sum_col), label=role)
            assert passed == mx.rows


@matrix_case
def test_group_splitting_predicates(ctx, tabs, geom, path):
    """literal at base + 2^(w-1) of one probed group: that group is split
    row by row (the top delta bit decides), the others are zonemap-dead or
    pass whole. Column m rides predicate slot 0, m2 slot 1."""
    mx = cmx.matrix(geom)
    n = 0
    for col, lead in (("m", []), ("m2", [ALL_M])):
        for label, rg in mx.probe_groups(col).items():
            lit = mx.split_literal(col, rg)
            for op in (cmx.LT, cmx.GE):
                for key in KEY_CODECS:
                    n += check(ctx, tabs[geom], mx, path, key,
                               lead + [(col, op, lit, 0)],
                               agg_list(path, col),
                               label=f"split {col} {label} rg={rg}")
    assert n > 0


@matrix_case
def test_zonemap_edges(ctx, tabs, geom, path):
    """literals exactly at, and one off, a group's vmin / vmax: an
    off-by-one in any copy of the zonemap compares drops or keeps a whole
    group on that path only"""
    mx = cmx.matrix(geom)
    for label, rg in mx.probe_groups("m").items():
        for name, op, lo, hi in mx.zonemap_cases("m", rg):
            for key in KEY_CODECS:
                check(ctx, tabs[geom], mx, path, key, [("m", op, lo, hi)],
                      agg_list(path, "m"),
                      label=f"zonemap {name} {label} rg={rg}")
    # the same compares from predicate slot 1 on the second column
    rg = mx.probe_groups("m2")["w32"]
    for name, op, lo, hi in mx.zonemap_cases("m2", rg):
        check(ctx, tabs[geom], mx, path, "key_for",
              [ALL_M, ("m2", op, lo, hi)], agg_list(path, "m2"),
              label=f"zonemap slot1 {name} rg={rg}")


@matrix_case
def test_two_column_and(ctx, tabs, geom, path):
    """m BETWEEN a span holding the minus5 / zero / 2^40 groups (and none of
    the extreme-base ones) AND m2 < a literal that splits one m2 group"""
    mx = cmx.matrix(geom)
    span = ("m", cmx.BETWEEN, -5, (1 << 40) + (1 << 32))
    inside = [g for g in range(mx.n_rowgroups - 1)
              if mx.m.kinds[g] in ("minus5", "zero", "2^40")]
    assert 0.4 < len(inside) / mx.n_rowgroups < 0.7
    rg = max(inside, key=lambda g: mx.m2.widths[g])
    assert mx.m2.widths[rg] >= 8
    lit = mx.split_literal("m2", rg)
    for key in KEY_CODECS:
        for sum_col in ("m", "m2"):
            passed = check(ctx, tabs[geom], mx, path, key,
                           [span, ("m2", cmx.LT, lit, 0)],
                           agg_list(path, sum_col),
                           label=f"and split m2 rg={rg}")
            assert 0 < passed < mx.rows


@matrix_case
def test_nulls_across_group_boundaries(ctx, tabs, geom, path):
    """validity words straddle the row groups (group_rows is no multiple of
    64): a comparison drops NULLs, IS NULL reads the plane alone, SUM skips
    NULL values while COUNT(*) keeps the row"""
    mx = cmx.matrix(geom)
    tab = tabs[geom]
    lit = mx.split_literal("m", mx.probe_groups("m")["w31"])
    try:
        ctx.attach_validity(tab, COL["m"], mx.validity_words("m"))
        for key in KEY_CODECS:
            for preds in ([("m", cmx.LT, lit, 0)], [("m", cmx.LT, 0, 0)],
                          [("m", cmx.ISNULL, 0, 0)],
                          [ALL_M2, ("m", cmx.NOTNULL, 0, 0)]):
                check(ctx, tab, mx, path, key, preds, agg_list(path, "m"),
                      nulls=("m",), label="nulls in m")
            # m unread by any predicate: only its SUM sees the plane
            check(ctx, tab, mx, path, key, [ALL_M2], agg_list(path, "m"),
                  nulls=("m",), label="nulls in m, sum only")
    finally:
        ctx.attach_validity(tab, COL["m"], None)
    try:
        ctx.attach_validity(tab, COL["f"], mx.validity_words("f"))
        for key in KEY_CODECS:
            check(ctx, tab, mx, path, key, [ALL_M], agg_list(path, "m"),
                  nulls=("f",), label="nulls in f")
            check(ctx, tab, mx, path, key, [("f", cmx.GE, 0.0, 0.0), ALL_M],
                  agg_list(path, "m"), nulls=("f",),
                  label="nulls in f, f predicate")
    finally:
        ctx.attach_validity(tab, COL["f"], None)


@pytest.mark.parametrize("env", [{}, {"SDB_SCAN_NOF32STAGE": "1"},
                                 {"SDB_SCAN_NOSTAGE": "1"}],
                         ids=["staged", "nof32stage", "nostage"])
@pytest.mark.parametrize("ngroups", [1088, 1500, 2048])
def test_lds_budget(ctx, tabs, monkeypatch, ngroups, env):
    """eight aggregates over three staged width-32 columns. The accumulators
    take 8*ngroups*8 bytes of LDS: at 1088 groups the 8192-row chunk still
    fits but the f32 stage buffer does not, 1500 groups halve the chunk
    once, and 2048 groups x 8 aggregates (128 KB) shrink it to 1024 rows —
    the largest dynamic-LDS launch the entry can make (about 140 KB). Must
    return SDB_OK with exact results."""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    mx = cmx.matrix("chunk")
    aggs = ((None, cmx.COUNT), ("m", cmx.SUM_I64), ("m2", cmx.SUM_I64),
            ("key", cmx.SUM_I64), ("f", cmx.SUM_F64), (None, cmx.COUNT),
            ("m", cmx.SUM_I64), ("f", cmx.SUM_F64))
    lit = mx.split_literal("m2", mx.probe_groups("m2")["w32"])
    for key in KEY_CODECS:
        passed = check(ctx, tabs["chunk"], mx, "dense", key, [ALL_M, ALL_M2],
                       aggs, label=f"lds ngroups={ngroups}", ngroups=ngroups)
        assert passed == mx.rows
        check(ctx, tabs["chunk"], mx, "dense", key,
              [ALL_M, ("m2", cmx.GE, lit, 0)], aggs,
              label=f"lds split ngroups={ngroups}", ngroups=ngroups)


def _check_hash(ctx, tab, mx, group_col, max_groups, preds, aggs, label):
    rk, ri, rf, rpassed = mx.ref_hash(group_col, tuple(preds), tuple(aggs))
    gp, ga = _gpu_specs("key_for", preds, aggs)
    keys, i64, f64, passed = ctx.scan_agg_hash(
        tab, COL.get(group_col, COL["key_for"]), max_groups, gp, ga)
    what = f"{mx.name} hash by {group_col} {label}"
    assert passed == rpassed, what
    np.testing.assert_array_equal(keys, rk, err_msg=what + ": keys")
    np.testing.assert_array_equal(i64, ri, err_msg=what + ": i64")
    np.testing.assert_array_equal(f64.view(np.uint64), rf.view(np.uint64),
                                  err_msg=what + ": f64 bits")
    return keys


@pytest.mark.parametrize("geom", GEOMS)
def test_hash_group_by_for_column(ctx, tabs, geom):
    """GROUP BY m: arbitrary i64 keys decoded from every FoR width, both
    ends of int64 and the table's reserved key -1, a few thousand distinct.
    An f32 predicate thins every row group alike so all widths feed keys;
    8192 max groups keeps the 4096-slot LDS table on while overfilling it
    (probe misses fall through to the global table)."""
    mx = cmx.matrix(geom)
    tab = tabs[geom]
    thin = ("f", cmx.GE, 1009.0 if geom == "chunk" else 768.0, 0.0)
    aggs = ((None, cmx.COUNT), ("m2", cmx.SUM_I64), ("f", cmx.SUM_F64))
    keys = _check_hash(ctx, tab, mx, "m", 8192, [ALL_M2, thin], aggs, "thin")
    assert 2000 < len(keys) <= 8192
    assert -1 in keys
    assert keys.min() < -(1 << 62) and keys.max() > (1 << 62)
    rows = np.flatnonzero(mx.pred_mask((ALL_M2, thin)))
    assert set((rows // mx.group_rows).tolist()) >= set(range(33))
    # m2 predicate that splits one group and kills the ones above it
    g2 = max((g for g in range(mx.n_rowgroups - 1)
              if mx.m2.kinds[g] == "2^40"), key=lambda g: mx.m2.widths[g])
    split = ("m2", cmx.LT, mx.split_literal("m2", g2), 0)
    keys = _check_hash(ctx, tab, mx, "m", 8192, [split, thin], aggs,
                       f"split m2 rg={g2}")
    assert 1000 < len(keys)
    # low cardinality: every key stays in the LDS table
    keys = _check_hash(ctx, tab, mx, "key", 2048, [split], aggs,
                       "low cardinality")
    assert len(keys) <= mx.ngroups
    # LDS table off (max_groups beyond twice its slots): global upserts only
    _check_hash(ctx, tab, mx, "m", 1 << 14, [ALL_M2, thin], aggs,
                "global table only")
