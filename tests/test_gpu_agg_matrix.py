"""MIN / MAX / COUNT(col) on every GPU scan path, against the aggregate
matrix (tests/agg_matrix.py; tests/test_agg_matrix.py proves its references
on the CPU). One pytest case per (geometry, path) so a failure names the
path. Every comparison is exact: integers equal, f64 as bit patterns.

Paths:
  raw          every column raw: scan_agg_kernel<1,0>, quad loop + rows&3 tail
  staged       scan_agg_staged_kernel<0>, f32 aggregate column staged in LDS
  nof32stage   the same with SDB_SCAN_NOF32STAGE (f32 read from global)
  nostage      scan_agg_kernel<0,0> (SDB_SCAN_NOSTAGE), pair loop + odd tail
  hash_lds     scan_agg_hash_kernel, max_groups 2048: LDS table + flush
  hash_global  max_groups 2^14: lds_slots == 0, upserts straight to global

Groups are `key` (each in one row group) and `kmod` = row % 61 (each in every
row group, so right only if the workgroups' partials merge with min / max),
both as a raw and as a FoR column.
"""

import numpy as np
import pytest

import agg_matrix as amx
import col_matrix as cmx
import serenedb_amd as sa

pytestmark = pytest.mark.gpu

COL = {"key_raw": 0, "key_for": 1, "m": 2, "m2": 3, "f": 4, "kmod_raw": 5,
       "kmod_for": 6, "fx": 7}
CODECS = {"for": ["raw", "for", "for", "for", "raw", "raw", "for", "raw"],
          "raw": ["raw"] * 8}
ENV_SWITCHES = ("SDB_SCAN_NOSTAGE", "SDB_SCAN_NOSHAPE", "SDB_SCAN_NOF32STAGE")
PATHS = {   # name: (environment, entry, table, max_groups)
    "raw": ({}, "dense", "raw", None),
    "staged": ({}, "dense", "for", None),
    "nof32stage": ({"SDB_SCAN_NOF32STAGE": "1"}, "dense", "for", None),
    "nostage": ({"SDB_SCAN_NOSTAGE": "1"}, "dense", "for", None),
    "hash_lds": ({}, "hash", "for", 2048),
    "hash_global": ({}, "hash", "for", 1 << 14),
}
FOR_PATHS = ("staged", "nof32stage", "nostage")
HASH_PATHS = ("hash_lds", "hash_global")
OP_NAME = {v: k for k, v in getattr(sa.GpuContext, "AGG_OPS", {}).items()}

ALL_M = ("m", cmx.GE, cmx.I64_MIN, 0)
ALL_M2 = ("m2", cmx.GE, cmx.I64_MIN, 0)
ALL_F = ("f", cmx.GE, -2048.0, 0.0)
EQ_MIN = ("m", cmx.EQ, cmx.I64_MIN, 0)
EQ_MAX = ("m", cmx.EQ, cmx.I64_MAX, 0)
FX_SMALL = ("fx", cmx.BETWEEN, -1.0, 1.0)
THIN = ("f", cmx.GE, 1020.0, 0.0)

C, CC = amx.COUNT, amx.COUNT_COL
MIN_I, MAX_I, MIN_F, MAX_F = (amx.MIN_I64, amx.MAX_I64, amx.MIN_F32,
                              amx.MAX_F32)
AGGS_NEW = ((None, C), ("m", CC), ("m", MIN_I), ("m2", MAX_I),
            ("fx", MIN_F), ("fx", MAX_F))


def split(am, col, op=cmx.LT, label="w31"):
    mx = am.mx
    return (col, op, mx.split_literal(col, mx.probe_groups(col)[label]), 0)


@pytest.fixture(scope="module")
def ctx():
    c = sa.GpuContext(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def tabs(ctx):
    """per geometry a FoR table and an all-raw one with the same columns"""
    out = {}
    for name in amx.GEOMS:
        am = amx.matrix(name)
        mx = am.mx
        arrays = [mx.key, mx.key, mx.m.vals, mx.m2.vals, mx.f, am.kmod,
                  am.kmod, am.fx]
        for kind, codecs in CODECS.items():
            out[name, kind] = ctx.load_table(arrays, codecs,
                                             group_rows=mx.group_rows)
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
        "geom,path", [(g, p) for g in amx.GEOMS for p in paths],
        indirect=["path"], ids=lambda v: v)


def codecs_of(path):
    return ("raw",) if PATHS[path][2] == "raw" else ("raw", "for")


def gpu_specs(group, codec, preds, aggs, names=False):
    """column names -> indices; `key` / `kmod` as an aggregate or predicate
    column mean the group column in the codec under test. Ops travel as
    SdbAggOp numbers, or by AGG_OPS name if names is set."""
    def col(c):
        return COL[f"{c}_{codec}" if c in ("key", "kmod") else c]
    return ([(col(c), op, lo, hi) for c, op, lo, hi in preds],
            [(col(c) if c else 0, OP_NAME[op] if names else op)
             for c, op in aggs])


def assert_exact(got, want, what, aggs, as_bits=False):
    g = np.ascontiguousarray(got)
    w = np.ascontiguousarray(want)
    if as_bits:
        g, w = g.view(np.uint64), w.view(np.uint64)
    bad = np.argwhere(g != w)
    if len(bad):
        k, q = (int(v) for v in bad[0])
        raise AssertionError(
            f"{what}: {len(bad)} slots differ; first group row {k} agg {q} "
            f"{aggs[q]} got {got[k, q]!r} want {want[k, q]!r}")


def check(ctx, tabs, am, path, group, codec, preds, aggs, nulls=(),
          label="", names=False):
    """one query on the active path == the numpy reference, exactly.
    Returns (i64, f64, present, dense) over all groups: present marks the
    groups with a passing row; a hash aggregate returns only those, so its
    other rows are filled from the reference and dense is False."""
    preds, aggs, nulls = tuple(preds), tuple(aggs), tuple(nulls)
    _, entry, kind, max_groups = PATHS[path]
    tab = tabs[am.name, kind]
    ri, rf, rpassed, present = am.ref_dense(group, preds, aggs, nulls)
    ng = len(present)
    gp, ga = gpu_specs(group, codec, preds, aggs, names)
    gcol = COL[f"{group}_{codec}"]
    what = f"{am.name} {path} {label} group={group}_{codec} preds={preds}"
    if entry == "hash":
        keys, hi, hf, passed = ctx.scan_agg_hash(tab, gcol, max_groups, gp,
                                                 ga)
        np.testing.assert_array_equal(keys, np.flatnonzero(present),
                                      err_msg=what + ": group keys")
        i64, f64 = ri.copy(), rf.copy()     # absent groups: not returned
        i64[keys] = hi
        f64[keys] = hf
    else:
        i64, f64, passed = ctx.scan_agg(tab, gcol, ng, gp, ga)
    assert passed == rpassed, what + ": rows_passed"
    assert_exact(i64, ri, what + " i64", aggs)
    assert_exact(f64, rf, what + " f64", aggs, as_bits=True)
    return i64, f64, present, entry == "dense"


@cases(PATHS)
def test_all_new_ops_together(ctx, tabs, geom, path):
    """the five new ops beside COUNT(*) in one list, every row passing and
    under a predicate that splits one row group row by row"""
    am = amx.matrix(geom)
    for group in ("key", "kmod"):
        for codec in codecs_of(path):
            for preds in ([ALL_M], [split(am, "m")],
                          [ALL_M, split(am, "m2", cmx.GE, "w32")]):
                i64, _, present, _ = check(ctx, tabs, am, path, group, codec,
                                           preds, AGGS_NEW, label="new ops")
                # no plane attached: COUNT(col) is COUNT(*)
                assert np.array_equal(i64[present, 1], i64[present, 0])
    # the same list with its ops given by AGG_OPS name
    check(ctx, tabs, am, path, "kmod", "raw", [ALL_M], AGGS_NEW,
          label="ops by name", names=True)


@cases(PATHS)
def test_code_zero_collisions(ctx, tabs, geom, path):
    """MAX over rows that all hold INT64_MIN (and MIN over INT64_MAX) gives
    accumulator code 0, the same as a group without a value: both return
    the identity, COUNT(col) tells them apart"""
    am = amx.matrix(geom)
    aggs = ((None, C), ("m", CC), ("m", MAX_I), ("m", MIN_I))
    for pred, q, want in ((EQ_MIN, 2, cmx.I64_MIN), (EQ_MAX, 3, cmx.I64_MAX)):
        for group in ("key", "kmod"):
            for codec in codecs_of(path):
                i64, _, present, dense = check(
                    ctx, tabs, am, path, group, codec, [pred], aggs,
                    label="code 0")
                assert present.any()
                assert np.all(i64[present, q] == want)
                assert np.all(i64[present, 1] > 0)
                if dense and group == "key":
                    assert (~present).any()
                if dense:       # empty groups: same value, COUNT(col) 0
                    assert np.all(i64[~present, q] == want)
                    assert np.all(i64[~present, 1] == 0)
                    assert np.all(i64[~present, 2] == cmx.I64_MIN)
                    assert np.all(i64[~present, 3] == cmx.I64_MAX)


@cases(PATHS)
def test_null_planes(ctx, tabs, geom, path):
    """planes on m and fx: NULLs are skipped by every op; the two kmod groups
    that are NULL in every row pass rows, count none, return identities"""
    am = amx.matrix(geom)
    tab = tabs[geom, PATHS[path][2]]
    aggs = ((None, C), ("m", CC), ("m", MIN_I), ("m", MAX_I), ("fx", CC),
            ("fx", MIN_F), ("fx", MAX_F))
    try:
        ctx.attach_validity(tab, COL["m"], am.validity_words("m"))
        ctx.attach_validity(tab, COL["fx"], am.validity_words("fx"))
        for group in ("key", "kmod"):
            for codec in codecs_of(path):
                for preds in ([ALL_M2], [split(am, "m2")]):
                    i64, f64, present, _ = check(
                        ctx, tabs, am, path, group, codec, preds, aggs,
                        nulls=("m", "fx"), label="nulls")
                    if group != "kmod":
                        continue
                    for k in amx.ALL_NULL:
                        assert present[k] and i64[k, 0] > 0
                        assert i64[k, 1] == 0 and i64[k, 4] == 0
                        assert i64[k, 2] == cmx.I64_MAX
                        assert i64[k, 3] == cmx.I64_MIN
                        assert f64[k, 5] == np.inf and f64[k, 6] == -np.inf
                    live = present.copy()
                    live[list(amx.ALL_NULL)] = False
                    assert np.all(i64[live, 1] < i64[live, 0])
                    assert np.all(i64[live, 1] > 0)
    finally:
        ctx.attach_validity(tab, COL["m"], None)
        ctx.attach_validity(tab, COL["fx"], None)


@cases(PATHS)
def test_f32_special_value_groups(ctx, tabs, geom, path):
    """NaN wins MAX; MIN ignores NaN unless every value is NaN; -0.0 < +0.0
    by bits; a sign-set NaN counts as greatest; infinities and denormals"""
    am = amx.matrix(geom)
    g = amx.FX_GROUPS
    aggs = ((None, C), ("fx", MIN_F), ("fx", MAX_F), ("fx", CC))
    for codec in codecs_of(path):
        _, f64, present, _ = check(ctx, tabs, am, path, "kmod", codec,
                                   [ALL_M], aggs, label="fx groups")
        assert present.all()
        lo, hi = amx.f64_bits(f64[:, 1]), amx.f64_bits(f64[:, 2])
        assert lo[g["all_nan"]] == hi[g["all_nan"]] == amx.F64_NAN
        assert lo[g["zeros"]] == 1 << 63 and hi[g["zeros"]] == 0
        assert hi[g["neg_nan_finite"]] == amx.F64_NAN
        assert np.isfinite(f64[g["neg_nan_finite"], 1])
        assert f64[g["neg_inf"], 1] == f64[g["neg_inf"], 2] == -np.inf
        assert f64[g["pos_inf"], 1] == f64[g["pos_inf"], 2] == np.inf
        flt_max = float(np.finfo(np.float32).max)
        assert f64[g["denorm_fltmax"], 1] == -flt_max
        assert f64[g["denorm_fltmax"], 2] == flt_max
        # |fx| <= 1 keeps zeros and denormals: the largest denormal wins
        _, f64, present, _ = check(ctx, tabs, am, path, "kmod", codec,
                                   [ALL_M, FX_SMALL], aggs,
                                   label="fx small")
        assert not present[g["all_nan"]] and present[g["denorm_fltmax"]]
        lo, hi = amx.f64_bits(f64[:, 1]), amx.f64_bits(f64[:, 2])
        assert hi[g["denorm_fltmax"]] == amx.f32_bits_to_f64_bits(0x007FFFFF)
        assert lo[g["denorm_fltmax"]] == amx.f32_bits_to_f64_bits(0x807FFFFF)
        assert lo[g["zeros"]] == 1 << 63 and hi[g["zeros"]] == 0
        # grouped by key too (each group one row group)
        check(ctx, tabs, am, path, "key", codec, [ALL_M], aggs,
              label="fx by key")


@cases(FOR_PATHS)
def test_minmax_by_extraction_role(ctx, tabs, geom, path):
    """MIN_I64 / MAX_I64 of a column a predicate also reads (its extracted
    value is reused), of a column no predicate reads, and of the group key"""
    am = amx.matrix(geom)
    roles = {
        "pred0 value reused": ([split(am, "m", cmx.GE)], "m"),
        "pred1 value reused": ([ALL_M, split(am, "m2")], "m2"),
        "third predicate": ([ALL_M2, ALL_F, split(am, "m", cmx.GE)], "m"),
        "independent column": ([ALL_M], "m2"),
    }
    for group in ("key", "kmod"):
        for codec in ("raw", "for"):
            for role, (preds, col) in roles.items():
                check(ctx, tabs, am, path, group, codec, preds,
                      ((None, C), (col, MIN_I), (col, MAX_I), (col, CC)),
                      label=role)
            check(ctx, tabs, am, path, group, codec, [split(am, "m")],
                  ((group, MAX_I), (None, C), (group, MIN_I)),
                  label="group key itself")


@cases(HASH_PATHS)
def test_hash_by_m_with_key_minus_one(ctx, tabs, geom, path):
    """GROUP BY m: arbitrary keys from both ends of int64 and the reserved
    key -1, whose accumulators live outside the table (neg_acc)"""
    am = amx.matrix(geom)
    tab = tabs[geom, "for"]
    aggs = ((None, C), ("m2", MIN_I), ("fx", MAX_F), ("fx", CC))
    preds = (ALL_M2, THIN)
    gp, ga = gpu_specs("key", "for", preds, aggs)
    for nulls in ((), ("fx",)):
        rk, ri, rf, rpassed = am.ref_hash("m", preds, aggs, nulls)
        assert -1 in rk and len(rk) <= 2048
        try:
            if nulls:
                ctx.attach_validity(tab, COL["fx"], am.validity_words("fx"))
            keys, i64, f64, passed = ctx.scan_agg_hash(
                tab, COL["m"], PATHS[path][3], gp, ga)
        finally:
            ctx.attach_validity(tab, COL["fx"], None)
        what = f"{geom} {path} hash by m nulls={nulls}"
        assert passed == rpassed, what
        np.testing.assert_array_equal(keys, rk, err_msg=what + ": keys")
        assert_exact(i64, ri, what + " i64", aggs)
        assert_exact(f64, rf, what + " f64", aggs, as_bits=True)


def test_hash_str_minmax(ctx, tabs):
    """GROUP BY a string column made from kmod, through the shared core"""
    am = amx.matrix("odd_t33")
    tab = tabs["odd_t33", "for"]
    names, values = am.kmod_strings()
    offsets, blob = sa.encode_col_str_raw(values)
    ctx.attach_strcol(tab, 0, offsets, blob)
    aggs = ((None, C), ("m", MIN_I), ("m2", MAX_I), ("fx", MIN_F),
            ("fx", MAX_F), ("fx", CC))
    preds = (split(am, "m"),)
    gp, ga = gpu_specs("kmod", "for", preds, aggs)
    keys, i64, f64, passed = ctx.scan_agg_hash_str(tab, 0, 2048, gp, ga,
                                                   values=names)
    ri, rf, rpassed, present = am.ref_dense("kmod", preds, aggs)
    assert passed == rpassed and present.all()
    order = [names.index(k) for k in keys]
    assert sorted(order) == list(range(amx.NKMOD))
    assert_exact(i64, ri[order], "hash_str i64", aggs)
    assert_exact(f64, rf[order], "hash_str f64", aggs, as_bits=True)


@pytest.mark.parametrize("entry", ["scan_agg", "scan_agg_hash",
                                   "scan_agg_hash_str"])
@pytest.mark.parametrize("bad", [
    pytest.param((0, 8), id="op_8"),
    pytest.param((len(COL), MIN_I), id="col_eq_ncols"),
    pytest.param((len(COL), CC), id="count_col_eq_ncols"),
    pytest.param((len(COL), amx.SUM_I64), id="sum_col_eq_ncols"),
    pytest.param((COL["fx"], MIN_I), id="min_i64_on_f32"),
    pytest.param((COL["fx"], MAX_I), id="max_i64_on_f32"),
    pytest.param((COL["m"], MIN_F), id="min_f32_on_i64"),
    pytest.param((COL["key_raw"], MAX_F), id="max_f32_on_raw_i64"),
])
def test_rejections(ctx, tabs, entry, bad):
    """SDB_ERR_INVALID (RuntimeError in the wrapper) from every entry, with
    the bad aggregate after a good one"""
    am = amx.matrix("odd_t33")
    tab = tabs["odd_t33", "for"]
    aggs = [(0, C), bad]
    with pytest.raises(RuntimeError, match="rc=-1"):
        if entry == "scan_agg":
            ctx.scan_agg(tab, COL["kmod_for"], amx.NKMOD, [], aggs)
        elif entry == "scan_agg_hash":
            ctx.scan_agg_hash(tab, COL["kmod_for"], 2048, [], aggs)
        else:
            offsets, blob = sa.encode_col_str_raw(am.kmod_strings()[1])
            ctx.attach_strcol(tab, 1, offsets, blob)
            ctx.scan_agg_hash_str(tab, 1, 2048, [], aggs)
    # the same list without the bad entry is accepted
    i64, _, passed = ctx.scan_agg(tab, COL["kmod_for"], amx.NKMOD, [],
                                  aggs[:1])
    assert passed == am.rows == int(i64.sum())


@cases(PATHS)
def test_old_ops_unchanged(ctx, tabs, geom, path):
    """lists of only COUNT / SUM_I64 / SUM_F64 on the same tables still match
    col_matrix's own references (they run the instantiations without the new
    arms)"""
    am = amx.matrix(geom)
    mx = am.mx
    _, entry, kind, max_groups = PATHS[path]
    tab = tabs[geom, kind]
    lists = (((None, cmx.COUNT), ("m", cmx.SUM_I64), ("f", cmx.SUM_F64)),
             (("m2", cmx.SUM_I64), ("f", cmx.SUM_F64), (None, cmx.COUNT),
              ("key", cmx.SUM_I64)))
    for codec in codecs_of(path):
        for preds in ((ALL_M,), (split(am, "m"),)):
            for aggs in lists:
                ri, rf, rpassed = mx.ref_scan(preds, aggs)
                gp, ga = gpu_specs("key", codec, preds, aggs)
                gcol = COL[f"key_{codec}"]
                what = f"{geom} {path} old ops key_{codec} {preds}"
                if entry == "hash":
                    qc = [op for _, op in aggs].index(cmx.COUNT)
                    keys, hi, hf, passed = ctx.scan_agg_hash(
                        tab, gcol, max_groups, gp, ga)
                    np.testing.assert_array_equal(
                        keys, np.flatnonzero(ri[:, qc]), err_msg=what)
                    ri, rf = ri[keys], rf[keys]
                    i64, f64 = hi, hf
                else:
                    i64, f64, passed = ctx.scan_agg(tab, gcol, mx.ngroups,
                                                    gp, ga)
                assert passed == rpassed, what
                assert_exact(i64, ri, what + " i64", aggs)
                assert_exact(f64, rf, what + " f64", aggs, as_bits=True)
