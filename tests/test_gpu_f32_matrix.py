"""f32 compares and SUM_F64 at their IEEE edges on every GPU scan path,
against the f32 predicate matrix (tests/f32_matrix.py; tests/test_f32_matrix.py
proves its cases, mutants and may-assert masks on the CPU). One pytest case
per (geometry, path); the case loop runs inside and a failure names the case.
Integers compare exactly; an asserted SUM_F64 compares as NaN-ness, else by
value (f32_matrix.check_sums).

Paths (the names of the other matrices, plus the later entries):
  raw          every column raw: scan_agg_kernel<1,0>, quad loop + rows&3 tail
  staged       scan_agg_staged_kernel, chunk loop; f32 aggregate staged in LDS
  nof32stage   the same with SDB_SCAN_NOF32STAGE (f32 read from global)
  nostage      scan_agg_kernel<0,0> (SDB_SCAN_NOSTAGE), pair loop + odd tail
  hash_lds     scan_agg_hash, max_groups 2048: LDS table + flush
  hash_global  max_groups 2^14: upserts straight to global
  nullkey      scan_agg_nullkey, a validity plane on the group column
  hash_nullkey scan_agg_hash_nullkey, the same
  multi        scan_agg_hash_multi over (kmod, key)
  topn         scan_topn ORDER BY key LIMIT 65536: the passing rows themselves

The staged kernels run only when the group key or one of the first two
predicates is a FoR column, and fl is raw: the loop alternates a FoR group
column with a raw one beside an all-passing FoR predicate, before or after
the f32 one.
"""

import numpy as np
import pytest

import col_matrix as cmx
import f32_matrix as fmx
import serenedb_amd as sa

pytestmark = pytest.mark.gpu

COL = {"key_raw": 0, "key_for": 1, "m": 2, "m2": 3, "f": 4, "kmod_raw": 5,
       "kmod_for": 6, "fx": 7, "fl": 8, "flabs": 9}
CODECS = {"for": ["raw", "for", "for", "for", "raw", "raw", "for", "raw",
                  "raw", "for"],
          "raw": ["raw"] * 10}
KEY_COLS = ("key_raw", "key_for", "kmod_raw", "kmod_for")
ENV_SWITCHES = ("SDB_SCAN_NOSTAGE", "SDB_SCAN_NOSHAPE", "SDB_SCAN_NOF32STAGE")
PATHS = {   # name: (environment, entry, table, max_groups)
    "raw": ({}, "dense", "raw", None),
    "staged": ({}, "dense", "for", None),
    "nof32stage": ({"SDB_SCAN_NOF32STAGE": "1"}, "dense", "for", None),
    "nostage": ({"SDB_SCAN_NOSTAGE": "1"}, "dense", "for", None),
    "hash_lds": ({}, "hash", "for", 2048),
    "hash_global": ({}, "hash", "for", 1 << 14),
    "nullkey": ({}, "nullkey", "for", None),
    "hash_nullkey": ({}, "hash_nullkey", "for", 2048),
    "multi": ({}, "multi", "for", 1 << 15),
    "topn": ({}, "topn", "for", None),
}
AGG_PATHS = tuple(p for p in PATHS if p != "topn")
TOPN_K = 65536

ALL_M2 = ("m2", cmx.GE, cmx.I64_MIN, 0)
# the case loop's aggregates: with kmod and key as groups, COUNT(*),
# COUNT(fl) and SUM(m) per group pin which rows passed
AGGS_ROWS = ((None, fmx.COUNT), ("fl", fmx.COUNT_COL), ("m", fmx.SUM_I64))
# (group, group codec, where the all-passing FoR predicate goes) by case
VARIANTS = (("kmod", "for", None), ("key", "for", None),
            ("kmod", "raw", 0), ("key", "raw", 1))


@pytest.fixture(scope="module")
def ctx():
    c = sa.GpuContext(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def tabs(ctx):
    """per geometry a FoR table and an all-raw one: the columns of
    tests/test_gpu_agg_matrix.py plus fl and flabs"""
    out = {}
    for name in fmx.GEOMS:
        fm = fmx.matrix(name)
        mx, am = fm.mx, fm.am
        arrays = [mx.key, mx.key, mx.m.vals, mx.m2.vals, mx.f, am.kmod,
                  am.kmod, am.fx, fm.fl, fm.flabs]
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
        "geom,path", [(g, p) for g in fmx.GEOMS for p in paths],
        indirect=["path"], ids=lambda v: v)


class Planes:
    """validity planes attached for a block, detached after it"""

    def __init__(self, ctx, tab, fm, planes):
        self.ctx, self.tab, self.fm, self.planes = ctx, tab, fm, planes

    def __enter__(self):
        for col, plane in self.planes.items():
            self.ctx.attach_validity(self.tab, COL[col],
                                     self.fm.validity_words(plane))

    def __exit__(self, *exc):
        for col in self.planes:
            self.ctx.attach_validity(self.tab, COL[col], None)


def key_planes(path):
    """the nullable-key entries run with the key plane on every group column"""
    if PATHS[path][1] in ("nullkey", "hash_nullkey"):
        return {c: "key" for c in KEY_COLS}
    return {}


def grouping(path, group):
    entry = PATHS[path][1]
    if entry in ("nullkey", "hash_nullkey"):
        return group + "_null"
    return "kmod_key" if entry == "multi" else group


def gpu_specs(codec, preds, aggs):
    def col(c):
        return COL[f"{c}_{codec}" if c in ("key", "kmod") else c]
    return ([(col(c), op, lo, hi) for c, op, lo, hi in preds],
            [(col(c) if c else 0, op) for c, op in aggs])


def scatter(ng, na, ids, i64, f64):
    """a hash result as dense rows; the groups it does not return hold the
    zeros the dense scan gives an empty group of COUNT / SUM"""
    di = np.zeros((ng, na), dtype=np.int64)
    df = np.zeros((ng, na), dtype=np.float64)
    di[ids] = i64
    df[ids] = f64
    return di, df


def run_agg(ctx, tab, fm, path, group, codec, preds, aggs, nulls, what):
    """one aggregate query on the active path, checked against fm.ref:
    rows_passed, the returned groups, every integer slot exactly and every
    SUM_F64 slot that may be asserted"""
    _, entry, _, max_groups = PATHS[path]
    gname = grouping(path, group)
    ri, rf, ok, rpassed, present = fm.ref(gname, tuple(preds), tuple(aggs),
                                          tuple(nulls))
    ng, na = ri.shape
    gp, ga = gpu_specs(codec, preds, aggs)
    gcol = COL[f"{group}_{codec}"]
    if entry == "dense":
        i64, f64, passed = ctx.scan_agg(tab, gcol, ng, gp, ga)
    elif entry == "hash":
        keys, hi, hf, passed = ctx.scan_agg_hash(tab, gcol, max_groups, gp,
                                                 ga)
        assert np.array_equal(keys, np.flatnonzero(present)), what + ": keys"
        i64, f64 = scatter(ng, na, keys, hi, hf)
    elif entry == "nullkey":
        i64, f64, passed, null_rows = ctx.scan_agg_nullkey(tab, gcol, ng - 1,
                                                           gp, ga)
        assert null_rows == fm.null_rows(preds, nulls), what + ": null_rows"
    elif entry == "hash_nullkey":
        keys, hi, hf, passed, ni, nf, null_rows = ctx.scan_agg_hash_nullkey(
            tab, gcol, max_groups, gp, ga)
        assert null_rows == fm.null_rows(preds, nulls), what + ": null_rows"
        assert np.array_equal(keys, np.flatnonzero(present[:-1])), \
            what + ": keys"
        i64, f64 = scatter(ng, na, keys, hi, hf)
        i64[-1], f64[-1] = ni, nf
    else:
        assert entry == "multi"
        nkey = fm.groups["key"][1]
        keys, keynull, hi, hf, passed = ctx.scan_agg_hash_multi(
            tab, [COL[f"kmod_{codec}"], COL[f"key_{codec}"]], max_groups, gp,
            ga)
        assert not keynull.any(), what + ": keynull"
        ids = keys[:, 0] * nkey + keys[:, 1]
        assert np.array_equal(ids, np.flatnonzero(present)), what + ": tuples"
        i64, f64 = scatter(ng, na, ids, hi, hf)
    assert passed == rpassed, f"{what}: rows_passed {passed} want {rpassed}"
    bad = np.argwhere(i64 != ri)
    if len(bad):
        k, q = (int(v) for v in bad[0])
        raise AssertionError(
            f"{what}: {len(bad)} integer slots differ; first group row {k} "
            f"agg {q} {aggs[q]} got {i64[k, q]} want {ri[k, q]}")
    for q, (_, op) in enumerate(aggs):
        if op == fmx.SUM_F64:
            fmx.check_sums(f64[:, q], rf[:, q], ok[:, q],
                           f"{what} agg {q} {aggs[q]}")


def case_query(i, case, path):
    """(group, codec, preds) of case i: the variants by turns"""
    group, codec, extra = VARIANTS[i % len(VARIANTS)]
    if PATHS[path][2] == "raw":
        codec = "raw"
    preds = [("fl",) + case[1:4]]
    if extra is not None:
        preds.insert(extra, ALL_M2)
    return group, codec, preds


@cases(PATHS)
def test_f32_predicate_cases(ctx, tabs, geom, path):
    """every case of the matrix, fl's plane detached and attached"""
    fm = fmx.matrix(geom)
    tab = tabs[geom, PATHS[path][2]]
    with Planes(ctx, tab, fm, key_planes(path)):
        for nulls in ((), ("fl",)):
            with Planes(ctx, tab, fm, {c: c for c in nulls}):
                for i, case in enumerate(fmx.CASES):
                    group, codec, preds = case_query(i, case, path)
                    what = (f"{geom} {path} case {case[0]} plane={nulls} "
                            f"group={group}_{codec}")
                    if path == "topn":
                        run_topn(ctx, tabs, fm, i, preds, nulls, what)
                    else:
                        run_agg(ctx, tab, fm, path, group, codec, preds,
                                AGGS_ROWS, nulls, what)


def run_topn(ctx, tabs, fm, i, preds, nulls, what):
    """ORDER BY key (raw) LIMIT 65536: on odd_t33 k >= rows, so the result
    is the exact set of passing rows; on chunk its first 65536"""
    kind = ("for", "raw")[i % 2]
    if nulls and kind == "raw":
        kind = "for"            # the plane is attached to the active table
    gp, _ = gpu_specs("raw", preds, ())
    rows, vals, isnull, passed = ctx.scan_topn(tabs[fm.name, kind],
                                               COL["key_raw"], TOPN_K, gp)
    want, rpassed = fm.ref_topn(tuple(preds), tuple(nulls), TOPN_K)
    assert passed == rpassed, f"{what}: rows_passed {passed} want {rpassed}"
    assert fm.rows > TOPN_K or len(want) == rpassed
    assert np.array_equal(rows, want), what + ": passing rows"
    assert np.array_equal(vals, fm.mx.key[want.astype(np.int64)]), what
    assert not isnull.any(), what


@cases(AGG_PATHS)
def test_sum_f64_special_values(ctx, tabs, geom, path):
    """SUM_F64 over fx and fl where the inputs hold +-inf, NaN and
    subnormals: the shape-specialised [COUNT, SUM_I64, SUM_F64] list and a
    permuted one, the predicate on the summed column (the staged kernel
    then reads it from LDS) and on another, planes detached and attached"""
    fm = fmx.matrix(geom)
    tab = tabs[geom, PATHS[path][2]]
    codec = "raw" if PATHS[path][2] == "raw" else "for"
    lists = (((None, fmx.COUNT), ("m", fmx.SUM_I64), ("fx", fmx.SUM_F64)),
             ((None, fmx.COUNT), ("m", fmx.SUM_I64), ("fl", fmx.SUM_F64)),
             (("fl", fmx.SUM_F64), ("m", fmx.SUM_I64), (None, fmx.COUNT),
              ("fx", fmx.SUM_F64)))
    with Planes(ctx, tab, fm, key_planes(path)):
        for nulls in ((), ("fx", "fl", "m")):
            with Planes(ctx, tab, fm, {c: c for c in nulls}):
                for name, group, preds in fmx.SUM_CASES:
                    for aggs in lists:
                        what = (f"{geom} {path} sum case {name} "
                                f"planes={nulls} group={group}_{codec}")
                        run_agg(ctx, tab, fm, path, group, codec, preds,
                                aggs, nulls, what)


# ---- the wrapper ------------------------------------------------------------
def test_literal_type_does_not_pick_the_field(ctx, tabs):
    """an int or np.float32 literal on an f32 column is the float literal"""
    fm = fmx.matrix("odd_t33")
    tab = tabs["odd_t33", "for"]
    _, ga = gpu_specs("for", (), AGGS_ROWS)
    for op, lits, hi in ((cmx.LT, (1.0, 1, np.float32(1.0), np.int64(1)), 0),
                         (cmx.GE, (-100.0, -100, np.float32(-100.0)), 0),
                         (cmx.EQ, (0.0, 0, np.float32(-0.0)), 0),
                         (cmx.BETWEEN, (-100.0, -100, np.float32(-100)), 1)):
        ri, _, _, rpassed, _ = fm.ref("kmod", (("fl", op, lits[0], hi),),
                                      AGGS_ROWS)
        assert 0 < rpassed < fm.rows
        for lo in lits:
            for h in (hi, float(hi), np.float32(hi)):
                i64, _, passed = ctx.scan_agg(
                    tab, COL["kmod_for"], fmx.NKMOD,
                    [(COL["fl"], op, lo, h)], ga)
                what = f"op {op} lo {lo!r} hi {h!r}"
                assert passed == rpassed, what
                assert np.array_equal(i64, ri), what


class NoLibrary:
    def __getattr__(self, name):
        raise AssertionError(f"the library was called: {name}")


@pytest.mark.parametrize("col", ["m", "key_raw", "key_for", "flabs"])
def test_float_literal_on_integer_column_raises(ctx, tabs, monkeypatch, col):
    """ValueError from every entry before anything reaches the library"""
    tab = tabs["odd_t33", "for"]
    aggs = [(0, fmx.COUNT)]
    g = COL["kmod_for"]
    entries = (
        lambda p: ctx.scan_agg(tab, g, fmx.NKMOD, p, aggs),
        lambda p: ctx.scan_agg_hash(tab, g, 2048, p, aggs),
        lambda p: ctx.scan_agg_hash_str(tab, 0, 2048, p, aggs),
        lambda p: ctx.scan_agg_nullkey(tab, g, fmx.NKMOD, p, aggs),
        lambda p: ctx.scan_agg_hash_nullkey(tab, g, 2048, p, aggs),
        lambda p: ctx.scan_agg_hash_multi(tab, [g], 2048, p, aggs),
        lambda p: ctx.scan_topn(tab, g, 5, p))
    monkeypatch.setattr(ctx, "_lib", NoLibrary())
    for bad in ((cmx.LT, 5.0, 0), (cmx.GE, 0.5, 0),
                (cmx.EQ, np.float32(1.0), 0), (cmx.BETWEEN, 1, 2.0)):
        for entry in entries:
            with pytest.raises(ValueError):
                entry([(COL["fl"], cmx.GE, 0.0, 0.0), (COL[col],) + bad])
