"""CPU proof of the f32 predicate matrix (tests/f32_matrix.py): the cases
cover what they claim, the four mutants of the reference are told from it
in every region of the table, the SUM_F64 may-assert masks cover the groups
that matter, and the wrapper picks the literal field by the column's type.
No GPU."""

import ctypes

import numpy as np
import pytest

import agg_matrix as amx
import col_matrix as cmx
import f32_matrix as fmx
import serenedb_amd as sa

geoms = pytest.mark.parametrize("geom", fmx.GEOMS)
PLANES = ((), ("fl",))


# ---- the column -----------------------------------------------------------
@geoms
def test_fl_holds_every_ladder_value_everywhere(geom):
    fm = fmx.matrix(geom)
    mx = fm.mx
    assert sorted(fmx.ORDER) == list(range(fmx.NLAD))
    assert len(fmx.CASES) == len({c[0] for c in fmx.CASES})
    every = set(range(fmx.NLAD))
    row = np.arange(fm.rows)
    for lane in range(4):                       # quad loop, pair loop
        assert set(fm.lad[row % 4 == lane].tolist()) == every
    for k in range(amx.NKMOD):
        assert set(fm.lad[fm.am.kmod == k].tolist()) == every
    for region in ("rg_last", "rg_first"):
        assert set(fm.lad[fm.regions[region]].tolist()) == every
    for lr in (0, 8191, 8192, mx.group_rows - 1):   # staged chunk edges
        if lr < mx.group_rows:
            sel = (row % mx.group_rows == lr) & (row < fm.rows - 97)
            assert set(fm.lad[sel].tolist()) == every
    # bit patterns: the ladder's, and every NaN of NAN_BITS
    nan = fm.lad == fmx.NLAD - 1
    assert np.array_equal(fm.fl_bits[~nan], fmx.LADDER[fm.lad[~nan]])
    assert set(fm.fl_bits[nan].tolist()) == set(amx.NAN_BITS)
    assert np.isnan(fm.fl[nan]).all() and not np.isnan(fm.fl[~nan]).any()
    # the rows the region conditions rest on
    sub = {5, 6, 9, 10}
    assert int(fm.lad[0]) in sub | {7, 8}
    tail = fm.lad[fm.regions["final"]].tolist()
    assert len(tail) == (fm.rows & 3) >= 2
    assert tail[-1] == 16 and tail[-2] in sub
    if geom == "chunk":
        assert tail[0] in (7, 8)
    # flabs names |fl|
    a = np.abs(fm.fl)
    assert np.array_equal(fm.flabs == fmx.RANK_INF, np.isinf(a))
    assert np.array_equal(fm.flabs == 8, nan)
    assert np.array_equal(fm.flabs == 0, a == 0)


@geoms
def test_planes(geom):
    fm = fmx.matrix(geom)
    v = fm.valid["fl"]
    assert 0.23 < 1 - v.mean() < 0.27
    for rows in fm.regions.values():
        assert v[rows].all()
    assert 0.10 < 1 - fm.valid["key"].mean() < 0.15
    words = fm.validity_words("fl")
    assert len(words) == (fm.rows + 63) // 64
    r = np.arange(fm.rows)
    got = (words[r >> 6] >> (r & 63).astype(np.uint64)) & np.uint64(1)
    assert np.array_equal(got.astype(bool), v)


# ---- the cases --------------------------------------------------------------
@geoms
def test_case_coverage(geom):
    """every case passes and rejects a valid row (the declared "none" cases
    pass nothing, ISNULL / NOTNULL read the plane alone); and the NULL rows
    are poison: some of them store a value that passes"""
    fm = fmx.matrix(geom)
    v = fm.valid["fl"]
    kinds = {"some": 0, "none": 0, "null": 0}
    for case in fmx.CASES:
        name, op, _, _, kind = case
        kinds[kind] += 1
        preds = fm.case_preds(case)
        bare = fm.pred_mask(preds)
        planed = fm.pred_mask(preds, ("fl",))
        if kind == "null":
            want = {fmx.ISNULL: (np.zeros_like(v), ~v),
                    fmx.NOTNULL: (np.ones_like(v), v)}[op]
            assert np.array_equal(bare, want[0]), name
            assert np.array_equal(planed, want[1]), name
            continue
        assert np.array_equal(planed, bare & v), name
        if kind == "none":
            assert not bare.any(), name
            continue
        assert planed.any() and (~bare & v).any(), name
        assert (bare & ~v).any(), name + ": no NULL row is poison"
    # none: NaN and -NaN under three ops, LT -inf, three empty BETWEENs
    assert kinds == {"some": 57, "none": 10, "null": 2}
    # the same through col_matrix's own statement of the semantics
    for case in fmx.CASES[::7]:
        _, op, lo, hi, _ = case
        x = fm.fl
        with np.errstate(invalid="ignore"):
            want = {cmx.LT: x < np.float32(lo), cmx.GE: x >= np.float32(lo),
                    cmx.BETWEEN: (x >= np.float32(lo)) & (x <= np.float32(hi)),
                    cmx.EQ: x == np.float32(lo)}.get(op)
        if want is not None:
            assert np.array_equal(fm.pred_mask(fm.case_preds(case)), want)


def test_named_semantics():
    """the sentences of the contract, on the 17 ladder values"""
    bits = fmx.LADDER
    L = {i: fmx.lit(int(b)) for i, b in enumerate(bits)}

    def passing(op, lo, hi=0.0):
        return set(np.flatnonzero(fmx.f32_compare(bits, op, lo, hi)).tolist())
    assert passing(fmx.EQ, L[7]) == passing(fmx.EQ, L[8]) == {7, 8}
    assert passing(fmx.BETWEEN, L[8], L[7]) == {7, 8}
    assert passing(fmx.BETWEEN, L[9], L[10]) == {9, 10}
    assert passing(fmx.EQ, L[9]) == {9} and passing(fmx.LT, L[9]) == set(
        range(9))
    assert passing(fmx.BETWEEN, L[0], L[15]) == set(range(16))
    assert passing(fmx.BETWEEN, L[15], L[15]) == {15}
    assert passing(fmx.BETWEEN, L[12], L[3]) == set()
    for op in (fmx.LT, fmx.GE, fmx.EQ):
        assert passing(op, L[16]) == set()
        assert 16 not in passing(op, L[12])
    assert passing(fmx.BETWEEN, L[16], L[12]) == set()
    assert passing(fmx.BETWEEN, L[3], L[16]) == set()
    assert passing(fmx.LT, 1) == passing(fmx.LT, 1.0) == set(range(12))


# ---- the mutants ------------------------------------------------------------
@geoms
@pytest.mark.parametrize("mutant", fmx.MUTANTS)
def test_mutants_are_killed_in_every_region(geom, mutant):
    """each mutant disagrees with the reference on at least one case inside
    the final rows & 3 rows, the last rows of the row groups, their first
    rows, and row 0 — bare and with the plane attached; and in at least one
    case it passes another NUMBER of rows, which is what fails every GPU
    path (each asserts rows_passed) if the mutant stands in for the
    reference"""
    fm = fmx.matrix(geom)
    for nulls in PLANES:
        killed = {r: [] for r in fm.regions}
        count_differs = []
        for case in fmx.CASES:
            if case[4] == "null":
                continue
            preds = fm.case_preds(case)
            ref = fm.pred_mask(preds, nulls)
            mut = fm.pred_mask(preds, nulls, mutant)
            for region, rows in fm.regions.items():
                if (ref[rows] != mut[rows]).any():
                    killed[region].append(case[0])
            if ref.sum() != mut.sum():
                count_differs.append(case[0])
        for region, by in killed.items():
            assert by, f"{mutant} survives in {region} of {geom} {nulls}"
        assert count_differs, f"{mutant} passes the same row counts"


# ---- SUM_F64 ----------------------------------------------------------------
def test_lsb_exponent():
    bits = np.array([0x00000001, 0x007FFFFF, 0x00800000, 0x3F800000,
                     0x3FC00000, 0x7F7FFFFF, 0x80000002, 0xC2C80000],
                    dtype=np.uint32)
    want = [-149, -149, -126, 0, -1, 104, -148, 2]
    assert fmx._lsb_exp(bits).tolist() == want
    for b, e in zip(bits.tolist(), want):
        v = abs(float(fmx.lit(b)))
        assert (v / 2.0 ** e) % 2 == 1          # an odd multiple of 2^e


@geoms
def test_sum_asserted_groups(geom):
    fm = fmx.matrix(geom)
    am = fm.am
    cases = {n: (g, p) for n, g, p in fmx.SUM_CASES}
    # by kmod, every row: the special groups of fx
    group, preds = cases["all_by_kmod"]
    for nulls in ((), ("fx", "fl")):
        ref, ok = fm.sum_ref(group, preds, nulls)["fx"]
        g = amx.FX_GROUPS
        for name in ("all_nan", "neg_nan_finite", "neg_inf", "pos_inf"):
            assert ok[g[name]], name
        assert np.isnan(ref[g["all_nan"]])
        assert np.isnan(ref[g["neg_nan_finite"]])
        assert ref[g["neg_inf"]] == -np.inf and ref[g["pos_inf"]] == np.inf
        assert ok[g["zeros"]] and ref[g["zeros"]] == 0
        if nulls:                   # no value at all under the plane
            for k in amx.ALL_NULL:
                assert ok[k] and ref[k] == 0
        # fl: a NaN in every kmod group
        ref, ok = fm.sum_ref(group, preds, nulls)["fl"]
        assert ok.all() and np.isnan(ref).all()
    # by key, only the +-inf rows of fl: inf - inf, a NaN made by the sum
    group, preds = cases["inf_rows_by_key"]
    for nulls in ((), ("fx", "fl")):
        ref, ok = fm.sum_ref(group, preds, nulls)["fl"]
        sel = fm.mask(preds, nulls)
        if nulls:
            sel = sel & fm.valid["fl"]
        assert not np.isnan(fm.fl[sel]).any() and np.isinf(fm.fl[sel]).all()
        d, ng = fm.groups[group]
        pos = np.bincount(d[sel & (fm.fl > 0)], minlength=ng) > 0
        neg = np.bincount(d[sel & (fm.fl < 0)], minlength=ng) > 0
        assert (pos & neg).sum() >= 1 and ok[pos | neg].all()
        assert np.isnan(ref[pos & neg]).all()
        assert (ref[pos & ~neg] == np.inf).all()
        assert (ref[neg & ~pos] == -np.inf).all()
        assert (pos & ~neg).any() and (neg & ~pos).any()
    # positive subnormals only: nonzero, exact
    for name in ("pos_subnormals_by_key", "pos_subnormals_by_kmod"):
        group, preds = cases[name]
        for nulls in ((), ("fl",)):
            ref, ok = fm.sum_ref(group, preds, nulls)["fl"]
            d, ng = fm.groups[group]
            present = np.bincount(d[fm.mask(preds, nulls)], minlength=ng) > 0
            assert ok.all() and present.any()
            assert (ref[present] > 0).all() and (ref[present] < 1e-30).all()
            # exact: an integer count of 2^-149, found in integers too
            sel = fm.mask(preds, nulls)
            want = np.zeros(ng, dtype=np.int64)
            np.add.at(want, d[sel], fm.fl_bits[sel].astype(np.int64))
            assert np.array_equal(np.ldexp(ref, 149), want.astype(np.float64))
    # an order-dependent sum is NOT asserted: +-FLT_MAX among subnormals
    # (FLT_MAX / 2^-149 is far past 2^53 units)
    ref, ok = fm.sum_ref("kmod", cases["all_by_kmod"][1])["fx"]
    k = amx.FX_GROUPS["denorm_fltmax"]
    assert not ok[k] and np.isfinite(ref[k])


def test_check_sums():
    ref = np.array([np.nan, np.inf, -np.inf, 1.5, 2.0])
    ok = np.array([True, True, True, True, False])
    neg_nan = np.frombuffer(np.uint64(0xFFF8000000000001).tobytes(),
                            dtype=np.float64)[0]
    fmx.check_sums(np.array([neg_nan, np.inf, -np.inf, 1.5, 99.0]), ref, ok,
                   "")
    for bad in ([1.0, np.inf, -np.inf, 1.5, 2.0],
                [np.nan, -np.inf, -np.inf, 1.5, 2.0],
                [np.nan, np.inf, np.nan, 1.5, 2.0],
                [np.nan, np.inf, -np.inf, 1.5000000000000002, 2.0]):
        with pytest.raises(AssertionError):
            fmx.check_sums(np.array(bad), ref, ok, "")


@geoms
def test_references_agree_with_agg_matrix(geom):
    """COUNT / COUNT_COL / SUM_I64 of this file against agg_matrix's own
    references on a query both can state"""
    fm = fmx.matrix(geom)
    preds = (("fx", cmx.BETWEEN, -1.0, 1.0),)
    aggs = ((None, fmx.COUNT), ("m", fmx.COUNT_COL), ("m", fmx.SUM_I64),
            ("f", fmx.SUM_F64))
    for group in ("key", "kmod"):
        ri, rf, rpassed, rpresent = fm.am.ref_dense(group, preds, aggs,
                                                    ("m",))
        i64, f64, ok, passed, present = fm.ref(group, preds, aggs, ("m",))
        assert passed == rpassed and np.array_equal(present, rpresent)
        assert np.array_equal(i64, ri)
        assert ok.all() and np.array_equal(f64, rf)     # f: eighths, exact
    rows, n = fm.ref_topn(preds, (), 65536)
    assert n == passed and len(rows) == min(n, 65536)
    key = fm.mx.key[rows.astype(np.int64)]
    dkey, drow = np.diff(key), np.diff(rows.astype(np.int64))
    assert np.all((dkey > 0) | ((dkey == 0) & (drow > 0)))


# ---- the wrapper: the column's type picks the literal field -------------
def test_pred_specs_fields_by_column_type():
    ctx = sa.GpuContext.__new__(sa.GpuContext)      # no device, no library
    ctx._ctx = None
    ctx._table_f32 = {7: (False, True)}
    tab = ctypes.c_void_p(7)
    one = np.float32(1.0)

    def spec(p):
        s = ctx._pred_specs([p], tab)[0]
        return s.col, s.op, s.ilo, s.ihi, s.flo, s.fhi
    for lo in (1, 1.0, one, np.int64(1), np.float64(1.0)):
        assert spec((1, cmx.LT, lo, 0)) == (1, cmx.LT, 0, 0, 1.0, 0.0)
    assert spec((1, cmx.BETWEEN, -100, one)) == (1, 3, 0, 0, -100.0, 1.0)
    sub = fmx.lit(fmx.SUB_MIN)
    assert spec((1, cmx.EQ, sub, 0.0))[4] == sub > 0
    assert spec((0, cmx.BETWEEN, np.int64(-5), 5)) == (0, 3, -5, 5, 0.0, 0.0)
    assert spec((0, cmx.EQ, cmx.I64_MIN, 0))[2] == cmx.I64_MIN
    assert spec((0, cmx.ISNULL, 0, 0)) == (0, 5, 0, 0, 0.0, 0.0)
    # without a table (a hand-made call) the literal's type is all there is
    assert ctx._pred_specs([(0, cmx.GE, 0, 0)])[0].ilo == 0
    assert ctx._pred_specs([(0, cmx.LT, 2.5, 0)])[0].flo == 2.5
    for bad in ((0, cmx.LT, 5.0, 0), (0, cmx.GE, 0.5, 0), (0, cmx.EQ, one, 0),
                (0, cmx.BETWEEN, 1, 2.0), (0, cmx.BETWEEN, 1.5, 2),
                (0, cmx.LT, np.float64(3.0), 0)):
        with pytest.raises(ValueError):
            ctx._pred_specs([bad], tab)
