"""CPU proofs for the ORDER BY ... LIMIT k matrix (tests/topn_matrix.py): the
numpy reference against a plain-Python sorted() witness, the facts about the
order columns that the GPU cases of tests/test_gpu_topn_matrix.py rely on, and
the public surface of the feature. Needs no GPU."""

import os
import re

import numpy as np
import pytest

import agg_matrix as amx
import col_matrix as cmx
import nullkey_matrix as nkx
import serenedb_amd as sa
import topn_matrix as tnx

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
geoms = pytest.mark.parametrize("geom", tnx.GEOMS)
INT64_MAX_RGS = [1, 6, 11, 16, 21, 26, 31]


def test_geometries():
    assert tnx.matrix("chunk").rows == 544003
    assert tnx.matrix("odd_t33").rows == 33858
    for g in tnx.GEOMS:
        assert (tnx.matrix(g).vals["c7"] == 7).all()


# ---- the reference against the second witness ----------------------------
WITNESS_PREDS = (
    (),
    (("m2", cmx.BETWEEN, -5, 1 << 41),),
    (("m", cmx.GE, 0, 0),),
    (("fx", cmx.GE, 0.0, 0.0),),
    (("kstr", nkx.PREFIX, b"k1", 0),),
)


@pytest.mark.parametrize("order", tnx.ORDER_COLS)
def test_reference_matches_sorted_witness(order):
    t = tnx.matrix("odd_t33")
    for preds in WITNESS_PREDS:
        for desc in (False, True):
            for nulls_first in (False, True):
                for k in (1, 64, 1000, t.rows + 5):
                    rows, vals, isnull, passed = t.ref(order, preds, k, desc,
                                                       nulls_first)
                    want = t.witness(order, preds, k, desc, nulls_first)
                    what = (order, preds, desc, nulls_first, k)
                    assert rows.tolist() == want, what
                    assert passed == int(t.pred_mask(preds).sum()), what
                    assert len(rows) == min(k, passed), what
                    r = rows.astype(np.int64)
                    assert (isnull == ~t.valid(order)[r]).all(), what
                    assert not vals[isnull].any(), what


def test_reference_f32_values_are_canonical_bits():
    t = tnx.matrix("odd_t33")
    rows, vals, isnull, _ = t.ref("fx", (), 200, desc=True)
    assert vals.dtype == np.uint32
    nan = (t.bits("fx")[rows.astype(np.int64)] & 0x7FFFFFFF) > 0x7F800000
    assert nan.any() and (vals[nan & ~isnull] == amx.CANON_NAN).all()


# ---- facts the GPU cases rely on -----------------------------------------
@geoms
def test_m_extremes(geom):
    t = tnx.matrix(geom)
    m, valid = t.vals["m"], t.valid("m")
    top = m == tnx.I64_MAX
    assert int(top.sum()) == {"chunk": 27070, "odd_t33": 525}[geom]
    assert int((top & valid).sum()) == {"chunk": 20303, "odd_t33": 395}[geom]
    assert sorted(set((np.flatnonzero(top) // t.group_rows).tolist())) == \
        INT64_MAX_RGS
    assert int((m == tnx.I64_MIN).sum()) == {"chunk": 570,
                                             "odd_t33": 357}[geom]
    # the top 11-bit digit of m's codes: four non-empty bins
    for desc in (False, True):
        top_digit = t.codes("m", desc) >> np.uint64(64 - tnx.DIGIT_BITS)
        assert len(np.unique(top_digit)) == 4


@geoms
def test_key_codes_differ_in_low_bits_only(geom):
    """all `key` codes share their top 53 bits (key < 1088 < 2^11), i.e. the
    first four 11-bit digits: a select that starts at the top learns nothing
    from them, and more than one histogram pass must run before the rows at
    or above the k-th code's prefix fit a capacity of k + group_rows"""
    t = tnx.matrix(geom)
    for desc in (False, True):
        c = t.codes("key", desc)
        assert len(np.unique(c >> np.uint64(11))) == 1
        assert len(np.unique(c >> np.uint64(64 - 4 * tnx.DIGIT_BITS))) == 1
        assert len(np.unique(c)) == len(np.unique(t.vals["key"]))
    # after ONE pass the top bin still holds every row: more than the cap
    assert t.rows > 1000 + t.group_rows


@geoms
def test_poisoned_key_holds_both_extremes_on_null_rows(geom):
    t = tnx.matrix(geom)
    null = ~t.valid("keyp")
    raw = t.stored("keyp", "raw")
    assert (raw[null] == tnx.I64_MIN).any()
    assert (raw[null] == tnx.I64_MAX).any()
    for codec in ("raw", "for"):
        a = t.stored("keyp", codec)
        assert (a[~null] == t.vals["key"][~null]).all()
        assert (a[null] != t.vals["key"][null]).any()
    v = t.vals["key"][~null]
    assert v.min() > tnx.I64_MIN and v.max() < tnx.I64_MAX


@geoms
def test_fx_special_values(geom):
    t = tnx.matrix(geom)
    b = t.bits("fx")[t.valid("fx")]
    assert ((b & 0x7FFFFFFF) > 0x7F800000).any()         # NaNs
    assert (b == 0x80000000).any() and (b == 0).any()    # both zeros
    assert (b == amx.POS_INF).any() and (b == amx.NEG_INF).any()
    # more than one NaN payload, both signs: they must all tie
    nan = b[(b & 0x7FFFFFFF) > 0x7F800000]
    assert len(np.unique(nan)) > 2 and (nan >> 31).any()


@geoms
def test_planes_are_72_to_75_percent_valid(geom):
    t = tnx.matrix(geom)
    for col in tnx.PLANED:
        assert 0.72 <= t.valid(col).mean() <= 0.75, col
    for col in ("key", "f", "c7"):
        assert t.plane(col) is None


@pytest.mark.parametrize("case", tnx.TIE_CASES, ids=lambda c: "-".join(
    str(x) for x in c))
def test_tie_arm_cases_cannot_fit(case):
    """Under SDB_TOPN_CAND_CAP=1 the capacity is its floor, k + group_rows.
    A "ties" case reaches the row-order arm because the rows equal to the
    k-th code exceed that floor: c7 by more than four times over; m DESC on
    chunk by 20,303 valid INT64_MAX rows against 17,482 (not four times: the
    column holds no longer tie)."""
    geom, order, desc, nulls_first, k, kind = case
    t = tnx.matrix(geom)
    floor = k + t.group_rows
    ties, nonnull = t.kth_ties(order, (), k, desc)
    if kind == "ties":
        assert ties > floor, (ties, floor)
        if order == "c7":
            assert ties > 4 * floor, (ties, floor)
        else:
            assert (ties, floor) == (20303, 17482)
    else:
        # the NULL class is needed: NULLS FIRST with NULL rows passing
        assert nulls_first and int((~t.valid(order)).sum()) > 0


def test_m_desc_ties_end_inside_a_row_group():
    """chunk, m DESC, k = 1000: the 1000th valid INT64_MAX row is neither
    the first nor the last such row of its row group"""
    t = tnx.matrix("chunk")
    rows, vals, isnull, _ = t.ref("m", (), 1000, desc=True)
    assert (vals == tnx.I64_MAX).all() and not isnull.any()
    last = int(rows[-1])
    rg = last // t.group_rows
    members = np.flatnonzero((t.vals["m"] == tnx.I64_MAX) & t.valid("m"))
    in_rg = members[members // t.group_rows == rg]
    assert in_rg[0] < last < in_rg[-1]


# ---- the public surface ---------------------------------------------------
def test_header_declares_topn_and_gather():
    hdr = open(os.path.join(REPO, "include", "sdb_gpu.h")).read()
    for fn in ("sdb_gpu_scan_topn", "sdb_gpu_table_gather"):
        assert re.search(r"^int\s+%s\s*\(" % fn, hdr, re.M), fn
    macros = dict(re.findall(
        r"^#define\s+(SDB_TOPN_\w+)\s+(\d+)u", hdr, re.M))
    assert macros == {"SDB_TOPN_MAX_K": "65536", "SDB_TOPN_DESC": "1",
                      "SDB_TOPN_NULLS_FIRST": "2"}
    assert "SdbTopnStats" in hdr
    assert callable(getattr(sa.GpuContext, "scan_topn"))
    assert callable(getattr(sa.GpuContext, "gather"))
    assert sa.GpuContext.TOPN_MAX_K == int(macros["SDB_TOPN_MAX_K"]) == \
        tnx.MAX_K
    assert sa.GpuContext.TOPN_DESC == 1
    assert sa.GpuContext.TOPN_NULLS_FIRST == 2
