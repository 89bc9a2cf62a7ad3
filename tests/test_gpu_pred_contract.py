"""One predicate contract on every columnar scan entry.

The seven entries that take a pushed predicate list (sdb_gpu_scan_agg,
_nullkey, _hash, _hash_nullkey, _hash_multi, _hash_str and sdb_gpu_scan_topn)
resolve it through one routine, so each must reject the same bad lists with
SDB_ERR_INVALID, before anything runs, and give the oracle's answer for a
valid STRMASK + BETWEEN pair. The entries are called through the ctypes
library directly: the Python wrappers never pass a NULL list.

Table: 5 rows; a raw i64 key, a FoR i64 column with group_rows 4 (row 4 is
the 1-row odd last group) and an f32 column; one raw string slot.
"""
import ctypes as C

import numpy as np
import pytest

import serenedb_amd as sa
from oracle import pyoracle as po

pytestmark = pytest.mark.gpu

SDB_ERR_INVALID = -1
NOTNULL, STRMASK, PREFIX = 6, 7, 8
MAX_PREDS = 4          # SCAN_MAX_PREDS
MAX_STRCOLS = 4        # SDB_MAX_STRCOLS

KEYS = np.array([0, 1, 2, 1, 0], dtype=np.int64)
V1 = np.array([10, 20, 30, 40, 50], dtype=np.int64)
V2 = np.array([1.5, 2.5, 3.5, 4.5, 5.5], dtype=np.float32)
STRS = ["ab", "ac", "b", "ad", "ae"]
NCOLS, NGROUPS, MAXG = 3, 3, 8
AGGS = [(0, "count"), (1, "sum_i64"), (2, "sum_f64")]

ENTRIES = ["scan_agg", "scan_agg_nullkey", "scan_agg_hash",
           "scan_agg_hash_nullkey", "scan_agg_hash_multi",
           "scan_agg_hash_str", "scan_topn"]


class Bench:
    """context + table + every output buffer an entry writes"""

    def __init__(self):
        self.ctx = sa.GpuContext(0)
        self.lib = self.ctx._lib
        self.tab = self.ctx.load_table([KEYS, V1, V2], ["raw", "for", "raw"],
                                       group_rows=4)
        off, blob = sa.encode_col_str_raw(STRS)
        self.ctx.attach_strcol(self.tab, 0, off, blob)
        self.ctx.attach_strcol(self.tab, 1, off, blob)  # slot 1: no mask set
        self.ctx.strpred_mask(self.tab, 0, "prefix", "a")
        na = len(AGGS)
        self.aa = self.ctx._agg_specs(AGGS)
        self.out = (self.ctx._AggResult * ((MAXG + 1) * na))()
        self.null_out = (self.ctx._AggResult * na)()
        self.keys_out = np.zeros(MAXG, dtype=np.int64)
        self.keynull = np.zeros(MAXG, dtype=np.uint32)
        self.rows_out = np.zeros(MAXG, dtype=np.uint64)
        self.isnull = np.zeros(MAXG, dtype=np.uint8)
        self.ng = C.c_uint64(0)
        self.passed = C.c_uint64(0)
        self.nulls = C.c_uint64(0)
        self.n = C.c_uint64(0)

    def close(self):
        self.ctx.free_table(self.tab)
        self.ctx.close()

    def call(self, entry, pa, npreds):
        """rc of one entry over the predicate list (pa, npreds); pa None is
        a NULL pointer"""
        c, lib, tab = self.ctx._ctx, self.lib, self.tab
        npr, na = C.c_uint32(npreds), C.c_uint32(len(AGGS))
        kp = self.keys_out.ctypes.data_as(C.POINTER(C.c_int64))
        ng, passed, nulls = (C.byref(self.ng), C.byref(self.passed),
                             C.byref(self.nulls))
        if entry == "scan_agg":
            return lib.sdb_gpu_scan_agg(
                c, tab, C.c_uint32(0), C.c_uint32(NGROUPS), pa, npr, self.aa,
                na, self.out, passed)
        if entry == "scan_agg_nullkey":
            return lib.sdb_gpu_scan_agg_nullkey(
                c, tab, C.c_uint32(0), C.c_uint32(NGROUPS), pa, npr, self.aa,
                na, self.out, passed, nulls)
        if entry == "scan_agg_hash":
            return lib.sdb_gpu_scan_agg_hash(
                c, tab, C.c_uint32(0), C.c_uint64(MAXG), pa, npr, self.aa, na,
                kp, self.out, ng, passed)
        if entry == "scan_agg_hash_nullkey":
            return lib.sdb_gpu_scan_agg_hash_nullkey(
                c, tab, C.c_uint32(0), C.c_uint64(MAXG), pa, npr, self.aa, na,
                kp, self.out, ng, passed, self.null_out, nulls)
        if entry == "scan_agg_hash_multi":
            gc = (C.c_uint32 * 1)(0)
            return lib.sdb_gpu_scan_agg_hash_multi(
                c, tab, gc, C.c_uint32(1), C.c_uint64(MAXG), pa, npr, self.aa,
                na, kp, self.keynull.ctypes.data_as(C.POINTER(C.c_uint32)),
                self.out, ng, passed)
        if entry == "scan_agg_hash_str":
            return lib.sdb_gpu_scan_agg_hash_str(
                c, tab, C.c_uint32(0), C.c_uint64(MAXG), pa, npr, self.aa, na,
                kp, self.out, ng, passed)
        assert entry == "scan_topn"
        return lib.sdb_gpu_scan_topn(
            c, tab, C.c_uint32(1), C.c_uint32(0), C.c_uint32(MAXG), pa, npr,
            self.rows_out.ctypes.data_as(C.POINTER(C.c_uint64)), self.out,
            self.isnull.ctypes.data_as(C.POINTER(C.c_uint8)),
            C.byref(self.n), passed, None)

    def specs(self, preds):
        return (self.ctx._PredSpec * max(len(preds), 1))(*[
            self.ctx._PredSpec(col, op, lo, hi, 0, 0)
            for col, op, lo, hi in preds])

    def aggs(self, n):
        return self.ctx._unpack_aggs(self.out, n, len(AGGS))


@pytest.fixture(scope="module")
def bench():
    b = Bench()
    yield b
    b.close()


GOOD = (1, 3, 0, 100)  # BETWEEN on the FoR column: every row passes

BAD_LISTS = {
    "npreds_5": ([GOOD] * (MAX_PREDS + 1), MAX_PREDS + 1),
    "col_eq_ncols": ([(NCOLS, 3, 0, 100)], 1),
    "op_prefix": ([(1, PREFIX, 0, 0)], 1),
    "op_past_enum": ([(1, 11, 0, 0)], 1),
    "op_bad_after_good": ([GOOD, (1, NOTNULL + 3, 0, 0)], 2),
    "strmask_no_mask_set": ([(1, STRMASK, 0, 0)], 1),
    "strmask_slot_4": ([(MAX_STRCOLS, STRMASK, 0, 0)], 1),
}


@pytest.mark.parametrize("entry", ENTRIES)
def test_bad_predicate_lists_are_invalid(bench, entry):
    assert bench.call(entry, None, 1) == SDB_ERR_INVALID, "preds = NULL"
    for name, (preds, npreds) in BAD_LISTS.items():
        assert bench.call(entry, bench.specs(preds), npreds) == \
            SDB_ERR_INVALID, name
    # the same entry still answers a good list, NULL with no predicate too
    assert bench.call(entry, bench.specs([GOOD]), 1) == 0
    assert bench.passed.value == len(KEYS)
    assert bench.call(entry, None, 0) == 0
    assert bench.passed.value == len(KEYS)


@pytest.fixture(scope="module")
def expected():
    """oracle: the string mask by pyoracle.str_pred_mask, the BETWEEN by the
    C oracle's own scan over the rows the mask keeps"""
    m = po.str_pred_mask(STRS, "prefix", "a")
    cnt, si, sf, passed = po.scan_agg(KEYS[m], V1[m], V2[m], NGROUPS,
                                      pred_op=3, lo=20, hi=50)
    sel = m & (V1 >= 20) & (V1 <= 50)
    assert passed == sel.sum() == 3 and sel[4]  # the odd last group passes
    return dict(cnt=cnt, si=si, sf=sf, passed=passed, sel=sel)


VALID = [(0, STRMASK, 0, 0), (1, 3, 20, 50)]


@pytest.mark.parametrize("entry", ENTRIES)
def test_strmask_and_between_match_oracle(bench, expected, entry):
    e = expected
    assert bench.call(entry, bench.specs(VALID), 2) == 0
    assert bench.passed.value == e["passed"]
    live = np.nonzero(e["cnt"])[0]
    if entry in ("scan_agg", "scan_agg_nullkey"):
        i64, f64 = bench.aggs(NGROUPS + (entry == "scan_agg_nullkey"))
        np.testing.assert_array_equal(i64[:NGROUPS, 0], e["cnt"])
        np.testing.assert_array_equal(i64[:NGROUPS, 1], e["si"])
        np.testing.assert_array_equal(f64[:NGROUPS, 2], e["sf"])
        if entry == "scan_agg_nullkey":  # no key plane: an empty NULL group
            assert bench.nulls.value == 0
            assert not i64[NGROUPS].any() and not f64[NGROUPS].any()
    elif entry == "scan_topn":
        n = bench.n.value
        rows = np.nonzero(e["sel"])[0]  # V1 ascends with the row number
        np.testing.assert_array_equal(bench.rows_out[:n], rows)
        i64, _ = bench.ctx._unpack_aggs(bench.out, n, 1)
        np.testing.assert_array_equal(i64[:, 0], V1[rows])
        assert not bench.isnull[:n].any()
    elif entry == "scan_agg_hash_str":
        # groups by the FNV-1a hash of the row's string, signed ascending
        sel = np.nonzero(e["sel"])[0]
        h = np.array([po.fnv1a64(STRS[r].encode()) for r in sel],
                     dtype=np.uint64).view(np.int64)
        order = np.argsort(h)
        n = bench.ng.value
        i64, f64 = bench.aggs(n)
        np.testing.assert_array_equal(bench.keys_out[:n], h[order])
        np.testing.assert_array_equal(i64[:, 0], np.ones(n, dtype=np.int64))
        np.testing.assert_array_equal(i64[:, 1], V1[sel][order])
        np.testing.assert_array_equal(f64[:, 2],
                                      V2[sel][order].astype(np.float64))
    else:  # the three i64-key hash entries: the groups with a passing row
        n = bench.ng.value
        i64, f64 = bench.aggs(n)
        np.testing.assert_array_equal(bench.keys_out[:n], live)
        np.testing.assert_array_equal(i64[:, 0], e["cnt"][live])
        np.testing.assert_array_equal(i64[:, 1], e["si"][live])
        np.testing.assert_array_equal(f64[:, 2], e["sf"][live])
        if entry == "scan_agg_hash_nullkey":
            assert bench.nulls.value == 0
        if entry == "scan_agg_hash_multi":
            assert not bench.keynull[:n].any()
