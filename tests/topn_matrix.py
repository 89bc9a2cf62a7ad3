"""ORDER BY col [DESC] LIMIT k matrix: the order columns and the numpy
reference of GpuContext.scan_topn, built on the column-codec, aggregate and
NULL-key matrices (tests/col_matrix.py, agg_matrix.py, nullkey_matrix.py;
geometries agg_matrix.GEOMS: "chunk" with 544,003 rows and "odd_t33" with
33,858). tests/test_topn_matrix.py proves this file on the CPU;
tests/test_gpu_topn_matrix.py runs the GPU against it.

Order columns (name: values, validity plane):

  m        the FoR width matrix, loaded raw and FoR; col_matrix's plane
           valid["m"]. Holds INT64_MAX and INT64_MIN many times over (every
           group of those base kinds), so its top is one long tie that ends
           inside a row group.
  keyp     the POISONED `key` arrays with plane `key`: a NULL row stores an
           int64 extreme (raw), -1, a live key or a value no valid row holds.
           Nothing a NULL row stores may rank.
  key      `key` clean, no plane: 1088 small values whose codes differ only in
           their low bits, so the radix select has to refine digit by digit.
  f        float32 eighths, no plane.
  fx       float32 special values (NaNs of every kind, both zeros, both
           infinities, denormals, +-FLT_MAX) with plane valid["fx"].
  c7       7 in every row: ordered purely by row.

The reference is a numpy lexsort over (NULL class, rank code, row) with the
rank code restated here: a u64 where bigger ranks first, i64 DESC = x ^ 2^63
and ASC its complement, f32 the 32-bit total-order key (agg_matrix.f32_key),
complemented within 32 bits for ASC. Nothing asks the code under test for an
expected value.
"""

import functools

import numpy as np

import agg_matrix as amx
import col_matrix as cmx
import nullkey_matrix as nkx

GEOMS = amx.GEOMS
I64_MIN, I64_MAX = cmx.I64_MIN, cmx.I64_MAX
MAX_K = 65536                   # SDB_TOPN_MAX_K
DIGIT_BITS = 11
ORDER_COLS = ("m", "keyp", "key", "f", "fx", "c7")
F32_COLS = ("f", "fx")
PLANED = ("m", "keyp", "fx")     # the columns with a validity plane
SIGN = np.uint64(1 << 63)


class TopnMatrix:
    def __init__(self, name):
        self.name = name
        self.nk = nk = nkx.matrix(name)
        self.am, self.mx = nk.am, nk.mx
        self.rows = nk.rows
        self.group_rows = self.mx.group_rows
        self.c7 = np.full(self.rows, 7, dtype=np.int64)
        self.c7.setflags(write=False)
        # the values a valid row holds (the poisoned arrays equal `key` there)
        self.vals = {"m": self.mx.m.vals, "keyp": self.mx.key,
                     "key": self.mx.key, "f": self.mx.f, "fx": self.am.fx,
                     "c7": self.c7}

    def plane(self, col):
        """the plane attached to a column in the GPU tables, or None"""
        return {"m": self.mx.valid["m"], "keyp": self.nk.valid["key"],
                "fx": self.am.valid["fx"]}.get(col)

    def valid(self, order):
        """the order column's plane (True = valid), all True without one"""
        v = self.plane(order)
        return np.ones(self.rows, dtype=bool) if v is None else v

    def validity_words(self, col):
        return self.nk.validity_words(None, self.plane(col))

    def stored(self, order, codec):
        """the array a table column holds for this order column"""
        if order == "keyp":
            return self.nk.poisoned["key", codec]
        return self.vals[order]

    def bits(self, order):
        """f32 order column as uint32 bit patterns"""
        return np.ascontiguousarray(self.vals[order]).view(np.uint32)

    def codes(self, order, desc):
        """the rank code of every row, bigger ranks first (NULL rows too:
        the caller masks them out)"""
        if order in F32_COLS:
            k = amx.f32_key(self.bits(order)).astype(np.uint32)
            return (k if desc else ~k).astype(np.uint64)
        c = self.vals[order].view(np.uint64) ^ SIGN
        return c if desc else ~c

    @functools.lru_cache(maxsize=None)
    def pred_mask(self, preds):
        """rows passing the AND of preds [(col, op, lo, hi)] under SQL
        three-valued logic with the planes of PLANED attached: a compare
        drops the column's NULL rows, ISNULL / NOTNULL read the plane alone.
        ("kstr", PREFIX, b"..", 0) is the string slot made of kmod."""
        mask = np.ones(self.rows, dtype=bool)
        for col, op, lo, hi in preds:
            if col == "kstr":
                assert op == nkx.PREFIX
                mask &= self.nk.str_mask(lo)
                continue
            valid = self.plane(col)
            if op == cmx.ISNULL:
                mask &= ~valid if valid is not None else False
                continue
            if op == cmx.NOTNULL:
                if valid is not None:
                    mask &= valid
                continue
            if col in ("keyp", "c7"):
                x = self.vals[col]
                mask &= {cmx.LT: x < lo, cmx.GE: x >= lo,
                         cmx.BETWEEN: (x >= lo) & (x <= hi),
                         cmx.EQ: x == lo}[op]
            else:
                mask &= self.am.pred_mask(((col, op, lo, hi),))
            if valid is not None:
                mask &= valid
        mask.setflags(write=False)
        return mask

    @functools.lru_cache(maxsize=None)
    def ranking(self, order, preds, desc, nulls_first):
        """every passing row in result order, and which of them are NULL"""
        mask = self.pred_mask(tuple(preds))
        rows = np.flatnonzero(mask)
        isnull = ~self.valid(order)[rows]
        code = np.where(isnull, np.uint64(0), self.codes(order, desc)[rows])
        cls = isnull != nulls_first     # 0 sorts first
        o = np.lexsort((rows, ~code, cls))
        rows, isnull = rows[o].astype(np.uint64), isnull[o]
        rows.setflags(write=False)
        isnull.setflags(write=False)
        return rows, isnull

    def ref(self, order, preds, k, desc=False, nulls_first=False):
        """(rows u64 [n], vals [n], isnull [n], rows_passed), laid out like
        GpuContext.scan_topn; vals int64, or canonical uint32 bit patterns
        for an f32 order column; 0 where NULL"""
        rows, isnull = self.ranking(order, tuple(preds), bool(desc),
                                    bool(nulls_first))
        passed = len(rows)
        rows, isnull = rows[:k], isnull[:k]
        if order in F32_COLS:
            b = self.bits(order)[rows.astype(np.int64)].copy()
            b[(b & np.uint32(0x7FFFFFFF)) > np.uint32(0x7F800000)] = \
                amx.CANON_NAN
            vals = np.where(isnull, np.uint32(0), b)
        else:
            vals = np.where(isnull, 0, self.vals[order][rows.astype(np.int64)])
        return rows, vals, isnull, passed

    def witness(self, order, preds, k, desc=False, nulls_first=False):
        """The second witness: the same rows by a plain-Python sorted() over
        (NULL class, value, row) tuples of Python ints — signed ints negated
        for DESC, f32 through f32_key_py; no rank code."""
        rows = np.flatnonzero(self.pred_mask(tuple(preds))).tolist()
        valid = self.valid(order)
        if order in F32_COLS:
            raw = self.bits(order)
            value = lambda r: amx.f32_key_py(int(raw[r]))   # noqa: E731
        else:
            raw = self.vals[order]
            value = lambda r: int(raw[r])                   # noqa: E731
        keyed = []
        for r in rows:
            null = not valid[r]
            v = 0 if null else (-value(r) if desc else value(r))
            keyed.append((null != nulls_first, v, r))
        return [r for _, _, r in sorted(keyed)[:k]]

    def kth_ties(self, order, preds, k, desc):
        """(passing non-NULL rows whose code equals the k-th value's code,
        passing non-NULL rows)"""
        mask = self.pred_mask(tuple(preds)) & self.valid(order)
        c = np.sort(self.codes(order, desc)[mask])[::-1]
        if k > len(c):
            return 0, len(c)
        return int((c == c[k - 1]).sum()), len(c)


@functools.lru_cache(maxsize=None)
def matrix(name):
    return TopnMatrix(name)


# ---- the tie-arm cases of the GPU tests ----------------------------------
# (geometry, order column, desc, nulls_first, k, kind): run under
# SDB_TOPN_CAND_CAP=1, i.e. a capacity of k + group_rows. kind "ties": the
# rows equal to the k-th code exceed that capacity (c7: more than four times
# over); kind "null": the NULL class is needed.
TIE_CASES = (
    ("chunk", "m", True, False, 1000, "ties"),
    ("odd_t33", "c7", False, False, 100, "ties"),
    ("odd_t33", "c7", False, False, 1025, "ties"),
    ("chunk", "m", False, True, 100, "null"),
    ("odd_t33", "m", False, True, 100, "null"),
)
