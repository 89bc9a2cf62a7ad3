"""f32 predicate matrix: the inputs and numpy references that pin the IEEE
edges of an f32 compare (LT, GE, BETWEEN, EQ, ISNULL, NOTNULL) and of
SUM_F64 on every columnar scan path, built on the two geometries of the
aggregate matrix (tests/agg_matrix.py: "chunk" and "odd_t33" with their
columns). tests/test_f32_matrix.py proves this file on the CPU;
tests/test_gpu_f32_matrix.py runs the GPU paths against it.

Added to the agg_matrix columns:

  fl       float32, built as bit patterns: fl[r] = ORDER[(r + shift) % 17],
           ORDER a fixed permutation of the 17 amx.LADDER values (+-inf,
           +-FLT_MAX, +-100, +-1, +-FLT_MIN, the largest and smallest
           subnormal of each sign, both zeros, NaN). The NaN slot cycles
           through amx.NAN_BITS. 17 is coprime to 4, 61, 1025, 8192 and
           16482, so every lane of every vector loop, every kmod group and
           every row-group edge meets every value. ORDER and the shifts put
           a zero or subnormal in row 0 and {subnormal, NaN} in the last two
           rows (chunk: {zero, subnormal, NaN} in its last three).
  flabs    int64, the rank of |fl| (0 zero .. 7 inf, 8 NaN): an integer
           handle on fl's value, for selections no AND of f32 compares can
           express (flabs == 7 keeps the rows holding +inf or -inf).
  valid    a plane for fl with about 25 % of its bits cleared, the region
           rows (F32Matrix.regions) forced valid; a plane for `key` (about 12 %
           cleared) for the nullable-key entries. A NULL row of fl keeps its
           ladder value, so for every case that passes anything there are
           NULL rows whose stored value passes it: a compare that forgets
           the plane passes too many rows in every such case.

The reference of a compare is numpy's float32 compare (cmx.pred_mask
semantics): NaN on either side fails, -0.0 == +0.0, subnormals are distinct
from zero. Four mutants of it (MUTANTS) model the ways a kernel goes wrong;
test_f32_matrix.py proves that the cases tell each from the reference in
every region. Nothing asks the code under test for an expected value.
"""

import functools
import struct

import numpy as np

import agg_matrix as amx
import col_matrix as cmx

GEOMS = amx.GEOMS
LT, GE, BETWEEN, EQ, ISNULL, NOTNULL = (cmx.LT, cmx.GE, cmx.BETWEEN, cmx.EQ,
                                        cmx.ISNULL, cmx.NOTNULL)
COUNT, SUM_I64, SUM_F64, COUNT_COL = (amx.COUNT, amx.SUM_I64, amx.SUM_F64,
                                      amx.COUNT_COL)
NLAD = len(amx.LADDER)                      # 17
LADDER = np.array(amx.LADDER, dtype=np.uint32)
# ladder index: 0 -inf, 1 -FLT_MAX, 2 -100, 3 -1, 4 -FLT_MIN, 5 -largest
# subnormal, 6 -smallest subnormal, 7 -0.0, 8 +0.0, 9 .. 15 mirrored, 16 NaN
ORDER = (6, 15, 3, 13, 0, 11, 5, 14, 8, 10, 16, 2, 9, 1, 12, 7, 4)
SHIFT = {"chunk": 8, "odd_t33": 0}
ABS_RANK = (7, 6, 5, 4, 3, 2, 1, 0, 0, 1, 2, 3, 4, 5, 6, 7, 8)
RANK_INF = 7
SUB_MIN, SUB_MAX = 0x00000001, 0x007FFFFF
NEG_NAN_LIT = 0xFFC00000
MUTANTS = ("flush", "unordered", "total_order", "int_field")
NKMOD = amx.NKMOD


def lit(bits):
    """a float32 bit pattern as the Python float a caller would pass"""
    return struct.unpack("<f", struct.pack("<I", bits))[0]


def f32_bits(x):
    return np.array([x], dtype=np.float32).view(np.uint32)[0]


# ---- cases ----------------------------------------------------------------
# (name, op, lo, hi, kind): kind "some" passes at least one valid row and
# rejects at least one; "none" passes no row; "null" is ISNULL / NOTNULL,
# which read the plane alone.
def _cases():
    names = ("-inf", "-fltmax", "-100", "-1", "-fltmin", "-submax", "-submin",
             "-0", "+0", "+submin", "+submax", "+fltmin", "+1", "+100",
             "+fltmax", "+inf", "nan")
    out = []
    for op, opn in ((LT, "lt"), (GE, "ge"), (EQ, "eq")):
        for b, n in zip(amx.LADDER + (NEG_NAN_LIT,), names + ("-nan",)):
            none = "nan" in n or (op == LT and n == "-inf")
            out.append((f"{opn}_{n}", op, lit(b), 0.0,
                        "none" if none else "some"))
    L = dict(zip(names, (lit(b) for b in amx.LADDER)))
    for n, lo, hi, kind in (
            ("-0_+0", L["-0"], L["+0"], "some"),
            ("+0_-0", L["+0"], L["-0"], "some"),
            ("-inf_+inf", L["-inf"], L["+inf"], "some"),
            ("-fltmax_+fltmax", L["-fltmax"], L["+fltmax"], "some"),
            ("pos_subnormals", L["+submin"], L["+submax"], "some"),
            ("+inf_+inf", L["+inf"], L["+inf"], "some"),
            ("nan_1", L["nan"], L["+1"], "none"),
            ("-1_nan", L["-1"], L["nan"], "none"),
            ("1_-1", L["+1"], L["-1"], "none")):
        out.append((f"between_{n}", BETWEEN, lo, hi, kind))
    out.append(("isnull", ISNULL, 0, 0, "null"))
    out.append(("notnull", NOTNULL, 0, 0, "null"))
    # int literals on the f32 column: the wrapper must route them to flo/fhi
    out.append(("int_lt_1", LT, 1, 0, "some"))
    out.append(("int_ge_-100", GE, -100, 0, "some"))
    out.append(("int_eq_0", EQ, 0, 0, "some"))
    out.append(("int_between_-100_1", BETWEEN, -100, 1, "some"))
    return tuple(out)


CASES = _cases()
POS_SUBNORMALS = next(c for c in CASES if c[0] == "between_pos_subnormals")

# SUM_F64 cases: (name, group, preds). Every one is summed over fx and fl.
ALL_M = ("m", GE, cmx.I64_MIN, 0)
SUM_CASES = (
    ("all_by_kmod", "kmod", (ALL_M,)),
    ("inf_rows_by_key", "key", (("flabs", EQ, RANK_INF, 0),)),
    ("pos_subnormals_by_key", "key", (("fl",) + POS_SUBNORMALS[1:4],)),
    ("pos_subnormals_by_kmod", "kmod", (("fl",) + POS_SUBNORMALS[1:4],)),
    ("fx_small_by_kmod", "kmod", (("fx", BETWEEN, -1.0, 1.0),)),
    ("fl_pos_inf_by_key", "key", (("fl", GE, lit(amx.POS_INF), 0.0),)),
    ("fl_neg_inf_by_kmod", "kmod",
     (("fl", LT, lit(0x80000000 | amx.FLT_MAX_BITS), 0.0),)),
)


# ---- f32 compares: the reference and its mutants ---------------------------
def _flush(bits):
    b = np.array(bits, dtype=np.uint32, copy=True)
    b[(b & np.uint32(0x7F800000)) == 0] &= np.uint32(0x80000000)
    return b


def f32_compare(bits, op, lo, hi, mutant=None):
    """bool mask of `x op literal` over float32 bit patterns. mutant None is
    the contract (numpy float32 compares); the others are wrong on purpose:
      flush        exponent-0 values of column and literal become zeros
      unordered    each compare is the negation of its opposite: NaN passes
      total_order  compares the amx.f32_key total order instead
      int_field    the literals are read from the wrong field: 0.0"""
    assert mutant is None or mutant in MUTANTS
    lo, hi = np.float32(lo), np.float32(hi)
    if mutant == "int_field":
        lo = hi = np.float32(0.0)
    bits = np.asarray(bits, dtype=np.uint32)
    if mutant == "flush":
        bits = _flush(bits)
        lo = _flush([f32_bits(lo)]).view(np.float32)[0]
        hi = _flush([f32_bits(hi)]).view(np.float32)[0]
    if mutant == "total_order":
        k = amx.f32_key(bits)
        klo = amx.f32_key([f32_bits(lo)])[0]
        khi = amx.f32_key([f32_bits(hi)])[0]
        return {LT: k < klo, GE: k >= klo, BETWEEN: (k >= klo) & (k <= khi),
                EQ: k == klo}[op]
    x = bits.view(np.float32)
    with np.errstate(invalid="ignore"):
        if mutant == "unordered":
            return {LT: ~(x >= lo), GE: ~(x < lo),
                    BETWEEN: ~(x < lo) & ~(x > hi),
                    EQ: ~(x < lo) & ~(x > lo)}[op]
        return {LT: x < lo, GE: x >= lo, BETWEEN: (x >= lo) & (x <= hi),
                EQ: x == lo}[op]


def _lsb_exp(bits):
    """per finite nonzero float32 bit pattern, the exponent e of its lowest
    set bit: the value is an odd multiple of 2^e"""
    b = np.asarray(bits, dtype=np.uint32).astype(np.int64)
    e = (b >> 23) & 0xFF
    sig = np.where(e == 0, b & 0x7FFFFF, (b & 0x7FFFFF) | 0x800000)
    low = sig & -sig                        # a power of two <= 2^23
    return np.maximum(e, 1) - 150 + np.log2(low).astype(np.int64)


class F32Matrix:
    def __init__(self, name):
        self.name = name
        self.am = am = amx.matrix(name)
        self.mx = mx = am.mx
        self.rows = rows = am.rows
        row = np.arange(rows, dtype=np.int64)
        idx = np.array(ORDER, dtype=np.int64)[(row + SHIFT[name]) % NLAD]
        bits = LADDER[idx]
        nan = idx == NLAD - 1
        bits[nan] = np.array(amx.NAN_BITS, dtype=np.uint32)[
            (row[nan] // NLAD) % len(amx.NAN_BITS)]
        self.lad = idx                      # ladder index per row
        self.fl_bits = bits
        self.fl = bits.view(np.float32)
        self.flabs = np.array(ABS_RANK, dtype=np.int64)[idx]

        nfull = mx.n_rowgroups - 1
        self.regions = {
            "final": row[rows - (rows & 3):],
            "rg_last": np.array([mx.bounds[g][1] - 1 for g in range(nfull)]),
            "rg_first": np.array([mx.bounds[g][0]
                                  for g in range(1, mx.n_rowgroups)]),
            "row0": row[:1]}
        rng = np.random.default_rng([cmx.SEED, 0xF32, GEOMS.index(name)])
        vfl = rng.random(rows) >= 0.25
        for r in self.regions.values():
            vfl[r] = True
        vkey = rng.random(rows) >= 0.125
        self.valid = {"fl": vfl, "key": vkey, "fx": am.valid["fx"],
                      "m": am.valid["m"]}
        self.cols = dict(am.cols, fl=self.fl, flabs=self.flabs)
        self._refs = {}
        self.col_bits = {"fl": self.fl_bits, "fx": am.fx_bits,
                         "f": np.ascontiguousarray(mx.f).view(np.uint32)}
        ng = mx.ngroups
        self.groups = {
            "key": (mx.key, ng), "kmod": (am.kmod, NKMOD),
            # NULL keys in one more group, the last row (scan_agg_nullkey);
            # the one key plane serves either group column
            "key_null": (np.where(vkey, mx.key, ng), ng + 1),
            "kmod_null": (np.where(vkey, am.kmod, NKMOD), NKMOD + 1),
            # the (kmod, key) tuple in tuple order (scan_agg_hash_multi)
            "kmod_key": (am.kmod * ng + mx.key, NKMOD * ng)}
        for a in (self.lad, self.fl_bits, self.fl, self.flabs, vfl, vkey,
                  *(g[0] for g in self.groups.values())):
            a.setflags(write=False)

    def validity_words(self, col):
        """the plane as attach_validity takes it: bit r of word r>>6"""
        b = np.zeros((self.rows + 63) // 64 * 64, dtype=np.uint8)
        b[:self.rows] = self.valid[col]
        return np.packbits(b, bitorder="little").view(np.uint64)

    # ---- references ----------------------------------------------------
    def pred_mask(self, preds, nulls=(), mutant=None):
        """rows passing the AND of preds [(col, op, lo, hi)] under SQL
        three-valued logic (cmx.pred_mask), over i64 and f32 columns; nulls
        names the columns whose plane is attached. mutant swaps the f32
        compare for a wrong one (f32_compare)."""
        mask = np.ones(self.rows, dtype=bool)
        for col, op, lo, hi in preds:
            valid = self.valid[col] if col in nulls else None
            if op == ISNULL:
                mask &= ~valid if valid is not None else False
                continue
            if op == NOTNULL:
                if valid is not None:
                    mask &= valid
                continue
            if col in self.col_bits:
                mask &= f32_compare(self.col_bits[col], op, lo, hi, mutant)
            else:
                x = self.cols[col]
                assert isinstance(lo, int) and isinstance(hi, int)
                mask &= {LT: x < lo, GE: x >= lo,
                         BETWEEN: (x >= lo) & (x <= hi), EQ: x == lo}[op]
            if valid is not None:
                mask &= valid
        return mask

    @functools.lru_cache(maxsize=None)
    def _packed_mask(self, preds, nulls):
        return np.packbits(self.pred_mask(preds, nulls))

    def mask(self, preds, nulls=()):
        """pred_mask of the reference, cached (packed) per query"""
        return np.unpackbits(self._packed_mask(tuple(preds), tuple(nulls)),
                             count=self.rows).view(bool)

    def case_preds(self, case):
        _, op, lo, hi, _ = case
        return (("fl", op, lo, hi),)

    def _sum_f64(self, d, ng, sel, col):
        """(reference [ng], may-assert [ng]) of SUM_F64(col) over the rows
        in sel with dense group ids d. A group may be asserted if its
        reference is NaN or an infinity, or if the sum is exact in any
        order: every summed value is a multiple of one power of two q and
        sum(|v|) / q < 2^53, so no partial sum ever rounds. The |v| sum is
        itself a rounded f64 sum, hence the spare bit in the bound."""
        b = self.col_bits[col][sel]
        g = d[sel]
        with np.errstate(invalid="ignore"):     # signalling NaNs, inf - inf
            v = b.view(np.float32).astype(np.float64)
            ref = np.bincount(g, weights=v, minlength=ng)
        finite = (b & np.uint32(0x7F800000)) != np.uint32(0x7F800000)
        nonfinite = np.bincount(g[~finite], minlength=ng) > 0
        nz = finite & ((b & np.uint32(0x7FFFFFFF)) != 0)
        qexp = np.full(ng, 1000, dtype=np.int64)
        np.minimum.at(qexp, g[nz], _lsb_exp(b[nz]))
        sumabs = np.bincount(g[nz], weights=np.abs(v[nz]), minlength=ng)
        units = np.ldexp(sumabs, -np.where(qexp == 1000, 0, qexp))
        exact = ~nonfinite & (units < 2.0 ** 52)
        assert not np.isfinite(ref[nonfinite]).any()
        return ref, nonfinite | exact

    def sum_ref(self, group, preds, nulls=()):
        """{"fx": (ref [ng], may-assert [ng]), "fl": ...}: SUM_F64 per group
        of `group` over the rows passing preds"""
        d, ng = self.groups[group]
        mask = self.mask(preds, nulls)
        return {c: self._sum_f64(d, ng, mask & self.valid[c]
                                 if c in nulls else mask, c)
                for c in ("fx", "fl")}

    def ref(self, group, preds, aggs, nulls=()):
        """One query grouped by a name of self.groups, laid out like
        GpuContext.scan_agg: (i64 [ng, naggs], f64 [ng, naggs], may-assert
        [ng, naggs] bool, rows_passed, present [ng] bool). aggs of COUNT,
        COUNT_COL, SUM_I64 and SUM_F64; may-assert is False only on SUM_F64
        slots whose sum depends on the order of the additions; f64 and
        may-assert are None for a list without SUM_F64. Computed once per
        query and shared read-only (the 66368-tuple grouping, which one
        path alone uses, is not kept)."""
        key = (group, tuple(preds), tuple(aggs), tuple(nulls))
        if key in self._refs:
            return self._refs[key]
        out = self._ref(*key)
        if self.groups[group][1] <= 4096:
            self._refs[key] = out
        return out

    def null_rows(self, preds, nulls=()):
        """passing rows whose key is NULL under the key plane"""
        return int((self.mask(preds, nulls) & ~self.valid["key"]).sum())

    def _ref(self, group, preds, aggs, nulls):
        d, ng = self.groups[group]
        mask = self.mask(preds, nulls)
        i64 = np.zeros((ng, len(aggs)), dtype=np.int64)
        f64 = ok = None
        if any(op == SUM_F64 for _, op in aggs):
            f64 = np.zeros(i64.shape, dtype=np.float64)
            ok = np.ones(i64.shape, dtype=bool)
        for q, (col, op) in enumerate(aggs):
            sel = mask & self.valid[col] \
                if op != COUNT and col in nulls else mask
            if op in (COUNT, COUNT_COL):
                i64[:, q] = np.bincount(d[sel], minlength=ng)
            elif op == SUM_I64:
                i64[:, q] = self._sum_i64(d[sel], ng, self.cols[col][sel])
            else:
                assert op == SUM_F64
                f64[:, q], ok[:, q] = self._sum_f64(d, ng, sel, col)
        present = np.bincount(d[mask], minlength=ng) > 0
        for a in (i64, f64, ok, present):
            if a is not None:
                a.setflags(write=False)
        return i64, f64, ok, int(mask.sum()), present

    @staticmethod
    def _sum_i64(g, ng, x):
        """wrap-around int64 sums per group: the 32-bit halves summed apart
        (each half-sum is below 2^53, so exact as bincount weights)"""
        lo = np.bincount(g, weights=(x & 0xFFFFFFFF).astype(np.float64),
                         minlength=ng)
        hi = np.bincount(g, weights=(x >> 32).astype(np.float64),
                         minlength=ng)
        return ((hi.astype(np.int64).view(np.uint64) << np.uint64(32))
                + lo.astype(np.int64).view(np.uint64)).view(np.int64)

    @functools.lru_cache(maxsize=None)
    def ref_topn(self, preds, nulls, k):
        """(rows [min(k, passing)] uint64, rows_passed): the passing rows
        ordered by (key, row) ascending — ORDER BY key LIMIT k"""
        rows = np.flatnonzero(self.mask(preds, nulls))
        order = np.argsort(self.mx.key[rows], kind="stable")
        out = rows[order][:k].astype(np.uint64)
        out.setflags(write=False)
        return out, len(rows)


def check_sums(got, ref, ok, what):
    """the asserted slots of a SUM_F64 column: NaN as "is NaN" (its sign and
    payload are unspecified), everything else by value — for an infinity
    that is bit for bit"""
    got, ref = np.asarray(got)[ok], np.asarray(ref)[ok]
    nan = np.isnan(ref)
    bad = np.flatnonzero(np.where(nan, ~np.isnan(got), got != ref))
    if len(bad):
        k = int(bad[0])
        raise AssertionError(
            f"{what}: {len(bad)} asserted sums differ; first (asserted slot "
            f"{k}) got {got[k]!r} want {ref[k]!r}")


@functools.lru_cache(maxsize=None)
def matrix(name):
    return F32Matrix(name)
