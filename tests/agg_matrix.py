"""Aggregate matrix: the inputs and numpy references for MIN / MAX /
COUNT(col) on every columnar scan path, built on two geometries of the
column-codec matrix (tests/col_matrix.py: "chunk" and "odd_t33", with their
columns, literals and pred_mask). tests/test_agg_matrix.py proves this file
on the CPU; tests/test_gpu_agg_matrix.py runs the GPU paths against it.

Added to the col_matrix columns:

  kmod     row % 61, a second dense group key. Every one of its 61 groups has
           rows in every row group and so in every workgroup: a kernel that
           never merged its workgroups' partials with min / max would get
           these groups wrong (each `key` group lives in one row group).
  fx       float32 column of special values. Six designated kmod groups hold
           only NaNs (both signs, quiet and signalling, varied payloads),
           only -0.0 / +0.0, a sign-set NaN among finite values, only -inf,
           only +inf, and denormals with +-FLT_MAX; the others hold ordinary
           values. Stored and compared as bit patterns.
  valid    one validity plane for `m` and one for `fx`: every bit of the two
           ALL_NULL kmod groups cleared (those groups pass rows yet have no
           value), about 25 % cleared elsewhere.

References are numpy reductions over the raw arrays (np.minimum.at /
np.maximum.at / np.bincount); the f32 order goes through the total-order
key map written here in numpy. Nothing decodes a blob or asks the code
under test for an expected value.
"""

import functools
import struct

import numpy as np

import col_matrix as cmx

GEOMS = ("chunk", "odd_t33")
NKMOD = 61
I64_MIN, I64_MAX = cmx.I64_MIN, cmx.I64_MAX

# SdbAggOp (include/sdb_gpu.h)
COUNT, SUM_I64, SUM_F64 = cmx.COUNT, cmx.SUM_I64, cmx.SUM_F64
COUNT_COL, MIN_I64, MAX_I64, MIN_F32, MAX_F32 = 3, 4, 5, 6, 7
F64_OPS = (SUM_F64, MIN_F32, MAX_F32)       # results in the f64 field

# designated kmod groups of fx
FX_GROUPS = {"all_nan": 3, "zeros": 7, "neg_nan_finite": 11, "neg_inf": 13,
             "pos_inf": 17, "denorm_fltmax": 19}
ALL_NULL = (23, 29)          # kmod groups with every validity bit cleared

CANON_NAN = 0x7FC00000
NAN_BITS = (0x7FC00000, 0xFFC00000, 0x7F800001, 0xFF800001, 0x7FFFFFFF,
            0xFFFFFFFF, 0x7FC12345, 0xFFA00001)
NEG_NAN = 0xFFC00001         # the sign-set NaN among finite values
FLT_MAX_BITS = 0x7F7FFFFF
DENORM_BITS = (0x00000001, 0x80000001, 0x007FFFFF, 0x807FFFFF,
               FLT_MAX_BITS, 0x80000000 | FLT_MAX_BITS)
POS_INF, NEG_INF = 0x7F800000, 0xFF800000
# ascending in the total order after canonicalisation (NaNs all tie on top)
LADDER = (NEG_INF, 0x80000000 | FLT_MAX_BITS, 0xC2C80000, 0xBF800000,
          0x80800000, 0x807FFFFF, 0x80000001, 0x80000000, 0x00000000,
          0x00000001, 0x007FFFFF, 0x00800000, 0x3F800000, 0x42C80000,
          FLT_MAX_BITS, POS_INF, CANON_NAN)


# ---- the f32 total-order key ------------------------------------------
def f32_key(bits):
    """uint32 bit patterns -> uint32 keys: every NaN becomes 0x7FC00000,
    then negative values complement and the others flip the sign bit, so
    unsigned key order is -inf < ... < -0.0 < +0.0 < ... < +inf < NaN"""
    b = np.array(bits, dtype=np.uint32, copy=True)
    b[(b & np.uint32(0x7FFFFFFF)) > np.uint32(0x7F800000)] = CANON_NAN
    return np.where(b >> np.uint32(31) == 1, ~b, b ^ np.uint32(0x80000000))


def f32_unkey(keys):
    """the inverse of f32_key on canonicalised values: keys -> bits"""
    k = np.asarray(keys, dtype=np.uint32)
    return np.where(k >> np.uint32(31) == 1, k ^ np.uint32(0x80000000), ~k)


def f32_key_py(b):
    """f32_key on one Python int"""
    if (b & 0x7FFFFFFF) > 0x7F800000:
        b = CANON_NAN
    return b ^ 0xFFFFFFFF if b >> 31 else b ^ 0x80000000


def f32_bits_to_f64_bits(b):
    """a float32 bit pattern widened to double, as a uint64 bit pattern —
    through struct only, so the sign of zero and the NaN are whatever the
    IEEE widening gives"""
    f = struct.unpack("<f", struct.pack("<I", b))[0]
    return struct.unpack("<Q", struct.pack("<d", f))[0]


def f64_bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


F64_NAN = f32_bits_to_f64_bits(CANON_NAN)       # 0x7FF8000000000000


def identity(op):
    """what a group with no non-NULL passing value returns"""
    return {COUNT_COL: 0, MIN_I64: I64_MAX, MAX_I64: I64_MIN,
            MIN_F32: float("inf"), MAX_F32: float("-inf")}[op]


class AggMatrix:
    def __init__(self, name):
        self.name = name
        self.mx = mx = cmx.matrix(name)
        self.rows = mx.rows
        rng = np.random.default_rng([cmx.SEED, 0xA66, GEOMS.index(name)])
        row = np.arange(self.rows, dtype=np.int64)
        self.kmod = row % NKMOD
        seq = row // NKMOD              # position of a row inside its group

        fx = (rng.normal(0.0, 100.0, self.rows)).astype(np.float32)
        bits = fx.view(np.uint32).copy()
        g = FX_GROUPS
        sel = self.kmod == g["all_nan"]
        bits[sel] = np.array(NAN_BITS, dtype=np.uint32)[seq[sel] % 8]
        sel = self.kmod == g["zeros"]
        bits[sel] = np.where(seq[sel] % 2 == 0, 0x80000000, 0).astype(
            np.uint32)
        sel = (self.kmod == g["neg_nan_finite"]) & (seq % 5 == 2)
        bits[sel] = NEG_NAN
        bits[self.kmod == g["neg_inf"]] = NEG_INF
        bits[self.kmod == g["pos_inf"]] = POS_INF
        sel = self.kmod == g["denorm_fltmax"]
        bits[sel] = np.array(DENORM_BITS, dtype=np.uint32)[seq[sel] % 6]
        self.fx_bits = bits
        self.fx = bits.view(np.float32)

        null_group = np.isin(self.kmod, ALL_NULL)
        self.valid = {
            "m": (rng.random(self.rows) >= 0.25) & ~null_group,
            "fx": (rng.random(self.rows) >= 0.25) & ~null_group}
        self.cols = dict(mx.cols, kmod=self.kmod, fx=self.fx)
        self.groups = {"key": (mx.key, mx.ngroups),
                       "kmod": (self.kmod, NKMOD)}
        for a in (self.kmod, self.fx_bits, self.fx, *self.valid.values()):
            a.setflags(write=False)

    def validity_words(self, col):
        """the plane as attach_validity takes it: bit r of word r>>6"""
        b = np.zeros((self.rows + 63) // 64 * 64, dtype=np.uint8)
        b[:self.rows] = self.valid[col]
        return np.packbits(b, bitorder="little").view(np.uint64)

    def kmod_strings(self):
        """kmod as a small string column: b'k00' .. b'k60' per row"""
        names = [b"k%02d" % k for k in range(NKMOD)]
        return names, [names[k] for k in self.kmod.tolist()]

    # ---- references ----------------------------------------------------
    @functools.lru_cache(maxsize=None)
    def pred_mask(self, preds):
        """col_matrix's pred_mask, extended to f32 compares on fx. No
        predicate here reads a column whose plane may be attached (m under
        nulls is only aggregated), so no plane enters the mask."""
        own = [p for p in preds if p[0] == "fx"]
        mask = self.mx.pred_mask([p for p in preds if p[0] != "fx"]).copy()
        for _, op, lo, hi in own:
            lo, hi = np.float32(lo), np.float32(hi)
            with np.errstate(invalid="ignore"):     # NaN fails each compare
                mask &= {cmx.LT: self.fx < lo, cmx.GE: self.fx >= lo,
                         cmx.BETWEEN: (self.fx >= lo) & (self.fx <= hi),
                         cmx.EQ: self.fx == lo}[op]
        mask.setflags(write=False)
        return mask

    def selected(self, preds, col, op, nulls):
        """rows that feed aggregate (col, op): passing, and not NULL"""
        mask = self.pred_mask(preds)
        if op != COUNT and col in nulls:
            assert not any(p[0] == col for p in preds)
            return mask & self.valid[col]
        return mask

    def agg_column(self, dense, ng, preds, col, op, nulls):
        """one aggregate over dense group ids 0..ng-1"""
        sel = self.selected(preds, col, op, nulls)
        d = dense[sel]
        if op in (COUNT, COUNT_COL):
            return np.bincount(d, minlength=ng).astype(np.int64)
        x = self.cols[col][sel] if col != "fx" else None
        if op == SUM_I64:
            acc = np.zeros(ng, dtype=np.uint64)
            np.add.at(acc, d, x.view(np.uint64))
            return acc.view(np.int64)
        if op == SUM_F64:
            return np.bincount(d, weights=x.astype(np.float64), minlength=ng)
        if op == MIN_I64:
            out = np.full(ng, I64_MAX, dtype=np.int64)
            np.minimum.at(out, d, x)
            return out
        if op == MAX_I64:
            out = np.full(ng, I64_MIN, dtype=np.int64)
            np.maximum.at(out, d, x)
            return out
        assert col == "fx" and op in (MIN_F32, MAX_F32)
        keys = f32_key(self.fx_bits[sel])
        some = np.bincount(d, minlength=ng) > 0
        if op == MIN_F32:
            k = np.full(ng, 0xFFFFFFFF, dtype=np.uint32)
            np.minimum.at(k, d, keys)
        else:
            k = np.zeros(ng, dtype=np.uint32)
            np.maximum.at(k, d, keys)
        k[~some] = f32_key([POS_INF if op == MIN_F32 else NEG_INF])[0]
        return f32_unkey(k).astype(np.uint32).view(np.float32).astype(
            np.float64)

    @staticmethod
    def _pack(columns, aggs):
        i64 = np.zeros((len(columns[0]), len(columns)), dtype=np.int64)
        f64 = np.zeros(i64.shape, dtype=np.float64)
        for q, (c, (_, op)) in enumerate(zip(columns, aggs)):
            (f64 if op in F64_OPS else i64)[:, q] = c
        i64.setflags(write=False)
        f64.setflags(write=False)
        return i64, f64

    @functools.lru_cache(maxsize=None)
    def ref_dense(self, group, preds, aggs, nulls=()):
        """Dense group-by `key` or `kmod`: (i64 [ng, naggs], f64 [ng, naggs],
        rows_passed, present [ng] bool), laid out like GpuContext.scan_agg;
        present marks the groups with a passing row, the ones a hash
        aggregate returns."""
        dense, ng = self.groups[group]
        i64, f64 = self._pack(
            [self.agg_column(dense, ng, preds, c, op, nulls)
             for c, op in aggs], aggs)
        mask = self.pred_mask(preds)
        present = np.bincount(dense[mask], minlength=ng) > 0
        return i64, f64, int(mask.sum()), present

    @functools.lru_cache(maxsize=None)
    def ref_hash(self, group_col, preds, aggs, nulls=()):
        """Hash group-by an arbitrary i64 column: (keys ascending, i64,
        f64, rows_passed), laid out like GpuContext.scan_agg_hash."""
        mask = self.pred_mask(preds)
        keys, inv = np.unique(self.cols[group_col][mask],
                              return_inverse=True)
        dense = np.zeros(self.rows, dtype=np.int64)
        dense[mask] = inv.reshape(-1)
        i64, f64 = self._pack(
            [self.agg_column(dense, len(keys), preds, c, op, nulls)
             for c, op in aggs], aggs)
        return keys, i64, f64, int(mask.sum())

    def minmax_python(self, group, preds, col, nulls=()):
        """The second witness: per group (min, max) in a plain Python loop.
        i64 columns as Python ints; fx as (f64 bits of min, f64 bits of max)
        found by comparing Python-int keys and widened through struct.
        Groups without a value hold the identities."""
        dense, ng = self.groups[group]
        sel = self.selected(preds, col, MIN_I64, nulls)
        gs = dense[sel].tolist()
        if col != "fx":
            lo, hi = [I64_MAX] * ng, [I64_MIN] * ng
            for g, v in zip(gs, self.cols[col][sel].tolist()):
                if v < lo[g]:
                    lo[g] = v
                if v > hi[g]:
                    hi[g] = v
            return lo, hi
        lo, hi = [None] * ng, [None] * ng
        for g, b in zip(gs, self.fx_bits[sel].tolist()):
            k = f32_key_py(b)
            if lo[g] is None or k < lo[g][0]:
                lo[g] = (k, b)
            if hi[g] is None or k > hi[g][0]:
                hi[g] = (k, b)

        def widen(slot, empty):
            if slot is None:
                return f32_bits_to_f64_bits(empty)
            b = slot[1]
            if (b & 0x7FFFFFFF) > 0x7F800000:
                b = CANON_NAN
            return f32_bits_to_f64_bits(b)
        return ([widen(s, POS_INF) for s in lo],
                [widen(s, NEG_INF) for s in hi])


@functools.lru_cache(maxsize=None)
def matrix(name):
    return AggMatrix(name)
