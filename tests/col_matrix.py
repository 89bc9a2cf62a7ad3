"""Column-codec matrix: deterministic tables in which every row group of a
FoR/bitpacked i64 column has a chosen bit width (0..32, each exactly once per
column) and a chosen base (INT64_MIN, the largest base the width allows, a
small negative, zero, 2^40), at row-group tilings the 65536-row default never
produces, plus the numpy references the CPU and GPU matrix tests compare
against. The columnar counterpart of tests/codec_matrix.py.

The raw numpy arrays are the ground truth; nothing here decodes a blob to
obtain an expected value.

Geometries (group_rows, full groups, tail rows):

  chunk    16482 = 2*8192 + 98 rows per group, so the staged scan kernel
           walks chunks of 8192, 8192 and 98 rows (the last no multiple of
           32); the 97-row tail group is odd.
  odd_t1   1025 rows per group: every full group ends in an odd row taken
  odd_t33  by thread 0, odd groups start at an odd row (16-byte raw pair
           loads at 8-byte alignment), and no group boundary falls on a
           64-row validity word. Tails of 1 and of 33 rows.

Columns:

  m, m2    FoR width matrices. Row group i < 33 of `m` has width order[i], a
           seeded permutation of 0..32; `m2` uses a second permutation with
           no fixed point in common, so two staged predicate columns differ
           in width in every group. The tail group has width 13 (a 1-row
           tail is constant, hence width 0). Deltas are uniform in
           [0, 2^w-1] with 2^w-1 forced at rows 0 and glen-2 and 0 forced at
           rows 1 and glen-1, so vmin = base and vmax = base + 2^w-1; delta
           2^w-2 is removed from every group of width >= 2, which leaves an
           interior value that is provably absent for EQ. Bases cycle
           through the five kinds by group index (shifted by two for m2).
           One row of `m` is forced to -1, the hash table's reserved key.
  key      rg*32 + (row-in-group mod 2^(rg mod 6)): dense group keys below
           34*32 = 1088 from which the row group (and so the width) of a
           wrong aggregate slot is key // 32; as a FoR column its width
           varies 0..5 with the group. Loaded raw and FoR from one array.
  f        float32 multiples of 1/8 with |f| < 1024: every f64 partial sum
           is an integer count of eighths below 2^53, exact in any order, so
           SUM_F64 is compared bit for bit.
  valid_m, valid_f   validity planes with ~25% NULLs.
"""

import functools
import struct

import numpy as np

import serenedb_amd as sa

SEED = 0x5DBC0101
I64_MIN = -(1 << 63)
I64_MAX = (1 << 63) - 1
TAIL_WIDTH = 13
KEYS_PER_RG = 32

# SdbPredOp / SdbAggOp (include/sdb_gpu.h)
LT, GE, BETWEEN, EQ, ISNULL, NOTNULL = 1, 2, 3, 4, 5, 6
COUNT, SUM_I64, SUM_F64 = 0, 1, 2

GEOMETRIES = {           # name: (group_rows, full groups, tail rows)
    "chunk": (16482, 33, 97),
    "odd_t1": (1025, 33, 1),
    "odd_t33": (1025, 33, 33),
}
BASE_KINDS = ("int64_min", "int64_max", "minus5", "zero", "2^40")


def base_of(kind, w):
    """The base of a group of width w: its deltas reach 2^w - 1, so the
    int64_max kind is the largest base that keeps base + delta in range."""
    return {"int64_min": I64_MIN, "int64_max": I64_MAX - ((1 << w) - 1),
            "minus5": -5, "zero": 0, "2^40": 1 << 40}[kind]


def fits_i64(x):
    return I64_MIN <= x <= I64_MAX


def parse_col_blob(blob):
    """(header dict, [group dict]) of an encode_col_i64 blob: the 48-byte
    SdbColHeader and the 40-byte SdbColGroupDesc table (sdb_host.cpp)."""
    magic, rows, group_rows, ngroups, off_desc, off_payload, size = \
        struct.unpack_from("<QQIIQQQ", blob, 0)
    hdr = dict(magic=magic, rows=rows, group_rows=group_rows,
               ngroups=ngroups, off_desc=off_desc, off_payload=off_payload,
               size=size)
    desc = []
    for g in range(ngroups):
        base, vmin, vmax, word_off, width = struct.unpack_from(
            "<qqqQH", blob, off_desc + 40 * g)
        desc.append(dict(base=base, vmin=vmin, vmax=vmax, word_off=word_off,
                         width=width))
    return hdr, desc


class WidthCol:
    """One FoR width-matrix column: values plus, per row group, the width,
    base kind and base it was built with."""

    def __init__(self, vals, widths, kinds, bases):
        self.vals = vals
        self.widths = widths
        self.kinds = kinds
        self.bases = bases


def _absent_delta(w):
    """the delta no row of a width-w group holds (None below width 2)"""
    return (1 << w) - 2 if w >= 2 else None


def _width_col(rng, bounds, order, base_shift):
    vals = np.empty(bounds[-1][1], dtype=np.int64)
    widths, kinds, bases = [], [], []
    for g, (r0, r1) in enumerate(bounds):
        glen = r1 - r0
        w = order[g] if g < len(order) else TAIL_WIDTH
        if glen == 1:
            w = 0                       # one row is a constant group
        hi = (1 << w) - 1
        d = rng.integers(0, hi + 1, glen, dtype=np.int64)
        if _absent_delta(w) is not None:
            d[d == _absent_delta(w)] = 1
        if glen > 1:
            assert glen >= 4
            d[0] = d[glen - 2] = hi
            d[1] = d[glen - 1] = 0
        kind = BASE_KINDS[(g + base_shift) % len(BASE_KINDS)]
        base = base_of(kind, w)
        vals[r0:r1] = np.int64(base) + d    # in range by construction
        widths.append(w)
        kinds.append(kind)
        bases.append(base)
    return WidthCol(vals, widths, kinds, bases)


class ColMatrix:
    COLS = ("key", "m", "m2", "f")

    def __init__(self, name):
        self.name = name
        self.group_rows, nfull, tail = GEOMETRIES[name]
        self.rows = self.group_rows * nfull + tail
        self.n_rowgroups = nfull + 1
        self.ngroups = self.n_rowgroups * KEYS_PER_RG
        self.bounds = [(g * self.group_rows,
                        min(self.rows, (g + 1) * self.group_rows))
                       for g in range(self.n_rowgroups)]
        rng = np.random.default_rng(
            [SEED, sorted(GEOMETRIES).index(name)])
        self.order = [int(x) for x in rng.permutation(nfull)]
        while True:
            self.order2 = [int(x) for x in rng.permutation(nfull)]
            if all(a != b for a, b in zip(self.order, self.order2)):
                break
        self.m = _width_col(rng, self.bounds, self.order, 0)
        self.m2 = _width_col(rng, self.bounds, self.order2, 2)
        # the hash aggregate's reserved key, as an ordinary FoR value
        g = next(g for g in range(nfull)
                 if self.m.kinds[g] == "minus5" and self.m.widths[g] >= 4)
        self.minus_one_row = self.bounds[g][0] + 2
        self.m.vals[self.minus_one_row] = -1

        row = np.arange(self.rows, dtype=np.int64)
        rg = row // self.group_rows
        self.key = rg * KEYS_PER_RG + \
            ((row - rg * self.group_rows) & ((1 << (rg % 6)) - 1))
        self.f = (rng.integers(-8191, 8192, self.rows) / 8.0).astype(
            np.float32)
        self.f[self.minus_one_row] = 1023.0     # passes any f >= t filter
        self.valid = {"m": rng.random(self.rows) >= 0.25,
                      "f": rng.random(self.rows) >= 0.25}
        self.cols = {"key": self.key, "m": self.m.vals, "m2": self.m2.vals,
                     "f": self.f}
        for a in list(self.cols.values()) + list(self.valid.values()):
            a.setflags(write=False)

    # ---- encoded forms -------------------------------------------------
    @functools.lru_cache(maxsize=None)
    def blob(self, col):
        return sa.encode_col_i64(self.cols[col], self.group_rows)

    def validity_words(self, col):
        """the plane as attach_validity takes it: bit r of word r>>6"""
        bits = np.zeros((self.rows + 63) // 64 * 64, dtype=np.uint8)
        bits[:self.rows] = self.valid[col]
        return np.packbits(bits, bitorder="little").view(np.uint64)

    # ---- literals that probe one row group -----------------------------
    def width_col(self, col):
        return {"m": self.m, "m2": self.m2}[col]

    def probe_groups(self, col):
        """label -> row group: widths 1, 2, 31, 32, the first group of each
        extreme base kind that is wider than 2 bits, and the tail."""
        wc = self.width_col(col)
        full = range(self.n_rowgroups - 1)
        out = {f"w{w}": wc.widths.index(w) for w in (1, 2, 31, 32)}
        for kind in ("int64_min", "int64_max"):
            out[kind] = next(g for g in full
                             if wc.kinds[g] == kind and wc.widths[g] > 2)
        out["tail"] = self.n_rowgroups - 1
        return out

    def split_literal(self, col, rg):
        """base + 2^(w-1): LT / GE at it splits the group row by row"""
        wc = self.width_col(col)
        w = wc.widths[rg]
        return wc.bases[rg] + ((1 << (w - 1)) if w else 0)

    def zonemap_cases(self, col, rg):
        """[(label, op, lo, hi)] with the literal exactly at, and one off,
        the group's zonemap bounds. A literal outside int64 is left out,
        never wrapped."""
        wc = self.width_col(col)
        r0, r1 = self.bounds[rg]
        vmin = int(self.cols[col][r0:r1].min())
        vmax = int(self.cols[col][r0:r1].max())
        cases = [("lt_vmin", LT, vmin, 0), ("lt_vmin+1", LT, vmin + 1, 0),
                 ("ge_vmax", GE, vmax, 0), ("ge_vmax+1", GE, vmax + 1, 0),
                 ("between_vmax", BETWEEN, vmax, vmax),
                 ("between_vmin", BETWEEN, vmin, vmin),
                 ("between_above", BETWEEN, vmax + 1, vmax + 2),
                 ("eq_vmin", EQ, vmin, 0), ("eq_vmax", EQ, vmax, 0)]
        if _absent_delta(wc.widths[rg]) is not None:
            cases.append(("eq_absent", EQ,
                          wc.bases[rg] + _absent_delta(wc.widths[rg]), 0))
        return [c for c in cases if fits_i64(c[2]) and fits_i64(c[3])]

    # ---- references ----------------------------------------------------
    def pred_mask(self, preds, nulls=()):
        """rows passing the AND of preds [(col, op, lo, hi)] under SQL
        three-valued logic: a comparison fails on NULL, ISNULL / NOTNULL
        read the plane alone. nulls: columns whose plane is attached."""
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
            x = self.cols[col]
            if x.dtype == np.float32:
                lo, hi = np.float32(lo), np.float32(hi)
            if op == LT:
                mask &= x < lo
            elif op == GE:
                mask &= x >= lo
            elif op == BETWEEN:
                mask &= (x >= lo) & (x <= hi)
            elif op == EQ:
                mask &= x == lo
            else:
                raise ValueError(op)
            if valid is not None:
                mask &= valid
        return mask

    def _agg_column(self, dense, ng, mask, col, op, nulls):
        """one aggregate over the rows in mask, grouped by dense keys"""
        if op == COUNT:
            return np.bincount(dense[mask], minlength=ng).astype(np.int64)
        sel = mask & self.valid[col] if col in nulls else mask
        if op == SUM_I64:       # wrap-around, like the kernels' u64 add
            acc = np.zeros(ng, dtype=np.uint64)
            np.add.at(acc, dense[sel], self.cols[col][sel].view(np.uint64))
            return acc.view(np.int64)
        if op == SUM_F64:       # exact: dyadic values (module docstring)
            return np.bincount(
                dense[sel], weights=self.cols[col][sel].astype(np.float64),
                minlength=ng)
        raise ValueError(op)

    def _aggregate(self, columns):
        i64 = np.zeros((len(columns[0]), len(columns)), dtype=np.int64)
        f64 = np.zeros(i64.shape, dtype=np.float64)
        for q, c in enumerate(columns):
            (f64 if c.dtype == np.float64 else i64)[:, q] = c
        i64.setflags(write=False)
        f64.setflags(write=False)
        return i64, f64

    @functools.lru_cache(maxsize=None)
    def _scan_column(self, preds, nulls, col, op, ng):
        """(one aggregate column of ref_scan, rows passed); cached per
        column so queries that differ only in their aggregate list share
        the work"""
        mask = self.pred_mask(preds, nulls)
        return (self._agg_column(self.key, ng, mask, col, op, nulls),
                int(mask.sum()))

    def ref_scan(self, preds, aggs, nulls=(), ngroups=None):
        """Dense group-by `key`: (i64 [ngroups, naggs], f64 [ngroups,
        naggs], rows_passed), laid out like GpuContext.scan_agg. preds,
        aggs [(col or None, op)] and nulls are tuples (the columns are
        computed once and shared read-only between tests)."""
        ng = ngroups or self.ngroups
        cols = [self._scan_column(preds, nulls, col, op, ng)
                for col, op in aggs]
        i64, f64 = self._aggregate([c for c, _ in cols])
        return i64, f64, cols[0][1]

    @functools.lru_cache(maxsize=None)
    def ref_hash(self, group_col, preds, aggs, nulls=()):
        """Hash group-by an arbitrary i64 column: (keys ascending, i64
        [n, naggs], f64 [n, naggs], rows_passed), laid out like
        GpuContext.scan_agg_hash (groups with no passing row are absent)."""
        mask = self.pred_mask(preds, nulls)
        keys, inv = np.unique(self.cols[group_col][mask],
                              return_inverse=True)
        dense = np.zeros(self.rows, dtype=np.int64)
        dense[mask] = inv.reshape(-1)
        i64, f64 = self._aggregate(
            [self._agg_column(dense, len(keys), mask, col, op, nulls)
             for col, op in aggs])
        return keys, i64, f64, int(mask.sum())

    def sum_i64_python(self, preds, col, nulls=()):
        """SUM_I64 per key in Python integers mod 2^64: the second witness
        for the uint64 np.add.at reference."""
        mask = self.pred_mask(preds, nulls)
        if col in nulls:
            mask = mask & self.valid[col]
        sums = [0] * self.ngroups
        for k, v in zip(self.key[mask].tolist(),
                        self.cols[col][mask].tolist()):
            sums[k] += v
        return [s % (1 << 64) for s in sums]

    def describe_keys(self, keys):
        """'rg 7 (m w=32 int64_min, m2 w=3 zero)' for the row groups behind
        dense keys: what a failing slot decodes"""
        out = []
        for rg in sorted({int(k) // KEYS_PER_RG for k in keys}):
            if rg >= self.n_rowgroups:
                out.append(f"rg {rg} (beyond the table)")
                continue
            out.append(f"rg {rg} (m w={self.m.widths[rg]} "
                       f"{self.m.kinds[rg]}, m2 w={self.m2.widths[rg]} "
                       f"{self.m2.kinds[rg]}, key w={self.key_width(rg)})")
        return ", ".join(out)

    def key_width(self, rg):
        r0, r1 = self.bounds[rg]
        k = self.key[r0:r1]
        return int(k.max() - k.min()).bit_length()


@functools.lru_cache(maxsize=None)
def matrix(name):
    return ColMatrix(name)
