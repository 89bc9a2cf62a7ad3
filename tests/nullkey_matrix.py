"""NULL-group-key matrix: validity planes for the group keys of the aggregate
matrix (tests/agg_matrix.py, geometries "chunk" and "odd_t33"), key arrays
whose NULL rows are overwritten with poison, a sparse hash key, and the numpy
references of GROUP BY over a nullable key. tests/test_nullkey_matrix.py
proves this file on the CPU; tests/test_gpu_nullkey_matrix.py runs the GPU
paths against it.

Planes (True = valid), one each for `key`, `kmod` and `ksparse`: about 25 %
of the bits cleared at random, then, on `key` and `kmod`:

  row 0 and the last row NULL (the last row sits in the raw kernel's rows & 3
  tail and is the odd tail row of its row group in the FoR and staged loops);
  rows 63 and 64 NULL, 62 and 65 valid: NULLs on both sides of a validity
  word boundary;
  row group ALL_NULL_RG entirely NULL: its workgroup feeds the NULL group
  alone, and the `key` groups that live in it come back empty;
  row group NO_NULL_RG without a NULL — in the `kmod` plane except for the
  rows of NULL_KMOD, the kmod group that is NULL in every row of the table
  (identities from the dense entry, absent from the hash result).

`ksparse` maps kmod through KSPARSE, 61 int64 values spread over the whole
range with INT64_MIN, INT64_MAX, 0 and the hash table's reserved key -1; its
plane has the random NULLs plus row 0 and the last row.

Poisoned arrays equal the originals on valid rows; NULL rows cycle through
values that would be wrong as an index, a hash key or a sum: outside
[0, ngroups), the int64 extremes (raw only: a FoR row group's deltas must
fit 32 bits), -1, and the value of a live group.

References go through AggMatrix.agg_column with the dense id
where(valid, id, ng) over ng + 1 groups; the predicate mask knows the planes
(a compare on a column drops its NULL rows, ISNULL / NOTNULL read the plane).
Nothing asks the code under test for an expected value.
"""

import functools

import numpy as np

import agg_matrix as amx
import col_matrix as cmx

GEOMS = amx.GEOMS
I64_MIN, I64_MAX = cmx.I64_MIN, cmx.I64_MAX
ALL_NULL_RG = 5
NO_NULL_RG = 9
NULL_KMOD = 31          # no FX_GROUPS / ALL_NULL group of agg_matrix
KEYCOLS = ("key", "kmod", "ksparse")
WORD_EDGE = (63, 64)    # NULL on both sides of the first word boundary
PREFIX = 8              # SDB_PRED_PREFIX: ("kstr", PREFIX, b"k1", 0) in a
                        # predicate list = the string slot made of kmod


def _ksparse_table():
    """61 distinct int64 values over the whole range, both extremes, 0, -1"""
    t = [(k * 0x9E3779B97F4A7C15 + 0x1234567) % (1 << 64) - (1 << 63)
         for k in range(amx.NKMOD)]
    t[0], t[60], t[30], t[2] = I64_MIN, I64_MAX, 0, -1
    return np.array(t, dtype=np.int64)


KSPARSE = _ksparse_table()
KSPARSE_MINUS_ONE = 2   # the kmod group whose ksparse key is -1


class NullKeyMatrix:
    def __init__(self, name):
        self.name = name
        self.am = am = amx.matrix(name)
        self.mx = mx = am.mx
        self.rows = rows = mx.rows
        G = mx.group_rows
        rng = np.random.default_rng([cmx.SEED, 0x4E4B, GEOMS.index(name)])
        rg = np.arange(rows) // G
        self.ksparse = KSPARSE[am.kmod]
        self.groups = {"key": (mx.key, mx.ngroups),
                       "kmod": (am.kmod, amx.NKMOD)}
        self.cols = dict(am.cols, ksparse=self.ksparse)

        self.valid = {"m": am.valid["m"], "fx": am.valid["fx"]}
        for col in KEYCOLS:
            v = rng.random(rows) >= 0.25
            if col != "ksparse":
                v[rg == ALL_NULL_RG] = False
                v[rg == NO_NULL_RG] = True
                v[[WORD_EDGE[0] - 1, WORD_EDGE[1] + 1]] = True
                v[list(WORD_EDGE)] = False
            if col == "kmod":
                v[am.kmod == NULL_KMOD] = False
            v[[0, rows - 1]] = False
            self.valid[col] = v

        # poison: what a NULL row stores. live = a key some valid row holds.
        self.live = {"key": int(mx.key[G * 7 + 1]), "kmod": 5,
                     "ksparse": int(KSPARSE[5])}
        self.poison_values = {}
        self.poisoned = {}
        for col in KEYCOLS:
            ng = self.groups[col][1] if col in self.groups else amx.NKMOD
            live = self.live[col]
            if col == "ksparse":        # raw only; every value is "in range"
                kinds = {"raw": (-1, 12345, I64_MIN + 1, live, I64_MAX - 1)}
            else:
                kinds = {"raw": (I64_MIN, I64_MAX, -1, ng, ng + 1000, live),
                         "for": (-1, -7, ng, ng + 1000, live)}
            for codec, cyc in kinds.items():
                a = self.cols[col].copy()
                null = np.flatnonzero(~self.valid[col])
                a[null] = np.array(cyc, dtype=np.int64)[
                    np.arange(len(null)) % len(cyc)]
                a.setflags(write=False)
                self.poisoned[col, codec] = a
                self.poison_values[col, codec] = cyc
        for a in (self.ksparse, *self.valid.values()):
            a.setflags(write=False)

    def validity_words(self, col, plane=None):
        """the plane as attach_validity takes it: bit r of word r>>6"""
        b = np.zeros((self.rows + 63) // 64 * 64, dtype=np.uint8)
        b[:self.rows] = self.valid[col] if plane is None else plane
        return np.packbits(b, bitorder="little").view(np.uint64)

    # ---- references ----------------------------------------------------
    def str_mask(self, prefix):
        """rows whose kmod string (b'k00' .. b'k60') starts with prefix"""
        names = self.am.kmod_strings()[0]
        hit = np.array([n.startswith(prefix) for n in names], dtype=bool)
        return hit[self.am.kmod]

    @functools.lru_cache(maxsize=None)
    def pred_mask(self, preds, nulls):
        """rows passing the AND of preds under SQL three-valued logic; nulls:
        the columns whose plane is attached"""
        mask = np.ones(self.rows, dtype=bool)
        for p in preds:
            col, op, lo, hi = p
            if col == "kstr":
                assert op == PREFIX
                mask &= self.str_mask(lo)
                continue
            valid = self.valid[col] if col in nulls else None
            if op == cmx.ISNULL:
                mask &= ~valid if valid is not None else False
                continue
            if op == cmx.NOTNULL:
                if valid is not None:
                    mask &= valid
                continue
            if col in KEYCOLS:
                x = self.cols[col]
                mask &= {cmx.LT: x < lo, cmx.GE: x >= lo,
                         cmx.BETWEEN: (x >= lo) & (x <= hi),
                         cmx.EQ: x == lo}[op]
            else:
                mask &= self.am.pred_mask((p,))
            if valid is not None:
                mask &= valid
        mask.setflags(write=False)
        return mask

    def selected(self, preds, col, op, nulls):
        """rows that feed aggregate (col, op): passing, and not NULL. This
        is what AggMatrix.agg_column asks of its matrix."""
        mask = self.pred_mask(preds, nulls)
        if op != amx.COUNT and col in nulls:
            return mask & self.valid[col]
        return mask

    fx_bits = property(lambda self: self.am.fx_bits)

    def agg_column(self, dense, ng, preds, col, op, nulls):
        return amx.AggMatrix.agg_column(self, dense, ng, preds, col, op,
                                        nulls)

    @functools.lru_cache(maxsize=None)
    def ref_dense(self, group, preds, aggs, nulls=(), plane=True):
        """Dense group-by a nullable `key` / `kmod`: (i64 [ng+1, naggs], f64
        [ng+1, naggs], rows_passed, null_rows, present [ng+1]), laid out like
        GpuContext.scan_agg_nullkey: row ng is the NULL group. nulls: other
        columns with an attached plane; plane=False: no key plane."""
        dense, ng = self.groups[group]
        if plane:
            nulls = tuple(nulls) + (group,)
            dense = np.where(self.valid[group], dense, ng)
        i64, f64 = amx.AggMatrix._pack(
            [self.agg_column(dense, ng + 1, preds, c, op, nulls)
             for c, op in aggs], aggs)
        mask = self.pred_mask(preds, nulls)
        present = np.bincount(dense[mask], minlength=ng + 1) > 0
        return (i64, f64, int(mask.sum()), int((dense[mask] == ng).sum()),
                present)

    @functools.lru_cache(maxsize=None)
    def ref_hash(self, group_col, preds, aggs, nulls=(), plane=True):
        """Hash group-by a nullable column: (keys ascending, i64 [n, naggs],
        f64 [n, naggs], rows_passed, null_i64 [naggs], null_f64 [naggs],
        null_rows), laid out like GpuContext.scan_agg_hash_nullkey"""
        valid = self.valid[group_col] if plane else np.ones(self.rows, bool)
        if plane:
            nulls = tuple(nulls) + (group_col,)
        mask = self.pred_mask(preds, nulls)
        keys, inv = np.unique(self.cols[group_col][mask & valid],
                              return_inverse=True)
        dense = np.full(self.rows, len(keys), dtype=np.int64)
        dense[mask & valid] = inv.reshape(-1)
        i64, f64 = amx.AggMatrix._pack(
            [self.agg_column(dense, len(keys) + 1, preds, c, op, nulls)
             for c, op in aggs], aggs)
        n = len(keys)
        return (keys, i64[:n], f64[:n], int(mask.sum()), i64[n], f64[n],
                int((mask & ~valid).sum()))

    @functools.lru_cache(maxsize=None)
    def ref_ungrouped(self, preds, aggs, nulls=()):
        """every passing row in one group: (i64 [naggs], f64 [naggs],
        rows_passed) — what the NULL group of an all-NULL key holds"""
        dense = np.zeros(self.rows, dtype=np.int64)
        i64, f64 = amx.AggMatrix._pack(
            [self.agg_column(dense, 1, preds, c, op, nulls)
             for c, op in aggs], aggs)
        return i64[0], f64[0], int(self.pred_mask(preds, nulls).sum())

    def null_group_python(self, group, preds, nulls=()):
        """The second witness: the NULL group of `group` in a plain Python
        loop over the rows. Returns a dict: count, count_m, sum_m (mod 2^64),
        min_m, max_m2, sum_f (exact: eighths), count_fx, and the (min, max)
        of fx as f64 bit patterns."""
        nulls = tuple(nulls) + (group,)
        rows = np.flatnonzero(self.pred_mask(preds, nulls)
                              & ~self.valid[group])
        vm = (self.valid["m"] if "m" in nulls
              else np.ones(self.rows, bool))[rows].tolist()
        vfx = (self.valid["fx"] if "fx" in nulls
               else np.ones(self.rows, bool))[rows].tolist()
        out = dict(count=0, count_m=0, sum_m=0, min_m=I64_MAX,
                   max_m2=I64_MIN, sum_f=0.0, count_fx=0)
        lo = hi = None
        for ok_m, ok_fx, m, m2, f, b in zip(
                vm, vfx, self.cols["m"][rows].tolist(),
                self.cols["m2"][rows].tolist(),
                self.cols["f"][rows].tolist(),
                self.am.fx_bits[rows].tolist()):
            out["count"] += 1
            out["sum_f"] += f
            if m2 > out["max_m2"]:
                out["max_m2"] = m2
            if ok_m:
                out["count_m"] += 1
                out["sum_m"] += m
                if m < out["min_m"]:
                    out["min_m"] = m
            if ok_fx:
                out["count_fx"] += 1
                k = amx.f32_key_py(b)
                if lo is None or k < lo[0]:
                    lo = (k, b)
                if hi is None or k > hi[0]:
                    hi = (k, b)
        out["sum_m"] %= 1 << 64

        def widen(slot, empty):
            b = empty if slot is None else slot[1]
            if (b & 0x7FFFFFFF) > 0x7F800000:
                b = amx.CANON_NAN
            return amx.f32_bits_to_f64_bits(b)
        out["min_fx"] = widen(lo, amx.POS_INF)
        out["max_fx"] = widen(hi, amx.NEG_INF)
        return out


@functools.lru_cache(maxsize=None)
def matrix(name):
    return NullKeyMatrix(name)


# ---- the predicate lists of the GPU tests -------------------------------
ALL_M = ("m", cmx.GE, I64_MIN, 0)
ALL_M2 = ("m2", cmx.GE, I64_MIN, 0)
THIN = ("f", cmx.GE, 1020.0, 0.0)
STR_K1 = ("kstr", PREFIX, b"k1", 0)


def split(nk, col, op=cmx.LT, label="w31"):
    mx = nk.mx
    return (col, op, mx.split_literal(col, mx.probe_groups(col)[label]), 0)


def pred_lists(nk, group):
    """name -> (preds, nulls, keeps_null_group): every predicate list the GPU
    tests run with `group` as the nullable key. keeps_null_group is False
    for the lists meant to empty the NULL group."""
    return {
        "all": ((ALL_M,), (), True),
        "split": ((split(nk, "m"),), (), True),
        "two_staged": ((ALL_M, split(nk, "m2", cmx.GE, "w32")), (), True),
        "all_nulls": ((ALL_M2,), ("m", "fx"), True),
        "split_nulls": ((split(nk, "m2"),), ("m", "fx"), True),
        "two_staged_nulls": ((ALL_M2, split(nk, "m", cmx.GE)), ("m", "fx"),
                             True),
        "key_ge_0": (((group, cmx.GE, 0, 0),), (), False),
        "key_isnull": (((group, cmx.ISNULL, 0, 0),), (), True),
        "key_notnull": (((group, cmx.NOTNULL, 0, 0), ALL_M), (), False),
        "strmask": ((STR_K1, split(nk, "m")), (), True),
    }
