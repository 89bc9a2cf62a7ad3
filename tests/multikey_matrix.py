"""Composite-group-key matrix: the numpy reference of GROUP BY over 1 to 4
nullable key columns, the Python restatement of the tuple hash, the LDS sizing
rule, and the cases of the GPU tests. Built on the NULL-group-key matrix
(tests/nullkey_matrix.py): its geometries, its key columns `key`, `kmod` and
`ksparse` with their planes and poisoned arrays, its predicate masks.
tests/test_multikey_matrix.py proves this file on the CPU;
tests/test_gpu_multikey_matrix.py runs sdb_gpu_scan_agg_hash_multi against it.

A group is a distinct tuple with None for NULL: in each position NULL is a
value of its own, equal only to NULL. The reference builds, for the passing
rows, one (is_null, value) column pair per key position — value 0 where NULL,
so what a NULL row stores never enters — finds the distinct rows of that
array (np.unique sorts them by column: NULL last in its column, values as
signed int64) and feeds the group ids to AggMatrix.agg_column, the aggregate
references of the sibling matrices. Every key column's plane counts as
attached, as it is on the GPU tables. Nothing asks the code under test for an
expected value.
"""

import functools

import numpy as np

import agg_matrix as amx
import col_matrix as cmx
import nullkey_matrix as nkx

GEOMS = nkx.GEOMS
KEYCOLS = nkx.KEYCOLS
I64_MIN, I64_MAX = cmx.I64_MIN, cmx.I64_MAX
MAX_GROUP_KEYS = 4
M64 = (1 << 64) - 1
HKEY_EMPTY = M64            # the tables' empty marker

C, CC = amx.COUNT, amx.COUNT_COL
AGGS_ALL = ((None, C), ("m", CC), ("m", amx.SUM_I64), ("f", amx.SUM_F64),
            ("m", amx.MIN_I64), ("m2", amx.MAX_I64), ("fx", amx.MIN_F32),
            ("fx", amx.MAX_F32))
AGGS_COUNT = ((None, C),)

# distinct tuples over all rows, by geometry (test_multikey_matrix proves them)
DISTINCT = {
    ("kmod", "ksparse"): {"odd_t33": 182, "chunk": 182},
    ("key", "kmod"): {"odd_t33": 10020, "chunk": 17803},
    ("key", "kmod", "ksparse"): {"odd_t33": 15499, "chunk": 47466},
}


# ---- the hash, restated from include/sdb_gpu.h --------------------------
def mix64(x):
    """splitmix64 finaliser on a Python int"""
    x &= M64
    x ^= x >> 30
    x = x * 0xBF58476D1CE4E5B9 & M64
    x ^= x >> 27
    x = x * 0x94D049BB133111EB & M64
    x ^= x >> 31
    return x


def tuple_hash(tup, seed=0, bits=64):
    """the 64-bit hash of a tuple (None = NULL) under `seed`, cut to `bits`
    bits as SDB_MK_HASH_BITS does"""
    h = mix64(seed + 1)
    nullmask = 0
    for j, k in enumerate(tup):
        if k is None:
            nullmask |= 1 << j
        h = mix64(h ^ (0 if k is None else k & M64))
    h = mix64(h ^ nullmask)
    h &= (1 << bits) - 1
    if h == HKEY_EMPTY:
        h -= 1
    return h


def collides(tuples, seed, bits):
    """two of the distinct tuples share a hash"""
    return len({tuple_hash(t, seed, bits) for t in tuples}) < len(set(tuples))


def lds_slots(naggs, nkeys, max_groups):
    """the documented sizing rule: the largest power of two <= 16384 with
    slots * 8 * (1 + naggs + 2*nkeys + 2) <= 150 KiB; 0 (no LDS staging)
    when max_groups > 2 * slots"""
    slots = 1 << 14
    while slots * 8 * (1 + naggs + 2 * nkeys + 2) > 150 * 1024:
        slots >>= 1
    return 0 if max_groups > 2 * slots else slots


class _Rows:
    """what AggMatrix.agg_column asks of its matrix, over a row subset"""

    def __init__(self, nk, keep):
        self.nk, self.keep = nk, keep
        self.cols, self.fx_bits = nk.cols, nk.fx_bits

    def selected(self, preds, col, op, nulls):
        return self.nk.selected(preds, col, op, nulls) & self.keep


class MultiKeyMatrix:
    def __init__(self, name):
        self.name = name
        self.nk = nk = nkx.matrix(name)
        self.rows = nk.rows

    def sample(self, step):
        """every step-th row plus the edge rows of the planes: the first and
        the last row, the word-edge rows and their neighbours, the first rows
        of the all-NULL and the NULL-free row group"""
        G = self.nk.mx.group_rows
        keep = np.zeros(self.rows, dtype=bool)
        keep[::step] = True
        edge = [0, self.rows - 1, *range(nkx.WORD_EDGE[0] - 1,
                                         nkx.WORD_EDGE[1] + 2)]
        for rg in (nkx.ALL_NULL_RG, nkx.NO_NULL_RG):
            edge += range(rg * G, rg * G + 3)
        keep[edge] = True
        return keep

    def passing(self, preds, nulls=(), step=None):
        nulls = tuple(nulls) + KEYCOLS
        mask = self.nk.pred_mask(tuple(preds), nulls)
        return mask if step is None else mask & self.sample(step)

    def tuples(self, group_cols, preds=(), nulls=(), step=None):
        """the distinct tuples of the passing rows as a set of Python tuples
        with None for NULL"""
        mask = self.passing(preds, nulls, step)
        cols = [np.where(self.nk.valid[c], self.nk.cols[c], 0)[mask].tolist()
                for c in group_cols]
        null = [(~self.nk.valid[c])[mask].tolist() for c in group_cols]
        return {tuple(None if n else v for v, n in zip(vs, ns))
                for vs, ns in zip(zip(*cols), zip(*null))}

    @functools.lru_cache(maxsize=None)
    def ref(self, group_cols, preds, aggs, nulls=(), step=None):
        """(keys int64 [n, nkeys], keynull bool [n, nkeys], i64 [n, naggs],
        f64 [n, naggs], rows_passed), laid out like
        GpuContext.scan_agg_hash_multi. nulls: the non-key columns whose
        plane is attached; step: only the rows of sample(step)."""
        nk = self.nk
        mask = self.passing(preds, nulls, step)
        nulls = tuple(nulls) + KEYCOLS
        pairs = np.zeros((int(mask.sum()), 2 * len(group_cols)),
                         dtype=np.int64)
        for j, c in enumerate(group_cols):
            v = nk.valid[c][mask]
            pairs[:, 2 * j] = ~v
            pairs[:, 2 * j + 1] = np.where(v, nk.cols[c][mask], 0)
        uniq, inv = np.unique(pairs, axis=0, return_inverse=True)
        n = len(uniq)
        dense = np.full(self.rows, n, dtype=np.int64)
        dense[mask] = inv.reshape(-1)
        src = _Rows(nk, np.ones(self.rows, bool) if step is None
                    else self.sample(step))
        i64, f64 = amx.AggMatrix._pack(
            [amx.AggMatrix.agg_column(src, dense, n + 1, tuple(preds), c, op,
                                      nulls) for c, op in aggs], aggs)
        keys = uniq[:, 1::2].copy()
        keynull = uniq[:, 0::2].astype(bool)
        for a in (keys, keynull):
            a.setflags(write=False)
        return keys, keynull, i64[:n], f64[:n], int(mask.sum())


@functools.lru_cache(maxsize=None)
def matrix(name):
    return MultiKeyMatrix(name)


# ---- the cases of the GPU tests ------------------------------------------
ALL = ()                        # no predicate: every row passes
NOTHING = (("m2", cmx.LT, I64_MIN, 0),)
KEY_BETWEEN = (("key", cmx.BETWEEN, 40, 400),)
# lds_spill: naggs = 1 and nkeys = 2 give 2048 LDS slots, staging on up to
# max_groups = 4096. (key, kmod) under this predicate on `key` has more
# tuples than slots and at most 4096 in both geometries, so the LDS tables
# flush into a global table that holds more tuples than any of them could.
# Each workgroup owns one row group, though, and no row group holds that
# many. But the GPU test also runs every case on an all-raw table, which
# tiles at RAW_TILE rows: odd_t33 is ONE row group there, one workgroup sees
# every tuple, and by pigeonhole rows must miss the full LDS table and go to
# the global one while the tuples that got a slot flush from LDS.
SPILL_PRED = ("key", cmx.BETWEEN, 0, 300)
SPILL_MAX_GROUPS = 4096
RAW_TILE = 65536            # the row group of a table without a FoR column

# name -> (group columns, max_groups, preds, aggs, nulls)
ARMS = {
    "lds": (("kmod", "ksparse"), 256, ALL, AGGS_ALL, ()),
    "global_2": (("key", "kmod"), 1 << 16, ALL, AGGS_ALL, ()),
    "global_3": (("key", "kmod", "ksparse"), 1 << 16, ALL, AGGS_ALL, ()),
    "global_4_repeat": (("key", "kmod", "key", "ksparse"), 1 << 16, ALL,
                        AGGS_ALL, ()),
}


SPILL = (("key", "kmod"), SPILL_MAX_GROUPS, (SPILL_PRED,), AGGS_COUNT, ())


def pred_cases(name):
    """name -> (group columns, max_groups, preds, aggs, nulls)"""
    nk = nkx.matrix(name)
    return {
        "between_key": (("key", "kmod"), 1 << 16, KEY_BETWEEN, AGGS_ALL, ()),
        "isnull_notnull": (("kmod", "ksparse"), 256,
                           (("kmod", cmx.ISNULL, 0, 0),
                            ("ksparse", cmx.NOTNULL, 0, 0)), AGGS_ALL, ()),
        "notnull_isnull": (("key", "kmod"), 1 << 16,
                           (("key", cmx.NOTNULL, 0, 0),
                            ("kmod", cmx.ISNULL, 0, 0)), AGGS_ALL, ()),
        "m_plane": (("kmod", "ksparse"), 256, (nkx.split(nk, "m"),),
                    AGGS_ALL, ("m", "fx")),
        "strmask": (("kmod", "ksparse"), 256, (nkx.STR_K1,), AGGS_ALL, ()),
        "nothing": (("kmod", "ksparse"), 256, NOTHING, AGGS_ALL, ()),
    }


def aggs_on_key(group):
    return ((None, C), (group, amx.SUM_I64), (group, CC),
            (group, amx.MIN_I64), (group, amx.MAX_I64))
