"""The composite-group-key matrix (tests/multikey_matrix.py) is what it claims:
its reference agrees with a plain-Python dict, the tuple counts and the
max_groups of every GPU case are what the cases assume, the restated hash has
the collisions the SDB_MK_HASH_BITS cases rely on, and the public surface of
the entry exists — all on the CPU. The GPU half is
tests/test_gpu_multikey_matrix.py."""

import ctypes
import os
import re

import numpy as np
import pytest

import agg_matrix as amx
import col_matrix as cmx
import multikey_matrix as mkx
import nullkey_matrix as nkx
import serenedb_amd as sa

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module", params=mkx.GEOMS)
def mk(request):
    return mkx.matrix(request.param)


# ---- public surface (fails before the entry exists) -----------------------
def test_public_surface():
    hdr = open(os.path.join(REPO, "include", "sdb_gpu.h")).read()
    assert re.search(r"^#define\s+SDB_ERR_COLLISION\s+\(-6\)", hdr, re.M)
    m = re.search(r"^#define\s+SDB_MAX_GROUP_KEYS\s+(\d+)", hdr, re.M)
    assert m and int(m.group(1)) == mkx.MAX_GROUP_KEYS == 4
    assert re.search(r"^int\s+sdb_gpu_scan_agg_hash_multi\s*\(", hdr, re.M)
    assert "SDB_MK_HASH_BITS" in hdr
    lib = ctypes.CDLL(os.path.join(REPO, "serenedb_amd", "libsdb_gpu.so"))
    assert hasattr(lib, "sdb_gpu_scan_agg_hash_multi")
    assert callable(getattr(sa.GpuContext, "scan_agg_hash_multi", None))


def test_header_states_the_restated_hash():
    """the constants and steps of mkx.mix64 / mkx.tuple_hash as the header
    gives them"""
    hdr = open(os.path.join(REPO, "include", "sdb_gpu.h")).read().lower()
    for piece in ("h = mix64(seed + 1)", "0xbf58476d1ce4e5b9",
                  "0x94d049bb133111eb", "x >> 30", "x >> 27", "x >> 31",
                  "h = mix64(h ^ nullmask)", "h &= hash_mask"):
        assert piece in hdr, piece
    # splitmix64's published first output for state 0 pins the finaliser
    assert mkx.mix64(0x9E3779B97F4A7C15) == 0xE220A8397B1DCDAF
    assert mkx.tuple_hash((1, 2)) != mkx.tuple_hash((2, 1))
    assert mkx.tuple_hash((None, 0)) != mkx.tuple_hash((0, None))
    assert mkx.tuple_hash((None, 0)) != mkx.tuple_hash((0, 0))
    assert mkx.tuple_hash((5,), seed=0) != mkx.tuple_hash((5,), seed=1)


# ---- the reference ---------------------------------------------------------
def dict_witness(mk, group_cols, preds, nulls, step):
    """GROUP BY in a plain Python loop over the sampled passing rows: tuple
    (None = NULL) -> [count, count(m), sum(m) mod 2^64, min(m), max(m2)]"""
    nk = mk.nk
    rows = np.flatnonzero(mk.passing(preds, nulls, step))
    vm = (nk.valid["m"] if "m" in nulls else np.ones(nk.rows, bool))[rows]
    keycols = [(nk.cols[c][rows].tolist(), nk.valid[c][rows].tolist())
               for c in group_cols]
    out = {}
    for i, (ok_m, m, m2) in enumerate(zip(vm.tolist(),
                                          nk.cols["m"][rows].tolist(),
                                          nk.cols["m2"][rows].tolist())):
        tup = tuple(v[i] if ok[i] else None for v, ok in keycols)
        g = out.setdefault(tup, [0, 0, 0, cmx.I64_MAX, cmx.I64_MIN])
        g[0] += 1
        g[4] = max(g[4], m2)
        if ok_m:
            g[1] += 1
            g[2] = (g[2] + m) % (1 << 64)
            g[3] = min(g[3], m)
    return out


def order_key(tup):
    """tuples ascending, column by column, NULL last in its column"""
    return tuple((k is None, 0 if k is None else k) for k in tup)


WITNESS_AGGS = ((None, mkx.C), ("m", mkx.CC), ("m", amx.SUM_I64),
                ("m", amx.MIN_I64), ("m2", amx.MAX_I64))


@pytest.mark.parametrize("group_cols,preds,nulls", [
    (("kmod", "ksparse"), (), ()),
    (("key", "kmod"), (), ("m",)),
    (("key", "kmod", "ksparse"), mkx.KEY_BETWEEN, ()),
    (("ksparse",), (("kmod", cmx.ISNULL, 0, 0),), ("m",)),
    (("key", "kmod", "key", "ksparse"), (), ()),
], ids=lambda v: None)
def test_reference_against_a_python_dict(mk, group_cols, preds, nulls):
    step = 7 if mk.name == "chunk" else 1       # odd_t33: every row
    keys, keynull, i64, f64, passed = mk.ref(group_cols, preds, WITNESS_AGGS,
                                             nulls, step)
    want = dict_witness(mk, group_cols, preds, nulls, step)
    assert passed == sum(g[0] for g in want.values()) > 0
    got = [tuple(None if n else int(k) for k, n in zip(kr, nr))
           for kr, nr in zip(keys.tolist(), keynull.tolist())]
    assert got == sorted(want, key=order_key)
    assert not keys[keynull].any()              # 0 in a NULL position
    for row, tup in zip(i64.tolist(), got):
        assert [v % (1 << 64) if q == 2 else v
                for q, v in enumerate(row)] == want[tup], tup
    assert not f64.any()
    # the edge rows are in the sample and NULL in `key` and `kmod`
    if step > 1:
        assert mk.sample(step)[[0, mk.rows - 1, *nkx.WORD_EDGE]].all()
    if group_cols[0] == "kmod" and not preds:
        assert (None, None) in want and any(
            a is None and b is not None for a, b in want)


def test_reference_ignores_what_null_rows_store(mk):
    """the tuples come from the clean arrays under the planes: none of the
    poison values that no valid row holds shows up as a key"""
    for codec in ("raw", "for"):
        dead = set(mk.nk.poison_values["kmod", codec]) - set(
            range(amx.NKMOD))
        assert dead
        tuples = mk.tuples(("kmod", "ksparse"))
        assert not dead & {t[0] for t in tuples}
    assert not any(t[0] == nkx.NULL_KMOD for t in tuples)
    assert any(t[1] == -1 for t in tuples)      # key -1 is live in ksparse
    assert {cmx.I64_MIN, cmx.I64_MAX} <= {t[1] for t in tuples}


# ---- group counts ----------------------------------------------------------
def test_distinct_tuple_counts(mk):
    for group_cols, by_geom in mkx.DISTINCT.items():
        keys, keynull, i64, _, passed = mk.ref(group_cols, (),
                                               mkx.AGGS_COUNT)
        assert len(keys) == by_geom[mk.name], group_cols
        assert passed == mk.rows == int(i64[:, 0].sum())
    assert len(mk.tuples(("kmod", "ksparse"))) == 182
    # four null-ness classes in the 182
    keys, keynull, _, _, _ = mk.ref(("kmod", "ksparse"), (), mkx.AGGS_COUNT)
    assert {tuple(r) for r in keynull.tolist()} == {
        (False, False), (False, True), (True, False), (True, True)}
    # a repeated column adds no tuple
    assert len(mk.ref(("key", "kmod", "key", "ksparse"), (),
                      mkx.AGGS_COUNT)[0]) == mkx.DISTINCT[
                          "key", "kmod", "ksparse"][mk.name]


def test_every_gpu_case_fits_its_max_groups(mk):
    cases = dict(mkx.ARMS, spill=mkx.SPILL, **mkx.pred_cases(mk.name))
    for name, (group_cols, max_groups, preds, aggs, nulls) in cases.items():
        n = len(mk.ref(group_cols, preds, mkx.AGGS_COUNT, nulls)[0])
        assert n <= max_groups, (name, n)
        assert (n == 0) == (name == "nothing"), (name, n)
        assert len(group_cols) <= mkx.MAX_GROUP_KEYS and len(aggs) <= 8
    # the arms take the table they are named for
    lds = mkx.ARMS["lds"]
    assert mkx.lds_slots(len(lds[3]), len(lds[0]), lds[1]) == 1024
    for name in ("global_2", "global_3", "global_4_repeat"):
        g = mkx.ARMS[name]
        assert mkx.lds_slots(len(g[3]), len(g[0]), g[1]) == 0, name


def test_lds_spill_case(mk):
    group_cols, max_groups, preds, aggs, nulls = mkx.SPILL
    slots = mkx.lds_slots(len(aggs), len(group_cols), max_groups)
    assert slots == 2048 and max_groups == 2 * slots     # staging still on
    assert mkx.lds_slots(len(aggs), len(group_cols), max_groups + 1) == 0
    n = len(mk.ref(group_cols, preds, aggs, nulls)[0])
    assert slots < n <= 2 * slots, n
    # odd_t33 fits one raw row group: one workgroup meets every tuple
    assert mkx.matrix("odd_t33").rows <= mkx.RAW_TILE


def test_sizing_rule():
    assert mkx.lds_slots(1, 1, 1) == 2048       # 6 words: 3200 -> 2048
    assert mkx.lds_slots(8, 4, 1) == 512        # 19 words: 1010 -> 512
    for naggs in range(1, 9):
        for nkeys in range(1, 5):
            s = mkx.lds_slots(naggs, nkeys, 1)
            words = 1 + naggs + 2 * nkeys + 2
            assert s & (s - 1) == 0 and s * 8 * words <= 150 * 1024
            assert 2 * s * 8 * words > 150 * 1024 or s == 1 << 14


# ---- the collision hook ----------------------------------------------------
def test_hook_facts(mk):
    tuples = mk.tuples(("kmod", "ksparse"))
    assert len(tuples) == 182
    assert [mkx.collides(tuples, s, 13) for s in range(4)][:2] == [True,
                                                                   False]
    assert all(mkx.collides(tuples, s, 12) for s in range(4))
    assert all(mkx.collides(tuples, s, 2) for s in range(4))    # pigeonhole
    assert not any(mkx.collides(tuples, s, 17) for s in range(4))
    assert not mkx.collides(tuples, 0, 64)
    # no case of the GPU file collides at 64 bits under seed 0
    for group_cols in mkx.DISTINCT:
        assert not mkx.collides(mk.tuples(group_cols), 0, 64), group_cols
