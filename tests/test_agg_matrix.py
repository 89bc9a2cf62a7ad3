"""The aggregate matrix (tests/agg_matrix.py) is what it claims and its
references are sound — all on the CPU. The GPU half is
tests/test_gpu_agg_matrix.py."""

import os
import re

import numpy as np
import pytest

import agg_matrix as amx
import col_matrix as cmx
import serenedb_amd as sa

ALL_M = ("m", cmx.GE, cmx.I64_MIN, 0)
ALL_M2 = ("m2", cmx.GE, cmx.I64_MIN, 0)
EQ_MIN = ("m", cmx.EQ, cmx.I64_MIN, 0)
EQ_MAX = ("m", cmx.EQ, cmx.I64_MAX, 0)
FX_SMALL = ("fx", cmx.BETWEEN, -1.0, 1.0)


@pytest.fixture(scope="module", params=amx.GEOMS)
def am(request):
    return amx.matrix(request.param)


def split_m2(am):
    mx = am.mx
    return ("m2", cmx.LT, mx.split_literal("m2", mx.probe_groups("m2")["w31"]),
            0)


def test_agg_ops_match_the_header():
    """GpuContext.AGG_OPS carries the SdbAggOp values of include/sdb_gpu.h"""
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(
        os.path.abspath(__file__))), "include", "sdb_gpu.h")).read()
    body = re.search(r"typedef enum SdbAggOp \{(.*?)\} SdbAggOp;", hdr,
                     re.S).group(1)
    parsed = {name.lower(): int(val) for name, val in
              re.findall(r"SDB_AGG_(\w+)\s*=\s*(\d+)", body)}
    assert parsed == sa.GpuContext.AGG_OPS
    assert sorted(parsed.values()) == list(range(8))
    assert (amx.COUNT_COL, amx.MIN_I64, amx.MAX_I64, amx.MIN_F32,
            amx.MAX_F32) == tuple(parsed[k] for k in (
                "count_col", "min_i64", "max_i64", "min_f32", "max_f32"))


def test_f32_key_is_strictly_monotone_and_round_trips():
    ladder = np.array(amx.LADDER, dtype=np.uint32)
    vals = ladder.view(np.float32)
    finite = vals[:-1]
    assert np.all(finite[:-1] <= finite[1:])    # the ladder really ascends
    assert np.isnan(vals[-1])
    keys = amx.f32_key(ladder)
    assert np.all(keys[:-1] < keys[1:])
    assert keys.min() > 0 and keys.max() < 0xFFFFFFFF   # codes never hit 0
    np.testing.assert_array_equal(amx.f32_unkey(keys), ladder)
    assert [amx.f32_key_py(int(b)) for b in ladder] == keys.tolist()
    # every NaN, of either sign and any payload, is the one top key
    nan_keys = amx.f32_key(np.array(amx.NAN_BITS + (amx.NEG_NAN,),
                                    dtype=np.uint32))
    assert set(nan_keys.tolist()) == {int(keys[-1])}
    # -0.0 sorts strictly below +0.0
    assert amx.f32_key([0x80000000])[0] < amx.f32_key([0])[0]
    assert amx.f32_bits_to_f64_bits(0x80000000) == 1 << 63
    assert amx.F64_NAN == 0x7FF8000000000000


def test_geometry_has_the_edges(am):
    mx = am.mx
    assert mx.rows % 4 != 0                 # raw quad loop leaves a tail
    # every kmod group has rows in every full row group (the short tail
    # group cannot hold all 61), every key group lives in exactly one
    rg = np.arange(mx.rows) // mx.group_rows
    full = set(range(mx.n_rowgroups - 1))
    for k in range(amx.NKMOD):
        assert set(rg[am.kmod == k].tolist()) >= full
    assert np.all((mx.key // cmx.KEYS_PER_RG) == rg)


def test_one_geometry_has_odd_groups():
    assert any(amx.matrix(g).mx.group_rows % 2 for g in amx.GEOMS)
    assert all(amx.matrix(g).mx.rows % 4 for g in amx.GEOMS)


def test_inputs_contain_the_edges(am):
    mx = am.mx
    assert am.pred_mask((EQ_MIN,)).sum() >= 1
    assert am.pred_mask((EQ_MAX,)).sum() >= 1
    bits = am.fx_bits
    g = amx.FX_GROUPS
    nan = (bits & 0x7FFFFFFF) > 0x7F800000
    sel = am.kmod == g["all_nan"]
    assert nan[sel].all() and set(bits[sel].tolist()) == set(amx.NAN_BITS)
    assert {b >> 31 for b in amx.NAN_BITS} == {0, 1}
    sel = am.kmod == g["zeros"]
    assert set(bits[sel].tolist()) == {0, 0x80000000}
    sel = am.kmod == g["neg_nan_finite"]
    assert set(bits[sel][nan[sel]].tolist()) == {amx.NEG_NAN}
    assert np.isfinite(am.fx[sel][~nan[sel]]).all() and (~nan[sel]).sum() > 3
    assert set(bits[am.kmod == g["neg_inf"]].tolist()) == {amx.NEG_INF}
    assert set(bits[am.kmod == g["pos_inf"]].tolist()) == {amx.POS_INF}
    sel = am.kmod == g["denorm_fltmax"]
    assert set(bits[sel].tolist()) == set(amx.DENORM_BITS)
    others = ~np.isin(am.kmod, list(g.values()))
    assert np.isfinite(am.fx[others]).all()
    # planes: the ALL_NULL groups have no value, the rest lose about 25 %
    for col in ("m", "fx"):
        v = am.valid[col]
        null_group = np.isin(am.kmod, amx.ALL_NULL)
        assert not v[null_group].any()
        assert 0.70 < v[~null_group].mean() < 0.80
    # every designated group passes rows under each predicate set in use,
    # and keeps a non-NULL fx value where it is not an ALL_NULL group
    for preds in ((ALL_M,), (ALL_M2,), (split_m2(am),)):
        mask = am.pred_mask(preds)
        assert 0 < mask.sum()
        for k in tuple(g.values()) + amx.ALL_NULL:
            assert (mask & (am.kmod == k)).sum() > 0, (preds, k)
        for k in g.values():
            assert (mask & (am.kmod == k) & am.valid["fx"]).sum() > 0
    assert 0 < am.pred_mask((split_m2(am),)).sum() < mx.rows
    # the f32 predicate keeps only zeros and denormals of the special groups
    small = am.pred_mask((FX_SMALL,))
    assert small[am.kmod == g["zeros"]].all()
    assert not small[am.kmod == g["all_nan"]].any()
    sel = small & (am.kmod == g["denorm_fltmax"])
    assert set(bits[sel].tolist()) == set(amx.DENORM_BITS[:4])
    # hash by m under the thin predicate: fits 2048 groups, holds key -1
    thin = ("f", cmx.GE, 1020.0, 0.0)
    keys = am.ref_hash("m", (ALL_M2, thin), ((None, amx.COUNT),))[0]
    assert 16 < len(keys) <= 2048 and -1 in keys


def test_references_agree_with_the_python_witness(am):
    for group in ("key", "kmod"):
        for preds, nulls in (((ALL_M,), ()), ((split_m2(am),), ("m", "fx")),
                             ((FX_SMALL,), ())):
            aggs = (("m", amx.MIN_I64), ("m", amx.MAX_I64),
                    ("fx", amx.MIN_F32), ("fx", amx.MAX_F32))
            i64, f64, _, _ = am.ref_dense(group, preds, aggs, nulls)
            lo, hi = am.minmax_python(group, preds, "m", nulls)
            assert i64[:, 0].tolist() == lo and i64[:, 1].tolist() == hi
            lo, hi = am.minmax_python(group, preds, "fx", nulls)
            assert amx.f64_bits(f64[:, 2]).tolist() == lo
            assert amx.f64_bits(f64[:, 3]).tolist() == hi


def test_reference_values_of_the_designated_groups(am):
    """the numpy references give what the header promises"""
    aggs = ((None, amx.COUNT), ("fx", amx.COUNT_COL), ("fx", amx.MIN_F32),
            ("fx", amx.MAX_F32), ("m", amx.MIN_I64), ("m", amx.MAX_I64),
            ("m", amx.COUNT_COL))
    i64, f64, passed, present = am.ref_dense("kmod", (ALL_M2,), aggs,
                                             ("m", "fx"))
    assert passed == am.rows and present.all()
    lo, hi = amx.f64_bits(f64[:, 2]), amx.f64_bits(f64[:, 3])
    g = amx.FX_GROUPS
    assert lo[g["all_nan"]] == hi[g["all_nan"]] == amx.F64_NAN
    assert lo[g["zeros"]] == 1 << 63 and hi[g["zeros"]] == 0
    assert hi[g["neg_nan_finite"]] == amx.F64_NAN
    assert np.isfinite(f64[g["neg_nan_finite"], 2])
    assert f64[g["neg_inf"], 2] == f64[g["neg_inf"], 3] == -np.inf
    assert f64[g["pos_inf"], 2] == f64[g["pos_inf"], 3] == np.inf
    flt_max = float(np.finfo(np.float32).max)
    assert f64[g["denorm_fltmax"], 2] == -flt_max
    assert f64[g["denorm_fltmax"], 3] == flt_max
    for k in amx.ALL_NULL:
        assert i64[k, 0] > 0 and i64[k, 1] == 0 and i64[k, 6] == 0
        assert f64[k, 2] == np.inf and f64[k, 3] == -np.inf
        assert i64[k, 4] == cmx.I64_MAX and i64[k, 5] == cmx.I64_MIN
    live = ~np.isin(np.arange(amx.NKMOD), amx.ALL_NULL)
    assert np.all(i64[live, 1] > 0) and np.all(i64[live, 1] < i64[live, 0])
    # no plane: COUNT_COL is COUNT(*)
    i64, _, _, _ = am.ref_dense("kmod", (ALL_M2,), aggs)
    assert np.array_equal(i64[:, 1], i64[:, 0])
    assert np.array_equal(i64[:, 6], i64[:, 0])
    # the code-0 collisions: a real INT64_MIN / INT64_MAX versus no value
    for pred, q, want in ((EQ_MIN, 5, cmx.I64_MIN), (EQ_MAX, 4, cmx.I64_MAX)):
        i64, _, passed, present = am.ref_dense("key", (pred,), aggs)
        assert passed > 0 and 0 < present.sum() < len(present)
        assert np.all(i64[:, q] == want)
        assert np.all((i64[:, 6] > 0) == present)
    # SUM / COUNT of the old ops agree with col_matrix's own references
    old = ((None, cmx.COUNT), ("m", cmx.SUM_I64), ("f", cmx.SUM_F64))
    i64, f64, passed, _ = am.ref_dense("key", (split_m2(am),), old)
    ri, rf, rpassed = am.mx.ref_scan((split_m2(am),), old)
    assert passed == rpassed and np.array_equal(i64, ri)
    assert np.array_equal(amx.f64_bits(f64), amx.f64_bits(rf))
