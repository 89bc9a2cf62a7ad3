"""The NULL-group-key matrix (tests/nullkey_matrix.py) is what it claims and
its references are sound — all on the CPU. The GPU half is
tests/test_gpu_nullkey_matrix.py."""

import numpy as np
import pytest

import agg_matrix as amx
import col_matrix as cmx
import nullkey_matrix as nkx
import serenedb_amd as sa


@pytest.fixture(scope="module", params=nkx.GEOMS)
def nk(request):
    return nkx.matrix(request.param)


def test_wrapper_has_the_nullable_key_entries():
    for name in ("scan_agg_nullkey", "scan_agg_hash_nullkey"):
        assert callable(getattr(sa.GpuContext, name, None)), name


def test_planes_hold_the_edges(nk):
    mx, am = nk.mx, nk.am
    rows, G = nk.rows, mx.group_rows
    rg = np.arange(rows) // G
    assert rows % 4 and (rows - 1) >= (rows & ~3)   # last row: raw quad tail
    assert (rows - mx.bounds[-1][0]) % 2 == 1       # and an odd tail row
    for col in nkx.KEYCOLS:
        v = nk.valid[col]
        assert not v[0] and not v[rows - 1], col
        assert 0.15 < (~v).mean() < 0.35, (col, (~v).mean())
    for col in ("key", "kmod"):
        v = nk.valid[col]
        lo, hi = nkx.WORD_EDGE
        assert lo % 64 == 63 and hi == lo + 1
        assert not v[lo] and not v[hi] and v[lo - 1] and v[hi + 1]
        assert not v[rg == nkx.ALL_NULL_RG].any()
        for g in range(mx.n_rowgroups):
            if g in (nkx.ALL_NULL_RG, nkx.NO_NULL_RG):
                continue
            assert v[rg == g].any() and (~v[rg == g]).any(), (col, g)
    assert nk.valid["key"][rg == nkx.NO_NULL_RG].all()
    # the kmod plane: that row group is NULL in the rows of NULL_KMOD only
    in_rg = rg == nkx.NO_NULL_RG
    np.testing.assert_array_equal(~nk.valid["kmod"][in_rg],
                                  am.kmod[in_rg] == nkx.NULL_KMOD)
    assert not nk.valid["kmod"][am.kmod == nkx.NULL_KMOD].any()
    assert nkx.NULL_KMOD not in tuple(amx.FX_GROUPS.values()) + amx.ALL_NULL
    # every other kmod group, and every key group outside the all-NULL row
    # group, keeps valid rows
    kv = np.bincount(am.kmod[nk.valid["kmod"]], minlength=amx.NKMOD)
    assert np.all((kv > 0) == (np.arange(amx.NKMOD) != nkx.NULL_KMOD))
    kk = np.bincount(mx.key[nk.valid["key"]], minlength=mx.ngroups)
    present = np.bincount(mx.key, minlength=mx.ngroups) > 0
    gone = present & (kk == 0)
    assert set(np.flatnonzero(gone) // cmx.KEYS_PER_RG) == {nkx.ALL_NULL_RG}
    assert gone.sum() == (present[nkx.ALL_NULL_RG * cmx.KEYS_PER_RG:][
        :cmx.KEYS_PER_RG]).sum()


def test_ksparse_table():
    t = nkx.KSPARSE
    assert len(t) == amx.NKMOD == len(set(t.tolist()))
    for v in (nkx.I64_MIN, nkx.I64_MAX, 0, -1):
        assert v in t
    assert t[nkx.KSPARSE_MINUS_ONE] == -1
    assert (t < -(1 << 62)).any() and (t > (1 << 62)).any()


def test_poison_touches_null_rows_only(nk):
    for (col, codec), a in nk.poisoned.items():
        v = nk.valid[col]
        clean = nk.cols[col]
        np.testing.assert_array_equal(a[v], clean[v])
        cyc = nk.poison_values[col, codec]
        assert set(a[~v].tolist()) == set(cyc), (col, codec)
        assert -1 in cyc and nk.live[col] in cyc
        assert nk.live[col] in clean[v]
        if col in nk.groups:
            ng = nk.groups[col][1]
            assert ng in cyc and ng + 1000 in cyc
            # whole-column min / max would fail the dense range proof
            assert a.min() < 0 and a.max() >= ng
            if codec == "raw":
                assert nkx.I64_MIN in cyc and nkx.I64_MAX in cyc
        else:
            dead = set(cyc) - set(nkx.KSPARSE.tolist())
            assert len(dead) >= 3       # poison that is no live key at all


def test_poisoned_for_arrays_encode(nk):
    for (col, codec), a in nk.poisoned.items():
        if codec != "for":
            continue
        blob = sa.encode_col_i64(a, nk.mx.group_rows)
        np.testing.assert_array_equal(sa.decode_col_i64(blob, nk.rows), a)
    assert {c for c, k in nk.poisoned if k == "for"} == {"key", "kmod"}


AGGS_ALL = ((None, amx.COUNT), ("m", amx.COUNT_COL), ("m", amx.SUM_I64),
            ("f", amx.SUM_F64), ("m", amx.MIN_I64), ("m2", amx.MAX_I64),
            ("fx", amx.MIN_F32), ("fx", amx.MAX_F32))


def test_null_group_agrees_with_the_python_witness(nk):
    for group in ("key", "kmod"):
        lists = nkx.pred_lists(nk, group)
        for name in ("all", "split_nulls", "two_staged"):
            preds, nulls, _ = lists[name]
            i64, f64, passed, null_rows, present = nk.ref_dense(
                group, preds, AGGS_ALL, nulls)
            ng = nk.groups[group][1]
            w = nk.null_group_python(group, preds, nulls)
            assert null_rows == w["count"] == i64[ng, 0] > 0
            assert present[ng]
            assert i64[ng, 1] == w["count_m"]
            assert int(i64[ng, 2]) % (1 << 64) == w["sum_m"]
            assert f64[ng, 3] == w["sum_f"]
            assert i64[ng, 4] == w["min_m"] and i64[ng, 5] == w["max_m2"]
            assert int(amx.f64_bits(f64[ng, 6:7])[0]) == w["min_fx"]
            assert int(amx.f64_bits(f64[ng, 7:8])[0]) == w["max_fx"]
            # the hash reference holds the same NULL group
            h = nk.ref_hash(group, preds, AGGS_ALL, nulls)
            assert h[6] == null_rows and h[3] == passed
            assert np.array_equal(h[4], i64[ng])
            assert np.array_equal(amx.f64_bits(h[5]), amx.f64_bits(f64[ng]))
            np.testing.assert_array_equal(h[0], np.flatnonzero(present[:ng]))
            # rows_passed counts NULL-key rows; key groups hold the rest
            assert i64[:ng, 0].sum() + null_rows == passed


def test_key_groups_equal_the_agg_matrix_on_valid_rows(nk):
    """without NULLs the references are agg_matrix's own; with the plane, a
    key group shrinks to its valid rows and the all-NULL ones empty"""
    for group in ("key", "kmod"):
        ng = nk.groups[group][1]
        preds = (nkx.ALL_M,)
        i64, f64, passed, null_rows, _ = nk.ref_dense(
            group, preds, AGGS_ALL, plane=False)
        ri, rf, rpassed, _ = nk.am.ref_dense(group, preds, AGGS_ALL)
        assert null_rows == 0 and passed == rpassed
        assert np.array_equal(i64[:ng], ri)
        assert i64[ng].tolist() == [0, 0, 0, 0, nkx.I64_MAX, nkx.I64_MIN,
                                    0, 0]
        assert f64[ng].tolist() == [0, 0, 0, 0, 0, 0, np.inf, -np.inf]
        assert np.array_equal(amx.f64_bits(f64[:ng]), amx.f64_bits(rf))
        i64, _, _, _, present = nk.ref_dense(group, preds, AGGS_ALL)
        assert np.all(i64[:ng, 0] <= ri[:, 0])
        if group == "kmod":
            assert not present[nkx.NULL_KMOD] and ri[nkx.NULL_KMOD, 0] > 0
            assert i64[nkx.NULL_KMOD, 4] == nkx.I64_MAX
        else:
            lo = nkx.ALL_NULL_RG * cmx.KEYS_PER_RG
            assert not present[lo:lo + cmx.KEYS_PER_RG].any()


def test_key_predicates_and_key_aggregates(nk):
    for group in ("key", "kmod"):
        ng = nk.groups[group][1]
        lists = nkx.pred_lists(nk, group)
        aggs = ((None, amx.COUNT), (group, amx.SUM_I64),
                (group, amx.COUNT_COL), (group, amx.MIN_I64),
                (group, amx.MAX_I64))
        valid = nk.valid[group]
        i64, _, passed, null_rows, _ = nk.ref_dense(
            group, lists["all"][0], aggs)
        assert passed == nk.rows and null_rows == (~valid).sum()
        assert i64[ng].tolist() == [null_rows, 0, 0, nkx.I64_MAX,
                                    nkx.I64_MIN]
        live = i64[:ng, 0] > 0
        assert np.array_equal(i64[:ng, 2], i64[:ng, 0])
        ids = np.arange(ng)
        assert np.array_equal(i64[:ng, 1], ids * i64[:ng, 0])
        assert np.array_equal(i64[:ng][live, 3], ids[live])
        assert np.array_equal(i64[:ng][live, 4], ids[live])
        i64, _, passed, null_rows, _ = nk.ref_dense(
            group, lists["key_ge_0"][0], aggs)
        assert null_rows == 0 and passed == valid.sum() and not i64[ng, 0]
        i64, _, passed, null_rows, _ = nk.ref_dense(
            group, lists["key_isnull"][0], aggs)
        assert passed == null_rows == (~valid).sum() == i64[ng, 0]
        assert not i64[:ng, 0].any()
        _, _, passed, null_rows, _ = nk.ref_dense(
            group, lists["key_notnull"][0], aggs)
        assert null_rows == 0 and passed == valid.sum()


def test_hash_references_are_not_vacuous(nk):
    """under every predicate list of the GPU tests, bar those built to empty
    it, the reference NULL group has a passing row: filling absent hash
    groups from the reference cannot hide a lost NULL group"""
    for group in nkx.KEYCOLS:
        for name, (preds, nulls, keeps) in nkx.pred_lists(nk, group).items():
            h = nk.ref_hash(group, preds, ((None, amx.COUNT),), nulls)
            assert (h[6] > 0) == keeps, (group, name)
            assert h[3] > 0 and (len(h[0]) > 0 or name == "key_isnull")
            if keeps:
                assert h[4][0] == h[6]
    # ksparse: key -1 is a live valid key beside the NULL group
    preds, nulls, _ = nkx.pred_lists(nk, "ksparse")["all"]
    h = nk.ref_hash("ksparse", preds, ((None, amx.COUNT),), nulls)
    assert -1 in h[0] and len(h[0]) == amx.NKMOD and h[6] > 0
    # the string mask of the STRMASK case keeps k10 .. k19
    m = nk.str_mask(b"k1")
    assert set(nk.am.kmod[m].tolist()) == set(range(10, 20))
