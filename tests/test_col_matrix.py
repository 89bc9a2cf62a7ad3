"""The column-codec matrix (tests/col_matrix.py) is what it claims, and its
references are sound — all on the CPU. The GPU half is
tests/test_gpu_col_matrix.py."""

import numpy as np
import pytest

import col_matrix as cmx
import serenedb_amd as sa

GEOMS = tuple(cmx.GEOMETRIES)
ALL_PASS = (("m", cmx.GE, cmx.I64_MIN, 0),)


@pytest.fixture(scope="module", params=GEOMS)
def mx(request):
    return cmx.matrix(request.param)


def test_geometry(mx):
    group_rows, nfull, tail = cmx.GEOMETRIES[mx.name]
    assert mx.rows == group_rows * nfull + tail
    assert mx.bounds[-1] == (group_rows * nfull, mx.rows)
    assert mx.n_rowgroups == 34 and mx.ngroups == 1088
    assert group_rows % 2 == 0 or mx.name.startswith("odd")
    assert group_rows % 64 != 0          # validity words straddle groups
    if mx.name == "chunk":
        assert mx.rows == 544003
        assert group_rows % 8192 == 98 and 98 % 32 != 0
    assert (mx.rows - group_rows * nfull) % 2 == 1   # odd tail group


@pytest.mark.parametrize("col", ["m", "m2"])
def test_widths_are_the_permutation(mx, col):
    wc = mx.width_col(col)
    order = {"m": mx.order, "m2": mx.order2}[col]
    hdr, desc = cmx.parse_col_blob(mx.blob(col))
    assert hdr["magic"] == 0x31304C4F43424453
    assert (hdr["rows"], hdr["group_rows"], hdr["ngroups"]) == \
        (mx.rows, mx.group_rows, mx.n_rowgroups)
    got = [d["width"] for d in desc]
    tail_w = 0 if mx.bounds[-1][1] - mx.bounds[-1][0] == 1 else 13
    assert got == order + [tail_w]
    assert got == wc.widths
    assert sorted(got[:-1]) == list(range(33))      # every width 0..32
    for g, (r0, r1) in enumerate(mx.bounds):
        x = mx.cols[col][r0:r1]
        assert desc[g]["vmin"] == int(x.min()) == desc[g]["base"], g
        assert desc[g]["vmax"] == int(x.max()), g
        if r1 - r0 > 1:
            assert desc[g]["base"] == wc.bases[g], g
            assert desc[g]["vmax"] - desc[g]["vmin"] == (1 << got[g]) - 1
    # both extreme bases really occur, at widths above 2 bits
    assert any(b == cmx.I64_MIN and w > 2
               for b, w in zip(wc.bases, wc.widths))
    assert any(b + (1 << w) - 1 == cmx.I64_MAX and w > 2
               for b, w in zip(wc.bases, wc.widths))
    assert int(mx.cols[col].min()) == cmx.I64_MIN
    assert int(mx.cols[col].max()) == cmx.I64_MAX


def test_predicate_columns_differ_in_width_everywhere(mx):
    full = mx.n_rowgroups - 1
    assert all(a != b for a, b in zip(mx.m.widths[:full],
                                      mx.m2.widths[:full]))


def test_key_column(mx):
    _, desc = cmx.parse_col_blob(mx.blob("key"))
    assert int(mx.key.min()) == 0 and int(mx.key.max()) < mx.ngroups <= 2048
    rg = np.arange(mx.rows) // mx.group_rows
    np.testing.assert_array_equal(mx.key // cmx.KEYS_PER_RG, rg)
    widths = {d["width"] for d in desc[:-1]}
    assert widths == set(range(6))
    for g, d in enumerate(desc):
        assert d["width"] == mx.key_width(g)


@pytest.mark.parametrize("col", ["m", "m2", "key"])
def test_round_trip(mx, col):
    out = sa.decode_col_i64(mx.blob(col), mx.rows)
    np.testing.assert_array_equal(out, mx.cols[col])


def test_minus_one_key_sits_inside_a_for_group(mx):
    r = mx.minus_one_row
    rg = r // mx.group_rows
    assert mx.m.vals[r] == -1 and mx.m.kinds[rg] == "minus5"
    assert mx.m.widths[rg] >= 4 and mx.f[r] == np.float32(1023.0)
    # the forced row moved neither the group's bounds nor its absent value
    x = mx.m.vals[slice(*mx.bounds[rg])]
    assert int(x.min()) == -5
    assert int(x.max()) == -5 + (1 << mx.m.widths[rg]) - 1


@pytest.mark.parametrize("col", ["m", "m2"])
def test_probe_literals(mx, col):
    wc = mx.width_col(col)
    probes = mx.probe_groups(col)
    assert set(probes) == {"w1", "w2", "w31", "w32", "int64_min",
                           "int64_max", "tail"}
    assert len(set(probes.values())) == len(probes)
    for label, rg in probes.items():
        x = mx.cols[col][slice(*mx.bounds[rg])]
        lit = mx.split_literal(col, rg)
        assert cmx.fits_i64(lit)
        if wc.widths[rg]:
            assert (x < lit).any() and (x >= lit).any(), label
        cases = {c[0]: c for c in mx.zonemap_cases(col, rg)}
        assert cases["lt_vmin"][2] == int(x.min())
        assert cases["ge_vmax"][2] == int(x.max())
        if int(x.max()) == cmx.I64_MAX:     # unrepresentable: left out
            assert "ge_vmax+1" not in cases
            assert "between_above" not in cases
        else:
            assert cases["ge_vmax+1"][2] == int(x.max()) + 1
        if wc.widths[rg] >= 2:
            absent = cases["eq_absent"][2]
            assert int(x.min()) < absent < int(x.max())
            assert not (x == absent).any(), label
        for _, _, lo, hi in cases.values():
            assert cmx.fits_i64(lo) and cmx.fits_i64(hi)
    assert wc.kinds[probes["int64_min"]] == "int64_min"
    assert wc.kinds[probes["int64_max"]] == "int64_max"


def test_validity_planes(mx):
    for col in ("m", "f"):
        v = mx.valid[col]
        assert 0.2 < 1.0 - v.mean() < 0.3
        words = mx.validity_words(col)
        assert len(words) == (mx.rows + 63) // 64
        r = np.arange(mx.rows)
        got = (words[r >> 6] >> (r & 63).astype(np.uint64)) & np.uint64(1)
        np.testing.assert_array_equal(got.astype(bool), v)
        # NULLs on both sides of every row-group boundary somewhere
        edge = [r0 for r0, _ in mx.bounds[1:]]
        assert not v[edge].all() and not v[[e - 1 for e in edge]].all()


@pytest.mark.parametrize("col", ["m", "m2", "key"])
def test_sum_i64_references_agree(mx, col):
    """uint64 np.add.at == Python integers mod 2^64, wrap-around included"""
    i64, _, passed = mx.ref_scan(ALL_PASS, ((col, cmx.SUM_I64),))
    assert passed == mx.rows
    want = mx.sum_i64_python(ALL_PASS, col)
    assert [int(x) % (1 << 64) for x in i64[:, 0]] == want
    if col != "key":        # some slot's true sum really leaves int64
        true = [0] * mx.ngroups
        for k, v in zip(mx.key.tolist(), mx.cols[col].tolist()):
            true[k] += v
        assert any(not cmx.fits_i64(t) for t in true)


def test_sum_i64_reference_with_nulls(mx):
    preds = (("m", cmx.LT, 1 << 39, 0),)
    i64, _, passed = mx.ref_scan(preds, ((None, cmx.COUNT),
                                         ("m", cmx.SUM_I64)), ("m",))
    mask = (mx.m.vals < (1 << 39)) & mx.valid["m"]
    assert passed == int(mask.sum()) == int(i64[:, 0].sum())
    want = mx.sum_i64_python(preds, "m", ("m",))
    assert [int(x) % (1 << 64) for x in i64[:, 1]] == want


def test_f_sums_are_order_independent(mx):
    f = mx.f
    assert np.all(f * 8 == np.round(f * 8)) and np.abs(f).max() < 1024
    assert not np.signbit(f[f == 0]).any()      # no -0.0 to disagree on
    _, f64, _ = mx.ref_scan(ALL_PASS, (("f", cmx.SUM_F64),))
    rng = np.random.default_rng(7)
    for _ in range(3):
        perm = rng.permutation(mx.rows)
        got = np.bincount(mx.key[perm], weights=f[perm].astype(np.float64),
                          minlength=mx.ngroups)
        np.testing.assert_array_equal(got.view(np.uint64),
                                      f64[:, 0].view(np.uint64))
    # and pairwise (np.sum) per key agrees with the sequential bincount
    for k in (0, 31, 500, mx.ngroups - 32):
        assert float(f[mx.key == k].astype(np.float64).sum()) == f64[k, 0]


def test_ref_hash_matches_ref_scan_on_the_dense_key(mx):
    preds = (("m2", cmx.LT, 0, 0),)
    aggs = ((None, cmx.COUNT), ("m", cmx.SUM_I64), ("f", cmx.SUM_F64))
    keys, hi, hf, hp = mx.ref_hash("key", preds, aggs)
    di, df, dp = mx.ref_scan(preds, aggs)
    assert hp == dp
    np.testing.assert_array_equal(keys, np.flatnonzero(di[:, 0]))
    np.testing.assert_array_equal(hi, di[keys])
    np.testing.assert_array_equal(hf, df[keys])
