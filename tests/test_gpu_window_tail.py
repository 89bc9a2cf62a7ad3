"""The sweep kernel's window tail on the window-tail matrix
(tests/window_tail_matrix.py): the candidate reservation issued first, the
threshold derivation beside it, the next window's snapshot, item counts and
staged descriptors fetched in the tail of the window before. Every case runs
at the smallest compiled geometry and the default one, with SDB_SWEEP_GRID at
1, 2, 3, 4, 8 and unset (workgroups of 10, 5, 4 + 4 + 2, 3 + 3 + 3 + 1, 2
and one window, and workgroups without any), and with the posting stage
unclamped and clamped to one slot per wave. Doc ids, score bits, totals and
hybrid buckets must equal the numpy fp32 reference exactly;
tests/test_window_tail_matrix.py proves that reference equals the CPU oracle
and that the corpus holds the shapes it claims."""

import ctypes as C
import itertools

import numpy as np
import pytest

import hybrid_matrix as hm
import round_stage_matrix as rs
import serenedb_amd as sa
import window_tail_matrix as wt

pytestmark = pytest.mark.gpu

ENV = ("SDB_TOPK_PATH", "SDB_SWEEP_GEOM", "SDB_SWEEP_ROUND_ITEMS",
       "SDB_SWEEP_GRID")
GEOMS = (wt.GEOM, None)          # None: the default geometry


@pytest.fixture(scope="module")
def m():
    return wt.matrix()


@pytest.fixture(scope="module")
def ctx():
    c = sa.GpuContext(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def seg(ctx, m):
    return ctx.load_segment(m.blob)


@pytest.fixture
def env(monkeypatch):
    for k in ENV:
        monkeypatch.delenv(k, raising=False)

    def set_(geom, grid, c=None):
        for k, v in (("SDB_SWEEP_GEOM", geom), ("SDB_SWEEP_GRID", grid),
                     ("SDB_SWEEP_ROUND_ITEMS", c)):
            if v is None:
                monkeypatch.delenv(k, raising=False)
            else:
                monkeypatch.setenv(k, str(v))
    return set_


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def configs(geom):
    """(grid, stage clamp): every grid with the stage unclamped and at one
    slot per wave"""
    nw = wt.NW if geom else 16
    return itertools.product(wt.GRIDS, (None, nw))


def last_grid(ctx):
    g = C.c_uint(0)
    assert ctx._lib.sdb_gpu_last_sweep_grid(ctx._ctx, C.byref(g)) == 0
    return g.value


def check(ctx, seg, m, terms, boosts, k, label, **kw):
    hits, total = ctx.execute_topk([seg], terms, boosts, k, **kw)
    rd, rsc, rtotal = m.ref_topk(terms, boosts, k, "bm25")
    if kw.get("wand"):           # under WAND the total counts visited docs
        assert total <= rtotal, label
    else:
        assert total == rtotal, label
    np.testing.assert_array_equal(hits["doc"], rd, err_msg=label)
    np.testing.assert_array_equal(bits(hits["score"]), bits(rsc),
                                  err_msg=label)


@pytest.mark.parametrize("geom", GEOMS, ids=("4096x256", "default"))
def test_cases(ctx, seg, m, env, geom):
    """window runs, windows without a reservation, term ends, the dense
    term and the k edges"""
    for grid, c in configs(geom):
        env(geom, grid, c)
        for label, terms, boosts, k in wt.cases(m):
            check(ctx, seg, m, terms, boosts, k,
                  f"{label} geom={geom} grid={grid} C={c}")


@pytest.mark.parametrize("geom", GEOMS, ids=("4096x256", "default"))
def test_early_threshold_keeps_candidates_few(ctx, seg, m, env, geom):
    """k = 3 on `early` in one workgroup: every spike is a candidate, and
    once the threshold has locked the quiet windows append nothing, so the
    candidates stay below the matches. (How many of the first windows'
    matches are appended depends on when the window's own histogram merge
    lands, so the count itself is only printed.)"""
    terms = m.groups["early"]
    env(geom, 1)
    check(ctx, seg, m, terms, [1.0], 3, f"early geom={geom}")
    ncand = C.c_uint(0)
    ctx._lib.sdb_gpu_last_stats(ctx._ctx, None, C.byref(ncand), None, None,
                                None)
    print(f"early geom={geom}: {ncand.value} candidates of "
          f"{wt.n_matches(m, terms)} matches, {len(m.spikes)} spikes")
    assert len(m.spikes) <= ncand.value <= wt.n_matches(m, terms)
    if geom:    # ten windows: the later quiet ones are behind the lock
        assert ncand.value < wt.n_matches(m, terms)


@pytest.mark.parametrize("geom", GEOMS, ids=("4096x256", "default"))
def test_live_mask(ctx, seg, m, env, geom):
    terms = m.groups["main"]
    boosts = rs.boosts_for(terms)
    live = wt.live_mask()
    ctx.attach_livemask(seg, wt.live_words(live))
    try:
        for grid, c in configs(geom):
            env(geom, grid, c)
            for k in (wt.DOC_COUNT, 10):
                hits, total = ctx.execute_topk([seg], terms, boosts, k)
                rd, rsc, rtotal = m.ref_topk_live(terms, boosts, k, "bm25",
                                                  live)
                assert total == rtotal
                np.testing.assert_array_equal(hits["doc"], rd)
                np.testing.assert_array_equal(bits(hits["score"]), bits(rsc))
    finally:
        ctx.attach_livemask(seg, None)
    check(ctx, seg, m, terms, boosts, 10, "mask detached")


@pytest.mark.parametrize("geom", GEOMS, ids=("4096x256", "default"))
def test_hybrid_buckets(ctx, env, geom):
    """the bucket flush in the tail, on hybrid_matrix's corpus (13 windows
    of 4096 docs, 3 of 24576) and reference"""
    mx = hm.matrix()
    hseg = ctx.load_segment(mx.seg.blob)
    for case in ("c01_ordinary", hm.FULL_SPAN[0]):
        lo, hi, nb = hm.CASES[case]
        ctx.attach_column(hseg, mx.bucket_col(case)[0])
        ref = mx.reference(case)
        exp = mx.expected_hits(ref, 64)
        for grid, c in configs(geom):
            env(geom, grid, c)
            hits, total, bcnt, bsum = ctx.execute_topk_hybrid(
                [hseg], list(hm.TERMS), [1.0] * len(hm.TERMS), 64, lo, hi,
                nb)
            label = f"{case} geom={geom} grid={grid} C={c}"
            assert total == ref.total, label
            np.testing.assert_array_equal(hits["doc"], exp["doc"], label)
            np.testing.assert_array_equal(bits(hits["score"]),
                                          bits(exp["score"]), label)
            np.testing.assert_array_equal(bcnt, ref.counts, label)
            np.testing.assert_array_equal(bsum, ref.sums, label)


@pytest.mark.parametrize("geom", GEOMS, ids=("4096x256", "default"))
def test_wand_many_windows(ctx, env, geom):
    """WAND on the round-stage WAND corpus with the grid clamped, so that a
    workgroup runs dozens of windows (its bound scan reads the descriptors
    staged in the tail before): pruning still fires, results are exact"""
    w = rs.wand_matrix()
    wseg = ctx.load_segment(w.blob)
    terms, boosts = [0, 1, 2], list(rs.WAND_BOOSTS)
    rd, rsc, rtotal = w.ref_topk(terms, boosts, rs.WAND_K, "bm25")
    nw = wt.NW if geom else 16
    for grid in ((64, 256) if geom else (16, 64)):
        for c in (None, nw):
            env(geom, grid, c)
            base, total = ctx.execute_topk([wseg], terms, boosts, rs.WAND_K)
            hits, visited = ctx.execute_topk([wseg], terms, boosts,
                                             rs.WAND_K, wand=True)
            assert last_grid(ctx) == grid
            print(f"wand geom={geom} grid={grid} C={c}: "
                  f"visited {visited} of {total}")
            assert total == rtotal
            assert visited < total, (geom, grid, c, visited, total)
            for got in (base, hits):
                np.testing.assert_array_equal(got["doc"], rd)
                np.testing.assert_array_equal(bits(got["score"]), bits(rsc))


@pytest.mark.parametrize("geom", GEOMS, ids=("4096x256", "default"))
def test_batch_equals_single(ctx, seg, m, env, geom):
    """the batch entry with nq = 3 (threshold state reset between queries)
    against the per-step entry and the reference"""
    terms = m.groups["main"]
    boosts = rs.boosts_for(terms)
    rd, rsc, rtotal = m.ref_topk(terms, boosts, 50, "bm25")
    for grid, c in configs(geom):
        env(geom, grid, c)
        single, total = ctx.execute_topk([seg], terms, boosts, 50)
        batch, btotals = ctx.execute_topk_batch([seg], terms, boosts, 50, 3,
                                                all_hits=True)
        np.testing.assert_array_equal(single["doc"], rd)
        np.testing.assert_array_equal(bits(single["score"]), bits(rsc))
        for q in range(3):
            np.testing.assert_array_equal(batch[q]["doc"], rd)
            np.testing.assert_array_equal(bits(batch[q]["score"]), bits(rsc))
        assert set(np.atleast_1d(btotals).tolist()) == {total} == {rtotal}


@pytest.mark.parametrize("geom", GEOMS, ids=("4096x256", "default"))
def test_knob_contract(ctx, seg, m, env, monkeypatch, geom):
    """SDB_SWEEP_GRID clamps the launch grid downward at both launch sites;
    0, garbage and values above the default change nothing"""
    terms = m.groups["main"]
    boosts = rs.boosts_for(terms)

    def grids():
        ctx.execute_topk([seg], terms, boosts, 10)
        g1 = last_grid(ctx)
        ctx.execute_topk_batch([seg], terms, boosts, 10, 2)
        return g1, last_grid(ctx)

    env(geom, None)
    nwin = -(-wt.DOC_COUNT // (wt.WIN if geom else 24576))
    assert grids() == (nwin, nwin)
    for bad in ("0", "abc", "3x", "", "-2", "100000", "4294967297"):
        monkeypatch.setenv("SDB_SWEEP_GRID", bad)
        assert grids() == (nwin, nwin), bad
        check(ctx, seg, m, terms, boosts, 10, f"grid={bad!r}")
    for n in (1, 2, 3, 4):
        monkeypatch.setenv("SDB_SWEEP_GRID", str(n))
        assert grids() == (min(n, nwin),) * 2, n
