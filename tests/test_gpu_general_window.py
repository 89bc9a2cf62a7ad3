"""The general window kernel (topk_window_kernel) over many windows per
workgroup, on the general-window matrix (tests/general_window_matrix.py):
per-term cursors carried from window to window and past the staged
descriptors, the derive cadence, the stale threshold snapshot and the
first-window recount, windows without a candidate reservation, the u8 match
counts under min-match 2, 3 and AND, count, match-docs, the live mask, hybrid
buckets, the batch entry's launch site and WAND. SDB_WINDOW_GRID runs at 1,
2, 3, 4, 8 and unset: workgroups of 10, 5 + 5, 4 + 4 + 2, 3 + 3 + 3 + 1, 2
and one window. Every call checks sdb_gpu_last_window_grid, so a case that
ran unclamped fails, and the OR cases check that the sweep kernel's grid stat
did not move. Doc ids, score bits, totals and buckets must equal the numpy
fp32 reference exactly; tests/test_general_window_matrix.py proves that
reference equals the CPU oracle and that the corpus holds the shapes it
claims."""

import ctypes as C

import numpy as np
import pytest

import general_window_matrix as gw
import hybrid_matrix as hm
import round_stage_matrix as rs
import serenedb_amd as sa

pytestmark = pytest.mark.gpu

ENV = ("SDB_TOPK_PATH", "SDB_SWEEP_GEOM", "SDB_SWEEP_GRID",
       "SDB_WINDOW_GRID")
GRID_IDS = [f"grid{g}" if g else "unset" for g in gw.GRIDS]
SENTINEL = 7      # a sweep grid no unclamped launch of these corpora has


@pytest.fixture(scope="module")
def m():
    return gw.matrix()


@pytest.fixture(scope="module")
def ctx():
    c = sa.GpuContext(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def seg(ctx, m):
    s = ctx.load_segment(m.blob)
    ctx.attach_column(s, m.column)
    return s


@pytest.fixture
def env(monkeypatch):
    """env(grid, general=False): the four switches cleared, then the grid
    set (None: unset) and SDB_TOPK_PATH=general if asked for"""
    for k in ENV:
        monkeypatch.delenv(k, raising=False)

    def set_(grid, general=False):
        for k, v in (("SDB_WINDOW_GRID", grid),
                     ("SDB_TOPK_PATH", "general" if general else None)):
            if v is None:
                monkeypatch.delenv(k, raising=False)
            else:
                monkeypatch.setenv(k, str(v))
    return set_


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _stat(ctx, name):
    g = C.c_uint(0)
    assert getattr(ctx._lib, name)(ctx._ctx, C.byref(g)) == 0
    return g.value


def window_grid(ctx):
    return _stat(ctx, "sdb_gpu_last_window_grid")


def sweep_grid(ctx):
    return _stat(ctx, "sdb_gpu_last_sweep_grid")


def arm_sweep_sentinel(ctx, seg, m, monkeypatch):
    """one sweep launch at grid SENTINEL: a later OR call that runs on the
    sweep kernel instead of the general one moves the stat off it"""
    monkeypatch.delenv("SDB_TOPK_PATH", raising=False)
    monkeypatch.setenv("SDB_SWEEP_GRID", str(SENTINEL))
    ctx.execute_topk([seg], m.groups["early"], [1.0, 1.0], 3)
    monkeypatch.delenv("SDB_SWEEP_GRID")
    assert sweep_grid(ctx) == SENTINEL


def expect_grid(ctx, grid, nwin=gw.NWIN, label=""):
    assert window_grid(ctx) == (nwin if grid is None else min(grid, nwin)), \
        label


def check(ctx, seg, ref, terms, boosts, k, mm, grid, label, **kw):
    hits, total = ctx.execute_topk([seg], terms, boosts, k, min_match=mm,
                                   **kw)
    expect_grid(ctx, grid, label=label)
    rd, rsc, rtotal = ref
    assert total == rtotal, label
    np.testing.assert_array_equal(hits["doc"], rd, err_msg=label)
    np.testing.assert_array_equal(bits(hits["score"]), bits(rsc),
                                  err_msg=label)


@pytest.mark.parametrize("grid", gw.GRIDS, ids=GRID_IDS)
def test_cases(ctx, seg, m, env, monkeypatch, grid):
    """every named case: OR under SDB_TOPK_PATH=general, min-match 2, 3 and
    AND by themselves"""
    arm_sweep_sentinel(ctx, seg, m, monkeypatch)
    for label, terms, boosts, mm, k in gw.cases(m):
        env(grid, general=(mm == 1))
        check(ctx, seg, m.ref_topk(terms, boosts, k, "bm25", mm), terms,
              boosts, k, mm, grid, f"{label} grid={grid}")
    assert sweep_grid(ctx) == SENTINEL


@pytest.mark.parametrize("grid", gw.GRIDS, ids=GRID_IDS)
def test_count(ctx, seg, m, env, grid):
    """the count-only branch (no derive, no candidates of its own), with
    and without the live mask"""
    env(grid)
    live = gw.live_mask(m)
    for masked in (False, True):
        ctx.attach_livemask(seg, gw.live_words(m, live) if masked else None)
        try:
            for label, terms, mm in gw.count_cases(m):
                got = ctx.execute_count([seg], terms, rs.boosts_for(terms),
                                        min_match=mm)
                lb = f"{label} grid={grid} masked={masked}"
                expect_grid(ctx, grid, label=lb)
                assert got == m.ref_count(terms, mm,
                                          live if masked else None), lb
        finally:
            ctx.attach_livemask(seg, None)


@pytest.mark.parametrize("grid", gw.GRIDS, ids=GRID_IDS)
def test_match_docs(ctx, seg, m, env, grid):
    """k = 0xFFFFFFFF: every match of every window is reserved and
    appended; docs ascending, the gathered column, the total"""
    env(grid)
    main, dense = m.groups["main"], m.groups["dense"]
    for name, terms, mm in (("main mm=2", main, 2), ("main and", main, 5),
                            ("dense and", dense, 2)):
        stream = m.ref_stream(terms, mm)
        total = len(stream)
        assert total > 1
        for cap in (total, total - 1, 1, total + 13):
            docs, col, got = ctx.execute_match_docs(
                seg, terms, rs.boosts_for(terms), cap, min_match=mm,
                with_col=True)
            lb = f"{name} cap={cap} grid={grid}"
            expect_grid(ctx, grid, label=lb)
            assert got == total, lb
            np.testing.assert_array_equal(docs, stream[:cap], err_msg=lb)
            np.testing.assert_array_equal(col, m.column[stream[:cap]],
                                          err_msg=lb)


@pytest.mark.parametrize("grid", gw.GRIDS, ids=GRID_IDS)
def test_live_mask(ctx, seg, m, env, monkeypatch, grid):
    """the dead spikes must stay out of the histogram: k = 5 with 8 dead
    and 2 live top scorers"""
    live = gw.live_mask(m)
    arm_sweep_sentinel(ctx, seg, m, monkeypatch)
    ctx.attach_livemask(seg, gw.live_words(m, live))
    try:
        for label, terms, boosts, mm, _ in gw.live_cases(m):
            env(grid, general=(mm == 1))
            for k in (gw.LIVE_K, m.doc_count):
                check(ctx, seg,
                      m.ref_topk_live(terms, boosts, k, "bm25", mm, live),
                      terms, boosts, k, mm, grid,
                      f"live {label} k={k} grid={grid}")
    finally:
        ctx.attach_livemask(seg, None)
    for label, terms, boosts, mm, _ in gw.live_cases(m):
        env(grid, general=(mm == 1))
        check(ctx, seg, m.ref_topk(terms, boosts, gw.LIVE_K, "bm25", mm),
              terms, boosts, gw.LIVE_K, mm, grid, f"detached {label}")
    assert sweep_grid(ctx) == SENTINEL


def test_threshold_locks(ctx, seg, m, env, capsys):
    """`early` AND `bg`, k = 3, one workgroup: every spike is a candidate,
    and once window 0 has locked the threshold the quiet windows append
    nothing. (How many of the first windows' matches are appended depends
    on when the window's own histogram merge lands: printed, not pinned.)"""
    terms = m.groups["early"]
    boosts = rs.boosts_for(terms)
    env(1)
    check(ctx, seg, m.ref_topk(terms, boosts, 3, "bm25", 2), terms, boosts,
          3, 2, 1, "early mm=2 k=3 grid=1")
    ncand = C.c_uint(0)
    ctx._lib.sdb_gpu_last_stats(ctx._ctx, None, C.byref(ncand), None, None,
                                None)
    n = m.ref_count(terms, 2)
    with capsys.disabled():
        print(f"\ngeneral kernel, early mm=2 k=3 grid=1: {ncand.value} "
              f"candidates of {n} matches, {len(m.spikes)} spikes")
    assert len(m.spikes) <= ncand.value < n


HYBRID_PATHS = (("general_mm1", True, 1), ("general_mm2", False, 2),
                ("general_mm3", False, 3))


@pytest.fixture(scope="module")
def hseg(ctx):
    mx = hm.matrix()
    s = ctx.load_segment(mx.seg.blob)
    for slot, col in mx.chain_cols.items():
        ctx.attach_column(s, col, slot=slot)
    return s


def check_hybrid(got, ref, exp, label):
    hits, total, bcnt, bsum = got
    assert total == ref.total, label
    np.testing.assert_array_equal(hits["doc"], exp["doc"], err_msg=label)
    np.testing.assert_array_equal(bits(hits["score"]), bits(exp["score"]),
                                  err_msg=label)
    np.testing.assert_array_equal(bcnt, ref.counts, err_msg=label)
    np.testing.assert_array_equal(bsum, ref.sums, err_msg=label)


@pytest.mark.parametrize("grid", (1, 2, None), ids=("grid1", "grid2",
                                                    "unset"))
def test_hybrid_buckets(ctx, hseg, env, grid):
    """the per-window bucket flush over the three windows of
    hybrid_matrix's corpus in one workgroup, in 2 + 1 and one each"""
    mx = hm.matrix()
    terms, ones = list(hm.TERMS), [1.0] * len(hm.TERMS)
    for case in ("c01_ordinary", hm.FULL_SPAN[0]):
        lo, hi, nb = hm.CASES[case]
        ctx.attach_column(hseg, mx.bucket_col(case)[0])
        for path, general, mm in HYBRID_PATHS:
            env(grid, general=general)
            ref = mx.reference(case, mm=mm)
            got = ctx.execute_topk_hybrid([hseg], terms, ones, 64, lo, hi,
                                          nb, min_match=mm)
            lb = f"{case} {path} grid={grid}"
            expect_grid(ctx, grid, nwin=3, label=lb)
            check_hybrid(got, ref, mx.expected_hits(ref, 64, mm=mm), lb)
    # one chain: four predicates, at min-match 2
    case = "c01_ordinary"
    ctx.attach_column(hseg, mx.bucket_col(case)[0])
    env(grid)
    ref = mx.reference(case, "max4", mm=2)
    got = ctx.execute_topk_hybrid_chain(
        [hseg], terms, ones, 64, list(mx.chain_preds(case, "max4")),
        hm.CASES[case][2], min_match=2)
    expect_grid(ctx, grid, nwin=3, label="chain")
    check_hybrid(got, ref, mx.expected_hits(ref, 64, mm=2),
                 f"chain max4 grid={grid}")


@pytest.mark.parametrize("grid", gw.GRIDS, ids=GRID_IDS)
def test_batch_equals_single(ctx, seg, hseg, m, env, grid):
    """the batch entry's launch site with nq = 3 (threshold and bucket
    state of both query parities) against the per-step entry and the
    reference, plain and hybrid, at min-match 2"""
    env(grid)
    terms = m.groups["main"]
    boosts = rs.boosts_for(terms)
    ref = m.ref_topk(terms, boosts, 50, "bm25", 2)
    check(ctx, seg, ref, terms, boosts, 50, 2, grid, f"single grid={grid}")
    env(None)       # moves the stat off this grid before the batch
    ctx.execute_count([seg], terms, boosts, min_match=2)
    expect_grid(ctx, None)
    env(grid)
    batch, totals = ctx.execute_topk_batch([seg], terms, boosts, 50, 3,
                                           min_match=2, all_hits=True)
    expect_grid(ctx, grid, label="batch")
    for q in range(3):
        np.testing.assert_array_equal(batch[q]["doc"], ref[0])
        np.testing.assert_array_equal(bits(batch[q]["score"]), bits(ref[1]))
    assert list(totals) == [ref[2]] * 3

    mx = hm.matrix()
    case = "c01_ordinary"
    lo, hi, nb = hm.CASES[case]
    ctx.attach_column(hseg, mx.bucket_col(case)[0])
    href = mx.reference(case, mm=2)
    exp = mx.expected_hits(href, 64, mm=2)
    hterms, ones = list(hm.TERMS), [1.0] * len(hm.TERMS)
    single = ctx.execute_topk_hybrid([hseg], hterms, ones, 64, lo, hi, nb,
                                     min_match=2)
    expect_grid(ctx, grid, nwin=3, label="hybrid single")
    check_hybrid(single, href, exp, f"hybrid single grid={grid}")
    hits, totals, bcnt, bsum = ctx.execute_topk_hybrid_batch(
        [hseg], hterms, ones, 64, lo, hi, nb, 3, min_match=2, all_hits=True)
    expect_grid(ctx, grid, nwin=3, label="hybrid batch")
    for q in range(3):
        check_hybrid((hits[q], totals[q], bcnt[q], bsum[q]), href, exp,
                     f"hybrid batch q={q} grid={grid}")


def test_wand_general_many_windows(ctx, env, capsys):
    """WAND on the general path over the round-stage WAND corpus (489
    windows) with the grid clamped, so that a workgroup walks dozens of
    windows: pruning fires, results are exact"""
    w = rs.wand_matrix()
    wseg = ctx.load_segment(w.blob)
    terms, boosts = [0, 1, 2], list(rs.WAND_BOOSTS)
    nwin = -(-rs.WAND_DOCS // gw.WIN)
    assert nwin == 489
    rd, rsc, rtotal = w.ref_topk(terms, boosts, rs.WAND_K, "bm25")
    for grid in (16, 64):
        env(grid, general=True)
        base, total = ctx.execute_topk([wseg], terms, boosts, rs.WAND_K)
        expect_grid(ctx, grid, nwin=nwin)
        hits, visited = ctx.execute_topk([wseg], terms, boosts, rs.WAND_K,
                                         wand=True)
        expect_grid(ctx, grid, nwin=nwin)
        with capsys.disabled():
            print(f"\ngeneral kernel, wand grid={grid}: visited {visited} "
                  f"of {total}")
        assert total == rtotal
        assert visited < total, (grid, visited, total)
        for got in (base, hits):
            np.testing.assert_array_equal(got["doc"], rd)
            np.testing.assert_array_equal(bits(got["score"]), bits(rsc))


def test_knob_contract(ctx, seg, m, env, monkeypatch):
    """SDB_WINDOW_GRID clamps the launch grid downward at both launch
    sites; 0, garbage, negative values and values at or above the default
    change nothing; it and SDB_SWEEP_GRID do not touch each other's kernel;
    the stat is 0 before the first launch of the general kernel"""
    terms = m.groups["main"]
    boosts = rs.boosts_for(terms)
    ref2 = m.ref_topk(terms, boosts, 10, "bm25", 2)
    ref1 = m.ref_topk(terms, boosts, 10, "bm25", 1)

    def same(hits, total, ref, label):
        assert total == ref[2], label
        np.testing.assert_array_equal(hits["doc"], ref[0], err_msg=label)
        np.testing.assert_array_equal(bits(hits["score"]), bits(ref[1]),
                                      err_msg=label)

    def grids(label):
        hits, total = ctx.execute_topk([seg], terms, boosts, 10, min_match=2)
        g1 = window_grid(ctx)
        same(hits, total, ref2, label)
        batch, totals = ctx.execute_topk_batch([seg], terms, boosts, 10, 2,
                                               min_match=2, all_hits=True)
        for q in range(2):
            same(batch[q], totals[q], ref2, label)
        return g1, window_grid(ctx)

    def sweep(label):
        hits, total = ctx.execute_topk([seg], terms, boosts, 10)
        same(hits, total, ref1, label)
        return sweep_grid(ctx)

    fresh = sa.GpuContext(0)
    try:
        assert window_grid(fresh) == 0
        fseg = fresh.load_segment(m.blob)
        fresh.execute_topk([fseg], terms, boosts, 10)     # the sweep kernel
        assert window_grid(fresh) == 0 and sweep_grid(fresh) == gw.NWIN
        fresh.execute_topk([fseg], terms, boosts, 10, min_match=2)
        assert window_grid(fresh) == gw.NWIN
    finally:
        fresh.close()

    env(None)
    nwin = gw.NWIN
    assert grids("unset") == (nwin, nwin)
    for bad in ("0", "abc", "3x", "", "-2", "100000", "4294967297"):
        monkeypatch.setenv("SDB_WINDOW_GRID", bad)
        assert grids(repr(bad)) == (nwin, nwin), bad
    for n in (1, 2, 3, 4):
        monkeypatch.setenv("SDB_WINDOW_GRID", str(n))
        assert grids(f"grid {n}") == (n, n), n
        assert sweep(f"sweep under window grid {n}") == nwin
    monkeypatch.delenv("SDB_WINDOW_GRID")
    for n in (1, 3):
        monkeypatch.setenv("SDB_SWEEP_GRID", str(n))
        assert sweep(f"sweep grid {n}") == n
        assert grids(f"under sweep grid {n}") == (nwin, nwin), n
