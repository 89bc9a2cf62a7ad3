"""The sweep kernel's round stage on the round-stage matrix
(tests/round_stage_matrix.py): windows whose item count sits around the
stage capacity C, round boundaries inside a term, window-edge blocks, terms
without items, non-fused blocks beside fused pairs, a dense term, a 32-term
plan, WAND, the live mask, hybrid buckets and the batch entry point, each
under SDB_SWEEP_ROUND_ITEMS at the smallest C, mid values and unset, at the
smallest compiled geometry and at the default one; WAND also on a corpus of
its own where pruning fires. Doc ids, score bits and
totals must equal the numpy fp32 term-major reference exactly;
tests/test_round_stage_matrix.py proves that reference equals the CPU oracle
and that the corpus holds the shapes it claims."""

import numpy as np
import pytest

import hybrid_matrix as hm
import round_stage_matrix as rs
import serenedb_amd as sa

pytestmark = pytest.mark.gpu

SCORERS = ("bm25", "tfidf_norm")
ENV = ("SDB_TOPK_PATH", "SDB_SWEEP_GEOM", "SDB_SWEEP_ROUND_ITEMS")
GEOMS = (rs.GEOM, None)          # None: the default geometry


@pytest.fixture(scope="module")
def m():
    return rs.matrix()


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

    def set_(geom, c):
        for k, v in (("SDB_SWEEP_GEOM", geom), ("SDB_SWEEP_ROUND_ITEMS", c)):
            if v is None:
                monkeypatch.delenv(k, raising=False)
            else:
                monkeypatch.setenv(k, str(v))
    return set_


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def n_matches(m, terms):
    return len(np.unique(np.concatenate([m.postings[t][0] for t in terms])))


def check(ctx, seg, m, terms, boosts, k, scorer, label, **kw):
    hits, total = ctx.execute_topk([seg], terms, boosts, k, scorer=scorer,
                                   **kw)
    rd, rsc, rtotal = m.ref_topk(terms, boosts, k, scorer)
    if kw.get("wand"):           # under WAND the total counts visited docs
        assert total <= rtotal, label
    else:
        assert total == rtotal, label
    np.testing.assert_array_equal(hits["doc"], rd, err_msg=label)
    np.testing.assert_array_equal(bits(hits["score"]), bits(rsc),
                                  err_msg=label)


def capacities(geom):
    """the override at one slot per wave, every value from there up to the
    host's own choice and past it (where it clamps nothing), and unset"""
    nw, top = (rs.NW, 12) if geom else (16, 44)
    return list(range(nw, top + 1)) + [None]


@pytest.mark.parametrize("geom", GEOMS, ids=("4096x256", "default"))
@pytest.mark.parametrize("scorer", SCORERS)
@pytest.mark.parametrize("group", ("steer", "edges", "first_empty"))
def test_capacities(ctx, seg, m, env, group, scorer, geom):
    """item counts C - 1, C, C + 1 and multiples of C (at C = NW = 4 the
    windows of these plans hold 3, 4, 5, 7, 8, 9 and 10 items); a round
    boundary inside term `a`; docs matched by every term under unequal
    boosts; at the default geometry, one window and C = 42, cross-term
    pairs (tests/test_round_stage_matrix.py proves each)"""
    terms = m.groups[group]
    boosts = rs.boosts_for(terms)
    for c in capacities(geom):
        env(geom, c)
        for k in (n_matches(m, terms), 10):
            check(ctx, seg, m, terms, boosts, k, scorer,
                  f"{group} geom={geom} C={c} k={k} {scorer}")


@pytest.mark.parametrize("geom", GEOMS, ids=("4096x256", "default"))
@pytest.mark.parametrize("group", ("first_empty", "edges", "mixed",
                                   "dense2", "all32"))
def test_groups(ctx, seg, m, env, group, geom):
    """window-edge blocks, terms without items, tails beside fused pairs,
    the dense term past the descriptor cache, the 32-term plan: override at
    NW, at a mid value and unset"""
    terms = m.groups[group]
    boosts = rs.boosts_for(terms)
    nw = rs.NW if geom else 16
    for c in (nw, nw + 3, None):
        env(geom, c)
        for scorer in SCORERS:
            for k in (n_matches(m, terms), 10):
                check(ctx, seg, m, terms, boosts, k, scorer,
                      f"{group} geom={geom} C={c} k={k} {scorer}")


@pytest.mark.parametrize("geom", GEOMS, ids=("4096x256", "default"))
def test_single_terms(ctx, seg, m, env, geom):
    """every term alone, all of its docs: each posting lands in the right
    slot entry and none twice (blocks on a window edge are decoded by both
    neighbours)"""
    for c in (rs.NW if geom else 16, None):
        env(geom, c)
        for t, (docs, _) in enumerate(m.postings):
            check(ctx, seg, m, [t], [1.0], len(docs) + 1, "bm25",
                  f"single {m.names[t]} geom={geom} C={c}")


@pytest.fixture(scope="module")
def wand_seg(ctx):
    return ctx.load_segment(rs.wand_matrix().blob)


@pytest.mark.parametrize("geom", GEOMS, ids=("4096x256", "default"))
def test_wand_prunes_inside_rounds(ctx, wand_seg, env, geom):
    """WAND with k = 10 on the corpus where every workgroup walks several
    windows, so that from its second window on it holds a threshold and
    prunes: pruned items leave all-absent slots inside a round, a pruned
    second item breaks up a pair, next to decoded items and cross-term
    pairs, in windows of several rounds (C = NW and a mid value) and of
    one or two (unset). visited < total proves the pruning fired."""
    w = rs.wand_matrix()
    terms, boosts = [0, 1, 2], list(rs.WAND_BOOSTS)
    rd, rsc, rtotal = w.ref_topk(terms, boosts, rs.WAND_K, "bm25")
    nw = rs.NW if geom else 16
    for c in (nw, nw + 3, None):
        env(geom, c)
        base, total = ctx.execute_topk([wand_seg], terms, boosts, rs.WAND_K)
        hits, visited = ctx.execute_topk([wand_seg], terms, boosts,
                                         rs.WAND_K, wand=True)
        print(f"wand geom={geom} C={c}: visited {visited} of {total}")
        assert total == rtotal
        assert visited < total, (geom, c, visited, total)
        for got in (base, hits):
            np.testing.assert_array_equal(got["doc"], rd)
            np.testing.assert_array_equal(bits(got["score"]), bits(rsc))


@pytest.mark.parametrize("geom", GEOMS, ids=("4096x256", "default"))
def test_wand(ctx, seg, m, env, geom):
    """WAND with k = 10 on the small corpus (one window per workgroup:
    nothing is pruned, the WAND bookkeeping runs beside the rounds)"""
    nw = rs.NW if geom else 16
    for group in ("steer", "mixed", "all32"):
        terms = m.groups[group]
        boosts = rs.boosts_for(terms)
        for c in (nw, nw + 3, None):
            env(geom, c)
            for scorer in SCORERS:
                check(ctx, seg, m, terms, boosts, 10, scorer,
                      f"wand {group} geom={geom} C={c} {scorer}", wand=True)


@pytest.mark.parametrize("geom", GEOMS, ids=("4096x256", "default"))
def test_live_mask(ctx, seg, m, env, geom):
    nw = rs.NW if geom else 16
    terms = m.groups["steer"]
    boosts = list(rs.STEER_BOOSTS)
    live = rs.live_mask()
    ctx.attach_livemask(seg, rs.live_words(live))
    try:
        for c in (nw, nw + 1, None):
            env(geom, c)
            for k in (rs.DOC_COUNT, 10):
                hits, total = ctx.execute_topk([seg], terms, boosts, k)
                rd, rsc, rtotal = m.ref_topk_live(terms, boosts, k, "bm25",
                                                  live)
                assert total == rtotal
                np.testing.assert_array_equal(hits["doc"], rd)
                np.testing.assert_array_equal(bits(hits["score"]), bits(rsc))
    finally:
        ctx.attach_livemask(seg, None)
    check(ctx, seg, m, terms, boosts, 10, "bm25", "mask detached")


@pytest.mark.parametrize("geom", GEOMS, ids=("4096x256", "default"))
def test_batch_equals_single(ctx, seg, m, env, geom):
    nw = rs.NW if geom else 16
    for group in ("steer", "mixed", "all32"):
        terms = m.groups[group]
        boosts = rs.boosts_for(terms)
        k = 50
        for c in (nw, nw + 3, None):
            env(geom, c)
            single, total = ctx.execute_topk([seg], terms, boosts, k)
            batch, btotals = ctx.execute_topk_batch([seg], terms, boosts, k,
                                                    3, all_hits=True)
            rd, rsc, rtotal = m.ref_topk(terms, boosts, k, "bm25")
            np.testing.assert_array_equal(single["doc"], rd)
            np.testing.assert_array_equal(bits(single["score"]), bits(rsc))
            for q in range(3):
                np.testing.assert_array_equal(batch[q]["doc"], single["doc"])
                np.testing.assert_array_equal(bits(batch[q]["score"]),
                                              bits(single["score"]))
            assert set(np.atleast_1d(btotals).tolist()) == {total}
            assert total == rtotal


@pytest.mark.parametrize("geom", GEOMS, ids=("4096x256", "default"))
def test_hybrid_buckets(ctx, env, geom):
    """the hybrid branch of the sweep kernel (the bucket accumulators sit in
    front of the posting stage in LDS) against hybrid_matrix's reference"""
    mx = hm.matrix()
    hseg = ctx.load_segment(mx.seg.blob)
    nw = rs.NW if geom else 16
    for case in ("c01_ordinary", hm.FULL_SPAN[0]):
        lo, hi, nb = hm.CASES[case]
        ctx.attach_column(hseg, mx.bucket_col(case)[0])
        ref = mx.reference(case)
        exp = mx.expected_hits(ref, 64)
        for c in (nw, nw + 3, None):
            env(geom, c)
            hits, total, bcnt, bsum = ctx.execute_topk_hybrid(
                [hseg], list(hm.TERMS), [1.0] * len(hm.TERMS), 64, lo, hi,
                nb)
            assert total == ref.total
            np.testing.assert_array_equal(hits["doc"], exp["doc"])
            np.testing.assert_array_equal(bits(hits["score"]),
                                          bits(exp["score"]))
            np.testing.assert_array_equal(bcnt, ref.counts)
            np.testing.assert_array_equal(bsum, ref.sums)
