"""Hybrid top-k (BM25 top-k AND pushed column predicates, per-bucket COUNT /
SUM) on every GPU path, against the hybrid filter matrix
(tests/hybrid_matrix.py; tests/test_hybrid_matrix.py proves its reference on
the CPU). One pytest case per (span case, path), so a failure names both.
Every comparison is exact: totals, hit docs, hit segments, score bit
patterns, counts and sums as int64.

Paths:
  sweep             min_match 1, the default: the sweep kernel's hybrid branch
  general_mm1       min_match 1 with SDB_TOPK_PATH=general: the window kernel
  general_mm2       min_match 2 (the window kernel)
  general_mm3       min_match 3 over the three terms: the AND, one doc, the
                    segment's last
  general_and_ab    min_match 2 over terms A and B alone: an AND with
                    thousands of docs
  sweep_live        sweep with the live mask attached, then detached again
  general_mm2_live  the same for the window kernel
  batch             execute_topk_hybrid_batch, nq = 3: both parities of the
                    double-buffered bucket planes, one of them reused
  two_seg           the main segment and the 129-doc one

The predicate chains of the matrix (four predicates, a repeated slot, the
INT64 extremes as literals) run on sweep and general_mm2, each with and
without the live mask.

Under the wrapping 64-bit bucket expression the kernels used to share with
the oracle (hm.old_bucket), cases c06 to c10 fail on every path except
general_mm3, whose single doc happens to land right; the c11 cases divide by
zero there.
"""

import numpy as np
import pytest

import hybrid_matrix as hm
import serenedb_amd as sa

pytestmark = pytest.mark.gpu

K = 64
ENV_SWITCHES = ("SDB_TOPK_PATH", "SDB_SWEEP_GEOM")
PATHS = {   # name: (environment, terms, min_match, live mask)
    "sweep": ({}, hm.TERMS, 1, False),
    "general_mm1": ({"SDB_TOPK_PATH": "general"}, hm.TERMS, 1, False),
    "general_mm2": ({}, hm.TERMS, 2, False),
    "general_mm3": ({}, hm.TERMS, 3, False),
    "general_and_ab": ({}, (0, 1), 2, False),
    "sweep_live": ({}, hm.TERMS, 1, True),
    "general_mm2_live": ({}, hm.TERMS, 2, True),
}
CASE_IDS = list(hm.CASES)
CHAINS = ("max4", "ge_min", "lt_min", "ge_max", "lt_max", "between_empty",
          "between_all", "same_slot")


@pytest.fixture(scope="module")
def mx():
    return hm.matrix()


@pytest.fixture(scope="module")
def ctx():
    c = sa.GpuContext(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def segs(ctx, mx):
    """(main segment with chain slots 1..3 attached, the 129-doc segment);
    slot 0 is attached per case"""
    s1 = ctx.load_segment(mx.seg.blob)
    s2 = ctx.load_segment(mx.seg2.blob)
    for slot, col in mx.chain_cols.items():
        ctx.attach_column(s1, col, slot=slot)
    return s1, s2


@pytest.fixture
def path(request, monkeypatch):
    for k in ENV_SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in PATHS[request.param][0].items():
        monkeypatch.setenv(k, v)
    return request.param


def cases(case_ids, paths):
    return pytest.mark.parametrize(
        "case,path", [(c, p) for c in case_ids for p in paths],
        indirect=["path"], ids=lambda v: v)


def check(got, ref, exp_hits):
    hits, total, bcnt, bsum = got
    assert total == ref.total
    np.testing.assert_array_equal(hits["doc"], exp_hits["doc"])
    np.testing.assert_array_equal(hits["segment"], exp_hits["segment"])
    np.testing.assert_array_equal(hits["score"].view(np.uint32),
                                  exp_hits["score"].view(np.uint32))
    assert bcnt.dtype == np.int64 and bsum.dtype == np.int64
    np.testing.assert_array_equal(bcnt, ref.counts)
    np.testing.assert_array_equal(bsum, ref.sums)


def run_single(ctx, mx, seg, case, terms, mm, live, k=K):
    """one execute_topk_hybrid against the reference"""
    lo, hi, nb = hm.CASES[case]
    ref = mx.reference(case, terms=terms, mm=mm, live=live)
    got = ctx.execute_topk_hybrid([seg], list(terms), [1.0] * len(terms), k,
                                  lo, hi, nb, min_match=mm)
    assert len(got[0]) == min(k, ref.total)
    check(got, ref, mx.expected_hits(ref, k, terms, mm, live))
    return ref


@cases(CASE_IDS, PATHS)
def test_single(ctx, mx, segs, case, path):
    _, terms, mm, live = PATHS[path]
    seg = segs[0]
    ctx.attach_column(seg, mx.bucket_col(case)[0])
    if not live:
        run_single(ctx, mx, seg, case, terms, mm, False)
        return
    ctx.attach_livemask(seg, mx.live_words())
    try:
        masked = run_single(ctx, mx, seg, case, terms, mm, True)
    finally:
        ctx.attach_livemask(seg, None)
    plain = run_single(ctx, mx, seg, case, terms, mm, False)
    assert plain.nmatch > masked.nmatch


@pytest.mark.parametrize("mm", (1, 2), ids=("mm1", "mm2"))
@pytest.mark.parametrize("case", CASE_IDS)
def test_batch(ctx, mx, segs, case, mm, monkeypatch):
    """nq = 3: queries 0 and 2 share a bucket plane, so a plane that is not
    cleared on reuse doubles query 2's counts"""
    for k in ENV_SWITCHES:
        monkeypatch.delenv(k, raising=False)
    lo, hi, nb = hm.CASES[case]
    seg = segs[0]
    ctx.attach_column(seg, mx.bucket_col(case)[0])
    ref = mx.reference(case, mm=mm)
    exp = mx.expected_hits(ref, K, mm=mm)
    hits, totals, bcnt, bsum = ctx.execute_topk_hybrid_batch(
        [seg], list(hm.TERMS), [1.0] * 3, K, lo, hi, nb, 3, min_match=mm,
        all_hits=True)
    assert len(hits) == 3 and bcnt.shape == bsum.shape == (3, nb)
    for q in range(3):
        check((hits[q], totals[q], bcnt[q], bsum[q]), ref, exp)


@pytest.mark.parametrize("mm", (1, 2), ids=("mm1", "mm2"))
@pytest.mark.parametrize("case", CASE_IDS)
def test_two_seg(ctx, mx, segs, case, mm, monkeypatch):
    """buckets accumulate over both segments; hits are ordered (score desc,
    segment, doc)"""
    for k in ENV_SWITCHES:
        monkeypatch.delenv(k, raising=False)
    lo, hi, nb = hm.CASES[case]
    ctx.attach_column(segs[0], mx.bucket_col(case)[0])
    ctx.attach_column(segs[1], mx.bucket_col2(case))
    ref = mx.reference(case, mm=mm, two_seg=True)
    exp = mx.expected_hits(ref, K, mm=mm, two_seg=True)
    if ref.total:
        assert {0, 1} <= {s for s, _ in ref.survivors}
    got = ctx.execute_topk_hybrid(list(segs), list(hm.TERMS), [1.0] * 3, K,
                                  lo, hi, nb, min_match=mm)
    check(got, ref, exp)
    key = [(-float(h["score"]), int(h["segment"]), int(h["doc"]))
           for h in got[0]]
    assert key == sorted(key)


@cases(hm.CHAIN_CASES, ("sweep", "general_mm2"))
def test_k_edges(ctx, mx, segs, case, path):
    _, terms, mm, _ = PATHS[path]
    seg = segs[0]
    ctx.attach_column(seg, mx.bucket_col(case)[0])
    ref = mx.reference(case, mm=mm)
    assert 1 < ref.total < ref.total + 1 < ref.nmatch
    for k in (1, ref.total, ref.total + 1, ref.nmatch):
        run_single(ctx, mx, seg, case, terms, mm, False, k=k)


def run_chain(ctx, mx, seg, case, chain, mm, live=False):
    nb = hm.CASES[case][2]
    ref = mx.reference(case, chain, mm=mm, live=live)
    got = ctx.execute_topk_hybrid_chain(
        [seg], list(hm.TERMS), [1.0] * 3, K,
        list(mx.chain_preds(case, chain)), nb, min_match=mm)
    check(got, ref, mx.expected_hits(ref, K, mm=mm, live=live))
    return got


@pytest.mark.parametrize("chain", CHAINS)
@cases(hm.CHAIN_CASES, ("sweep", "general_mm2", "sweep_live",
                        "general_mm2_live"))
def test_chain(ctx, mx, segs, case, path, chain):
    _, _, mm, live = PATHS[path]
    seg = segs[0]
    ctx.attach_column(seg, mx.bucket_col(case)[0])
    if live:
        ctx.attach_livemask(seg, mx.live_words())
        try:
            run_chain(ctx, mx, seg, case, chain, mm, True)
        finally:
            ctx.attach_livemask(seg, None)
    got = run_chain(ctx, mx, seg, case, chain, mm)
    if chain in ("ge_min", "between_all"):   # equal the single predicate
        lo, hi, nb = hm.CASES[case]
        one = ctx.execute_topk_hybrid([seg], list(hm.TERMS), [1.0] * 3, K,
                                      lo, hi, nb, min_match=mm)
        for a, b in zip(got, one):
            np.testing.assert_array_equal(a, b)
    if chain in ("lt_min", "between_empty"):
        assert got[1] == 0 and len(got[0]) == 0 and not got[2].any()


P0 = (0, hm.BETWEEN, 1000, 1999)
ALL1 = (1, hm.GE, hm.I64_MIN, 0)
REJECTIONS = {
    # name: (entry, predicates or None, nbuckets, both segments)
    "nbuckets_0": ("hybrid", None, 0, False),
    "nbuckets_129": ("hybrid", None, 129, False),
    "chain_nbuckets_0": ("chain", (P0,), 0, False),
    "chain_nbuckets_129": ("chain", (P0,), 129, False),
    "batch_nbuckets_0": ("batch", None, 0, False),
    "batch_nbuckets_129": ("batch", None, 129, False),
    "five_preds": ("chain", (P0, ALL1, ALL1, ALL1, ALL1), 64, False),
    "first_not_between": ("chain", ((0, hm.GE, 1000, 0), ALL1), 64, False),
    "first_lt": ("chain", ((0, hm.LT, 1999, 0),), 64, False),
    "eq_in_chain": ("chain", (P0, (1, hm.EQ, 5, 0)), 64, False),
    "eq_first": ("chain", ((0, hm.EQ, 1000, 1999),), 64, False),
    "isnull_in_chain": ("chain", (P0, ALL1, (2, hm.ISNULL, 0, 0)), 64,
                        False),
    "slot_4": ("chain", (P0, (4, hm.GE, hm.I64_MIN, 0)), 64, False),
    "slot_4_first": ("chain", ((4, hm.BETWEEN, 1000, 1999),), 64, False),
    "slot_missing_on_segment_2": ("chain", (P0, ALL1), 64, True),
}


@pytest.mark.parametrize("name", list(REJECTIONS))
def test_rejections(ctx, mx, segs, name, monkeypatch):
    """each is refused with SDB_ERR_INVALID and leaves the next good call
    correct"""
    for k in ENV_SWITCHES:
        monkeypatch.delenv(k, raising=False)
    entry, preds, nb, both = REJECTIONS[name]
    case = "c01_ordinary"
    lo, hi, _ = hm.CASES[case]
    ctx.attach_column(segs[0], mx.bucket_col(case)[0])
    ctx.attach_column(segs[1], mx.bucket_col2(case))
    use = list(segs) if both else [segs[0]]
    terms, boosts = list(hm.TERMS), [1.0] * 3
    with pytest.raises(RuntimeError, match="rc=-1"):
        if entry == "hybrid":
            ctx.execute_topk_hybrid(use, terms, boosts, K, lo, hi, nb)
        elif entry == "batch":
            ctx.execute_topk_hybrid_batch(use, terms, boosts, K, lo, hi, nb,
                                          3)
        else:
            ctx.execute_topk_hybrid_chain(use, terms, boosts, K, list(preds),
                                          nb)
    run_single(ctx, mx, segs[0], case, hm.TERMS, 1, False)
    run_chain(ctx, mx, segs[0], case, "max4", 2)
