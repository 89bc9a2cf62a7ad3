"""CPU side of the round-stage matrix (tests/round_stage_matrix.py): the numpy
fp32 term-major reference equals the CPU oracle on every plan the GPU test
runs, and the corpus holds the shapes its docstring claims, read from the
blob's descriptors."""

import numpy as np
import pytest

import round_stage_matrix as rs
from oracle import pyoracle as po

SCORERS = ("bm25", "tfidf_norm")


@pytest.fixture(scope="module")
def m():
    return rs.matrix()


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@pytest.mark.parametrize("scorer", SCORERS)
@pytest.mark.parametrize("group", ("steer", "first_empty", "edges", "mixed",
                                   "dense2", "all32"))
def test_reference_equals_oracle(m, group, scorer):
    terms = m.groups[group]
    boosts = rs.boosts_for(terms)
    n = len(np.unique(np.concatenate([m.postings[t][0] for t in terms])))
    for k in (n, 10):
        rd, rsc, rtotal = m.ref_topk(terms, boosts, k, scorer)
        od, osc, ototal = m.oracle_topk(terms, boosts, k, scorer)
        assert rtotal == ototal == n
        np.testing.assert_array_equal(rd, od)
        np.testing.assert_array_equal(bits(rsc), bits(osc))


def test_live_reference_equals_oracle(m):
    terms = m.groups["steer"]
    boosts = rs.boosts_for(terms)
    live = rs.live_mask()
    for k in (rs.DOC_COUNT, 10):
        rd, rsc, rtotal = m.ref_topk_live(terms, boosts, k, "bm25", live)
        hits, ototal = po.execute_topk([m.blob], terms, boosts, k,
                                       live_mask=rs.live_words(live))
        assert rtotal == ototal
        np.testing.assert_array_equal(rd, hits["doc"])
        np.testing.assert_array_equal(bits(rsc), bits(hits["score"]))
    plain = m.ref_topk(terms, boosts, 10, "bm25")[2]
    assert rtotal < plain


def test_add_order_shows_in_the_bits(m):
    """on docs matched by every steer term, summing the terms in another
    order gives other score bits: a merge out of term order cannot pass"""
    terms = m.groups["steer"]
    boosts = rs.boosts_for(terms)
    for scorer in SCORERS:
        u, s, cnt, _ = m.ref_scores(terms, boosts, scorer)
        u2, s2, _, _ = m.ref_scores(terms[::-1], boosts[::-1], scorer)
        assert np.array_equal(u, u2)
        every = cnt == len(terms)
        assert every.sum() >= 30
        assert (bits(s[every]) != bits(s2[every])).sum() >= 5


def test_item_counts_around_the_capacity(m):
    """at C = NW, the capacity every launch can be clamped to, the windows
    of the plans that test_capacities runs hold C - 1, C, C + 1, 2C - 1,
    2C, 2C + 1 and more items, and `mixed` ten times C; in two windows a
    round of NW ends inside term `a`"""
    C = rs.NW
    counts = set()
    for g in ("steer", "edges", "first_empty"):
        for items in m.window_items(m.groups[g]):
            terms = [p for p, _ in items]
            assert terms == sorted(terms)
            counts.add(len(items))
    assert counts >= {C - 1, C, C + 1, 2 * C - 1, 2 * C, 2 * C + 1, 10}
    assert 10 * C in {len(it) for it in m.window_items(m.groups["mixed"])}
    wins = m.window_items(m.groups["steer"])
    assert sum(len(it) > C and it[C - 1][0] == it[C][0] == 0
               for it in wins) >= 2
    # the host's own choice for these plans, mirrored: the values that
    # test_capacities sweeps reach it at both geometries
    assert rs.default_c(4) == 5 and rs.default_c(4, 24576, 1024) == 42


def test_cross_term_pairs(m):
    """rs.deal replays how the kernel deals a window's items over the waves
    and pairs them. At the default geometry the corpus is one window and a
    4-term plan gets 42 slots (the figure of the headline shape): the steer
    plan then forms fused pairs whose two blocks belong to different terms,
    and so it does at C = NW + 1 and above at 4096x256; at C = NW no wave
    holds two items, so no pair forms at all."""
    def cross(items, c, nw):
        return [(i, j) for i, j in rs.deal(items, c, nw)
                if items[i][0] != items[j][0]]
    (one,) = m.window_items(m.groups["steer"], 24576)
    assert len(one) <= 42
    assert len(cross(one, 42, 16)) >= 1
    assert len(cross(one, 19, 16)) >= 1
    wins = m.window_items(m.groups["steer"])
    for c in (rs.NW + 1, rs.NW + 3):
        assert any(cross(it, c, rs.NW) for it in wins), c
    assert not any(rs.deal(it, rs.NW) for it in wins)


def test_wand_corpus(m):
    """the WAND corpus: reference equals oracle; more windows than any
    launch has workgroups (1024 at 4096x256, 256 at the default geometry),
    so every workgroup walks several; windows of more than NW items, the
    terms interleaved so that pairs span terms; the first term's spikes
    above what three plain blocks can reach"""
    w = rs.wand_matrix()
    terms, boosts = [0, 1, 2], list(rs.WAND_BOOSTS)
    rd, rsc, rtotal = w.ref_topk(terms, boosts, rs.WAND_K, "bm25")
    od, osc, ototal = w.oracle_topk(terms, boosts, rs.WAND_K, "bm25")
    assert rtotal == ototal
    np.testing.assert_array_equal(rd, od)
    np.testing.assert_array_equal(bits(rsc), bits(osc))
    assert -(-rs.WAND_DOCS // rs.WIN) > 2 * 1024
    assert -(-rs.WAND_DOCS // 24576) > 256
    for items in w.window_items(terms, last=4):
        assert len(items) > rs.NW + 1
        assert any(items[i][0] != items[j][0]
                   for i, j in rs.deal(items, rs.NW + 3))
    for items in w.window_items(terms, 24576, last=2):
        assert len(items) > 16 + 3
        assert sum(r["fused"] for _, r in items) > len(items) // 2
    # every hit is a spike of `a`; a doc with freq 1 or 2 in `a` scores lower
    # than the k-th hit by more than the other two terms can add
    docs, freqs = w.postings[0]
    assert np.all(freqs[np.searchsorted(docs, rd)] == 200)
    u, s, _, _ = w.ref_scores([0], [1.0], "bm25")
    plain_max = s[freqs <= 2].max()
    u2, s2, _, _ = w.ref_scores([1, 2], boosts[1:], "bm25")
    assert plain_max + 2 * s2.max() < rsc[-1]


def test_shared_docs(m):
    # the shared docs: every block of `a` holds a doc that all terms match
    recs, _, _ = m.parse()
    u, _, cnt, _ = m.ref_scores(m.groups["steer"], rs.STEER_BOOSTS, "bm25")
    every = u[cnt == 4]
    for r in recs[m.idx["a"]]:
        assert np.any((every > r["prev"]) & (every <= r["last"]))


def test_edge_shapes(m):
    recs, _, _ = m.parse()
    W = rs.WIN
    firsts = {n: [int(m.postings[m.idx[n]][0][rs.BLOCK * i])
                  for i in range(len(recs[m.idx[n]]))] for n in m.names}
    e = recs[m.idx["edge"]]
    assert [r["last"] for r in e[:3]] == [W, e[1]["last"], 2 * W]
    assert firsts["edge"][1] == W + 1 and firsts["edge"][3] == 2 * W + 1
    assert e[1]["prev"] == W           # starts on lo: prev_doc == lo - 1
    # straddling: a block over window 0's hi, and one over both edges of
    # window 2
    s = recs[m.idx["sparse"]]
    assert s[0]["prev"] < W < s[0]["last"]
    assert s[-1]["prev"] < 2 * W + 1 and s[-1]["last"] > 3 * W
    # gap: no posting in the middle window, and no block across it
    g = m.postings[m.idx["gap"]][0]
    assert not np.any((g > W) & (g <= 2 * W))
    assert recs[m.idx["gap"]][0]["last"] <= W
    assert firsts["gap"][1] > 2 * W
    # the first term of first_empty has no item after window 0
    wins = m.window_items(m.groups["first_empty"])
    assert [sum(1 for p, _ in it if p == 0) for it in wins] == [2, 0, 0, 0]
    # tails
    assert [r["len"] for r in recs[m.idx["one_tail"]]] == [128, 1]
    assert W < firsts["one_tail"][1] <= 2 * W
    assert [r["len"] for r in recs[m.idx["w0only"]]] == [128, 5]
    assert [r["len"] for r in recs[m.idx["gap"]]] == [128, 128, 2]


def test_mixed_round_holds_fused_and_non_fused(m):
    """the mixed plan: some round holds fused items next to the 1-doc tail,
    at C = NW in window 1 of 4096 docs and at the default geometry's own C
    in its single window; full non-fused blocks (the dense term) as well"""
    def rounds(items, c):
        return [items[r0:r0 + c] for r0 in range(0, len(items), c)]
    for items, c in ((m.window_items(m.groups["mixed"])[1], rs.NW),
                     (m.window_items(m.groups["mixed"], 24576)[0],
                      rs.default_c(5, 24576, 1024))):
        assert any(any(r["fused"] for _, r in rd) and
                   any(not r["fused"] and r["len"] == 1 for _, r in rd)
                   for rd in rounds(items, c))
        assert any(not r["fused"] and r["len"] == 128 for _, r in items)


def test_dense_exceeds_the_descriptor_cache(m):
    for win in (rs.WIN, 24576):
        items = m.window_items([m.idx["dense"]], win)
        assert max(len(it) for it in items) > rs.DCACHE
    # and a window of the 32-term plan takes more than one round at any C the
    # 160 KB of LDS allow next to a 4096-doc window
    wins = m.window_items(m.groups["all32"])
    assert min(len(it) for it in wins[:3]) > rs.default_c(32)
