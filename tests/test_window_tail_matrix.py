"""CPU side of the window-tail matrix (tests/window_tail_matrix.py): the numpy
fp32 term-major reference equals the CPU oracle bit for bit on every case
the GPU test runs, and the corpus holds the shapes its docstring claims,
read from the raw arrays and the blob's descriptors."""

import numpy as np
import pytest

import window_tail_matrix as wt
from oracle import pyoracle as po


@pytest.fixture(scope="module")
def m():
    return wt.matrix()


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def test_reference_equals_oracle(m):
    for label, terms, boosts, k in wt.cases(m):
        rd, rsc, rtotal = m.ref_topk(terms, boosts, k, "bm25")
        od, osc, ototal = m.oracle_topk(terms, boosts, k, "bm25")
        assert rtotal == ototal == wt.n_matches(m, terms), label
        np.testing.assert_array_equal(rd, od, err_msg=label)
        np.testing.assert_array_equal(bits(rsc), bits(osc), err_msg=label)


def test_live_reference_equals_oracle(m):
    terms = m.groups["main"]
    boosts = wt.rs.boosts_for(terms)
    live = wt.live_mask()
    for k in (wt.DOC_COUNT, 10):
        rd, rsc, rtotal = m.ref_topk_live(terms, boosts, k, "bm25", live)
        hits, ototal = po.execute_topk([m.blob], terms, boosts, k,
                                       live_mask=wt.live_words(live))
        assert rtotal == ototal
        np.testing.assert_array_equal(rd, hits["doc"])
        np.testing.assert_array_equal(bits(rsc), bits(hits["score"]))
    assert rtotal < m.ref_topk(terms, boosts, 10, "bm25")[2]


def test_window_runs():
    """how the clamped grids deal the ten windows, and which of them derive"""
    assert wt.DOC_COUNT == 9 * wt.WIN + 300
    assert [wt.split(g) for g in (1, 2, 3, 4)] == [
        [10], [5, 5], [4, 4, 2], [3, 3, 3, 1]]
    assert wt.split(8) == [2, 2, 2, 2, 2, 0, 0, 0]   # workgroups w/o window
    assert wt.split(10) == [1] * 10                  # unset: one each
    # grid 1: first-window recount, a derive right after it, a derive at an
    # absolute w % 4 == 0 that is not the first, three non-derive in a row
    assert wt.derive_windows(0, 10) == [0, 1, 4, 8]
    # grid 2, second workgroup: its first window is no multiple of 4
    assert wt.derive_windows(5, 10) == [5, 6, 8]
    # the default geometry: two windows, both in one workgroup at grid 1
    assert -(-wt.DOC_COUNT // 24576) == 2


def test_early_locks_the_threshold(m):
    """k = 3 on `early`: the three best of window 0 score more than twice
    what any doc of the quiet windows scores, so with 256 score bins the
    quiet windows hold no candidate once window 0 has been derived; windows
    5 and 8 hold two docs each in the top bin again"""
    terms = m.groups["early"]
    u, s, _, _ = m.ref_scores(terms, [1.0], "bm25")
    w = wt.window_of(u)
    spike = np.isin(u, m.spikes)
    assert {int(x): int(spike[w == x].sum()) for x in np.unique(w[spike])} \
        == wt.SPIKES
    third = np.sort(s[w == 0])[-3]
    for q in wt.QUIET:
        assert (w == q).sum() >= 40
        assert s[w == q].max() * 2 < third
    assert s[spike].min() * 256 > s.max() * 255       # all in the top bin
    rd, _, _ = m.ref_topk(terms, [1.0], 3, "bm25")
    assert np.all(np.isin(rd, m.spikes))


def test_hole_and_term_ends(m):
    recs, _, _ = m.parse()
    W = wt.WIN
    # hole: window 2 holds exactly one item and no posting of it
    wins = m.window_items(m.groups["hole"])
    assert len(wins[2]) == 1
    docs = m.postings[m.idx["hole"]][0]
    assert not np.any(wt.window_of(docs) == 2)
    assert np.any(wt.window_of(docs) == 3)
    r = wins[2][0][1]
    assert r["prev"] < 2 * W and r["last"] > 3 * W
    # ends_mid: items in windows 0-3, none behind
    wins = m.window_items(m.groups["ends_mid"])
    assert [len(it) > 0 for it in wins] == [True] * 4 + [False] * 6
    # ends_on_hi: the last block ends exactly on window 4's hi
    assert recs[m.idx["ends_on_hi"]][-1]["last"] == 5 * W
    wins = m.window_items(m.groups["ends"])
    assert len(wins[4]) >= 1 and all(len(it) == 0 for it in wins[5:])


def test_dense_term(m):
    """more blocks in a window than descriptors are staged (32) at 4096
    docs, more than a 64-lane ballot counts at 24576, and a block across
    every window edge"""
    d = [m.idx["dense"]]
    small = m.window_items(d)
    assert max(len(it) for it in small) > wt.rs.DCACHE
    big = m.window_items(d, 24576)
    assert len(big) == 2 and len(big[0]) > 128 and len(big[1]) > 64
    recs, _, _ = m.parse()
    for e in range(1, wt.NWIN):
        hi = e * wt.WIN
        assert any(r["prev"] < hi < r["last"] for r in recs[d[0]])
