"""CPU side of the general-window matrix (tests/general_window_matrix.py):
the numpy fp32 term-major reference equals the CPU oracle bit for bit on
every case the GPU test runs, the corpus holds the shapes its docstring
claims (read from the raw arrays and the blob's descriptors), the conditions
that keep a GPU case from passing vacuously hold on the reference alone, and
each wrong-on-purpose reference differs from the true one on a named case."""

import numpy as np
import pytest

import general_window_matrix as gw
from oracle import pyoracle as po


@pytest.fixture(scope="module")
def m():
    return gw.matrix()


@pytest.fixture(scope="module")
def by_label(m):
    return {c[0]: c for c in gw.cases(m)}


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def same(a, b):
    return (a[2] == b[2] and np.array_equal(a[0], b[0]) and
            np.array_equal(bits(a[1]), bits(b[1])))


def test_cases_cover_the_issue(m):
    labels = [c[0] for c in gw.cases(m)]
    assert len(set(labels)) == len(labels)
    seen = {(lb.split()[0], mm) for lb, _, _, mm, _ in gw.cases(m)}
    for g in ("main", "decoys", "early", "hole", "ends", "dense", "wide32"):
        assert any(p == g for p, _ in seen), g
    assert {(g, mm) for g, mm in seen if g == "main"} == {
        ("main", 1), ("main", 2), ("main", 3), ("main", 5)}
    assert {("decoys", 2), ("decoys", 3), ("dense", 2), ("wide32", 3),
            ("wide32", 32)} <= seen
    terms = m.groups["main"]
    for mm in (1, 2, 3, 5):
        n = m.ref_count(terms, mm)
        ks = {k for lb, _, _, mm_, k in gw.cases(m)
              if lb.startswith("main ") and mm_ == mm}
        assert ks == {1, 3, 10, 1000, n, n + 7}, mm
        assert len(ks) == 6


def test_reference_equals_oracle(m):
    """doc ids, score bits and totals; and the restated histogram model
    (bins over smax, threshold at the k-th counted doc) returns the same"""
    for label, terms, boosts, mm, k in gw.cases(m):
        ref = m.ref_topk(terms, boosts, k, "bm25", mm)
        orc = m.oracle_topk(terms, boosts, k, "bm25", mm)
        assert ref[2] == orc[2] == m.ref_count(terms, mm), label
        np.testing.assert_array_equal(ref[0], orc[0], err_msg=label)
        np.testing.assert_array_equal(bits(ref[1]), bits(orc[1]),
                                      err_msg=label)
        assert same(ref, m.binned_topk(terms, boosts, k, mm)), label
        assert len(ref[0]) == min(k, ref[2]), label


def test_live_reference_equals_oracle(m):
    live = gw.live_mask(m)
    words = gw.live_words(m, live)
    for label, terms, boosts, mm, _ in gw.live_cases(m):
        for k in (gw.LIVE_K, m.doc_count):
            rd, rsc, rtotal = m.ref_topk_live(terms, boosts, k, "bm25", mm,
                                              live)
            hits, ototal = po.execute_topk([m.blob], terms, boosts, k,
                                           min_match=mm, live_mask=words)
            assert rtotal == ototal == m.ref_count(terms, mm, live), label
            np.testing.assert_array_equal(rd, hits["doc"], err_msg=label)
            np.testing.assert_array_equal(bits(rsc), bits(hits["score"]),
                                          err_msg=label)
            assert same((rd, rsc, rtotal),
                        m.binned_topk(terms, boosts, k, mm, live)), label
        assert rtotal < m.ref_count(terms, mm), label


def test_dealing():
    """how the clamped grids deal the ten windows, and which derive"""
    assert gw.DOC_COUNT == 9 * 24576 + 300 == 221484 and gw.WIN == 24576
    assert [gw.split(g) for g in (1, 2, 3, 4)] == [
        [10], [5, 5], [4, 4, 2], [3, 3, 3, 1]]
    assert gw.split(8) == [2, 2, 2, 2, 2, 0, 0, 0]
    assert gw.split(10) == [1] * 10                  # unset: one each
    assert gw.runs(1) == [(0, 10)]
    assert gw.runs(2) == [(0, 5), (5, 10)]
    assert gw.runs(3) == [(0, 4), (4, 8), (8, 10)]
    assert gw.runs(4) == [(0, 3), (3, 6), (6, 9), (9, 10)]
    assert gw.runs(8) == [(0, 2), (2, 4), (4, 6), (6, 8), (8, 10)]
    # grid 1: w_lo and w_lo + 1 derive, 2 and 3 do not, 4 derives without
    # being the first, 5-7 are three non-derive in a row, 8 derives, 9 is
    # the short one and does not
    assert gw.derive_windows(0, 10) == [0, 1, 4, 8]
    assert [w for w in range(10) if w not in gw.derive_windows(0, 10)] == [
        2, 3, 5, 6, 7, 9]
    # grid 2, second workgroup: its first window is no multiple of 4
    assert gw.derive_windows(5, 10) == [5, 6, 8]
    assert gw.derive_windows(3, 6) == [3, 4]         # grid 4
    assert gw.derive_windows(9, 10) == [9]           # the short window first
    los, his = gw.bounds()
    assert his[9] - los[9] + 1 == 300 and his[9] == gw.DOC_COUNT


def test_dense_term(m):
    """192 blocks in every full window, six times the staged descriptors;
    a block across every window edge"""
    d = [m.idx["dense"]]
    wins = m.window_items(d, gw.WIN)
    assert len(wins) == 10
    for it in wins[:9]:
        assert len(it) > gw.rs.DCACHE and len(it) >= 192
    recs, _, _ = m.parse()
    for e in range(1, gw.NWIN):
        hi = e * gw.WIN
        assert any(r["prev"] < hi < r["last"] for r in recs[d[0]])


def test_hole_and_term_ends(m):
    recs, _, _ = m.parse()
    W = gw.WIN
    hole = m.idx["hole"]
    wins = m.window_items([hole], W)
    assert len(wins[2]) == 1
    docs = m.postings[hole][0]
    assert not np.any(gw.window_of(docs) == 2)
    assert np.any(gw.window_of(docs) == 3)
    r = wins[2][0][1]
    assert r["prev"] < 2 * W and r["last"] > 3 * W
    assert {0, 1} <= set(gw.window_of(docs[:gw.BLOCK]).tolist())
    # ends_mid: items in windows 0-3, none from window 4 on
    wins = m.window_items([m.idx["ends_mid"]], W)
    assert [len(it) > 0 for it in wins] == [True] * 4 + [False] * 6
    last = m.postings[m.idx["ends_mid"]][0][-1]
    assert 3 * W + 1 < last == 3 * W + W // 2 < 4 * W
    # ends_on_hi: the last doc is window 4's hi
    los, his = gw.bounds()
    assert recs[m.idx["ends_on_hi"]][-1]["last"] == his[4] == 5 * W
    wins = m.window_items(m.groups["ends"][:2], W)
    assert len(wins[4]) >= 1 and all(len(it) == 0 for it in wins[5:])
    # partners: each shape exists under min-match 2 with bg as well
    bg = m.postings[m.idx["bg"]][0]
    for name in ("hole", "ends_mid", "ends_on_hi"):
        docs = m.postings[m.idx[name]][0]
        shared = np.isin(docs, bg)
        assert 0.25 < shared.mean() < 0.6, name
        assert shared[-1] or name == "hole"
    assert np.isin(his[4], bg) and np.isin(3 * W + W // 2, bg)


def counts_at(m, terms, docs):
    u, _, cnt, _ = m.ref_scores(terms, [1.0] * len(terms), "bm25")
    out = np.zeros(len(docs), dtype=np.int64)
    at = np.searchsorted(u, docs)
    hit = (at < len(u)) & (u[np.minimum(at, len(u) - 1)] == docs)
    out[hit] = cnt[at[hit]]
    return out


def test_edges_and_their_neighbours(m):
    los, his = gw.bounds()
    edges = np.unique(np.concatenate([los, his]))
    np.testing.assert_array_equal(edges, m.edges)
    assert len(edges) == 20
    # every edge is an AND match of (bg, bg2), and of `near`'s AND? no:
    # near holds lo + 1 and hi - 1 only
    two = m.terms(["bg", "bg2"])
    assert np.all(counts_at(m, two, edges) == 2)
    # lo + 1 and hi - 1 of every window: exactly min_match - 1 terms
    near = np.concatenate([los + 1, his - 1])
    assert len(np.unique(near)) == 20
    assert np.all(counts_at(m, two, near) == 1)
    for g, mm in (("main", 2), ("decoys", 2), ("near", 3), ("wide32", 3)):
        assert np.all(counts_at(m, m.groups[g], near) == mm - 1), g
    # ... and half of them under (early, bg) at its AND
    c = counts_at(m, m.groups["early"], near)
    assert set(c.tolist()) == {0, 1}
    # the edges have count min_match - 1 under decoys at min-match 3
    assert np.all(counts_at(m, m.groups["decoys"], edges) == 2)
    # the 32-term doc on each edge; doc 1 is not in dense
    c = counts_at(m, m.groups["wide32"], edges)
    assert c[0] == 31 and edges[0] == 1 and np.all(c[1:] == 32)
    # five-term docs in the edge words of windows 0-3
    five = np.concatenate([los[0:4] + 3, his[0:3] - 3])
    assert np.all(counts_at(m, m.groups["main"], five) == 5)
    # decoys in edge words
    planted = np.concatenate([los[1:5] + 2, his[4:8] - 2])
    assert np.all(np.isin(planted, m.decoys))


def test_decoys(m, by_label):
    """a decoy is in no term of its plan but `decoy`, is no match at
    min-match 2, and sits in a score bin above every true match (bins as
    the kernel computes them: (u32)(s * 256 / smax), smax restated from
    prep_plan_stats): a leak into the histogram drops every true hit"""
    terms = m.groups["decoys"]
    boosts = gw.rs.boosts_for(terms)
    assert len(m.decoys) == gw.NDECOY == 40
    w = gw.window_of(m.decoys)
    assert (w == 0).sum() == 31 and (w == 9).sum() == 1
    for name in m.names:
        if name not in ("decoy", "dense"):
            assert not np.any(np.isin(m.decoys, m.postings[m.idx[name]][0]))
    assert np.all(counts_at(m, terms, m.decoys) == 1)
    u, s, cnt, _ = m.ref_scores(terms, boosts, "bm25")
    b = m.bins(terms, boosts, s)
    is_decoy = np.isin(u, m.decoys)
    assert b[is_decoy].min() > b[cnt >= 2].max()
    assert s[is_decoy].min() > 2 * s[cnt >= 2].max()
    seen = 0
    for label, _, _, mm, k in by_label.values():
        if label.startswith("decoys ") and mm == 2 and k <= gw.NDECOY:
            seen += 1
            true = m.ref_topk(terms, boosts, k, "bm25", 2)
            assert len(true[0]) == k and not np.any(np.isin(true[0],
                                                            m.decoys))
            leak = m.wrong("decoys_counted", terms, boosts, k, 2)
            assert len(leak[0]) == 0, label
    assert seen >= 4
    # min-match 3: no match at all, count 2 everywhere
    assert m.ref_count(terms, 3) == 0
    assert (cnt == 2).sum() > 2000


def test_live_mask(m):
    """8 dead top scorers, 2 live ones, k = 5: counting dead docs locks the
    threshold on the spike bin and leaves 2 hits"""
    live = gw.live_mask(m)
    sw = gw.window_of(m.spikes)
    assert {int(x): int((sw == x).sum()) for x in np.unique(sw)} == gw.SPIKES
    dead = m.spikes[~live[m.spikes]]
    alive = m.spikes[live[m.spikes]]
    assert len(dead) == 8 and len(alive) == 2
    assert set(gw.window_of(alive).tolist()) == {8}
    assert len(dead) >= gw.LIVE_K > len(alive)
    assert 0.2 < 1 - live[1:].mean() < 0.3
    W = gw.WIN
    assert not live[W] and live[W + 1] and live[4 * W] and not live[4 * W + 1]
    assert not live[9 * W] and live[9 * W + 1]
    for label, terms, boosts, mm, spiky in gw.live_cases(m):
        true = m.ref_topk_live(terms, boosts, gw.LIVE_K, "bm25", mm, live)
        assert len(true[0]) == gw.LIVE_K, label
        if not spiky:
            continue
        assert np.all(counts_at(m, terms, m.spikes) >= mm), label
        assert np.all(np.isin(alive, true[0])), label
        wrong = m.wrong("dead_counted", terms, boosts, gw.LIVE_K, mm, live)
        np.testing.assert_array_equal(np.sort(wrong[0]), np.sort(alive),
                                      err_msg=label)


def test_early_locks_the_threshold(m, by_label):
    """`early` at its AND with k = 3: the six spikes of window 0 match at
    min-match 2 and every quiet doc's bin is below theirs, so the quiet
    windows hold no candidate once window 0 has been derived"""
    label, terms, boosts, mm, k = by_label["early mm=2 k=3"]
    u, s, cnt, _ = m.ref_scores(terms, boosts, "bm25")
    match = cnt >= 2
    spike = np.isin(u, m.spikes)
    assert np.all(match[spike]) and spike.sum() == 10
    w = gw.window_of(u)
    assert (spike & (w == 0)).sum() == 6
    b = m.bins(terms, boosts, s)
    # one bin for all ten: every spike stays a candidate whatever the
    # threshold locks on, so the candidate count is at least their number
    assert len(set(b[spike].tolist())) == 1 and b[spike][0] >= 250
    assert b[match & ~spike].max() < b[spike].min()
    assert s[match & ~spike].max() * 2 < s[spike].min()
    for q in gw.QUIET:
        assert (match & (w == q)).sum() >= 40
    rd, _, total = m.ref_topk(terms, boosts, 3, "bm25", 2)
    assert np.all(np.isin(rd, m.spikes[gw.window_of(m.spikes) == 0]))
    assert total == match.sum() > 500


WRONG_ON = {    # wrong reference -> the named cases on which it must differ
    "decoys_counted": ("decoys mm=2 k=1", "decoys mm=2 k=10",
                       "decoys mm=2 k=40"),
    "mm_minus_1": ("decoys mm=2 k=10", "main mm=2 k=10", "main mm=5 k=10",
                   "dense mm=2 k=10", "wide32 mm=32 k=10",
                   "near mm=3 k=10"),
    "edges_dropped": ("near mm=2 k=10", "wide32 mm=32 k=10",
                      "dense mm=2 k=1000", "main mm=2 k=1000"),
    "no_recount_total": ("main mm=2 k=10", "dense mm=2 k=10",
                         "wide32 mm=3 k=10", "early mm=2 k=3"),
}


@pytest.mark.parametrize("kind", list(WRONG_ON))
def test_wrong_references_differ(m, by_label, kind):
    for label in WRONG_ON[kind]:
        _, terms, boosts, mm, k = by_label[label]
        true = m.ref_topk(terms, boosts, k, "bm25", mm)
        for grid in (1, 2, 3, 4, 8):
            wrong = m.wrong(kind, terms, boosts, k, mm, grid=grid)
            assert not same(true, wrong), (kind, label, grid)


def test_wrong_dead_counted_differs(m):
    live = gw.live_mask(m)
    for label, terms, boosts, mm, spiky in gw.live_cases(m):
        if not spiky:
            continue
        true = m.ref_topk_live(terms, boosts, gw.LIVE_K, "bm25", mm, live)
        wrong = m.wrong("dead_counted", terms, boosts, gw.LIVE_K, mm, live)
        assert not same(true, wrong), label


def test_count_and_stream_references(m):
    live = gw.live_mask(m)
    for label, terms, mm in gw.count_cases(m):
        _, _, total = m.oracle_topk(terms, [1.0] * len(terms), 1, "bm25", mm)
        assert m.ref_count(terms, mm) == total, label
        assert m.ref_count(terms, mm, live) <= total, label
        s = m.ref_stream(terms, mm)
        assert np.all(np.diff(s.astype(np.int64)) > 0), label
    labels = [c[0] for c in gw.count_cases(m)]
    assert labels == ["main mm=1", "main mm=2", "main mm=3", "main mm=5",
                      "decoys mm=1", "decoys mm=2", "decoys mm=3",
                      "dense mm=1", "dense mm=2",
                      "wide32 mm=1", "wide32 mm=2", "wide32 mm=3",
                      "wide32 mm=32"]
