"""Codec-matrix corpus, CPU side: the corpus really contains every block
family, bit width, tail length and straddle state it claims to, the CPU
oracle reproduces an independent numpy fp32 scorer over the raw arrays bit
for bit on it, and that fp32 scorer stays inside the documented 1e-5 of an
fp64 evaluation of the same formulas. tests/test_gpu_codec_matrix.py then
holds every GPU top-k path to the same numpy reference."""

import numpy as np
import pytest

import codec_matrix as cm


@pytest.fixture(scope="module")
def m():
    return cm.matrix()


def test_matrix_coverage(m):
    """Keeps the matrix from silently thinning when the encoder's size
    heuristics change: every targeted tag, both flag states, every fused
    width triple (checked against the payload tags), both straddle states,
    every tail length, and fused/non-fused neighbours at the wave strides."""
    blks = m.blocks()
    dtags, ftags, ntags = set(), set(), set()
    fdb, ffb, fnb = set(), set(), set()
    straddle = set()
    tails = set()
    for recs in blks:
        for i, r in enumerate(recs):
            dtags.add(r["dtag"])
            ftags.add(r["ftag"])
            ntags.add(r["ntag"])
            crosses = (r["first"] - 1) // cm.WIN != (r["last"] - 1) // cm.WIN
            straddle.add((r["fused"], crosses))
            if r["len"] < cm.BLOCK:
                assert i == len(recs) - 1
                tails.add((r["len"], len(recs) == 1))
            if r["fused"]:
                db = (r["flags"] >> 1) & 31
                fb = (r["flags"] >> 6) & 31
                nb = (r["flags"] >> 11) & 31
                assert r["len"] == cm.BLOCK
                assert r["dtag"] - 8 + 2 == db
                assert r["ftag"] - 5 + 1 == fb
                assert r["ntag"] - 5 + 1 == nb
                fdb.add(db)
                ffb.add(fb)
                fnb.add(nb)
            else:
                # not the fused shape: some stream is not bitpacked
                assert (r["len"] < cm.BLOCK or r["dtag"] < 8 or
                        r["ftag"] < 5 or r["ntag"] < 5)
    # doc families: VALUES, all-same 8/16/32, bitset, svb, delta-svb and
    # delta-bitpack 2..24 (tag 8 = width 2); tag 6 is never written
    assert dtags >= {0, 1, 2, 3, 4, 5, 7} | {8 + w - 2 for w in cm.DOC_WIDTHS}
    # freq / norm families: VALUES, all-same 8/16/32, svb, bitpack 2..31
    # (tag 5 = width 1, which needs a zero value: excluded, freq/norm >= 1)
    want = {0, 1, 2, 3, 4} | {5 + w - 1 for w in cm.FREQ_WIDTHS}
    assert ftags >= want
    assert ntags >= want
    # the descriptor-carried widths the fused decoders read
    assert fdb >= set(cm.DOC_WIDTHS)
    assert ffb >= set(cm.FREQ_WIDTHS)
    assert fnb >= set(cm.NORM_WIDTHS)
    assert straddle == {(0, False), (0, True), (1, False), (1, True)}
    assert tails >= {(n, only) for n in cm.TAIL_LENGTHS
                     for only in (False, True)}
    # one term of >= 64 blocks in which a fused block is paired with a
    # non-fused one at the wave stride of every compiled sweep geometry
    # (1024, 512, 256 threads = 16, 8, 4 waves), both inside one window
    recs = blks[m.idx["mixed"]]
    assert len(recs) >= 64
    for stride in (16, 8, 4):
        kinds = set()
        for a, b in zip(recs, recs[stride:]):
            hi = ((a["first"] - 1) // cm.WIN + 1) * cm.WIN
            if a["len"] == b["len"] == cm.BLOCK and b["prev"] < hi:
                kinds.add((a["fused"], b["fused"]))
        assert kinds == {(0, 0), (0, 1), (1, 0), (1, 1)}, (stride, kinds)
    # descriptors bound their blocks exactly (WAND reads these)
    for t, recs in enumerate(blks):
        docs, freqs = m.postings[t]
        for i, r in enumerate(recs):
            sl = slice(cm.BLOCK * i, cm.BLOCK * i + r["len"])
            assert r["max_freq"] == int(freqs[sl].max())
            assert r["min_norm"] == int(m.norms[docs[sl]].min())
            assert r["last"] == int(docs[sl][-1])
    assert m.norms[1:].min() >= 1
    # the bin-edge pair: B outscores A, both outscore the rest of the term
    a, b = m.edge_docs
    rd, rs, _ = m.ref_topk([m.idx["edge"]], [1.0], 3, "bm25")
    assert [int(d) for d in rd[:2]] == [b, a] and rs[0] > rs[1] > rs[2]
    assert (a - 1) // cm.WIN == 300 and (b - 1) // cm.WIN == 302


def _check_oracle(m, terms, boosts, k, scorer, min_match=1):
    rd, rs, rtotal = m.ref_topk(terms, boosts, k, scorer, min_match)
    od, os_, ototal = m.oracle_topk(terms, boosts, k, scorer, min_match)
    assert ototal == rtotal
    np.testing.assert_array_equal(od, rd)
    np.testing.assert_array_equal(os_.view(np.uint32), rs.view(np.uint32))


@pytest.mark.parametrize("scorer", cm.SCORERS)
def test_oracle_equals_numpy_single_terms(m, scorer):
    """every term alone with k > df: the oracle's hits are the complete
    posting list with the numpy scores, bit for bit, and total == df"""
    for t, (docs, _) in enumerate(m.postings):
        _check_oracle(m, [t], [1.0], len(docs) + 1, scorer)
        assert m.ref_topk([t], [1.0], 1, scorer)[2] == len(docs)


@pytest.mark.parametrize("scorer", cm.SCORERS)
def test_oracle_equals_numpy_groups(m, scorer):
    """the multi-term plans the GPU tests run (term-major fp32 sums)"""
    for gi, (name, g) in enumerate(m.groups.items()):
        boosts = cm.group_boosts(len(g), gi)
        n_all = len(m.ref_scores(g, boosts, scorer)[0])
        for k in (n_all + 1, 10, 1):
            _check_oracle(m, g, boosts, k, scorer)
    for name, g in m.small_groups.items():
        _check_oracle(m, g, [1.0] * 4, 1000, scorer)
    g = m.groups["freq_widths"]
    _check_oracle(m, g, [1.0] * len(g), 500, scorer, min_match=2)


def test_fp32_reference_within_documented_tolerance(m):
    """The fp32 reference against an fp64 evaluation of the same formulas,
    matched by doc id. Tolerance: the project's documented 1e-5 — for BM25
    as an absolute error relative to the sum of num over the doc's matched
    terms (num - num*c1/(c1+f) cancels at huge norms, so relative-to-score
    is meaningless there), for the TFIDF scorers relative to the score.

    Measured on this corpus (max over every single term and every group):
    bm25 1.65e-07, tfidf 1.99e-07, tfidf_norm 2.27e-07."""
    plans = [([t], [1.0]) for t in range(len(m.names))]
    plans += [(g, cm.group_boosts(len(g), gi))
              for gi, g in enumerate(m.groups.values())]
    worst = {}
    for scorer in cm.SCORERS:
        w = 0.0
        for terms, boosts in plans:
            d32, s32, _, _ = m.ref_scores(terms, boosts, scorer)
            d64, s64, _, nsum = m.ref_scores(terms, boosts, scorer,
                                             fp64=True)
            np.testing.assert_array_equal(d32, d64)
            denom = nsum if scorer == "bm25" else s64
            assert np.all(denom > 0)
            w = max(w, float(np.max(np.abs(s32.astype(np.float64) - s64) /
                                    denom)))
        worst[scorer] = w
    print("fp32 vs fp64 max deviation:", worst)
    for scorer, w in worst.items():
        assert w <= 1e-5, (scorer, w)
