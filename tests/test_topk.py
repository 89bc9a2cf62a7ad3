"""Segment + BM25 + top-k oracle tests (CPU).

Pins:
  - the transcribed bm25_test golden corpus rank orders (tests/golden/)
  - oracle exact vs mechanics vs multithreaded paths agree
  - oracle scores vs an independent numpy fp32/fp64 scorer
  - sharded execution with injected global stats == single-segment result
  - full-term decode round trip on synthetic corpora
"""

import json
import os

import numpy as np
import pytest

import serenedb_amd as sa
from oracle import pyoracle as po

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")


def build_term_corpus(docs_fields, unit_features=False):
    """docs_fields: list (per doc, 1-based ids implied) of token lists.
    Returns (blob, vocab dict term->idx, norms). unit_features mirrors the
    reference's test_query corpora indexed WITHOUT freq/norm features
    (bm25_test.cpp:465-500 StringField insert): freq=1 per posting and a
    constant norm, making BM25 rank by idf sums with doc-order ties."""
    vocab = {}
    for f in docs_fields:
        for t in f:
            vocab.setdefault(t, len(vocab))
    postings = [[] for _ in vocab]
    for d, f in enumerate(docs_fields, start=1):
        for t in sorted(set(f), key=lambda x: vocab[x]):
            postings[vocab[t]].append((d, 1 if unit_features else f.count(t)))
    plist = []
    for pl in postings:
        docs = np.array([d for d, _ in pl], dtype=np.uint32)
        freqs = np.array([c for _, c in pl], dtype=np.uint32)
        plist.append((docs, freqs))
    norms = np.zeros(len(docs_fields) + 1, dtype=np.uint32)
    for d, f in enumerate(docs_fields, start=1):
        norms[d] = 1 if unit_features else len(f)
    blob = sa.build_segment(len(docs_fields), plist, norms)
    return blob, vocab, norms


def numpy_bm25_topk(docs_fields, terms, k1=1.2, b=0.75, fp64=False):
    """independent reference scorer (term-major fp32, or fp64)."""
    N = len(docs_fields)
    lens = np.array([len(f) for f in docs_fields], dtype=np.uint32)
    ttf = int(lens.sum())
    dt = np.float64 if fp64 else np.float32
    scores = np.zeros(N, dtype=dt)
    matched = np.zeros(N, dtype=bool)
    for t in terms:
        df = sum(1 for f in docs_fields if t in f)
        if df == 0:
            continue
        idf = dt(np.log1p((np.float64(N - df) + 0.5) / (np.float64(df) + 0.5)))
        nc = dt(np.float32(k1) - np.float32(k1) * np.float32(b))
        avg = dt(np.float32(ttf) / np.float32(N))
        nl = dt(np.float32(np.float32(k1) * np.float32(b)) / avg)
        num = dt(np.float32(1.0) * np.float32(k1 + 1)) * idf
        for d, f in enumerate(docs_fields):
            freq = f.count(t)
            if freq:
                matched[d] = True
                c1 = nc + nl * dt(lens[d])
                scores[d] += num - num * c1 / (c1 + dt(freq))
    order = sorted(np.nonzero(matched)[0],
                   key=lambda d: (-float(scores[d]), d))
    return order, scores


@pytest.mark.parametrize("case_idx", [0, 1, 2, 3, 4, 5, 6, 7])
def test_golden_rank_order(case_idx):
    g = json.load(open(os.path.join(GOLDEN,
                                    "bm25_simple_sequential_order.json")))
    docs_fields = g["docs"]
    case = g["cases"][case_idx]
    scorer = case.get("scorer", "bm25")
    unit = case.get("features") == "no_freq_no_norm"
    blob, vocab, _ = build_term_corpus(docs_fields, unit_features=unit)
    term_idx = [vocab[t] for t in case["terms"]]
    boosts = [1.0] * len(term_idx)
    hits, total = po.execute_topk([blob], term_idx, boosts, k=8,
                                  scorer=scorer)
    got_seq = [int(h["doc"]) - 1 for h in hits]  # seq = doc-1 in this corpus
    assert got_seq == case["expected_seq_order"], case["cite"]
    if scorer == "bm25" and not unit:
        # mechanics path agrees
        mhits, mtotal = po.execute_topk_mech([blob], term_idx, boosts, k=8)
        assert total == mtotal
        assert [int(h["doc"]) for h in mhits[:len(got_seq)]] == \
            [g + 1 for g in got_seq]
        # independent numpy scorer agrees bit-for-bit on scores
        order, scores = numpy_bm25_topk(docs_fields, case["terms"])
        for h in hits:
            assert h["score"] == np.float32(scores[int(h["doc"]) - 1])


def synth_corpus(seed, doc_count, sels):
    postings = [sa.synth_postings(seed, doc_count, t, s)
                for t, s in enumerate(sels)]
    norms = sa.synth_norms(seed, doc_count)
    blob = sa.build_segment(doc_count, postings, norms)
    return blob, postings, norms


def test_segment_decode_roundtrip():
    blob, postings, _ = synth_corpus(42, 50_000, [0.05, 0.02, 0.5, 0.001])
    for t, (docs, freqs) in enumerate(postings):
        ddocs, dfreqs = po.decode_term(blob, t, len(docs))
        np.testing.assert_array_equal(ddocs, docs)
        np.testing.assert_array_equal(dfreqs, freqs)


def brute_topk(postings, norms, doc_count, sels_used, k, min_match=1,
               k1=1.2, b=0.75):
    """independent dense fp32 scorer over raw postings"""
    ttf = int(norms[1:].sum())
    scores = np.zeros(doc_count + 1, dtype=np.float32)
    cnt = np.zeros(doc_count + 1, dtype=np.int32)
    for (docs, freqs) in postings:
        df = len(docs)
        if df == 0:
            continue
        idf = np.float32(np.log1p(
            (np.float64(doc_count - df) + 0.5) / (np.float64(df) + 0.5)))
        nc = np.float32(np.float32(k1) - np.float32(k1) * np.float32(b))
        avg = np.float32(np.float32(ttf) / np.float32(doc_count))
        nl = np.float32(np.float32(np.float32(k1) * np.float32(b)) / avg)
        num = np.float32(np.float32(1.0) * np.float32(k1 + 1)) * idf
        c1 = nc + nl * norms[docs].astype(np.float32)
        contrib = num - num * c1 / (c1 + freqs.astype(np.float32))
        scores[docs] += contrib
        cnt[docs] += 1
    match_docs = np.nonzero(cnt >= min_match)[0]
    flt_min = np.float32(1.17549435e-38)
    acc = match_docs[scores[match_docs] > flt_min]
    order = sorted(acc, key=lambda d: (-float(scores[d]), d))[:k]
    return order, scores, len(match_docs)


@pytest.mark.parametrize("seed,mm", [(42, 1), (43, 1), (44, 2), (45, 4)])
def test_topk_exact_vs_brute(seed, mm):
    doc_count = 30_000
    sels = [0.1, 0.05, 0.02, 0.01]
    blob, postings, norms = synth_corpus(seed, doc_count, sels)
    k = 100
    term_idx = list(range(4))
    boosts = [1.0] * 4
    hits, total = po.execute_topk([blob], term_idx, boosts, k, min_match=mm)
    order, scores, nmatch = brute_topk(postings, norms, doc_count, sels, k,
                                       min_match=mm)
    assert total == nmatch
    assert [int(h["doc"]) for h in hits] == [int(d) for d in order]
    for h in hits:  # fp32 bit-exact (term-major order both sides)
        assert h["score"] == scores[int(h["doc"])], int(h["doc"])


def test_wand_block_max_fixture():
    """Transcribed WAND pruning fixture (formats_15_tests.cpp:901-917
    LongPostingsWandThreshold60/100): docs 1..10000 with freqs from a
    default-seeded mt19937 normal draw (committed vectors +
    tools/gen_wand_freqs.cpp). The reference's wanderator visits exactly
    the docs of 128-blocks whose block-max freq exceeds the threshold,
    plus the tail block (its skip list has no tail entry): 1680 at
    threshold 60 over N(40,7), 16 at threshold 100 over N(50,13). This
    repo's per-block max_freq descriptors must reproduce those counts
    (the tail is modeled separately: our descriptors DO bound the tail —
    a documented refinement that can only prune more, never less)."""
    import ctypes as CT

    class _Desc(CT.Structure):
        _fields_ = [("prev_doc", CT.c_uint32), ("last_doc", CT.c_uint32),
                    ("doc_off", CT.c_uint32), ("freq_off", CT.c_uint32),
                    ("len", CT.c_uint16), ("flags", CT.c_uint16),
                    ("max_freq", CT.c_uint32), ("min_norm", CT.c_uint32)]

    class _View(CT.Structure):
        _fields_ = [("hdr", CT.c_void_p), ("terms", CT.c_void_p),
                    ("desc", CT.c_void_p), ("norms", CT.c_void_p),
                    ("payload", CT.c_void_p)]

    class _Term(CT.Structure):
        _fields_ = [("desc_begin", CT.c_uint64), ("desc_end", CT.c_uint64),
                    ("payload_begin", CT.c_uint64), ("df", CT.c_uint64),
                    ("max_freq", CT.c_uint32), ("pad", CT.c_uint32)]

    for fname, thr, expected_ref in (("wand_freqs_n40_7.txt", 60, 1680),
                                     ("wand_freqs_n50_13.txt", 100, 16)):
        freqs = np.array([int(x) for x in open(
            os.path.join(GOLDEN, fname))], dtype=np.uint32)
        assert len(freqs) == 10000
        docs = np.arange(1, 10001, dtype=np.uint32)
        norms = np.ones(10001, dtype=np.uint32)
        norms[0] = 0
        blob = sa.build_segment(10000, [(docs, freqs)], norms)
        buf = np.frombuffer(blob, dtype=np.uint8)
        v = _View()
        rc = sa.host().sdb_host_segment_parse(
            buf.ctypes.data_as(CT.c_void_p), CT.c_uint64(len(buf)),
            CT.byref(v))
        assert rc == 0, rc
        te = CT.cast(v.terms, CT.POINTER(_Term))[0]
        nblocks = te.desc_end - te.desc_begin
        darr = CT.cast(v.desc, CT.POINTER(_Desc))
        visited_ref_model = 0  # reference: tail block always visited
        for b in range(nblocks):
            d = darr[te.desc_begin + b]
            # our descriptor max_freq must equal the true block max
            exp_max = int(freqs[d.prev_doc:d.last_doc].max())
            assert d.max_freq == exp_max, (b, d.max_freq, exp_max)
            if d.len < 128 or d.max_freq > thr:
                visited_ref_model += d.len
        assert visited_ref_model == expected_ref, (fname, visited_ref_model)


def test_filter_boost_oracle():
    """Per-doc filter boost (HasFilterBoost scorer variants,
    bm25.cpp:112-140): fb folds into num BEFORE the score form, mirroring
    the reference's op order (c0 = boost*num, then c0 - c0*c1/(c1+freq)).
    Scores must equal the independent numpy replication bitwise; BM1
    (k1=0) + boost = f32(num * fb)."""
    doc_count = 30_000
    sels = [0.1, 0.05]
    blob, postings, norms = synth_corpus(50, doc_count, sels)
    rng = np.random.default_rng(13)
    fb = rng.uniform(0.5, 2.0, doc_count + 1).astype(np.float32)
    fb[0] = 0.0

    # multi-term: replicate the oracle's arithmetic independently in numpy
    ttf = int(norms[1:].sum())
    scores = np.zeros(doc_count + 1, dtype=np.float32)
    cnt = np.zeros(doc_count + 1, dtype=np.int32)
    for docs, freqs in postings:
        df = len(docs)
        idf = np.float32(np.log1p(
            (np.float64(doc_count - df) + 0.5) / (np.float64(df) + 0.5)))
        nc = np.float32(np.float32(1.2) - np.float32(1.2) * np.float32(0.75))
        avg = np.float32(np.float32(ttf) / np.float32(doc_count))
        nl = np.float32(np.float32(np.float32(1.2) * np.float32(0.75)) / avg)
        num = np.float32(np.float32(2.2)) * idf
        c1 = nc + nl * norms[docs].astype(np.float32)
        nm = num * fb[docs]  # reference op order: boost folds into num
        contrib = nm - nm * c1 / (c1 + freqs.astype(np.float32))
        scores[docs] += contrib
        cnt[docs] += 1
    hits, total = po.execute_topk([blob], [0, 1], [1.0, 1.0], 300,
                                  filter_boost=fb)
    assert total == int((cnt > 0).sum())
    for h in hits:
        assert h["score"] == scores[int(h["doc"])], int(h["doc"])

    # BM1 + filter boost: freq-independent fb*num per matching term
    hits1, _ = po.execute_topk([blob], [0], [1.0], 100, k1=0.0,
                               filter_boost=fb)
    df = len(postings[0][0])
    idf = np.float32(np.log1p(
        (np.float64(doc_count - df) + 0.5) / (np.float64(df) + 0.5)))
    num = np.float32(np.float32(1.0)) * idf  # (k+1)=1 at k=0
    assert len(hits1) == 100
    for h in hits1:
        assert h["score"] == np.float32(num * fb[int(h["doc"])])


def test_golden_multisegment_order():
    """Transcribed multi-segment disjunction fixture: the corpus split into
    even-seq / odd-seq segments, OR of terms {6, 8}, no freq/norm features.
    Expected {3, 7, 0, 2, 5} for BOTH scorers — bm25_test.cpp:734 and
    tfidf_test.cpp:759 — which pins the CROSS-SEGMENT stats merge (global
    df ranks term-8 docs above term-6 docs) and the tie order (the
    reference's multimap preserves segment-then-doc insertion order; this
    repo's total order reproduces it)."""
    g = json.load(open(os.path.join(GOLDEN,
                                    "bm25_simple_sequential_order.json")))
    docs_fields = g["docs"]
    vocab = {}
    for f in docs_fields:
        for t in f:
            vocab.setdefault(t, len(vocab))

    def build(seqs):
        postings = [[] for _ in vocab]
        for local, seq in enumerate(seqs, start=1):
            for t in sorted(set(docs_fields[seq]), key=lambda x: vocab[x]):
                postings[vocab[t]].append((local, 1))
        plist = [(np.array([d for d, _ in pl], dtype=np.uint32),
                  np.array([c for _, c in pl], dtype=np.uint32))
                 for pl in postings]
        norms = np.ones(len(seqs) + 1, dtype=np.uint32)
        norms[0] = 0
        return sa.build_segment(len(seqs), plist, norms)

    seq0, seq1 = [0, 2, 4, 6], [1, 3, 5, 7]
    b0, b1 = build(seq0), build(seq1)
    ti = [vocab["6"], vocab["8"]]
    for scorer in ("bm25", "tfidf"):
        hits, total = po.execute_topk([b0, b1], ti, [1.0, 1.0], 8,
                                      scorer=scorer)
        seqs = [(seq0 if h["segment"] == 0 else seq1)[int(h["doc"]) - 1]
                for h in hits]
        assert seqs == [3, 7, 0, 2, 5], (scorer, seqs)
        assert total == 5
    # single-term multi-segment case (bm25_test.cpp:609, tfidf_test.cpp:635
    # kExpected{0, 2, 5}): term "6" spans both segments, equal scores tie
    # in (segment, doc) order
    for scorer in ("bm25", "tfidf"):
        hits, total = po.execute_topk([b0, b1], [vocab["6"]], [1.0], 8,
                                      scorer=scorer)
        seqs = [(seq0 if h["segment"] == 0 else seq1)[int(h["doc"]) - 1]
                for h in hits]
        assert seqs == [0, 2, 5], (scorer, seqs)
        assert total == 3


def test_hybrid_chain_vs_brute():
    """Predicate-chain hybrid (ColFilterChain AND semantics): oracle chain
    vs independent numpy evaluation, and a vacuous extra predicate must
    reproduce the single-predicate hybrid exactly."""
    doc_count = 25_000
    sels = [0.1, 0.05]
    blob, postings, norms = synth_corpus(49, doc_count, sels)
    rng = np.random.default_rng(10)
    span = 1 << 20
    col0 = rng.integers(0, span, doc_count + 1).astype(np.int64)
    col1 = rng.integers(0, span, doc_count + 1).astype(np.int64)
    flo, fhi = int(span * 0.2), int(span * 0.8) - 1
    glim = int(span * 0.5)
    nb = 16
    hits, total, bcnt, bsum = po.execute_topk_hybrid_chain(
        blob, [0, 1], [1.0, 1.0], 50, [col0, col1], [3, 2],
        [flo, glim], [fhi, 0], nb)
    # numpy: survivors = matches AND col0 BETWEEN AND col1 >= glim
    order, scores, _ = brute_topk(postings, norms, doc_count, sels, 10**9)
    surv = [d for d in order
            if flo <= col0[d] <= fhi and col1[d] >= glim]
    assert total == len(surv)
    assert [int(h["doc"]) for h in hits] == surv[:50]
    ecnt = np.zeros(nb, dtype=np.int64)
    esum = np.zeros(nb, dtype=np.int64)
    for d in surv:
        b_ = min((col0[d] - flo) * nb // (fhi - flo + 1), nb - 1)
        ecnt[b_] += 1
        esum[b_] += col0[d]
    np.testing.assert_array_equal(bcnt, ecnt)
    np.testing.assert_array_equal(bsum, esum)
    # vacuous extra pred == single-pred hybrid
    h1, t1, c1, s1 = po.execute_topk_hybrid(
        blob, [0, 1], [1.0, 1.0], 50, col0, flo, fhi, nb)
    h2, t2, c2, s2 = po.execute_topk_hybrid_chain(
        blob, [0, 1], [1.0, 1.0], 50, [col0, col1], [3, 2],
        [flo, 0], [fhi, 0], nb)
    assert t1 == t2
    np.testing.assert_array_equal(h1["doc"], h2["doc"])
    np.testing.assert_array_equal(c1, c2)
    np.testing.assert_array_equal(s1, s2)


def test_bm1_zero_scores():
    """BM1 (k=0, bm25.cpp:112-140 Bm1Score + :333-336 dispatch): without a
    filter boost every score is memset to 0, so nothing beats the
    collector's FLT_MIN threshold -> empty top-k, matches still counted."""
    doc_count = 30_000
    sels = [0.1, 0.05]
    blob, postings, norms = synth_corpus(48, doc_count, sels)
    hits, total = po.execute_topk([blob], [0, 1], [1.0, 1.0], 50, k1=0.0)
    _, _, nmatch = brute_topk(postings, norms, doc_count, sels, 50)
    assert len(hits) == 0
    assert total == nmatch


def test_wide_plan_vs_brute():
    """32-term disjunction and min-match on the oracle side (the GPU wide
    -plan parity test leans on this being right)."""
    doc_count = 20_000
    rng = np.random.default_rng(7)
    sels = [float(s) for s in rng.uniform(0.005, 0.06, 32)]
    blob, postings, norms = synth_corpus(46, doc_count, sels)
    for mm in (1, 12):
        hits, total = po.execute_topk([blob], list(range(32)), [1.0] * 32,
                                      80, min_match=mm)
        order, scores, nmatch = brute_topk(postings, norms, doc_count, sels,
                                           80, min_match=mm)
        assert total == nmatch
        assert [int(h["doc"]) for h in hits] == [int(d) for d in order]
        for h in hits:
            assert h["score"] == scores[int(h["doc"])]


def test_mech_equals_exact():
    doc_count = 30_000
    blob, postings, norms = synth_corpus(7, doc_count, [0.08, 0.03, 0.01])
    for k in (1, 10, 100, 1000):
        hits, total = po.execute_topk([blob], [0, 1, 2], [1.0] * 3, k)
        mhits, mtotal = po.execute_topk_mech([blob], [0, 1, 2], [1.0] * 3, k)
        assert total == mtotal
        n = len(hits)
        np.testing.assert_array_equal(hits["doc"], mhits["doc"][:n])
        np.testing.assert_array_equal(hits["score"], mhits["score"][:n])


def test_mt_equals_exact():
    doc_count = 100_000
    blob, postings, norms = synth_corpus(9, doc_count, [0.05, 0.02])
    hits, total = po.execute_topk([blob], [0, 1], [1.0, 1.0], 200)
    for nthreads in (1, 4, 8):
        th, tt = po.execute_topk_mt(blob, [0, 1], [1.0, 1.0], 200,
                                    nthreads=nthreads)
        assert tt == total
        np.testing.assert_array_equal(th["doc"], hits["doc"])
        np.testing.assert_array_equal(th["score"], hits["score"])


def test_sharded_with_global_stats():
    """Two shards + injected global stats == one segment (multi-GPU path)."""
    doc_count = 40_000
    sels = [0.06, 0.02, 0.01]
    seed = 11
    full_blob, postings, norms = synth_corpus(seed, doc_count, sels)
    hits, total = po.execute_topk([full_blob], [0, 1, 2], [1.0] * 3, 150)

    half = doc_count // 2
    shard_blobs = []
    for lo, hi in ((1, half), (half + 1, doc_count)):
        shard_blobs.append(sa.build_synth_segment(seed, lo, hi, sels))
    dwt = [len(d) for d, _ in postings]
    gstats = (doc_count, int(norms[1:].sum()), dwt)
    all_cands = []
    totals = 0
    for si, (blob, base) in enumerate(zip(shard_blobs, (0, half))):
        h, t = po.execute_topk([blob], [0, 1, 2], [1.0] * 3, 150,
                               global_stats=gstats)
        totals += t
        for x in h:
            all_cands.append((float(x["score"]), int(x["doc"]) + base))
    # merge (allgather + host nth_element analogue)
    all_cands.sort(key=lambda sd: (-sd[0], sd[1]))
    got = all_cands[:150]
    assert totals == total
    assert [d for _, d in got] == [int(d) for d in hits["doc"]]
    assert [s for s, _ in got] == [float(s) for s in hits["score"]]


def test_empty_and_edge_cases():
    # term with no postings; k > matches; single-doc segment
    doc_count = 1000
    docs = np.array([500], dtype=np.uint32)
    freqs = np.array([3], dtype=np.uint32)
    norms = np.ones(doc_count + 1, dtype=np.uint32)
    blob = sa.build_segment(doc_count, [(docs, freqs),
                                        (np.array([], dtype=np.uint32),
                                         np.array([], dtype=np.uint32))],
                            norms)
    hits, total = po.execute_topk([blob], [0, 1], [1.0, 1.0], 10)
    assert total == 1
    assert len(hits) == 1 and hits[0]["doc"] == 500
    # empty term alone
    hits, total = po.execute_topk([blob], [1], [1.0], 10)
    assert total == 0 and len(hits) == 0
    # conjunction with empty term -> empty
    hits, total = po.execute_topk([blob], [0, 1], [1.0, 1.0], 10,
                                  min_match=2)
    assert total == 0 and len(hits) == 0


def test_boost_zero_scores_rejected():
    """boost 0 -> score 0 -> not accepted (threshold FLT_MIN,
    doc_collector.hpp:58) but still counted as a match (TotalMatches)."""
    doc_count = 100
    docs = np.arange(1, 51, dtype=np.uint32)
    freqs = np.ones(50, dtype=np.uint32)
    blob = sa.build_segment(doc_count, [(docs, freqs)], None)
    hits, total = po.execute_topk([blob], [0], [0.0], 10)
    assert total == 50
    assert len(hits) == 0


def test_multi_segment_stats_merge():
    """Cross-segment BM25 stats must be merged BEFORE scoring (PrepareCollector
    Finish / PreparePhase, duckdb_search_full_scan.cpp:1359-1384): two
    segments == one concatenated segment with the same global stats."""
    seed, n1, n2 = 21, 20_000, 30_000
    sels = [0.05, 0.02]
    b1 = sa.build_synth_segment(seed, 1, n1, sels)
    b2 = sa.build_synth_segment(seed, n1 + 1, n1 + n2, sels)
    full = sa.build_synth_segment(seed, 1, n1 + n2, sels)
    hits, total = po.execute_topk([b1, b2], [0, 1], [1.0, 1.0], 100)
    fhits, ftotal = po.execute_topk([full], [0, 1], [1.0, 1.0], 100)
    assert total == ftotal
    # map (seg, local doc) -> global doc
    got = [int(h["doc"]) + (n1 if h["segment"] == 1 else 0) for h in hits]
    np.testing.assert_array_equal(got, fhits["doc"])
    np.testing.assert_array_equal(hits["score"], fhits["score"])


def test_hybrid_vs_brute():
    """BM25 top-k AND col BETWEEN + per-bucket COUNT/SUM (configs[3]
    semantics: TableFilterDocIterator + aggregate consumer)."""
    doc_count = 30_000
    sels = [0.1, 0.05, 0.02]
    seed = 51
    blob, postings, norms = synth_corpus(seed, doc_count, sels)
    rng = np.random.default_rng(45)
    col = rng.integers(0, 1 << 31, doc_count + 1).astype(np.int64)
    span = 1 << 31
    flo, fhi = int(span * 0.4), int(span * 0.6) - 1  # 20% selectivity
    nbuckets = 64
    k = 100
    hits, total, bcnt, bsum = po.execute_topk_hybrid(
        blob, [0, 1, 2], [1.0] * 3, k, col, flo, fhi, nbuckets)
    # brute force
    order, scores, _ = brute_topk(postings, norms, doc_count, sels, 10**9)
    match = np.zeros(doc_count + 1, dtype=bool)
    for docs, _f in postings:
        match[docs] = True
    docs_all = np.nonzero(match)[0]
    passing = docs_all[(col[docs_all] >= flo) & (col[docs_all] <= fhi)]
    assert total == len(passing)
    exp_order = sorted(passing, key=lambda d: (-float(scores[d]), d))[:k]
    assert [int(h["doc"]) for h in hits] == [int(d) for d in exp_order]
    # buckets
    w = (fhi - flo + 1)
    bks = ((col[passing] - flo) * nbuckets // w).astype(np.int64)
    bks = np.minimum(bks, nbuckets - 1)
    exp_cnt = np.bincount(bks, minlength=nbuckets)
    exp_sum = np.zeros(nbuckets, dtype=np.int64)   # exact: integer adds
    np.add.at(exp_sum, bks, col[passing])
    np.testing.assert_array_equal(bcnt, exp_cnt)
    np.testing.assert_array_equal(bsum, exp_sum)


def test_match_docs_streaming():
    """Streaming emission (RunStreamingScan/HitBatcher analogue): every
    matching doc ascending + gathered column values."""
    doc_count = 25_000
    blob, postings, _ = synth_corpus(61, doc_count, [0.05, 0.02])
    col = np.random.default_rng(3).integers(0, 1000, doc_count + 1
                                            ).astype(np.int64)
    docs, vals, total = po.execute_match_docs(blob, [0, 1], [1.0, 1.0],
                                              doc_count, col=col)
    exp = np.union1d(postings[0][0], postings[1][0])
    assert total == len(exp)
    np.testing.assert_array_equal(docs, exp)
    np.testing.assert_array_equal(vals, col[exp])


def test_scan_agg_mt_equals_single():
    rng = np.random.default_rng(71)
    rows, ngroups = 500_000, 64
    keys = rng.integers(0, ngroups, rows).astype(np.int64)
    v1 = rng.integers(0, 1 << 20, rows).astype(np.int64)
    v2 = rng.normal(0, 1, rows).astype(np.float32)
    c1, s1, f1, p1 = po.scan_agg(keys, v1, v2, ngroups, pred_op=1,
                                 lo=100000)
    c2, s2, f2, p2 = po.scan_agg_mt(keys, v1, v2, ngroups, pred_op=1,
                                    lo=100000, nthreads=4, iters=2)
    assert p1 == p2
    np.testing.assert_array_equal(c1, c2)
    np.testing.assert_array_equal(s1, s2)
    np.testing.assert_allclose(f1, f2, rtol=1e-12)


def test_config1_cpu_plumbing():
    """BASELINE configs[0]: BM25 top-10, 2-term OR, 1M-doc synthetic
    segment, CPU oracle only (seed 42, selectivities 5%/2%, geometric
    freqs, lognormal norms — SURVEY.md §8d). Pins the oracle end to end at
    the named shape: exact vs mechanics vs brute force."""
    doc_count = 1_000_000
    sels = [0.05, 0.02]
    seed = 42
    blob, postings, norms = synth_corpus(seed, doc_count, sels)
    hits, total = po.execute_topk([blob], [0, 1], [1.0, 1.0], 10)
    mhits, mtotal = po.execute_topk_mech([blob], [0, 1], [1.0, 1.0], 10)
    assert total == mtotal
    np.testing.assert_array_equal(hits["doc"], mhits["doc"][:len(hits)])
    order, scores, nmatch = brute_topk(postings, norms, doc_count, sels, 10)
    assert total == nmatch
    assert [int(h["doc"]) for h in hits] == [int(d) for d in order]
    for h in hits:
        assert h["score"] == scores[int(h["doc"])]
