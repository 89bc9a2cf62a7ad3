"""Every GPU top-k path on the codec-matrix segment (tests/codec_matrix.py):
every postings block family, every bit width of the packed extract, tails,
window straddles, fused next to non-fused blocks. One function per path so a
failure names the path. The expected values are the numpy fp32 scorer over
the raw arrays (bit-exact: doc ids, score bits, totals), with the CPU oracle
as a second witness; tests/test_codec_matrix.py proves those two agree and
that the corpus covers what it claims.

Also WAND exactness beyond four terms: on the matrix (where spiky freqs make
blocks really prune) and on 8-, 20- and 32-term synthetic plans."""

import numpy as np
import pytest

import codec_matrix as cm
import serenedb_amd as sa
from oracle import pyoracle as po

pytestmark = pytest.mark.gpu

GPU_SCORERS = ("bm25", "tfidf_norm")


@pytest.fixture(scope="module")
def m():
    return cm.matrix()


@pytest.fixture(scope="module")
def ctx():
    c = sa.GpuContext(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def seg(ctx, m):
    return ctx.load_segment(m.blob)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def check_plan(ctx, seg, m, terms, boosts, k, scorer, min_match=1,
               label="", **kw):
    """one GPU query == the numpy fp32 reference == the oracle"""
    hits, total = ctx.execute_topk([seg], terms, boosts, k, scorer=scorer,
                                   min_match=min_match, **kw)
    rd, rs, rtotal = m.ref_topk(terms, boosts, k, scorer, min_match)
    what = f"{label} scorer={scorer} k={k} mm={min_match}"
    assert total == rtotal, what
    np.testing.assert_array_equal(hits["doc"], rd, err_msg=what)
    np.testing.assert_array_equal(bits(hits["score"]), bits(rs),
                                  err_msg=what)
    od, os_, ototal = m.oracle_topk(terms, boosts, k, scorer, min_match)
    assert total == ototal, what
    np.testing.assert_array_equal(hits["doc"], od, err_msg=what)
    np.testing.assert_array_equal(bits(hits["score"]), bits(os_),
                                  err_msg=what)
    return hits


def n_matches(m, terms, min_match=1):
    """match count by set arithmetic on the raw doc arrays"""
    _, c = np.unique(np.concatenate([m.postings[t][0] for t in terms]),
                     return_counts=True)
    return int((c >= min_match).sum())


def run_groups(ctx, seg, m, scorer):
    for gi, (name, g) in enumerate(m.groups.items()):
        boosts = cm.group_boosts(len(g), gi)
        for k in (n_matches(m, g), 10, 1):
            check_plan(ctx, seg, m, g, boosts, k, scorer, label=name)


def test_decode_term(ctx, seg, m):
    for t, (docs, freqs) in enumerate(m.postings):
        ddocs, dfreqs = ctx.decode_term(seg, t, len(docs))
        np.testing.assert_array_equal(ddocs, docs, err_msg=m.names[t])
        np.testing.assert_array_equal(dfreqs, freqs, err_msg=m.names[t])


@pytest.mark.parametrize("scorer", GPU_SCORERS + ("tfidf",))
def test_sweep_single_terms(ctx, seg, m, scorer):
    """default path, every term alone with k = df + 1: the hits are the
    complete decoded posting list with its scores, total == df"""
    for t, (docs, _) in enumerate(m.postings):
        hits = check_plan(ctx, seg, m, [t], [1.0], len(docs) + 1, scorer,
                          label=m.names[t])
        assert len(hits) <= len(docs)


@pytest.mark.parametrize("scorer", GPU_SCORERS)
def test_sweep_groups(ctx, seg, m, scorer):
    run_groups(ctx, seg, m, scorer)


@pytest.mark.parametrize("scorer", GPU_SCORERS)
def test_general_kernel_groups(ctx, seg, m, scorer, monkeypatch):
    """plain OR plans through topk_window_kernel"""
    monkeypatch.setenv("SDB_TOPK_PATH", "general")
    run_groups(ctx, seg, m, scorer)


def test_general_kernel_minmatch_count_matchdocs(ctx, seg, m, monkeypatch):
    g = m.groups["freq_widths"]      # terms that share low docs
    ones = [1.0] * len(g)
    u, c = np.unique(np.concatenate([m.postings[t][0] for t in g]),
                     return_counts=True)
    assert (c >= 2).sum() > 1000     # the plan really overlaps
    for path in (None, "general"):
        if path:
            monkeypatch.setenv("SDB_TOPK_PATH", path)
        for scorer in GPU_SCORERS:
            check_plan(ctx, seg, m, g, ones, 500, scorer, min_match=2,
                       label="freq_widths")
        for mm in (1, 2, 5):
            assert ctx.execute_count([seg], g, ones, min_match=mm) == \
                int((c >= mm).sum()), mm
            docs, _, total = ctx.execute_match_docs(seg, g, ones, len(u) + 8,
                                                    min_match=mm)
            assert total == int((c >= mm).sum())
            np.testing.assert_array_equal(docs, u[c >= mm])
    # every other group: counts and streamed docs of the plain OR
    for name, g in m.groups.items():
        u = np.unique(np.concatenate([m.postings[t][0] for t in g]))
        ones = [1.0] * len(g)
        assert ctx.execute_count([seg], g, ones) == len(u), name
        docs, _, total = ctx.execute_match_docs(seg, g, ones, len(u) + 8)
        assert total == len(u), name
        np.testing.assert_array_equal(docs, u, err_msg=name)


@pytest.mark.parametrize("scorer", GPU_SCORERS)
def test_wave_kernel_small_groups(ctx, seg, m, scorer, monkeypatch):
    monkeypatch.setenv("SDB_TOPK_PATH", "wave")
    for name, g in m.small_groups.items():
        for k in (n_matches(m, g), 10):
            check_plan(ctx, seg, m, g, [1.0] * 4, k, scorer, label=name)


@pytest.mark.parametrize("geom", ["4096x256", "32768x512"])
def test_sweep_geometries(ctx, seg, m, geom, monkeypatch):
    monkeypatch.setenv("SDB_SWEEP_GEOM", geom)
    for name in ("mixed", "overlap"):
        g = m.small_groups[name]
        for scorer in GPU_SCORERS:
            for k in (n_matches(m, g), 10):
                check_plan(ctx, seg, m, g, [1.0] * 4, k, scorer,
                           label=f"{geom} {name}")


def test_batch_equals_single(ctx, seg, m):
    g = m.groups["families"]
    boosts = cm.group_boosts(len(g), 3)
    k = 777
    single = check_plan(ctx, seg, m, g, boosts, k, "bm25", label="families")
    total = n_matches(m, g)
    batch, btotals = ctx.execute_topk_batch([seg], g, boosts, k, 2,
                                            all_hits=True)
    assert btotals == [total] * 2
    for q in range(2):
        np.testing.assert_array_equal(batch[q]["doc"], single["doc"])
        np.testing.assert_array_equal(bits(batch[q]["score"]),
                                      bits(single["score"]))


# ---------------------------------------------------------------------------
# WAND exactness beyond four terms
# ---------------------------------------------------------------------------

def check_wand(ctx, segs, terms, boosts, k, expect, label="", **kw):
    """wand=True returns the identical hits as wand=False and as `expect`
    (docs, scores); returns (visited, total)."""
    base, total = ctx.execute_topk(segs, terms, boosts, k, **kw)
    wand, visited = ctx.execute_topk(segs, terms, boosts, k, wand=True, **kw)
    what = f"{label} k={k} {kw}"
    for got in (base, wand):
        np.testing.assert_array_equal(got["doc"], expect[0], err_msg=what)
        np.testing.assert_array_equal(bits(got["score"]), bits(expect[1]),
                                      err_msg=what)
    np.testing.assert_array_equal(wand["segment"], base["segment"])
    assert visited <= total, what
    return visited, total


@pytest.mark.parametrize("path", ["default", "general"])
def test_wand_matrix(ctx, seg, m, path, monkeypatch):
    """The pinned freq spikes make blocks really prune; the 32-term "wide"
    plan has every term bounding every window."""
    if path != "default":
        monkeypatch.setenv("SDB_TOPK_PATH", path)
    for gi, (name, g) in enumerate(m.groups.items()):
        boosts = cm.group_boosts(len(g), gi)
        for scorer in GPU_SCORERS:
            for k in (1, 10) + ((1000,) if name == "wide" else ()):
                rd, rs, _ = m.ref_topk(g, boosts, k, scorer)
                v, t = check_wand(ctx, [seg], g, boosts, k, (rd, rs),
                                  label=f"{path} {name}", scorer=scorer)
                print(f"wand {path} {name} {scorer} k={k}: "
                      f"visited {v} of {t}")
    # one long spiky term, k = 1: every workgroup's first window holds a
    # spike doc, so from its third window on (the second derives from the
    # first's merged histogram) all-freq-1 blocks fall below the threshold
    t_spiky = [m.idx["spiky"]]
    for scorer in GPU_SCORERS:
        rd, rs, _ = m.ref_topk(t_spiky, [1.0], 1, scorer)
        v, t = check_wand(ctx, [seg], t_spiky, [1.0], 1, (rd, rs),
                          label=f"{path} spiky", scorer=scorer)
        print(f"wand {path} spiky {scorer} k=1: visited {v} of {t}")
        assert t == len(m.postings[t_spiky[0]][0])
        assert v < t, (path, scorer, v, t)   # pruning actually fired


@pytest.mark.parametrize("path", ["default", "general"])
def test_wand_bin_edge(ctx, seg, m, path, monkeypatch):
    """The "edge" term (codec_matrix._build): doc A locks the k = 1
    threshold at a bin whose float floor is A's score; doc B, two windows
    later in the same workgroup, scores one ulp more and its block's bound
    is exactly its score. B must survive the bound test and come back as
    the top hit, while the block of low scores next to it is pruned."""
    if path != "default":
        monkeypatch.setenv("SDB_TOPK_PATH", path)
    t = [m.idx["edge"]]
    a, b = m.edge_docs
    for k in (1, 2):
        rd, rs, _ = m.ref_topk(t, [1.0], k, "bm25")
        assert [int(d) for d in rd] == [b, a][:k]
        v, total = check_wand(ctx, [seg], t, [1.0], k, (rd, rs),
                              label=f"{path} edge")
        print(f"wand {path} edge k={k}: visited {v} of {total}")
        assert total == 3 * cm.BLOCK
        if k == 1:
            assert v < total, (path, v, total)


@pytest.fixture(scope="module")
def wide_corpus():
    """300 000 docs, 32 terms (the shape test_wide_plans uses)."""
    rng = np.random.default_rng(171)
    doc_count = 300_000
    sels = [float(s) for s in rng.uniform(0.003, 0.04, 32)]
    postings = [sa.synth_postings(172, doc_count, t, s)
                for t, s in enumerate(sels)]
    norms = sa.synth_norms(172, doc_count)
    blob = sa.build_segment(doc_count, postings, norms)
    boosts = [float(b) for b in rng.uniform(0.25, 4.0, 32)]
    return blob, doc_count, sels, boosts


def oracle_expect(blobs, terms, boosts, k, **kw):
    oh, _ = po.execute_topk(blobs, terms, boosts, k, **kw)
    return oh["doc"], oh["score"]


@pytest.mark.parametrize("nterms", [8, 20, 32])
def test_wand_wide_plans(ctx, wide_corpus, nterms):
    blob, _, _, boosts = wide_corpus
    s = ctx.load_segment(blob)
    terms = list(range(nterms))
    for scorer in GPU_SCORERS:
        for k in (1, 10, 1000):
            exp = oracle_expect([blob], terms, boosts[:nterms], k,
                                scorer=scorer)
            check_wand(ctx, [s], terms, boosts[:nterms], k, exp,
                       label=f"{nterms} terms", scorer=scorer)


def test_wand_wide_plan_livemask_boost_multiseg(ctx, wide_corpus):
    blob, doc_count, sels, boosts = wide_corpus
    terms = list(range(32))
    rng = np.random.default_rng(173)
    # live mask (~25% deleted)
    s = ctx.load_segment(blob)
    nwords = (doc_count + 64) // 64
    mask = rng.integers(0, 1 << 64, nwords, dtype=np.uint64)
    mask |= rng.integers(0, 1 << 64, nwords, dtype=np.uint64)
    ctx.attach_livemask(s, mask)
    for k in (1, 10, 1000):
        exp = oracle_expect([blob], terms, boosts, k, live_mask=mask)
        check_wand(ctx, [s], terms, boosts, k, exp, label="live mask")
    ctx.attach_livemask(s, None)
    # per-doc filter boost
    fb = rng.uniform(0.5, 2.0, doc_count + 1).astype(np.float32)
    fb[0] = 0.0
    ctx.attach_boost(s, fb)
    for k in (1, 10, 1000):
        exp = oracle_expect([blob], terms, boosts, k, filter_boost=fb)
        check_wand(ctx, [s], terms, boosts, k, exp, label="filter boost",
                   filter_boost=True)
    # two segments (stats merge across them)
    n2 = 200_000
    postings2 = [sa.synth_postings(174, n2, t, sel)
                 for t, sel in enumerate(sels)]
    blob2 = sa.build_segment(n2, postings2, sa.synth_norms(174, n2))
    s1, s2 = ctx.load_segment(blob), ctx.load_segment(blob2)
    for scorer in GPU_SCORERS:
        for k in (1, 10, 1000):
            oh, _ = po.execute_topk([blob, blob2], terms, boosts, k,
                                    scorer=scorer)
            base, _ = ctx.execute_topk([s1, s2], terms, boosts, k,
                                       scorer=scorer)
            np.testing.assert_array_equal(base["segment"], oh["segment"])
            check_wand(ctx, [s1, s2], terms, boosts, k,
                       (oh["doc"], oh["score"]), label="two segments",
                       scorer=scorer)
