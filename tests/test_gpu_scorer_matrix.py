"""Every GPU top-k path on the scorer-matrix segments (tests/
scorer_matrix.py): scorer, k1/b, term boosts, the per-doc filter boost,
injected global stats, the live mask and the score > FLT_MIN acceptance
rule. One function per path so a failure names the path; every function
runs every case its path takes. The expected values are the numpy fp32
scorer over the raw arrays (bit-exact: segment ids, doc ids, score bits,
out_count, total), with the CPU oracle as a further witness where it can run
the case; tests/test_scorer_matrix.py proves those agree and that the corpus
covers what it claims.

Also the plan contract (include/sdb_gpu.h, SdbQueryPlan): plans the library
cannot answer correctly are SDB_ERR_INVALID on every entry."""

import ctypes as C

import numpy as np
import pytest

import scorer_matrix as sm
import serenedb_amd as sa

pytestmark = pytest.mark.gpu

SDB_ERR_INVALID = -1


@pytest.fixture(scope="module")
def m():
    return sm.matrix()


@pytest.fixture(scope="module")
def ctx():
    c = sa.GpuContext(0)
    yield c
    c.close()


class Dev:
    """the two resident segments and what is attached to them"""

    def __init__(self, ctx, m):
        self.ctx, self.m = ctx, m
        self.segs = [ctx.load_segment(s.blob) for s in m.segs]
        self.fb = [None, None]
        self.live = [False, False]

    def prepare(self, c):
        """attach the case's filter-boost columns and live mask; returns
        (segment handles, the scoring keywords of the wrapper)"""
        for si in range(c["nseg"]):
            want = c["fb"][si] if c["fb"] else None
            if want is not None and self.fb[si] != want:
                self.ctx.attach_boost(self.segs[si], self.m.segs[si].fb[want])
                self.fb[si] = want
            if self.live[si] != c["live"]:
                self.ctx.attach_livemask(
                    self.segs[si],
                    self.m.segs[si].live_words if c["live"] else None)
                self.live[si] = c["live"]
        kw = dict(min_match=c["mm"], k1=c["k1"], b=c["b"],
                  global_stats=c["gstats"], scorer=c["scorer"],
                  filter_boost=c["fb"] is not None)
        return self.segs[:c["nseg"]], kw


@pytest.fixture(scope="module")
def dev(ctx, m):
    return Dev(ctx, m)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def check(m, name, k, hits, total, label="", check_total=True):
    """one GPU answer == the numpy fp32 reference == the oracle"""
    what = f"{label} {name} k={k}"
    witnesses = [m.ref_topk(name, k)]
    if m.cases[name]["oracle"]:
        witnesses.append(m.oracle_topk(name, k))
    for sg, d, s, wtotal in witnesses:
        if check_total:
            assert total == wtotal, what
        assert len(hits) == len(d), what          # out_count
        np.testing.assert_array_equal(hits["segment"], sg, err_msg=what)
        np.testing.assert_array_equal(hits["doc"], d, err_msg=what)
        np.testing.assert_array_equal(bits(hits["score"]), bits(s),
                                      err_msg=what)


def run_single(ctx, dev, m, label, names=None):
    n = 0
    for name, c in m.cases.items():
        if names is not None and name not in names:
            continue
        segs, kw = dev.prepare(c)
        for k in c["ks"]:
            hits, total = ctx.execute_topk(segs, c["terms"], c["boosts"], k,
                                           **kw)
            check(m, name, k, hits, total, label)
            n += 1
    return n


# ---------------------------------------------------------------------------
# one function per path
# ---------------------------------------------------------------------------

def test_default_sweep(ctx, dev, m):
    assert run_single(ctx, dev, m, "sweep") > 150


def test_sweep_geometry_4096x256(ctx, dev, m, monkeypatch):
    monkeypatch.setenv("SDB_SWEEP_GEOM", "4096x256")
    run_single(ctx, dev, m, "sweep 4096x256")


def test_general_kernel(ctx, dev, m, monkeypatch):
    monkeypatch.setenv("SDB_TOPK_PATH", "general")
    run_single(ctx, dev, m, "general")


def test_wave_kernel(ctx, dev, m, monkeypatch):
    """every plan has at most four terms, so the per-wave kernel takes
    every min_match 1 case (the others it hands to the general kernel)"""
    monkeypatch.setenv("SDB_TOPK_PATH", "wave")
    run_single(ctx, dev, m, "wave")


def test_batch(ctx, dev, m):
    """execute_topk_batch, nq = 2: both queries equal the single entry and
    the reference"""
    for name, c in m.cases.items():
        segs, kw = dev.prepare(c)
        for k in c["ks"]:
            single, stotal = ctx.execute_topk(segs, c["terms"], c["boosts"],
                                              k, **kw)
            batch, totals = ctx.execute_topk_batch(
                segs, c["terms"], c["boosts"], k, 2, all_hits=True, **kw)
            for q in range(2):
                check(m, name, k, batch[q], totals[q], f"batch q{q}")
                assert totals[q] == stotal
                np.testing.assert_array_equal(batch[q]["doc"], single["doc"])
                np.testing.assert_array_equal(batch[q]["segment"],
                                              single["segment"])
                np.testing.assert_array_equal(bits(batch[q]["score"]),
                                              bits(single["score"]))


def test_batch_carry_over(ctx, dev, m):
    """two different plans back to back on one context, in both orders: a
    query-state slot that kept the previous plan's nc, nl, fb or scorer
    would answer the second with the first's arithmetic"""
    a, b = "fb_bm15_mm1", "tfidf_mm1"
    for order in ((a, b), (b, a)):
        for name in order:
            c = m.cases[name]
            segs, kw = dev.prepare(c)
            for k in (10, c["ks"][-1]):
                batch, totals = ctx.execute_topk_batch(
                    segs, c["terms"], c["boosts"], k, 2, all_hits=True, **kw)
                for q in range(2):
                    check(m, name, k, batch[q], totals[q],
                          f"carry-over {order} q{q}")


@pytest.mark.parametrize("path", ["default", "general"])
def test_wand(ctx, dev, m, path, monkeypatch):
    """wand=True returns the hits of wand=False and of the reference for
    every min_match 1 case; where no score passes FLT_MIN no threshold ever
    forms, so every match is visited"""
    if path != "default":
        monkeypatch.setenv("SDB_TOPK_PATH", path)
    n = 0
    for name, c in m.cases.items():
        if c["mm"] != 1:
            continue
        segs, kw = dev.prepare(c)
        for k in c["ks"]:
            base, total = ctx.execute_topk(segs, c["terms"], c["boosts"], k,
                                           **kw)
            wand, visited = ctx.execute_topk(segs, c["terms"], c["boosts"],
                                             k, wand=True, **kw)
            check(m, name, k, base, total, f"{path} wand off")
            check(m, name, k, wand, visited, f"{path} wand on",
                  check_total=False)
            assert visited <= total, (path, name, k)
            if name == "all_zero" or name.startswith("bm1_"):
                assert len(wand) == 0 and visited == total, (path, name, k)
            n += 1
    assert n > 50


def test_count_and_match_docs(ctx, dev, m):
    """execute_count and execute_match_docs equal set arithmetic on the raw
    doc arrays under every k1/b, scorer, boost, stats and filter-boost
    column of the matrix: scoring knobs must not change what matches"""
    for name, c in m.cases.items():
        segs, kw = dev.prepare(c)
        want = m.match_docs(name)
        n = sum(len(u) for u in want)
        assert ctx.execute_count(segs, c["terms"], c["boosts"], **kw) == n, \
            name
        for seg, u in zip(segs, want):
            docs, _, total = ctx.execute_match_docs(
                seg, c["terms"], c["boosts"], len(u) + 8, **kw)
            assert total == len(u), name
            np.testing.assert_array_equal(docs, u, err_msg=name)


# ---------------------------------------------------------------------------
# the plan contract
# ---------------------------------------------------------------------------

class Entries:
    """the four plan-taking entries through ctypes: the return code is the
    thing under test"""

    def __init__(self, ctx):
        self.ctx, self.lib, self.k = ctx, ctx._lib, 10
        self.hits = (sa.SdbScoreDoc * (2 * self.k))()
        self.docs = np.zeros(64, dtype=np.uint32)

    def rcs(self, segs, plan):
        lib, c, k = self.lib, self.ctx._ctx, self.k
        arr = (C.c_void_p * len(segs))(*[C.c_void_p(s.value) for s in segs])
        n, tot, out_n = C.c_uint32(0), C.c_uint64(0), C.c_uint64(0)
        counts, totals = (C.c_uint32 * 2)(), (C.c_uint64 * 2)()
        out = {}
        out["topk"] = lib.sdb_gpu_execute_topk(
            c, arr, C.c_uint32(len(segs)), C.byref(plan), C.c_uint32(k),
            self.hits, C.byref(n), C.byref(tot))
        out["batch"] = lib.sdb_gpu_execute_topk_batch(
            c, arr, C.c_uint32(len(segs)), C.byref(plan), C.c_uint32(k),
            C.c_uint32(2), self.hits, counts, totals)
        out["count"] = lib.sdb_gpu_execute_count(
            c, arr, C.c_uint32(len(segs)), C.byref(plan), C.byref(tot))
        for i, s in enumerate(segs):
            out[f"match_docs[{i}]"] = lib.sdb_gpu_execute_match_docs(
                c, s, C.byref(plan),
                self.docs.ctypes.data_as(C.POINTER(C.c_uint32)), None,
                C.c_uint64(len(self.docs)), C.byref(out_n), C.byref(tot))
        return out


def make_plan(ctx, m, boosts=(1.0, 1.0, 1.0), k1=1.2, b=0.75, gstats=None,
              scorer="bm25", fb=False, raw_scorer=None):
    """a plan over the three terms of the parameter cases"""
    p = ctx._make_plan(m.cases["bm25_mm1"]["terms"], list(boosts), 1, k1, b,
                       gstats, scorer, False, fb)
    if raw_scorer is not None:
        p.scorer = raw_scorer
    return p


def bad_plans(ctx, m):
    """name -> a plan outside the contract"""
    inf, nan = float("inf"), float("nan")

    def plan(**kw):
        return make_plan(ctx, m, **kw)

    bad = {
        "scorer 3": plan(raw_scorer=3),
        "scorer 2^32-1": plan(raw_scorer=0xFFFFFFFF),
        "k1 NaN": plan(k1=nan),
        "k1 inf": plan(k1=inf),
        "k1 negative": plan(k1=-1.0),
        "b NaN": plan(b=nan),
        "b negative": plan(b=-0.25),
        "b above 1": plan(b=1.5),
        "b inf": plan(b=inf),
        "boost inf": plan(boosts=[1.0, inf, 1.0]),
        "boost NaN": plan(boosts=[1.0, nan, 1.0]),
        "boost negative": plan(boosts=[1.0, -1.0, 1.0]),
        # num = boost * (k1 + 1) * idf overflows
        "boost 3e38, bm25": plan(boosts=[1.0, 3e38, 1.0]),
        # num is finite (1.4e34), the bound num * sqrt(max_freq) is not:
        # the dense term's largest freq is 2^32 - 1
        "boost 1e34, tfidf": plan(boosts=[1e34, 1.0, 1.0], scorer="tfidf"),
        "dwt above dwf": plan(gstats=(1000, 10**6, [10, 1001, 10])),
        "dwt above dwf, tfidf": plan(gstats=(1000, 10**6, [10, 10, 2000]),
                                     scorer="tfidf"),
    }
    null_dwt = plan()
    null_dwt.g_docs_with_field = 1000
    null_dwt.g_total_term_freq = 10**6
    bad["dwf set, dwt NULL"] = null_dwt
    return bad


def test_plan_contract(ctx, dev, m):
    """Plans the library cannot answer correctly return SDB_ERR_INVALID from
    every entry, and the context stays usable: a valid query right after
    each still matches the reference."""
    e = Entries(ctx)
    inf, nan = float("inf"), float("nan")
    seg0 = dev.segs[:1]

    def plan(**kw):
        return make_plan(ctx, m, **kw)

    def still_usable():
        c = m.cases["bm25_mm1"]
        segs, kw = dev.prepare(c)
        hits, total = ctx.execute_topk(segs, c["terms"], c["boosts"], 10,
                                       **kw)
        check(m, "bm25_mm1", 10, hits, total, "after a rejected plan")

    def rejected(what, segs, p, only=None):
        rcs = e.rcs(segs, p)
        for entry, rc in rcs.items():
            if only is None or entry in only:
                assert rc == SDB_ERR_INVALID, (what, entry, rc)
        still_usable()

    # the same calls accept a valid plan
    dev.prepare(m.cases["fb_bm25_mm1"])
    for p in (plan(), plan(fb=True), plan(scorer="tfidf_norm", k1=0.0, b=1.0),
              plan(gstats=(10**6, 10**9, [10**6, 1, 0]))):
        assert set(e.rcs(seg0, p).values()) == {0}

    for what, p in bad_plans(ctx, m).items():
        rejected(what, seg0, p)
        rejected(what + ", two segments", dev.segs, p)

    # ---- filter boost: fresh segments, so that one really has no column
    small = m.segs[1]
    with_col = ctx.load_segment(small.blob)
    without = ctx.load_segment(small.blob)
    ctx.attach_boost(with_col, small.fb["ladder"])
    p = plan(fb=True)
    assert set(e.rcs([with_col], p).values()) == {0}
    rejected("column missing on segment 1", [with_col, without], p,
             only=("topk", "batch", "count", "match_docs[1]"))
    rejected("column missing on segment 0", [without, with_col], p,
             only=("topk", "batch", "count", "match_docs[0]"))
    zeros = np.zeros(sm.DOC_COUNT2 + 1, dtype=np.float32)
    ctx.attach_boost(without, zeros)
    rejected("all-zero column", [without], p)
    # a bad column is refused at attach and the old one stays in place
    lib, fp = ctx._lib, C.POINTER(C.c_float)
    for what, v in (("inf", inf), ("NaN", nan), ("negative", -1.0),
                    ("-inf", -inf)):
        col = small.fb["ladder"].copy()
        col[sm.DOC_COUNT2 // 2] = v
        assert lib.sdb_gpu_segment_attach_boost(
            ctx._ctx, with_col, col.ctypes.data_as(fp)) == SDB_ERR_INVALID, \
            what
        col[sm.DOC_COUNT2 // 2] = 1.0
        col[sm.DOC_COUNT2] = v          # the last doc is checked too
        assert lib.sdb_gpu_segment_attach_boost(
            ctx._ctx, with_col, col.ctypes.data_as(fp)) == SDB_ERR_INVALID, \
            what
    assert set(e.rcs([with_col], p).values()) == {0}
    # a finite column maximum at which smax * fbmax overflows is accepted by
    # the attach (it knows no plan) and refused when the plan is prepared
    col = small.fb["ladder"].copy()
    col[7] = 3e38
    assert lib.sdb_gpu_segment_attach_boost(
        ctx._ctx, with_col, col.ctypes.data_as(fp)) == 0
    rejected("smax * fbmax overflows", [with_col], p)
    assert set(e.rcs([with_col], plan(boosts=[1e-3] * 3, fb=True))
               .values()) == {0}
