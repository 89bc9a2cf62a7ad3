"""Every GPU top-k entry over sets of segments (tests/segset_matrix.py): many,
tiny, empty and tied segments in one call. What is pinned here exists only
because a call takes segs[], nsegs: the 64-slot term-table ring of the
single and batch executors, the threshold, histogram, candidate and bucket
state every segment's launch accumulates into, the cross-segment order
(score desc, segment asc, doc asc) with segment = position in this call's
array, launches with nothing to do, per-segment masks, boost and filter
columns mixed within one call, and statistics merged over the set.

All comparisons are exact: doc, segment, score bits, out_count, total, bucket
counts and sums. The expected values are the numpy fp32 reference and the
plain-Python references over the raw arrays; tests/test_segset_matrix.py
proves them against the CPU oracle and proves that the cases tell the
plausible mistakes apart."""

import ctypes as C

import numpy as np
import pytest

import segset_matrix as ss
import serenedb_amd as sa

pytestmark = pytest.mark.gpu

SDB_ERR_INVALID = -1
BETWEEN = 3
PATHS = {
    "sweep": {},
    "sweep4096": {"SDB_SWEEP_GEOM": "4096x256"},
    "general": {"SDB_TOPK_PATH": "general"},
    "wave": {"SDB_TOPK_PATH": "wave"},
}


@pytest.fixture(scope="module")
def m():
    return ss.matrix()


@pytest.fixture(scope="module")
def ctx():
    c = sa.GpuContext(0)
    yield c
    c.close()


@pytest.fixture(autouse=True)
def clean_env(monkeypatch):
    monkeypatch.delenv("SDB_TOPK_PATH", raising=False)
    monkeypatch.delenv("SDB_SWEEP_GEOM", raising=False)


def use(monkeypatch, path):
    for k, v in PATHS[path].items():
        monkeypatch.setenv(k, v)


class Dev:
    """the resident segments of every set (one load per occurrence, except
    same_handle: one handle three times) and what is attached to each"""

    def __init__(self, ctx, m):
        self.ctx, self.m = ctx, m
        self.sets = {}
        self.state = {}     # handle value -> dict(bi, live, fb, col)

    def load(self, bi):
        h = self.ctx.load_segment(self.m.blobs[bi].blob)
        self.state[h.value] = dict(bi=bi, live=False, fb=None, col=False)
        return h

    def handles(self, set_):
        if set_ not in self.sets:
            bis = ss.SETS[set_]
            if set_ == "same_handle":
                h = self.load(bis[0])
                self.sets[set_] = [h] * len(bis)
            else:
                self.sets[set_] = [self.load(bi) for bi in bis]
        return self.sets[set_]

    def prepare(self, c, col=False):
        """attach what the case names to each of its segments (live masks
        on the blobs of MASKED only, the others stay bare), detach what it
        does not; returns (handles, the wrapper's keywords)"""
        segs = self.handles(c["set"])
        for h in segs:
            st = self.state[h.value]
            blob = self.m.blobs[st["bi"]]
            want = bool(c["masked"] and blob.masked)
            if st["live"] != want:
                self.ctx.attach_livemask(h, blob.live_words if want else None)
                st["live"] = want
            if c["fb"] is not None and st["fb"] != c["fb"]:
                self.ctx.attach_boost(h, blob.fb[c["fb"]])
                st["fb"] = c["fb"]
            if col and not st["col"]:
                self.ctx.attach_column(h, blob.col)
                st["col"] = True
        kw = dict(min_match=c["mm"], k1=c["k1"], b=c["b"],
                  global_stats=c["gstats"])
        return segs, kw

    def score_kw(self, c):
        return dict(scorer=c["scorer"], filter_boost=c["fb"] is not None)


@pytest.fixture(scope="module")
def dev(ctx, m):
    return Dev(ctx, m)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def check(m, c, k, hits, total, label="", check_total=True):
    what = f"{label} {c['name']} k={k}"
    sg, d, s, wtotal = m.ref_topk(c, k)
    if check_total:
        assert total == wtotal, what
    assert len(hits) == len(d), what          # out_count
    np.testing.assert_array_equal(hits["segment"], sg, err_msg=what)
    np.testing.assert_array_equal(hits["doc"], d, err_msg=what)
    np.testing.assert_array_equal(bits(hits["score"]), bits(s), err_msg=what)


def run_single(ctx, dev, m, names, label, ks=None, max_terms=None):
    n = 0
    for name in names:
        c = m.cases[name]
        if max_terms and len(c["terms"]) > max_terms:
            continue
        segs, kw = dev.prepare(c)
        for k in ks or c["ks"]:
            hits, total = ctx.execute_topk(segs, c["terms"], c["boosts"], k,
                                           **kw, **dev.score_kw(c))
            check(m, c, k, hits, total, label)
            n += 1
    return n


def run_batch(ctx, dev, m, names, label, nq=2, ks=None):
    """every query of the batch equals the reference and the single entry"""
    for name in names:
        c = m.cases[name]
        segs, kw = dev.prepare(c)
        for k in ks or c["ks"]:
            single, stotal = ctx.execute_topk(
                segs, c["terms"], c["boosts"], k, **kw, **dev.score_kw(c))
            batch, totals = ctx.execute_topk_batch(
                segs, c["terms"], c["boosts"], k, nq, all_hits=True, **kw,
                **dev.score_kw(c))
            check(m, c, k, single, stotal, f"{label} single")
            for q in range(nq):
                check(m, c, k, batch[q], totals[q], f"{label} q{q}/{nq}")


# ---------------------------------------------------------------------------
# orders and k edges
# ---------------------------------------------------------------------------

ORDER_CASES = [f"{s}_{v}" for s in ("asc", "desc", "spike_first",
                                    "spike_last")
               for v in ("or", "mm2", "and", "wide")]


@pytest.mark.parametrize("path", list(PATHS))
def test_orders_and_k_edges(ctx, dev, m, path, monkeypatch):
    """all twelve segments by size, reversed, and with the segment that owns
    the whole top 10 first or last: the threshold a segment locks decides
    what every later one appends. OR, min_match 2, AND and the 32-term plan;
    the per-wave kernel takes plans of at most four terms."""
    use(monkeypatch, path)
    n = run_single(ctx, dev, m, ORDER_CASES, path,
                   max_terms=4 if path == "wave" else None)
    assert n >= 48


@pytest.mark.parametrize("path", ["sweep", "sweep4096", "general"])
def test_spike_first_candidate_count(ctx, dev, m, path, monkeypatch, capsys):
    """the twelve spikes of the first segment score bit-equal, so whatever
    bin the threshold locks holds all of them; how far below the matches the
    candidate count lands depends on when the histogram merges arrive"""
    use(monkeypatch, path)
    c = m.cases["spike_first_or"]
    segs, kw = dev.prepare(c)
    hits, total = ctx.execute_topk(segs, c["terms"], c["boosts"], 3, **kw)
    check(m, c, 3, hits, total, path)
    ncand = C.c_uint(0)
    ctx._lib.sdb_gpu_last_stats(ctx._ctx, None, C.byref(ncand), None, None,
                                None)
    with capsys.disabled():
        print(f"\nspike_first {path}: {ncand.value} candidates of {total} "
              f"matches, {len(ss.SPIKE_DOCS)} spikes")
    assert len(ss.SPIKE_DOCS) <= ncand.value <= total


# ---------------------------------------------------------------------------
# ties across segments
# ---------------------------------------------------------------------------

TIE_CASES = ["dups_tie", "dups_p2", "same_handle_tie", "same_handle_p2",
             "asc_tie"]


@pytest.mark.parametrize("path", ["sweep", "general", "wave"])
def test_ties_across_segments(ctx, dev, m, path, monkeypatch):
    """one blob three times (three loads, and one handle passed three
    times): every doc scores bit-equal in each copy, and k walks through the
    classes one entry at a time; the tie term over all twelve segments, k
    inside classes spread over six of them"""
    use(monkeypatch, path)
    assert run_single(ctx, dev, m, TIE_CASES, path) > 80


def test_ties_across_segments_batch(ctx, dev, m):
    run_batch(ctx, dev, m, TIE_CASES, "batch")


# ---------------------------------------------------------------------------
# hollow, tiny and empty
# ---------------------------------------------------------------------------

HOLLOW_CASES = ["hollow_first", "hollow_mid", "hollow_last", "all_hollow",
                "void", "void_in_or", "only_one_doc"]


@pytest.mark.parametrize("path", list(PATHS))
def test_hollow_tiny_and_empty(ctx, dev, m, path, monkeypatch):
    """a segment where every plan term has df == 0 (a launch with nothing to
    do) first, in the middle and last; a plan that is empty in every
    segment; a term that matches nothing, alone and inside an OR; a set of
    one 1-doc segment"""
    use(monkeypatch, path)
    run_single(ctx, dev, m, HOLLOW_CASES, path)
    c = m.cases["all_hollow"]
    segs, kw = dev.prepare(c)
    hits, total = ctx.execute_topk(segs, c["terms"], c["boosts"], 10, **kw)
    assert (len(hits), total) == (0, 0)


def test_hollow_tiny_and_empty_batch(ctx, dev, m):
    run_batch(ctx, dev, m, HOLLOW_CASES, "batch")


def test_no_segments(ctx, dev, m):
    """nsegs == 0 is SDB_OK with no hits and total 0 on the single, batch,
    count and hybrid entries (include/sdb_gpu.h)"""
    c = m.cases["empty"]
    hits, total = ctx.execute_topk([], c["terms"], c["boosts"], 10)
    assert (len(hits), total) == (0, 0)
    batch, totals = ctx.execute_topk_batch([], c["terms"], c["boosts"], 10,
                                           3, all_hits=True)
    assert [len(b) for b in batch] == [0, 0, 0] and totals == [0, 0, 0]
    assert ctx.execute_count([], c["terms"], c["boosts"]) == 0
    hits, total, bcnt, bsum = ctx.execute_topk_hybrid(
        [], c["terms"], c["boosts"], 10, -5, 5, 4)
    assert (len(hits), total) == (0, 0)
    assert not bcnt.any() and not bsum.any()
    hits, total, bcnt, bsum = ctx.execute_topk_hybrid_chain(
        [], c["terms"], c["boosts"], 10, [(0, BETWEEN, -5, 5)], 4)
    assert (len(hits), total) == (0, 0)
    assert not bcnt.any() and not bsum.any()
    batch, totals, bcnt, bsum = ctx.execute_topk_hybrid_batch(
        [], c["terms"], c["boosts"], 10, -5, 5, 4, 3, all_hits=True)
    assert [len(b) for b in batch] == [0, 0, 0] and totals == [0, 0, 0]
    assert not bcnt.any() and not bsum.any()
    # a filter_boost plan over no segments has no column maximum
    p = ctx._make_plan(c["terms"], c["boosts"], 1, 1.2, 0.75, None, "bm25",
                       False, True)
    assert set(rcs(ctx, [], p).values()) == {SDB_ERR_INVALID}
    # and the context answers the next call
    run_single(ctx, dev, m, ["only_one_doc"], "after nsegs == 0")


# ---------------------------------------------------------------------------
# more than 64 launches in one call
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("set_", ["s65", "s70", "s130"])
@pytest.mark.parametrize("path", ["sweep", "general"])
def test_more_than_64_segments(ctx, dev, m, path, set_, monkeypatch):
    """Segment s is staged into term-table slot s % 64 and the stream is
    synchronised when the slot wraps; s130 crosses the ring twice. Slots s
    and s + 64 hold different blobs, so a segment scored with the other's
    descriptors gives another answer.

    This pins the answer. It cannot make the device fall 64 launches behind
    the host, so a missing wait is caught only when the queue happens to be
    that deep."""
    use(monkeypatch, path)
    assert run_single(ctx, dev, m, [set_], path) == 2


@pytest.mark.parametrize("set_,nq,ks", [("s70", 2, None), ("s130", 2, None),
                                        ("trio", 45, (10, 500))])
def test_batch_more_than_64_launches(ctx, dev, m, set_, nq, ks):
    """The batch executor walks slot (q * nsegs + sg) % 64. With three
    segments and 45 queries the ring wraps in mid-query: at launch 64
    (q = 21, sg = 1) and at launch 128 (q = 42, sg = 2). Every query equals
    the single entry and the reference. As above, the answer is pinned; the
    queue depth at which a missing wait would show cannot be forced."""
    if set_ == "trio":
        assert divmod(64, 3) == (21, 1) and divmod(128, 3) == (42, 2)
    run_batch(ctx, dev, m, [set_], "batch", nq=nq, ks=ks)


# ---------------------------------------------------------------------------
# mixed attachments on asc
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("path", ["sweep", "sweep4096", "general", "wave"])
def test_masks_on_some_segments(ctx, dev, m, path, monkeypatch):
    """five segments masked (one with every doc dead, one with exactly the
    last doc dead, the 64- and 65-doc ones at bits 63 and 64 and in the last
    word), seven bare; then the same plan with the masks detached"""
    use(monkeypatch, path)
    run_single(ctx, dev, m, ["masked", "masked_mm2", "unboosted", "masked"],
               path)


BOOST_CASES = ["flat_bm25", "peak_bm25", "peak_desc_bm25", "flat_tfidf_norm",
               "peak_tfidf_norm", "peak_desc_tfidf_norm",
               "gstats_masked_peak"]


@pytest.mark.parametrize("path", ["sweep", "general", "wave"])
def test_filter_boost_columns(ctx, dev, m, path, monkeypatch):
    """per-segment boost columns; with `peak` the set's largest boost sits
    in one small segment that is neither first nor last"""
    use(monkeypatch, path)
    run_single(ctx, dev, m, BOOST_CASES, path)


def test_filter_boost_columns_batch(ctx, dev, m):
    run_batch(ctx, dev, m, BOOST_CASES, "batch", ks=(1, 10, 1000))


@pytest.mark.parametrize("path", ["sweep", "general"])
def test_wand_over_a_set(ctx, dev, m, path, monkeypatch):
    """block-max pruning with bounds scaled by the set's fbmax: the hits are
    exact; visited <= total is the only claim about the count"""
    use(monkeypatch, path)
    for name in ["unboosted", "masked", "gstats"] + BOOST_CASES:
        c = m.cases[name]
        segs, kw = dev.prepare(c)
        total = m.ref_full(c)[3]
        for k in c["ks"]:
            wand, visited = ctx.execute_topk(
                segs, c["terms"], c["boosts"], k, wand=True, **kw,
                **dev.score_kw(c))
            check(m, c, k, wand, visited, f"{path} wand", check_total=False)
            assert visited <= total, (path, name, k)


def test_injected_stats_over_a_set(ctx, dev, m, monkeypatch):
    names = ["gstats", "gstats_tfidf", "gstats_masked_peak"]
    run_batch(ctx, dev, m, names, "batch")
    for path in ("sweep4096", "general", "wave"):
        with monkeypatch.context() as mp:
            use(mp, path)
            run_single(ctx, dev, m, names, path)


# ---------------------------------------------------------------------------
# count and streaming
# ---------------------------------------------------------------------------

def test_count_every_set(ctx, dev, m):
    """execute_count over every set, OR, min_match 2 and AND, against the
    Counter reference; and over the masked set"""
    n = 0
    for set_, plan in ss.SET_PLAN.items():
        for mm in sorted({1, min(2, len(plan)), len(plan)}):
            c = m.case(set_, plan, mm=mm)
            segs, kw = dev.prepare(c)
            got = ctx.execute_count(segs, c["terms"], c["boosts"], **kw)
            assert got == m.ref_count(c), (set_, mm)
            n += 1
    assert n >= 30
    for name in ("masked", "masked_mm2", "asc_wide", "void"):
        c = m.cases[name]
        segs, kw = dev.prepare(c)
        assert ctx.execute_count(segs, c["terms"], c["boosts"], **kw) == \
            m.ref_count(c), name


@pytest.mark.parametrize("set_", ["asc", "desc", "hollow_mid"])
def test_match_docs_over_a_set(ctx, dev, m, set_):
    """the streamed (segment, doc) sequence with the gathered column: a cap
    above the total, one that falls inside the third segment, one equal to
    the first segment's matches exactly, and cap 1; the total keeps counting
    past the cap"""
    c = m.case(set_, ss.SET_PLAN[set_])
    segs, kw = dev.prepare(c, col=True)
    per = [len(m.match_list(bi, c["terms"], 1, False))
           for bi in ss.SETS[set_]]
    total = sum(per)
    if set_ != "hollow_mid":
        assert per[0] and per[2] > 1
    caps = (total + 9, per[0] + per[1] + max(per[2] // 2, 1), per[0], 1)
    for cap in caps:
        if cap == 0:        # hollow first: nothing to ask for
            continue
        sg, docs, cols, got_total = ctx.execute_match_docs_multi(
            segs, c["terms"], c["boosts"], cap, with_col=True, **{
                k: v for k, v in kw.items() if k != "global_stats"})
        pairs, vals, want_total = m.ref_stream(c, cap)
        assert got_total == want_total == total, (set_, cap)
        assert list(zip(sg.tolist(), docs.tolist())) == pairs, (set_, cap)
        assert cols.tolist() == vals, (set_, cap)


# ---------------------------------------------------------------------------
# hybrid over a set
# ---------------------------------------------------------------------------

def hybrid_check(m, c, ref, k, hits, total, bcnt, bsum, what):
    sg, d, s = m.hybrid_hits(c, ref, k)
    assert total == ref.total, what
    assert len(hits) == len(d), what
    np.testing.assert_array_equal(hits["segment"], sg, err_msg=what)
    np.testing.assert_array_equal(hits["doc"], d, err_msg=what)
    np.testing.assert_array_equal(bits(hits["score"]), bits(s), err_msg=what)
    np.testing.assert_array_equal(bcnt, ref.counts, err_msg=what)
    np.testing.assert_array_equal(bsum, ref.sums, err_msg=what)


@pytest.mark.parametrize("entry", ["hybrid", "chain", "batch"])
@pytest.mark.parametrize("set_", ["asc", "hollow_mid"])
def test_hybrid_over_a_set(ctx, dev, m, set_, entry):
    """per-segment columns feeding one set of buckets: an ordinary range, a
    range one whole segment fails, and one whose sums wrap; min_match 1 is
    the sweep branch, min_match 2 the window kernel"""
    for mm in (1, 2):
        c = m.case(set_, ss.SET_PLAN[set_], mm=mm)
        c["name"] = f"hybrid {set_} mm{mm}"     # cache the ranking
        segs, kw = dev.prepare(c, col=True)
        for rname, (lo, hi, nb) in ss.RANGES.items():
            ref = m.ref_hybrid(c, lo, hi, nb)
            for k in (10, ref.total + 7):
                what = f"{entry} {set_} mm{mm} {rname} k={k}"
                if entry == "hybrid":
                    out = ctx.execute_topk_hybrid(
                        segs, c["terms"], c["boosts"], k, lo, hi, nb, **kw)
                    hybrid_check(m, c, ref, k, *out, what)
                elif entry == "chain":
                    out = ctx.execute_topk_hybrid_chain(
                        segs, c["terms"], c["boosts"], k,
                        [(0, BETWEEN, lo, hi)], nb, **kw)
                    hybrid_check(m, c, ref, k, *out, what)
                else:
                    hits, totals, bcnt, bsum = \
                        ctx.execute_topk_hybrid_batch(
                            segs, c["terms"], c["boosts"], k, lo, hi, nb, 3,
                            all_hits=True, **kw)
                    for q in range(3):
                        hybrid_check(m, c, ref, k, hits[q], totals[q],
                                     bcnt[q], bsum[q], f"{what} q{q}")


# ---------------------------------------------------------------------------
# the contract over a set
# ---------------------------------------------------------------------------

def rcs(ctx, segs, plan, hybrid=False):
    """return codes of the set-taking entries, through ctypes"""
    lib, c, k = ctx._lib, ctx._ctx, 10
    arr = (C.c_void_p * len(segs))(*[C.c_void_p(s.value) for s in segs])
    hits = (sa.SdbScoreDoc * (2 * k))()
    n, tot = C.c_uint32(0), C.c_uint64(0)
    counts, totals = (C.c_uint32 * 2)(), (C.c_uint64 * 2)()
    out = {}
    if hybrid:
        PI64 = C.POINTER(C.c_int64)
        bc = np.zeros(2 * 4, dtype=np.int64)
        bs = np.zeros(2 * 4, dtype=np.int64)
        out["hybrid"] = lib.sdb_gpu_execute_topk_hybrid(
            c, arr, C.c_uint32(len(segs)), C.byref(plan), C.c_uint32(k),
            C.c_int64(-300), C.c_int64(400), C.c_uint32(4),
            bc.ctypes.data_as(PI64), bs.ctypes.data_as(PI64), hits,
            C.byref(n), C.byref(tot))
        out["hybrid_batch"] = lib.sdb_gpu_execute_topk_hybrid_batch(
            c, arr, C.c_uint32(len(segs)), C.byref(plan), C.c_uint32(k),
            C.c_int64(-300), C.c_int64(400), C.c_uint32(4), C.c_uint32(2),
            bc.ctypes.data_as(PI64), bs.ctypes.data_as(PI64), hits, counts,
            totals)
        return out
    out["topk"] = lib.sdb_gpu_execute_topk(
        c, arr, C.c_uint32(len(segs)), C.byref(plan), C.c_uint32(k), hits,
        C.byref(n), C.byref(tot))
    out["batch"] = lib.sdb_gpu_execute_topk_batch(
        c, arr, C.c_uint32(len(segs)), C.byref(plan), C.c_uint32(k),
        C.c_uint32(2), hits, counts, totals)
    out["count"] = lib.sdb_gpu_execute_count(
        c, arr, C.c_uint32(len(segs)), C.byref(plan), C.byref(tot))
    return out


def test_contract_over_a_set(ctx, dev, m):
    """One segment of a set that cannot take the plan makes the whole call
    SDB_ERR_INVALID (the check runs before anything is launched), and the
    context answers the next valid call correctly."""
    def still_usable():
        run_single(ctx, dev, m, ["trio"], "after a rejected call", ks=(10,))

    def plan_of(terms, fb=False):
        return ctx._make_plan([ss.T[t] for t in terms], [1.0] * len(terms),
                              1, 1.2, 0.75, None, "bm25", False, fb)

    # fresh loads of the trio's blobs, so that one really lacks its column
    first, mid, last = (ctx.load_segment(m.blobs[bi].blob)
                        for bi in ss.SETS["trio"])
    ok = plan_of(ss.P2)
    assert set(rcs(ctx, [first, mid, last], ok).values()) == {0}

    # ---- a term_idx valid for all but the middle segment
    short_src = m.blobs[ss.HOLLOW]
    short = ctx.load_segment(sa.build_segment(
        short_src.doc_count, short_src.postings[:2], short_src.norms))
    p = plan_of(("common", "rare"))             # term 2: past short's table
    assert set(rcs(ctx, [first, mid, last], p).values()) == {0}
    for entry, rc in rcs(ctx, [first, short, last], p).items():
        assert rc == SDB_ERR_INVALID, ("term_idx", entry, rc)
    still_usable()
    assert set(rcs(ctx, [first, short, last], ok).values()) == {0}

    # ---- a filter_boost plan, the middle segment without its column
    ctx.attach_boost(first, m.blobs[ss.SETS["trio"][0]].fb["flat"])
    ctx.attach_boost(last, m.blobs[ss.SETS["trio"][2]].fb["flat"])
    p = plan_of(ss.P2, fb=True)
    assert set(rcs(ctx, [first, last], p).values()) == {0}
    for entry, rc in rcs(ctx, [first, mid, last], p).items():
        assert rc == SDB_ERR_INVALID, ("filter_boost", entry, rc)
    still_usable()

    # ---- a hybrid call, the middle segment without the column
    ctx.attach_column(first, m.blobs[ss.SETS["trio"][0]].col)
    ctx.attach_column(last, m.blobs[ss.SETS["trio"][2]].col)
    assert set(rcs(ctx, [first, last], ok, hybrid=True).values()) == {0}
    for entry, rc in rcs(ctx, [first, mid, last], ok, hybrid=True).items():
        assert rc == SDB_ERR_INVALID, ("hybrid column", entry, rc)
    still_usable()
