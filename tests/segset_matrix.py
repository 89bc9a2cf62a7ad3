"""Segment-set matrix corpus: twelve small segments of very different sizes,
the sets (lists of segments, as one call takes them) that reach the code
which exists only because a call takes several segments, and the references
the CPU and GPU matrix tests compare against.

What a set exercises and one segment cannot: the 64-slot term-table ring
(sets of 65, 70 and 130 segments), the threshold, histogram, candidate and
bucket state that every segment's launch accumulates into (all top hits in
the first segment, or in the last), the cross-segment order (score desc,
segment asc, doc asc) with segment = position in the call's array, launches
with nothing to do (a segment where every plan term has df == 0), tiny
segments (1, 2, 63, 64, 65 docs: the live-mask word count), per-segment
attachments mixed within one call, and statistics merged over the set.

The raw (docs, freqs) arrays per term, the norms column, the int64 column,
the filter-boost columns and the live masks are the ground truth; nothing
here decodes a blob or asks the library for an expected value. The fp32
scorer is scorer_matrix's plan_consts and score_form, applied per segment
with the set's merged (or injected) statistics.

Twelve does not divide 64: in a cyclic set, segments s and s + 64 are
different blobs with different descriptor ranges, which is what lets a
slot-ring mistake show. Keep that if DOC_COUNTS changes.
"""

import collections
import ctypes as C
import functools

import numpy as np

import round_stage_matrix as rs
import scorer_matrix as sm
import serenedb_amd as sa
from oracle import pyoracle as po

# 4095..4097: the window of SDB_SWEEP_GEOM=4096x256 and one either side;
# 9000: three windows at that geometry; 24576, 24577: the default window and
# one doc more
DOC_COUNTS = (1, 2, 63, 64, 65, 127, 4095, 4096, 4097, 9000, 24576, 24577)
NBLOBS = len(DOC_COUNTS)
assert 64 % NBLOBS != 0
SEED = 0x5E65E7
FLT_MIN = sm.FLT_MIN
NWIDE = 30
TERMS = ("common", "mid", "rare", "void", "tie", "spike") + tuple(
    f"w{j}" for j in range(NWIDE))
T = {n: i for i, n in enumerate(TERMS)}
NORM_LADDER = (3, 7, 20, 50, 120, 300)       # norms[d] = ladder[d % 6]
SPIKE = 9                                     # the blob holding the spikes
# freq 250 on norm 1, and bit-equal scores under P3: one histogram bin
SPIKE_DOCS = tuple(600 * j + 7 for j in range(12))
QUIET_SPIKE_DOCS = (5, 11, 35, 59, 4001, 20003)   # d % 6 == 5: norm 300
RARE_IN = (3, 6, 9, 11)
TIE_IN = (4, 5, 7, 8, 10, 11)
# doc -> freq; docs 3 and 9 share freq and norm (one class of two docs per
# segment), the others are a class of one doc per segment
TIE_DOCS = {3: 9, 9: 9, 10: 7, 17: 5, 24: 3}
MASKED = (1, 3, 4, 6, 10)
PEAK = 2                                      # blob holding peak's maximum
PEAK_VALUE = np.float32(64.0)
HOLLOW = 5                 # 127 docs: no rare and no wide postings
COLD = 7                   # blob whose column fails both narrow ranges
HUGE_IN = (10, 11)

P2 = ("common", "mid")
P3 = ("common", "mid", "spike")
PR = ("rare", "w0")
PT = ("tie",)
P32 = P3 + tuple(f"w{j}" for j in range(NWIDE - 1))
assert len(P32) == 32
# a doc holding several wide terms must stay below the spikes
WIDE_BOOSTS = rs.boosts_for(P32)
WIDE_BOOSTS[2] = 25.0

# hybrid ranges over the int64 column: (lo, hi, nbuckets)
RANGES = {
    "ordinary": (-300, 400, 16),
    # blob COLD holds 5000 + d: the whole segment fails
    "fails_one": (-1000, 1000, 7),
    # only blobs HUGE_IN hold such values; their sums wrap int64
    "huge": (2**62, 2**63 - 1, 8),
}

SETS = {
    "asc": list(range(NBLOBS)),
    "desc": list(range(NBLOBS))[::-1],
    "spike_first": [SPIKE] + [i for i in range(NBLOBS) if i != SPIKE],
    "spike_last": [i for i in range(NBLOBS) if i != SPIKE] + [SPIKE],
    "dups": [8, 8, 8],           # one blob loaded three times
    "same_handle": [8, 8, 8],    # one handle passed three times
    "hollow_first": [HOLLOW, 6, 9, 11],
    "hollow_mid": [6, 9, HOLLOW, 11],
    "hollow_last": [6, 9, 11, HOLLOW],
    "all_hollow": [0, 1, 2, HOLLOW],
    "only_one_doc": [0],
    "trio": [6, 3, 9],
    "s65": [i % NBLOBS for i in range(65)],
    "s70": [i % NBLOBS for i in range(70)],
    "s130": [i % NBLOBS for i in range(130)],
    "empty": [],
}
# the plan a set is scored with where a test walks every set
SET_PLAN = {s: PR if "hollow" in s else P2 for s in SETS}
SET_PLAN["only_one_doc"] = ("common",)

# the mistakes a reference can make on purpose (the wrong= argument):
# segment = the blob's index instead of the position in the call; ties
# ordered (doc, segment); statistics per segment instead of merged; fbmax of
# the first segment only, which changes no score and shows in ref_smax
WRONG = ("blob_index", "doc_first", "local_stats", "fbmax_first")


def to_i64(x):
    x &= (1 << 64) - 1
    return x - (1 << 64) if x >> 63 else x


class Blob:
    """one segment: raw arrays, blob, column, boost columns, live mask"""

    def __init__(self, bi):
        n = DOC_COUNTS[bi]
        rng = np.random.default_rng(SEED + bi)
        ids = np.arange(1, n + 1, dtype=np.uint32)
        self.index, self.doc_count = bi, n

        def pick(p, *extra):
            keep = ids[rng.random(n) < p]
            ex = [d for d in extra if 1 <= d <= n]
            return np.union1d(keep, ex).astype(np.uint32)

        def ladder(docs, values, shift=0):
            v = np.array(values, dtype=np.uint32)
            return v[(np.arange(len(docs)) + shift) % len(v)]

        none = np.zeros(0, dtype=np.uint32)
        post = {t: (none, none) for t in TERMS}
        d = pick(1 / 3, 1, n)
        post["common"] = (d, ladder(d, (1, 2, 3, 5, 9, 14), bi))
        if n > 1:      # in the 1-doc segment common is the only posting
            d = pick(1 / 11, 2)
            post["mid"] = (d, ladder(d, (1, 4, 2, 7)))
        if bi in RARE_IN:
            d = pick(1 / 40, n // 2 + 1)
            post["rare"] = (d, ladder(d, (1, 2, 6)))
        if bi in TIE_IN:
            post["tie"] = (np.array(sorted(TIE_DOCS), dtype=np.uint32),
                           np.array([TIE_DOCS[x] for x in sorted(TIE_DOCS)],
                                    dtype=np.uint32))
        if bi == SPIKE:
            d = np.array(SPIKE_DOCS, dtype=np.uint32)
            post["spike"] = (d, np.full(len(d), 250, dtype=np.uint32))
            # every spike doc also holds common and mid at freq 1: the
            # twelve match every term of P3 and score bit-equal under it
            for t in ("common", "mid"):
                docs = np.union1d(post[t][0], d).astype(np.uint32)
                freqs = np.ones(len(docs), dtype=np.uint32)
                old = ~np.isin(docs, d)
                freqs[old] = post[t][1][~np.isin(post[t][0], d)]
                post[t] = (docs, freqs)
        else:
            d = np.array([x for x in QUIET_SPIKE_DOCS if x <= n],
                         dtype=np.uint32)
            post["spike"] = (d, np.ones(len(d), dtype=np.uint32))
        if n >= 4095:
            for j in range(NWIDE):
                d = pick(1 / 200, (37 * j + 11) % n + 1)
                post[f"w{j}"] = (d, ladder(d, (1, 3), j))
        self.postings = [post[t] for t in TERMS]

        self.norms = np.zeros(n + 1, dtype=np.uint32)
        self.norms[1:] = np.array(NORM_LADDER, dtype=np.uint32)[
            ids % len(NORM_LADDER)]
        if bi == SPIKE:
            self.norms[list(SPIKE_DOCS)] = 1
        self.ttf = int(self.norms[1:].sum(dtype=np.uint64))
        self.blob = sa.build_segment(n, self.postings, self.norms)

        # int64 column: values on both sides of the narrow ranges
        col = np.zeros(n + 1, dtype=np.int64)
        di = ids.astype(np.int64)
        col[1:] = (di * 2654435761 + 97 * bi) % 2001 - 1000
        if bi == COLD:
            col[1:] = 5000 + di
        if bi in HUGE_IN:
            sel = di[di % 3 == 0]
            col[sel] = 2**62 + sel % 1000 + (2**61 if bi == HUGE_IN[1] else 0)
        self.col = col

        flat = np.zeros(n + 1, dtype=np.float32)
        flat[1:] = np.array([0.5, 1.0, 0.75, 1.25], dtype=np.float32)[ids % 4]
        peak = flat.copy()
        if bi == PEAK:
            peak[n] = PEAK_VALUE     # the last doc: a common posting
        self.fb = {"flat": flat, "peak": peak}

        # live mask, for the blobs of MASKED only
        nwords = (n + 64) // 64
        live = np.zeros(nwords * 64, dtype=bool)
        live[1:n + 1] = True
        self.masked = bi in MASKED
        if bi == 1:
            live[:] = False                       # every doc dead
        elif bi == 3:
            live[[63, 64]] = False                # bit 63, and the last word
        elif bi == 4:
            live[[63, 64, 65]] = False            # bits 63, 64: both words
        elif bi == 6:
            live[n] = False                       # exactly the last doc
        elif bi == 10:
            live[5::5] = False
            live[n] = False
        self.live = live[:n + 1]
        self.live_words = np.packbits(live, bitorder="little").view(np.uint64)
        assert len(self.live_words) == nwords

    def df(self, t):
        return len(self.postings[t][0])


def oracle_topk(blobs, terms, boosts, k, mm=1, k1=1.2, b=0.75, scorer="bm25",
                gstats=None, fb=None, live_words=None):
    """po.execute_topk with the hits read in one copy (its own conversion
    walks them in Python): (segment, doc, score, total)"""
    lib = po.lib()
    lib.o_set_scorer(C.c_uint32(po.SCORERS[scorer]))
    if fb is not None:
        assert len(blobs) == 1
        fb = np.ascontiguousarray(fb, dtype=np.float32)
        lib.o_set_filter_boost(fb.ctypes.data_as(C.POINTER(C.c_float)))
    if live_words is not None:
        assert len(blobs) == 1
        live_words = np.ascontiguousarray(live_words, dtype=np.uint64)
        lib.o_set_live_mask(live_words.ctypes.data_as(po.PU64))
    arr, keep = po._mkblobs(blobs)
    ti = np.ascontiguousarray(terms, dtype=np.uint32)
    bo = np.ascontiguousarray(boosts, dtype=np.float32)
    g_dwf = g_ttf = 0
    g_dwt = dwt_ptr = None
    if gstats is not None:
        g_dwf, g_ttf, dwt = gstats
        g_dwt = np.ascontiguousarray(dwt, dtype=np.uint64)
        dwt_ptr = g_dwt.ctypes.data_as(po.PU64)
    k = max(int(k), 1)
    hits = (po.OScoreDoc * k)()
    n, total = C.c_uint32(0), C.c_uint64(0)
    rc = lib.o_execute_topk(
        arr, C.c_uint32(len(blobs)), ti.ctypes.data_as(po.PU32),
        bo.ctypes.data_as(C.POINTER(C.c_float)), C.c_uint32(len(ti)),
        C.c_uint32(mm), C.c_float(k1), C.c_float(b), C.c_uint64(g_dwf),
        dwt_ptr, C.c_uint64(g_ttf), C.c_uint32(k), hits, C.byref(n),
        C.byref(total))
    lib.o_set_scorer(C.c_uint32(0))
    lib.o_set_filter_boost(None)
    lib.o_set_live_mask(None)
    assert rc == 0, rc
    del keep, g_dwt
    v = np.frombuffer(hits, dtype=[("score", "f4"), ("doc", "u4"),
                                   ("segment", "u4")], count=n.value)
    return (v["segment"].copy(), v["doc"].copy(), v["score"].copy(),
            total.value)


Hybrid = collections.namedtuple("Hybrid", "total survivors counts sums")


class Matrix:
    """blobs: the twelve Blobs. cases[name]: dict(set, terms, boosts,
    scorer, k1, b, mm, gstats, masked, fb, ks); masked attaches the live
    masks of MASKED (the other segments stay bare), fb names the
    filter-boost column every segment carries, or is None."""

    def __init__(self):
        self.blobs = [Blob(bi) for bi in range(NBLOBS)]
        self.cases = {}
        self._full = {}
        self._match = {}

    # ---- cases ---------------------------------------------------------
    def case(self, set_, terms, boosts=None, param="bm25", mm=1, gstats=None,
             masked=False, fb=None, ks=None):
        """a case dict; add() registers one under a name"""
        scorer, k1, b = sm.PARAMS[param]
        if mm == "and":
            mm = len(terms)
        if gstats is True:
            gstats = self.injected(terms)
        c = dict(set=set_, terms=[T[t] for t in terms],
                 boosts=rs.boosts_for(terms) if boosts is None
                 else [float(x) for x in boosts],
                 scorer=scorer, k1=k1, b=b, mm=mm, gstats=gstats,
                 masked=masked, fb=fb, name=None)
        n = self.ref_count(c)
        c["ks"] = tuple(ks(n)) if callable(ks) else \
            tuple(ks) if ks else (1, 10, 1000, n + 7)
        return c

    def add(self, name, *a, **kw):
        assert name not in self.cases, name
        c = self.case(*a, **kw)
        c["name"] = name
        self.cases[name] = c
        return c

    @staticmethod
    def injected(terms):
        """global stats at which both f32 narrowings round
        (scorer_matrix.G_DWF, G_TTF) and no docs_with_term is a segment's or
        the set's own df"""
        return (sm.G_DWF, sm.G_TTF,
                [sm.G_DWF // (3 + 5 * i) + i for i in range(len(terms))])

    def positions(self, c):
        return SETS[c["set"]]

    # ---- statistics ----------------------------------------------------
    def merged_stats(self, c, only=None):
        """(docs_with_field, total_term_freq, df per term) summed over the
        set (over blob `only` alone: the per-segment mistake)"""
        bis = self.positions(c) if only is None else [only]
        bl = [self.blobs[bi] for bi in bis]
        return (sum(x.doc_count for x in bl), sum(x.ttf for x in bl),
                [sum(x.df(t) for x in bl) for t in c["terms"]])

    def stats(self, c, wrong=None, only=None):
        if c["gstats"] is not None:
            return c["gstats"]
        return self.merged_stats(c, only if wrong == "local_stats" else None)

    def fbmax(self, c, wrong=None):
        """the largest filter boost over the set (of the first segment
        only: the mistake)"""
        if c["fb"] is None:
            return np.float32(1.0)
        bis = self.positions(c)
        if wrong == "fbmax_first":
            bis = bis[:1]
        return np.float32(max(self.blobs[bi].fb[c["fb"]][1:].max()
                              for bi in bis))

    def ref_smax(self, c, wrong=None):
        """the score bound prep_plan_stats scales the histogram bins and the
        WAND bounds with: the f32 sum of the term bounds times fbmax; for
        TFIDF a term's bound takes its largest freq over the set"""
        F = np.float32
        dwf, ttf, dwt = self.stats(c)
        nums, _, _ = sm.plan_consts(dwf, ttf, dwt, c["boosts"], c["scorer"],
                                    c["k1"], c["b"], c["fb"] is not None)
        smax = F(0.0)
        for t, num, d in zip(c["terms"], nums, dwt):
            if d == 0:
                continue
            if c["scorer"] != "bm25":
                mf = max([1] + [int(self.blobs[bi].postings[t][1].max())
                                for bi in self.positions(c)
                                if self.blobs[bi].df(t)])
                num = num * np.sqrt(F(mf))
            smax = smax + (num if num > 0 else F(0.0))
        if c["fb"] is not None:
            smax = smax * self.fbmax(c, wrong)
        return smax if smax > 0 else F(1.0)

    # ---- the fp32 reference ----------------------------------------------
    def _blob_scores(self, c, bi, consts):
        """(docs ascending, score, matched-term count) of one blob: term-
        major, the live mask and the filter boost of this segment applied"""
        nums, nc, nl = consts
        seg = self.blobs[bi]
        F = np.float32
        fbcol = seg.fb[c["fb"]] if c["fb"] else None
        u = np.unique(np.concatenate(
            [seg.postings[t][0] for t in c["terms"]]))
        scores = np.zeros(len(u), dtype=F)
        cnt = np.zeros(len(u), dtype=np.int32)
        for t, num in zip(c["terms"], nums):
            docs, freqs = seg.postings[t]
            if not len(docs):
                continue
            at = np.searchsorted(u, docs)
            nm = np.full(len(docs), num, dtype=F)
            if fbcol is not None:
                nm = num * fbcol[docs]          # before the form
            contrib = sm.score_form(c["scorer"], nm, nc, nl, freqs.astype(F),
                                    seg.norms[docs].astype(F))
            assert contrib.dtype == F
            scores[at] += contrib
            cnt[at] += 1
        if c["masked"] and seg.masked:
            keep = seg.live[u]
            u, scores, cnt = u[keep], scores[keep], cnt[keep]
        return u, scores, cnt

    def ref_full(self, c, wrong=None):
        """every accepted match in rank order, and the total: (segment, doc,
        score, total). Score descending, then segment (the position in the
        set), then doc; scores <= FLT_MIN dropped; the total counts every
        live doc matched by >= mm terms."""
        key = (c["name"], wrong)
        if c["name"] is not None and key in self._full:
            return self._full[key]
        per_blob = {}
        consts = None
        if wrong != "local_stats" or c["gstats"] is not None:
            dwf, ttf, dwt = self.stats(c)
            consts = sm.plan_consts(dwf, ttf, dwt, c["boosts"], c["scorer"],
                                    c["k1"], c["b"], c["fb"] is not None)
        sg, u, s, cnt = [], [], [], []
        for pos, bi in enumerate(self.positions(c)):
            if bi not in per_blob:
                k = consts
                if k is None:
                    dwf, ttf, dwt = self.stats(c, wrong, bi)
                    k = sm.plan_consts(dwf, ttf, dwt, c["boosts"],
                                       c["scorer"], c["k1"], c["b"],
                                       c["fb"] is not None)
                per_blob[bi] = self._blob_scores(c, bi, k)
            bu, bs, bc = per_blob[bi]
            sg.append(np.full(len(bu), bi if wrong == "blob_index" else pos,
                              dtype=np.uint32))
            u.append(bu)
            s.append(bs)
            cnt.append(bc)
        if not sg:
            z = np.zeros(0, dtype=np.uint32)
            return z, z, np.zeros(0, dtype=np.float32), 0
        sg, u, s, cnt = (np.concatenate(x) for x in (sg, u, s, cnt))
        sel = cnt >= c["mm"]
        total = int(sel.sum())
        sel &= s > FLT_MIN
        sg, u, s = sg[sel], u[sel], s[sel]
        if wrong == "doc_first":
            order = np.lexsort((sg, u, -s))
        else:
            order = np.lexsort((u, sg, -s))
        out = (sg[order], u[order], s[order], total)
        for a in out[:3]:
            a.setflags(write=False)
        if c["name"] is not None:
            self._full[key] = out
        return out

    def ref_topk(self, c, k, wrong=None):
        sg, u, s, total = self.ref_full(c, wrong)
        return sg[:k], u[:k], s[:k], total

    # ---- plain-Python references -----------------------------------------
    def match_list(self, bi, terms, mm, masked):
        """ascending docs of blob bi matched by >= mm of the terms and
        live: Python ints and a Counter, no numpy set arithmetic"""
        key = (bi, tuple(terms), mm, masked)
        if key not in self._match:
            seg = self.blobs[bi]
            tally = collections.Counter()
            for t in terms:
                tally.update(seg.postings[t][0].tolist())
            alive = seg.live.tolist() if masked and seg.masked else None
            self._match[key] = sorted(
                d for d, n in tally.items()
                if n >= mm and (alive is None or alive[d]))
        return self._match[key]

    def ref_count(self, c):
        return sum(len(self.match_list(bi, c["terms"], c["mm"], c["masked"]))
                   for bi in self.positions(c))

    def ref_stream(self, c, cap):
        """the streamed sequence: ([(segment, doc)] segment ascending then
        doc ascending, cut at cap; the column value of each; the total,
        which keeps counting past the cap)"""
        pairs, vals, total = [], [], 0
        for pos, bi in enumerate(self.positions(c)):
            docs = self.match_list(bi, c["terms"], c["mm"], c["masked"])
            total += len(docs)
            col = self.blobs[bi].col
            for d in docs[:max(cap - len(pairs), 0)]:
                pairs.append((pos, d))
                vals.append(int(col[d]))
        return pairs, vals, total

    def ref_hybrid(self, c, lo, hi, nb):
        """survivors (matching, live, lo <= value <= hi), bucket counts and
        wrap-around int64 bucket sums added over the set, in Python ints"""
        cnt, raw, surv = [0] * nb, [0] * nb, set()
        span = hi - lo + 1
        for pos, bi in enumerate(self.positions(c)):
            col = self.blobs[bi].col
            for d in self.match_list(bi, c["terms"], c["mm"], c["masked"]):
                v = int(col[d])
                if lo <= v <= hi:
                    bkt = (v - lo) * nb // span
                    cnt[bkt] += 1
                    raw[bkt] += v
                    surv.add((pos, d))
        return Hybrid(len(surv), surv, np.array(cnt, dtype=np.int64),
                      np.array([to_i64(x) for x in raw], dtype=np.int64))

    def hybrid_hits(self, c, ref, k):
        """the first k survivors in rank order: (segment, doc, score)"""
        sg, u, s, _ = self.ref_full(c)
        keep = np.fromiter(((a, d) in ref.survivors
                            for a, d in zip(sg.tolist(), u.tolist())),
                           dtype=bool, count=len(u))
        return sg[keep][:k], u[keep][:k], s[keep][:k]


def _build():
    m = Matrix()
    add = m.add

    # ---- orders and k edges
    for s in ("asc", "desc", "spike_first", "spike_last"):
        add(f"{s}_or", s, P3,
            ks=lambda n: (1, 3, 10, 1000, n + 7))
        add(f"{s}_mm2", s, P3, mm=2)
        add(f"{s}_and", s, P3, mm="and")
        add(f"{s}_wide", s, P32, boosts=WIDE_BOOSTS)

    # ---- ties across segments
    for s in ("dups", "same_handle"):
        add(f"{s}_tie", s, PT, ks=range(1, 3 * len(TIE_DOCS) + 2))
        # every doc is a class of three: k walks the first classes
        add(f"{s}_p2", s, P2, ks=range(1, 14))
    add("asc_tie", "asc", PT, ks=range(1, len(TIE_IN) * len(TIE_DOCS) + 2))

    # ---- hollow, tiny and empty
    for s in ("hollow_first", "hollow_mid", "hollow_last", "all_hollow"):
        add(s, s, PR)
    add("void", "asc", ("void",))
    add("void_in_or", "asc", ("common", "void", "mid"))
    add("only_one_doc", "only_one_doc", ("common",))
    add("empty", "empty", P2)

    # ---- more than 64 launches
    for s in ("s65", "s70", "s130"):
        add(s, s, P2, ks=lambda n: (10, n + 7))
    add("trio", "trio", P2, ks=lambda n: (10, n + 7))

    # ---- mixed attachments on asc
    add("masked", "asc", P3, masked=True)
    add("masked_mm2", "asc", P3, mm=2, masked=True)
    add("unboosted", "asc", P3)
    for p in ("bm25", "tfidf_norm"):
        add(f"flat_{p}", "asc", P3, param=p, fb="flat")
        add(f"peak_{p}", "asc", P3, param=p, fb="peak")
        add(f"peak_desc_{p}", "desc", P3, param=p, fb="peak")
    add("gstats", "asc", P3, gstats=True)
    add("gstats_tfidf", "desc", P3, param="tfidf", gstats=True)
    add("gstats_masked_peak", "asc", P3, gstats=True, masked=True, fb="peak")
    return m


@functools.lru_cache(maxsize=None)
def matrix():
    """The corpus, built once per process."""
    return _build()
