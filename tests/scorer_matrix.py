"""Scorer-matrix corpus: two small segments on which every scoring knob of a
top-k plan (scorer, k1, b, per-term boosts, the per-doc filter boost,
injected global stats, the live mask, the score > FLT_MIN acceptance rule)
is exercised by a named case, plus the independent numpy references the CPU
and GPU matrix tests compare against.

The raw (docs, freqs) arrays per term, the norms column, the filter-boost
columns and the live mask are the ground truth; nothing here decodes a blob
or asks the library for an expected value.

Scale: segment 0 has 3 * 24576 + 77 docs: three full windows of the default
top-k kernels and a partial fourth, 19 windows of the 4096-doc sweep
geometry and 73 sub-windows of the per-wave kernel. Segment 1 is a third of
that. Decode geometry belongs to codec_matrix and block_fetch_matrix; this
matrix is about path dispatch and arithmetic, so it stays small.

Freqs cycle FREQ_LADDER through a term's consecutive postings (rotated by
one per 128-posting block, so every lane and block position sees every
value; see freq_ladder for the two terms that stop one value short); norms cycle NORM_LADDER and the filter boost cycles FB_LADDER
through consecutive docs. No norm is 0: TFIDF-norm divides by sqrt(norm).
"""

import ctypes as C
import functools
import struct

import numpy as np

import serenedb_amd as sa
from oracle import pyoracle as po

WIN = 24576          # docs per window of the default top-k kernels
BLOCK = 128
DOC_COUNT = 3 * WIN + 77
DOC_COUNT2 = WIN + 129
SEED = 0x5C08E8
FLT_MIN = np.float32(1.17549435e-38)
# the last three are where (float)freq rounds
FREQ_LADDER = (1, 2, 3, 255, 65535, 2**24, 2**24 + 1, 2**32 - 1)
# norm 1 is the TFIDF-norm maximum; the large values push total_term_freq
# past 2^24 so the f32 avg_dl quotient rounds
NORM_LADDER = (1, 2, 3, 255, 65536, 2**24 + 1)
FB_LADDER = np.array([0.0, 2.0**-149, FLT_MIN, 0.5, 1.0, 1.0 + 2.0**-23,
                      2.0**20], dtype=np.float32)
ACCEPT_DF = 5000
TERMS = ("dense", "medium", "last", "straddle", "accept", "sparse")
FUSED_TERMS = ("medium", "straddle")
T = {n: i for i, n in enumerate(TERMS)}
SCORERS = ("bm25", "tfidf", "tfidf_norm")
# name -> (scorer, k1, b)
PARAMS = {
    "bm25": ("bm25", 1.2, 0.75),
    "bm25_k09_b04": ("bm25", 0.9, 0.4),
    "bm25_k100": ("bm25", 100.0, 0.75),
    "bm15": ("bm25", 1.2, 0.0),        # b == 0: nc = k1, nl = 0
    "bm25_b1": ("bm25", 1.2, 1.0),     # nc exactly 0
    "bm1": ("bm25", 0.0, 0.75),        # k1 == 0: no score without a boost
    "tfidf": ("tfidf", 1.2, 0.75),
    "tfidf_norm": ("tfidf_norm", 1.2, 0.75),
}
FB_PARAMS = ("bm25", "bm15", "tfidf", "tfidf_norm", "bm1")
# Injected global stats: both f32 narrowings round (dwf is odd above 2^25,
# ttf is far above 2^24), and every docs_with_term differs from the
# segment's own df. The ttf is one at which (float)ttf / (float)dwf and the
# quotient taken in double and narrowed afterwards are different floats
# (2801169.25 and 2801169.0).
G_DWF = 3 * 2**24 + 1
G_TTF = G_DWF * 2_801_169 + 6_000_019
# the scorers a test can substitute for the right one; each restates one
# plausible kernel or host-select mistake
WRONG = ("fb_after", "accept_ge", "avg_double", "local_stats",
         "norm_nosqrt", "total_skips_zero", "b1_as_b0")


def freq_ladder(term):
    """The freqs a term cycles. A freq block holding 2^32 - 1 cannot be
    bitpacked (31 bits is the widest), and only all-bitpacked blocks take the
    kernels' fused decode-and-score path, which has its own copy of the
    scoring fold. So two terms stop one value short: their blocks are fused,
    the other terms' are not, and the three-term plans hold both."""
    return FREQ_LADDER[:-1] if term in FUSED_TERMS else FREQ_LADDER


def fused_blocks(blob):
    """per term, one bool per postings block: the fused shape or not
    (bit 0 of the descriptor flags, sdb_format.h)"""
    hdr = struct.unpack("<QIIIIQQQQQQQQ", blob[:88])
    off_terms, off_desc = hdr[7], hdr[8]
    out = []
    for t in range(hdr[2]):
        te = struct.unpack("<QQQQIIQ", blob[off_terms + 48 * t:
                                            off_terms + 48 * t + 48])
        out.append([bool(struct.unpack(
            "<IIIIHHII", blob[off_desc + 28 * bi:
                              off_desc + 28 * bi + 28])[5] & 1)
            for bi in range(te[0], te[1])])
    return out


class Segment:
    def __init__(self, doc_count, seed):
        rng = np.random.default_rng(seed)
        n = doc_count
        ids = np.arange(1, n + 1, dtype=np.uint32)

        def pick(p):
            return ids[rng.random(n) < p]

        edges = [d for w in range(WIN, n, WIN) for d in (w, w + 1)]
        docs = {
            "dense": pick(1 / 3),
            "medium": pick(1 / 8),
            "last": np.array([n], dtype=np.uint32),
            "straddle": np.union1d(pick(1 / 50), edges).astype(np.uint32),
            "accept": np.sort(rng.choice(ids, ACCEPT_DF, replace=False)),
            "sparse": pick(1 / 64),
        }
        self.doc_count = n
        self.postings = []
        for t, name in enumerate(TERMS):
            ladder = np.array(freq_ladder(name), dtype=np.uint32)
            i = np.arange(len(docs[name]))
            self.postings.append((docs[name].astype(np.uint32),
                                  ladder[(i + i // BLOCK + t) % len(ladder)]))
        self.norms = np.zeros(n + 1, dtype=np.uint32)
        self.norms[1:] = np.array(NORM_LADDER, dtype=np.uint32)[
            ids % len(NORM_LADDER)]
        self.ttf = int(self.norms[1:].sum(dtype=np.uint64))
        self.blob = sa.build_segment(n, self.postings, self.norms)
        fb = np.zeros(n + 1, dtype=np.float32)
        fb[1:] = FB_LADDER[ids % len(FB_LADDER)]
        self.fb = {"ladder": fb}
        # live mask: dead docs are the ones holding the largest boost
        nwords = (n + 64) // 64
        live = np.zeros(nwords * 64, dtype=bool)
        live[1:n + 1] = fb[1:] != FB_LADDER[-1]
        self.live = live[:n + 1]
        self.live_words = np.packbits(live, bitorder="little").view(np.uint64)


def plan_consts(dwf, ttf, dwt, boosts, scorer, k1, b, has_fb, fp64=False,
                wrong=None):
    """(num per term, nc, nl) as prep_plan_stats and the oracle's
    o_prep_cursors compute them: fp32 rounds after every operation; fp64 is
    the same formulas in double from the same f32 parameters."""
    dt = np.float64 if fp64 else np.float32
    F = np.float32
    fk1, fbb = F(k1), F(b)
    nc = nl = dt(0.0)
    if scorer == "bm25":
        kb = dt(fk1) * dt(fbb)
        if fbb == 0 or (wrong == "b1_as_b0" and fbb == 1):
            nc, nl = dt(fk1), dt(0.0)
        else:
            nc = dt(fk1) - kb
            if ttf and dwf:
                if fp64:
                    avg = np.float64(ttf) / np.float64(dwf)
                elif wrong == "avg_double":
                    avg = F(np.float64(ttf) / np.float64(dwf))
                else:
                    avg = F(ttf) / F(dwf)
                nl = kb / avg
            else:
                nl = kb
    nums = []
    for boost, d in zip(boosts, dwt):
        if d == 0:
            nums.append(dt(0.0))
        elif scorer == "bm25":
            idf = dt(np.log1p((np.float64(dwf - d) + 0.5) /
                              (np.float64(d) + 0.5)))
            num = dt(F(boost)) * (dt(fk1) + dt(1.0)) * idf
            if fk1 == 0 and not has_fb:
                num = dt(0.0)
            nums.append(num)
        else:
            idf = dt(np.log1p((np.float64(dwf) + 1.0) /
                              (np.float64(d) + 1.0)))
            nums.append(dt(F(boost)) * idf)
    for x in nums + [nc, nl]:
        assert type(x) is dt
    return nums, nc, nl


def score_form(scorer, nm, nc, nl, f, nrm, wrong=None):
    """score_one: one term's contribution per posting"""
    if scorer == "bm25":
        c1 = nc + nl * nrm
        return nm - nm * c1 / (c1 + f)
    s = nm * np.sqrt(f)
    if scorer == "tfidf_norm":
        s = s / (nrm if wrong == "norm_nosqrt" else np.sqrt(nrm))
    return s


class Matrix:
    """segs: the two Segments. cases[name]: dict(terms, boosts, scorer, k1,
    b, mm, ks, fb, gstats, live, nseg, oracle); fb names one filter-boost
    column per segment (Segment.fb) or is None."""

    def __init__(self):
        self.segs = [Segment(DOC_COUNT, SEED), Segment(DOC_COUNT2, SEED + 1)]
        self.cases = {}
        self.accept = None      # dict(docs, bits) of the acceptance ladder
        self._ref_cache = {}
        self._oracle_cache = {}

    # ---- raw-array arithmetic ------------------------------------------
    def match_docs(self, name):
        """per segment, the docs matched by >= mm terms (and live), by set
        arithmetic on the raw doc arrays"""
        c = self.cases[name]
        out = []
        for seg in self.segs[:c["nseg"]]:
            u, n = np.unique(np.concatenate(
                [seg.postings[t][0] for t in c["terms"]]), return_counts=True)
            u = u[n >= c["mm"]]
            if c["live"]:
                u = u[seg.live[u]]
            out.append(u)
        return out

    def matches(self, name):
        return sum(len(u) for u in self.match_docs(name))

    def stats(self, c, wrong=None):
        if c["gstats"] is not None and wrong != "local_stats":
            return c["gstats"]
        segs = self.segs[:c["nseg"]]
        return (sum(s.doc_count for s in segs), sum(s.ttf for s in segs),
                [sum(len(s.postings[t][0]) for s in segs)
                 for t in c["terms"]])

    # ---- references ------------------------------------------------------
    def ref_scores(self, name, fp64=False, wrong=None):
        """Term-major replication of the scorers over the raw arrays. Per
        segment: (docs ascending, score per doc, matched-term count per doc,
        sum over the doc's matched terms of num * fb[doc])."""
        key = (name, fp64, wrong)
        if key in self._ref_cache:
            return self._ref_cache[key]
        c = self.cases[name]
        dt = np.float64 if fp64 else np.float32
        dwf, ttf, dwt = self.stats(c, wrong)
        nums, nc, nl = plan_consts(dwf, ttf, dwt, c["boosts"], c["scorer"],
                                   c["k1"], c["b"], c["fb"] is not None,
                                   fp64, wrong)
        out = []
        for si, seg in enumerate(self.segs[:c["nseg"]]):
            fbcol = seg.fb[c["fb"][si]] if c["fb"] else None
            u = np.unique(np.concatenate(
                [seg.postings[t][0] for t in c["terms"]]))
            scores = np.zeros(len(u), dtype=dt)
            numsum = np.zeros(len(u), dtype=np.float64)
            cnt = np.zeros(len(u), dtype=np.int32)
            for t, num in zip(c["terms"], nums):
                docs, freqs = seg.postings[t]
                at = np.searchsorted(u, docs)
                f = freqs.astype(dt)
                nrm = seg.norms[docs].astype(dt)
                if fbcol is None:
                    nm = np.full(len(docs), num, dtype=dt)
                    contrib = score_form(c["scorer"], nm, nc, nl, f, nrm,
                                         wrong)
                elif wrong == "fb_after":
                    nm = np.full(len(docs), num, dtype=dt)
                    contrib = score_form(c["scorer"], nm, nc, nl, f, nrm) * \
                        fbcol[docs].astype(dt)
                else:
                    nm = num * fbcol[docs].astype(dt)   # before the form
                    contrib = score_form(c["scorer"], nm, nc, nl, f, nrm,
                                         wrong)
                assert contrib.dtype == dt and nm.dtype == dt
                scores[at] += contrib   # docs are unique within a term
                numsum[at] += nm.astype(np.float64) if fbcol is None \
                    else np.float64(num) * fbcol[docs].astype(np.float64)
                cnt[at] += 1
            if c["live"]:
                keep = seg.live[u]
                u, scores, cnt, numsum = (u[keep], scores[keep], cnt[keep],
                                          numsum[keep])
            out.append((u, scores, cnt, numsum))
        self._ref_cache[key] = out
        return out

    def ref_topk(self, name, k, wrong=None):
        """fp32 reference top-k: (segment, doc, score, total). Score
        descending, then segment, then doc; scores <= FLT_MIN dropped;
        total counts every doc matched by >= mm terms, whatever its score."""
        c = self.cases[name]
        per = self.ref_scores(name, wrong=wrong)
        sg = np.concatenate([np.full(len(p[0]), i, dtype=np.uint32)
                             for i, p in enumerate(per)])
        u = np.concatenate([p[0] for p in per])
        s = np.concatenate([p[1] for p in per])
        cnt = np.concatenate([p[2] for p in per])
        sel = cnt >= c["mm"]
        if wrong == "total_skips_zero":
            total = int((sel & (s > 0)).sum())
        else:
            total = int(sel.sum())
        sel &= (s >= FLT_MIN) if wrong == "accept_ge" else (s > FLT_MIN)
        sg, u, s = sg[sel], u[sel], s[sel]
        order = np.lexsort((u, sg, -s))[:k]
        return sg[order], u[order], s[order], total

    def oracle_topk(self, name, k):
        """The C oracle (third witness) where it can run the case:
        (segment, doc, score, total). One call per case at its largest k;
        the oracle's order is total, so a smaller k is a prefix."""
        c = self.cases[name]
        assert c["oracle"], name
        if name not in self._oracle_cache:
            kmax = max(c["ks"])
            lib = po.lib()
            lib.o_set_scorer(C.c_uint32(po.SCORERS[c["scorer"]]))
            if c["fb"]:
                assert c["nseg"] == 1
                fb = self.segs[0].fb[c["fb"][0]]
                lib.o_set_filter_boost(fb.ctypes.data_as(
                    C.POINTER(C.c_float)))
            if c["live"]:
                assert c["nseg"] == 1
                lib.o_set_live_mask(self.segs[0].live_words.ctypes.data_as(
                    po.PU64))
            arr, keep = po._mkblobs([s.blob for s in self.segs[:c["nseg"]]])
            ti = np.ascontiguousarray(c["terms"], dtype=np.uint32)
            bo = np.ascontiguousarray(c["boosts"], dtype=np.float32)
            g_dwf = g_ttf = 0
            g_dwt = dwt_ptr = None
            if c["gstats"] is not None:
                g_dwf, g_ttf, dwt = c["gstats"]
                g_dwt = np.ascontiguousarray(dwt, dtype=np.uint64)
                dwt_ptr = g_dwt.ctypes.data_as(po.PU64)
            hits = (po.OScoreDoc * kmax)()
            n = C.c_uint32(0)
            total = C.c_uint64(0)
            rc = lib.o_execute_topk(
                arr, C.c_uint32(c["nseg"]), ti.ctypes.data_as(po.PU32),
                bo.ctypes.data_as(C.POINTER(C.c_float)), C.c_uint32(len(ti)),
                C.c_uint32(c["mm"]), C.c_float(c["k1"]), C.c_float(c["b"]),
                C.c_uint64(g_dwf), dwt_ptr, C.c_uint64(g_ttf),
                C.c_uint32(kmax), hits, C.byref(n), C.byref(total))
            lib.o_set_scorer(C.c_uint32(0))
            lib.o_set_filter_boost(None)
            lib.o_set_live_mask(None)
            assert rc == 0, rc
            del keep, g_dwt
            v = np.frombuffer(hits, dtype=[("score", "f4"), ("doc", "u4"),
                                           ("segment", "u4")], count=n.value)
            self._oracle_cache[name] = (v["segment"].copy(), v["doc"].copy(),
                                        v["score"].copy(), total.value)
        sg, u, s, total = self._oracle_cache[name]
        return sg[:k], u[:k], s[:k], total

    # ---- cases -------------------------------------------------------------
    def add(self, name, terms, boosts=None, param="bm25", mm=1, ks=None,
            fb=None, gstats=None, live=False, nseg=1, oracle=None):
        assert name not in self.cases and 1 <= len(terms) <= 4, name
        scorer, k1, b = PARAMS[param]
        if fb is not None and isinstance(fb, str):
            fb = (fb,) * nseg
        c = dict(terms=[T[t] for t in terms],
                 boosts=[1.0] * len(terms) if boosts is None
                 else [float(x) for x in boosts],
                 scorer=scorer, k1=k1, b=b, mm=mm, fb=fb, gstats=gstats,
                 live=live, nseg=nseg, param=param)
        # the oracle takes a filter boost and a live mask for one segment
        c["oracle"] = (not ((fb or live) and nseg > 1)) if oracle is None \
            else oracle
        self.cases[name] = c
        n = self.matches(name)
        c["ks"] = tuple(ks(n)) if callable(ks) else \
            tuple(ks) if ks else (1, 10, n + 1)
        return c


def _accept_boosts(num):
    """Filter boosts whose f32 product with num is, in bits: FLT_MIN + 2,
    + 1, FLT_MIN exactly, - 1, - 2 ulp (the last two subnormal), one
    subnormal far below, and 0. Found by stepping nextafter around
    FLT_MIN / num; num and the boosts are normal, so one step moves the
    product by at most one ulp."""
    F = np.float32
    base = FLT_MIN.view(np.uint32)
    found = {}
    x = F(np.float64(FLT_MIN) / np.float64(num))
    for _ in range(64):
        x = np.nextafter(x, F(0))
    for _ in range(128):
        found.setdefault(int((num * x).view(np.uint32)), x)
        x = np.nextafter(x, F(1))
    want = [int(base) + d for d in (2, 1, 0, -1, -2)]
    for w in want:
        assert w in found, hex(w)
    fbs = [found[w] for w in want]
    fbs.append(F(np.float64(FLT_MIN) / np.float64(num) / 4.0))
    fbs.append(F(2.0**-149))
    return np.array(fbs, dtype=F)


def _build():
    m = Matrix()
    s0, s1 = m.segs
    base3 = ("dense", "medium", "straddle")

    # ---- filter-boost columns beyond the plain ladder
    # "capped"/"split": fbmax (2^20) sits on a segment-1 doc no plan term
    # matches, while segment 0, whose boosts stop at 1 + 2^-23, holds the
    # top hit
    capped = s0.fb["ladder"].copy()
    capped[capped == FB_LADDER[-1]] = 0.5
    s0.fb["capped"] = capped
    split = np.full(DOC_COUNT2 + 1, 2.0**-10, dtype=np.float32)
    split[0] = 0.0
    hit = np.unique(np.concatenate([s1.postings[T[t]][0] for t in base3]))
    lone = np.setdiff1d(np.arange(1, DOC_COUNT2 + 1), hit)[0]
    split[lone] = FB_LADDER[-1]
    s1.fb["split"] = split

    # ---- scorers and parameters, one and two segments
    for nseg in (1, 2):
        for p in PARAMS:
            for mm in (1, 2, 3):
                m.add(f"{p}_mm{mm}" + ("_2seg" if nseg == 2 else ""), base3,
                      param=p, mm=mm, nseg=nseg)

    # ---- term boosts
    m.add("zero_boost_term", ("medium", "dense"), boosts=(1.0, 0.0),
          ks=lambda n: (10, n + 1))
    m.add("all_zero", ("dense", "medium"), boosts=(0.0, 0.0), ks=(10,))
    n_sparse = len(s0.postings[T["sparse"]][0])
    m.add("dynamic_range", ("dense", "medium", "sparse", "last"),
          boosts=(2.0**-100, 1.0, 2.0**60, 1.0),
          ks=lambda n: (n_sparse + 5, n - 100))
    m.add("dynamic_range_2seg", ("dense", "medium", "sparse", "last"),
          boosts=(2.0**-100, 1.0, 2.0**60, 1.0), nseg=2,
          ks=lambda n: (n_sparse + 5, n - 100))

    # ---- filter boost
    for p in FB_PARAMS:
        for mm in (1, 2):
            m.add(f"fb_{p}_mm{mm}", base3, param=p, mm=mm, fb="ladder")
    m.add("fb_split_2seg", base3, fb=("capped", "split"), nseg=2)

    # ---- acceptance boundary: BM1 with a filter boost, score = fl(num * fb)
    nums, _, _ = plan_consts(DOC_COUNT, s0.ttf, [ACCEPT_DF], [2.0**-100],
                             "bm25", 0.0, 0.75, True)
    fbs = _accept_boosts(nums[0])
    adocs = s0.postings[T["accept"]][0][[3, 700, 1400, 2100, 2800, 3500,
                                         4200]]
    col = s0.fb["ladder"].copy()
    col[adocs] = fbs
    s0.fb["accept"] = col
    m.accept = dict(docs=adocs, fbs=fbs, num=nums[0])
    m.add("accept", ("accept",), boosts=(2.0**-100,), param="bm1",
          fb="accept", ks=lambda n: (n + 1,))

    # ---- injected global stats
    g = (G_DWF, G_TTF, [G_DWF // 3, G_DWF // 8 + 1, 1_000_003])
    m.add("gstats_bm25", base3, gstats=g, ks=lambda n: (10, n + 1))
    m.add("gstats_tfidf", base3, param="tfidf", gstats=g,
          ks=lambda n: (10, n + 1))
    # dwt == 0 although the segment has postings: num = 0, the docs are
    # counted and never returned. The oracle drops such a term's iterator
    # altogether (its docs leave the total), so it is no witness here.
    m.add("gstats_dwt0", base3, gstats=(G_DWF, G_TTF, [g[2][0], 0, g[2][2]]),
          ks=lambda n: (10, n + 1), oracle=False)
    m.add("gstats_fb", base3, gstats=g, fb="ladder",
          ks=lambda n: (10, n + 1))

    # ---- live mask under the filter-boost BM25 plan
    m.add("live_fb_bm25", base3, fb="ladder", live=True)
    return m


@functools.lru_cache(maxsize=None)
def matrix():
    """The corpus, built once per process."""
    return _build()
