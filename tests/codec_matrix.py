"""Codec-matrix corpus: one deterministic segment in which every term
isolates one property of the postings block format (a bit width, a block
family, a tail length, a window straddle), plus the independent numpy
references the CPU and GPU matrix tests compare against.

The raw (docs, freqs) arrays per term and the norms column are the ground
truth; nothing here decodes the blob to obtain an expected value.

Scale: DOC_COUNT is 13M rather than the ~5M that doc-gap width 22 needs,
because the top-k kernels launch min(256 x workgroups/CU, windows) workgroups
over 24576-doc windows and a workgroup only prunes (WAND) in windows after
the ones whose histogram it has already merged: with fewer than three windows
per workgroup (<= 2 x 256 x 24576 = 12.58M docs) block-max pruning provably
never has a threshold to prune with, and `visited < total` could not be
asserted. 13M docs also lets doc-gap widths 23 and 24 in.
"""

import ctypes as C
import functools
import struct

import numpy as np

import serenedb_amd as sa
from oracle import pyoracle as po

DOC_COUNT = 13_000_000
SEED = 0x5DB0C0DE
WIN = 24576          # docs per window of the default top-k kernels
BLOCK = 128
FLT_MIN = np.float32(1.17549435e-38)
TAIL_LENGTHS = (1, 2, 3, 63, 64, 65, 127)
DOC_WIDTHS = tuple(range(2, 25))    # 25..31 need a gap >= 2^24 > DOC_COUNT
FREQ_WIDTHS = tuple(range(2, 32))
NORM_WIDTHS = tuple(range(2, 32))
SCORERS = ("bm25", "tfidf", "tfidf_norm")


def _pin(rng, w):
    """A value of bit width exactly w with at most 24 significant bits, so
    its float conversion is exact."""
    sig = min(w, 24)
    top = int(rng.integers(1 << (sig - 1), 1 << sig))
    return top << (w - sig)


def _small(rng, w, n):
    """n values in [1, min(2^12, 2^w)): below the pinned width and small
    enough that a mis-extracted high bit moves the fp32 score."""
    return rng.integers(1, min(1 << 12, 1 << w), n).astype(np.uint32)


def _walk(rng, start, n, lo, hi):
    """n ascending doc ids after `start` with gaps uniform in [lo, hi]."""
    return (start + np.cumsum(rng.integers(lo, hi + 1, n))).astype(np.uint32)


def _edge_pair(df, ttf_base):
    """Two (freq, norm) pairs whose single-term fp32 BM25 scores lie a few
    ulp above the same edge of the kernels' 256-bin score histogram
    (bin = (u32)(s * (256 / smax)), smax = num for a one-term plan), the
    second scoring strictly higher. ttf_base: the norm sum without the two
    docs, whose norms feed back into the average length."""
    F = np.float32
    f, n = np.meshgrid(np.arange(1, 65), np.arange(1, 4095), indexing="ij")
    f, n = f.ravel(), n.ravel()
    idf = F(np.log1p((np.float64(DOC_COUNT - df) + 0.5) /
                     (np.float64(df) + 0.5)))
    num = F(1.0) * (F(1.2) + F(1.0)) * idf
    inv_smax = F(256.0) / num
    nc = F(1.2) - F(1.2) * F(0.75)

    def scores(ttf, f, n):
        nl = F(F(1.2) * F(0.75)) / (F(ttf) / F(DOC_COUNT))
        c1 = nc + nl * n.astype(F)
        s = num - num * c1 / (c1 + f.astype(F))
        b = (s * inv_smax).astype(np.uint32)
        floor = b.astype(F) / inv_smax        # the bin's float floor
        return s, b, s.astype(np.float64) / floor.astype(np.float64) - 1.0

    guess = ttf_base + 4000
    for _ in range(8):
        s, b, delta = scores(guess, f, n)
        delta[b == 0] = np.inf
        first = {}
        pair = None
        for i in np.argsort(delta)[:5000]:
            j = first.setdefault(int(b[i]), int(i))
            if s[j] != s[i]:
                pair = (j, int(i)) if s[j] < s[i] else (int(i), j)
                break
        assert pair is not None
        exact = ttf_base + int(n[pair[0]]) + int(n[pair[1]])
        if F(exact) == F(guess):
            a, bb = pair
            assert b[a] == b[bb] and s[a] < s[bb] and delta[bb] < 1e-5
            return (int(f[a]), int(n[a])), (int(f[bb]), int(n[bb]))
        guess = exact
    raise AssertionError("edge pair search did not settle")


class Matrix:
    """The built corpus. postings[t] = (docs, freqs) raw arrays; names[t]
    the term's label; idx[name] its term index; groups = OR plans of at
    most 32 terms that together cover every term; small_groups = 4-term
    plans for the per-wave kernel and the non-default sweep geometries."""

    def __init__(self):
        self.names = []
        self.postings = []
        self.idx = {}
        self.norms = None
        self.ttf = 0
        self.blob = None
        self.groups = {}
        self.small_groups = {}
        self.edge_docs = None    # (A, B) of the "edge" term
        self._ref_cache = {}
        self._oracle_cache = {}

    def add(self, name, docs, freqs):
        docs = np.ascontiguousarray(docs, dtype=np.uint32)
        freqs = np.ascontiguousarray(freqs, dtype=np.uint32)
        assert len(docs) == len(freqs) and len(docs) > 0, name
        assert docs[0] >= 1 and docs[-1] <= DOC_COUNT, (name, docs[-1])
        assert np.all(np.diff(docs.astype(np.int64)) > 0), name
        assert freqs.min() >= 1, name
        self.idx[name] = len(self.names)
        self.names.append(name)
        self.postings.append((docs, freqs))

    def terms(self, names):
        return [self.idx[n] for n in names]

    # ---- references -----------------------------------------------------
    def ref_scores(self, terms, boosts, scorer, fp64=False, k1=1.2, b=0.75):
        """Term-major replication of the scorers over the raw arrays.
        Returns (docs ascending, score per doc, matched-term count per doc,
        sum of num over the doc's matched terms). fp32: every operation is
        rounded to float exactly where the C scorers round; fp64: the same
        formulas in double from the same float parameters."""
        key = (tuple(terms), tuple(float(x) for x in boosts), scorer, fp64)
        if key in self._ref_cache:
            return self._ref_cache[key]
        dt = np.float64 if fp64 else np.float32
        n_docs = DOC_COUNT
        u = np.unique(np.concatenate([self.postings[t][0] for t in terms]))
        scores = np.zeros(len(u), dtype=dt)
        numsum = np.zeros(len(u), dtype=np.float64)
        cnt = np.zeros(len(u), dtype=np.int32)
        ttf = self.ttf
        fk1, fb = np.float32(k1), np.float32(b)
        nc = dt(fk1) - dt(fk1) * dt(fb)
        avg = dt(np.float32(ttf)) / dt(np.float32(n_docs)) if not fp64 \
            else np.float64(ttf) / np.float64(n_docs)
        nl = dt(dt(fk1) * dt(fb)) / avg
        for t, boost in zip(terms, boosts):
            docs, freqs = self.postings[t]
            df = len(docs)
            at = np.searchsorted(u, docs)
            f = freqs.astype(dt)
            nrm = self.norms[docs].astype(dt)
            if scorer == "bm25":
                idf = dt(np.log1p((np.float64(n_docs - df) + 0.5) /
                                  (np.float64(df) + 0.5)))
                num = dt(np.float32(boost)) * (dt(fk1) + dt(1.0)) * idf
                c1 = nc + nl * nrm
                contrib = num - num * c1 / (c1 + f)
            else:
                idf = dt(np.log1p((np.float64(n_docs) + 1.0) /
                                  (np.float64(df) + 1.0)))
                num = dt(np.float32(boost)) * idf
                contrib = num * np.sqrt(f)
                if scorer == "tfidf_norm":
                    contrib = contrib / np.sqrt(nrm)
            assert contrib.dtype == dt
            scores[at] += contrib   # docs are unique within a term
            numsum[at] += float(num)
            cnt[at] += 1
        out = (u, scores, cnt, numsum)
        self._ref_cache[key] = out
        return out

    def ref_topk(self, terms, boosts, k, scorer, min_match=1):
        """fp32 reference top-k: score descending then doc ascending,
        scores <= FLT_MIN dropped; total counts every match."""
        u, s, cnt, _ = self.ref_scores(terms, boosts, scorer)
        sel = cnt >= min_match
        total = int(sel.sum())
        u, s = u[sel], s[sel]
        keep = s > FLT_MIN
        u, s = u[keep], s[keep]
        order = np.lexsort((u, -s))[:k]
        return u[order], s[order], total

    def oracle_topk(self, terms, boosts, k, scorer, min_match=1):
        """The CPU oracle on the blob (second witness), (docs, scores,
        total). Same entry point as pyoracle.execute_topk, reading the hits
        through a numpy view (whole posting lists come back here)."""
        key = (tuple(terms), tuple(float(x) for x in boosts), k, scorer,
               min_match)
        if key in self._oracle_cache:
            return self._oracle_cache[key]
        lib = po.lib()
        lib.o_set_scorer(C.c_uint32(po.SCORERS[scorer]))
        arr, keep = po._mkblobs([self.blob])
        ti = np.ascontiguousarray(terms, dtype=np.uint32)
        bo = np.ascontiguousarray(boosts, dtype=np.float32)
        hits = (po.OScoreDoc * k)()
        n = C.c_uint32(0)
        total = C.c_uint64(0)
        rc = lib.o_execute_topk(
            arr, C.c_uint32(1), ti.ctypes.data_as(po.PU32),
            bo.ctypes.data_as(C.POINTER(C.c_float)), C.c_uint32(len(ti)),
            C.c_uint32(min_match), C.c_float(1.2), C.c_float(0.75),
            C.c_uint64(0), None, C.c_uint64(0), C.c_uint32(k), hits,
            C.byref(n), C.byref(total))
        lib.o_set_scorer(C.c_uint32(0))
        assert rc == 0, rc
        del keep
        view = np.frombuffer(hits, dtype=[("score", "f4"), ("doc", "u4"),
                                          ("segment", "u4")], count=n.value)
        out = (view["doc"].copy(), view["score"].copy(), total.value)
        self._oracle_cache[key] = out
        return out

    # ---- blob structure -------------------------------------------------
    def blocks(self):
        """Per term, the list of block records parsed from the blob's term
        table, descriptors and payload tag bytes (sdb_format.h)."""
        blob = self.blob
        hdr = struct.unpack("<QIIIIQQQQQQQQ", blob[:88])
        nterms = hdr[2]
        off_terms, off_desc, _off_norms, off_payload = hdr[7:11]
        out = []
        for t in range(nterms):
            te = struct.unpack("<QQQQIIQ", blob[off_terms + 48 * t:
                                                off_terms + 48 * t + 48])
            d_begin, d_end, p_begin = te[0], te[1], te[2]
            docs = self.postings[t][0]
            recs = []
            for i, bi in enumerate(range(d_begin, d_end)):
                d = struct.unpack("<IIIIHHII", blob[off_desc + 28 * bi:
                                                    off_desc + 28 * bi + 28])
                prev, last, doc_off, freq_off, length, flags, mf, mn = d
                base = off_payload + p_begin
                dtag = blob[base + doc_off]
                ftag = blob[base + freq_off]
                fused = flags & 1
                nsz = 1 + 16 * ((flags >> 6) & 31) if fused else flags >> 1
                ntag = blob[base + freq_off + nsz]
                recs.append(dict(
                    prev=prev, last=last, len=length, flags=flags,
                    fused=fused, dtag=dtag, ftag=ftag, ntag=ntag,
                    first=int(docs[BLOCK * i]), max_freq=mf, min_norm=mn))
            out.append(recs)
        return out


def _build():
    rng = np.random.default_rng(SEED)
    m = Matrix()
    norms = rng.integers(1, 1 << 12, DOC_COUNT + 1).astype(np.uint32)
    norms[0] = 0

    def plain_freqs(n):
        return rng.integers(1, 16, n).astype(np.uint32)

    # -- freq width 2..31: all in the same low doc range so the terms share
    # docs (term-major accumulation); one pinned value per full block
    for w in FREQ_WIDTHS:
        n = 3 * BLOCK + 50
        docs = _walk(rng, int(rng.integers(0, 50)), n, 4, 19)
        freqs = _small(rng, w, n)
        for blk in range(3):
            freqs[BLOCK * blk + int(rng.integers(0, BLOCK))] = _pin(rng, w)
        m.add(f"fw{w}", docs, freqs)

    # -- norm width 2..31: each in its own doc-id region whose norms are
    # written for the purpose
    for w in NORM_WIDTHS:
        base = 10_000 + (w - 2) * 6000
        norms[base:base + 6000] = _small(rng, w, 6000)
        n = 3 * BLOCK + 50
        docs = _walk(rng, base + int(rng.integers(0, 50)), n, 4, 19)
        assert docs[-1] < base + 6000
        for blk in range(3):
            norms[docs[BLOCK * blk + int(rng.integers(0, BLOCK))]] = \
                _pin(rng, w)
        m.add(f"nw{w}", docs, plain_freqs(n))

    # -- doc-gap width 2..24: one gap per full block pins the width; the
    # other gaps are drawn large enough that bitpack beats the bitset
    for w in DOC_WIDTHS:
        hi_g = min((1 << w) - 1, 31)
        lo_g = (hi_g + 1) // 2
        n = 2 * BLOCK + 40
        gaps = rng.integers(lo_g, hi_g + 1, n).astype(np.int64)
        start = int(rng.integers(200_000, 260_000))
        for blk in range(2):
            pin = (int(rng.integers(1 << (w - 1), 1 << w)) if w <= 21
                   else (1 << (w - 1)) + int(rng.integers(0, 1 << 16)))
            if start + int(gaps.sum()) + pin > DOC_COUNT - 100_000:
                break   # width 24: only one such gap fits the doc space
            gaps[BLOCK * blk + int(rng.integers(0, BLOCK))] = pin
        m.add(f"dw{w}", start + np.cumsum(gaps), plain_freqs(n))

    # -- doc families
    n = 2 * BLOCK + 40
    m.add("same8", 7 * np.arange(1, n + 1), plain_freqs(n))
    m.add("same16", 300 * np.arange(1, n + 1), plain_freqs(n))
    m.add("same32", 100_000 * np.arange(1, 21), plain_freqs(20))
    m.add("bitset", np.sort(rng.choice(np.arange(400_000, 401_000), 700,
                                       replace=False)), plain_freqs(700))
    m.add("svb_tail", _walk(rng, 0, 63, 256, 1000), plain_freqs(63))
    m.add("dsvb_tail", _walk(rng, 1_000_000, 63, 1, 200), plain_freqs(63))
    m.add("values2", [70_000, 200_001], [3, 9])
    full = _walk(rng, 500_000, BLOCK, 4, 19)
    m.add("values2_after",
          np.concatenate([full, [full[-1] + 70_000, full[-1] + 210_001]]),
          plain_freqs(BLOCK + 2))

    # -- freq families (docs and norms ordinary)
    big = lambda: (1 << 31) | (int(rng.integers(0, 1 << 16)) << 8)
    for i, (name, val) in enumerate((("f_same8", 3), ("f_same16", 1000),
                                     ("f_same32", 100_000))):
        n = 2 * BLOCK + 30
        m.add(name, _walk(rng, 450_000 + 10_000 * i, n, 4, 19),
              np.full(n, val))
    n = 2 * BLOCK + 2
    freqs = plain_freqs(n)
    freqs[17], freqs[BLOCK + 99] = big(), big()
    freqs[-2:] = [1 << 31, 70_000]           # 2-value tail: VALUES too
    m.add("f_values", _walk(rng, 480_000, n, 4, 19), freqs)

    # -- norm families: constant-norm regions give all-same norm streams
    for i, (name, val) in enumerate((("n_same8", 5), ("n_same16", 1000),
                                     ("n_same32", 100_000))):
        base = 600_000 + 10_000 * i
        norms[base:base + 6000] = val
        n = 2 * BLOCK + 30
        m.add(name, _walk(rng, base, n, 4, 19), plain_freqs(n))
    n = 2 * BLOCK + 2
    docs = _walk(rng, 630_000, n, 4, 19)
    norms[docs[40]], norms[docs[BLOCK + 3]] = big(), big()
    norms[docs[-2]], norms[docs[-1]] = 1 << 31, 70_000
    m.add("n_values", docs, plain_freqs(n))

    # -- tail lengths, after full blocks and as a term's only block, placed
    # at window boundaries so some blocks straddle one and some do not
    for i, length in enumerate(TAIL_LENGTHS):
        n = 2 * BLOCK + length
        m.add(f"tail_after{length}",
              _walk(rng, WIN * (30 + i) - 300, n, 1, 12), plain_freqs(n))
        m.add(f"tail_only{length}",
              _walk(rng, WIN * (40 + i) - 100, length, 4, 19),
              plain_freqs(length))

    # -- 160 blocks whose doc and freq family is drawn per block: fused
    # and non-fused blocks sit next to each other at every wave stride.
    # ~30 blocks fall in each window, so stride-16 pairs share a window.
    docs_parts, freq_parts = [], []
    prev = 1_200_000
    for _ in range(160):
        kind = rng.choice(3, p=[0.6, 0.2, 0.2])
        if kind == 0:
            d = _walk(rng, prev, BLOCK, 1, 12)                # bitpack
        elif kind == 1:
            d = prev + np.cumsum(1 + (rng.random(BLOCK) < 0.3))  # bitset
        else:
            d = prev + int(rng.integers(3, 10)) * np.arange(1, BLOCK + 1)
        fkind = rng.choice(3, p=[0.6, 0.25, 0.15])
        if fkind == 0:
            f = plain_freqs(BLOCK)
        elif fkind == 1:
            f = np.full(BLOCK, 2, dtype=np.uint32)
        else:
            f = plain_freqs(BLOCK)
            f[int(rng.integers(0, BLOCK))] = big()
        docs_parts.append(np.asarray(d, dtype=np.uint32))
        freq_parts.append(f)
        prev = int(d[-1])
    docs_parts.append(_walk(rng, prev, 77, 1, 12))
    freq_parts.append(plain_freqs(77))
    m.add("mixed", np.concatenate(docs_parts), np.concatenate(freq_parts))

    # -- one long term across every window with rare freq spikes: blocks
    # without a spike are all-same freq blocks (non-fused) that block-max
    # pruning can drop once a spike doc sets the threshold
    docs = _walk(rng, 0, DOC_COUNT // 32 - 1000, 24, 40)
    freqs = np.ones(len(docs), dtype=np.uint32)
    freqs[::1009] = 200
    m.add("spiky", docs, freqs)

    # -- 31 sparse terms across the whole doc space: with "spiky" a 32-term
    # plan in which every term bounds every window (a 128-doc block spans
    # ~3.5 windows), the shape where WAND sums and subtracts the most
    # per-term bounds. A few planted docs, one every 12 windows, carry all
    # 31 terms at freq 1000 and norm 1: they are the top hits, their score
    # is close to the summed bound, and windows far from them hold only
    # low-freq, long-norm postings that the bound can really rule out.
    planted = (1 + WIN * 12 * np.arange(44) + 7000).astype(np.uint32)
    wide_docs = []
    for i in range(31):
        docs = np.union1d(rng.choice(DOC_COUNT, 20_000, replace=False) + 1,
                          planted).astype(np.uint32)
        freqs = rng.integers(1, 4, len(docs)).astype(np.uint32)
        freqs[int(rng.integers(0, 997))::997] = 60
        freqs[np.searchsorted(docs, planted)] = 1000
        wide_docs.append(docs)
        m.add(f"wide{i:02d}", docs, freqs)
    # long norms on the wide terms' docs, clear of the regions above whose
    # norms were written on purpose (all below 700 000)
    wd = np.unique(np.concatenate(wide_docs))
    wd = wd[wd >= 700_000]
    norms[wd] = rng.integers(2000, 1 << 12, len(wd))
    norms[planted] = 1

    # -- "edge": WAND at a histogram-bin edge. Workgroup 100 of the 256
    # that the 529 windows are dealt to owns windows 300..302. Doc A (window
    # 300) and doc B (window 302) get BM25 scores a few ulp above the same
    # bin edge, B's the higher; every other posting scores far lower. With
    # k = 1, A locks the threshold at that bin before window 302 is staged,
    # so B's block survives only if its bound (exactly B's score: B holds
    # its block's max freq and min norm) times the slack is not below the
    # bin's float floor: a slack below 1 - ~1e-6 drops the true top hit.
    # The third block is there to be pruned.
    docs = np.concatenate([_walk(rng, WIN * 300 + 1000, BLOCK, 4, 19),
                           _walk(rng, WIN * 302 + 1000, 2 * BLOCK, 4, 19)])
    freqs = np.ones(len(docs), dtype=np.uint32)
    norms[docs] = 4095
    m.add("edge", docs, freqs)
    m.edge_docs = (int(docs[5]), int(docs[BLOCK + 70]))
    (fa, na), (fb_, nb) = _edge_pair(
        len(docs), int(norms[1:].sum(dtype=np.uint64)) - 2 * 4095)
    freqs[5], freqs[BLOCK + 70] = fa, fb_
    norms[docs[5]], norms[docs[BLOCK + 70]] = na, nb
    m.postings[m.idx["edge"]] = (docs, freqs)

    m.norms = norms
    m.ttf = int(norms[1:].sum(dtype=np.uint64))  # BM25 total_term_freq
    m.blob = sa.build_segment(DOC_COUNT, m.postings, norms)

    # OR plans of at most 32 terms that together cover every term
    t = m.terms
    m.groups = {
        "freq_widths": t([f"fw{w}" for w in FREQ_WIDTHS] +
                         ["same8", "spiky"]),
        "norm_widths": t([f"nw{w}" for w in NORM_WIDTHS] +
                         ["same16", "svb_tail"]),
        "doc_widths": t([f"dw{w}" for w in DOC_WIDTHS] +
                        ["same32", "bitset", "dsvb_tail", "values2",
                         "values2_after", "f_same8", "f_same16", "f_same32",
                         "f_values"]),
        "families": t(["n_same8", "n_same16", "n_same32", "n_values",
                       "mixed", "edge"] +
                      [f"tail_after{n}" for n in TAIL_LENGTHS] +
                      [f"tail_only{n}" for n in TAIL_LENGTHS]),
        "wide": t([f"wide{i:02d}" for i in range(31)] + ["spiky"]),
    }
    covered = set()
    for g in m.groups.values():
        assert len(g) <= 32 and len(set(g)) == len(g)
        covered.update(g)
    assert covered == set(range(len(m.names)))
    # 4-term plans: non-fused, tail-only and mixed-family terms, and one of
    # overlapping terms in the low doc range
    m.small_groups = {
        "mixed": t(["mixed", "f_same8", "tail_only63", "fw17"]),
        "spiky": t(["spiky", "n_values", "values2", "dw13"]),
        "overlap": t(["same8", "fw31", "fw2", "svb_tail"]),
        "norms": t(["n_same32", "f_values", "tail_after127", "nw31"]),
    }
    return m


@functools.lru_cache(maxsize=None)
def matrix():
    """The corpus, built once per process."""
    return _build()


def group_boosts(n, seed):
    """Deterministic per-term boosts in [0.25, 4] for an n-term plan."""
    return [float(x) for x in
            np.random.default_rng(seed).uniform(0.25, 4.0, n)]
