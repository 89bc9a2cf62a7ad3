"""Round-stage matrix: one small segment aimed at how the sweep kernel
numbers a window's blocks as items, decodes them in rounds into its LDS
posting stage and merges the stage term by term, not at which block
families or scorers exist (codec_matrix, block_fetch_matrix and
scorer_matrix cover those). What can go wrong there is

  * a window whose item count is one under, exactly, one over and several
    times the stage capacity C: under SDB_SWEEP_ROUND_ITEMS=NW (C = 4 at
    4096x256, the one capacity every launch can be clamped to) the windows
    of the `edges`, `steer`, `first_empty` and `mixed` plans hold 3, 4, 5,
    7, 8, 9, 10 and 40 items,
  * a round boundary inside a term, next to a doc that later terms match
    as well (every block of term `a` holds docs of every steer term),
  * the fp32 add order on a doc matched by every term (unequal boosts),
  * blocks that straddle a window edge or touch it exactly (`edge`: a block
    ending on hi, the next starting on lo; `sparse`: a block wider than a
    window), a term without a posting in the middle window (`gap`), a term
    without an item in the later windows (`w0only`),
  * non-fused blocks next to fused pairs in one round (`one_tail`'s 1-doc
    tail, `w0only`'s 5-doc tail, the `dense` term's blocks), a pair formed
    across a term boundary,
  * a term denser than the descriptor cache is deep (`dense`: every doc from
    2 on, 33 blocks in a 4096-doc window, 192 in a 24576-doc one),
  * a 32-term plan, which shrinks the descriptor cache and C,
  * WAND-pruned items inside a round: pruning needs a threshold from an
    earlier window of the same workgroup, so it has a corpus of its own
    (wand_matrix(): 12M docs, 2930 windows of 4096 or 489 of 24576, more
    than any grid, three terms whose rare freq spikes set the threshold).

The corpus is 3 windows of 4096 docs (the smallest compiled sweep geometry,
4 waves) plus 300. The raw (docs, freqs) arrays and the norms column are the
ground truth; the references never decode the blob."""

import functools

import numpy as np

import block_fetch_matrix as bf
import codec_matrix as cm
import serenedb_amd as sa

BLOCK = cm.BLOCK
WIN = 4096                 # docs per window at SDB_SWEEP_GEOM=4096x256
GEOM = "4096x256"
NW = 4                     # waves of that geometry: the smallest C
DOC_COUNT = 3 * WIN + 300
SEED = 0x524F554E
DCACHE = 32                # descriptors staged per term (SDB_DESC_CACHE)
STEER = ("a", "b", "c", "d")
STEER_BOOSTS = (1.0, 0.37, 2.5, 0.11)
assert DOC_COUNT <= cm.DOC_COUNT   # Matrix.add checks against the larger


def default_c(nterms, win=WIN, nth=256, hybrid=False):
    """the stage capacity the host picks when nothing clamps it
    (plan_sweep_lds in sdb_gpu.hip, mirrored): a slot per 512 window docs
    plus one per term, within what 160 KB leave next to the other arrays
    without costing a resident workgroup. 5 for 4 terms at 4096x256, 42 at
    24576x1024."""
    lds, nw = 163840, nth // 64
    fixed = (win * 4 + win // 8 + nw * 1536 + 1024 + (2 + nw) * 4 + 512 +
             40 * nterms + (2048 if hybrid else 0))

    def total(dn, c):
        return fixed + 28 * dn * nterms + 16 + 768 * c
    dn = DCACHE
    while dn > 1 and total(dn, nw) > lds:
        dn -= 1
    wgs = min(lds // total(dn, nw), 32 // nw)
    fit = (lds // wgs - total(dn, 0)) // 768
    return max(nw, min(win // 512 + nterms, fit))


def deal(items, c, nw=NW):
    """The fused pairs the kernel forms in one window without WAND, as
    (i, i + nw) item index pairs: rounds of c items, wave w takes items
    r0 + w, + nw, ...; two full fused blocks in a row pair up."""
    pairs = []
    for r0 in range(0, len(items), c):
        r1 = min(r0 + c, len(items))
        for w in range(nw):
            i = r0 + w
            while i < r1:
                i2 = i + nw
                if i2 < r1 and all(items[j][1]["fused"] and
                                   items[j][1]["len"] == BLOCK
                                   for j in (i, i2)):
                    pairs.append((i, i2))
                    i = i2 + nw
                else:
                    i = i2
    return pairs


class RoundMatrix(bf.FetchMatrix):
    """Same references as the block-fetch matrix, over this doc count."""

    doc_count = DOC_COUNT

    def ref_scores(self, terms, boosts, scorer, k1=1.2, b=0.75):
        key = (tuple(terms), tuple(float(x) for x in boosts), scorer)
        if key in self._ref_cache:
            return self._ref_cache[key]
        F = np.float32
        u = np.unique(np.concatenate([self.postings[t][0] for t in terms]))
        scores = np.zeros(len(u), dtype=F)
        cnt = np.zeros(len(u), dtype=np.int32)
        fk1, fb = F(k1), F(b)
        nc = fk1 - fk1 * fb
        DOC_COUNT = self.doc_count
        nl = F(fk1 * fb) / (F(self.ttf) / F(DOC_COUNT))
        for t, boost in zip(terms, boosts):
            docs, freqs = self.postings[t]
            df = len(docs)
            at = np.searchsorted(u, docs)
            f = freqs.astype(F)
            nrm = self.norms[docs].astype(F)
            if scorer == "bm25":
                idf = F(np.log1p((np.float64(DOC_COUNT - df) + 0.5) /
                                 (np.float64(df) + 0.5)))
                num = F(boost) * (fk1 + F(1.0)) * idf
                c1 = nc + nl * nrm
                contrib = num - num * c1 / (c1 + f)
            else:
                idf = F(np.log1p((np.float64(DOC_COUNT) + 1.0) /
                                 (np.float64(df) + 1.0)))
                num = F(boost) * idf
                contrib = num * np.sqrt(f)
                if scorer == "tfidf_norm":
                    contrib = contrib / np.sqrt(nrm)
            assert contrib.dtype == F
            scores[at] += contrib   # term-major; docs unique within a term
            cnt[at] += 1
        out = (u, scores, cnt, None)
        self._ref_cache[key] = out
        return out

    def ref_topk_live(self, terms, boosts, k, scorer, live):
        """ref_topk with the docs where live[doc] is False invisible"""
        u, s, _, _ = self.ref_scores(terms, boosts, scorer)
        keep = live[u]
        u, s = u[keep], s[keep]
        total = len(u)
        pos = s > cm.FLT_MIN
        u, s = u[pos], s[pos]
        order = np.lexsort((u, -s))[:k]
        return u[order], s[order], total

    # ---- items, as the kernel numbers them ------------------------------
    def window_items(self, terms, win=WIN, last=None):
        """Per window, the term-major item list [(plan position, block
        record)]: from each term's cursor (first block with last >= lo) the
        blocks with prev < hi."""
        recs, _, _ = self.parse()
        nwin = (self.doc_count + win - 1) // win
        out = []
        for w in range(nwin if last is None else min(nwin, last)):
            lo = 1 + w * win
            hi = min(lo + win - 1, self.doc_count)
            items = []
            for pos, t in enumerate(terms):
                for r in recs[t]:
                    if r["last"] >= lo and r["prev"] < hi:
                        items.append((pos, r))
            out.append(items)
        return out


def live_mask():
    """~1/4 of the docs dead, the window edges among them and next to them"""
    d = np.arange(DOC_COUNT + 1, dtype=np.uint64)
    h = (d * np.uint64(0x9E3779B1)) & np.uint64(0xFFFFFFFF)
    live = ((h >> np.uint64(13)) & np.uint64(3)) != 0
    live[0] = True
    live[[WIN, 2 * WIN + 1]] = False
    live[[WIN + 1, 2 * WIN]] = True
    live.setflags(write=False)
    return live


def live_words(live):
    """as attach_livemask takes it: bit d of word d >> 6, the bits past the
    last doc set"""
    nwords = (DOC_COUNT + 64) // 64
    b = np.ones(nwords * 64, dtype=np.uint8)
    b[:DOC_COUNT + 1] = live
    return np.packbits(b, bitorder="little").view(np.uint64)


def _sample(rng, n, lo=1, hi=DOC_COUNT):
    return np.sort(rng.choice(np.arange(lo, hi + 1), n, replace=False))


def _build():
    rng = np.random.default_rng(SEED)
    norms = rng.integers(1, 1 << 10, DOC_COUNT + 1).astype(np.uint32)
    norms[0] = 0
    m = RoundMatrix()
    edges = np.array([1, WIN, WIN + 1, 2 * WIN, 2 * WIN + 1, 3 * WIN,
                      3 * WIN + 1, DOC_COUNT])

    def freqs(n):
        return rng.integers(1, 30, n).astype(np.uint32)

    # -- the steer plan: about 5 + 2 + 2 + 1 items per window. Every
    # term holds the window edges and two docs of every block of `a`
    a = np.union1d(_sample(rng, 1560), edges)
    shared = np.union1d(a[::64], edges)
    for name, n in (("a", 0), ("b", 300), ("c", 150), ("d", 60)):
        docs = a if name == "a" else np.union1d(_sample(rng, n), shared)
        m.add(name, docs, freqs(len(docs)))

    # -- every doc from 2 on
    docs = np.arange(2, DOC_COUNT + 1)
    m.add("dense", docs, freqs(len(docs)))

    # -- block 0 ends on window 0's hi, block 1 starts on window 1's lo,
    # block 2 ends on window 1's hi, block 3 starts on window 2's lo
    parts = [np.append(_sample(rng, BLOCK - 1, 2000, WIN - 1), WIN),
             np.append(WIN + 1, _sample(rng, BLOCK - 1, WIN + 2, 6000)),
             np.append(_sample(rng, BLOCK - 1, 6001, 2 * WIN - 1), 2 * WIN),
             np.append(2 * WIN + 1,
                       _sample(rng, 40, 2 * WIN + 2, DOC_COUNT))]
    docs = np.concatenate(parts)
    m.add("edge", docs, freqs(len(docs)))

    # -- a block wider than a window: 128 docs over ~6400, then a tail that
    # covers the rest (straddles both edges of window 2)
    docs = np.arange(3, DOC_COUNT, 50)
    m.add("sparse", docs, freqs(len(docs)))

    # -- one block in window 0, then one block and a 2-doc tail in window 2
    docs = np.concatenate([_sample(rng, BLOCK, 1, WIN),
                           _sample(rng, BLOCK + 2, 2 * WIN + 1, DOC_COUNT)])
    m.add("gap", docs, freqs(len(docs)))

    # -- window 0 only: a block and a 5-doc tail
    docs = _sample(rng, BLOCK + 5, 1, WIN - 1)
    m.add("w0only", docs, freqs(len(docs)))

    # -- a full block and a 1-doc tail, the tail in the middle window
    docs = np.append(_sample(rng, BLOCK, 100, WIN + 500), WIN + 900)
    m.add("one_tail", docs, freqs(len(docs)))

    # -- 22 fillers to make a 32-term plan: two blocks and a tail each,
    # over all windows, sharing the edges
    for i in range(22):
        docs = np.union1d(_sample(rng, 2 * BLOCK + 10 + i), edges)
        m.add(f"f{i}", docs, freqs(len(docs)))

    m.norms = norms
    m.ttf = int(norms[1:].sum(dtype=np.uint64))
    m.blob = sa.build_segment(DOC_COUNT, m.postings, norms)
    t = m.terms
    m.groups = {
        "steer": t(STEER),
        # the first term has no item in windows 1 and 2
        "first_empty": t(["w0only", "a", "gap", "b"]),
        "edges": t(["edge", "sparse", "gap", "one_tail"]),
        # non-fused families in one round with fused pairs
        "mixed": t(["a", "one_tail", "w0only", "dense", "b"]),
        "dense2": t(["dense", "a"]),
        "all32": list(range(32)),
    }
    assert len(m.names) == 32
    return m


@functools.lru_cache(maxsize=None)
def matrix():
    return _build()


# ---- the WAND corpus ------------------------------------------------------
WAND_DOCS = 12_000_000
WAND_BOOSTS = (1.0, 0.02, 0.01)
WAND_K = 10


def _build_wand():
    """Three terms on four fifths of every 10th, 20th and 40th doc (about
    8 items per 4096-doc window, 30 per 24576-doc one, nearly all of the
    fused shape), freq 1 or 2 but for rare spikes of 200. Under WAND_BOOSTS the first term's spikes set the top-10
    threshold above the sum of the three terms' plain-block bounds, so in a
    window without a spike every item is pruned, in one with a spike in
    `a` the plain blocks of `a` are, next to decoded ones."""
    rng = np.random.default_rng(SEED + 1)
    m = RoundMatrix()
    m.doc_count = WAND_DOCS
    norms = rng.integers(1, 1 << 10, WAND_DOCS + 1).astype(np.uint32)
    norms[0] = 0
    for name, start, step, spike in (("a", 1, 10, 1009), ("b", 3, 20, 2003),
                                     ("c", 7, 40, 4001)):
        docs = np.arange(start, WAND_DOCS + 1, step, dtype=np.uint32)
        docs = docs[rng.random(len(docs)) < 0.8]   # uneven gaps: bitpacked
        freqs = rng.integers(1, 3, len(docs)).astype(np.uint32)
        freqs[::spike] = 200
        m.add(name, docs, freqs)
    m.norms = norms
    m.ttf = int(norms[1:].sum(dtype=np.uint64))
    m.blob = sa.build_segment(WAND_DOCS, m.postings, norms)
    return m


@functools.lru_cache(maxsize=None)
def wand_matrix():
    return _build_wand()


def boosts_for(terms):
    """unequal boosts, so that the add order shows in the score bits"""
    cyc = STEER_BOOSTS + (1.9, 0.73, 3.1, 0.051)
    return [cyc[i % len(cyc)] for i in range(len(terms))]
