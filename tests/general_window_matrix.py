"""General-window matrix: one small segment aimed at what the general window
kernel (topk_window_kernel: min_match > 1, AND, count, match-docs, hybrid,
and min_match 1 under SDB_TOPK_PATH=general) carries from one window of a
workgroup to the next, the counterpart of window_tail_matrix for the sweep
kernel. That kernel's window is a compile-time 24576 docs, so a workgroup
gets a second window only above 6.3M docs unless SDB_WINDOW_GRID clamps the
launch grid. The corpus is ten windows (nine of `win` docs and 300 docs);
the kernel deals ceil(10 / grid) windows to a workgroup: grid 1 runs 10 in
one workgroup, 2 runs 5 + 5, 3 runs 4 + 4 + 2, 4 runs 3 + 3 + 3 + 1, 8 runs
2 each in five workgroups and leaves three without a window. At grid 1
windows 0 and 1 derive the threshold (the first-window recount, a derive
right after it), 2 and 3 do not, 4 derives without being the first, 5 to 7
are three non-derive windows in a row, 8 derives, 9 has 300 docs.

The builder takes the window width (window_tail_matrix's is tied to the
sweep geometry and has no min-match shapes, so this is a sibling, not a
parameter of it); the suite uses 24576 alone.

The kernel reads its u8 match counts a 32-bit word at a time, so the first
and the last four docs of every window (lo .. lo + 3, hi - 3 .. hi) are a
zone no random draw touches. What is planted there:

  lo, hi        the window edge: in `bg`, `bg2`, `early` and every filler,
                so in all 32 terms of `wide32` (doc 1 is not in `dense`: 31),
  lo + 1, hi - 1  `near`: in exactly one of `bg` / `bg2`, alternating,
  lo + 2, hi - 2  a decoy in some windows,
  lo + 3, hi - 3  in windows 0-3 a doc of all five `main` terms.

Terms:

  * `bg`, `bg2`: one doc in nine each and every window edge; their
    intersection gives AND and min-match-2 matches in every window and on
    every edge.
  * `near`: lo + 1 and hi - 1 of every window. Under `main` and `decoys` at
    min-match 2 these docs match one term, under `near` (bg, bg2, near) and
    `wide32` at min-match 3 two: min_match - 1 next to every edge, in the
    count word of an edge doc that does match.
  * `early`: six top scores in window 0, two in windows 5 and 8 (freq 250,
    norm 1), about 50 quiet docs per window (freq 1, norm 1000), the edges
    and the five-term docs. Every `early` doc is a `bg` doc, so the spikes
    match at min-match 2. With k = 3 the threshold locks in window 0;
    windows 1-4, 6, 7 and 9 then hold matches but no candidate, each run
    followed by a window with candidates.
  * `decoy`: 40 docs of freq 250 and norm 1 that are in no other term of the
    plan that uses them (bg, bg2, decoy): 31 in window 0, lo + 2 of windows
    1-4, hi - 2 of windows 4-7, one in the last window. The edges themselves
    are in `bg` and `bg2` by construction, so "on the edge" is the edge's
    count word here. Under min-match 2 they are no matches, yet each scores
    above every match: a kernel that lets a doc with count < min_match into
    the histogram, the candidate count or the append is caught. Under
    min-match 3 the plan has no match at all, and thousands of docs with
    count 2, every edge among them.
  * `hole`: one block over windows 0-1, the next starts in window 3: window
    2 is a single item without a posting. `ends_mid` ends in the middle of
    window 3, `ends_on_hi` on window 4's hi. A third of each is in `bg`.
  * `dense`: every doc from 2 on, 192 blocks per window (six times the 32
    staged descriptors), a block across every window edge.
  * `f00` .. `f27`: about 200 docs each and the edges; with bg, bg2, dense
    and early the 32-term plan, at which the descriptor stage shrinks to 14.

The raw (docs, freqs) arrays and the norms column are the ground truth; the
references never decode the blob."""

import functools

import numpy as np

import codec_matrix as cm
import round_stage_matrix as rs
import serenedb_amd as sa

BLOCK = cm.BLOCK
WIN = cm.WIN                           # SDB_WIN_DOCS
NWIN = 10
TAIL = 300                             # docs of the last window
DOC_COUNT = 9 * WIN + TAIL
SEED = 0x6E57A11
GRIDS = (1, 2, 3, 4, 8, None)          # None: SDB_WINDOW_GRID unset
SPIKE_FREQ, SPIKE_NORM, QUIET_NORM = 250, 1, 1000
SPIKES = {0: 6, 5: 2, 8: 2}            # window -> top-scoring docs of `early`
DEAD_SPIKE_WINDOWS = (0, 5)            # their spikes are dead under the mask
QUIET = (1, 2, 3, 4, 6, 7, 9)
NDECOY = 40
NFILL = 28
HIST_BINS = 256                        # SDB_HIST_BINS
LIVE_K = 5
F = np.float32


# ---- the kernel's dealing, restated ---------------------------------------
def split(grid, nwin=NWIN):
    """windows per workgroup: per = ceil(nwin / grid), w_lo = b * per"""
    per = -(-nwin // grid)
    return [max(0, min(nwin, (b + 1) * per) - b * per) for b in range(grid)]


def runs(grid, nwin=NWIN):
    """(w_lo, w_hi) of every workgroup that has a window"""
    per = -(-nwin // grid)
    return [(b * per, min(nwin, (b + 1) * per)) for b in range(grid)
            if b * per < nwin]


def derive_windows(w_lo, w_hi):
    return [w for w in range(w_lo, w_hi) if w % 4 == 0 or w < w_lo + 2]


def bounds(win=WIN):
    """(lo[10], hi[10]) of the windows"""
    los = 1 + win * np.arange(NWIN, dtype=np.int64)
    his = np.minimum(los + win - 1, 9 * win + TAIL)
    return los, his


def window_of(docs, win=WIN):
    return (np.asarray(docs, dtype=np.int64) - 1) // win


# ---- the corpus -----------------------------------------------------------
class GeneralMatrix(rs.RoundMatrix):
    win = WIN
    doc_count = DOC_COUNT

    def ref_topk_live(self, terms, boosts, k, scorer, min_match, live):
        """ref_topk with the docs where live[doc] is False invisible"""
        u, s, cnt, _ = self.ref_scores(terms, boosts, scorer)
        sel = (cnt >= min_match) & live[u]
        return _rank(u[sel], s[sel], k) + (int(sel.sum()),)

    def ref_count(self, terms, min_match, live=None):
        return len(self.ref_stream(terms, min_match, live))

    def ref_stream(self, terms, min_match, live=None):
        """every match, docs ascending"""
        u, _, cnt, _ = self.ref_scores(terms, [1.0] * len(terms), "bm25")
        sel = cnt >= min_match
        if live is not None:
            sel &= live[u]
        return u[sel]

    # ---- the histogram's score bins, as the kernel computes them --------
    def smax(self, terms, boosts):
        """the plan's BM25 score bound (prep_plan_stats): the fp32 sum of
        the terms' num = boost * (k1 + 1) * idf in plan order"""
        out = F(0.0)
        for t, boost in zip(terms, boosts):
            df = len(self.postings[t][0])
            idf = F(np.log1p((np.float64(self.doc_count - df) + 0.5) /
                             (np.float64(df) + 0.5)))
            num = F(boost) * (F(1.2) + F(1.0)) * idf
            if num > 0:
                out = F(out + num)
        return out

    def bins(self, terms, boosts, scores):
        """score_bin: (u32)(s * (256 / smax)), capped at 255"""
        inv = F(HIST_BINS) / self.smax(terms, boosts)
        x = (np.asarray(scores, dtype=F) * inv).astype(np.uint32)
        return np.minimum(x, HIST_BINS - 1)

    # ---- wrong on purpose ------------------------------------------------
    def binned_topk(self, terms, boosts, k, min_match, live=None,
                    counted="matches", accept=None):
        """What a kernel returns whose histogram counts the docs `counted`
        and whose candidates are the docs `accept` (default: the live
        matches) in a bin at or above the k-th counted one. counted =
        "matches" with the default accept is the true result (the CPU test
        proves it equals ref_topk); "any_term" counts every doc with a
        posting, "with_dead" the dead matches too."""
        u, s, cnt, _ = self.ref_scores(terms, boosts, "bm25")
        alive = np.ones(len(u), dtype=bool) if live is None else live[u]
        match = (cnt >= min_match) & alive
        hist_docs = {"matches": match, "any_term": (cnt >= 1) & alive,
                     "with_dead": cnt >= min_match}[counted]
        b = self.bins(terms, boosts, s)
        suffix = np.cumsum(np.bincount(b[hist_docs],
                                       minlength=HIST_BINS)[::-1])[::-1]
        reach = np.flatnonzero(suffix >= k)
        tb = int(reach.max()) if len(reach) else 0
        sel = (match if accept is None else accept) & (b >= tb)
        return _rank(u[sel], s[sel], k) + (int(match.sum()),)

    def wrong(self, kind, terms, boosts, k, min_match, live=None, grid=1):
        """the five wrong references of the issue, (docs, scores, total)"""
        u, s, cnt, _ = self.ref_scores(terms, boosts, "bm25")
        if kind == "decoys_counted":
            return self.binned_topk(terms, boosts, k, min_match, live,
                                    counted="any_term")
        if kind == "dead_counted":
            return self.binned_topk(terms, boosts, k, min_match, live,
                                    counted="with_dead")
        if kind == "mm_minus_1":
            return self.ref_topk(terms, boosts, k, "bm25",
                                 max(min_match - 1, 1))
        if kind == "edges_dropped":
            sel = (cnt >= min_match) & ~np.isin(u, self.edges)
            return _rank(u[sel], s[sel], k) + (int(sel.sum()),)
        if kind == "no_recount_total":
            d, sc, total = self.ref_topk(terms, boosts, k, "bm25", min_match)
            w = window_of(u[cnt >= min_match], self.win)
            firsts = [lo for lo, _ in runs(grid)]
            return d, sc, total + int(np.isin(w, firsts).sum())
        raise KeyError(kind)


def _rank(u, s, k):
    keep = s > cm.FLT_MIN
    u, s = u[keep], s[keep]
    order = np.lexsort((u, -s))[:k]
    return u[order], s[order]


def live_mask(m):
    """~1/4 of the docs dead, window edges dead and alive; every `early`
    spike of windows 0 and 5 dead, those of window 8 alive"""
    win = m.win
    d = np.arange(m.doc_count + 1, dtype=np.uint64)
    h = (d * np.uint64(0x9E3779B1)) & np.uint64(0xFFFFFFFF)
    live = ((h >> np.uint64(11)) & np.uint64(3)) != 0
    live[0] = True
    live[[win, 4 * win + 1, 9 * win]] = False
    live[[win + 1, 4 * win, 9 * win + 1]] = True
    sw = window_of(m.spikes, win)
    live[m.spikes[np.isin(sw, DEAD_SPIKE_WINDOWS)]] = False
    live[m.spikes[~np.isin(sw, DEAD_SPIKE_WINDOWS)]] = True
    live.setflags(write=False)
    return live


def live_words(m, live):
    nwords = (m.doc_count + 64) // 64
    b = np.ones(nwords * 64, dtype=np.uint8)
    b[:m.doc_count + 1] = live
    return np.packbits(b, bitorder="little").view(np.uint64)


def _build(win):
    dc = 9 * win + TAIL
    rng = np.random.default_rng(SEED)
    norms = rng.integers(1, 1 << 10, dc + 1).astype(np.uint32)
    norms[0] = 0
    m = GeneralMatrix()
    m.win, m.doc_count = win, dc
    los, his = bounds(win)
    edges = np.unique(np.concatenate([los, his]))
    near = np.concatenate([los + 1, his - 1])
    end_mid = 3 * win + win // 2

    # what no random draw may take: the count words of the window edges,
    # the planted ends, and every planted doc once it is placed
    free = np.ones(dc + 1, dtype=bool)
    free[0] = False
    for lo, hi in zip(los, his):
        free[lo:lo + 4] = False
        free[hi - 3:hi + 1] = False
    free[end_mid] = False

    def sample(n, lo, hi, take=False):
        pool = lo + np.flatnonzero(free[lo:hi + 1])
        out = np.sort(rng.choice(pool, n, replace=False))
        if take:
            free[out] = False
        return out

    def freqs(n):
        return rng.integers(1, 30, n).astype(np.uint32)

    # -- decoys: in no term but `dense`
    decoy = np.concatenate([sample(31, 100, win - 100, take=True),
                            los[1:5] + 2, his[4:8] - 2,
                            sample(1, int(los[9]) + 10, dc - 10, take=True)])
    decoy = np.sort(decoy)
    assert len(decoy) == NDECOY
    norms[decoy] = SPIKE_NORM

    # -- docs of all five `main` terms: windows 0-3, before ends_mid's end
    all5 = np.concatenate(
        [los[0:4] + 3, his[0:3] - 3] +
        [sample(10, int(los[w]) + 4, min(int(his[w]) - 4, end_mid - 1),
                take=True) for w in range(4)])
    all5 = np.sort(all5)

    # -- early: spikes and ~50 quiet docs per window, the edges, all5
    spikes, quiet = [], []
    for w in range(NWIN):
        ns = SPIKES.get(w, 0)
        pool = sample(50 + ns, int(los[w]) + 4, int(his[w]) - 4, take=True)
        mask = np.zeros(len(pool), dtype=bool)
        mask[rng.permutation(len(pool))[:ns]] = True
        spikes.append(pool[mask])
        quiet.append(pool[~mask])
    spikes = np.concatenate(spikes)
    quiet = np.unique(np.concatenate(quiet + [edges, all5]))
    early = np.union1d(spikes, quiet)
    f_early = np.ones(len(early), dtype=np.uint32)
    f_early[np.searchsorted(early, spikes)] = SPIKE_FREQ
    norms[quiet] = QUIET_NORM
    norms[spikes] = SPIKE_NORM

    hole = np.concatenate([sample(BLOCK, 100, 2 * win - 100),
                           sample(BLOCK + 40, 3 * win + 5, dc - 4)])
    ends_mid = np.union1d(np.append(sample(300, 5, end_mid - 1), end_mid),
                          all5)
    ends_on_hi = np.union1d(
        np.append(sample(2 * BLOCK + 17, 5, 5 * win - 4), 5 * win), all5)

    # -- bg holds every early doc, a third of hole / ends_*, half of near
    bg = np.unique(np.concatenate([
        sample(dc // 9, 1, dc), edges, early, all5, near[0::2], hole[::3],
        ends_mid[::3], ends_on_hi[::3], [end_mid]]))
    bg2 = np.unique(np.concatenate([sample(dc // 9, 1, dc), edges, all5,
                                    near[1::2]]))
    # a spike's bg posting is a spike as well: all ten score alike under
    # every plan and share a histogram bin, the top one
    f_bg = freqs(len(bg))
    f_bg[np.searchsorted(bg, spikes)] = SPIKE_FREQ
    m.add("bg", bg, f_bg)
    m.add("bg2", bg2, freqs(len(bg2)))
    m.add("near", np.sort(near), freqs(len(near)))
    m.add("early", early, f_early)
    m.add("decoy", decoy, np.full(NDECOY, SPIKE_FREQ, dtype=np.uint32))
    m.add("hole", hole, freqs(len(hole)))
    m.add("ends_mid", ends_mid, freqs(len(ends_mid)))
    m.add("ends_on_hi", ends_on_hi, freqs(len(ends_on_hi)))
    dense = np.arange(2, dc + 1)
    m.add("dense", dense, freqs(len(dense)))
    for i in range(NFILL):
        docs = np.union1d(sample(200, 1, dc), edges)
        m.add(f"f{i:02d}", docs, freqs(len(docs)))

    norms.setflags(write=False)
    m.norms = norms
    m.ttf = int(norms[1:].sum(dtype=np.uint64))
    m.edges, m.near, m.spikes, m.decoys, m.all5 = (edges, np.sort(near),
                                                   spikes, decoy, all5)
    for a in (m.edges, m.near, m.spikes, m.decoys, m.all5):
        a.setflags(write=False)
    # the column execute_match_docs gathers
    m.column = rng.integers(-(1 << 40), 1 << 40, dc + 1, dtype=np.int64)
    m.column.setflags(write=False)
    m.blob = sa.build_segment(dc, m.postings, norms)
    t = m.terms
    m.groups = {
        "main": t(["bg", "bg2", "early", "ends_mid", "ends_on_hi"]),
        "decoys": t(["bg", "bg2", "decoy"]),
        "early": t(["early", "bg"]),
        "hole": t(["hole", "bg"]),
        "ends": t(["ends_on_hi", "ends_mid", "bg"]),
        "dense": t(["dense", "bg"]),
        "near": t(["bg", "bg2", "near"]),
        "wide32": t(["bg", "bg2", "dense", "early"] +
                    [f"f{i:02d}" for i in range(NFILL)]),
    }
    assert len(m.groups["wide32"]) == 32
    return m


@functools.lru_cache(maxsize=None)
def matrix(win=WIN):
    return _build(win)


# ---- the named cases ------------------------------------------------------
AND = "and"     # min_match = number of terms
# plan -> ((min_match, k values), ...); "n" is the number of matches at that
# min_match, "n+7" seven more (the threshold never rises: every match is a
# candidate in every window)
PLAN_CASES = (
    ("main", ((1, (1, 3, 10, 1000, "n", "n+7")),
              (2, (1, 3, 10, 1000, "n", "n+7")),
              (3, (1, 3, 10, 1000, "n", "n+7")),
              (AND, (1, 3, 10, 1000, "n", "n+7")))),
    # at min-match 3 no doc matches (a decoy is in neither bg nor bg2)
    ("decoys", ((2, (1, 3, 10, NDECOY, 1000, "n", "n+7")),
                (3, (1, 10, "n+7")))),
    ("early", ((1, (3,)), (AND, (3, 10, "n")))),
    ("hole", ((1, (5,)), (AND, (5, "n+7")))),
    ("ends", ((1, (10,)), (2, (10, "n")), (AND, (10, "n+7")))),
    ("dense", ((1, (10,)), (AND, (1, 10, 1000, "n", "n+7")))),
    # at AND no doc matches (a near doc is in one of bg / bg2); the near
    # docs have count 2 there, the edges beside them too
    ("near", ((2, (10, "n")), (AND, (3, 10, "n+7")))),
    ("wide32", ((1, (10,)), (3, (3, 10, 1000, "n+7")),
                (AND, (1, 10, "n", "n+7")))),
)


def n_matches(m, terms, min_match):
    return m.ref_count(terms, min_match)


def cases(m):
    """(label, terms, boosts, min_match, k)"""
    out = []
    for g, per_mm in PLAN_CASES:
        terms = m.groups[g]
        boosts = rs.boosts_for(terms)
        for mm, ks in per_mm:
            mm_ = len(terms) if mm == AND else mm
            n = n_matches(m, terms, mm_)
            for k in ks:
                kk = {"n": n, "n+7": n + 7}.get(k, k)
                assert kk >= 1, (g, mm, k)
                out.append((f"{g} mm={mm_} k={kk}", terms, boosts, mm_, kk))
    return out


def live_cases(m):
    """(label, terms, boosts, min_match, spikes match): min-match 1 (the
    general path by SDB_TOPK_PATH), 2 and AND, each at k = LIVE_K and
    k = doc_count"""
    main, early = m.groups["main"], m.groups["early"]
    # under boosts_for a five-term doc outscores a spike (ends_on_hi gets
    # 1.9); here `early` dominates, so the spikes are main's top scorers
    boosts = [1.0, 0.37, 2.5, 0.11, 0.19]
    return [("main mm=1", main, boosts, 1, True),
            ("main mm=2", main, boosts, 2, True),
            ("main and", main, boosts, len(main), False),
            ("early and", early, rs.boosts_for(early), 2, True)]


def count_cases(m):
    """(label, terms, min_match): OR, 2, 3 and AND of main, decoys, dense
    and wide32 (dense has two terms: OR and AND)"""
    out = []
    for g in ("main", "decoys", "dense", "wide32"):
        terms = m.groups[g]
        for mm in sorted({1, 2, min(3, len(terms)), len(terms)}):
            out.append((f"{g} mm={mm}", terms, mm))
    return out
