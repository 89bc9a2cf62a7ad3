"""Window-tail matrix: one small segment aimed at what the sweep kernel does
between two windows of one workgroup, not at how a window is decoded
(round_stage_matrix covers that). After a window's sparse sweep the kernel
reserves candidate space, derives the threshold bin on its derive cadence
(a workgroup's first two windows and every window with w % 4 == 0), takes
the next window's threshold snapshot and fetches the next window's item
counts and descriptors from the advanced cursors. Without SDB_SWEEP_GRID a
workgroup runs more than three windows only on tens of millions of docs, so
the corpus is ten windows of 4096 docs (nine and 300 docs) and the grid is
clamped: the kernel deals ceil(10 / grid) windows to a workgroup, so grid 1
runs 10 in one workgroup, 2 runs 5 + 5, 3 runs 4 + 4 + 2, 4 runs 3 + 3 + 3
+ 1, and 8 runs 2 each in five workgroups and leaves three with no window.
At grid 1 windows 0 and 1 derive (the first-window recount, a second derive
directly after it), 2 and 3 do not, 4 derives without being the first, 5 to
7 are three non-derive windows in a row, and window 9 has 300 docs.

What the terms are for:

  * `bg`: matches and candidates in every window,
  * `early`: six top scores in window 0, two more in windows 5 and 8,
    everything else far below: with k = 3 the threshold locks in window 0
    and windows 1-4, 6, 7 and 9 hold matches but no candidate (no
    reservation), each run followed by a window that has candidates,
  * `hole`: one block in windows 0-1, the next one starts in window 3.
    A block is an item of every window between its predecessor's last doc
    and its own, so a middle window cannot be without any item; window 2
    is the nearest thing, a single item without a posting in it, followed
    by a window with candidates. Windows with no item at all are the ones
    behind a plan's last doc (`ends_mid` alone: windows 4-9; at grid 2 the
    second workgroup never sees an item),
  * `ends_mid`: ends in window 3, nothing to stage for the later windows,
  * `ends_on_hi`: its last doc is window 4's hi,
  * `dense`: every doc from 2 on, 33 blocks in a 4096-doc window (past the
    32 staged descriptors), 192 and 99 in the two 24576-doc ones (several
    ballots in the count loop), a block across every window edge.

The raw (docs, freqs) arrays and the norms column are the ground truth; the
references never decode the blob."""

import functools

import numpy as np

import codec_matrix as cm
import round_stage_matrix as rs
import serenedb_amd as sa

BLOCK = cm.BLOCK
WIN = rs.WIN
GEOM = rs.GEOM
NW = rs.NW
NWIN = 10
DOC_COUNT = 9 * WIN + 300
SEED = 0x7A11
GRIDS = (1, 2, 3, 4, 8, None)          # None: SDB_SWEEP_GRID unset
SPIKE_FREQ, SPIKE_NORM, QUIET_NORM = 250, 1, 1000
SPIKES = {0: 6, 5: 2, 8: 2}            # window -> top-scoring docs of `early`
QUIET = (1, 2, 3, 4, 6, 7, 9)


def split(grid, nwin=NWIN):
    """windows per workgroup as the kernel deals them"""
    per = -(-nwin // grid)
    return [max(0, min(nwin, (b + 1) * per) - b * per) for b in range(grid)]


def derive_windows(w_lo, w_hi):
    return [w for w in range(w_lo, w_hi) if w % 4 == 0 or w < w_lo + 2]


def window_of(docs):
    return (np.asarray(docs, dtype=np.int64) - 1) // WIN


class TailMatrix(rs.RoundMatrix):
    doc_count = DOC_COUNT


def live_mask():
    """~1/4 of the docs dead, window edges among them and next to them"""
    d = np.arange(DOC_COUNT + 1, dtype=np.uint64)
    h = (d * np.uint64(0x9E3779B1)) & np.uint64(0xFFFFFFFF)
    live = ((h >> np.uint64(11)) & np.uint64(3)) != 0
    live[0] = True
    live[[WIN, 4 * WIN + 1, 9 * WIN]] = False
    live[[WIN + 1, 4 * WIN, 9 * WIN + 1]] = True
    live.setflags(write=False)
    return live


def live_words(live):
    nwords = (DOC_COUNT + 64) // 64
    b = np.ones(nwords * 64, dtype=np.uint8)
    b[:DOC_COUNT + 1] = live
    return np.packbits(b, bitorder="little").view(np.uint64)


def _build():
    rng = np.random.default_rng(SEED)
    norms = rng.integers(1, 1 << 10, DOC_COUNT + 1).astype(np.uint32)
    norms[0] = 0
    m = TailMatrix()
    edges = np.concatenate([[1], WIN * np.arange(1, NWIN),
                            WIN * np.arange(1, NWIN) + 1, [DOC_COUNT]])

    def sample(n, lo, hi):
        return np.sort(rng.choice(np.arange(lo, hi + 1), n, replace=False))

    def freqs(n):
        return rng.integers(1, 30, n).astype(np.uint32)

    docs = np.union1d(sample(DOC_COUNT // 9, 1, DOC_COUNT), edges)
    m.add("bg", docs, freqs(len(docs)))

    # -- early: the spikes and 50 quiet docs per window, none on an edge
    spikes, quiet = [], []
    for w in range(NWIN):
        lo = 2 + w * WIN
        hi = min(lo + WIN - 3, DOC_COUNT - 1)
        pool = sample(min(50, hi - lo) + SPIKES.get(w, 0), lo, hi)
        pick = rng.permutation(len(pool))[:SPIKES.get(w, 0)]
        mask = np.zeros(len(pool), dtype=bool)
        mask[pick] = True
        spikes.append(pool[mask])
        quiet.append(pool[~mask])
    spikes, quiet = np.concatenate(spikes), np.concatenate(quiet)
    docs = np.union1d(spikes, quiet)
    f = np.ones(len(docs), dtype=np.uint32)
    f[np.searchsorted(docs, spikes)] = SPIKE_FREQ
    norms[spikes] = SPIKE_NORM
    norms[quiet] = QUIET_NORM
    m.add("early", docs, f)
    m.spikes = spikes

    # -- hole: a full block over windows 0-1, then from window 3 on
    docs = np.concatenate([sample(BLOCK, 100, 2 * WIN - 100),
                           sample(BLOCK + 40, 3 * WIN + 1, DOC_COUNT)])
    m.add("hole", docs, freqs(len(docs)))

    docs = np.append(sample(300, 1, 3 * WIN + 2000), 3 * WIN + 2001)
    m.add("ends_mid", docs, freqs(len(docs)))

    docs = np.append(sample(2 * BLOCK + 17, 1, 5 * WIN - 1), 5 * WIN)
    m.add("ends_on_hi", docs, freqs(len(docs)))

    docs = np.arange(2, DOC_COUNT + 1)
    m.add("dense", docs, freqs(len(docs)))

    norms.setflags(write=False)
    m.norms = norms
    m.ttf = int(norms[1:].sum(dtype=np.uint64))
    m.blob = sa.build_segment(DOC_COUNT, m.postings, norms)
    t = m.terms
    m.groups = {
        "main": t(["bg", "early", "ends_mid", "ends_on_hi"]),
        "early": t(["early"]),
        "hole": t(["hole"]),
        "ends_mid": t(["ends_mid"]),
        "ends": t(["ends_on_hi", "ends_mid"]),
        "dense": t(["dense", "bg"]),
    }
    return m


@functools.lru_cache(maxsize=None)
def matrix():
    return _build()


def n_matches(m, terms):
    return len(np.unique(np.concatenate([m.postings[t][0] for t in terms])))


def cases(m):
    """(label, terms, boosts, k): the plans and the k edges. k = 1000 and
    k above the match total (the threshold never rises: every match is a
    candidate in every window) run on the plans with that many matches."""
    out = []
    for g, ks in (("main", (10, 1, 1000, None)), ("early", (3,)),
                  ("hole", (5,)), ("ends_mid", (10,)), ("ends", (10, None)),
                  ("dense", (10, 1000))):
        terms = m.groups[g]
        for k in ks:
            kk = n_matches(m, terms) + 7 if k is None else k
            out.append((f"{g} k={kk}", terms, rs.boosts_for(terms), kk))
    return out
