"""Hybrid top-k filter matrix: the inputs and an exact reference for BM25
top-k AND pushed column predicates with per-bucket COUNT / SUM
(sdb_gpu_execute_topk_hybrid, _chain, _batch). tests/test_hybrid_matrix.py
proves this file on the CPU; tests/test_gpu_hybrid_matrix.py runs every GPU
path against it.

Segment   49281 docs = two full 24576-doc windows and a partial third that
          ends one doc into a new 64-bit match word. Term A is every 3rd doc,
          term B every 7th (docs = 1 mod 7), term C exactly the first and last
          doc of every window and the segment's last two docs. A second
          segment of 129 docs has its own postings and column.
Live mask deterministic, about 1/4 dead; of each pair of docs straddling a
          window boundary exactly one is dead; term C keeps four live docs.
Spans     CASES: (lo, hi, nbuckets), from the ordinary one to the full int64
          range, where hi - lo + 1 = 2^64 and (v - lo) * nbuckets needs 71
          bits.
Columns   the bucket column of a case is laid out by doc, not drawn: every
          edge value (around lo and hi, INT64_MIN / MAX, the first value of
          every bucket and the value below it) sits on a "holder", a live doc
          that matches at min_match 2 and so on every path. Dead and
          non-matching docs hold values inside [lo, hi]: a kernel that
          ignored the mask or the match word would count them.
Reference Python integers over the postings and the columns:
          bucket = (v - lo) * nb // (hi - lo + 1); counts per bucket; sums per
          bucket reduced mod 2^64 and read as int64. Nothing here asks the
          oracle or the library for a bucket, a count, a sum or a survivor.
Hits      the expected hits are the full unfiltered ranking cut down to the
          survivors. ranking() takes it from the oracle's plain top-k (pinned
          bit-exact by the postings matrix and the parity tests), which gives
          scores and order only.
"""

import collections
import functools

import numpy as np

import serenedb_amd as sa

WIN = 24576
DOCS = 2 * WIN + 129
DOCS2 = 129
SEED = 0x48594252
I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1
M64 = (1 << 64) - 1

# SdbPredOp (include/sdb_gpu.h)
LT, GE, BETWEEN, EQ, ISNULL = 1, 2, 3, 4, 5

TERMS = (0, 1, 2)
C_DOCS = (1, WIN, WIN + 1, 2 * WIN, 2 * WIN + 1, DOCS - 1, DOCS)
DEAD_C, LIVE_C = (WIN, 2 * WIN + 1), (1, WIN + 1, 2 * WIN, DOCS)

CASES = collections.OrderedDict([
    ("c01_ordinary", (1000, 1999, 64)),
    ("c02_negative", (-1000, 999, 7)),
    ("c03_tiny_span", (5, 7, 128)),
    ("c04_single_nb1", (42, 42, 1)),
    ("c04_single_nb128", (42, 42, 128)),
    ("c05_empty", (10, 9, 16)),
    # (span - 1) * nb = 2^64 - 128: the widest span whose every product
    # (v - lo) * nb still fits 64 bits
    ("c06a_2p57m1", (0, (1 << 57) - 1, 128)),
    # one wider: only v = hi has a product of 2^64
    ("c06_2p57", (0, 1 << 57, 128)),
    ("c07_2p58", (0, (1 << 58) - 1, 128)),
    ("c08_pm2p62", (-(1 << 62), 1 << 62, 3)),
    ("c09_0_max", (0, I64_MAX, 3)),
    ("c10_min_m1", (I64_MIN, -1, 128)),
    ("c11_full_nb1", (I64_MIN, I64_MAX, 1)),
    ("c11_full_nb2", (I64_MIN, I64_MAX, 2)),
    ("c11_full_nb3", (I64_MIN, I64_MAX, 3)),
    ("c11_full_nb128", (I64_MIN, I64_MAX, 128)),
])
FULL_SPAN = tuple(c for c in CASES if c.startswith("c11"))
OLD_WRONG = ("c07_2p58", "c08_pm2p62", "c09_0_max", "c10_min_m1")
# one bucket of these holds values within 8 of INT64_MAX: its sum wraps
WRAP_CASES = ("c09_0_max",) + FULL_SPAN
CHAIN_CASES = ("c01_ordinary", "c08_pm2p62")


def to_i64(x):
    x &= M64
    return x - (1 << 64) if x >> 63 else x


# ---- segments -----------------------------------------------------------
class Segment:
    def __init__(self, doc_count, postings, norm_seed):
        self.doc_count = doc_count
        self.postings = [(np.asarray(d, dtype=np.uint32),
                          np.asarray(f, dtype=np.uint32))
                         for d, f in postings]
        self.norms = sa.synth_norms(norm_seed, doc_count)
        self.blob = sa.build_segment(doc_count, self.postings, self.norms)

    @functools.lru_cache(maxsize=None)
    def match(self, terms, mm):
        """docs held by at least mm of the terms, ascending"""
        cnt = np.zeros(self.doc_count + 1, dtype=np.int64)
        for t in terms:
            cnt[self.postings[t][0]] += 1
        out = np.nonzero(cnt >= mm)[0]
        out.setflags(write=False)
        return out


def _main_segment():
    a = np.arange(3, DOCS + 1, 3)
    b = np.arange(1, DOCS + 1, 7)
    c = np.array(C_DOCS)
    return Segment(DOCS, [(a, 1 + (a // 3) % 4), (b, 1 + (b // 7) % 3),
                          (c, 1 + np.arange(len(c)) % 3)], 7)


def _second_segment():
    a = np.arange(2, DOCS2 + 1, 2)
    b = np.arange(5, DOCS2 + 1, 5)
    c = np.array((1, 64, 65, 128, 129))
    return Segment(DOCS2, [(a, 1 + (a // 2) % 3), (b, 1 + (b // 5) % 2),
                           (c, 1 + np.arange(len(c)) % 2)], 11)


def _live():
    d = np.arange(DOCS + 1, dtype=np.uint64)
    h = (d * np.uint64(0x9E3779B1)) & np.uint64(0xFFFFFFFF)
    live = ((h >> np.uint64(16)) & np.uint64(3)) != 0
    live[0] = True                      # bit 0 is no doc
    live[list(DEAD_C)] = False
    live[list(LIVE_C)] = True
    live.setflags(write=False)
    return live


class Matrix:
    def __init__(self):
        self.seg = _main_segment()
        self.seg2 = _second_segment()
        self.live = _live()
        rng = np.random.default_rng([SEED, 1])
        m2 = self.seg.match(TERMS, 2)
        # holders: live docs matching at min_match 2 (so at 1 as well), in
        # a fixed order that takes the windows in turn (third, first,
        # second, ... while each lasts; the partial third has only a few),
        # each window's docs shuffled: every case has edges in all three
        held = rng.permutation(m2[self.live[m2]])
        turn = [held[(held - 1) // WIN == w].tolist() for w in (2, 0, 1)]
        self.holders = [q[i] for i in range(max(map(len, turn)))
                        for q in turn if i < len(q)]
        self.chain_cols, self.chain_plants = self._chain_cols()

    def live_words(self):
        """the mask as attach_livemask takes it: bit d of word d >> 6;
        bits past the last doc are set"""
        nwords = (DOCS + 64) // 64
        b = np.ones(nwords * 64, dtype=np.uint8)
        b[:DOCS + 1] = self.live
        return np.packbits(b, bitorder="little").view(np.uint64)

    # ---- the bucket column of a case -----------------------------------
    @staticmethod
    def edge_values(case):
        lo, hi, nb = CASES[case]
        span = hi - lo + 1
        vals = [lo - 1, lo, lo + 1, hi - 1, hi, hi + 1, I64_MIN, I64_MAX]
        if span > 0:
            first = [lo + -((-b * span) // nb) for b in range(nb + 1)]
            for b in range(nb):
                if first[b] < first[b + 1]:          # nonempty range
                    vals += [first[b], first[b] - 1]
            if span < nb:
                vals += range(lo, hi + 1)
        if case in WRAP_CASES:
            assert hi == I64_MAX
            vals += [I64_MAX - i for i in range(1, 5)]
        seen, out = set(), []
        for v in vals:
            if I64_MIN <= v <= I64_MAX and v not in seen:
                seen.add(v)
                out.append(v)
        return out

    @functools.lru_cache(maxsize=None)
    def bucket_col(self, case):
        """(column int64[DOCS + 1], {edge value: its doc})"""
        lo, hi, nb = CASES[case]
        span = max(hi - lo + 1, 0)
        pad = max(span // 4, 2)
        rng = np.random.default_rng([SEED, 2, list(CASES).index(case)])
        col = rng.integers(max(lo - pad, I64_MIN), min(hi + pad, I64_MAX),
                           DOCS + 1, dtype=np.int64, endpoint=True)
        if lo <= hi:
            inside = rng.integers(lo, hi, DOCS + 1, dtype=np.int64,
                                  endpoint=True)
            seen = np.zeros(DOCS + 1, dtype=bool)
            seen[self.seg.match(TERMS, 1)] = True
            hidden = ~(seen & self.live)   # dead or non-matching
            col[hidden] = inside[hidden]
        edges = {}
        vals = self.edge_values(case)
        assert len(vals) <= 400 < len(self.holders)
        for v, d in zip(vals, self.holders):
            col[d] = v
            edges[v] = d
        col.setflags(write=False)
        return col, edges

    @functools.lru_cache(maxsize=None)
    def bucket_col2(self, case):
        """the second segment's column: the edge values laid cyclically,
        from the far end of the list, over its 129 docs"""
        vals = self.edge_values(case)[::-1]
        col = np.array([vals[d % len(vals)] for d in range(DOCS2 + 1)],
                       dtype=np.int64)
        col.setflags(write=False)
        return col

    def _chain_cols(self):
        """slots 1..3: uniform over all of int64, INT64_MIN and INT64_MAX
        planted on holders that no case uses for an edge"""
        cols, plants = {}, {}
        for slot in (1, 2, 3):
            rng = np.random.default_rng([SEED, 3, slot])
            col = rng.integers(I64_MIN, I64_MAX, DOCS + 1, dtype=np.int64,
                               endpoint=True)
            at = self.holders[400 + 40 * slot:400 + 40 * slot + 24]
            for i, d in enumerate(at):
                col[d] = I64_MIN if i % 2 else I64_MAX
            col.setflags(write=False)
            cols[slot] = col
            plants[slot] = tuple(at)
        return cols, plants

    def column(self, case, slot):
        return self.bucket_col(case)[0] if slot == 0 else \
            self.chain_cols[slot]

    # ---- predicate chains ----------------------------------------------
    @staticmethod
    def chain_preds(case, chain):
        """the full chain as (slot, op, lo, hi); preds[0] is the case's span"""
        lo, hi, nb = CASES[case]
        q = (hi - lo + 1) // 4
        extra = {
            None: (),
            "max4": ((1, GE, -(1 << 62), 0), (2, LT, 1 << 62, 0),
                     (3, BETWEEN, -(1 << 62), (1 << 62) - 1)),
            "ge_min": ((1, GE, I64_MIN, 0),),
            "lt_min": ((1, LT, I64_MIN, 0),),
            "ge_max": ((1, GE, I64_MAX, 0),),
            "lt_max": ((1, LT, I64_MAX, 0),),
            "between_empty": ((2, BETWEEN, 5, 4),),
            "between_all": ((3, BETWEEN, I64_MIN, I64_MAX),),
            "same_slot": ((0, BETWEEN, lo + q, hi - q),),
        }[chain]
        return ((0, BETWEEN, lo, hi),) + extra

    # ---- the reference --------------------------------------------------
    @functools.lru_cache(maxsize=None)
    def reference(self, case, chain=None, terms=TERMS, mm=1, live=False,
                  two_seg=False):
        """Ref of one query, all in Python integers. survivors: (segment,
        doc) of every doc that matches, is live and passes every predicate;
        nmatch: matching live docs before the predicates."""
        lo, hi, nb = CASES[case]
        span = hi - lo + 1
        preds = self.chain_preds(case, chain)
        segs = [(self.seg, lambda s: self.column(case, s))]
        if two_seg:
            assert chain is None and not live
            segs.append((self.seg2, lambda s: self.bucket_col2(case)))
        cnt, raw = [0] * nb, [0] * nb
        surv, nmatch = [], 0
        alive = self.live.tolist()
        for si, (seg, colof) in enumerate(segs):
            docs = seg.match(tuple(terms), mm)
            v0 = colof(0)[docs].tolist()
            xs = [(colof(s)[docs].tolist(), op, plo, phi)
                  for s, op, plo, phi in preds[1:]]
            for i, d in enumerate(docs.tolist()):
                if live and not alive[d]:
                    continue
                nmatch += 1
                v = v0[i]
                if not lo <= v <= hi:
                    continue
                ok = True
                for xv, op, plo, phi in xs:
                    x = xv[i]
                    ok = ok and {LT: x < plo, GE: x >= plo,
                                 BETWEEN: plo <= x <= phi}[op]
                if not ok:
                    continue
                b = (v - lo) * nb // span
                cnt[b] += 1
                raw[b] += v
                surv.append((si, d))
        counts = np.array(cnt, dtype=np.int64)
        sums = np.array([to_i64(s) for s in raw], dtype=np.int64)
        counts.setflags(write=False)
        sums.setflags(write=False)
        return Ref(len(surv), tuple(surv), counts, sums, tuple(raw), nmatch)

    # ---- hits -----------------------------------------------------------
    @functools.lru_cache(maxsize=None)
    def ranking(self, terms=TERMS, mm=1, live=False, two_seg=False):
        """every matching (live) doc in rank order, (score desc, segment,
        doc), from the oracle's plain top-k. Scores and order only: nothing
        about the filter comes from here."""
        from oracle import pyoracle as po

        blobs = [self.seg.blob] + ([self.seg2.blob] if two_seg else [])
        n = len(self.seg.match(tuple(terms), mm)) + (
            len(self.seg2.match(tuple(terms), mm)) if two_seg else 0)
        hits, _ = po.execute_topk(
            blobs, list(terms), [1.0] * len(terms), max(n, 1), min_match=mm,
            live_mask=self.live_words() if live else None)
        hits.setflags(write=False)
        return hits

    def expected_hits(self, ref, k, terms=TERMS, mm=1, live=False,
                      two_seg=False):
        rank = self.ranking(tuple(terms), mm, live, two_seg)
        assert len(rank) == ref.nmatch
        surv = set(ref.survivors)
        keep = [i for i, (s, d) in enumerate(zip(rank["segment"].tolist(),
                                                 rank["doc"].tolist()))
                if (s, d) in surv]
        assert len(keep) == ref.total
        return rank[keep[:k]]


Ref = collections.namedtuple("Ref", "total survivors counts sums raw nmatch")


def old_bucket(v, lo, hi, nb):
    """the expression this matrix replaces, with its 64-bit wraps written
    out: None where its span wraps to 0 (a division by zero)"""
    span = (((hi - lo) & M64) + 1) & M64
    if span == 0:
        return None
    return min((((v - lo) & M64) * nb & M64) // span, nb - 1)


@functools.lru_cache(maxsize=None)
def matrix():
    return Matrix()
