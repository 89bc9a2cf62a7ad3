"""Block-fetch matrix: three small segments aimed at how the GPU decoders
fetch packed words, not at which block families exist (tests/codec_matrix.py
covers those). The decoders read every value through aligned, branch-free
loads of the value's word and the next word; what can go wrong there is

  * the over-read behind the very last stream of the payload (three builds
    that differ only in their final term: a fused full block with the widest
    norm stream the builder produces, one with the narrowest widths, and a
    non-fused tail block),
  * the byte residue of a block start (fused blocks at every residue 0..7
    mod 8, steered by the tail blocks of different lengths that end the
    preceding terms),
  * a value straddling two words or not (widths such as 31, where nearly
    every value straddles, and 2, 4, 8, 16, where none does).

The corpus is 3 windows of 24576 docs plus a few hundred, so blocks straddle
windows. As in codec_matrix the raw (docs, freqs) arrays and the norms
column are the ground truth; the references never decode the blob."""

import ctypes as C
import functools

import numpy as np

import codec_matrix as cm
import serenedb_amd as sa

WIN = cm.WIN
BLOCK = cm.BLOCK
DOC_COUNT = 3 * WIN + 300
SEED = 0xB10CFE7C
BUILDS = ("wide_end", "narrow_end", "tail_end")
# freq / norm widths of the width terms: both sides of every word-straddle
# pattern (2, 4, 8, 16 never straddle; odd widths straddle somewhere; at 31
# all groups but the first straddle) and the top of the range
WIDTHS = (2, 3, 4, 5, 7, 8, 15, 16, 17, 23, 24, 25, 29, 30, 31)
# doc-gap widths of the same terms (a pinned gap of width w costs 2^w docs,
# so the wider ones live in the roaming "d<w>" terms)
TERM_DOC_WIDTHS = (2, 3, 4, 5, 6, 7, 8, 9, 2, 3, 4, 5, 6, 7, 8)
ROAMING_DOC_WIDTHS = (10, 11, 12, 13, 16, 17)


class SdbBlockDesc(C.Structure):
    """include/sdb_format.h"""
    _fields_ = [("prev_doc", C.c_uint32), ("last_doc", C.c_uint32),
                ("doc_off", C.c_uint32), ("freq_off", C.c_uint32),
                ("len", C.c_uint16), ("flags", C.c_uint16),
                ("max_freq", C.c_uint32), ("min_norm", C.c_uint32)]


class SdbTermEntry(C.Structure):
    _fields_ = [("desc_begin", C.c_uint64), ("desc_end", C.c_uint64),
                ("payload_begin", C.c_uint64), ("payload_end", C.c_uint64),
                ("df", C.c_uint32), ("max_freq", C.c_uint32),
                ("total_freq", C.c_uint64)]


class SdbSegHeader(C.Structure):
    _fields_ = [("magic", C.c_uint64), ("version", C.c_uint32),
                ("nterms", C.c_uint32), ("doc_count", C.c_uint32),
                ("docs_with_field", C.c_uint32),
                ("total_term_freq", C.c_uint64), ("total_blocks", C.c_uint64),
                ("off_terms", C.c_uint64), ("off_desc", C.c_uint64),
                ("off_norms", C.c_uint64), ("off_payload", C.c_uint64),
                ("payload_size", C.c_uint64), ("blob_size", C.c_uint64)]


class SdbSegmentView(C.Structure):
    _fields_ = [("hdr", C.POINTER(SdbSegHeader)),
                ("terms", C.POINTER(SdbTermEntry)),
                ("desc", C.POINTER(SdbBlockDesc)),
                ("norms", C.POINTER(C.c_uint32)),
                ("payload", C.POINTER(C.c_uint8))]


class FetchMatrix(cm.Matrix):
    """One build. Same references as codec_matrix.Matrix, over this
    corpus's doc count."""

    def ref_scores(self, terms, boosts, scorer, k1=1.2, b=0.75):
        """Term-major fp32 replication of the scorers over the raw arrays:
        (docs ascending, score per doc, matched-term count per doc)."""
        key = (tuple(terms), tuple(float(x) for x in boosts), scorer)
        if key in self._ref_cache:
            return self._ref_cache[key]
        F = np.float32
        u = np.unique(np.concatenate([self.postings[t][0] for t in terms]))
        scores = np.zeros(len(u), dtype=F)
        cnt = np.zeros(len(u), dtype=np.int32)
        fk1, fb = F(k1), F(b)
        nc = fk1 - fk1 * fb
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
            scores[at] += contrib   # docs are unique within a term
            cnt[at] += 1
        out = (u, scores, cnt, None)
        self._ref_cache[key] = out
        return out

    def parse(self):
        """Per term, the block records read from the descriptors that
        sdb_host_segment_parse exposes, plus where each block's streams sit
        in the payload section (abs_off: byte offset from the payload
        start, which the GPU loader places on an aligned allocation)."""
        buf = np.frombuffer(self.blob, dtype=np.uint8)
        view = SdbSegmentView()
        rc = sa.host().sdb_host_segment_parse(
            buf.ctypes.data_as(C.c_void_p), C.c_uint64(len(buf)),
            C.byref(view))
        assert rc == 0, rc
        hdr = view.hdr.contents
        assert hdr.nterms == len(self.names)
        out = []
        for t in range(hdr.nterms):
            te = view.terms[t]
            recs = []
            for bi in range(te.desc_begin, te.desc_end):
                d = view.desc[bi]
                fused = d.flags & 1
                db, fb, nb = ((d.flags >> 1) & 31, (d.flags >> 6) & 31,
                              (d.flags >> 11) & 31)
                if fused:
                    end = d.freq_off + 2 + 16 * (fb + nb)
                else:
                    end = None
                recs.append(dict(
                    prev=d.prev_doc, last=d.last_doc, len=d.len,
                    fused=fused, db=db, fb=fb, nb=nb, doc_off=d.doc_off,
                    abs_off=te.payload_begin + d.doc_off,
                    abs_end=None if end is None else te.payload_begin + end,
                    payload_end=te.payload_end))
            out.append(recs)
        return out, hdr.payload_size, hdr.blob_size - hdr.off_payload


def _gaps(rng, w, n):
    """n doc gaps of bit width <= w, large enough on average that the
    encoder's bitpack beats its bitset (16*w bytes against ~2 bytes per
    unit of mean gap)."""
    hi = min((1 << w) - 1, 19)
    lo = max(1, (hi + 1) // 2)
    return rng.integers(lo, hi + 1, n).astype(np.int64)


def _base(rng):
    """Everything the three builds share: the norms column and every term
    but the last. Returns (norms, [(name, docs, freqs)], end-term specs)."""
    norms = rng.integers(1, 1 << 12, DOC_COUNT + 1).astype(np.uint32)
    norms[0] = 0
    terms = []
    cursor = [1]

    def region(docs_needed):
        start = cursor[0]
        cursor[0] = start + docs_needed
        assert cursor[0] <= DOC_COUNT, "doc space exhausted"
        return start

    def width_term(name, dw, fw, nw, full, tail):
        """`full` full blocks then a tail of `tail` docs, in a doc region
        of its own whose norms are written for the purpose: every full
        block holds one gap, one freq and one norm of exactly the pinned
        width and nothing wider."""
        n = BLOCK * full + tail
        gaps = _gaps(rng, dw, n)
        for blk in range(full):
            gaps[BLOCK * blk + int(rng.integers(1, BLOCK))] = \
                int(rng.integers(1 << (dw - 1), 1 << dw))
        span = int(gaps.sum())
        start = region(span + 1)
        docs = (start - 1 + np.cumsum(gaps)).astype(np.uint32)
        freqs = cm._small(rng, fw, n)
        norms[start:start + span + 1] = cm._small(rng, nw, span + 1)
        for blk in range(full):
            freqs[BLOCK * blk + int(rng.integers(0, BLOCK))] = \
                cm._pin(rng, fw)
            norms[docs[BLOCK * blk + int(rng.integers(0, BLOCK))]] = \
                cm._pin(rng, nw)
        return name, docs, freqs

    # -- the three candidate final terms first, so they get regions no
    # matter how much the width terms take
    ends = {
        "wide_end": width_term("end", 9, 31, 31, 2, 0),
        "narrow_end": width_term("end", 2, 2, 2, 2, 0),
        "tail_end": width_term("end", 5, 7, 9, 1, 5),
    }

    # -- width terms: freq width ascending against norm width descending,
    # two full blocks and a tail of a different length each (the tails
    # shift the byte residue at which the next term's blocks start)
    for i, fw in enumerate(WIDTHS):
        nw = WIDTHS[len(WIDTHS) - 1 - i]
        terms.append(width_term(f"w{fw}_{nw}", TERM_DOC_WIDTHS[i], fw, nw,
                                2, i + 1))

    # -- nine fused blocks in a row: a fused block is 3 + 16*(db+fb+nb)
    # bytes, 3 mod 8, so nine consecutive ones start at every residue
    n = 9 * BLOCK
    docs = cm._walk(rng, 15_000, n, 4, 19)   # crosses the window-0/1 border
    terms.append(("res9", docs, rng.integers(1, 16, n).astype(np.uint32)))

    # -- wider doc gaps: terms that roam over the whole doc space (their
    # norms are whatever the docs they land on carry)
    for w in ROAMING_DOC_WIDTHS:
        n = 2 * BLOCK + 3
        gaps = _gaps(rng, w, n)
        npin = 1 if w >= 16 else 2
        for blk in range(npin):
            lo_pin = 1 << (w - 1)
            gaps[BLOCK * blk + int(rng.integers(1, BLOCK))] = \
                lo_pin + int(rng.integers(0, min(lo_pin, 1500)))
        start = int(rng.integers(1, 300))
        docs = (start + np.cumsum(gaps)).astype(np.uint32)
        assert docs[-1] <= DOC_COUNT, (w, docs[-1])
        terms.append((f"d{w}", docs,
                      rng.integers(1, 16, n).astype(np.uint32)))

    # -- two terms spread over all three windows that share docs with every
    # other term (term-major accumulation on shared docs)
    for name, step in (("span_a", 31), ("span_b", 43)):
        docs = np.sort(rng.choice(DOC_COUNT, DOC_COUNT // step,
                                  replace=False) + 1).astype(np.uint32)
        terms.append((name, docs,
                      rng.integers(1, 64, len(docs)).astype(np.uint32)))
    return norms, terms, ends


def _build_all():
    rng = np.random.default_rng(SEED)
    norms, terms, ends = _base(rng)
    ttf = int(norms[1:].sum(dtype=np.uint64))
    out = {}
    for build in BUILDS:
        m = FetchMatrix()
        for name, docs, freqs in terms + [ends[build]]:
            m.add(name, docs, freqs)
        m.norms = norms
        m.ttf = ttf
        m.blob = sa.build_segment(DOC_COUNT, m.postings, norms)
        t = m.terms
        m.groups = {"all": list(range(len(m.names)))}
        assert len(m.groups["all"]) <= 32
        # 4-term plans for the per-wave kernel; the final term is in each
        m.small_groups = {
            "end_res": t(["end", "res9", "span_a", "w31_2"]),
            "end_wide": t(["end", "d16", "w2_31", "span_b"]),
            "end_mid": t(["end", "d13", "w16_16", "w17_15"]),
        }
        out[build] = m
    return out


@functools.lru_cache(maxsize=None)
def builds():
    """{build name: FetchMatrix}, built once per process."""
    return _build_all()
