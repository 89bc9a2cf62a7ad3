"""The segment-set matrix on the CPU (tests/segset_matrix.py): the numpy fp32
reference over a set of segments equals the C oracle bit for bit, a second
witness covers the masked and boosted sets the oracle cannot take in one
call, and the corpus holds what the GPU matrix relies on: tie classes that
are bit-equal across segments, a spike segment that owns the top 10, hollow
segments, a 130-segment cycle whose slots s and s + 64 are different blobs,
and cases on which each plausible mistake shows."""

import numpy as np
import pytest

import segset_matrix as ss


@pytest.fixture(scope="module")
def m():
    return ss.matrix()


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def same(a, b, what):
    """two (segment, doc, score, total) answers, bit for bit"""
    assert a[3] == b[3], what
    assert len(a[1]) == len(b[1]), what
    np.testing.assert_array_equal(a[0], b[0], err_msg=what)
    np.testing.assert_array_equal(a[1], b[1], err_msg=what)
    np.testing.assert_array_equal(bits(a[2]), bits(b[2]), err_msg=what)


# ---------------------------------------------------------------------------
# 1. the reference against the oracle, on every set
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("set_", sorted(ss.SETS))
def test_reference_equals_oracle(m, set_):
    """no mask and no boost: the oracle takes the whole set in one call"""
    plan = ss.SET_PLAN[set_]
    blobs = [m.blobs[bi].blob for bi in ss.SETS[set_]]
    n = 0
    for mm in sorted({1, min(2, len(plan)), len(plan)}):
        for param in ("bm25", "tfidf_norm"):
            for g in (None, True):
                c = m.case(set_, plan, param=param, mm=mm, gstats=g)
                ref = m.ref_full(c)
                assert ref[3] == m.ref_count(c)
                got = ss.oracle_topk(
                    blobs, c["terms"], c["boosts"], len(ref[1]) + 7, mm=mm,
                    k1=c["k1"], b=c["b"], scorer=c["scorer"],
                    gstats=c["gstats"])
                same(got, ref, f"{set_} mm={mm} {param} gstats={g}")
                n += 1
    assert n >= 8 or len(plan) == 1


def test_named_plain_cases_equal_oracle(m):
    """every named case without a mask or a boost, at its own plan (the
    3-term, 32-term, tie and void plans the walk above does not take)"""
    n = 0
    for name, c in m.cases.items():
        if c["masked"] or c["fb"] or name in ("s65", "s70", "s130"):
            continue
        blobs = [m.blobs[bi].blob for bi in m.positions(c)]
        ref = m.ref_full(c)
        got = ss.oracle_topk(blobs, c["terms"], c["boosts"],
                             len(ref[1]) + 7, mm=c["mm"], k1=c["k1"],
                             b=c["b"], scorer=c["scorer"],
                             gstats=c["gstats"])
        same(got, ref, name)
        n += 1
    assert n > 30


# ---------------------------------------------------------------------------
# 2. masked and boosted sets: the oracle once per segment, merged in Python
# ---------------------------------------------------------------------------

def test_masked_and_boosted_second_witness(m):
    n = 0
    for name, c in m.cases.items():
        if not (c["masked"] or c["fb"]):
            continue
        g = c["gstats"] if c["gstats"] is not None else m.merged_stats(c)
        sg, u, s, total = [], [], [], 0
        for pos, bi in enumerate(m.positions(c)):
            seg = m.blobs[bi]
            _, d, sc, t = ss.oracle_topk(
                [seg.blob], c["terms"], c["boosts"], seg.doc_count,
                mm=c["mm"], k1=c["k1"], b=c["b"], scorer=c["scorer"],
                gstats=g, fb=seg.fb[c["fb"]] if c["fb"] else None,
                live_words=seg.live_words
                if c["masked"] and seg.masked else None)
            sg.append(np.full(len(d), pos, dtype=np.uint32))
            u.append(d)
            s.append(sc)
            total += t
        sg, u, s = (np.concatenate(x) for x in (sg, u, s))
        order = np.lexsort((u, sg, -s))
        same((sg[order], u[order], s[order], total), m.ref_full(c), name)
        n += 1
    assert n >= 9


# ---------------------------------------------------------------------------
# 3. the corpus holds what it claims
# ---------------------------------------------------------------------------

def test_shapes(m):
    assert [b.doc_count for b in m.blobs] == list(ss.DOC_COUNTS)
    one = m.blobs[0]
    assert [one.df(t) for t in range(len(ss.TERMS))] == \
        [1] + [0] * (len(ss.TERMS) - 1)
    for b in m.blobs:
        n = b.doc_count
        common = b.postings[ss.T["common"]][0]
        assert common[0] == 1 and common[-1] == n
        assert b.df(ss.T["void"]) == 0
        assert (b.df(ss.T["rare"]) > 0) == (b.index in ss.RARE_IN)
        assert (b.df(ss.T["tie"]) > 0) == (b.index in ss.TIE_IN)
        for j in range(ss.NWIDE):
            assert (b.df(ss.T[f"w{j}"]) > 0) == (n >= 4095)
        assert len(b.live_words) == (n + 64) // 64
    assert sum(b.masked for b in m.blobs) == 5
    assert not m.blobs[1].live.any()                         # all dead
    six = m.blobs[6]
    assert (~six.live[1:]).nonzero()[0].tolist() == [six.doc_count - 1]
    assert not m.blobs[3].live[63] and not m.blobs[3].live[64]
    assert not m.blobs[4].live[64] and not m.blobs[4].live[65]
    # unequal densities, unequal boosts
    big = m.blobs[11]
    assert big.df(ss.T["common"]) > 2 * big.df(ss.T["mid"])
    c = m.cases["asc_or"]
    assert len(set(c["boosts"])) == len(c["boosts"])


def test_tie_classes_are_bit_equal_across_segments(m):
    c = m.cases["asc_tie"]
    sg, u, s, total = m.ref_full(c)
    assert total == len(ss.TIE_IN) * len(ss.TIE_DOCS) == len(u)
    tie_pos = [p for p, bi in enumerate(ss.SETS["asc"]) if bi in ss.TIE_IN]
    by_doc = {}
    for a, d, x in zip(sg.tolist(), u.tolist(), bits(s).tolist()):
        by_doc.setdefault(d, []).append((a, x))
    assert sorted(by_doc) == sorted(ss.TIE_DOCS)
    for d, v in by_doc.items():
        assert [a for a, _ in v] == tie_pos, d         # segment ascending
        assert len({x for _, x in v}) == 1, d          # one score, six times
    # docs 3 and 9 are one class; the other docs are classes of their own
    assert by_doc[3][0][1] == by_doc[9][0][1]
    assert len({v[0][1] for v in by_doc.values()}) == len(ss.TIE_DOCS) - 1


@pytest.mark.parametrize("name", ["asc_tie", "dups_tie", "same_handle_tie",
                                  "dups_p2"])
def test_k_edges_split_tie_classes(m, name):
    """at a tie-splitting k the k-th and (k+1)-th entries differ only in
    segment; each tie case holds several such k"""
    c = m.cases[name]
    sg, u, s, _ = m.ref_full(c)
    split = [k for k in c["ks"] if k < len(u) and u[k - 1] == u[k]
             and bits(s)[k - 1] == bits(s)[k] and sg[k - 1] != sg[k]]
    assert len(split) >= (6 if name.endswith("_tie") else 4), split
    # and k values at which the next entry is the same segment's next doc
    # with the same score: (doc, segment) order would take another one
    if name.endswith("_tie"):
        assert any(sg[k - 1] == sg[k] and u[k - 1] != u[k]
                   and bits(s)[k - 1] == bits(s)[k]
                   for k in c["ks"] if k < len(u))


def test_spike_segment_owns_the_top_10(m):
    for s in ("asc", "desc", "spike_first", "spike_last"):
        for name in (f"{s}_or", f"{s}_mm2", f"{s}_wide"):
            c = m.cases[name]
            sg, u, _, _ = m.ref_topk(c, 10)
            pos = ss.SETS[s].index(ss.SPIKE)
            assert set(sg.tolist()) == {pos}, name
            assert set(u.tolist()) <= set(ss.SPIKE_DOCS), name
    assert ss.SETS["spike_first"][0] == ss.SPIKE == ss.SETS["spike_last"][-1]


def test_hollow_segments_have_no_postings_of_the_plan(m):
    for s in ("hollow_first", "hollow_mid", "hollow_last"):
        c = m.cases[s]
        empty = [pos for pos, bi in enumerate(m.positions(c))
                 if all(m.blobs[bi].df(t) == 0 for t in c["terms"])]
        want = {"hollow_first": 0, "hollow_mid": 2, "hollow_last": 3}[s]
        assert empty == [want], s
        assert m.ref_full(c)[3] > 10
    c = m.cases["all_hollow"]
    assert all(m.blobs[bi].df(t) == 0 for bi in m.positions(c)
               for t in c["terms"])
    assert m.ref_full(c)[3] == 0 and len(m.ref_full(c)[1]) == 0
    for name in ("void", "empty"):
        assert m.ref_full(m.cases[name])[3] == 0
    a, b = m.ref_full(m.cases["void_in_or"]), m.ref_full(
        m.case("asc", ("common", "mid"), boosts=m.cases["void_in_or"][
            "boosts"][::2]))
    same(a, b, "void adds nothing")
    sg, u, s, total = m.ref_full(m.cases["only_one_doc"])
    assert (sg.tolist(), u.tolist(), total) == ([0], [1], 1)


def test_slot_ring_neighbours_are_different_blobs(m):
    s130 = ss.SETS["s130"]
    for s in range(len(s130) - 64):
        a, b = m.blobs[s130[s]], m.blobs[s130[s + 64]]
        assert a.index != b.index and a.blob != b.blob
        assert a.doc_count != b.doc_count
    assert len(ss.SETS["s65"]) == 65 and len(ss.SETS["s70"]) == 70


def test_fbmax_comes_from_a_later_segment(m):
    for name in ("peak_bm25", "peak_desc_bm25"):
        c = m.cases[name]
        at = m.positions(c).index(ss.PEAK)
        assert 0 < at < len(m.positions(c)) - 1
        assert m.fbmax(c) == ss.PEAK_VALUE
        assert m.fbmax(c, "fbmax_first") < ss.PEAK_VALUE
    assert m.fbmax(m.cases["flat_bm25"]) == np.float32(1.25)


def test_column_and_ranges(m):
    """values on both sides of every range; one whole segment fails the
    narrow ranges; the huge range wraps its sums"""
    c = m.cases["unboosted"]
    for rname, (lo, hi, nb) in ss.RANGES.items():
        ref = m.ref_hybrid(c, lo, hi, nb)
        assert 0 < ref.total < m.ref_count(c), rname
        assert ref.counts.sum() == ref.total
    lo, hi, nb = ss.RANGES["fails_one"]
    cold = ss.SETS["asc"].index(ss.COLD)
    surv = m.ref_hybrid(c, lo, hi, nb).survivors
    assert not any(pos == cold for pos, _ in surv)
    assert len({pos for pos, _ in surv}) == ss.NBLOBS - 1
    lo, hi, nb = ss.RANGES["huge"]
    ref = m.ref_hybrid(c, lo, hi, nb)
    assert {pos for pos, _ in ref.survivors} == set(ss.HUGE_IN)
    assert (ref.sums < 0).any()         # a positive sum that wrapped


def test_stream_reference(m):
    c = m.case("asc", ss.P2)
    pairs, vals, total = m.ref_stream(c, 10**9)
    assert len(pairs) == total == m.ref_count(c) == len(vals)
    assert pairs == sorted(pairs)
    cut, _, t2 = m.ref_stream(c, 100)
    assert cut == pairs[:100] and t2 == total


# ---------------------------------------------------------------------------
# wrong-on-purpose references: the cases tell each mistake apart
# ---------------------------------------------------------------------------

def differs(m, name, k, wrong):
    c = m.cases[name]
    a, b = m.ref_topk(c, k), m.ref_topk(c, k, wrong=wrong)
    return not (a[3] == b[3] and np.array_equal(a[0], b[0])
                and np.array_equal(a[1], b[1])
                and np.array_equal(bits(a[2]), bits(b[2])))


def test_wrong_segment_index_shows(m):
    """segment = the blob's own index, not the position in the call"""
    for name in ("desc_or", "spike_first_or", "spike_last_or", "dups_tie",
                 "s65", "s130", "hollow_mid"):
        assert differs(m, name, 10, "blob_index"), name
    assert not differs(m, "asc_or", 10, "blob_index")   # position == index


def test_wrong_tie_order_shows(m):
    """ties ordered (doc, segment)"""
    for name in ("asc_tie", "dups_tie", "same_handle_tie"):
        assert differs(m, name, 4, "doc_first"), name


def test_per_segment_statistics_show(m):
    for name in ("asc_or", "desc_mm2", "spike_last_and", "s70", "masked",
                 "peak_bm25", "hollow_first"):
        assert differs(m, name, 10, "local_stats"), name
    # injected statistics override both
    assert not differs(m, "gstats", 10, "local_stats")


def test_fbmax_of_the_first_segment_shows(m):
    """fbmax changes no score: it scales the score bound (the histogram bins
    and the WAND bounds). The observable is the bound itself: with the set's
    fbmax no score exceeds it; with the first segment's fbmax the top score
    is above it. The slack is the rounding of (sum of num) * fbmax
    against the sum of (num * fb) terms: three f32 operations, under
    2^-21 relative."""
    slack = np.float64(1.0 + 2.0**-21)
    for name, c in m.cases.items():
        top = m.ref_topk(c, 1)[2]
        if len(top):
            assert np.float64(top[0]) <= np.float64(m.ref_smax(c)) * slack, \
                name
    for name in ("peak_bm25", "peak_tfidf_norm", "peak_desc_bm25",
                 "gstats_masked_peak"):
        c = m.cases[name]
        top = m.ref_topk(c, 1)[2][0]
        assert m.ref_smax(c, "fbmax_first") < top, name
