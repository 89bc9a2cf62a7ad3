"""The hybrid filter matrix (tests/hybrid_matrix.py) proved on the CPU: every
edge is where the matrix says, the old wrapped bucket expression is wrong on
it, and the CPU oracle agrees with the Python-integer reference on every case
its signature can express (one segment, no live mask). No GPU needed."""

import numpy as np
import pytest

import hybrid_matrix as hm
from oracle import pyoracle as po

K = 64
CASE_IDS = list(hm.CASES)
MODES = [(1, False), (1, True), (2, False), (2, True)]   # (min_match, live)


@pytest.fixture(scope="module")
def mx():
    return hm.matrix()


def test_segment_shape(mx):
    assert hm.DOCS == 49281 and hm.DOCS % hm.WIN == 129
    assert (hm.DOCS - 2 * hm.WIN - 1) % 64 == 0   # one doc into a new word
    a, b, c = (p[0].tolist() for p in mx.seg.postings)
    assert a == list(range(3, hm.DOCS + 1, 3))
    assert b == list(range(1, hm.DOCS + 1, 7))
    assert c == [1, 24576, 24577, 49152, 49153, 49280, 49281]
    assert mx.seg.match(hm.TERMS, 3).tolist() == [hm.DOCS]   # the AND
    assert mx.seg2.doc_count == 129
    assert len(mx.seg2.match(hm.TERMS, 2)) > 10


def test_live_mask(mx):
    live = mx.live
    dead = 1.0 - live[1:].mean()
    assert 0.2 < dead < 0.3
    assert sum(not live[d] for d in hm.C_DOCS) >= 2
    assert sum(bool(live[d]) for d in hm.C_DOCS) >= 2
    for w in (1, 2):   # exactly one dead doc across each window boundary
        assert live[w * hm.WIN] != live[w * hm.WIN + 1]
    assert live[hm.DOCS]          # the AND's only doc
    words = mx.live_words()
    assert len(words) == (hm.DOCS + 64) // 64
    for d in (1, 63, 64, 24576, 24577, 49216, 49217, 49281):
        assert bool((int(words[d >> 6]) >> (d & 63)) & 1) == bool(live[d])
    # every window holds dead matches, so a path that skipped the mask in
    # one window would be seen
    m = mx.seg.match(hm.TERMS, 2)
    for w in range(3):
        inw = m[(m > w * hm.WIN) & (m <= (w + 1) * hm.WIN)]
        assert (~live[inw]).sum() >= 2 and live[inw].sum() >= 4


@pytest.mark.parametrize("case", CASE_IDS)
def test_edges_are_held(mx, case):
    """each planted edge value sits on a live doc matching at min_match 2
    (and 1); inside [lo, hi] that doc is a survivor in every mode"""
    lo, hi, nb = hm.CASES[case]
    col, edges = mx.bucket_col(case)
    assert set(edges) == set(mx.edge_values(case))
    for v in (lo - 1, lo, lo + 1, hi - 1, hi, hi + 1, hm.I64_MIN,
              hm.I64_MAX):
        assert (v in edges) == (hm.I64_MIN <= v <= hm.I64_MAX)
    m1 = set(mx.seg.match(hm.TERMS, 1).tolist())
    m2 = set(mx.seg.match(hm.TERMS, 2).tolist())
    windows = set()
    for v, d in edges.items():
        assert int(col[d]) == v and mx.live[d] and d in m2 and d in m1
        windows.add((d - 1) // hm.WIN)
    assert windows == {0, 1, 2}
    for mm, live in MODES:
        surv = {d for _, d in mx.reference(case, mm=mm, live=live).survivors}
        for v, d in edges.items():
            assert (d in surv) == (lo <= v <= hi), (v, d, mm, live)


@pytest.mark.parametrize("case", CASE_IDS)
def test_hidden_docs_are_inside(mx, case):
    """dead and non-matching docs hold values inside [lo, hi]: ignoring the
    mask or the match word would count them"""
    lo, hi, nb = hm.CASES[case]
    if lo > hi:
        return
    col, _ = mx.bucket_col(case)
    seen = np.zeros(hm.DOCS + 1, dtype=bool)
    seen[mx.seg.match(hm.TERMS, 1)] = True
    hidden = ~(seen & mx.live)
    hidden[0] = False
    assert hidden.sum() > 20000
    assert ((col[hidden] >= lo) & (col[hidden] <= hi)).all()
    masked = mx.reference(case, live=True)
    plain = mx.reference(case)
    assert masked.total < plain.total or plain.total == 0


@pytest.mark.parametrize("case", CASE_IDS)
def test_reference_is_consistent(mx, case):
    lo, hi, nb = hm.CASES[case]
    span = hi - lo + 1
    for mm, live in MODES:
        ref = mx.reference(case, mm=mm, live=live)
        assert int(ref.counts.sum()) == ref.total == len(ref.survivors)
        assert ref.total <= ref.nmatch
        if lo > hi:
            assert ref.total == 0 and not ref.counts.any() \
                and not ref.sums.any()
            continue
        assert ref.total > 0
        if case in ("c03_tiny_span", "c04_single_nb1", "c04_single_nb128"):
            continue
        first = [lo + -((-b * span) // nb) for b in range(nb + 1)]
        for b in range(nb):   # every bucket with a nonempty range is used
            assert first[b] < first[b + 1]
            assert ref.counts[b] > 0, (case, b, mm, live)


def test_tiny_span_covers_every_value(mx):
    lo, hi, nb = hm.CASES["c03_tiny_span"]
    ref = mx.reference("c03_tiny_span", mm=2, live=True)
    used = [(v - lo) * nb // (hi - lo + 1) for v in range(lo, hi + 1)]
    assert used == [0, 42, 85]
    assert sorted(np.nonzero(ref.counts)[0].tolist()) == used


def _old_vs_exact(mx, case, mm=2, live=True):
    lo, hi, nb = hm.CASES[case]
    col, _ = mx.bucket_col(case)
    ref = mx.reference(case, mm=mm, live=live)
    diff = []
    for _, d in ref.survivors:
        v = int(col[d])
        if hm.old_bucket(v, lo, hi, nb) != (v - lo) * nb // (hi - lo + 1):
            diff.append(v)
    return diff


@pytest.mark.parametrize("case", hm.OLD_WRONG)
def test_old_expression_is_wrong_on_wide_spans(mx, case):
    """the proof that the GPU tests fail on the old kernels: at least 100
    survivors of every mode land in another bucket under the wrapped
    64-bit expression"""
    for mm, live in MODES:
        assert len(_old_vs_exact(mx, case, mm, live)) >= 100


def test_old_expression_is_right_up_to_the_fast_path_edge(mx):
    """c06a is the widest span on which the old expression is exact for
    every value, so the narrow path may keep it there. c06, one value
    wider, has exactly one product of 2^64: v = hi; the old expression is
    right on every other value and wrong there (bucket 0 for 127)."""
    lo, hi, nb = hm.CASES["c06a_2p57m1"]
    assert (hi - lo) * nb < 1 << 64 <= (hi - lo + 1) * nb
    for mm, live in MODES:
        assert _old_vs_exact(mx, "c06a_2p57m1", mm, live) == []
        assert _old_vs_exact(mx, "c06_2p57", mm, live) == [1 << 57]
    assert hm.old_bucket(1 << 57, 0, 1 << 57, 128) == 0
    assert (1 << 57) * 128 // ((1 << 57) + 1) == 127
    for case in CASE_IDS[:5]:
        assert _old_vs_exact(mx, case) == []


@pytest.mark.parametrize("case", hm.FULL_SPAN)
def test_full_span_has_no_old_expression(mx, case):
    lo, hi, nb = hm.CASES[case]
    assert ((hi - lo) & hm.M64) + 1 & hm.M64 == 0
    assert hm.old_bucket(0, lo, hi, nb) is None


@pytest.mark.parametrize("case", hm.WRAP_CASES)
def test_wrap_cases_wrap(mx, case):
    lo, hi, nb = hm.CASES[case]
    col, edges = mx.bucket_col(case)
    near = [v for v in edges if v >= hm.I64_MAX - 8]
    assert len(near) >= 3
    assert all((v - lo) * nb // (hi - lo + 1) == nb - 1 for v in near)
    for mm, live in MODES:
        ref = mx.reference(case, mm=mm, live=live)
        raw = ref.raw[nb - 1]
        assert not hm.I64_MIN <= raw <= hm.I64_MAX
        assert int(ref.sums[nb - 1]) == hm.to_i64(raw) != raw


@pytest.mark.parametrize("case", hm.CHAIN_CASES)
def test_chains(mx, case):
    single = mx.reference(case, mm=2, live=True)
    ref = {c: mx.reference(case, c, mm=2, live=True)
           for c in ("max4", "ge_min", "lt_min", "ge_max", "lt_max",
                     "between_empty", "between_all", "same_slot")}
    assert len(mx.chain_preds(case, "max4")) == 4
    assert {p[0] for p in mx.chain_preds(case, "max4")} == {0, 1, 2, 3}
    assert [p[0] for p in mx.chain_preds(case, "same_slot")] == [0, 0]
    for c in ("ge_min", "between_all"):
        assert ref[c].survivors == single.survivors
        assert (ref[c].counts == single.counts).all()
        assert (ref[c].sums == single.sums).all()
    for c in ("lt_min", "between_empty"):
        assert ref[c].total == 0 and not ref[c].counts.any()
    assert 0 < ref["ge_max"].total <= 12
    assert ref["ge_max"].total + ref["lt_max"].total == single.total
    assert 0 < ref["max4"].total < single.total // 2
    assert 0 < ref["same_slot"].total < single.total
    for slot in (1, 2, 3):   # the planted extremes sit on holders
        col = mx.chain_cols[slot]
        vals = {int(col[d]) for d in mx.chain_plants[slot]}
        assert vals == {hm.I64_MIN, hm.I64_MAX}
        assert all(d in mx.holders for d in mx.chain_plants[slot])


def test_second_segment_and_and(mx):
    for case in CASE_IDS:
        one = mx.reference(case)
        two = mx.reference(case, two_seg=True)
        assert two.total >= one.total
        assert two.survivors[:one.total] == one.survivors
        if hm.CASES[case][0] <= hm.CASES[case][1]:
            assert any(s == 1 for s, _ in two.survivors), case
    ref = mx.reference("c01_ordinary", terms=(0, 1), mm=2)
    assert ref.nmatch == len(range(15, hm.DOCS + 1, 21)) and ref.total > 100


# ---- the CPU oracle against the reference --------------------------------
def _check(got, ref, exp_hits):
    hits, total, bcnt, bsum = got
    assert total == ref.total
    np.testing.assert_array_equal(hits["doc"], exp_hits["doc"])
    np.testing.assert_array_equal(hits["score"].view(np.uint32),
                                  exp_hits["score"].view(np.uint32))
    np.testing.assert_array_equal(bcnt, ref.counts)
    np.testing.assert_array_equal(bsum, ref.sums)


@pytest.mark.parametrize("mm", (1, 2, 3))
@pytest.mark.parametrize("case", CASE_IDS)
def test_oracle_hybrid(mx, case, mm):
    lo, hi, nb = hm.CASES[case]
    ref = mx.reference(case, mm=mm)
    got = po.execute_topk_hybrid(mx.seg.blob, list(hm.TERMS), [1.0] * 3, K,
                                 mx.bucket_col(case)[0], lo, hi, nb,
                                 min_match=mm)
    _check(got, ref, mx.expected_hits(ref, K, mm=mm))


@pytest.mark.parametrize("chain", ("max4", "ge_min", "lt_min", "ge_max",
                                   "lt_max", "between_empty", "between_all",
                                   "same_slot"))
@pytest.mark.parametrize("case", hm.CHAIN_CASES + ("c11_full_nb128",))
def test_oracle_hybrid_chain(mx, case, chain):
    nb = hm.CASES[case][2]
    preds = mx.chain_preds(case, chain)
    for mm in (1, 2):
        ref = mx.reference(case, chain, mm=mm)
        got = po.execute_topk_hybrid_chain(
            mx.seg.blob, list(hm.TERMS), [1.0] * 3, K,
            [mx.column(case, p[0]) for p in preds], [p[1] for p in preds],
            [p[2] for p in preds], [p[3] for p in preds], nb, min_match=mm)
        _check(got, ref, mx.expected_hits(ref, K, mm=mm))
