"""Block-fetch matrix, CPU side (tests/block_fetch_matrix.py): the three
builds really end the way they claim, fused blocks really start at every
byte residue, the straddling and the never-straddling widths are really
there, and the CPU oracle reproduces the numpy fp32 reference bit for bit.
tests/test_gpu_block_fetch_matrix.py then holds every GPU path to that
reference and cannot silently cover nothing."""

import numpy as np
import pytest

import block_fetch_matrix as bf

SCORERS = ("bm25", "tfidf_norm")


@pytest.fixture(scope="module")
def builds():
    return bf.builds()


def test_corpus_shape(builds):
    assert set(builds) == set(bf.BUILDS)
    assert 3 * bf.WIN < bf.DOC_COUNT < 3 * bf.WIN + 1000
    first = builds[bf.BUILDS[0]]
    for m in builds.values():
        assert m.names[:-1] == first.names[:-1] and m.names[-1] == "end"
        assert m.norms is first.norms


@pytest.mark.parametrize("build", bf.BUILDS)
def test_final_block_shape(builds, build):
    """The last bytes of the payload belong to the block the build is named
    for, and the blob's pad behind them covers the decoders' over-read."""
    m = builds[build]
    blks, payload_size, room = m.parse()
    last = blks[-1][-1]
    assert last["payload_end"] == payload_size
    # the decoders touch up to 20 bytes past a stream; the builder leaves
    # SDB_PAYLOAD_TAIL_PAD = 64 behind the payload (sdb_format.h)
    assert room - payload_size >= 64
    if build == "tail_end":
        assert not last["fused"] and last["len"] == 5
        assert blks[-1][-2]["fused"]
    else:
        assert last["fused"] and last["len"] == bf.BLOCK
        assert last["abs_end"] == payload_size   # norm stream ends the blob
        if build == "wide_end":
            # 31 is the widest bitpack tag there is (SDB_E_BITPACK_31)
            assert (last["fb"], last["nb"]) == (31, 31)
        else:
            assert (last["db"], last["fb"], last["nb"]) == (2, 2, 2)


@pytest.mark.parametrize("build", bf.BUILDS)
def test_residues_widths_and_straddles(builds, build):
    m = builds[build]
    blks, _, _ = m.parse()
    res_abs, res_rel = set(), set()
    dbs, fbs, nbs = set(), set(), set()
    crossing = set()
    tails = set()
    for t, recs in enumerate(blks):
        docs = m.postings[t][0]
        assert sum(r["len"] for r in recs) == len(docs)
        for i, r in enumerate(recs):
            assert r["last"] == int(docs[bf.BLOCK * i + r["len"] - 1])
            if not r["fused"]:
                if r["len"] < bf.BLOCK:
                    tails.add(r["len"])
                continue
            assert r["len"] == bf.BLOCK
            res_abs.add(r["abs_off"] % 8)
            res_rel.add(r["doc_off"] % 8)
            dbs.add(r["db"])
            fbs.add(r["fb"])
            nbs.add(r["nb"])
            first = int(docs[bf.BLOCK * i])
            crossing.add((first - 1) // bf.WIN != (r["last"] - 1) // bf.WIN)
    # every residue of a fused block's start, in the payload section (what
    # the device address sees) and within its term
    assert res_abs == set(range(8))
    assert res_rel == set(range(8))
    # the width terms came out fused at their pinned widths
    assert fbs >= set(bf.WIDTHS)
    assert nbs >= set(bf.WIDTHS)
    assert dbs >= set(bf.TERM_DOC_WIDTHS) | set(bf.ROAMING_DOC_WIDTHS)
    assert crossing == {False, True}
    assert tails >= set(range(1, len(bf.WIDTHS) + 1))
    # nine fused blocks in a row step through all residues by themselves
    r9 = blks[m.idx["res9"]]
    assert len(r9) == 9 and all(r["fused"] for r in r9)
    assert {r["doc_off"] % 8 for r in r9[:8]} == set(range(8))


def _check_oracle(m, terms, boosts, k, scorer):
    rd, rs, rtotal = m.ref_topk(terms, boosts, k, scorer)
    od, os_, ototal = m.oracle_topk(terms, boosts, k, scorer)
    assert ototal == rtotal
    np.testing.assert_array_equal(od, rd)
    np.testing.assert_array_equal(os_.view(np.uint32), rs.view(np.uint32))


@pytest.mark.parametrize("scorer", SCORERS)
@pytest.mark.parametrize("build", bf.BUILDS)
def test_oracle_equals_numpy(builds, build, scorer):
    """every plan the GPU test runs: each term alone with k = df + 1, the
    OR of all terms and the 4-term plans with k = all matches and 10"""
    m = builds[build]
    for t, (docs, _) in enumerate(m.postings):
        _check_oracle(m, [t], [1.0], len(docs) + 1, scorer)
        assert m.ref_topk([t], [1.0], 1, scorer)[2] == len(docs)
    for g in list(m.groups.values()) + list(m.small_groups.values()):
        ones = [1.0] * len(g)
        n_all = len(m.ref_scores(g, ones, scorer)[0])
        for k in (n_all, 10):
            _check_oracle(m, g, ones, k, scorer)
