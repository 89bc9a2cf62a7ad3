"""Every GPU top-k path on the three block-fetch builds
(tests/block_fetch_matrix.py): the over-read behind the last stream of the
payload, fused blocks at every byte residue, straddling and non-straddling
widths. Doc ids, score bits and totals must equal the numpy fp32 reference
exactly; tests/test_block_fetch_matrix.py proves that reference equals the
CPU oracle and that the corpus holds the shapes it claims."""

import numpy as np
import pytest

import block_fetch_matrix as bf
import serenedb_amd as sa

pytestmark = pytest.mark.gpu

SCORERS = ("bm25", "tfidf_norm")


@pytest.fixture(scope="module")
def ctx():
    c = sa.GpuContext(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def segs(ctx):
    return {b: ctx.load_segment(m.blob) for b, m in bf.builds().items()}


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def check_plan(ctx, seg, m, terms, k, scorer, label):
    ones = [1.0] * len(terms)
    hits, total = ctx.execute_topk([seg], terms, ones, k, scorer=scorer)
    rd, rs, rtotal = m.ref_topk(terms, ones, k, scorer)
    what = f"{label} scorer={scorer} k={k}"
    assert total == rtotal, what
    np.testing.assert_array_equal(hits["doc"], rd, err_msg=what)
    np.testing.assert_array_equal(bits(hits["score"]), bits(rs),
                                  err_msg=what)


def n_matches(m, terms):
    return len(np.unique(np.concatenate([m.postings[t][0] for t in terms])))


def run_singles_and_or(ctx, seg, m, scorer, label):
    for t, (docs, _) in enumerate(m.postings):
        check_plan(ctx, seg, m, [t], len(docs) + 1, scorer,
                   f"{label} {m.names[t]}")
    g = m.groups["all"]
    for k in (n_matches(m, g), 10):
        check_plan(ctx, seg, m, g, k, scorer, f"{label} all")


@pytest.mark.parametrize("build", bf.BUILDS)
def test_decode_term(ctx, segs, build):
    m = bf.builds()[build]
    for t, (docs, freqs) in enumerate(m.postings):
        ddocs, dfreqs = ctx.decode_term(segs[build], t, len(docs))
        np.testing.assert_array_equal(ddocs, docs, err_msg=m.names[t])
        np.testing.assert_array_equal(dfreqs, freqs, err_msg=m.names[t])


@pytest.mark.parametrize("scorer", SCORERS)
@pytest.mark.parametrize("build", bf.BUILDS)
def test_sweep(ctx, segs, build, scorer):
    run_singles_and_or(ctx, segs[build], bf.builds()[build], scorer,
                       f"{build} sweep")


@pytest.mark.parametrize("scorer", SCORERS)
@pytest.mark.parametrize("build", bf.BUILDS)
def test_general_kernel(ctx, segs, build, scorer, monkeypatch):
    monkeypatch.setenv("SDB_TOPK_PATH", "general")
    run_singles_and_or(ctx, segs[build], bf.builds()[build], scorer,
                       f"{build} general")


@pytest.mark.parametrize("scorer", SCORERS)
@pytest.mark.parametrize("build", bf.BUILDS)
def test_wave_kernel(ctx, segs, build, scorer, monkeypatch):
    monkeypatch.setenv("SDB_TOPK_PATH", "wave")
    m = bf.builds()[build]
    for name, g in m.small_groups.items():
        for k in (n_matches(m, g), 10):
            check_plan(ctx, segs[build], m, g, k, scorer,
                       f"{build} wave {name}")
