"""SUFFIX / CONTAINS / LIKE, negation and mask combination on every GPU
string path, over the LIKE matrix (tests/like_matrix.py): strlike_kernel,
strlike_fsst_kernel and the cooperative strlike_coop_kernel of sdb_scan.hip,
and the flagged store of strpred_kernel / strpred_fsst_kernel. One pytest case
per (path, case), so a failure names the kernel.

Paths: "raw" takes the cooperative kernel wherever the pattern is one
unanchored segment and the row-wise kernel otherwise; "raw_rowwise" sets the
SDB_LIKE_ROWWISE=1 test hook, which keeps every raw pattern on the row-wise
kernel; the three FSST encodings run strlike_fsst_kernel.

A device mask is read back row by row, as in tests/test_gpu_str_matrix.py:
scan_agg_hash grouped by the row-id column under [(slot, STRMASK, 0, 0)]
returns the passing row ids. Every expectation is Python's `re` (or plain
bytes operators) over the rows; all of it is integer and asserted exactly.
"""

import numpy as np
import pytest

import like_matrix as lmx
import serenedb_amd as sa
import str_matrix as smx

pytestmark = pytest.mark.gpu

PATHS = ("raw", "raw_rowwise", "fsst_auto", "fsst_escape", "fsst_max")
ENC = {"raw": "raw", "raw_rowwise": "raw", "fsst_auto": "fsst_auto",
       "fsst_escape": "fsst_escape", "fsst_max": "fsst_max"}
SLOT = {"raw": 0, "raw_rowwise": 0, "fsst_auto": 1, "fsst_escape": 2,
        "fsst_max": 3}
HOOK = "SDB_LIKE_ROWWISE"
ROWID, VAL, KEY_RAW, KEY_FOR = 0, 1, 2, 3      # table columns
STRMASK = 7
COUNT, SUM_I64 = 0, 1
GROUP_ROWS = 1025
NKEYS = 2048
ERR_INVALID = "rc=-1$"


@pytest.fixture(scope="module")
def ctx():
    c = sa.GpuContext(0)
    yield c
    c.close()


@pytest.fixture(autouse=True)
def hook_off(monkeypatch):
    monkeypatch.delenv(HOOK, raising=False)


def use_path(monkeypatch, path):
    if path == "raw_rowwise":
        monkeypatch.setenv(HOOK, "1")
    else:
        monkeypatch.delenv(HOOK, raising=False)


def load(ctx, cols, n=None, group_rows=GROUP_ROWS):
    return ctx.load_table(
        [cols.rowid[:n], cols.val[:n], cols.key[:n], cols.key[:n]],
        ["raw", "raw", "raw", "for"], group_rows=group_rows)


def attach(ctx, tab, slot, encoded):
    off, blob, syms = encoded
    if syms is None:
        ctx.attach_strcol(tab, slot, off, blob)
    else:
        ctx.attach_strcol_fsst(tab, slot, off, blob, syms)


@pytest.fixture(scope="module")
def base(ctx):
    """the 4099-row table, one encoding per slot"""
    mx = lmx.matrix()
    tab = load(ctx, mx)
    for enc in lmx.ENCODINGS:
        attach(ctx, tab, SLOT[enc], mx.encoded(enc))
    yield tab
    ctx.free_table(tab)


def like(ctx, tab, slot, case, **kw):
    pattern, escape = lmx.CASES[case][:2]
    ctx.strpred_like(tab, slot, pattern, escape, **kw)


def mask_rows(ctx, tab, slot, rows):
    keys, i64, _, passed = ctx.scan_agg_hash(
        tab, ROWID, max(rows, 64), [(slot, STRMASK, 0, 0)], [(0, COUNT)])
    assert (i64 == 1).all()
    assert passed == len(keys)
    return keys


def assert_rows(got, ref, values, what):
    want = np.flatnonzero(ref)
    if len(got) == len(want) and (got == want).all():
        return
    wrong = np.setxor1d(got, want)
    r = int(wrong[0])
    v = values[r] if r < len(values) else None
    raise AssertionError(
        f"{what}: {len(wrong)} rows differ; first row {r} "
        f"{'passes' if r in set(got.tolist()) else 'is dropped'} on the "
        f"device, len {None if v is None else len(v)} bytes "
        f"{None if v is None else v[:80]!r}")


def dense_count(ctx, tab, slot):
    """rows the dense scan counts under the mask: a stray bit at a row >=
    rows of the last mask word shows here"""
    i64, _, passed = ctx.scan_agg(tab, KEY_RAW, NKEYS,
                                  [(slot, STRMASK, 0, 0)], [(0, COUNT)])
    assert passed == int(i64.sum())
    return passed


# ---- the matrix ------------------------------------------------------------
@pytest.mark.parametrize("case", list(lmx.CASES))
@pytest.mark.parametrize("path", PATHS)
def test_matrix(ctx, base, monkeypatch, path, case):
    use_path(monkeypatch, path)
    mx = lmx.matrix()
    pattern, escape, _, op = lmx.CASES[case]
    like(ctx, base, SLOT[path], case)
    assert_rows(mask_rows(ctx, base, SLOT[path], mx.rows), mx.ref_mask(case),
                mx.values(), f"{path} LIKE {pattern!r} escape {escape!r}")
    if op is not None:      # the same literal through strpred_mask
        kind, lit = op
        like(ctx, base, SLOT[path], "empty")        # stale bits would show
        ctx.strpred_mask(base, SLOT[path], kind, lit)
        assert_rows(mask_rows(ctx, base, SLOT[path], mx.rows),
                    mx.ref_mask(case), mx.values(), f"{path} {kind} {lit!r}")


# ---- row counts around the 64-row mask word ----------------------------------
@pytest.mark.parametrize("n", lmx.PREFIX_ROWS)
@pytest.mark.parametrize("path", ["raw", "raw_rowwise", "fsst_auto"])
def test_row_counts(ctx, monkeypatch, path, n):
    use_path(monkeypatch, path)
    mx = lmx.matrix()
    tab = load(ctx, mx, n)
    try:
        attach(ctx, tab, 0, mx.encoded(ENC[path], n))
        case = lmx.ROWCOUNT_CASE
        ref = mx.ref_mask(case, n)
        like(ctx, tab, 0, case)
        assert_rows(mask_rows(ctx, tab, 0, n), ref, mx.values(n),
                    f"{path} rows={n} {case}")
        assert dense_count(ctx, tab, 0) == int(ref.sum())
        like(ctx, tab, 0, case, negate=True)
        assert_rows(mask_rows(ctx, tab, 0, n), ~ref, mx.values(n),
                    f"{path} rows={n} NOT {case}")
        assert dense_count(ctx, tab, 0) == n - int(ref.sum())
        like(ctx, tab, 0, "all")
        np.testing.assert_array_equal(mask_rows(ctx, tab, 0, n), np.arange(n))
        assert dense_count(ctx, tab, 0) == n
        like(ctx, tab, 0, "all", negate=True)
        assert len(mask_rows(ctx, tab, 0, n)) == 0
        assert dense_count(ctx, tab, 0) == 0
    finally:
        ctx.free_table(tab)


# ---- a literal split over adjacent rows ----------------------------------------
@pytest.mark.parametrize("variant", ["full", "short"])
@pytest.mark.parametrize("path", ["raw", "raw_rowwise", "fsst_escape"])
def test_split_geometry(ctx, monkeypatch, path, variant):
    use_path(monkeypatch, path)
    g = lmx.split(variant)
    tab = load(ctx, g.cols)
    try:
        attach(ctx, tab, 0, lmx.encode_rows(ENC[path], g.values()))
        for lit in lmx.SPLIT_LITS:
            ref = g.ref_mask(lit)
            ctx.strpred_like(tab, 0, b"%" + lmx.q(lit) + b"%", lmx.ESC)
            got = mask_rows(ctx, tab, 0, g.rows)
            assert_rows(got, ref, g.values(),
                        f"{path} {variant} contains {lit[:8]!r}")
            assert not set(got.tolist()) & set(g.halves[lit])
            assert (g.rows - 1 in got) == (variant == "full" and lit == g.last)
            ctx.strpred_mask(tab, 0, "contains", lit, negate=True)
            assert_rows(mask_rows(ctx, tab, 0, g.rows), ~ref, g.values(),
                        f"{path} {variant} NOT contains {lit[:8]!r}")
            assert dense_count(ctx, tab, 0) == g.rows - int(ref.sum())
    finally:
        ctx.free_table(tab)


# ---- a literal at every offset relative to a chunk edge --------------------------
@pytest.mark.parametrize("path", ["raw", "raw_rowwise"])
def test_chunk_geometry(ctx, monkeypatch, path):
    use_path(monkeypatch, path)
    g = lmx.chunk()
    tab = load(ctx, g.cols, group_rows=4096)
    try:
        ctx.attach_strcol(tab, 0, g.offsets, b"".join(g.values()))
        like(ctx, tab, 0, "contains_SA")
        got = mask_rows(ctx, tab, 0, g.rows)
        assert_rows(got, g.ref_mask(), g.values(), f"{path} chunk")
        assert len(got) == lmx.CHUNK_PAIRS
    finally:
        ctx.free_table(tab)


# ---- the grid-stride pass ----------------------------------------------------------
@pytest.fixture(scope="module")
def large(ctx):
    mx = smx.matrix("large")
    tab = ctx.load_table([mx.rowid, mx.val, mx.key, mx.key],
                         ["raw", "raw", "raw", "for"], group_rows=65536)
    attach(ctx, tab, 0, mx.encoded("raw"))
    attach(ctx, tab, 1, mx.encoded("fsst_auto"))
    yield tab
    ctx.free_table(tab)


@pytest.mark.parametrize("enc", ["raw", "fsst_auto"])
def test_grid_stride(ctx, large, enc):
    """4096*256 + 101 rows: past one pass of the row-wise launches and of
    the cooperative kernel's windows"""
    mx = smx.matrix("large")
    slot = {"raw": 0, "fsst_auto": 1}[enc]
    like(ctx, large, slot, lmx.LARGE_CASE)
    keys, i64, _, passed = ctx.scan_agg_hash(
        large, ROWID, 1 << 18, [(slot, STRMASK, 0, 0)], [(0, COUNT)])
    want = np.flatnonzero(lmx.smx_vocab_mask(lmx.LARGE_CASE)[mx.draw])
    assert passed == len(want) < (1 << 18)
    bad = np.setxor1d(keys, want)
    assert len(bad) == 0, f"{enc}: {len(bad)} rows differ, first {bad[:5]}"
    assert (i64 == 1).all()
    assert (keys >= smx.GRID_ROWS).sum() == smx.LARGE_TAIL


# ---- flags ---------------------------------------------------------------------------
def _old_ref(mx, op, lo, hi=None):
    m = np.array([smx.eval_case(v, op, lo, hi) for v in lmx.VOCAB])
    return m[mx.draw]


@pytest.mark.parametrize("path", ["raw", "raw_rowwise", "fsst_auto"])
def test_flags(ctx, monkeypatch, path):
    use_path(monkeypatch, path)
    mx = lmx.matrix()
    vals = mx.values()
    tab = load(ctx, mx)

    def rows():
        return mask_rows(ctx, tab, 0, mx.rows)

    # (how to compute it with flags, its reference): old ops and new ones
    preds = {
        "ge_a": (lambda **kw: ctx.strpred_mask(tab, 0, "ge", b"a", **kw),
                 _old_ref(mx, "ge", b"a")),
        "between": (lambda **kw: ctx.strpred_mask(
            tab, 0, "between", smx.S, b"a\x80", **kw),
            _old_ref(mx, "between", smx.S, b"a\x80")),
        "prefix_S": (lambda **kw: ctx.strpred_mask(
            tab, 0, "prefix", smx.S, **kw), _old_ref(mx, "prefix", smx.S)),
        "contains_ab": (lambda **kw: ctx.strpred_mask(
            tab, 0, "contains", b"ab", **kw),
            np.array([b"ab" in v for v in vals])),
        "suffix_a": (lambda **kw: ctx.strpred_mask(
            tab, 0, "suffix", b"a", **kw),
            np.array([v.endswith(b"a") for v in vals])),
        "like_ab_ab": (lambda **kw: like(ctx, tab, 0, "ab_ab", **kw),
                       mx.ref_mask("ab_ab")),
        "like_contains_S": (lambda **kw: like(ctx, tab, 0, "contains_S",
                                              **kw),
                            mx.ref_mask("contains_S")),
    }
    try:
        attach(ctx, tab, 0, mx.encoded(ENC[path]))
        # combining needs a mask computed since the attach
        for comb in ("and", "or"):
            with pytest.raises(RuntimeError, match=ERR_INVALID):
                ctx.strpred_mask(tab, 0, "ge", b"a", combine=comb)
            with pytest.raises(RuntimeError, match=ERR_INVALID):
                like(ctx, tab, 0, "contains_a", combine=comb)
        with pytest.raises(RuntimeError):       # and there is still none
            ctx.scan_agg(tab, KEY_RAW, NKEYS, [(0, STRMASK, 0, 0)],
                         [(0, COUNT)])
        for name, (run, ref) in preds.items():
            assert 0 < ref.sum() < mx.rows, name
            run(negate=True)
            assert_rows(rows(), ~ref, vals, f"{path} NOT {name}")
        names = list(preds)
        for i, a in enumerate(names):
            b = names[(i + 3) % len(names)]
            (run_a, ref_a), (run_b, ref_b) = preds[a], preds[b]
            run_a()
            run_b(combine="and")
            assert_rows(rows(), ref_a & ref_b, vals, f"{path} {a} AND {b}")
            run_a()
            run_b(combine="or")
            assert_rows(rows(), ref_a | ref_b, vals, f"{path} {a} OR {b}")
            run_a()
            run_b(negate=True, combine="and")
            assert_rows(rows(), ref_a & ~ref_b, vals,
                        f"{path} {a} AND NOT {b}")
            run_a(negate=True)
            run_b(negate=True, combine="or")
            assert_rows(rows(), ~ref_a | ~ref_b, vals,
                        f"{path} NOT {a} OR NOT {b}")
        # rejected calls leave the previous mask as it was
        run, ref = preds["like_ab_ab"]
        run()
        for bad in (lambda: ctx.strpred_mask(tab, 0, "ge", b"a", combine=6),
                    lambda: ctx.strpred_mask(tab, 0, "ge", b"a", combine=8),
                    lambda: ctx.strpred_mask(tab, 0, "contains", b"a",
                                             combine=16),
                    lambda: ctx.strpred_like(tab, 0, b"%", combine=6),
                    lambda: ctx.strpred_like(tab, 0, b"%", combine=1 << 31),
                    lambda: ctx.strpred_like(tab, 0, b"a_b"),
                    lambda: ctx.strpred_like(tab, 0, b"ab!", b"!"),
                    lambda: ctx.strpred_like(tab, 0, b"x" * 64),
                    lambda: ctx.strpred_like(tab, 0, b"%" * 256),
                    lambda: ctx.strpred_like(tab, 0, b"ab", b"%"),
                    lambda: ctx.strpred_like(tab, 0, b"ab", 256),
                    lambda: ctx.strpred_mask(tab, 0, "contains", b"x" * 64),
                    lambda: ctx.strpred_mask(tab, 0, 11, b"a")):
            with pytest.raises(RuntimeError, match=ERR_INVALID):
                bad()
            assert_rows(rows(), ref, vals, f"{path} after a rejected call")
    finally:
        ctx.free_table(tab)


# ---- malformed FSST rows ------------------------------------------------------------
def test_malformed_fsst_rows(ctx):
    off, blob, values = smx.malformed_escape()
    n = len(values)
    good = np.array([v is not None for v in values])
    assert n == 65 and np.flatnonzero(~good).tolist() == [3, 7]
    cols = lmx.Columns(n, 3)
    tab = load(ctx, cols)
    try:
        ctx.attach_strcol_fsst(tab, 0, off, blob, [])
        for case in lmx.CASES:
            ref = lmx.values_mask(case, values)
            for negate, want in ((False, ref), (True, good & ~ref)):
                like(ctx, tab, 0, case, negate=negate)
                got = mask_rows(ctx, tab, 0, n)
                assert_rows(got, want, values,
                            f"malformed {case} negate={negate}")
                assert not set(got.tolist()) & {3, 7}
                if case == "all":
                    assert len(got) == (0 if negate else n - 2)
        # the flagged old ops treat them alike
        ctx.strpred_mask(tab, 0, "prefix", b"", negate=True)
        assert len(mask_rows(ctx, tab, 0, n)) == 0
        ctx.strpred_mask(tab, 0, "lt", b"", negate=True)
        assert_rows(mask_rows(ctx, tab, 0, n), good, values, "NOT lt ''")
    finally:
        ctx.free_table(tab)


# ---- consumers of a LIKE mask ---------------------------------------------------------
def test_dense_scan_consumes_a_like_mask(ctx, base):
    mx = lmx.matrix()
    like(ctx, base, SLOT["fsst_auto"], "pct_ab_ab")
    ref = mx.ref_mask("pct_ab_ab")
    cnt = np.bincount(mx.key[ref], minlength=NKEYS).astype(np.int64)
    acc = np.zeros(NKEYS, dtype=np.uint64)
    np.add.at(acc, mx.key[ref], mx.val[ref].view(np.uint64))
    i64, _, passed = ctx.scan_agg(
        base, KEY_FOR, NKEYS, [(SLOT["fsst_auto"], STRMASK, 0, 0)],
        [(0, COUNT), (VAL, SUM_I64)])
    assert passed == int(ref.sum()) > 0
    np.testing.assert_array_equal(i64[:, 0], cnt)
    np.testing.assert_array_equal(i64[:, 1], acc.view(np.int64))


def test_group_by_string_under_its_own_like_mask(ctx, base):
    mx = lmx.matrix()
    slot = SLOT["raw"]
    like(ctx, base, slot, "contains_S", negate=True)
    ref = ~mx.ref_mask("contains_S")
    want = {}
    for i, v in zip(mx.draw[ref].tolist(), mx.val[ref].tolist()):
        c, s = want.get(lmx.VOCAB[i], (0, 0))
        want[lmx.VOCAB[i]] = (c + 1, s + v)
    want = {k: (c, smx.signed64(s % (1 << 64))) for k, (c, s) in want.items()}
    ks, i64, _, passed = ctx.scan_agg_hash_str(
        base, slot, 256, [(slot, STRMASK, 0, 0)],
        [(0, COUNT), (VAL, SUM_I64)], values=lmx.VOCAB)
    assert passed == int(ref.sum())
    got = {bytes(k): (int(i64[i, 0]), int(i64[i, 1]))
           for i, k in enumerate(ks)}
    assert got == want and 0 < len(got) < len(lmx.VOCAB)


def test_topn_consumes_a_like_mask(ctx, base):
    mx = lmx.matrix()
    slot = SLOT["fsst_max"]
    like(ctx, base, slot, "S_r")
    ref = mx.ref_mask("S_r")
    k = 25
    assert ref.sum() > k
    idx = np.flatnonzero(ref)
    order = idx[np.lexsort((idx, mx.val[idx]))][:k]
    rows, vals, isnull, passed = ctx.scan_topn(
        base, VAL, k, [(slot, STRMASK, 0, 0)])[:4]
    assert passed == int(ref.sum())
    np.testing.assert_array_equal(rows.astype(np.int64), order)
    np.testing.assert_array_equal(vals, mx.val[order])
    assert not isnull.any()


# ---- the five old ops, flags 0, after a LIKE mask ---------------------------------------
OLD_CASES = ("prefix_empty", "lt_empty", "eq_empty", "ge_80", "prefix_a",
             "between_a81_aff", "lt_abcdefghi", "prefix_S", "eq_SA",
             "between_S80_ff63")


@pytest.fixture(scope="module")
def smx_base(ctx):
    mx = smx.matrix("base")
    tab = ctx.load_table([mx.rowid, mx.val, mx.key, mx.key],
                         ["raw", "raw", "raw", "for"], group_rows=GROUP_ROWS)
    attach(ctx, tab, 0, mx.encoded("raw"))
    attach(ctx, tab, 1, mx.encoded("fsst_max"))
    yield tab
    ctx.free_table(tab)


@pytest.mark.parametrize("case", OLD_CASES)
@pytest.mark.parametrize("enc", ["raw", "fsst_max"])
def test_old_ops_unchanged(ctx, smx_base, enc, case):
    mx = smx.matrix("base")
    slot = {"raw": 0, "fsst_max": 1}[enc]
    # a LIKE mask first: every bit set, so a stale one would show
    ctx.strpred_like(smx_base, slot, b"%")
    assert len(mask_rows(ctx, smx_base, slot, mx.rows)) == mx.rows
    op, lo, hi, _ = smx.CASES[case]
    ctx.strpred_mask(smx_base, slot, op, lo, hi)
    assert_rows(mask_rows(ctx, smx_base, slot, mx.rows), mx.ref_mask(case),
                mx.values(), f"{enc} {case}")
    # and the other way round: no bit set before the old op
    ctx.strpred_like(smx_base, slot, b"%", negate=True)
    ctx.strpred_mask(smx_base, slot, op, lo, hi)
    assert_rows(mask_rows(ctx, smx_base, slot, mx.rows), mx.ref_mask(case),
                mx.values(), f"{enc} {case} after an empty mask")
