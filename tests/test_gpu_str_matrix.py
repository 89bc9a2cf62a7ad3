"""Every GPU string path on the string-predicate matrix
(tests/str_matrix.py): strpred_kernel, strpred_fsst_kernel and
strhash_kernel of sdb_scan.hip over raw slots and three FSST encodings, with
bytes on both sides of the sign boundary, literals of 0..63 bytes, rows
that differ at and beyond byte 62, a full and an empty symbol table, row
counts around the 64-row mask word, the grid-stride pass above 4096*256
rows, the life cycle of the four slot masks and every consumer of
SDB_PRED_STRMASK. One pytest case per (encoding, operation), so a failure
names the path.

A device mask is read back row by row: scan_agg_hash grouped by the row-id
column under [(slot, STRMASK, 0, 0)] returns the passing row ids, which must
equal np.flatnonzero of the reference mask. Expected values are Python bytes
comparisons and Python-int sums (tests/test_str_matrix.py proves them); all
aggregates are integer and asserted exactly.
"""

import numpy as np
import pytest

import serenedb_amd as sa
import str_matrix as smx
from oracle import pyoracle as po

pytestmark = pytest.mark.gpu

ENCS = smx.ENCODINGS
SLOT = {e: i for i, e in enumerate(ENCS)}
ROWID, VAL, KEY_RAW, KEY_FOR = 0, 1, 2, 3      # table columns
STRMASK, GE = 7, 2           # SdbPredOp
COUNT, SUM_I64 = 0, 1
GROUP_ROWS = 1025       # mask words straddle the row groups
NKEYS = 2048


@pytest.fixture(scope="module")
def ctx():
    c = sa.GpuContext(0)
    yield c
    c.close()


def load(ctx, mx, n=None, group_rows=GROUP_ROWS):
    return ctx.load_table(
        [mx.rowid[:n], mx.val[:n], mx.key[:n], mx.key[:n]],
        ["raw", "raw", "raw", "for"], group_rows=group_rows)


def attach(ctx, tab, slot, mx, enc, n=None):
    off, blob, syms = mx.encoded(enc, n)
    if syms is None:
        ctx.attach_strcol(tab, slot, off, blob)
    else:
        ctx.attach_strcol_fsst(tab, slot, off, blob, syms)


@pytest.fixture(scope="module")
def base(ctx):
    """the 4099-row table, one encoding per slot"""
    mx = smx.matrix("base")
    tab = load(ctx, mx)
    for enc in ENCS:
        attach(ctx, tab, SLOT[enc], mx, enc)
    yield tab
    ctx.free_table(tab)


@pytest.fixture
def scratch(ctx):
    """a 4099-row table of its own for the tests that re-attach slots"""
    tab = load(ctx, smx.matrix("base"))
    yield tab
    ctx.free_table(tab)


def compute(ctx, tab, slot, case):
    op, lo, hi, _ = smx.CASES[case]
    ctx.strpred_mask(tab, slot, op, lo, hi)


def mask_rows(ctx, tab, slots, rows, extra=()):
    """(row ids passing the AND of the slots' masks, rows_passed)"""
    preds = [(s, STRMASK, 0, 0) for s in slots] + list(extra)
    keys, i64, _, passed = ctx.scan_agg_hash(
        tab, ROWID, max(rows, 64), preds, [(0, COUNT)])
    assert (i64 == 1).all()
    assert passed == len(keys)
    return keys, passed


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


@pytest.mark.parametrize("case", list(smx.CASES))
@pytest.mark.parametrize("enc", ENCS)
def test_mask(ctx, base, enc, case):
    mx = smx.matrix("base")
    compute(ctx, base, SLOT[enc], case)
    got, _ = mask_rows(ctx, base, [SLOT[enc]], mx.rows)
    assert_rows(got, mx.ref_mask(case), mx.values(),
                f"{enc} {case} {smx.CASES[case][:3]}")


@pytest.mark.parametrize("n", smx.PREFIX_ROWS)
@pytest.mark.parametrize("enc", ["raw", "fsst_auto"])
def test_row_counts(ctx, enc, n):
    """tail bits of the last mask word: 1, 63, 64, 65 and 257 rows"""
    mx = smx.matrix("base")
    tab = load(ctx, mx, n)
    try:
        attach(ctx, tab, 0, mx, enc, n)
        compute(ctx, tab, 0, smx.ROWCOUNT_CASE)
        got, _ = mask_rows(ctx, tab, [0], n)
        assert_rows(got, mx.ref_mask(smx.ROWCOUNT_CASE, n), mx.values(n),
                    f"{enc} rows={n} {smx.ROWCOUNT_CASE}")
        compute(ctx, tab, 0, "prefix_empty")
        got, passed = mask_rows(ctx, tab, [0], n)
        assert passed == n
        np.testing.assert_array_equal(got, np.arange(n))
        # the dense scan counts the same rows (no bit set beyond row n-1)
        i64, _, passed = ctx.scan_agg(tab, KEY_RAW, NKEYS,
                                      [(0, STRMASK, 0, 0)], [(0, COUNT)])
        assert passed == n and int(i64.sum()) == n
    finally:
        ctx.free_table(tab)


@pytest.fixture(scope="module")
def large(ctx):
    mx = smx.matrix("large")
    tab = load(ctx, mx, group_rows=65536)
    attach(ctx, tab, 0, mx, "raw")
    attach(ctx, tab, 1, mx, "fsst_auto")
    yield tab
    ctx.free_table(tab)


@pytest.mark.parametrize("enc", ["raw", "fsst_auto"])
def test_grid_stride_mask(ctx, large, enc):
    """4096*256 + 101 rows: the rows above 1,048,576 are the second pass of
    the r += stride loop, its ballot word store included"""
    mx = smx.matrix("large")
    slot = {"raw": 0, "fsst_auto": 1}[enc]
    compute(ctx, large, slot, smx.LARGE_CASE)
    keys, i64, _, passed = ctx.scan_agg_hash(
        large, ROWID, 65536, [(slot, STRMASK, 0, 0)], [(0, COUNT)])
    ref = mx.ref_mask(smx.LARGE_CASE)
    want = np.flatnonzero(ref)
    assert passed == len(want) < 65536
    bad = np.setxor1d(keys, want)
    assert len(bad) == 0, f"{enc}: {len(bad)} rows differ, first {bad[:5]}"
    assert (i64 == 1).all()
    assert (keys >= smx.GRID_ROWS).sum() == (smx.LARGE_TAIL + 1) // 2


@pytest.mark.parametrize("enc", ["raw", "fsst_auto"])
def test_grid_stride_hash(ctx, large, enc):
    """strhash_kernel's second pass: counts per string over all rows"""
    mx = smx.matrix("large")
    slot = {"raw": 0, "fsst_auto": 1}[enc]
    hs, i64, _, passed = ctx.scan_agg_hash_str(
        large, slot, 256, [], [(0, COUNT), (ROWID, SUM_I64)])
    assert passed == mx.rows
    h = smx.vocab_hashes()
    order = np.argsort(h)
    np.testing.assert_array_equal(hs, h[order])
    cnt = np.bincount(mx.draw, minlength=len(smx.VOCAB))
    np.testing.assert_array_equal(i64[:, 0], cnt[order])
    sums = np.zeros(len(smx.VOCAB), dtype=np.int64)
    np.add.at(sums, mx.draw, mx.rowid)
    np.testing.assert_array_equal(i64[:, 1], sums[order])


def test_recompute_clears_stale_bits(ctx, scratch):
    mx = smx.matrix("base")
    attach(ctx, scratch, 0, mx, "raw")
    compute(ctx, scratch, 0, "prefix_empty")
    _, passed = mask_rows(ctx, scratch, [0], mx.rows)
    assert passed == mx.rows            # every bit was set ...
    compute(ctx, scratch, 0, "eq_absent")
    got, passed = mask_rows(ctx, scratch, [0], mx.rows)
    assert passed == 0 and len(got) == 0    # ... and every bit is cleared
    i64, _, passed = ctx.scan_agg(scratch, KEY_FOR, NKEYS,
                                  [(0, STRMASK, 0, 0)], [(0, COUNT)])
    assert passed == 0 and not i64.any()


def test_slots_are_independent_and_and_together(ctx, base):
    mx = smx.matrix("base")
    vals = mx.values()
    a, b = "prefix_S", "ge_SA"
    ra, rb = mx.ref_mask(a), mx.ref_mask(b)
    both = ra & rb
    assert 0 < both.sum() < min(ra.sum(), rb.sum())
    compute(ctx, base, 0, a)
    assert_rows(mask_rows(ctx, base, [0], mx.rows)[0], ra, vals, "slot 0")
    for other in (1, 2, 3):
        compute(ctx, base, other, b)
        assert_rows(mask_rows(ctx, base, [other], mx.rows)[0], rb, vals,
                    f"slot {other}")
        assert_rows(mask_rows(ctx, base, [0], mx.rows)[0], ra, vals,
                    f"slot 0 after slot {other} was recomputed")
        assert_rows(mask_rows(ctx, base, [0, other], mx.rows)[0], both, vals,
                    f"slot 0 AND slot {other}")
    # and with a numeric predicate behind the two masks
    lit = int(np.median(mx.val))
    got, _ = mask_rows(ctx, base, [1, 0], mx.rows,
                       extra=[(VAL, GE, lit, 0)])
    assert_rows(got, both & (mx.val >= lit), vals, "two masks AND val >= lit")


def test_reattach_resets_the_mask(ctx, scratch):
    mx = smx.matrix("base")
    vals = mx.values()
    pred = [(2, STRMASK, 0, 0)]
    attach(ctx, scratch, 2, mx, "raw")
    with pytest.raises(RuntimeError):       # attached, no mask yet
        ctx.scan_agg(scratch, KEY_RAW, NKEYS, pred, [(0, COUNT)])
    compute(ctx, scratch, 2, "prefix_a")
    assert_rows(mask_rows(ctx, scratch, [2], mx.rows)[0],
                mx.ref_mask("prefix_a"), vals, "raw slot")
    for enc in ("fsst_max", "raw"):
        attach(ctx, scratch, 2, mx, enc)
        with pytest.raises(RuntimeError):
            ctx.scan_agg(scratch, KEY_RAW, NKEYS, pred, [(0, COUNT)])
        with pytest.raises(RuntimeError):
            ctx.scan_agg_hash(scratch, ROWID, 8192, pred, [(0, COUNT)])
        with pytest.raises(RuntimeError):
            ctx.scan_agg_hash_str(scratch, 2, 256, pred, [(0, COUNT)])
        compute(ctx, scratch, 2, "lt_S80")
        assert_rows(mask_rows(ctx, scratch, [2], mx.rows)[0],
                    mx.ref_mask("lt_S80"), vals, f"re-attached as {enc}")


def _dense_ref(mx, mask, col):
    cnt = np.bincount(mx.key[mask], minlength=NKEYS).astype(np.int64)
    acc = np.zeros(NKEYS, dtype=np.uint64)
    np.add.at(acc, mx.key[mask], col[mask].view(np.uint64))
    return cnt, acc.view(np.int64)


@pytest.mark.parametrize("key", ["key_raw", "key_for"])
def test_dense_scan_consumes_the_mask(ctx, base, key):
    mx = smx.matrix("base")
    kcol = {"key_raw": KEY_RAW, "key_for": KEY_FOR}[key]
    for enc, case in (("raw", "between_SA_S80"), ("fsst_max", "ge_ff63"),
                      ("fsst_auto", "lt_a80")):
        compute(ctx, base, SLOT[enc], case)
        ref = mx.ref_mask(case)
        cnt, ids = _dense_ref(mx, ref, mx.rowid)
        i64, _, passed = ctx.scan_agg(
            base, kcol, NKEYS, [(SLOT[enc], STRMASK, 0, 0)],
            [(0, COUNT), (ROWID, SUM_I64)])
        what = f"{key} {enc} {case}"
        assert passed == int(ref.sum()), what
        np.testing.assert_array_equal(i64[:, 0], cnt, err_msg=what)
        np.testing.assert_array_equal(i64[:, 1], ids, err_msg=what)


@pytest.mark.parametrize("key", ["key_raw", "key_for"])
def test_sum_over_the_column_numbered_like_the_slot(ctx, base, key):
    """STRMASK on slot 1 with SUM_I64 over column 1: the predicate's `col`
    is a slot number, so the sum must read column 1 and not reuse what the
    STRMASK predicate staged (the group key)"""
    mx = smx.matrix("base")
    kcol = {"key_raw": KEY_RAW, "key_for": KEY_FOR}[key]
    assert VAL == 1 and not np.array_equal(mx.val, mx.key)
    case = "prefix_S"
    compute(ctx, base, 1, case)
    ref = mx.ref_mask(case)
    lit = int(np.median(mx.val))
    num = mx.val >= lit
    assert 0 < (ref & num).sum() < ref.sum()
    for preds, mask in (
            ([(1, STRMASK, 0, 0)], ref),
            ([(1, STRMASK, 0, 0), (VAL, GE, lit, 0)], ref & num),
            ([(VAL, GE, lit, 0), (1, STRMASK, 0, 0)], ref & num)):
        cnt, sums = _dense_ref(mx, mask, mx.val)
        for aggs, q in (([(0, COUNT), (VAL, SUM_I64)], 1),
                        ([(VAL, SUM_I64), (0, COUNT)], 0)):
            i64, _, passed = ctx.scan_agg(base, kcol, NKEYS, preds, aggs)
            what = f"{key} preds={preds} aggs={aggs}"
            assert passed == int(mask.sum()), what
            np.testing.assert_array_equal(i64[:, q], sums, err_msg=what)
            np.testing.assert_array_equal(i64[:, 1 - q], cnt, err_msg=what)


def _check_group_by(ctx, tab, mx, slot, preds, mask, what):
    ref = mx.ref_group_by(mask)
    # values=None: the hashes themselves, signed-i64 ascending
    hs, i64, _, _ = ctx.scan_agg_hash_str(tab, slot, 256, preds,
                                          [(0, COUNT)])
    want = sorted(smx.signed64(po.fnv1a64(k)) for k in ref)
    hs = [int(h) for h in hs]
    assert hs == want, (
        f"{what}: {len(hs)} groups for {len(want)} strings, "
        f"{len(set(hs) - set(want))} of them no string's FNV-1a hash"
        if set(hs) != set(want) else f"{what}: hashes out of order")
    assert want[0] < 0 < want[-1]
    # values=: hashes resolved to strings, collisions checked by the wrapper
    ks, i64, _, passed = ctx.scan_agg_hash_str(
        tab, slot, 256, preds, [(0, COUNT), (VAL, SUM_I64)],
        values=smx.VOCAB)
    assert passed == sum(c for c, _ in ref.values()), what
    got = {bytes(k): (int(i64[i, 0]), int(i64[i, 1]))
           for i, k in enumerate(ks)}
    assert len(got) == len(ks), what
    missing = sorted(set(ref) - set(got), key=len)
    assert got == ref, (
        f"{what}: {len(missing)} of {len(ref)} groups missing, "
        f"{len(set(got) - set(ref))} unexpected; first missing "
        f"{missing[0][:40]!r} len {len(missing[0])}" if missing else what)


@pytest.mark.parametrize("enc", ENCS)
def test_group_by_string(ctx, base, enc):
    mx = smx.matrix("base")
    _check_group_by(ctx, base, mx, SLOT[enc], [], None, f"{enc} all rows")


@pytest.mark.parametrize("enc", ENCS)
def test_group_by_string_under_mask(ctx, base, enc):
    mx = smx.matrix("base")
    case = "between_S_ff63"
    compute(ctx, base, SLOT[enc], case)
    _check_group_by(ctx, base, mx, SLOT[enc],
                    [(SLOT[enc], STRMASK, 0, 0)], mx.ref_mask(case),
                    f"{enc} {case}")


def test_malformed_fsst_rows(ctx):
    """a code beyond the symbol table and a row ending in a bare escape are
    caught before any read: such rows match no predicate and group under
    the sentinel key"""
    mx = smx.matrix("base")
    off, blob, values = smx.malformed_escape()
    n = len(values)
    good = np.array([v is not None for v in values])
    tab = load(ctx, mx, n)
    try:
        ctx.attach_strcol_fsst(tab, 0, off, blob, [])
        cases = [(name,) + smx.CASES[name][:3] for name in smx.CASES]
        cases.append(("ge_empty", "ge", b"", None))
        for name, op, lo, hi in cases:
            ctx.strpred_mask(tab, 0, op, lo, hi)
            ref = np.array([v is not None and smx.eval_case(v, op, lo, hi)
                            for v in values])
            got, _ = mask_rows(ctx, tab, [0], n)
            assert_rows(got, ref, values, f"malformed {name}")
            assert not set(got.tolist()) & {3, 7}
            if name in ("prefix_empty", "ge_empty"):
                assert len(got) == n - 2
        hs, i64, _, passed = ctx.scan_agg_hash_str(
            tab, 0, 256, [], [(0, COUNT), (ROWID, SUM_I64)])
        assert passed == n
        ref = {}
        for r, v in enumerate(values):
            k = smx.MALFORMED_KEY if v is None else \
                smx.signed64(po.fnv1a64(v))
            c, s = ref.get(k, (0, 0))
            ref[k] = (c + 1, s + r)
        assert ref[smx.MALFORMED_KEY] == (2, 10)
        assert [int(h) for h in hs] == sorted(ref)
        assert int(hs[0]) == smx.MALFORMED_KEY
        assert [(int(c), int(s)) for c, s in i64] == \
            [ref[k] for k in sorted(ref)]
        assert good.sum() == n - 2
    finally:
        ctx.free_table(tab)
