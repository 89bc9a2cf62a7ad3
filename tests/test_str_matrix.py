"""The string-predicate matrix (tests/str_matrix.py) is what it claims, and
its references are sound — all on the CPU. The GPU half is
tests/test_gpu_str_matrix.py."""

import numpy as np
import pytest

import serenedb_amd as sa
import str_matrix as smx
from oracle import pyoracle as po

FSST = ("fsst_auto", "fsst_escape", "fsst_max")
S, SA, FF = smx.S, smx.SA, smx.FF


@pytest.fixture(scope="module")
def mx():
    return smx.matrix("base")


def _codes(enc_row, symbols):
    """[(code or None for an escape, decoded offset, decoded bytes)]"""
    out, i, pos = [], 0, 0
    while i < len(enc_row):
        c = enc_row[i]
        if c == 255:
            out.append((None, pos, enc_row[i + 1:i + 2]))
            i += 2
        else:
            out.append((c, pos, symbols[c]))
            i += 1
        pos += len(out[-1][2])
    return out


def test_vocabulary_classes(mx):
    assert all(type(v) is bytes for v in smx.VOCAB)
    assert 24 <= len(smx.VOCAB) <= 60
    lens = {len(v) for v in smx.VOCAB}
    assert {0, 1, 7, 8, 9, 62, 63, 64, 65} <= lens
    assert any(180 <= n <= 220 for n in lens)
    assert any(900 <= n <= 1100 for n in lens)
    have = set(smx.VOCAB)
    assert {b"\x00", b"\x7f", b"\x80", b"\xfe", FF, FF + FF} <= have
    assert {b"a", b"a\x00", b"a\x7f", b"a\x80", b"a\x81", b"a\xff"} <= have
    assert {b"abcdefg", b"abcdefgh", b"abcdefghi", b"abcdefgi",
            b"abcdefgh\xff"} <= have
    assert {FF * 62, FF * 63, FF * 64} <= have
    # the stem: 62 bytes, no two equal 8-byte windows
    wins = [S[i:i + 8] for i in range(55)]
    assert len(S) == 62 and len(set(wins)) == 55
    assert S in have
    at62 = {v[62] for v in have if len(v) == 63 and v.startswith(S)}
    assert at62 == set(smx.X) and min(at62) < 0x80 <= max(at62)
    for x in (0x41, 0x80):      # differ at index 63 only
        assert {smx.sx(x) + b"\x00", smx.sx(x) + b"\x01"} <= have
    assert any(v.startswith(S) and v.endswith(b"r" * 100) for v in have)
    assert any(v.startswith(S) and v.endswith(FF * 900) for v in have)
    # every class is a row of the base table and of each longer prefix
    assert mx.rows == smx.BASE_ROWS == 4099
    assert mx.values(len(smx.VOCAB)) == list(smx.VOCAB)
    assert set(mx.values()) == have
    assert len(smx.VOCAB) <= 63 and smx.PREFIX_ROWS == (1, 63, 64, 65, 257)
    assert mx.val.min() < -(1 << 62) and mx.val.max() > (1 << 62)


def test_case_table_covers_the_issue():
    by_op = {}
    for op, lo, hi, _ in smx.CASES.values():
        assert len(lo) <= smx.STRLIT_MAX and len(hi or b"") <= smx.STRLIT_MAX
        by_op.setdefault(op, set()).add(len(lo))
        if op == "between":
            by_op.setdefault("between_hi", set()).add(len(hi))
    for op in ("lt", "ge", "eq", "prefix"):
        assert {1, 2, 8, 9, 62, 63} <= by_op[op], op
    assert 0 in by_op["lt"] and 0 in by_op["eq"] and 0 in by_op["prefix"]
    assert {0, 1, 2, 8, 9, 62, 63} <= by_op["between"]
    assert {1, 2, 8, 9, 63} <= by_op["between_hi"]
    c = smx.CASES
    for op in ("lt", "ge", "eq", "prefix"):
        assert c[f"{op}_80"][1] == b"\x80"
        assert c[f"{op}_a80"][1] == b"a\x80"
        assert c[f"{op}_SA"][1] == SA and len(SA) == 63
    assert c["prefix_S"][1] == S and c["between_S_ff63"][1:3] == (S, FF * 63)
    assert c["between_lo_eq_hi"][1] == c["between_lo_eq_hi"][2]
    assert c["between_lo_gt_hi"][1] > c["between_lo_gt_hi"][2]
    assert {len(x) for x in c["between_SA_S80"][1:3]} == {63}
    have = set(smx.VOCAB)
    # equal to a row / proper prefix of rows / a row is its proper prefix
    assert c["eq_abcdefgh"][1] in have
    assert sum(v.startswith(b"a") and v != b"a" for v in have) > 3
    lit = c["lt_a80_00"][1]
    assert lit not in have and lit[:-1] in have
    assert c["ge_a80_00"][1] == c["between_a_a80_00"][2] == lit
    hi = c["between_hi_is_prefix"][2]
    assert any(v.startswith(hi) and v != hi for v in have)
    assert c["eq_absent"][1] not in have


def test_ref_mask_is_the_oracle(mx):
    vals = mx.values()
    for name, (op, lo, hi, _) in smx.CASES.items():
        np.testing.assert_array_equal(
            mx.ref_mask(name), po.str_pred_mask(vals, op, lo, hi),
            err_msg=name)


def test_every_case_splits_the_rows(mx):
    declared = {n: d for n, (_, _, _, d) in smx.CASES.items() if d}
    assert declared == {"prefix_empty": "all", "lt_empty": "none",
                        "eq_absent": "none", "between_lo_gt_hi": "none"}
    for name in smx.CASES:
        for n in (None, 257):
            passed = int(mx.ref_mask(name, n).sum())
            rows = n or mx.rows
            want = {"all": rows, "none": 0}.get(declared.get(name))
            if want is None:
                assert 0 < passed < rows, (name, n)
            else:
                assert passed == want, (name, n)
    assert 0 < int(mx.ref_mask(smx.ROWCOUNT_CASE, 1).sum())  # row 0 passes
    for n in smx.PREFIX_ROWS[1:]:
        assert 0 < int(mx.ref_mask(smx.ROWCOUNT_CASE, n).sum()) < n


def test_63_byte_cases_reach_beyond_the_literal():
    """a row longer than 63 bytes on both sides of every 63-byte case. EQ
    cannot accept one: there a longer row that starts with the literal is
    among the rejected."""
    n63 = 0
    for name, (op, lo, hi, _) in smx.CASES.items():
        if max(len(lo), len(hi or b"")) != 63:
            continue
        n63 += 1
        m = smx.vocab_mask(name)
        acc = [v for v, k in zip(smx.VOCAB, m) if k and len(v) > 63]
        rej = [v for v, k in zip(smx.VOCAB, m) if not k and len(v) > 63]
        assert rej, name
        if op == "eq":
            assert any(v.startswith(lo) for v in rej), name
        else:
            assert acc, name
    assert n63 >= 10


@pytest.mark.parametrize("enc", FSST)
def test_fsst_decodes_back(mx, enc):
    for geom, n in (("base", None), ("base", 65), ("large", None)):
        g = smx.matrix(geom)
        off, blob, syms = g.encoded(enc, n)
        rows = n or g.rows
        assert len(off) == rows + 1 and off[0] == 0 and off[-1] == len(blob)
        assert len(syms) <= 254 and all(1 <= len(s) <= 8 for s in syms)
    per, syms = smx.vocab_encoded(enc)
    for v, e in zip(smx.VOCAB, per):
        assert po.fsst_decode(e, syms) == v
    # the rows really are the joined per-entry encodings
    off, blob, _ = mx.encoded(enc)
    for r in (0, 1, 62, 63, 64, 4098):
        assert po.fsst_decode(blob[int(off[r]):int(off[r + 1])], syms) == \
            smx.VOCAB[mx.draw[r]]
    roff, rblob, none = mx.encoded("raw")
    assert none is None
    woff, wblob = sa.encode_col_str_raw(mx.values())
    assert rblob == wblob
    np.testing.assert_array_equal(roff, woff)


def test_fsst_auto_is_the_project_encoder(mx):
    aoff, ablob, asyms = smx.auto_encoded()
    off, blob, syms = mx.encoded("fsst_auto")
    assert syms == list(asyms) and blob == ablob
    np.testing.assert_array_equal(off, aoff)
    assert len(syms) == 254 and len({len(s) for s in syms}) >= 3
    assert any(0xFF in s for s in syms)
    used = [c for e in smx.vocab_encoded("fsst_auto")[0]
            for c in _codes(e, syms)]
    assert any(c is not None and 0xFF in b for c, _, b in used)
    assert any(c is None and b == FF for c, _, b in used)   # escaped ff


def test_fsst_max_table():
    per, syms = smx.vocab_encoded("fsst_max")
    assert len(syms) == 254 == len(set(syms))
    assert all(len(s) == 8 for s in syms) and sum(map(len, syms)) == 2032
    used = {c for e in per for c, _, _ in _codes(e, syms) if c is not None}
    assert 253 in used and syms[253] == FF * 8
    # an 8-byte code over bytes 56..63: it spans byte 62, the last byte a
    # 63-byte literal compares
    spans = [v for v, e in zip(smx.VOCAB, per)
             if any(c is not None and pos == 56 for c, pos, _ in
                    _codes(e, syms))]
    assert any(v.startswith(SA) for v in spans) and FF * 64 in spans
    # ff both inside symbols and as an escaped data byte
    e62 = _codes(per[smx.VOCAB.index(FF * 62)], syms)
    assert [c for c, _, _ in e62] == [253] * 7 + [None] * 6


def test_fsst_escape_table():
    per, syms = smx.vocab_encoded("fsst_escape")
    assert syms == []
    for v, e in zip(smx.VOCAB, per):
        assert len(e) == 2 * len(v) and set(e[::2]) <= {255}


def test_hashes():
    h = smx.vocab_hashes()
    assert len(set(h.tolist())) == len(smx.VOCAB)       # injective
    assert [int(x) & ((1 << 64) - 1) for x in h] == \
        [po.fnv1a64(v) for v in smx.VOCAB]
    srt = np.sort(h)
    assert srt[0] < 0 < srt[-1]     # a negative hash sorts before a positive
    assert smx.MALFORMED_KEY not in h and -1 not in h
    assert smx.MALFORMED_KEY & ((1 << 64) - 1) == 0x8000000000000001


def test_ref_group_by(mx):
    full = mx.ref_group_by()
    assert set(full) == set(smx.VOCAB)
    cnt = np.bincount(mx.draw, minlength=len(smx.VOCAB))
    acc = np.zeros(len(smx.VOCAB), dtype=np.uint64)
    np.add.at(acc, mx.draw, mx.val.view(np.uint64))     # second witness
    for i, v in enumerate(smx.VOCAB):
        assert full[v] == (int(cnt[i]), int(acc.view(np.int64)[i]))
    assert any(abs(s) > (1 << 62) for _, s in full.values())
    m = mx.ref_mask("prefix_S")
    part = mx.ref_group_by(m)
    assert set(part) == {v for v in smx.VOCAB if v.startswith(S)}
    assert sum(c for c, _ in part.values()) == int(m.sum())


def test_large_geometry():
    g = smx.matrix("large")
    assert g.rows == 4096 * 256 + 101 and g.rows % 64 == 37
    assert set(g.draw.tolist()) == set(range(len(smx.VOCAB)))
    m = g.ref_mask(smx.LARGE_CASE)
    hits = np.flatnonzero(m)
    assert 0.01 < len(hits) / g.rows < 0.04 and len(hits) < 65536
    assert hits[0] < smx.GRID_ROWS <= hits[-1]
    # the explicit tail: matches and near misses alternate, in the partial
    # last mask word too
    tail = m[-smx.LARGE_TAIL:]
    assert tail[0::2].all() and not tail[1::2].any()
    assert set(g.values()[-smx.LARGE_TAIL:]) == {SA, smx.LARGE_MISS}
    last = m[g.rows // 64 * 64:]
    assert len(last) == 37 and 0 < last.sum() < 37


def test_malformed_rows():
    off, blob, values = smx.malformed_escape()
    bad = [r for r, v in enumerate(values) if v is None]
    assert bad == [3, 7]
    for r, v in enumerate(values):
        row = blob[int(off[r]):int(off[r + 1])]
        if v is None:
            with pytest.raises(ValueError):
                po.fsst_decode(row, [])
        else:
            assert po.fsst_decode(row, []) == v
    assert blob[int(off[3]):int(off[4])] == b"\x05"
    assert blob[int(off[8]) - 1] == 0xFF and blob[int(off[8]) - 2] != 0xFF
