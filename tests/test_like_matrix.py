"""The LIKE matrix (tests/like_matrix.py) is what it claims, and the matcher
the GPU kernels share (serenedb_amd/csrc/sdb_like.h, reached through the
sdb_host_like_* entries of libsdb_host.so) agrees with Python's `re` on every
case, on a fuzz and on every rejection, all on the CPU. The GPU half is
tests/test_gpu_like_matrix.py."""

import ctypes as C

import numpy as np
import pytest

import like_matrix as lmx
import serenedb_amd as sa
import str_matrix as smx
from oracle import pyoracle as po

FSST = ("fsst_auto", "fsst_escape", "fsst_max")
S, SA = smx.S, smx.SA


@pytest.fixture(scope="module")
def mx():
    return lmx.matrix()


def test_vocabulary(mx):
    have = set(lmx.VOCAB)
    assert set(smx.VOCAB) <= have and len(have) == len(lmx.VOCAB)
    assert {b"ab", b"aab", b"aaab", b"aba", b"abab", b"ababa", b"ababab",
            b"abcabd", b"abcabcabd", b"%", b"a%b", b"a_b", b"a!b", b"\\",
            b"a\\b", b"x" * 63, b"x" * 64, b"x" * 62 + b"y", b"y" + b"x" * 63,
            b"r" * 999 + b"s", b"s" + b"r" * 999, b"\x00\x00", b"a\x00b",
            b"ab" * 40, S + S, S[1:] + S} <= have
    assert mx.rows == 4099 and mx.values(len(lmx.VOCAB)) == list(lmx.VOCAB)
    assert set(mx.values()) == have
    assert 0x5F in S and 0x5C in S      # so every stem pattern needs q()
    assert lmx.q(b"a%_!b") == b"a!%!_!!b"


def test_case_table_covers_the_issue():
    c = lmx.CASES
    assert len(c) >= 49
    pats = {(p, e) for p, e, _, _ in c.values()}
    for p in (b"%", b"%%%", b"", b"%a%", b"%\x80%", b"%\xff%", b"%\x00%",
              b"%aab%", b"%abab%", b"%abcabd%", b"%rrs%", b"%sr%",
              b"%" + lmx.q(S) + b"%", b"%" + lmx.q(SA) + b"%",
              b"%" + b"x" * 63 + b"%", b"%" + b"\xff" * 63 + b"%",
              b"%" + b"r" * 63 + b"%", b"%" + lmx.q(S[40:]) + b"A%",
              b"%" + lmx.q(S[31:] + S[:31]) + b"%",
              b"%a", b"%ab", b"%aba", b"%\xff", b"%\x00", b"%rs",
              b"%" + b"x" * 63, b"%" + lmx.q(SA),
              b"a%", lmx.q(S) + b"%", b"abab", lmx.q(SA),
              b"a%a", b"ab%ab", b"%ab%ab", b"aba%ba", b"%ab%ab%ab%",
              lmx.q(S) + b"%r",
              lmx.q(S[:31]) + b"%" + lmx.q(S[31:]) + b"%\xff%",
              b"r%s", b"s%r", b"x" * 32 + b"%" + b"x" * 31,
              b"%a%b%c%a%b%d%",
              b"%!%%", b"a!%b", b"a!_b", b"%!!%", b"!a!b"):
        assert (p, b"!") in pats, p
    assert (b"%\\%", None) in pats and (b"a\\\\b", b"\\") in pats
    # the single-literal forms name their strpred_mask twin
    for name, (p, e, _, op) in c.items():
        if op is not None:
            kind, lit = op
            want = b"%" + lmx.q(lit) + (b"%" if kind == "contains" else b"")
            assert p == want and e == b"!", name
    assert sum(op is not None for _, _, _, op in c.values()) == 24
    assert lmx.literal_bytes(c["S31_S31_ff"][0], b"!") == 63


def test_reference_translation():
    assert lmx.like_to_re(b"a%b.c", None).pattern == b"a.*b\\.c"
    assert lmx.like_to_re(b"!%!a%", b"!").pattern == b"%a.*"
    assert lmx.ref_match(b"%\n%", None, b"a\nb")        # re.S
    assert not lmx.ref_match(b"a%a", None, b"a")
    assert lmx.ref_match(b"%ab%ab", None, b"abab")
    assert not lmx.ref_match(b"%ab%ab", None, b"aba")
    assert lmx.ref_match(b"aba%ba", None, b"ababa")
    assert not lmx.ref_match(b"aba%ba", None, b"abab")


def test_every_case_splits_the_vocabulary(mx):
    declared = {n: d for n, (_, _, d, _) in lmx.CASES.items() if d}
    assert declared == {"all": "all", "all3": "all", "empty": "one"}
    nv = len(lmx.VOCAB)
    for name in lmx.CASES:
        passed = int(lmx.vocab_mask(name).sum())
        want = {"all": nv, "one": 1}.get(declared.get(name))
        if want is None:
            assert 0 < passed < nv, name
            assert 0 < int(mx.ref_mask(name).sum()) < mx.rows, name
        else:
            assert passed == want, name
    assert lmx.VOCAB[int(np.flatnonzero(lmx.vocab_mask("empty"))[0])] == b""
    assert mx.ref_mask(lmx.ROWCOUNT_CASE, 1).all()      # row 0 passes
    for n in lmx.PREFIX_ROWS[1:]:
        assert 0 < int(mx.ref_mask(lmx.ROWCOUNT_CASE, n).sum()) < n
    # the cases also split str_matrix's own rows where the GPU tests use them
    m = lmx.smx_vocab_mask(lmx.LARGE_CASE)
    assert {v for v, k in zip(smx.VOCAB, m) if k} >= {
        SA, smx.LARGE_MISS, SA + smx.RUN, SA + smx.FF900}


@pytest.mark.parametrize("case", list(lmx.CASES))
def test_matcher_equals_re_on_the_vocabulary(case):
    pattern, escape, _, op = lmx.CASES[case]
    prog = sa.like_compile(pattern, escape)
    got = np.array([sa.like_match(prog, v) for v in lmx.VOCAB])
    bad = np.flatnonzero(got != lmx.vocab_mask(case))
    assert len(bad) == 0, (case, pattern, [lmx.VOCAB[i][:40] for i in bad[:4]])
    if op is not None:      # the plain-Python meaning of the twin op
        kind, lit = op
        want = [(lit in v) if kind == "contains" else v.endswith(lit)
                for v in lmx.VOCAB]
        assert got.tolist() == want, case


def test_str_patterns_are_utf8():
    prog = sa.like_compile("%é%")
    assert sa.like_match(prog, "café au lait")
    assert sa.like_match(prog, "café".encode())
    assert not sa.like_match(prog, b"cafe")
    assert sa.like_match(sa.like_compile("a!%", escape="!"), "a%")


def test_fuzz_against_re():
    """seeded pattern/row pairs over a b % ! with '!' the escape: rows of
    0..8 bytes, patterns of 0..6 bytes, the patterns the rules reject
    skipped (and seen to be rejected)"""
    rng = np.random.default_rng(20240)
    alpha = b"ab%!"
    npat, nrow = 6000, 128
    plen = rng.integers(0, 7, npat)
    pats = {bytes(alpha[i] for i in rng.integers(0, 4, n)) for n in plen}
    pats |= {b"", b"%", b"a", b"%a", b"a%", b"%a%"}
    rows = [bytes(b"ab%!"[i] for i in rng.integers(0, 4, n))
            for n in rng.integers(0, 9, nrow * 8)]
    rows = sorted(set(rows))
    rsel = rng.integers(0, len(rows), (len(pats), nrow))
    pairs = rejected = 0
    for k, p in enumerate(sorted(pats)):
        try:
            rx = lmx.like_to_re(p, b"!")
        except ValueError:
            with pytest.raises(RuntimeError, match="rc=-1$"):
                sa.like_compile(p, b"!")
            rejected += 1
            continue
        prog = sa.like_compile(p, b"!")
        for r in rsel[k]:
            v = rows[r]
            assert sa.like_match(prog, v) == (rx.fullmatch(v) is not None), \
                (p, v)
            pairs += 1
    assert pairs >= 100_000 and rejected > 50


def _raw_compile(pattern, n, escape):
    """(rc, buffer after the call) through the C entry itself, the output
    poisoned beforehand"""
    h = sa.host()
    size = h.sdb_host_like_prog_size()
    prog = C.create_string_buffer(b"\xa5" * size, size)
    pa = (C.c_uint8 * max(len(pattern), 1))(*pattern)
    rc = h.sdb_host_like_compile(pa, C.c_uint32(n), C.c_int32(escape), prog)
    return rc, prog.raw, size


@pytest.mark.parametrize("what,pattern,escape", [
    ("trailing escape", b"ab!", 0x21),
    ("trailing escape after %", b"%!", 0x21),
    ("bare _", b"a_b", -1),
    ("bare _ with an escape set", b"%_%", 0x21),
    ("64 literal bytes", b"x" * 64, -1),
    ("64 literal bytes in segments", b"x" * 32 + b"%" + b"y" * 32, -1),
    ("64 literal bytes after escapes", b"!x" * 64, 0x21),
    ("256 pattern bytes", b"%" * 256, -1),
    ("escape %", b"abc", 0x25),
    ("escape 256", b"abc", 256),
    ("escape -2", b"abc", -2),
])
def test_rejections_leave_the_output_alone(what, pattern, escape):
    rc, raw, size = _raw_compile(pattern, len(pattern), escape)
    assert rc == -1, what
    assert raw == b"\xa5" * size, what
    with pytest.raises(RuntimeError, match="rc=-1$"):
        sa.like_compile(pattern, None if escape == -1 else escape)


def test_limits_are_accepted():
    # 63 literal bytes over 63 one-byte segments, 62 '%' between them
    lits = bytes(range(0x61, 0x61 + 26)) * 3
    p = b"%".join(lits[i:i + 1] for i in range(63))
    assert len(p) == 125 and lmx.literal_bytes(p) == 63
    prog = sa.like_compile(p)
    rx = lmx.like_to_re(p)
    for v in (lits[:63], lits[:62], lits[:63] + b"a", b"q".join(
            lits[i:i + 1] for i in range(63)), b"a" + lits[:63],
            lits[:62] + b"zzk", b""):
        assert sa.like_match(prog, v) == (rx.fullmatch(v) is not None), v
    assert sa.like_match(prog, lits[:63])
    # 255 pattern bytes: 63 literal bytes and 192 '%'
    p = b"%" * 96 + b"x" * 63 + b"%" * 96
    assert len(p) == 255
    prog = sa.like_compile(p)
    assert sa.like_match(prog, b"y" + b"x" * 63)
    assert not sa.like_match(prog, b"x" * 62 + b"y")
    # a 63-byte literal: EQ, and one escaped byte per literal byte
    assert sa.like_match(sa.like_compile(lmx.q(SA), b"!"), SA)
    p = b"".join(b"!" + SA[i:i + 1] for i in range(63))
    assert len(p) == 126 and sa.like_match(sa.like_compile(p, b"!"), SA)
    # the escape may be any byte but '%', NUL and '_' included
    assert sa.like_match(sa.like_compile(b"a\x00%b", 0), b"a%b")
    assert sa.like_match(sa.like_compile(b"a__b", b"_"), b"a_b")


@pytest.mark.parametrize("enc", FSST)
def test_fsst_decodes_back(mx, enc):
    syms = lmx.symbols(enc)
    assert syms == smx.vocab_encoded(enc)[1]    # the str_matrix tables
    for v, e in zip(lmx.VOCAB, lmx.vocab_encoded(enc)):
        assert po.fsst_decode(e, syms) == v
    off, blob, syms2 = mx.encoded(enc)
    assert syms2 == syms and len(off) == mx.rows + 1
    assert off[0] == 0 and off[-1] == len(blob)
    for r in (0, 1, 62, 63, 64, 4098):
        assert po.fsst_decode(blob[int(off[r]):int(off[r + 1])], syms) == \
            lmx.VOCAB[mx.draw[r]]
    roff, rblob, none = mx.encoded("raw")
    assert none is None and rblob == b"".join(mx.values())
    # a prefix of the rows is a prefix of the encoding
    off65, blob65, _ = mx.encoded(enc, 65)
    assert blob65 == blob[:int(off[65])]
    # the arbitrary-row encoder of the geometries is the same encoder
    off2, blob2, _ = lmx.encode_rows(enc, mx.values(300))
    assert blob2 == blob[:int(off[300])]
    np.testing.assert_array_equal(off2, off[:301])


@pytest.mark.parametrize("variant", ["full", "short"])
def test_split_geometry(variant):
    g = lmx.split(variant)
    vals = g.values()
    assert 300 <= g.rows <= 1000
    assert lmx.SPLIT_LITS == (SA, b"xy") and len(SA) == 63
    for lit in lmx.SPLIT_LITS:
        m, ref = len(lit), g.ref_mask(lit)
        h = g.halves[lit]
        assert len(h) == 2 * 3 * (m - 1)
        seen = set()
        for a, b in zip(h[0::2], h[1::2]):
            gap = b - a - 1
            t = len(vals[a]) - 2
            seen.add((gap, t))
            assert vals[a] == b"zz" + lit[:t] and vals[b] == lit[t:] + b"zz"
            assert all(v == b"" for v in vals[a + 1:b])
            assert not ref[a] and not ref[b]        # no straddling match
        assert seen == {(gap, t) for gap in (0, 1, 3) for t in range(1, m)}
        assert 0 < ref.sum() < g.rows
    # runs of 70 empty rows, and empty rows never match a literal
    run = best = 0
    for v in vals:
        run = run + 1 if v == b"" else 0
        best = max(best, run)
    assert best >= 70
    # the last row ends the blob: the literal, or the literal cut short
    off, blob, _ = lmx.encode_rows("raw", vals)
    assert int(off[-1]) == len(blob)
    if variant == "full":
        assert vals[-1] == SA and blob.endswith(SA) and g.ref_mask(SA)[-1]
    else:
        assert vals[-1] == SA[:-1] and not g.ref_mask(SA)[-1]
        assert vals[-2] == b""


def test_chunk_geometry():
    g = lmx.chunk()
    assert g.rows >= 8192 and g.rows == 2 * lmx.CHUNK_PAIRS
    vals = g.values()
    ref = g.ref_mask()
    assert ref[0::2].all() and not ref[1::2].any()
    blob = b"".join(vals)
    assert len(blob) == int(g.offsets[-1]) < (4 << 20)
    for r in (0, 1, 2, 17, g.rows - 2, g.rows - 1):
        at = int(g.planted[r])
        assert blob[at:at + 63] == (SA if r % 2 == 0 else lmx.CHUNK_MISS)
    assert lmx.CHUNK_MISS[:-1] == SA[:-1] and lmx.CHUNK_MISS != SA
    # the planted offsets of the hits, and of the near misses, each cover
    # every residue mod 8192 (so every residue mod any smaller power of two)
    for part in (g.planted[0::2], g.planted[1::2]):
        assert len(np.unique(part % np.uint64(lmx.CHUNK_MOD))) == lmx.CHUNK_MOD
    # 64-row windows longer than 8192 bytes, and ordinary short ones
    span = (g.offsets[64::64] - g.offsets[:-64:64]).astype(np.int64)
    assert (span > 8192).sum() >= 8 and (span < 8192).sum() >= 8


def test_large_case_on_the_str_matrix_rows():
    g = smx.matrix("large")
    ref = lmx.smx_vocab_mask(lmx.LARGE_CASE)[g.draw]
    hits = np.flatnonzero(ref)
    assert 0.05 < len(hits) / g.rows < 0.2 and len(hits) < (1 << 18)
    assert (hits >= smx.GRID_ROWS).sum() == smx.LARGE_TAIL   # hit and miss


def test_malformed_rows_reference():
    _, _, values = smx.malformed_escape()
    for case in ("all", "contains_a", "empty"):
        m = lmx.values_mask(case, values)
        assert not m[3] and not m[7]
    assert int(lmx.values_mask("all", values).sum()) == len(values) - 2
