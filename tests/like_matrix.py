"""LIKE matrix: the vocabulary, row geometries, pattern cases and the `re`
references that the CPU test (tests/test_like_matrix.py) and the GPU test
(tests/test_gpu_like_matrix.py) of SUFFIX / CONTAINS / LIKE share. The
pattern counterpart of tests/str_matrix.py, whose vocabulary, stem, encoders
and table idiom it reuses.

Reference. Python's `re` decides every expectation: a pattern is translated
byte by byte ('%' becomes `.*`, an escaped byte and every other byte go
through re.escape), compiled with re.S and used with fullmatch on bytes.
Nothing here calls the library to obtain an expected value.

Vocabulary. str_matrix.VOCAB plus EXTRA, the overlap and escape traps:
self-overlapping literals (aab, abab, abcabcabd), the pattern's own special
bytes as data (% _ ! and the backslash), 62..64-byte runs around the
63-byte literal limit, a needle at the far end of a 1000-byte row, NUL
bytes, and the stem doubled so that a rotated stem window occurs.

Row sets.

  base    4099 rows: every VOCAB entry once, then a seeded draw; prefixes of
          1, 63, 64, 65 and 257 rows share it. Encoded raw, fsst_auto,
          fsst_escape and fsst_max with the str_matrix tables (entries the
          tables do not know are escape-coded).
  split   for each literal of SPLIT_LITS (the 63-byte SA and a 2-byte one)
          and every t in 1..m-1, two adjacent rows that hold the literal's
          first t bytes at the end of one and the rest at the start of the
          next, and the same with one and with three empty rows between;
          runs of 70 empty rows; real hits between them; the last row is
          the literal itself (variant "full", it ends at blob_len) or the
          literal minus its last byte (variant "short").
  chunk   CHUNK_PAIRS pairs of filler + SA + filler and its near miss
          (SA with the last byte changed), the filler lengths chosen so
          that the blob offsets of the hits, and of the near misses, each
          cover every residue mod 8192: whatever power-of-two chunk up to
          8192 bytes a kernel streams, a literal sits at every position
          relative to a chunk edge. Bands of 1024-byte fillers make 64-row
          windows longer than 8192 bytes.
"""

import functools
import re

import numpy as np

import str_matrix as smx
from str_matrix import FF, S, SA

SEED = 11
BASE_ROWS = smx.BASE_ROWS
PREFIX_ROWS = smx.PREFIX_ROWS
ENCODINGS = smx.ENCODINGS
ESC = b"!"
PATTERN_MAX = 255               # SDB_LIKE_PATTERN_MAX
LIT_MAX = smx.STRLIT_MAX        # 63 literal bytes in total


def q(b):
    """quote b for a pattern whose escape is '!': %, _ and ! are escaped"""
    out = bytearray()
    for c in b:
        if c in b"%_!":
            out += ESC
        out.append(c)
    return bytes(out)


def like_to_re(pattern, escape=None):
    """the reference translation; raises ValueError on what the library
    must reject for its form (trailing escape, bare '_')"""
    esc = None if escape is None else escape[0]
    out, i = [], 0
    while i < len(pattern):
        c = pattern[i]
        if esc is not None and c == esc:
            i += 1
            if i >= len(pattern):
                raise ValueError("trailing escape")
            out.append(re.escape(pattern[i:i + 1]))
        elif c == 0x25:
            out.append(b".*")
        elif c == 0x5F:
            raise ValueError("bare _")
        else:
            out.append(re.escape(pattern[i:i + 1]))
        i += 1
    return re.compile(b"".join(out), re.S)


def literal_bytes(pattern, escape=None):
    """number of literal bytes of a well-formed pattern"""
    esc = None if escape is None else escape[0]
    n, i = 0, 0
    while i < len(pattern):
        if esc is not None and pattern[i] == esc:
            i += 1
            n += 1
        elif pattern[i] != 0x25:
            n += 1
        i += 1
    return n


EXTRA = (
    b"ab", b"aab", b"aaab", b"aba", b"abab", b"ababa", b"ababab",
    b"abcabd", b"abcabcabd",
    b"%", b"a%b", b"a_b", b"a!b", b"\\", b"a\\b",
    b"x" * 63, b"x" * 64, b"x" * 62 + b"y", b"y" + b"x" * 63,
    b"r" * 999 + b"s", b"s" + b"r" * 999,
    b"\x00\x00", b"a\x00b", b"ab" * 40, S + S, S[1:] + S,
)
VOCAB = smx.VOCAB + EXTRA
assert len(set(VOCAB)) == len(VOCAB)

# ---- cases: name -> (pattern, escape, declared, (op, literal) or None) ----
# declared: "all" / "one" for the cases that pass every row / exactly one
# vocabulary entry by construction; every other case must split VOCAB. The
# last field is the strpred_mask form of a pure CONTAINS / SUFFIX pattern.
_C = {}


def _case(name, pattern, escape=ESC, declared=None, op=None):
    assert name not in _C
    assert len(pattern) <= PATTERN_MAX
    assert literal_bytes(pattern, escape) <= LIT_MAX
    _C[name] = (pattern, escape, declared, op)


def _contains(name, lit):
    _case("contains_" + name, b"%" + q(lit) + b"%", op=("contains", lit))


def _suffix(name, lit):
    _case("suffix_" + name, b"%" + q(lit), op=("suffix", lit))


_case("all", b"%", declared="all")
_case("all3", b"%%%", declared="all")
_case("empty", b"", declared="one")
_contains("a", b"a")
_contains("80", b"\x80")
_contains("ff", FF)
_contains("00", b"\x00")
_contains("aab", b"aab")
_contains("abab", b"abab")
_contains("abcabd", b"abcabd")
_contains("rrs", b"rrs")
_contains("sr", b"sr")
_contains("S", S)
_contains("SA", SA)
_contains("x63", b"x" * 63)
_contains("ff63", FF * 63)
_contains("r63", b"r" * 63)
_contains("S40_A", S[40:] + b"A")
_contains("S_rotated", S[31:] + S[:31])
_suffix("a", b"a")
_suffix("ab", b"ab")
_suffix("aba", b"aba")
_suffix("ff", FF)
_suffix("00", b"\x00")
_suffix("rs", b"rs")
_suffix("x63", b"x" * 63)
_suffix("SA", SA)
# prefix and equality through LIKE
_case("prefix_a", b"a%")
_case("prefix_S", q(S) + b"%")
_case("eq_abab", b"abab")
_case("eq_SA", q(SA))
# multi-segment
_case("a_a", b"a%a")                        # must not match "a"
_case("ab_ab", b"ab%ab")
_case("pct_ab_ab", b"%ab%ab")               # abab, not aba
_case("aba_ba", b"aba%ba")                  # ababa, not abab
_case("ab3", b"%ab%ab%ab%")
_case("S_r", q(S) + b"%r")
_case("S31_S31_ff", q(S[:31]) + b"%" + q(S[31:]) + b"%\xff%")
_case("r_s", b"r%s")
_case("s_r", b"s%r")
_case("x32_x31", b"x" * 32 + b"%" + b"x" * 31)
_case("abcabd_scattered", b"%a%b%c%a%b%d%")
# escapes
_case("contains_pct", b"%!%%")
_case("eq_a_pct_b", b"a!%b")
_case("eq_a_us_b", b"a!_b")
_case("contains_bang", b"%!!%")
_case("eq_ab_escaped", b"!a!b")
_case("suffix_backslash_noescape", b"%\\%", escape=None)
_case("eq_a_bs_b", b"a\\\\b", escape=b"\\")

CASES = dict(_C)
ROWCOUNT_CASE = "contains_S"     # row 0 (sx(ff)) passes it
LARGE_CASE = "contains_SA"


def ref_match(pattern, escape, v):
    return like_to_re(pattern, escape).fullmatch(v) is not None


@functools.lru_cache(maxsize=None)
def case_re(case):
    pattern, escape = CASES[case][:2]
    return like_to_re(pattern, escape)


def values_mask(case, values):
    """reference verdict per row of `values` (None = malformed: no match),
    evaluated once per distinct value"""
    rx, memo = case_re(case), {}
    out = np.zeros(len(values), dtype=bool)
    for i, v in enumerate(values):
        if v is None:
            continue
        hit = memo.get(v)
        if hit is None:
            hit = memo[v] = rx.fullmatch(v) is not None
        out[i] = hit
    return out


@functools.lru_cache(maxsize=None)
def vocab_mask(case):
    m = values_mask(case, VOCAB)
    m.setflags(write=False)
    return m


@functools.lru_cache(maxsize=None)
def smx_vocab_mask(case):
    """the case over str_matrix.VOCAB (the rows of str_matrix's tables)"""
    m = values_mask(case, smx.VOCAB)
    m.setflags(write=False)
    return m


# ---- encodings -------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def symbols(enc):
    return None if enc == "raw" else smx.vocab_encoded(enc)[1]


@functools.lru_cache(maxsize=None)
def vocab_encoded(enc):
    """[encoded bytes per VOCAB entry] with the str_matrix tables"""
    if enc == "raw":
        return list(VOCAB)
    encode = smx.fsst_encoder(symbols(enc))
    return [encode(v) for v in VOCAB]


def encode_rows(enc, rows):
    """(offsets uint64[n+1], blob, symbols or None) of arbitrary rows"""
    if enc == "raw":
        per = rows
    else:
        encode, memo = smx.fsst_encoder(symbols(enc)), {}
        per = []
        for v in rows:
            e = memo.get(v)
            if e is None:
                e = memo[v] = encode(v)
            per.append(e)
    offsets = np.zeros(len(per) + 1, dtype=np.uint64)
    np.cumsum([len(p) for p in per], out=offsets[1:])
    return offsets, b"".join(per), symbols(enc)


class Columns:
    """the numeric columns every table of these tests carries"""

    def __init__(self, rows, seed):
        rng = np.random.default_rng([SEED, seed])
        self.rows = rows
        self.rowid = np.arange(rows, dtype=np.int64)
        self.key = self.rowid % 2048
        self.val = rng.integers(smx.I64_MIN, (1 << 63) - 1, rows,
                                dtype=np.int64, endpoint=True)
        for a in (self.rowid, self.key, self.val):
            a.setflags(write=False)


class LikeMatrix(Columns):
    """VOCAB drawn into BASE_ROWS rows: every entry once, then seeded"""

    def __init__(self):
        super().__init__(BASE_ROWS, 0)
        nv = len(VOCAB)
        rng = np.random.default_rng([SEED, 100])
        self.draw = np.concatenate(
            [np.arange(nv), rng.integers(0, nv, BASE_ROWS - nv)]
        ).astype(np.int64)
        self.draw.setflags(write=False)

    def values(self, n=None):
        return [VOCAB[i] for i in self.draw[:n].tolist()]

    def encoded(self, enc, n=None):
        per = vocab_encoded(enc)
        d = self.draw[:n]
        offsets = np.zeros(len(d) + 1, dtype=np.uint64)
        np.cumsum(np.array([len(p) for p in per], dtype=np.uint64)[d],
                  out=offsets[1:])
        return offsets, b"".join(per[i] for i in d.tolist()), symbols(enc)

    def ref_mask(self, case, n=None):
        return vocab_mask(case)[self.draw[:n]]


@functools.lru_cache(maxsize=None)
def matrix():
    return LikeMatrix()


# ---- split geometry --------------------------------------------------------
SPLIT_LITS = (SA, b"xy")        # neither occurs in the filler "zz"
EMPTY_RUN = 70
GAPS = (0, 1, 3)


class SplitGeometry:
    """rows, and per literal the row numbers of its straddling halves"""

    def __init__(self, variant):
        assert variant in ("full", "short")
        fill = b"zz"
        rows, halves = [], {lit: [] for lit in SPLIT_LITS}
        for lit in SPLIT_LITS:
            rows.append(fill + lit + fill)              # a plain hit
            for gap in GAPS:
                for t in range(1, len(lit)):
                    halves[lit] += [len(rows), len(rows) + 1 + gap]
                    rows.append(fill + lit[:t])
                    rows += [b""] * gap
                    rows.append(lit[t:] + fill)
                rows.append(lit)                        # a hit after a half
            rows += [b""] * EMPTY_RUN
        last = SPLIT_LITS[0] if variant == "full" else SPLIT_LITS[0][:-1]
        rows.append(last)
        self.values_ = rows
        self.halves = halves
        self.last = last
        self.cols = Columns(len(rows), 1)
        self.rows = len(rows)

    def values(self):
        return self.values_

    def ref_mask(self, lit):
        rx = like_to_re(b"%" + q(lit) + b"%", ESC)
        return np.array([rx.fullmatch(v) is not None for v in self.values_])


@functools.lru_cache(maxsize=None)
def split(variant):
    return SplitGeometry(variant)


# ---- chunk geometry --------------------------------------------------------
CHUNK_MOD = 8192
CHUNK_PAIRS = 8192 + 256
CHUNK_MISS = SA[:-1] + b"B"
CHUNK_LONG = 1024               # filler of the long bands
CHUNK_BAND = (512, 8)           # pairs k with k % 512 < 8 are long


class ChunkGeometry:
    """pair k = (pre + SA + "z", pre' + CHUNK_MISS + "z"): |pre| = 1 and
    |pre'| = 2, so a pair is 131 bytes, an odd step that walks the planted
    offsets through every residue mod 8192; a long band adds 16 * 1024 bytes,
    a multiple of 8192, so the walk goes on behind it."""

    def __init__(self):
        rows = []
        for k in range(CHUNK_PAIRS):
            extra = CHUNK_LONG if k % CHUNK_BAND[0] < CHUNK_BAND[1] else 0
            rows.append(b"z" * (1 + extra) + SA + b"z")
            rows.append(b"z" * (2 + extra) + CHUNK_MISS + b"z")
        self.values_ = rows
        self.rows = len(rows)
        lens = np.array([len(r) for r in rows], dtype=np.uint64)
        self.offsets = np.zeros(self.rows + 1, dtype=np.uint64)
        np.cumsum(lens, out=self.offsets[1:])
        pre = np.array([len(r) - 64 for r in rows], dtype=np.uint64)
        self.planted = self.offsets[:-1] + pre      # blob offset of SA / miss
        self.cols = Columns(self.rows, 2)

    def values(self):
        return self.values_

    def ref_mask(self):
        return values_mask("contains_SA", self.values_)


@functools.lru_cache(maxsize=None)
def chunk():
    return ChunkGeometry()
