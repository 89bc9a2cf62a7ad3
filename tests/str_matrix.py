"""String-predicate matrix: one small vocabulary of byte strings that holds
every byte, length and FSST edge the string kernels of sdb_scan.hip can get
wrong, drawn into deterministic row sets, encoded four ways, plus the
predicate cases and the plain-Python references the CPU and GPU matrix tests
compare against. The string counterpart of tests/col_matrix.py.

All values are `bytes`. The vocabulary is the ground truth: a reference is
evaluated once per vocabulary entry with Python's bytes operators and indexed
by the draw; nothing here decodes a blob to obtain an expected value.

Vocabulary (VOCAB, a few dozen entries):

  bytes    00 7f 80 fe ff, ff ff, and a / a00 / a7f / a80 / a81 / aff: the
           sign boundary as first and as second byte.
  stem     S = bytes 0x30..0x6d, 62 bytes, all distinct, so no two 8-byte
           windows are equal. S itself; S+x for x in 00 41 7f 80 ff (63
           bytes, differing at byte index 62); S+x+00, S+x+01 (differing at
           index 63, beyond any literal); a 65-byte row; S+x+"r"*137 (200
           bytes); S+x+ff*900 (963 bytes); "r"*1000.
  ff runs  ff*62, ff*63, ff*64.
  8 bytes  abcdefg, abcdefgh, abcdefghi, abcdefgi, abcdefgh+ff.

Row sets (StrMatrix.draw indexes VOCAB):

  base     4099 rows: every entry once, then a seeded draw. Prefixes of 1,
           63, 64, 65 and 257 rows (PREFIX_ROWS) share its encodings.
  large    4096*256 + 101 rows, past the 4096-block x 256-thread launch, so
           the grid-stride loops of the string kernels take a second pass;
           entries longer than 100 bytes are drawn rarely to keep the blob
           small, and the last 101 rows alternate between a match and a
           near miss of LARGE_CASE. 37 rows in the last mask word.

Encodings (ENCODINGS) of the same rows, each (offsets, blob, symbols):

  raw          plain bytes, symbols None
  fsst_auto    the project's encoder, trained on the head of the base table
               (AUTO_SAMPLE_BYTES): symbols of 3..8 bytes, some holding ff,
               and no 1-byte symbol, so every ff outside them is escaped
  fsst_escape  no symbols: every byte is written as ff b
  fsst_max     254 symbols of exactly 8 bytes (2032 table bytes): fillers
               first, so the symbols rows use have the highest codes and
               table offsets; aligned and unaligned stem windows, one
               symbol per (x, next byte) over bytes 56..63 of the long stem
               rows, "r"*8 and ff*8 (code 253)

Every encoding of every row set is the join of per-entry encodings made by
the greedy longest-match encoder below; tests/test_str_matrix.py shows it
equal to serenedb_amd.encode_col_str_fsst on the base table and decodes all
of it back with pyoracle.fsst_decode, the decoder of record.
"""

import functools

import numpy as np

import serenedb_amd as sa
from oracle import pyoracle as po

SEED = 5
BASE_ROWS = 4099
PREFIX_ROWS = (1, 63, 64, 65, 257)
LARGE_ROWS = 4096 * 256 + 101
LARGE_TAIL = 101
GRID_ROWS = 4096 * 256          # rows the first grid-stride pass covers
ENCODINGS = ("raw", "fsst_auto", "fsst_escape", "fsst_max")
AUTO_SAMPLE_BYTES = 64          # the training sample is VOCAB[:2]
STRLIT_MAX = 63                 # SDB_STRLIT_MAX
I64_MIN = -(1 << 63)
MALFORMED_KEY = -(1 << 63) + 1  # 0x8000000000000001 as signed i64

S = bytes(range(0x30, 0x6E))
X = (0x00, 0x41, 0x7F, 0x80, 0xFF)
FF = b"\xff"


def sx(x):
    return S + bytes([x])


RUN = b"r" * 137
FF900 = FF * 900
SA = sx(0x41)                   # the 63-byte literal of record

VOCAB = (
    # the first two train fsst_auto: stem windows, some holding ff, the 8-byte
    # neighbours, and too few ff for ff to become a symbol of its own
    sx(0xFF), b"abcdefgh\xff", b"\x80",
    b"", b"\x00", b"\x7f", b"\xfe", FF, FF + FF,
    b"a", b"a\x00", b"a\x7f", b"a\x80", b"a\x81", b"a\xff",
    S, sx(0x00), SA, sx(0x7F), sx(0x80),
    SA + b"\x00", SA + b"\x01", sx(0x80) + b"\x00", sx(0x80) + b"\x01",
    SA + b"\x01\x01",
    sx(0x00) + RUN, SA + RUN, SA + FF900, sx(0x80) + FF900,
    b"r" * 1000,
    FF * 62, FF * 63, FF * 64,
    b"abcdefg", b"abcdefgh", b"abcdefghi", b"abcdefgi",
)
assert len(set(VOCAB)) == len(VOCAB) and len(S) == 62 and len(SA) == 63

# ---- predicate cases: name -> (op, lo, hi, declared result) ---------------
# declared: "all" / "none" for the cases that pass every / no row by
# construction; every other case must split the rows.
_C = {}


def _case(name, op, lo, hi=None, declared=None):
    assert name not in _C
    _C[name] = (op, lo, hi, declared)


_case("prefix_empty", "prefix", b"", declared="all")
_case("lt_empty", "lt", b"", declared="none")
_case("eq_absent", "eq", b"abcdefgj", declared="none")
_case("between_lo_gt_hi", "between", b"b", b"a", declared="none")
# literal length 0
_case("eq_empty", "eq", b"")
_case("between_empty_a", "between", b"", b"a")
# length 1, the sign boundary first
for _op in ("lt", "ge", "eq", "prefix"):
    _case(f"{_op}_80", _op, b"\x80")
_case("eq_a", "eq", b"a")
_case("prefix_a", "prefix", b"a")               # proper prefix of rows
_case("prefix_ff", "prefix", FF)
_case("lt_ff", "lt", FF)
_case("between_7f_fe", "between", b"\x7f", b"\xfe")
# length 2, the sign boundary second
for _op in ("lt", "ge", "eq", "prefix"):
    _case(f"{_op}_a80", _op, b"a\x80")
_case("between_a00_a80", "between", b"a\x00", b"a\x80")
_case("between_a81_aff", "between", b"a\x81", b"a\xff")
_case("eq_ffff", "eq", FF + FF)
_case("ge_ffff", "ge", FF + FF)
# a literal that has a row as its proper prefix
_case("lt_a80_00", "lt", b"a\x80\x00")
_case("ge_a80_00", "ge", b"a\x80\x00")
_case("between_a_a80_00", "between", b"a", b"a\x80\x00")
# length 8 and 9
for _op in ("lt", "ge", "eq", "prefix"):
    _case(f"{_op}_abcdefgh", _op, b"abcdefgh")
_case("between_lo_eq_hi", "between", b"abcdefgh", b"abcdefgh")
_case("eq_abcdefgh_ff", "eq", b"abcdefgh\xff")
_case("ge_abcdefgh_ff", "ge", b"abcdefgh\xff")
_case("lt_abcdefghi", "lt", b"abcdefghi")
_case("prefix_abcdefghi", "prefix", b"abcdefghi")
_case("between_abcdefgh_00_ff", "between", b"abcdefgh\x00", b"abcdefgh\xff")
# hi a proper prefix of rows: those rows are above it
_case("between_hi_is_prefix", "between", b"a", b"abcdefg")
# length 62
for _op in ("lt", "ge", "eq", "prefix"):
    _case(f"{_op}_S", _op, S)
    _case(f"{_op}_ff62", _op, FF * 62)
_case("between_S_ff63", "between", S, FF * 63)
# length 63, the longest literal
for _op in ("lt", "ge", "eq", "prefix"):
    _case(f"{_op}_SA", _op, SA)
    _case(f"{_op}_ff63", _op, FF * 63)
_case("eq_S80", "eq", sx(0x80))
_case("lt_S80", "lt", sx(0x80))
_case("between_SA_S80", "between", SA, sx(0x80))
_case("between_S00_S7f", "between", sx(0x00), sx(0x7F))
_case("between_S80_ff63", "between", sx(0x80), FF * 63)

CASES = dict(_C)
LARGE_CASE = "eq_SA"            # about 2% of the large geometry's rows
LARGE_MISS = SA + b"\x00"       # its near miss in the explicit tail
ROWCOUNT_CASE = "prefix_S"        # row 0 passes it


def eval_case(v, op, lo, hi=None):
    """one row against one case, in Python's unsigned-byte order"""
    if op == "lt":
        return v < lo
    if op == "ge":
        return v >= lo
    if op == "eq":
        return v == lo
    if op == "between":
        return lo <= v <= hi
    if op == "prefix":
        return v.startswith(lo)
    raise ValueError(op)


def signed64(h):
    return h - (1 << 64) if h >= (1 << 63) else h


def fsst_encoder(symbols):
    """greedy longest-match encoder over a given symbol table: code c for
    symbols[c], ff b for a byte no symbol starts at"""
    by_first = {}
    for code, s in sorted(enumerate(symbols), key=lambda cs: -len(cs[1])):
        by_first.setdefault(s[0], []).append((s, code))

    def encode(b):
        out, i = bytearray(), 0
        while i < len(b):
            for s, code in by_first.get(b[i], ()):
                if b.startswith(s, i):
                    out.append(code)
                    i += len(s)
                    break
            else:
                out += bytes((255, b[i]))
                i += 1
        return bytes(out)
    return encode


def max_symbols():
    """the fsst_max table: 254 distinct symbols of 8 bytes"""
    used = [S[i:i + 8] for i in range(0, 56, 8)]        # aligned windows
    used += [S[i:i + 8] for i in range(55) if i % 8]    # the other windows
    used += sorted({v[56:64] for v in VOCAB             # bytes 56..63
                    if v.startswith(S) and len(v) >= 64})
    used += [b"r" * 8, FF * 8]
    assert len(set(used)) == len(used)
    # byte 0x02 occurs in no row, so no filler ever matches
    fillers = [b"\x02fill" + bytes([0x30 + i // 16, 0x30 + i % 16, 0x02])
               for i in range(254 - len(used))]
    return fillers + used


class StrMatrix:
    """VOCAB drawn into `rows` rows (module docstring)."""

    def __init__(self, name):
        self.name = name
        nv = len(VOCAB)
        rng = np.random.default_rng([SEED, int(name == "large")])
        if name == "base":
            self.rows = BASE_ROWS
            draw = np.concatenate(
                [np.arange(nv), rng.integers(0, nv, BASE_ROWS - nv)])
        else:
            self.rows = LARGE_ROWS
            w = np.array([1.0 if len(v) <= 100 else 1 / 16 for v in VOCAB])
            draw = rng.choice(nv, LARGE_ROWS, p=w / w.sum())
            hit, miss = VOCAB.index(SA), VOCAB.index(LARGE_MISS)
            draw[-LARGE_TAIL:] = [hit if i % 2 == 0 else miss
                                  for i in range(LARGE_TAIL)]
        self.draw = draw.astype(np.int64)
        self.rowid = np.arange(self.rows, dtype=np.int64)
        self.key = self.rowid % 2048
        self.val = rng.integers(I64_MIN, (1 << 63) - 1, self.rows,
                                dtype=np.int64, endpoint=True)
        for a in (self.draw, self.rowid, self.key, self.val):
            a.setflags(write=False)

    def values(self, n=None):
        return [VOCAB[i] for i in self.draw[:n].tolist()]

    # ---- encoded forms -------------------------------------------------
    def encoded(self, enc, n=None):
        """(offsets uint64[n+1], blob, symbols or None) of the first n rows"""
        per, symbols = vocab_encoded(enc)
        d = self.draw[:n]
        offsets = np.zeros(len(d) + 1, dtype=np.uint64)
        np.cumsum(np.array([len(p) for p in per], dtype=np.uint64)[d],
                  out=offsets[1:])
        return offsets, b"".join(per[i] for i in d.tolist()), symbols

    # ---- references ----------------------------------------------------
    def ref_mask(self, case, n=None):
        return vocab_mask(case)[self.draw[:n]]

    def ref_group_by(self, mask=None):
        """{string: (count, wrap-around i64 sum of val)} over the rows in
        mask, in Python integers"""
        out = {}
        sel = np.ones(self.rows, bool) if mask is None else mask
        for i, v in zip(self.draw[sel].tolist(), self.val[sel].tolist()):
            c, s = out.get(VOCAB[i], (0, 0))
            out[VOCAB[i]] = (c + 1, s + v)
        return {k: (c, signed64(s % (1 << 64))) for k, (c, s) in out.items()}


@functools.lru_cache(maxsize=None)
def matrix(name):
    return StrMatrix(name)


@functools.lru_cache(maxsize=None)
def auto_encoded():
    """serenedb_amd.encode_col_str_fsst over the base rows"""
    return sa.encode_col_str_fsst(matrix("base").values(),
                                  sample_bytes=AUTO_SAMPLE_BYTES)


@functools.lru_cache(maxsize=None)
def vocab_encoded(enc):
    """([encoded bytes per VOCAB entry], symbols or None)"""
    if enc == "raw":
        return list(VOCAB), None
    symbols = {"fsst_auto": lambda: list(auto_encoded()[2]),
               "fsst_escape": lambda: [],
               "fsst_max": max_symbols}[enc]()
    encode = fsst_encoder(symbols)
    return [encode(v) for v in VOCAB], symbols


@functools.lru_cache(maxsize=None)
def vocab_mask(case):
    op, lo, hi, _ = CASES[case]
    m = np.array([eval_case(v, op, lo, hi) for v in VOCAB], dtype=bool)
    m.setflags(write=False)
    return m


@functools.lru_cache(maxsize=None)
def vocab_hashes():
    """signed FNV-1a 64 of every VOCAB entry, in VOCAB order"""
    h = np.array([signed64(po.fnv1a64(v)) for v in VOCAB], dtype=np.int64)
    h.setflags(write=False)
    return h


def malformed_escape(n=65):
    """(offsets, blob, [row bytes or None]) of the first n base rows in the
    fsst_escape encoding with two malformed rows: row 3 is the single code
    05 (out of range without symbols), row 7 ends in a bare ff. None marks
    them."""
    mx = matrix("base")
    per, _ = vocab_encoded("fsst_escape")
    rows = [per[i] for i in mx.draw[:n].tolist()]
    rows[3] = b"\x05"
    rows[7] = b"\xffa\xff"
    values = mx.values(n)
    values[3] = values[7] = None
    offsets = np.zeros(n + 1, dtype=np.uint64)
    np.cumsum([len(r) for r in rows], out=offsets[1:])
    return offsets, b"".join(rows), values
