// sdb_like.h — the one byte-wise LIKE matcher, shared by the host library
// and the HIP string kernels (include/sdb_gpu.h holds the semantics of
// record). Plain C++, no HIP include: g++ builds it into libsdb_host.so,
// hipcc into sdb_scan.hip.
//
// A pattern compiles (host only) to an SdbLikeProg: the literal bytes of
// all its segments concatenated (<= 63), so every segment is a bit range of
// one 64-bit word, and a 256-entry table whose entry b has bit i set iff
// concatenated byte i equals b. CONTAINS x, SUFFIX x, PREFIX x, EQ x and
// every LIKE share that form. The streaming step is Shift-And over the
// current segment, one byte at a time:
//
//     state = ((state << 1) | seed) & table[b] & range
//
// leftmost-greedy and non-overlapping: an anchored-start first segment
// seeds at byte 0 only and the row fails when its state dies; a middle
// segment that matched hands over to the next one with state 0; an
// anchored-end last segment runs to the row end and matches iff its top
// bit is set after the last byte (a last segment that is also the first,
// no '%', seeds at byte 0 only, so it additionally needs row length ==
// literal length).

#ifndef SDB_LIKE_H_
#define SDB_LIKE_H_

#include <stdint.h>

#if defined(__HIPCC__)
#define SDB_HD __host__ __device__
#else
#define SDB_HD
#endif

#define SDB_LIKE_PATTERN_MAX 255
#define SDB_LIKE_LIT_MAX 63  // == SDB_STRLIT_MAX: bits 0..62 of the word

struct SdbLikeProg {
  uint64_t table[256];    // bit i set iff lit[i] == index
  uint8_t seg_start[64];  // first bit of segment k
  uint8_t seg_len[64];    // its length, >= 1
  uint8_t lit[64];        // concatenated literal bytes
  uint32_t nseg;
  uint32_t lit_len;
  uint32_t anchored_start;  // pattern does not begin with '%'
  uint32_t anchored_end;    // pattern does not end with '%'
};

struct SdbLikeState {
  uint64_t st;    // Shift-And state of the current segment
  uint32_t seg;   // current segment; == nseg once all have matched
  uint32_t n;     // bytes fed so far
  uint32_t fail;  // the anchored first segment died
};

SDB_HD inline void sdb_like_init(SdbLikeState& s) {
  s.st = 0;
  s.seg = 0;
  s.n = 0;
  s.fail = 0;
}

// one row byte. `p` may live in LDS or in host memory.
SDB_HD inline void sdb_like_feed(const SdbLikeProg& p, SdbLikeState& s,
                                 uint8_t b) {
  const uint32_t pos = s.n++;
  if (s.fail || s.seg >= p.nseg) return;
  const uint32_t k = s.seg;
  const uint32_t start = p.seg_start[k], len = p.seg_len[k];
  const uint64_t lo = 1ull << start;
  const uint64_t range = ((1ull << len) - 1ull) << start;
  const uint64_t top = 1ull << (start + len - 1u);
  const bool first_anch = k == 0 && p.anchored_start;
  const bool last_anch = k + 1 == p.nseg && p.anchored_end;
  const uint64_t seed = (first_anch && pos) ? 0ull : lo;
  s.st = ((s.st << 1) | seed) & p.table[b] & range;
  if (first_anch && !s.st) {
    s.fail = 1;
    return;
  }
  if (!last_anch && (s.st & top)) {
    s.seg = k + 1;
    s.st = 0;
  }
}

// the verdict after the last byte; row_len is the number of bytes fed
SDB_HD inline bool sdb_like_finish(const SdbLikeProg& p,
                                   const SdbLikeState& s, uint64_t row_len) {
  if (s.fail) return false;
  if (p.nseg == 0) return !p.anchored_start || row_len == 0;
  if (!p.anchored_end) return s.seg == p.nseg;
  if (s.seg + 1 != p.nseg) return false;
  const uint32_t k = p.nseg - 1;
  return (s.st >> (p.seg_start[k] + p.seg_len[k] - 1u)) & 1ull;
}

// the same step in a scalar loop
SDB_HD inline bool sdb_like_match(const SdbLikeProg& p, const uint8_t* s,
                                  uint64_t n) {
  SdbLikeState st;
  sdb_like_init(st);
  for (uint64_t i = 0; i < n; ++i) sdb_like_feed(p, st, s[i]);
  return sdb_like_finish(p, st, n);
}

// ---- the compiler: host only (no SDB_HD) --------------------------------

// incremental builder behind both front ends below
struct SdbLikeBuilder {
  SdbLikeProg p;
  uint32_t cur;  // bytes in the open segment
  bool ok;
};
inline void sdb_like_b_init(SdbLikeBuilder& b) {
  for (int i = 0; i < 256; ++i) b.p.table[i] = 0;
  for (int i = 0; i < 64; ++i)
    b.p.seg_start[i] = b.p.seg_len[i] = b.p.lit[i] = 0;
  b.p.nseg = b.p.lit_len = 0;
  b.p.anchored_start = b.p.anchored_end = 1;
  b.cur = 0;
  b.ok = true;
}
inline void sdb_like_b_byte(SdbLikeBuilder& b, uint8_t c) {
  if (b.p.lit_len >= SDB_LIKE_LIT_MAX) {
    b.ok = false;
    return;
  }
  if (!b.cur) b.p.seg_start[b.p.nseg] = (uint8_t)b.p.lit_len;
  b.p.table[c] |= 1ull << b.p.lit_len;
  b.p.lit[b.p.lit_len++] = c;
  ++b.cur;
}
inline void sdb_like_b_close(SdbLikeBuilder& b) {  // at a '%' or the end
  if (!b.cur) return;
  b.p.seg_len[b.p.nseg++] = (uint8_t)b.cur;
  b.cur = 0;
}

// pattern + escape (0..255, or -1 = none) -> program. 0 on success, -1
// (SDB_ERR_INVALID) on a rejected pattern; *out is written on success only.
inline int sdb_like_compile(const uint8_t* pat, uint32_t len, int32_t escape,
                            SdbLikeProg* out) {
  if (!out || (len && !pat)) return -1;
  if (len > SDB_LIKE_PATTERN_MAX) return -1;
  if (escape < -1 || escape > 255 || escape == '%') return -1;
  SdbLikeBuilder b;
  sdb_like_b_init(b);
  bool first_pct = false, last_pct = false;
  for (uint32_t i = 0; i < len; ++i) {
    const uint8_t c = pat[i];
    if (escape >= 0 && c == (uint8_t)escape) {
      if (++i >= len) return -1;  // escape as the last pattern byte
      sdb_like_b_byte(b, pat[i]);
      last_pct = false;
    } else if (c == '%') {
      sdb_like_b_close(b);
      if (i == 0) first_pct = true;
      last_pct = true;
    } else if (c == '_') {
      return -1;  // one CHARACTER in SQL; this matcher compares bytes
    } else {
      sdb_like_b_byte(b, c);
      last_pct = false;
    }
    if (!b.ok) return -1;  // more than 63 literal bytes
  }
  sdb_like_b_close(b);
  b.p.anchored_start = first_pct ? 0 : 1;
  b.p.anchored_end = last_pct ? 0 : 1;
  *out = b.p;
  return 0;
}

// one literal with chosen anchors: EQ (1, 1), PREFIX (1, 0), SUFFIX (0, 1),
// CONTAINS (0, 0). An empty literal with a free side matches every row.
inline int sdb_like_literal(const uint8_t* lit, uint32_t len, bool anch_start,
                            bool anch_end, SdbLikeProg* out) {
  if (!out || (len && !lit) || len > SDB_LIKE_LIT_MAX) return -1;
  SdbLikeBuilder b;
  sdb_like_b_init(b);
  for (uint32_t i = 0; i < len; ++i) sdb_like_b_byte(b, lit[i]);
  sdb_like_b_close(b);
  if (!len && !(anch_start && anch_end)) anch_start = anch_end = false;
  b.p.anchored_start = anch_start;
  b.p.anchored_end = anch_end;
  *out = b.p;
  return 0;
}

#endif  // SDB_LIKE_H_
