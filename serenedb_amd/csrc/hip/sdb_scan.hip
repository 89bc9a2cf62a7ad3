// sdb_scan.hip — columnar scan -> predicate -> hash-group-by on MI355X.
//
// Replaces the reference's FullScanner::Scan + ColFilterChain predicate
// narrowing (server/connector/full_scanner.h:40-90,
// index/table_filter_iterator.hpp:104-227) fused with the consumer the
// reference delegates to external DuckDB (PhysicalHashAggregate, un-vendored;
// result-level parity per SURVEY.md §8c).
//
// MI355X design: pure HBM-bandwidth work (no MFMA). Columns are either
// dense device-resident arrays or FoR/bitpack row groups (this repo's own
// codec, sdb_host.cpp: per-group frame-of-reference base + horizontal
// bitpack + min/max zonemap — the reference's block codecs live in the
// un-vendored DuckDB fork, so parity is at result level). The kernel walks
// row GROUPS grid-stride: one zonemap check per group can skip the whole
// group (DeadUntil analogue, full_scanner.h:61-71); within a group,
// threads decode packed values in registers (coalesced u32 payload reads),
// evaluate predicates, and accumulate into LDS per-group-key slots (dense
// keys = perfect hash); one device-atomic flush per block at kernel end.
// COUNT/SUM(i64) exact (wrap-around); SUM(f32) in f64 (atomic order
// nondeterministic, like the reference's thread-order-dependent fp
// aggregation; parity vs the oracle's sequential sum at ~1e-12 relative).
// COUNT(col) / MIN / MAX (i64 and f32) are exact and order-independent:
// MIN/MAX accumulate as one u64 atomicMax over order-preserving codes (see
// agg_row), f32 in a NaN-greatest total order.

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "../../../include/sdb_gpu.h"
#include "../sdb_like.h"
#include "sdb_internal.h"

#ifndef SCAN_NTHREADS
#define SCAN_NTHREADS 1024u  // swept on-box: 1024t/2048b beats 256t/4096b;
#endif                       // with 4 rows/thread: 5.17 TB/s at 1B rows
#ifndef SCAN_MAXB
#define SCAN_MAXB 2048u
#endif
#define SCAN_MAX_GROUPS 2048u
#define SCAN_MAX_AGGS 8u
#define SCAN_MAX_PREDS 4u

// the one error path of this file: HIP_CHECK returns sdb_hip_rc of a failed
// call, and a DevBuf frees a call's temporary allocation on every return
#include "sdb_hip_rc.h"

// mirrors the host codec (sdb_host.cpp sdb_host_encode_col_i64)
struct SdbColHeaderDev {
  uint64_t magic;
  uint64_t rows;
  uint32_t group_rows;
  uint32_t ngroups;
  uint64_t off_desc;
  uint64_t off_payload;
  uint64_t size;
};
struct SdbColGroupDescDev {
  int64_t base;
  int64_t vmin;
  int64_t vmax;
  uint64_t word_off;
  uint16_t width;
  uint16_t pad[3];
};
#define SDB_COL_MAGIC_DEV 0x31304C4F43424453ull

struct ColRef {
  const void* data;                  // raw array, or FoR payload (u32*)
  const SdbColGroupDescDev* desc;    // FoR group table (null = raw)
};

#define SDB_MAX_STRCOLS 4
#ifndef SDB_STRLIT_MAX
#define SDB_STRLIT_MAX 63  // literal bytes per side in strpred_mask
#endif

struct SdbGpuTable {
  void* cols[16];        // raw device array or whole FoR blob
  SdbColType types[16];
  ColRef refs[16];       // device pointers into cols[] allocations
  uint16_t max_w[16];    // FoR cols: max bit width over all groups
  uint64_t paywords[16]; // FoR cols: total payload u32 words (for clamped
                         // slack loads in the staged kernel)
  // i64 column value range, known for every FoR column (zonemaps) and for
  // every raw i64 column (one load-time GPU reduction): lets scan_agg
  // prove a group-key column fits [0, ngroups) instead of letting a stray
  // key scribble past the LDS accumulators (ADVICE r1 / VERDICT weak #4)
  int64_t col_min[16], col_max[16];
  uint8_t has_minmax[16];
  unsigned long long* valid[16];  // device validity bitmaps or null
  // i64 column value range over the VALID rows of the attached plane: the
  // same proof for a nullable group key, whose NULL rows may hold anything.
  // One GPU reduction at the first nullable-key scan after an attach;
  // dropped by every attach / detach. vmin > vmax = no valid row.
  int64_t valid_min[16], valid_max[16];
  uint8_t has_valid_minmax[16];
  uint32_t ncols;
  uint64_t rows;
  uint32_t group_rows;   // shared by every FoR column (0 if none)
  // raw variable-width string columns (include/sdb_gpu.h attach_strcol):
  // per slot offsets[rows+1] + byte blob + the last strpred_mask result
  uint64_t* str_off[SDB_MAX_STRCOLS];
  uint8_t* str_blob[SDB_MAX_STRCOLS];
  uint64_t str_blob_len[SDB_MAX_STRCOLS];
  unsigned long long* str_mask[SDB_MAX_STRCOLS];
  uint8_t str_mask_set[SDB_MAX_STRCOLS];
  // FSST-style compressed slots: codes 0..nsym-1 expand to 1..8-byte
  // symbols, 255 escapes the next literal byte. The table is small and
  // travels by kernel argument (staged to LDS in the kernel).
  uint8_t str_fsst[SDB_MAX_STRCOLS];
  uint16_t str_nsym[SDB_MAX_STRCOLS];
  uint16_t str_symoff[SDB_MAX_STRCOLS][256];   // byte offsets, nsym+1 used
  uint8_t str_syms[SDB_MAX_STRCOLS][2048];
  // the compiled pattern of the running SUFFIX / CONTAINS / LIKE call
  // (sdb_like.h), allocated at the first such call
  SdbLikeProg* like_prog;
};

// load-time min/max reduction over a raw i64 column. Signed order via the
// sign-flip trick so u64 atomics suffice on every ROCm.
__global__ void col_minmax_kernel(const long long* __restrict__ v, uint64_t n,
                                  unsigned long long* __restrict__ mm) {
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  long long lmin = 0x7FFFFFFFFFFFFFFFll, lmax = 0x8000000000000000ll;
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += stride) {
    const long long x = v[i];
    lmin = x < lmin ? x : lmin;
    lmax = x > lmax ? x : lmax;
  }
#pragma unroll
  for (int off = 32; off; off >>= 1) {
    const long long a = __shfl_down(lmin, off, 64);
    const long long b = __shfl_down(lmax, off, 64);
    lmin = a < lmin ? a : lmin;
    lmax = b > lmax ? b : lmax;
  }
  if ((threadIdx.x & 63) == 0) {
    atomicMin(&mm[0], (unsigned long long)lmin ^ 0x8000000000000000ull);
    atomicMax(&mm[1], (unsigned long long)lmax ^ 0x8000000000000000ull);
  }
}

// The pushed predicate list resolved against a table (preds_resolve), as
// every columnar kernel takes it inside its argument struct; the count
// (npreds) stays a field of that struct. 224 bytes, 8-aligned.
struct PredSet {
  ColRef col[SCAN_MAX_PREDS];
  int op[SCAN_MAX_PREDS];
  int isf32[SCAN_MAX_PREDS];  // f32 predicate columns
  int64_t lo[SCAN_MAX_PREDS];
  int64_t hi[SCAN_MAX_PREDS];
  float flo[SCAN_MAX_PREDS], fhi[SCAN_MAX_PREDS];
  const unsigned long long* valid[SCAN_MAX_PREDS];  // null = all valid
};

struct ScanArgs {
  ColRef keys;
  uint64_t rows;
  uint32_t group_rows;  // row-group tiling (also used for raw-only tables)
  uint32_t ngroups;
  uint32_t naggs;
  uint32_t npreds;
  PredSet ps;
  ColRef agg_col[SCAN_MAX_AGGS];
  int agg_op[SCAN_MAX_AGGS];
  int agg_src[SCAN_MAX_AGGS];  // 0=own col_read, 1+p=pred p's value, 9=key
  const unsigned long long* agg_valid[SCAN_MAX_AGGS];  // all but COUNT(*)
                                                       // skip nulls
  unsigned long long* out;
  unsigned long long* rows_passed;
  // --- staged-FoR variant only (scan_agg_staged_kernel) ---
  uint32_t chunk_rows;  // LDS staging chunk (multiple of 32)
  uint32_t nstage;      // distinct FoR cols staged (<=3: keys, pred0, pred1)
  int key_st;           // stage slot of the key column, -1 = unstaged
  int pred_st[2];       // stage slot of pred 0/1's column, -1 = unstaged
  const SdbColGroupDescDev* st_desc[3];
  const uint32_t* st_pay[3];
  uint64_t st_paywords[3];  // clamp for slack loads past the chunk
  uint32_t st_lds_off[3];   // u32 offset of each stage buffer in smem
  // optional f32 agg-column staging: the scattered per-passing-row 4 B
  // gather becomes one coalesced burst per chunk. Reads the whole column
  // (vs ~81% of its lines via the gather at 10% selectivity), so it can
  // lose on very low-pass non-dead groups; SDB_SCAN_NOF32STAGE opts out.
  const float* f32_pay;     // null = no f32 staging
  uint32_t f32_lds_off;
};

// Kernel argument of the nullable-group-key (NK = 1) instantiations. The
// NK = 0 ones keep taking ScanArgs itself, so their kernel-argument segment
// — and with it every offset they load from — is what it was.
struct ScanArgsNK : ScanArgs {
  const unsigned long long* key_valid;  // the key column's own plane
  unsigned long long* null_rows;        // passing rows whose key is NULL
};
template <int NK> struct ScanArgsOf { using type = ScanArgs; };
template <> struct ScanArgsOf<1> { using type = ScanArgsNK; };

// predicate evaluation — the SdbPredOp set mirrors the reference's pushed
// table filters (index/table_filter_iterator.hpp:104-227: typed compares;
// EQ added round 2 per VERDICT #7). NaN floats fail every compare (SQL
// semantics of the reference's filter chain).
__device__ __forceinline__ bool pred_eval_i(int op, int64_t x, int64_t lo,
                                            int64_t hi) {
  switch (op) {
    case SDB_PRED_LT: return x < lo;
    case SDB_PRED_GE: return x >= lo;
    case SDB_PRED_BETWEEN: return (x >= lo) & (x <= hi);
    case SDB_PRED_EQ: return x == lo;
    default: return true;
  }
}
__device__ __forceinline__ bool valid_at(const unsigned long long* v,
                                         uint64_t r) {
  return !v || ((v[r >> 6] >> (r & 63u)) & 1ull);
}
// predicate with SQL three-valued logic over an optional validity plane:
// comparisons fail on NULL; ISNULL/NOTNULL evaluate the plane alone
__device__ __forceinline__ bool pred_eval_iv(
  int op, const unsigned long long* vb, uint64_t r, int64_t x, int64_t lo,
  int64_t hi) {
  if (op == SDB_PRED_ISNULL) return vb && !valid_at(vb, r);
  if (op == SDB_PRED_NOTNULL) return valid_at(vb, r);
  return valid_at(vb, r) && pred_eval_i(op, x, lo, hi);
}
__device__ __forceinline__ bool pred_eval_f(int op, float x, float lo,
                                            float hi) {
  switch (op) {
    case SDB_PRED_LT: return x < lo;
    case SDB_PRED_GE: return x >= lo;
    case SDB_PRED_BETWEEN: return (x >= lo) & (x <= hi);
    case SDB_PRED_EQ: return x == lo;
    default: return true;
  }
}

__device__ __forceinline__ bool pred_eval_fv(
  int op, const unsigned long long* vb, uint64_t r, float x, float lo,
  float hi) {
  if (op == SDB_PRED_ISNULL) return vb && !valid_at(vb, r);
  if (op == SDB_PRED_NOTNULL) return valid_at(vb, r);
  return valid_at(vb, r) && pred_eval_f(op, x, lo, hi);
}

// branchless funnel-shift extraction: value = bits [bit, bit+width) of the
// packed stream = v_alignbit_b32 of the two covering words (width <= 32 so
// one alignbit covers any in-word offset), masked. The +1 word read is
// unconditional; table_load over-allocates 4 pad bytes so the final value's
// slack read stays in bounds (its bits are masked out).
__device__ __forceinline__ uint32_t bits_at(const uint32_t* w, uint64_t bit) {
  const uint64_t wi = bit >> 5;
  return __builtin_amdgcn_alignbit(w[wi + 1], w[wi], (uint32_t)bit & 31u);
}

// desc fields are read per call from desc[rg]: the address is wave-uniform
// so the loads scalarize/broadcast from cache (a register-cached desc array
// indexed by a runtime agg index would spill to scratch — guide rule 20:
// that variant measured 2x slower than the raw path)
__device__ __forceinline__ int64_t col_read(const ColRef& c, uint32_t rg,
                                            uint64_t r0, uint64_t r) {
  if (!c.desc) return ((const long long*)c.data)[r];
  const SdbColGroupDescDev& d = c.desc[rg];
  if (d.width == 0) return d.base;
  const uint32_t* w = (const uint32_t*)c.data + d.word_off;
  const uint32_t mask =
    d.width >= 32 ? 0xFFFFFFFFu : ((1u << d.width) - 1u);
  return d.base + (int64_t)(bits_at(w, (r - r0) * d.width) & mask);
}

// paired FoR extraction: values r and r+1
__device__ __forceinline__ void col_read2(const ColRef& c, uint32_t rg,
                                          uint64_t r0, uint64_t r,
                                          int64_t& x0, int64_t& x1) {
  if (!c.desc) {
    longlong2 x;
    __builtin_memcpy(&x, &((const long long*)c.data)[r], 16);
    x0 = x.x;
    x1 = x.y;
    return;
  }
  const SdbColGroupDescDev& d = c.desc[rg];
  if (d.width == 0) {
    x0 = x1 = d.base;
    return;
  }
  const uint32_t* w = (const uint32_t*)c.data + d.word_off;
  const uint64_t bit0 = (r - r0) * d.width;
  const uint32_t mask =
    d.width >= 32 ? 0xFFFFFFFFu : ((1u << d.width) - 1u);
  x0 = d.base + (int64_t)(bits_at(w, bit0) & mask);
  x1 = d.base + (int64_t)(bits_at(w, bit0 + d.width) & mask);
}

// staged analogue of col_read2: the chunk's packed words sit in LDS (sw),
// bit offsets are chunk-relative (lr = row - chunk_start; chunks start on a
// 32-row multiple so the chunk's first bit is word-aligned). Desc fields are
// read per call — the address is wave-uniform so the loads scalarize, same
// rationale as col_read.
__device__ __forceinline__ void col_read2_lds(const SdbColGroupDescDev* desc,
                                              const uint32_t* sw, uint32_t rg,
                                              uint32_t lr, int64_t& x0,
                                              int64_t& x1) {
  const SdbColGroupDescDev& d = desc[rg];
  if (d.width == 0) {
    x0 = x1 = d.base;
    return;
  }
  const uint64_t bit0 = (uint64_t)lr * d.width;
  const uint32_t mask =
    d.width >= 32 ? 0xFFFFFFFFu : ((1u << d.width) - 1u);
  x0 = d.base + (int64_t)(bits_at(sw, bit0) & mask);
  x1 = d.base + (int64_t)(bits_at(sw, bit0 + d.width) & mask);
}

// zonemap skip (DeadUntil analogue): no row of row group rg can pass, by the
// group min/max of some FoR predicate column. Every walker asks this first.
// An f32 column is never FoR (its desc is null), so the isf32 test decides
// nothing; the two dense walkers never had it and instantiate the helper
// without it (F32_GUARD = 0), which keeps their code what was measured.
template <bool F32_GUARD = true>
__device__ __forceinline__ bool preds_zone_dead(const PredSet& ps,
                                                uint32_t npreds,
                                                uint32_t rg) {
  bool dead = false;
  for (uint32_t p = 0; p < npreds; ++p) {
    if (ps.col[p].desc && !(F32_GUARD && ps.isf32[p])) {
      const SdbColGroupDescDev& d = ps.col[p].desc[rg];
      switch (ps.op[p]) {
        case SDB_PRED_LT: dead |= d.vmin >= ps.lo[p]; break;
        case SDB_PRED_GE: dead |= d.vmax < ps.lo[p]; break;
        case SDB_PRED_BETWEEN:
          dead |= (d.vmax < ps.lo[p]) | (d.vmin > ps.hi[p]);
          break;
        case SDB_PRED_EQ:
          dead |= (d.vmax < ps.lo[p]) | (d.vmin > ps.lo[p]);
          break;
        default: break;
      }
    }
  }
  return dead;
}

// the AND of the predicates on row r of row group rg (first row r0). ISNULL /
// NOTNULL read the plane alone and never the column: a STRMASK predicate
// arrives as NOTNULL over the slot's mask, and in sdb_gpu_scan_topn with no
// column behind it. Used by the hash kernel and the top-n kernel. The dense
// walkers keep their own loops (the decode-once bodies reuse the decoded
// values), and so does the composite-key kernel, for the reason given there.
__device__ __forceinline__ bool preds_pass(const PredSet& ps, uint32_t npreds,
                                           uint32_t rg, uint64_t r0,
                                           uint64_t r) {
  bool ok = true;
  for (uint32_t p = 0; p < npreds; ++p) {
    const int op = ps.op[p];
    const unsigned long long* vb = ps.valid[p];
    if (op == SDB_PRED_ISNULL)
      ok &= vb && !valid_at(vb, r);
    else if (op == SDB_PRED_NOTNULL)
      ok &= valid_at(vb, r);
    else if (ps.isf32[p])
      ok &= pred_eval_fv(op, vb, r, ((const float*)ps.col[p].data)[r],
                         ps.flo[p], ps.fhi[p]);
    else
      ok &= pred_eval_iv(op, vb, r, col_read(ps.col[p], rg, r0, r), ps.lo[p],
                         ps.hi[p]);
  }
  return ok;
}

// min/max of a raw or FoR i64 column over its VALID rows only: the range
// proof of a nullable group key (NULL rows may hold anything). Run once per
// attached plane, never per scan. mm as in col_minmax_kernel; a column with
// no valid row leaves the {~0, 0} fill, i.e. min > max.
__global__ void col_minmax_valid_kernel(ColRef c,
                                        const unsigned long long* valid,
                                        uint64_t n, uint32_t group_rows,
                                        unsigned long long* __restrict__ mm) {
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  long long lmin = 0x7FFFFFFFFFFFFFFFll, lmax = 0x8000000000000000ll;
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += stride) {
    if (!valid_at(valid, i)) continue;
    const uint32_t rg = (uint32_t)(i / group_rows);
    const long long x = col_read(c, rg, (uint64_t)rg * group_rows, i);
    lmin = x < lmin ? x : lmin;
    lmax = x > lmax ? x : lmax;
  }
#pragma unroll
  for (int off = 32; off; off >>= 1) {
    const long long a = __shfl_down(lmin, off, 64);
    const long long b = __shfl_down(lmax, off, 64);
    lmin = a < lmin ? a : lmin;
    lmax = b > lmax ? b : lmax;
  }
  if ((threadIdx.x & 63) == 0) {
    atomicMin(&mm[0], (unsigned long long)lmin ^ 0x8000000000000000ull);
    atomicMax(&mm[1], (unsigned long long)lmax ^ 0x8000000000000000ull);
  }
}

// ---- MIN / MAX accumulator encoding -------------------------------------
// Every MIN/MAX accumulator holds an unsigned "bigger wins" code whose
// identity is 0, so all four ops are one u64 atomicMax (ds_max_u64 in LDS,
// global_atomic_umax_x2 in HBM) on the same 8-byte slots the sums use, and
// the zero fills of acc / d_out / gacc / neg_acc and the "skip a zero slot"
// flushes stay valid. MAX_I64: x ^ 2^63 (signed order as unsigned);
// MIN_I64: its complement. MAX_F32 / MIN_F32: the same pair over the
// 32-bit total-order key of the NaN-canonicalised value. Code 0 decodes on
// the host to the op's identity (agg_decode): for i64 it IS the identity's
// code, and a canonicalised f32 can never produce it.
#define SDB_I64_SIGN 0x8000000000000000ull

// every NaN -> +qNaN 0x7FC00000, then IEEE total order as an unsigned key:
// -inf < ... < -0.0 < +0.0 < ... < +inf < NaN. Keys span
// [0x007FFFFF (-inf), 0xFFC00000 (NaN)]: neither 0 nor 0xFFFFFFFF occurs.
__device__ __forceinline__ uint32_t f32_order_key(float f) {
  uint32_t b = __float_as_uint(f);
  if ((b & 0x7FFFFFFFu) > 0x7F800000u) b = 0x7FC00000u;
  return b ^ ((b & 0x80000000u) ? 0xFFFFFFFFu : 0x80000000u);
}

// One row into one aggregate slot — the single statement of the per-row
// aggregate switch, shared by every generic body (raw quad + tail, FoR pair
// + odd tail, staged chunk + odd tail, hash LDS / global / key -1). geti /
// getf fetch the row's i64 / f32 value the way the calling body does (own
// read, decode-once reuse, LDS stage) and run only in the arm that needs
// them. EXT = 0 is the [COUNT, SUM_I64, SUM_F64] switch exactly as it
// stood before the ops >= SDB_AGG_COUNT_COL existed; the host launches
// EXT = 1 instantiations only when the aggregate list holds such an op.
template <int EXT, class GetI, class GetF>
__device__ __forceinline__ void agg_row(unsigned long long* slot, int op,
                                        const unsigned long long* valid,
                                        uint64_t r, GetI geti, GetF getf) {
  if (op != SDB_AGG_COUNT && !valid_at(valid, r))
    return;  // every column aggregate skips NULLs; COUNT(*) counts the row
  switch (op) {
    case SDB_AGG_COUNT:
      atomicAdd(slot, 1ull);
      break;
    case SDB_AGG_SUM_I64:
      atomicAdd(slot, (unsigned long long)geti());
      break;
    case SDB_AGG_SUM_F64:
      atomicAdd((double*)slot, (double)getf());
      break;
    default:
      if (EXT) {
        switch (op) {
          case SDB_AGG_COUNT_COL:
            atomicAdd(slot, 1ull);
            break;
          case SDB_AGG_MIN_I64:
            atomicMax(slot, ~((unsigned long long)geti() ^ SDB_I64_SIGN));
            break;
          case SDB_AGG_MAX_I64:
            atomicMax(slot, (unsigned long long)geti() ^ SDB_I64_SIGN);
            break;
          case SDB_AGG_MIN_F32:
            atomicMax(slot, (unsigned long long)(~f32_order_key(getf())));
            break;
          case SDB_AGG_MAX_F32:
            atomicMax(slot, (unsigned long long)f32_order_key(getf()));
            break;
        }
      }
      break;
  }
}

// One partial (a workgroup's LDS slot) into its global slot: sums add,
// MIN/MAX codes take the max. Zero partials (no row, or the identity) are
// skipped.
template <int EXT>
__device__ __forceinline__ void agg_merge(unsigned long long* dst, int op,
                                          unsigned long long v) {
  if (op == SDB_AGG_SUM_F64) {
    double d;
    __builtin_memcpy(&d, &v, 8);
    if (d != 0.0) atomicAdd((double*)dst, d);
  } else if (v) {
    if (EXT && op >= SDB_AGG_MIN_I64)
      atomicMax(dst, v);
    else
      atomicAdd(dst, v);
  }
}

// ASHAPE: compile-time aggregate-shape dispatch (DuckDB-style operator
// specialization). 0 = generic runtime loop; 1 = the common 3-agg shape
// [COUNT(*), SUM(i64), SUM(f32->f64)] with the per-row per-agg op/src
// switches straight-lined (the FoR walker is instruction-issue-bound —
// tools/ROUND2_NOTES.md). Any other shape falls back to ASHAPE=0.
// EXT: 1 = the aggregate list holds an op >= SDB_AGG_COUNT_COL (agg_row).
// NK: 1 = the key column carries a validity plane (a.key_valid): a row whose
// key bit is cleared goes to the NULL group, accumulator row ngroups. NK = 1
// exists with ASHAPE = 0, EXT = 1 only; NK = 0 is the code as it stood.

// The accumulator row of a passing row, chosen before anything is indexed:
// the stored key of a NULL-key row may be any value and is never used.
template <int NK>
__device__ __forceinline__ uint32_t key_group(
  const typename ScanArgsOf<NK>::type& a, uint32_t key, uint64_t r) {
  if constexpr (NK) {
    if (!valid_at(a.key_valid, r)) return a.ngroups;
  }
  return key;
}

// NULL-key passing rows of a workgroup into a.null_rows (NK = 1 only)
__device__ __forceinline__ void null_rows_flush(unsigned long long* dst,
                                                unsigned long long mine) {
#pragma unroll
  for (int off = 32; off; off >>= 1) mine += __shfl_down(mine, off, 64);
  if ((threadIdx.x & 63) == 0 && mine) atomicAdd(dst, mine);
}

template <int RAW, int ASHAPE, int EXT, int NK = 0>
__launch_bounds__(SCAN_NTHREADS) __global__
void scan_agg_kernel(typename ScanArgsOf<NK>::type a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  unsigned long long* acc = (unsigned long long*)smem;  // ngroups*naggs
  const uint32_t nslots = (a.ngroups + (NK ? 1u : 0u)) * a.naggs;
  unsigned long long my_null = 0;  // NK: passing rows with a NULL key
  for (uint32_t i = threadIdx.x; i < nslots; i += SCAN_NTHREADS) acc[i] = 0;
  __syncthreads();

  if (RAW) {
    // raw dense columns: 4 rows/thread with 2x16-byte loads per column
    // (measured +9% over 2 rows/thread: 1.79 -> 1.64 ms per 400M rows)
    const uint64_t quad_stride = (uint64_t)gridDim.x * SCAN_NTHREADS * 4u;
    unsigned long long my_passed = 0;
    const uint64_t rows4 = a.rows & ~3ull;
    for (uint64_t r =
           ((uint64_t)blockIdx.x * SCAN_NTHREADS + threadIdx.x) * 4u;
         r < rows4; r += quad_stride) {
      bool okv[4] = {true, true, true, true};
      for (uint32_t p = 0; p < a.npreds; ++p) {
        if (a.ps.isf32[p]) {
          float4 f;
          __builtin_memcpy(&f, &((const float*)a.ps.col[p].data)[r], 16);
          const float fs[4] = {f.x, f.y, f.z, f.w};
#pragma unroll
          for (int e = 0; e < 4; ++e)
            okv[e] &= pred_eval_fv(a.ps.op[p], a.ps.valid[p], r + e,
                                   fs[e], a.ps.flo[p], a.ps.fhi[p]);
          continue;
        }
        longlong2 x, y;
        __builtin_memcpy(&x, &((const long long*)a.ps.col[p].data)[r], 16);
        __builtin_memcpy(&y, &((const long long*)a.ps.col[p].data)[r + 2],
                         16);
        const int64_t xs[4] = {x.x, x.y, y.x, y.y};
#pragma unroll
        for (int e = 0; e < 4; ++e)
          okv[e] &= pred_eval_iv(a.ps.op[p], a.ps.valid[p], r + e,
                                 xs[e], a.ps.lo[p], a.ps.hi[p]);
      }
      if (!okv[0] && !okv[1] && !okv[2] && !okv[3]) continue;
      longlong2 k0, k1;
      __builtin_memcpy(&k0, &((const long long*)a.keys.data)[r], 16);
      __builtin_memcpy(&k1, &((const long long*)a.keys.data)[r + 2], 16);
      const int64_t ks[4] = {k0.x, k0.y, k1.x, k1.y};
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        if (!okv[e]) continue;
        ++my_passed;
        uint32_t g = (uint32_t)ks[e];
        if constexpr (NK) {
          g = key_group<NK>(a, g, r + e);
          my_null += g == a.ngroups;  // valid keys are proved < ngroups
        }
        if (ASHAPE == 1) {  // straight-lined 3-agg shape (dead if generic)
          unsigned long long* s3 = &acc[g * 3u];
          atomicAdd(s3, 1ull);
          if (valid_at(a.agg_valid[1], r + e))
            atomicAdd(s3 + 1, (unsigned long long)((const long long*)
                                                     a.agg_col[1]
                                                       .data)[r + e]);
          if (valid_at(a.agg_valid[2], r + e))
            atomicAdd((double*)(s3 + 2),
                      (double)((const float*)a.agg_col[2].data)[r + e]);
          continue;
        }
        for (uint32_t q = 0; q < a.naggs; ++q)
          agg_row<EXT>(
            &acc[g * a.naggs + q], a.agg_op[q], a.agg_valid[q], r + e,
            [&] { return ((const long long*)a.agg_col[q].data)[r + e]; },
            [&] { return ((const float*)a.agg_col[q].data)[r + e]; });
      }
    }
    if ((a.rows & 3ull) && blockIdx.x == 0 && threadIdx.x == 0)
      for (uint64_t r = rows4; r < a.rows; ++r) {
      // the tail keeps its own eager loop: through preds_pass the EXT = 1
      // instantiation measured 0.4 % slower, outside the parent's spread
      bool ok = true;
      for (uint32_t p = 0; p < a.npreds; ++p) {
        if (a.ps.isf32[p])
          ok &= pred_eval_fv(a.ps.op[p], a.ps.valid[p], r,
                             ((const float*)a.ps.col[p].data)[r],
                             a.ps.flo[p], a.ps.fhi[p]);
        else
          ok &= pred_eval_iv(a.ps.op[p], a.ps.valid[p], r,
                             ((const long long*)a.ps.col[p].data)[r],
                             a.ps.lo[p], a.ps.hi[p]);
      }
      if (ok) {
        ++my_passed;
        uint32_t g = (uint32_t)((const long long*)a.keys.data)[r];
        if constexpr (NK) {
          g = key_group<NK>(a, g, r);
          my_null += g == a.ngroups;
        }
        for (uint32_t q = 0; q < a.naggs; ++q)
          agg_row<EXT>(
            &acc[g * a.naggs + q], a.agg_op[q], a.agg_valid[q], r,
            [&] { return ((const long long*)a.agg_col[q].data)[r]; },
            [&] { return ((const float*)a.agg_col[q].data)[r]; });
      }
    }
    unsigned long long wp = my_passed;
#pragma unroll
    for (int off = 32; off; off >>= 1) wp += __shfl_down(wp, off, 64);
    if ((threadIdx.x & 63) == 0 && wp) atomicAdd(a.rows_passed, wp);
    if constexpr (NK) null_rows_flush(a.null_rows, my_null);
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < nslots; i += SCAN_NTHREADS)
      agg_merge<EXT>(&a.out[i], a.agg_op[i % a.naggs], acc[i]);
    return;
  }

  const uint32_t n_rowgroups =
    (uint32_t)((a.rows + a.group_rows - 1) / a.group_rows);
  unsigned long long my_passed = 0;

  for (uint32_t rg = blockIdx.x; rg < n_rowgroups; rg += gridDim.x) {
    const uint64_t r0 = (uint64_t)rg * a.group_rows;
    const uint64_t r1 = min(a.rows, r0 + a.group_rows);
    if (preds_zone_dead<false>(a.ps, a.npreds, rg)) continue;

    // 2 rows per thread, paired word extraction; odd tail row by thread 0
    const uint64_t glen = r1 - r0;
    const uint64_t gpairs = glen >> 1;
    for (uint64_t pr = threadIdx.x; pr < gpairs; pr += SCAN_NTHREADS) {
      const uint64_t r = r0 + 2 * pr;
      bool okv[2] = {true, true};
      int64_t pva[2] = {0, 0}, pvb[2] = {0, 0};
#pragma unroll
      for (uint32_t p = 0; p < 2; ++p) {  // fast path: first two preds
        if (p >= a.npreds) break;
        if (a.ps.isf32[p]) {
          const float* fc = (const float*)a.ps.col[p].data;
#pragma unroll
          for (int e = 0; e < 2; ++e)
            okv[e] &= pred_eval_fv(a.ps.op[p], a.ps.valid[p], r + e,
                                   fc[r + e], a.ps.flo[p],
                                   a.ps.fhi[p]);
          continue;
        }
        int64_t x0, x1;
        col_read2(a.ps.col[p], rg, r0, r, x0, x1);
        if (p == 0) { pva[0] = x0; pva[1] = x1; }
        else { pvb[0] = x0; pvb[1] = x1; }
        const int64_t xs[2] = {x0, x1};
#pragma unroll
        for (int e = 0; e < 2; ++e)
          okv[e] &= pred_eval_iv(a.ps.op[p], a.ps.valid[p], r + e,
                                 xs[e], a.ps.lo[p], a.ps.hi[p]);
      }
      for (uint32_t p = 2; p < a.npreds; ++p) {  // rare: >2 predicates
#pragma unroll
        for (int e = 0; e < 2; ++e) {
          if (a.ps.isf32[p])
            okv[e] &= pred_eval_fv(
              a.ps.op[p], a.ps.valid[p], r + e,
              ((const float*)a.ps.col[p].data)[r + e], a.ps.flo[p],
              a.ps.fhi[p]);
          else
            okv[e] &= pred_eval_iv(a.ps.op[p], a.ps.valid[p], r + e,
                                   col_read(a.ps.col[p], rg, r0, r + e),
                                   a.ps.lo[p], a.ps.hi[p]);
        }
      }
      if (!okv[0] && !okv[1]) continue;
      int64_t k0, k1;
      col_read2(a.keys, rg, r0, r, k0, k1);
      const int64_t ks[2] = {k0, k1};
#pragma unroll
      for (int e = 0; e < 2; ++e) {
        if (!okv[e]) continue;
        ++my_passed;
        uint32_t grp = (uint32_t)ks[e];
        if constexpr (NK) {
          grp = key_group<NK>(a, grp, r + e);
          my_null += grp == a.ngroups;
        }
        if (ASHAPE == 1) {  // straight-lined 3-agg shape (dead if generic)
          unsigned long long* s3 = &acc[grp * 3u];
          atomicAdd(s3, 1ull);
          if (valid_at(a.agg_valid[1], r + e)) {
            int64_t x;
            switch (a.agg_src[1]) {
              case 1: x = pva[e]; break;
              case 2: x = pvb[e]; break;
              case 9: x = ks[e]; break;
              default: x = col_read(a.agg_col[1], rg, r0, r + e); break;
            }
            atomicAdd(s3 + 1, (unsigned long long)x);
          }
          if (valid_at(a.agg_valid[2], r + e))
            atomicAdd((double*)(s3 + 2),
                      (double)((const float*)a.agg_col[2].data)[r + e]);
          continue;
        }
        for (uint32_t q = 0; q < a.naggs; ++q)
          agg_row<EXT>(
            &acc[grp * a.naggs + q], a.agg_op[q], a.agg_valid[q], r + e,
            [&]() -> int64_t {
              switch (a.agg_src[q]) {  // decode-once dedup vs preds/key
                case 1: return pva[e];
                case 2: return pvb[e];
                case 9: return ks[e];
                default: return col_read(a.agg_col[q], rg, r0, r + e);
              }
            },
            [&] { return ((const float*)a.agg_col[q].data)[r + e]; });
      }
    }
    if ((glen & 1ull) && threadIdx.x == 0) {
      const uint64_t r = r1 - 1;
      bool ok = true;
      int64_t pv0s = 0, pv1s = 0;
      for (uint32_t p = 0; p < a.npreds; ++p) {
        if (a.ps.isf32[p]) {
          ok &= pred_eval_fv(a.ps.op[p], a.ps.valid[p], r,
                             ((const float*)a.ps.col[p].data)[r],
                             a.ps.flo[p], a.ps.fhi[p]);
          continue;
        }
        const int64_t x = col_read(a.ps.col[p], rg, r0, r);
        if (p == 0) pv0s = x;
        else if (p == 1) pv1s = x;
        ok &= pred_eval_iv(a.ps.op[p], a.ps.valid[p], r, x,
                           a.ps.lo[p], a.ps.hi[p]);
      }
      if (ok) {
        ++my_passed;
        // NK: a NULL key gives grp == ngroups; agg_src 9 then never reads
        // grp as a value, agg_row having skipped the NULL first
        uint32_t grp = (uint32_t)col_read(a.keys, rg, r0, r);
        if constexpr (NK) {
          grp = key_group<NK>(a, grp, r);
          my_null += grp == a.ngroups;
        }
        if (ASHAPE == 1) {  // straight-lined 3-agg shape
          unsigned long long* s3 = &acc[grp * 3u];
          atomicAdd(s3, 1ull);
          if (valid_at(a.agg_valid[1], r)) {
            int64_t x;
            switch (a.agg_src[1]) {
              case 1: x = pv0s; break;
              case 2: x = pv1s; break;
              case 9: x = (int64_t)grp; break;
              default: x = col_read(a.agg_col[1], rg, r0, r); break;
            }
            atomicAdd(s3 + 1, (unsigned long long)x);
          }
          if (valid_at(a.agg_valid[2], r))
            atomicAdd((double*)(s3 + 2),
                      (double)((const float*)a.agg_col[2].data)[r]);
        } else
        for (uint32_t q = 0; q < a.naggs; ++q)
          agg_row<EXT>(
            &acc[grp * a.naggs + q], a.agg_op[q], a.agg_valid[q], r,
            [&]() -> int64_t {
              switch (a.agg_src[q]) {
                case 1: return pv0s;
                case 2: return pv1s;
                case 9: return (int64_t)grp;
                default: return col_read(a.agg_col[q], rg, r0, r);
              }
            },
            [&] { return ((const float*)a.agg_col[q].data)[r]; });
      }
    }
  }

  unsigned long long wp = my_passed;
#pragma unroll
  for (int off = 32; off; off >>= 1) wp += __shfl_down(wp, off, 64);
  if ((threadIdx.x & 63) == 0 && wp) atomicAdd(a.rows_passed, wp);
  if constexpr (NK) null_rows_flush(a.null_rows, my_null);
  __syncthreads();
  for (uint32_t i = threadIdx.x; i < nslots; i += SCAN_NTHREADS)
    agg_merge<EXT>(&a.out[i], a.agg_op[i % a.naggs], acc[i]);
}

// FoR walker with LDS payload staging: the plain walker (scan_agg_kernel<0>)
// is latency-bound on its per-pair global extract chains (3 dependent word
// loads per column per pair; measured 137G rows/s vs the raw path's 233G).
// Here each chunk's packed words for the key + first two predicate columns
// are staged cooperatively (one coalesced burst per column), and all pair
// extraction reads hit LDS. Zonemap skips, predicate fast path, and the
// agg_src decode-once dedup are identical to the unstaged walker.
template <int ASHAPE, int EXT, int NK = 0>
__launch_bounds__(SCAN_NTHREADS) __global__
void scan_agg_staged_kernel(typename ScanArgsOf<NK>::type a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  unsigned long long* acc = (unsigned long long*)smem;  // ngroups*naggs
  uint32_t* sw = (uint32_t*)smem;  // stage buffers live past acc
  const uint32_t nslots = (a.ngroups + (NK ? 1u : 0u)) * a.naggs;
  unsigned long long my_null = 0;  // NK: passing rows with a NULL key
  for (uint32_t i = threadIdx.x; i < nslots; i += SCAN_NTHREADS) acc[i] = 0;
  __syncthreads();  // a 1-row group accumulates before any chunk barrier

  const uint32_t n_rowgroups =
    (uint32_t)((a.rows + a.group_rows - 1) / a.group_rows);
  unsigned long long my_passed = 0;

  for (uint32_t rg = blockIdx.x; rg < n_rowgroups; rg += gridDim.x) {
    const uint64_t r0 = (uint64_t)rg * a.group_rows;
    const uint64_t r1 = min(a.rows, r0 + a.group_rows);
    if (preds_zone_dead<false>(a.ps, a.npreds, rg)) continue;

    const uint64_t glen = r1 - r0;
    const uint64_t glen_even = glen & ~1ull;
    for (uint64_t c0 = 0; c0 < glen_even; c0 += a.chunk_rows) {
      const uint32_t clen =
        (uint32_t)min((uint64_t)a.chunk_rows, glen_even - c0);
      __syncthreads();  // prior chunk's extraction done before overwrite
      for (uint32_t s = 0; s < a.nstage; ++s) {
        const SdbColGroupDescDev& d = a.st_desc[s][rg];
        if (d.width == 0) continue;
        // chunk starts on a 32-row multiple => word-aligned bit offset
        const uint64_t wstart = d.word_off + ((c0 * d.width) >> 5);
        const uint32_t nw =
          (uint32_t)(((uint64_t)clen * d.width + 31) >> 5) + 2;
        const uint64_t limit = a.st_paywords[s] - 1;
        uint32_t* dst = sw + a.st_lds_off[s];
        const uint32_t* src = a.st_pay[s];
        for (uint32_t i = threadIdx.x; i < nw; i += SCAN_NTHREADS)
          dst[i] = src[min(wstart + i, limit)];
      }
      if (a.f32_pay) {
        const float* src = a.f32_pay + (r0 + c0);
        float* dst = (float*)(sw + a.f32_lds_off);
        for (uint32_t i = threadIdx.x; i < clen; i += SCAN_NTHREADS)
          dst[i] = src[i];
      }
      __syncthreads();
      const uint32_t cpairs = clen >> 1;
      for (uint32_t pr = threadIdx.x; pr < cpairs; pr += SCAN_NTHREADS) {
        const uint32_t lr = 2 * pr;       // chunk-relative row
        const uint64_t r = r0 + c0 + lr;  // absolute row
        bool okv[2] = {true, true};
        int64_t pva[2] = {0, 0}, pvb[2] = {0, 0};
#pragma unroll
        for (uint32_t p = 0; p < 2; ++p) {  // fast path: first two preds
          if (p >= a.npreds) break;
          if (a.ps.isf32[p]) {
            const float* fc = (const float*)a.ps.col[p].data;
#pragma unroll
            for (int e = 0; e < 2; ++e)
              okv[e] &= pred_eval_fv(a.ps.op[p], a.ps.valid[p], r + e,
                                     fc[r + e], a.ps.flo[p],
                                     a.ps.fhi[p]);
            continue;
          }
          int64_t x0, x1;
          if (a.pred_st[p] >= 0)
            col_read2_lds(a.st_desc[a.pred_st[p]],
                          sw + a.st_lds_off[a.pred_st[p]], rg, lr, x0, x1);
          else
            col_read2(a.ps.col[p], rg, r0, r, x0, x1);
          if (p == 0) { pva[0] = x0; pva[1] = x1; }
          else { pvb[0] = x0; pvb[1] = x1; }
          const int64_t xs[2] = {x0, x1};
#pragma unroll
          for (int e = 0; e < 2; ++e)
            okv[e] &= pred_eval_iv(a.ps.op[p], a.ps.valid[p], r + e,
                                   xs[e], a.ps.lo[p], a.ps.hi[p]);
        }
        for (uint32_t p = 2; p < a.npreds; ++p) {  // rare: >2 predicates
#pragma unroll
          for (int e = 0; e < 2; ++e) {
            if (a.ps.isf32[p])
              okv[e] &= pred_eval_fv(
                a.ps.op[p], a.ps.valid[p], r + e,
                ((const float*)a.ps.col[p].data)[r + e], a.ps.flo[p],
                a.ps.fhi[p]);
            else
              okv[e] &= pred_eval_iv(a.ps.op[p], a.ps.valid[p], r + e,
                                     col_read(a.ps.col[p], rg, r0,
                                              r + e),
                                     a.ps.lo[p], a.ps.hi[p]);
          }
        }
        if (!okv[0] && !okv[1]) continue;
        int64_t k0, k1;
        if (a.key_st >= 0)
          col_read2_lds(a.st_desc[a.key_st], sw + a.st_lds_off[a.key_st],
                        rg, lr, k0, k1);
        else
          col_read2(a.keys, rg, r0, r, k0, k1);
        const int64_t ks[2] = {k0, k1};
#pragma unroll
        for (int e = 0; e < 2; ++e) {
          if (!okv[e]) continue;
          ++my_passed;
          uint32_t grp = (uint32_t)ks[e];
          if constexpr (NK) {
            grp = key_group<NK>(a, grp, r + e);
            my_null += grp == a.ngroups;
          }
          if (ASHAPE == 1) {  // straight-lined 3-agg shape
            unsigned long long* s3 = &acc[grp * 3u];
            atomicAdd(s3, 1ull);
            if (valid_at(a.agg_valid[1], r + e)) {
              int64_t x;
              switch (a.agg_src[1]) {
                case 1: x = pva[e]; break;
                case 2: x = pvb[e]; break;
                case 9: x = ks[e]; break;
                default: x = col_read(a.agg_col[1], rg, r0, r + e); break;
              }
              atomicAdd(s3 + 1, (unsigned long long)x);
            }
            if (valid_at(a.agg_valid[2], r + e)) {
              const float* fc = (const float*)a.agg_col[2].data;
              const float fv = fc == a.f32_pay
                                 ? ((const float*)(sw +
                                                   a.f32_lds_off))[lr + e]
                                 : fc[r + e];
              atomicAdd((double*)(s3 + 2), (double)fv);
            }
            continue;
          }
          for (uint32_t q = 0; q < a.naggs; ++q)
            agg_row<EXT>(
              &acc[grp * a.naggs + q], a.agg_op[q], a.agg_valid[q], r + e,
              [&]() -> int64_t {
                switch (a.agg_src[q]) {  // decode-once dedup vs preds/key
                  case 1: return pva[e];
                  case 2: return pvb[e];
                  case 9: return ks[e];
                  default: return col_read(a.agg_col[q], rg, r0, r + e);
                }
              },
              [&] {
                const float* fc = (const float*)a.agg_col[q].data;
                return fc == a.f32_pay
                         ? ((const float*)(sw + a.f32_lds_off))[lr + e]
                         : fc[r + e];
              });
        }
      }
    }
    if ((glen & 1ull) && threadIdx.x == 0) {  // odd tail row: global reads
      const uint64_t r = r1 - 1;
      bool ok = true;
      int64_t pv0s = 0, pv1s = 0;
      for (uint32_t p = 0; p < a.npreds; ++p) {
        if (a.ps.isf32[p]) {
          ok &= pred_eval_fv(a.ps.op[p], a.ps.valid[p], r,
                             ((const float*)a.ps.col[p].data)[r],
                             a.ps.flo[p], a.ps.fhi[p]);
          continue;
        }
        const int64_t x = col_read(a.ps.col[p], rg, r0, r);
        if (p == 0) pv0s = x;
        else if (p == 1) pv1s = x;
        ok &= pred_eval_iv(a.ps.op[p], a.ps.valid[p], r, x,
                           a.ps.lo[p], a.ps.hi[p]);
      }
      if (ok) {
        ++my_passed;
        // NK: a NULL key gives grp == ngroups; agg_src 9 then never reads
        // grp as a value, agg_row having skipped the NULL first
        uint32_t grp = (uint32_t)col_read(a.keys, rg, r0, r);
        if constexpr (NK) {
          grp = key_group<NK>(a, grp, r);
          my_null += grp == a.ngroups;
        }
        if (ASHAPE == 1) {  // straight-lined 3-agg shape
          unsigned long long* s3 = &acc[grp * 3u];
          atomicAdd(s3, 1ull);
          if (valid_at(a.agg_valid[1], r)) {
            int64_t x;
            switch (a.agg_src[1]) {
              case 1: x = pv0s; break;
              case 2: x = pv1s; break;
              case 9: x = (int64_t)grp; break;
              default: x = col_read(a.agg_col[1], rg, r0, r); break;
            }
            atomicAdd(s3 + 1, (unsigned long long)x);
          }
          if (valid_at(a.agg_valid[2], r))
            atomicAdd((double*)(s3 + 2),
                      (double)((const float*)a.agg_col[2].data)[r]);
        } else
        for (uint32_t q = 0; q < a.naggs; ++q)
          agg_row<EXT>(
            &acc[grp * a.naggs + q], a.agg_op[q], a.agg_valid[q], r,
            [&]() -> int64_t {
              switch (a.agg_src[q]) {
                case 1: return pv0s;
                case 2: return pv1s;
                case 9: return (int64_t)grp;
                default: return col_read(a.agg_col[q], rg, r0, r);
              }
            },
            [&] { return ((const float*)a.agg_col[q].data)[r]; });
      }
    }
  }

  unsigned long long wp = my_passed;
#pragma unroll
  for (int off = 32; off; off >>= 1) wp += __shfl_down(wp, off, 64);
  if ((threadIdx.x & 63) == 0 && wp) atomicAdd(a.rows_passed, wp);
  if constexpr (NK) null_rows_flush(a.null_rows, my_null);
  __syncthreads();
  for (uint32_t i = threadIdx.x; i < nslots; i += SCAN_NTHREADS)
    agg_merge<EXT>(&a.out[i], a.agg_op[i % a.naggs], acc[i]);
}


// ---------------------------------------------------------------------------
// General hash aggregate (round-2): arbitrary i64 group keys.
// north_star: "hash-group-by with LDS-staged open-addressed buckets" — the
// consumer the reference hands to DuckDB's PhysicalHashAggregate
// (duckdb_search_full_scan.cpp:2141-2171) for keys the dense perfect-hash
// kernel cannot take. Per-workgroup open-addressed LDS table (linear
// probing, 64-bit key CAS), flushed once into a global open-addressed
// table; rows that miss the LDS probe bound go straight to the global
// table. Exact integer aggregates; SUM(f32) in f64 (atomic order
// nondeterministic, as the dense kernel).
// ---------------------------------------------------------------------------

#define SDB_HKEY_EMPTY 0xFFFFFFFFFFFFFFFFull /* key -1 uses neg_acc */

__device__ __forceinline__ uint64_t mix64(uint64_t x) {
  // splitmix64 finalizer
  x ^= x >> 30;
  x *= 0xbf58476d1ce4e5b9ull;
  x ^= x >> 27;
  x *= 0x94d049bb133111ebull;
  x ^= x >> 31;
  return x;
}

struct HashAggArgs {
  ColRef keys;
  uint64_t rows;
  uint32_t group_rows;
  uint32_t naggs;
  uint32_t npreds;
  PredSet ps;
  ColRef agg_col[SCAN_MAX_AGGS];
  int agg_op[SCAN_MAX_AGGS];
  const unsigned long long* agg_valid[SCAN_MAX_AGGS];
  // global open-addressed table (pow2 capacity, keys init SDB_HKEY_EMPTY)
  unsigned long long* gkeys;
  unsigned long long* gacc;  // [cap * naggs]
  uint32_t gcap_mask;
  uint32_t max_groups;
  uint32_t* ginserts;   // distinct-key counter (contract check)
  uint32_t* goverflow;  // probe bound exceeded
  unsigned long long* neg_acc;  // [naggs+1]: key == -1 accumulators + flag
  unsigned long long* rows_passed;
  uint32_t lds_slots;   // pow2 (0 = LDS staging disabled)
};

// argument of the nullable-group-key (NK = 1) instantiation; NK = 0 keeps
// HashAggArgs itself (see ScanArgsNK)
struct HashAggArgsNK : HashAggArgs {
  const unsigned long long* key_valid;  // the key column's own plane
  unsigned long long* null_acc;  // [naggs+1]: NULL-group accumulators +
                                 // count of passing NULL-key rows
};
template <int NK> struct HashAggArgsOf { using type = HashAggArgs; };
template <> struct HashAggArgsOf<1> { using type = HashAggArgsNK; };

// probe/insert into the global table; returns slot or -1 (overflow).
__device__ __forceinline__ int64_t hash_global_upsert(
  const HashAggArgs& a, uint64_t k) {
  uint32_t h = (uint32_t)mix64(k) & a.gcap_mask;
  for (uint32_t i = 0; i <= a.gcap_mask; ++i) {
    const unsigned long long cur = __hip_atomic_load(
      &a.gkeys[h], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (cur == k) return (int64_t)h;
    if (cur == SDB_HKEY_EMPTY) {
      const unsigned long long prev =
        atomicCAS(&a.gkeys[h], SDB_HKEY_EMPTY, k);
      if (prev == SDB_HKEY_EMPTY) {
        atomicAdd(a.ginserts, 1u);
        return (int64_t)h;
      }
      if (prev == k) return (int64_t)h;
    }
    h = (h + 1) & a.gcap_mask;
  }
  atomicExch(a.goverflow, 1u);
  return -1;
}

template <int EXT>
__device__ __forceinline__ void hash_acc_add(const HashAggArgs& a,
                                             unsigned long long* acc,
                                             uint32_t q, uint32_t rg,
                                             uint64_t r0, uint64_t r,
                                             bool global_scope) {
  agg_row<EXT>(
    &acc[q], a.agg_op[q], a.agg_valid[q], r,
    [&] { return col_read(a.agg_col[q], rg, r0, r); },
    [&] { return ((const float*)a.agg_col[q].data)[r]; });
  (void)global_scope;
}

// NK: 1 = the key column carries a validity plane (a.key_valid). A passing
// row whose key bit is cleared feeds the NULL group and nothing else: its
// stored key is not read, so it can light neither the key -1 group nor a
// table slot. The NULL group follows the key -1 pattern — [naggs]
// accumulators plus a word in the misc buffer (a.null_acc), here the count
// of such rows — with one difference: a quarter of all rows may be NULL,
// so each workgroup accumulates them in LDS (lnull, past the table) and
// merges once at the end, where key -1 rows go to global one by one.
template <int EXT, int NK = 0>
__launch_bounds__(SCAN_NTHREADS) __global__
void scan_agg_hash_kernel(typename HashAggArgsOf<NK>::type a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  unsigned long long* lkey = (unsigned long long*)smem;     // lds_slots
  unsigned long long* lacc = lkey + a.lds_slots;            // slots*naggs
  unsigned long long* lnull = lacc + a.lds_slots * a.naggs;  // NK: naggs
  const uint32_t S_mask = a.lds_slots ? a.lds_slots - 1 : 0;
  for (uint32_t i = threadIdx.x; i < a.lds_slots * (1 + a.naggs);
       i += SCAN_NTHREADS)
    lkey[i] = i < a.lds_slots ? SDB_HKEY_EMPTY : 0ull;
  if (NK && threadIdx.x < a.naggs) lnull[threadIdx.x] = 0ull;
  unsigned long long my_null = 0;  // NK: passing rows with a NULL key
  __syncthreads();

  const uint32_t n_rowgroups =
    (uint32_t)((a.rows + a.group_rows - 1) / a.group_rows);
  unsigned long long my_passed = 0;

  for (uint32_t rg = blockIdx.x; rg < n_rowgroups; rg += gridDim.x) {
    const uint64_t r0 = (uint64_t)rg * a.group_rows;
    const uint64_t r1 = min(a.rows, r0 + a.group_rows);
    if (preds_zone_dead(a.ps, a.npreds, rg)) continue;

    for (uint64_t r = r0 + threadIdx.x; r < r1; r += SCAN_NTHREADS) {
      if (!preds_pass(a.ps, a.npreds, rg, r0, r)) continue;
      ++my_passed;
      if constexpr (NK) {
        if (!valid_at(a.key_valid, r)) {  // NULL key: before key -1
          ++my_null;
          for (uint32_t q = 0; q < a.naggs; ++q)
            hash_acc_add<EXT>(a, lnull, q, rg, r0, r, false);
          continue;
        }
      }
      const uint64_t k = (uint64_t)col_read(a.keys, rg, r0, r);
      if (k == SDB_HKEY_EMPTY) {  // actual key -1: dedicated accumulators
        if (!__hip_atomic_load(&a.neg_acc[a.naggs], __ATOMIC_RELAXED,
                               __HIP_MEMORY_SCOPE_AGENT))
          atomicExch(&a.neg_acc[a.naggs], 1ull);
        for (uint32_t q = 0; q < a.naggs; ++q)
          hash_acc_add<EXT>(a, a.neg_acc, q, rg, r0, r, true);
        continue;
      }
      // LDS open-addressed probe (bounded), then global fallback
      int slot = -1;
      if (a.lds_slots) {
        uint32_t h = (uint32_t)mix64(k) & S_mask;
        for (uint32_t i = 0; i < 32; ++i) {
          const unsigned long long cur = lkey[h];
          if (cur == k) {
            slot = (int)h;
            break;
          }
          if (cur == SDB_HKEY_EMPTY) {
            const unsigned long long prev =
              atomicCAS(&lkey[h], SDB_HKEY_EMPTY, k);
            if (prev == SDB_HKEY_EMPTY || prev == k) {
              slot = (int)h;
              break;
            }
          }
          h = (h + 1) & S_mask;
        }
      }
      if (slot >= 0) {
        hash_acc_add<EXT>(a, &lacc[(uint32_t)slot * a.naggs], 0, rg, r0,
                          r, false);
        for (uint32_t q = 1; q < a.naggs; ++q)
          hash_acc_add<EXT>(a, &lacc[(uint32_t)slot * a.naggs], q, rg, r0,
                            r, false);
      } else {
        const int64_t g = hash_global_upsert(a, k);
        if (g < 0) return;  // table overflow: host reports SDB_ERR_OOM
        for (uint32_t q = 0; q < a.naggs; ++q)
          hash_acc_add<EXT>(a, &a.gacc[(uint64_t)g * a.naggs], q, rg, r0,
                            r, true);
      }
    }
  }

  unsigned long long wp = my_passed;
#pragma unroll
  for (int off = 32; off; off >>= 1) wp += __shfl_down(wp, off, 64);
  if ((threadIdx.x & 63) == 0 && wp) atomicAdd(a.rows_passed, wp);
  if constexpr (NK) null_rows_flush(&a.null_acc[a.naggs], my_null);
  __syncthreads();
  if constexpr (NK) {  // the workgroup's NULL group into the global one
    if (threadIdx.x < a.naggs)
      agg_merge<EXT>(&a.null_acc[threadIdx.x], a.agg_op[threadIdx.x],
                     lnull[threadIdx.x]);
  }
  // flush the LDS table into the global table
  for (uint32_t i = threadIdx.x; i < a.lds_slots; i += SCAN_NTHREADS) {
    const unsigned long long k = lkey[i];
    if (k == SDB_HKEY_EMPTY) continue;
    const int64_t g = hash_global_upsert(a, k);
    if (g < 0) return;
    for (uint32_t q = 0; q < a.naggs; ++q)
      agg_merge<EXT>(&a.gacc[(uint64_t)g * a.naggs + q], a.agg_op[q],
                     lacc[i * a.naggs + q]);
  }
}

// ---------------------------------------------------------------------------
// Composite group key: GROUP BY 1..SDB_MAX_GROUP_KEYS nullable i64 columns.
// A tuple does not fit the 64-bit key the tables CAS, and a wider key would
// need a thread to wait for another's publish — a spin inside a divergent
// wave. So the tables keep what they key on today, one u64: a 64-bit hash of
// the row's tuple, computed in registers (tuple_hash). What makes the answer
// exact is carried NEXT TO the accumulators: every slot, in LDS and in the
// global table, ends in 2*nkeys + 2 witness words —
//   [naggs + 2j]     MIN of key j over the slot's rows where key j is valid
//   [naggs + 2j + 1] MAX of the same; both as agg_row's "bigger wins" codes
//   [naggs + 2*nkeys]      OR of the rows' null masks (bit j = key j NULL)
//   [naggs + 2*nkeys + 1]  OR of their complements (the AND, zero-initialised)
// The host reads them back: a slot holds ONE tuple iff the two masks are
// disjoint and min_j == max_j in every position not NULL, and that tuple is
// then (min_j) with the mask. Two different tuples differ in some position,
// in null-ness (the masks overlap) or in value (min != max), so the check is
// complete; a slot that fails it makes the host run the scan again under the
// next seed. No thread ever waits for another.
// ---------------------------------------------------------------------------

// argument of the composite-key kernel; the other instantiations keep their
// own structs (see ScanArgsNK)
struct HashAggArgsMK : HashAggArgs {
  uint32_t nkeys;                    // 1..SDB_MAX_GROUP_KEYS
  uint32_t stride;                   // words per slot: naggs + 2*nkeys + 2
  ColRef mkeys[SDB_MAX_GROUP_KEYS];
  const unsigned long long* key_valid[SDB_MAX_GROUP_KEYS];  // null = no plane
  uint64_t seed;                     // 0..3, one per attempt
  uint64_t hash_mask;                // all ones unless SDB_MK_HASH_BITS
};

// The hash of a tuple (include/sdb_gpu.h states it; the tests restate it).
// A NULL position contributes 0, whatever the row stores there.
__device__ __forceinline__ uint64_t tuple_hash(
  const HashAggArgsMK& a, const int64_t (&key)[SDB_MAX_GROUP_KEYS],
  uint32_t nullmask) {
  uint64_t h = mix64(a.seed + 1);
#pragma unroll
  for (uint32_t j = 0; j < SDB_MAX_GROUP_KEYS; ++j)
    if (j < a.nkeys)
      h = mix64(h ^ (((nullmask >> j) & 1u) ? 0ull : (uint64_t)key[j]));
  h = mix64(h ^ (uint64_t)nullmask);
  h &= a.hash_mask;
  if (h == SDB_HKEY_EMPTY) h -= 1;  // the empty marker is no hash
  return h;
}

// One row's tuple into the witness words of its slot. In LDS (GLOBAL = 0)
// the words take the row as the accumulators do, one no-return atomic each.
// In the global table every atomic is a trip to L2, so there each word is
// read first and the atomic issued only if it would change the word: every
// word only ever grows (a max, or an OR), and from a slot's second row on it
// already holds what the row would write unless two tuples share the slot.
// A stale read can only cost a redundant atomic, never lose one.
template <int GLOBAL>
__device__ __forceinline__ bool witness_has(const unsigned long long* p,
                                            unsigned long long v,
                                            bool is_or) {
  if (!GLOBAL) return false;
  const unsigned long long cur =
    __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  return is_or ? (v & ~cur) == 0 : cur >= v;
}

template <int GLOBAL>
__device__ __forceinline__ void witness_row(
  unsigned long long* w, uint32_t nkeys,
  const int64_t (&key)[SDB_MAX_GROUP_KEYS], uint32_t nullmask) {
#pragma unroll
  for (uint32_t j = 0; j < SDB_MAX_GROUP_KEYS; ++j)
    if (j < nkeys && !((nullmask >> j) & 1u)) {
      const unsigned long long c = (unsigned long long)key[j] ^ SDB_I64_SIGN;
      if (!witness_has<GLOBAL>(&w[2 * j], ~c, false))
        atomicMax(&w[2 * j], ~c);
      if (!witness_has<GLOBAL>(&w[2 * j + 1], c, false))
        atomicMax(&w[2 * j + 1], c);
    }
  const unsigned long long nm = nullmask;
  const unsigned long long comp = ~nullmask & ((1u << nkeys) - 1u);
  if (nm && !witness_has<GLOBAL>(&w[2 * nkeys], nm, true))
    atomicOr(&w[2 * nkeys], nm);
  if (comp && !witness_has<GLOBAL>(&w[2 * nkeys + 1], comp, true))
    atomicOr(&w[2 * nkeys + 1], comp);
}

// The live slots of the global table, accumulators and witness words, packed
// into out[max_out * stride] in no particular order (the host sorts): the
// readback is then the groups found, not the whole half-empty table. *nout
// counts every live slot; slots past max_out are dropped, and the host has
// by then answered SDB_ERR_OOM from the insert count.
__global__ void hash_multi_compact_kernel(
  const unsigned long long* __restrict__ gkeys,
  const unsigned long long* __restrict__ gacc, uint32_t cap, uint32_t stride,
  uint32_t max_out, unsigned long long* __restrict__ out, uint32_t* nout) {
  const uint32_t step = gridDim.x * blockDim.x;
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < cap;
       i += step) {
    if (gkeys[i] == SDB_HKEY_EMPTY) continue;
    const uint32_t at = atomicAdd(nout, 1u);
    if (at >= max_out) continue;
    for (uint32_t w = 0; w < stride; ++w)
      out[(uint64_t)at * stride + w] = gacc[(uint64_t)i * stride + w];
  }
}

__launch_bounds__(SCAN_NTHREADS) __global__
void scan_agg_hash_multi_kernel(HashAggArgsMK a) {
  constexpr int EXT = 1;  // one instantiation: EXT = 1 handles every op
  extern __shared__ __attribute__((aligned(16))) char smem[];
  unsigned long long* lkey = (unsigned long long*)smem;  // lds_slots
  unsigned long long* lacc = lkey + a.lds_slots;         // slots*stride
  const uint32_t S_mask = a.lds_slots ? a.lds_slots - 1 : 0;
  for (uint32_t i = threadIdx.x; i < a.lds_slots * (1 + a.stride);
       i += SCAN_NTHREADS)
    lkey[i] = i < a.lds_slots ? SDB_HKEY_EMPTY : 0ull;
  __syncthreads();

  const uint32_t n_rowgroups =
    (uint32_t)((a.rows + a.group_rows - 1) / a.group_rows);
  unsigned long long my_passed = 0;

  for (uint32_t rg = blockIdx.x; rg < n_rowgroups; rg += gridDim.x) {
    const uint64_t r0 = (uint64_t)rg * a.group_rows;
    const uint64_t r1 = min(a.rows, r0 + a.group_rows);
    // This kernel keeps its own zonemap switch and eager predicate loop:
    // with preds_pass its 1024-group probe arm measured 1 % slower, once
    // outside the parent's spread, and with preds_zone_dead alone 3 %. Its
    // STRMASK column is the first key, so the eager read is in bounds.
    bool dead = false;
    for (uint32_t p = 0; p < a.npreds; ++p) {
      if (a.ps.col[p].desc && !a.ps.isf32[p]) {
        const SdbColGroupDescDev& d = a.ps.col[p].desc[rg];
        switch (a.ps.op[p]) {
          case SDB_PRED_LT: dead |= d.vmin >= a.ps.lo[p]; break;
          case SDB_PRED_GE: dead |= d.vmax < a.ps.lo[p]; break;
          case SDB_PRED_BETWEEN:
            dead |= (d.vmax < a.ps.lo[p]) | (d.vmin > a.ps.hi[p]);
            break;
          case SDB_PRED_EQ:
            dead |= (d.vmax < a.ps.lo[p]) | (d.vmin > a.ps.lo[p]);
            break;
          default: break;
        }
      }
    }
    if (dead) continue;

    for (uint64_t r = r0 + threadIdx.x; r < r1; r += SCAN_NTHREADS) {
      bool ok = true;
      for (uint32_t p = 0; p < a.npreds; ++p) {
        if (a.ps.isf32[p])
          ok &= pred_eval_fv(a.ps.op[p], a.ps.valid[p], r,
                             ((const float*)a.ps.col[p].data)[r],
                             a.ps.flo[p], a.ps.fhi[p]);
        else
          ok &= pred_eval_iv(a.ps.op[p], a.ps.valid[p], r,
                             col_read(a.ps.col[p], rg, r0, r),
                             a.ps.lo[p], a.ps.hi[p]);
      }
      if (!ok) continue;
      ++my_passed;
      // the tuple in registers: a NULL position's stored value is read (the
      // row is in bounds) and discarded by tuple_hash / witness_row
      int64_t key[SDB_MAX_GROUP_KEYS];
      uint32_t nullmask = 0;
#pragma unroll
      for (uint32_t j = 0; j < SDB_MAX_GROUP_KEYS; ++j) {
        key[j] = 0;
        if (j < a.nkeys) {
          key[j] = col_read(a.mkeys[j], rg, r0, r);
          if (!valid_at(a.key_valid[j], r)) nullmask |= 1u << j;
        }
      }
      const uint64_t k = tuple_hash(a, key, nullmask);
      // LDS open-addressed probe (bounded), then global fallback
      int slot = -1;
      if (a.lds_slots) {
        uint32_t h = (uint32_t)mix64(k) & S_mask;
        for (uint32_t i = 0; i < 32; ++i) {
          const unsigned long long cur = lkey[h];
          if (cur == k) {
            slot = (int)h;
            break;
          }
          if (cur == SDB_HKEY_EMPTY) {
            const unsigned long long prev =
              atomicCAS(&lkey[h], SDB_HKEY_EMPTY, k);
            if (prev == SDB_HKEY_EMPTY || prev == k) {
              slot = (int)h;
              break;
            }
          }
          h = (h + 1) & S_mask;
        }
      }
      // two arms, so that each knows its address space (LDS / global)
      if (slot >= 0) {
        unsigned long long* acc = &lacc[(uint32_t)slot * a.stride];
        for (uint32_t q = 0; q < a.naggs; ++q)
          hash_acc_add<EXT>(a, acc, q, rg, r0, r, false);
        witness_row<0>(acc + a.naggs, a.nkeys, key, nullmask);
      } else {
        const int64_t g = hash_global_upsert(a, k);
        if (g < 0) return;  // table overflow: host reports SDB_ERR_OOM
        unsigned long long* acc = &a.gacc[(uint64_t)g * a.stride];
        for (uint32_t q = 0; q < a.naggs; ++q)
          hash_acc_add<EXT>(a, acc, q, rg, r0, r, true);
        witness_row<1>(acc + a.naggs, a.nkeys, key, nullmask);
      }
    }
  }

  unsigned long long wp = my_passed;
#pragma unroll
  for (int off = 32; off; off >>= 1) wp += __shfl_down(wp, off, 64);
  if ((threadIdx.x & 63) == 0 && wp) atomicAdd(a.rows_passed, wp);
  __syncthreads();
  // flush the LDS table into the global table: aggregates as agg_merge has
  // them, min/max witness codes by max, the two masks by OR
  for (uint32_t i = threadIdx.x; i < a.lds_slots; i += SCAN_NTHREADS) {
    const unsigned long long k = lkey[i];
    if (k == SDB_HKEY_EMPTY) continue;
    const int64_t g = hash_global_upsert(a, k);
    if (g < 0) return;
    const unsigned long long* src = &lacc[i * a.stride];
    unsigned long long* dst = &a.gacc[(uint64_t)g * a.stride];
    for (uint32_t q = 0; q < a.naggs; ++q)
      agg_merge<EXT>(&dst[q], a.agg_op[q], src[q]);
    for (uint32_t w = a.naggs; w < a.naggs + 2 * a.nkeys; ++w)
      if (src[w]) atomicMax(&dst[w], src[w]);
    for (uint32_t w = a.naggs + 2 * a.nkeys; w < a.stride; ++w)
      if (src[w]) atomicOr(&dst[w], src[w]);
  }
}

// ---------------------------------------------------------------------------
// ORDER BY col [DESC] LIMIT k over the scan (sdb_gpu_scan_topn): an exact MSD
// radix select, then a collect pass. Every passing non-NULL row has a rank
// code, a u64 where BIGGER RANKS FIRST: i64 DESC is x ^ 2^63 (the MAX_I64
// code of agg_row), ASC its complement; f32 is the 32-bit f32_order_key,
// complemented within 32 bits for ASC, so a code is W = 64 or 32 bits wide.
// NULL is a class of its own and never a code (INT64_MIN DESC is code 0).
//
// One kernel body, three modes, in the unstaged walker's shape (a workgroup
// per row group, grid-strided, predicate zonemap skips):
//   HIST     histogram of the next 11-bit digit over the rows whose higher
//            digits equal the prefix the host has chosen so far; 2048 u32 bins
//            in LDS, flushed once per workgroup into the global u64 bins.
//            The first pass also counts rows passed and passing NULL rows.
//   COUNT    members of one class (code == thr, or NULL) per row group, for
//            the row-order arm: each row group belongs to one workgroup, which
//            stores its count with a plain store.
//   COLLECT  appends (code, row): code > thr from every row group, code == thr
//            (or NULL, for the NULL class) from row groups < tie_rg_end only.
//            Appends are wave-aggregated (ballot, one cursor add per wave,
//            lanes write at base + rank), first into an LDS stage that the
//            workgroup moves to the candidate buffer with one add on the
//            global cursor per row group, and straight to the global cursor
//            once the stage is full. Every global store is bounds-checked
//            against cand_cap.
// A FoR order column skips row groups on its own zonemap in every value mode;
// the NULL class never does (a NULL row's stored value is not its rank).
// ---------------------------------------------------------------------------
#define TOPN_BINS 2048u
#define TOPN_MISC 8u  // words after the bins: rows passed, NULL rows passed,
                      // collect cursor, overflow flag, row groups skipped
#ifndef TOPN_STAGE
#define TOPN_STAGE 4096u  // candidates a workgroup stages in LDS (64 KiB)
#endif
enum { TOPN_HIST = 0, TOPN_COUNT = 1, TOPN_COLLECT = 2 };

struct TopnCand {
  unsigned long long code, row;
};

struct TopnArgs {
  ColRef order;
  const unsigned long long* order_valid;  // null = no NULL rows
  uint64_t rows;
  uint32_t group_rows;
  uint32_t desc;
  uint32_t npreds;
  PredSet ps;
  // HIST: rows with (code & prefix_mask) == prefix, digit (code >> shift) &
  // digit_mask; first = this pass also counts rows passed / NULL rows
  unsigned long long prefix_mask, prefix;
  uint32_t shift, digit_mask;
  uint32_t first;
  unsigned long long* hist;  // [TOPN_BINS]
  unsigned long long* misc;  // [TOPN_MISC]
  // COUNT / COLLECT
  uint32_t cls_null;    // the class is NULL, not code == thr
  uint32_t tie_rg_end;  // class members count from row groups below this
  unsigned long long thr;
  uint32_t* rg_count;   // [row groups]
  TopnCand* cand;
  unsigned long long cand_cap;
};

// PredSet sits where the eight predicate arrays sat in each struct, so every
// kernel-argument offset is what it was before the arrays were shared
static_assert(sizeof(PredSet) == 224 && alignof(PredSet) == 8, "PredSet");
static_assert(offsetof(ScanArgs, ps) == 40 &&
              offsetof(ScanArgs, agg_col) == 264, "ScanArgs layout");
static_assert(offsetof(HashAggArgs, ps) == 40 &&
              offsetof(HashAggArgs, agg_col) == 264, "HashAggArgs layout");
static_assert(offsetof(TopnArgs, ps) == 48 &&
              offsetof(TopnArgs, prefix_mask) == 272, "TopnArgs layout");

// OT: 0 = raw i64, 1 = FoR i64, 2 = f32
template <int OT>
__device__ __forceinline__ unsigned long long topn_code(const TopnArgs& a,
                                                        uint32_t rg,
                                                        uint64_t r0,
                                                        uint64_t r) {
  if (OT == 2) {
    const uint32_t key = f32_order_key(((const float*)a.order.data)[r]);
    return a.desc ? key : (uint32_t)~key;
  }
  const int64_t x = OT == 1 ? col_read(a.order, rg, r0, r)
                            : ((const long long*)a.order.data)[r];
  const unsigned long long c = (unsigned long long)x ^ SDB_I64_SIGN;
  return a.desc ? c : ~c;
}

template <int OT, int MODE>
__launch_bounds__(SCAN_NTHREADS) __global__ void topn_kernel(TopnArgs a) {
  __shared__ uint32_t lh[MODE == TOPN_HIST ? TOPN_BINS : 1];
  // COLLECT: the candidates of one row group, staged so that a sparse row
  // group costs one add on the global cursor, not one per emitting wave
  __shared__ TopnCand lbuf[MODE == TOPN_COLLECT ? TOPN_STAGE : 1];
  __shared__ uint32_t lcnt;
  __shared__ unsigned long long lbase;
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t n_rowgroups =
    (uint32_t)((a.rows + a.group_rows - 1) / a.group_rows);
  unsigned long long my_passed = 0, my_null = 0;
  if (MODE == TOPN_HIST) {
    for (uint32_t i = threadIdx.x; i < TOPN_BINS; i += SCAN_NTHREADS)
      lh[i] = 0;
    __syncthreads();
  }

  for (uint32_t rg = blockIdx.x; rg < n_rowgroups; rg += gridDim.x) {
    const uint64_t r0 = (uint64_t)rg * a.group_rows;
    const uint64_t r1 = min(a.rows, r0 + a.group_rows);
    // predicate zonemaps, as in the aggregate walkers
    bool dead = preds_zone_dead(a.ps, a.npreds, rg);
    if (MODE != TOPN_HIST && a.cls_null && rg >= a.tie_rg_end) dead = true;
    // the ORDER column's own zonemap: the code range of the row group
    // against what this pass can still use. Never for the NULL class.
    if (OT == 1 && !dead && !(MODE != TOPN_HIST && a.cls_null)) {
      const SdbColGroupDescDev& d = a.order.desc[rg];
      const unsigned long long lo = (unsigned long long)d.vmin ^ SDB_I64_SIGN;
      const unsigned long long hi = (unsigned long long)d.vmax ^ SDB_I64_SIGN;
      const unsigned long long cmin = a.desc ? lo : ~hi;
      const unsigned long long cmax = a.desc ? hi : ~lo;
      bool odead;
      if (MODE == TOPN_HIST)
        odead = (cmax < a.prefix) | (cmin > (a.prefix | ~a.prefix_mask));
      else if (MODE == TOPN_COUNT)
        odead = (a.thr < cmin) | (a.thr > cmax);
      else
        odead = (cmax < a.thr) | (cmax == a.thr && rg >= a.tie_rg_end);
      if (odead) {
        if (threadIdx.x == 0) atomicAdd(&a.misc[4], 1ull);
        dead = true;
      }
    }
    if (dead) {
      if (MODE == TOPN_COUNT && threadIdx.x == 0) a.rg_count[rg] = 0;
      continue;
    }
    if (MODE == TOPN_COUNT) {
      if (threadIdx.x == 0) lh[0] = 0;
      __syncthreads();
    }
    if (MODE == TOPN_COLLECT) {
      if (threadIdx.x == 0) lcnt = 0;
      __syncthreads();
    }

    // every lane of the workgroup runs every trip (a row past r1 merely
    // fails), so the ballots below see whole waves
    for (uint64_t b = r0; b < r1; b += SCAN_NTHREADS) {
      const uint64_t r = b + threadIdx.x;
      const bool ok = r < r1 && preds_pass(a.ps, a.npreds, rg, r0, r);
      const bool isnull = ok && !valid_at(a.order_valid, r);
      const bool val = ok && !isnull;
      unsigned long long code = 0;
      if (val && !(MODE != TOPN_HIST && a.cls_null))
        code = topn_code<OT>(a, rg, r0, r);

      if (MODE == TOPN_HIST) {
        if (a.first) {
          my_passed += ok;
          my_null += isnull;
        }
        const bool in = val && (code & a.prefix_mask) == a.prefix;
        const uint32_t dg = (uint32_t)(code >> a.shift) & a.digit_mask;
        const unsigned long long m = __ballot(in);
        if (m) {
          // sorted and low-cardinality columns put a whole wave into one
          // bin: one lane adds the popcount instead of 64 adds serialising
          // on one LDS address
          const int lead = __ffsll((long long)m) - 1;
          const uint32_t d0 = (uint32_t)__shfl((int)dg, lead, 64);
          if (__ballot(in && dg == d0) == m) {
            if ((int)lane == lead) atomicAdd(&lh[d0], (uint32_t)__popcll(m));
          } else if (in) {
            atomicAdd(&lh[dg], 1u);
          }
        }
      } else if (MODE == TOPN_COUNT) {
        const bool member = a.cls_null ? isnull : (val && code == a.thr);
        const unsigned long long m = __ballot(member);
        if (m && lane == 0) atomicAdd(&lh[0], (uint32_t)__popcll(m));
      } else {
        const bool emit =
          a.cls_null ? isnull
                     : (val && (code > a.thr ||
                                (code == a.thr && rg < a.tie_rg_end)));
        const unsigned long long m = __ballot(emit);
        if (m) {
          // wave-aggregated append into the workgroup's LDS stage: one LDS
          // cursor add per wave, lanes write at base + rank
          const int lead = __ffsll((long long)m) - 1;
          const uint32_t rank =
            (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
          uint32_t lb = 0;
          if ((int)lane == lead)
            lb = atomicAdd(&lcnt, (uint32_t)__popcll(m));
          lb = (uint32_t)__shfl((int)lb, lead, 64);
          const bool staged = emit && lb + rank < TOPN_STAGE;
          if (staged) lbuf[lb + rank] = TopnCand{code, r};
          // stage full: the rest of the wave goes to the global cursor,
          // again one add per wave
          const unsigned long long ms = __ballot(emit && !staged);
          if (ms) {
            const int lead2 = __ffsll((long long)ms) - 1;
            unsigned long long base = 0;
            if ((int)lane == lead2)
              base = atomicAdd(&a.misc[2], (unsigned long long)__popcll(ms));
            base = __shfl(base, lead2, 64);
            if (emit && !staged) {
              const unsigned long long idx =
                base +
                (unsigned long long)__popcll(ms & ((1ull << lane) - 1ull));
              if (idx < a.cand_cap)
                a.cand[idx] = TopnCand{code, r};
              else
                atomicOr(&a.misc[3], 1ull);  // the host returns SDB_ERR_OOM
            }
          }
        }
      }
    }
    if (MODE == TOPN_COLLECT) {
      // the row group's stage into the candidate buffer: one global cursor
      // add per workgroup, every store bounds-checked
      __syncthreads();
      const uint32_t ns = min(lcnt, TOPN_STAGE);
      if (threadIdx.x == 0 && ns)
        lbase = atomicAdd(&a.misc[2], (unsigned long long)ns);
      __syncthreads();
      for (uint32_t i = threadIdx.x; i < ns; i += SCAN_NTHREADS) {
        const unsigned long long idx = lbase + i;
        if (idx < a.cand_cap)
          a.cand[idx] = lbuf[i];
        else
          atomicOr(&a.misc[3], 1ull);
      }
    }
    if (MODE == TOPN_COUNT) {
      __syncthreads();
      if (threadIdx.x == 0) a.rg_count[rg] = lh[0];
    }
  }

  if (MODE == TOPN_HIST) {
    if (a.first) {
#pragma unroll
      for (int off = 32; off; off >>= 1) {
        my_passed += __shfl_down(my_passed, off, 64);
        my_null += __shfl_down(my_null, off, 64);
      }
      if (lane == 0 && my_passed) atomicAdd(&a.misc[0], my_passed);
      if (lane == 0 && my_null) atomicAdd(&a.misc[1], my_null);
    }
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < TOPN_BINS; i += SCAN_NTHREADS)
      if (lh[i]) atomicAdd(&a.hist[i], (unsigned long long)lh[i]);
  }
}

// value and NULL flag of one column at n given rows (sdb_gpu_table_gather).
// type: SdbColType. i64 values travel as their bits, f32 as the float's bits
// in the low word, every NaN canonicalised; a NULL row returns 0.
struct GatherArgs {
  ColRef col;
  const unsigned long long* valid;
  int type;
  uint32_t group_rows;
  const unsigned long long* rows;
  uint64_t n;
  unsigned long long* vals;
  uint8_t* nulls;
};

__global__ void table_gather_kernel(GatherArgs g) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= g.n) return;
  const uint64_t r = g.rows[i];
  const bool isnull = !valid_at(g.valid, r);
  unsigned long long v = 0;
  if (!isnull) {
    if (g.type == SDB_COL_F32) {
      uint32_t b = __float_as_uint(((const float*)g.col.data)[r]);
      if ((b & 0x7FFFFFFFu) > 0x7F800000u) b = 0x7FC00000u;
      v = b;
    } else {
      const uint32_t rg = (uint32_t)(r / g.group_rows);
      v = (unsigned long long)col_read(g.col, rg,
                                       (uint64_t)rg * g.group_rows, r);
    }
  }
  g.vals[i] = v;
  g.nulls[i] = isnull ? 1 : 0;
}

template <int OT>
static void topn_launch_ot(int mode, uint32_t nblocks, hipStream_t stream,
                           const TopnArgs& a) {
  if (mode == TOPN_HIST)
    hipLaunchKernelGGL((topn_kernel<OT, TOPN_HIST>), dim3(nblocks),
                       dim3(SCAN_NTHREADS), 0, stream, a);
  else if (mode == TOPN_COUNT)
    hipLaunchKernelGGL((topn_kernel<OT, TOPN_COUNT>), dim3(nblocks),
                       dim3(SCAN_NTHREADS), 0, stream, a);
  else
    hipLaunchKernelGGL((topn_kernel<OT, TOPN_COLLECT>), dim3(nblocks),
                       dim3(SCAN_NTHREADS), 0, stream, a);
}

static void topn_launch(int ot, int mode, uint32_t nblocks,
                        hipStream_t stream, const TopnArgs& a) {
  if (ot == 2) topn_launch_ot<2>(mode, nblocks, stream, a);
  else if (ot == 1) topn_launch_ot<1>(mode, nblocks, stream, a);
  else topn_launch_ot<0>(mode, nblocks, stream, a);
}

extern "C" {

static void table_free_str(SdbGpuTable* tab) {
  for (uint32_t k = 0; k < SDB_MAX_STRCOLS; ++k) {
    if (tab->str_off[k]) (void)hipFree(tab->str_off[k]);
    if (tab->str_blob[k]) (void)hipFree(tab->str_blob[k]);
    if (tab->str_mask[k]) (void)hipFree(tab->str_mask[k]);
  }
  if (tab->like_prog) (void)hipFree(tab->like_prog);
}

static void table_free_partial(SdbGpuTable* tab) {
  for (uint32_t c = 0; c < 16; ++c)
    if (tab->cols[c]) (void)hipFree(tab->cols[c]);
  table_free_str(tab);
  delete tab;
}

int sdb_gpu_table_load(SdbGpuCtx* ctx, const SdbColumnView* cols,
                       uint32_t ncols, uint64_t rows, SdbGpuTable** out) {
  if (!ctx || !cols || !out || ncols == 0 || ncols > 16)
    return SDB_ERR_INVALID;
  // owns the partially loaded table: every early return frees its columns
  std::unique_ptr<SdbGpuTable, void (*)(SdbGpuTable*)> hold(
    new SdbGpuTable{}, table_free_partial);
  SdbGpuTable* tab = hold.get();
  tab->ncols = ncols;
  tab->rows = rows;
  tab->group_rows = 0;
  for (uint32_t c = 0; c < ncols; ++c) {
    tab->types[c] = cols[c].type;
    if (cols[c].type == SDB_COL_I64_FOR) {
      // encoded blob: upload whole blob, point refs into it
      SdbColHeaderDev hdr;
      std::memcpy(&hdr, cols[c].data, sizeof(hdr));
      // internal consistency (the view carries no external size, so the
      // declared extents must at least agree with themselves and `rows`)
      if (hdr.magic != SDB_COL_MAGIC_DEV || hdr.rows != rows ||
          hdr.group_rows == 0 ||
          hdr.ngroups != (rows + hdr.group_rows - 1) / hdr.group_rows ||
          hdr.off_desc > hdr.size || hdr.off_payload > hdr.size ||
          (uint64_t)hdr.ngroups * sizeof(SdbColGroupDescDev) >
            hdr.size - hdr.off_desc)
        return SDB_ERR_INVALID;
      // FoR columns must share the group tiling
      if (tab->group_rows && tab->group_rows != hdr.group_rows)
        return SDB_ERR_INVALID;
      tab->group_rows = hdr.group_rows;
      // +4 pad bytes: bits_at reads one slack word past the final value
      HIP_CHECK(hipMalloc(&tab->cols[c], hdr.size + 4));
      HIP_CHECK(hipMemcpy(tab->cols[c], cols[c].data, hdr.size,
                          hipMemcpyHostToDevice));
      tab->refs[c].data = (const uint8_t*)tab->cols[c] + hdr.off_payload;
      tab->refs[c].desc = (const SdbColGroupDescDev*)((const uint8_t*)
                            tab->cols[c] + hdr.off_desc);
      // host-side pass over the group table: max width sizes the staged
      // kernel's LDS budget; payword count bounds its slack loads
      const SdbColGroupDescDev* hdesc =
        (const SdbColGroupDescDev*)((const uint8_t*)cols[c].data +
                                    hdr.off_desc);
      uint16_t mw = 0;
      int64_t cmin = INT64_MAX, cmax = INT64_MIN;
      const uint64_t payw = (hdr.size - hdr.off_payload) / 4;
      for (uint32_t g = 0; g < hdr.ngroups; ++g) {
        const SdbColGroupDescDev& gd = hdesc[g];
        if (gd.vmin < cmin) cmin = gd.vmin;
        if (gd.vmax > cmax) cmax = gd.vmax;
        const uint64_t glen =
          std::min<uint64_t>(rows, (uint64_t)(g + 1) * hdr.group_rows) -
          (uint64_t)g * hdr.group_rows;
        if (gd.width > 32 ||
            (gd.width && (gd.word_off > payw ||
                          (glen * gd.width + 31) / 32 > payw - gd.word_off)))
          return SDB_ERR_INVALID;
        if (gd.width > mw) mw = gd.width;
      }
      tab->max_w[c] = mw;
      tab->paywords[c] = payw;
      tab->col_min[c] = cmin;
      tab->col_max[c] = cmax;
      tab->has_minmax[c] = hdr.ngroups > 0;
    } else {
      const size_t esz = cols[c].type == SDB_COL_I64 ? 8 : 4;
      HIP_CHECK(hipMalloc(&tab->cols[c], esz * rows));
      HIP_CHECK(hipMemcpy(tab->cols[c], cols[c].data, esz * rows,
                          hipMemcpyHostToDevice));
      tab->refs[c].data = tab->cols[c];
      tab->refs[c].desc = nullptr;
      if (cols[c].type == SDB_COL_I64 && rows) {
        // one ~HBM-rate pass at load; makes the raw-key range provable
        DevBuf d_mm;
        HIP_CHECK(d_mm.alloc(16));
        const unsigned long long init[2] = {~0ull, 0ull};
        HIP_CHECK(hipMemcpy(d_mm.p, init, 16, hipMemcpyHostToDevice));
        const uint32_t nb =
          (uint32_t)std::min<uint64_t>(2048, (rows + 255) / 256);
        hipLaunchKernelGGL(col_minmax_kernel, dim3(nb), dim3(256), 0, 0,
                           (const long long*)tab->cols[c], rows,
                           d_mm.as<unsigned long long>());
        unsigned long long h_mm[2];
        HIP_CHECK(hipMemcpy(h_mm, d_mm.p, 16, hipMemcpyDeviceToHost));
        tab->col_min[c] = (int64_t)(h_mm[0] ^ 0x8000000000000000ull);
        tab->col_max[c] = (int64_t)(h_mm[1] ^ 0x8000000000000000ull);
        tab->has_minmax[c] = 1;
      }
    }
  }
  if (tab->group_rows == 0) tab->group_rows = 65536;  // raw-only tiling
  *out = hold.release();
  return SDB_OK;
}

int sdb_gpu_table_free(SdbGpuCtx* ctx, SdbGpuTable* tab) {
  if (!ctx || !tab) return SDB_ERR_INVALID;
  for (uint32_t c = 0; c < tab->ncols; ++c) {
    (void)hipFree(tab->cols[c]);
    if (tab->valid[c]) (void)hipFree(tab->valid[c]);
  }
  table_free_str(tab);
  delete tab;
  return SDB_OK;
}

int sdb_gpu_table_attach_validity(SdbGpuCtx* ctx, SdbGpuTable* tab,
                                  uint32_t col, const uint64_t* bits) {
  if (!ctx || !tab || col >= tab->ncols) return SDB_ERR_INVALID;
  tab->has_valid_minmax[col] = 0;  // the valid-rows range dies with the plane
  if (!bits) {
    if (tab->valid[col]) (void)hipFree(tab->valid[col]);
    tab->valid[col] = nullptr;
    return SDB_OK;
  }
  const uint64_t nwords = (tab->rows + 63) / 64;
  if (!tab->valid[col])
    HIP_CHECK(hipMalloc(&tab->valid[col], 8 * (nwords + 1)));
  HIP_CHECK(hipMemcpy(tab->valid[col], bits, 8 * nwords,
                      hipMemcpyHostToDevice));
  // synchronous for the same null-stream-ordering reason as the live
  // mask's pad word
  HIP_CHECK(hipMemset(tab->valid[col] + nwords, 0xFF, 8));
  return SDB_OK;
}

// ---- raw variable-width string columns (VERDICT r1 missing #5; the
// reference stores raw strings through its DuckDB fork's var-width
// vectors, column_reader.hpp:247-255 — parity at result level like the
// rest of the columnstore). Comparisons are memcmp order on unsigned
// bytes; predicates evaluate once into a row bitmask that scans consume
// through the existing validity-plane machinery (SDB_PRED_STRMASK). ----

int sdb_gpu_table_attach_strcol(SdbGpuCtx* ctx, SdbGpuTable* tab,
                                uint32_t slot, const uint64_t* offsets,
                                const uint8_t* blob, uint64_t blob_len) {
  if (!ctx || !tab || slot >= SDB_MAX_STRCOLS || !offsets ||
      (!blob && blob_len))
    return SDB_ERR_INVALID;
  // offsets must be monotone and span exactly the blob
  if (offsets[tab->rows] != blob_len) return SDB_ERR_INVALID;
  for (uint64_t r = 0; r < tab->rows; ++r)
    if (offsets[r] > offsets[r + 1]) return SDB_ERR_INVALID;
  if (tab->str_off[slot]) (void)hipFree(tab->str_off[slot]);
  if (tab->str_blob[slot]) (void)hipFree(tab->str_blob[slot]);
  if (tab->str_mask[slot]) (void)hipFree(tab->str_mask[slot]);
  tab->str_off[slot] = nullptr;
  tab->str_blob[slot] = nullptr;
  tab->str_mask[slot] = nullptr;
  tab->str_mask_set[slot] = 0;
  tab->str_fsst[slot] = 0;
  HIP_CHECK(hipMalloc(&tab->str_off[slot], 8 * (tab->rows + 1)));
  HIP_CHECK(hipMemcpy(tab->str_off[slot], offsets, 8 * (tab->rows + 1),
                      hipMemcpyHostToDevice));
  // the blob is padded to a multiple of 16 bytes (zero-filled): the
  // cooperative substring kernel reads it in aligned 16-byte vectors
  const uint64_t blob_pad = (blob_len + 16) & ~15ull;
  HIP_CHECK(hipMalloc(&tab->str_blob[slot], blob_pad));
  HIP_CHECK(hipMemset(tab->str_blob[slot] + (blob_pad - 16), 0, 16));
  if (blob_len)
    HIP_CHECK(hipMemcpy(tab->str_blob[slot], blob, blob_len,
                        hipMemcpyHostToDevice));
  tab->str_blob_len[slot] = blob_len;
  const uint64_t nwords = (tab->rows + 63) / 64;
  HIP_CHECK(hipMalloc(&tab->str_mask[slot], 8 * (nwords + 1)));
  return SDB_OK;
}

struct StrPredArgs {
  const uint64_t* off;
  const uint8_t* blob;
  uint64_t rows;
  unsigned long long* mask;
  uint32_t op;
  uint32_t lo_len, hi_len;
  uint32_t flags;  // SDB_STRPRED_*
  uint8_t lo[SDB_STRLIT_MAX + 1], hi[SDB_STRLIT_MAX + 1];
};

// The last step of every string-predicate kernel: one mask word per wave of
// 64 consecutive rows. wf = the row exists and is well formed; NEGATE
// inverts such rows only, so a malformed row and the bits at rows >= rows
// stay 0. The word replaces the slot's old one, or is AND-ed / OR-ed into it.
// With flags 0 this is the plain ballot store.
__device__ __forceinline__ void strmask_store(unsigned long long* mask,
                                              uint64_t r, bool wf, bool m,
                                              uint32_t flags) {
  const bool neg = (flags & SDB_STRPRED_NEGATE) != 0;
  unsigned long long w = __ballot(wf && (m != neg));
  if ((threadIdx.x & 63u) == 0) {
    if (flags & SDB_STRPRED_AND) w &= mask[r >> 6];
    else if (flags & SDB_STRPRED_OR) w |= mask[r >> 6];
    mask[r >> 6] = w;
  }
}

// lexicographic compare, memcmp order on unsigned bytes
__device__ __forceinline__ int str_cmp_dev(const uint8_t* s, uint32_t n,
                                           const uint8_t* t, uint32_t m) {
  const uint32_t k = n < m ? n : m;
  for (uint32_t i = 0; i < k; ++i)
    if (s[i] != t[i]) return s[i] < t[i] ? -1 : 1;
  return n < m ? -1 : (n > m ? 1 : 0);
}

__global__ void strpred_kernel(StrPredArgs a) {
  // 64 consecutive rows per wave so one __ballot builds each mask word
  const uint64_t rpad = (a.rows + 63) & ~63ull;
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
       r < rpad; r += stride) {
    bool m = false;
    if (r < a.rows) {
      const uint64_t o0 = a.off[r];
      const uint32_t len = (uint32_t)(a.off[r + 1] - o0);
      const uint8_t* sp = a.blob + o0;
      if (a.op == SDB_PRED_PREFIX) {
        m = len >= a.lo_len;
        for (uint32_t i = 0; m && i < a.lo_len; ++i) m = sp[i] == a.lo[i];
      } else {
        const int c = str_cmp_dev(sp, len, a.lo, a.lo_len);
        switch (a.op) {
          case SDB_PRED_LT: m = c < 0; break;
          case SDB_PRED_GE: m = c >= 0; break;
          case SDB_PRED_EQ: m = c == 0; break;
          case SDB_PRED_BETWEEN:
            m = c >= 0 && str_cmp_dev(sp, len, a.hi, a.hi_len) <= 0;
            break;
          default: break;
        }
      }
    }
    strmask_store(a.mask, r, r < a.rows, m, a.flags);
  }
}

struct StrPredFsstArgs {
  StrPredArgs base;
  uint32_t nsym;
  uint16_t symoff[256];
  uint8_t syms[2048];
};

// streaming comparator over the decoded byte stream: res 0 = equal so
// far, +-1 = decided by a byte inside the literal, 2 = row extends past
// an equal literal (row > literal). Final cmp derives at row end.
struct FsstCmp {
  int res;
  uint32_t pos;
};
__device__ __forceinline__ void fsst_feed(FsstCmp& st, uint8_t b,
                                          const uint8_t* lit,
                                          uint32_t litlen) {
  if (st.res) return;
  if (st.pos < litlen) {
    if (b != lit[st.pos]) st.res = b < lit[st.pos] ? -1 : 1;
    ++st.pos;
  } else {
    st.res = 2;
  }
}
__device__ __forceinline__ int fsst_final(const FsstCmp& st,
                                          uint32_t litlen) {
  if (st.res == 2) return 1;
  if (st.res) return st.res;
  return st.pos == litlen ? 0 : -1;  // proper prefix of literal => less
}

__global__ void strpred_fsst_kernel(StrPredFsstArgs fa) {
  __shared__ uint8_t ssym[2048];
  __shared__ uint16_t soff[256];
  for (uint32_t i = threadIdx.x; i < 2048; i += blockDim.x)
    ssym[i] = fa.syms[i];
  for (uint32_t i = threadIdx.x; i < 256; i += blockDim.x)
    soff[i] = fa.symoff[i];
  __syncthreads();
  const StrPredArgs a = fa.base;
  const uint64_t rpad = (a.rows + 63) & ~63ull;
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
       r < rpad; r += stride) {
    bool m = false;
    bool malformed = false;
    if (r < a.rows) {
      const uint64_t o0 = a.off[r], o1 = a.off[r + 1];
      FsstCmp clo{0, 0}, chi{0, 0};
      for (uint64_t i = o0; i < o1; ++i) {
        const uint8_t c = a.blob[i];
        if (c == 255u) {  // escape: next byte is a literal
          if (++i >= o1) { malformed = true; break; }
          fsst_feed(clo, a.blob[i], a.lo, a.lo_len);
          if (a.op == SDB_PRED_BETWEEN)
            fsst_feed(chi, a.blob[i], a.hi, a.hi_len);
        } else {
          if (c >= fa.nsym) { malformed = true; break; }
          for (uint32_t j = soff[c]; j < (uint32_t)soff[c + 1]; ++j) {
            fsst_feed(clo, ssym[j], a.lo, a.lo_len);
            if (a.op == SDB_PRED_BETWEEN)
              fsst_feed(chi, ssym[j], a.hi, a.hi_len);
          }
        }
      }
      if (!malformed) {
        const int cl = fsst_final(clo, a.lo_len);
        switch (a.op) {
          case SDB_PRED_LT: m = cl < 0; break;
          case SDB_PRED_GE: m = cl >= 0; break;
          case SDB_PRED_EQ: m = cl == 0; break;
          case SDB_PRED_BETWEEN:
            m = cl >= 0 && fsst_final(chi, a.hi_len) <= 0;
            break;
          case SDB_PRED_PREFIX:
            // prefix iff no mismatch INSIDE the literal and the decoded
            // row reached the literal's end
            m = clo.res == 2 || (clo.res == 0 && clo.pos == a.lo_len);
            break;
          default: break;
        }
      }
    }
    strmask_store(a.mask, r, r < a.rows && !malformed, m, a.flags);
  }
}

// ---- SUFFIX / CONTAINS / LIKE: the sdb_like.h program on the device ----
// The compiled pattern (2.2 KB, too large to ride beside the FSST symbol
// table in the kernel arguments) sits in device memory and is staged into
// LDS once per block.

struct StrLikeArgs {
  const uint64_t* off;
  const uint8_t* blob;
  uint64_t rows;
  unsigned long long* mask;
  const SdbLikeProg* prog;
  uint32_t flags;
};

static_assert(sizeof(SdbLikeProg) % 8 == 0, "staged as u64 words");
__device__ __forceinline__ void like_prog_stage(SdbLikeProg* dst,
                                                const SdbLikeProg* src) {
  const uint64_t* s = reinterpret_cast<const uint64_t*>(src);
  uint64_t* d = reinterpret_cast<uint64_t*>(dst);
  for (uint32_t i = threadIdx.x; i < sizeof(SdbLikeProg) / 8; i += blockDim.x)
    d[i] = s[i];
}

// row-wise automaton over a raw slot: one thread per row, any program
__global__ void strlike_kernel(StrLikeArgs a) {
  __shared__ SdbLikeProg sp;
  like_prog_stage(&sp, a.prog);
  __syncthreads();
  const uint64_t rpad = (a.rows + 63) & ~63ull;
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
       r < rpad; r += stride) {
    bool m = false;
    if (r < a.rows) {
      const uint64_t o0 = a.off[r], o1 = a.off[r + 1];
      SdbLikeState st;
      sdb_like_init(st);
      // a raw row is decided as soon as the anchored first segment died or
      // every segment matched with the end free
      for (uint64_t i = o0; i < o1 && !st.fail && st.seg < sp.nseg; ++i)
        sdb_like_feed(sp, st, a.blob[i]);
      m = sdb_like_finish(sp, st, o1 - o0);
    }
    strmask_store(a.mask, r, r < a.rows, m, a.flags);
  }
}

struct StrLikeFsstArgs {
  StrLikeArgs base;
  uint32_t nsym;
  uint16_t symoff[256];
  uint8_t syms[2048];
};

// the same over an FSST slot: decoded bytes go to the step one at a time.
// Every code of a row is read, so a malformed row is seen whatever the
// pattern decided before it.
__global__ void strlike_fsst_kernel(StrLikeFsstArgs fa) {
  __shared__ SdbLikeProg sp;
  __shared__ uint8_t ssym[2048];
  __shared__ uint16_t soff[256];
  like_prog_stage(&sp, fa.base.prog);
  for (uint32_t i = threadIdx.x; i < 2048; i += blockDim.x)
    ssym[i] = fa.syms[i];
  for (uint32_t i = threadIdx.x; i < 256; i += blockDim.x)
    soff[i] = fa.symoff[i];
  __syncthreads();
  const StrLikeArgs a = fa.base;
  const uint64_t rpad = (a.rows + 63) & ~63ull;
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
       r < rpad; r += stride) {
    bool m = false;
    bool malformed = false;
    if (r < a.rows) {
      const uint64_t o0 = a.off[r], o1 = a.off[r + 1];
      SdbLikeState st;
      sdb_like_init(st);
      for (uint64_t i = o0; i < o1; ++i) {
        const uint8_t c = a.blob[i];
        if (c == 255u) {  // escape: next byte is a literal
          if (++i >= o1) { malformed = true; break; }
          sdb_like_feed(sp, st, a.blob[i]);
        } else {
          if (c >= fa.nsym) { malformed = true; break; }
          for (uint32_t j = soff[c]; j < (uint32_t)soff[c + 1]; ++j)
            sdb_like_feed(sp, st, ssym[j]);
        }
      }
      if (!malformed) m = sdb_like_finish(sp, st, st.n);
    }
    strmask_store(a.mask, r, r < a.rows && !malformed, m, a.flags);
  }
}

// Cooperative substring kernel: raw slot, one unanchored segment of m >= 1
// bytes (CONTAINS, LIKE '%x%'). One wave (= one block) owns 64 consecutive
// rows, whose bytes are the contiguous span [off[r0], off[r0 + 64]) of the
// blob. It streams the span through LDS in STRLIKE_CHUNK-byte steps of
// aligned 16-byte loads, keeping the last STRLIKE_CARRY >= m - 1 bytes of
// a step in front of the next, so work follows the bytes and not the
// longest row of the wave. Each step tests the start positions whose LAST
// byte lies in the newly loaded bytes, so every position is tested once. A
// hit at blob position p belongs to the row found by binary search in the 65
// staged offsets, and counts only if p + m <= off[row + 1]: a match never
// straddles rows. Loads start at 16-byte multiples below the end of the
// span; the blob allocation is padded to a multiple of 16 bytes
// (sdb_gpu_table_attach_strcol), so none leaves it.
#define STRLIKE_CHUNK 4096u  // a power of two, at most 8192
#define STRLIKE_CARRY 64u

struct StrLikeCoopArgs {
  StrLikeArgs base;
  uint32_t m;
  uint8_t lit[64];
};

__global__ void __launch_bounds__(64) strlike_coop_kernel(StrLikeCoopArgs ca) {
  __shared__ uint4 sbuf4[(STRLIKE_CARRY + STRLIKE_CHUNK) / 16];
  __shared__ uint64_t soff[65];
  __shared__ unsigned long long sword;
  __shared__ uint8_t slit[64];
  uint8_t* sbuf = reinterpret_cast<uint8_t*>(sbuf4);
  const StrLikeArgs a = ca.base;
  const uint32_t lane = threadIdx.x;
  const uint32_t m = ca.m;
  slit[lane] = ca.lit[lane];
  const uint8_t l0 = ca.lit[0];
  const uint64_t nwin = (a.rows + 63) / 64;
  for (uint64_t w = blockIdx.x; w < nwin; w += gridDim.x) {
    const uint64_t r0 = w * 64;
    const uint32_t nr = a.rows - r0 < 64 ? (uint32_t)(a.rows - r0) : 64u;
    __syncthreads();  // the previous window is stored
    soff[lane] = a.off[r0 + (lane < nr ? lane : nr)];
    if (lane == 0) {
      soff[64] = a.off[r0 + nr];
      sword = 0;
    }
    __syncthreads();
    const uint64_t b0 = soff[0], b1 = soff[64];
    if (b1 - b0 >= m) {
      for (uint64_t cs = b0 & ~15ull; cs < b1; cs += STRLIKE_CHUNK) {
        // carry the tail of the last step over, then load this one; before
        // the first step the carried bytes lie below b0 and are never used
        const uint8_t carry = sbuf[STRLIKE_CHUNK + lane];
        __syncthreads();
        sbuf[lane] = carry;
        for (uint32_t v = lane; v < STRLIKE_CHUNK / 16; v += 64) {
          const uint64_t at = cs + (uint64_t)v * 16;
          if (at < b1)
            sbuf4[STRLIKE_CARRY / 16 + v] =
              *reinterpret_cast<const uint4*>(a.blob + at);
        }
        __syncthreads();
        // start position p = cs + j - (m - 1) sits at sbuf[i]; j runs over
        // b0 <= p and p + m <= b1, i.e. b0 + m - 1 <= cs + j < b1
        const uint32_t jlo =
          cs < b0 + (m - 1) ? (uint32_t)(b0 + (m - 1) - cs) : 0u;
        const uint32_t jhi =
          b1 - cs < STRLIKE_CHUNK ? (uint32_t)(b1 - cs) : STRLIKE_CHUNK;
        for (uint32_t j = jlo + lane; j < jhi; j += 64) {
          const uint32_t i = STRLIKE_CARRY - (m - 1) + j;
          if (sbuf[i] != l0) continue;
          bool hit = true;
          for (uint32_t k = 1; k < m && hit; ++k) hit = sbuf[i + k] == slit[k];
          if (!hit) continue;
          const uint64_t p = cs + j - (m - 1);
          uint32_t lo = 0, hi = nr;  // soff[lo] <= p < soff[hi]
          while (hi - lo > 1) {
            const uint32_t mid = (lo + hi) >> 1;
            if (soff[mid] <= p) lo = mid; else hi = mid;
          }
          if (p + m <= soff[lo + 1]) atomicOr(&sword, 1ull << lo);
        }
      }
    }
    __syncthreads();
    if (lane == 0) {
      unsigned long long wv = sword;
      if (a.flags & SDB_STRPRED_NEGATE)
        wv = ~wv & (nr == 64 ? ~0ull : (1ull << nr) - 1ull);
      if (a.flags & SDB_STRPRED_AND) wv &= a.mask[w];
      else if (a.flags & SDB_STRPRED_OR) wv |= a.mask[w];
      a.mask[w] = wv;
    }
  }
}

// flags and slot checks shared by the three entries, before any launch
static int strpred_check(const SdbGpuCtx* ctx, const SdbGpuTable* tab,
                         uint32_t slot, uint32_t flags) {
  if (!ctx || !tab || slot >= SDB_MAX_STRCOLS || !tab->str_off[slot])
    return SDB_ERR_INVALID;
  if (flags & ~(SDB_STRPRED_NEGATE | SDB_STRPRED_AND | SDB_STRPRED_OR))
    return SDB_ERR_INVALID;
  const uint32_t comb = flags & (SDB_STRPRED_AND | SDB_STRPRED_OR);
  if (comb == (SDB_STRPRED_AND | SDB_STRPRED_OR)) return SDB_ERR_INVALID;
  if (comb && !tab->str_mask_set[slot]) return SDB_ERR_INVALID;
  return SDB_OK;
}

static int strlike_run(SdbGpuCtx* ctx, SdbGpuTable* tab, uint32_t slot,
                       const SdbLikeProg& prog, uint32_t flags) {
  if (!tab->like_prog)
    HIP_CHECK(hipMalloc(&tab->like_prog, sizeof(SdbLikeProg)));
  HIP_CHECK(hipMemcpy(tab->like_prog, &prog, sizeof(prog),
                      hipMemcpyHostToDevice));
  StrLikeArgs a{};
  a.off = tab->str_off[slot];
  a.blob = tab->str_blob[slot];
  a.rows = tab->rows;
  a.mask = tab->str_mask[slot];
  a.prog = tab->like_prog;
  a.flags = flags;
  const uint32_t nb =
    (uint32_t)std::min<uint64_t>(4096, (tab->rows + 255) / 256);
  // the cooperative kernel takes the substring shape on a raw slot; the
  // SDB_LIKE_ROWWISE test hook (sdb_gpu.h) keeps it on the row-wise one
  bool coop = !tab->str_fsst[slot] && prog.nseg == 1 &&
              !prog.anchored_start && !prog.anchored_end;
  if (coop)
    if (const char* e = std::getenv("SDB_LIKE_ROWWISE"))
      if (std::strtoul(e, nullptr, 10) == 1) coop = false;
  if (tab->str_fsst[slot]) {
    StrLikeFsstArgs fa{};
    fa.base = a;
    fa.nsym = tab->str_nsym[slot];
    std::memcpy(fa.symoff, tab->str_symoff[slot], sizeof(fa.symoff));
    std::memcpy(fa.syms, tab->str_syms[slot], sizeof(fa.syms));
    hipLaunchKernelGGL(strlike_fsst_kernel, dim3(nb ? nb : 1), dim3(256), 0,
                       ctx->stream, fa);
  } else if (coop) {
    StrLikeCoopArgs ca{};
    ca.base = a;
    ca.m = prog.lit_len;
    std::memcpy(ca.lit, prog.lit, sizeof(ca.lit));
    const uint32_t nw =
      (uint32_t)std::min<uint64_t>(8192, (tab->rows + 63) / 64);
    hipLaunchKernelGGL(strlike_coop_kernel, dim3(nw ? nw : 1), dim3(64), 0,
                       ctx->stream, ca);
  } else {
    hipLaunchKernelGGL(strlike_kernel, dim3(nb ? nb : 1), dim3(256), 0,
                       ctx->stream, a);
  }
  HIP_CHECK(hipGetLastError());
  HIP_CHECK(hipStreamSynchronize(ctx->stream));
  tab->str_mask_set[slot] = 1;
  return SDB_OK;
}

int sdb_gpu_strpred_like(SdbGpuCtx* ctx, SdbGpuTable* tab, uint32_t slot,
                         const uint8_t* pattern, uint32_t pattern_len,
                         int32_t escape, uint32_t flags) {
  const int rc = strpred_check(ctx, tab, slot, flags);
  if (rc) return rc;
  SdbLikeProg prog;
  if (sdb_like_compile(pattern, pattern_len, escape, &prog))
    return SDB_ERR_INVALID;
  return strlike_run(ctx, tab, slot, prog, flags);
}

int sdb_gpu_strpred_mask(SdbGpuCtx* ctx, SdbGpuTable* tab, uint32_t slot,
                         SdbPredOp op, const uint8_t* lo, uint32_t lo_len,
                         const uint8_t* hi, uint32_t hi_len) {
  return sdb_gpu_strpred_mask_ex(ctx, tab, slot, op, lo, lo_len, hi, hi_len,
                                 0);
}

int sdb_gpu_strpred_mask_ex(SdbGpuCtx* ctx, SdbGpuTable* tab, uint32_t slot,
                            SdbPredOp op, const uint8_t* lo, uint32_t lo_len,
                            const uint8_t* hi, uint32_t hi_len,
                            uint32_t flags) {
  const int rc = strpred_check(ctx, tab, slot, flags);
  if (rc) return rc;
  if (op == SDB_PRED_SUFFIX || op == SDB_PRED_CONTAINS) {
    if (lo_len > SDB_STRLIT_MAX || (lo_len && !lo)) return SDB_ERR_INVALID;
    SdbLikeProg prog;
    if (sdb_like_literal(lo, lo_len, false, op == SDB_PRED_SUFFIX, &prog))
      return SDB_ERR_INVALID;
    return strlike_run(ctx, tab, slot, prog, flags);
  }
  if (op != SDB_PRED_LT && op != SDB_PRED_GE && op != SDB_PRED_BETWEEN &&
      op != SDB_PRED_EQ && op != SDB_PRED_PREFIX)
    return SDB_ERR_INVALID;
  if (lo_len > SDB_STRLIT_MAX || hi_len > SDB_STRLIT_MAX)
    return SDB_ERR_INVALID;
  if ((lo_len && !lo) || (hi_len && !hi)) return SDB_ERR_INVALID;
  if (op == SDB_PRED_BETWEEN && !hi && hi_len) return SDB_ERR_INVALID;
  StrPredArgs a{};
  a.flags = flags;
  a.off = tab->str_off[slot];
  a.blob = tab->str_blob[slot];
  a.rows = tab->rows;
  a.mask = tab->str_mask[slot];
  a.op = (uint32_t)op;
  a.lo_len = lo_len;
  a.hi_len = hi_len;
  if (lo_len) std::memcpy(a.lo, lo, lo_len);
  if (hi_len) std::memcpy(a.hi, hi, hi_len);
  const uint32_t nb =
    (uint32_t)std::min<uint64_t>(4096, (tab->rows + 255) / 256);
  if (tab->str_fsst[slot]) {
    StrPredFsstArgs fa{};
    std::memcpy(&fa.base, &a, sizeof(a));
    fa.nsym = tab->str_nsym[slot];
    std::memcpy(fa.symoff, tab->str_symoff[slot], sizeof(fa.symoff));
    std::memcpy(fa.syms, tab->str_syms[slot], sizeof(fa.syms));
    hipLaunchKernelGGL(strpred_fsst_kernel, dim3(nb ? nb : 1), dim3(256),
                       0, ctx->stream, fa);
  } else {
    hipLaunchKernelGGL(strpred_kernel, dim3(nb ? nb : 1), dim3(256), 0,
                       ctx->stream, a);
  }
  HIP_CHECK(hipGetLastError());
  HIP_CHECK(hipStreamSynchronize(ctx->stream));
  tab->str_mask_set[slot] = 1;
  return SDB_OK;
}

// FSST-style compressed string slot (second half of
// "dict/FSST-style"; the reference defers string codecs to its DuckDB
// fork's COMPRESSION_AUTO, column_writer.cpp:141-204 — parity at result
// level). Encoded rows expand deterministically, so predicates decode on
// the fly and never materialize the string.
int sdb_gpu_table_attach_strcol_fsst(SdbGpuCtx* ctx, SdbGpuTable* tab,
                                     uint32_t slot,
                                     const uint64_t* offsets,
                                     const uint8_t* enc_blob,
                                     uint64_t enc_len,
                                     const uint8_t* symbols,
                                     const uint32_t* sym_offsets,
                                     uint32_t nsym) {
  if (nsym > 254 || !sym_offsets || (!symbols && nsym))
    return SDB_ERR_INVALID;
  if (sym_offsets[nsym] > 2048) return SDB_ERR_INVALID;
  for (uint32_t i = 0; i < nsym; ++i) {
    const uint32_t l = sym_offsets[i + 1] - sym_offsets[i];
    if (sym_offsets[i] > sym_offsets[i + 1] || l == 0 || l > 8)
      return SDB_ERR_INVALID;
  }
  // escape codes must reference in-bounds literals: enforced by the
  // offsets-monotone check (an escape at a row end would make the row's
  // decode read past its span; validated at predicate time per row)
  const int rc = sdb_gpu_table_attach_strcol(ctx, tab, slot, offsets,
                                             enc_blob, enc_len);
  if (rc) return rc;
  tab->str_fsst[slot] = 1;
  tab->str_nsym[slot] = (uint16_t)nsym;
  std::memset(tab->str_symoff[slot], 0, sizeof(tab->str_symoff[slot]));
  std::memset(tab->str_syms[slot], 0, sizeof(tab->str_syms[slot]));
  for (uint32_t i = 0; i <= nsym; ++i)
    tab->str_symoff[slot][i] = (uint16_t)sym_offsets[i];
  if (nsym)
    std::memcpy(tab->str_syms[slot], symbols, sym_offsets[nsym]);
  return SDB_OK;
}

// Aggregate-list validation shared by every scan entry, run before anything
// is launched: op inside SdbAggOp, column inside the table for every op but
// COUNT(*), and the op's column type. *ext = the list holds an op >=
// SDB_AGG_COUNT_COL, which selects the EXT = 1 kernel instantiations.
static int agg_specs_check(const SdbGpuTable* tab, const SdbAggSpec* aggs,
                           uint32_t naggs, bool* ext) {
  if (!aggs) return SDB_ERR_INVALID;
  *ext = false;
  for (uint32_t q = 0; q < naggs; ++q) {
    const uint32_t op = (uint32_t)aggs[q].op;
    if (op > (uint32_t)SDB_AGG_MAX_F32) return SDB_ERR_INVALID;
    if (op == SDB_AGG_COUNT) continue;
    if (aggs[q].col >= tab->ncols) return SDB_ERR_INVALID;
    const bool f32 = tab->types[aggs[q].col] == SDB_COL_F32;
    switch (op) {
      case SDB_AGG_SUM_I64:
      case SDB_AGG_MIN_I64:
      case SDB_AGG_MAX_I64:
        if (f32) return SDB_ERR_INVALID;
        break;
      case SDB_AGG_SUM_F64:
      case SDB_AGG_MIN_F32:
      case SDB_AGG_MAX_F32:
        if (!f32) return SDB_ERR_INVALID;
        break;
      default: break;  // COUNT_COL: any column type
    }
    *ext |= op >= (uint32_t)SDB_AGG_COUNT_COL;
  }
  return SDB_OK;
}

// The pushed predicate list resolved against the table, for every scan entry
// and before anything is allocated or launched. A STRMASK predicate (.col is
// a string slot) becomes NOTNULL over the slot's precomputed row bitmask,
// consumed through the validity machinery: NOTNULL evaluates the plane alone,
// so strmask_col, the column it nominally rides on, is never read — the
// aggregate entries pass their (already resident) group key, top-n none.
static int preds_resolve(PredSet& ps, const SdbGpuTable* tab,
                         const SdbPredSpec* preds, uint32_t npreds,
                         ColRef strmask_col) {
  if (npreds > SCAN_MAX_PREDS || (npreds && !preds)) return SDB_ERR_INVALID;
  for (uint32_t p = 0; p < npreds; ++p) {
    if (preds[p].op == SDB_PRED_STRMASK) {
      const uint32_t slot = preds[p].col;
      if (slot >= SDB_MAX_STRCOLS || !tab->str_mask_set[slot])
        return SDB_ERR_INVALID;
      ps.col[p] = strmask_col;
      ps.op[p] = SDB_PRED_NOTNULL;
      ps.isf32[p] = 0;
      ps.valid[p] = tab->str_mask[slot];
      continue;
    }
    if (preds[p].col >= tab->ncols) return SDB_ERR_INVALID;
    if (preds[p].op < SDB_PRED_LT || preds[p].op > SDB_PRED_NOTNULL)
      return SDB_ERR_INVALID;
    ps.col[p] = tab->refs[preds[p].col];
    ps.op[p] = preds[p].op;
    ps.isf32[p] = tab->types[preds[p].col] == SDB_COL_F32 ? 1 : 0;
    ps.lo[p] = preds[p].ilo;
    ps.hi[p] = preds[p].ihi;
    ps.flo[p] = preds[p].flo;
    ps.fhi[p] = preds[p].fhi;
    ps.valid[p] = tab->valid[preds[p].col];
  }
  return SDB_OK;
}

// the aggregate list (agg_specs_check has passed) into the three parallel
// arrays of a kernel-argument struct: COUNT(*) reads no column and no plane
static void aggs_resolve(ColRef* agg_col, int* agg_op,
                         const unsigned long long** agg_valid,
                         const SdbGpuTable* tab, const SdbAggSpec* aggs,
                         uint32_t naggs) {
  for (uint32_t q = 0; q < naggs; ++q) {
    const bool star = aggs[q].op == SDB_AGG_COUNT;
    agg_op[q] = aggs[q].op;
    agg_col[q] = star ? ColRef{nullptr, nullptr} : tab->refs[aggs[q].col];
    agg_valid[q] = star ? nullptr : tab->valid[aggs[q].col];
  }
}

// grid of every row-group walker: a workgroup per row group, grid-strided
// past SCAN_MAXB, never empty
static uint32_t scan_nblocks(const SdbGpuTable* tab) {
  const uint64_t n = (tab->rows + tab->group_rows - 1) / tab->group_rows;
  return (uint32_t)std::min<uint64_t>(std::max<uint64_t>(n, 1), SCAN_MAXB);
}

// Sizing of a hash aggregate's two tables; slot_words = 8-byte words a slot
// holds beside its key. Global: pow2 capacity >= 2*max_groups (load factor
// <= 0.5). LDS: the largest pow2 slot count that fits. When the distinct-key
// bound dwarfs the LDS table, nearly every row would burn a full probe chain
// before falling through to the global table anyway (measured 3.3G rows/s at
// 100k groups vs 67.9G dense): then LDS staging is off (*lds_slots = 0) and
// rows upsert straight into the global table.
static void hash_table_sizes(uint64_t max_groups, uint32_t slot_words,
                             uint64_t* cap, uint32_t* lds_slots) {
  *cap = 64;
  while (*cap < 2 * max_groups) *cap <<= 1;
  uint32_t slots = 1u << 14;
  while (slots && (uint64_t)slots * 8 * (1 + slot_words) > 150 * 1024)
    slots >>= 1;
  if (max_groups > (uint64_t)slots * 2) slots = 0;
  *lds_slots = slots;
}

// device accumulator -> SdbAggResult. MIN/MAX slots hold "bigger wins"
// codes (see agg_row); code 0 is the identity: INT64_MAX / INT64_MIN fall
// out of the i64 decode, +inf / -inf are mapped here.
static void agg_decode(int op, unsigned long long raw, SdbAggResult* r) {
  r->i64 = 0;
  r->f64 = 0;
  switch (op) {
    case SDB_AGG_SUM_F64:
      std::memcpy(&r->f64, &raw, 8);
      break;
    case SDB_AGG_MIN_I64:
      r->i64 = (int64_t)(~raw ^ SDB_I64_SIGN);
      break;
    case SDB_AGG_MAX_I64:
      r->i64 = (int64_t)(raw ^ SDB_I64_SIGN);
      break;
    case SDB_AGG_MIN_F32:
    case SDB_AGG_MAX_F32: {
      const bool is_min = op == SDB_AGG_MIN_F32;
      uint32_t bits = is_min ? 0x7F800000u : 0xFF800000u;  // +inf / -inf
      if (raw) {
        const uint32_t key = is_min ? ~(uint32_t)raw : (uint32_t)raw;
        bits = (key & 0x80000000u) ? key ^ 0x80000000u : ~key;
      }
      float f;
      std::memcpy(&f, &bits, 4);
      r->f64 = (double)f;  // exact; keeps the sign of zero
      break;
    }
    default:
      r->i64 = (int64_t)raw;
      break;
  }
}

// The range of column col over the valid rows of its attached plane, cached
// on the table: one reduction per attached plane (attach_validity drops it),
// so a nullable-key scan in steady state runs no extra pass and allocates
// nothing.
static int valid_minmax(SdbGpuCtx* ctx, SdbGpuTable* tab, uint32_t col) {
  if (tab->has_valid_minmax[col]) return SDB_OK;
  DevBuf d_mm;
  HIP_CHECK(d_mm.alloc(16));
  const unsigned long long init[2] = {~0ull, 0ull};
  unsigned long long h_mm[2] = {~0ull, 0ull};
  HIP_CHECK(hipMemcpy(d_mm.p, init, 16, hipMemcpyHostToDevice));
  if (tab->rows) {
    const uint32_t nb =
      (uint32_t)std::min<uint64_t>(2048, (tab->rows + 255) / 256);
    hipLaunchKernelGGL(col_minmax_valid_kernel, dim3(nb), dim3(256), 0,
                       ctx->stream, tab->refs[col], tab->valid[col],
                       tab->rows, tab->group_rows,
                       d_mm.as<unsigned long long>());
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipStreamSynchronize(ctx->stream));
  }
  HIP_CHECK(hipMemcpy(h_mm, d_mm.p, 16, hipMemcpyDeviceToHost));
  tab->valid_min[col] = (int64_t)(h_mm[0] ^ 0x8000000000000000ull);
  tab->valid_max[col] = (int64_t)(h_mm[1] ^ 0x8000000000000000ull);
  tab->has_valid_minmax[col] = 1;
  return SDB_OK;
}

// Dense scan shared by sdb_gpu_scan_agg (null_rows == nullptr: out holds
// ngroups rows and a key plane is rejected) and sdb_gpu_scan_agg_nullkey
// (out holds ngroups + 1 rows, the last one the NULL group).
static int scan_agg_dense(SdbGpuCtx* ctx, SdbGpuTable* tab,
                          uint32_t group_col, uint32_t ngroups,
                          const SdbPredSpec* preds, uint32_t npreds,
                          const SdbAggSpec* aggs, uint32_t naggs,
                          SdbAggResult* out, uint64_t* rows_passed,
                          uint64_t* null_rows) {
  if (!ctx || !tab || !out || !rows_passed || group_col >= tab->ncols ||
      ngroups == 0 || ngroups > SCAN_MAX_GROUPS || naggs == 0 ||
      naggs > SCAN_MAX_AGGS)
    return SDB_ERR_INVALID;
  bool ext = false;
  if (agg_specs_check(tab, aggs, naggs, &ext)) return SDB_ERR_INVALID;
  if (tab->types[group_col] == SDB_COL_F32) return SDB_ERR_INVALID;
  if (!null_rows && tab->valid[group_col])
    return SDB_ERR_INVALID;  // NULL groups: sdb_gpu_scan_agg_nullkey
  ScanArgsNK a{};  // the NK = 0 launches take its ScanArgs base
  a.keys = tab->refs[group_col];
  if (preds_resolve(a.ps, tab, preds, npreds, a.keys)) return SDB_ERR_INVALID;
  // nk: the NK = 1 instantiations run, with the NULL group as accumulator
  // row ngroups. Without a key plane the nullable entry launches exactly
  // what sdb_gpu_scan_agg launches and its NULL row decodes from zeros.
  const bool nk = null_rows && tab->valid[group_col];
  // dense-key contract: keys must be provably inside [0, ngroups) or the
  // perfect-hash accumulate acc[key*naggs+q] corrupts LDS. Both column
  // kinds carry a load-time range (FoR zonemaps / raw-column reduction).
  // Under a key plane the contract binds the valid rows alone, and the
  // range is taken over them (valid_minmax); no valid row proves trivially.
  if (nk) {
    const int rc = valid_minmax(ctx, tab, group_col);
    if (rc) return rc;
    if (tab->valid_min[group_col] <= tab->valid_max[group_col] &&
        (tab->valid_min[group_col] < 0 ||
         tab->valid_max[group_col] >= (int64_t)ngroups))
      return SDB_ERR_INVALID;
  } else if (tab->rows && tab->has_minmax[group_col] &&
             (tab->col_min[group_col] < 0 ||
              tab->col_max[group_col] >= (int64_t)ngroups))
    return SDB_ERR_INVALID;

  hipStream_t stream = ctx->stream;

  a.key_valid = nk ? tab->valid[group_col] : nullptr;
  a.rows = tab->rows;
  a.group_rows = tab->group_rows;
  a.ngroups = ngroups;
  a.naggs = naggs;
  a.npreds = npreds;
  // the table column whose values predicate p decodes: its own, or the group
  // key for a mask predicate, the one op past NOTNULL that preds_resolve lets
  // through (its .col is a string slot, no column)
  uint32_t pcol[SCAN_MAX_PREDS];
  for (uint32_t p = 0; p < npreds; ++p)
    pcol[p] = preds[p].op > SDB_PRED_NOTNULL ? group_col : preds[p].col;
  aggs_resolve(a.agg_col, a.agg_op, a.agg_valid, tab, aggs, naggs);
  for (uint32_t q = 0; q < naggs; ++q) {
    a.agg_src[q] = 0;
    if (aggs[q].op == SDB_AGG_SUM_I64 || aggs[q].op == SDB_AGG_MIN_I64 ||
        aggs[q].op == SDB_AGG_MAX_I64) {
      if (aggs[q].col == group_col) a.agg_src[q] = 9;
      for (uint32_t p = 0; p < npreds; ++p)
        if (aggs[q].col == pcol[p]) a.agg_src[q] = 1 + (int)p;
    }
  }
  // accumulator slots in LDS and in d_out; the staged-chunk sizing below
  // works from this, i.e. from the table enlarged by the NULL row
  const uint32_t nslots = (ngroups + (nk ? 1u : 0u)) * naggs;
  // ctx-cached workspace: the dense scan hot path allocates nothing per
  // call (grown on demand; buffers owned and freed by the context)
  if (ctx->scan_out_cap < nslots) {
    if (ctx->d_scan_out) (void)hipFree(ctx->d_scan_out);
    ctx->d_scan_out = nullptr;
    ctx->scan_out_cap = 0;
    HIP_CHECK(hipMalloc(&ctx->d_scan_out, 8ull * nslots));
    ctx->scan_out_cap = nslots;
  }
  if (!ctx->d_scan_passed)  // [0] rows passed, [1] NULL-key rows passed
    HIP_CHECK(hipMalloc(&ctx->d_scan_passed, 16));
  unsigned long long* d_out = ctx->d_scan_out;
  unsigned long long* d_passed = ctx->d_scan_passed;
  HIP_CHECK(hipMemsetAsync(d_out, 0, 8ull * nslots, stream));
  HIP_CHECK(hipMemsetAsync(d_passed, 0, 16, stream));
  a.out = d_out;
  a.rows_passed = d_passed;
  a.null_rows = d_passed + 1;

  const uint32_t nblocks = scan_nblocks(tab);
  size_t lds = 8ull * nslots;
  bool any_for = a.keys.desc != nullptr;
  for (uint32_t p = 0; p < npreds; ++p) any_for |= a.ps.col[p].desc != nullptr;
  for (uint32_t q = 0; q < naggs; ++q) any_for |= a.agg_col[q].desc != nullptr;

  // staged-FoR eligibility: distinct FoR columns among {keys, pred0, pred1}
  // get LDS chunk staging; the chunk is shrunk until acc + stage buffers fit
  // the 160 KB LDS. SDB_SCAN_NOSTAGE falls back to the unstaged walker.
  uint32_t st_col[3];
  a.nstage = 0;
  a.key_st = -1;
  a.pred_st[0] = a.pred_st[1] = -1;
  auto add_stage = [&](uint32_t col) -> int {
    if (!tab->refs[col].desc) return -1;
    for (uint32_t s = 0; s < a.nstage; ++s)
      if (st_col[s] == col) return (int)s;
    st_col[a.nstage] = col;
    return (int)a.nstage++;
  };
  a.key_st = add_stage(group_col);
  for (uint32_t p = 0; p < npreds && p < 2; ++p)
    a.pred_st[p] = add_stage(pcol[p]);
  bool staged = any_for && a.nstage > 0 && !getenv("SDB_SCAN_NOSTAGE");
  if (staged) {
    uint32_t C = 8192;  // rows per chunk; multiple of 32 (word alignment)
    size_t ldsb = 0;
    for (;;) {
      ldsb = (8ull * nslots + 15) & ~15ull;
      for (uint32_t s = 0; s < a.nstage; ++s) {
        a.st_lds_off[s] = (uint32_t)(ldsb / 4);
        const uint64_t capw = (uint64_t)C * tab->max_w[st_col[s]] / 32 + 4;
        ldsb = (ldsb + 4 * capw + 15) & ~15ull;
      }
      if (ldsb <= 160 * 1024 || C <= 1024) break;
      C >>= 1;
    }
    if (ldsb > 160 * 1024) {
      staged = false;  // huge group table: unstaged walker
    } else {
      a.chunk_rows = C;
      for (uint32_t s = 0; s < a.nstage; ++s) {
        a.st_desc[s] = tab->refs[st_col[s]].desc;
        a.st_pay[s] = (const uint32_t*)tab->refs[st_col[s]].data;
        a.st_paywords[s] = tab->paywords[st_col[s]];
      }
      a.f32_pay = nullptr;
      if (!getenv("SDB_SCAN_NOF32STAGE") &&
          ldsb + 4ull * C + 16 <= 160 * 1024) {
        for (uint32_t q = 0; q < naggs; ++q) {
          if ((a.agg_op[q] == SDB_AGG_SUM_F64 ||
               a.agg_op[q] == SDB_AGG_MIN_F32 ||
               a.agg_op[q] == SDB_AGG_MAX_F32) &&
              !a.agg_col[q].desc) {
            a.f32_pay = (const float*)a.agg_col[q].data;
            a.f32_lds_off = (uint32_t)(ldsb / 4);
            ldsb = (ldsb + 4ull * C + 15) & ~15ull;
            break;
          }
        }
      }
      lds = ldsb;
    }
  }

  // compile-time agg-shape dispatch: the common [COUNT, SUM_I64,
  // SUM_F64] shape gets the straight-lined FoR accumulate bodies
  const bool shape3 = naggs == 3 && aggs[0].op == SDB_AGG_COUNT &&
                      aggs[1].op == SDB_AGG_SUM_I64 &&
                      aggs[2].op == SDB_AGG_SUM_F64 &&
                      !getenv("SDB_SCAN_NOSHAPE");
  // The last template argument (EXT) is set only when the list holds an op
  // >= SDB_AGG_COUNT_COL: lists of the three original ops launch
  // instantiations whose per-row switch has no arm for the new ones (a
  // shape3 list never has one, so ASHAPE = 1 exists with EXT = 0 only).
  // A key plane (nk) launches the NK = 1 instantiations, which exist for
  // ASHAPE = 0, EXT = 1 only — EXT = 1 handles every op, the old three
  // included: one each for staged, FoR and raw.
  if (nk && staged)
    hipLaunchKernelGGL((scan_agg_staged_kernel<0, 1, 1>), dim3(nblocks),
                       dim3(SCAN_NTHREADS), lds, stream, a);
  else if (nk && any_for)
    hipLaunchKernelGGL((scan_agg_kernel<0, 0, 1, 1>), dim3(nblocks),
                       dim3(SCAN_NTHREADS), lds, stream, a);
  else if (nk)
    hipLaunchKernelGGL((scan_agg_kernel<1, 0, 1, 1>), dim3(nblocks),
                       dim3(SCAN_NTHREADS), lds, stream, a);
  else if (staged && shape3)
    hipLaunchKernelGGL((scan_agg_staged_kernel<1, 0>), dim3(nblocks),
                       dim3(SCAN_NTHREADS), lds, stream, a);
  else if (staged && ext)
    hipLaunchKernelGGL((scan_agg_staged_kernel<0, 1>), dim3(nblocks),
                       dim3(SCAN_NTHREADS), lds, stream, a);
  else if (staged)
    hipLaunchKernelGGL((scan_agg_staged_kernel<0, 0>), dim3(nblocks),
                       dim3(SCAN_NTHREADS), lds, stream, a);
  else if (any_for && shape3)
    hipLaunchKernelGGL((scan_agg_kernel<0, 1, 0>), dim3(nblocks),
                       dim3(SCAN_NTHREADS), lds, stream, a);
  else if (any_for && ext)
    hipLaunchKernelGGL((scan_agg_kernel<0, 0, 1>), dim3(nblocks),
                       dim3(SCAN_NTHREADS), lds, stream, a);
  else if (any_for)
    hipLaunchKernelGGL((scan_agg_kernel<0, 0, 0>), dim3(nblocks),
                       dim3(SCAN_NTHREADS), lds, stream, a);
  else if (ext)
    hipLaunchKernelGGL((scan_agg_kernel<1, 0, 1>), dim3(nblocks),
                       dim3(SCAN_NTHREADS), lds, stream, a);
  else
    // RAW stays generic: the straight-lined 3-agg arm measured 183G vs
    // 234G rows/s on the same box (r2_raw_shape_ab.log) — the runtime
    // agg loop bounds the e-unroll better there; only the
    // instruction-bound FoR walkers keep ASHAPE=1
    hipLaunchKernelGGL((scan_agg_kernel<1, 0, 0>), dim3(nblocks),
                       dim3(SCAN_NTHREADS), lds, stream, a);
  HIP_CHECK(hipGetLastError());
  std::vector<unsigned long long> h_out(nslots);
  unsigned long long h_passed[2] = {0, 0};
  HIP_CHECK(hipMemcpyAsync(h_out.data(), d_out, 8ull * nslots,
                           hipMemcpyDeviceToHost, stream));
  HIP_CHECK(hipMemcpyAsync(h_passed, d_passed, 16, hipMemcpyDeviceToHost,
                           stream));
  HIP_CHECK(hipStreamSynchronize(stream));
  // d_out/d_passed are ctx-cached; freed with the context
  for (uint32_t g = 0; g < ngroups; ++g) {
    for (uint32_t q = 0; q < naggs; ++q)
      agg_decode(aggs[q].op, h_out[g * naggs + q], &out[g * naggs + q]);
  }
  if (null_rows) {  // row ngroups: the NULL group (zeros without a plane)
    for (uint32_t q = 0; q < naggs; ++q)
      agg_decode(aggs[q].op, nk ? h_out[ngroups * naggs + q] : 0ull,
                 &out[ngroups * naggs + q]);
    *null_rows = nk ? h_passed[1] : 0;
  }
  *rows_passed = h_passed[0];
  return SDB_OK;
}

int sdb_gpu_scan_agg(SdbGpuCtx* ctx, SdbGpuTable* tab, uint32_t group_col,
                     uint32_t ngroups, const SdbPredSpec* preds,
                     uint32_t npreds, const SdbAggSpec* aggs, uint32_t naggs,
                     SdbAggResult* out, uint64_t* rows_passed) {
  return scan_agg_dense(ctx, tab, group_col, ngroups, preds, npreds, aggs,
                        naggs, out, rows_passed, nullptr);
}

int sdb_gpu_scan_agg_nullkey(SdbGpuCtx* ctx, SdbGpuTable* tab,
                             uint32_t group_col, uint32_t ngroups,
                             const SdbPredSpec* preds, uint32_t npreds,
                             const SdbAggSpec* aggs, uint32_t naggs,
                             SdbAggResult* out, uint64_t* rows_passed,
                             uint64_t* null_rows) {
  if (!null_rows) return SDB_ERR_INVALID;
  return scan_agg_dense(ctx, tab, group_col, ngroups, preds, npreds, aggs,
                        naggs, out, rows_passed, null_rows);
}


// The scan description every hash-aggregate kernel shares: the predicate
// and aggregate lists resolved against the table. gkeys is the value column a
// STRMASK predicate rides on. Run before anything is allocated or launched.
static int hash_args_fill(HashAggArgs& a, const SdbGpuTable* tab,
                          ColRef gkeys, const SdbPredSpec* preds,
                          uint32_t npreds, const SdbAggSpec* aggs,
                          uint32_t naggs) {
  a.keys = gkeys;
  a.rows = tab->rows;
  a.group_rows = tab->group_rows;
  a.naggs = naggs;
  a.npreds = npreds;
  aggs_resolve(a.agg_col, a.agg_op, a.agg_valid, tab, aggs, naggs);
  return preds_resolve(a.ps, tab, preds, npreds, gkeys);
}

// core shared by the i64-key entry and the string-key entry: gkeys is
// the group-key column (a table column or a derived device array)
static int scan_agg_hash_core(SdbGpuCtx* ctx, SdbGpuTable* tab,
                              ColRef gkeys, uint64_t max_groups,
                              const SdbPredSpec* preds, uint32_t npreds,
                              const SdbAggSpec* aggs, uint32_t naggs,
                              int64_t* keys_out, SdbAggResult* out,
                              uint64_t* ngroups_out,
                              uint64_t* rows_passed,
                              const unsigned long long* key_valid = nullptr,
                              SdbAggResult* null_out = nullptr,
                              uint64_t* null_rows = nullptr) {
  // key_valid: the key column's own plane (sdb_gpu_scan_agg_hash_nullkey
  // only): launches the NK = 1 instantiation and fills null_out/null_rows
  if (!ctx || !tab || !keys_out || !out || !ngroups_out || !rows_passed ||
      max_groups == 0 || max_groups > (1u << 22) || naggs == 0 ||
      naggs > SCAN_MAX_AGGS)
    return SDB_ERR_INVALID;
  bool ext = false;
  if (agg_specs_check(tab, aggs, naggs, &ext)) return SDB_ERR_INVALID;

  hipStream_t stream = ctx->stream;
  HashAggArgsNK a{};  // the NK = 0 launches take its HashAggArgs base
  if (hash_args_fill(a, tab, gkeys, preds, npreds, aggs, naggs))
    return SDB_ERR_INVALID;
  uint64_t cap;  // a slot holds its key and naggs accumulators
  hash_table_sizes(max_groups, naggs, &cap, &a.lds_slots);
  a.gcap_mask = (uint32_t)(cap - 1);
  a.max_groups = (uint32_t)max_groups;
  a.key_valid = key_valid;
  // NK = 1 keeps the workgroup's NULL-group accumulators past the table
  const size_t lds = std::max<size_t>(
    (size_t)a.lds_slots * 8 * (1 + naggs) + (key_valid ? 8 * naggs : 0), 16);

  // d_misc: [0]=inserts|overflow, then neg_acc[naggs+1], rows_passed,
  // null_acc[naggs+1]
  const size_t misc_words = 1 + (naggs + 1) + 1 + (naggs + 1);
  DevBuf b_keys, b_acc, b_misc;
  HIP_CHECK(b_keys.alloc(cap * 8));
  HIP_CHECK(b_acc.alloc(cap * 8 * naggs));
  HIP_CHECK(b_misc.alloc(misc_words * 8));
  unsigned long long* d_keys = b_keys.as<unsigned long long>();
  unsigned long long* d_acc = b_acc.as<unsigned long long>();
  unsigned long long* d_misc = b_misc.as<unsigned long long>();
  HIP_CHECK(hipMemsetAsync(d_keys, 0xFF, cap * 8, stream));
  HIP_CHECK(hipMemsetAsync(d_acc, 0, cap * 8 * naggs, stream));
  HIP_CHECK(hipMemsetAsync(d_misc, 0, misc_words * 8, stream));
  a.gkeys = d_keys;
  a.gacc = d_acc;
  a.ginserts = (uint32_t*)d_misc;
  a.goverflow = (uint32_t*)d_misc + 1;
  a.neg_acc = d_misc + 1;
  a.rows_passed = d_misc + 1 + (naggs + 1);
  a.null_acc = d_misc + 1 + (naggs + 1) + 1;

  const uint32_t nblocks = scan_nblocks(tab);
  if (key_valid)  // the one NK = 1 instantiation: EXT = 1 handles every op
    hipLaunchKernelGGL((scan_agg_hash_kernel<1, 1>), dim3(nblocks),
                       dim3(SCAN_NTHREADS), lds, stream, a);
  else if (ext)  // as in sdb_gpu_scan_agg: old-op lists keep the old switch
    hipLaunchKernelGGL((scan_agg_hash_kernel<1>), dim3(nblocks),
                       dim3(SCAN_NTHREADS), lds, stream, a);
  else
    hipLaunchKernelGGL((scan_agg_hash_kernel<0>), dim3(nblocks),
                       dim3(SCAN_NTHREADS), lds, stream, a);
  HIP_CHECK(hipGetLastError());

  // sized while the kernel runs
  std::vector<unsigned long long> h_keys(cap);
  std::vector<unsigned long long> h_acc(cap * naggs);
  std::vector<unsigned long long> h_misc(misc_words);
  HIP_CHECK(hipMemcpyAsync(h_keys.data(), d_keys, cap * 8,
                           hipMemcpyDeviceToHost, stream));
  HIP_CHECK(hipMemcpyAsync(h_acc.data(), d_acc, cap * 8 * naggs,
                           hipMemcpyDeviceToHost, stream));
  HIP_CHECK(hipMemcpyAsync(h_misc.data(), d_misc, misc_words * 8,
                           hipMemcpyDeviceToHost, stream));
  HIP_CHECK(hipStreamSynchronize(stream));

  const uint32_t inserts = (uint32_t)(h_misc[0] & 0xFFFFFFFFu);
  const uint32_t overflow = (uint32_t)(h_misc[0] >> 32);
  const bool neg_present = h_misc[1 + naggs] != 0;
  const uint64_t distinct = (uint64_t)inserts + (neg_present ? 1 : 0);
  if (overflow || distinct > max_groups) return SDB_ERR_OOM;

  // compact + sort by key ascending (deterministic result order)
  std::vector<uint32_t> live;
  live.reserve(inserts);
  for (uint64_t i = 0; i < cap; ++i)
    if (h_keys[i] != SDB_HKEY_EMPTY) live.push_back((uint32_t)i);
  std::sort(live.begin(), live.end(), [&](uint32_t x, uint32_t y) {
    return (int64_t)h_keys[x] < (int64_t)h_keys[y];
  });
  uint64_t n = 0;
  auto emit = [&](int64_t key, const unsigned long long* acc) {
    keys_out[n] = key;
    for (uint32_t q = 0; q < naggs; ++q)
      agg_decode(aggs[q].op, acc[q], &out[n * naggs + q]);
    ++n;
  };
  // negative keys sort before -1? No: -1 is the LARGEST negative value,
  // so emit live keys < -1 first, then -1, then the rest.
  size_t li = 0;
  while (li < live.size() && (int64_t)h_keys[live[li]] < -1)
    emit((int64_t)h_keys[live[li]], &h_acc[(uint64_t)live[li] * naggs]),
      ++li;
  if (neg_present) emit(-1, &h_misc[1]);
  for (; li < live.size(); ++li)
    emit((int64_t)h_keys[live[li]], &h_acc[(uint64_t)live[li] * naggs]);
  *ngroups_out = n;
  *rows_passed = h_misc[1 + naggs + 1];
  // the NULL group: outside the key groups, no share of max_groups; all
  // zeros (identities once decoded) when no NULL-key row passed
  if (null_out)
    for (uint32_t q = 0; q < naggs; ++q)
      agg_decode(aggs[q].op, h_misc[1 + (naggs + 1) + 1 + q], &null_out[q]);
  if (null_rows) *null_rows = h_misc[1 + (naggs + 1) + 1 + naggs];
  return SDB_OK;
}

int sdb_gpu_scan_agg_hash(SdbGpuCtx* ctx, SdbGpuTable* tab,
                          uint32_t group_col, uint64_t max_groups,
                          const SdbPredSpec* preds, uint32_t npreds,
                          const SdbAggSpec* aggs, uint32_t naggs,
                          int64_t* keys_out, SdbAggResult* out,
                          uint64_t* ngroups_out, uint64_t* rows_passed) {
  if (!ctx || !tab || group_col >= tab->ncols) return SDB_ERR_INVALID;
  if (tab->types[group_col] == SDB_COL_F32) return SDB_ERR_INVALID;
  if (tab->valid[group_col])
    return SDB_ERR_INVALID;  // NULL groups: sdb_gpu_scan_agg_hash_nullkey
  return scan_agg_hash_core(ctx, tab, tab->refs[group_col], max_groups,
                            preds, npreds, aggs, naggs, keys_out, out,
                            ngroups_out, rows_passed);
}

int sdb_gpu_scan_agg_hash_nullkey(SdbGpuCtx* ctx, SdbGpuTable* tab,
                                  uint32_t group_col, uint64_t max_groups,
                                  const SdbPredSpec* preds, uint32_t npreds,
                                  const SdbAggSpec* aggs, uint32_t naggs,
                                  int64_t* keys_out, SdbAggResult* out,
                                  uint64_t* ngroups_out,
                                  uint64_t* rows_passed,
                                  SdbAggResult* null_out,
                                  uint64_t* null_rows) {
  if (!ctx || !tab || group_col >= tab->ncols || !null_out || !null_rows)
    return SDB_ERR_INVALID;
  if (tab->types[group_col] == SDB_COL_F32) return SDB_ERR_INVALID;
  // no plane: key_valid is null and the old instantiations run
  return scan_agg_hash_core(ctx, tab, tab->refs[group_col], max_groups,
                            preds, npreds, aggs, naggs, keys_out, out,
                            ngroups_out, rows_passed, tab->valid[group_col],
                            null_out, null_rows);
}

// GROUP BY 1..SDB_MAX_GROUP_KEYS nullable i64 columns (include/sdb_gpu.h;
// the scheme is described at scan_agg_hash_multi_kernel). One scan per seed;
// the host proves every slot from its witness words before it returns one.
int sdb_gpu_scan_agg_hash_multi(SdbGpuCtx* ctx, SdbGpuTable* tab,
                                const uint32_t* group_cols, uint32_t nkeys,
                                uint64_t max_groups,
                                const SdbPredSpec* preds, uint32_t npreds,
                                const SdbAggSpec* aggs, uint32_t naggs,
                                int64_t* keys_out, uint32_t* keynull_out,
                                SdbAggResult* out, uint64_t* ngroups_out,
                                uint64_t* rows_passed) {
  if (!ctx || !tab || !group_cols || !keys_out || !keynull_out || !out ||
      !ngroups_out || !rows_passed || nkeys == 0 ||
      nkeys > SDB_MAX_GROUP_KEYS || max_groups == 0 ||
      max_groups > (1u << 22) || naggs == 0 || naggs > SCAN_MAX_AGGS)
    return SDB_ERR_INVALID;
  for (uint32_t j = 0; j < nkeys; ++j)
    if (group_cols[j] >= tab->ncols ||
        tab->types[group_cols[j]] == SDB_COL_F32)
      return SDB_ERR_INVALID;
  bool ext = false;
  if (agg_specs_check(tab, aggs, naggs, &ext)) return SDB_ERR_INVALID;

  hipStream_t stream = ctx->stream;
  HashAggArgsMK a{};
  if (hash_args_fill(a, tab, tab->refs[group_cols[0]], preds, npreds, aggs,
                     naggs))
    return SDB_ERR_INVALID;
  a.nkeys = nkeys;
  a.stride = naggs + 2 * nkeys + 2;
  for (uint32_t j = 0; j < nkeys; ++j) {
    a.mkeys[j] = tab->refs[group_cols[j]];
    a.key_valid[j] = tab->valid[group_cols[j]];
  }
  // test hook, read per call: keep only the low bits of the hash so that
  // the witness check and the reseeded scan can be exercised
  a.hash_mask = ~0ull;
  if (const char* hb = getenv("SDB_MK_HASH_BITS")) {
    const long bits = std::strtol(hb, nullptr, 10);
    if (bits >= 1 && bits < 64) a.hash_mask = (1ull << bits) - 1;
  }
  const uint32_t stride = a.stride;
  uint64_t cap;  // a slot holds its hash, accumulators and witness words
  hash_table_sizes(max_groups, stride, &cap, &a.lds_slots);
  a.gcap_mask = (uint32_t)(cap - 1);
  a.max_groups = (uint32_t)max_groups;
  const size_t lds =
    std::max<size_t>((size_t)a.lds_slots * 8 * (1 + stride), 16);

  // one allocation: [keys cap][acc cap*stride][misc 3][out max_groups*stride]
  // misc: [0]=inserts|overflow, rows_passed, live slots packed; out: the
  // live slots packed
  DevBuf d_ws;
  const uint64_t acc_words = cap * stride;
  HIP_CHECK(d_ws.alloc((cap + acc_words + 3 + max_groups * stride) * 8));
  unsigned long long* d_keys = d_ws.as<unsigned long long>();
  unsigned long long* d_acc = d_keys + cap;
  unsigned long long* d_misc = d_acc + acc_words;
  unsigned long long* d_out = d_misc + 3;
  a.gkeys = d_keys;
  a.gacc = d_acc;
  a.ginserts = (uint32_t*)d_misc;
  a.goverflow = (uint32_t*)d_misc + 1;
  a.rows_passed = d_misc + 1;

  const uint32_t nblocks = scan_nblocks(tab);
  const uint32_t cblocks =
    (uint32_t)std::min<uint64_t>(1024, (cap + 255) / 256);

  std::vector<unsigned long long> h_out;  // [n * stride], as d_out
  unsigned long long h_misc[3] = {0, 0, 0};
  uint64_t n = 0;
  const uint32_t wit = naggs;                // first witness word
  const uint32_t w_or = naggs + 2 * nkeys;   // OR of null masks; +1: of
                                             // their complements
  bool proved = false;
  for (uint64_t seed = 0; seed < 4 && !proved; ++seed) {
    a.seed = seed;
    HIP_CHECK(hipMemsetAsync(d_keys, 0xFF, cap * 8, stream));
    HIP_CHECK(hipMemsetAsync(d_acc, 0, (acc_words + 3) * 8, stream));
    hipLaunchKernelGGL(scan_agg_hash_multi_kernel, dim3(nblocks),
                       dim3(SCAN_NTHREADS), lds, stream, a);
    HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(hash_multi_compact_kernel, dim3(cblocks), dim3(256),
                       0, stream, d_keys, d_acc, (uint32_t)cap, stride,
                       (uint32_t)max_groups, d_out, (uint32_t*)(d_misc + 2));
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipMemcpyAsync(h_misc, d_misc, 24, hipMemcpyDeviceToHost,
                             stream));
    HIP_CHECK(hipStreamSynchronize(stream));
    const uint32_t inserts = (uint32_t)(h_misc[0] & 0xFFFFFFFFu);
    const uint32_t overflow = (uint32_t)(h_misc[0] >> 32);
    // distinct hashes never outnumber distinct tuples: too many is final
    if (overflow || inserts > max_groups) return SDB_ERR_OOM;
    n = std::min<uint64_t>(h_misc[2] & 0xFFFFFFFFu, max_groups);
    h_out.resize(n * stride);
    if (n) {
      HIP_CHECK(hipMemcpyAsync(h_out.data(), d_out, n * stride * 8,
                               hipMemcpyDeviceToHost, stream));
      HIP_CHECK(hipStreamSynchronize(stream));
    }
    // the witness: one null mask, and one value in each position it leaves
    proved = true;
    for (uint64_t i = 0; i < n && proved; ++i) {
      const unsigned long long* w = &h_out[i * stride];
      const unsigned long long nm = w[w_or];
      proved = (nm & w[w_or + 1]) == 0;
      for (uint32_t j = 0; j < nkeys && proved; ++j)
        if (!((nm >> j) & 1ull))
          proved = ~w[wit + 2 * j] == w[wit + 2 * j + 1];
    }
  }
  if (!proved) return SDB_ERR_COLLISION;

  // tuples ascending, column by column as signed i64, NULL last in its
  // column. Sorted as packed records (the slot's null mask, and per position
  // the MAX code = key ^ sign, unsigned order = signed order), not through
  // the slots.
  struct Rec {
    unsigned long long code[SDB_MAX_GROUP_KEYS];
    uint32_t nullmask, slot;
  };
  std::vector<Rec> recs(n);
  for (uint32_t i = 0; i < n; ++i) {
    const unsigned long long* w = &h_out[(uint64_t)i * stride];
    recs[i].nullmask = (uint32_t)w[w_or];
    recs[i].slot = i;
    for (uint32_t j = 0; j < SDB_MAX_GROUP_KEYS; ++j)
      recs[i].code[j] = j < nkeys ? w[wit + 2 * j + 1] : 0;
  }
  std::sort(recs.begin(), recs.end(), [&](const Rec& x, const Rec& y) {
    for (uint32_t j = 0; j < nkeys; ++j) {
      const bool jx = (x.nullmask >> j) & 1u, jy = (y.nullmask >> j) & 1u;
      if (jx != jy) return jy;
      if (!jx && x.code[j] != y.code[j]) return x.code[j] < y.code[j];
    }
    return false;
  });
  for (size_t g = 0; g < n; ++g) {
    const Rec& r = recs[g];
    keynull_out[g] = r.nullmask;
    for (uint32_t j = 0; j < nkeys; ++j)
      keys_out[g * nkeys + j] =
        ((r.nullmask >> j) & 1u) ? 0 : (int64_t)(r.code[j] ^ SDB_I64_SIGN);
    for (uint32_t q = 0; q < naggs; ++q)
      agg_decode(aggs[q].op, h_out[(uint64_t)r.slot * stride + q],
                 &out[g * naggs + q]);
  }
  *ngroups_out = n;
  *rows_passed = h_misc[1];
  return SDB_OK;
}

// FNV-1a 64 over each row's DECODED string bytes (raw slot: the bytes
// themselves; FSST slot: symbols expanded on the fly). Deterministic and
// restated in oracle/pyoracle.fnv1a64 — the string-key GROUP BY below
// groups by this hash, with injectivity over the column's distinct
// strings checked host-side by the caller (collision => exact fallback).
struct StrHashArgs {
  const uint64_t* off;
  const uint8_t* blob;
  uint64_t rows;
  long long* out;
  uint32_t fsst;  // 0 = raw slot; an FSST slot may have nsym == 0
  uint32_t nsym;
  uint16_t symoff[256];
  uint8_t syms[2048];
};

__global__ void strhash_kernel(StrHashArgs ha) {
  __shared__ uint8_t ssym[2048];
  __shared__ uint16_t soff[256];
  for (uint32_t i = threadIdx.x; i < 2048; i += blockDim.x)
    ssym[i] = ha.syms[i];
  for (uint32_t i = threadIdx.x; i < 256; i += blockDim.x)
    soff[i] = ha.symoff[i];
  __syncthreads();
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
       r < ha.rows; r += stride) {
    const uint64_t o0 = ha.off[r], o1 = ha.off[r + 1];
    unsigned long long h = 14695981039346656037ull;
    bool bad = false;
    if (!ha.fsst) {  // raw bytes
      for (uint64_t i = o0; i < o1; ++i) {
        h ^= ha.blob[i];
        h *= 1099511628211ull;
      }
    } else {
      for (uint64_t i = o0; i < o1; ++i) {
        const uint8_t c = ha.blob[i];
        if (c == 255u) {
          if (++i >= o1) { bad = true; break; }
          h ^= ha.blob[i];
          h *= 1099511628211ull;
        } else if (c >= ha.nsym) {
          bad = true;
          break;
        } else {
          for (uint32_t j = soff[c]; j < (uint32_t)soff[c + 1]; ++j) {
            h ^= ssym[j];
            h *= 1099511628211ull;
          }
        }
      }
    }
    // malformed rows hash to the FNV basis of the empty string XOR a
    // sentinel so they cannot silently merge with a real group
    ha.out[r] = bad ? (long long)0x8000000000000001ull : (long long)h;
  }
}

// GROUP BY string keys ("GROUP BY text keys" on
// non-dictionary columns; the reference hands this to its DuckDB fork's
// PhysicalHashAggregate over string vectors — result-level parity).
// keys_out receives the FNV-1a 64 hash of each group's string; the
// caller resolves hashes back to strings host-side and MUST verify
// injectivity over the column's distinct strings (the python wrapper
// does both; a collision is detected, never silent).
int sdb_gpu_scan_agg_hash_str(SdbGpuCtx* ctx, SdbGpuTable* tab,
                              uint32_t str_slot, uint64_t max_groups,
                              const SdbPredSpec* preds, uint32_t npreds,
                              const SdbAggSpec* aggs, uint32_t naggs,
                              int64_t* keys_out, SdbAggResult* out,
                              uint64_t* ngroups_out,
                              uint64_t* rows_passed) {
  if (!ctx || !tab || str_slot >= SDB_MAX_STRCOLS ||
      !tab->str_off[str_slot])
    return SDB_ERR_INVALID;
  // the core repeats this; here it keeps a bad list from launching the
  // hash kernel first
  bool ext = false;
  if (naggs > SCAN_MAX_AGGS || agg_specs_check(tab, aggs, naggs, &ext))
    return SDB_ERR_INVALID;
  DevBuf d_hash;
  HIP_CHECK(d_hash.alloc(8ull * (tab->rows ? tab->rows : 1)));
  StrHashArgs ha{};
  ha.off = tab->str_off[str_slot];
  ha.blob = tab->str_blob[str_slot];
  ha.rows = tab->rows;
  ha.out = d_hash.as<long long>();
  if (tab->str_fsst[str_slot]) {
    ha.fsst = 1;
    ha.nsym = tab->str_nsym[str_slot];
    std::memcpy(ha.symoff, tab->str_symoff[str_slot], sizeof(ha.symoff));
    std::memcpy(ha.syms, tab->str_syms[str_slot], sizeof(ha.syms));
  }
  const uint32_t nb =
    (uint32_t)std::min<uint64_t>(4096, (tab->rows + 255) / 256);
  hipLaunchKernelGGL(strhash_kernel, dim3(nb ? nb : 1), dim3(256), 0,
                     ctx->stream, ha);
  HIP_CHECK(hipGetLastError());
  return scan_agg_hash_core(ctx, tab, ColRef{d_hash.p, nullptr}, max_groups,
                            preds, npreds, aggs, naggs, keys_out, out,
                            ngroups_out, rows_passed);
}

// ---- ORDER BY col [DESC] LIMIT k (include/sdb_gpu.h; the scheme is
// described at topn_kernel) ----

int sdb_gpu_scan_topn(SdbGpuCtx* ctx, SdbGpuTable* tab, uint32_t order_col,
                      uint32_t flags, uint32_t k, const SdbPredSpec* preds,
                      uint32_t npreds, uint64_t* rows_out,
                      SdbAggResult* vals_out, uint8_t* null_out,
                      uint64_t* n_out, uint64_t* rows_passed,
                      SdbTopnStats* stats) {
  if (!ctx || !tab || !rows_out || !vals_out || !null_out || !n_out ||
      !rows_passed || k == 0 || k > SDB_TOPN_MAX_K ||
      order_col >= tab->ncols ||
      (flags & ~(SDB_TOPN_DESC | SDB_TOPN_NULLS_FIRST)))
    return SDB_ERR_INVALID;
  TopnArgs a{};
  a.order = tab->refs[order_col];
  a.order_valid = tab->valid[order_col];
  a.rows = tab->rows;
  a.group_rows = tab->group_rows;
  a.desc = (flags & SDB_TOPN_DESC) ? 1u : 0u;
  a.npreds = npreds;
  // a mask predicate rides on no column here: preds_pass reads none for it
  if (preds_resolve(a.ps, tab, preds, npreds, ColRef{nullptr, nullptr}))
    return SDB_ERR_INVALID;
  const bool isf32 = tab->types[order_col] == SDB_COL_F32;
  const int ot = isf32 ? 2 : (a.order.desc ? 1 : 0);
  const bool nulls_first = (flags & SDB_TOPN_NULLS_FIRST) != 0;

  // candidate capacity: 2^20 entries, or the SDB_TOPN_CAND_CAP test hook,
  // never below what the row-order arm needs
  uint64_t cand_cap = 1ull << 20;
  if (const char* e = std::getenv("SDB_TOPN_CAND_CAP"))
    cand_cap = std::strtoull(e, nullptr, 10);
  cand_cap = std::max<uint64_t>(cand_cap, (uint64_t)k + tab->group_rows);

  SdbTopnStats st{};
  st.cand_cap = cand_cap;
  *n_out = 0;
  *rows_passed = 0;
  if (tab->rows == 0) {
    if (stats) *stats = st;
    return SDB_OK;
  }

  hipStream_t stream = ctx->stream;
  const uint64_t n_rowgroups =
    (tab->rows + tab->group_rows - 1) / tab->group_rows;
  // ctx-cached workspace: a repeated call allocates nothing
  if (!ctx->d_topn_hist)
    HIP_CHECK(hipMalloc(&ctx->d_topn_hist, 8ull * (TOPN_BINS + TOPN_MISC)));
  if (ctx->topn_cand_cap < cand_cap) {
    if (ctx->d_topn_cand) (void)hipFree(ctx->d_topn_cand);
    ctx->d_topn_cand = nullptr;
    ctx->topn_cand_cap = 0;
    HIP_CHECK(hipMalloc(&ctx->d_topn_cand, sizeof(TopnCand) * cand_cap));
    ctx->topn_cand_cap = cand_cap;
  }
  if (ctx->topn_rg_cap < n_rowgroups) {
    if (ctx->d_topn_rg) (void)hipFree(ctx->d_topn_rg);
    ctx->d_topn_rg = nullptr;
    ctx->topn_rg_cap = 0;
    HIP_CHECK(hipMalloc(&ctx->d_topn_rg, 4ull * n_rowgroups));
    ctx->topn_rg_cap = n_rowgroups;
  }
  a.hist = ctx->d_topn_hist;
  a.misc = ctx->d_topn_hist + TOPN_BINS;
  a.rg_count = ctx->d_topn_rg;
  a.cand = (TopnCand*)ctx->d_topn_cand;
  a.cand_cap = cand_cap;
  const uint32_t nblocks = scan_nblocks(tab);

  std::vector<unsigned long long> h(TOPN_BINS + TOPN_MISC);
  std::vector<uint32_t> h_rg;
  std::vector<TopnCand> vcand, ncand;

  // the first `want` members of a class in row order: count them per row
  // group, find the last row group needed, collect up to it
  auto count_class = [&](uint64_t want) -> int {
    a.tie_rg_end = 0xFFFFFFFFu;
    topn_launch(ot, TOPN_COUNT, nblocks, stream, a);
    HIP_CHECK(hipGetLastError());
    h_rg.resize(n_rowgroups);
    HIP_CHECK(hipMemcpyAsync(h_rg.data(), a.rg_count, 4ull * n_rowgroups,
                              hipMemcpyDeviceToHost, stream));
    HIP_CHECK(hipStreamSynchronize(stream));
    uint64_t run = 0;
    uint32_t g = 0;
    for (; g < n_rowgroups; ++g) {
      run += h_rg[g];
      if (run >= want) break;
    }
    if (g == n_rowgroups) return SDB_ERR_HIP;  // the passes disagree
    a.tie_rg_end = g + 1;
    return SDB_OK;
  };
  auto collect = [&](std::vector<TopnCand>& dst) -> int {
    HIP_CHECK(hipMemsetAsync(a.misc + 2, 0, 16, stream));
    topn_launch(ot, TOPN_COLLECT, nblocks, stream, a);
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipMemcpyAsync(h.data() + TOPN_BINS, a.misc, 8ull * TOPN_MISC,
                              hipMemcpyDeviceToHost, stream));
    HIP_CHECK(hipStreamSynchronize(stream));
    const uint64_t n = h[TOPN_BINS + 2];
    if (h[TOPN_BINS + 3] || n > cand_cap) return SDB_ERR_OOM;
    st.candidates += n;
    dst.resize(n);
    if (n) HIP_CHECK(hipMemcpy(dst.data(), a.cand, sizeof(TopnCand) * n,
                                hipMemcpyDeviceToHost));
    return SDB_OK;
  };

  // ---- histogram passes: digits of 11 bits from the top of the code ----
  const uint32_t W = isf32 ? 32u : 64u;
  const uint32_t ndigits = (W + 10u) / 11u;
  uint64_t passed = 0, null_passed = 0, kv = 0, r_null = 0;
  uint64_t above = 0, ge = 0;  // rows above the prefix's range / at or above
  unsigned long long prefix = 0, prefix_mask = 0;
  bool resolved = false;       // ge <= cand_cap: collect at the lower bound
  for (uint32_t d = 0; d < ndigits; ++d) {
    const uint32_t bits = std::min(11u, W - 11u * d);
    const uint32_t shift = W - 11u * d - bits;
    a.prefix = prefix;
    a.prefix_mask = prefix_mask;
    a.shift = shift;
    a.digit_mask = (1u << bits) - 1u;
    a.first = d == 0;
    HIP_CHECK(hipMemsetAsync(
      a.hist, 0, 8ull * (TOPN_BINS + (d == 0 ? TOPN_MISC : 0u)), stream));
    topn_launch(ot, TOPN_HIST, nblocks, stream, a);
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipMemcpyAsync(h.data(), a.hist,
                              8ull * (TOPN_BINS + TOPN_MISC),
                              hipMemcpyDeviceToHost, stream));
    HIP_CHECK(hipStreamSynchronize(stream));
    ++st.hist_passes;
    if (d == 0) {
      passed = h[TOPN_BINS + 0];
      null_passed = h[TOPN_BINS + 1];
      const uint64_t nonnull = passed - null_passed;
      if (nulls_first) {
        r_null = std::min<uint64_t>(k, null_passed);
        kv = std::min<uint64_t>(k - r_null, nonnull);
      } else {
        kv = std::min<uint64_t>(k, nonnull);
        r_null = std::min<uint64_t>(k - kv, null_passed);
      }
      if (kv == 0) break;
    }
    // from the top bin down to the one in which the running count reaches kv
    uint64_t run = above;
    int b = (int)a.digit_mask;
    for (; b >= 0; --b) {
      if (run + h[b] >= kv) break;
      run += h[b];
    }
    if (b < 0) return SDB_ERR_HIP;  // the passes disagree
    above = run;
    ge = run + h[b];
    prefix |= (unsigned long long)b << shift;
    prefix_mask |= (unsigned long long)a.digit_mask << shift;
    if (ge <= cand_cap) {
      resolved = true;
      break;
    }
  }

  // ---- values: everything at or above the prefix's lower bound, or, with
  // every digit resolved and the ties at the k-th code still too many, the
  // rows above it and the first kv - above of the ties in row order ----
  if (kv) {
    a.cls_null = 0;
    a.thr = prefix;
    a.tie_rg_end = 0xFFFFFFFFu;
    if (!resolved) {
      st.tie_arm = 1;
      const int rc = count_class(kv - above);
      if (rc) return rc;
    }
    const int rc = collect(vcand);
    if (rc) return rc;
    if (vcand.size() < kv) return SDB_ERR_HIP;
    std::partial_sort(vcand.begin(), vcand.begin() + kv, vcand.end(),
                      [](const TopnCand& x, const TopnCand& y) {
                        return x.code != y.code ? x.code > y.code
                                                : x.row < y.row;
                      });
  }
  // ---- the NULL class: its first r_null members in row order ----
  if (r_null) {
    st.tie_arm = 1;
    a.cls_null = 1;
    a.thr = 0;
    int rc = count_class(r_null);
    if (rc) return rc;
    rc = collect(ncand);
    if (rc) return rc;
    if (ncand.size() < r_null) return SDB_ERR_HIP;
    std::partial_sort(ncand.begin(), ncand.begin() + r_null, ncand.end(),
                      [](const TopnCand& x, const TopnCand& y) {
                        return x.row < y.row;
                      });
  }
  st.rowgroups_skipped = (uint32_t)h[TOPN_BINS + 4];

  uint64_t n = 0;
  auto emit_nulls = [&] {
    for (uint64_t i = 0; i < r_null; ++i, ++n) {
      rows_out[n] = ncand[i].row;
      vals_out[n] = SdbAggResult{0, 0.0};
      null_out[n] = 1;
    }
  };
  if (nulls_first) emit_nulls();
  for (uint64_t i = 0; i < kv; ++i, ++n) {
    const unsigned long long c = vcand[i].code;
    rows_out[n] = vcand[i].row;
    null_out[n] = 0;
    if (isf32) {
      const uint32_t key = a.desc ? (uint32_t)c : ~(uint32_t)c;
      const uint32_t fb =
        (key & 0x80000000u) ? key ^ 0x80000000u : ~key;
      float f;
      std::memcpy(&f, &fb, 4);
      vals_out[n] = SdbAggResult{0, (double)f};
    } else {
      vals_out[n] =
        SdbAggResult{(int64_t)((a.desc ? c : ~c) ^ SDB_I64_SIGN), 0.0};
    }
  }
  if (!nulls_first) emit_nulls();
  *n_out = n;
  *rows_passed = passed;
  if (stats) *stats = st;
  return SDB_OK;
}

int sdb_gpu_table_gather(SdbGpuCtx* ctx, SdbGpuTable* tab, uint32_t col,
                         const uint64_t* rows, uint64_t n, SdbAggResult* out,
                         uint8_t* null_out) {
  if (!ctx || !tab || col >= tab->ncols || n > (1ull << 20) ||
      (n && (!rows || !out || !null_out)))
    return SDB_ERR_INVALID;
  for (uint64_t i = 0; i < n; ++i)
    if (rows[i] >= tab->rows) return SDB_ERR_INVALID;
  if (n == 0) return SDB_OK;
  // one allocation: rows in, values out, NULL flags out
  DevBuf buf;
  HIP_CHECK(buf.alloc(17ull * n));
  unsigned char* d_buf = buf.as<unsigned char>();
  GatherArgs g{};
  g.col = tab->refs[col];
  g.valid = tab->valid[col];
  g.type = (int)tab->types[col];
  g.group_rows = tab->group_rows;
  g.rows = (const unsigned long long*)d_buf;
  g.n = n;
  g.vals = (unsigned long long*)(d_buf + 8ull * n);
  g.nulls = d_buf + 16ull * n;
  std::vector<unsigned long long> h_vals(n);
  HIP_CHECK(hipMemcpyAsync(d_buf, rows, 8ull * n, hipMemcpyHostToDevice,
                           ctx->stream));
  hipLaunchKernelGGL(table_gather_kernel, dim3((uint32_t)((n + 255) / 256)),
                     dim3(256), 0, ctx->stream, g);
  HIP_CHECK(hipGetLastError());
  HIP_CHECK(hipMemcpyAsync(h_vals.data(), g.vals, 8ull * n,
                           hipMemcpyDeviceToHost, ctx->stream));
  HIP_CHECK(hipMemcpyAsync(null_out, g.nulls, n, hipMemcpyDeviceToHost,
                           ctx->stream));
  HIP_CHECK(hipStreamSynchronize(ctx->stream));
  for (uint64_t i = 0; i < n; ++i) {
    if (tab->types[col] == SDB_COL_F32) {
      const uint32_t fb = (uint32_t)h_vals[i];
      float f;
      std::memcpy(&f, &fb, 4);
      out[i] = SdbAggResult{0, null_out[i] ? 0.0 : (double)f};
    } else {
      out[i] = SdbAggResult{(int64_t)h_vals[i], 0.0};
    }
  }
  return SDB_OK;
}


}  // extern "C"
