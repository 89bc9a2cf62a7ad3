// sdb_internal.h — shared internal context layout between sdb_gpu.hip and
// sdb_scan.hip (not part of the public C ABI).
#pragma once
#include <hip/hip_runtime.h>
#include "../../../include/sdb_gpu.h"

struct TermDev {
  uint64_t desc_begin;
  uint64_t desc_end;
  uint64_t payload_begin;
  float num;  // boost*(k+1)*idf  (Bm25Score::num, bm25.cpp:225)
  float nc;   // norm_const = k(1-b)
  float nl;   // norm_length = k*b/avgDL
};

// ---- hybrid bucket rule (sdb_gpu.h, "hybrid") ----
// bucket = floor(d * nb / span), d = (u64)(v - lo), span = (hi - lo) + 1,
// exact for every int64 lo <= v <= hi: span reaches 2^64 and d * nb 2^71.
// The span travels as span_m1 = span - 1 = (u64)hi - (u64)lo, which always
// fits; the subtraction is unsigned, so no signed overflow.
//
// The host decides once per call which of the two forms is exact and
// launches the kernel instantiation compiled for it, so a narrow span runs
// the one-multiply, one-divide code alone. A span is wide iff
// span_m1 * nb >= 2^64, i.e. iff d * nb can leave 64 bits, or the span
// itself is 2^64 (which nb = 1 reaches without the former).
__host__ __device__ inline bool sdb_bucket_span_wide(
  unsigned long long span_m1, uint32_t nb) {
  return nb != 0 && (span_m1 == ~0ull || span_m1 > ~0ull / nb);
}

__host__ __device__ inline uint32_t sdb_bucket_narrow(
  unsigned long long d, uint32_t nb, unsigned long long span_m1) {
  uint32_t bkt = (uint32_t)((d * nb) / (span_m1 + 1ull));
  if (bkt >= nb) bkt = nb - 1;
  return bkt;
}

__host__ __device__ inline unsigned long long sdb_mul64hi(
  unsigned long long x, unsigned long long y) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __umul64hi(x, y);
#else
  return (unsigned long long)(((unsigned __int128)x * y) >> 64);
#endif
}

// any span: the quotient is < nb <= 128 (as d < span), found in 7 steps of
// a 128-bit compare; no 128-bit division on the device
__host__ __device__ inline uint32_t sdb_bucket_wide(
  unsigned long long d, uint32_t nb, unsigned long long span_m1) {
  const unsigned long long nhi = sdb_mul64hi(d, nb), nlo = d * nb;
  if (span_m1 == ~0ull) return (uint32_t)nhi;  // span = 2^64
  const unsigned long long span = span_m1 + 1ull;
  uint32_t q = 0;  // largest q < nb with q * span <= d * nb
  for (uint32_t step = 64; step; step >>= 1) {
    const uint32_t c = q + step;
    if (c >= nb) continue;
    const unsigned long long chi = sdb_mul64hi(c, span), clo = c * span;
    if (chi < nhi || (chi == nhi && clo <= nlo)) q = c;
  }
  return q;
}

struct SdbGpuCtx {
  int device;
  hipStream_t stream;
  // cached dense-scan workspace: the dense scan_agg hot path is
  // allocation-free across calls (grown on demand, freed with the ctx)
  unsigned long long* d_scan_out;
  uint64_t scan_out_cap;  // slots
  unsigned long long* d_scan_passed;  // [2]: rows passed, NULL-key rows
  SdbScoreDoc* d_cands;
  uint32_t* d_cand_count;
  unsigned long long* d_total_matches;
  uint32_t* d_gthresh;  // float bits
  uint32_t* d_ghist;    // global 256-bin score histogram (threshold tightening)
  unsigned long long* d_buckets;  // hybrid bucket aggregates [2*128]
  TermDev* d_terms;
  uint32_t* d_overflow;
  uint32_t* h_counts;  // pinned: [cand_count, overflow, final_bin]
  unsigned long long* h_matches;
  hipEvent_t ev_a, ev_b;   // bracket the window kernels of one execute call
  // pipelined-batch state (sdb_gpu_execute_topk_batch): second query-state
  // set + dedicated copy stream + pinned readback
  hipStream_t copy_stream;
  SdbScoreDoc* d_cands2;
  uint32_t* d_ghist2;
  unsigned char* d_qmisc;   // 2 x 64 B: {gthresh u32, pad, cand_count u32,
                            //  overflow u32, total u64} per set
  unsigned char* h_qmisc;   // pinned mirror
  TermDev* h_terms_pin;     // pinned term-table staging (SDB_TERM_SLOTS
                            // x SDB_MAX_TERMS): pageable-source async
                            // copies block the host until the stream
                            // drains, which serialized the batch pipeline
  SdbScoreDoc* h_cands_pin; // pinned candidate staging (SDB_PIN_CANDS)
  hipEvent_t ev_q[2];
  double last_kernel_ms;   // read back via sdb_gpu_last_kernel_ms
  // breakdown of the last execute_topk (sdb_gpu_last_stats)
  unsigned last_ncand;
  unsigned last_sweep_grid;  // sdb_gpu_last_sweep_grid
  unsigned last_window_grid; // sdb_gpu_last_window_grid
  float last_gtau;
  double last_readback_ms;
  double last_select_ms;
  // cached sdb_gpu_scan_topn workspace, grown on demand like d_scan_out:
  // digit histogram + counters, candidate buffer, per-row-group counts
  unsigned long long* d_topn_hist;
  void* d_topn_cand;
  uint64_t topn_cand_cap;  // entries
  uint32_t* d_topn_rg;
  uint64_t topn_rg_cap;    // row groups
};
