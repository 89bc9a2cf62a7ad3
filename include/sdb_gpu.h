/* sdb_gpu.h — C ABI of the MI355X-native SereneDB search/analytics hot path.
 *
 * This is the drop-in boundary of SURVEY.md §8(b): the entry points a
 * maintainer of the reference would bind where its scan operator hands a
 * prepared per-segment query to the execution hot loop:
 *
 *   sdb_gpu_execute_topk  replaces the per-segment collect loop
 *     CollectSegmentTopK / RunTopKScan
 *     (server/connector/duckdb_search_full_scan.cpp:1868-1943) and the
 *     standalone driver irs::ExecuteTopK/ExecuteTopKWithCount
 *     (libs/iresearch/include/iresearch/search/doc_collector.hpp:44-136),
 *     i.e. DocIterator::Collect (index/iterators.hpp:297-298,400-428) over a
 *     BlockDisjunction/Conjunction (search/block_disjunction.hpp:122-732,
 *     search/conjunction.hpp:248-529) scored by BM25
 *     (search/bm25.cpp:60-109,279-310) into an NthPartitionScoreCollector
 *     (index/iterators.hpp:103-253).
 *
 *   sdb_gpu_scan_agg  replaces FullScanner::Scan + ColFilterChain predicate
 *     narrowing (server/connector/full_scanner.h:40-90,
 *     index/table_filter_iterator.hpp:104-312) feeding the external DuckDB
 *     PhysicalHashAggregate (un-vendored; parity pinned at SQL-result level,
 *     SURVEY.md §8c).
 *
 * Conventions: every function returns 0 on success or a negative SDB_ERR_*
 * code; all buffers are caller-allocated; an opaque context owns the device,
 * streams and workspace; one context is single-threaded, use one per thread.
 * Hot entry points never allocate on the device after segment load. The
 * implementation REQUIRES a GPU: calls fail loudly (SDB_ERR_NO_GPU) rather
 * than fall back to any CPU path.
 *
 * ScoreDoc mirrors irs::ScoreDoc (index/iterators.hpp:93-99). Doc-id
 * conventions follow utils/type_limits.hpp:41-47 (invalid=0, min=1,
 * eof=0xFFFFFFFF).
 */
#ifndef SDB_GPU_H
#define SDB_GPU_H

#include <stddef.h>
#include <stdint.h>

#include "sdb_format.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SDB_OK 0
#define SDB_ERR_INVALID (-1)
#define SDB_ERR_NO_GPU (-2)
#define SDB_ERR_HIP (-3)
#define SDB_ERR_OOM (-4)
#define SDB_ERR_BAD_SEGMENT (-5)
#define SDB_ERR_COLLISION (-6) /* sdb_gpu_scan_agg_hash_multi: see there */
/* Every sdb_gpu_table_* / sdb_gpu_strpred_* / sdb_gpu_scan_* entry maps a
 * failed device call the same way: no device -> SDB_ERR_NO_GPU, a failed
 * device allocation -> SDB_ERR_OOM (the attach, string-predicate, string-key
 * and gather entries too, which once answered SDB_ERR_HIP for it), anything
 * else -> SDB_ERR_HIP. */

/* mirrors irs::ScoreDoc: {score_t score; doc_id_t doc; uint32_t segment_idx}
 * (index/iterators.hpp:93-99) */
typedef struct SdbScoreDoc {
  float score;
  uint32_t doc;
  uint32_t segment_idx;
} SdbScoreDoc;

typedef struct SdbGpuCtx SdbGpuCtx;     /* opaque: device, stream, workspace */
typedef struct SdbGpuSegment SdbGpuSegment; /* opaque: device-resident segment */

/* ---- context ---- */
int sdb_gpu_ctx_create(int device, SdbGpuCtx** out);
int sdb_gpu_ctx_destroy(SdbGpuCtx* ctx);
/* version/build string (static) */
const char* sdb_gpu_version(void);

/* ---- segment residency ----
 * Uploads a segment blob (the byte span of sdb_format.h) into HBM and keeps
 * it resident — the analogue of the reference's mmap'd segment files
 * (store/mmap_directory.hpp) with 288 GB HBM3E standing in for the page
 * cache. `blob` must stay valid during the call only. */
int sdb_gpu_segment_load(SdbGpuCtx* ctx, const void* blob, size_t blob_size,
                         SdbGpuSegment** out);
int sdb_gpu_segment_free(SdbGpuCtx* ctx, SdbGpuSegment* seg);

/* ---- query plan ----
 * Terms are addressed by index into the segment's term table: the term-dict
 * lookup (burst-trie .tm) is a per-query O(#terms) CPU step in the reference
 * and stays on the host (SURVEY.md §2 "formats/index": out of scope).
 * Per-term boost mirrors irs::Filter boost. min_match = 1 is an OR
 * (BlockDisjunction), min_match = nterms an AND (Conjunction), anything
 * between mirrors BlockDisjunction's min-match counting
 * (block_disjunction.hpp:122-732 match counts). */
typedef struct SdbTermRef {
  uint32_t term_idx;
  float boost;
} SdbTermRef;

typedef enum SdbScorerType {
  SDB_SCORER_BM25 = 0,       /* search/bm25.cpp:89-109 */
  SDB_SCORER_TFIDF = 1,      /* search/tfidf.cpp:60-62: idf*sqrt(freq) */
  SDB_SCORER_TFIDF_NORM = 2, /* tfidf.cpp:72-76: idf*sqrt(freq)/sqrt(norm) */
} SdbScorerType;

/* The plan contract. Every entry that takes a plan (sdb_gpu_execute_topk,
 * _batch, _count, _match_docs and the hybrid forms) checks it before anything
 * is launched and returns SDB_ERR_INVALID otherwise; the context stays
 * usable. Scores must be finite and >= 0: the histogram bins, the bin
 * threshold and the WAND bounds all rest on that.
 *   terms      non-NULL, 1..32 of them, no term twice, every term_idx below
 *              the term count of every segment passed
 *   boost      finite and >= 0 per term (0 is fine: the term's docs match
 *              and count, and add nothing to a score)
 *   scorer     a value of SdbScorerType
 *   k1         finite and >= 0 (0 is BM1); checked whatever the scorer
 *   b          in [0, 1] (0 is BM15); a b above 1 would make norm_const =
 *              k1 - k1*b negative, and with it the scores
 *   g_*        g_docs_with_field != 0 switches to the injected stats; then
 *              g_docs_with_term is non-NULL and no entry exceeds
 *              g_docs_with_field (0 is fine: that term scores nothing)
 *   bound      every per-term numerator (boost * (k1 + 1) * idf, or boost *
 *              idf) and the plan's score bound (their sum, times
 *              sqrt(max freq) for the TFIDF forms, times the largest filter
 *              boost) must be finite floats
 * total_matches counts every doc matched by at least min_match terms (and
 * live), whatever it scores: a doc scoring 0 or below the acceptance
 * threshold is counted and never returned. */
typedef struct SdbQueryPlan {
  const SdbTermRef* terms;
  uint32_t nterms;
  uint32_t min_match;
  float k1; /* BM25 k (search/bm25.hpp:62: default 1.2) */
  float b;  /* BM25 b (search/bm25.hpp:64: default 0.75) */
  uint32_t scorer; /* SdbScorerType; TFIDF idf = log1p((N+1)/(df+1)),
                      tfidf.cpp:148-151 */
  /* WAND block-max pruning (max_score_iterator.hpp Block-Max MaxScore
   * analogue over the descriptor max_freq/min_norm bounds): skips postings
   * blocks that provably cannot reach the current k-th score. EXACT top-k
   * (every skipped doc's full score < the threshold); only valid for pure
   * disjunctions (min_match == 1); total_matches then counts only VISITED
   * matches (the reference's WAND path likewise stops counting,
   * reader.hpp:517-524 wand gate). 0 = off. */
  uint32_t wand;
  /* Optional GLOBAL BM25 stats for sharded (multi-rank) execution, where
   * each device holds only its shard: the cross-rank stats merge is the
   * PreparePhase barrier analogue (duckdb_search_full_scan.cpp:1359-1384)
   * done over RCCL by the caller. Zero/NULL = derive from the segments
   * passed to this call (single-node ExecuteTopKWithCount semantics). */
  uint64_t g_docs_with_field;
  uint64_t g_total_term_freq;
  const uint64_t* g_docs_with_term; /* per plan term, or NULL */
  /* HasFilterBoost scorer variants (bm25.cpp:112-140 Bm1Boost, :69-109
   * Bm15/Bm25 boost[i]*num; tfidf equivalents): when nonzero, every
   * segment must have a boost column attached (sdb_gpu_segment_attach_
   * boost) and each term contribution is multiplied by boost[doc]. The
   * boost folds into the numerator BEFORE the score form, the reference's
   * order of operations: nm = fl(num * boost[doc]), then nm - nm*c1/(c1 +
   * freq) or nm*sqrt(freq)[/sqrt(norm)]; multiplying the finished score
   * instead rounds differently. A segment without a column, or columns
   * that are 0 everywhere, are SDB_ERR_INVALID. With
   * k1 == 0 this is BM1's only nonzero form: score = boost[doc]*num.
   * (The reference's Bm1Boost ASSIGNS rather than merges under multi-term
   * disjunctions; this implementation sums term contributions uniformly —
   * single-term BM1 parity is exact, the multi-term BM1 merge order is a
   * documented refinement.) */
  uint32_t filter_boost;
} SdbQueryPlan;

/* Execute BM25 top-k over segments resident on this context's device.
 *
 * Mirrors ExecuteTopKWithCount (doc_collector.hpp:44-86): a two-phase
 * stats-then-collect execution (PreparePhase analogue,
 * duckdb_search_full_scan.cpp:1359-1384): BM25Stats idf/norm_const/
 * norm_length are computed on the host in double then narrowed to f32
 * exactly as bm25.cpp:288-306 does, then every segment is scored on the GPU
 * and a global top-k is selected.
 *
 * Results: hits[0..*out_count) sorted by (score desc, segment asc, doc asc);
 * *out_count = min(k, accepted); *total_matches = number of matching docs
 * (TotalMatches analogue, index/iterators.hpp:133). Acceptance mirrors the
 * collector: score > FLT_MIN (doc_collector.hpp:58 initial threshold).
 * Determinism: scores are bit-exact reproductions of the reference fp32
 * arithmetic with term-major merge order; ties at the k-th score resolve by
 * (segment, doc) ascending — a deterministic refinement of the reference's
 * unspecified nth_element tie order (DESIGN.md "Determinism").
 *
 * segment_idx is the index into this call's segs, not the order in which the
 * segments were loaded; the same handle may appear more than once, and each
 * occurrence is a segment of its own. nsegs == 0 is SDB_OK with *out_count =
 * 0 and *total_matches = 0, here and on the batch, count and hybrid entries
 * (every bucket zero); a filter_boost plan over no segments has no column
 * maximum and is SDB_ERR_INVALID.
 *
 * hits must have room for k entries. */
int sdb_gpu_execute_topk(SdbGpuCtx* ctx, SdbGpuSegment* const* segs,
                         uint32_t nsegs, const SdbQueryPlan* plan, uint32_t k,
                         SdbScoreDoc* hits, uint32_t* out_count,
                         uint64_t* total_matches);

/* Pipelined batch: nq queries of the SAME plan, each fully re-executed
 * (nothing cached between queries); query q+1's kernels overlap query
 * q's candidate readback and exact host select — the production QPS
 * shape of RunTopKScan's worker loop (duckdb_search_full_scan.cpp:
 * 1925-2000). hits: nq*k entries; out_counts/totals: nq entries.
 * Results of every query are identical to sdb_gpu_execute_topk's. */
int sdb_gpu_execute_topk_batch(SdbGpuCtx* ctx, SdbGpuSegment* const* segs,
                               uint32_t nsegs, const SdbQueryPlan* plan,
                               uint32_t k, uint32_t nq, SdbScoreDoc* hits,
                               uint32_t* out_counts, uint64_t* totals);

/* pipelined-batch form of the hybrid entry (same per-query semantics as
 * sdb_gpu_execute_topk_hybrid): bucket_counts/bucket_sums hold
 * nq * nbuckets rows, query-major. Bucket state is double-buffered by
 * query parity so query k+1's kernels overlap query k's readback. */
int sdb_gpu_execute_topk_hybrid_batch(
  SdbGpuCtx* ctx, SdbGpuSegment* const* segs, uint32_t nsegs,
  const SdbQueryPlan* plan, uint32_t k, int64_t flo, int64_t fhi,
  uint32_t nbuckets, uint32_t nq, int64_t* bucket_counts,
  int64_t* bucket_sums, SdbScoreDoc* hits, uint32_t* out_counts,
  uint64_t* totals);

/* CountFast — exact match count without scoring (docs-only decode;
 * DecideScanMode Count/CountFast, duckdb_search_full_scan.cpp:972). */
int sdb_gpu_execute_count(SdbGpuCtx* ctx, SdbGpuSegment* const* segs,
                          uint32_t nsegs, const SdbQueryPlan* plan,
                          uint64_t* total_matches);

/* Streaming scan — the RunStreamingScan / HitBatcher analogue
 * (duckdb_search_full_scan.cpp:2370, index/hit_batcher.hpp:39-190): emit
 * every matching doc id ascending into docs_out (up to cap) and, when
 * col_out != NULL and a column is attached, the gathered i64 value per hit.
 * *total_matches = full match count. Single segment. */
int sdb_gpu_execute_match_docs(SdbGpuCtx* ctx, SdbGpuSegment* seg,
                               const SdbQueryPlan* plan, uint32_t* docs_out,
                               int64_t* col_out, uint64_t cap,
                               uint64_t* out_count, uint64_t* total_matches);

/* Raw postings-block decode of one term into caller buffers (docs+freqs,
 * df entries each). Parity/diagnostic entry (mirrors
 * FormatTraits128::ReadBlockDelta/ReadBlock, format_block_128.hpp:446-636);
 * runs on the GPU. */
int sdb_gpu_decode_term(SdbGpuCtx* ctx, SdbGpuSegment* seg, uint32_t term_idx,
                        uint32_t* docs, uint32_t* freqs);

/* ---- hybrid: top-k AND pushed column predicates ----
 * MaybeWrapColFilter semantics (duckdb_search_full_scan.cpp TableFilter
 * wrap; index/table_filter_iterator.hpp:104-312 ColFilterChain): matches
 * survive only if EVERY attached-column predicate passes; the analytics
 * consumer's per-bucket COUNT/SUM aggregates over the survivors.
 * Columns attach to numbered slots (up to 4); the original
 * sdb_gpu_segment_attach_column is slot 0. */
#define SDB_MAX_FILTER_COLS 4

typedef enum SdbPredOp {
  SDB_PRED_NONE = 0,
  SDB_PRED_LT = 1,  /* col < v */
  SDB_PRED_GE = 2,  /* col >= v */
  SDB_PRED_BETWEEN = 3, /* lo <= col <= hi */
  SDB_PRED_EQ = 4,  /* col == v (table_filter_iterator.hpp typed compares) */
  /* bare null checks, evaluated on the validity plane alone
   * (table_filter_iterator.hpp:65-67 NullCheckKind) */
  SDB_PRED_ISNULL = 5,
  SDB_PRED_NOTNULL = 6,
  /* raw variable-width string columns (non-dictionary; SURVEY.md 8f row
   * 3, second half — the dictionary path shipped round 1):
   * SDB_PRED_STRMASK consumes the row bitmask a prior
   * sdb_gpu_strpred_mask() call computed for string slot `col`
   * (lo/hi/flo/fhi ignored); SDB_PRED_PREFIX is valid only as the `op`
   * of sdb_gpu_strpred_mask (starts-with). */
  SDB_PRED_STRMASK = 7,
  SDB_PRED_PREFIX = 8,
  /* ends-with lo / holds lo as a substring: like PREFIX, valid only as the
   * `op` of sdb_gpu_strpred_mask / _ex (see there) */
  SDB_PRED_SUFFIX = 9,
  SDB_PRED_CONTAINS = 10,
} SdbPredOp;

int sdb_gpu_segment_attach_column(SdbGpuCtx* ctx, SdbGpuSegment* seg,
                                  const int64_t* data);
int sdb_gpu_segment_attach_column_slot(SdbGpuCtx* ctx, SdbGpuSegment* seg,
                                       uint32_t slot, const int64_t* data);
/* per-doc f32 filter-boost column (doc_count+1 entries, 1-based docs; entry
 * 0 is not looked at); consumed when SdbQueryPlan.filter_boost is set. Every
 * value must be finite and >= 0 (subnormals and 0 are fine): a column
 * holding a negative value, NaN or an infinity is SDB_ERR_INVALID, nothing
 * is uploaded and a column attached earlier stays in place. A finite
 * maximum can still be too large for a given plan (score bound times the
 * maximum overflows); that is refused when the plan is prepared. */
int sdb_gpu_segment_attach_boost(SdbGpuCtx* ctx, SdbGpuSegment* seg,
                                 const float* boost);
/* live-document bitmap — the deleted-docs mask the reference wraps around
 * every scan when a segment has deletes (seg.mask(it),
 * duckdb_search_full_scan.cpp:1898,2002,2226; Masked count mode :2475).
 * bit d of mask[d>>6] set = doc d live (docs 1..doc_count; bit 0 of word
 * 0 unused); (doc_count+64)/64 words. Once attached, every execute on the
 * segment sees only live docs (hits, counts, WAND thresholds, streaming
 * emission, hybrid aggregates). NULL detaches. */
int sdb_gpu_segment_attach_livemask(SdbGpuCtx* ctx, SdbGpuSegment* seg,
                                    const uint64_t* mask);

typedef struct SdbHybridPred {
  uint32_t slot;  /* attached column slot */
  SdbPredOp op;   /* LT / GE / BETWEEN (table_filter_iterator.hpp ops) */
  int64_t lo, hi; /* BETWEEN inclusive; LT/GE use lo */
} SdbHybridPred;

/* Single-predicate hybrid (BASELINE configs[3]): col0 BETWEEN [flo,fhi],
 * buckets over its value span.
 *
 * Bucket rule (this entry, _chain and _batch): a survivor with value v
 * lands in
 *     bucket = floor((v - flo) * nbuckets / (fhi - flo + 1))
 * in exact integer arithmetic, for any int64 flo <= fhi -- the full span
 * flo = INT64_MIN, fhi = INT64_MAX (fhi - flo + 1 = 2^64) included; no
 * intermediate wraps. 1 <= nbuckets <= 128. flo > fhi is an empty range:
 * SDB_OK with total 0, no hits and every bucket zero. bucket_count[b] is
 * the number of survivors in bucket b; bucket_sum[b] is the sum of their
 * values as a wrap-around (mod 2^64) int64, as SDB_AGG_SUM_I64 is. */
int sdb_gpu_execute_topk_hybrid(SdbGpuCtx* ctx, SdbGpuSegment* const* segs,
                                uint32_t nsegs, const SdbQueryPlan* plan,
                                uint32_t k, int64_t flo, int64_t fhi,
                                uint32_t nbuckets, int64_t* bucket_count,
                                int64_t* bucket_sum, SdbScoreDoc* hits,
                                uint32_t* out_count, uint64_t* total_matches);

/* Predicate-chain hybrid: preds[0] must be BETWEEN (it defines the bucket
 * span); preds[1..] are additional AND-ed predicates on any attached slot.
 * bucket_count/bucket_sum aggregate preds[0]'s column over full survivors,
 * by the bucket rule above with flo/fhi = preds[0].lo/hi (exact for any
 * int64 lo <= hi; lo > hi is an empty result; sums wrap as int64). */
int sdb_gpu_execute_topk_hybrid_chain(
  SdbGpuCtx* ctx, SdbGpuSegment* const* segs, uint32_t nsegs,
  const SdbQueryPlan* plan, uint32_t k, const SdbHybridPred* preds,
  uint32_t npreds, uint32_t nbuckets, int64_t* bucket_count,
  int64_t* bucket_sum, SdbScoreDoc* hits, uint32_t* out_count,
  uint64_t* total_matches);

/* ---- columnar scan -> filter -> hash aggregate ---- */

/* Column layout: dense device-resident columns, or FoR/bitpack row groups
 * with min/max zonemaps (this repo's own codec — the reference's column
 * codecs live in the un-vendored DuckDB fork). */
typedef enum SdbColType {
  SDB_COL_I64 = 0,     /* dense i64 array */
  SDB_COL_F32 = 1,     /* dense f32 array */
  SDB_COL_I64_FOR = 2, /* FoR/bitpack row groups + zonemaps: the blob from
                          sdb_host_encode_col_i64 (data = blob pointer) */
} SdbColType;

typedef struct SdbColumnView {
  const void* data; /* HOST pointer at load time */
  uint64_t rows;
  SdbColType type;
} SdbColumnView;

typedef struct SdbGpuTable SdbGpuTable;

int sdb_gpu_table_load(SdbGpuCtx* ctx, const SdbColumnView* cols,
                       uint32_t ncols, uint64_t rows, SdbGpuTable** out);
int sdb_gpu_table_free(SdbGpuCtx* ctx, SdbGpuTable* tab);

/* Column validity (null) bitmap — SQL three-valued logic as the
 * reference's pushed filters implement it (null_semantics_fuzz.py;
 * table_filter_iterator.hpp NullCheckKind): a comparison predicate drops
 * NULL rows; SDB_PRED_ISNULL / SDB_PRED_NOTNULL evaluate the validity
 * plane alone; SUM aggregates skip NULL values while COUNT(*) counts the
 * row. bit r of bits[r>>6] set = row r VALID; (rows+63)/64 words. NULL
 * detaches (all valid). A plane on the GROUP-KEY column makes the key
 * nullable: sdb_gpu_scan_agg_nullkey and sdb_gpu_scan_agg_hash_nullkey
 * put every passing NULL-key row into one NULL group, whatever value the
 * row stores; sdb_gpu_scan_agg and sdb_gpu_scan_agg_hash have no place
 * for that group and return SDB_ERR_INVALID for such a column. */
int sdb_gpu_table_attach_validity(SdbGpuCtx* ctx, SdbGpuTable* tab,
                                  uint32_t col, const uint64_t* bits);

/* Raw variable-width string column (non-dictionary; VERDICT r1 missing
 * #5): rows strings stored as offsets[rows+1] byte offsets into blob
 * (offsets monotone, offsets[rows] == blob_len; bytes arbitrary incl.
 * NUL — comparisons are lexicographic on unsigned bytes, i.e. memcmp
 * order, which for UTF-8 equals code-point order). Up to 4 slots per
 * table, independent of the i64/f32 column list. */
int sdb_gpu_table_attach_strcol(SdbGpuCtx* ctx, SdbGpuTable* tab,
                                uint32_t slot, const uint64_t* offsets,
                                const uint8_t* blob, uint64_t blob_len);

/* Evaluate a string predicate over slot `slot` into a device-resident
 * row bitmask (bit r set = row matches). op: LT / GE / BETWEEN / EQ
 * (lexicographic vs lo[/hi]) or SDB_PRED_PREFIX (starts-with lo).
 * Literals are byte strings up to 63 bytes. The mask is then consumed by
 * scans via a predicate {col: slot, op: SDB_PRED_STRMASK}. Recompute the
 * mask before reuse with a different predicate (one mask per slot). */
int sdb_gpu_strpred_mask(SdbGpuCtx* ctx, SdbGpuTable* tab, uint32_t slot,
                         SdbPredOp op, const uint8_t* lo, uint32_t lo_len,
                         const uint8_t* hi, uint32_t hi_len);

/* ---- SUFFIX, CONTAINS, LIKE, negation and mask combination ----
 *
 * Everything is byte-wise, like the rest of the string slots: NUL is an
 * ordinary byte and matching is case sensitive.
 *
 * SDB_PRED_SUFFIX (row ends with lo) and SDB_PRED_CONTAINS (lo occurs in the
 * row) take their literal in lo, 0..63 bytes; hi is ignored. The empty
 * literal matches every well-formed row. sdb_gpu_strpred_mask accepts them
 * too.
 *
 * sdb_gpu_strpred_mask_ex is sdb_gpu_strpred_mask plus `flags`
 * (sdb_gpu_strpred_mask(...) == sdb_gpu_strpred_mask_ex(..., 0)):
 *
 *   SDB_STRPRED_NEGATE  the row result is inverted, for well-formed rows
 *                       only: a malformed FSST row (below) still matches
 *                       nothing, negated or not. String slots hold no NULLs,
 *                       so over well-formed rows NEGATE is plain complement.
 *   SDB_STRPRED_AND     the (possibly negated) result is AND-ed / OR-ed into
 *   SDB_STRPRED_OR      the slot's current mask instead of replacing it, so
 *                       `s >= 'a' AND s NOT LIKE '%bot%'` needs one slot.
 *                       Both bits together are SDB_ERR_INVALID, and so is
 *                       either on a slot whose mask was never computed since
 *                       its attach.
 *
 * Any other bit is SDB_ERR_INVALID. Bits of the last mask word at rows >=
 * rows stay 0 in every mode. A rejected call launches nothing and leaves
 * the slot's mask as it was.
 *
 * sdb_gpu_strpred_like evaluates a LIKE pattern of up to
 * SDB_LIKE_PATTERN_MAX bytes. A row matches iff the WHOLE row matches the
 * pattern:
 *   - '%' matches any byte sequence, the empty one included; consecutive
 *     '%' collapse;
 *   - the escape byte (escape = 0..255, or -1 for none) makes the byte after
 *     it literal, whatever that byte is;
 *   - every other byte is literal.
 * So '' matches only the empty row and '%' every well-formed row. These are
 * SDB_ERR_INVALID:
 *   - an escape as the last pattern byte;
 *   - an unescaped '_'. SQL's '_' stands for one CHARACTER and this library
 *     compares BYTES: a byte-wise '_' would be silently wrong on UTF-8 data
 *     (one code point is 1..4 bytes), so it is rejected rather than
 *     approximated. Escape it to match the byte 0x5f;
 *   - pattern_len > SDB_LIKE_PATTERN_MAX;
 *   - more than SDB_STRLIT_MAX (63) literal bytes in total, counted after
 *     the escapes are removed;
 *   - escape outside -1..255, or escape == '%'.
 * flags are those of sdb_gpu_strpred_mask_ex.
 *
 * Matching is leftmost-greedy over the pattern's literal segments (the runs
 * between '%'), which decides LIKE exactly; serenedb_amd/csrc/sdb_like.h is
 * the one matcher, compiled into the kernels and into libsdb_host.so
 * (sdb_host_like_prog_size / sdb_host_like_compile / sdb_host_like_match).
 *
 * Test hook: the environment variable SDB_LIKE_ROWWISE=1 (read per call)
 * makes a raw slot use the row-wise kernel where the cooperative
 * substring kernel would run (one unanchored segment: CONTAINS, LIKE
 * '%x%'). The masks are identical. Not for production use. */
#define SDB_STRLIT_MAX 63
#define SDB_LIKE_PATTERN_MAX 255
#define SDB_STRPRED_NEGATE 1u
#define SDB_STRPRED_AND 2u
#define SDB_STRPRED_OR 4u

int sdb_gpu_strpred_mask_ex(SdbGpuCtx* ctx, SdbGpuTable* tab, uint32_t slot,
                            SdbPredOp op, const uint8_t* lo, uint32_t lo_len,
                            const uint8_t* hi, uint32_t hi_len,
                            uint32_t flags);

int sdb_gpu_strpred_like(SdbGpuCtx* ctx, SdbGpuTable* tab, uint32_t slot,
                         const uint8_t* pattern, uint32_t pattern_len,
                         int32_t escape /* 0..255, or -1 = none */,
                         uint32_t flags);

/* FSST-style compressed string slot (SURVEY.md 8f row 3 "dict/FSST"):
 * rows hold code streams — code c < nsym expands to symbol bytes
 * symbols[sym_offsets[c]..sym_offsets[c+1]) (1..8 bytes each, nsym <=
 * 254, total symbol bytes <= 2048); code 255 escapes the next literal
 * byte. offsets[rows+1] index the ENCODED blob. Predicates on such a
 * slot (same sdb_gpu_strpred_mask call) decode on the fly against the
 * plain-byte literal — semantics identical to the uncompressed slot.
 * A malformed row (a code >= nsym, or an escape as its last byte) is
 * detected before any read past it: it matches no predicate at all,
 * PREFIX "" and GE "" included, and in sdb_gpu_scan_agg_hash_str all such
 * rows form one group whose key is 0x8000000000000001. */
int sdb_gpu_table_attach_strcol_fsst(SdbGpuCtx* ctx, SdbGpuTable* tab,
                                     uint32_t slot,
                                     const uint64_t* offsets,
                                     const uint8_t* enc_blob,
                                     uint64_t enc_len,
                                     const uint8_t* symbols,
                                     const uint32_t* sym_offsets,
                                     uint32_t nsym);

/* One predicate of a scan. The column's type decides which literal pair a
 * compare (LT, GE, BETWEEN, EQ) reads: an I64 or I64_FOR column reads
 * ilo / ihi, an F32 column reads flo / fhi; the other pair is ignored.
 * ihi / fhi matter to BETWEEN only.
 *
 * The f32 compares are IEEE-754 compares carried out in f32:
 *   - a NaN in the column or in a literal fails LT, GE, BETWEEN and EQ
 *     (so BETWEEN with a NaN bound, and EQ NaN, are empty);
 *   - -0.0 equals +0.0, as a value and as a literal;
 *   - subnormals are not flushed: they are distinct from zero and from
 *     each other, in the column and in the literals;
 *   - +-inf compare as the extremes; BETWEEN with lo > hi is empty.
 * This is the order of a compare, not the total order MIN_F32 / MAX_F32 and
 * the top-n use (where NaN is greatest and -0.0 < +0.0).
 * tests/f32_matrix.py pins each of these on every scan path. */
typedef struct SdbPredSpec {
  uint32_t col;
  SdbPredOp op;
  int64_t ilo, ihi;
  float flo, fhi;
} SdbPredSpec;

/* Aggregates. Every op but COUNT(*) reads column `col` and skips NULL
 * values (a cleared validity bit), as SUM always has.
 *
 * COUNT_COL takes a column of any type (I64, I64_FOR or F32) and counts
 * the passing rows whose value is not NULL; with no validity plane
 * attached it equals COUNT(*).
 *
 * MIN_I64 / MAX_I64 take an i64 or FoR column, MIN_F32 / MAX_F32 an f32
 * column. The f32 order is bitwise deterministic whatever order the
 * device atomics run in: every NaN is first canonicalised to the positive
 * quiet NaN 0x7FC00000 (so a NaN with the sign bit set lands at the top,
 * not the bottom), then values compare in IEEE total order
 *   -inf < ... < -0.0 < +0.0 < ... < +inf < NaN.
 * MAX is NaN as soon as one non-NULL NaN passes; MIN is NaN only if every
 * non-NULL passing value is NaN — the "NaN is the greatest value" rule of
 * the DuckDB consumer being replaced; -0.0 < +0.0 is a deterministic
 * refinement of it.
 *
 * SUM_F64 widens each f32 value to f64 (exact, subnormals included) and
 * adds in f64 in an unspecified order. Over +-inf / NaN inputs the result
 * is the IEEE sum: NaN if a NaN is summed or both infinities are, else the
 * infinity that is summed; the NaN's sign and payload are unspecified.
 *
 * A group with no non-NULL passing value (an empty group of the dense
 * scan, or one whose passing rows are all NULL in `col`) returns the op's
 * identity: MIN_I64 INT64_MAX, MAX_I64 INT64_MIN, MIN_F32 +inf, MAX_F32
 * -inf. SQL's NULL result is "COUNT_COL of the same column is 0": ask for
 * it alongside when the distinction matters.
 *
 * An op outside this enum, a column index >= ncols (for any op but
 * COUNT(*)), SUM_I64 / MIN_I64 / MAX_I64 on an f32 column and SUM_F64 /
 * MIN_F32 / MAX_F32 on a non-f32 column return SDB_ERR_INVALID before
 * anything is launched. */
typedef enum SdbAggOp {
  SDB_AGG_COUNT = 0,
  SDB_AGG_SUM_I64 = 1, /* exact wrap-around i64 sum */
  SDB_AGG_SUM_F64 = 2, /* f32 column summed in f64 */
  SDB_AGG_COUNT_COL = 3, /* COUNT(col): passing rows whose value is not NULL */
  SDB_AGG_MIN_I64 = 4,   /* i64 / FoR column */
  SDB_AGG_MAX_I64 = 5,
  SDB_AGG_MIN_F32 = 6,   /* f32 column */
  SDB_AGG_MAX_F32 = 7,
} SdbAggOp;

typedef struct SdbAggSpec {
  uint32_t col; /* ignored for COUNT */
  SdbAggOp op;
} SdbAggSpec;

/* group_key column must be i64 with values in [0, ngroups).
 * out layout: for each group g, naggs consecutive values. COUNT, SUM_I64,
 * COUNT_COL, MIN_I64 and MAX_I64 results are int64 stored in the i64 field
 * (f64 = 0); SUM_F64, MIN_F32 and MAX_F32 results are stored in the f64
 * field (i64 = 0) — for MIN/MAX the winning f32 widened to double, exact,
 * sign of zero preserved. */
typedef struct SdbAggResult {
  int64_t i64;
  double f64;
} SdbAggResult;

int sdb_gpu_scan_agg(SdbGpuCtx* ctx, SdbGpuTable* tab, uint32_t group_col,
                     uint32_t ngroups, const SdbPredSpec* preds,
                     uint32_t npreds, const SdbAggSpec* aggs, uint32_t naggs,
                     SdbAggResult* out /* ngroups*naggs */,
                     uint64_t* rows_passed);

/* General hash aggregate: ARBITRARY i64 group keys (sparse, any range) —
 * the north_star "hash-group-by with LDS-staged open-addressed buckets",
 * replacing the DuckDB PhysicalHashAggregate consumer
 * (duckdb_search_full_scan.cpp:2141-2171) for keys the dense perfect-hash
 * kernel (sdb_gpu_scan_agg) cannot take. Per-workgroup open-addressed LDS
 * table flushed once into a global open-addressed table; same predicate
 * pushdown and zonemap skips.
 *
 * max_groups bounds DISTINCT keys (<= 4M); more distinct keys (or a
 * pathological probe chain) returns SDB_ERR_OOM. Results: rows 0..
 * *ngroups_out sorted by key ascending; keys_out/out must hold max_groups
 * rows. Allocates/frees its device workspace per call (the dense kernel
 * remains the allocation-free hot path). */
int sdb_gpu_scan_agg_hash(SdbGpuCtx* ctx, SdbGpuTable* tab,
                          uint32_t group_col, uint64_t max_groups,
                          const SdbPredSpec* preds, uint32_t npreds,
                          const SdbAggSpec* aggs, uint32_t naggs,
                          int64_t* keys_out /* max_groups */,
                          SdbAggResult* out /* max_groups*naggs */,
                          uint64_t* ngroups_out, uint64_t* rows_passed);

/* ---- GROUP BY a nullable key ----
 * The two entries above with a NULL group, as the DuckDB hash-aggregate
 * consumer forms it: a passing row whose key validity bit is cleared
 * belongs to the NULL group. Its stored key is never an index, a hash key
 * or an aggregate input, so it may equal a live key or -1 or lie outside
 * [0, ngroups). Predicates on the key column keep their meaning (a compare
 * drops NULL-key rows, ISNULL keeps only them, NOTNULL empties the NULL
 * group), and so do aggregates over it: in the NULL group COUNT_COL(key)
 * and SUM_I64(key) are 0 and MIN / MAX return their identities.
 * *rows_passed counts NULL-key rows like any other passing row;
 * *null_rows is how many of them there were. A key column with no plane
 * attached is accepted too: *null_rows == 0 and the key groups are those
 * of the entry above.
 *
 * Dense: valid keys must lie in [0, ngroups), proved before launch from
 * the column's range over its VALID rows (one reduction per attached
 * plane, at the first such scan; a column with no valid row proves
 * trivially); a valid key outside returns SDB_ERR_INVALID.
 *
 * Hash: the NULL group is separate from every key group, key -1
 * included, and does not count against max_groups.
 *
 * Across shards the NULL group merges like any other group: sums add,
 * MIN_* take the min, MAX_* the max. */

/* out holds (ngroups + 1) * naggs results: row ngroups is the NULL group.
 * *null_rows = passing rows whose key is NULL (0 = no NULL group). */
int sdb_gpu_scan_agg_nullkey(SdbGpuCtx* ctx, SdbGpuTable* tab,
                             uint32_t group_col, uint32_t ngroups,
                             const SdbPredSpec* preds, uint32_t npreds,
                             const SdbAggSpec* aggs, uint32_t naggs,
                             SdbAggResult* out /* (ngroups+1)*naggs */,
                             uint64_t* rows_passed, uint64_t* null_rows);

/* keys_out/out as in sdb_gpu_scan_agg_hash (key groups only, ascending);
 * null_out[naggs] = the NULL group, identities/zeros if *null_rows == 0. */
int sdb_gpu_scan_agg_hash_nullkey(SdbGpuCtx* ctx, SdbGpuTable* tab,
                                  uint32_t group_col, uint64_t max_groups,
                                  const SdbPredSpec* preds, uint32_t npreds,
                                  const SdbAggSpec* aggs, uint32_t naggs,
                                  int64_t* keys_out /* max_groups */,
                                  SdbAggResult* out /* max_groups*naggs */,
                                  uint64_t* ngroups_out,
                                  uint64_t* rows_passed,
                                  SdbAggResult* null_out /* naggs */,
                                  uint64_t* null_rows);

#define SDB_MAX_GROUP_KEYS 4

/* ---- GROUP BY several key columns ----
 * The hash aggregate over a COMPOSITE key: 1..SDB_MAX_GROUP_KEYS columns,
 * each I64 or I64_FOR, each with or without a validity plane (F32 is
 * rejected; a repeated column is allowed and harmless). nkeys == 0, nkeys >
 * SDB_MAX_GROUP_KEYS, a column index >= ncols and every bad aggregate /
 * predicate case of the entries above return SDB_ERR_INVALID before
 * anything is launched.
 *
 * Group identity: a group is a distinct tuple, and in each position NULL is
 * a value of its own, equal only to NULL (SQL GROUP BY, and what the DuckDB
 * consumer does). The stored key of a NULL position is never an input: it
 * may be -1, an int64 extreme or a live key. Every distinct tuple counts
 * against max_groups, tuples with NULLs included — unlike
 * sdb_gpu_scan_agg_hash_nullkey, whose single NULL group is kept apart.
 * More tuples than max_groups (<= 4M) returns SDB_ERR_OOM. Predicates and
 * aggregates over a key column keep their meaning: a compare drops that
 * column's NULL rows, ISNULL / NOTNULL read its plane, STRMASK works as
 * above, and SUM / MIN / MAX / COUNT_COL over a key skip its NULL rows.
 *
 * Result order: tuples ascending, compared column by column as signed
 * int64, NULL last in its column. keys_out row n holds the nkeys values of
 * group n (0 in a NULL position), keynull_out[n] has bit j set when key j of
 * the group is NULL.
 *
 * How it is exact. No tuple is stored on the device and no thread waits
 * for another. Each passing row hashes its tuple to 64 bits,
 *   h = mix64(seed + 1)
 *   for j in 0..nkeys-1:  h = mix64(h ^ (null_j ? 0 : (uint64)key_j))
 *   h = mix64(h ^ nullmask)            bit j of nullmask = null_j
 *   h &= hash_mask                     all ones unless the hook below is set
 *   if (h == 2^64 - 1) h -= 1          the tables' empty marker
 * with mix64 the splitmix64 finaliser (x ^= x >> 30; x *= 0xbf58476d1ce4e5b9;
 * x ^= x >> 27; x *= 0x94d049bb133111eb; x ^= x >> 31), and upserts h into
 * the open-addressed tables of sdb_gpu_scan_agg_hash. Beside its naggs
 * accumulators every slot carries 2*nkeys + 2 witness words: per key the MIN
 * and the MAX of that key over the slot's rows where it is valid, plus the
 * bitwise OR and the bitwise AND of the rows' null masks. On readback the
 * host proves each slot: it holds exactly one tuple iff OR == AND and
 * min_j == max_j in every position not NULL, and the tuple is then (min_j)
 * with the mask. The proof is complete — two different tuples differ in
 * some position, in null-ness (OR != AND) or in value (min != max).
 *
 * If any slot fails the proof the whole scan repeats with the next seed, 0
 * through 3; if all four fail the call returns SDB_ERR_COLLISION. A wrong
 * answer is never returned. At 64 bits and 4M groups one seed collides with
 * probability about 5e-7, so callers do not see the error in practice.
 *
 * Test hook: the environment variable SDB_MK_HASH_BITS (1..64, read per
 * call) sets hash_mask = 2^bits - 1, so that the witness and the retry can
 * be exercised. Not for production use.
 *
 * Allocates / frees its device workspace per call, as the hash entries do. */
int sdb_gpu_scan_agg_hash_multi(SdbGpuCtx* ctx, SdbGpuTable* tab,
                                const uint32_t* group_cols,
                                uint32_t nkeys /* 1..SDB_MAX_GROUP_KEYS */,
                                uint64_t max_groups,
                                const SdbPredSpec* preds, uint32_t npreds,
                                const SdbAggSpec* aggs, uint32_t naggs,
                                int64_t* keys_out /* max_groups*nkeys */,
                                uint32_t* keynull_out /* max_groups */,
                                SdbAggResult* out /* max_groups*naggs */,
                                uint64_t* ngroups_out,
                                uint64_t* rows_passed);

/* GROUP BY string keys over an attached raw or FSST string slot (the
 * reference hands text group-by to its DuckDB fork's hash aggregate —
 * result-level parity). Each row's decoded bytes hash with FNV-1a 64 on
 * device; the hash feeds the same hash-aggregate core; keys_out holds
 * the group hashes sorted ascending as signed i64 (the core's
 * deterministic result order; hash -1 routes via the core's neg_acc
 * path like any other -1 key). The caller resolves
 * hashes back to strings and must verify injectivity over the column's
 * distinct strings (the python wrapper does both; collisions are
 * detected, never silent). */
int sdb_gpu_scan_agg_hash_str(SdbGpuCtx* ctx, SdbGpuTable* tab,
                              uint32_t str_slot, uint64_t max_groups,
                              const SdbPredSpec* preds, uint32_t npreds,
                              const SdbAggSpec* aggs, uint32_t naggs,
                              int64_t* keys_out, SdbAggResult* out,
                              uint64_t* ngroups_out,
                              uint64_t* rows_passed);

/* ---- ORDER BY col [DESC] LIMIT k over the scan ----
 * The row-returning half of the scan operator: SELECT ... WHERE preds ORDER
 * BY order_col [DESC] LIMIT k, DuckDB's TopN over FullScanner::Scan ("the
 * latest 100 events matching a filter"). order_col is I64, I64_FOR or F32.
 * Predicates are exactly those of sdb_gpu_scan_agg_hash: up to 4, AND-ed;
 * compares drop NULLs, ISNULL / NOTNULL read the plane, STRMASK consumes a
 * slot mask.
 *
 * The result is the first min(k, rows passing) of the passing rows in the
 * total order (NULL class, value, row ascending):
 *   - i64 values order as signed integers; f32 values in the library's total
 *     order, every NaN canonicalised:
 *       -inf < ... < -0.0 < +0.0 < ... < +inf < NaN;
 *   - SDB_TOPN_DESC reverses the value order only;
 *   - ties are always by row ascending — a deterministic refinement of an
 *     unspecified tie order, as (segment, doc) is for the BM25 top-k;
 *   - a row whose order-column validity bit is cleared is NULL whatever it
 *     stores. All passing NULL rows rank after every value (NULLS LAST, in
 *     both directions, as DuckDB), or before every value under
 *     SDB_TOPN_NULLS_FIRST, and among themselves by row ascending.
 * rows_out[i] is the row number; vals_out[i] holds the value in the i64
 * field for i64 / FoR columns and in the f64 field (the f32 widened, exact)
 * for F32; a NaN returns as the canonical quiet NaN. NULL rows return zeros
 * with null_out[i] = 1. *n_out = rows returned; *rows_passed counts every
 * passing row. All three arrays hold k entries.
 *
 * k == 0, k > SDB_TOPN_MAX_K, order_col >= ncols, unknown flag bits and
 * every bad predicate case of the entries above return SDB_ERR_INVALID
 * before anything is launched, with the outputs untouched. An empty table or
 * an empty pass set is SDB_OK with *n_out = 0.
 *
 * How it is exact: an MSD radix select over order-preserving u64 rank codes
 * (11-bit digits, one histogram scan each) narrows the k-th code until the
 * rows at or above its prefix fit the candidate buffer; a collect pass
 * appends those (code, row) pairs and the host sorts them. When every digit
 * is resolved and the rows equal to the k-th code still do not fit, or when
 * NULL rows are needed, the row-order arm runs: members of that one class are
 * counted per row group, and only the row groups up to the last one needed
 * are collected, so the buffer never needs more than k + group_rows entries.
 * A candidate overflow returns SDB_ERR_OOM; never a wrong answer.
 *
 * Device workspace (histogram, candidate buffer, per-row-group counts) is
 * cached on the context and grown on demand: a repeated call allocates
 * nothing.
 *
 * Test hook: the environment variable SDB_TOPN_CAND_CAP (read per call)
 * replaces the default candidate capacity of 2^20 entries; the effective
 * value is max(value, k + group_rows) and is reported in stats->cand_cap. It
 * makes every arm reachable on a small table. Not for production use. */
#define SDB_TOPN_MAX_K 65536u
#define SDB_TOPN_DESC        1u   /* default ascending */
#define SDB_TOPN_NULLS_FIRST 2u   /* default NULLS LAST, in both directions (DuckDB) */

typedef struct SdbTopnStats {
  uint32_t hist_passes;        /* histogram scans run */
  uint32_t tie_arm;            /* 1 = the row-order arm ran */
  uint64_t candidates;         /* entries the collect pass appended */
  uint64_t cand_cap;           /* effective candidate capacity of this call */
  uint32_t rowgroups_skipped;  /* row groups skipped by the ORDER column's zonemap, all passes */
} SdbTopnStats;

int sdb_gpu_scan_topn(SdbGpuCtx* ctx, SdbGpuTable* tab, uint32_t order_col,
                      uint32_t flags, uint32_t k, const SdbPredSpec* preds,
                      uint32_t npreds, uint64_t* rows_out /* k */,
                      SdbAggResult* vals_out /* k */,
                      uint8_t* null_out /* k */, uint64_t* n_out,
                      uint64_t* rows_passed,
                      SdbTopnStats* stats /* may be NULL */);

/* The rest of the SELECT list: value and NULL flag of column `col` (any
 * type) at each of the n given rows, in the output convention above.
 * n <= 2^20; a row >= the table's rows returns SDB_ERR_INVALID, checked on
 * the host before anything is launched. */
int sdb_gpu_table_gather(SdbGpuCtx* ctx, SdbGpuTable* tab, uint32_t col,
                         const uint64_t* rows, uint64_t n,
                         SdbAggResult* out /* n */, uint8_t* null_out /* n */);

#ifdef __cplusplus
}
#endif
#endif /* SDB_GPU_H */
