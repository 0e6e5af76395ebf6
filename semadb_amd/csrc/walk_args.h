// walk_args.h -- what a walk is called with: SearchArgs (the walk kernels' kernarg layout), the two-precision hop's
// stages and the constants the routing reads.  HIP-free: walk_plan.h decides a call's kernel from these alone, and
// tests/host/test_walk_plan.cpp compiles both as plain C++.
#pragma once
#include <cstdint>

#include "../../include/semadb_amd.h"

#ifdef __HIPCC__
#include <hip/hip_runtime.h>
#else
struct uint2;  // SearchArgs::dcache's element (HIP's vector type in a HIP build); a host build only carries the pointer
#endif

namespace sdb {

// The two-precision hop's first stage: which copy of the rows a walk reads first (SearchArgs::sketch), if any.
enum class Stage : uint32_t { kNone = 0, kHalf = 1, kInt8 = 2 };
// Which tables and calls get which stage -- stated here once, for the launcher, the index and the kernels alike.
// A stage at all: the group counts whose float16 rounds fit the walk's registers.
constexpr bool stage_shape(int ng) { return ng == 1 || ng == 2 || ng == 3 || ng == 4 || ng == 6; }
// Rows asked for ahead: rows of up to 384 floats, where all 64 edges' copy rows fit the register file.
constexpr bool stage_ahead(int ng) { return stage_shape(ng) && ng <= 3; }
// The int8 stage: those tables, cosine / dot, plain calls (a filtered call reads the float16 copy or none).
constexpr bool stage_int8(int ng, bool euclidean, bool filtered) { return stage_ahead(ng) && !euclidean && !filtered; }

struct SearchArgs {
  const float *slab;
  const uint32_t *adj;
  const uint64_t *ids;
  uint32_t *bitsets;
  uint32_t words_per_query;
  const float *queries;  // [nq][dim] original layout
  uint32_t dim, nblk, ng, tail, ld;
  uint32_t start_slot;
  // the start node's edges beyond its 64-entry row (index.h h_start_ext), kNoSlot-padded to whole chunks of 64
  const uint32_t *start_ext;
  uint32_t start_ext_n;
  uint32_t search_size;
  uint32_t limit;
  int metric;
  uint64_t *out_ids;
  float *out_dists;
  uint32_t *out_counts;
  uint32_t *tr_ndist, *tr_nhop, *tr_nedges;
  uint64_t *tr_visit;
  uint32_t visit_cap;
  // build path: the visit log as (slot, dist), in visit order
  uint32_t *vis_slots;
  float *vis_dists;
  uint32_t *vis_count;
  uint32_t vis_cap;
  // product-quantized store (product.go:238-277): per-query LUT [nq][M*K] and per-slot codes [n][M]
  const float *pq_lut;
  const uint8_t *pq_codes;
  uint32_t pq_M, pq_K;
  // != NULL: the code rows of every node's neighbours behind its adjacency row, [rows][64][M] (index.h GraphCopy::adjcodes), for
  // the copy of the graph `adj` points at
  const uint8_t *adj_codes;
  uint32_t adj_rows;  // rows of `adj` (what tells an adjacency row from a chunk of the start node's overflow list)
  uint32_t pq_lut_in_lds;  // != 0: the kernel copies its LUT into LDS first
  uint32_t pq_narrow;      // 1: never a multi-wave walk (k_greedy_search_pqw, k_greedy_search_pq2); 2: the one-query-per-CU variant of the former for M = 192

  // filtered search (search.go:33-51,93-95): per query CSR of seeds (<= searchSize slots, ascending id
  // order) and of the whole filter as ascending slots; rbitsets = the result set's own visited set
  const uint32_t *seed_off, *seeds, *filt_off, *filt_slots;
  // filter lists resolved on the device (search_batch.hip k_filter_resolve): the counts are not offset differences then
  // (segments keep the caller's offsets, unknown ids leave gaps at their ends); NULL: offset differences
  const uint32_t *seed_cnt, *filt_cnt;
  // != NULL: Contains (:93) is answered from the filter's IDS -- the uploaded lists, strictly ascending, at filt_off's
  // offsets -- with the id of the expanded node (ids[slot]), for tables where ascending ids are not ascending slots
  // (an id that was deleted and inserted again sits behind larger ids); filt_slots is not read then
  const uint64_t *filt_ids;
  uint32_t *rbitsets;
  // build path, full-precision store: every evaluated (slot, distance) also goes into the query's
  // direct-mapped table of 2^(32 - dcache_shift) entries (last writer wins); the back-edge prunes of the
  // round look their pair distances up there (build.hip BuildArgs::dcache).  NULL: not collected.
  uint2 *dcache;
  uint32_t dcache_shift;
  unsigned long long *totals;  // build path: [0] += n_dist, [1] += n_edges of every query (sdb_index_build_stats)
  uint32_t prefer_bitset;  // != 0: never use the LDS hash visited set (large build rounds)
  uint32_t wide_hash;      // != 0: quantized store keeps the 32-bit-cell set (HashVisited) instead of HashVisited16
  uint32_t hash16_probes;  // test knob: buckets a key of HashVisited16 may try (0 = all 15); fewer make the `stuck` spill common
  uint32_t hash_limit;     // ids the LDS hash set may hold before the query falls back to its bitset
  uint32_t wide_mode;      // the workgroup-per-query walk: 0 = calls of up to kWideMaxQueries queries, 1 = never, 2 = always
  uint32_t wide_pull;      // 2: that walk's other waves work ahead on the row the walk expands next (PlainWideDist); 0: they only share a hop's rows
  // Two-precision hop (index.h d_sketch; SDB_TUNE_SKETCH): a float16 copy of the slab, same element order, rows of
  // `ld` halves.  A neighbour whose float16 distance lies above the candidate array's last distance by more than the
  // bound on |float16 distance - the reference's float32 distance| is discarded by AddWithLimit whatever its exact
  // distance is (distset.go:184; the distance is never looked at again), so only the others are read in float32.
  const void *sketch;                // Stage::kHalf: rows of `ld` halves; Stage::kInt8: rows of `ld` bytes
  const float *sketch_norm;          // [rows] ||y16||^2 of every row (euclidean tables: d16 = ||q16||^2 + ||y16||^2 - 2 q16.y16)
  float sk_emax, sk_ymax;            // max over the rows of ||y - y16|| and of ||y16|| (k_sketch_rows), rounded up; the int8 copy's likewise
  Stage stage;                       // this call's first stage, decided once where the arguments are filled (search_batch.hip choose_stage); kNone: `sketch` is NULL
  float sk8_scale;                   // the int8 copy's scale s: y8 = clamp(rint(y / s), -127, 127)
  uint32_t sk_audit;                 // != 0: evaluate everything exactly as well and count decisions the exact distance contradicts
  unsigned long long *sk_counters;   // [0] += neighbours discarded on their float16 distance, [1] += contradicted ones (audit)
  // binary-quantized store (binary.go:187-200): per-slot codes [n][W] of 64-bit words, the threshold [dim] the walk
  // encodes its query with, and the bit metric (SDB_METRIC_HAMMING / SDB_METRIC_JACCARD); bq_codes == NULL: none
  const uint64_t *bq_codes;
  const float *bq_thr;
  uint32_t bq_W, bq_metric;
};

// keys an LDS visited set may hold before it spills to the query's bitset (visited_set.h HashVisited; any CAP:
// limit * CAP / 8192)
constexpr uint32_t kHashLimit = 6000;

// The workgroup-per-query walk (walk_dist_rows.h PlainWideDist) for calls with few queries: a 256-query call is one
// workgroup per CU.  Waves per workgroup, measured at 1M x 384 (tools/bench_latency.py, whole call of 1 / 256 queries;
// one wave per query: 0.538 / 0.598 ms): 2 waves 0.78 / 0.86, 4 waves 0.536 / 0.607, 8 waves 0.410 / 0.469, 16 waves
// 0.361 / 0.416 ms -- a hop's ~50 rows are 2 pairs per wave then, one short burst of loads each.  With the helpers
// pulling the likely next hop's rows through L2 (PlainWideDist::pull_ahead): 0.336 / 0.419 ms; 0.371 at 128 queries
// (0.408 without); with the helpers COMPUTING that hop's distances ahead (compute_ahead): 0.316 / 0.405 ms, 0.362 at 128.
// Past 256 queries eight waves per query (0.58 ms at 512 against 0.66 for one wave per query, 0.80 for sixteen).  Plain store, query in registers; the build's warm-up rounds (up to 512 points) included.
constexpr uint32_t kWideMaxQueries = 256;
#ifndef SDB_WIDE_AHEAD
#define SDB_WIDE_AHEAD 256
#endif
constexpr uint32_t kWideAheadQueries = SDB_WIDE_AHEAD;
#ifndef SDB_WIDE_WAVES
#define SDB_WIDE_WAVES 16
#endif
constexpr int kWideWaves = SDB_WIDE_WAVES;

}  // namespace sdb
