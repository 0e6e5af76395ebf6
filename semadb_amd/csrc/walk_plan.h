// walk_plan.h -- which walk kernel serves a call, decided once: plan_walk() answers every question about a call's
// kernel, walk_launch.hip maps the plan to the instantiation, and the callers (search_batch.hip, build.hip) read from
// the same plan whether the bitsets must be cleared ahead.  HIP-free (tests/host/test_walk_plan.cpp).
#pragma once
#include "walk_args.h"

namespace sdb {

// k_greedy_search over PlainDist (one wave per query, float32 rows), the same with the float16 / the int8 first stage
// (SearchArgs::sketch), k_greedy_search_wide (a workgroup per query, for calls with few queries), k_greedy_search over
// PQLdsDist / PQGlobalDist (one wave; a table over 64 KB stays in device memory), k_greedy_search_pq2 (walker and
// merger), k_greedy_search_pqw (tables too large to sit beside a one-wave walk), k_greedy_search over BitDist
enum class WalkFamily : uint32_t { kPlain, kStageHalf, kStageInt8, kWide, kPqLds, kPqGlobal, kPqTwoWaves, kPqWide, kBits };
// the HBM bitset, HashVisited<kHashCap>, HashVisited<kHashCapPQ>, HashVisited16
enum class WalkVisited : uint32_t { kBitset, kHash, kHashPQ, kHash16 };

struct WalkPlan {
  bool bad_search_size = false;  // no kernel serves the call: searchSize outside 1..512 (walk_launch.hip has the message)
  WalkFamily family = WalkFamily::kPlain;
  WalkVisited visited = WalkVisited::kBitset;
  bool clear_bitsets = false;  // the caller zeroes the call's bitsets ahead of the launch (ClearAll, distset.go:101)
  int ng = -1;                 // NG; -1: the run-time-length kernel (query tile in LDS)
  bool l2 = false, filt = false, jaccard = false;
  int nreg = 2;                      // registers of the candidate array: 2 up to searchSize 128, else 8
  int waves = 1;                     // W
  int nl = 0, rt = 0, nlw = 0;       // kPqWide: tables per wave in LDS / in registers, the walker's in LDS
  bool split = false;                // kPqWide: the candidate array in a helper wave (search_kernel.h pqw_split_walker)
  uint32_t hash_limit = kHashLimit;  // SearchArgs::hash_limit as the kernel gets it
  uint32_t wide_pull = 0;            // SearchArgs::wide_pull as the kernel gets it
};

inline WalkPlan plan_walk(const SearchArgs &a, uint32_t nq) {
  WalkPlan p;
  if (a.hash_limit != 0 && a.hash_limit <= kHashLimit) p.hash_limit = a.hash_limit;
  if ((p.bad_search_size = a.search_size == 0 || a.search_size > 512)) return p;
  p.filt = a.filt_off != nullptr;
  p.nreg = a.search_size <= 128 ? 2 : 8;
  p.l2 = a.metric == SDB_METRIC_EUCLIDEAN;
  // An LDS visited set at all: the reference's searchSize range, filtered searches too (their result set takes a 4 KB
  // table beside it, visited_set.h kHashCapResult) -- no bitset clear per batch, no HBM atomic per edge.
  const bool small = a.search_size <= 96 && !a.prefer_bitset;
  // The set beside a code table: 16-bit cells (16 KB, six walks per CU) for up to 2^24 rows, 32-bit cells beyond.
  const WalkVisited beside_codes =
      (uint64_t)a.words_per_query * 32 <= (1u << 24) && !a.wide_hash ? WalkVisited::kHash16 : WalkVisited::kHashPQ;
  const bool plain_call = !a.vis_slots && !a.dcache && !a.start_ext_n;  // no build's visit log or distance table, no overflow list on the start node

  if (a.bq_codes) {  // binary quantizer with a threshold attached (binary.go:191-200): the query is 512 bytes of LDS
    p.family = WalkFamily::kBits;
    p.jaccard = a.bq_metric == SDB_METRIC_JACCARD;
    if (small) p.visited = beside_codes;
  } else if (a.pq_codes) {  // fitted product quantizer attached (product.go:250-277)
    const bool wide_m = a.pq_M == 128 || a.pq_M == 192 || a.pq_M == 256 || a.pq_M == 384;  // M <= 64: the table fits beside a one-wave walk
    if (wide_m && small && a.pq_narrow != 1 && !p.filt && a.pq_K <= 256 && a.pq_K % 32 == 0) {
      p.family = WalkFamily::kPqWide, p.visited = beside_codes, p.waves = 4;
      // M = 128 / 192: 15 tables per wave in LDS leave room for TWO queries per CU (M = 192: 643 k against 570 k QPS
      // at 10M x 768 with 32 + 16, one query per CU: profiles/r03_c4_10Mx768_pq.log); SDB_TUNE_PQ_NARROW = 2: the latter
      const bool one_per_cu = a.pq_narrow == 2;
      switch (a.pq_M) {
        case 128: p.nl = one_per_cu ? 32 : 15, p.rt = one_per_cu ? 0 : 17; break;
        case 192: p.nl = one_per_cu ? 32 : 15, p.rt = one_per_cu ? 16 : 33; break;
        case 256: p.nl = 32, p.rt = 32; break;
        // M = 384: eight waves with M = 192's per-wave layout, the walker 24 + 24 (129 tables in LDS: with the
        // 32-bit-cell visited set 162 064 of the 162 816 bytes a workgroup may ask for)
        default: p.nl = 15, p.rt = 33, p.waves = 8; break;
      }
      p.nlw = p.waves == 8 ? 24 : p.nl;
      // (M = 192 at 2M x 768: 1.050 -> 0.989 ms per batch; SDB_TUNE_PQ_NARROW = 3 keeps the walker-does-everything form)
      p.split = p.waves == 4 && p.nl == 15 && a.pq_narrow != 3 && plain_call;
    } else {
      // M*K <= 2048 entries next to the visited set (M = 32's 32 KB LUT leaves room for three walks per CU beside the
      // 16 KB table: 0.95 M QPS against 1.31 M on the bitset at five)
      if (small && a.pq_lut_in_lds && (size_t)a.pq_M * a.pq_K <= 2048) p.visited = beside_codes;
      // two waves per query: plain unfiltered searches; SDB_TUNE_PQ_NARROW = 1 keeps the one-wave kernel
      if (p.visited != WalkVisited::kBitset && a.pq_narrow != 1 && !p.filt && plain_call)
        p.family = WalkFamily::kPqTwoWaves, p.waves = 2;
      else
        p.family = a.pq_lut_in_lds ? WalkFamily::kPqLds : WalkFamily::kPqGlobal;
    }
  } else {
    switch (a.ng) {  // the query in registers
      case 0: case 1: case 2: case 3: case 4: case 6: case 8: case 12: case 16: case 24: p.ng = (int)a.ng; break;
      default: break;
    }
    if (p.ng >= 0 && small) p.visited = WalkVisited::kHash;
    // The workgroup-per-query walk (walk_args.h kWideMaxQueries; the build's warm-up rounds come here too).  257 .. 512
    // queries: faster than one wave per query for rows of up to 384 floats only (d = 384: 0.56 against 0.65 ms; 512:
    // 0.98 against 0.78; 768: 1.20 against 1.05; profiles/r05_latency.json)
    const bool wide = p.ng >= 1 && p.ng <= 8 && p.visited == WalkVisited::kHash && a.wide_mode != 1 &&
                      (a.wide_mode == 2 || nq <= (a.ng <= 3 ? 2 : 1) * kWideMaxQueries);
    // The two-precision hop: batch walks, plain and -- where the caller handed the copy to a filtered call
    // (SDB_TUNE_SKETCH_FILTERED) -- filtered.  A filtered call keeps the hop up to searchSize 128 (the two array
    // registers of the kernel), also at 97 .. 128, where plain calls take the bitset kernel: the LDS sets spill to the
    // query's bitsets by themselves (HashVisited::spill clears the bitset first), so no bitset is cleared ahead.
    const bool staged = a.stage != Stage::kNone && !a.vis_slots && !a.dcache && a.tail == 0 && a.search_size <= 128 &&
                        stage_shape(p.ng) && !wide && (p.visited == WalkVisited::kHash || (p.filt && !a.prefer_bitset));
    if (wide) {
      p.family = WalkFamily::kWide;
      // up to 256 queries: 16 waves per query (one workgroup per CU); up to 512: 8 waves (two per CU: 0.56 ms per call
      // against 0.66 for one wave per query and 0.78 for 16 waves).  Rows of 1 024 floats: at sixteen waves the query
      // and two pairs of rows spill 17 .. 57 registers, so every small call of that shape takes eight (214, none spilled)
      p.waves = p.ng != 8 && (nq <= kWideMaxQueries || kWideWaves != 16) ? kWideWaves : 8;
      // a workgroup per CU at most: the other waves work ahead on the row the walk expands next
      p.wide_pull = (p.waves == 16 || p.ng == 8) && nq <= kWideAheadQueries ? 2u : 0u;
    } else if (staged) {
      p.visited = WalkVisited::kHash;
      // the int8 first stage (SDB_TUNE_SKETCH = 3, 4): plain calls of cosine / dot tables (choose_stage hands it to no other)
      p.family = a.stage == Stage::kInt8 && stage_int8(p.ng, p.l2, false) ? WalkFamily::kStageInt8 : WalkFamily::kStageHalf;
      if (p.family == WalkFamily::kStageInt8) p.filt = false;
    }
  }
  p.clear_bitsets = p.visited == WalkVisited::kBitset;  // every LDS set clears its query's bitset itself if it spills
  return p;
}

}  // namespace sdb
