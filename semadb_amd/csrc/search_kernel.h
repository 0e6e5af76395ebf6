// search_kernel.h -- K2: GPU-resident greedySearch, one wavefront per query.
//
// Restates shard/index/vamana/search.go:9-102 (greedySearch) on top of
// shard/index/vamana/distset.go:166-200 (DistSet.AddWithLimit) with bit-identical distances
// (dist_core.h), so result ids, distances, visit order, n_dist and n_hop equal the reference's.
//
// Wave-level mapping (64 lanes, one wave per workgroup, no workgroup barriers):
//   * candidate set S (cap = searchSize): a sorted array held in VGPRs, entry e in lane e%64 of
//     register e/64; the `visited` flag rides in bit 31 of the slot word.
//   * one hop: wave-uniform pick of the first unvisited entry -> one coalesced 256-byte read of
//     its adjacency row (lane j = edge j, edge order preserved) -> per-lane test-and-set in the
//     query's visited set (an exact hash set in LDS, or the HBM bitset; the ids of one row are
//     distinct) -> distances for the new neighbours, two candidates per wave instruction (one per
//     32-lane half), 16-byte row loads, up to U pairs of rows in flight -> AddWithLimit for the
//     neighbours that beat the current tail, in edge order (the tail only shrinks, so a neighbour
//     that fails the current threshold can never pass a later one).
//   * with one wave per SIMD every instruction of any kind costs an issue slot, so the hop is written
//     for instruction count: the reduce tree is DPP adds (dist_core.h), row slots reach the lanes
//     through a rank-compacted LDS list, a row address is one 64-bit mad (PlainDist::hop_fast).
#pragma once
#include "bq.h"
#include "index.h"
#include "walk_args.h"
#include "wave_dist.h"
#include <type_traits>

namespace sdb {

// The kernel's own arguments once more, through a pointer the optimiser cannot see through.  Every walk kernel takes
// its SearchArgs by value as its first parameter, i.e. at offset 0 of the kernarg segment; a field read through `a` is
// loaded in the kernel's first instructions and -- with ~60 fields against ~100 SGPRs -- parked in a VGPR lane until it
// is used.  A field that only the hop's stage or the epilogue reads is read through this view: one scalar load
// (s_load_dword*) at the point of use.  The view keeps the kernarg segment's address space (constant, 4): laundered
// into a generic pointer, as it once was, every field read became a vector flat_load of a uniform address behind a
// full s_waitcnt, and every pointer read through it a generic one (flat loads, stores and atomics).  A pointer field
// read through the view is generic by its declared type; as_global() says what it is -- device memory -- before it
// is dereferenced (tests/test_stage_load_schedule.py: no flat_ instruction in any walk kernel).
typedef const __attribute__((address_space(4))) SearchArgs ColdArgs;
__device__ __forceinline__ ColdArgs &cold_args(const SearchArgs &) {
  uintptr_t p = (uintptr_t)(ColdArgs *)__builtin_amdgcn_kernarg_segment_ptr();
  asm volatile("" : "+s"(p));
  return *(ColdArgs *)p;
}

}  // namespace sdb

// The walk's parts by concern, each on what stands above it; this header is the one a .hip file includes.
#include "walk_stage.h"       // the two-precision hop's first stage
#include "walk_dist_rows.h"   // distance policies over stored rows
#include "cand_array.h"       // the candidate array's operations
#include "visited_set.h"      // the visited-set policies, VisitedFor
#include "walk_dist_codes.h"  // distance policies over codes

namespace sdb {

// A walk's counters, by the wave that walked: the trace rows the caller asked for, and the build path's totals.  `e`: the
// caller's view of the arguments, as with write_results; edges_out: what goes to tr_nedges (the measurement builds
// report another figure there).
template <class Args>
__device__ __forceinline__ void write_walk_counters(uint32_t q, int lane, uint32_t n_dist, uint32_t n_hop, uint32_t n_edges, uint32_t edges_out, Args &e) {
  if (lane != 0) return;
  if (e.tr_ndist) as_global(e.tr_ndist)[q] = n_dist;
  if (e.tr_nhop) as_global(e.tr_nhop)[q] = n_hop;
  if (e.tr_nedges) as_global(e.tr_nedges)[q] = edges_out;
  if (e.vis_count) as_global(e.vis_count)[q] = n_hop;
  if (e.totals) {  // one of 64 copies of the counters (index.h kStatCopies)
    unsigned long long *t = e.totals + (q & 63u) * 16u;
    atomicAdd(t, (unsigned long long)n_dist), atomicAdd(t + 1, (unsigned long long)n_edges);
  }
}

// greedySearch for one query by one wavefront.  RVis: the visited set of the filtered search's result set.
template <class Dist, int NREG, bool FILT, class Visited, class RVis>
__device__ __forceinline__ void search_body(const SearchArgs &a, const uint32_t q, const int lane, Dist &dist,
                                            Visited &vis, RVis &rvis) {
  uint32_t cid[NREG];
  float cd[NREG];
#pragma unroll
  for (int r = 0; r < NREG; r++) cid[r] = kNoSlot, cd[r] = 0.0f;
  int len = 0;
  const int cap = (int)a.search_size;
  uint32_t n_dist = 0, n_hop = 0, n_edges = 0;
  constexpr bool kStaged = Dist::kStage != Stage::kNone;  // the two-precision hop
  uint32_t n_sk_bad = 0;  // two-precision hop, audited: discards the exact distance contradicts
  uint32_t n_sk_out = 0;  // ... its neighbours discarded on their first-stage distance
  __shared__ uint32_t s_scatter[2 * NREG * 64];  // add_with_limit_merge scratch

  // filtered search (search.go:33-51): resultSet = DistSet(cap k) with its own visited set
  uint32_t rid[FILT ? NREG : 1];
  float rd[FILT ? NREG : 1];
  int rlen = 0;
  const int rcap = (int)a.limit;
  const uint32_t *__restrict__ fsorted = nullptr;
  const uint64_t *__restrict__ fids = nullptr;
  uint32_t nfilt = 0;
  if constexpr (FILT) {
#pragma unroll
    for (int r = 0; r < NREG; r++) rid[r] = kNoSlot, rd[r] = 0.0f;
    fsorted = a.filt_slots + a.filt_off[q];
    nfilt = a.filt_cnt ? a.filt_cnt[q] : a.filt_off[q + 1] - a.filt_off[q];
    if (a.filt_ids) fids = a.filt_ids + a.filt_off[q], nfilt = a.filt_off[q + 1] - a.filt_off[q];
    // seeds: the first <= searchSize filter ids in ascending id order that exist (:41-48)
    const uint32_t s0 = a.seed_off[q], ns = a.seed_cnt ? a.seed_cnt[q] : a.seed_off[q + 1] - s0;
    for (uint32_t base = 0; base < ns; base += 64) {
      const uint32_t j = base + lane;
      const bool has = j < ns;
      const uint32_t slot = has ? a.seeds[s0 + j] : kNoSlot;
      // searchSet.Add (:49): CheckAndVisit, distance, plain append -- NOT sorted
      dist.prefetch(a, slot, has);
      const bool isnew = vis.test_and_set(has, slot, lane);
      const uint64_t pend = __ballot(isnew);
      n_dist += (uint32_t)__popcll(pend);
      const float mydist = dist.hop(a, slot, pend, lane);
      for (uint64_t t = pend; t; t &= t - 1) {
        const int j0 = __ffsll((unsigned long long)t) - 1;
        const uint32_t id = rl(slot, j0);
        const float d = rlf(mydist, j0);
#pragma unroll
        for (int r = 0; r < NREG; r++)
          if ((len >> 6) == r && lane == (len & 63)) cid[r] = id, cd[r] = d;
        len++;
      }
      // resultSet.AddWithLimit(filterPoints...) (:50): its own CheckAndVisit, distances evaluated again
      const bool rnew = rvis.test_and_set(has, slot, lane);
      const uint64_t rpend = __ballot(rnew);
      n_dist += (uint32_t)__popcll(rpend);
      add_with_limit_lanes(rid, rd, rlen, rcap, slot, mydist, rpend, lane);
    }
  }

  // ---- searchSet.AddWithLimit(startNode)  search.go:57-61
  {
    const uint32_t s = a.start_slot;
    const bool snew = vis.test_and_set(lane == 0, s, lane);
    if (__ballot(snew)) {
      const float d = dist.one(a, s, lane);
      n_dist++;
      if (!(len == cap && d > list_tail(cd, cap))) list_insert(cid, cd, len, cap, s, d, lane);
    }
  }

#ifdef SDB_STAMPS  // diagnostic build only: where does a hop spend its cycles (never in the shipped library)
  unsigned long long st_adj = 0, st_atom = 0, st_vec = 0, st_ins = 0, st_t0 = 0;
  unsigned long long st_m[4] = {0, 0, 0, 0};  // inside the merge: preamble, <2-candidates path, per-point pass, scatter
  unsigned long long st_w[4] = {0, 0, 0, 0};  // Dist::kSpeculate: pick + guess, the marker's verdict, the late guess, naming the row
#define SDB_STAMP(acc)                                              \
  {                                                                 \
    unsigned long long _t = __builtin_amdgcn_s_memtime();           \
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");              \
    acc += _t - st_t0;                                              \
    st_t0 = _t;                                                     \
  }
#else
#define SDB_STAMP(acc)
#endif
  uint32_t spec_pid = kNoSlot, spec_nb = kNoSlot;  // Dist::kSpeculate: the row fetched ahead, and whose it is
  float spec_d = 0.0f;                             // ... and that candidate's distance
  bool have_marks = false;                         // ... and whether its neighbours have been through the visited set
  uint64_t mark_mask = 0;
#ifdef SDB_SPEC_STATS
  uint32_t n_spec_hit = 0;  // measurement builds: hops that found their row fetched ahead, reported in place of n_edges
#endif
  // ---- main loop search.go:65-98
  while (true) {
#ifdef SDB_STAMPS
    st_t0 = __builtin_amdgcn_s_memtime();
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#endif
    // the first unvisited entry :66-71.  (Written out here and for sel2 below, as it always was: as calls of one helper
    // the same loops cost the one-wave walks 0.4 % of a small call, profiles/walk_steps_ab.json call_sites.)
    int sel = -1;
#pragma unroll
    for (int r = 0; r < NREG; r++) {
      uint64_t m = __ballot((r * 64 + lane) < len && !(cid[r] & kVisBit));
      if (sel < 0 && m) sel = r * 64 + __ffsll((unsigned long long)m) - 1;
    }
    if (sel < 0) break;
    uint32_t pid = 0;
    float pdist = 0.0f;
#pragma unroll
    for (int r = 0; r < NREG; r++)
      if ((sel >> 6) == r) {
        pid = rl(cid[r], sel & 63);
        pdist = rlf(cd[r], sel & 63);
        if (lane == (sel & 63)) cid[r] |= kVisBit;  // :74
      }
    if (lane == 0) {  // visitedSet.AddAlreadyUnique :73
#ifndef SDB_STAMPS
      if (a.tr_visit && n_hop < a.visit_cap) a.tr_visit[(size_t)q * a.visit_cap + n_hop] = a.ids[pid];
#endif
      if (a.vis_slots && n_hop < a.vis_cap) {
        a.vis_slots[(size_t)q * a.vis_cap + n_hop] = pid;
        a.vis_dists[(size_t)q * a.vis_cap + n_hop] = pdist;
      }
    }
    n_hop++;
    uint64_t pid_id = 0;  // FILT by ids: asked for now, looked at after the hop
    if constexpr (FILT)
      if (fids) pid_id = a.ids[pid];

    // node.neighbours in edge order :77-91.  One pass per 64 edges: every node has one, except a start node
    // that carries an overflow list (index.h h_start_ext) -- its chunks follow in the same edge order, which
    // is all AddWithLimit(neighbours...) depends on.
    const uint32_t *__restrict__ rowp = a.adj + (size_t)pid * kAdjStride;
    uint32_t ext_left = pid == a.start_slot ? a.start_ext_n : 0u, ext_done = 0;
    // Dist::kSpeculate: is this hop's row the one named during the last hop (then its adjacency row is in spec_nb), and
    // who is first in line now -- this hop's own entry is marked already -- with its distance: the hop names either it
    // or a nearer new point once its distances are known (below)
    bool use_spec = false;
    const uint32_t *spec_rowp = nullptr;
    if constexpr (Dist::kSpeculate) {
      use_spec = pid == spec_pid;
      int sel2 = -1;
#pragma unroll
      for (int r = 0; r < NREG; r++) {
        const uint64_t m2 = __ballot((r * 64 + lane) < len && !(cid[r] & kVisBit));
        if (sel2 < 0 && m2) sel2 = r * 64 + __ffsll((unsigned long long)m2) - 1;
      }
      spec_pid = kNoSlot;
      spec_d = __int_as_float(0x7f800000);
#pragma unroll
      for (int r = 0; r < NREG; r++)
        if (sel2 >= 0 && (sel2 >> 6) == r) spec_pid = rl(cid[r], sel2 & 63) & ~kVisBit, spec_d = rlf(cd[r], sel2 & 63);
      if (spec_pid != kNoSlot) spec_rowp = a.adj + (size_t)spec_pid * kAdjStride;
      dist.speculation(use_spec, spec_rowp);
      SDB_STAMP(st_w[0])
      // the visited-set test of the row named last has been run ahead (PlainWideDist's marker): its verdict, or back out
      have_marks = false;
      if (dist.marked) {
        uint32_t cell;
        dist.take_marks(lane, mark_mask, cell);
        if (use_spec) have_marks = true, vis.credit((uint32_t)__popcll(mark_mask), lane);
        else vis.unmark((mark_mask >> lane) & 1ull, cell);
      }
      SDB_STAMP(st_w[1])
    }
    bool first_chunk = true;
    while (true) {
      dist.begin_row(a, rowp, lane);
      uint32_t nb;
      if (Dist::kSpeculate && first_chunk && use_spec) {
        nb = spec_nb;  // fetched during the hop before this one
#ifdef SDB_SPEC_STATS
        n_spec_hit++;
#endif
      } else {
        nb = rowp[lane];
      }
      const bool valid = nb != kNoSlot;
      n_edges += (uint32_t)__popcll(__ballot(valid));
#ifdef SDB_STAMPS
      if (!Dist::kSpeculate) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // charge the adjacency round trip to st_adj
#endif
      SDB_STAMP(st_adj)
      if constexpr (kStaged) dist.stage_begin(a, nb, valid, len == cap);
      else dist.prefetch(a, nb, valid);
      // (the audit flag: a scalar load issued with the copy rows and back long before the visited-set test is through --
      // read behind the stage's sums it was a memory round trip of its own on a wave with nobody to cover it)
      uint32_t audit = 0;
      if constexpr (kStaged) audit = cold_args(a).sk_audit;
      // CheckAndVisit distset.go:174 -- marks before any distance test
      bool isnew;
      if (Dist::kSpeculate && have_marks && first_chunk) isnew = (mark_mask >> lane) & 1ull;
      else isnew = vis.test_and_set(valid, nb, lane);
      uint64_t pend = __ballot(isnew);
      SDB_STAMP(st_atom)
      if (pend) {
        n_dist += (uint32_t)__popcll(pend);
        if constexpr (kStaged) {
          // two-precision hop: with the array full, the neighbours whose float16 distance is provably above every last
          // distance the array can have at their turn are discarded here; AddWithLimit would discard them one by one
          // (distset.go:184) and nothing else ever reads their distance.  Plain walk: the array is sorted, its last
          // distance only falls while this row's points are inserted, the threshold is the last distance as it is now.
          // Filtered walk: the array is unsorted and its last distance can RISE within the chunk; the threshold is the
          // maximum of its last min(k, cap) distances for the chunk's k new neighbours (list_tail_bound).
          if (len == cap) {
            const float tail_d = FILT ? list_tail_bound(cd, cap, __popcll(pend), lane) : list_tail(cd, cap);
            uint64_t out = 0;
            const uint64_t keep = dist.stage_keep(a, nb, pend, lane, tail_d, out);
            if (audit) {  // (rare path; the count goes out with the discarded count in the epilogue: the counters' address
                          // read here, a scalar load inside the hop, left the filtered euclidean walk at d = 384 with a dead
                          // 32-byte stack slot, i.e. a private segment)
              const float dx = dist.hop(a, nb, pend, lane);
              n_sk_bad += (uint32_t)__popcll(__ballot(((out >> lane) & 1ull) && !(dx > tail_d)));
            }
            n_sk_out += (uint32_t)__popcll(out);
            pend = keep;
          }
        }
        const float mydist = pend ? dist.hop(a, nb, pend, lane) : 0.0f;  // lane j: distance of edge j
        if constexpr (Dist::kPointDistances)
          if (a.dcache && ((pend >> lane) & 1ull))
            a.dcache[((size_t)q << (32 - a.dcache_shift)) + ((nb * 2654435761u) >> a.dcache_shift)] =
                make_uint2(nb, __float_as_uint(mydist));
#ifdef SDB_STAMPS
        asm volatile("" ::"v"(mydist));
#endif
        SDB_STAMP(st_vec)
        if constexpr (Dist::kSpeculate) {
          // With this hop's distances the next pick is no guess any more: it is the nearest of the new points when that
          // one is nearer than the candidate first in line (and gets into the array), else that candidate.  Known
          // BEFORE the points are inserted -- so the row to fetch and work ahead on is named now, and the insert below
          // runs beside that work.  (A tie or a NaN can still make it wrong; the next hop checks pid == spec_pid.)
          if (first_chunk) {
            if (ext_left == 0) {
              uint64_t nearer = __ballot(((pend >> lane) & 1ull) && mydist < spec_d);
              if (nearer) {
                int bj = -1;
                float bd = spec_d;
                for (; nearer; nearer &= nearer - 1) {
                  const int j = __ffsll((unsigned long long)nearer) - 1;
                  const float dj = rlf(mydist, j);
                  if (dj < bd) bd = dj, bj = j;
                }
                if (bj >= 0 && (len < cap || !(bd > list_tail(cd, cap)))) {
                  spec_pid = rl(nb, bj);
                  spec_rowp = a.adj + (size_t)spec_pid * kAdjStride;
                }
              }
            }
            // (the marker only when no overflow chunk follows: the walker's own tests of those must have the table to themselves)
            // its row, for the next hop: asked for HERE and not when the hop began -- a load in flight is waited for at
            // every workgroup barrier (the fence of __syncthreads), and the hop's handshake would stand still for it
            if (spec_rowp) spec_nb = spec_rowp[lane];
            SDB_STAMP(st_w[2])
            dist.ahead(a, spec_rowp, lane, vis.markable() && ext_left == 0);
            SDB_STAMP(st_w[3])
          }
        }
        // AddWithLimit over the new neighbours, in edge order distset.go:184-198
        if (!kStaged || pend) {  // (the two-precision hop may have discarded every new neighbour)
          if constexpr (FILT) add_with_limit_lanes(cid, cd, len, cap, nb, mydist, pend, lane);  // array may be unsorted
          // (fewer than 2 candidates are replayed one by one; the two-precision hop hands over ~5 points per hop, and a
          // threshold of 7 for it measured 0.756 against 0.729 ms)
#ifdef SDB_STAMPS
          else add_with_limit_merge<NREG, 2>(cid, cd, len, cap, nb, mydist, pend, lane, s_scatter, st_m);
#else
          else add_with_limit_merge<NREG, 2>(cid, cd, len, cap, nb, mydist, pend, lane, s_scatter);
#endif
        }
        SDB_STAMP(st_ins)
      } else {
        dist.skip(lane);
        if constexpr (Dist::kSpeculate)
          if (first_chunk) {  // no new point: the candidate first in line stays it
            if (spec_rowp) spec_nb = spec_rowp[lane];
            dist.ahead(a, spec_rowp, lane, vis.markable() && ext_left == 0);
          }
      }
      if constexpr (Dist::kSpeculate) first_chunk = false;
      if (__builtin_expect(ext_left == 0, 1)) break;
      rowp = a.start_ext + ext_done;
      ext_done += 64;
      ext_left = ext_left > 64 ? ext_left - 64 : 0;
    }
    if constexpr (FILT) {  // :93-95 resultSet.AddWithLimit(distElem.Point) when the node passes the filter
      if (fids ? filter_contains(fids, nfilt, pid_id, lane) : filter_contains(fsorted, nfilt, pid, lane)) {
        const bool rnew = rvis.test_and_set(lane == 0, pid, lane);  // CheckAndVisit of the result set
        if (__ballot(rnew)) {
          n_dist++;  // distFn is evaluated again by the reference; same inputs, same bits as pdist
          if (!(rlen == rcap && pdist > list_tail(rd, rcap))) list_insert(rid, rd, rlen, rcap, pid, pdist, lane);
        }
      }
    }
  }
#ifdef SDB_STAMPS
  if (lane == 0 && a.tr_visit && a.visit_cap >= 4) {
    a.tr_visit[(size_t)q * a.visit_cap + 0] = st_adj;
    a.tr_visit[(size_t)q * a.visit_cap + 1] = st_atom;
    a.tr_visit[(size_t)q * a.visit_cap + 2] = st_vec;
    a.tr_visit[(size_t)q * a.visit_cap + 3] = st_ins;
    if constexpr (!Dist::kHasStamps)
      if (a.visit_cap >= 8)
        for (int i = 0; i < 4; i++) a.tr_visit[(size_t)q * a.visit_cap + 4 + i] = st_m[i];
    if constexpr (Dist::kHasStamps)
      if (a.visit_cap >= 8) {
        a.tr_visit[(size_t)q * a.visit_cap + 4] = dist.st[0];
        a.tr_visit[(size_t)q * a.visit_cap + 5] = dist.st[1];
        a.tr_visit[(size_t)q * a.visit_cap + 6] = dist.st[2];
        if (a.visit_cap >= 12)
          for (int i = 0; i < 4; i++) a.tr_visit[(size_t)q * a.visit_cap + 8 + i] = st_m[i];
        if (a.visit_cap >= 28)
          for (int i = 0; i < 4; i++) a.tr_visit[(size_t)q * a.visit_cap + 24 + i] = st_w[i];
      }
  }
#endif

  // ---- the result copy (cand_array.h write_results; from resultSet when filtered, search.go:36)
  // (what only this epilogue reads -- outputs, trace, counters -- comes through cold_args(): loaded here, once, instead
  // of being carried, spilled into VGPR lanes, from the kernel's first instruction through the whole walk)
  ColdArgs &e = cold_args(a);
  if constexpr (FILT) write_results(rid, rd, rlen, a.start_slot, lane, q, e);
  else write_results(cid, cd, len, a.start_slot, lane, q, e);
  if constexpr (kStaged)
    if (lane == 0 && e.sk_counters && n_sk_out) {
      atomicAdd(e.sk_counters, (unsigned long long)n_sk_out);
      if (n_sk_bad) atomicAdd(e.sk_counters + 1, (unsigned long long)n_sk_bad);  // (only a discarded neighbour can be contradicted)
    }
#ifdef SDB_SPEC_STATS
  const uint32_t edges_out = Dist::kSpeculate ? n_spec_hit : n_edges;
#else
  const uint32_t edges_out = n_edges;
#endif
  write_walk_counters(q, lane, n_dist, n_hop, n_edges, edges_out, e);
}

// HCAP names the visited set (visited_set.h VisitedFor): an LDS hash set, which spills to the HBM bitset when it fills
// and sits first in dynamic LDS, the distance policy's tile / LUT after it; or (HCAP == 0) the HBM bitset from the start.
template <class Dist, int NREG, bool FILT, uint32_t HCAP>
__global__ __launch_bounds__(64) void k_greedy_search(const SearchArgs a) {
  const int lane = threadIdx.x;
  const uint32_t q = blockIdx.x;
  extern __shared__ __attribute__((aligned(16))) float lds_f[];
  // dynamic LDS: [search set's hash table][filtered: result set's hash table][distance policy's tile / LUT / scratch]
  using Vis = VisitedFor<HCAP>;
  using RVis = VisitedFor<FILT && HCAP != 0 ? kHashCapResult : 0>;  // (a walk on the bitset keeps its result set there too)
  uint32_t *lds = reinterpret_cast<uint32_t *>(lds_f);
  Dist dist;
  // (the bitset's address before the policy's init: taken behind it, the NG = 0 kernels came out with 12 .. 22 more
  // registers and a wave per SIMD fewer: profiles/walk_steps_ab.json prologue_order)
  uint32_t *bits = a.bitsets + (size_t)q * a.words_per_query;
  dist.init(a, q, lane, lds_f + Vis::kWords + RVis::kWords);
  typename Vis::type vis;
  vis.init_nosync(lds, bits, lane, a);
  if constexpr (HCAP != 0) __syncthreads();
  if constexpr (FILT) {
    typename RVis::type rv;
    rv.init_nosync(lds + Vis::kWords, a.rbitsets + (size_t)q * a.words_per_query, lane, a);
    if constexpr (HCAP != 0) __syncthreads();
    search_body<Dist, NREG, FILT>(a, q, lane, dist, vis, rv);
  } else {
    NoVisited rv;
    search_body<Dist, NREG, FILT>(a, q, lane, dist, vis, rv);
  }
}

// ---- the one-wave quantized walk on two waves -------------------------------------------------------------
// A quantizer whose table sits in LDS beside the walk (M x K <= 2 048) makes a hop a matter of instructions, not of
// bytes: at 10M x 768, M = 8 a hop is ~7 200 cycles of ONE wave's instruction stream -- 1 550 the row and its code
// rows, 2 100 the visited-set test, 500 the table sums, 3 050 AddWithLimit (profiles/r05_stamps_c4.txt) -- and a batch
// of 1 024 queries is four lone waves per CU.  Here a query is two waves, and the stream is cut where its only
// dependency allows:
//   * the WALKER (wave 0) fetches the row, runs the visited-set test and the sums -- and names the next hop's node
//     itself, from one fact about the candidate array (its first unvisited entry F1 after the last insertions) and
//     this hop's distances: a new point lands in front of F1 iff its distance is smaller (distset.go:196-198 moves a
//     point left while it is `<` its neighbour, so it stops behind every entry `<=` it), the smallest such point --
//     if it is the only one at that distance -- is then the array's first unvisited entry (it is always inserted: at
//     its turn the array's tail is F1 or a point not smaller than it; nothing inserted later is in front of it or
//     overwrites it), and if there is none F1 stays where it is;
//   * the MERGER (wave 1) owns the candidate array: it takes the hop's (slot, distance) points from LDS, runs
//     AddWithLimit exactly as the one-wave kernel does, marks the named node, and answers with the next F1 -- while the
//     walker is already at the named node's row.
// (The merger answering AHEAD of its insertions -- the same rule one step on, from the array's first two unvisited
// entries and the batch's two smallest points; 79 of a walk's 83 answers, none wrong -- was built and measured: 0.308
// against 0.306 ms per batch.  The walker's own stream, ~3 700 cycles of fetch, visited-set test and sums plus ~800 of
// naming and hand-over, is what a hop takes; the merger is idle a third of the time either way.  Removed.)
// Nothing is guessed: whenever the rule above does not apply -- no unvisited entry left, a point equal to F1, two points
// sharing the smallest distance, a NaN among
// the distances now or earlier (a NaN entry stops every later point behind it, distset.go:197) -- the walker names nothing, waits for the
// merge and is told the next node (or that the walk is over) by the merger.
// name_next is that rule, for both walkers that have a merger (pq2_walker, pqw_split_walker).  f1 / f1d: the array's
// first unvisited entry after the last insertions; lanes with `mine` hold a new point (nb, mydist); seen_nan: a NaN
// among the walk's distances so far.  The node the walk goes to next, or kNoSlot: the merger says.
__device__ __forceinline__ uint32_t name_next(uint32_t f1, float f1d, bool mine, float mydist, uint32_t nb, bool seen_nan, int lane) {
  // (a point EQUAL to F1 goes behind it -- unless F1 is the full array's tail, which the point overwrites before it
  // moves, distset.go:189-194: rare enough to leave to the merger as well)
  if (seen_nan || f1 == kNoSlot || __ballot(mine && mydist == f1d)) return kNoSlot;
  uint32_t b1 = f1;
  float b1d = f1d, b2d = f1d;  // the two smallest distances in front of F1, edge order among equals
  for (uint64_t t = __ballot(mine && mydist < f1d); t; t &= t - 1) {
    const int j = __ffsll((unsigned long long)t) - 1;
    const float dj = rlf(mydist, j);
    if (dj < b1d) b2d = b1d, b1d = dj, b1 = rl(nb, j);
    else if (dj < b2d) b2d = dj;
  }
  // two points share the smallest distance: the first in edge order is in front -- unless it is the full array's
  // tail when the second arrives and is overwritten by it (distset.go:189-194); left to the merger
  return (b1 == f1 || b2d != b1d) ? b1 : kNoSlot;
}

// a 64-bit LDS word read / written as ONE ds instruction (a volatile access through a generic pointer compiles to
// flat_load / flat_store with system scope: the aperture check and the vector-memory path cost a mailbox poll ~600 cycles)
typedef __attribute__((address_space(3))) volatile unsigned long long lds_u64_t;
__device__ __forceinline__ unsigned long long lds_load_u64(const void *p) {
  return *(lds_u64_t *)p;
}
__device__ __forceinline__ void lds_store_u64(void *p, unsigned long long v) { *(lds_u64_t *)p = v; }
// the mailboxes' payload goes through volatile LDS accesses as well: the compiler keeps volatile accesses in program
// order among themselves, so the payload's stores stay in front of the store of the word that carries the sequence
// number and its loads stay behind the load that saw it -- the hardware performs one wave's LDS instructions in issue
// order, and the emitted instructions are the same ds_read / ds_write as before
typedef __attribute__((address_space(3))) volatile uint32_t lds_u32_t;
__device__ __forceinline__ uint32_t lds_load_u32(const void *p) { return *(lds_u32_t *)p; }
__device__ __forceinline__ void lds_store_u32(void *p, uint32_t v) { *(lds_u32_t *)p = v; }

struct Pq2Shared {
  // Both mailboxes are written by one lane with volatile LDS stores, the word that carries the sequence number last: a
  // wave's LDS instructions are performed in the order it issued them (and volatile accesses are issued in program
  // order), so whoever sees the number sees what was written before it -- no s_waitcnt on either side (a workgroup-scope
  // release would wait for every global load the walker has in flight: the next hop's rows).
  uint2 pts_word;  // x: the node the walker goes to next, or kNoSlot: the merger says; y: batches posted (monotonic)
  uint2 pts_mask;  // lanes of the batch that hold a point
  uint2 ans_word;  // x: pts_word.x == kNoSlot: the first unvisited entry after the insertions (marked now), kNoSlot: none left; y: batches merged
  uint2 ans_f1;    // the first unvisited entry behind the node the walk goes to (x: slot or kNoSlot, y: its distance's bits)
  uint32_t pad[8];
  uint32_t pts_id[64];
  float pts_d[64];
};
constexpr uint32_t kPq2SharedWords = sizeof(Pq2Shared) / 4;

template <class Visited>
__device__ __forceinline__ void pq2_walker(const SearchArgs &a, const uint32_t q, const int lane, PQDist &dist, Visited &vis,
                                           Pq2Shared *sh) {
  uint32_t n_dist = 0, n_hop = 0, n_edges = 0, seq = 0;
  bool seen_nan = false;
#ifdef SDB_PQ2_STATS
  uint32_t n_slow = 0;
  unsigned long long w_t0 = __builtin_amdgcn_s_memtime(), w_tot0 = w_t0, w_acc[4] = {0, 0, 0, 0};  // front part, wait, naming + post, told
#define SDB_PQ2_W(i)                                          \
  {                                                           \
    unsigned long long _t = __builtin_amdgcn_s_memtime();     \
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");        \
    w_acc[i] += _t - w_t0;                                    \
    w_t0 = _t;                                                \
  }
#else
#define SDB_PQ2_W(i)
#endif
  // one batch of points to the merger; `named`: where the walk goes next, if the walker knows
  auto post = [&](uint64_t pend, uint32_t id, float d, uint32_t named) {
    if ((pend >> lane) & 1ull) lds_store_u32(&sh->pts_id[lane], id), lds_store_u32(&sh->pts_d[lane], __float_as_uint(d));
    seq++;
    if (lane == 0) lds_store_u64(&sh->pts_mask, (unsigned long long)pend);
    wave_lds_sync();
    if (lane == 0) lds_store_u64(&sh->pts_word, (unsigned long long)named | ((unsigned long long)seq << 32));
#ifdef SDB_PQ2_STATS  // hand-over timeline of query 0, sequence numbers 17 .. 24 (tools/pq2_stats.py, visit_cap >= 40)
    if (q == 0 && lane == 0 && seq >= 17 && seq < 25 && a.tr_visit && a.visit_cap >= 40)
      a.tr_visit[8 + (seq - 17) * 4 + 0] = __builtin_amdgcn_s_memtime();
#endif
  };
  uint32_t told = kNoSlot;  // the merger's word on where to go (read by answered())
  auto answered = [&]() {   // the merger is through with everything posted
    unsigned long long w;
    while (w = lds_load_u64(&sh->ans_word), (uint32_t)(w >> 32) != seq) __builtin_amdgcn_s_sleep(1);
    told = (uint32_t)w;
    wave_lds_sync();
#ifdef SDB_PQ2_STATS
    if (q == 0 && lane == 0 && seq >= 17 && seq < 25 && a.tr_visit && a.visit_cap >= 40)
      a.tr_visit[8 + (seq - 17) * 4 + 1] = __builtin_amdgcn_s_memtime();
#endif
  };
  // ---- searchSet.AddWithLimit(startNode)  search.go:57-61: a batch of one point, the merger names the first node
  {
    const uint32_t s = a.start_slot;
    const bool snew = vis.test_and_set(lane == 0, s, lane);
    const uint64_t pend = __ballot(snew);
    float d = 0.0f;
    if (pend) d = dist.one(a, s, lane), n_dist++;
    seen_nan = d != d;
    post(pend, s, d, kNoSlot);
  }
  answered();
  uint32_t pid = told;
  // ---- main loop search.go:65-98
  while (pid != kNoSlot) {
#ifndef SDB_PQ2_STATS
    if (lane == 0 && a.tr_visit && n_hop < a.visit_cap) a.tr_visit[(size_t)q * a.visit_cap + n_hop] = a.ids[pid];  // :73
#endif
    n_hop++;
    const uint32_t *__restrict__ rowp = a.adj + (size_t)pid * kAdjStride;
    dist.begin_row(a, rowp, lane);
    const uint32_t nb = rowp[lane];  // node.neighbours in edge order :77-91
    const bool valid = nb != kNoSlot;
    n_edges += (uint32_t)__popcll(__ballot(valid));
    dist.prefetch(a, nb, valid);
    const bool ahead8 = dist.ahead8(a);
    float t8[8];
    if (ahead8) dist.load8(a, valid, t8);
    const bool isnew = vis.test_and_set(valid, nb, lane);  // CheckAndVisit distset.go:174
    const uint64_t pend = __ballot(isnew);
    float mydist = 0.0f;
    if (pend) {
      n_dist += (uint32_t)__popcll(pend);
      mydist = ahead8 ? dist.sum8(t8, pend, lane) : dist.hop(a, nb, pend, lane);
    } else {
      dist.skip(lane);
    }
    const bool mine = (pend >> lane) & 1ull;
    seen_nan = seen_nan || (__ballot(mine && mydist != mydist) != 0ull);
#ifdef SDB_PQ2_STATS
    asm volatile("" ::"v"(mydist));
#endif
    SDB_PQ2_W(0)
    // the array after the LAST hop's insertions (the merger has had this hop's fetch, test and sums for them)
    answered();
    SDB_PQ2_W(1)
    const unsigned long long f1w64 = lds_load_u64(&sh->ans_f1);
    const uint2 f1w = make_uint2((uint32_t)f1w64, (uint32_t)(f1w64 >> 32));
    uint32_t named = name_next(f1w.x, __uint_as_float(f1w.y), mine, mydist, nb, seen_nan, lane);
    post(pend, nb, mydist, named);
    SDB_PQ2_W(2)
    if (named == kNoSlot) {
#ifdef SDB_PQ2_STATS  // measurement builds: hops the merger named, reported in place of n_edges
      n_slow++;
#endif
      answered();
      named = told;
      SDB_PQ2_W(3)
    }
    pid = named;
  }
#ifdef SDB_PQ2_STATS
  if (lane == 0 && a.tr_visit && a.visit_cap >= 8) {
    for (int i = 0; i < 4; i++) a.tr_visit[(size_t)q * a.visit_cap + i] = w_acc[i];
    a.tr_visit[(size_t)q * a.visit_cap + 4] = __builtin_amdgcn_s_memtime() - w_tot0;
  }
  const uint32_t edges_out = n_slow;
#else
  const uint32_t edges_out = n_edges;
#endif
  write_walk_counters(q, lane, n_dist, n_hop, n_edges, edges_out, a);
}

__device__ __forceinline__ void pq2_merger(const SearchArgs &a, const uint32_t q, const int lane, Pq2Shared *sh, uint32_t *scratch) {
  constexpr int NREG = 2;
  uint32_t cid[NREG];
  float cd[NREG];
#pragma unroll
  for (int r = 0; r < NREG; r++) cid[r] = kNoSlot, cd[r] = 0.0f;
  int len = 0;
  const int cap = (int)a.search_size;
  uint32_t pulling = 0, pulled = 0;  // words of the rows pulled ahead (see below)
#ifdef SDB_PQ2_STATS
  unsigned long long m_t0 = __builtin_amdgcn_s_memtime(), m_acc[3] = {0, 0, 0};  // waiting for points, AddWithLimit, mark + answer
#define SDB_PQ2_M(i)                                          \
  {                                                           \
    unsigned long long _t = __builtin_amdgcn_s_memtime();     \
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");        \
    m_acc[i] += _t - m_t0;                                    \
    m_t0 = _t;                                                \
  }
#else
#define SDB_PQ2_M(i)
#endif
  for (uint32_t seq = 1;; seq++) {
    unsigned long long w;
    while (w = lds_load_u64(&sh->pts_word), (uint32_t)(w >> 32) != seq) __builtin_amdgcn_s_sleep(1);
    wave_lds_sync();
#ifdef SDB_PQ2_STATS
    if (q == 0 && lane == 0 && seq >= 17 && seq < 25 && a.tr_visit && a.visit_cap >= 40)
      a.tr_visit[8 + (seq - 17) * 4 + 2] = __builtin_amdgcn_s_memtime();
#endif
    SDB_PQ2_M(0)
    const uint32_t named = (uint32_t)w;
    const unsigned long long pm64 = lds_load_u64(&sh->pts_mask);
    const uint2 pm = make_uint2((uint32_t)pm64, (uint32_t)(pm64 >> 32));
    const uint64_t pend = (uint64_t)pm.x | ((uint64_t)pm.y << 32);
    const bool mine = (pend >> lane) & 1ull;
    const uint32_t id = mine ? lds_load_u32(&sh->pts_id[lane]) : kNoSlot;
    const float d = mine ? __uint_as_float(lds_load_u32(&sh->pts_d[lane])) : 0.0f;
    // AddWithLimit over the new neighbours, in edge order distset.go:184-198
    if (pend) add_with_limit_merge(cid, cd, len, cap, id, d, pend, lane, scratch);
#ifdef SDB_PQ2_STATS
    asm volatile("" ::"v"(cd[0]));
#endif
    SDB_PQ2_M(1)
    // the node the walk goes to -- named by the walker, or the first unvisited entry (search.go:66-71) -- is marked :74
    // and with it the first unvisited entry behind it: what the walker names the hop after this one with
    uint32_t next, f1;
    float f1d;
    pick_and_mark(cid, cd, len, named, lane, next, f1, f1d);
    if (lane == 0) lds_store_u64(&sh->ans_f1, (unsigned long long)f1 | ((unsigned long long)__float_as_uint(f1d) << 32));
    wave_lds_sync();
    if (lane == 0) lds_store_u64(&sh->ans_word, (unsigned long long)next | ((unsigned long long)seq << 32));
#ifdef SDB_PQ2_STATS
    if (q == 0 && lane == 0 && seq >= 17 && seq < 25 && a.tr_visit && a.visit_cap >= 40)
      a.tr_visit[8 + (seq - 17) * 4 + 3] = __builtin_amdgcn_s_memtime();
#endif
    // That entry is where the walk goes next unless the hop under way finds a nearer point: its adjacency row and the
    // code rows behind it are pulled through L2 now, a whole hop before the walker asks for them (the values are not
    // used; they are waited for one batch later, when they have long arrived): 0.321 -> 0.306 ms per batch at 4M x 768
    pulled ^= pulling;
    pulling = 0;
    if (f1 != kNoSlot && a.adj_codes) {
      pulling = a.adj[(size_t)f1 * kAdjStride + lane];
      const size_t row_bytes = (size_t)64 * a.pq_M;  // one 64-byte line per lane
      if ((uint32_t)lane * 64u < row_bytes) pulling ^= *reinterpret_cast<const uint32_t *>(a.adj_codes + (size_t)f1 * row_bytes + (size_t)lane * 64);
    }
    SDB_PQ2_M(2)
    if (named == kNoSlot && next == kNoSlot) break;  // no unvisited entry left :66-71 -- the walker has been waiting for this
  }
#ifdef SDB_PQ2_STATS
  if (lane == 0 && a.tr_visit && a.visit_cap >= 8)
    for (int i = 0; i < 3; i++) a.tr_visit[(size_t)q * a.visit_cap + 5 + i] = m_acc[i];
#endif
  if ((pulled ^ pulling) == 0x9e3779b9u && a.limit == 0xFFFFFFFFu) a.out_counts[q] = pulled;  // (keeps the pulls alive; never true)
  write_results(cid, cd, len, a.start_slot, lane, q, a);
}

// Dynamic LDS: [visited set's table][the query's M x K table][Pq2Shared].  Unfiltered searches with searchSize <= 128,
// no visit log for a build, no overflow list on the start node (walk_plan.h decides).
// (A workgroup of four waves with the walker on wave (blockIdx / 256) % 4 and the merger two SIMDs on -- the placement
// trick of k_greedy_search_pqw -- was slower: 0.370 against 0.323 ms at 4M x 768.)
template <uint32_t HCAP>
__global__ __launch_bounds__(128) void k_greedy_search_pq2(const SearchArgs a) {
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const uint32_t q = blockIdx.x;
  extern __shared__ __attribute__((aligned(16))) float lds_f[];
  __shared__ uint32_t s_scatter2[2 * 2 * 64];  // add_with_limit_merge scratch
  float *lut = lds_f + VisitedFor<HCAP>::kWords;
  Pq2Shared *sh = reinterpret_cast<Pq2Shared *>(lut + ((a.pq_M * a.pq_K + 3u) & ~3u));
  uint32_t *bits = a.bitsets + (size_t)q * a.words_per_query;
  if (wave == 1) {
    const float *g = a.pq_lut + (size_t)q * a.pq_M * a.pq_K;
    for (uint32_t i = lane; i < a.pq_M * a.pq_K; i += 64) lut[i] = g[i];
    if (lane == 0) sh->pts_word = make_uint2(kNoSlot, 0u), sh->ans_word = make_uint2(kNoSlot, 0u);
    __syncthreads();  // table, visited set and mailbox in place
    return pq2_merger(a, q, lane, sh, s_scatter2);
  }
  PQDist dist;
  dist.table_in_lds(lut);
  typename VisitedFor<HCAP>::type hv;
  hv.init_nosync(reinterpret_cast<uint32_t *>(lds_f), bits, lane, a);
  __syncthreads();
  pq2_walker(a, q, lane, dist, hv, sh);
}

// The walker of the multi-wave quantized walk in its split form: k_greedy_search_pq2's division of labour inside
// k_greedy_search_pqw.  The candidate array lives in a helper wave (PQWideDist::serve<true>, the merger), which inserts
// a hop's points one round late, under the next row's code fetch and visited-set test; this wave names the next node
// from the array's first unvisited entry and the hop's sums, by the rule and with the exceptions described above
// pq2_walker -- when the rule does not apply it asks (a round of two barriers) and the merger picks.
template <class Dist, class Visited>
__device__ __forceinline__ void pqw_split_walker(const SearchArgs &a, const uint32_t q, const int lane, Dist &dist, Visited &vis) {
  uint32_t n_dist = 0, n_hop = 0, n_edges = 0;
  bool seen_nan = false;
  // ---- searchSet.AddWithLimit(startNode)  search.go:57-61
  {
    const uint32_t s = a.start_slot;
    const bool snew = vis.test_and_set(lane == 0, s, lane);
    if (__ballot(snew)) {
      const float d = dist.one(a, s, lane);
      n_dist++;
      seen_nan = d != d;
    }
  }
  uint32_t pid = dist.ask_next(lane);
  dist.post_named = kNoSlot;
  // ---- main loop search.go:65-98
  while (pid != kNoSlot) {
    if (lane == 0 && a.tr_visit && n_hop < a.visit_cap) a.tr_visit[(size_t)q * a.visit_cap + n_hop] = a.ids[pid];  // :73
    n_hop++;
    const uint32_t *__restrict__ rowp = a.adj + (size_t)pid * kAdjStride;
    dist.begin_row(a, rowp, lane);
    const uint32_t nb = rowp[lane];  // node.neighbours in edge order :77-91
    const bool valid = nb != kNoSlot;
    n_edges += (uint32_t)__popcll(__ballot(valid));
    dist.prefetch(a, nb, valid);
    const bool isnew = vis.test_and_set(valid, nb, lane);  // CheckAndVisit distset.go:174
    const uint64_t pend = __ballot(isnew);
    float mydist = 0.0f;
    if (pend) {
      n_dist += (uint32_t)__popcll(pend);
      mydist = dist.hop(a, nb, pend, lane);
    } else {
      dist.skip(lane);
    }
    const bool mine = (pend >> lane) & 1ull;
    seen_nan = seen_nan || (__ballot(mine && mydist != mydist) != 0ull);
    // the array after the LAST hop's insertions and with this hop's node marked: written by the merger before this
    // round's second barrier
    const uint32_t named = name_next(dist.sh->f1, dist.sh->f1d, mine, mydist, nb, seen_nan, lane);
    dist.post_named = named;  // (with the next row; kNoSlot: the merger has settled by then)
    pid = named != kNoSlot ? named : dist.ask_next(lane);
  }
  write_walk_counters(q, lane, n_dist, n_hop, n_edges, n_edges, a);
}

// The multi-wave quantized walk: one query per workgroup of four waves (PQWideDist above).  Dynamic LDS: the visited
// set's table, the command area, the LDS-resident tables [4][NL][K].
// NL < 16: the variant meant to run two queries per CU (half the LDS each) -- its registers are capped accordingly
// NLW: tables the WALKER keeps in LDS (the rest of its NL + RT in registers).  The walker carries search_body's state
// (candidate array, visited set, ~100 registers) on top of what every wave holds; at eight waves per query (M = 384,
// 256 registers per wave) that state plus 33 register tables plus the 48 looked-up values did not fit -- 43 registers
// spilled.  There the walker takes 24 of its 48 tables from LDS and 24 from registers; the helpers keep 15 + 33.
// SPLIT: the candidate array lives in the helper next to the walker (pqw_split_walker, PQWideDist::serve<true>)
template <int NL, int RT, uint32_t HCAP, int W = 4, int NLW = NL, bool SPLIT = false>
__global__ __launch_bounds__(64 * W, (NL < 16 && W == 4) ? 2 : 1) void k_greedy_search_pqw(const SearchArgs a) {
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const uint32_t q = blockIdx.x;
  // Which wave walks.  Every wave owns its index range whatever its role; the walker additionally runs search_body
  // (visited set, candidate array), about twice a helper's instruction count, on ITS SIMD.  Two queries share a CU in
  // the NL < 16 variant, and the k-th wave of a workgroup lands on the k-th SIMD: with wave 0 walking in both, one
  // SIMD carried both walkers.  Workgroups that share a CU are 256 (or a multiple) apart in the grid, so the role
  // rotates with blockIdx / 256.  Any choice is correct; this one balances.
  const int walker = (NL < 16 && W == 4) ? (int)((blockIdx.x >> 8) & 3u) : 0;
  extern __shared__ __attribute__((aligned(16))) float lds_f[];
  constexpr uint32_t kVisWords = VisitedFor<HCAP>::kWords;
  PQWideShared *sh = reinterpret_cast<PQWideShared *>(lds_f + kVisWords);
  float *lut_lds = lds_f + kVisWords + kPqwSharedWords;
  static_assert(NLW == NL || W == 8, "a walker with its own split is wave 0 of the eight-wave form");
  using Walker = PQWideDist<NLW, NL + RT - NLW, W>;
  using Helper = PQWideDist<NL, RT, W>;
  uint32_t *bits = a.bitsets + (size_t)q * a.words_per_query;
  __shared__ uint32_t s_scatter_m[SPLIT ? 2 * 2 * 64 : 1];  // the merger's add_with_limit_merge scratch
  if (wave != walker) {
    Helper dist;
    // (NLW != NL: the walker is wave 0 and its NLW tables come first in the block)
    dist.init_wave(a, q, lane, wave, lut_lds, sh, NLW == NL ? (uint32_t)wave * NL : (uint32_t)(NLW + (wave - 1) * NL));
    __syncthreads();  // tables and visited set in place
    if constexpr (SPLIT)
      if (wave == ((walker + 1) & (W - 1))) return dist.template serve<true>(a, lane, q, s_scatter_m);
    return dist.serve(a, lane);
  }
  Walker dist;
  dist.init_wave(a, q, lane, wave, lut_lds, sh, NLW == NL ? (uint32_t)wave * NL : 0u);
  NoVisited rv;
  typename VisitedFor<HCAP>::type hv;
  hv.init_nosync(reinterpret_cast<uint32_t *>(lds_f), bits, lane, a);
  __syncthreads();  // tables and visited set in place
  if constexpr (SPLIT) pqw_split_walker(a, q, lane, dist, hv);
  else search_body<Walker, 2, false>(a, q, lane, dist, hv, rv);
  dist.finish(lane);
}

// The workgroup-per-query walk of a plain store (PlainWideDist): W waves, wave 0 walks.  Dynamic LDS: the visited set's
// table, then the policy's hop scratch and command word.
template <int NG, bool L2, int W, bool FILT>
__global__ __launch_bounds__(64 * W) void k_greedy_search_wide(const SearchArgs a) {
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const uint32_t q = blockIdx.x;
  extern __shared__ __attribute__((aligned(16))) float lds_f[];
  // dynamic LDS: [search set's hash table][filtered: the result set's][the policy's hop scratch and command words]
  constexpr uint32_t kRWords = FILT ? HashVisited<kHashCapResult>::kWords : 0;
  PlainWideDist<NG, L2, W> dist;
  dist.init_wave(a, q, lane, wave, lds_f + HashVisited<kHashCap>::kWords + kRWords);
  HashVisited<kHashCap> hv;
  HashVisited<kHashCapResult> rv;
  if (wave == 0) {
    hv.init_nosync(reinterpret_cast<uint32_t *>(lds_f), a.bitsets + (size_t)q * a.words_per_query, lane, a);
    if constexpr (FILT)
      rv.init_nosync(reinterpret_cast<uint32_t *>(lds_f) + HashVisited<kHashCap>::kWords, a.rbitsets + (size_t)q * a.words_per_query, lane, a);
  }
  __syncthreads();
  if (wave != 0) return dist.template serve<HashVisited<kHashCap>>(a, lane, reinterpret_cast<uint32_t *>(lds_f));
  if constexpr (FILT) {
    search_body<PlainWideDist<NG, L2, W>, 2, true>(a, q, lane, dist, hv, rv);
  } else {
    NoVisited nv;
    search_body<PlainWideDist<NG, L2, W>, 2, false>(a, q, lane, dist, hv, nv);
  }
  dist.finish(lane);
}

}  // namespace sdb
