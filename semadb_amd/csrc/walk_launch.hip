// walk_launch.hip -- K2's launcher: the walk kernels (search_kernel.h) are instantiated here and nowhere else.
// launch_walk_plan() maps a WalkPlan (walk_plan.h decides it) to its instantiation; it asks no routing question itself.
// LDS sizes are stated here, from the device structs and Dist::kLdsBytes.
#include "search_kernel.h"
#include "walk_plan.h"

namespace sdb {

// the one launch: the plan's two patched fields, the large-LDS attribute of the multi-wave quantized walk, the error check
template <void (*KERNEL)(const SearchArgs)>
static int launch(const WalkPlan &p, const SearchArgs &a, uint32_t nq, size_t lds, hipStream_t stream) {
  if (p.family == WalkFamily::kPqWide) {
    static std::atomic<uint64_t> seen{0};
    if (first_use_on_this_device(seen))
      SDB_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(KERNEL), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024 - 1024));
  }
  SearchArgs b = a;
  b.hash_limit = p.hash_limit, b.wide_pull = p.wide_pull;
  hipLaunchKernelGGL(KERNEL, dim3(nq), dim3(64 * p.waves), lds, stream, b);
  SDB_HIP(hipGetLastError());
  return SDB_OK;
}

static int no_kernel(const WalkPlan &p) {
  return fail(SDB_ERR_STATE, "no walk kernel for plan (family %u, visited %u, ng %d, waves %d)", (unsigned)p.family, (unsigned)p.visited, p.ng, p.waves);
}

// the visited set HCAP names (visited_set.h VisitedFor) precedes the policy's own LDS
template <uint32_t HCAP>
constexpr size_t set_bytes() { return VisitedFor<HCAP>::kWords * sizeof(uint32_t); }
constexpr size_t kResultSetBytes = set_bytes<kHashCapResult>();  // a filtered walk's result set, beside an LDS set

// k_greedy_search, one wave per query; dist_lds: the distance policy's own LDS
template <class Dist, uint32_t HCAP>
static int launch_one_wave(const WalkPlan &p, const SearchArgs &a, uint32_t nq, hipStream_t stream, size_t dist_lds) {
  const size_t lds = set_bytes<HCAP>() + (HCAP != 0 && p.filt ? kResultSetBytes : 0) + dist_lds;
  if constexpr (HCAP == 0)  // eight array registers: searchSize > 128, which no LDS set serves
    if (p.nreg == 8)
      return p.filt ? launch<k_greedy_search<Dist, 8, true, 0>>(p, a, nq, lds, stream) : launch<k_greedy_search<Dist, 8, false, 0>>(p, a, nq, lds, stream);
  return p.filt ? launch<k_greedy_search<Dist, 2, true, HCAP>>(p, a, nq, lds, stream) : launch<k_greedy_search<Dist, 2, false, HCAP>>(p, a, nq, lds, stream);
}

// code tables (PQLdsDist, PQGlobalDist, BitDist): every visited-set policy
template <class Dist>
static int launch_codes(const WalkPlan &p, const SearchArgs &a, uint32_t nq, hipStream_t stream, size_t dist_lds) {
  switch (p.visited) {
    case WalkVisited::kBitset: return launch_one_wave<Dist, 0>(p, a, nq, stream, dist_lds);
    case WalkVisited::kHash16: return launch_one_wave<Dist, kHash16>(p, a, nq, stream, dist_lds);
    case WalkVisited::kHashPQ: return launch_one_wave<Dist, kHashCapPQ>(p, a, nq, stream, dist_lds);
    default: return no_kernel(p);
  }
}

template <uint32_t HCAP>
static int launch_pq2(const WalkPlan &p, const SearchArgs &a, uint32_t nq, hipStream_t stream) {
  const size_t lds = set_bytes<HCAP>() + ((((size_t)a.pq_M * a.pq_K + 3) & ~(size_t)3) + kPq2SharedWords) * sizeof(uint32_t);
  return launch<k_greedy_search_pq2<HCAP>>(p, a, nq, lds, stream);
}

template <int NL, int RT, int W = 4, int NLW = NL, bool SPLIT = false>
static int launch_pqw(const WalkPlan &p, const SearchArgs &a, uint32_t nq, hipStream_t stream) {
  if constexpr (W == 4 && NL == 15 && !SPLIT)  // the forms with room for a helper wave's candidate array
    if (p.split) return launch_pqw<NL, RT, W, NLW, true>(p, a, nq, stream);
  const size_t lds = sizeof(PQWideShared) + (size_t)((W - 1) * NL + NLW) * a.pq_K * sizeof(float);
  if (p.visited == WalkVisited::kHash16) return launch<k_greedy_search_pqw<NL, RT, kHash16, W, NLW, SPLIT>>(p, a, nq, set_bytes<kHash16>() + lds, stream);
  return launch<k_greedy_search_pqw<NL, RT, kHashCapPQ, W, NLW, SPLIT>>(p, a, nq, set_bytes<kHashCapPQ>() + lds, stream);
}
constexpr int pqw_form(int w, int nl, int rt) { return (w * 64 + nl) * 64 + rt; }  // one switch over the three

template <int NG, bool L2, int W>
static int launch_wide(const WalkPlan &p, const SearchArgs &a, uint32_t nq, hipStream_t stream) {
  const size_t lds = set_bytes<kHashCap>() + PlainWideDist<NG, L2, W>::kLdsBytes;
  return p.filt ? launch<k_greedy_search_wide<NG, L2, W, true>>(p, a, nq, lds + kResultSetBytes, stream)
                : launch<k_greedy_search_wide<NG, L2, W, false>>(p, a, nq, lds, stream);
}

template <int NG, bool L2>  // plain rows, the query in registers
static int launch_rows(const WalkPlan &p, const SearchArgs &a, uint32_t nq, hipStream_t stream) {
  switch (p.family) {
    case WalkFamily::kWide:
      if constexpr (NG >= 1 && NG <= 8) {
        if constexpr (NG != 8)
          if (p.waves == kWideWaves) return launch_wide<NG, L2, kWideWaves>(p, a, nq, stream);
        if (p.waves == 8) return launch_wide<NG, L2, 8>(p, a, nq, stream);
      }
      return no_kernel(p);
    case WalkFamily::kStageInt8:
      if constexpr (stage_int8(NG, L2, false))
        return launch<k_greedy_search<Int8Dist<NG>, 2, false, kHashCap>>(p, a, nq, set_bytes<kHashCap>() + Int8Dist<NG>::kLdsBytes, stream);
      return no_kernel(p);
    case WalkFamily::kStageHalf:
      // (few float32 rows survive the first stage: four pairs of them in flight per round leave the registers to the copy's rows)
      if constexpr (stage_shape(NG)) return launch_one_wave<PlainDist<NG, L2, true, 4, Stage::kHalf>, kHashCap>(p, a, nq, stream, PlainDist<NG, L2, true, 4, Stage::kHalf>::kLdsBytes);
      return no_kernel(p);
    case WalkFamily::kPlain:  // DEEP (wave_dist.h ChunkPairs): the LDS set's kernel runs one wave per SIMD
      if (p.visited == WalkVisited::kHash) return launch_one_wave<PlainDist<NG, L2, true>, kHashCap>(p, a, nq, stream, PlainDist<NG, L2, true>::kLdsBytes);
      return launch_one_wave<PlainDist<NG, L2, false>, 0>(p, a, nq, stream, PlainDist<NG, L2, false>::kLdsBytes);
    default: return no_kernel(p);
  }
}

template <bool L2>
static int launch_ng(const WalkPlan &p, const SearchArgs &a, uint32_t nq, hipStream_t stream) {
  switch (p.ng) {
    case 0: return launch_rows<0, L2>(p, a, nq, stream);
    case 1: return launch_rows<1, L2>(p, a, nq, stream);
    case 2: return launch_rows<2, L2>(p, a, nq, stream);
    case 3: return launch_rows<3, L2>(p, a, nq, stream);
    case 4: return launch_rows<4, L2>(p, a, nq, stream);
    case 6: return launch_rows<6, L2>(p, a, nq, stream);
    case 8: return launch_rows<8, L2>(p, a, nq, stream);
    case 12: return launch_rows<12, L2>(p, a, nq, stream);  // 1536
    case 16: return launch_rows<16, L2>(p, a, nq, stream);  // 2048
    case 24: return launch_rows<24, L2>(p, a, nq, stream);  // 3072
    default:  // any other length: the query tile in LDS, on the bitset
      if (p.family != WalkFamily::kPlain || p.visited != WalkVisited::kBitset) return no_kernel(p);
      return launch_one_wave<PlainDist<-1, L2>, 0>(p, a, nq, stream, (size_t)(a.ng * 128 + 32) * sizeof(float));
  }
}

int launch_walk_plan(const WalkPlan &p, const SearchArgs &a, uint32_t nq, hipStream_t stream) {
  if (nq == 0) return SDB_OK;
  if (p.bad_search_size) return fail(SDB_ERR_INVALID, "searchSize %u not supported on device (1..512)", a.search_size);
  switch (p.family) {
    case WalkFamily::kBits:
      return p.jaccard ? launch_codes<BitDist<true>>(p, a, nq, stream, BitDist<true>::kLdsBytes)
                       : launch_codes<BitDist<false>>(p, a, nq, stream, BitDist<false>::kLdsBytes);
    case WalkFamily::kPqLds: return launch_codes<PQLdsDist>(p, a, nq, stream, (size_t)a.pq_M * a.pq_K * sizeof(float));
    case WalkFamily::kPqGlobal: return launch_codes<PQGlobalDist>(p, a, nq, stream, 0);
    case WalkFamily::kPqTwoWaves:
      return p.visited == WalkVisited::kHash16 ? launch_pq2<kHash16>(p, a, nq, stream) : launch_pq2<kHashCapPQ>(p, a, nq, stream);
    case WalkFamily::kPqWide:
      switch (pqw_form(p.waves, p.nl, p.rt)) {
        case pqw_form(4, 32, 0): return launch_pqw<32, 0>(p, a, nq, stream);
        case pqw_form(4, 15, 17): return launch_pqw<15, 17>(p, a, nq, stream);
        case pqw_form(4, 32, 16): return launch_pqw<32, 16>(p, a, nq, stream);
        case pqw_form(4, 15, 33): return launch_pqw<15, 33>(p, a, nq, stream);
        case pqw_form(4, 32, 32): return launch_pqw<32, 32>(p, a, nq, stream);
        case pqw_form(8, 15, 33): return launch_pqw<15, 33, 8, 24>(p, a, nq, stream);
        default: return no_kernel(p);
      }
    default: return p.l2 ? launch_ng<true>(p, a, nq, stream) : launch_ng<false>(p, a, nq, stream);
  }
}

int launch_greedy_search(const SearchArgs &a, uint32_t nq, hipStream_t stream) { return launch_walk_plan(plan_walk(a, nq), a, nq, stream); }

}  // namespace sdb
