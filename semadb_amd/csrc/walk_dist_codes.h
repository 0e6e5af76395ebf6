// walk_dist_codes.h -- K2: the distance policies over codes (PQDistT, BitDist, PQWideDist).
// (a part of search_kernel.h, which includes it after what it builds on; no .hip file includes it directly)
#pragma once
#include "cand_array.h"

namespace sdb {

// Fitted product quantizer: dist = sum_i lut[i*K + code_i], plain fp32 adds in index order
// (product.go:271-275).  One lane per neighbour: all new neighbours of a hop in one pass.
// IN_LDS: the query's table was copied into LDS (SearchArgs::pq_lut_in_lds), else it is read where k_pq_lut left it.  Two
// kernels and a pointer typed by its address space, not one kernel and a generic pointer: through a generic pointer every
// lookup is a flat load, which counts on both wait counters (tests/test_stage_load_schedule.py).
template <bool IN_LDS, bool OPAQUE_K = false>
struct PQDistT {
  static constexpr Stage kStage = Stage::kNone;
  // (the same naming of the next hop's row, with its code rows fetched ahead: 0.419 against 0.359 ms per batch at
  // 4M x 768, M = 8 -- a one-wave hop is bound by its instruction count, not by the fetch; measured and removed)
  static constexpr bool kSpeculate = false;
  static constexpr bool kHasStamps = false;
  static constexpr bool kPointDistances = false;  // LUT distance != the centroid-pair distance of the prunes
  // K, the table's row stride.  OPAQUE_K (the one-wave walk with its table in LDS): read through a value the optimiser
  // cannot see through, so that the rows' offsets k K are computed where they are used.  Known to be loop-invariant
  // they are hoisted out of the walk, one SGPR each for the up to 32 rows of a lookup, and parked in VGPR lanes: 139
  // spilled SGPRs on the filtered kernel (limit 128), 82 so.  (Seen with the clang of ROCm's LLVM this library is built
  // with, AMD clang 22.0.0git of ROCm 7.2.0; when a compiler keeps the filtered PQLdsDist kernels under the limit of
  // tools/kernel_table.py --check without it, the barrier can go.)
  static __device__ __forceinline__ uint32_t row_stride(const SearchArgs &a) {
    uint32_t K = a.pq_K;
    if constexpr (OPAQUE_K) asm volatile("" : "+s"(K));
    return K;
  }
  typedef const __attribute__((address_space(3))) float *lds_table;
  typedef const __attribute__((address_space(1))) float *global_table;
  typename std::conditional<IN_LDS, lds_table, global_table>::type lut;  // this query's [M][K] table
  __device__ __forceinline__ void table_in_lds(const float *lds) {
    static_assert(IN_LDS, "a table in LDS");
    lut = (lds_table)lds;
  }
  __device__ __forceinline__ void init(const SearchArgs &a, uint32_t q, int lane, float *lds) {
    const float *g = a.pq_lut + (size_t)q * a.pq_M * row_stride(a);
    if constexpr (IN_LDS) {
      for (uint32_t i = lane; i < a.pq_M * row_stride(a); i += 64) lds[i] = g[i];
      __syncthreads();
      lut = (lds_table)lds;
    } else {
      lut = as_global(g);
    }
  }
  // dist = 0; dist += lut[i][code_i] for i = 0 .. M-1, plain fp32 adds in index order (product.go:271-275), over the
  // code row at `c` (M bytes; rows are M apart from an aligned base, so whole words when M is a multiple of four)
  __device__ __forceinline__ float sum_row(const SearchArgs &a, const uint8_t *__restrict__ c) const {
    float dist = 0.0f;
    const uint32_t K = row_stride(a);
    if ((a.pq_M & 3u) == 0) {
      const uint32_t *__restrict__ w = reinterpret_cast<const uint32_t *>(c);
      for (uint32_t i = 0; i < a.pq_M; i += 4) {
        const uint32_t v = w[i >> 2];
        dist += lut[(i + 0) * K + (v & 0xFF)];
        dist += lut[(i + 1) * K + ((v >> 8) & 0xFF)];
        dist += lut[(i + 2) * K + ((v >> 16) & 0xFF)];
        dist += lut[(i + 3) * K + (v >> 24)];
      }
    } else {
      for (uint32_t i = 0; i < a.pq_M; i++) dist += lut[i * K + c[i]];
    }
    return dist;
  }
  __device__ __forceinline__ float sum(const SearchArgs &a, uint32_t slot) const {
    return sum_row(a, a.pq_codes + (size_t)slot * a.pq_M);
  }
  __device__ __forceinline__ float one(const SearchArgs &a, uint32_t s, int lane) { return sum(a, s); }
  __device__ __forceinline__ void speculation(bool, const uint32_t *) {}
  __device__ __forceinline__ void ahead(const SearchArgs &, const uint32_t *, int, bool) {}
  __device__ __forceinline__ void skip(int) {}
  // The chunk's code rows.  With the neighbours' codes stored behind the adjacency row (SearchArgs::adj_codes) lane j's
  // row is at a fixed place next to edge j: it is asked for TOGETHER with the row of ids -- one round trip per hop, 64 M
  // contiguous bytes -- instead of after it, by slot (64 scattered M-byte reads, a 64-byte sector each).  The start
  // node's overflow chunks and the filter's seeds are no adjacency rows: those gather by slot.
  const uint8_t *row_codes = nullptr;  // this lane's code row of the chunk being expanded, or NULL: by slot
  __device__ __forceinline__ void begin_row(const SearchArgs &a, const uint32_t *rowp, int lane) {
    row_codes = nullptr;
    pre_ready = false;
    if (a.adj_codes && rowp >= a.adj && rowp < a.adj + (size_t)a.adj_rows * kAdjStride) {  // not a chunk of the overflow list
      const size_t e0 = (size_t)(rowp - a.adj);  // = row * 64
      row_codes = a.adj_codes + (e0 + (size_t)lane) * a.pq_M;
      if (a.pq_M == 8) {
        pre = *reinterpret_cast<const uint2 *>(row_codes), pre_ready = true;
      } else if (a.pq_M == 16) {
        prew[0] = *reinterpret_cast<const uint4 *>(row_codes), pre_ready = true;
      } else if (a.pq_M == 32) {
        prew[0] = reinterpret_cast<const uint4 *>(row_codes)[0], prew[1] = reinterpret_cast<const uint4 *>(row_codes)[1];
        pre_ready = true;
      }
    }
  }
  uint4 prew[2];  // M = 16 / 32: the lane's code row, asked for with the row of ids
  __device__ __forceinline__ float add4(float dist, uint32_t v, uint32_t i, uint32_t K) const {
    dist += lut[(i + 0) * K + (v & 0xFF)];
    dist += lut[(i + 1) * K + ((v >> 8) & 0xFF)];
    dist += lut[(i + 2) * K + ((v >> 16) & 0xFF)];
    dist += lut[(i + 3) * K + (v >> 24)];
    return dist;
  }
  __device__ __forceinline__ float sum16(float dist, const uint4 &v, uint32_t i, uint32_t K) const {
    dist = add4(dist, v.x, i, K), dist = add4(dist, v.y, i + 4, K);
    dist = add4(dist, v.z, i + 8, K), dist = add4(dist, v.w, i + 12, K);
    return dist;
  }
  // M == 8 (the documented configuration): the 8 code bytes of every neighbour are fetched as one 8-byte
  // load BEFORE the visited-set test, so the code fetch and the test-and-set round trip overlap; codes of
  // neighbours that turn out to be already visited are simply not used (8 bytes each).
  uint2 pre;
  bool pre_ready = false;
  __device__ __forceinline__ void prefetch(const SearchArgs &a, uint32_t nb, bool valid) {
    if (pre_ready) return;  // came with the row
    pre = make_uint2(0u, 0u);
    if (a.pq_M == 8 && valid && !row_codes) pre = *reinterpret_cast<const uint2 *>(a.pq_codes + (size_t)nb * 8);
  }
  // M == 8 with the code row at hand (it came with the row of ids): the eight table entries can be asked for AHEAD of
  // the visited-set test, whose first LDS round trip then covers theirs, and summed after it (k_greedy_search_pq2)
  __device__ __forceinline__ bool ahead8(const SearchArgs &a) const { return a.pq_M == 8 && pre_ready; }
  __device__ __forceinline__ void load8(const SearchArgs &a, bool valid, float (&t)[8]) const {
    const uint32_t K = row_stride(a);
    const uint32_t x = valid ? pre.x : 0u, y = valid ? pre.y : 0u;
    t[0] = lut[0 * K + (x & 0xFF)], t[1] = lut[1 * K + ((x >> 8) & 0xFF)];
    t[2] = lut[2 * K + ((x >> 16) & 0xFF)], t[3] = lut[3 * K + (x >> 24)];
    t[4] = lut[4 * K + (y & 0xFF)], t[5] = lut[5 * K + ((y >> 8) & 0xFF)];
    t[6] = lut[6 * K + ((y >> 16) & 0xFF)], t[7] = lut[7 * K + (y >> 24)];
  }
  __device__ __forceinline__ float sum8(const float (&t)[8], uint64_t pend, int lane) {
    row_codes = nullptr, pre_ready = false;
    if (!((pend >> lane) & 1ull)) return 0.0f;
    float dist = 0.0f;  // the same sequential adds in index order (product.go:271-275)
#pragma unroll
    for (int i = 0; i < 8; i++) dist += t[i];
    return dist;
  }
  __device__ __forceinline__ float hop(const SearchArgs &a, uint32_t nb, uint64_t pend, int lane) {
    const uint8_t *rc = row_codes;
    const bool ready = pre_ready;
    row_codes = nullptr, pre_ready = false;  // one chunk's worth (the seeds of a filtered search call hop without begin_row)
    if (!((pend >> lane) & 1ull)) return 0.0f;
    if (a.pq_M != 8) {
      if (ready && a.pq_M == 16) return sum16(0.0f, prew[0], 0, row_stride(a));
      if (ready && a.pq_M == 32) return sum16(sum16(0.0f, prew[0], 0, row_stride(a)), prew[1], 16, row_stride(a));
      return rc ? sum_row(a, rc) : sum(a, nb);
    }
    float dist = 0.0f;  // same sequential adds in index order (product.go:271-275)
    const uint32_t K = row_stride(a);
    dist += lut[0 * K + (pre.x & 0xFF)];
    dist += lut[1 * K + ((pre.x >> 8) & 0xFF)];
    dist += lut[2 * K + ((pre.x >> 16) & 0xFF)];
    dist += lut[3 * K + (pre.x >> 24)];
    dist += lut[4 * K + (pre.y & 0xFF)];
    dist += lut[5 * K + ((pre.y >> 8) & 0xFF)];
    dist += lut[6 * K + ((pre.y >> 16) & 0xFF)];
    dist += lut[7 * K + (pre.y >> 24)];
    return dist;
  }
};
typedef PQDistT<true> PQDist;               // (k_greedy_search_pq2, which keeps its table in LDS always)
typedef PQDistT<true, true> PQLdsDist;      // the one-wave walk, table copied into LDS
typedef PQDistT<false> PQGlobalDist;        // the one-wave walk, table where k_pq_lut left it

// Binary quantizer with a threshold: dist = bitDistFn(encode(query), code[slot]) (binary.go:191-200), hammingDistance
// or jaccardDistance of distance.go:45-67 -- integer population counts, one conversion (hamming) or one float32
// division and one subtraction (jaccard).  One lane per neighbour, like PQDist: the lane reads its W-word code row by
// slot (16-byte loads when W is even: rows are 8 W bytes from a 256-byte-aligned base), the query's words -- encoded
// once by init, the wave's ballots (binary.go:123-127) -- are read from LDS at a wave-uniform address.
template <bool JACCARD>
struct BitDist {
  static constexpr Stage kStage = Stage::kNone;
  static constexpr bool kSpeculate = false;
  static constexpr bool kHasStamps = false;
  static constexpr bool kPointDistances = false;  // (the build's distance table is a full-precision store's)
  static constexpr size_t kLdsBytes = 64 * sizeof(uint64_t) + 8;  // W <= 64 query words, on an 8-byte boundary
  typedef __attribute__((address_space(3))) uint64_t lds_word;
  const lds_word *xq;  // LDS [W] (typed as LDS: a generic pointer's reads and writes would be flat instructions)
  uint32_t W;
  __device__ __forceinline__ void init(const SearchArgs &a, uint32_t q, int lane, float *lds) {
    lds_word *w = (lds_word *)(((uint32_t)(uintptr_t)(__attribute__((address_space(3))) float *)lds + 7u) & ~7u);
    const float *v = a.queries + (size_t)q * a.dim;
    W = a.bq_W;
    for (uint32_t k = 0; k < W; k++) {
      const uint32_t i = k * 64 + (uint32_t)lane;
      const bool bit = i < a.dim && v[i] > a.bq_thr[i];  // strict: never for a NaN; bits past dim stay 0
      const uint64_t word = __ballot(bit);
      if (lane == 0) w[k] = word;
    }
    wave_lds_sync();
    xq = w;
  }
  __device__ __forceinline__ float row_dist(const SearchArgs &a, uint32_t slot) const {
    const uint64_t *__restrict__ y = a.bq_codes + (size_t)slot * W;
    return (W & 1u) == 0 ? bit_pair_dist<JACCARD, true>(xq, y, W) : bit_pair_dist<JACCARD, false>(xq, y, W);
  }
  __device__ __forceinline__ float one(const SearchArgs &a, uint32_t s, int) { return row_dist(a, s); }
  __device__ __forceinline__ void speculation(bool, const uint32_t *) {}
  __device__ __forceinline__ void ahead(const SearchArgs &, const uint32_t *, int, bool) {}
  __device__ __forceinline__ void skip(int) {}
  __device__ __forceinline__ void begin_row(const SearchArgs &, const uint32_t *, int) {}
  __device__ __forceinline__ void prefetch(const SearchArgs &, uint32_t, bool) {}
  __device__ __forceinline__ float hop(const SearchArgs &a, uint32_t nb, uint64_t pend, int lane) {
    if (!((pend >> lane) & 1ull)) return 0.0f;
    return row_dist(a, nb);
  }
};

// Fitted product quantizer whose per-query table does not fit beside a one-wave walk (M x K x 4 bytes > 64 KB:
// M = 192 at d = 768 is 192 KB).  Round 2 left that table in global memory and every lookup was a 4-byte gather from
// a 200 MB working set: 125 k QPS at 10M x 768 against 450 k for the full-precision walk.  Here ONE query owns a
// workgroup of four waves, one per SIMD, and with it a CU's LDS and register file:
//   * the table of sub-quantizer i (K floats) lives in LDS, or in the registers of one of the four waves (four
//     registers per table: lane l holds entries l, 64 + l, 128 + l, 192 + l; a lookup is four ds_bpermute and a
//     select -- the register file as a second, larger LDS);
//   * wave w owns the contiguous index range [w M/4, (w + 1) M/4): its first NL tables in LDS, its last RT in its
//     registers (M = 4 (NL + RT)).  Wave 0 is the walker: it runs search_body exactly as the one-wave kernels do
//     (candidate array, visited set, AddWithLimit).  Per adjacency chunk it publishes the row pointer, every wave
//     reads the row (lane j = edge j) and fetches its range of the neighbours' code bytes while the walker runs the
//     visited-set test; then all four look their table entries up in parallel;
//   * the sum is the reference's: dist = 0; dist += lut[i][code_i] for i = 0 .. M-1, plain fp32 adds in index order
//     (product.go:271-275).  The waves take turns -- wave 0 adds its M/4 values to 0 and hands the partial sums on
//     through LDS, wave 1 adds its own, ... -- so the adds happen in exactly the sequential order.
// Barriers per chunk (all four waves): B0 row published, B1 pending mask published, then one per wave's turn.
struct PQWideShared {
  unsigned long long rowp;  // mode 1: the adjacency chunk to expand
  uint32_t mode;            // 0: the walk is over, 1: expand rowp, 2: the single point `slot` (start node), 3: (split form) the merger inserts what it holds and names the next node
  uint32_t slot;
  unsigned long long pend;  // lanes whose neighbour passed CheckAndVisit
  // the split form (k_greedy_search_pqw<..., SPLIT>: the candidate array lives in a helper wave, the merger)
  uint32_t named;  // walker -> merger, with mode 1 / 3: the node the walk went to after the chunk the merger still holds, kNoSlot: the merger picks
  uint32_t next;   // merger -> walker, mode 3: the node it picked (marked), kNoSlot: no unvisited entry left
  uint32_t f1;     // merger -> walker: the first unvisited entry behind the node the walk went to, kNoSlot: none
  float f1d;
  float psum[64];           // partial sums on their way from wave to wave, by lane
};
constexpr uint32_t kPqwSharedWords = sizeof(PQWideShared) / 4;

// NL / RT: tables per wave in LDS / in registers (NL + RT a multiple of 16); W: waves per query, M = W (NL + RT).
// W = 8 (two waves per SIMD, 256 registers each) carries M = 384 with the per-wave layout of M = 192: round 3's
// four-wave form of it kept 64 tables = 256 registers per wave and spilled 80 more.
template <int NL, int RT, int W = 4>
struct PQWideDist {
  static constexpr Stage kStage = Stage::kNone;
  // Fetching ahead (search_body, Dist::kSpeculate) was built for this walk too -- every wave fetched the likely next
  // row at the start of a hop and its neighbours' codes at the end of it, so that 70 % of the hops started with both in
  // registers -- and measured no gain at two queries per CU (M = 192, 1M x 768: 1.089 ms per batch against 1.04 without,
  // twice the code traffic): the other query's waves already fill the waits.  Removed.
  static constexpr bool kSpeculate = false;
  static constexpr bool kHasStamps = false;
  static constexpr bool kPointDistances = false;
  static constexpr int MS = NL + RT;  // sub-quantizers per wave; M = 4 MS
  static constexpr int RTR = RT > 0 ? RT : 1;
  PQWideShared *sh;
  const float *lds_lut;  // this wave's LDS-resident tables, [NL][K]
  uint32_t K, lo;
  int wave;
  float T[RTR][4];    // register-resident tables
  // (a native vector type: copies of HIP's uint4 struct between members become 16-byte memcpys that keep the whole
  // policy object -- register tables included -- in scratch memory)
  typedef uint32_t code16 __attribute__((ext_vector_type(4)));
  code16 cw[MS / 16];  // the wave's range of the lane's neighbour's code bytes

  // All four waves: tables in, from the query's [M][K] block that pq_build_lut left in global memory.  (Computing the
  // entries here instead -- no 200 MB block written and read back per batch -- was built and measured: the loads and
  // chains of the build share the walk's register budget, and the two-per-CU variant went from 1.04 to 1.23 ms per
  // batch with a loop per entry, to 1.89 ms with the loads batched; removed.  The block costs 0.12 ms per batch.)
  // `before`: tables of the waves in front of this one in the workgroup's LDS block (w * NL when every wave has the same
  // split; the walker of the eight-wave form keeps more of its tables in LDS, k_greedy_search_pqw)
  __device__ __forceinline__ void init_wave(const SearchArgs &a, uint32_t q, int lane, int w, float *lut_lds, PQWideShared *shared,
                                            uint32_t before) {
    sh = shared, wave = w, K = a.pq_K, lo = (uint32_t)w * MS;

    float *dst = lut_lds + (size_t)before * K;
    lds_lut = dst;
    const float *g = a.pq_lut + ((size_t)q * a.pq_M + lo) * K;
    for (uint32_t i = lane; i < NL * K; i += 64) dst[i] = g[i];
#pragma unroll
    for (int t = 0; t < RT; t++)
#pragma unroll
      for (int c = 0; c < 4; c++) {
        const uint32_t e = c * 64 + lane;
        T[t][c] = e < K ? g[(size_t)(NL + t) * K + e] : 0.0f;
      }
  }
  __device__ __forceinline__ void load_codes(const SearchArgs &a, uint32_t nb) {
    const uint32_t s = nb == kNoSlot ? 0u : nb;  // lanes without a neighbour read row 0 and are never looked at
    const code16 *cp = reinterpret_cast<const code16 *>(a.pq_codes + (size_t)s * a.pq_M + lo);
#pragma unroll
    for (int j = 0; j < MS / 16; j++) cw[j] = cp[j];
  }
  template <int I>
  __device__ __forceinline__ uint32_t code_at() const {  // code byte I of the wave's range
    const code16 v = cw[I / 16];
    constexpr int wsel = (I / 4) % 4;
    const uint32_t word = wsel == 0 ? v.x : wsel == 1 ? v.y : wsel == 2 ? v.z : v.w;
    return (word >> (8 * (I % 4))) & 0xFFu;
  }
  template <int I>
  __device__ __forceinline__ float lookup() const {
    const uint32_t e = code_at<I>();
    if constexpr (I < NL) {
      return lds_lut[(size_t)I * K + e];
    } else {
      constexpr int t = I - NL;
      const int addr = (int)((e & 63u) << 2);
      const float v0 = __int_as_float(__builtin_amdgcn_ds_bpermute(addr, __float_as_int(T[t][0])));
      const float v1 = __int_as_float(__builtin_amdgcn_ds_bpermute(addr, __float_as_int(T[t][1])));
      const float v2 = __int_as_float(__builtin_amdgcn_ds_bpermute(addr, __float_as_int(T[t][2])));
      const float v3 = __int_as_float(__builtin_amdgcn_ds_bpermute(addr, __float_as_int(T[t][3])));
      const uint32_t c = e >> 6;
      return c == 0 ? v0 : c == 1 ? v1 : c == 2 ? v2 : v3;
    }
  }
  template <int I>
  __device__ __forceinline__ void lookups(float (&val)[MS]) const {
    if constexpr (I < MS) {
      val[I] = lookup<I>();
      lookups<I + 1>(val);
    }
  }
  // The turns: wave w adds its MS values, in index order, on top of what the waves before it left.  Returns the
  // finished sums (valid after the last turn) by lane.
  __device__ __forceinline__ float turns(const float (&val)[MS]) const {
    const int lane_ = threadIdx.x & 63;
#pragma unroll
    for (int stage = 0; stage < W; stage++) {
      if (stage == wave) {
        float acc = stage == 0 ? 0.0f : sh->psum[lane_];
#pragma unroll
        for (int i = 0; i < MS; i++) acc += val[i];  // product.go:271-275: dist += dists[i*K + code[i]]
        sh->psum[lane_] = acc;
      }
      __syncthreads();  // B2 + stage
    }
    return sh->psum[lane_];
  }

  // ---- the walker's side (wave 0): the policy interface search_body calls
  __device__ __forceinline__ void speculation(bool, const uint32_t *) {}
  __device__ __forceinline__ void ahead(const SearchArgs &, const uint32_t *, int, bool) {}
  uint32_t post_named = kNoSlot;  // split form: what begin_row tells the merger about the chunk before this one
  __device__ __forceinline__ void begin_row(const SearchArgs &, const uint32_t *rowp, int lane) {
    if (lane == 0) sh->rowp = reinterpret_cast<unsigned long long>(rowp), sh->mode = 1u, sh->named = post_named;
    __syncthreads();  // B0
  }
  // split form: the merger inserts the chunk it holds, picks the first unvisited entry and says which (B0, B1)
  __device__ __forceinline__ uint32_t ask_next(int lane) {
    if (lane == 0) sh->mode = 3u, sh->named = kNoSlot;
    __syncthreads();  // B0
    __syncthreads();  // B1: the answer is there
    return sh->next;
  }
  __device__ __forceinline__ void prefetch(const SearchArgs &a, uint32_t nb, bool) { load_codes(a, nb); }
  __device__ __forceinline__ void skip(int lane) {
    if (lane == 0) sh->pend = 0ull;
    __syncthreads();  // B1: nobody passed CheckAndVisit, the chunk ends here for every wave
  }
  __device__ __forceinline__ float hop(const SearchArgs &, uint32_t, uint64_t pend, int lane) {
    if (lane == 0) sh->pend = pend;
    __syncthreads();  // B1
    float val[MS];
    lookups<0>(val);  // the helpers did theirs while this wave ran the visited-set test
    return turns(val);
  }
  __device__ __forceinline__ float one(const SearchArgs &a, uint32_t s, int lane) {
    if (lane == 0) sh->slot = s, sh->mode = 2u, sh->named = kNoSlot;
    __syncthreads();  // B0
    load_codes(a, lane == 0 ? s : kNoSlot);
    return rlf(hop(a, s, 1ull, lane), 0);
  }
  __device__ __forceinline__ void finish(int lane) {
    if (lane == 0) sh->mode = 0u;
    __syncthreads();  // B0: the helpers leave
  }
  // ---- waves 1..3
  // MERGER (split form): this helper also owns the candidate array.  It keeps the chunk it has just helped to sum -- the
  // row's slots, the finished sums, the pending mask: every wave has them -- and runs AddWithLimit over it one round
  // LATER, after the next row's codes have been asked for and while the walker runs that row's visited-set test; then
  // it marks the node the walker went to and leaves the first unvisited entry behind it in sh->f1 before B1, which is
  // when the walker needs it: after that round's sums.  No polling: the walk's own barriers order every word.
  // (Pulling that entry's adjacency row through L2 here, as k_greedy_search_pq2's merger does, cost more than it hid:
  // 1.027 against 0.989 ms per batch at 2M x 768, M = 192 -- this wave is the one the round's second barrier waits for.)
  template <bool MERGER = false>
  __device__ __forceinline__ void serve(const SearchArgs &a, int lane, const uint32_t q = 0, uint32_t *scratch = nullptr) {
    constexpr int NREG = 2;
    uint32_t cid[MERGER ? NREG : 1];
    float cd[MERGER ? NREG : 1];
    int len = 0;
    const int cap = (int)a.search_size;
    uint32_t h_nb = kNoSlot;  // the chunk held back
    float h_d = 0.0f;
    uint64_t h_pend = 0;
    bool held = false;
    if constexpr (MERGER) {
#pragma unroll
      for (int r = 0; r < NREG; r++) cid[r] = kNoSlot, cd[r] = 0.0f;
    }
    // AddWithLimit over the chunk held back (distset.go:184-198), then the node the walk went to -- named by the walker,
    // or the first unvisited entry (search.go:66-71) -- is marked :74; answers in sh->next / f1 / f1d
    auto settle = [&](uint32_t named) {
      if constexpr (MERGER) {
        if (h_pend) add_with_limit_merge(cid, cd, len, cap, h_nb, h_d, h_pend, lane, scratch);
        held = false, h_pend = 0;
        uint32_t next, f1;
        float f1d;
        pick_and_mark(cid, cd, len, named, lane, next, f1, f1d);
        if (lane == 0) sh->next = next, sh->f1 = f1, sh->f1d = f1d;
      }
    };
    for (;;) {
      __syncthreads();  // B0
      const uint32_t mode = sh->mode;
      if (mode == 0u) break;
      if (mode == 3u) {
        if constexpr (MERGER) settle(kNoSlot);
        __syncthreads();  // B1
        continue;
      }
      const uint32_t named = sh->named;
      uint32_t nb;
      if (mode == 1u) nb = as_global(reinterpret_cast<const uint32_t *>(sh->rowp))[lane];  // (an adjacency row: device memory)
      else nb = lane == 0 ? sh->slot : kNoSlot;
      load_codes(a, nb);
      float val[MS];
      // one query per CU (512 registers per wave): the lookups run now, for every lane, pending or not, under the
      // walker's CheckAndVisit (1.59 -> 1.47 ms per batch at 1M x 768).  The two-per-CU variant has no registers to
      // keep 48 values across the barrier -- there it cost 1.38 -> 1.89 ms in spills -- and looks up after it.
      if constexpr (NL >= 16) lookups<0>(val);
      if constexpr (MERGER)
        if (held) settle(named);
      __syncthreads();  // B1
      const uint64_t pend = sh->pend;
      if constexpr (MERGER) held = true, h_nb = nb, h_pend = pend, h_d = 0.0f;
      if (pend == 0ull) continue;
      if constexpr (NL < 16) lookups<0>(val);
      const float sum = turns(val);
      if constexpr (MERGER) h_d = sum;
    }
    if constexpr (MERGER) {
      write_results(cid, cd, len, a.start_slot, lane, q, a);
    }
  }
};

}  // namespace sdb
