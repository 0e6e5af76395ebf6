// wave_dist.h -- the wave-level primitives every translation unit with a distance kernel shares: lane reads, the
// in-wave LDS ordering point, U pairs of exact distances per wave instruction (chunk_dist, chunk_dist_lds; dist_core.h
// rounds them like the reference) and the candidate array held in registers.  The walk kernels themselves:
// search_kernel.h.
#pragma once
#include "dist_core.h"

namespace sdb {

// pairs of candidate rows a wave keeps in flight per chunk.  DEEP (one wave per SIMD, the batch-search
// configuration: 4 waves per CU, the whole 512-entry register file available): ~190 VGPRs of loads;
// otherwise ~96 so that three waves per SIMD still fit (large build rounds).
template <int NG, bool DEEP>
struct ChunkPairs {
  static constexpr int base = NG <= 3 ? 8 : NG <= 4 ? 6 : NG <= 6 ? 4 : NG <= 8 ? 3 : NG <= 12 ? 2 : 1;
#ifndef SDB_DEEP3_PAIRS
#define SDB_DEEP3_PAIRS 16  // measurement builds: pairs per round of the d = 384 batch walk (tools/kernel_ab.py)
#endif
  static constexpr int value = DEEP ? (NG == 3 ? SDB_DEEP3_PAIRS : 2 * base) : base;  // DEEP: 32 / 24 / 16 / 12 / 8 / 4 rows in flight
};

template <class T>
__device__ __forceinline__ __attribute__((address_space(1))) T *as_global(T *p) {
  return (__attribute__((address_space(1))) T *)p;
}
// 1, 2 or 3 dwords of device memory at a 4-byte-aligned address, one load instruction
typedef uint32_t gwords2 __attribute__((ext_vector_type(2), aligned(4)));
typedef uint32_t gwords3 __attribute__((ext_vector_type(3), aligned(4)));
typedef const __attribute__((address_space(1))) char *gbytes;  // a byte address in device memory

__device__ __forceinline__ uint32_t rl(uint32_t v, int lane) {
  return (uint32_t)__builtin_amdgcn_readlane((int)v, lane);
}
__device__ __forceinline__ float rlf(float v, int lane) {
  return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), lane));
}

// Ordering point for LDS traffic inside ONE wavefront (the search kernels run one wave per workgroup): the
// LDS queue is in order per wave, so a ds_write is visible to the wave's later ds_reads without a barrier;
// only the compiler has to keep the order (and nothing waits for outstanding global loads, as a
// __syncthreads() would).
__device__ __forceinline__ void wave_lds_sync() {
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
}

// U pairs of (query, candidate) raw distances; slot[u] is this lane's candidate row (same for the
// 32 lanes of a half).  res[u] is valid in lanes 0 and 32.
template <int NG, bool L2, int U>
__device__ __forceinline__ void chunk_dist(const float *__restrict__ slab, uint32_t ld, uint32_t tail,
                                           const float4 (&xq)[NG > 0 ? NG : 1], float xt,
                                           const uint32_t (&slot)[U], float (&res)[U], int lane
#ifdef SDB_STAMPS
                                           , unsigned long long *st = nullptr
#endif
) {
  const int L = lane & 31;
  float4 y[U][NG > 0 ? NG : 1];
  float yt[U];
#ifdef SDB_STAMPS
  unsigned long long t0 = __builtin_amdgcn_s_memtime();
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#endif
#pragma unroll
  for (int u = 0; u < U; u++) {
    const float *row = slab + (size_t)slot[u] * ld;
    const float4 *r4 = reinterpret_cast<const float4 *>(row) + L;
#pragma unroll
    for (int g = 0; g < NG; g++) y[u][g] = r4[g * 32];
    yt[u] = tail ? row[NG * 128 + L] : 0.0f;
  }
#ifdef SDB_STAMPS
  unsigned long long t1 = __builtin_amdgcn_s_memtime();
  asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
  unsigned long long t2 = __builtin_amdgcn_s_memtime();
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#endif
#pragma unroll
  for (int u = 0; u < U; u++) {
    float acc = 0.0f;
#pragma unroll
    for (int g = 0; g < NG; g++) acc = chain4<L2>(acc, xq[g], y[u][g]);
    float t = tail ? tail_chain<L2>(xt, yt[u], tail, lane) : 0.0f;
    res[u] = asm_reduce(acc, t, lane);
  }
#ifdef SDB_STAMPS
  asm volatile("" ::"v"(res[U - 1]));
  unsigned long long t3 = __builtin_amdgcn_s_memtime();
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  if (st) st[0] += t1 - t0, st[1] += t2 - t1, st[2] += t3 - t2;  // issue, wait, compute
#endif
}

// Generic-dimension variant: the permuted query tile lives in LDS (qs, ng*32 float4 + 32 tail floats).
template <bool L2, int U>
__device__ __forceinline__ void chunk_dist_lds(const float *__restrict__ slab, uint32_t ld, uint32_t ng,
                                               uint32_t tail, const float *qs, const uint32_t (&slot)[U],
                                               float (&res)[U], int lane) {
  const int L = lane & 31;
  float acc[U];
  const float4 *r4[U];
#pragma unroll
  for (int u = 0; u < U; u++) {
    acc[u] = 0.0f;
    r4[u] = reinterpret_cast<const float4 *>(slab + (size_t)slot[u] * ld) + L;
  }
  const float4 *q4 = reinterpret_cast<const float4 *>(qs) + L;
  // four 128-float groups of every row per step: 4 * U row loads in flight instead of U; the partial sums
  // still take their groups in ascending order
  constexpr int GC = 4;
  for (uint32_t g0 = 0; g0 < ng; g0 += GC) {
    float4 y[U][GC];
#pragma unroll
    for (int k = 0; k < GC; k++)
      if (g0 + k < ng) {
#pragma unroll
        for (int u = 0; u < U; u++) y[u][k] = r4[u][(g0 + k) * 32];
      }
#pragma unroll
    for (int k = 0; k < GC; k++)
      if (g0 + k < ng) {
        const float4 x = q4[(g0 + k) * 32];
#pragma unroll
        for (int u = 0; u < U; u++) acc[u] = chain4<L2>(acc[u], x, y[u][k]);
      }
  }
  float xt = tail ? qs[ng * 128 + L] : 0.0f;
#pragma unroll
  for (int u = 0; u < U; u++) {
    float yt = tail ? slab[(size_t)slot[u] * ld + ng * 128 + L] : 0.0f;
    float t = tail ? tail_chain<L2>(xt, yt, tail, lane) : 0.0f;
    res[u] = asm_reduce(acc[u], t, lane);
  }
}

typedef _Float16 sk_h2 __attribute__((ext_vector_type(2)));
// float -> float16 as the sketch stores it: round to nearest, magnitudes below the smallest NORMAL half become 0 (no
// denormal half is ever an operand of v_dot2_f32_f16, whatever the mode register says about them); what this loses is
// part of the measured error ||v - v16||, not an assumption
__device__ __forceinline__ _Float16 sk_half(float v) { return fabsf(v) < 6.103515625e-5f ? (_Float16)0.0f : (_Float16)v; }

// ---- the candidate array (DistSet.items, distset.go:133-138) held in registers -------------------------
// entry e lives in lane e % 64 of register e / 64; bit 31 of the slot word is the `visited` flag.

// bubble position + shift of DistSet.AddWithLimit (distset.go:189-198) for one accepted point
template <int NREG>
__device__ __forceinline__ void list_insert(uint32_t (&cid)[NREG], float (&cd)[NREG], int &len, int cap, uint32_t id,
                                            float d, int lane) {
  const bool full = (len == cap);
  const int newlen = full ? len : len + 1;  // :189-194 append, or overwrite the tail
  const int range = newlen - 1;             // entries the bubble loop compares against
  int pos = 0;                              // :196-198 stops at the first i with !(d < items[i-1])
#pragma unroll
  for (int r = 0; r < NREG; r++) {
    uint64_t m = __ballot((r * 64 + lane) < range && !(d < cd[r]));
    if (m) pos = r * 64 + 64 - __clzll(m);
  }
#pragma unroll
  for (int r = NREG - 1; r >= 0; r--) {
    // entry e-1 -> e: one v_mov_b32_dpp wave_shr:1 per register; lane 0 takes the carry (lane 63 of the
    // previous register) through the DPP `old` operand
    uint32_t c_id = 0;
    float c_d = 0.0f;
    if (r > 0) c_id = rl(cid[r - 1], 63), c_d = rlf(cd[r - 1], 63);
    const uint32_t up_id = (uint32_t)__builtin_amdgcn_update_dpp((int)c_id, (int)cid[r], 0x138, 0xf, 0xf, false);
    const float up_d =
        __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(c_d), __float_as_int(cd[r]), 0x138, 0xf, 0xf, false));
    const int e = r * 64 + lane;
    if (e > pos && e < newlen) cid[r] = up_id, cd[r] = up_d;
    else if (e == pos) cid[r] = id, cd[r] = d;
  }
  len = newlen;
}

template <int NREG>
__device__ __forceinline__ float list_tail(const float (&cd)[NREG], int cap) {
  float t = 0.0f;
#pragma unroll
  for (int r = 0; r < NREG; r++)
    if (((cap - 1) >> 6) == r) t = rlf(cd[r], (cap - 1) & 63);
  return t;
}

}  // namespace sdb
