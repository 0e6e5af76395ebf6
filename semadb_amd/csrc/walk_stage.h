// walk_stage.h -- K2: the two-precision hop's first stage, one implementation over two formats of the copy.
// (a part of search_kernel.h, which includes it after what it builds on; no .hip file includes it directly)
#pragma once

namespace sdb {

// ---- the two-precision hop's first stage (SearchArgs::sketch, SDB_TUNE_SKETCH): one implementation (FirstStage) over
// two formats of the copy.  A format says how the query is converted and its error measured, how one copy row is
// loaded and summed per lane, and how a complete sum becomes the dot product the verdict looks at.

// The float16 format: rows of `ld` halves in the slab's element order; lane L's 4 elements of group g at byte
// 256 g + 8 L of the row (NG loads per row, 256 bytes apart).
template <int NG, bool L2>
struct HalfRows {
  typedef float sum_t;
  struct row_t { uint2 g[NG]; };
  static constexpr int kLaneBytes = 8, kElemBytes = 2;
  static constexpr bool kCompacts = true;  // rows that were not asked for ahead are read by rank through LDS (range)
  // pairs of rows in flight per round of that path -- all of a hop's new neighbours in ONE round where the registers allow
  // it, 2 NG registers per row: a round is a dependent memory round trip of the hop
  static constexpr int kBudget = L2 ? 72 : 96;  // (the euclidean exact stage holds differences as well)
  static constexpr int kRound = 32 < kBudget / NG ? 32 : kBudget / NG;
  sk_h2 qh[NG][2];      // the query in float16, in xq's element order
  float qq, delta, yy;  // euclidean: ||q16||^2; ||q - q16|| + max ||y - y16|| (rounded up); rows ahead: ||y16||^2 of this lane's edge

  // The bound.  With q16, y16 the float16 copies (exact in float32): q.y - q16.y16 = (q - q16).y16 + q.(y - y16), so
  // |q.y - q16.y16| <= ||q - q16|| Ymax16 + ||q|| Emax (Cauchy-Schwarz; Emax, Ymax16 measured over all rows by
  // k_sketch_rows, ||q - q16|| and ||q|| measured here).  The two computed sums differ from the exact ones by their
  // rounding: the reference's 32 chains of NG x 4 / 32 ... fused multiply-adds and its 6-level tree, at most 4 NG + 6
  // roundings of relative size 2^-24 on sums bounded by ||q|| ||y||; the sketch's 2 NG v_dot2_f32_f16 (products of
  // halves are exact in float32, three additions each) and the same tree: 6 NG + 6.  For NG <= 8 that is below
  // 110 x 2^-24 = 6.6e-6; 2e-5 ||q|| (Ymax16 + Emax) is charged (stage_eps).  Norms are inflated by 1e-4 for their own
  // rounding; the final 1 - dot / -dot and the subtraction of the bound are covered per comparison (FirstStage::out).  A
  // query or a table with a non-finite or float16-overflowing element makes the bound infinite or NaN: nothing is
  // discarded then.
  __device__ __forceinline__ void query(const float4 (&xq)[NG], int lane, ColdArgs &c, float &qerr, float &qn) {
    float e2 = 0.0f, n2 = 0.0f;
#pragma unroll
    for (int g = 0; g < NG; g++) {
      const float v[4] = {xq[g].x, xq[g].y, xq[g].z, xq[g].w};
      _Float16 h[4];
#pragma unroll
      for (int k = 0; k < 4; k++) {
        h[k] = sk_half(v[k]);
        const float dv = v[k] - (float)h[k];
        e2 = __builtin_fmaf(dv, dv, e2), n2 = __builtin_fmaf(v[k], v[k], n2);
      }
      qh[g][0] = sk_h2{h[0], h[1]}, qh[g][1] = sk_h2{h[2], h[3]};
    }
    // (both halves of the wave hold the same query: the sum over one half's 32 lanes)
    e2 = rlf(asm_reduce(e2, 0.0f, lane), 0), n2 = rlf(asm_reduce(n2, 0.0f, lane), 0);
    qerr = __builtin_sqrtf(e2) * 1.0001f, qn = __builtin_sqrtf(n2) * 1.0001f;
    if constexpr (L2) {
      float hh = 0.0f;
#pragma unroll
      for (int g = 0; g < NG; g++) {
        const float h0 = (float)qh[g][0][0], h1 = (float)qh[g][0][1], h2 = (float)qh[g][1][0], h3 = (float)qh[g][1][1];
        hh = __builtin_fmaf(h0, h0, hh), hh = __builtin_fmaf(h1, h1, hh), hh = __builtin_fmaf(h2, h2, hh), hh = __builtin_fmaf(h3, h3, hh);
      }
      qq = rlf(asm_reduce(hh, 0.0f, lane), 0);
      delta = (qerr + c.sk_emax) * 1.0001f;
    }
  }
  static __device__ __forceinline__ void load(row_t &y, gbytes r) {
#pragma unroll
    for (int g = 0; g < NG; g++) {
      const gwords2 p = *(const __attribute__((address_space(1))) gwords2 *)(r + g * 256);
      y.g[g] = make_uint2(p.x, p.y);
    }
  }
  __device__ __forceinline__ float partial(const row_t &y) const {
    float acc = 0.0f;
#pragma unroll
    for (int g = 0; g < NG; g++) {
      acc = __builtin_amdgcn_fdot2(__builtin_bit_cast(sk_h2, y.g[g].x), qh[g][0], acc, false);
      acc = __builtin_amdgcn_fdot2(__builtin_bit_cast(sk_h2, y.g[g].y), qh[g][1], acc, false);
    }
    return acc;
  }
  __device__ __forceinline__ float dot(float sum16) const { return sum16; }

  // Squared euclidean distance.  With D16 = ||q16 - y16||^2 (exact) and delta >= ||q - q16|| + ||y - y16||:
  // | sqrt(D) - sqrt(D16) | <= delta, so D >= D16 - 2 delta sqrt(D16) (when sqrt(D16) < delta the right side is
  // negative and proves nothing, as it should).  D16 is computed as ||q16||^2 + ||y16||^2 - 2 q16.y16 from three rounded
  // sums: its error is below 1e-5 (||q16||^2 + ||y16||^2 + 2 |q16.y16|) (the same roundings as the dot form, 2^-24 each for
  // the two norms, three more for the combination -- well under 100 x 2^-24 = 6e-6).  The reference's own sum of rounded
  // squares of rounded differences is within (NG x 4 + 10) x 2^-24 < 1e-5 of D, relatively (all terms are >= 0).
  __device__ __forceinline__ bool out_l2(float sum16, float yy_row, float tail_d) const {
    const float d16 = (qq + yy_row) - 2.0f * sum16;
    const float err = 1e-5f * (qq + yy_row + 2.0f * fabsf(sum16)) + 1e-30f;
    const float up = d16 + err;  // D16 <= up
    const float root = __builtin_sqrtf(up > 0.0f ? up : 0.0f) * 1.00001f;  // >= sqrt(D16)
    const float lower = ((d16 - err) - 2.0f * delta * root) * (1.0f - 2e-5f);  // <= the reference's distance, rounding of this line included below
    return lower - 1e-6f * (fabsf(d16) + err + delta * root) > tail_d;  // (the roundings of the two lines above; a NaN anywhere: false)
  }

  // float16 dot products of the pending rows by rank, two rows per wave instruction like PlainDist::rows_range; `dump`
  // takes the writes of the lanes that hold no result
  __device__ __forceinline__ void range(const SearchArgs &a, const uint32_t *s_slot, float *s_res, float *dump, int cnt, int lane) const {
    const int L = lane & 31, half = lane >> 5;
    const gbytes baseL = as_global(static_cast<const char *>(cold_args(a).sketch)) + L * kLaneBytes;
    const uint32_t row_bytes = a.ld * kElemBytes;
    for (int c0 = 0; c0 < cnt; c0 += 2 * kRound) {
      const int m = cnt - c0 < 2 * kRound ? cnt - c0 : 2 * kRound;
      const int h0 = (m + 1) >> 1;
      const int base = c0 + (half ? h0 : 0);
      uint32_t sl[kRound];
#pragma unroll
      for (int u = 0; u < kRound; u++) sl[u] = s_slot[base + u];
      row_t y[kRound];
#pragma unroll
      for (int u = 0; u < kRound; u++)
        if (u < h0) load(y[u], baseL + (uint64_t)sl[u] * row_bytes);
      float *wp = (L == 0) ? s_res + base : dump;
#pragma unroll
      for (int u = 0; u < kRound; u++)
        if (u < h0) wp[u] = asm_reduce(partial(y[u]), 0.0f, lane);
    }
  }
};

// The int8 format (SDB_TUNE_SKETCH = 3; cosine / dot, rows of 128 .. 384 floats): the index keeps
// y8 = clamp(rint(y / s), -127, 127) of every row, one scale s per table (index_sketch.hip k_sketch8_rows), in place of the
// float16 copy -- half the bytes of the stage that reads a row for every edge of every hop.  A copy row is ld bytes; lane
// L's 4 NG bytes of it are contiguous (bytes [4 NG L, 4 NG (L + 1)): group g's elements 4 L .. 4 L + 3 at + 4 g), so a
// lane asks for a row with ONE load of NG dwords.
//
// The query becomes two int8 terms once per wave: with s_q = max |q_i| / 127, a = clamp(rint(q / s_q)) and
// b = clamp(rint((q - s_q a) 128 / s_q)) (the residual of a, |b| <= 64), q^ = (s_q / 128) (128 a + b).  Per row and lane
// W = (sum a y8 << 7) + sum b y8 from 2 NG v_dot4_i32_i8 -- an exact integer, |W| <= 16 320 x 127 x 384 < 2^31 -- and the
// 32 sums of a hop go through the transposing butterfly as INTEGER adds: nothing is rounded before the one conversion
// d8 = metric_finish((s s_q / 128) float(W)), and q^ . y^ = (s s_q / 128) W exactly with y^ = s y8.
//
// The bound, as for the float16 format: q.y - q^.y^ = (q - q^).y^ + q.(y - y^), so |q.y - q^.y^| <= ||q - q^|| Y8max +
// ||q|| E8max (Cauchy-Schwarz; E8max = max ||y - s y8|| and Y8max = max ||s y8|| measured in double over all rows and
// rounded up by k_sketch8_rows; ||q - q^|| and ||q|| measured here).  ||q - q^|| is measured against the float32 value
// of q^_i, one rounding (2^-24 |q^_i|) away from the exact product: 2e-7 ||q|| is added.  The reference's float32 chain
// and tree round 4 NG + 6 times (2^-24 each, on sums bounded by ||q|| ||y||); d8's scale product, conversion and
// multiplication three times: below 21 x 2^-24 = 1.3e-6 for NG <= 3, and 2e-5 ||q|| (Y8max + E8max) is charged, the
// term the float16 format charges (stage_eps).  Norms are inflated by 1e-4 for their own rounding; the final 1 - dot /
// -dot and the subtraction of the bound are covered per comparison (FirstStage::out: 4e-7 of the magnitudes, which also
// covers a scale product that underflows).  A query or a table with a non-finite element makes the bound infinite or
// NaN: nothing is discarded then.  A survivor goes straight to the float32 stage (PlainDist::hop): reference order,
// same bits.
template <int NG>
struct Int8Rows {
  static_assert(stage_int8(NG, false, false), "a hop's 64 int8 rows are held in 32 NG registers");
  typedef int sum_t;
  struct row_t { uint32_t w[NG]; };
  static constexpr int kLaneBytes = 4 * NG, kElemBytes = 1;
  static constexpr bool kCompacts = false;  // (never needed: the rows are asked for ahead whenever the array is full)
  uint32_t qa[NG], qb[NG];  // four int8 each, in xq's element order
  float scale;              // s s_q / 128

  __device__ __forceinline__ void query(const float4 (&xq)[NG], int lane, ColdArgs &c, float &qerr, float &qn) {
    float mx = 0.0f;
#pragma unroll
    for (int g = 0; g < NG; g++)
      mx = fmaxf(mx, fmaxf(fmaxf(fabsf(xq[g].x), fabsf(xq[g].y)), fmaxf(fabsf(xq[g].z), fabsf(xq[g].w))));
    // (fmaxf drops a NaN: a query with one is caught by the measured error below, which becomes NaN)
#pragma unroll
    for (int o = 16; o; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o));
    const float sq = mx / 127.0f, inv = sq > 0.0f ? 1.0f / sq : 0.0f, sq128 = sq * 0.0078125f;
    float e2 = 0.0f, n2 = 0.0f;
#pragma unroll
    for (int g = 0; g < NG; g++) {
      const float v[4] = {xq[g].x, xq[g].y, xq[g].z, xq[g].w};
      uint32_t pa = 0, pb = 0;
#pragma unroll
      for (int k = 0; k < 4; k++) {
        const float fa = fminf(fmaxf(__builtin_rintf(v[k] * inv), -127.0f), 127.0f);
        const float fb = fminf(fmaxf(__builtin_rintf((v[k] - sq * fa) * inv * 128.0f), -127.0f), 127.0f);
        const float dv = v[k] - sq128 * (fa * 128.0f + fb);  // (128 a + b is exact in float32)
        e2 = __builtin_fmaf(dv, dv, e2), n2 = __builtin_fmaf(v[k], v[k], n2);
        pa |= ((uint32_t)(int)fa & 0xFFu) << (8 * k), pb |= ((uint32_t)(int)fb & 0xFFu) << (8 * k);
      }
      qa[g] = pa, qb[g] = pb;
    }
    // (both halves of the wave hold the same query: the sum over one half's 32 lanes)
    e2 = rlf(asm_reduce(e2, 0.0f, lane), 0), n2 = rlf(asm_reduce(n2, 0.0f, lane), 0);
    qn = __builtin_sqrtf(n2) * 1.0001f, qerr = __builtin_sqrtf(e2) * 1.0001f + 2e-7f * qn;
    scale = c.sk8_scale * sq128;
  }
  static __device__ __forceinline__ void load(row_t &y, gbytes r) {
    if constexpr (NG == 1) {
      y.w[0] = *(const __attribute__((address_space(1))) uint32_t *)r;
    } else if constexpr (NG == 2) {
      const gwords2 p = *(const __attribute__((address_space(1))) gwords2 *)r;
      y.w[0] = p.x, y.w[1] = p.y;
    } else {
      const gwords3 p = *(const __attribute__((address_space(1))) gwords3 *)r;
      y.w[0] = p.x, y.w[1] = p.y, y.w[2] = p.z;
    }
  }
  __device__ __forceinline__ int partial(const row_t &y) const {
    int sa = 0, sb = 0;
#pragma unroll
    for (int g = 0; g < NG; g++) {
      sa = __builtin_amdgcn_sdot4((int)y.w[g], (int)qa[g], sa, false);
      sb = __builtin_amdgcn_sdot4((int)y.w[g], (int)qb[g], sb, false);
    }
    return sa * 128 + sb;
  }
  __device__ __forceinline__ float dot(int w) const { return scale * (float)w; }
};

// One stage of the transposing butterfly: at stride S a lane keeps the rows whose bit S equals its own and hands the
// others to lane ^ S.
// No exchange goes through the LDS pipe (each was a ds_swizzle behind two selects):
//   * stride 16: v_permlane16_swap(w[i], w[i + 16]) leaves, in every lane, what it keeps in one register and what it
//     receives in the other -- the result is their sum;
//   * strides 8 .. 1: a lane keeps w[i] and receives its partner's w[i], or the same of w[i + S]: both sums as DPP adds
//     (row_ror:8; row_shl:4 for the lanes that keep w[i], row_shr:4 for the others; quad_perm), one select between
//     them -- a lane a shift reads from outside its row adds 0 to the sum the select does not take.
// (keep + received or received + keep: float adds commute, the float16 stage's bits are what they were.)
template <int CTRL, class T>
__device__ __forceinline__ T dpp_from(T v) {  // v of the lane CTRL names (0 from outside the row)
  return __builtin_bit_cast(T, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, 0xf, 0xf, true));
}
template <int S, class T>
__device__ __forceinline__ void butterfly_stage(T (&w)[32], int lane) {
#pragma unroll
  for (int i = 0; i < S; i++) {
    if constexpr (S == 16) {
      const auto sw = __builtin_amdgcn_permlane16_swap(__builtin_bit_cast(uint32_t, w[i]), __builtin_bit_cast(uint32_t, w[i + S]), false, false);
      w[i] = __builtin_bit_cast(T, (uint32_t)sw[0]) + __builtin_bit_cast(T, (uint32_t)sw[1]);
    } else {
      // lane ^ S, for the lanes without / with bit S
      constexpr int kLo = S == 8 ? 0x128 : S == 4 ? 0x104 : S == 2 ? 0x4E : 0xB1, kHi = S == 4 ? 0x114 : kLo;
      const T lo = w[i] + dpp_from<kLo>(w[i]), hi = w[i + S] + dpp_from<kHi>(w[i + S]);
      w[i] = (lane & S) ? hi : lo;
    }
  }
}
// 32 sums per half-wave (pair u: edge 2u in lanes 0..31, edge 2u + 1 in lanes 32..63), each spread over the 32 lanes.
// Instead of 32 reductions that each end in one lane (and a trip through LDS to get edge j's sum to lane j), one
// transposing butterfly: 16 + 8 + 4 + 2 + 1 exchanges instead of 32 x 5, and lane L of a half ends with the complete sum
// of pair L.  One ds_bpermute then puts edge j's sum into lane j.  (Any order of additions is within the float16 bound,
// and integer sums are exact; no LDS memory is touched.)
template <class T>
__device__ __forceinline__ T edge_sums(T (&w)[32], int lane) {
  butterfly_stage<16>(w, lane), butterfly_stage<8>(w, lane), butterfly_stage<4>(w, lane), butterfly_stage<2>(w, lane);
  butterfly_stage<1>(w, lane);
  // lane 32 h + L holds edge 2 L + h: lane j takes its own from lane 32 (j & 1) + (j >> 1)
  return __builtin_bit_cast(T, __builtin_amdgcn_ds_bpermute(((lane & 1) * 32 + (lane >> 1)) * 4, __builtin_bit_cast(int, w[0])));
}

// bound on |first-stage dot product - the reference's float32 one| for a query, any row (derived above each format)
__device__ __forceinline__ float stage_eps(float qerr, float qn, float ymax, float emax) {
  return (qerr * ymax + qn * emax + 2e-5f * qn * (ymax + emax)) * 1.0001f;
}

// A float32-only walk carries no stage state.  (Held as a plain one-byte member, not [[no_unique_address]] and not an empty
// base: when the int8 walk at NG = 3 took 228 VGPRs, either moved Int8Dist's members and cost it one, 229, and a stage as
// a base in front of xq measured 235.  Re-measured with the hop's loads issued in every hop, 184 VGPRs:
// [[no_unique_address]] makes no difference any more; the layout is left as it was.)
struct NoStage {};

template <class Fmt, bool L2, bool AHEAD>
struct FirstStage {
  typedef typename Fmt::row_t row_t;
  typedef typename Fmt::sum_t sum_t;
  Fmt fmt;
  float eps;  // stage_eps of this query
  // Rows of up to 384 floats (stage_ahead): the copy rows of ALL 64 edges of an adjacency row fit the register file, so
  // they are asked for as soon as the edge ids are there -- BEFORE the visited-set test, whose LDS round trips (~2 100
  // cycles) then run under the rows' flight instead of in front of it.  That only happens if nothing between the loads
  // and the test waits for them: the loads are global loads (the copy's address is typed as device memory; as flat loads
  // they could only be drained whole, and were, in front of the test), they are issued in every hop, not only with the
  // array full (registers that are loaded on one side of a branch are copied into place, with a wait, on that side),
  // and the first wait on them is the counted one in front of the first sum (tests/test_stage_load_schedule.py reads
  // all of this from the built library).  Rows of edges that turn out to be visited already were read for nothing (a
  // quarter more copy bytes; the walk is not bound by bytes), and so are the rows of the hops before the array is full
  // (at searchSize 75 the first two hops of about 79).  (Asking after the test, compacted, was the measured alternative
  // and lost; HISTORY.md keeps the figures.)
  bool loaded = false;
  row_t y[AHEAD ? 32 : 1];  // pair u: edge 2u (lanes 0..31) and edge 2u + 1 (lanes 32..63); (kept last: with the rows in
                            // front of the flag the int8 walk at NG = 3 took 233 registers for 228; at today's 184 the
                            // order makes no difference, re-measured)

  template <int NG>
  __device__ __forceinline__ void init(const SearchArgs &a, const float4 (&xq)[NG], int lane) {
    ColdArgs &c = cold_args(a);  // (what only the hop reads: through the opaque view, not parked in SGPRs)
    float qerr, qn;
    fmt.query(xq, lane, c, qerr, qn);
    eps = stage_eps(qerr, qn, c.sk_ymax, c.sk_emax);
  }

  // A hop asks for its copy rows ahead; `loaded` says whether keep() may use them (the array is full).  The walk is
  // launched only with the copy (walk_plan.h: the staged families), so the pointer need not be tested -- and untested, the compiler
  // sees that keep()'s compacting path is never taken with the rows asked for ahead: 87 -> 14 spilled SGPRs at NG = 3
  // (cosine / dot).  The euclidean walk keeps the test (through the opaque view) in front of its loads: untested, this
  // compiler spills 4 VGPRs there; tested, none.
  __device__ __forceinline__ void begin(const SearchArgs &a, uint32_t nb, bool valid, bool full) {
    if constexpr (AHEAD) {
      loaded = false;
      if constexpr (L2)
        if (cold_args(a).sketch == nullptr) return;
      const int lane = (int)__builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u));
      const int L = lane & 31;
      const bool hi = lane >= 32;
      // (the copy's addresses through the opaque view at each use: one scalar load, in flight beside the adjacency
      // row's, where arguments that live through the walk would hold SGPR pairs spilled into VGPR lanes --
      // tools/kernel_table.py)
      const gbytes baseL = as_global(static_cast<const char *>(cold_args(a).sketch)) + L * Fmt::kLaneBytes;
      const uint32_t row_bytes = a.ld * Fmt::kElemBytes;
      const uint32_t safe = valid ? nb : a.start_slot;  // an edge that is not there: any row (its result is not looked at)
      // pair u's slot: edge 2u for lanes 0..31, edge 2u + 1 for lanes 32..63 -- ONE ds_bpermute of `safe` from lane
      // 2u + hi, the constant 8u in the instruction's offset field (two readlanes, two moves and a select before);
      // with the 64-bit mad that is two vector instructions in front of a row's load
      // (`pick` is made opaque per hop: as a value the compiler knows across hops, the 32 sums pick + 8u were hoisted
      // out of the walk into 32 registers; inside the hop they fold into the offset field)
      int pick = hi ? 4 : 0;
      asm volatile("" : "+v"(pick));
#pragma unroll
      for (int u = 0; u < 32; u++) {
        const uint32_t s = (uint32_t)__builtin_amdgcn_ds_bpermute(pick + 8 * u, (int)safe);
        Fmt::load(y[u], baseL + (uint64_t)s * row_bytes);
      }
      if constexpr (L2) fmt.yy = as_global(cold_args(a).sketch_norm)[safe];
      loaded = full;
    }
  }

  // is the neighbour's reference distance provably above `tail_d`?  (every comparison with a NaN is false)
  __device__ __forceinline__ bool out(const SearchArgs &a, sum_t sum, float yy, float tail_d) const {
    if constexpr (L2) {
      return fmt.out_l2(sum, yy, tail_d);
    } else {
      const float d = metric_finish(fmt.dot(sum), a.metric);
      // (1 - dot, -dot and the subtraction below round once each: 3 x 2^-24 of magnitudes below 1 + |d| + eps)
      const float slack = eps + 4e-7f * (1.0f + fabsf(d) + eps);
      return d - slack > tail_d;
    }
  }

  // the pending neighbours that AddWithLimit may keep: `out` gets the ones whose first-stage distance is above `tail_d`
  // by more than the bound (a NaN: such a neighbour is kept for the exact evaluation).  hs: the policy's hop scratch,
  // slots by rank [hop_slots], sums by rank [hop_slots], a dump.
  __device__ __forceinline__ uint64_t keep(const SearchArgs &a, uint32_t *hs, uint32_t hop_slots, uint32_t nb, uint64_t pend,
                                           int lane, float tail_d, uint64_t &outm) {
    if constexpr (AHEAD) {
      if (loaded) {  // the rows are in registers, by edge position
        sum_t w[32];
#pragma unroll
        for (int u = 0; u < 32; u++) w[u] = fmt.partial(y[u]);
        const sum_t mysum = edge_sums(w, lane);
        const bool mine = (pend >> lane) & 1ull;
        float yy = 0.0f;
        if constexpr (L2) yy = fmt.yy;
        const bool above = out(a, mysum, yy, tail_d);  // (for every lane: no branch around the arithmetic)
        outm = __ballot(mine && above);
        return pend & ~outm;
      }
    }
    if constexpr (Fmt::kCompacts) {
      const int cnt = __popcll(pend);
      const bool mine = (pend >> lane) & 1ull;
      float yy_me = 0.0f;
      if constexpr (L2)
        if (mine) yy_me = as_global(cold_args(a).sketch_norm)[nb];  // (in flight while the rows are summed)
      const uint32_t rank =
          __builtin_amdgcn_mbcnt_hi((uint32_t)(pend >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)pend, 0u));
      uint32_t *s_slot = hs;
      float *s_res = reinterpret_cast<float *>(hs + hop_slots);
      if (mine) {
        s_slot[rank] = nb;
        if ((int)rank == cnt - 1) s_slot[cnt] = nb;  // the spare entry
      }
      wave_lds_sync();
      fmt.range(a, s_slot, s_res, s_res + hop_slots, cnt, lane);
      wave_lds_sync();
      outm = __ballot(mine && out(a, s_res[rank], yy_me, tail_d));
      wave_lds_sync();  // hop() compacts into the same scratch
      return pend & ~outm;
    } else {
      outm = 0;
      return pend;
    }
  }
};

// the stage a PlainDist holds itself: the float16 one (the int8 stage is held by its subclass, Int8Dist)
template <int NG, bool L2, Stage ST>
struct StageOf { typedef NoStage type; };
template <int NG, bool L2>
struct StageOf<NG, L2, Stage::kHalf> { typedef FirstStage<HalfRows<NG, L2>, L2, stage_ahead(NG)> type; };

}  // namespace sdb
