// cand_array.h -- K2: the candidate array in registers and what the walks do with it.
// (a part of search_kernel.h, which includes it after what it builds on; no .hip file includes it directly)
#pragma once

namespace sdb {

// ---- the candidate array (DistSet.items, distset.go:133-138) held in registers -------------------------
// entry e lives in lane e % 64 of register e / 64; bit 31 of the slot word is the `visited` flag.
// (list_insert and list_tail, which the flat scan shares: wave_dist.h)

// The filtered walk's array is NOT sorted (its seeds are appended by Add, distset.go:203-211, and AddWithLimit bubbles a
// point left only while it is `<` its neighbour, :193-198), so its last distance can RISE while a chunk's points are
// inserted: the new last entry is the old second-to-last one.  What holds instead: one kept insertion puts x <= tail
// somewhere and shifts the entries behind it right by one, so the last m + 1 entries of the new array lie within {x}
// plus the last m + 2 of the old one, and x is at most one of those -- by induction the tail after j insertions is at
// most the maximum of the ORIGINAL last j + 1 entries.  The i-th of a chunk's k new neighbours meets the array after at
// most i <= k - 1 insertions: a neighbour whose distance is above the maximum of the last min(k, cap) distances, as the
// chunk starts, is discarded at its turn whatever happens before it.  (Sorted array: that maximum is the tail.)
// A NaN among those distances makes the result NaN (`d > NaN` is false: nothing is discarded in that chunk) -- a plain
// fmaxf reduction would drop it.  Wave-uniform result.
template <int NREG>
__device__ __forceinline__ float list_tail_bound(const float (&cd)[NREG], int cap, int k, int lane) {
  const int first = k < cap ? cap - k : 0;
  float m = __int_as_float(0xff800000);  // -inf
  bool nan = false;
#pragma unroll
  for (int r = 0; r < NREG; r++) {
    const int e = r * 64 + lane;
    if (e >= first && e < cap) nan |= cd[r] != cd[r], m = fmaxf(m, cd[r]);
  }
#pragma unroll
  for (int o = 32; o; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
  return __ballot(nan) ? __int_as_float(0x7fc00000) : m;
}

// AddWithLimit (distset.go:184-198) over the lanes in `pd`, IN LANE ORDER, each lane holding (idreg,
// mydist).  Every pending lane is tested against the tail AS IT IS NOW, again after every insertion, and the first that
// passes is inserted; the lanes in front of it failed the tail they met at their turn and are dropped.  The re-test is
// what makes this the reference's replay for an UNSORTED array too (the filtered walk's: there the tail can rise with
// an insertion, and a lane behind the inserted one may pass a tail that an earlier tail would have refused).
template <int NREG>
__device__ __forceinline__ void add_with_limit_lanes(uint32_t (&cid)[NREG], float (&cd)[NREG], int &len, int cap,
                                                     uint32_t idreg, float mydist, uint64_t pd, int lane) {
  while (pd) {
    bool ok = true;
    if (len == cap) ok = !(mydist > list_tail(cd, cap));  // :184 strict '>'
    const uint64_t am = __ballot(ok) & pd;
    if (!am) break;
    const int j = __ffsll((unsigned long long)am) - 1;
    const float d = rlf(mydist, j);
    const uint32_t id = rl(idreg, j);
    pd = (j == 63) ? 0ull : ((pd >> (j + 1)) << (j + 1));
    list_insert(cid, cd, len, cap, id, d, lane);
  }
}

// The same AddWithLimit over several points at once, for a FULL and SORTED candidate array (the unfiltered
// search after its first hops).  With no two equal distances among the array and the points that beat the
// tail, replaying them one by one ends in exactly one state: the `cap` smallest of (array U points), in
// order -- so that state is computed directly: every array entry moves up by the number of points below
// it, every point lands at (#entries below it + #points below it), entries pushed past `cap` vanish.  The
// scatter goes through a 2*NREG*64-word LDS scratch.  Any tie, NaN, or a not-yet-full array falls back to
// the one-by-one replay, which is the specification.  FEW: fewer candidates than this are replayed one by one as well
// (the two-precision hop hands over ~5 points per hop, not ~50: the scatter's fixed cost is not worth it then).
template <int NREG, int FEW = 2>
__device__ __forceinline__ void add_with_limit_merge(uint32_t (&cid)[NREG], float (&cd)[NREG], int &len, int cap,
                                                     uint32_t idreg, float mydist, uint64_t pd, int lane,
                                                     uint32_t *scratch
#ifdef SDB_STAMPS
                                                     , unsigned long long *mst = nullptr
#endif
) {
#ifdef SDB_STAMPS
  unsigned long long m_t0 = __builtin_amdgcn_s_memtime();
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#define SDB_MST(i)                                              \
  if (mst) {                                                    \
    unsigned long long _t = __builtin_amdgcn_s_memtime();       \
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");          \
    mst[i] += _t - m_t0;                                        \
    m_t0 = _t;                                                  \
  }
#else
#define SDB_MST(i)
#endif
  if (len != cap) {
    return add_with_limit_lanes(cid, cd, len, cap, idreg, mydist, pd, lane);
  }
  const float tail0 = list_tail(cd, cap);
  const uint64_t cm = __ballot(!(mydist > tail0)) & pd;  // the points the replay would look at first
  SDB_MST(0)
  if (__popcll(cm) < FEW || (__ballot(mydist != mydist) & pd)) {
    add_with_limit_lanes(cid, cd, len, cap, idreg, mydist, pd, lane);
#ifdef SDB_STAMPS
    asm volatile("" ::"v"(cd[0]));
#endif
    SDB_MST(1)
    return;
  }
  const bool inC = (cm >> lane) & 1ull;
  // The pass over the points is the hot part (about a dozen points per hop): per point one readlane, and per
  // array register one compare-and-count each way.  Ties are not looked for here; they show up afterwards
  // as two elements on one position (checked below), which costs nothing per point.
  float cdx[NREG];    // the array's distances, +inf in the lanes past its end
  uint32_t up[NREG];  // per array entry: points strictly below it
#pragma unroll
  for (int r = 0; r < NREG; r++) up[r] = 0, cdx[r] = (r * 64 + lane) < cap ? cd[r] : __int_as_float(0x7f800000);
  uint32_t rl_me = 0, rc_me = 0;  // per point lane: entries below it, points below it
  for (uint64_t t = cm; t; t &= t - 1) {
    const int j = __ffsll((unsigned long long)t) - 1;
    const float dj = rlf(mydist, j);
    uint32_t below = 0;
#pragma unroll
    for (int r = 0; r < NREG; r++) {
      up[r] += dj < cdx[r] ? 1u : 0u;
      below += (uint32_t)__popcll(__ballot(cdx[r] < dj));
    }
    if (lane == j) rl_me = below;
    rc_me += dj < mydist ? 1u : 0u;
  }
#ifdef SDB_STAMPS
  asm volatile("" ::"v"(rc_me), "v"(up[0]));
#endif
  SDB_MST(2)
  // positions; with no two equal distances they are a permutation and exactly `cap` of them lie below `cap`
  const uint32_t np_me = rl_me + rc_me;
  uint32_t kept = (uint32_t)__popcll(__ballot(inC && np_me < (uint32_t)cap));
  uint32_t *s_id = scratch;
  float *s_d = reinterpret_cast<float *>(scratch + NREG * 64);
#pragma unroll
  for (int r = 0; r < NREG; r++) {
    const int e = r * 64 + lane;
    kept += (uint32_t)__popcll(__ballot(e < cap && (uint32_t)e + up[r] < (uint32_t)cap));
    if (e < cap) s_id[e] = kNoSlot;  // a position nobody lands on stays marked
  }
  if (kept != (uint32_t)cap) {
    return add_with_limit_lanes(cid, cd, len, cap, idreg, mydist, pd, lane);
  }
  wave_lds_sync();
#pragma unroll
  for (int r = 0; r < NREG; r++) {
    const int e = r * 64 + lane;
    const uint32_t np = (uint32_t)e + up[r];
    if (e < cap && np < (uint32_t)cap) s_id[np] = cid[r], s_d[np] = cd[r];
  }
  if (inC && np_me < (uint32_t)cap) s_id[np_me] = idreg, s_d[np_me] = mydist;
  wave_lds_sync();
  uint32_t nid[NREG];
  float nd[NREG];
  bool hole = false;
#pragma unroll
  for (int r = 0; r < NREG; r++) {
    const int e = r * 64 + lane;
    nid[r] = e < cap ? s_id[e] : cid[r], nd[r] = e < cap ? s_d[e] : cd[r];
    hole |= e < cap && nid[r] == kNoSlot;
  }
  wave_lds_sync();
  // an unfilled position = two elements shared another one = equal distances: replay one by one
  if (__ballot(hole)) {
    return add_with_limit_lanes(cid, cd, len, cap, idreg, mydist, pd, lane);
  }
#pragma unroll
  for (int r = 0; r < NREG; r++) cid[r] = nid[r], cd[r] = nd[r];
#ifdef SDB_STAMPS
  asm volatile("" ::"v"(cd[0]));
#endif
  SDB_MST(3)
}

// What a merger wave does once a hop's points are in the array: the node the walk goes to -- `named` by the walker, or
// (kNoSlot) the first unvisited entry, search.go:66-71 -- is marked :74 and returned in `next` (kNoSlot: no unvisited
// entry left); f1 / f1d: the first unvisited entry behind it, which the walker names the hop after this one with
// (search_kernel.h name_next), kNoSlot: none.
template <int NREG>
__device__ __forceinline__ void pick_and_mark(uint32_t (&cid)[NREG], const float (&cd)[NREG], int len, uint32_t named, int lane,
                                              uint32_t &next, uint32_t &f1, float &f1d) {
  uint64_t um[NREG];  // the array's unvisited entries, by position
#pragma unroll
  for (int r = 0; r < NREG; r++) um[r] = __ballot((r * 64 + lane) < len && !(cid[r] & kVisBit));
  int sel = -1;
  if (named != kNoSlot) {
#pragma unroll
    for (int r = 0; r < NREG; r++) {
      const uint64_t m = __ballot((r * 64 + lane) < len && cid[r] == named);
      if (m) sel = r * 64 + __ffsll((unsigned long long)m) - 1;
    }
  } else {
#pragma unroll
    for (int r = NREG - 1; r >= 0; r--)
      if (um[r]) sel = r * 64 + __ffsll((unsigned long long)um[r]) - 1;
  }
  next = kNoSlot;
#pragma unroll
  for (int r = 0; r < NREG; r++)
    if (sel >= 0 && (sel >> 6) == r) {
      next = rl(cid[r], sel & 63);
      if (lane == (sel & 63)) cid[r] |= kVisBit;
      um[r] &= ~(1ull << (sel & 63));
    }
  f1 = kNoSlot, f1d = 0.0f;
#pragma unroll
  for (int r = NREG - 1; r >= 0; r--)
    if (um[r]) {
      const int s2 = __ffsll((unsigned long long)um[r]) - 1;
      f1 = rl(cid[r], s2), f1d = rlf(cd[r], s2);
    }
}

// IndexVamana.Search's result copy, vamana.go:293-307: the array without the start node, `limit` entries at most, into
// query q's output row; a row shorter than `limit` ends in zeros, not in whatever was there.  `e` is the caller's view of
// the arguments -- cold_args() or the kernel's own copy: its choice -- and every pointer is loaded through it where it
// is used.  (Handed over as values, loaded ahead of the call, they cost the workgroup-per-query walk 1 % of a small
// call: profiles/walk_steps_ab.json call_sites.)
template <int NREG, class Args>
__device__ __forceinline__ void write_results(const uint32_t (&cid)[NREG], const float (&cd)[NREG], int len, uint32_t start_slot, int lane,
                                              uint32_t q, Args &e) {
  if (!e.out_ids) return;
  int base = 0;
  const int limit = (int)e.limit;
  auto *const o_ids = as_global(e.out_ids) + (size_t)q * limit;
  auto *const o_d = as_global(e.out_dists) + (size_t)q * limit;
  const auto *const ids = as_global(e.ids);
#pragma unroll
  for (int r = 0; r < NREG; r++) {
    const uint32_t s = cid[r] & ~kVisBit;
    const bool ok = (r * 64 + lane) < len && s != start_slot;  // :294-296
    const uint64_t m = __ballot(ok);
    const int rank = base + __popcll(m & ((1ull << lane) - 1));
    if (ok && rank < limit) {  // :297-299
      o_ids[rank] = ids[s];
      o_d[rank] = cd[r];
    }
    base += __popcll(m);
  }
  const int got = base < limit ? base : limit;
  if (lane == 0) as_global(e.out_counts)[q] = (uint32_t)got;
  for (int i = got + lane; i < limit; i += 64) o_ids[i] = 0, o_d[i] = 0.0f;
}

// roaring Contains on this query's ascending slot list: 64-ary search, all lanes probe at once
template <typename T>  // uint32_t slots or uint64_t ids
__device__ __forceinline__ bool filter_contains(const T *__restrict__ arr, uint32_t n, T target, int lane) {
  uint32_t lo = 0, hi = n;
  while (hi - lo > 64) {
    const uint32_t step = (hi - lo + 63) / 64;
    const uint32_t idx = lo + (uint32_t)lane * step;
    const T v = idx < hi ? arr[idx] : ~(T)0;
    const uint64_t m = __ballot(idx < hi && v <= target);
    if (!m) return false;  // target below the first pivot
    const uint32_t k = (uint32_t)__popcll(m);
    lo = lo + (k - 1) * step;
    hi = (lo + step < hi) ? lo + step : hi;
  }
  const T v = (lo + (uint32_t)lane < hi) ? arr[lo + lane] : ~(T)0;
  return __ballot(lo + (uint32_t)lane < hi && v == target) != 0ull;
}

}  // namespace sdb
