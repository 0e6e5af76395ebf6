// bigprune.inc -- included by build.hip: robustPrune of ONE node over a very large candidate set, spread over
// the whole chip.
//
// insert.go:47-58 for a node B and the m new points that want a back-edge to it in this round:
// candidateSet = B's neighbours + the m points, Sort, robustPrune(B).  For almost every target m is 1 or 2 and
// one wavefront does it (k_backedges).  But the entry node of the graph is a candidate of EVERY insert (each
// search starts there), it is far from all data, so no selected neighbour ever prunes it (alpha * d(p, start)
// < d(A, start) fails), and with room left in the row it becomes an edge of nearly every new node: in a
// 16 384-point round it receives ~16 000 requests.  One wave walking that list reads ~1M rows by itself
// (27 ms, during which the rest of the chip has nothing to do -- it was 45 % of the whole build).  Here the
// same prune runs as a short sequence of chip-wide kernels:
//   fill     candidates and their distances from B (cached per-edge distances where they exist)
//   dist     the missing distances, a wave per 2*U candidates
//   sort     hipCUB radix sort of (ordered distance bits, arrival index): DistSet.Sort is stable
//   R times  pick  (one block: first candidate still alive -> next edge, search.go:115-121)
//            sweep (all waves: alpha * d(picked, c_j) < c_j.Distance -> removed, :132)
//   write    the new row
// Every step is the reference's arithmetic; the result equals robust_prune_wave on the same candidates
// (tests/test_gpu_build.py::test_union_prune_paths_match_oracle).

namespace sdb {

struct BigArgs {
  BuildArgs b;
  uint32_t node;
  uint32_t nc;           // candidates
  uint32_t *c_slot;      // [nc] arrival order
  float *c_dist;         // [nc]; NaN = not known yet
  uint64_t *keys;        // [nc] (ordered distance bits << 32 | arrival index)
  uint64_t *keys_sorted;
  uint32_t *s_slot;      // [nc] sorted
  float *s_dist;
  uint8_t *removed;      // [nc]
  uint32_t *state;       // [1] cnt: edges picked so far
  uint32_t *next;        // [R + 1] the candidate picked in step i (first live one), written during step i - 1
  uint32_t *out_slot;    // [64]
  float *out_dist;
};

__device__ __forceinline__ uint32_t order_bits(float f) {  // monotone float -> uint (total order, -0 < +0)
  const uint32_t u = __float_as_uint(f);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// candidates of a build round: B's row (for a start node with an overflow list: then those `ext` edges), then
// requests [pos, pos + m) of the sorted key array, in insert order
__global__ void k_big_fill_round(const BigArgs g, size_t pos, uint32_t deg, uint32_t ext) {
  const uint32_t c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= g.nc) return;
  const BuildArgs &a = g.b;
  uint32_t slot;
  float d = __uint_as_float(0x7fc00000u);
  if (c < deg) {
    slot = a.adj[(size_t)g.node * kAdjStride + c];
    if (c < a.dcount[g.node]) d = a.adjdist[(size_t)g.node * kAdjStride + c];
  } else if (c < deg + ext) {
    slot = a.start_ext[c - deg];
  } else {
    const uint64_t key = a.keys_sorted[pos + (c - deg - ext)];
    slot = a.first_slot + (uint32_t)((key & 0xFFFFFFFFull) >> 6);
    const uint32_t epos = (uint32_t)(key & 63ull);
    if (a.dcount[slot] > epos) d = a.adjdist[(size_t)slot * kAdjStride + epos];  // distFn(A, B) = distFn(B, A)
  }
  g.c_slot[c] = slot, g.c_dist[c] = d;
}

// candidates given explicitly (sdb_index_union_prune): B's row, then `extra`; an extra that is already a
// neighbour, or B itself, is dropped the way candidateSet.Add drops it (distset.go:203-211)
__global__ void k_big_fill_extra(const BigArgs g, const uint32_t *__restrict__ extra, uint32_t deg) {
  const uint32_t c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= g.nc) return;
  const BuildArgs &a = g.b;
  uint32_t slot;
  float d = __uint_as_float(0x7fc00000u);
  if (c < deg) {
    slot = a.adj[(size_t)g.node * kAdjStride + c];
    if (c < a.dcount[g.node]) d = a.adjdist[(size_t)g.node * kAdjStride + c];
  } else {
    slot = extra[c - deg];
    bool dup = false;
    for (uint32_t e = 0; e < deg; e++) dup |= a.adj[(size_t)g.node * kAdjStride + e] == slot;
    if (dup) slot = kNoSlot;
  }
  g.c_slot[c] = slot, g.c_dist[c] = d;
}

// candidates given as a complete list (already first-occurrence unique): the start node's delete prune when it
// carries an overflow list (delete.inc)
__global__ void k_big_fill_list(const BigArgs g, const uint32_t *__restrict__ list) {
  const uint32_t c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= g.nc) return;
  g.c_slot[c] = list[c], g.c_dist[c] = __uint_as_float(0x7fc00000u);
}

// distFn(x, c_j) for the candidates of this wave's chunk selected by `want`; results through `emit`
template <int NG, bool L2, class Want, class Emit>
__device__ __forceinline__ void big_chunk(const BuildArgs &a, uint32_t x, const uint32_t *slots, uint32_t n, uint32_t j0,
                                          float *qs, int lane, Want want, Emit emit) {
  constexpr int U = NG >= 0 ? ChunkPairs<NG, false>::value : 4;
  if constexpr (is_quantized(NG)) {  // one candidate per lane, table lookups / population counts
    const uint8_t *cx = a.pq_codes + (size_t)x * a.pq_M;
    const uint32_t j = j0 + lane;
    if (j < n && want(j)) emit(j, code_pair_dist<NG>(a, cx, a.pq_codes + (size_t)slots[j] * a.pq_M));
  } else {
    const int L = lane & 31;
    // any work in this chunk?
    uint32_t jj[2 * U];
    bool need = false;
#pragma unroll
    for (int k = 0; k < 2 * U; k++) {
      jj[k] = j0 + k;
      need |= jj[k] < n && want(jj[k]);
    }
    if (!need) return;
    PointRow<NG> pr;
    const float *xrow = a.slab + (size_t)x * a.ld;
    if constexpr (NG >= 0) {
#pragma unroll
      for (int g = 0; g < NG; g++) pr.xq[g] = reinterpret_cast<const float4 *>(xrow)[g * 32 + L];
      if (NG == 0) pr.xq[0] = make_float4(0.f, 0.f, 0.f, 0.f);
      pr.xt = a.tail ? xrow[NG * 128 + L] : 0.0f;
    } else {
      for (uint32_t t = lane; t < a.ld; t += 64) qs[t] = xrow[t];
      __syncthreads();
    }
    uint32_t slot[U];
    float res[U];
#pragma unroll
    for (int u = 0; u < U; u++) {
      const uint32_t ja = jj[2 * u] < n ? jj[2 * u] : n - 1, jb = jj[2 * u + 1] < n ? jj[2 * u + 1] : n - 1;
      uint32_t sa = slots[ja], sb = slots[jb];
      if (sa == kNoSlot) sa = x;  // dropped candidate: any valid row, the result is not used
      if (sb == kNoSlot) sb = x;
      slot[u] = lane < 32 ? sa : sb;
    }
    if constexpr (NG >= 0) chunk_dist<NG, L2, U>(a.slab, a.ld, a.tail, pr.xq, pr.xt, slot, res, lane);
    else chunk_dist_lds<L2, U>(a.slab, a.ld, a.ng, a.tail, qs, slot, res, lane);
#pragma unroll
    for (int u = 0; u < U; u++) {
      const float d0 = metric_finish(rlf(res[u], 0), a.metric);
      const float d1 = metric_finish(rlf(res[u], 32), a.metric);
      if (lane == 0) {
        if (jj[2 * u] < n && want(jj[2 * u])) emit(jj[2 * u], d0);
        if (jj[2 * u + 1] < n && want(jj[2 * u + 1])) emit(jj[2 * u + 1], d1);
      }
    }
  }
}

template <int NG>
static constexpr uint32_t big_chunk_rows() {
  return is_quantized(NG) ? 64 : 2 * (NG >= 0 ? ChunkPairs<NG, false>::value : 4);
}

// the distances from B that no cache had
template <int NG, bool L2>
__global__ __launch_bounds__(64) void k_big_dist(const BigArgs g) {
  extern __shared__ __attribute__((aligned(16))) float big_qs[];
  const int lane = threadIdx.x;
  const uint32_t j0 = blockIdx.x * big_chunk_rows<NG>();
  big_chunk<NG, L2>(
      g.b, g.node, g.c_slot, g.nc, j0, big_qs, lane,
      [&](uint32_t j) { return g.c_slot[j] != kNoSlot && g.c_dist[j] != g.c_dist[j]; },
      [&](uint32_t j, float d) { g.c_dist[j] = d; });
}

__global__ void k_big_keys(const BigArgs g) {
  const uint32_t c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c <= kAdjStride) g.next[c] = 0xFFFFFFFFu;  // the picks of the steps to come (a launch has at least 256 threads)
  if (c >= g.nc) return;
  // dropped candidates (duplicates of a neighbour, B itself) sort behind everything and are never picked
  const bool dropped = g.c_slot[c] == kNoSlot || g.c_slot[c] == g.node;
  const float d = g.c_dist[c];
  const uint32_t hi = dropped ? 0xFFFFFFFFu : order_bits(d == 0.0f ? 0.0f : d);  // -0 and +0 compare equal
  g.keys[c] = ((uint64_t)hi << 32) | c;
}

__global__ void k_big_unpack(const BigArgs g) {
  const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= g.nc) return;
  const uint32_t c = (uint32_t)(g.keys_sorted[r] & 0xFFFFFFFFull);
  const uint32_t slot = g.c_slot[c];
  g.s_slot[r] = slot, g.s_dist[r] = g.c_dist[c];
  const bool dead = slot == kNoSlot || slot == g.node;  // search.go:115-117 skips the node itself
  g.removed[r] = dead ? 1 : 0;
  if (!dead) atomicMin(&g.next[0], r);  // the first pick (dropped candidates sort behind everything: few threads get here twice)
  if (r == 0) g.state[0] = 0, g.state[1] = 0, g.state[2] = 0, g.state[3] = 0;
}

// One step of the selection loop (search.go:112-135) per launch: the candidate picked for this step -- the first live
// one, found while the previous step swept (k_big_unpack for the first) -- becomes an edge (:118); everything after it
// that it beats is removed (:124-135), and every wave reports the first candidate of its chunk that survived: the
// smallest of those is the next step's pick.  (Round 3 ran a pick kernel and a sweep kernel per step, 2 x 11 904
// launches in a 1M build.)  The walk has ended when a step finds no pick; the host launches degree-bound steps (:119-121).
template <int NG, bool L2>
__global__ __launch_bounds__(64) void k_big_step(const BigArgs g, uint32_t i) {
  extern __shared__ __attribute__((aligned(16))) float big_qs[];
  const uint32_t found = g.next[i];
  if (found == 0xFFFFFFFFu) return;
  const int lane = threadIdx.x;
  if (blockIdx.x == 0 && lane == 0) g.out_slot[i] = g.s_slot[found], g.out_dist[i] = g.s_dist[found], g.state[1] = i + 1;
  if (i + 1 >= g.b.R) return;  // the degree bound: the last edge, nothing left to decide
  const uint32_t j0 = blockIdx.x * big_chunk_rows<NG>();
  if (j0 + big_chunk_rows<NG>() <= found + 1) return;
  const float alpha = g.b.alpha;
  uint32_t first_alive = 0xFFFFFFFFu;
  big_chunk<NG, L2>(
      g.b, g.s_slot[found], g.s_slot, g.nc, j0, big_qs, lane,
      [&](uint32_t j) { return j > found && !g.removed[j]; },
      [&](uint32_t j, float d) {
        if (alpha * d < g.s_dist[j]) g.removed[j] = 1;  // :132
        else if (j < first_alive) first_alive = j;
      });
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) first_alive = min(first_alive, (uint32_t)__shfl_down((int)first_alive, o, 64));
  if (lane == 0 && first_alive != 0xFFFFFFFFu) atomicMin(&g.next[i + 1], first_alive);
}

__global__ __launch_bounds__(64) void k_big_write(const BigArgs g) {
  const int lane = threadIdx.x;
  const uint32_t cnt = g.state[1];
  const BuildArgs &a = g.b;
  a.adj[(size_t)g.node * kAdjStride + lane] = lane < (int)cnt ? g.out_slot[lane] : kNoSlot;
  a.adjdist[(size_t)g.node * kAdjStride + lane] = lane < (int)cnt ? g.out_dist[lane] : 0.0f;
  if (lane == 0) {
    a.deg[g.node] = cnt, a.clean[g.node] = cnt, a.dcount[g.node] = cnt;
    if (a.dirty) a.dirty[g.node] = 1;
  }
}

// pruneDeleteNeighbour's other branch (prune.go:69-80): the candidates fit the degree bound, all of them become
// edges in candidateSet.Sort() order, the node itself left out.  nc <= 64 here.
__global__ __launch_bounds__(64) void k_big_take_all(const BigArgs g) {
  const int lane = threadIdx.x;
  const BuildArgs &a = g.b;
  const bool keep = lane < (int)g.nc && !g.removed[lane];
  const uint64_t m = __ballot(keep);
  const uint32_t pos = (uint32_t)__popcll(m & ((1ull << lane) - 1));
  const uint32_t s = keep ? g.s_slot[lane] : kNoSlot;
  a.adj[(size_t)g.node * kAdjStride + lane] = kNoSlot;
  __syncthreads();
  if (keep) a.adj[(size_t)g.node * kAdjStride + pos] = s;
  if (lane == 0) {
    a.deg[g.node] = (uint32_t)__popcll(m), a.clean[g.node] = 0, a.dcount[g.node] = 0;
    if (a.dirty) a.dirty[g.node] = 1;
  }
}

// scratch of the big path, grown on demand, owned by the caller
struct BigScratch {
  char *buf = nullptr;
  size_t bytes = 0;
  void *sort_tmp = nullptr;
  size_t sort_bytes = 0;
  ~BigScratch() {
    if (buf || sort_tmp) (void)hipDeviceSynchronize();  // error paths return with kernels still queued
    if (buf) (void)hipFree(buf);
    if (sort_tmp) (void)hipFree(sort_tmp);
  }
};

template <int NG, bool L2, class Fill>
static int big_prune(const BuildArgs &ba, uint32_t node, uint32_t nc, BigScratch &sc, hipStream_t stream, Fill fill,
                     bool take_all = false) {
  size_t off = 0;
  auto carve = [&](size_t b) {
    const size_t o = off;
    off += (b + 255) & ~(size_t)255;
    return o;
  };
  const size_t o_cs = carve((size_t)nc * 4), o_cd = carve((size_t)nc * 4), o_k = carve((size_t)nc * 8);
  const size_t o_ks = carve((size_t)nc * 8), o_ss = carve((size_t)nc * 4), o_sd = carve((size_t)nc * 4);
  const size_t o_rm = carve(nc), o_st = carve(16), o_os = carve(64 * 4), o_od = carve(64 * 4), o_nx = carve(66 * 4);
  if (off > sc.bytes) {
    if (sc.buf) (void)hipFree(sc.buf);
    sc.buf = nullptr, sc.bytes = 0;
    SDB_HIP(hipMalloc(&sc.buf, off * 2));
    sc.bytes = off * 2;
  }
  size_t need = 0;
  SDB_HIP(hipcub::DeviceRadixSort::SortKeys(nullptr, need, (uint64_t *)nullptr, (uint64_t *)nullptr, (int)nc, 0, 64, stream));
  if (need > sc.sort_bytes) {
    if (sc.sort_tmp) (void)hipFree(sc.sort_tmp);
    sc.sort_tmp = nullptr, sc.sort_bytes = 0;
    SDB_HIP(hipMalloc(&sc.sort_tmp, need * 2));
    sc.sort_bytes = need * 2;
  }
  BigArgs g{};
  g.b = ba, g.node = node, g.nc = nc;
  g.c_slot = (uint32_t *)(sc.buf + o_cs), g.c_dist = (float *)(sc.buf + o_cd);
  g.keys = (uint64_t *)(sc.buf + o_k), g.keys_sorted = (uint64_t *)(sc.buf + o_ks);
  g.s_slot = (uint32_t *)(sc.buf + o_ss), g.s_dist = (float *)(sc.buf + o_sd);
  g.removed = (uint8_t *)(sc.buf + o_rm), g.state = (uint32_t *)(sc.buf + o_st);
  g.out_slot = (uint32_t *)(sc.buf + o_os), g.out_dist = (float *)(sc.buf + o_od), g.next = (uint32_t *)(sc.buf + o_nx);
  const unsigned tb = (nc + 255) / 256;
  const unsigned wb = (nc + big_chunk_rows<NG>() - 1) / big_chunk_rows<NG>();
  const size_t lds = NG == -1 ? (size_t)ba.ld * 4 + 16 : 0;
  fill(g, tb);
  hipLaunchKernelGGL((k_big_dist<NG, L2>), dim3(wb), dim3(64), lds, stream, g);
  hipLaunchKernelGGL(k_big_keys, dim3(tb), dim3(256), 0, stream, g);
  size_t tmp = sc.sort_bytes;
  SDB_HIP(hipcub::DeviceRadixSort::SortKeys(sc.sort_tmp, tmp, g.keys, g.keys_sorted, (int)nc, 0, 64, stream));
  hipLaunchKernelGGL(k_big_unpack, dim3(tb), dim3(256), 0, stream, g);
  if (take_all) {
    if (nc > kAdjStride) return fail(SDB_ERR_INVALID, "take-all over %u candidates", nc);
    hipLaunchKernelGGL(k_big_take_all, dim3(1), dim3(64), 0, stream, g);
    SDB_HIP(hipGetLastError());
    return SDB_OK;
  }
  for (uint32_t i = 0; i < ba.R; i++)  // unconditional: a step returns at once after the walk has ended
    hipLaunchKernelGGL((k_big_step<NG, L2>), dim3(wb), dim3(64), lds, stream, g, i);
  hipLaunchKernelGGL(k_big_write, dim3(1), dim3(64), 0, stream, g);
  SDB_HIP(hipGetLastError());
  return SDB_OK;
}

}  // namespace sdb
