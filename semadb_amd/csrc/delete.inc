// delete.inc -- included at the end of build.hip (shares robust_prune_wave / PruneLds).
//
// IndexVamana.InsertUpdateDelete, delete branch (shard/index/vamana/vamana.go:175-233):
//   removeInboundEdges (prune.go:88-154) = EdgeScan (node.go:142-199) + pruneDeleteNeighbour (prune.go:12-84)
//   + stragglers re-attached to the start node (prune.go:131-151), then vecStore.Delete / nodeStore.Delete.
// The reference iterates Go maps in EdgeScan, so the order in which it re-attaches stragglers is
// unspecified; here it is storage order.  pruneDeleteNeighbour only writes its own node and only reads
// deleted nodes, so all nodes to prune run in parallel, one wavefront each.

namespace sdb {

constexpr uint32_t kDelCap = 64 + 64 * 64;  // A's valid edges + all edges of up to 64 deleted neighbours

struct DeleteArgs {
  BuildArgs b;
  const uint64_t *ids;       // [n] slot -> id, 0 = tombstone
  const uint8_t *del;        // [n] 1 = in deleteSet
  uint8_t *has_inbound;      // [n]
  uint8_t *to_prune;         // [n]
  const uint32_t *prune_list;
  uint32_t n;
  uint32_t *bound;  // [n] for a node to prune: upper bound of its candidate count (before Add drops repeats)
  uint32_t cap;     // candidate capacity the prune kernel's LDS is laid out for
  // candidate lists handed to the LDS-tiled prune (k_prune_new_tiled) instead of being pruned by this wave: [launch
  // size][kTileMaxCand] slots and distances in arrival order, [launch size] counts (0: pruned here); or NULL
  uint32_t *t_slots;
  float *t_dists;
  uint32_t *t_count;
};

// EdgeScan (node.go:142-199): one wavefront per valid node
__global__ __launch_bounds__(64) void k_edge_scan(const DeleteArgs a) {
  const uint32_t v = blockIdx.x;
  const int lane = threadIdx.x;
  if (v >= a.n || a.ids[v] == 0 || a.del[v]) return;  // deleted nodes are skipped (:158-160)
  const uint32_t nb = a.b.adj[(size_t)v * kAdjStride + lane];
  const bool valid = nb != kNoSlot;
  if (valid) a.has_inbound[nb] = 1;                       // :168
  const bool hit = valid && a.del[nb];                    // :170-174
  if (__ballot(hit)) {
    // how many candidates pruneDeleteNeighbour will stage for this node at most: its surviving edges plus every
    // edge of its deleted neighbours -- the host sizes the prune kernel's LDS by it
    uint32_t c = hit ? a.b.deg[nb] : (valid ? 1u : 0u);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o, 64);
    if (lane == 0) a.to_prune[v] = 1, a.bound[v] = c;
  }
}

// pruneDeleteNeighbour (prune.go:12-84) for node prune_list[blockIdx.x]
template <int NG, bool L2>
__global__ __launch_bounds__(64) void k_prune_deleted(const DeleteArgs a) {
  extern __shared__ __attribute__((aligned(16))) char lds_raw[];
  PruneLds l(lds_raw, a.cap);
  const int lane = threadIdx.x;
  const uint32_t A = a.prune_list[blockIdx.x];
  const uint32_t row = a.b.adj[(size_t)A * kAdjStride + lane];
  const bool valid = row != kNoSlot;
  const bool isdel = valid && a.del[row];
  // validCandidateIds (:22-34): A's surviving edges in edge order ...
  uint32_t cnt = 0;
  {
    const uint64_t m = __ballot(valid && !isdel);
    if (valid && !isdel) l.s_slot[__popcll(m & ((1ull << lane) - 1))] = row;
    cnt = (uint32_t)__popcll(m);
  }
  // ... then the surviving edges of every deleted neighbour, in A's edge order (:46-55)
  for (uint64_t t = __ballot(isdel); t; t &= t - 1) {
    const int j = __ffsll((unsigned long long)t) - 1;
    const uint32_t b = rl(row, j);
    const uint32_t rb = a.b.adj[(size_t)b * kAdjStride + lane];
    const bool ok = rb != kNoSlot && !a.del[rb];
    const uint64_t m = __ballot(ok);
    if (ok) l.s_slot[cnt + __popcll(m & ((1ull << lane) - 1))] = rb;
    cnt += (uint32_t)__popcll(m);
  }
  __syncthreads();
  // candidateSet.Add (:63) keeps the first occurrence of every id
  uint32_t nc = 0;
  for (uint32_t base = 0; base < cnt; base += 64) {
    const uint32_t i = base + lane;
    bool keep = i < cnt;
    uint32_t s = keep ? l.s_slot[i] : kNoSlot;
    if (keep)
      for (uint32_t j = 0; j < i; j++)
        if (l.s_slot[j] == s) {
          keep = false;
          break;
        }
    const uint64_t m = __ballot(keep);
    if (keep) l.in_slot[nc + __popcll(m & ((1ull << lane) - 1))] = s;
    nc += (uint32_t)__popcll(m);
  }
  __syncthreads();
  // distances from A (DistanceFromPoint(pointA) :58)
  dists_from_point<NG, L2>(a.b, A, nc, l, lane);
  if (a.t_count && lane == 0) a.t_count[blockIdx.x] = 0;
  if (nc > a.b.R) {  // :66-68 keep the degree bound
    // robustPrune over ~64 + 64 candidates walks pick by pick here, each pick's row against everything after it
    // (~4 000 row reads from L2 per node); the tiled kernel stages the rows once and takes all pairs from LDS
    if (a.t_count && nc <= (uint32_t)kTileMaxCand) {
      for (uint32_t i = lane; i < nc; i += 64)
        a.t_slots[(size_t)blockIdx.x * kTileMaxCand + i] = l.in_slot[i], a.t_dists[(size_t)blockIdx.x * kTileMaxCand + i] = l.in_dist[i];
      if (lane == 0) a.t_count[blockIdx.x] = nc;
      return;
    }
    robust_prune_wave<NG, L2>(a.b, A, (int)nc, l.in_slot, l.in_dist, l.s_slot, l.s_dist, l.s_rem, l.qs, lane);
    return;
  }
  // :69-80 enough room: candidateSet.Sort() order, every candidate except A itself
  const bool any_nan = wave_any_nan(l.in_dist, (int)nc, lane);
  for (uint32_t i = lane; i < nc; i += 64) l.s_slot[dist_sort_rank(l.in_dist, (int)nc, (int)i, any_nan)] = l.in_slot[i];
  __syncthreads();
  const uint32_t s = lane < (int)nc ? l.s_slot[lane] : kNoSlot;  // nc <= R <= 64
  const bool keep = s != kNoSlot && s != A;
  const uint64_t m = __ballot(keep);
  const uint32_t pos = (uint32_t)__popcll(m & ((1ull << lane) - 1));
  a.b.adj[(size_t)A * kAdjStride + lane] = kNoSlot;
  __syncthreads();
  if (keep) a.b.adj[(size_t)A * kAdjStride + pos] = s;
  if (lane == 0) {
    if (a.b.dirty) a.b.dirty[A] = 1;
    a.b.deg[A] = (uint32_t)__popcll(m);
    a.b.clean[A] = 0;  // these edges were taken as they came, not through robustPrune
    a.b.dcount[A] = 0;  // and their distances are not kept
  }
}

// insert.go:47-58 for a node and several candidates at once, by one wavefront: candidateSet = neighbours + extra,
// Sort, robustPrune (sdb_index_union_prune; the build applies the same rule to a target with several requests).
template <int NG, bool L2>
__global__ __launch_bounds__(64) void k_union_prune(const BuildArgs a, uint32_t node, const uint32_t *extra, uint32_t m) {
  extern __shared__ __attribute__((aligned(16))) char lds_raw[];
  PruneLds l(lds_raw, kDelCap);
  const int lane = threadIdx.x;
  const uint32_t row = a.adj[(size_t)node * kAdjStride + lane];
  const uint64_t vm = __ballot(row != kNoSlot);
  uint32_t nc = (uint32_t)__popcll(vm);
  if (row != kNoSlot) l.in_slot[__popcll(vm & ((1ull << lane) - 1))] = row;
  for (uint32_t i = lane; i < m && nc + i < kDelCap; i += 64) l.in_slot[nc + i] = extra[i];
  nc = nc + m < kDelCap ? nc + m : kDelCap;
  __syncthreads();
  dists_from_point<NG, L2>(a, node, nc, l, lane);
  robust_prune_wave<NG, L2>(a, node, (int)nc, l.in_slot, l.in_dist, l.s_slot, l.s_dist, l.s_rem, l.qs, lane);
}

template <int NG, bool L2>
static int launch_delete(const DeleteArgs &a0, uint32_t n_prune, hipStream_t stream) {
  if (n_prune == 0) return SDB_OK;
  DeleteArgs a = a0;
  a.t_slots = nullptr, a.t_dists = nullptr, a.t_count = nullptr;
  char *tbuf = nullptr;
  bool tiled = false;
  if constexpr (NG >= 1) {
    // the lists of up to kTileMaxCand candidates (a node with one deleted neighbour: ~64 + 64) go to the LDS-tiled prune
    const uint32_t worst = kTileFixedBytes + 80 * 80 * 4 + 1024;
    tiled = a.b.no_tile != 1 && worst + 24 * a.b.ld * 4 <= kTileLdsBytes;
    if (tiled) {
      const size_t per = (size_t)kTileMaxCand * 8 + 8;
      SDB_HIP(hipMallocAsync(reinterpret_cast<void **>(&tbuf), (size_t)n_prune * per, stream));
      a.t_slots = reinterpret_cast<uint32_t *>(tbuf);
      a.t_dists = reinterpret_cast<float *>(tbuf + (size_t)n_prune * kTileMaxCand * 4);
      a.t_count = reinterpret_cast<uint32_t *>(tbuf + (size_t)n_prune * kTileMaxCand * 8);
    }
  }
  hipLaunchKernelGGL((k_prune_deleted<NG, L2>), dim3(n_prune), dim3(64), prune_lds_bytes(a.cap, NG, a.b.ld), stream, a);
  hipError_t e = hipGetLastError();
  if constexpr (NG >= 1) {
    if (tiled && e == hipSuccess) {
      BuildArgs b = a.b;
      b.self_list = a.prune_list, b.nnew = n_prune, b.first_slot = 0;
      b.vis_slots = a.t_slots, b.vis_dists = a.t_dists, b.vis_count = a.t_count, b.vis_cap = kTileMaxCand;
      b.prune_done = a.t_count + n_prune, b.pair_tab = nullptr, b.keys_in = nullptr, b.stats = nullptr;
      static std::atomic<uint64_t> attr_set{0};  // per instantiation, a bit per device
      if (first_use_on_this_device(attr_set)) {
        e = hipFuncSetAttribute(reinterpret_cast<const void *>(&k_prune_new_tiled<NG, L2, true, 4>),
                                hipFuncAttributeMaxDynamicSharedMemorySize, (int)kTileLdsBytes);
        if (e == hipSuccess)
          e = hipFuncSetAttribute(reinterpret_cast<const void *>(&k_prune_new_tiled<NG, L2, false, 8>),
                                  hipFuncAttributeMaxDynamicSharedMemorySize, (int)kTileLdsBytes);
      }
      if (e == hipSuccess) {
        if (b.tail) hipLaunchKernelGGL((k_prune_new_tiled<NG, L2, true, 4>), dim3(n_prune), dim3(256), kTileLdsBytes, stream, b);
        else hipLaunchKernelGGL((k_prune_new_tiled<NG, L2, false, 8>), dim3(n_prune), dim3(512), kTileLdsBytes, stream, b);
        e = hipGetLastError();
      }
    }
  }
  if (tbuf) (void)hipFreeAsync(tbuf, stream);
  SDB_HIP(e);
  return SDB_OK;
}

template <int NG, bool L2>
static int launch_union(const BuildArgs &a, uint32_t node, const uint32_t *extra, uint32_t m, hipStream_t stream) {
  hipLaunchKernelGGL((k_union_prune<NG, L2>), dim3(1), dim3(64), prune_lds_bytes(kDelCap, NG, a.ld), stream, a, node,
                     extra, m);
  SDB_HIP(hipGetLastError());
  return SDB_OK;
}

#define SDB_NG_DISPATCH(fn, ng, ...)          \
  switch (ng) {                               \
    case 0: return fn<0, L2>(__VA_ARGS__);    \
    case 1: return fn<1, L2>(__VA_ARGS__);    \
    case 2: return fn<2, L2>(__VA_ARGS__);    \
    case 3: return fn<3, L2>(__VA_ARGS__);    \
    case 4: return fn<4, L2>(__VA_ARGS__);    \
    case 6: return fn<6, L2>(__VA_ARGS__);    \
    case 8: return fn<8, L2>(__VA_ARGS__);    \
    case 12: return fn<12, L2>(__VA_ARGS__);  \
    case 16: return fn<16, L2>(__VA_ARGS__);  \
    case 24: return fn<24, L2>(__VA_ARGS__);  \
    default: return fn<-1, L2>(__VA_ARGS__);  \
  }

template <bool L2>
static int launch_delete_ng(const DeleteArgs &a, uint32_t n_prune, hipStream_t s) {
  SDB_NG_DISPATCH(launch_delete, a.b.ng, a, n_prune, s)
}
template <bool L2>
static int launch_union_ng(const BuildArgs &a, uint32_t node, const uint32_t *extra, uint32_t m, hipStream_t s) {
  SDB_NG_DISPATCH(launch_union, a.ng, a, node, extra, m, s)
}

// vecStore.Delete / nodeStore.Delete (vamana.go:228-233): the slot becomes a tombstone -- id 0, empty row
__global__ __launch_bounds__(64) void k_tombstone(uint32_t *adj, uint32_t *deg, uint64_t *ids, uint8_t *dirty,
                                                  const uint32_t *dead) {
  const uint32_t s = dead[blockIdx.x];
  adj[(size_t)s * kAdjStride + threadIdx.x] = kNoSlot;
  if (threadIdx.x == 0) deg[s] = 0, ids[s] = 0, dirty[s] = 1;
}

// big_prune for the index's row layout / metric / store
template <class Fill>
static int big_prune_any(const sdb_index *ix, const BuildArgs &a, uint32_t node, uint32_t nc, BigScratch &sc,
                         hipStream_t stream, Fill fill, bool take_all = false) {
  if (ix->pq) return big_prune<kQuantized, false>(a, node, nc, sc, stream, fill, take_all);
  if (ix->bq)
    return ix->bq->metric == SDB_METRIC_JACCARD ? big_prune<kBitJaccard, false>(a, node, nc, sc, stream, fill, take_all)
                                                : big_prune<kBitHamming, false>(a, node, nc, sc, stream, fill, take_all);
  const bool l2 = ix->P.metric == SDB_METRIC_EUCLIDEAN;
#define SDB_BIG_CASE(NGV) \
  case NGV: return l2 ? big_prune<NGV, true>(a, node, nc, sc, stream, fill, take_all) : big_prune<NGV, false>(a, node, nc, sc, stream, fill, take_all);
  switch (a.ng) {
    SDB_BIG_CASE(0) SDB_BIG_CASE(1) SDB_BIG_CASE(2) SDB_BIG_CASE(3) SDB_BIG_CASE(4) SDB_BIG_CASE(6) SDB_BIG_CASE(8)
    SDB_BIG_CASE(12) SDB_BIG_CASE(16) SDB_BIG_CASE(24)
    default: return l2 ? big_prune<-1, true>(a, node, nc, sc, stream, fill, take_all) : big_prune<-1, false>(a, node, nc, sc, stream, fill, take_all);
  }
#undef SDB_BIG_CASE
}

}  // namespace sdb

static int delete_batch_impl(sdb_index *ix, uint64_t n, const uint64_t *ids, void *stream_, bool *changed);

extern "C" int sdb_index_delete_batch(sdb_index *ix, uint64_t n, const uint64_t *ids, void *stream_) try {
  bool changed = false;  // set once the writer's copy of the graph has been touched
  int rc;
  try {
    rc = delete_batch_impl(ix, n, ids, stream_, &changed);
  } catch (...) {  // no host memory for one of the scan's lists: the same two outcomes as any other failure
    rc = sdb::on_exception("sdb_index_delete_batch");
  }
  // a delete that fails half-way leaves rows pruned against nodes that are still there: unusable (index.h `broken`)
  if (rc != SDB_OK && changed) ix->broken = true;
  // a delete that failed before it wrote anything and opened its own transaction closes it again
  if (rc != SDB_OK && !changed && ix && ix->in_tx && !ix->tx_explicit && !ix->tx_dirty) ix->in_tx = false;
  return rc;
}
SDB_API_CATCH("sdb_index_delete_batch")

static int delete_batch_impl(sdb_index *ix, uint64_t n, const uint64_t *ids, void *stream_, bool *changed) {
  if (!ix) return fail(SDB_ERR_INVALID, "index is NULL");
  if (n == 0) return SDB_OK;
  if (!ids) return fail(SDB_ERR_INVALID, "ids is NULL");
  if (ix->broken) return fail(SDB_ERR_STATE, "index is unusable after a failed write; reload it from the bucket");
  if (ix->start_slot < 0) return fail(SDB_ERR_STATE, "could not get start node for saving");
  std::vector<uint32_t> dslots;
  for (uint64_t i = 0; i < n; i++) {
    if (ids[i] == SDB_STARTID) return fail(SDB_ERR_INVALID, "cannot modify point with start id: %llu", SDB_STARTID);
    if (ids[i] == 0) return fail(SDB_ERR_INVALID, "invalid point id: 0");  // vamana.go:150-157
    const int64_t s = ix->slot_of(ids[i]);
    if (s >= 0) dslots.push_back((uint32_t)s);  // !exists && Vector == nil: skip (vamana.go:161-163)
  }
  std::sort(dslots.begin(), dslots.end());
  dslots.erase(std::unique(dslots.begin(), dslots.end()), dslots.end());
  if (dslots.empty()) return SDB_OK;
  DeviceGuard dg(ix->P.device);
  hipStream_t stream = as_stream(stream_);
  const uint32_t N = ix->n;
  const RowLayout &l = ix->lay;
  SDB_TRY(ix->begin_write());  // the writer's copy of the graph changes; searches stay on the committed one
  const uint8_t one = 1;       // rows written from the host below are flagged by hand (start node)
  std::vector<uint8_t> h_del(N, 0);
  for (uint32_t s : dslots) h_del[s] = 1;
  uint8_t *d_flags = nullptr;  // del | has_inbound | to_prune
  SDB_HIP(hipMalloc(&d_flags, (size_t)N * 3));
  struct Free {
    std::vector<void *> p;
    hipStream_t s;
    ~Free() {
      (void)hipStreamSynchronize(s);
      for (void *x : p)
        if (x) (void)hipFree(x);
    }
  } fr{{d_flags}, stream};
  fr.p.reserve(8);
  SDB_HIP(hipMemcpyAsync(d_flags, h_del.data(), N, hipMemcpyHostToDevice, stream));
  SDB_HIP(hipMemsetAsync(d_flags + N, 0, (size_t)N * 2, stream));
  DeleteArgs a{};
  a.b.slab = ix->d_slab, a.b.adj = ix->wr.adj, a.b.deg = ix->d_deg, a.b.clean = ix->d_clean;
  a.b.adjdist = ix->d_adjdist, a.b.dcount = ix->d_dcount;
  a.b.dim = l.dim, a.b.nblk = l.nblk, a.b.ng = l.ng, a.b.tail = l.tail, a.b.ld = l.ld;
  a.b.metric = (int)ix->P.metric, a.b.alpha = ix->P.alpha, a.b.R = ix->P.degree_bound;
  a.b.dirty = ix->d_dirty, a.b.no_tile = ix->tune_no_tile ? 1u : 0u;  // the test knob of the build's tiled prune switches this one too
  const sdb_pq *pq = ix->pq;  // fitted quantizer: DistanceFromPoint is the centroid-pair sum (product.go:296-304)
  if (pq) a.b.pq_codes = ix->d_codes, a.b.pq_cdists = pq->d_cdists, a.b.pq_M = pq->M, a.b.pq_K = pq->K;
  const sdb_bq *bq = ix->bq;  // binary quantizer: the bit distance of two code rows (binary.go:213-223)
  if (bq) a.b.pq_codes = ix->d_codes, a.b.pq_M = ix->code_bytes;
  a.ids = ix->wr.ids, a.del = d_flags, a.has_inbound = d_flags + N, a.to_prune = d_flags + 2 * (size_t)N, a.n = N;
  uint32_t *d_bound = nullptr;
  SDB_HIP(hipMalloc(&d_bound, (size_t)N * 4));
  fr.p.push_back(d_bound);
  a.bound = d_bound, a.cap = kDelCap;
  hipLaunchKernelGGL(k_edge_scan, dim3(N), dim3(64), 0, stream, a);
  SDB_HIP(hipGetLastError());
  std::vector<uint8_t> h_flags((size_t)N * 2);
  std::vector<uint32_t> h_bound(N);
  SDB_HIP(hipMemcpyAsync(h_flags.data(), d_flags + N, (size_t)N * 2, hipMemcpyDeviceToHost, stream));
  SDB_HIP(hipMemcpyAsync(h_bound.data(), d_bound, (size_t)N * 4, hipMemcpyDeviceToHost, stream));
  SDB_HIP(hipStreamSynchronize(stream));
  uint8_t *has_inbound = h_flags.data(), *to_prune = h_flags.data() + N;
  // the start node's overflow edges are edges like any other for EdgeScan (node.go:163-175)
  const uint32_t st = (uint32_t)ix->start_slot;
  bool start_long = false;  // the start node must be pruned and its edge list is longer than a row
  if (!ix->h_start_ext.empty()) {
    bool hit = to_prune[st] != 0;
    for (uint32_t t : ix->h_start_ext) {
      has_inbound[t] = 1;
      hit |= h_del[t] != 0;
    }
    start_long = hit;
    to_prune[st] = 0;  // not through k_prune_deleted, which reads one row
  }
  // ---- stragglers (prune.go:131-151): valid nodes nobody points at, storage order.  Known from the scan alone.
  std::vector<uint32_t> to_save;
  for (uint32_t v = 0; v < N; v++)
    if (ix->h_ids[v] != 0 && !h_del[v] && !has_inbound[v] && (int64_t)v != ix->start_slot) to_save.push_back(v);
  ix->h_start_ext.reserve(ix->h_start_ext.size() + to_save.size());
  // ---- the host tables' memory before the first row is written: what could fail for want of memory once the graph
  // has changed would leave the index unusable, here it leaves it as it was.  A dense id table gets its hash map now
  // (a dense table ignores the map: filling it changes no answer); the deleted ids are entered into the transaction's
  // record now (a search consults it only for an id that no longer resolves, sdb_index::slot_of_committed).
  struct HostPrep {
    sdb_index *ix;
    const bool *changed;
    bool was_dense = false;
    std::vector<uint64_t> recorded;  // ids this call entered into tx_deleted
    ~HostPrep() {
      if (*changed) return;  // the delete went ahead (or the index is marked unusable)
      std::unique_lock<sdb::ViewMutex> wl(ix->view_mu);
      for (uint64_t id : recorded) ix->tx_deleted.erase(id);
      if (was_dense) ix->id2slot.clear();
    }
  } prep{ix, changed};
  {
    std::unique_lock<sdb::ViewMutex> wl(ix->view_mu);  // searches translate filter ids with these tables
    prep.recorded.reserve(dslots.size());
    if (ix->dense_ids) {
      prep.was_dense = true;
      ix->id2slot.clear();
      ix->id2slot.reserve((size_t)N * 2);
      for (uint32_t s = 0; s < N; s++)
        if (ix->h_ids[s] != 0) ix->id2slot.emplace(ix->h_ids[s], s);
    }
    for (uint32_t s : dslots)  // only rows that were committed; first record wins
      if (s < ix->tx_n0 && ix->tx_deleted.emplace(ix->h_ids[s], s).second) prep.recorded.push_back(ix->h_ids[s]);
  }
  // nodes to prune, in classes by how many candidates they can have: nearly all of them have one or two deleted
  // neighbours (<= 64 + 2 * 64 candidates) and run with a small LDS footprint, many waves per CU; only the rest
  // pay for the worst-case layout (64 + 64 * 64 candidates: one wave per CU)
  constexpr uint32_t kTierCap[3] = {448, 1152, kDelCap};
  std::vector<uint32_t> tier_list[3];
  for (uint32_t v = 0; v < N; v++)
    if (to_prune[v]) tier_list[h_bound[v] <= kTierCap[0] ? 0 : h_bound[v] <= kTierCap[1] ? 1 : 2].push_back(v);
  std::vector<uint32_t> prune_list;
  for (auto &t : tier_list) prune_list.insert(prune_list.end(), t.begin(), t.end());
  uint32_t *d_dead = nullptr;  // the tombstone kernel's list (below)
  SDB_HIP(hipMalloc(&d_dead, dslots.size() * 4));
  fr.p.push_back(d_dead);
  uint32_t *d_list = nullptr;
  if (!prune_list.empty()) {
    SDB_HIP(hipMalloc(&d_list, prune_list.size() * 4));
    fr.p.push_back(d_list);
  }
  *changed = true, ix->tx_dirty = true;  // everything below writes rows
  if (!prune_list.empty()) {
    SDB_HIP(hipMemcpyAsync(d_list, prune_list.data(), prune_list.size() * 4, hipMemcpyHostToDevice, stream));
    size_t first = 0;
    for (int tier = 0; tier < 3; tier++) {
      const size_t cnt = tier_list[tier].size();
      if (cnt == 0) continue;
      a.prune_list = d_list + first;
      a.cap = kTierCap[tier];
      first += cnt;
      int rc = pq ? launch_delete<kQuantized, false>(a, (uint32_t)cnt, stream)
           : bq ? (bq->metric == SDB_METRIC_JACCARD ? launch_delete<kBitJaccard, false>(a, (uint32_t)cnt, stream)
                                                    : launch_delete<kBitHamming, false>(a, (uint32_t)cnt, stream))
           : ix->P.metric == SDB_METRIC_EUCLIDEAN ? launch_delete_ng<true>(a, (uint32_t)cnt, stream)
                                                  : launch_delete_ng<false>(a, (uint32_t)cnt, stream);
      if (rc != SDB_OK) return rc;
    }
  }
  BigScratch big_sc;
  if (start_long) {
    // pruneDeleteNeighbour(start) over row + overflow (prune.go:22-64): surviving edges in edge order, then the
    // surviving edges of every deleted neighbour, first occurrence kept -- ids only, so the list is put together
    // here; distances, Sort and robustPrune (or take-all, :66-81) run chip-wide (bigprune.inc)
    SDB_HIP(hipStreamSynchronize(stream));
    auto fetch_row = [&](uint32_t node, std::vector<uint32_t> &out) -> int {
      uint32_t row[kAdjStride], deg = 0;
      SDB_HIP(hipMemcpy(row, ix->wr.adj + (size_t)node * kAdjStride, sizeof(row), hipMemcpyDeviceToHost));
      SDB_HIP(hipMemcpy(&deg, ix->d_deg + node, 4, hipMemcpyDeviceToHost));
      out.assign(row, row + (deg < kAdjStride ? deg : kAdjStride));
      return SDB_OK;
    };
    std::vector<uint32_t> full, tmp, cand;
    SDB_TRY(fetch_row(st, full));
    full.insert(full.end(), ix->h_start_ext.begin(), ix->h_start_ext.end());
    std::unordered_map<uint32_t, char> seen;
    for (uint32_t e : full)
      if (!h_del[e] && seen.emplace(e, 1).second) cand.push_back(e);
    for (uint32_t b : full) {
      if (!h_del[b]) continue;
      SDB_TRY(fetch_row(b, tmp));
      for (uint32_t c : tmp)
        if (!h_del[c] && seen.emplace(c, 1).second) cand.push_back(c);
    }
    const uint32_t nc = (uint32_t)cand.size();
    if (nc == 0) {
      std::vector<uint32_t> empty_row(kAdjStride, kNoSlot);
      const uint32_t zero = 0;
      SDB_HIP(hipMemcpy(ix->wr.adj + (size_t)st * kAdjStride, empty_row.data(), kAdjStride * 4, hipMemcpyHostToDevice));
      SDB_HIP(hipMemcpy(ix->d_dirty + st, &one, 1, hipMemcpyHostToDevice));
      SDB_HIP(hipMemcpy(ix->d_deg + st, &zero, 4, hipMemcpyHostToDevice));
      SDB_HIP(hipMemcpy(ix->d_clean + st, &zero, 4, hipMemcpyHostToDevice));
      SDB_HIP(hipMemcpy(ix->d_dcount + st, &zero, 4, hipMemcpyHostToDevice));
    } else {
      uint32_t *d_cand = nullptr;
      SDB_HIP(hipMalloc(&d_cand, (size_t)nc * 4));
      fr.p.push_back(d_cand);
      SDB_HIP(hipMemcpy(d_cand, cand.data(), (size_t)nc * 4, hipMemcpyHostToDevice));
      auto fill = [&](const BigArgs &g, unsigned tb) {
        hipLaunchKernelGGL(k_big_fill_list, dim3(tb), dim3(256), 0, stream, g, d_cand);
      };
      SDB_TRY(big_prune_any(ix, a.b, st, nc, big_sc, stream, fill, /*take_all=*/nc <= a.b.R));  // prune.go:66
    }
    ix->h_start_ext.clear();
  }
  // ---- stragglers (prune.go:131-151), listed above
  if (!to_save.empty()) {
    SDB_HIP(hipStreamSynchronize(stream));
    uint32_t row[kAdjStride];
    SDB_HIP(hipMemcpy(row, ix->wr.adj + (size_t)st * kAdjStride, sizeof(row), hipMemcpyDeviceToHost));
    uint32_t deg = 0;
    while (deg < kAdjStride && row[deg] != kNoSlot) deg++;
    // AddNeighbourIfNotExists (node.go:73-80) has no bound: past the 64 entries of the row the edges go on the
    // start node's overflow list (index.h), which searches, inserts and deletes read after the row
    std::vector<uint32_t> &ext = ix->h_start_ext;
    for (uint32_t v : to_save) {
      bool exists = false;
      for (uint32_t e = 0; e < deg; e++) exists |= row[e] == v;
      exists = exists || std::find(ext.begin(), ext.end(), v) != ext.end();
      if (exists) continue;
      if (deg < kAdjStride && ext.empty()) row[deg++] = v;
      else ext.push_back(v);
    }
    SDB_HIP(hipMemcpy(ix->wr.adj + (size_t)st * kAdjStride, row, sizeof(row), hipMemcpyHostToDevice));
    SDB_HIP(hipMemcpy(ix->d_dirty + st, &one, 1, hipMemcpyHostToDevice));
    SDB_HIP(hipMemcpy(ix->d_deg + st, &deg, 4, hipMemcpyHostToDevice));
    SDB_TRY(ix->sync_start_ext());
  }
  // ---- vecStore.Delete / nodeStore.Delete (vamana.go:228-233): tombstones (id 0), empty rows
  SDB_HIP(hipStreamSynchronize(stream));
  {
    std::unique_lock<sdb::ViewMutex> wl(ix->view_mu);  // searches translate filter ids with these tables
    ix->dense_ids = false;  // the dense id -> slot shortcut does not survive holes (the map was filled above)
    for (uint32_t s : dslots) {
      // until commit a search on the committed graph still finds it (recorded in tx_deleted above)
      ix->id2slot.erase(ix->h_ids[s]);
      ix->h_ids[s] = 0;
    }
  }
  {
    SDB_HIP(hipMemcpyAsync(d_dead, dslots.data(), dslots.size() * 4, hipMemcpyHostToDevice, stream));
    hipLaunchKernelGGL(k_tombstone, dim3((unsigned)dslots.size()), dim3(64), 0, stream, ix->wr.adj, ix->d_deg, ix->wr.ids,
                       ix->d_dirty, d_dead);
    SDB_HIP(hipGetLastError());
  }
  SDB_HIP(hipStreamSynchronize(stream));
  ix->n_dead += (uint32_t)dslots.size();
  if (!ix->tx_explicit) {  // the call is its own transaction: publish
    SDB_TRY(ix->commit(stream));
    SDB_HIP(hipStreamSynchronize(stream));
  }
  return SDB_OK;
}

// IndexVamana.EdgeScan (node.go:142-199) on its own, read-only: for a delete set, the nodes with an edge into it
// (toPrune) and the valid nodes nobody points at (toSave, the start node excepted).  The reference returns both in
// Go-map order (unspecified); here in storage order.  The same kernel delete_batch runs first.
extern "C" int sdb_index_edge_scan(const sdb_index *ix, uint64_t n, const uint64_t *delete_ids, uint64_t *to_prune,
                                   uint64_t cap_prune, uint64_t *n_prune, uint64_t *to_save, uint64_t cap_save,
                                   uint64_t *n_save, void *stream_) try {
  if (!ix || !n_prune || !n_save) return fail(SDB_ERR_INVALID, "NULL argument");
  *n_prune = 0, *n_save = 0;
  if (n && !delete_ids) return fail(SDB_ERR_INVALID, "delete_ids is NULL");
  if (ix->broken) return fail(SDB_ERR_STATE, "index is unusable after a failed write; reload it from the bucket");
  const uint32_t N = ix->n;
  if (N == 0) return SDB_OK;
  std::vector<uint8_t> h_del(N, 0);
  for (uint64_t i = 0; i < n; i++) {
    const int64_t s = ix->slot_of(delete_ids[i]);
    if (s >= 0) h_del[s] = 1;  // ids that are not stored cannot be pointed at
  }
  DeviceGuard dg(ix->P.device);
  hipStream_t stream = as_stream(stream_);
  uint8_t *d_flags = nullptr;  // del | has_inbound | to_prune
  uint32_t *d_bound = nullptr;
  SDB_HIP(hipMalloc(&d_flags, (size_t)N * 3));
  struct Free {
    std::vector<void *> p;
    hipStream_t s;
    ~Free() {
      (void)hipStreamSynchronize(s);
      for (void *x : p)
        if (x) (void)hipFree(x);
    }
  } fr{{d_flags}, stream};
  SDB_HIP(hipMalloc(&d_bound, (size_t)N * 4));
  fr.p.push_back(d_bound);
  SDB_HIP(hipMemcpyAsync(d_flags, h_del.data(), N, hipMemcpyHostToDevice, stream));
  SDB_HIP(hipMemsetAsync(d_flags + N, 0, (size_t)N * 2, stream));
  DeleteArgs a{};
  a.b.adj = ix->wr.adj, a.b.deg = ix->d_deg;
  a.ids = ix->wr.ids, a.del = d_flags, a.has_inbound = d_flags + N, a.to_prune = d_flags + 2 * (size_t)N, a.n = N;
  a.bound = d_bound;
  hipLaunchKernelGGL(k_edge_scan, dim3(N), dim3(64), 0, stream, a);
  SDB_HIP(hipGetLastError());
  std::vector<uint8_t> h_flags((size_t)N * 2);
  SDB_HIP(hipMemcpyAsync(h_flags.data(), d_flags + N, (size_t)N * 2, hipMemcpyDeviceToHost, stream));
  SDB_HIP(hipStreamSynchronize(stream));
  uint8_t *has_inbound = h_flags.data(), *prune = h_flags.data() + N;
  const uint32_t st = (uint32_t)ix->start_slot;
  for (uint32_t t : ix->h_start_ext) {  // the start node's overflow edges are edges like any other (node.go:163-175)
    has_inbound[t] = 1;
    if (h_del[t]) prune[st] = 1;
  }
  uint64_t np = 0, ns = 0;
  for (uint32_t v = 0; v < N; v++) {
    if (ix->h_ids[v] == 0 || h_del[v]) continue;  // tombstones and the delete set itself are not valid nodes (:158-160)
    if (prune[v]) {
      if (to_prune && np < cap_prune) to_prune[np] = ix->h_ids[v];
      np++;
    }
    if (!has_inbound[v] && (int64_t)v != ix->start_slot) {  // :191-195
      if (to_save && ns < cap_save) to_save[ns] = ix->h_ids[v];
      ns++;
    }
  }
  *n_prune = np, *n_save = ns;
  if ((to_prune && np > cap_prune) || (to_save && ns > cap_save))
    return fail(SDB_ERR_INVALID, "output arrays too small: %llu to prune, %llu to save", (unsigned long long)np,
                (unsigned long long)ns);
  return SDB_OK;
}
SDB_API_CATCH("sdb_index_edge_scan")

// insert.go:47-58 for a node and several candidates at once: candidateSet.Add(neighbours...), Add(extra...),
// Sort, robustPrune(node).  The build applies exactly this to a target with several requests in one round, and
// the delete path to an overflowing start row; exposed so that both device forms of it -- one wavefront
// (k_union_prune) and the chip-wide sequence of bigprune.inc -- can be held against the oracle.
extern "C" int sdb_index_union_prune(sdb_index *ix, uint64_t id, uint64_t m, const uint64_t *extra_ids, int chip_wide,
                                     void *stream_) try {
  if (!ix) return fail(SDB_ERR_INVALID, "index is NULL");
  if (m && !extra_ids) return fail(SDB_ERR_INVALID, "extra_ids is NULL");
  const int64_t s = ix->slot_of(id);
  if (s < 0) return fail(SDB_ERR_NOT_FOUND, "point %llu not found", (unsigned long long)id);
  std::vector<uint32_t> extra;
  {
    std::unordered_map<uint32_t, char> seen;  // Add keeps the first occurrence (distset.go:203-211)
    for (uint64_t i = 0; i < m; i++) {
      const int64_t e = ix->slot_of(extra_ids[i]);
      if (e < 0 || e == s) continue;
      if (seen.emplace((uint32_t)e, 1).second) extra.push_back((uint32_t)e);
    }
  }
  if ((int64_t)s == ix->start_slot && !ix->h_start_ext.empty())
    return fail(SDB_ERR_STATE, "the start node carries an overflow list; it is pruned by the next insert or delete");
  if (!chip_wide && extra.size() + kAdjStride > kDelCap)
    return fail(SDB_ERR_INVALID, "at most %u candidates on the single-wavefront path", kDelCap - kAdjStride);
  DeviceGuard dg(ix->P.device);
  hipStream_t stream = as_stream(stream_);
  const RowLayout &l = ix->lay;
  BuildArgs a{};
  a.slab = ix->d_slab, a.adj = ix->wr.adj, a.deg = ix->d_deg, a.clean = ix->d_clean;
  a.adjdist = ix->d_adjdist, a.dcount = ix->d_dcount;
  a.dim = l.dim, a.nblk = l.nblk, a.ng = l.ng, a.tail = l.tail, a.ld = l.ld;
  a.metric = (int)ix->P.metric, a.alpha = ix->P.alpha, a.R = ix->P.degree_bound;
  const sdb_pq *pq = ix->pq;
  if (pq) a.pq_codes = ix->d_codes, a.pq_cdists = pq->d_cdists, a.pq_M = pq->M, a.pq_K = pq->K;
  const sdb_bq *bq = ix->bq;
  if (bq) a.pq_codes = ix->d_codes, a.pq_M = ix->code_bytes;
  uint32_t *d_extra = nullptr;
  SDB_HIP(hipMalloc(&d_extra, (extra.size() + 1) * 4));
  struct Free {
    void *p;
    hipStream_t s;
    ~Free() {
      (void)hipStreamSynchronize(s);
      (void)hipFree(p);
    }
  } fr{d_extra, stream};
  if (!extra.empty()) SDB_HIP(hipMemcpyAsync(d_extra, extra.data(), extra.size() * 4, hipMemcpyHostToDevice, stream));
  const uint32_t node = (uint32_t)s, me = (uint32_t)extra.size();
  SDB_TRY(ix->begin_write());
  ix->tx_dirty = true;
  a.dirty = ix->d_dirty;
  int rc;
  try {
  if (!chip_wide) {
    rc = pq ? launch_union<kQuantized, false>(a, node, d_extra, me, stream)
         : bq ? (bq->metric == SDB_METRIC_JACCARD ? launch_union<kBitJaccard, false>(a, node, d_extra, me, stream)
                                                  : launch_union<kBitHamming, false>(a, node, d_extra, me, stream))
         : ix->P.metric == SDB_METRIC_EUCLIDEAN ? launch_union_ng<true>(a, node, d_extra, me, stream)
                                                : launch_union_ng<false>(a, node, d_extra, me, stream);
  } else {
    uint32_t deg = 0;
    SDB_HIP(hipMemcpy(&deg, ix->d_deg + node, 4, hipMemcpyDeviceToHost));
    BigScratch sc;
    auto fill = [&](const BigArgs &g, unsigned tb) {
      hipLaunchKernelGGL(k_big_fill_extra, dim3(tb), dim3(256), 0, stream, g, d_extra, deg);
    };
    rc = big_prune_any(ix, a, node, deg + me, sc, stream, fill);
    (void)hipStreamSynchronize(stream);  // `sc` is freed on return
  }
  } catch (...) {
    rc = sdb::on_exception("sdb_index_union_prune");
    ix->broken = true;  // the row may be half-written
  }
  if (rc == SDB_OK && !ix->tx_explicit) {
    rc = ix->commit(stream);
    (void)hipStreamSynchronize(stream);
  }
  return rc;
}
SDB_API_CATCH("sdb_index_union_prune")
