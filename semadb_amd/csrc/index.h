// index.h -- host-side state of one HBM-resident Vamana index (internal; the public surface is
// include/semadb_amd.h).
#pragma once
#include <array>
#include <map>
#include <shared_mutex>
#include <thread>
#include <unordered_map>

#include "common.h"
#include "view_mutex.h"

namespace sdb {

constexpr uint32_t kAdjStride = 64;  // adjacency row stride in u32 (DegreeBound <= 64, models/index.go:279)

// A buffer that only grows, kept with its byte count.  ensure() frees, nulls both fields, allocates, then sets the size: a
// failed allocation leaves {nullptr, 0}, never a pointer with a stale size.  pinned: page-locked host memory, which
// grows in steps of a quarter (pinning is the expensive part); otherwise device memory.
struct GrowBuf {
  void *p = nullptr;
  size_t bytes = 0;
  bool pinned = false;
  int ensure(size_t want);
  void free();
  template <class T>
  T *as() const { return static_cast<T *>(p); }
};

// Lays arrays out in one buffer, each at a 256-byte boundary: take<T>(count) while the sizes are being added up (`off`
// is then what the buffer needs), Part::in(base) once the buffer is there.
struct Carve {
  template <class T>
  struct Part {
    size_t at;
    T *in(void *base) const { return reinterpret_cast<T *>(static_cast<char *>(base) + at); }
  };
  size_t off = 0;
  template <class T>
  Part<T> take(size_t count) {
    const Part<T> part{off};
    off += (count * sizeof(T) + 255) & ~(size_t)255;
    return part;
  }
};

// Everything one in-flight batch needs besides the index itself.  One per stream.
struct Workspace {
  int device = 0;
  hipStream_t own_stream = nullptr;  // used by host-memory calls
  GrowBuf bitsets;      // uint32 [nq][words]: the per-search VisitedBitSet (distset.go:89-116)
  GrowBuf scratch;      // staging for host-memory calls
  GrowBuf lut;          // float [nq][M*K] product-quantizer distance tables of the batch
  GrowBuf filter;       // seeds / filter slot lists of a filtered batch
  GrowBuf filter_aux;   // a batch's filter bitmaps and their per-query counts (sdb_index_search_batch_bitmap)
  GrowBuf filter_host{nullptr, 0, true};  // the same lists as the host threads write them: pinned, so that the upload is one DMA
  GrowBuf rerank;       // a re-ranked batch's walk results: [nq][rerank] ids, [nq][rerank] distances, [nq] counts (rerank.hip)
  hipEvent_t launched = nullptr;   // recorded behind the last search kernels that were given a graph version
  bool launched_valid = false;
  // a device-memory search returns right behind its kernels: `launched` then also marks the end of the call's device
  // work, and release_ws lets it stand for `done` instead of recording a second event behind it (one marker packet less
  // per batch on the stream)
  bool launched_is_tail = false, done_is_launched = false;
  bool busy = false;               // held by a call that has not returned yet
  bool pending = false;            // device work of an asynchronous call may still be running
  hipStream_t bound_stream = nullptr;
  hipEvent_t done = nullptr;
  void release();
};

struct PQState;  // pq.hip

// Freshly allocated device buffers, owned until they change hands: released by the destructor (or drop()) unless
// keep() has been called.  Every buffer of a step is taken BEFORE anything of the index is replaced, so that a failed
// allocation returns the ones before it and leaves the index as it was (reserve, sdb_index_compact).
struct FreshBufs {
  std::vector<void *> p;
  FreshBufs() = default;
  FreshBufs(const FreshBufs &) = delete;
  FreshBufs &operator=(const FreshBufs &) = delete;
  ~FreshBufs() { drop(); }
  // (room for the pointer first: nothing here fails between an allocation and its being owned)
  int get_bytes(void **out, size_t bytes) {
    p.reserve(p.size() + 1);
    SDB_HIP(hipMalloc(out, bytes));
    p.push_back(*out);
    return SDB_OK;
  }
  template <class T>
  int get_n(T **out, size_t count) { return get_bytes(reinterpret_cast<void **>(out), count * sizeof(T)); }
  // two buffers of a CACHE: both or neither, and no room for them is no error.  pair_if_room: the same without an
  // owner, for buffers that go straight into the index (alloc_adjcodes); it does not throw.
  static bool pair_if_room(void **a, void **b, size_t bytes) noexcept {
    *a = *b = nullptr;
    if (hipMalloc(a, bytes) == hipSuccess && hipMalloc(b, bytes) == hipSuccess) return true;
    (void)hipGetLastError();
    if (*a) (void)hipFree(*a);
    *a = *b = nullptr;
    return false;
  }
  bool get_pair_if_room(void **a, void **b, size_t bytes) {
    p.reserve(p.size() + 2);
    if (!pair_if_room(a, b, bytes)) return false;
    p.push_back(*a), p.push_back(*b);
    return true;
  }
  void drop() {
    for (void *x : p)
      if (x) (void)hipFree(x);
    p.clear();
  }
  void keep() { p.clear(); }
};

// One of the two copies of everything a walk reads and a write changes in place (sdb_index graph versions).
struct GraphCopy {
  uint32_t *adj = nullptr;        // [cap][kAdjStride] neighbour slots, kNoSlot padded, edge order kept
  uint64_t *ids = nullptr;        // [cap] slot -> node id
  uint32_t *start_ext = nullptr;  // the start node's overflow list, kNoSlot-padded to a multiple of 64 (sdb_index::h_start_ext)
  uint32_t start_ext_cap = 0;
  uint8_t *adjcodes = nullptr;    // [cap][kAdjStride][M] the neighbours' code rows, or NULL (sdb_index::has_adjcodes)
  // room for `need` overflow entries: a buffer too small gives way to one of 2 * need, whose contents are for the
  // caller to write (a failed allocation leaves the copy as it was).  Nothing may still read the old buffer.
  int grow_start_ext(uint32_t need);
};

// One per-row device array of the index: where its pointer is kept, what a row of it takes, what byte a fresh one is
// filled with, and whether the index can do without it (sdb_index::row_tables).
struct RowTable {
  enum Kind { kRequired, kQuantizer /* present with a quantizer only */, kCache /* may be dropped */ };
  enum Id { kSlab, kWrAdj, kCmAdj, kDeg, kClean, kWrIds, kCmIds, kDirty, kAdjDist, kDCount, kCodes, kWrAdjCodes, kCmAdjCodes, kCount };
  static constexpr int kNoFill = -1;
  void **slot;
  size_t row_bytes;  // 0: the index has none
  int fill;          // 0xFF, 0 or kNoFill
  Kind kind;
};

// Re-ranking of a walk's candidates by their stored float32 rows (rerank.hip k_rerank; semadb_amd.h
// sdb_index_search_batch_rerank).  cand_*: what the walk wrote with limit = rerank; out_*: where the call's answer goes.
struct RerankArgs {
  const float *slab = nullptr, *queries = nullptr;
  const uint64_t *cand_ids = nullptr;   // [nq][rerank], walk order
  const uint32_t *cand_cnt = nullptr;   // [nq]
  uint64_t *out_ids = nullptr;          // [nq][limit]
  float *out_dists = nullptr;           // [nq][limit]
  uint32_t *out_counts = nullptr;       // [nq]
  // id -> slot on the committed view: keys == NULL: id - base_id (consecutive ids); else a probe of sdb_index::IdMap
  const uint64_t *keys = nullptr;
  const uint32_t *vals = nullptr;
  uint32_t mask = 0;
  uint64_t base_id = 0;
  uint32_t view_n = 0;
  uint32_t dim = 0, nblk = 0, ng = 0, tail = 0, ld = 0;
  uint32_t rerank = 0, limit = 0;
  int metric = 0;
};
constexpr uint32_t kRerankMax = 512;  // searchSize's ceiling on the device (walk_plan.h plan_walk)
int launch_rerank(const RerankArgs &a, uint32_t nq, hipStream_t stream);

// walk_launch.hip: launches the kernel that plan_walk() (walk_plan.h) chose for the call (search_batch.hip, build.hip)
struct SearchArgs;
struct WalkPlan;
int launch_walk_plan(const WalkPlan &plan, const SearchArgs &a, uint32_t nq, hipStream_t stream);
// index.hip: n original-layout rows (host or device memory, `mem`) into slab rows [first, first + n); slab rows back into
// original layout at dst (device); binaryQuantizer.Set (binary.go:131-139) for slab rows of an index with a binary quantizer
int store_rows(sdb_index *ix, uint32_t first, uint32_t n, const float *vectors, int mem, hipStream_t stream);
int unpermute_rows(const sdb_index *ix, uint32_t first, uint32_t n, float *dst, hipStream_t stream);
int encode_bit_rows(sdb_index *ix, uint32_t first, uint32_t n, hipStream_t stream);
// Are ids[0, n) dense (ids[i] == ids[0] + i, ids[0] != 0; or n == 0)?  `map` is cleared; if they are not, it gets
// id -> slot of every id != 0, and *first_dup the first slot whose id was there already (n: none).
bool index_ids(const uint64_t *ids, size_t n, std::unordered_map<uint64_t, uint32_t> &map, size_t *first_dup = nullptr);
int launch_greedy_search(const SearchArgs &a, uint32_t nq, hipStream_t stream);  // plan, then launch, for a call whose bitsets are zero already: nothing here clears them
// the device's address of page-locked host memory the kernels can read and write in place; false: pageable, or not mapped
bool device_view_of_host(const void *p, size_t bytes, void **dev);

#ifdef __HIPCC__
// the hash of sdb_index::IdMap (index.hip k_idmap_build fills the table; search_batch.hip k_filter_resolve and k_rerank probe it)
__device__ __forceinline__ uint32_t idmap_hash(uint64_t id) { return (uint32_t)((id * 0x9E3779B97F4A7C15ull) >> 32); }
#endif

// (sdb::ViewMutex, the writer-preferring lock around an index's committed view: view_mutex.h -- HIP-free, stress-tested
// under ThreadSanitizer by tests/host/test_concurrency.cpp)
}  // namespace sdb

struct sdb_index {
  sdb_index_params P{};
  sdb::RowLayout lay;
  uint32_t n = 0;    // rows in use (slot ids are 0..n-1)
  uint32_t n_dead = 0;  // of which deleted: tombstones with id 0, empty row, unreachable
  uint32_t cap = 0;  // rows allocated
  int64_t start_slot = -1;
  uint64_t max_node_id = 0;  // vamana.go:47
  float *d_slab = nullptr;   // [cap][lay.ld] float32, permuted rows (common.h RowLayout)
  uint32_t *d_deg = nullptr; // [cap]
  uint32_t *d_clean = nullptr; // [cap] leading edges of a row produced by its last robustPrune (build.hip)
  // write-path cache: d_adjdist[r][e] = distFn(r, adj[r][e]) for e < d_dcount[r] (a prefix of the row).  A full
  // node that gets one more back-edge is re-pruned over neighbours + new point (insert.go:47-58); the
  // distances to its old neighbours are the ones computed when those edges were made -- same vectors, same
  // arithmetic -- so they are read back (256 B) instead of recomputed from 64 rows.  Full-precision store only.
  float *d_adjdist = nullptr;    // [cap][kAdjStride]
  uint32_t *d_dcount = nullptr;  // [cap]
  // The start node's edges beyond the 64 of its adjacency row.  Stragglers of a delete are appended to the start
  // node with no bound (AddNeighbourIfNotExists, node.go:73-80 / prune.go:131-151); the list stays that long until
  // the start node is next pruned (a back-edge from an insert, insert.go:47-58, or a delete among its edges).
  // Host copy in edge order; the device copy is padded with kNoSlot to a multiple of 64 so the search reads it in
  // row-sized chunks.  Every other node is bounded by DegreeBound <= 64.
  std::vector<uint32_t> h_start_ext;
  uint32_t start_ext_need() const { return (uint32_t)((h_start_ext.size() + 63) / 64 * 64); }  // entries of the padded device copy
  std::vector<uint64_t> h_ids;
  bool dense_ids = true;  // ids[i] == ids[0] + i  (then no hash map is needed)
  std::unordered_map<uint64_t, uint32_t> id2slot;
  // product quantizer attachment (product.go): codes per slot + tables
  const sdb_pq *pq = nullptr;
  uint8_t *d_codes = nullptr;
  // binary quantizer attachment (binary.go): d_codes then holds [cap][W] uint64 words, the BinaryVector of every
  // stored point (start node included), and travels wherever product codes do (growth, compaction).  At most one of
  // pq / bq is set.  code_bytes: bytes of one row of d_codes (M, or 8 W; 0 without a quantizer).
  const sdb_bq *bq = nullptr;
  uint32_t code_bytes = 0;
  bool quantized() const { return pq != nullptr || bq != nullptr; }
  // Quantizers of up to kAdjCodesMaxM sub-vectors: every node's neighbours' code rows once more, BEHIND ITS ADJACENCY
  // ROW -- [cap][kAdjStride][M] bytes, entry e = the code row of edge e -- the way the reference keeps a node's
  // neighbours as cached point objects (node.go:37-54 LoadNeighbours: one fetch gives ids and codes).  A hop of the
  // quantized walk then reads 256 B of ids and 64 M contiguous bytes of codes with ONE round trip, where the gather
  // by slot was a second, dependent one and paid a 64-byte sector per 8-byte code (M = 8: 6.1 x the algorithmic
  // bytes).  One block per adjacency copy (graph versions below): searches read the committed one; the writer's is
  // brought up to date from the dirty-row flags when a transaction commits (k_adjcodes_rows) -- no write kernel
  // maintains it, and the build's own searches gather by slot as before.
  // (GraphCopy::adjcodes; index_codes.hip)
  static constexpr uint32_t kAdjCodesMaxM = 32;
  bool has_adjcodes() const { return wr.adjcodes != nullptr; }
  int alloc_adjcodes();                       // after a quantizer has been attached (cap rows)
  int rebuild_adjcodes(hipStream_t stream);   // every row of both copies from (adjacency, codes); maintenance calls
  // rows [0, rows) of g.adjcodes from (g.adj, codes; NULL: d_codes) on `stream`, not waited for; dirty != NULL: only the
  // rows a transaction wrote or appended (`from`: rows at its start).  The one launch of k_adjcodes_rows.
  int fill_adjcodes(const sdb::GraphCopy &g, uint32_t rows, const uint8_t *dirty, uint32_t from, hipStream_t stream,
                    const uint8_t *codes = nullptr);
  int forget_prune_state();  // d_clean / d_dcount start over: the store's distance function has changed (index_codes.hip)
  // ---- graph versions (SURVEY 8b Threading; shard/cache/manager.go:159-181) --------------------------------
  // A search walks the last COMMITTED graph while a write transaction changes the graph: everything a walk reads
  // and a write changes in place exists twice -- adjacency rows, the slot -> id table, the start node's overflow
  // list, and the neighbours' code rows (one GraphCopy each).  `wr` is the writer's copy (all write paths use it);
  // `cm` is the committed one, which `view` hands to searches.  Commit swaps the two and then brings the writer's
  // (now stale) copy up to date from the dirty-row flags the write kernels left, once the searches that were
  // launched on it have drained (stream-side waits on their events).  Outside a transaction both are identical.
  // The slab is append-only (rows past view.n are invisible), so it exists once.  (index_versions.hip)
  sdb::GraphCopy wr, cm;
  uint8_t *d_dirty = nullptr;  // [cap] != 0: the open transaction wrote this row's adjacency or id
  struct View {
    uint32_t n = 0;  // committed rows
    const uint32_t *adj = nullptr;
    const uint64_t *ids = nullptr;
    const uint32_t *start_ext = nullptr;
    uint32_t start_ext_n = 0;
    const uint8_t *adj_codes = nullptr;  // cm.adjcodes, or NULL
  } view;
  // view_mu held exclusively.  publish_pointers: `view` reads the committed copy's buffers as they are now (growth
  // inside an open transaction: view.n and the transaction stay).  publish: that, with the rows and the overflow list
  // of the writer's state, and the open transaction ends.
  void publish_pointers();
  void publish();
  void end_tx();  // the transaction's host-side marks go (tx_dirty included)
  // readers: shared from taking `view` until their kernels are enqueued and their event recorded; writers:
  // exclusive while they change the host-side id tables or publish a view
  mutable sdb::ViewMutex view_mu;
  uint64_t view_gen = 1;  // counts the views published (view_mu held exclusively)
  // The committed view's id -> slot table on the device, for the filters of a table whose ids are no longer
  // consecutive (deletes, arbitrary ids): an open-addressing table over view.ids[0, view.n), tombstones left out,
  // built by the first filtered search of a view and kept until the next view is published.  A search reads it
  // under the shared view lock, so a rebuild (another view) never meets a reader of the old one.
  struct IdMap {
    uint64_t *keys = nullptr;  // 0 = empty cell (0 is no node id)
    uint32_t *vals = nullptr;
    uint32_t cells = 0;        // power of two, >= 2 * view.n
    uint64_t gen = 0;          // the view it was built from; 0 = none
    std::mutex mu;
  };
  mutable IdMap idmap;
  int ensure_idmap(const View &vw, hipStream_t stream) const;  // view_mu held (shared)
  std::atomic<bool> in_tx{false};  // read by searches (under the shared view lock) while the writer opens a transaction
  bool tx_explicit = false;
  bool tx_dirty = false;  // the open transaction has changed the writer's copy or the host tables (sdb_index_abort_write)
  uint32_t tx_n0 = 0;  // rows at the start of the open transaction
  uint32_t tx_dead0 = 0;        // tombstones, largest node id and id-table form at the start of it (rollback)
  uint64_t tx_max_id0 = 0;
  int rollback();               // sdb_index_abort_write: the writer's copy and the host tables back to the committed state
  std::unordered_map<uint64_t, uint32_t> tx_deleted;  // ids the open transaction has removed -> their slots
  int begin_write();
  int commit(hipStream_t stream);   // publish the writer's state; `stream` carries the write
  int publish_full();               // exclusive maintenance calls (load, attach_pq ...): drain, copy everything
  int64_t slot_of_committed(uint64_t id, uint32_t view_n) const;  // what a search may resolve; view_mu held
  // sdb_index_set_tuning
  uint32_t tune_hub_min = 512, tune_hash_limit = 0;
  bool tune_no_hash = false;
  bool tune_wide_hash = false;  // quantized searches with 32-bit visited-set cells (4 walks per CU) instead of 16-bit ones (6)
  uint32_t tune_hash16_probes = 0;  // test knob: probe budget of the 16-bit visited set (0 = 15 buckets)
  bool tune_host_filters = false;  // filter ids are resolved to slots by the host's hash map even when the table's ids are consecutive
  uint32_t tune_wide_walk = 0;  // the workgroup-per-query walk of small calls: 0 = up to 256 queries, 1 = never, 2 = always
  bool tune_no_zero_copy = false;  // A/B and parity tests: host-memory searches stage even page-locked buffers
  // Two-precision hop (SDB_TUNE_SKETCH; walk_args.h SearchArgs::sketch): a float16 copy of the slab's rows, an
  // optional cache like GraphCopy::adjcodes.  It describes the rows of the view published as number `sketch_gen`; a search
  // uses it only while that is the current view.  Every path that publishes rows (load, commit, publish_full,
  // rollback, compact) brings it up to date behind the searches of the old view, and reserve() carries it across
  // table growth.  Pointers, capacity, maxima and generation change under the exclusive view_mu only (searches read
  // them once under the shared lock); the conversion kernel runs outside it, serialised against the knob by sketch_mu.
  // Best-effort: no room for it (build_sketch's headroom rule) or a device error while building it leaves it off and
  // the walk reads float32 rows -- never a failed write.
  bool tune_sketch_filtered = false;  // SDB_TUNE_SKETCH_FILTERED: filtered batch searches take the hop too (opt-in: its speed against the float32 walk is not measured)
  // 3 / 4: as 1 / 2 with an INT8 copy in place of the float16 one where the table has that stage (sketch8_supported():
  // cosine / dot, rows of up to 384 floats) and its rows quantise well enough under one scale (kSketch8MaxRatio);
  // every other table behaves under 3 / 4 exactly as under 1 / 2.  A table never holds both copies.
  uint32_t tune_sketch = 3;  // 0 off (the copy is freed), 1 on, 2 on + audit (every discarded neighbour is evaluated exactly as well and checked), 3 (default) / 4: see above
  bool sketch8 = false;      // the copy in d_sketch is the int8 one: rows of ld BYTES, no per-row floats (d_sketch_norm == NULL)
  bool sketch8_refused = false;  // this table's rows failed kSketch8MaxRatio: it keeps the float16 copy until the knob is set again
  float sk8_scale = 0.0f;    // the int8 copy's scale s (y8 = clamp(rint(y / s), -127, 127)): the largest |element| seen / 127, rounded up
  float sk8_amax = 0.0f;     // that largest |element| (carried across appends, never lowered by deletes)
  float sk8_rel = 0.0f;      // max over the rows with ||y|| > 0 of ||y - s y8|| / ||y||, rounded up: a row far below the table's scale quantises to nothing
  // Largest E8max / Y8max (= max ||y - s y8|| / max ||s y8||), and largest error of a single row relative to its own norm
  // (sk8_rel: dot tables whose row norms differ widely have small rows that all quantise to 0 under one scale while the
  // ratio of the two maxima, both set by the largest rows, stays small), at which a table takes the int8 copy.  The stage pays while
  // its int8 rows (1.23 d bytes per evaluated neighbour, rows of visited edges included) plus the float32 rows of the kept
  // and within-margin neighbours (4 d each) stay below the float16 stage's 2.86 d, i.e. while kept + within-margin stays
  // below 0.41 of the evaluated; DESIGN 4 records the replay that turns that share into this ratio.
  static constexpr float kSketch8MaxRatio = 0.16f;
  bool sketch8_supported() const;  // sketch_supported() and walk_args.h stage_int8(): cosine / dot, rows of up to 384 floats
  bool sketch8_wanted() const { return tune_sketch >= 3 && !tune_sketch_filtered && !sketch8_refused && sketch8_supported(); }  // (SDB_TUNE_SKETCH_FILTERED: the filtered hop reads the float16 copy)
  size_t sketch_row_bytes(bool int8) const { return int8 ? (size_t)lay.ld : (size_t)lay.ld * 2; }
  void *d_sketch = nullptr;  // rows of ld halves, or (sketch8) of ld bytes
  float *d_sketch_norm = nullptr;  // [sketch_cap] ||y16||^2 per row (the euclidean form of the first stage)
  uint32_t sketch_cap = 0;   // rows d_sketch has room for
  std::atomic<uint64_t> sketch_gen{0};  // view_gen the copy was built for (0: none); written under the exclusive view_mu
  float sk_emax = 0.0f, sk_ymax = 0.0f;
  unsigned long long *d_sk_counters = nullptr;  // [0] neighbours discarded on their float16 distance, [1] contradicted (audit)
  std::mutex sketch_mu;  // held by build_sketch on the commit path (view_mu released) and by the knob: lock order sketch_mu, view_mu
  // plain rows of whole 32-float blocks in one of the walk's register layouts (walk_args.h stage_shape()), any metric, no quantizer
  bool sketch_supported() const;
  bool sketch_current() const { return d_sketch && sketch_gen == view_gen; }  // describes the current view's rows
  static bool sketch_room(size_t bytes);  // the device keeps max(4 GB, total / 16) free after `bytes` more (a cache's rule, build.hip pairc)
  // (Re)build for the rows as they are (from > 0: only the rows from there on).  `locked`: the caller holds view_mu
  // exclusively.  Never fails: no room or a device error drops the copy.  Off or unsupported: the copy is freed.
  void build_sketch(hipStream_t stream, uint32_t from, bool locked);
  // one attempt at one kind of copy: 0 = built, 1 = dropped (no room, a device error), 2 = the int8 copy was refused (kSketch8MaxRatio)
  int build_sketch_kind(hipStream_t stream, uint32_t from, bool locked, std::unique_lock<sdb::ViewMutex> &wl, bool int8);
  void drop_sketch();  // view_mu held exclusively (or no search can run); waits for the walks that may read it
  bool tune_no_defer = false;  // A/B and parity tests: every back-edge re-prune runs in k_backedges (BuildArgs::def_*)
  uint32_t tune_pq_narrow = 0;  // 1: quantized searches never take a multi-wave walk (k_greedy_search_pqw, k_greedy_search_pq2): A/B and parity tests
  bool tune_no_mfma = false;  // exact scan of dot/cosine rows on the packed-FMA kernel instead of the matrix cores
  uint32_t tune_no_tile = 0;  // 0: LDS-tiled prune of new nodes, 1: one-wave kernel only, 2: tiled with 4 waves instead of 8, 3: tiled without the separate selection kernel (measurement)
  // a write that failed after it had started to change the graph leaves it unusable: every later call fails
  // until the host rebuilds the index from the bucket -- the reference scraps its cache on any error inside a
  // write transaction the same way (shard/cache/manager.go:231-240)
  bool broken = false;
  // counters of the last insert_batch (sdb_index_build_stats); device-side, added to by the kernels.  kStatCopies
  // copies of kStatStride slots, one 128-byte line each: a wave adds to the copy its block index picks, so tens of
  // millions of waves do not queue up on one address (a single set cost the build 1 s of its 3); summed on read
  static constexpr uint32_t kStatCopies = 64, kStatStride = 16;
  uint64_t *d_bstats = nullptr;
  // measurement hook: events around the last K2 launch
  bool profiling = false;
  static constexpr uint32_t kProfRing = 256;
  std::vector<hipEvent_t> ev0, ev1;  // ring of event pairs
  uint64_t prof_count = 0;           // launches recorded since the last read
  mutable std::mutex mu;
  mutable std::vector<sdb::Workspace *> pool;

  int64_t slot_of(uint64_t id) const;
  // Every per-row device array of the index (the two sketch buffers apart: they have a capacity and rules of their
  // own, sketch_cap / sketch_room).  reserve, sdb_index_compact, sdb_index_destroy and sdb_index_load's undo go by it.
  std::array<sdb::RowTable, sdb::RowTable::kCount> row_tables();
  // A fresh set of row tables for `rows` rows, filled with their fill bytes; t[i] stays NULL where the index has no such
  // table, and a kCache table there was no room for is NULL as well (the neighbour-code pair: both or neither).
  // may_drop_sketch (the caller holds sketch_mu and not view_mu): a required allocation that fails while a sketch exists
  // drops the sketch and is tried once more.
  int alloc_row_tables(uint32_t rows, sdb::FreshBufs &fresh, std::array<void *, sdb::RowTable::kCount> &t, bool may_drop_sketch);
  // view_mu held exclusively, device idle: the old tables are freed and `t` takes their place (fresh.keep()).
  void adopt_row_tables(sdb::FreshBufs &fresh, const std::array<void *, sdb::RowTable::kCount> &t);
  int reserve(uint32_t rows);
  int sync_start_ext();  // h_start_ext -> device
  sdb::Workspace *acquire_ws(hipStream_t stream, bool async) const;
  void release_ws(sdb::Workspace *ws, hipStream_t stream, bool async) const;
};

// id -> slot on the host (inline: a filter's translation asks once per id, search_batch.hip resolve_ids_on_host)
inline int64_t sdb_index::slot_of(uint64_t id) const {
  if (n == 0) return -1;
  if (dense_ids) {
    uint64_t base = h_ids[0];
    if (id < base || id - base >= n) return -1;
    return (int64_t)(id - base);
  }
  auto it = id2slot.find(id);
  // (an insert in progress has entered its ids at the slots they will have: rows past n are not there yet)
  return it == id2slot.end() || it->second >= n ? -1 : (int64_t)it->second;
}

inline int64_t sdb_index::slot_of_committed(uint64_t id, uint32_t view_n) const {
  int64_t s = slot_of(id);
  if ((s < 0 || (uint32_t)s >= view_n) && in_tx) {  // removed or replaced by the open transaction: the committed row is still there for a search on the committed graph
    auto it = tx_deleted.find(id);
    if (it != tx_deleted.end()) s = (int64_t)it->second;
  }
  return (s >= 0 && (uint32_t)s < view_n) ? s : -1;  // rows past the committed count belong to the transaction
}
