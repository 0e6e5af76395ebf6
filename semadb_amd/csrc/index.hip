// index.hip -- K3 (HBM slab + adjacency loader) and the index's host-side state: the device tables and their growth,
// lifecycle, load / export / compact.  The two graph copies and their transactions are index_versions.hip, the
// first-stage copy of the rows index_sketch.hip, quantizer code rows index_codes.hip; the search call itself is
// search_batch.hip, the walk's launcher walk_launch.hip.
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <memory>
#include <new>
#include <stdexcept>

#include "bq.h"
#include "pq.h"
#include "walk_args.h"

namespace sdb {

// ------------------------------------------------------------------------------------------
// error plumbing
// ------------------------------------------------------------------------------------------
char *last_error_buf() noexcept {
  static thread_local char e[kErrBytes] = {0};
  return e;
}

int fail(int code, const char *fmt, ...) noexcept {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(last_error_buf(), kErrBytes, fmt, ap);
  va_end(ap);
  return code;
}

// the one place where exceptions end (common.h SDB_API_CATCH)
int on_exception(const char *fn) noexcept {
  try {
    throw;
  } catch (const std::bad_alloc &) {
    return fail(SDB_ERR_DEVICE, "%s: out of host memory", fn);
  } catch (const std::exception &e) {
    return fail(SDB_ERR_STATE, "%s: %s", fn, e.what());
  } catch (...) {
    return fail(SDB_ERR_STATE, "%s: unknown C++ exception", fn);
  }
}

// ------------------------------------------------------------------------------------------
// workspaces
// ------------------------------------------------------------------------------------------
int GrowBuf::ensure(size_t want) {
  if (want <= bytes) return SDB_OK;
  if (p) SDB_HIP(pinned ? hipHostFree(p) : hipFree(p));
  p = nullptr, bytes = 0;
  if (pinned) {
    want += want / 4;
    SDB_HIP(hipHostMalloc(&p, want, hipHostMallocDefault));
  } else {
    SDB_HIP(hipMalloc(&p, want));
  }
  bytes = want;
  return SDB_OK;
}

void GrowBuf::free() {
  if (p) (void)(pinned ? hipHostFree(p) : hipFree(p));
  p = nullptr, bytes = 0;
}

void Workspace::release() {
  for (GrowBuf *b : {&filter, &filter_host, &filter_aux, &lut, &rerank, &bitsets, &scratch}) b->free();
  if (own_stream) (void)hipStreamDestroy(own_stream);
  own_stream = nullptr;
  if (done) (void)hipEventDestroy(done);
  done = nullptr;
  if (launched) (void)hipEventDestroy(launched);
  launched = nullptr, launched_valid = false;
}

// ------------------------------------------------------------------------------------------
// layout kernels
// ------------------------------------------------------------------------------------------
// original row-major [n][dim]  ->  slab rows [n][ld] (RowLayout in common.h)
__global__ void k_permute_rows(const float *__restrict__ src, float *__restrict__ dst, uint32_t n,
                               uint32_t dim, uint32_t nblk, uint32_t ng, uint32_t tail, uint32_t ld) {
  const uint32_t row = blockIdx.x;
  if (row >= n) return;
  const float *s = src + (size_t)row * dim;
  float *d = dst + (size_t)row * ld;
  for (uint32_t t = threadIdx.x; t < ld; t += blockDim.x) {
    float v = 0.0f;
    if (t < ng * 128) {
      uint32_t g = t / 128, r = t % 128, Lx = r / 4, k = r % 4, b = 4 * g + k;
      if (b < nblk) v = s[32 * b + Lx];
    } else {
      uint32_t i = t - ng * 128;
      if (i < tail) v = s[nblk * 32 + i];
    }
    d[t] = v;
  }
}

__global__ void k_unpermute_rows(const float *__restrict__ src, float *__restrict__ dst, uint32_t n,
                                 uint32_t dim, uint32_t nblk, uint32_t ng, uint32_t ld) {
  const uint32_t row = blockIdx.x;
  if (row >= n) return;
  const float *s = src + (size_t)row * ld;
  float *d = dst + (size_t)row * dim;
  for (uint32_t e = threadIdx.x; e < dim; e += blockDim.x) {
    uint32_t b = e / 32, Lx = e % 32;
    d[e] = b < nblk ? s[(b / 4) * 128 + Lx * 4 + (b % 4)] : s[ng * 128 + Lx];
  }
}

// slab rows by slot list -> original-layout rows (kNoSlot: a zero row)
__global__ void k_gather_rows(const float *__restrict__ slab, const uint32_t *__restrict__ slots, float *__restrict__ dst,
                              uint32_t n, uint32_t dim, uint32_t nblk, uint32_t ng, uint32_t ld) {
  const uint32_t i = blockIdx.x;
  if (i >= n) return;
  const uint32_t slot = slots[i];
  const float *s = slab + (size_t)slot * ld;
  float *d = dst + (size_t)i * dim;
  for (uint32_t e = threadIdx.x; e < dim; e += blockDim.x) {
    const uint32_t b = e / 32, Lx = e % 32;
    d[e] = slot == kNoSlot ? 0.0f : (b < nblk ? s[(b / 4) * 128 + Lx * 4 + (b % 4)] : s[ng * 128 + Lx]);
  }
}

// sdb_index_compact: new row j <- old row live[j], adjacency renumbered through map[]
__global__ __launch_bounds__(64) void k_compact_rows(const uint32_t *__restrict__ live, const uint32_t *__restrict__ map,
                                                     uint32_t ld, const float *__restrict__ slab, float *__restrict__ nslab,
                                                     const uint32_t *__restrict__ adj, uint32_t *__restrict__ nadj,
                                                     const float *__restrict__ adjdist, float *__restrict__ nadjdist,
                                                     const uint32_t *__restrict__ deg, uint32_t *__restrict__ ndeg,
                                                     const uint32_t *__restrict__ clean, uint32_t *__restrict__ nclean,
                                                     const uint32_t *__restrict__ dcount, uint32_t *__restrict__ ndcount,
                                                     const uint64_t *__restrict__ ids, uint64_t *__restrict__ nids,
                                                     const uint8_t *__restrict__ codes, uint8_t *__restrict__ ncodes,
                                                     uint32_t M, uint32_t *__restrict__ lost) {
  const uint32_t j = blockIdx.x, s = live[j];
  const int lane = threadIdx.x;
  const float4 *src = reinterpret_cast<const float4 *>(slab + (size_t)s * ld);
  float4 *dst = reinterpret_cast<float4 *>(nslab + (size_t)j * ld);
  for (uint32_t i = lane; i < ld / 4; i += 64) dst[i] = src[i];
  const uint32_t e = adj[(size_t)s * kAdjStride + lane];
  const uint32_t ne = e == kNoSlot ? kNoSlot : map[e];
  if (e != kNoSlot && ne == kNoSlot) atomicAdd(lost, 1u);  // an edge into a tombstone: delete_batch never leaves one
  nadj[(size_t)j * kAdjStride + lane] = ne;
  nadjdist[(size_t)j * kAdjStride + lane] = adjdist[(size_t)s * kAdjStride + lane];
  if (lane == 0) ndeg[j] = deg[s], nclean[j] = clean[s], ndcount[j] = dcount[s], nids[j] = ids[s];
  if (codes)
    for (uint32_t i = lane; i < M; i += 64) ncodes[(size_t)j * M + i] = codes[(size_t)s * M + i];
}

// fills the committed view's id -> slot table (sdb_index::IdMap; ensure_idmap), which search_batch.hip k_filter_resolve and
// rerank.hip k_rerank probe
__global__ void k_idmap_build(const uint64_t *__restrict__ ids, uint32_t n, uint64_t *__restrict__ keys,
                              uint32_t *__restrict__ vals, uint32_t mask) {
  const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= n) return;
  const uint64_t id = ids[s];
  if (id == 0) return;  // tombstone
  uint32_t h = idmap_hash(id) & mask;
  while (true) {
    const unsigned long long old = atomicCAS(reinterpret_cast<unsigned long long *>(keys + h), 0ull, (unsigned long long)id);
    if (old == 0ull || old == id) {
      vals[h] = s;
      return;
    }
    h = (h + 1) & mask;
  }
}

__global__ void k_fill_u32(uint32_t *p, uint32_t v, size_t n) {
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) p[i] = v;
}

// copies n original-layout rows (host or device) into slab rows [first, first+n)
int store_rows(sdb_index *ix, uint32_t first, uint32_t n, const float *vectors, int mem, hipStream_t stream) {
  if (n == 0) return SDB_OK;
  const RowLayout &l = ix->lay;
  const float *src = vectors;
  float *staging = nullptr;
  if (mem == SDB_MEM_HOST) {
    SDB_HIP(hipMalloc(&staging, (size_t)n * l.dim * sizeof(float)));
    hipError_t e = hipMemcpyAsync(staging, vectors, (size_t)n * l.dim * sizeof(float), hipMemcpyHostToDevice, stream);
    if (e != hipSuccess) {
      (void)hipFree(staging);
      return fail(SDB_ERR_DEVICE, "H2D copy failed: %s", hipGetErrorString(e));
    }
    src = staging;
  }
  hipLaunchKernelGGL(k_permute_rows, dim3(n), dim3(128), 0, stream, src, ix->d_slab + (size_t)first * l.ld, n,
                     l.dim, l.nblk, l.ng, l.tail, l.ld);
  hipError_t e = hipGetLastError();
  if (staging) {
    (void)hipStreamSynchronize(stream);
    (void)hipFree(staging);
  }
  if (e != hipSuccess) return fail(SDB_ERR_DEVICE, "permute launch failed: %s", hipGetErrorString(e));
  return SDB_OK;
}

// binaryQuantizer.Set (binary.go:131-139) for slab rows [first, first + n) of an index with a binary quantizer attached
int encode_bit_rows(sdb_index *ix, uint32_t first, uint32_t n, hipStream_t stream) {
  return bq_encode_slab(ix->bq->d_thr, ix->lay, ix->d_slab, first, n, reinterpret_cast<uint64_t *>(ix->d_codes), stream);
}

// original-layout copy of slab rows [first, first+n) into dst (device)
int unpermute_rows(const sdb_index *ix, uint32_t first, uint32_t n, float *dst, hipStream_t stream) {
  if (n == 0) return SDB_OK;
  const RowLayout &l = ix->lay;
  hipLaunchKernelGGL(k_unpermute_rows, dim3(n), dim3(128), 0, stream, ix->d_slab + (size_t)first * l.ld, dst, n, l.dim,
                     l.nblk, l.ng, l.ld);
  SDB_HIP(hipGetLastError());
  return SDB_OK;
}

bool index_ids(const uint64_t *ids, size_t n, std::unordered_map<uint64_t, uint32_t> &map, size_t *first_dup) {
  map.clear();
  if (first_dup) *first_dup = n;
  bool dense = n == 0 || ids[0] != 0;  // (a tombstoned first row: id - ids[0] names no row)
  for (size_t i = 1; i < n && dense; i++) dense = ids[i] == ids[0] + i;
  if (dense) return true;
  map.reserve(n * 2);
  for (size_t i = 0; i < n; i++)
    if (ids[i] != 0 && !map.emplace(ids[i], (uint32_t)i).second && first_dup && i < *first_dup) *first_dup = i;
  return false;
}

}  // namespace sdb

using namespace sdb;

// ------------------------------------------------------------------------------------------
// sdb_index methods
// ------------------------------------------------------------------------------------------
std::array<RowTable, RowTable::kCount> sdb_index::row_tables() {
  using T = RowTable;
  const size_t adj_row = (size_t)kAdjStride * 4, ac_row = has_adjcodes() ? (size_t)kAdjStride * code_bytes : 0;  // (code_bytes = M; the quantizer itself is borrowed and may be gone when the index is destroyed)
  return {{
      // (in the order of RowTable::Id)
      {(void **)&d_slab, (size_t)lay.ld * sizeof(float), T::kNoFill, T::kRequired},
      {(void **)&wr.adj, adj_row, 0xFF, T::kRequired},
      {(void **)&cm.adj, adj_row, 0xFF, T::kRequired},
      {(void **)&d_deg, sizeof(uint32_t), 0, T::kRequired},
      {(void **)&d_clean, sizeof(uint32_t), 0, T::kRequired},  // loaded / appended edges are not "clean"
      {(void **)&wr.ids, sizeof(uint64_t), T::kNoFill, T::kRequired},
      {(void **)&cm.ids, sizeof(uint64_t), T::kNoFill, T::kRequired},
      {(void **)&d_dirty, 1, 0, T::kRequired},
      {(void **)&d_adjdist, adj_row, T::kNoFill, T::kRequired},  // edge-distance cache of the write path (index.h)
      {(void **)&d_dcount, sizeof(uint32_t), 0, T::kRequired},   // a row without cached distances has d_dcount 0
      {(void **)&d_codes, code_bytes, T::kNoFill, T::kQuantizer},  // the code rows of a quantized store grow with it
      // ... and the neighbours' code rows behind both adjacency copies.  2 x 64 M bytes per row: 41 GB at 10M rows and
      // M = 32, more than the vectors of d = 768.  A table that grows past the room for them drops them instead of
      // failing the insert -- the index works without (searches gather code rows by slot)
      {(void **)&wr.adjcodes, ac_row, T::kNoFill, T::kCache},
      {(void **)&cm.adjcodes, ac_row, T::kNoFill, T::kCache},
  }};
}

int sdb_index::alloc_row_tables(uint32_t rows, FreshBufs &fresh, std::array<void *, RowTable::kCount> &t, bool may_drop_sketch) {
  const auto tabs = row_tables();
  // every new buffer first; if one allocation fails the ones before it are returned and the index is as it was
  auto get_required = [&]() -> int {
    t.fill(nullptr);
    for (int i = 0; i < RowTable::kCount; i++)
      if (tabs[i].kind != RowTable::kCache && tabs[i].row_bytes) SDB_TRY(fresh.get_bytes(&t[i], (size_t)rows * tabs[i].row_bytes));
    return SDB_OK;
  };
  if (int rc = get_required()) {
    if (!may_drop_sketch || !d_sketch) return rc;
    // a required buffer never goes without for the float16 copy's sake (a cache): drop it and try once more
    (void)hipGetLastError();
    fresh.drop();
    {
      std::unique_lock<sdb::ViewMutex> wl(view_mu);
      drop_sketch();
    }
    SDB_TRY(get_required());
  }
  if (const size_t ac_row = tabs[RowTable::kWrAdjCodes].row_bytes)
    (void)fresh.get_pair_if_room(&t[RowTable::kWrAdjCodes], &t[RowTable::kCmAdjCodes], (size_t)rows * ac_row);
  for (int i = 0; i < RowTable::kCount; i++)
    if (t[i] && tabs[i].fill != RowTable::kNoFill) SDB_HIP(hipMemset(t[i], tabs[i].fill, (size_t)rows * tabs[i].row_bytes));
  return SDB_OK;
}

void sdb_index::adopt_row_tables(FreshBufs &fresh, const std::array<void *, RowTable::kCount> &t) {
  const auto tabs = row_tables();
  for (int i = 0; i < RowTable::kCount; i++) {
    if (!tabs[i].row_bytes) continue;
    if (*tabs[i].slot) (void)hipFree(*tabs[i].slot);
    *tabs[i].slot = t[i];  // (NULL: a cache there was no room for is dropped)
  }
  fresh.keep();
}

int sdb_index::reserve(uint32_t rows) {
  if (rows <= cap) return SDB_OK;
  uint32_t ncap = cap ? cap : std::min<uint32_t>(rows, 1024);  // (a first capacity below 1024 is honoured; above, doubled up from 1024)
  while (ncap < rows) ncap = ncap < (1u << 30) ? ncap * 2 : rows;
  FreshBufs fresh;
  std::array<void *, RowTable::kCount> t;
  std::unique_lock<std::mutex> sg(sketch_mu);  // the knob waits until the float16 copy has followed the growth
  SDB_TRY(alloc_row_tables(ncap, fresh, t, true));
  // the float16 copy grows with the slab, best-effort under the headroom rule: rows do not move, so it stays current and
  // the next commit converts only the rows it appends (without room the copy keeps covering the rows it has).  Chosen
  // order: a table that already serves from the copy keeps it through growth, so on a device near capacity a bulk
  // insert_batch into a grown table may find no headroom left for its pair cache (build.hip pairc) and build without
  // it -- slower, same graph -- rather than have every search fall back to float32 rows.
  const bool sk_keep = sketch_current();
  void *nsk = nullptr;
  float *nskn = nullptr;
  if (sk_keep && sketch_cap < ncap) {
    fresh.p.reserve(fresh.p.size() + 2);
    // (the int8 copy: rows of ld bytes and no per-row floats)
    const size_t rows_b = (size_t)ncap * sketch_row_bytes(sketch8), norm_b = sketch8 ? 0 : (size_t)ncap * sizeof(float);
    const uint32_t have = std::min(n, sketch_cap);
    if (!sketch_room(rows_b + norm_b) || hipMalloc(&nsk, rows_b) != hipSuccess || (norm_b && hipMalloc(&nskn, norm_b) != hipSuccess) ||
        (have && (hipMemcpy(nsk, d_sketch, (size_t)have * sketch_row_bytes(sketch8), hipMemcpyDeviceToDevice) != hipSuccess ||
                  (norm_b && hipMemcpy(nskn, d_sketch_norm, (size_t)have * sizeof(float), hipMemcpyDeviceToDevice) != hipSuccess)))) {
      (void)hipGetLastError();
      if (nsk) (void)hipFree(nsk);
      if (nskn) (void)hipFree(nskn);
      nsk = nullptr, nskn = nullptr;
    } else {
      fresh.p.push_back(nsk);  // returned with the rest if a step below fails
      if (nskn) fresh.p.push_back(nskn);
    }
  }
  // the old buffers are freed below: nothing may still be walking them (searches run on streams of their own)
  if (cap) SDB_HIP(hipDeviceSynchronize());
  if (n) {
    const auto tabs = row_tables();
    for (int i = 0; i < RowTable::kCount; i++)
      if (t[i]) SDB_HIP(hipMemcpy(t[i], *tabs[i].slot, (size_t)n * tabs[i].row_bytes, hipMemcpyDeviceToDevice));
  }
  SDB_HIP(hipDeviceSynchronize());
  {
    std::unique_lock<sdb::ViewMutex> wl(view_mu);  // searches pick their pointers up under this lock
    adopt_row_tables(fresh, t);
    cap = ncap;
    publish_pointers();  // (growth happens inside open transactions: view.n and the transaction stay)
    if (nsk) {
      (void)hipFree(d_sketch);
      if (d_sketch_norm) (void)hipFree(d_sketch_norm);
      d_sketch = nsk, d_sketch_norm = nskn, sketch_cap = ncap;
    }
    if (sk_keep) sketch_gen = view_gen;
  }
  return SDB_OK;
}

int sdb_index::ensure_idmap(const View &vw, hipStream_t stream) const {
  std::lock_guard<std::mutex> g(idmap.mu);
  if (idmap.gen == view_gen) return SDB_OK;
  // every reader of the previous table held the shared view lock over its probe kernel and the wait behind it, and
  // the view has been published (exclusively) since: nothing reads the old cells any more
  uint32_t cells = 1024;
  while (cells < 2ull * vw.n && cells < (1u << 31)) cells <<= 1;
  if (cells < 2ull * vw.n) return fail(SDB_ERR_INVALID, "too many rows for the id table");
  idmap.gen = 0;
  if (cells > idmap.cells) {
    if (idmap.keys) (void)hipFree(idmap.keys);
    if (idmap.vals) (void)hipFree(idmap.vals);
    idmap.keys = nullptr, idmap.vals = nullptr, idmap.cells = 0;
    if (hipMalloc(&idmap.keys, (size_t)cells * 8) != hipSuccess || hipMalloc(&idmap.vals, (size_t)cells * 4) != hipSuccess) {
      (void)hipGetLastError();
      if (idmap.keys) (void)hipFree(idmap.keys);
      idmap.keys = nullptr;
      return fail(SDB_ERR_DEVICE, "out of device memory for the id table (%u cells)", cells);
    }
    idmap.cells = cells;
  }
  SDB_HIP(hipMemsetAsync(idmap.keys, 0, (size_t)idmap.cells * 8, stream));
  hipLaunchKernelGGL(sdb::k_idmap_build, dim3((vw.n + 255) / 256), dim3(256), 0, stream, vw.ids, vw.n, idmap.keys, idmap.vals,
                     idmap.cells - 1);
  SDB_HIP(hipGetLastError());
  SDB_HIP(hipStreamSynchronize(stream));  // other searches probe it from their own streams
  idmap.gen = view_gen;
  return SDB_OK;
}

// A workspace (visited bitsets, staging, LUTs) belongs to one in-flight batch.  Host-memory calls hold it
// until they have synchronised.  Device-memory calls return before the kernel runs, so the workspace
// stays bound to the caller's stream: it is handed out again only to a call on the same stream (stream
// order then serialises the reuse) or once its completion event has fired.
Workspace *sdb_index::acquire_ws(hipStream_t stream, bool async) const {
  std::lock_guard<std::mutex> g(mu);
  for (auto *w : pool) {
    if (w->busy) continue;
    if (w->pending) {
      if (async && w->bound_stream == stream) {
        w->busy = true;
        w->launched_is_tail = false;
        return w;
      }
      if (hipEventQuery(w->done_is_launched ? w->launched : w->done) != hipSuccess) continue;
      w->pending = false;
    }
    w->busy = true;
    w->launched_is_tail = false;
    return w;
  }
  std::unique_ptr<Workspace> w(new Workspace());
  w->device = P.device;
  w->busy = true;
  pool.push_back(w.get());
  return w.release();
}

void sdb_index::release_ws(Workspace *ws, hipStream_t stream, bool async) const {
  std::lock_guard<std::mutex> g(mu);
  if (async) {
    if (ws->launched_is_tail && ws->launched_valid) {  // recorded on `stream` behind everything this call enqueued
      ws->pending = true, ws->bound_stream = stream, ws->done_is_launched = true;
    } else {
      ws->done_is_launched = false;
      if (!ws->done) (void)hipEventCreateWithFlags(&ws->done, hipEventDisableTiming);
      if (ws->done && hipEventRecord(ws->done, stream) == hipSuccess) {
        ws->pending = true;
        ws->bound_stream = stream;
      }
    }
  }
  ws->busy = false;
}

// ------------------------------------------------------------------------------------------
// C ABI
// ------------------------------------------------------------------------------------------
// Page-locked host memory the kernels can address in place.  Blocks from sdb_host_alloc are kept in a table (exact,
// and dropped by sdb_host_free before the memory goes back); any other pointer is asked of the runtime -- memory the
// caller page-locked itself (hipHostMalloc, hipHostRegister; torch's pin_memory) says so, a pageable pointer does not.
struct PinnedRange {
  size_t bytes;
  char *dev;  // the device's address of the block's first byte (NULL: not mapped)
};
static std::shared_mutex g_pinned_mu;
static std::map<uintptr_t, PinnedRange> g_pinned;

bool sdb::device_view_of_host(const void *p, size_t bytes, void **dev) {
  const uintptr_t a = reinterpret_cast<uintptr_t>(p);
  {
    std::shared_lock<std::shared_mutex> g(g_pinned_mu);
    auto it = g_pinned.upper_bound(a);
    if (it != g_pinned.begin()) {
      --it;
      if (a >= it->first && a + bytes <= it->first + it->second.bytes) {
        if (!it->second.dev) return false;
        *dev = it->second.dev + (a - it->first);
        return true;
      }
    }
  }
  hipPointerAttribute_t attr{};
  if (hipPointerGetAttributes(&attr, p) != hipSuccess) {
    (void)hipGetLastError();  // a pageable pointer is not an error of this call
    return false;
  }
  if (attr.type != hipMemoryTypeHost || !attr.devicePointer) return false;
  *dev = attr.devicePointer;
  return true;
}

extern "C" {

const char *sdb_last_error(void) { return last_error_buf(); }

int sdb_abi_version(void) { return SDB_ABI_VERSION; }

int sdb_device_count(int *count) try {
  if (!count) return fail(SDB_ERR_INVALID, "count is NULL");
  int n = 0;
  hipError_t e = hipGetDeviceCount(&n);
  if (e != hipSuccess || n <= 0) {
    *count = 0;
    return fail(SDB_ERR_DEVICE, "no HIP device visible: %s", hipGetErrorString(e));
  }
  *count = n;
  return SDB_OK;
}
SDB_API_CATCH("sdb_device_count")

int sdb_host_alloc(size_t bytes, void **out) try {
  if (!out) return fail(SDB_ERR_INVALID, "out is NULL");
  *out = nullptr;
  if (bytes == 0) return SDB_OK;
  void *p = nullptr;
  SDB_HIP(hipHostMalloc(&p, bytes, hipHostMallocDefault));
  void *dev = nullptr;
  if (hipHostGetDevicePointer(&dev, p, 0) != hipSuccess) dev = nullptr, (void)hipGetLastError();
  try {
    std::unique_lock<std::shared_mutex> g(g_pinned_mu);
    g_pinned[reinterpret_cast<uintptr_t>(p)] = PinnedRange{bytes, static_cast<char *>(dev)};
  } catch (...) {  // no room for the note: the block is still good memory, searches just stage through it
  }
  *out = p;
  return SDB_OK;
}
SDB_API_CATCH("sdb_host_alloc")

int sdb_host_free(void *p) try {
  if (!p) return SDB_OK;
  {
    std::unique_lock<std::shared_mutex> g(g_pinned_mu);
    g_pinned.erase(reinterpret_cast<uintptr_t>(p));
  }
  SDB_HIP(hipHostFree(p));
  return SDB_OK;
}
SDB_API_CATCH("sdb_host_free")

int sdb_index_create(const sdb_index_params *p, sdb_index **out) try {
  if (!p || !out) return fail(SDB_ERR_INVALID, "NULL argument");
  *out = nullptr;
  if (p->dim < 1 || p->dim > 4096)  // models/index.go:285-287
    return fail(SDB_ERR_INVALID, "vector size must be between 1 and 4096, got %u", p->dim);
  if (p->metric > SDB_METRIC_DOT) return fail(SDB_ERR_INVALID, "unknown distance metric %u", p->metric);
  if (p->degree_bound < 1 || p->degree_bound > kAdjStride)
    return fail(SDB_ERR_INVALID, "degree bound must be between 1 and %u, got %u", kAdjStride, p->degree_bound);
  if (p->search_size < 1 || p->search_size > 512)
    return fail(SDB_ERR_INVALID, "search size must be between 1 and 512, got %u", p->search_size);
  if (p->strict) {  // models/index.go:299-307
    if (p->search_size < 25 || p->search_size > 75)
      return fail(SDB_ERR_INVALID, "search size must be between 25 and 75, got %u", p->search_size);
    if (p->degree_bound < 32 || p->degree_bound > 64)
      return fail(SDB_ERR_INVALID, "degree bound must be between 32 and 64, got %u", p->degree_bound);
    if (p->alpha < 1.1f || p->alpha > 1.5f)
      return fail(SDB_ERR_INVALID, "alpha must be between 1.1 and 1.5, got %f", (double)p->alpha);
  }
  int ndev = 0;
  SDB_TRY(sdb_device_count(&ndev));
  if (p->device < 0 || p->device >= ndev) return fail(SDB_ERR_INVALID, "device %d out of range", p->device);
  DeviceGuard dg(p->device);
  if (!dg.ok) return fail(SDB_ERR_DEVICE, "hipSetDevice(%d) failed", p->device);
  std::unique_ptr<sdb_index> ix(new sdb_index());
  ix->P = *p;
  ix->lay = RowLayout(p->dim);
  SDB_TRY(ix->reserve((uint32_t)std::max<uint64_t>(p->capacity ? p->capacity : 1024, 16)));
  *out = ix.release();
  return SDB_OK;
}
SDB_API_CATCH("sdb_index_create")

int sdb_index_destroy(sdb_index *ix) try {
  if (!ix) return SDB_OK;
  DeviceGuard dg(ix->P.device);
  (void)hipDeviceSynchronize();
  for (const RowTable &t : ix->row_tables())
    if (*t.slot) (void)hipFree(*t.slot);
  ix->drop_sketch();
  if (ix->d_sk_counters) (void)hipFree(ix->d_sk_counters);
  if (ix->idmap.keys) (void)hipFree(ix->idmap.keys);
  if (ix->idmap.vals) (void)hipFree(ix->idmap.vals);
  if (ix->wr.start_ext) (void)hipFree(ix->wr.start_ext);
  if (ix->cm.start_ext) (void)hipFree(ix->cm.start_ext);
  if (ix->d_bstats) (void)hipFree(ix->d_bstats);
  for (auto e : ix->ev0)
    if (e) (void)hipEventDestroy(e);
  for (auto e : ix->ev1)
    if (e) (void)hipEventDestroy(e);
  for (auto *w : ix->pool) {
    w->release();
    delete w;
  }
  delete ix;
  return SDB_OK;
}
SDB_API_CATCH("sdb_index_destroy")

int sdb_index_set_start(sdb_index *ix, const float *vec, int mem) try {
  if (!ix || !vec) return fail(SDB_ERR_INVALID, "NULL argument");
  if (ix->start_slot >= 0) return SDB_OK;  // vamana.go:95-97: already there
  if (ix->n != 0) return fail(SDB_ERR_STATE, "start node must be the first node of an empty index");
  DeviceGuard dg(ix->P.device);
  SDB_TRY(ix->reserve(1));
  SDB_TRY(store_rows(ix, 0, 1, vec, mem, nullptr));
  if (ix->bq) SDB_TRY(encode_bit_rows(ix, 0, 1, nullptr));  // vecStore.Set encodes (binary.go:131-139)
  uint64_t id = SDB_STARTID;
  SDB_HIP(hipMemcpy(ix->wr.ids, &id, sizeof(id), hipMemcpyHostToDevice));
  SDB_HIP(hipDeviceSynchronize());
  ix->h_ids.assign(1, id);
  ix->dense_ids = true;
  ix->n = 1;
  ix->start_slot = 0;
  return ix->publish_full();
}
SDB_API_CATCH("sdb_index_set_start")

int sdb_index_load(sdb_index *ix, uint64_t n, const uint64_t *ids, const float *vectors,
                   const uint64_t *offsets, const uint64_t *edges, int mem) try {
  if (!ix || !vectors || !offsets) return fail(SDB_ERR_INVALID, "NULL argument");
  if (ix->n != 0) return fail(SDB_ERR_STATE, "index is not empty");
  if (n == 0 || n >= 0x7FFFFFFFull) return fail(SDB_ERR_INVALID, "node count %llu out of range", (unsigned long long)n);
  if (offsets[n] && !edges) return fail(SDB_ERR_INVALID, "edges is NULL");
  DeviceGuard dg(ix->P.device);
  SDB_TRY(ix->reserve((uint32_t)n));
  // whatever ends this call early -- an error return, a host allocation that fails (the adjacency staging is 3.2 GB at
  // 12.5 M rows) -- leaves the index empty, as it was
  struct Undo {
    sdb_index *ix;
    bool keep = false;
    uint32_t wrote = 0;  // device rows that may hold part of the graph: empty again (rows past n are assumed empty)
    ~Undo() {
      if (keep) return;
      ix->n = 0, ix->start_slot = -1, ix->max_node_id = 0, ix->dense_ids = true;
      ix->h_ids.clear(), ix->id2slot.clear(), ix->h_start_ext.clear();
      if (wrote) {
        for (const RowTable &t : ix->row_tables())
          if (*t.slot && t.fill != RowTable::kNoFill) (void)hipMemset(*t.slot, t.fill, (size_t)wrote * t.row_bytes);
        (void)hipDeviceSynchronize();
      }
    }
  } undo{ix};
  // id table
  ix->h_ids.resize(n);
  for (uint64_t i = 0; i < n; i++) ix->h_ids[i] = ids ? ids[i] : i + 1;
  size_t dup = n;
  ix->dense_ids = index_ids(ix->h_ids.data(), n, ix->id2slot, &dup);
  ix->start_slot = -1;
  ix->max_node_id = 0;
  for (uint64_t i = 0; i < n; i++) {
    uint64_t id = ix->h_ids[i];
    if (id == 0) {
      ix->h_ids.clear();
      return fail(SDB_ERR_INVALID, "invalid point id: 0");
    }
    if (i == dup) {
      ix->h_ids.clear();
      return fail(SDB_ERR_INVALID, "duplicate node id %llu", (unsigned long long)id);
    }
    if (id == SDB_STARTID) ix->start_slot = (int64_t)i;
    else if (id > ix->max_node_id) ix->max_node_id = id;
  }
  if (ix->start_slot < 0) {
    ix->h_ids.clear();
    ix->id2slot.clear();
    return fail(SDB_ERR_INVALID, "start node (id %llu) is not among the loaded ids", SDB_STARTID);
  }
  ix->n = (uint32_t)n;  // slot_of works from here on
  ix->h_start_ext.clear();
  // adjacency rows: ids -> slots, unknown ids dropped, first occurrence kept, edge order kept
  std::vector<uint32_t> adj((size_t)n * kAdjStride, kNoSlot), deg(n, 0);
  for (uint64_t i = 0; i < n; i++) {
    uint32_t *row = adj.data() + (size_t)i * kAdjStride;
    uint32_t dcnt = 0;
    for (uint64_t e = offsets[i]; e < offsets[i + 1]; e++) {
      int64_t s = ix->slot_of(edges[e]);
      if (s < 0) continue;  // itemcache.go:109-128
      bool dup = false;
      for (uint32_t k = 0; k < dcnt; k++) dup |= (row[k] == (uint32_t)s);
      if (dup) continue;
      if (dcnt == kAdjStride) {
        if ((int64_t)i == ix->start_slot) {  // the start node has no bound (node.go:73-80): the rest is its overflow list
          if (std::find(ix->h_start_ext.begin(), ix->h_start_ext.end(), (uint32_t)s) == ix->h_start_ext.end())
            ix->h_start_ext.push_back((uint32_t)s);
          continue;
        }
        ix->n = 0;
        ix->h_start_ext.clear();
        return fail(SDB_ERR_INVALID, "node %llu has more than %u edges", (unsigned long long)ix->h_ids[i], kAdjStride);
      }
      row[dcnt++] = (uint32_t)s;
    }
    deg[i] = dcnt;
  }
  SDB_TRY(ix->sync_start_ext());
  undo.wrote = (uint32_t)n;
  SDB_HIP(hipMemcpy(ix->wr.adj, adj.data(), adj.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
  SDB_HIP(hipMemcpy(ix->d_deg, deg.data(), deg.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
  SDB_HIP(hipMemcpy(ix->wr.ids, ix->h_ids.data(), n * sizeof(uint64_t), hipMemcpyHostToDevice));
  SDB_TRY(store_rows(ix, 0, (uint32_t)n, vectors, mem, nullptr));
  if (ix->bq) SDB_TRY(encode_bit_rows(ix, 0, (uint32_t)n, nullptr));
  SDB_TRY(ix->publish_full());
  undo.keep = true;
  return SDB_OK;
}
SDB_API_CATCH("sdb_index_load")

int sdb_index_set_tuning(sdb_index *ix, int key, uint64_t value) try {
  if (!ix) return fail(SDB_ERR_INVALID, "index is NULL");
  switch (key) {
    case SDB_TUNE_HUB_MIN:
      if (value < 2 || value > 0xFFFFFFFFull) return fail(SDB_ERR_INVALID, "hub threshold must be at least 2");
      ix->tune_hub_min = (uint32_t)value;
      return SDB_OK;
    case SDB_TUNE_HASH_LIMIT:
      if (value > kHashLimit) return fail(SDB_ERR_INVALID, "hash limit is at most %u", kHashLimit);
      ix->tune_hash_limit = (uint32_t)value;  // 0 = default
      return SDB_OK;
    case SDB_TUNE_NO_HASH:
      ix->tune_no_hash = value != 0;
      return SDB_OK;
    case SDB_TUNE_NO_TILE:
      ix->tune_no_tile = (uint32_t)(value > 3 ? 1 : value);  // 3: tiled, selection loop inside the tiled kernel (no k_prune_select)
      return SDB_OK;
    case SDB_TUNE_NO_MFMA:
      ix->tune_no_mfma = value != 0;
      return SDB_OK;
    case SDB_TUNE_WIDE_HASH:
      ix->tune_wide_hash = value != 0;
      return SDB_OK;
    case SDB_TUNE_PQ_NARROW:
      ix->tune_pq_narrow = (uint32_t)value;
      return SDB_OK;
    case SDB_TUNE_WIDE_WALK:
      if (value > 2) return fail(SDB_ERR_INVALID, "wide walk: 0 = few queries, 1 = never, 2 = always");
      ix->tune_wide_walk = (uint32_t)value;
      return SDB_OK;
    case SDB_TUNE_HOST_FILTERS:
      ix->tune_host_filters = value != 0;
      return SDB_OK;
    case SDB_TUNE_NO_ZERO_COPY:
      ix->tune_no_zero_copy = value != 0;
      return SDB_OK;
    case SDB_TUNE_SKETCH: {
      if (value > 4) return fail(SDB_ERR_INVALID, "sketch: 0 = off, 1 = float16 copy, 2 = 1 with audit, 3 = int8 copy where the table has one, 4 = 3 with audit");
      DeviceGuard dg(ix->P.device);
      std::lock_guard<std::mutex> sg(ix->sketch_mu);  // a commit converting rows on another thread finishes first
      std::unique_lock<sdb::ViewMutex> wl(ix->view_mu);
      SDB_HIP(hipDeviceSynchronize());  // walks that read the copy
      ix->tune_sketch = (uint32_t)value;
      if (ix->d_sk_counters) SDB_HIP(hipMemset(ix->d_sk_counters, 0, 2 * sizeof(unsigned long long)));  // (every set clears the counters)
      if (!value) {
        ix->drop_sketch();
        return SDB_OK;
      }
      ix->sketch8_refused = false;  // (a set knob asks again)
      // inside a transaction: its commit builds it; the other kind of copy than the one held: that one is freed first
      if (!ix->in_tx && (!ix->sketch_current() || ix->sketch8 != ix->sketch8_wanted())) ix->build_sketch(nullptr, 0, true);
      return SDB_OK;
    }
    case SDB_TUNE_SKETCH_FILTERED: {
      // the filtered hop is the float16 stage's: a table with the opt-in keeps the float16 copy under 3 / 4 too, for
      // both its walks (sketch8_wanted()); the copy of the other kind is freed and this one built under the knob's locks
      DeviceGuard dg(ix->P.device);
      std::lock_guard<std::mutex> sg(ix->sketch_mu);
      std::unique_lock<sdb::ViewMutex> wl(ix->view_mu);
      ix->tune_sketch_filtered = value != 0;
      if (ix->tune_sketch && !ix->in_tx && ix->d_sketch && ix->sketch8 != ix->sketch8_wanted()) {
        SDB_HIP(hipDeviceSynchronize());  // walks that read the copy
        ix->build_sketch(nullptr, 0, true);
      }
      return SDB_OK;
    }
    case SDB_TUNE_NO_DEFER:
      ix->tune_no_defer = value != 0;
      return SDB_OK;
    case SDB_TUNE_HASH16_PROBES:
      if (value > 15) return fail(SDB_ERR_INVALID, "at most 15 probes");
      ix->tune_hash16_probes = (uint32_t)value;
      return SDB_OK;
    default:
      return fail(SDB_ERR_INVALID, "unknown tuning key %d", key);
  }
}
SDB_API_CATCH("sdb_index_set_tuning")

int sdb_index_build_stats(const sdb_index *ix, uint64_t *out, uint32_t cap) try {
  if (!ix || !out) return fail(SDB_ERR_INVALID, "NULL argument");
#ifdef SDB_BACK_PROFILE  // measurement builds: the five spare slots carry k_backedges' cycle counters (tools/backprof.py)
  const uint32_t n = cap < sdb_index::kStatStride ? cap : sdb_index::kStatStride;
#else
  const uint32_t n = cap < SDB_BUILD_STATS ? cap : SDB_BUILD_STATS;
#endif
  for (uint32_t i = 0; i < n; i++) out[i] = 0;
  if (!ix->d_bstats || n == 0) return SDB_OK;
  DeviceGuard dg(ix->P.device);
  SDB_HIP(hipDeviceSynchronize());
  std::vector<uint64_t> all((size_t)sdb_index::kStatCopies * sdb_index::kStatStride);
  SDB_HIP(hipMemcpy(all.data(), ix->d_bstats, all.size() * 8, hipMemcpyDeviceToHost));
  for (uint32_t c = 0; c < sdb_index::kStatCopies; c++)
    for (uint32_t i = 0; i < n; i++) out[i] += all[(size_t)c * sdb_index::kStatStride + i];
  return SDB_OK;
}
SDB_API_CATCH("sdb_index_build_stats")

int sdb_index_get_vectors(const sdb_index *ix, uint64_t n, const uint64_t *ids, float *out, uint8_t *found) try {
  if (!ix) return fail(SDB_ERR_INVALID, "index is NULL");
  if (n == 0) return SDB_OK;
  if (!ids || !out) return fail(SDB_ERR_INVALID, "NULL argument");
  if (n > 0x7FFFFFFFull) return fail(SDB_ERR_INVALID, "too many ids");
  if (ix->broken) return fail(SDB_ERR_STATE, "index is unusable after a failed write; reload it from the bucket");
  DeviceGuard dg(ix->P.device);
  const RowLayout &l = ix->lay;
  std::vector<uint32_t> slots(n);
  struct Bufs {
    uint32_t *slots = nullptr;
    float *out = nullptr;
    ~Bufs() {
      if (slots) (void)hipFree(slots);
      if (out) (void)hipFree(out);
    }
  } b;
  SDB_HIP(hipMalloc(&b.slots, n * 4));
  SDB_HIP(hipMalloc(&b.out, n * l.dim * 4));
  // the shared lock is held until the rows are on the host: compact and reserve replace the slab (and renumber the
  // rows) under the exclusive lock, and a slot resolved before that must not be read after it
  std::shared_lock<sdb::ViewMutex> rl(ix->view_mu);
  for (uint64_t i = 0; i < n; i++) {
    const int64_t s = ix->slot_of_committed(ids[i], ix->view.n);
    slots[i] = s < 0 ? kNoSlot : (uint32_t)s;
    if (found) found[i] = s < 0 ? 0 : 1;
  }
  SDB_HIP(hipMemcpy(b.slots, slots.data(), n * 4, hipMemcpyHostToDevice));
  hipLaunchKernelGGL(k_gather_rows, dim3((unsigned)n), dim3(128), 0, nullptr, ix->d_slab, b.slots, b.out, (uint32_t)n, l.dim,
                     l.nblk, l.ng, l.ld);
  SDB_HIP(hipGetLastError());
  SDB_HIP(hipMemcpy(out, b.out, n * l.dim * 4, hipMemcpyDeviceToHost));
  return SDB_OK;
}
SDB_API_CATCH("sdb_index_get_vectors")

int sdb_index_exists_batch(const sdb_index *ix, uint64_t n, const uint64_t *ids, uint8_t *out) try {
  if (!ix) return fail(SDB_ERR_INVALID, "index is NULL");
  if (n == 0) return SDB_OK;
  if (!ids || !out) return fail(SDB_ERR_INVALID, "NULL argument");
  std::shared_lock<sdb::ViewMutex> rl(ix->view_mu);  // a writer rehashes the id tables under the exclusive lock
  for (uint64_t i = 0; i < n; i++) out[i] = ix->slot_of(ids[i]) >= 0 ? 1 : 0;
  return SDB_OK;
}
SDB_API_CATCH("sdb_index_exists_batch")

int sdb_index_set_profiling(sdb_index *ix, int enabled) try {
  if (!ix) return fail(SDB_ERR_INVALID, "index is NULL");
  DeviceGuard dg(ix->P.device);
  if (enabled && ix->ev0.empty()) {
    ix->ev0.resize(sdb_index::kProfRing, nullptr);
    ix->ev1.resize(sdb_index::kProfRing, nullptr);
    for (uint32_t i = 0; i < sdb_index::kProfRing; i++) {
      SDB_HIP(hipEventCreate(&ix->ev0[i]));
      SDB_HIP(hipEventCreate(&ix->ev1[i]));
    }
  }
  ix->profiling = enabled != 0;
  ix->prof_count = 0;
  return SDB_OK;
}
SDB_API_CATCH("sdb_index_set_profiling")

int sdb_index_profile_read(sdb_index *ix, float *ms, uint32_t cap, uint32_t *n) try {
  if (!ix || !ms || !n) return fail(SDB_ERR_INVALID, "NULL argument");
  *n = 0;
  if (ix->ev0.empty()) return fail(SDB_ERR_STATE, "profiling was never enabled");
  DeviceGuard dg(ix->P.device);
  uint64_t have = std::min<uint64_t>(ix->prof_count, sdb_index::kProfRing);
  if (have > cap) have = cap;
  for (uint64_t k = 0; k < have; k++) {
    const uint32_t slot = (uint32_t)((ix->prof_count - have + k) % sdb_index::kProfRing);
    SDB_HIP(hipEventSynchronize(ix->ev1[slot]));
    SDB_HIP(hipEventElapsedTime(&ms[k], ix->ev0[slot], ix->ev1[slot]));
  }
  *n = (uint32_t)have;
  ix->prof_count = 0;
  return SDB_OK;
}
SDB_API_CATCH("sdb_index_profile_read")

int sdb_index_last_search_ms(sdb_index *ix, float *ms) try {
  if (!ix || !ms) return fail(SDB_ERR_INVALID, "NULL argument");
  if (!ix->profiling || ix->prof_count == 0) return fail(SDB_ERR_STATE, "no profiled search_batch yet");
  DeviceGuard dg(ix->P.device);
  const uint32_t slot = (uint32_t)((ix->prof_count - 1) % sdb_index::kProfRing);
  SDB_HIP(hipEventSynchronize(ix->ev1[slot]));
  SDB_HIP(hipEventElapsedTime(ms, ix->ev0[slot], ix->ev1[slot]));
  return SDB_OK;
}
SDB_API_CATCH("sdb_index_last_search_ms")

int sdb_index_size_in_memory(const sdb_index *ix, int64_t *bytes) try {
  if (!ix || !bytes) return fail(SDB_ERR_INVALID, "NULL argument");
  // vecStore.SizeInMemory + nodeStore.SizeInMemory (vamana.go:83-85), as held in HBM
  // slab row + adjacency row + its distance cache + degree / clean / cached counters + id (+ code row)
  // (+ the second adjacency / id copy of the graph versions, + the neighbours' code rows behind both adjacency copies)
  *bytes = (int64_t)ix->cap * (ix->lay.ld * 4 + 3 * kAdjStride * 4 + 3 * 4 + 2 * 8 + ix->code_bytes +
                               (ix->has_adjcodes() ? 2 * kAdjStride * ix->pq->M : 0)) +
           (int64_t)ix->sketch_cap * (ix->sketch8 ? ix->lay.ld : ix->lay.ld * 2 + 4);  // (+ the float16 copy of the rows and their norms, or the int8 copy, SDB_TUNE_SKETCH)
  return SDB_OK;
}
SDB_API_CATCH("sdb_index_size_in_memory")

int sdb_index_stats(const sdb_index *ix, uint64_t *n_nodes, uint64_t *n_edges, uint64_t *max_node_id) try {
  if (!ix) return fail(SDB_ERR_INVALID, "index is NULL");
  if (n_nodes) *n_nodes = ix->n - ix->n_dead;  // live nodes (start node included)
  if (max_node_id) *max_node_id = ix->max_node_id;
  if (n_edges) {
    DeviceGuard dg(ix->P.device);
    std::vector<uint32_t> deg(ix->n);
    if (ix->n) SDB_HIP(hipMemcpy(deg.data(), ix->d_deg, (size_t)ix->n * 4, hipMemcpyDeviceToHost));
    uint64_t t = 0;
    for (uint32_t d : deg) t += d;
    *n_edges = t + ix->h_start_ext.size();
  }
  return SDB_OK;
}
SDB_API_CATCH("sdb_index_stats")

int sdb_index_row_usage(const sdb_index *ix, uint64_t *rows, uint64_t *dead) try {
  if (!ix) return fail(SDB_ERR_INVALID, "index is NULL");
  if (rows) *rows = ix->n;
  if (dead) *dead = ix->n_dead;
  return SDB_OK;
}
SDB_API_CATCH("sdb_index_row_usage")

int sdb_index_compact(sdb_index *ix) try {
  if (!ix) return fail(SDB_ERR_INVALID, "index is NULL");
  if (ix->broken) return fail(SDB_ERR_STATE, "index is unusable after a failed write; reload it from the bucket");
  if (ix->in_tx) return fail(SDB_ERR_STATE, "a write transaction is open");
  if (ix->n_dead == 0) return SDB_OK;
  DeviceGuard dg(ix->P.device);
  std::unique_lock<sdb::ViewMutex> wl(ix->view_mu);  // searches wait: every buffer they read is replaced
  SDB_HIP(hipDeviceSynchronize());
  const uint32_t n = ix->n, cap = ix->cap, ld = ix->lay.ld;
  const uint32_t M = ix->code_bytes;  // bytes of a code row (product or bit codes)
  std::vector<uint32_t> map(n, kNoSlot), live;
  live.reserve(n - ix->n_dead);
  for (uint32_t s = 0; s < n; s++)
    if (ix->h_ids[s] != 0) map[s] = (uint32_t)live.size(), live.push_back(s);
  const uint32_t nn = (uint32_t)live.size();
  // ---- every allocation first: a failure leaves the index as it was
  using T = RowTable;
  FreshBufs nb, tmp;
  std::array<void *, T::kCount> t;
  SDB_TRY(ix->alloc_row_tables(cap, nb, t, false));
  // (the neighbours' code rows follow the renumbered adjacency; without room for them the compacted index goes on without)
  const GraphCopy nwr{(uint32_t *)t[T::kWrAdj], (uint64_t *)t[T::kWrIds], nullptr, 0, (uint8_t *)t[T::kWrAdjCodes]};
  uint8_t *const ncodes = (uint8_t *)t[T::kCodes];
  uint32_t *d_live = nullptr, *d_map = nullptr, *d_lost = nullptr;
  SDB_TRY(tmp.get_n(&d_live, (size_t)nn + 1));
  SDB_TRY(tmp.get_n(&d_map, n));
  SDB_TRY(tmp.get_n(&d_lost, 1));
  SDB_HIP(hipMemcpy(d_live, live.data(), (size_t)nn * 4, hipMemcpyHostToDevice));
  SDB_HIP(hipMemcpy(d_map, map.data(), (size_t)n * 4, hipMemcpyHostToDevice));
  SDB_HIP(hipMemset(d_lost, 0, 4));
  hipLaunchKernelGGL(k_compact_rows, dim3(nn), dim3(64), 0, nullptr, d_live, d_map, ld, ix->d_slab, (float *)t[T::kSlab], ix->wr.adj,
                     nwr.adj, ix->d_adjdist, (float *)t[T::kAdjDist], ix->d_deg, (uint32_t *)t[T::kDeg], ix->d_clean,
                     (uint32_t *)t[T::kClean], ix->d_dcount, (uint32_t *)t[T::kDCount], ix->wr.ids, nwr.ids, ix->d_codes, ncodes, M,
                     d_lost);
  SDB_HIP(hipGetLastError());
  SDB_HIP(hipMemcpy(t[T::kCmAdj], nwr.adj, (size_t)cap * kAdjStride * 4, hipMemcpyDeviceToDevice));
  SDB_HIP(hipMemcpy(t[T::kCmIds], nwr.ids, (size_t)nn * 8, hipMemcpyDeviceToDevice));
  if (nwr.adjcodes && nn) {
    SDB_TRY(ix->fill_adjcodes(nwr, nn, nullptr, 0, nullptr, ncodes));
    SDB_HIP(hipMemcpy(t[T::kCmAdjCodes], nwr.adjcodes, (size_t)nn * kAdjStride * M, hipMemcpyDeviceToDevice));
  }
  uint32_t lost = 0;
  SDB_HIP(hipMemcpy(&lost, d_lost, 4, hipMemcpyDeviceToHost));
  if (lost) return fail(SDB_ERR_STATE, "%u edges point at deleted rows: the graph is inconsistent, nothing was changed", lost);
  // the host tables of the compacted index, complete before anything changes hands (their memory may not be there)
  std::vector<uint64_t> h(nn);
  for (uint32_t j = 0; j < nn; j++) h[j] = ix->h_ids[live[j]];
  std::unordered_map<uint64_t, uint32_t> nmap;
  const bool dense = index_ids(h.data(), nn, nmap);
  const uint32_t need = ix->start_ext_need();
  std::vector<uint32_t> padded(need, kNoSlot);
  // room for the committed copy of the overflow list (the writer's has it: the list does not grow here); a failure
  // leaves the copy, and the index, as they were
  SDB_TRY(ix->cm.grow_start_ext(need));
  // ---- swap in (nothing below can fail)
  ix->adopt_row_tables(nb, t);
  ix->h_ids.swap(h);
  ix->id2slot.swap(nmap);
  ix->dense_ids = dense;
  if (ix->start_slot >= 0) ix->start_slot = (int64_t)map[(uint32_t)ix->start_slot];  // a flat index has none
  for (auto &e : ix->h_start_ext) e = map[e];
  ix->n = nn, ix->n_dead = 0;
  if (need) {  // both copies of the overflow list, renumbered
    std::copy(ix->h_start_ext.begin(), ix->h_start_ext.end(), padded.begin());
    (void)hipMemcpy(ix->wr.start_ext, padded.data(), (size_t)need * 4, hipMemcpyHostToDevice);
    (void)hipMemcpy(ix->cm.start_ext, padded.data(), (size_t)need * 4, hipMemcpyHostToDevice);
  }
  ix->publish();  // (no transaction is open: nothing of one to end)
  (void)hipDeviceSynchronize();
  ix->build_sketch(nullptr, 0, true);  // rows have moved (a stale copy is never used: sketch_gen); best-effort
  return SDB_OK;
}
SDB_API_CATCH("sdb_index_compact")

int sdb_index_export(const sdb_index *ix, uint64_t *ids, float *vectors, uint64_t *offsets, uint64_t *edges) try {
  if (!ix) return fail(SDB_ERR_INVALID, "index is NULL");
  if (ix->broken) return fail(SDB_ERR_STATE, "index is unusable after a failed write; reload it from the bucket");
  DeviceGuard dg(ix->P.device);
  SDB_HIP(hipDeviceSynchronize());
  const uint32_t n = ix->n;
  // deleted nodes (tombstones: id 0) are gone from the bucket (node.go:129-134); live rows keep their order
  if (ids) {
    uint64_t k = 0;
    for (uint32_t i = 0; i < n; i++)
      if (ix->h_ids[i] != 0) ids[k++] = ix->h_ids[i];
  }
  if (offsets || edges) {
    std::vector<uint32_t> adj((size_t)n * kAdjStride), deg(n);
    if (n) {
      SDB_HIP(hipMemcpy(adj.data(), ix->wr.adj, adj.size() * 4, hipMemcpyDeviceToHost));
      SDB_HIP(hipMemcpy(deg.data(), ix->d_deg, deg.size() * 4, hipMemcpyDeviceToHost));
    }
    uint64_t o = 0, k = 0;
    for (uint32_t i = 0; i < n; i++) {
      if (ix->h_ids[i] == 0) continue;
      if (offsets) offsets[k] = o;
      for (uint32_t e = 0; e < deg[i]; e++, o++)
        if (edges) edges[o] = ix->h_ids[adj[(size_t)i * kAdjStride + e]];
      if ((int64_t)i == ix->start_slot)
        for (uint32_t t : ix->h_start_ext) {
          if (edges) edges[o] = ix->h_ids[t];
          o++;
        }
      k++;
    }
    if (offsets) offsets[k] = o;
  }
  if (vectors && n) {
    const RowLayout &l = ix->lay;
    float *tmp = nullptr;
    SDB_HIP(hipMalloc(&tmp, (size_t)n * l.dim * sizeof(float)));
    hipLaunchKernelGGL(k_unpermute_rows, dim3(n), dim3(128), 0, nullptr, ix->d_slab, tmp, n, l.dim, l.nblk, l.ng, l.ld);
    hipError_t e = hipSuccess;
    if (ix->n_dead == 0) {
      e = hipMemcpy(vectors, tmp, (size_t)n * l.dim * sizeof(float), hipMemcpyDeviceToHost);
    } else {
      std::vector<float> all((size_t)n * l.dim);
      e = hipMemcpy(all.data(), tmp, all.size() * sizeof(float), hipMemcpyDeviceToHost);
      uint64_t k = 0;
      for (uint32_t i = 0; i < n && e == hipSuccess; i++)
        if (ix->h_ids[i] != 0) memcpy(vectors + (k++) * l.dim, all.data() + (size_t)i * l.dim, l.dim * sizeof(float));
    }
    (void)hipFree(tmp);
    if (e != hipSuccess) return fail(SDB_ERR_DEVICE, "D2H copy failed: %s", hipGetErrorString(e));
  }
  return SDB_OK;
}
SDB_API_CATCH("sdb_index_export")

}  // extern "C"

