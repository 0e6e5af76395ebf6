// index_versions.hip -- the two copies of the graph (index.h graph versions): what a transaction does to them when it
// begins, commits and rolls back, the one step that publishes a view, and the ABI calls around them.
#include <algorithm>

#include "pq.h"

namespace sdb {
// rows the transaction wrote (dirty flags) and rows it appended: committed copy -> the writer's stale copy; with the
// neighbours' code rows behind them (index.h GraphCopy::adjcodes; code_bytes = 64 M per row, 0: none)
__global__ void k_sync_rows(const uint32_t *__restrict__ src_adj, uint32_t *__restrict__ dst_adj,
                            const uint64_t *__restrict__ src_ids, uint64_t *__restrict__ dst_ids,
                            uint8_t *__restrict__ dirty, uint32_t n, uint32_t first_new,
                            const uint8_t *__restrict__ src_codes, uint8_t *__restrict__ dst_codes, uint32_t code_bytes) {
  const uint32_t row = blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (row >= n) return;
  if (row < first_new && !dirty[row]) return;
  dst_adj[(size_t)row * kAdjStride + lane] = src_adj[(size_t)row * kAdjStride + lane];
  if (code_bytes) {  // a multiple of 64: whole words when M is a multiple of four, bytes otherwise
    if ((code_bytes & 255u) == 0) {
      const uint32_t *s4 = reinterpret_cast<const uint32_t *>(src_codes + (size_t)row * code_bytes);
      uint32_t *d4 = reinterpret_cast<uint32_t *>(dst_codes + (size_t)row * code_bytes);
      for (uint32_t i = lane; i < code_bytes / 4; i += 64) d4[i] = s4[i];
    } else {
      for (uint32_t i = lane; i < code_bytes; i += 64) dst_codes[(size_t)row * code_bytes + i] = src_codes[(size_t)row * code_bytes + i];
    }
  }
  if (lane == 0) dst_ids[row] = src_ids[row], dirty[row] = 0;
}
// sdb_index_abort_write: the rows the transaction wrote take the committed copy back, the rows it appended become
// empty again.  What only the write path keeps per row -- degree, clean prefix, cached edge distances -- is rebuilt
// conservatively: the degree from the row, no clean prefix, no cached distances (both only ever save work: a prune
// that finds none evaluates everything and arrives at the same row, build.hip).
__global__ void k_restore_rows(const uint32_t *__restrict__ c_adj, uint32_t *__restrict__ w_adj,
                               const uint64_t *__restrict__ c_ids, uint64_t *__restrict__ w_ids, uint32_t *__restrict__ deg,
                               uint32_t *__restrict__ clean, uint32_t *__restrict__ dcount, uint8_t *__restrict__ dirty,
                               uint32_t n_now, uint32_t n_committed) {
  const uint32_t row = blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (row >= n_now) return;
  const bool appended = row >= n_committed;
  if (!appended && !dirty[row]) return;
  const uint32_t e = appended ? kNoSlot : c_adj[(size_t)row * kAdjStride + lane];
  w_adj[(size_t)row * kAdjStride + lane] = e;
  const uint32_t d = (uint32_t)__popcll(__ballot(e != kNoSlot));
  if (lane == 0) {
    w_ids[row] = appended ? 0ull : c_ids[row];
    deg[row] = d, clean[row] = 0, dcount[row] = 0, dirty[row] = 0;
  }
}
// test support: rows on which the two copies differ
__global__ void k_count_version_diff(const uint32_t *a_adj, const uint32_t *b_adj, const uint64_t *a_ids,
                                     const uint64_t *b_ids, uint32_t n, unsigned long long *out) {
  const uint32_t row = blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (row >= n) return;
  const bool diff = a_adj[(size_t)row * kAdjStride + lane] != b_adj[(size_t)row * kAdjStride + lane] ||
                    (lane == 0 && a_ids[row] != b_ids[row]);
  if (__ballot(diff) && lane == 0) atomicAdd(out, 1ull);
}

int GraphCopy::grow_start_ext(uint32_t need) {
  if (need <= start_ext_cap) return SDB_OK;
  uint32_t *grown = nullptr;
  SDB_HIP(hipMalloc(&grown, (size_t)need * 2 * 4));
  if (start_ext) (void)hipFree(start_ext);
  start_ext = grown, start_ext_cap = need * 2;
  return SDB_OK;
}
}  // namespace sdb

using namespace sdb;

void sdb_index::publish_pointers() {
  view.adj = cm.adj, view.ids = cm.ids, view.start_ext = cm.start_ext, view.adj_codes = cm.adjcodes;
  view_gen++;
}

void sdb_index::end_tx() {
  tx_deleted.clear();
  in_tx = false, tx_explicit = false, tx_dirty = false;
}

void sdb_index::publish() {
  publish_pointers();
  view.n = n, view.start_ext_n = (uint32_t)h_start_ext.size();
  end_tx();
}

int sdb_index::begin_write() {
  if (!in_tx) in_tx = true, tx_n0 = n, tx_dead0 = n_dead, tx_max_id0 = max_node_id, tx_dirty = false;
  return SDB_OK;
}

int sdb_index::commit(hipStream_t stream) {
  if (!in_tx) return SDB_OK;
  const bool sk_current = sketch_current();  // the float16 copy describes the rows below tx_n0
  const uint32_t need = start_ext_need();
  const uint32_t ac_bytes = has_adjcodes() ? kAdjStride * pq->M : 0;
  const uint32_t first_new = tx_n0 < n ? tx_n0 : n;
  if (ac_bytes && n) {
    // the writer's copy of the neighbours' code rows catches up with what the transaction did to the adjacency rows --
    // before the copies change hands, while the searches still walk the other one
    SDB_TRY(fill_adjcodes(wr, n, d_dirty, first_new, stream));
    SDB_HIP(hipStreamSynchronize(stream));
  }
  {
    std::unique_lock<sdb::ViewMutex> wl(view_mu);
    // every search that took the old view has enqueued its kernels and recorded its event by now (it held the
    // shared lock until then): the writer's stream waits for them before it touches the copy they walk
    {
      std::lock_guard<std::mutex> g(mu);
      for (auto *w : pool)
        if (w->launched_valid) SDB_HIP(hipStreamWaitEvent(stream, w->launched, 0));
    }
    std::swap(wr, cm);
    publish();
  }
  // the writer's copy is now the one the last version's searches walked: bring it up to date
  if (n) {
    hipLaunchKernelGGL(sdb::k_sync_rows, dim3((n + 3) / 4), dim3(256), 0, stream, cm.adj, wr.adj, cm.ids, wr.ids, d_dirty, n,
                       first_new, cm.adjcodes, wr.adjcodes, ac_bytes);
    SDB_HIP(hipGetLastError());
  }
  if (need) {
    if (need > wr.start_ext_cap) {
      SDB_HIP(hipStreamSynchronize(stream));
      SDB_TRY(wr.grow_start_ext(need));
    }
    SDB_HIP(hipMemcpyAsync(wr.start_ext, cm.start_ext, (size_t)need * 4, hipMemcpyDeviceToDevice, stream));
  }
  // the float16 copy follows: on `stream`, which has waited for the searches of the old view (above); searches of the
  // new one read float32 rows until sketch_gen says the copy is theirs.  Best-effort: the write is published already.
  build_sketch(stream, sk_current && start_slot >= 0 ? tx_n0 : 0, false);
  return SDB_OK;
}

int sdb_index::rollback() {
  std::unique_lock<sdb::ViewMutex> wl(view_mu);  // searches translate filter ids with the tables changed below
  SDB_HIP(hipDeviceSynchronize());               // the transaction's kernels are done
  if (n)
    hipLaunchKernelGGL(sdb::k_restore_rows, dim3((n + 3) / 4), dim3(256), 0, nullptr, cm.adj, wr.adj, cm.ids, wr.ids, d_deg,
                       d_clean, d_dcount, d_dirty, n, tx_n0);
  SDB_HIP(hipGetLastError());
  // The writer's copy of the neighbours' code rows follows the restored adjacency rows.  commit() brings it to the
  // transaction's state BEFORE the copies change hands, so a commit that failed after that step -- or a transaction that
  // is simply aborted after its rows were written -- would leave restored rows carrying the transaction's code rows:
  // edge e walked with another node's codes, silently.  All committed rows (a rollback is rare; 64 M bytes per row).
  if (has_adjcodes() && tx_n0) SDB_TRY(fill_adjcodes(wr, tx_n0, nullptr, 0, nullptr));
  // the start node's overflow list as committed
  const uint32_t ext_n = view.start_ext_n, need = (ext_n + 63) / 64 * 64;
  h_start_ext.assign(ext_n, 0);
  if (ext_n) {
    SDB_HIP(hipMemcpy(h_start_ext.data(), cm.start_ext, (size_t)ext_n * 4, hipMemcpyDeviceToHost));
    SDB_TRY(wr.grow_start_ext(need));
    SDB_HIP(hipMemcpy(wr.start_ext, cm.start_ext, (size_t)need * 4, hipMemcpyDeviceToDevice));
  }
  SDB_HIP(hipDeviceSynchronize());
  // host tables: appended rows go, rows the transaction tombstoned get their ids back
  h_ids.resize(tx_n0);
  for (auto &kv : tx_deleted)
    if (kv.second < tx_n0) h_ids[kv.second] = kv.first;
  n = tx_n0, n_dead = tx_dead0, max_node_id = tx_max_id0;
  dense_ids = index_ids(h_ids.data(), n, id2slot);  // (a tombstoned first row: not dense)
  end_tx();
  // the committed rows are where they were: a current copy still describes them (exclusive lock held, device idle)
  if (!sketch_current() || sketch_cap < n) build_sketch(nullptr, 0, true);
  return SDB_OK;
}

int sdb_index::publish_full() {
  SDB_HIP(hipDeviceSynchronize());
  std::unique_lock<sdb::ViewMutex> wl(view_mu);
  if (n) {
    SDB_HIP(hipMemcpy(cm.adj, wr.adj, (size_t)n * kAdjStride * 4, hipMemcpyDeviceToDevice));
    SDB_HIP(hipMemcpy(cm.ids, wr.ids, (size_t)n * 8, hipMemcpyDeviceToDevice));
    SDB_HIP(hipMemset(d_dirty, 0, n));
    if (has_adjcodes()) {
      SDB_TRY(fill_adjcodes(wr, n, nullptr, 0, nullptr));
      SDB_HIP(hipMemcpy(cm.adjcodes, wr.adjcodes, (size_t)n * kAdjStride * pq->M, hipMemcpyDeviceToDevice));
    }
  }
  if (const uint32_t need = start_ext_need()) {
    SDB_TRY(cm.grow_start_ext(need));
    SDB_HIP(hipMemcpy(cm.start_ext, wr.start_ext, (size_t)need * 4, hipMemcpyDeviceToDevice));
  }
  publish();
  SDB_HIP(hipDeviceSynchronize());  // searches that slipped in between the first wait and the lock
  build_sketch(nullptr, 0, true);  // (best-effort: the view is published)
  return SDB_OK;
}

// uploads the start node's overflow edges, padded with kNoSlot to whole 64-entry chunks (search_kernel.h reads them
// like adjacency rows).  Writers are exclusive (the reference holds the shard's write lock), so nothing reads the
// old buffer once the device is idle.
int sdb_index::sync_start_ext() {
  const uint32_t need = start_ext_need();
  if (need > wr.start_ext_cap) {
    SDB_HIP(hipDeviceSynchronize());
    SDB_TRY(wr.grow_start_ext(need));
  }
  if (need) {
    std::vector<uint32_t> padded(need, kNoSlot);
    std::copy(h_start_ext.begin(), h_start_ext.end(), padded.begin());
    SDB_HIP(hipMemcpy(wr.start_ext, padded.data(), (size_t)need * 4, hipMemcpyHostToDevice));
  }
  return SDB_OK;
}

extern "C" {

// IndexVamana.InsertUpdateDelete is ONE write transaction made of several calls here (inserts, one delete scan,
// re-inserts of the updated points); the shard runs it under its write lock while searches keep being served --
// by a cold index built from the bucket when the cached one is locked (shard/cache/manager.go:159-181).  Here the
// searches simply keep walking the last committed graph: between begin_write and commit every insert_batch /
// delete_batch changes the writer's copy only.  Without begin_write each such call is a transaction by itself.
int sdb_index_begin_write(sdb_index *ix) try {
  if (!ix) return fail(SDB_ERR_INVALID, "index is NULL");
  if (ix->broken) return fail(SDB_ERR_STATE, "index is unusable after a failed write; reload it from the bucket");
  if (ix->in_tx && ix->tx_explicit) return fail(SDB_ERR_STATE, "a write transaction is already open");
  SDB_TRY(ix->begin_write());
  ix->tx_explicit = true;
  return SDB_OK;
}
SDB_API_CATCH("sdb_index_begin_write")

int sdb_index_commit(sdb_index *ix, void *stream_) try {
  if (!ix) return fail(SDB_ERR_INVALID, "index is NULL");
  if (!ix->in_tx) return fail(SDB_ERR_STATE, "no write transaction is open");
  if (ix->broken) return fail(SDB_ERR_STATE, "index is unusable after a failed write; reload it from the bucket");
  DeviceGuard dg(ix->P.device);
  hipStream_t stream = as_stream(stream_);
  SDB_TRY(ix->commit(stream));
  SDB_HIP(hipStreamSynchronize(stream));
  return SDB_OK;
}
SDB_API_CATCH("sdb_index_commit")

// The way out of a transaction that will not be committed (a host that found a bad point after begin_write, a failed
// call, a cancelled request).  Searches never saw the transaction: they walk the committed copy of the graph (index.h
// graph versions), which is exactly what a rollback needs -- the rows the transaction wrote take the committed copy
// back, the rows it appended are dropped, the host's id tables follow.  The reference has no such thing: after an
// error inside a transaction its cache manager scraps the shard's cache and rebuilds it from the bucket
// (shard/cache/manager.go:231-240); here the index is what it was at begin_write, in milliseconds.  Only a handle that
// a device failure left half-written (index.h `broken`) cannot be brought back.
int sdb_index_abort_write(sdb_index *ix) try {
  if (!ix) return fail(SDB_ERR_INVALID, "index is NULL");
  if (ix->broken) return fail(SDB_ERR_STATE, "index is unusable after a failed write; reload it from the bucket");
  if (!ix->in_tx) return SDB_OK;
  if (!ix->tx_dirty) {  // nothing to undo
    std::unique_lock<sdb::ViewMutex> wl(ix->view_mu);
    ix->end_tx();
    return SDB_OK;
  }
  DeviceGuard dg(ix->P.device);
  int rc;
  try {
    rc = ix->rollback();
  } catch (...) {
    rc = on_exception("sdb_index_abort_write");
  }
  if (rc != SDB_OK) ix->broken = true;  // a device error (or no host memory for the id tables) half-way through the restore
  return rc;
}
SDB_API_CATCH("sdb_index_abort_write")

// test support: the number of rows on which the two graph copies differ (0 whenever no transaction is open)
int sdb_index_version_diff(const sdb_index *ix, uint64_t *rows) try {
  if (!ix || !rows) return fail(SDB_ERR_INVALID, "NULL argument");
  *rows = 0;
  if (ix->n == 0) return SDB_OK;
  DeviceGuard dg(ix->P.device);
  unsigned long long *d = nullptr;
  SDB_HIP(hipMalloc(&d, 8));
  SDB_HIP(hipMemset(d, 0, 8));
  SDB_HIP(hipDeviceSynchronize());
  hipLaunchKernelGGL(k_count_version_diff, dim3((ix->n + 3) / 4), dim3(256), 0, nullptr, ix->wr.adj, ix->cm.adj, ix->wr.ids,
                     ix->cm.ids, ix->n, d);
  unsigned long long h = 0;
  hipError_t e = hipMemcpy(&h, d, 8, hipMemcpyDeviceToHost);
  (void)hipFree(d);
  if (e != hipSuccess) return fail(SDB_ERR_DEVICE, "version check failed: %s", hipGetErrorString(e));
  *rows = h;
  if (ix->h_start_ext.size()) {
    const size_t m = ix->h_start_ext.size();
    std::vector<uint32_t> a(m), b(m);
    SDB_HIP(hipMemcpy(a.data(), ix->wr.start_ext, m * 4, hipMemcpyDeviceToHost));
    SDB_HIP(hipMemcpy(b.data(), ix->cm.start_ext, m * 4, hipMemcpyDeviceToHost));
    if (a != b) *rows += 1;
  }
  return SDB_OK;
}
SDB_API_CATCH("sdb_index_version_diff")

}  // extern "C"
