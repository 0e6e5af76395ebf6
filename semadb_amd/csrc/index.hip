// index.hip -- K3 (HBM slab + adjacency loader) and the index's host-side state; the search call itself is
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
#include "wave_dist.h"

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

}  // namespace sdb

using namespace sdb;

// ------------------------------------------------------------------------------------------
// sdb_index methods
// ------------------------------------------------------------------------------------------
int sdb_index::reserve(uint32_t rows) {
  if (rows <= cap) return SDB_OK;
  uint32_t ncap = cap ? cap : 1024;
  while (ncap < rows) ncap = ncap < (1u << 30) ? ncap * 2 : rows;
  // every new buffer first; if one allocation fails the ones before it are returned and the index is as it was
  struct Fresh {
    std::vector<void *> p;
    bool keep = false;
    ~Fresh() {
      if (!keep)
        for (void *x : p)
          if (x) (void)hipFree(x);
    }
    int get(void **out, size_t bytes) {
      SDB_HIP(hipMalloc(out, bytes));
      p.push_back(*out);
      return SDB_OK;
    }
    // two buffers of a CACHE (the neighbours' code rows behind both adjacency copies): both or neither, and no room
    // for them is no error -- the index works without (searches gather code rows by slot)
    bool get_pair_if_room(void **a, void **b, size_t bytes) {
      *a = *b = nullptr;
      if (hipMalloc(a, bytes) == hipSuccess && hipMalloc(b, bytes) == hipSuccess) {
        p.push_back(*a), p.push_back(*b);
        return true;
      }
      (void)hipGetLastError();
      if (*a) (void)hipFree(*a);
      *a = *b = nullptr;
      return false;
    }
  } fresh;
  float *nslab = nullptr, *nad = nullptr;
  uint32_t *nadj = nullptr, *nradj = nullptr, *ndeg = nullptr, *nclean = nullptr, *ndc = nullptr;
  uint64_t *nids = nullptr, *nrids = nullptr;
  uint8_t *ndirty = nullptr, *ncodes = nullptr;
  std::unique_lock<std::mutex> sg(sketch_mu);  // the knob waits until the float16 copy has followed the growth
  auto get_required = [&]() -> int {
    SDB_TRY(fresh.get((void **)&nslab, (size_t)ncap * lay.ld * sizeof(float)));
    SDB_TRY(fresh.get((void **)&nadj, (size_t)ncap * kAdjStride * sizeof(uint32_t)));
    SDB_TRY(fresh.get((void **)&nradj, (size_t)ncap * kAdjStride * sizeof(uint32_t)));
    SDB_TRY(fresh.get((void **)&ndeg, (size_t)ncap * sizeof(uint32_t)));
    SDB_TRY(fresh.get((void **)&nclean, (size_t)ncap * sizeof(uint32_t)));
    SDB_TRY(fresh.get((void **)&nids, (size_t)ncap * sizeof(uint64_t)));
    SDB_TRY(fresh.get((void **)&nrids, (size_t)ncap * sizeof(uint64_t)));
    SDB_TRY(fresh.get((void **)&ndirty, (size_t)ncap));
    SDB_TRY(fresh.get((void **)&nad, (size_t)ncap * kAdjStride * sizeof(float)));  // edge-distance cache of the write path (index.h)
    SDB_TRY(fresh.get((void **)&ndc, (size_t)ncap * sizeof(uint32_t)));
    if (code_bytes) SDB_TRY(fresh.get((void **)&ncodes, (size_t)ncap * code_bytes));  // the code rows of a quantized store grow with it
    return SDB_OK;
  };
  if (int rc = get_required()) {
    if (!d_sketch) return rc;
    // a required buffer never goes without for the float16 copy's sake (a cache): drop it and try once more
    (void)hipGetLastError();
    for (void *x : fresh.p)
      if (x) (void)hipFree(x);
    fresh.p.clear();
    {
      std::unique_lock<sdb::ViewMutex> wl(view_mu);
      drop_sketch();
    }
    SDB_TRY(get_required());
  }
  uint8_t *nacw = nullptr, *nacr = nullptr;  // ... and the neighbours' code rows behind both adjacency copies
  const bool had_ac = has_adjcodes();
  size_t ac_row = had_ac ? (size_t)kAdjStride * pq->M : 0;
  // (2 x 64 M bytes per row: 41 GB at 10M rows and M = 32, more than the vectors of d = 768.  A table that grows past
  // the room for them drops them instead of failing the insert -- alloc_adjcodes treats them as optional the same way)
  if (ac_row && !fresh.get_pair_if_room((void **)&nacw, (void **)&nacr, (size_t)ncap * ac_row)) ac_row = 0;
  // the float16 copy grows with the slab, best-effort under the headroom rule: rows do not move, so it stays current and
  // the next commit converts only the rows it appends (without room the copy keeps covering the rows it has).  Chosen
  // order: a table that already serves from the copy keeps it through growth, so on a device near capacity a bulk
  // insert_batch into a grown table may find no headroom left for its pair cache (build.hip pairc) and build without
  // it -- slower, same graph -- rather than have every search fall back to float32 rows.
  const bool sk_keep = sketch_current();
  void *nsk = nullptr;
  float *nskn = nullptr;
  if (sk_keep && sketch_cap < ncap) {
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
  SDB_HIP(hipMemset(nadj, 0xFF, (size_t)ncap * kAdjStride * sizeof(uint32_t)));
  SDB_HIP(hipMemset(nradj, 0xFF, (size_t)ncap * kAdjStride * sizeof(uint32_t)));
  SDB_HIP(hipMemset(ndeg, 0, (size_t)ncap * sizeof(uint32_t)));
  SDB_HIP(hipMemset(nclean, 0, (size_t)ncap * sizeof(uint32_t)));  // loaded / appended edges are not "clean"
  SDB_HIP(hipMemset(ndirty, 0, (size_t)ncap));
  if (n) {
    SDB_HIP(hipMemcpy(nslab, d_slab, (size_t)n * lay.ld * sizeof(float), hipMemcpyDeviceToDevice));
    SDB_HIP(hipMemcpy(nadj, d_adj, (size_t)n * kAdjStride * sizeof(uint32_t), hipMemcpyDeviceToDevice));
    SDB_HIP(hipMemcpy(nradj, r_adj, (size_t)n * kAdjStride * sizeof(uint32_t), hipMemcpyDeviceToDevice));
    SDB_HIP(hipMemcpy(ndeg, d_deg, (size_t)n * sizeof(uint32_t), hipMemcpyDeviceToDevice));
    SDB_HIP(hipMemcpy(nclean, d_clean, (size_t)n * sizeof(uint32_t), hipMemcpyDeviceToDevice));
    SDB_HIP(hipMemcpy(nids, d_ids, (size_t)n * sizeof(uint64_t), hipMemcpyDeviceToDevice));
    SDB_HIP(hipMemcpy(nrids, r_ids, (size_t)n * sizeof(uint64_t), hipMemcpyDeviceToDevice));
    SDB_HIP(hipMemcpy(ndirty, d_dirty, (size_t)n, hipMemcpyDeviceToDevice));
  }
  SDB_HIP(hipMemset(ndc, 0, (size_t)ncap * sizeof(uint32_t)));  // a row without cached distances has d_dcount 0
  if (n) {
    SDB_HIP(hipMemcpy(nad, d_adjdist, (size_t)n * kAdjStride * sizeof(float), hipMemcpyDeviceToDevice));
    SDB_HIP(hipMemcpy(ndc, d_dcount, (size_t)n * sizeof(uint32_t), hipMemcpyDeviceToDevice));
    if (code_bytes) SDB_HIP(hipMemcpy(ncodes, d_codes, (size_t)n * code_bytes, hipMemcpyDeviceToDevice));
    if (ac_row) {
      SDB_HIP(hipMemcpy(nacw, d_adjcodes, (size_t)n * ac_row, hipMemcpyDeviceToDevice));
      SDB_HIP(hipMemcpy(nacr, r_adjcodes, (size_t)n * ac_row, hipMemcpyDeviceToDevice));
    }
  }
  SDB_HIP(hipDeviceSynchronize());
  {
    std::unique_lock<sdb::ViewMutex> wl(view_mu);  // searches pick their pointers up under this lock
    for (void *p : {(void *)d_slab, (void *)d_adj, (void *)r_adj, (void *)d_deg, (void *)d_clean, (void *)d_ids,
                    (void *)r_ids, (void *)d_dirty, (void *)d_adjdist, (void *)d_dcount})
      if (p) (void)hipFree(p);
    if (code_bytes && d_codes) (void)hipFree(d_codes);
    if (had_ac) (void)hipFree(d_adjcodes), (void)hipFree(r_adjcodes), d_adjcodes = nacw, r_adjcodes = nacr;  // (NULL: dropped)
    d_slab = nslab, d_adj = nadj, r_adj = nradj, d_deg = ndeg, d_clean = nclean, d_ids = nids, r_ids = nrids;
    d_dirty = ndirty, d_adjdist = nad, d_dcount = ndc;
    if (code_bytes) d_codes = ncodes;
    fresh.keep = true;
    cap = ncap;
    view.adj = r_adj, view.ids = r_ids, view.adj_codes = r_adjcodes;
    view_gen++;
    if (nsk) {
      (void)hipFree(d_sketch);
      if (d_sketch_norm) (void)hipFree(d_sketch_norm);
      d_sketch = nsk, d_sketch_norm = nskn, sketch_cap = ncap;
    }
    if (sk_keep) sketch_gen = view_gen;
  }
  return SDB_OK;
}

// ------------------------------------------------------------------------------------------
// graph versions
// ------------------------------------------------------------------------------------------
namespace sdb {
// rows the transaction wrote (dirty flags) and rows it appended: committed copy -> the writer's stale copy; with the
// neighbours' code rows behind them (index.h d_adjcodes; code_bytes = 64 M per row, 0: none)
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
// The neighbours' code rows behind the adjacency rows (index.h d_adjcodes): out[row][e] = codes[adj[row][e]], zeros behind
// the edges.  dirty != NULL: only the rows a transaction wrote or appended (first_new: rows at its start).
__global__ __launch_bounds__(256) void k_adjcodes_rows(const uint32_t *__restrict__ adj, const uint8_t *__restrict__ codes,
                                                       uint8_t *__restrict__ out, const uint8_t *__restrict__ dirty, uint32_t n,
                                                       uint32_t first_new, uint32_t M) {
  const uint32_t row = blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (row >= n) return;
  if (dirty && row < first_new && !dirty[row]) return;
  const uint32_t nb = adj[(size_t)row * kAdjStride + lane];
  const size_t at = ((size_t)row * kAdjStride + lane) * M;
  if ((M & 7u) == 0) {
    const uint2 *src = reinterpret_cast<const uint2 *>(codes + (size_t)(nb == kNoSlot ? 0u : nb) * M);
    uint2 *dst = reinterpret_cast<uint2 *>(out + at);
    for (uint32_t i = 0; i < M / 8; i++) dst[i] = nb == kNoSlot ? make_uint2(0u, 0u) : src[i];
  } else {
    for (uint32_t i = 0; i < M; i++) out[at + i] = nb == kNoSlot ? (uint8_t)0 : codes[(size_t)nb * M + i];
  }
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
}  // namespace sdb

int sdb_index::begin_write() {
  if (!in_tx) in_tx = true, tx_n0 = n, tx_dead0 = n_dead, tx_max_id0 = max_node_id, tx_dirty = false;
  return SDB_OK;
}

// ---- the float16 copy of the slab (two-precision hop) ----------------------------------------------------------
namespace sdb {
// one wave per row: element t of the row -> half t of the copy (sk_half: round to nearest, no denormals), and the
// row's ||y - y16||, ||y16|| into the table-wide maxima (non-negative floats order like their bit patterns; a NaN's
// pattern is above every number's, so a row with a NaN makes the bound NaN and the stage discards nothing)
__global__ __launch_bounds__(256) void k_sketch_rows(const float *__restrict__ slab, uint16_t *__restrict__ sk,
                                                      float *__restrict__ sk_norm, uint32_t n, uint32_t ld,
                                                      uint32_t *__restrict__ stats) {
  const uint32_t row = blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (row >= n) return;
  const float *s = slab + (size_t)row * ld;
  uint16_t *d = sk + (size_t)row * ld;
  double e2 = 0.0, n2 = 0.0;
  for (uint32_t t = lane; t < ld; t += 64) {
    const float v = s[t];
    const _Float16 h = sk_half(v);
    d[t] = __builtin_bit_cast(uint16_t, h);
    const double dv = (double)v - (double)(float)h, hv = (double)(float)h;
    e2 += dv * dv, n2 += hv * hv;
  }
  for (int o = 32; o; o >>= 1) e2 += __shfl_xor(e2, o), n2 += __shfl_xor(n2, o);
  if (lane == 0) {
    sk_norm[row] = (float)n2;  // ||y16||^2 (the sum in double: one rounding)
    const float e = (float)(sqrt(e2) * 1.0001), y = (float)(sqrt(n2) * 1.0001);  // rounded up past their own rounding
    atomicMax(stats, __float_as_uint(e < 0.0f ? 0.0f : e));
    atomicMax(stats + 1, __float_as_uint(y < 0.0f ? 0.0f : y));
  }
}

// ---- the int8 copy (SDB_TUNE_SKETCH = 3, 4; walk_stage.h Int8Rows) ----
// the largest |element| of `count` floats into *out (a NaN's pattern is above every number's)
__global__ __launch_bounds__(256) void k_sketch8_absmax(const float *__restrict__ v, size_t count, uint32_t *__restrict__ out) {
  uint32_t m = 0;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < count; i += (size_t)gridDim.x * 256) {
    const uint32_t b = __float_as_uint(fabsf(v[i]));
    m = b > m ? b : m;
  }
  for (int o = 32; o; o >>= 1) {
    const uint32_t x = (uint32_t)__shfl_xor((int)m, o);
    m = x > m ? x : m;
  }
  if ((threadIdx.x & 63) == 0 && m) atomicMax(out, m);
}
// one wave per row: y8 = clamp(rint(y / s), -127, 127) (s == 0, a table of zeros: 0), element 128 g + 4 L + k of the row at
// byte 4 ng L + 4 g + k of the copy's (a lane of the walk reads its 4 ng bytes with one load); the row's ||y - s y8|| and
// ||s y8||, measured in double and rounded up, into the table-wide maxima stats[0], stats[1], and its error relative to its
// own norm into stats[3] (rows of zeros have none).  A NaN or Inf in a row makes its figures NaN or infinite, and the
// maxima with them: the stage then discards nothing (and the table fails kSketch8MaxRatio).
__global__ __launch_bounds__(256) void k_sketch8_rows(const float *__restrict__ slab, uint8_t *__restrict__ sk, uint32_t n,
                                                       uint32_t ld, uint32_t ng, float scale, uint32_t *__restrict__ stats) {
  const uint32_t row = blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (row >= n) return;
  const float *s = slab + (size_t)row * ld;
  uint8_t *d = sk + (size_t)row * ld;
  double e2 = 0.0, n2 = 0.0, y2 = 0.0;
  for (uint32_t t = lane; t < ld; t += 64) {
    const float v = s[t];
    const float f = scale != 0.0f ? fminf(fmaxf(__builtin_rintf(__fdiv_rn(v, scale)), -127.0f), 127.0f) : 0.0f;
    const uint32_t g = t >> 7, r = t & 127u;
    d[(r >> 2) * 4 * ng + g * 4 + (r & 3u)] = (uint8_t)(int8_t)(int)f;
    const double hv = (double)scale * (double)f, dv = (double)v - hv;
    e2 += dv * dv, n2 += hv * hv, y2 += (double)v * (double)v;
  }
  for (int o = 32; o; o >>= 1) e2 += __shfl_xor(e2, o), n2 += __shfl_xor(n2, o), y2 += __shfl_xor(y2, o);
  if (lane == 0) {
    const float e = (float)(sqrt(e2) * 1.0001), y = (float)(sqrt(n2) * 1.0001);  // rounded up past their own rounding
    atomicMax(stats, __float_as_uint(e < 0.0f ? 0.0f : e));
    atomicMax(stats + 1, __float_as_uint(y < 0.0f ? 0.0f : y));
    if (!(y2 == 0.0)) {
      const float rel = (float)(sqrt(e2 / y2) * 1.0001);
      atomicMax(stats + 3, __float_as_uint(rel < 0.0f ? 0.0f : rel));
    }
  }
}
}  // namespace sdb

bool sdb_index::sketch8_supported() const {
  return sketch_supported() && stage_int8((int)lay.ng, P.metric == SDB_METRIC_EUCLIDEAN, false);
}

bool sdb_index::sketch_supported() const {
  if (lay.tail != 0 || pq || bq) return false;
  return stage_shape((int)lay.ng);
}

bool sdb_index::sketch_room(size_t bytes) {
  size_t free_b = 0, total_b = 0;
  if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) {
    (void)hipGetLastError();
    return false;
  }
  return free_b >= bytes + std::max<size_t>((size_t)4 << 30, total_b / 16);
}

void sdb_index::drop_sketch() {
  if (d_sketch || d_sketch_norm) (void)hipDeviceSynchronize();  // walks of earlier views may still read it
  if (d_sketch) (void)hipFree(d_sketch);
  if (d_sketch_norm) (void)hipFree(d_sketch_norm);
  d_sketch = nullptr, d_sketch_norm = nullptr, sketch_cap = 0, sketch_gen = 0, sketch8 = false;
}

// `from` > 0: the copy is current for rows [0, from) -- a Vamana table never rewrites a committed row, it appends
// (updates are delete + insert, vamana.go:170-251) -- and only the rows behind them are converted; the two maxima
// carry on from their values (they stay upper bounds when rows are deleted).  Pointers, capacity, maxima and the
// generation change under the exclusive view lock; the conversion runs outside it when the caller does not hold it
// (commit: searches of the new view go on reading float32 rows until sketch_gen names it).  Rows below `from` are
// not written, so the walks of the previous view that still read them are undisturbed.
void sdb_index::build_sketch(hipStream_t stream, uint32_t from, bool locked) {
  std::unique_lock<std::mutex> sg(sketch_mu, std::defer_lock);
  std::unique_lock<sdb::ViewMutex> wl(view_mu, std::defer_lock);
  if (!locked) sg.lock(), wl.lock();
  if (!tune_sketch || !sketch_supported()) {  // off, or a table the walk cannot take it for: no memory held for it
    drop_sketch();
    return;
  }
  // SDB_TUNE_SKETCH = 3, 4: the int8 copy where the table has that stage; a table whose rows fail kSketch8MaxRatio (now, or
  // with the rows a later commit appends) frees it and takes the float16 copy from then on
  if (build_sketch_kind(stream, from, locked, wl, sketch8_wanted()) == 2) {
    sketch8_refused = true;
    drop_sketch();
    (void)build_sketch_kind(stream, 0, locked, wl, false);
  }
}

int sdb_index::build_sketch_kind(hipStream_t stream, uint32_t from, bool locked, std::unique_lock<sdb::ViewMutex> &wl, bool int8) {
  if (d_sketch && sketch8 != int8) drop_sketch();  // the other kind of copy (the knob moved between 1 / 2 and 3 / 4): never both
  const bool carry = from > 0 && from <= n && d_sketch && sketch_cap >= n && sketch_gen != 0;
  if (!carry) from = 0;
  sketch_gen = 0;
  if (n == 0) return 0;
  const bool reused = d_sketch != nullptr;
  if (sketch_cap < n) {
    drop_sketch();
    const size_t rows = (size_t)cap * sketch_row_bytes(int8), norms = int8 ? 0 : (size_t)cap * sizeof(float);
    // a cache: without room for it (the rule of build.hip's pair cache) the walk reads float32 rows
    if (!sketch_room(rows + norms) || hipMalloc(&d_sketch, rows) != hipSuccess || (norms && hipMalloc(&d_sketch_norm, norms) != hipSuccess)) {
      (void)hipGetLastError();  // (a failed hipMalloc of this cache)
      drop_sketch();
      return 1;
    }
    sketch_cap = cap, sketch8 = int8;
  }
  if (!d_sk_counters) {
    if (hipMalloc(&d_sk_counters, 4 * sizeof(unsigned long long)) != hipSuccess ||
        hipMemset(d_sk_counters, 0, 4 * sizeof(unsigned long long)) != hipSuccess) {  // (the copy is optional: so is this)
      (void)hipGetLastError();  // (a failed allocation or memset of this cache)
      if (d_sk_counters) (void)hipFree(d_sk_counters);
      d_sk_counters = nullptr;
      drop_sketch();
      return 1;
    }
  }
  void *const sk = d_sketch;
  float *const sk_norm = d_sketch_norm;
  uint32_t *stats = reinterpret_cast<uint32_t *>(d_sk_counters + 2);  // four words: the two maxima; int8: + the new rows' largest |element|, the largest relative row error
  uint32_t h[4] = {0, 0, 0, 0};
  if (from) memcpy(&h[0], &sk_emax, 4), memcpy(&h[1], &sk_ymax, 4), memcpy(&h[3], &sk8_rel, 4);
  const uint32_t rows = n, ld = lay.ld, ng = lay.ng;
  const float *slab = d_slab;
  float scale = sk8_scale, amax = sk8_amax;
  bool ok = true;
  if (int8) {
    // The scale: appended rows inside the table's range take the scale the copy has; rows beyond it (and a first build)
    // set a new one from the largest |element| of ALL rows, and every row is converted again -- one pass over the slab.
    // Walks of the previous view may still read the copy they were given: they finish before a row of it is rewritten.
    float newmax = 0.0f;
    ok = hipMemcpyAsync(stats, h, 16, hipMemcpyHostToDevice, stream) == hipSuccess;
    if (ok && rows > from) {
      const size_t count = (size_t)(rows - from) * ld;
      hipLaunchKernelGGL(sdb::k_sketch8_absmax, dim3((uint32_t)std::min<size_t>((count + 255) / 256, 4096)), dim3(256), 0, stream,
                         slab + (size_t)from * ld, count, stats + 2);
      ok = hipGetLastError() == hipSuccess;
    }
    ok = ok && hipMemcpyAsync(&newmax, stats + 2, 4, hipMemcpyDeviceToHost, stream) == hipSuccess;
    ok = hipStreamSynchronize(stream) == hipSuccess && ok;
    if (ok && !(from && newmax <= amax)) {  // (a NaN among the new rows: not inside any range)
      amax = (!from || newmax > amax || newmax != newmax) ? newmax : amax;
      const float s0 = amax / 127.0f;
      scale = (s0 > 0.0f && s0 < 3.0e38f) ? nextafterf(s0, 3.4e38f) : s0;  // rounded up; 0 (a table of zeros), Inf and NaN as they are
      from = 0, h[0] = h[1] = h[3] = 0;
      if (reused) ok = hipDeviceSynchronize() == hipSuccess;
    }
  }
  if (!locked) wl.unlock();  // (sketch_mu stays held: the knob cannot free the copy under the kernel)
  ok = ok && hipMemcpyAsync(stats, h, 16, hipMemcpyHostToDevice, stream) == hipSuccess;
  if (ok && rows > from) {
    if (int8)
      hipLaunchKernelGGL(sdb::k_sketch8_rows, dim3((rows - from + 3) / 4), dim3(256), 0, stream, slab + (size_t)from * ld,
                         static_cast<uint8_t *>(sk) + (size_t)from * ld, rows - from, ld, ng, scale, stats);
    else
      hipLaunchKernelGGL(sdb::k_sketch_rows, dim3((rows - from + 3) / 4), dim3(256), 0, stream, slab + (size_t)from * ld,
                         static_cast<uint16_t *>(sk) + (size_t)from * ld, sk_norm + from, rows - from, ld, stats);
    ok = hipGetLastError() == hipSuccess;
  }
  ok = ok && hipMemcpyAsync(h, stats, 16, hipMemcpyDeviceToHost, stream) == hipSuccess;
  ok = hipStreamSynchronize(stream) == hipSuccess && ok;
  if (!locked) wl.lock();
  if (!ok) {  // best-effort: the write this follows has been published; its searches read float32 rows
    (void)hipGetLastError();
    drop_sketch();
    return 1;
  }
  if (int8) {
    float e, y, rel;
    memcpy(&e, &h[0], 4), memcpy(&y, &h[1], 4), memcpy(&rel, &h[3], 4);
    if (!(e <= kSketch8MaxRatio * y) || !(rel <= kSketch8MaxRatio)) return 2;  // (NaN and Inf included)
    sk8_scale = scale, sk8_amax = amax, sk8_rel = rel;
  }
  memcpy(&sk_emax, &h[0], 4), memcpy(&sk_ymax, &h[1], 4);
  sketch_gen = view_gen;
  return 0;
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

int sdb_index::alloc_adjcodes() {
  if (d_adjcodes) (void)hipFree(d_adjcodes);
  if (r_adjcodes) (void)hipFree(r_adjcodes);
  d_adjcodes = r_adjcodes = nullptr;
  view.adj_codes = nullptr;
  if (!pq || pq->M > kAdjCodesMaxM) return SDB_OK;
  const size_t bytes = (size_t)cap * kAdjStride * pq->M;
  // a cache of what the code rows hold: without room for it the walk gathers by slot, as it does for larger M
  if (hipMalloc(&d_adjcodes, bytes) != hipSuccess || hipMalloc(&r_adjcodes, bytes) != hipSuccess) {
    (void)hipGetLastError();
    if (d_adjcodes) (void)hipFree(d_adjcodes);
    d_adjcodes = r_adjcodes = nullptr;
  }
  return SDB_OK;
}

int sdb_index::rebuild_adjcodes(hipStream_t stream) {
  if (!has_adjcodes()) return SDB_OK;
  const uint32_t M = pq->M;
  if (n) hipLaunchKernelGGL(sdb::k_adjcodes_rows, dim3((n + 3) / 4), dim3(256), 0, stream, d_adj, d_codes, d_adjcodes, nullptr, n, 0u, M);
  if (view.n)
    hipLaunchKernelGGL(sdb::k_adjcodes_rows, dim3((view.n + 3) / 4), dim3(256), 0, stream, r_adj, d_codes, r_adjcodes, nullptr, view.n,
                       0u, M);
  SDB_HIP(hipGetLastError());
  SDB_HIP(hipStreamSynchronize(stream));
  view.adj_codes = r_adjcodes;
  return SDB_OK;
}

int sdb_index::commit(hipStream_t stream) {
  if (!in_tx) return SDB_OK;
  const bool sk_current = sketch_current();  // the float16 copy describes the rows below tx_n0
  const uint32_t need = (uint32_t)((h_start_ext.size() + 63) / 64 * 64);
  const uint32_t ac_bytes = has_adjcodes() ? kAdjStride * pq->M : 0;
  if (ac_bytes && n) {
    // the writer's copy of the neighbours' code rows catches up with what the transaction did to the adjacency rows --
    // before the copies change hands, while the searches still walk the other one
    hipLaunchKernelGGL(sdb::k_adjcodes_rows, dim3((n + 3) / 4), dim3(256), 0, stream, d_adj, d_codes, d_adjcodes, d_dirty, n,
                       tx_n0 < n ? tx_n0 : n, pq->M);
    SDB_HIP(hipGetLastError());
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
    std::swap(d_adj, r_adj);
    std::swap(d_adjcodes, r_adjcodes);
    std::swap(d_ids, r_ids);
    std::swap(d_start_ext, r_start_ext);
    std::swap(start_ext_cap, r_start_ext_cap);
    view.n = n, view.adj = r_adj, view.ids = r_ids, view.start_ext = r_start_ext;
    view.start_ext_n = (uint32_t)h_start_ext.size();
    view.adj_codes = r_adjcodes;
    view_gen++;
    tx_deleted.clear();
    in_tx = false, tx_explicit = false, tx_dirty = false;
  }
  // the writer's copy is now the one the last version's searches walked: bring it up to date
  if (n) {
    hipLaunchKernelGGL(sdb::k_sync_rows, dim3((n + 3) / 4), dim3(256), 0, stream, r_adj, d_adj, r_ids, d_ids, d_dirty, n,
                       tx_n0 < n ? tx_n0 : n, r_adjcodes, d_adjcodes, ac_bytes);
    SDB_HIP(hipGetLastError());
  }
  if (need) {
    if (need > start_ext_cap) {
      SDB_HIP(hipStreamSynchronize(stream));
      if (d_start_ext) (void)hipFree(d_start_ext);
      d_start_ext = nullptr, start_ext_cap = 0;
      SDB_HIP(hipMalloc(&d_start_ext, (size_t)need * 2 * 4));
      start_ext_cap = need * 2;
    }
    SDB_HIP(hipMemcpyAsync(d_start_ext, r_start_ext, (size_t)need * 4, hipMemcpyDeviceToDevice, stream));
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
    hipLaunchKernelGGL(sdb::k_restore_rows, dim3((n + 3) / 4), dim3(256), 0, nullptr, r_adj, d_adj, r_ids, d_ids, d_deg,
                       d_clean, d_dcount, d_dirty, n, tx_n0);
  SDB_HIP(hipGetLastError());
  // The writer's copy of the neighbours' code rows follows the restored adjacency rows.  commit() brings it to the
  // transaction's state BEFORE the copies change hands, so a commit that failed after that step -- or a transaction that
  // is simply aborted after its rows were written -- would leave restored rows carrying the transaction's code rows:
  // edge e walked with another node's codes, silently.  All committed rows (a rollback is rare; 64 M bytes per row).
  if (has_adjcodes() && tx_n0) {
    hipLaunchKernelGGL(sdb::k_adjcodes_rows, dim3((tx_n0 + 3) / 4), dim3(256), 0, nullptr, d_adj, d_codes, d_adjcodes, nullptr,
                       tx_n0, 0u, pq->M);
    SDB_HIP(hipGetLastError());
  }
  // the start node's overflow list as committed
  const uint32_t ext_n = view.start_ext_n, need = (ext_n + 63) / 64 * 64;
  h_start_ext.assign(ext_n, 0);
  if (ext_n) {
    SDB_HIP(hipMemcpy(h_start_ext.data(), r_start_ext, (size_t)ext_n * 4, hipMemcpyDeviceToHost));
    if (need > start_ext_cap) {
      if (d_start_ext) (void)hipFree(d_start_ext);
      d_start_ext = nullptr, start_ext_cap = 0;
      SDB_HIP(hipMalloc(&d_start_ext, (size_t)need * 2 * 4));
      start_ext_cap = need * 2;
    }
    SDB_HIP(hipMemcpy(d_start_ext, r_start_ext, (size_t)need * 4, hipMemcpyDeviceToDevice));
  }
  SDB_HIP(hipDeviceSynchronize());
  // host tables: appended rows go, rows the transaction tombstoned get their ids back
  h_ids.resize(tx_n0);
  for (auto &kv : tx_deleted)
    if (kv.second < tx_n0) h_ids[kv.second] = kv.first;
  n = tx_n0, n_dead = tx_dead0, max_node_id = tx_max_id0;
  bool dense = n > 0;
  for (uint32_t i = 1; i < n && dense; i++) dense = h_ids[i] == h_ids[0] + i;
  if (n && h_ids[0] == 0) dense = false;
  dense_ids = n == 0 ? true : dense;
  id2slot.clear();
  if (!dense_ids) {
    id2slot.reserve((size_t)n * 2);
    for (uint32_t sl = 0; sl < n; sl++)
      if (h_ids[sl] != 0) id2slot.emplace(h_ids[sl], sl);
  }
  tx_deleted.clear();
  in_tx = false, tx_explicit = false, tx_dirty = false;
  // the committed rows are where they were: a current copy still describes them (exclusive lock held, device idle)
  if (!sketch_current() || sketch_cap < n) build_sketch(nullptr, 0, true);
  return SDB_OK;
}

int sdb_index::publish_full() {
  SDB_HIP(hipDeviceSynchronize());
  std::unique_lock<sdb::ViewMutex> wl(view_mu);
  if (n) {
    SDB_HIP(hipMemcpy(r_adj, d_adj, (size_t)n * kAdjStride * 4, hipMemcpyDeviceToDevice));
    SDB_HIP(hipMemcpy(r_ids, d_ids, (size_t)n * 8, hipMemcpyDeviceToDevice));
    SDB_HIP(hipMemset(d_dirty, 0, n));
    if (has_adjcodes()) {
      hipLaunchKernelGGL(sdb::k_adjcodes_rows, dim3((n + 3) / 4), dim3(256), 0, nullptr, d_adj, d_codes, d_adjcodes, nullptr, n, 0u, pq->M);
      SDB_HIP(hipGetLastError());
      SDB_HIP(hipMemcpy(r_adjcodes, d_adjcodes, (size_t)n * kAdjStride * pq->M, hipMemcpyDeviceToDevice));
    }
  }
  const uint32_t need = (uint32_t)((h_start_ext.size() + 63) / 64 * 64);
  if (need) {
    if (need > r_start_ext_cap) {
      if (r_start_ext) (void)hipFree(r_start_ext);
      r_start_ext = nullptr, r_start_ext_cap = 0;
      SDB_HIP(hipMalloc(&r_start_ext, (size_t)need * 2 * 4));
      r_start_ext_cap = need * 2;
    }
    SDB_HIP(hipMemcpy(r_start_ext, d_start_ext, (size_t)need * 4, hipMemcpyDeviceToDevice));
  }
  view.n = n, view.adj = r_adj, view.ids = r_ids, view.start_ext = r_start_ext;
  view.start_ext_n = (uint32_t)h_start_ext.size();
  view.adj_codes = r_adjcodes;
  view_gen++;
  tx_deleted.clear();
  in_tx = false, tx_explicit = false, tx_dirty = false;
  SDB_HIP(hipDeviceSynchronize());  // searches that slipped in between the first wait and the lock
  build_sketch(nullptr, 0, true);  // (best-effort: the view is published)
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

// uploads the start node's overflow edges, padded with kNoSlot to whole 64-entry chunks (search_kernel.h reads them
// like adjacency rows).  Writers are exclusive (the reference holds the shard's write lock), so nothing reads the
// old buffer once the device is idle.
int sdb_index::sync_start_ext() {
  const uint32_t need = (uint32_t)((h_start_ext.size() + 63) / 64 * 64);
  if (need > start_ext_cap) {
    SDB_HIP(hipDeviceSynchronize());
    if (d_start_ext) (void)hipFree(d_start_ext);
    d_start_ext = nullptr, start_ext_cap = 0;
    const uint32_t ncap = need * 2;
    SDB_HIP(hipMalloc(&d_start_ext, (size_t)ncap * 4));
    start_ext_cap = ncap;
  }
  if (need) {
    std::vector<uint32_t> padded(need, kNoSlot);
    std::copy(h_start_ext.begin(), h_start_ext.end(), padded.begin());
    SDB_HIP(hipMemcpy(d_start_ext, padded.data(), (size_t)need * 4, hipMemcpyHostToDevice));
  }
  return SDB_OK;
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
  if (ix->d_slab) (void)hipFree(ix->d_slab);
  ix->drop_sketch();
  if (ix->d_sk_counters) (void)hipFree(ix->d_sk_counters);
  if (ix->d_adj) (void)hipFree(ix->d_adj);
  if (ix->d_deg) (void)hipFree(ix->d_deg);
  if (ix->d_clean) (void)hipFree(ix->d_clean);
  if (ix->d_adjdist) (void)hipFree(ix->d_adjdist);
  if (ix->d_dcount) (void)hipFree(ix->d_dcount);
  if (ix->d_ids) (void)hipFree(ix->d_ids);
  if (ix->r_adj) (void)hipFree(ix->r_adj);
  if (ix->r_ids) (void)hipFree(ix->r_ids);
  if (ix->idmap.keys) (void)hipFree(ix->idmap.keys);
  if (ix->idmap.vals) (void)hipFree(ix->idmap.vals);
  if (ix->r_start_ext) (void)hipFree(ix->r_start_ext);
  if (ix->d_dirty) (void)hipFree(ix->d_dirty);
  if (ix->d_start_ext) (void)hipFree(ix->d_start_ext);
  if (ix->d_codes) (void)hipFree(ix->d_codes);
  if (ix->d_adjcodes) (void)hipFree(ix->d_adjcodes);
  if (ix->r_adjcodes) (void)hipFree(ix->r_adjcodes);
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

// copies n original-layout rows (host or device) into slab rows [first, first+n)
static int store_rows(sdb_index *ix, uint32_t first, uint32_t n, const float *vectors, int mem, hipStream_t stream);
static int store_rows(sdb_index *ix, uint32_t first, uint32_t n, const float *vectors, int mem,
                      hipStream_t stream) {
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
static int encode_bit_rows(sdb_index *ix, uint32_t first, uint32_t n, hipStream_t stream) {
  return bq_encode_slab(ix->bq->d_thr, ix->lay, ix->d_slab, first, n, reinterpret_cast<uint64_t *>(ix->d_codes), stream);
}
int sdb_index_set_start(sdb_index *ix, const float *vec, int mem) try {
  if (!ix || !vec) return fail(SDB_ERR_INVALID, "NULL argument");
  if (ix->start_slot >= 0) return SDB_OK;  // vamana.go:95-97: already there
  if (ix->n != 0) return fail(SDB_ERR_STATE, "start node must be the first node of an empty index");
  DeviceGuard dg(ix->P.device);
  SDB_TRY(ix->reserve(1));
  SDB_TRY(store_rows(ix, 0, 1, vec, mem, nullptr));
  if (ix->bq) SDB_TRY(encode_bit_rows(ix, 0, 1, nullptr));  // vecStore.Set encodes (binary.go:131-139)
  uint64_t id = SDB_STARTID;
  SDB_HIP(hipMemcpy(ix->d_ids, &id, sizeof(id), hipMemcpyHostToDevice));
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
        (void)hipMemset(ix->d_adj, 0xFF, (size_t)wrote * kAdjStride * 4);
        (void)hipMemset(ix->d_deg, 0, (size_t)wrote * 4);
        (void)hipDeviceSynchronize();
      }
    }
  } undo{ix};
  // id table
  ix->h_ids.resize(n);
  bool dense = true;
  for (uint64_t i = 0; i < n; i++) {
    ix->h_ids[i] = ids ? ids[i] : i + 1;
    if (i && ix->h_ids[i] != ix->h_ids[0] + i) dense = false;
  }
  ix->dense_ids = dense;
  ix->id2slot.clear();
  ix->start_slot = -1;
  ix->max_node_id = 0;
  if (!dense) ix->id2slot.reserve(n * 2);
  for (uint64_t i = 0; i < n; i++) {
    uint64_t id = ix->h_ids[i];
    if (id == 0) {
      ix->h_ids.clear();
      return fail(SDB_ERR_INVALID, "invalid point id: 0");
    }
    if (!dense && !ix->id2slot.emplace(id, (uint32_t)i).second) {
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
  SDB_HIP(hipMemcpy(ix->d_adj, adj.data(), adj.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
  SDB_HIP(hipMemcpy(ix->d_deg, deg.data(), deg.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
  SDB_HIP(hipMemcpy(ix->d_ids, ix->h_ids.data(), n * sizeof(uint64_t), hipMemcpyHostToDevice));
  SDB_TRY(store_rows(ix, 0, (uint32_t)n, vectors, mem, nullptr));
  if (ix->bq) SDB_TRY(encode_bit_rows(ix, 0, (uint32_t)n, nullptr));
  SDB_TRY(ix->publish_full());
  undo.keep = true;
  return SDB_OK;
}
SDB_API_CATCH("sdb_index_load")

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
    ix->tx_deleted.clear();
    ix->in_tx = false, ix->tx_explicit = false;
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
  hipLaunchKernelGGL(k_count_version_diff, dim3((ix->n + 3) / 4), dim3(256), 0, nullptr, ix->d_adj, ix->r_adj, ix->d_ids,
                     ix->r_ids, ix->n, d);
  unsigned long long h = 0;
  hipError_t e = hipMemcpy(&h, d, 8, hipMemcpyDeviceToHost);
  (void)hipFree(d);
  if (e != hipSuccess) return fail(SDB_ERR_DEVICE, "version check failed: %s", hipGetErrorString(e));
  *rows = h;
  if (ix->h_start_ext.size()) {
    const size_t m = ix->h_start_ext.size();
    std::vector<uint32_t> a(m), b(m);
    SDB_HIP(hipMemcpy(a.data(), ix->d_start_ext, m * 4, hipMemcpyDeviceToHost));
    SDB_HIP(hipMemcpy(b.data(), ix->r_start_ext, m * 4, hipMemcpyDeviceToHost));
    if (a != b) *rows += 1;
  }
  return SDB_OK;
}
SDB_API_CATCH("sdb_index_version_diff")

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

int sdb_index_sketch_stats(sdb_index *ix, uint64_t out[3]) try {
  if (!ix || !out) return fail(SDB_ERR_INVALID, "NULL argument");
  DeviceGuard dg(ix->P.device);
  out[0] = out[1] = out[2] = 0;
  std::shared_lock<sdb::ViewMutex> rl(ix->view_mu);
  if (ix->d_sk_counters) {
    SDB_HIP(hipDeviceSynchronize());
    unsigned long long h[2] = {0, 0};
    SDB_HIP(hipMemcpy(h, ix->d_sk_counters, sizeof(h), hipMemcpyDeviceToHost));
    out[0] = h[0], out[1] = h[1];
  }
  out[2] = (ix->tune_sketch && ix->sketch_current() && !ix->in_tx) ? 1 : 0;
  return SDB_OK;
}
SDB_API_CATCH("sdb_index_sketch_stats")

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
  struct Bufs {
    std::vector<void *> p;
    bool keep = false;
    ~Bufs() {
      if (!keep)
        for (void *x : p)
          if (x) (void)hipFree(x);
    }
    int get(void **out, size_t bytes) {
      SDB_HIP(hipMalloc(out, bytes));
      p.push_back(*out);
      return SDB_OK;
    }
  } nb, tmp;
  float *nslab = nullptr, *nad = nullptr;
  uint32_t *nadj = nullptr, *nradj = nullptr, *ndeg = nullptr, *nclean = nullptr, *ndc = nullptr;
  uint64_t *nids = nullptr, *nrids = nullptr;
  uint8_t *ncodes = nullptr;
  uint32_t *d_live = nullptr, *d_map = nullptr, *d_lost = nullptr;
  SDB_TRY(nb.get((void **)&nslab, (size_t)cap * ld * 4));
  SDB_TRY(nb.get((void **)&nadj, (size_t)cap * kAdjStride * 4));
  SDB_TRY(nb.get((void **)&nradj, (size_t)cap * kAdjStride * 4));
  SDB_TRY(nb.get((void **)&nad, (size_t)cap * kAdjStride * 4));
  SDB_TRY(nb.get((void **)&ndeg, (size_t)cap * 4));
  SDB_TRY(nb.get((void **)&nclean, (size_t)cap * 4));
  SDB_TRY(nb.get((void **)&ndc, (size_t)cap * 4));
  SDB_TRY(nb.get((void **)&nids, (size_t)cap * 8));
  SDB_TRY(nb.get((void **)&nrids, (size_t)cap * 8));
  if (M) SDB_TRY(nb.get((void **)&ncodes, (size_t)cap * M));
  uint8_t *nacw = nullptr, *nacr = nullptr;  // the neighbours' code rows follow the renumbered adjacency
  const bool had_ac = ix->has_adjcodes();
  if (had_ac && (hipMalloc((void **)&nacw, (size_t)cap * kAdjStride * M) != hipSuccess ||
                 hipMalloc((void **)&nacr, (size_t)cap * kAdjStride * M) != hipSuccess)) {
    // a cache (reserve, alloc_adjcodes): without room for its second copy the compacted index goes on without it
    (void)hipGetLastError();
    if (nacw) (void)hipFree(nacw);
    nacw = nacr = nullptr;
  }
  struct AcGuard {  // until they change hands below
    uint8_t *&a, *&b;
    bool keep = false;
    ~AcGuard() {
      if (!keep) {
        if (a) (void)hipFree(a);
        if (b) (void)hipFree(b);
      }
    }
  } ac_guard{nacw, nacr};
  SDB_TRY(tmp.get((void **)&d_live, (size_t)nn * 4 + 4));
  SDB_TRY(tmp.get((void **)&d_map, (size_t)n * 4));
  SDB_TRY(tmp.get((void **)&d_lost, 4));
  SDB_HIP(hipMemcpy(d_live, live.data(), (size_t)nn * 4, hipMemcpyHostToDevice));
  SDB_HIP(hipMemcpy(d_map, map.data(), (size_t)n * 4, hipMemcpyHostToDevice));
  SDB_HIP(hipMemset(d_lost, 0, 4));
  SDB_HIP(hipMemset(nadj, 0xFF, (size_t)cap * kAdjStride * 4));
  SDB_HIP(hipMemset(ndeg, 0, (size_t)cap * 4));
  SDB_HIP(hipMemset(nclean, 0, (size_t)cap * 4));
  SDB_HIP(hipMemset(ndc, 0, (size_t)cap * 4));
  hipLaunchKernelGGL(k_compact_rows, dim3(nn), dim3(64), 0, nullptr, d_live, d_map, ld, ix->d_slab, nslab, ix->d_adj, nadj,
                     ix->d_adjdist, nad, ix->d_deg, ndeg, ix->d_clean, nclean, ix->d_dcount, ndc, ix->d_ids, nids,
                     ix->d_codes, ncodes, M, d_lost);
  SDB_HIP(hipGetLastError());
  SDB_HIP(hipMemcpy(nradj, nadj, (size_t)cap * kAdjStride * 4, hipMemcpyDeviceToDevice));
  SDB_HIP(hipMemcpy(nrids, nids, (size_t)nn * 8, hipMemcpyDeviceToDevice));
  if (nacw && nn) {
    hipLaunchKernelGGL(k_adjcodes_rows, dim3((nn + 3) / 4), dim3(256), 0, nullptr, nadj, ncodes, nacw, nullptr, nn, 0u, M);
    SDB_HIP(hipGetLastError());
    SDB_HIP(hipMemcpy(nacr, nacw, (size_t)nn * kAdjStride * M, hipMemcpyDeviceToDevice));
  }
  uint32_t lost = 0;
  SDB_HIP(hipMemcpy(&lost, d_lost, 4, hipMemcpyDeviceToHost));
  if (lost) return fail(SDB_ERR_STATE, "%u edges point at deleted rows: the graph is inconsistent, nothing was changed", lost);
  // the host tables of the compacted index, complete before anything changes hands (their memory may not be there)
  std::vector<uint64_t> h(nn);
  bool dense = true;
  for (uint32_t j = 0; j < nn; j++) {
    h[j] = ix->h_ids[live[j]];
    if (j && h[j] != h[0] + j) dense = false;
  }
  std::unordered_map<uint64_t, uint32_t> nmap;
  if (!dense) {
    nmap.reserve((size_t)nn * 2);
    for (uint32_t j = 0; j < nn; j++) nmap.emplace(h[j], j);
  }
  std::vector<uint32_t> padded((ix->h_start_ext.size() + 63) / 64 * 64, kNoSlot);
  // ---- swap in (nothing below can fail)
  for (void *x : {(void *)ix->d_slab, (void *)ix->d_adj, (void *)ix->r_adj, (void *)ix->d_adjdist, (void *)ix->d_deg,
                  (void *)ix->d_clean, (void *)ix->d_dcount, (void *)ix->d_ids, (void *)ix->r_ids})
    (void)hipFree(x);
  if (M) (void)hipFree(ix->d_codes);
  if (had_ac) (void)hipFree(ix->d_adjcodes), (void)hipFree(ix->r_adjcodes), ix->d_adjcodes = nacw, ix->r_adjcodes = nacr;  // (NULL: dropped)
  ac_guard.keep = true;
  nb.keep = true;
  ix->d_slab = nslab, ix->d_adj = nadj, ix->r_adj = nradj, ix->d_adjdist = nad, ix->d_deg = ndeg, ix->d_clean = nclean;
  ix->d_dcount = ndc, ix->d_ids = nids, ix->r_ids = nrids;
  if (M) ix->d_codes = ncodes;
  (void)hipMemset(ix->d_dirty, 0, cap);
  ix->h_ids.swap(h);
  ix->id2slot.swap(nmap);
  ix->dense_ids = dense;
  if (ix->start_slot >= 0) ix->start_slot = (int64_t)map[(uint32_t)ix->start_slot];  // a flat index has none
  for (auto &t : ix->h_start_ext) t = map[t];
  ix->n = nn, ix->n_dead = 0;
  const uint32_t need = (uint32_t)((ix->h_start_ext.size() + 63) / 64 * 64);
  if (need) {  // both copies of the overflow list, renumbered
    std::copy(ix->h_start_ext.begin(), ix->h_start_ext.end(), padded.begin());
    (void)hipMemcpy(ix->d_start_ext, padded.data(), (size_t)need * 4, hipMemcpyHostToDevice);
    if (need > ix->r_start_ext_cap) {
      if (ix->r_start_ext) (void)hipFree(ix->r_start_ext);
      ix->r_start_ext = nullptr, ix->r_start_ext_cap = 0;
      if (hipMalloc(&ix->r_start_ext, (size_t)need * 2 * 4) == hipSuccess) ix->r_start_ext_cap = need * 2;
    }
    if (ix->r_start_ext) (void)hipMemcpy(ix->r_start_ext, padded.data(), (size_t)need * 4, hipMemcpyHostToDevice);
  }
  ix->view.n = nn, ix->view.adj = ix->r_adj, ix->view.ids = ix->r_ids, ix->view.start_ext = ix->r_start_ext;
  ix->view.start_ext_n = (uint32_t)ix->h_start_ext.size();
  ix->view.adj_codes = ix->r_adjcodes;
  ix->view_gen++;
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
      SDB_HIP(hipMemcpy(adj.data(), ix->d_adj, adj.size() * 4, hipMemcpyDeviceToHost));
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

namespace sdb {
int encode_bit_rows_public(sdb_index *ix, uint32_t first, uint32_t n, hipStream_t stream) {
  return encode_bit_rows(ix, first, n, stream);
}
int store_rows_public(sdb_index *ix, uint32_t first, uint32_t n, const float *dev_vectors, hipStream_t stream) {
  return store_rows(ix, first, n, dev_vectors, SDB_MEM_DEVICE, stream);
}
}  // namespace sdb

namespace sdb {
int unpermute_rows_public(const sdb_index *ix, uint32_t first, uint32_t n, float *dst, hipStream_t stream) {
  if (n == 0) return SDB_OK;
  const RowLayout &l = ix->lay;
  hipLaunchKernelGGL(k_unpermute_rows, dim3(n), dim3(128), 0, stream, ix->d_slab + (size_t)first * l.ld, dst, n, l.dim,
                     l.nblk, l.ng, l.ld);
  SDB_HIP(hipGetLastError());
  return SDB_OK;
}
}  // namespace sdb

// productQuantizer.Set -> encode for every stored vector (product.go:161-169), then searches use the
// LUT distance (product.go:250-277).
// The write path keeps two things per row from its last robustPrune: how many leading edges came out of it
// (d_clean: those do not dominate each other, build.hip) and the distances to them (d_dcount / d_adjdist).  Both
// are statements about the store's distance function.  When that changes -- the store switches to the quantizer's
// table distances, or centroid ids are overwritten -- they no longer hold and every row starts over.
static int forget_prune_state(sdb_index *ix) {
  if (ix->n == 0) return SDB_OK;
  SDB_HIP(hipMemset(ix->d_clean, 0, (size_t)ix->n * sizeof(uint32_t)));
  SDB_HIP(hipMemset(ix->d_dcount, 0, (size_t)ix->n * sizeof(uint32_t)));
  return SDB_OK;
}

extern "C" int sdb_index_attach_pq(sdb_index *ix, const sdb_pq *pq, void *stream_) try {
  if (!ix || !pq) return fail(SDB_ERR_INVALID, "NULL argument");
  if (!pq->fitted) return fail(SDB_ERR_STATE, "quantizer is not fitted");
  if (pq->dim != ix->lay.dim) return fail(SDB_ERR_INVALID, "quantizer dim %u != index dim %u", pq->dim, ix->lay.dim);
  if (pq->device != ix->P.device) return fail(SDB_ERR_INVALID, "quantizer and index live on different devices");
  {
    // the reference swaps cosine for euclidean inside the quantizer only (product.go:52-61); any other
    // mismatch between the index metric and the quantizer metric is a configuration error
    const int want = ix->P.metric == SDB_METRIC_COSINE ? SDB_METRIC_EUCLIDEAN : (int)ix->P.metric;
    if (pq->metric != want) return fail(SDB_ERR_INVALID, "quantizer metric does not match the index metric");
  }
  if (ix->bq) return fail(SDB_ERR_STATE, "a binary quantizer is attached");
  if (ix->in_tx) return fail(SDB_ERR_STATE, "a write transaction is open");
  DeviceGuard dg(ix->P.device);
  hipStream_t stream = as_stream(stream_);
  // The hosts run Fit after a commit while their batcher keeps searching.  The new code rows are encoded into a
  // buffer of their own while searches go on with what they have (full precision, or the previous quantizer's
  // codes); then (quantizer, codes) change hands together under the exclusive lock, once the walks that were
  // launched with the old pair have drained -- a search sees either pair whole, never the new tables over
  // half-written codes, never freed rows.
  uint8_t *ncodes = nullptr;
  SDB_HIP(hipMalloc(&ncodes, (size_t)ix->cap * pq->M));
  const uint32_t chunk = 1u << 18;
  float *tmp = nullptr;
  if (hipMalloc(&tmp, (size_t)std::min<uint32_t>(chunk, std::max<uint32_t>(ix->n, 1)) * ix->lay.dim * sizeof(float)) != hipSuccess) {
    (void)hipFree(ncodes);
    return fail(SDB_ERR_DEVICE, "out of device memory for the encode staging");
  }
  int rc = SDB_OK;
  for (uint32_t first = 0; first < ix->n && rc == SDB_OK; first += chunk) {
    const uint32_t m = std::min<uint32_t>(chunk, ix->n - first);
    rc = unpermute_rows_public(ix, first, m, tmp, stream);
    if (rc == SDB_OK) rc = pq_encode_device(pq, tmp, m, ncodes + (size_t)first * pq->M, stream);
  }
  (void)hipStreamSynchronize(stream);
  (void)hipFree(tmp);
  if (rc != SDB_OK) {
    (void)hipFree(ncodes);
    return rc;
  }
  std::unique_lock<sdb::ViewMutex> wl(ix->view_mu);
  (void)hipDeviceSynchronize();  // walks launched with the old (quantizer, codes) pair
  if (ix->d_codes) (void)hipFree(ix->d_codes);
  ix->d_codes = ncodes;
  ix->pq = pq;
  ix->code_bytes = pq->M;
  ix->drop_sketch();  // a quantized walk has no use for the float16 copy (sketch_supported)
  // the neighbours' code rows behind the adjacency rows, for the new codes (M <= 32; index.h d_adjcodes)
  SDB_TRY(ix->alloc_adjcodes());
  SDB_TRY(ix->rebuild_adjcodes(stream));
  return forget_prune_state(ix);
}
SDB_API_CATCH("sdb_index_attach_pq")

// Centroid ids that do NOT come from encode(): the k-means labels productQuantizer.Fit leaves on its
// training points (product.go:216-218) and the codes a bucket persisted under 'q' (product.go:349-383).
extern "C" int sdb_index_set_codes(sdb_index *ix, uint64_t n, const uint64_t *ids, const uint8_t *codes) try {
  if (!ix) return fail(SDB_ERR_INVALID, "index is NULL");
  if (!ix->pq) return fail(SDB_ERR_STATE, "no quantizer attached");
  // (code rows exist once, not per graph version: rewritten inside a transaction they could not be rolled back with it)
  if (ix->in_tx) return fail(SDB_ERR_STATE, "a write transaction is open: centroid ids are set outside it");
  if (n == 0) return SDB_OK;
  if (!ids || !codes) return fail(SDB_ERR_INVALID, "NULL argument");
  const uint32_t M = ix->pq->M;
  DeviceGuard dg(ix->P.device);
  for (uint64_t i = 0; i < n; i++)  // nothing is written unless every id resolves
    if (ix->slot_of(ids[i]) < 0) return fail(SDB_ERR_NOT_FOUND, "point %llu not found", (unsigned long long)ids[i]);
  // code rows are rewritten in place: searches stand aside (exclusive lock) and the walks in flight drain first
  std::unique_lock<sdb::ViewMutex> wl(ix->view_mu);
  SDB_HIP(hipDeviceSynchronize());
  // group runs of consecutive slots into one copy each (ids in storage order give one run)
  uint64_t i = 0;
  while (i < n) {
    const int64_t s0 = ix->slot_of(ids[i]);
    uint64_t j = i + 1;
    while (j < n && ix->slot_of(ids[j]) == s0 + (int64_t)(j - i)) j++;
    SDB_HIP(hipMemcpy(ix->d_codes + (size_t)s0 * M, codes + i * M, (j - i) * M, hipMemcpyHostToDevice));
    i = j;
  }
  SDB_TRY(ix->rebuild_adjcodes(nullptr));  // every node that has one of these as a neighbour carries a copy of its code row
  return forget_prune_state(ix);
}
SDB_API_CATCH("sdb_index_set_codes")

extern "C" int sdb_index_get_codes(const sdb_index *ix, uint64_t n, const uint64_t *ids, uint8_t *codes) try {
  if (!ix) return fail(SDB_ERR_INVALID, "index is NULL");
  if (!ix->pq) return fail(SDB_ERR_STATE, "no quantizer attached");
  if (n == 0) return SDB_OK;
  if (!ids || !codes) return fail(SDB_ERR_INVALID, "NULL argument");
  const uint32_t M = ix->pq->M;
  DeviceGuard dg(ix->P.device);
  uint64_t i = 0;
  while (i < n) {
    const int64_t s0 = ix->slot_of(ids[i]);
    if (s0 < 0) return fail(SDB_ERR_NOT_FOUND, "point %llu not found", (unsigned long long)ids[i]);
    uint64_t j = i + 1;
    while (j < n && ix->slot_of(ids[j]) == s0 + (int64_t)(j - i)) j++;
    SDB_HIP(hipMemcpy(codes + i * M, ix->d_codes + (size_t)s0 * M, (j - i) * M, hipMemcpyDeviceToHost));
    i = j;
  }
  return SDB_OK;
}
SDB_API_CATCH("sdb_index_get_codes")

// binaryQuantizer with a threshold (binary.go:131-139, 187-234): every stored point's BinaryVector in HBM, searches on
// bitDistFn(encode(query), code), prunes on bitDistFn(code, code).  Without a threshold the quantizer is fitted first
// (Fit, :145-185) from the index's own rows.
extern "C" int sdb_index_attach_bq(sdb_index *ix, sdb_bq *bq, void *stream_) try {
  if (!ix || !bq) return fail(SDB_ERR_INVALID, "NULL argument");
  if (bq->dim != ix->lay.dim) return fail(SDB_ERR_INVALID, "quantizer dim %u != index dim %u", bq->dim, ix->lay.dim);
  if (bq->device != ix->P.device) return fail(SDB_ERR_INVALID, "quantizer and index live on different devices");
  if (ix->broken) return fail(SDB_ERR_STATE, "index is unusable after a failed write; reload it from the bucket");
  if (ix->pq) return fail(SDB_ERR_STATE, "a product quantizer is attached");
  if (ix->bq) return fail(SDB_ERR_STATE, "a binary quantizer is attached");
  if (ix->in_tx) return fail(SDB_ERR_STATE, "a write transaction is open");
  if (!bq->has_thr && ix->n == ix->n_dead) return fail(SDB_ERR_STATE, "quantizer has no threshold and the index no rows to fit it from");
  DeviceGuard dg(ix->P.device);
  hipStream_t stream = as_stream(stream_);
  // like attach_pq: the code rows are written into a buffer of their own while searches go on in full precision, then
  // (quantizer, codes) change hands under the exclusive lock
  const bool fitted_here = !bq->has_thr;
  if (fitted_here) {  // Fit's first pass over the items in storage order, tombstones skipped (outside a transaction the writer's ids are the committed ones)
    SDB_TRY(bq_fit_slab(ix->lay, ix->d_slab, ix->d_ids, ix->n, bq->d_thr, stream));
    SDB_HIP(hipStreamSynchronize(stream));
    bq->has_thr = true;
  }
  uint64_t *ncodes = nullptr;
  hipError_t me = hipMalloc(&ncodes, (size_t)ix->cap * bq->W * 8);
  int rc = me == hipSuccess ? bq_encode_slab(bq->d_thr, ix->lay, ix->d_slab, 0, ix->n, ncodes, stream)  // Fit's second pass / Set
                            : fail(SDB_ERR_DEVICE, "hipMalloc failed: %s", hipGetErrorString(me));
  (void)hipStreamSynchronize(stream);
  if (rc != SDB_OK) {  // nothing changes hands: a quantizer fitted by this call is unfitted again
    if (ncodes) (void)hipFree(ncodes);
    if (fitted_here) bq->has_thr = false;
    return rc;
  }
  std::unique_lock<sdb::ViewMutex> wl(ix->view_mu);
  (void)hipDeviceSynchronize();  // walks launched on the float rows
  ix->d_codes = reinterpret_cast<uint8_t *>(ncodes);
  ix->bq = bq;
  bq->attached = true;
  ix->code_bytes = bq->W * 8;
  ix->drop_sketch();  // a bit-code walk has no use for the float16 copy (sketch_supported)
  return forget_prune_state(ix);
}
SDB_API_CATCH("sdb_index_attach_bq")

// What a bucket holds under NodeKey(id, 'q') for a binary store (binaryQuantizedPoint.ReadFrom / WriteTo,
// binary.go:275-310): ids [n], codes [n][W] u64, host memory.  The rules of sdb_index_set_codes.
extern "C" int sdb_index_set_bit_codes(sdb_index *ix, uint64_t n, const uint64_t *ids, const uint64_t *codes) try {
  if (!ix) return fail(SDB_ERR_INVALID, "index is NULL");
  if (!ix->bq) return fail(SDB_ERR_STATE, "no binary quantizer attached");
  if (ix->in_tx) return fail(SDB_ERR_STATE, "a write transaction is open: codes are set outside it");
  if (n == 0) return SDB_OK;
  if (!ids || !codes) return fail(SDB_ERR_INVALID, "NULL argument");
  const size_t B = ix->code_bytes;
  DeviceGuard dg(ix->P.device);
  for (uint64_t i = 0; i < n; i++)  // nothing is written unless every id resolves
    if (ix->slot_of(ids[i]) < 0) return fail(SDB_ERR_NOT_FOUND, "point %llu not found", (unsigned long long)ids[i]);
  std::unique_lock<sdb::ViewMutex> wl(ix->view_mu);
  SDB_HIP(hipDeviceSynchronize());
  uint64_t i = 0;
  while (i < n) {
    const int64_t s0 = ix->slot_of(ids[i]);
    uint64_t j = i + 1;
    while (j < n && ix->slot_of(ids[j]) == s0 + (int64_t)(j - i)) j++;
    SDB_HIP(hipMemcpy(ix->d_codes + (size_t)s0 * B, reinterpret_cast<const uint8_t *>(codes) + i * B, (j - i) * B, hipMemcpyHostToDevice));
    i = j;
  }
  return forget_prune_state(ix);
}
SDB_API_CATCH("sdb_index_set_bit_codes")

extern "C" int sdb_index_get_bit_codes(const sdb_index *ix, uint64_t n, const uint64_t *ids, uint64_t *codes) try {
  if (!ix) return fail(SDB_ERR_INVALID, "index is NULL");
  if (!ix->bq) return fail(SDB_ERR_STATE, "no binary quantizer attached");
  if (n == 0) return SDB_OK;
  if (!ids || !codes) return fail(SDB_ERR_INVALID, "NULL argument");
  const size_t B = ix->code_bytes;
  DeviceGuard dg(ix->P.device);
  uint64_t i = 0;
  while (i < n) {
    const int64_t s0 = ix->slot_of(ids[i]);
    if (s0 < 0) return fail(SDB_ERR_NOT_FOUND, "point %llu not found", (unsigned long long)ids[i]);
    uint64_t j = i + 1;
    while (j < n && ix->slot_of(ids[j]) == s0 + (int64_t)(j - i)) j++;
    SDB_HIP(hipMemcpy(reinterpret_cast<uint8_t *>(codes) + i * B, ix->d_codes + (size_t)s0 * B, (j - i) * B, hipMemcpyDeviceToHost));
    i = j;
  }
  return SDB_OK;
}
SDB_API_CATCH("sdb_index_get_bit_codes")
