// index_codes.hip -- the code rows of a quantized store: attaching a quantizer, reading and writing code rows by id, and
// the neighbours' code rows behind the adjacency rows (index.h GraphCopy::adjcodes).
#include <algorithm>

#include "bq.h"
#include "pq.h"

namespace sdb {
// The neighbours' code rows behind the adjacency rows (index.h GraphCopy::adjcodes): out[row][e] = codes[adj[row][e]],
// zeros behind the edges.  dirty != NULL: only the rows a transaction wrote or appended (first_new: rows at its start).
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
}  // namespace sdb

using namespace sdb;

int sdb_index::fill_adjcodes(const GraphCopy &g, uint32_t rows, const uint8_t *dirty, uint32_t from, hipStream_t stream,
                             const uint8_t *codes) {
  if (!rows) return SDB_OK;
  hipLaunchKernelGGL(sdb::k_adjcodes_rows, dim3((rows + 3) / 4), dim3(256), 0, stream, g.adj, codes ? codes : d_codes, g.adjcodes,
                     dirty, rows, from, pq->M);
  SDB_HIP(hipGetLastError());
  return SDB_OK;
}

int sdb_index::alloc_adjcodes() {
  if (wr.adjcodes) (void)hipFree(wr.adjcodes);
  if (cm.adjcodes) (void)hipFree(cm.adjcodes);
  wr.adjcodes = cm.adjcodes = nullptr;
  view.adj_codes = nullptr;
  if (!pq || pq->M > kAdjCodesMaxM) return SDB_OK;
  // a cache of what the code rows hold: without room for it the walk gathers by slot, as it does for larger M
  (void)FreshBufs::pair_if_room((void **)&wr.adjcodes, (void **)&cm.adjcodes, (size_t)cap * kAdjStride * pq->M);
  return SDB_OK;
}

int sdb_index::rebuild_adjcodes(hipStream_t stream) {
  if (!has_adjcodes()) return SDB_OK;
  SDB_TRY(fill_adjcodes(wr, n, nullptr, 0, stream));
  SDB_TRY(fill_adjcodes(cm, view.n, nullptr, 0, stream));
  SDB_HIP(hipStreamSynchronize(stream));
  view.adj_codes = cm.adjcodes;
  return SDB_OK;
}

// The write path keeps two things per row from its last robustPrune: how many leading edges came out of it
// (d_clean: those do not dominate each other, build.hip) and the distances to them (d_dcount / d_adjdist).  Both
// are statements about the store's distance function.  When that changes -- the store switches to the quantizer's
// table distances, or centroid ids are overwritten -- they no longer hold and every row starts over.
int sdb_index::forget_prune_state() {
  if (n == 0) return SDB_OK;
  SDB_HIP(hipMemset(d_clean, 0, (size_t)n * sizeof(uint32_t)));
  SDB_HIP(hipMemset(d_dcount, 0, (size_t)n * sizeof(uint32_t)));
  return SDB_OK;
}

// Code rows by id, between d_codes and `host` ([n][code_bytes]), in direction `dir`: ids resolve to slots, and runs of
// consecutive slots go as one copy each (ids in storage order give one run).  An id that does not resolve ends the call
// with SDB_ERR_NOT_FOUND: with copy == false nothing is copied at all -- the pass a setter makes first, so that nothing
// is written unless every id resolves.
static int code_rows_by_id(const sdb_index *ix, uint64_t n, const uint64_t *ids, const void *host, hipMemcpyKind dir, bool copy = true) {
  const size_t B = ix->code_bytes;
  uint64_t j;
  for (uint64_t i = 0; i < n; i = j) {
    const int64_t s0 = ix->slot_of(ids[i]);
    if (s0 < 0) return fail(SDB_ERR_NOT_FOUND, "point %llu not found", (unsigned long long)ids[i]);
    for (j = i + 1; j < n && ix->slot_of(ids[j]) == s0 + (int64_t)(j - i);) j++;
    if (!copy) continue;
    uint8_t *dev = ix->d_codes + (size_t)s0 * B, *h = static_cast<uint8_t *>(const_cast<void *>(host)) + i * B;
    SDB_HIP(dir == hipMemcpyHostToDevice ? hipMemcpy(dev, h, (j - i) * B, dir) : hipMemcpy(h, dev, (j - i) * B, dir));
  }
  return SDB_OK;
}

extern "C" {

// productQuantizer.Set -> encode for every stored vector (product.go:161-169), then searches use the
// LUT distance (product.go:250-277).
int sdb_index_attach_pq(sdb_index *ix, const sdb_pq *pq, void *stream_) try {
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
    rc = unpermute_rows(ix, first, m, tmp, stream);
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
  // the neighbours' code rows behind the adjacency rows, for the new codes (M <= 32; index.h GraphCopy::adjcodes)
  SDB_TRY(ix->alloc_adjcodes());
  SDB_TRY(ix->rebuild_adjcodes(stream));
  return ix->forget_prune_state();
}
SDB_API_CATCH("sdb_index_attach_pq")

// Centroid ids that do NOT come from encode(): the k-means labels productQuantizer.Fit leaves on its
// training points (product.go:216-218) and the codes a bucket persisted under 'q' (product.go:349-383).
int sdb_index_set_codes(sdb_index *ix, uint64_t n, const uint64_t *ids, const uint8_t *codes) try {
  if (!ix) return fail(SDB_ERR_INVALID, "index is NULL");
  if (!ix->pq) return fail(SDB_ERR_STATE, "no quantizer attached");
  // (code rows exist once, not per graph version: rewritten inside a transaction they could not be rolled back with it)
  if (ix->in_tx) return fail(SDB_ERR_STATE, "a write transaction is open: centroid ids are set outside it");
  if (n == 0) return SDB_OK;
  if (!ids || !codes) return fail(SDB_ERR_INVALID, "NULL argument");
  DeviceGuard dg(ix->P.device);
  SDB_TRY(code_rows_by_id(ix, n, ids, codes, hipMemcpyHostToDevice, false));  // nothing is written unless every id resolves
  // code rows are rewritten in place: searches stand aside (exclusive lock) and the walks in flight drain first
  std::unique_lock<sdb::ViewMutex> wl(ix->view_mu);
  SDB_HIP(hipDeviceSynchronize());
  SDB_TRY(code_rows_by_id(ix, n, ids, codes, hipMemcpyHostToDevice));
  SDB_TRY(ix->rebuild_adjcodes(nullptr));  // every node that has one of these as a neighbour carries a copy of its code row
  return ix->forget_prune_state();
}
SDB_API_CATCH("sdb_index_set_codes")

int sdb_index_get_codes(const sdb_index *ix, uint64_t n, const uint64_t *ids, uint8_t *codes) try {
  if (!ix) return fail(SDB_ERR_INVALID, "index is NULL");
  if (!ix->pq) return fail(SDB_ERR_STATE, "no quantizer attached");
  if (n == 0) return SDB_OK;
  if (!ids || !codes) return fail(SDB_ERR_INVALID, "NULL argument");
  DeviceGuard dg(ix->P.device);
  return code_rows_by_id(ix, n, ids, codes, hipMemcpyDeviceToHost);
}
SDB_API_CATCH("sdb_index_get_codes")

// binaryQuantizer with a threshold (binary.go:131-139, 187-234): every stored point's BinaryVector in HBM, searches on
// bitDistFn(encode(query), code), prunes on bitDistFn(code, code).  Without a threshold the quantizer is fitted first
// (Fit, :145-185) from the index's own rows.
int sdb_index_attach_bq(sdb_index *ix, sdb_bq *bq, void *stream_) try {
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
    SDB_TRY(bq_fit_slab(ix->lay, ix->d_slab, ix->wr.ids, ix->n, bq->d_thr, stream));
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
  return ix->forget_prune_state();
}
SDB_API_CATCH("sdb_index_attach_bq")

// What a bucket holds under NodeKey(id, 'q') for a binary store (binaryQuantizedPoint.ReadFrom / WriteTo,
// binary.go:275-310): ids [n], codes [n][W] u64, host memory.  The rules of sdb_index_set_codes.
int sdb_index_set_bit_codes(sdb_index *ix, uint64_t n, const uint64_t *ids, const uint64_t *codes) try {
  if (!ix) return fail(SDB_ERR_INVALID, "index is NULL");
  if (!ix->bq) return fail(SDB_ERR_STATE, "no binary quantizer attached");
  if (ix->in_tx) return fail(SDB_ERR_STATE, "a write transaction is open: codes are set outside it");
  if (n == 0) return SDB_OK;
  if (!ids || !codes) return fail(SDB_ERR_INVALID, "NULL argument");
  DeviceGuard dg(ix->P.device);
  SDB_TRY(code_rows_by_id(ix, n, ids, codes, hipMemcpyHostToDevice, false));  // nothing is written unless every id resolves
  // code rows are rewritten in place: searches stand aside (exclusive lock) and the walks in flight drain first
  std::unique_lock<sdb::ViewMutex> wl(ix->view_mu);
  SDB_HIP(hipDeviceSynchronize());
  SDB_TRY(code_rows_by_id(ix, n, ids, codes, hipMemcpyHostToDevice));
  return ix->forget_prune_state();
}
SDB_API_CATCH("sdb_index_set_bit_codes")

int sdb_index_get_bit_codes(const sdb_index *ix, uint64_t n, const uint64_t *ids, uint64_t *codes) try {
  if (!ix) return fail(SDB_ERR_INVALID, "index is NULL");
  if (!ix->bq) return fail(SDB_ERR_STATE, "no binary quantizer attached");
  if (n == 0) return SDB_OK;
  if (!ids || !codes) return fail(SDB_ERR_INVALID, "NULL argument");
  DeviceGuard dg(ix->P.device);
  return code_rows_by_id(ix, n, ids, codes, hipMemcpyDeviceToHost);
}
SDB_API_CATCH("sdb_index_get_bit_codes")

}  // extern "C"
