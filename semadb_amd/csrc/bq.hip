// bq.hip -- the binary quantizer of shard/vectorstore/binary.go as an object of the C ABI: the threshold (given,
// read back from a bucket, or fitted as the column means), encode, and the two bit distances of distance/distance.go.
//
//   * Fit's first pass (binary.go:152-173) adds the rows to ONE float32 sum per column, row after row, and divides
//     once.  Float addition does not associate, so the kernel keeps that order: one lane per column walks the rows in
//     the order given (eight loads in flight, the adds in row order) -- never a tree.
//   * encode (binary.go:103-129): one wave per row; lane l of step w compares element 64 w + l with its threshold and
//     the wave's ballot IS word w.  `>` is false for a NaN on either side, lanes past the row's end vote 0.
//   * hammingDistance / jaccardDistance (distance.go:45-67): integer population counts, converted to float32 once
//     (hamming) or divided once as float32 (jaccard); one lane per candidate, the query words at wave-uniform
//     addresses.
#include "bq.h"

namespace sdb {

// Where the rows come from: caller rows [n][dim], or the index slab's permuted rows (common.h RowLayout), whose
// element i sits at (i / 128) * 128 + (i % 32) * 4 + (i / 32) % 4 of a row of `stride` floats (the tail block after the groups).
struct BqRows {
  const float *base;
  uint32_t stride;    // floats from one row to the next
  uint32_t nblk, ng;  // slab layout; unused for caller rows
  uint32_t permuted;
  const uint64_t *ids;  // fit over the slab: rows with id 0 are tombstones and are skipped; NULL: every row counts
};
__device__ __forceinline__ uint32_t bq_elem(const BqRows &r, uint32_t i) {
  if (!r.permuted) return i;
  const uint32_t b = i / 32, L = i % 32;
  return b < r.nblk ? (b / 4) * 128 + L * 4 + (b % 4) : r.ng * 128 + L;
}

__global__ __launch_bounds__(64) void k_bq_fit(const BqRows rows, uint64_t n, uint32_t dim, float *__restrict__ thr) {
  const uint32_t c = blockIdx.x * 64 + threadIdx.x;
  if (c >= dim) return;
  const float *p = rows.base + bq_elem(rows, c);
  const uint64_t *ids = rows.ids;
  float acc = 0.0f;
  uint64_t count = 0, r = 0;
  for (; r + 8 <= n; r += 8) {
    float v[8];
    bool live[8];
#pragma unroll
    for (int u = 0; u < 8; u++) v[u] = p[(r + u) * rows.stride], live[u] = !ids || ids[r + u] != 0;
#pragma unroll
    for (int u = 0; u < 8; u++)
      if (live[u]) acc += v[u], count++;  // sum[i] += v, binary.go:161-163
  }
  for (; r < n; r++)
    if (!ids || ids[r] != 0) acc += p[r * rows.stride], count++;
  thr[c] = acc / (float)count;  // sum[i] /= float32(count), :170-172
}

constexpr uint32_t kEncWaves = 4;  // rows per workgroup

__global__ __launch_bounds__(64 * kEncWaves) void k_bq_encode(const float *__restrict__ thr, uint32_t dim, uint32_t W,
                                                              const BqRows rows, uint64_t n, uint64_t *__restrict__ codes) {
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (uint64_t row = (uint64_t)blockIdx.x * kEncWaves + wave; row < n; row += (uint64_t)gridDim.x * kEncWaves) {
    const float *v = rows.base + row * rows.stride;
    uint64_t mine = 0;  // lane w keeps word w (W <= 64)
    for (uint32_t w = 0; w < W; w++) {
      const uint32_t i = w * 64 + lane;
      const bool bit = i < dim && v[bq_elem(rows, i)] > thr[i];  // strict, binary.go:124
      const uint64_t word = __ballot(bit);
      if (lane == w) mine = word;
    }
    if (lane < W) codes[row * W + lane] = mine;
  }
}

// out[q * nc + c]; VEC: rows of an even number of words on 16-byte boundaries, read two words per load
template <bool JACCARD, bool VEC>
__global__ __launch_bounds__(256) void k_bit_distance(const uint64_t *__restrict__ qcodes, const uint64_t *__restrict__ ccodes,
                                                      uint64_t nc, uint32_t W, float *__restrict__ out) {
  const uint64_t c = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  const uint64_t q = blockIdx.y;
  if (c >= nc) return;
  out[q * nc + c] = bit_pair_dist<JACCARD, VEC>(qcodes + q * W, ccodes + c * W, W);
}

int bq_fit_device(const float *d_X, uint64_t n, uint32_t dim, float *d_thr, hipStream_t stream) {
  const BqRows rows{d_X, dim, 0, 0, 0, nullptr};
  hipLaunchKernelGGL(k_bq_fit, dim3((dim + 63) / 64), dim3(64), 0, stream, rows, n, dim, d_thr);
  SDB_HIP(hipGetLastError());
  return SDB_OK;
}

int bq_fit_slab(const RowLayout &l, const float *d_slab, const uint64_t *d_ids, uint32_t n, float *d_thr, hipStream_t stream) {
  const BqRows rows{d_slab, l.ld, l.nblk, l.ng, 1, d_ids};
  hipLaunchKernelGGL(k_bq_fit, dim3((l.dim + 63) / 64), dim3(64), 0, stream, rows, (uint64_t)n, l.dim, d_thr);
  SDB_HIP(hipGetLastError());
  return SDB_OK;
}

static int launch_encode(const float *d_thr, uint32_t dim, const BqRows &rows, uint64_t n, uint64_t *d_codes, hipStream_t stream) {
  if (n == 0) return SDB_OK;
  const uint64_t blocks = (n + kEncWaves - 1) / kEncWaves;
  const unsigned grid = (unsigned)(blocks < (1u << 20) ? blocks : (1u << 20));  // the kernel strides over the rest
  hipLaunchKernelGGL(k_bq_encode, dim3(grid), dim3(64 * kEncWaves), 0, stream, d_thr, dim, (dim + 63) / 64, rows, n, d_codes);
  SDB_HIP(hipGetLastError());
  return SDB_OK;
}

int bq_encode_device(const float *d_thr, uint32_t dim, const float *d_vecs, uint64_t n, uint64_t *d_codes,
                     hipStream_t stream) {
  return launch_encode(d_thr, dim, BqRows{d_vecs, dim, 0, 0, 0, nullptr}, n, d_codes, stream);
}

int bq_encode_slab(const float *d_thr, const RowLayout &l, const float *d_slab, uint32_t first, uint32_t n, uint64_t *d_codes,
                   hipStream_t stream) {
  const uint32_t W = (l.dim + 63) / 64;
  return launch_encode(d_thr, l.dim, BqRows{d_slab + (size_t)first * l.ld, l.ld, l.nblk, l.ng, 1, nullptr}, n,
                       d_codes + (size_t)first * W, stream);
}

static bool is_bit_metric(int m) { return m == SDB_METRIC_HAMMING || m == SDB_METRIC_JACCARD; }

}  // namespace sdb

using namespace sdb;

extern "C" {

int sdb_bq_create(uint32_t dim, uint32_t bit_metric, int device, sdb_bq **out) try {
  if (!out) return fail(SDB_ERR_INVALID, "NULL argument");
  *out = nullptr;
  if (dim < 1 || dim > 4096) return fail(SDB_ERR_INVALID, "vector size must be between 1 and 4096, got %u", dim);
  if (!is_bit_metric((int)bit_metric))  // distance.go:91-93
    return fail(SDB_ERR_INVALID, "unknown bit distance function: %u", bit_metric);
  int ndev = 0;
  SDB_TRY(sdb_device_count(&ndev));
  if (device < 0 || device >= ndev) return fail(SDB_ERR_INVALID, "device %d out of range", device);
  DeviceGuard dg(device);
  auto *bq = new sdb_bq();
  bq->dim = dim, bq->W = (dim + 63) / 64, bq->metric = (int)bit_metric, bq->device = device;
  hipError_t e = hipMalloc(&bq->d_thr, (size_t)dim * 4);
  if (e != hipSuccess) {
    delete bq;
    return fail(SDB_ERR_DEVICE, "hipMalloc failed: %s", hipGetErrorString(e));
  }
  *out = bq;
  return SDB_OK;
}
SDB_API_CATCH("sdb_bq_create")

int sdb_bq_destroy(sdb_bq *bq) try {
  if (!bq) return SDB_OK;
  DeviceGuard dg(bq->device);
  (void)hipDeviceSynchronize();
  if (bq->d_thr) (void)hipFree(bq->d_thr);
  delete bq;
  return SDB_OK;
}
SDB_API_CATCH("sdb_bq_destroy")

int sdb_bq_set_threshold(sdb_bq *bq, const float *thr, int mem) try {
  if (!bq || !thr) return fail(SDB_ERR_INVALID, "NULL argument");
  if (bq->attached)  // stored codes and query codes would be cut at different thresholds
    return fail(SDB_ERR_STATE, "the quantizer is attached to an index: its threshold stays as it is");
  DeviceGuard dg(bq->device);
  SDB_HIP(hipMemcpy(bq->d_thr, thr, (size_t)bq->dim * 4, mem == SDB_MEM_HOST ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice));
  SDB_HIP(hipDeviceSynchronize());
  bq->has_thr = true;
  return SDB_OK;
}
SDB_API_CATCH("sdb_bq_set_threshold")

int sdb_bq_get_threshold(const sdb_bq *bq, float *thr, int *is_set) try {
  if (!bq || !is_set) return fail(SDB_ERR_INVALID, "NULL argument");
  *is_set = bq->has_thr ? 1 : 0;
  if (!bq->has_thr || !thr) return SDB_OK;
  DeviceGuard dg(bq->device);
  SDB_HIP(hipDeviceSynchronize());
  SDB_HIP(hipMemcpy(thr, bq->d_thr, (size_t)bq->dim * 4, hipMemcpyDeviceToHost));
  return SDB_OK;
}
SDB_API_CATCH("sdb_bq_get_threshold")

int sdb_bq_fit(sdb_bq *bq, const float *X, uint64_t n, int mem, void *stream_) try {
  if (!bq || !X) return fail(SDB_ERR_INVALID, "NULL argument");
  if (bq->has_thr) return SDB_OK;  // binary.go:148: a quantizer that has its threshold is not fitted again
  if (n == 0) return fail(SDB_ERR_INVALID, "no vectors to fit");
  DeviceGuard dg(bq->device);
  hipStream_t stream = as_stream(stream_);
  Staged sx;
  SDB_TRY(stage_in(sx, X, (size_t)n * bq->dim * 4, mem, stream));
  int rc = bq_fit_device((const float *)sx.dev, n, bq->dim, bq->d_thr, stream);
  if (mem == SDB_MEM_HOST) {  // the staging copy is freed on return
    hipError_t e = hipStreamSynchronize(stream);
    if (rc == SDB_OK && e != hipSuccess) rc = fail(SDB_ERR_DEVICE, "bq_fit failed: %s", hipGetErrorString(e));
  }
  if (rc == SDB_OK) bq->has_thr = true;
  return rc;
}
SDB_API_CATCH("sdb_bq_fit")

int sdb_bq_encode(const sdb_bq *bq, const float *vectors, uint64_t n, uint64_t *codes, int mem, void *stream_) try {
  if (!bq || !vectors || !codes) return fail(SDB_ERR_INVALID, "NULL argument");
  if (!bq->has_thr) return fail(SDB_ERR_STATE, "quantizer has no threshold");  // encode returns nil, binary.go:104-106
  if (n == 0) return SDB_OK;
  DeviceGuard dg(bq->device);
  hipStream_t stream = as_stream(stream_);
  Staged sv, sc;
  SDB_TRY(stage_in(sv, vectors, n * bq->dim * 4, mem, stream));
  SDB_TRY(stage_in(sc, codes, n * bq->W * 8, mem, stream, false));
  int rc = bq_encode_device(bq->d_thr, bq->dim, (const float *)sv.dev, n, (uint64_t *)sc.dev, stream);
  if (rc == SDB_OK) rc = stage_out(sc, stream);
  if (mem == SDB_MEM_HOST) {
    hipError_t e = hipStreamSynchronize(stream);
    if (rc == SDB_OK && e != hipSuccess) rc = fail(SDB_ERR_DEVICE, "bq_encode failed: %s", hipGetErrorString(e));
  }
  return rc;
}
SDB_API_CATCH("sdb_bq_encode")

int sdb_bit_distance_batch(int bit_metric, uint32_t W, const uint64_t *qcodes, uint64_t nq, const uint64_t *ccodes,
                           uint64_t nc, float *out, int mem, int device, void *stream_) try {
  if (!is_bit_metric(bit_metric)) return fail(SDB_ERR_INVALID, "unknown bit distance function: %d", bit_metric);
  if (W < 1 || W > 64) return fail(SDB_ERR_INVALID, "codes have 1 to 64 words, got %u", W);
  if (nq == 0 || nc == 0) return SDB_OK;
  if (!qcodes || !ccodes || !out) return fail(SDB_ERR_INVALID, "NULL argument");
  if (nq > 65535) return fail(SDB_ERR_INVALID, "at most 65535 queries per call, got %llu", (unsigned long long)nq);
  int ndev = 0;
  SDB_TRY(sdb_device_count(&ndev));
  if (device < 0 || device >= ndev) return fail(SDB_ERR_INVALID, "device %d out of range", device);
  DeviceGuard dg(device);
  hipStream_t stream = as_stream(stream_);
  Staged sq, sc, so;
  SDB_TRY(stage_in(sq, qcodes, nq * W * 8, mem, stream));
  SDB_TRY(stage_in(sc, ccodes, nc * W * 8, mem, stream));
  SDB_TRY(stage_in(so, out, nq * nc * 4, mem, stream, false));
  const uint64_t *dq = (const uint64_t *)sq.dev, *dc = (const uint64_t *)sc.dev;
  float *dout = (float *)so.dev;
  const bool vec = W % 2 == 0 && (uintptr_t)dc % 16 == 0;
  const bool jac = bit_metric == SDB_METRIC_JACCARD;
  const dim3 grid((unsigned)((nc + 255) / 256), (unsigned)nq), block(256);
  if (jac && vec) hipLaunchKernelGGL((k_bit_distance<true, true>), grid, block, 0, stream, dq, dc, nc, W, dout);
  else if (jac) hipLaunchKernelGGL((k_bit_distance<true, false>), grid, block, 0, stream, dq, dc, nc, W, dout);
  else if (vec) hipLaunchKernelGGL((k_bit_distance<false, true>), grid, block, 0, stream, dq, dc, nc, W, dout);
  else hipLaunchKernelGGL((k_bit_distance<false, false>), grid, block, 0, stream, dq, dc, nc, W, dout);
  int rc = SDB_OK;
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) rc = fail(SDB_ERR_DEVICE, "bit_distance launch failed: %s", hipGetErrorString(e));
  if (rc == SDB_OK) rc = stage_out(so, stream);
  if (mem == SDB_MEM_HOST) {
    e = hipStreamSynchronize(stream);
    if (rc == SDB_OK && e != hipSuccess) rc = fail(SDB_ERR_DEVICE, "bit_distance failed: %s", hipGetErrorString(e));
  }
  return rc;
}
SDB_API_CATCH("sdb_bit_distance_batch")

}  // extern "C"
