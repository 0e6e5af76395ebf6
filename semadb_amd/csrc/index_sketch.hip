// index_sketch.hip -- the float16 / int8 copy of the slab that the two-precision hop reads first (index.h SDB_TUNE_SKETCH):
// the conversion kernels, when a table takes which copy, and how the copy follows the rows.
#include <algorithm>
#include <cmath>

#include "index.h"
#include "walk_args.h"
#include "wave_dist.h"

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

using namespace sdb;

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

extern "C" int sdb_index_sketch_stats(sdb_index *ix, uint64_t out[3]) try {
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
