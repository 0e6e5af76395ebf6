// bq.h -- binary quantizer state (internal; the public surface is include/semadb_amd.h).
#pragma once
#include "common.h"

// binaryQuantizer (shard/vectorstore/binary.go:25-34) with its threshold pinned in HBM
struct sdb_bq {
  uint32_t dim = 0, W = 0;  // W = ceil(dim / 64) words per code (binary.go:107-111)
  int metric = 0;           // SDB_METRIC_HAMMING / SDB_METRIC_JACCARD (distance.go:85-94)
  int device = 0;
  float *d_thr = nullptr;  // [dim]
  bool has_thr = false;    // the reference's `threshold != nil`
  bool attached = false;   // an index holds codes cut at this threshold: it stays as it is (sdb_bq_set_threshold)
};

struct sdb_index;

namespace sdb {
// hammingDistance / jaccardDistance (distance.go:45-67) of two codes of W words -- the one home of the counts, of the
// jaccard rounding (one float32 division, one subtraction) and of the empty-union rule.  Hamming: s = |x ^ y|;
// jaccard: s = |x & y|, u = |x | y|.  VEC2: W is even and y sits on a 16-byte boundary, two words per load.
template <bool JACCARD, bool VEC2 = false, class XP>  // XP: pointer to the query's words, in any address space
__device__ __forceinline__ float bit_pair_dist(XP x, const uint64_t *__restrict__ y, uint32_t W) {
  typedef unsigned long long word2 __attribute__((ext_vector_type(2)));
  uint32_t s = 0, u = 0;
  if constexpr (VEC2) {
    const word2 *__restrict__ y2 = reinterpret_cast<const word2 *>(y);
    for (uint32_t k = 0; k < W; k += 2) {
      const word2 yy = y2[k >> 1];
      const uint64_t x0 = x[k], x1 = x[k + 1];
      if constexpr (JACCARD) {
        s += __popcll(x0 & yy.x) + __popcll(x1 & yy.y);
        u += __popcll(x0 | yy.x) + __popcll(x1 | yy.y);
      } else {
        s += __popcll(x0 ^ yy.x) + __popcll(x1 ^ yy.y);
      }
    }
  } else {
    for (uint32_t k = 0; k < W; k++) {
      const uint64_t xx = x[k], yy = y[k];
      if constexpr (JACCARD) s += __popcll(xx & yy), u += __popcll(xx | yy);
      else s += __popcll(xx ^ yy);
    }
  }
  if constexpr (JACCARD) {
    if (u == 0) return 0.0f;            // distance.go:63-65
    return 1.0f - (float)s / (float)u;  // :66
  } else {
    return (float)s;  // :53
  }
}

// thr[c] = (sum of X[r][c] over r = 0..n-1, one float32 add per row in that order) / float32(n)  (binary.go:152-173)
int bq_fit_device(const float *d_X, uint64_t n, uint32_t dim, float *d_thr, hipStream_t stream);
// codes[v][i / 64] bit i % 64 = vecs[v][i] > thr[i]  (binary.go:103-129); device buffers
int bq_encode_device(const float *d_thr, uint32_t dim, const float *d_vecs, uint64_t n, uint64_t *d_codes, hipStream_t stream);
// the same two over rows of an index slab (common.h RowLayout): Fit over the n rows in storage order, tombstones (id 0 in
// d_ids) skipped, divided by the number of live rows; encode of slab rows [first, first + n) into d_codes[first ..]
int bq_fit_slab(const RowLayout &l, const float *d_slab, const uint64_t *d_ids, uint32_t n, float *d_thr, hipStream_t stream);
int bq_encode_slab(const float *d_thr, const RowLayout &l, const float *d_slab, uint32_t first, uint32_t n, uint64_t *d_codes,
                   hipStream_t stream);
}  // namespace sdb
