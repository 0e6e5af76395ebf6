// rerank.hip -- the candidates of a walk over a quantized store, ordered by their stored float32 rows
// (semadb_amd.h sdb_index_search_batch_rerank; the reference does not re-rank: this is the library's own call).
//
// The walk ran with limit = rerank and left, per query, up to `rerank` ids in its own order (quantizer distances).
// One workgroup of four waves per query: the query tile goes to LDS in the slab's element order (as in
// distance.hip k_index_distance), the ids become slots (a subtraction, or a probe of the view's id -> slot table as
// search_batch.hip k_filter_resolve probes it), every wave takes chunks of 2 U candidates through chunk_dist_lds -- the
// reference's FMA chains, tail chain and reduce tree (dist_core.h), so the distances are plainStore.DistanceFromFloat's
// bit for bit --, the <= 512 exact distances meet in LDS, and every candidate counts the candidates whose key
// (isnan(e), e, walk position) is below its own: that count is its place.  IEEE compares: -0.0 and 0.0 tie, ties keep
// the walk's order, NaNs come last in the walk's order.  No atomics, no scratch.
#include <cfloat>

#include "index.h"
#include "wave_dist.h"

namespace sdb {

constexpr int kRerankThreads = 256;

template <bool L2, bool MAP>
__global__ __launch_bounds__(kRerankThreads) void k_rerank(const RerankArgs a) {
  constexpr int U = 4;
  extern __shared__ float qs[];                                // ng * 128 + 32 floats: the query tile
  float *e = qs + a.ng * 128 + 32;                             // [kRerankMax] exact distances
  uint32_t *s_slot = reinterpret_cast<uint32_t *>(e + kRerankMax);  // [kRerankMax]
  const uint32_t q = blockIdx.x;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, L = lane & 31;
  const float *qv = a.queries + (size_t)q * a.dim;
  for (uint32_t i = tid; i < a.ng * 128; i += kRerankThreads) {
    const uint32_t g = i / 128, r = i % 128;
    qs[i] = q_elem(qv, a.nblk, g, r % 4, (int)(r / 4));
  }
  if (tid < 32) qs[a.ng * 128 + tid] = (uint32_t)tid < a.tail ? qv[a.nblk * 32 + tid] : 0.0f;
  const uint32_t have = a.cand_cnt[q];
  const uint32_t cn = have < a.rerank ? have : a.rerank;
  const uint64_t *cid = a.cand_ids + (size_t)q * a.rerank;
  for (uint32_t j = tid; j < cn; j += kRerankThreads) {
    const uint64_t id = cid[j];
    uint32_t s = kNoSlot;
    if constexpr (MAP) {
      if (id != 0) {
        uint32_t h = idmap_hash(id) & a.mask;
        while (true) {  // (the table has at least twice as many cells as keys: an empty one ends every probe)
          const uint64_t k = a.keys[h];
          if (k == id) {
            s = a.vals[h];
            break;
          }
          if (k == 0) break;
          h = (h + 1) & a.mask;
        }
      }
    } else {
      if (id >= a.base_id && id - a.base_id < (uint64_t)a.view_n) s = (uint32_t)(id - a.base_id);
    }
    s_slot[j] = s < a.view_n ? s : kNoSlot;  // rows past the committed count do not exist yet
  }
  __syncthreads();
  const uint32_t nchunk = (cn + 2 * U - 1) / (2 * U);
  for (uint32_t c = wave; c < nchunk; c += kRerankThreads / 64) {
    uint32_t slot[U], at[U];
    bool known[U];
#pragma unroll
    for (int u = 0; u < U; u++) {
      at[u] = c * (2 * U) + 2 * u + (lane >> 5);
      const uint32_t s = at[u] < cn ? s_slot[at[u]] : kNoSlot;
      known[u] = s != kNoSlot;
      slot[u] = known[u] ? s : 0;
    }
    float res[U];
    chunk_dist_lds<L2, U>(a.slab, a.ld, a.ng, a.tail, qs, slot, res, lane);
#pragma unroll
    for (int u = 0; u < U; u++)
      if (L == 0 && at[u] < cn)  // a point the store does not know -> math.MaxFloat32 (plain.go:78-82)
        e[at[u]] = known[u] ? metric_finish(res[u], a.metric) : FLT_MAX;
  }
  __syncthreads();
  uint64_t *oi = a.out_ids + (size_t)q * a.limit;
  float *od = a.out_dists + (size_t)q * a.limit;
  for (uint32_t t = tid; t < cn; t += kRerankThreads) {
    const float et = e[t];
    const bool nt = et != et;
    uint32_t rank = 0;
    for (uint32_t u = 0; u < cn; u++) {
      const float eu = e[u];
      const bool nu = eu != eu;
      const bool below = nt ? (!nu || u < t) : (!nu && (eu < et || (eu == et && u < t)));
      rank += below ? 1u : 0u;
    }
    if (rank < a.limit) oi[rank] = cid[t], od[rank] = et;
  }
  for (uint32_t p = cn + tid; p < a.limit; p += kRerankThreads) oi[p] = 0, od[p] = 0.0f;  // as the walks leave them
  if (tid == 0) a.out_counts[q] = cn < a.limit ? cn : a.limit;
}

int launch_rerank(const RerankArgs &a, uint32_t nq, hipStream_t stream) {
  if (nq == 0) return SDB_OK;
  if (a.limit < 1 || a.limit > a.rerank || a.rerank > kRerankMax)
    return fail(SDB_ERR_INVALID, "re-rank of %u candidates for %u results not supported on device (limit <= rerank <= %u)", a.rerank,
                a.limit, kRerankMax);
  // at most (32 * 128 + 32 + 2 * 512) floats = 20.6 KB: below what a workgroup gets without asking
  const size_t lds = ((size_t)a.ng * 128 + 32 + 2 * kRerankMax) * sizeof(float);
  const dim3 grid(nq), block(kRerankThreads);
  const bool l2 = a.metric == SDB_METRIC_EUCLIDEAN, map = a.keys != nullptr;
  if (l2 && map) hipLaunchKernelGGL((k_rerank<true, true>), grid, block, lds, stream, a);
  else if (l2) hipLaunchKernelGGL((k_rerank<true, false>), grid, block, lds, stream, a);
  else if (map) hipLaunchKernelGGL((k_rerank<false, true>), grid, block, lds, stream, a);
  else hipLaunchKernelGGL((k_rerank<false, false>), grid, block, lds, stream, a);
  SDB_HIP(hipGetLastError());
  return SDB_OK;
}

}  // namespace sdb
