// search_batch.hip -- the host side of K2: one batch search call from its arguments to the launch (the four
// sdb_index_search_batch* entry points), and the kernels that turn a call's filter into slot lists.  Which
// kernel walks is walk_plan.h's decision; walk_launch.hip launches it.
#include <algorithm>
#include <memory>
#include <new>
#include <shared_mutex>
#include <thread>

#include "bq.h"
#include "filter_host.h"
#include "pq.h"
#include "walk_plan.h"

namespace sdb {

// The filter of a search is a set of node ids (a roaring bitmap in the reference, search.go:33-51,93); the walk wants
// slots: per query the slots of the ids that exist, ascending (Contains, :93), and how many of the first searchSize ids
// exist (the seeds, :41-48).  One wave per query resolves its ids in place -- the compacted slots at the start of the
// query's own segment.  MAP = false: a table whose ids are consecutive (id = base + slot: resolving is a subtraction,
// and ascending ids are ascending slots).  MAP = true: any other table -- a probe of the committed view's id -> slot
// table (sdb_index::IdMap); rows are appended in the order they arrive, so ascending ids USUALLY are ascending slots,
// and a query for which they are not raises flags[2]: the walk then answers Contains from the ids themselves
// (SearchArgs::filt_ids); the seeds are the first slots in id order either way.
// flags[0]: != 0 when some query's ids are not strictly ascending; flags[1]: one such query.
template <bool MAP>
__global__ __launch_bounds__(64) void k_filter_resolve(const uint64_t *__restrict__ ids, const uint32_t *__restrict__ off,
                                                       uint64_t base_id, uint32_t view_n, uint32_t search_size,
                                                       uint32_t *__restrict__ slots, uint32_t *__restrict__ fcnt,
                                                       uint32_t *__restrict__ scnt, uint32_t *__restrict__ flags,
                                                       const uint64_t *__restrict__ keys, const uint32_t *__restrict__ vals,
                                                       uint32_t mask) {
  const uint32_t q = blockIdx.x;
  const int lane = threadIdx.x;
  const uint32_t b = off[q], e = off[q + 1];
  uint32_t pos = 0, ns = 0;
  bool bad = false, unsorted = false;
  int64_t last = -1;  // MAP: the slot of the last id that resolved (wave-uniform)
  for (uint32_t base = b; base < e; base += 64) {
    const uint32_t i = base + lane;
    const bool has = i < e;
    const uint64_t id = has ? ids[i] : 0;
    if (has && i > b && id <= ids[i - 1]) bad = true;
    uint64_t s = id - base_id;
    bool ok = has && id >= base_id && s < (uint64_t)view_n;  // rows past the committed count do not exist yet
    if constexpr (MAP) {
      ok = false;
      if (has && id != 0) {
        uint32_t h = idmap_hash(id) & mask;
        while (true) {
          const uint64_t k = keys[h];
          if (k == id) {
            s = vals[h], ok = true;
            break;
          }
          if (k == 0) break;
          h = (h + 1) & mask;
        }
      }
    }
    const uint64_t m = __ballot(ok);
    if constexpr (MAP) {
      if (m) {
        const uint64_t below = m & ((1ull << lane) - 1);
        const int prev_lane = below ? 63 - __clzll((long long)below) : lane;
        const uint32_t sp = (uint32_t)__shfl((int)(uint32_t)s, prev_lane, 64);
        const int64_t prev = below ? (int64_t)sp : last;
        if (ok && (int64_t)s <= prev) unsorted = true;
        last = (int64_t)(uint32_t)__shfl((int)(uint32_t)s, 63 - __clzll((long long)m), 64);
      }
    }
    if (ok) slots[b + pos + (uint32_t)__popcll(m & ((1ull << lane) - 1))] = (uint32_t)s;
    if (base - b < search_size) {  // GetMany(first searchSize ids) skips the unknown ones (itemcache.go:109-128)
      const uint32_t left = search_size - (base - b);
      ns += (uint32_t)__popcll(left >= 64 ? m : (m & ((1ull << left) - 1)));
    }
    pos += (uint32_t)__popcll(m);
  }
  if (__ballot(bad) && lane == 0) atomicOr(flags, 1u), flags[1] = q;
  if (MAP && __ballot(unsorted) && lane == 0) flags[2] = 1u;
  if (lane == 0) fcnt[q] = pos, scnt[q] = ns;
}

// The same for a filter handed over as a BITMAP (sdb_index_search_batch_bitmap): bit i of query q's words is the id
// first_id[q] + i.  A roaring bitmap keeps its dense chunks in exactly this form, and at 100 000 ids out of a million it is
// an eighth of the bytes of the id list -- the upload is what a large filter costs.  Pass 1 (this kernel, one wave per
// query, a lane per 64-bit word): how many of its bits name rows that exist (fcnt) and how many of its FIRST searchSize
// bits do (scnt: the seeds are GetMany(first searchSize ids), unknown ids skipped, search.go:41-48).
__device__ __forceinline__ uint64_t bitmap_valid_mask(uint64_t id0, uint64_t base_id, uint32_t view_n) {
  // bits b of a word whose first id is id0 with base_id <= id0 + b < base_id + view_n  (ids wrap nowhere near 2^64 here)
  uint64_t m = ~0ull;
  if (id0 < base_id) {
    const uint64_t skip = base_id - id0;
    m = skip >= 64 ? 0ull : (m << skip);
  }
  const uint64_t end = base_id + view_n;  // first id past the table
  if (id0 >= end) return 0ull;
  const uint64_t room = end - id0;
  if (room < 64) m &= (1ull << room) - 1;
  return m;
}
__device__ __forceinline__ uint64_t lowest_set_bits(uint64_t w, uint32_t k) {  // the k lowest set bits of w (k < popc(w))
  uint64_t out = 0;
  for (uint32_t i = 0; i < k; i++) {
    const uint64_t b = w & (0 - w);
    out |= b, w ^= b;
  }
  return out;
}
template <bool ALL>  // ALL: every bit counts (the ids are resolved afterwards, k_filter_resolve<true>); scnt is not written
__global__ __launch_bounds__(64) void k_filter_bitmap_count(const uint64_t *__restrict__ words, const uint32_t *__restrict__ woff,
                                                            const uint64_t *__restrict__ first_id, uint64_t base_id,
                                                            uint32_t view_n, uint32_t search_size, uint32_t *__restrict__ fcnt,
                                                            uint32_t *__restrict__ scnt) {
  const uint32_t q = blockIdx.x;
  const int lane = threadIdx.x;
  const uint32_t b = woff[q], e = woff[q + 1];
  const uint64_t f0 = first_id[q];
  uint32_t total = 0, seeds = 0, seen = 0;  // seen: set bits before this round of 64 words
  for (uint32_t base = b; base < e; base += 64) {
    const uint32_t w = base + lane;
    const uint64_t word = w < e ? words[w] : 0ull;
    const uint64_t valid = ALL ? word : (word & bitmap_valid_mask(f0 + (uint64_t)(w - b) * 64u, base_id, view_n));
    uint32_t pc = (uint32_t)__popcll(word), incl = pc;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {  // inclusive scan of the words' populations over the lanes
      const uint32_t up = __shfl_up(incl, o, 64);
      if (lane >= o) incl += up;
    }
    const uint32_t before = seen + incl - pc;  // set bits of the filter in front of this word
    if (before < search_size) {
      const uint32_t left = search_size - before;
      seeds += (uint32_t)__popcll(left >= pc ? valid : (valid & lowest_set_bits(word, left)));
    }
    total += (uint32_t)__popcll(valid);
    seen += __shfl(incl, 63, 64);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) total += __shfl_down(total, o, 64), seeds += __shfl_down(seeds, o, 64);
  if (lane == 0) {
    fcnt[q] = total;
    if (!ALL) scnt[q] = seeds;
  }
}
// exclusive scan of the per-query counts -> where each query's slot list starts (one workgroup; nq is a batch size)
__global__ __launch_bounds__(1024) void k_filter_offsets(const uint32_t *__restrict__ cnt, uint32_t nq, uint32_t *__restrict__ off,
                                                          uint32_t *__restrict__ overflow) {
  __shared__ uint64_t s_part[1024];
  const uint32_t t = threadIdx.x, per = (nq + 1023) / 1024;
  uint64_t sum = 0;
  for (uint32_t i = t * per; i < min(nq, (t + 1) * per); i++) sum += cnt[i];
  s_part[t] = sum;
  __syncthreads();
  if (t == 0) {
    uint64_t run = 0;
    for (uint32_t i = 0; i < 1024; i++) {
      const uint64_t v = s_part[i];
      s_part[i] = run, run += v;
    }
    off[nq] = (uint32_t)run;
    if (run > 0xFFFFFFFFull) *overflow = 1u;
  }
  __syncthreads();
  uint64_t run = s_part[t];
  for (uint32_t i = t * per; i < min(nq, (t + 1) * per); i++) off[i] = (uint32_t)run, run += cnt[i];
}
// pass 2: the slots, ascending, at the query's place in the list
template <bool IDS>  // IDS: every bit, as the id it stands for (64-bit), for k_filter_resolve<true>
__global__ __launch_bounds__(64) void k_filter_bitmap_expand(const uint64_t *__restrict__ words, const uint32_t *__restrict__ woff,
                                                             const uint64_t *__restrict__ first_id, uint64_t base_id,
                                                             uint32_t view_n, const uint32_t *__restrict__ off,
                                                             uint32_t *__restrict__ slots, uint64_t *__restrict__ ids_out) {
  const uint32_t q = blockIdx.x;
  const int lane = threadIdx.x;
  const uint32_t b = woff[q], e = woff[q + 1];
  const uint64_t f0 = first_id[q];
  uint32_t pos = off[q];
  for (uint32_t base = b; base < e; base += 64) {
    const uint32_t w = base + lane;
    const uint64_t id0 = f0 + (uint64_t)(w - b) * 64u;
    uint64_t valid = w < e ? (IDS ? words[w] : (words[w] & bitmap_valid_mask(id0, base_id, view_n))) : 0ull;
    const uint32_t pc = (uint32_t)__popcll(valid);
    uint32_t incl = pc;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const uint32_t up = __shfl_up(incl, o, 64);
      if (lane >= o) incl += up;
    }
    uint32_t at = pos + incl - pc;
    while (valid) {
      const int bit = __ffsll((unsigned long long)valid) - 1;
      valid &= valid - 1;
      if constexpr (IDS) ids_out[at++] = id0 + (uint64_t)bit;
      else slots[at++] = (uint32_t)(id0 + (uint64_t)bit - base_id);
    }
    pos += __shfl(incl, 63, 64);
  }
}

}  // namespace sdb

using namespace sdb;

// ---- step 3: the filter -> slot lists
// a filter as it is handed over: id lists (sdb_index_search_batch; offsets == NULL: no filter) or bitmaps
// (sdb_index_search_batch_bitmap).  Both are host memory.
struct IdFilters {
  const uint64_t *offsets, *ids;
};
struct BitmapFilters {
  const uint64_t *first_id, *word_offsets, *words;
};

// What the walk reads of a filter (SearchArgs' fields of the same names), whoever resolved it.
struct FilterLists {
  const uint32_t *seed_off = nullptr, *filt_off = nullptr, *seeds = nullptr, *filt_slots = nullptr;
  const uint32_t *seed_cnt = nullptr, *filt_cnt = nullptr;
  const uint64_t *filt_ids = nullptr;
  // resolved on the device: seeds and filter are one list per query, in the caller's segments, with counts of their own
  void one_list(const uint32_t *off, const uint32_t *slots, const uint32_t *scnt, const uint32_t *fcnt) {
    seed_off = filt_off = off, seeds = filt_slots = slots, seed_cnt = scnt, filt_cnt = fcnt;
  }
  void into(SearchArgs &a, uint32_t *rbitsets) const {
    a.seed_off = seed_off, a.filt_off = filt_off, a.seeds = seeds, a.filt_slots = filt_slots, a.seed_cnt = seed_cnt,
    a.filt_cnt = filt_cnt, a.filt_ids = filt_ids, a.rbitsets = rbitsets;
  }
};

// What a resolver works with: the table, the committed view the batch walks (its lock is held), the call's workspace and
// the stream its work goes to.
struct FilterCall {
  const sdb_index *ix;
  const sdb_index::View &vw;
  Workspace *ws;
  hipStream_t stream;
  uint64_t nq;
  uint32_t search_size;
};

// The tail both device resolvers share: one wave per query turns its ids into slots (k_filter_resolve), the stream is
// synchronised -- the caller's filter arrays are free again, and the id -> slot table has been probed before the view
// lock goes -- and the kernel's flag words become the call's answer: an invalid filter is an error, not a search.
// d_flags: three zeroed words; h_flags: three words the device can write to.
static int resolve_ids_tail(const FilterCall &c, bool by_map, const uint64_t *d_ids, const uint32_t *d_off, uint32_t *d_sl,
                            uint32_t *d_fc, uint32_t *d_sc, uint32_t *d_flags, uint32_t *h_flags, FilterLists *f) {
  const sdb_index::IdMap &m = c.ix->idmap;
  const auto kernel = by_map ? &k_filter_resolve<true> : &k_filter_resolve<false>;
  hipLaunchKernelGGL(kernel, dim3((unsigned)c.nq), dim3(64), 0, c.stream, d_ids, d_off, c.ix->h_ids[0], c.vw.n, c.search_size,
                     d_sl, d_fc, d_sc, d_flags, by_map ? m.keys : nullptr, by_map ? m.vals : nullptr, by_map ? m.cells - 1 : 0u);
  SDB_HIP(hipGetLastError());
  SDB_HIP(hipMemcpyAsync(h_flags, d_flags, 12, hipMemcpyDeviceToHost, c.stream));
  SDB_HIP(hipStreamSynchronize(c.stream));
  if (h_flags[0])
    return fail(SDB_ERR_INVALID, "filter ids of query %llu are not strictly ascending", (unsigned long long)h_flags[1]);
  f->one_list(d_off, d_sl, d_sc, d_fc);
  // ids and slots disagree on the order somewhere (an id deleted and inserted again sits behind larger ids): the seeds
  // are the first slots in ID order either way; Contains is answered from the ids themselves then (search_kernel.h)
  if (h_flags[2]) f->filt_ids = d_ids;
  return SDB_OK;
}

// Id lists on the device.  Consecutive ids (the bulk-loaded and append-only table: id = first id + slot, no holes): the
// ids go up as they are and one wave per query turns them into slots.  What the host did for this -- a hash lookup per id
// on up to 16 threads, two passes, an upload of the slots -- cost 1.2 ms per batch at 1 000 ids per query next to a 1.5 ms
// walk, 26 ms at 100 000.  The ids of the open transaction's appended rows resolve to slots past the committed count and
// are dropped.  by_map (deletes left holes, arbitrary ids): the same kernel probes the committed view's id -> slot table.
static int resolve_ids_on_device(const FilterCall &c, const IdFilters &idf, bool by_map, FilterLists *f) {
  const uint64_t nq = c.nq;
  for (uint64_t q = 0; q < nq; q++)
    if (idf.offsets[q + 1] < idf.offsets[q]) return fail(SDB_ERR_INVALID, "filter_offsets must be non-decreasing");
  const uint64_t total_ids = idf.offsets[nq] - idf.offsets[0];
  Carve dev, host;
  const auto p_off = dev.take<uint32_t>(nq + 1);
  const auto p_raw = dev.take<uint64_t>(total_ids);
  const auto p_sl = dev.take<uint32_t>(total_ids);
  const auto p_fc = dev.take<uint32_t>(nq), p_sc = dev.take<uint32_t>(nq), p_flags = dev.take<uint32_t>(3);
  const auto p_hoff = host.take<uint32_t>(nq + 1), p_hflags = host.take<uint32_t>(3);
  SDB_TRY(c.ws->filter.ensure(dev.off));
  SDB_TRY(c.ws->filter_host.ensure(host.off));
  void *fb = c.ws->filter.p, *hb = c.ws->filter_host.p;
  uint32_t *h_off = p_hoff.in(hb);
  for (uint64_t q = 0; q <= nq; q++) h_off[q] = (uint32_t)(idf.offsets[q] - idf.offsets[0]);
  SDB_HIP(hipMemcpyAsync(p_off.in(fb), h_off, (nq + 1) * 4, hipMemcpyHostToDevice, c.stream));
  // straight from the caller's array: one DMA when it is pinned (sdb_host_alloc), a staged copy otherwise
  if (total_ids)
    SDB_HIP(hipMemcpyAsync(p_raw.in(fb), idf.ids + idf.offsets[0], total_ids * 8, hipMemcpyHostToDevice, c.stream));
  SDB_HIP(hipMemsetAsync(p_flags.in(fb), 0, 12, c.stream));
  return resolve_ids_tail(c, by_map, p_raw.in(fb), p_off.in(fb), p_sl.in(fb), p_fc.in(fb), p_sc.in(fb), p_flags.in(fb),
                          p_hflags.in(hb), f);
}

// Bitmaps on the device: two passes (count, expand) turn them into the same ascending slot lists.  A table with
// consecutive ids: a bit's slot is a subtraction.  by_map: the bitmaps become id lists ON THE DEVICE (every bit, as the id
// it stands for) and those are resolved through the committed view's id -> slot table like uploaded id lists are.
static int resolve_bitmaps_on_device(const FilterCall &c, const BitmapFilters &bm, bool by_map, FilterLists *f) {
  const uint64_t nq = c.nq;
  for (uint64_t q = 0; q < nq; q++)
    if (bm.word_offsets[q + 1] < bm.word_offsets[q]) return fail(SDB_ERR_INVALID, "filter_word_offsets must be non-decreasing");
  const uint64_t total_words = bm.word_offsets[nq] - bm.word_offsets[0];
  if (total_words >= (1ull << 32)) return fail(SDB_ERR_INVALID, "filter bitmaps of one batch are limited to 2^32 words");
  const uint64_t base_id = c.ix->h_ids[0];
  const uint32_t view_n = c.vw.n;
  const dim3 grid((unsigned)nq), wave(64);
  Carve aux, host;
  const auto p_woff = aux.take<uint32_t>(nq + 1), p_off = aux.take<uint32_t>(nq + 1);
  const auto p_first = aux.take<uint64_t>(nq), p_words = aux.take<uint64_t>(total_words);
  const auto p_fc = aux.take<uint32_t>(nq), p_sc = aux.take<uint32_t>(nq);
  const auto p_flags = aux.take<uint32_t>(4);  // [0]: the offsets' overflow word; [1..3]: k_filter_resolve's three
  const auto p_hoff = host.take<uint32_t>(nq + 1);
  const auto p_hback = host.take<uint32_t>(2);  // [0] total slots, [1] overflow
  const auto p_hflags = host.take<uint32_t>(3);
  SDB_TRY(c.ws->filter_host.ensure(host.off));
  SDB_TRY(c.ws->filter_aux.ensure(aux.off));
  void *ab = c.ws->filter_aux.p, *hb = c.ws->filter_host.p;
  uint32_t *d_woff = p_woff.in(ab), *d_off = p_off.in(ab), *d_fc = p_fc.in(ab), *d_sc = p_sc.in(ab), *d_flags = p_flags.in(ab);
  uint64_t *d_first = p_first.in(ab), *d_words = p_words.in(ab);
  uint32_t *h_off = p_hoff.in(hb), *h_back = p_hback.in(hb);
  for (uint64_t q = 0; q <= nq; q++) h_off[q] = (uint32_t)(bm.word_offsets[q] - bm.word_offsets[0]);
  SDB_HIP(hipMemcpyAsync(d_woff, h_off, (nq + 1) * 4, hipMemcpyHostToDevice, c.stream));
  SDB_HIP(hipMemcpyAsync(d_first, bm.first_id, nq * 8, hipMemcpyHostToDevice, c.stream));
  if (total_words)
    SDB_HIP(hipMemcpyAsync(d_words, bm.words + bm.word_offsets[0], total_words * 8, hipMemcpyHostToDevice, c.stream));
  SDB_HIP(hipMemsetAsync(d_flags, 0, 16, c.stream));
  const auto count = by_map ? &k_filter_bitmap_count<true> : &k_filter_bitmap_count<false>;
  hipLaunchKernelGGL(count, grid, wave, 0, c.stream, d_words, d_woff, d_first, base_id, view_n, c.search_size, d_fc, d_sc);
  hipLaunchKernelGGL(k_filter_offsets, dim3(1), dim3(1024), 0, c.stream, d_fc, (uint32_t)nq, d_off, d_flags);
  SDB_HIP(hipGetLastError());
  SDB_HIP(hipMemcpyAsync(h_back, d_off + nq, 4, hipMemcpyDeviceToHost, c.stream));
  SDB_HIP(hipMemcpyAsync(h_back + 1, d_flags, 4, hipMemcpyDeviceToHost, c.stream));
  SDB_HIP(hipStreamSynchronize(c.stream));  // the slot list's size; the caller's arrays are free again
  if (h_back[1]) return fail(SDB_ERR_INVALID, "the filters of one batch name more than 2^32 stored ids");
  Carve dev;
  const auto p_sl = dev.take<uint32_t>(h_back[0]);
  const auto p_ids = dev.take<uint64_t>(by_map ? h_back[0] : 0);
  dev.take<uint32_t>(1);  // (never an empty buffer)
  SDB_TRY(c.ws->filter.ensure(dev.off));
  uint32_t *d_sl = p_sl.in(c.ws->filter.p);
  uint64_t *d_ids = by_map ? p_ids.in(c.ws->filter.p) : nullptr;
  const auto expand = by_map ? &k_filter_bitmap_expand<true> : &k_filter_bitmap_expand<false>;
  hipLaunchKernelGGL(expand, grid, wave, 0, c.stream, d_words, d_woff, d_first, base_id, view_n, d_off, d_sl, d_ids);
  if (by_map) return resolve_ids_tail(c, true, d_ids, d_off, d_sl, d_fc, d_sc, d_flags + 1, p_hflags.in(hb), f);
  SDB_HIP(hipGetLastError());
  f->one_list(d_off, d_sl, d_sc, d_fc);
  return SDB_OK;
}

// Id lists on the host (filter_host.h), for what the device resolvers do not take: search.go:41-48: seeds = the first
// <= searchSize filter ids (ascending) that exist; Contains (:93) is answered from the whole filter as ascending slots.
static int resolve_ids_on_host(const FilterCall &c, const IdFilters &idf, FilterLists *f) {
  const uint64_t nq = c.nq, total_ids = idf.offsets[nq] - idf.offsets[0];
  // one thread per 128 k ids, at most 16 (and what the machine has): a million ids take 5 ms on one core, a thread ~50 us to start
  const unsigned nthr = (unsigned)std::min<uint64_t>(std::min<unsigned>(16u, std::max(1u, std::thread::hardware_concurrency())),
                                                     std::max<uint64_t>(1, total_ids >> 17));
  const auto slot_of = [ix = c.ix, view_n = c.vw.n](uint64_t id) { return ix->slot_of_committed(id, view_n); };
  std::vector<uint32_t> off_seed, off_filt;
  uint64_t bad_q = 0;
  switch (filter_host_count(nq, idf.offsets, idf.ids, c.search_size, nthr, slot_of, off_seed, off_filt, &bad_q)) {
    case kFilterOffsetsDecrease: return fail(SDB_ERR_INVALID, "filter_offsets must be non-decreasing");
    case kFilterIdsNotAscending:
      return fail(SDB_ERR_INVALID, "filter ids of query %llu are not strictly ascending", (unsigned long long)bad_q);
    case kFilterHostOk: break;
  }
  // the two lists are written where the DMA engine can take them from (pinned, kept with the workspace): a pageable
  // vector of 10^8 slots costs its zero-fill and a staged copy on top of the translation
  const size_t n_seeds = off_seed[nq], n_fslots = off_filt[nq];
  Carve host, dev;
  const auto p_hseeds = host.take<uint32_t>(n_seeds), p_hslots = host.take<uint32_t>(n_fslots);
  host.take<uint32_t>(1);  // (never an empty buffer)
  std::unique_ptr<char[]> pageable;  // when the pinned buffer cannot be had (the limit on locked memory): an ordinary one
  void *hb = nullptr;
  if (c.ws->filter_host.ensure(host.off) == SDB_OK) {
    hb = c.ws->filter_host.p;
  } else {
    (void)hipGetLastError();
    pageable.reset(new (std::nothrow) char[host.off]);
    if (!pageable) return fail(SDB_ERR_DEVICE, "out of host memory for the filter lists");
    hb = pageable.get();
  }
  filter_host_fill(nq, idf.offsets, idf.ids, c.search_size, nthr, slot_of, off_seed, off_filt, p_hseeds.in(hb), p_hslots.in(hb));
  const auto p_so = dev.take<uint32_t>(nq + 1), p_fo = dev.take<uint32_t>(nq + 1);
  const auto p_seeds = dev.take<uint32_t>(n_seeds), p_slots = dev.take<uint32_t>(n_fslots);
  SDB_TRY(c.ws->filter.ensure(dev.off));
  void *fb = c.ws->filter.p;
  SDB_HIP(hipMemcpyAsync(p_so.in(fb), off_seed.data(), (nq + 1) * 4, hipMemcpyHostToDevice, c.stream));
  SDB_HIP(hipMemcpyAsync(p_fo.in(fb), off_filt.data(), (nq + 1) * 4, hipMemcpyHostToDevice, c.stream));
  if (n_seeds) SDB_HIP(hipMemcpyAsync(p_seeds.in(fb), p_hseeds.in(hb), n_seeds * 4, hipMemcpyHostToDevice, c.stream));
  if (n_fslots) SDB_HIP(hipMemcpyAsync(p_slots.in(fb), p_hslots.in(hb), n_fslots * 4, hipMemcpyHostToDevice, c.stream));
  SDB_HIP(hipStreamSynchronize(c.stream));  // the staging vectors die with this scope
  f->seed_off = p_so.in(fb), f->filt_off = p_fo.in(fb), f->seeds = p_seeds.in(fb), f->filt_slots = p_slots.in(fb);
  return SDB_OK;
}

// bitmaps as id lists, for a table that cannot take them on the device -- the reference iterates its roaring bitmap the
// same way (search.go:41-48)
static int bitmaps_to_ids(uint64_t nq, const BitmapFilters &bm, std::vector<uint64_t> &off, std::vector<uint64_t> &ids) {
  off.assign(nq + 1, 0);
  for (uint64_t q = 0; q < nq; q++) {
    if (bm.word_offsets[q + 1] < bm.word_offsets[q]) return fail(SDB_ERR_INVALID, "filter_word_offsets must be non-decreasing");
    for (uint64_t w = bm.word_offsets[q]; w < bm.word_offsets[q + 1]; w++)
      for (uint64_t word = bm.words[w]; word; word &= word - 1)
        ids.push_back(bm.first_id[q] + (w - bm.word_offsets[q]) * 64 + (uint64_t)__builtin_ctzll(word));
    off[q + 1] = ids.size();
  }
  if (ids.empty()) ids.push_back(0);
  return SDB_OK;
}

// Which resolver a call gets.  On the device: a table with committed rows, unless SDB_TUNE_HOST_FILTERS says otherwise
// (and id lists of less than 2^32 ids).  A table whose ids are not consecutive needs the view's id -> slot table there:
// ensure_idmap runs first, before anything of this call is enqueued, and no memory for the table is no error -- the
// host's map serves.  Bitmaps that cannot stay on the device become id lists, resolved in this same call: one workspace,
// one committed view.  (The id tables only change under the view lock, which the call holds shared.)
static int resolve_filter(const FilterCall &c, IdFilters idf, const BitmapFilters *bm, FilterLists *f) {
  const sdb_index *ix = c.ix;
  bool on_device = ix->n > 0 && c.vw.n > 0 && !ix->tune_host_filters &&
                   (bm || idf.offsets[c.nq] - idf.offsets[0] < (1ull << 32));
  const bool by_map = on_device && !ix->dense_ids;
  if (by_map && ix->ensure_idmap(c.vw, c.stream) != SDB_OK) on_device = false;
  if (bm && on_device) return resolve_bitmaps_on_device(c, *bm, by_map, f);
  std::vector<uint64_t> own_off, own_ids;
  if (bm) {
    SDB_TRY(bitmaps_to_ids(c.nq, *bm, own_off, own_ids));
    idf = IdFilters{own_off.data(), own_ids.data()};
  }
  return on_device ? resolve_ids_on_device(c, idf, by_map, f) : resolve_ids_on_host(c, idf, f);
}

// ---- steps 1, 2, 4: the arguments, the re-rank workspace, SearchArgs
static int validate_call(const sdb_index *ix, uint64_t nq, const float *queries, uint32_t limit, uint32_t search_size,
                         uint32_t rerank, const IdFilters &idf, const uint64_t *out_ids, const float *out_dists,
                         const uint32_t *out_counts) {
  if (!queries || !out_ids || !out_dists || !out_counts) return fail(SDB_ERR_INVALID, "NULL argument");
  if (limit < 1) return fail(SDB_ERR_INVALID, "invalid limit %u for vector query", limit);
  if (search_size < limit)  // search.go:23-25
    return fail(SDB_ERR_INVALID, "searchSize (%u) must be greater than k (%u)", search_size, limit);
  if (rerank && (rerank < limit || rerank > search_size))
    return fail(SDB_ERR_INVALID, "rerank (%u) must lie between k (%u) and searchSize (%u)", rerank, limit, search_size);
  if (rerank && search_size > kRerankMax)
    return fail(SDB_ERR_INVALID, "searchSize %u not supported on device (1..512)", search_size);
  if (ix->P.strict && (search_size < 25 || search_size > 75 || limit > 75))  // models/search.go:287-297
    return fail(SDB_ERR_INVALID, "invalid searchSize %u / limit %u for vector query, expected 25-75 / 1-75",
                search_size, limit);
  if (ix->broken) return fail(SDB_ERR_STATE, "index is unusable after a failed write; reload it from the bucket");
  if (ix->start_slot < 0) return fail(SDB_ERR_STATE, "failed to get start point");  // search.go:57-60
  if (idf.offsets && idf.offsets[nq] && !idf.ids) return fail(SDB_ERR_INVALID, "filter_ids is NULL");
  if (nq > 0x7FFFFFFFull) return fail(SDB_ERR_INVALID, "too many queries");
  return SDB_OK;
}

// Re-ranking (sdb_index_search_batch_rerank): the walk is launched exactly as without it, with limit = rerank and its
// three outputs in the workspace; k_rerank (rerank.hip) then writes where the walk would have written.
struct RerankPlan {
  RerankArgs ra{};
  float *walk_dists = nullptr;  // the quantizer's distances: written by the walk, read by nobody
};
// The walk's candidates stay in the workspace, and their ids become slots again on the device -- by the committed view's
// id -> slot table where the ids are not consecutive (built here, before anything is enqueued).
static int plan_rerank(const sdb_index *ix, const sdb_index::View &vw, Workspace *ws, uint64_t nq, uint32_t limit, uint32_t rerank,
                       hipStream_t stream, RerankPlan *rp) {
  Carve c;
  const auto p_ids = c.take<uint64_t>(nq * rerank);
  const auto p_d = c.take<float>(nq * rerank);
  const auto p_cnt = c.take<uint32_t>(nq);
  SDB_TRY(ws->rerank.ensure(c.off));
  RerankArgs &ra = rp->ra;
  if (!ix->dense_ids) {
    SDB_TRY(ix->ensure_idmap(vw, stream));
    ra.keys = ix->idmap.keys, ra.vals = ix->idmap.vals, ra.mask = ix->idmap.cells - 1;
  }
  const RowLayout &l = ix->lay;
  ra.cand_ids = p_ids.in(ws->rerank.p), ra.cand_cnt = p_cnt.in(ws->rerank.p);
  rp->walk_dists = p_d.in(ws->rerank.p);
  ra.base_id = ix->h_ids.empty() ? 0 : ix->h_ids[0], ra.view_n = vw.n;
  ra.slab = ix->d_slab, ra.dim = l.dim, ra.nblk = l.nblk, ra.ng = l.ng, ra.tail = l.tail, ra.ld = l.ld;
  ra.rerank = rerank, ra.limit = limit, ra.metric = (int)ix->P.metric;
  return SDB_OK;
}

// everything of SearchArgs that the table, the view and the knobs decide
static void fill_search_args(const sdb_index *ix, const sdb_index::View &vw, uint32_t *bitsets, uint32_t words,
                             uint32_t search_size, uint32_t walk_limit, SearchArgs &a) {
  const RowLayout &l = ix->lay;
  a.slab = ix->d_slab, a.adj = vw.adj, a.ids = vw.ids;
  a.adj_codes = vw.adj_codes, a.adj_rows = vw.n;
  a.bitsets = bitsets, a.words_per_query = words;
  a.dim = l.dim, a.nblk = l.nblk, a.ng = l.ng, a.tail = l.tail, a.ld = l.ld;
  a.start_slot = (uint32_t)ix->start_slot;
  a.start_ext = vw.start_ext, a.start_ext_n = vw.start_ext_n;
  a.search_size = search_size, a.limit = walk_limit, a.metric = (int)ix->P.metric;
  a.hash_limit = ix->tune_hash_limit, a.prefer_bitset = ix->tune_no_hash ? 1u : 0u;
  a.wide_hash = ix->tune_wide_hash ? 1u : 0u, a.hash16_probes = ix->tune_hash16_probes;
  a.pq_narrow = ix->tune_pq_narrow;
  a.wide_mode = ix->tune_wide_walk;
}

// The two-precision hop: only with the copy of exactly this view's rows, outside a write transaction.  Every field is read
// once, under the shared lock the writer's changes to them exclude.  This call's stage is decided here, once: the int8
// copy serves the calls stage_int8() names (a filtered call reads float32 rows then), the float16 copy every plain
// call and -- opt-in, SDB_TUNE_SKETCH_FILTERED -- the filtered ones.
static void choose_stage(const sdb_index *ix, bool filtered, SearchArgs &a) {
  const uint32_t knob = ix->tune_sketch;
  const void *sk = ix->d_sketch;
  if (knob && sk && ix->sketch_gen.load(std::memory_order_acquire) == ix->view_gen && !ix->in_tx) {
    if (ix->sketch8)
      a.stage = stage_int8((int)ix->lay.ng, ix->P.metric == SDB_METRIC_EUCLIDEAN, filtered) ? Stage::kInt8 : Stage::kNone;
    else a.stage = (!filtered || ix->tune_sketch_filtered) ? Stage::kHalf : Stage::kNone;
  }
  if (a.stage != Stage::kNone)
    a.sketch = sk, a.sketch_norm = ix->d_sketch_norm, a.sk_emax = ix->sk_emax, a.sk_ymax = ix->sk_ymax,
    a.sk_audit = (knob == 2 || knob == 4) ? 1u : 0u, a.sk_counters = ix->d_sk_counters, a.sk8_scale = ix->sk8_scale;
}

// ---- step 5: where the walk reads its queries and writes its answers
// Device memory: the caller's pointers as they are.  Host memory: page-locked buffers (sdb_host_alloc, or locked by the
// caller) are read and written IN PLACE by the walk: a wave reads its query once, when it starts (PlainDist::init), and
// writes its <= limit results when it ends, so what crosses the bus is what a copy would have moved, without the copy
// packets around the kernel and without a staging buffer -- the call is one launch and one wait.  (Not with a quantizer:
// the table kernel reads a query's sub-vectors once per centroid block, and host memory is not cached on the device.  Not
// with a trace: test calls.  Not under SDB_TUNE_NO_ZERO_COPY.)  Otherwise: staged through one scratch allocation; what is
// page-locked still skips its copy.
struct Placement {
  uint64_t nq;
  uint32_t limit, dim;
  const float *queries;
  uint64_t *out_ids;
  float *out_dists;
  uint32_t *out_counts;
  const sdb_search_trace *trace;
  bool on_host = false, copy_out = false, copy_trace = false;

  size_t b_ids() const { return nq * limit * sizeof(uint64_t); }
  size_t b_dists() const { return nq * limit * sizeof(float); }
  uint32_t vcap() const { return trace ? trace->visit_cap : 0; }

  // before the launch: SearchArgs' queries, out_* and tr_*, and whatever has to be on the device by then
  int place(const sdb_index *ix, Workspace *ws, int mem, hipStream_t stream, SearchArgs &a) {
    if (mem == SDB_MEM_DEVICE) {
      a.queries = queries;
      a.out_ids = out_ids, a.out_dists = out_dists, a.out_counts = out_counts;
      if (trace) {
        a.tr_ndist = trace->n_dist, a.tr_nhop = trace->n_hop, a.tr_nedges = trace->n_edges;
        a.tr_visit = trace->visit_ids, a.visit_cap = trace->visit_ids ? vcap() : 0;
      }
      return SDB_OK;
    }
    on_host = true;
    const bool zc_ok = !trace && !ix->tune_no_zero_copy;
    void *z_q = nullptr, *z_i = nullptr, *z_d = nullptr, *z_c = nullptr;
    const bool zc_out = zc_ok && device_view_of_host(out_ids, b_ids(), &z_i) && device_view_of_host(out_dists, b_dists(), &z_d) &&
                        device_view_of_host(out_counts, nq * sizeof(uint32_t), &z_c);
    const bool zc_q = zc_ok && !ix->pq && !ix->bq && device_view_of_host(queries, nq * dim * sizeof(float), &z_q);
    if (zc_q) a.queries = static_cast<const float *>(z_q);
    if (zc_out) a.out_ids = static_cast<uint64_t *>(z_i), a.out_dists = static_cast<float *>(z_d), a.out_counts = static_cast<uint32_t *>(z_c);
    if (zc_out && zc_q) return SDB_OK;
    Carve c;
    const auto p_q = c.take<float>(nq * dim);
    const auto p_ids = c.take<uint64_t>(nq * limit);
    const auto p_d = c.take<float>(nq * limit);
    const auto p_c = c.take<uint32_t>(nq);
    const auto p_nd = c.take<uint32_t>(nq), p_nh = c.take<uint32_t>(nq), p_ne = c.take<uint32_t>(nq);
    const auto p_v = c.take<uint64_t>((trace && trace->visit_ids) ? nq * vcap() : 0);
    SDB_TRY(ws->scratch.ensure(c.off));
    void *base = ws->scratch.p;
    if (!zc_q) {
      SDB_HIP(hipMemcpyAsync(p_q.in(base), queries, nq * dim * sizeof(float), hipMemcpyHostToDevice, stream));
      a.queries = p_q.in(base);
    }
    if (!zc_out) a.out_ids = p_ids.in(base), a.out_dists = p_d.in(base), a.out_counts = p_c.in(base);
    if (trace) {
      a.tr_ndist = p_nd.in(base), a.tr_nhop = p_nh.in(base), a.tr_nedges = p_ne.in(base);
      if (trace->visit_ids) a.tr_visit = p_v.in(base), a.visit_cap = vcap();
    }
    // the staged ids and distances start out as zeros
    SDB_HIP(hipMemsetAsync(p_ids.in(base), 0, p_c.at - p_ids.at, stream));
    copy_out = !zc_out, copy_trace = trace != nullptr;
    return SDB_OK;
  }

  // behind the launch, the view lock released: staged answers go back to the caller, and a host-memory call waits
  int collect(const SearchArgs &a, hipStream_t stream) const {
    if (!on_host) return SDB_OK;
    if (copy_out) {
      SDB_HIP(hipMemcpyAsync(out_ids, a.out_ids, b_ids(), hipMemcpyDeviceToHost, stream));
      SDB_HIP(hipMemcpyAsync(out_dists, a.out_dists, b_dists(), hipMemcpyDeviceToHost, stream));
      SDB_HIP(hipMemcpyAsync(out_counts, a.out_counts, nq * sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
    }
    if (copy_trace) {
      if (trace->n_dist) SDB_HIP(hipMemcpyAsync(trace->n_dist, a.tr_ndist, nq * 4, hipMemcpyDeviceToHost, stream));
      if (trace->n_hop) SDB_HIP(hipMemcpyAsync(trace->n_hop, a.tr_nhop, nq * 4, hipMemcpyDeviceToHost, stream));
      if (trace->n_edges) SDB_HIP(hipMemcpyAsync(trace->n_edges, a.tr_nedges, nq * 4, hipMemcpyDeviceToHost, stream));
      if (trace->visit_ids)
        SDB_HIP(hipMemcpyAsync(trace->visit_ids, a.tr_visit, nq * vcap() * sizeof(uint64_t), hipMemcpyDeviceToHost, stream));
    }
    SDB_HIP(hipStreamSynchronize(stream));
    return SDB_OK;
  }
};

// ---- step 6: the launch
// the attached quantizer's share of SearchArgs; a.queries is where the walk will read them
static int attach_quantizer(const sdb_index *ix, Workspace *ws, uint64_t nq, hipStream_t stream, SearchArgs &a) {
  if (ix->bq)  // DistanceFromFloat encodes the query once (binary.go:192): the walk does, when it starts (BitDist::init)
    a.bq_codes = reinterpret_cast<const uint64_t *>(ix->d_codes), a.bq_thr = ix->bq->d_thr, a.bq_W = ix->bq->W,
    a.bq_metric = (uint32_t)ix->bq->metric;
  if (ix->pq) {  // fitted quantizer: DistanceFromFloat builds the M x K table first (product.go:255-263)
    const sdb_pq *pq = ix->pq;
    SDB_TRY(ws->lut.ensure((size_t)nq * pq->M * pq->K * sizeof(float)));
    SDB_TRY(pq_build_lut(pq, a.queries, nq, ws->lut.as<float>(), stream));
    a.pq_lut = ws->lut.as<float>(), a.pq_codes = ix->d_codes, a.pq_M = pq->M, a.pq_K = pq->K;
    a.pq_lut_in_lds = ((size_t)pq->M * pq->K * sizeof(float) <= 64 * 1024) ? 1u : 0u;
  }
  return SDB_OK;
}

// The walk (and the re-rank behind it), between its profiling events, and the `launched` event behind both.  The caller
// holds the shared view lock and lets go of it when this returns: by then the event is recorded -- sdb_index::commit
// waits for it before it hands the copy this batch walks to the writer -- or, without an event, the stream has been
// synchronised.  tail: nothing of this call follows on the stream (a device-memory call).
static int launch_walk(sdb_index *ix, Workspace *ws, SearchArgs &a, RerankPlan *rp, uint64_t nq, size_t bitset_bytes, bool tail,
                       hipStream_t stream) {
  SDB_TRY(attach_quantizer(ix, ws, nq, stream, a));
  const WalkPlan plan = plan_walk(a, (uint32_t)nq);
  // ClearAll (distset.go:101); the LDS hash variant clears a bitset only for a query that overflows it
  if (plan.clear_bitsets) SDB_HIP(hipMemsetAsync(ws->bitsets.p, 0, bitset_bytes, stream));
  RerankArgs *ra = rp ? &rp->ra : nullptr;
  if (ra) {  // the walk's outputs go to the workspace; what the caller (or the staging) named is k_rerank's to write
    ra->queries = a.queries, ra->out_ids = a.out_ids, ra->out_dists = a.out_dists, ra->out_counts = a.out_counts;
    a.out_ids = const_cast<uint64_t *>(ra->cand_ids), a.out_dists = rp->walk_dists, a.out_counts = const_cast<uint32_t *>(ra->cand_cnt);
  }
  const bool prof = ix->profiling && !ix->ev0.empty();
  const uint32_t slot = (uint32_t)(ix->prof_count % sdb_index::kProfRing);
  if (prof) (void)hipEventRecord(ix->ev0[slot], stream);
  int rc = launch_walk_plan(plan, a, (uint32_t)nq, stream);
  if (prof) {
    (void)hipEventRecord(ix->ev1[slot], stream);
    ix->prof_count++;
  }
  if (ra) a.out_ids = ra->out_ids, a.out_dists = ra->out_dists, a.out_counts = ra->out_counts;  // (Placement::collect reads these)
  if (ra && rc == SDB_OK) {  // same stream, same view, still under the shared lock: no commit comes between the two
    const uint32_t slot2 = (uint32_t)(ix->prof_count % sdb_index::kProfRing);  // a profiled call records two entries: walk, re-rank
    if (prof) (void)hipEventRecord(ix->ev0[slot2], stream);
    rc = launch_rerank(*ra, (uint32_t)nq, stream);
    if (prof) {
      (void)hipEventRecord(ix->ev1[slot2], stream);
      ix->prof_count++;
    }
    // the id -> slot table is this view's only while the shared lock is held (sdb_index::IdMap: the next view's first
    // filtered or re-ranked search rebuilds it in place): like k_filter_resolve, the probe has run before the lock goes
    if (ra->keys && rc == SDB_OK && hipStreamSynchronize(stream) != hipSuccess) {
      (void)hipGetLastError();
      rc = fail(SDB_ERR_DEVICE, "re-ranked search failed on the device");
    }
  }
  // from here on a commit may hand the copy this batch walks to the writer: it waits for this event first
  if (!ws->launched) (void)hipEventCreateWithFlags(&ws->launched, hipEventDisableTiming);
  if (ws->launched && hipEventRecord(ws->launched, stream) == hipSuccess) ws->launched_valid = true, ws->launched_is_tail = tail;
  else if (rc == SDB_OK) (void)hipStreamSynchronize(stream);  // no event: finish before letting go of the version
  return rc;
}

// ---- the call
// a workspace held for one call (sdb_index::acquire_ws / release_ws)
struct WorkspaceHold {
  const sdb_index *ix;
  Workspace *ws;
  hipStream_t stream;
  bool async;
  ~WorkspaceHold() { ix->release_ws(ws, stream, async); }
};

static int search_batch_impl(sdb_index *ix, uint64_t nq, const float *queries, uint32_t limit, uint32_t search_size,
                             const IdFilters &idf, const BitmapFilters *bm, uint64_t *out_ids, float *out_dists,
                             uint32_t *out_counts, const sdb_search_trace *trace, int mem, void *stream_, uint32_t rerank) {
  // 1. the arguments
  if (!ix) return fail(SDB_ERR_INVALID, "index is NULL");
  if (nq == 0) return SDB_OK;
  SDB_TRY(validate_call(ix, nq, queries, limit, search_size, rerank, idf, out_ids, out_dists, out_counts));
  const bool filtered = idf.offsets != nullptr || bm != nullptr;

  // 2. the workspace, and the graph version this batch walks: the last committed one, whatever a writer is doing
  // meanwhile.  The shared lock is taken before the first workspace allocation and held until launch_walk has recorded
  // the `launched` event (sdb_index::commit counts on that); every return before that releases it too.
  DeviceGuard dg(ix->P.device);
  hipStream_t stream = as_stream(stream_);
  const bool async = mem == SDB_MEM_DEVICE;
  Workspace *ws = ix->acquire_ws(stream, async);
  WorkspaceHold hold{ix, ws, stream, async};
  if (mem == SDB_MEM_HOST) {
    if (!ws->own_stream) SDB_HIP(hipStreamCreateWithFlags(&ws->own_stream, hipStreamNonBlocking));
    stream = ws->own_stream;
  }
  std::shared_lock<sdb::ViewMutex> view_lock(ix->view_mu);
  const sdb_index::View vw = ix->view;
  const uint32_t words = ((vw.n + 31) / 32 + 31) & ~31u;  // per-query bitset, 128-byte multiple
  const size_t bitset_bytes = (size_t)nq * words * sizeof(uint32_t) * (filtered ? 2 : 1);  // filtered: the result set's own behind it
  SDB_TRY(ws->bitsets.ensure(bitset_bytes));
  RerankPlan rp;
  if (rerank) SDB_TRY(plan_rerank(ix, vw, ws, nq, limit, rerank, stream, &rp));

  // 3. the filter
  FilterLists lists;
  if (filtered) SDB_TRY(resolve_filter(FilterCall{ix, vw, ws, stream, nq, search_size}, idf, bm, &lists));

  // 4. SearchArgs
  SearchArgs a{};
  fill_search_args(ix, vw, ws->bitsets.as<uint32_t>(), words, search_size, rerank ? rerank : limit, a);
  if (filtered) lists.into(a, ws->bitsets.as<uint32_t>() + (size_t)nq * words);
  choose_stage(ix, filtered, a);

  // 5. the buffers
  Placement pl{nq, limit, ix->lay.dim, queries, out_ids, out_dists, out_counts, trace};
  SDB_TRY(pl.place(ix, ws, mem, stream, a));

  // 6. the launch
  const int rc = launch_walk(ix, ws, a, rerank ? &rp : nullptr, nq, bitset_bytes, mem == SDB_MEM_DEVICE, stream);
  view_lock.unlock();
  return rc != SDB_OK ? rc : pl.collect(a, stream);
}

extern "C" {

int sdb_index_search_batch(sdb_index *ix, uint64_t nq, const float *queries, uint32_t limit,
                           uint32_t search_size, const uint64_t *filter_offsets,
                           const uint64_t *filter_ids, uint64_t *out_ids, float *out_dists,
                           uint32_t *out_counts, const sdb_search_trace *trace, int mem, void *stream_) try {
  return search_batch_impl(ix, nq, queries, limit, search_size, IdFilters{filter_offsets, filter_ids}, nullptr, out_ids, out_dists,
                           out_counts, trace, mem, stream_, 0);
}
SDB_API_CATCH("sdb_index_search_batch")

// sdb_index_search_batch_bitmap and its re-ranked form (rerank != 0)
static int search_batch_bitmap_impl(sdb_index *ix, uint64_t nq, const float *queries, uint32_t limit, uint32_t search_size,
                                    const uint64_t *filter_first_id, const uint64_t *filter_word_offsets,
                                    const uint64_t *filter_words, uint64_t *out_ids, float *out_dists, uint32_t *out_counts,
                                    const sdb_search_trace *trace, int mem, void *stream_, uint32_t rerank) {
  if (!filter_first_id || !filter_word_offsets) return fail(SDB_ERR_INVALID, "NULL filter argument");
  if (nq && filter_word_offsets[nq] > filter_word_offsets[0] && !filter_words) return fail(SDB_ERR_INVALID, "filter_words is NULL");
  const BitmapFilters bm{filter_first_id, filter_word_offsets, filter_words};
  return search_batch_impl(ix, nq, queries, limit, search_size, IdFilters{nullptr, nullptr}, &bm, out_ids, out_dists, out_counts, trace,
                           mem, stream_, rerank);
}

int sdb_index_search_batch_bitmap(sdb_index *ix, uint64_t nq, const float *queries, uint32_t limit, uint32_t search_size,
                                  const uint64_t *filter_first_id, const uint64_t *filter_word_offsets,
                                  const uint64_t *filter_words, uint64_t *out_ids, float *out_dists, uint32_t *out_counts,
                                  const sdb_search_trace *trace, int mem, void *stream_) try {
  return search_batch_bitmap_impl(ix, nq, queries, limit, search_size, filter_first_id, filter_word_offsets, filter_words, out_ids,
                                  out_dists, out_counts, trace, mem, stream_, 0);
}
SDB_API_CATCH("sdb_index_search_batch_bitmap")

// The library's own extension (the reference does not re-rank): the walk's first `rerank` candidates in the order of
// their stored float32 rows' distances (semadb_amd.h; rerank.hip).  rerank = 0 is no re-ranked search.
int sdb_index_search_batch_rerank(sdb_index *ix, uint64_t nq, const float *queries, uint32_t limit, uint32_t search_size,
                                  uint32_t rerank, const uint64_t *filter_offsets, const uint64_t *filter_ids, uint64_t *out_ids,
                                  float *out_dists, uint32_t *out_counts, const sdb_search_trace *trace, int mem, void *stream_) try {
  if (rerank == 0) return fail(SDB_ERR_INVALID, "rerank (0) must lie between k (%u) and searchSize (%u)", limit, search_size);
  return search_batch_impl(ix, nq, queries, limit, search_size, IdFilters{filter_offsets, filter_ids}, nullptr, out_ids, out_dists,
                           out_counts, trace, mem, stream_, rerank);
}
SDB_API_CATCH("sdb_index_search_batch_rerank")

int sdb_index_search_batch_bitmap_rerank(sdb_index *ix, uint64_t nq, const float *queries, uint32_t limit, uint32_t search_size,
                                         uint32_t rerank, const uint64_t *filter_first_id, const uint64_t *filter_word_offsets,
                                         const uint64_t *filter_words, uint64_t *out_ids, float *out_dists, uint32_t *out_counts,
                                         const sdb_search_trace *trace, int mem, void *stream_) try {
  if (rerank == 0) return fail(SDB_ERR_INVALID, "rerank (0) must lie between k (%u) and searchSize (%u)", limit, search_size);
  return search_batch_bitmap_impl(ix, nq, queries, limit, search_size, filter_first_id, filter_word_offsets, filter_words, out_ids,
                                  out_dists, out_counts, trace, mem, stream_, rerank);
}
SDB_API_CATCH("sdb_index_search_batch_bitmap_rerank")

}  // extern "C"
