// filter_host.h -- a batch's filter id lists translated to slot lists on the host's threads (search_batch.hip
// resolve_ids_on_host: tables and knobs the device resolvers do not take).  Free of HIP so that it compiles -- and runs
// under ThreadSanitizer and AddressSanitizer -- on a box without a GPU (tests/host/test_concurrency.cpp).
//
// ids -> slots is a hash lookup per id; a batch of 1 024 queries with 1 000-id filters carries a million of them (5 ms on
// one core), so big batches are split over a few host threads.  Pass 1 validates and counts, pass 2 fills the two CSR
// arrays in place.  slot_of(id): the row an id names, < 0 when it names none.
#pragma once
#include <algorithm>
#include <atomic>
#include <cstdint>
#include <thread>
#include <vector>

namespace sdb {

// fn(q) for every query of the batch, on nthr threads (this one among them when a thread cannot be had)
template <class Fn>
void for_queries(uint64_t nq, unsigned nthr, Fn &&fn) {
  if (nthr <= 1) {
    for (uint64_t q = 0; q < nq; q++) fn(q);
    return;
  }
  // a thread that cannot be had (std::system_error, or no memory for its state) must not leave joinable threads
  // behind -- their destructors would end the process: whatever did start is joined, the rest of the queries are
  // done here
  std::vector<std::thread> pool;
  unsigned started = 0;
  try {
    pool.reserve(nthr);
    for (; started < nthr; started++)
      pool.emplace_back([&, t = started] {
        for (uint64_t q = (uint64_t)nq * t / nthr; q < (uint64_t)nq * (t + 1) / nthr; q++) fn(q);
      });
  } catch (...) {
  }
  for (uint64_t q = (uint64_t)nq * started / nthr; q < nq; q++) fn(q);
  for (auto &th : pool) th.join();
}

enum FilterHostError { kFilterHostOk = 0, kFilterOffsetsDecrease = 1, kFilterIdsNotAscending = 2 };

// Pass 1: per query, how many of its first search_size ids exist (the seeds, search.go:41-48) and how many of all of
// them (Contains, :93), as the offsets of the two lists: off_seed, off_filt [nq + 1].  *bad_q: a query whose ids are
// not strictly ascending, when that is the answer.
template <class SlotOf>
FilterHostError filter_host_count(uint64_t nq, const uint64_t *offsets, const uint64_t *ids, uint32_t search_size, unsigned nthr,
                                  SlotOf &&slot_of, std::vector<uint32_t> &off_seed, std::vector<uint32_t> &off_filt,
                                  uint64_t *bad_q) {
  std::vector<uint32_t> n_seed(nq, 0), n_filt(nq, 0);
  std::atomic<int> bad{0};
  std::atomic<uint64_t> bad_at{0};
  for_queries(nq, nthr, [&](uint64_t q) {
    const uint64_t b = offsets[q], e = offsets[q + 1];
    if (e < b) {
      bad = kFilterOffsetsDecrease;
      return;
    }
    uint32_t ns = 0, nf = 0;
    for (uint64_t i = b; i < e; i++) {
      if (i > b && ids[i] <= ids[i - 1]) {
        bad = kFilterIdsNotAscending, bad_at = q;
        return;
      }
      if (slot_of(ids[i]) < 0) continue;  // GetMany skips unknown ids (itemcache.go:109-128)
      if (i - b < search_size) ns++;
      nf++;
    }
    n_seed[q] = ns, n_filt[q] = nf;
  });
  *bad_q = bad_at.load();
  if (bad) return (FilterHostError)bad.load();
  off_seed.assign(nq + 1, 0), off_filt.assign(nq + 1, 0);
  for (uint64_t q = 0; q < nq; q++) off_seed[q + 1] = off_seed[q] + n_seed[q], off_filt[q + 1] = off_filt[q] + n_filt[q];
  return kFilterHostOk;
}

// Pass 2: the slots themselves, at pass 1's offsets: seeds in id order, the filter's slots ascending.
template <class SlotOf>
void filter_host_fill(uint64_t nq, const uint64_t *offsets, const uint64_t *ids, uint32_t search_size, unsigned nthr,
                      SlotOf &&slot_of, const std::vector<uint32_t> &off_seed, const std::vector<uint32_t> &off_filt,
                      uint32_t *seeds, uint32_t *fslots) {
  for_queries(nq, nthr, [&](uint64_t q) {
    const uint64_t b = offsets[q], e = offsets[q + 1];
    uint32_t *sp = seeds + off_seed[q], *fp = fslots + off_filt[q];
    bool ascending = true;  // rows stored in id order (the usual case) translate to ascending slots: nothing to sort
    int64_t last = -1;
    for (uint64_t i = b; i < e; i++) {
      const int64_t s = slot_of(ids[i]);
      if (s < 0) continue;
      if (i - b < search_size) *sp++ = (uint32_t)s;  // search.go:41-48: the first <= searchSize filter ids that exist
      *fp++ = (uint32_t)s;
      ascending &= s > last;
      last = s;
    }
    if (!ascending) std::sort(fslots + off_filt[q], fp);  // Contains (:93) is answered from ascending slots
  });
}

}  // namespace sdb
