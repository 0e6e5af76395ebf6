// visited_set.h -- K2: the visited-set policies.
// (a part of search_kernel.h, which includes it after what it builds on; no .hip file includes it directly)
#pragma once

namespace sdb {

// ---- visited-set policies (the visitedSet interface, distset.go:66-69) -----------------------------------

// Every policy: init_nosync(lds, bits, lane, a) -- its LDS table (if it has one), the query's HBM bitset, and whatever
// else it needs picked out of the arguments; the caller puts the barrier behind it -- and test_and_set (CheckAndVisit).

// VisitedBitSet (distset.go:89-116): one bit per slot in HBM, test-and-set with a returning atomicOr.  The LDS sets
// carry on with it once they have spilled.
__device__ __forceinline__ bool bitset_test_and_set(uint32_t *bits, bool active, uint32_t slot) {
  if (!active) return false;
  const uint32_t bit = 1u << (slot & 31);
  return !(atomicOr(&bits[slot >> 5], bit) & bit);
}
struct BitVisited {
  uint32_t *__restrict__ bits;
  __device__ __forceinline__ void init_nosync(uint32_t *, uint32_t *bitset, int, const SearchArgs &) { bits = bitset; }
  __device__ __forceinline__ bool test_and_set(bool active, uint32_t slot, int lane) { return bitset_test_and_set(bits, active, slot); }
};

// VisitedMap (distset.go:71-87) as an exact open-addressing hash set in LDS: a query marks a few thousand
// ids, so the set fits next to the wave and CheckAndVisit costs an LDS atomic instead of an HBM round
// trip.  Keys inserted by one instruction are distinct (rows are deduplicated), so the CAS loop only
// resolves slot collisions.  When the table fills past `limit` the set SPILLS: the wave clears its HBM
// bitset, replays every stored key into it and carries on there -- the set stays exact and the walk is
// not repeated (the reference makes the same kind of switch by id range, distset.go:140-153).
constexpr uint32_t kHashCap = 8192;    // plain store: 32 KB per wave -> 4 waves per CU
// (kHashLimit, the keys a table may hold before it spills -- any CAP: limit * CAP / 8192 -- is walk_args.h's)
constexpr uint32_t kHashCapPQ = 7417;  // quantized store: a prime, 29 KB, leaves room for the 8 KB LUT (M = 8)
#ifndef SDB_HASH_PROBES
#define SDB_HASH_PROBES 4  // 6 and 8 measured the same (tools/kernel_ab.py: 0.947 / 0.947 / 0.946 ms plain, 0.315 / 0.312 / 0.317 ms quantized)
#endif
constexpr int kProbes = SDB_HASH_PROBES;  // probe positions a round of the visited-set test reads at once
// CAP is a power of two (mask) or a prime (conditional subtract): either way every probe stride in
// [1, CAP) reaches every slot.
template <uint32_t CAP>
struct HashVisited {
  static constexpr bool kPow2 = (CAP & (CAP - 1)) == 0;
  static constexpr uint32_t kWords = (CAP + 3) & ~3u;  // LDS words reserved (16-byte multiple)
  uint32_t *tab;
  uint32_t *bits;
  uint32_t words, count, limit;
  bool spilled;
  __device__ __forceinline__ void init_nosync(uint32_t *lds, uint32_t *bitset, int lane, const SearchArgs &a) {
    tab = lds, bits = bitset, words = a.words_per_query;
    count = 0, spilled = false;
    limit = (uint32_t)(((uint64_t)a.hash_limit * CAP) >> 13);
    uint4 *t4 = reinterpret_cast<uint4 *>(lds);
    for (uint32_t i = lane; i < kWords / 4; i += 64) t4[i] = make_uint4(kNoSlot, kNoSlot, kNoSlot, kNoSlot);
  }
  __device__ __forceinline__ void spill(int lane) {
    for (uint32_t i = lane; i < words; i += 64) bits[i] = 0u;  // ClearAll distset.go:101
    __threadfence();                                           // the clears land before the atomics below
    for (uint32_t i = lane; i < CAP; i += 64) {
      const uint32_t k = tab[i];
      if (k != kNoSlot) atomicOr(&bits[k >> 5], 1u << (k & 31));
    }
    __threadfence();
    spilled = true;
  }
  // The probe-and-claim round, on a table alone: no count, no spill.  `cell` is where a new key went.  test_and_set runs
  // it on its own table; PlainWideDist's marker wave -- ANOTHER wave of the workgroup -- runs it on the walker's table
  // ahead of the walk, and the cells let the walker take the marks back should the walk not go there after all (unmark).
  // The walker stays away from the table meanwhile.
  static __device__ __forceinline__ bool claim(uint32_t *tab, bool active, uint32_t slot, uint32_t &cell) {
    bool isnew = false, done = !active;
    // double hashing: probe chains of different keys do not pile up the way linear probing clusters.
    // start = hash1 * CAP >> 32 in [0, CAP); stride in [1, CAP), odd for the power-of-two table
    uint32_t h = (uint32_t)(((uint64_t)(slot * 2654435761u) * CAP) >> 32);
    uint32_t step = 1u + (uint32_t)(((uint64_t)(slot * 0x9E3779B1u) * (CAP - 1)) >> 32);
    if (kPow2) step |= 1u;
    auto next = [&](uint32_t x) {
      x += step;
      if (kPow2) x &= CAP - 1;
      else if (x >= CAP) x -= CAP;
      return x;
    };
    cell = 0;
    // A round reads kProbes consecutive probe positions at once (one LDS round trip), takes the first that is
    // empty or already holds the key -- nothing is ever removed, so a key that is present sits before the
    // first empty position of its chain -- and only then spends the atomic: almost every lane finishes in one
    // round, where a compare-and-swap per probe made the whole wave wait for its longest chain.
    while (__ballot(!done)) {
      uint32_t hp[kProbes], kp[kProbes];
      hp[0] = h;
#pragma unroll
      for (int i = 1; i < kProbes; i++) hp[i] = next(hp[i - 1]);
#pragma unroll
      for (int i = 0; i < kProbes; i++) kp[i] = tab[hp[i]];
      bool any = false;
      uint32_t hs = hp[kProbes - 1], ks = kp[kProbes - 1];
#pragma unroll
      for (int i = kProbes - 1; i >= 0; i--) {
        const bool si = kp[i] == slot || kp[i] == kNoSlot;
        hs = si ? hp[i] : hs, ks = si ? kp[i] : ks;
        any |= si;
      }
      if (!done) {
        if (!any) {
          h = next(hp[kProbes - 1]);
        } else if (ks == slot) {
          done = true;
        } else {
          const uint32_t old = atomicCAS(&tab[hs], kNoSlot, slot);
          if (old == kNoSlot) isnew = true, done = true, cell = hs;
          else if (old == slot) done = true;
          else h = hs;  // another lane's key landed there in this round: carry on from it
        }
      }
    }
    return isnew;
  }
  __device__ __forceinline__ bool test_and_set(bool active, uint32_t slot, int lane) {
    if (spilled) return bitset_test_and_set(bits, active, slot);
    uint32_t cell;
    const bool isnew = claim(tab, active, slot, cell);
    count += (uint32_t)__popcll(__ballot(isnew));
    if (count > limit) spill(lane);  // at most 64 keys past the limit: the table never fills
    return isnew;
  }
  __device__ __forceinline__ bool markable() const { return !spilled; }
  // marks made by claim() on the walker's behalf: now part of the set ...
  __device__ __forceinline__ void credit(uint32_t n, int lane) {
    count += n;
    if (count > limit) spill(lane);  // at most 128 keys past the limit
  }
  // ... or taken back (nothing has been added since they were made: the table is as it was before them)
  __device__ __forceinline__ void unmark(bool mine, uint32_t cell) {
    if (mine) tab[cell] = kNoSlot;
    wave_lds_sync();
  }
};

// The same exact set in half the LDS, for stores of up to 2^24 rows: 16-bit cells.  h = slot * odd mod 2^24 is a
// bijection of the 24-bit universe; its top 12 bits name a bucket -- one 32-bit LDS word, two cells -- and its low
// 12 bits are the remainder a cell stores, next to the number (0..14) of the probe that placed the key: probe i of
// a key looks at bucket (b + i * (2 rem + 1)) mod 4096, double hashing over buckets with a stride the cell itself
// gives back.  Position and content of a cell therefore identify its key exactly -- nothing is a fingerprint --
// and spill() rebuilds every key.  The cells of a bucket fill low half first and nothing is ever removed, so a key
// that is present sits before the first bucket of its sequence that is not full.  A key that finds 15 full buckets
// (probability ~1e-7 at 60 % load), or a table past its limit, spills to the HBM bitset like HashVisited does.
// 8 192 cells = 16 KB: with the 8 KB LUT of M = 8 six walks fit a CU instead of four.
constexpr uint32_t inverse24(uint32_t a) {  // a * x = 1 mod 2^24, Newton steps double the correct bits
  uint32_t x = a;
  for (int i = 0; i < 5; i++) x *= 2u - a * x;
  return x & 0xFFFFFFu;
}
constexpr uint32_t kHash16Mul = 0x9E3779B1u & 0xFFFFFFu, kHash16Inv = inverse24(kHash16Mul);
static_assert(((kHash16Mul * kHash16Inv) & 0xFFFFFFu) == 1u, "kHash16Inv must invert kHash16Mul mod 2^24");
struct HashVisited16 {
  static constexpr uint32_t kBuckets = 4096, kCells = 2 * kBuckets;
  static constexpr uint32_t kWords = kBuckets;  // 32-bit LDS words
  static constexpr uint32_t kMaxProbe = 14;     // (probe 15, remainder 0xFFF) is the empty cell
  uint32_t *tab;
  uint32_t *bits;
  uint32_t words, count, limit, maxp;
  bool spilled;
  __device__ __forceinline__ void init_nosync(uint32_t *lds, uint32_t *bitset, int lane, const SearchArgs &a) {
    tab = lds, bits = bitset, words = a.words_per_query;
    count = 0, spilled = false;
    const uint32_t probes = a.hash16_probes;
    maxp = (probes >= 1 && probes <= kMaxProbe) ? probes - 1 : kMaxProbe;  // last probe number a key may use
    limit = (uint32_t)(((uint64_t)a.hash_limit * kCells) >> 13);  // 6 000 of 8 192 cells by default
    uint4 *t4 = reinterpret_cast<uint4 *>(lds);
    for (uint32_t i = lane; i < kWords / 4; i += 64) t4[i] = make_uint4(~0u, ~0u, ~0u, ~0u);
  }
  __device__ __forceinline__ void spill(int lane) {
    for (uint32_t i = lane; i < words; i += 64) bits[i] = 0u;  // ClearAll distset.go:101
    __threadfence();
    for (uint32_t c = lane; c < kCells; c += 64) {
      const uint32_t v = (tab[c >> 1] >> ((c & 1u) * 16u)) & 0xFFFFu;
      if (v != 0xFFFFu) {
        const uint32_t rem = v & 0xFFFu, probe = v >> 12;
        const uint32_t b = ((c >> 1) - probe * (2u * rem + 1u)) & (kBuckets - 1);
        const uint32_t k = (((b << 12) | rem) * kHash16Inv) & 0xFFFFFFu;
        atomicOr(&bits[k >> 5], 1u << (k & 31));
      }
    }
    __threadfence();
    spilled = true;
  }
  __device__ __forceinline__ bool test_and_set(bool active, uint32_t slot, int lane) {
    if (spilled) return bitset_test_and_set(bits, active, slot);
    const uint32_t h = (slot * kHash16Mul) & 0xFFFFFFu;
    const uint32_t rem = h & 0xFFFu, step = 2u * rem + 1u;
    uint32_t bucket = h >> 12, probe = 0;
    bool isnew = false, done = !active, stuck = false;
    // a round reads kProbes buckets of the sequence at once and takes the first that holds the key or has room
    while (__ballot(!done)) {
      uint32_t bp[kProbes], wp[kProbes];
      bp[0] = bucket;
#pragma unroll
      for (int i = 1; i < kProbes; i++) bp[i] = (bp[i - 1] + step) & (kBuckets - 1);
#pragma unroll
      for (int i = 0; i < kProbes; i++) wp[i] = tab[bp[i]];
      int hit = -1;  // first bucket of this round that ends the search
      bool present = false;
#pragma unroll
      for (int i = kProbes - 1; i >= 0; i--) {
        const uint32_t target = rem | ((probe + i) << 12);
        const bool has = (wp[i] & 0xFFFFu) == target || (wp[i] >> 16) == target;
        const bool room = (wp[i] >> 16) == 0xFFFFu;
        if ((has || room) && probe + i <= maxp) hit = i, present = has;
      }
      if (!done) {
        if (hit < 0) {
          probe += kProbes;
          if (probe > maxp) done = stuck = true;
          else bucket = (bp[kProbes - 1] + step) & (kBuckets - 1);
        } else if (present) {
          done = true;
        } else {
          uint32_t old = wp[0], at = bp[0];
#pragma unroll
          for (int i = 1; i < kProbes; i++)
            if (hit == i) old = wp[i], at = bp[i];
          const uint32_t target = rem | ((probe + (uint32_t)hit) << 12);
          const uint32_t neu = (old & 0xFFFFu) == 0xFFFFu ? ((old & 0xFFFF0000u) | target) : ((old & 0xFFFFu) | (target << 16));
          if (atomicCAS(tab + at, old, neu) == old) isnew = true, done = true;
          else probe += (uint32_t)hit, bucket = at;  // another lane's key took a cell of that bucket: look at it again
        }
      }
    }
    count += (uint32_t)__popcll(__ballot(isnew));
    const uint64_t st = __ballot(stuck);
    if (st || count > limit) {
      spill(lane);
      if (stuck) isnew = bitset_test_and_set(bits, true, slot);  // after the replay: the set is the bitset now
    }
    return isnew;
  }
};

// the unfiltered search has no result set of its own
struct NoVisited {
  __device__ __forceinline__ bool test_and_set(bool, uint32_t, int) { return false; }
};
// The filtered search's resultSet has a visited set of its own (search.go:37: NewDistSet(k, ...)): it sees the seeds
// (<= searchSize ids) and the expanded nodes that pass the filter -- a few hundred ids at most, so a 1 024-entry table
// (4 KB) next to the search set's; past 750 ids it spills to its HBM bitset like the big one does.
constexpr uint32_t kHashCapResult = 1024;

// The walk kernels' HCAP parameter names the policy: 0 the HBM bitset from the start, kHash16 the 16-bit-cell set, any
// other value the capacity of HashVisited.  kWords: the LDS words the set takes, first in dynamic LDS.
constexpr uint32_t kHash16 = 0xFFFFFFFFu;
template <uint32_t HCAP>
struct VisitedFor {
  typedef HashVisited<HCAP> type;
  static constexpr uint32_t kWords = type::kWords;
};
template <>
struct VisitedFor<0> {
  typedef BitVisited type;
  static constexpr uint32_t kWords = 0;
};
template <>
struct VisitedFor<kHash16> {
  typedef HashVisited16 type;
  static constexpr uint32_t kWords = HashVisited16::kWords;
};

}  // namespace sdb
