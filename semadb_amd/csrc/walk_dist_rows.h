// walk_dist_rows.h -- K2: the distance policies over stored rows (PlainDist, Int8Dist, PlainWideDist).
// (a part of search_kernel.h, which includes it after what it builds on; no .hip file includes it directly)
#pragma once

namespace sdb {

// ---- distance policies: what vecStore.DistanceFromFloat(query) binds (plain.go:76-85 / product.go:238-277)

// Full-precision store.  NG >= 0: compile-time group count, query in registers.  NG == -1: run-time
// ng, query tile in LDS.
template <int NG, bool L2, bool DEEP = false, int UPAIRS = 0, Stage ST = Stage::kNone>  // UPAIRS != 0: that many pairs of rows per chunk; ST: two-precision hop
struct PlainDist {
  static constexpr Stage kStage = ST;
  static constexpr bool kHasStamps = true;
  static constexpr bool kPointDistances = true;  // dist(query, row) is distFn between two stored vectors
  // search_body: nothing is worked ahead on between the hops.  (Round 5 tried the walker's naming of the next hop's row
  // here too -- its adjacency row asked for under AddWithLimit, a round trip less per hop in the batch's tail: 0.983
  // against 0.975 ms per batch, the naming's ~300 instructions per hop cost a lone wave more than the hidden latency.
  // The cheap half -- no naming, only the adjacency row of the array's first unvisited entry asked for before
  // AddWithLimit and taken from the register when the walk does go there -- made no difference at all: 0.955 / 0.958 /
  // 0.957 against 0.957 / 0.954 / 0.973 ms in alternating runs; the batch walk is bound by bytes, not by a wave's round trips.)
  // ... with the two-precision hop the walk IS bound by its round trips; naming the next hop's adjacency row and asking
  // for it before AddWithLimit runs (search_body's kSpeculate path without the small-call kernel's marker wave) was
  // measured there too: 0.716 against 0.722 ms (min of 10), within the noise -- the naming costs about what the hidden
  // round trip saves.  Off.
  // ... and on the int8 walk WITHOUT naming anything: both rows the next hop can go to -- the array's first unvisited
  // entry as it stands, and the nearest new point (a wave minimum by DPP, one ballot) -- asked for before AddWithLimit
  // and taken from the register when the walk goes there, which it does in 0.987 of the hops.  Per hop the adjacency
  // row fell from 1 468 to 481 cycles and AddWithLimit ROSE from 3 038 to 4 283 (the hop 13 117 -> 13 351): this
  // compiler waits for the two loads (s_waitcnt vmcnt(0)) at the first instruction of AddWithLimit that overwrites the
  // temporary their address was computed in, with a scalar base and a long-lived offset register too, so the round
  // trip moved and did not vanish, and the ~75 instructions of asking were added.  bench.py 2.059 - 2.079 M queries/s
  // against 2.121 - 2.141 M, five alternating runs: a loss.  Left out (HISTORY.md).
  static constexpr bool kSpeculate = false;
  static constexpr bool marked = false;  // (no marker wave: nothing is tested ahead)
  __device__ __forceinline__ void take_marks(int, uint64_t &, uint32_t &) {}
  static constexpr int NGR = NG > 0 ? NG : 1;
  static constexpr int U = UPAIRS ? UPAIRS : (NG >= 0 ? ChunkPairs<NG, DEEP>::value : 4);
  // dynamic LDS of the policy: NG == -1 the query tile; NG >= 0 the hop scratch -- pending slots by rank
  // [kHopSlots], raw distances by rank [kHopSlots], a UX-word dump (UX: the float16 stage's rounds may be longer than U)
  static constexpr int stage_round() {
    if constexpr (ST == Stage::kHalf) return HalfRows<NG, L2>::kRound;
    return 0;
  }
  static constexpr int UX = U > stage_round() ? U : stage_round();
  static constexpr uint32_t kHopSlots = 64 + UX;  // ranks 0..63 and the overrun of the last half-wave run
  static constexpr size_t kLdsBytes = NG >= 0 ? (2 * kHopSlots + UX) * sizeof(uint32_t) : 0;
  float4 xq[NGR];
  float xt;
  float *qs;
  uint32_t *hs;
  typename StageOf<NG, L2, ST>::type stage;
#ifdef SDB_STAMPS
  unsigned long long st[3] = {0, 0, 0};  // issue, wait, compute
#endif

  __device__ __forceinline__ void init(const SearchArgs &a, uint32_t q, int lane, float *lds) {
    const int L = lane & 31;
    const float *__restrict__ qv = a.queries + (size_t)q * a.dim;
    qs = lds;
    hs = reinterpret_cast<uint32_t *>(lds);
    xt = 0.0f;
    if constexpr (NG >= 0) {
#pragma unroll
      for (int g = 0; g < NG; g++)
        xq[g] = make_float4(q_elem(qv, a.nblk, g, 0, L), q_elem(qv, a.nblk, g, 1, L),
                            q_elem(qv, a.nblk, g, 2, L), q_elem(qv, a.nblk, g, 3, L));
      if (NG == 0) xq[0] = make_float4(0.f, 0.f, 0.f, 0.f);
      xt = (a.tail && (uint32_t)L < a.tail) ? qv[a.nblk * 32 + L] : 0.0f;
      if constexpr (ST == Stage::kHalf) stage.init(a, xq, lane);
    } else {
      for (uint32_t i = lane; i < a.ng * 128; i += 64) {
        uint32_t g = i / 128, r = i % 128;
        qs[i] = q_elem(qv, a.nblk, g, r % 4, (int)(r / 4));
      }
      if (a.tail && lane < 32) qs[a.ng * 128 + lane] = (uint32_t)lane < a.tail ? qv[a.nblk * 32 + lane] : 0.0f;
      __syncthreads();
    }
  }

  __device__ __forceinline__ void chunk(const SearchArgs &a, const uint32_t (&slot)[U], float (&res)[U], int lane) {
#ifdef SDB_STAMPS
    if constexpr (NG >= 0) chunk_dist<NG, L2, U>(a.slab, a.ld, a.tail, xq, xt, slot, res, lane, st);
    else chunk_dist_lds<L2, U>(a.slab, a.ld, a.ng, a.tail, qs, slot, res, lane);
#else
    if constexpr (NG >= 0) chunk_dist<NG, L2, U>(a.slab, a.ld, a.tail, xq, xt, slot, res, lane);
    else chunk_dist_lds<L2, U>(a.slab, a.ld, a.ng, a.tail, qs, slot, res, lane);
#endif
  }

  // distance to one row (wave-uniform result)
  __device__ __forceinline__ float one(const SearchArgs &a, uint32_t s, int lane) {
    uint32_t slot[U];
    float res[U];
#pragma unroll
    for (int u = 0; u < U; u++) slot[u] = s;
    chunk(a, slot, res, lane);
    return metric_finish(rlf(res[0], 0), a.metric);
  }

  // search_body's hooks of the two-precision hop: a hop's copy rows asked for, and the verdict.  These two are the
  // float16 stage's; with ST == Stage::kInt8 this class holds no stage and is only Int8Dist's base, which brings its own
  // (used directly, these two would not compile: NoStage has no begin / keep).
  __device__ __forceinline__ void stage_begin(const SearchArgs &a, uint32_t nb, bool valid, bool full) { stage.begin(a, nb, valid, full); }
  __device__ __forceinline__ uint64_t stage_keep(const SearchArgs &a, uint32_t nb, uint64_t pend, int lane, float tail_d, uint64_t &out) {
    return stage.keep(a, hs, kHopSlots, nb, pend, lane, tail_d, out);
  }
  __device__ __forceinline__ void prefetch(const SearchArgs &, uint32_t, bool) {}  // float32 rows are fetched in hop()
  __device__ __forceinline__ void speculation(bool, const uint32_t *) {}
  __device__ __forceinline__ void ahead(const SearchArgs &, const uint32_t *, int, bool) {}
  // hooks of the multi-wave quantized walk (PQWideDist); nothing to do for a one-wave policy
  __device__ __forceinline__ void begin_row(const SearchArgs &, const uint32_t *, int) {}
  __device__ __forceinline__ void skip(int) {}

  // The hop with the per-row instruction count cut to the arithmetic: the pending slots are compacted into LDS by rank (mbcnt), each
  // half-wave takes a contiguous run of them (so a lane fetches its 16 slots with plain ds_reads, no bit
  // scans or readlanes), a row address is ONE v_mad_u64_u32 (slot * row bytes + [slab + 16 * L]), the raw
  // distance leaves lane 0 of its half through one ds_write at the row's rank, and every pending lane reads
  // its own rank back.  With one wave per SIMD an instruction of any kind costs an issue slot, so this is
  // where the kernel's time was.  Rows beyond an odd count are read twice (one spare entry behind the
  // list); their results land behind the ranks anybody reads.
  // TAIL (dim % 32 != 0, e.g. 100, 784): the sequential scalar chain over the tail elements (dot.s:35-43)
  // runs in lane 0 of each half -- the query element comes from a readlane (once per element, shared by all
  // rows of the chunk), the row's elements walk down to lane 0 with one wave_shl DPP move per step.
  // raw distances of the pending rows of ranks [first, first + count) of the list in s_slot (one spare entry behind its
  // last rank), two rows per wave instruction, into s_res by rank.  `first` is even.
  // ALL: every one of the U row slots of a round is loaded and summed, the ones past the range as copies of its last row
  // (their sums go to the dump) -- no branch between the rows, so that all loads of a round are in flight at once.  (With
  // the rows conditional, as the one-wave kernels have them, the compiler here -- inside the multi-wave kernels -- placed
  // each row's wait and arithmetic right behind its three loads: one memory round trip PER ROW, three in sequence for a
  // wave's six rows ahead.)
  template <bool TAIL, bool ALL = false>
  __device__ __forceinline__ void rows_range(const SearchArgs &a, const uint32_t *s_slot, float *s_res, int first, int count,
                                             int lane) {
    const int L = lane & 31, half = lane >> 5;
    const char *baseL = reinterpret_cast<const char *>(a.slab) + L * 16;
    const uint32_t row_bytes = a.ld * 4u;
    const int cnt = first + count;
    for (int c0 = first; c0 < cnt; c0 += 2 * U) {
      const int m = cnt - c0 < 2 * U ? cnt - c0 : 2 * U;
      const int h0 = (m + 1) >> 1;  // rows of half 0; half 1 takes the other m - h0 (+ the spare when m is odd)
      const int base = c0 + (half ? h0 : 0);
#ifdef SDB_STAMPS
      unsigned long long t0 = __builtin_amdgcn_s_memtime();
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#endif
      uint32_t sl[U];
#pragma unroll
      for (int u = 0; u < U; u++) sl[u] = s_slot[base + (ALL ? (u < h0 ? u : h0 - 1) : u)];
      float4 y[U][NGR];
#pragma unroll
      for (int u = 0; u < U; u++)
        if (ALL || u < h0) {
          const float4 *r4 = reinterpret_cast<const float4 *>(baseL + (uint64_t)sl[u] * row_bytes);
#pragma unroll
          for (int g = 0; g < NG; g++) y[u][g] = r4[g * 32];
        }
      float yt[TAIL ? U : 1];
      if constexpr (TAIL) {
        const char *baseT = reinterpret_cast<const char *>(a.slab) + (NG * 128 + L) * 4;
#pragma unroll
        for (int u = 0; u < U; u++) {
          yt[u] = 0.0f;
          if (ALL || u < h0) yt[u] = *reinterpret_cast<const float *>(baseT + (uint64_t)sl[u] * row_bytes);
        }
      }
#ifdef SDB_STAMPS
      unsigned long long t1 = __builtin_amdgcn_s_memtime();
      asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
      unsigned long long t2 = __builtin_amdgcn_s_memtime();
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#endif
      float *wp = (L == 0) ? s_res + base : s_res + kHopSlots;  // the other lanes write to a dump
      if constexpr (!TAIL) {
#pragma unroll
        for (int u = 0; u < U; u++)
          if (ALL || u < h0) {
            float acc = 0.0f;
#pragma unroll
            for (int g = 0; g < NG; g++) acc = chain4<L2>(acc, xq[g], y[u][g]);
            const float r = asm_reduce(acc, 0.0f, lane);
            if constexpr (ALL) (u < h0 ? wp : s_res + kHopSlots)[u] = r;
            else wp[u] = r;
          }
      } else {
        float acc[U], t[U];
#pragma unroll
        for (int u = 0; u < U; u++) {
          acc[u] = 0.0f, t[u] = 0.0f;
          if (ALL || u < h0) {
#pragma unroll
            for (int g = 0; g < NG; g++) acc[u] = chain4<L2>(acc[u], xq[g], y[u][g]);
          }
        }
        for (uint32_t i = 0; i < a.tail; i++) {
          const float xi = rlf(xt, (int)i);  // both halves hold the query's tail in lanes 0..31
#pragma unroll
          for (int u = 0; u < U; u++) {
            t[u] = chain1<L2>(t[u], xi, yt[u]);  // lane 0 of each half: element i of its row
            yt[u] = __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(yt[u]), 0x130, 0xf, 0xf, true));
          }
        }
#pragma unroll
        for (int u = 0; u < U; u++)
          if (ALL || u < h0) {
            const float r = asm_reduce(acc[u], t[u], lane);
            if constexpr (ALL) (u < h0 ? wp : s_res + kHopSlots)[u] = r;
            else wp[u] = r;
          }
      }
#ifdef SDB_STAMPS
      unsigned long long t3 = __builtin_amdgcn_s_memtime();
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      st[0] += t1 - t0, st[1] += t2 - t1, st[2] += t3 - t2;  // issue, wait, compute
#endif
    }
  }

  template <bool TAIL>
  __device__ __forceinline__ float hop_fast(const SearchArgs &a, uint32_t nb, uint64_t pend, int lane) {
    const int cnt = __popcll(pend);
    const bool mine = (pend >> lane) & 1ull;
    const uint32_t rank =
        __builtin_amdgcn_mbcnt_hi((uint32_t)(pend >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)pend, 0u));
    uint32_t *s_slot = hs;
    float *s_res = reinterpret_cast<float *>(hs + kHopSlots);
    if (mine) {
      s_slot[rank] = nb;
      if ((int)rank == cnt - 1) s_slot[cnt] = nb;  // the spare entry
    }
    wave_lds_sync();
    rows_range<TAIL>(a, s_slot, s_res, 0, cnt, lane);
    wave_lds_sync();
    return mine ? metric_finish(s_res[rank], a.metric) : 0.0f;
  }

  // distances of the new neighbours of one hop: lane j (bit j of pend) gets dist(query, row nb_j)
  __device__ __forceinline__ float hop(const SearchArgs &a, uint32_t nb, uint64_t pend, int lane) {
    if constexpr (NG >= 0) return a.tail ? hop_fast<true>(a, nb, pend, lane) : hop_fast<false>(a, nb, pend, lane);
    float mydist = 0.0f;
    uint64_t todo = pend;
    while (todo) {
      int jj[2 * U];
#pragma unroll
      for (int i = 0; i < 2 * U; i++) {
        if (todo) {
          jj[i] = __ffsll((unsigned long long)todo) - 1;
          todo &= todo - 1;
        } else {
          jj[i] = jj[i > 0 ? i - 1 : 0];
        }
      }
      uint32_t slot[U];
      float res[U];
#pragma unroll
      for (int u = 0; u < U; u++) {
        uint32_t s0 = rl(nb, jj[2 * u]), s1 = rl(nb, jj[2 * u + 1]);
        slot[u] = lane < 32 ? s0 : s1;
      }
      chunk(a, slot, res, lane);
#pragma unroll
      for (int u = 0; u < U; u++) {
        float d0 = metric_finish(rlf(res[u], 0), a.metric);
        float d1 = metric_finish(rlf(res[u], 32), a.metric);
        if (lane == jj[2 * u]) mydist = d0;
        if (lane == jj[2 * u + 1]) mydist = d1;
      }
    }
    return mydist;
  }
};

// The walk with the int8 first stage.  A subclass, not a third choice of PlainDist's `stage` member: held as that member
// the same code takes 229 registers at NG = 3, here 228 (this compiler's allocation follows the object's layout).  It adds
// the stage's state and the three calls that reach it; everything else, the float32 stage included, is the base's.
template <int NG>
struct Int8Dist : PlainDist<NG, false, true, 4, Stage::kInt8> {
  using Base = PlainDist<NG, false, true, 4, Stage::kInt8>;
  FirstStage<Int8Rows<NG>, false, true> rows8;
  __device__ __forceinline__ void init(const SearchArgs &a, uint32_t q, int lane, float *lds) {
    Base::init(a, q, lane, lds);
    rows8.init(a, this->xq, lane);
  }
  __device__ __forceinline__ void stage_begin(const SearchArgs &a, uint32_t nb, bool valid, bool full) { rows8.begin(a, nb, valid, full); }
  __device__ __forceinline__ uint64_t stage_keep(const SearchArgs &a, uint32_t nb, uint64_t pend, int lane, float tail_d, uint64_t &out) {
    return rows8.keep(a, this->hs, Base::kHopSlots, nb, pend, lane, tail_d, out);
  }
};

// The same store walked by a WORKGROUP per query, for calls with few queries (a single REST request is one query,
// vamana.go:278-310): one wave per query leaves most of the chip idle and a hop costs two dependent memory round trips
// plus the issue time of ~50 rows' loads on one SIMD.  Here wave 0 is the walker -- search_body as it stands: candidate
// array, visited set, AddWithLimit -- and a hop's pending rows are split over all W waves of the workgroup: the walker
// publishes the rank-compacted slot list (the one hop_fast builds anyway), every wave takes a contiguous share of it,
// two rows per instruction, and leaves the raw sums at the rows' ranks; the walker reads them back.  Same pairs, same
// arithmetic, same bits, same visit order; two workgroup barriers per hop.
constexpr uint32_t kWideAheadPad = 24;  // spare entry + rows_range's dump behind the 64 positions (kHopSlots = 64 + U, U <= 8)
// The walker talks to the other waves in WORDS: it fills the fields, then raises `word` by one; a wave that is through
// with the last word spins on it.  The walker sends a word only when every other wave has taken the one before -- it
// has waited for their completion counts by then -- so a field is never overwritten under a reader.
constexpr uint32_t kWordShare = 1u;  // `cnt` pending rows are listed: take your share (one barrier behind it)
constexpr uint32_t kWordAhead = 2u;  // `ahead` is the adjacency row of the candidate the walk expands next: work ahead on it
constexpr uint32_t kWordDone = 3u;   // the walk is over
struct WideShared {
  uint32_t word;       // words sent, ever (monotonic)
  uint32_t kind;       // what the last one says
  uint32_t cnt;        // kWordShare: pending rows of the hop
  uint32_t mark_on;    // kWordAhead: != 0: the marker wave runs the visited-set test of that row's neighbours
  unsigned long long ahead;  // kWordAhead: the row
  uint32_t ahead_done; // rows ahead the computing waves are through with, times their number (monotonic)
  uint32_t mark_seq;   // kWordAhead words the marker is through with (monotonic)
  unsigned long long mark_pend;  // the neighbours (by edge position) that were new to the visited set
  uint32_t mark_cell[64];        // where each of those went in the table
  uint32_t ahead_slot[64 + kWideAheadPad];  // that row's slots by edge position
  float ahead_res[64 + kWideAheadPad];      // raw sums of distFn(query, neighbour) by edge position
};

// pairs of rows per round of loads: a wave's share of a hop is at most 64 / W rows (rounded up to even), so 32 / W pairs
// hold it -- but its share of the distances AHEAD is 6 rows at W = 16 (14 waves compute): three pairs where the registers
// allow it (rows of up to 512 floats; 128 registers per wave at 16 waves)
// -- euclidean from 384 floats up stays at two: its separately rounded differences are live beside the rows, and the
// third pair spilled (1 register at 384 floats, 33 .. 69 at 512; tools/kernel_table.py --check holds every walk kernel
// to zero scratch)
template <int NG, int W, bool L2>
struct WidePairs {
  static constexpr int kMin = 32 / W > 0 ? 32 / W : 1;
  static constexpr int value = (kMin < 3 && (NG <= 2 || (NG <= 4 && !L2))) ? 3 : kMin;
};
template <int NG, bool L2, int W>
struct PlainWideDist : PlainDist<NG, L2, true, WidePairs<NG, W, L2>::value> {
  using Base = PlainDist<NG, L2, true, WidePairs<NG, W, L2>::value>;
  // A call of few queries has bandwidth to spare and a dependent chain to shorten.  Once a hop's distances are known, so
  // is the candidate the walk expands next (search_body, Dist::kSpeculate: 99 % of the hops expand exactly it) -- BEFORE
  // the hop's points are inserted.  The walker names it there (a.wide_pull = 2), and while it inserts
  //   * the marker (wave 1) runs the visited-set test of that candidate's neighbours on the walker's table,
  //   * the computing waves (2 .. W-1) COMPUTE the raw distances to all of its neighbours, by edge position,
  // so that the next hop starts with its adjacency row in a register, its CheckAndVisit verdict and its distances in LDS:
  // what is left of it is AddWithLimit.  Nothing is decided on a guess: should the walk go elsewhere (a tie, a NaN, the
  // start node's overflow list), the marks are taken back, the rows are shared out the plain way (kWordShare), and the
  // guess has cost traffic.  Same pairs, same arithmetic, same bits, same visit order.
  static constexpr bool kSpeculate = true;
  static constexpr size_t kLdsBytes = Base::kLdsBytes + sizeof(WideShared);
  // Wave 1 is the MARKER (W >= 4): CheckAndVisit marks before any distance is looked at (distset.go:174) and nothing else
  // touches the set between the naming and the next hop, so the marks are exactly the ones the walker's own test would
  // have made.  Waves kFirstAhead .. W-1 compute the distances ahead.
  static constexpr int kFirstAhead = W >= 4 ? 2 : 1;
  static constexpr int kAheadWaves = W - kFirstAhead;
  static constexpr int kAheadPer = ((64 + kAheadWaves - 1) / kAheadWaves + 1) & ~1;  // rows ahead per computing wave (even)
  WideShared *sh;
  int wave;
  bool hit_cur;         // walker: this hop expands the candidate named one hop ago, and its distances were computed ahead
  bool ahead_computed;  // walker: the last hop named a row
  bool marked;          // walker: ... and the marker was sent through it
  uint32_t ahead_expect;  // walker: value of sh->ahead_done once every computing wave is through with what was named
  uint32_t mark_expect;   // walker: value of sh->mark_seq once the marker is
  uint32_t words;         // words sent (walker) / taken (the others)
  SearchArgs const *args_;
#ifdef SDB_STAMPS
  unsigned long long t_named = 0;
#endif
  __device__ __forceinline__ void init_wave(const SearchArgs &a, uint32_t q, int lane, int w, float *lds) {
    Base::init(a, q, lane, lds);  // every wave keeps the query in its registers
    sh = reinterpret_cast<WideShared *>(reinterpret_cast<char *>(lds) + Base::kLdsBytes);
    wave = w, args_ = &a;
    hit_cur = false, ahead_computed = false, marked = false, ahead_expect = 0, mark_expect = 0, words = 0;
    if (w == 0 && lane == 0) sh->word = 0, sh->ahead_done = 0, sh->mark_seq = 0, sh->mark_on = 0;
  }
  __device__ __forceinline__ void speculation(bool use, const uint32_t *) { hit_cur = use && ahead_computed; }

  // ---- the walker (wave 0)
  // every other wave is through with the last word (and spins for the next)
  __device__ __forceinline__ void quiesce() {
    while (__atomic_load_n(&sh->ahead_done, __ATOMIC_RELAXED) != ahead_expect) __builtin_amdgcn_s_sleep(1);
    if (kFirstAhead == 2)
      while (__atomic_load_n(&sh->mark_seq, __ATOMIC_RELAXED) != mark_expect) __builtin_amdgcn_s_sleep(1);
  }
  __device__ __forceinline__ void send(uint32_t kind, int lane) {  // the fields are written (lane 0)
    words++;
    if (lane == 0) {
      sh->kind = kind;
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
      __atomic_store_n(&sh->word, words, __ATOMIC_RELAXED);
    }
  }
  // The walker's word on the row to work ahead on, once per hop and AFTER the hop's distances are known (search_body).
  __device__ __forceinline__ void ahead(const SearchArgs &a, const uint32_t *rowp, int lane, bool markable) {
    ahead_computed = a.wide_pull == 2 && rowp != nullptr;
    marked = ahead_computed && markable && kFirstAhead == 2;
    if (!ahead_computed) return;
    quiesce();
#ifdef SDB_STAMPS
    t_named = __builtin_amdgcn_s_memtime();
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#endif
    ahead_expect += (uint32_t)kAheadWaves;
    if (kFirstAhead == 2) mark_expect++;
    if (lane == 0) sh->mark_on = marked ? 1u : 0u, sh->ahead = reinterpret_cast<unsigned long long>(rowp);
    send(kWordAhead, lane);
  }
  // what the marker found for the row named last: the neighbours that were new to the set, and where they went
  __device__ __forceinline__ void take_marks(int lane, uint64_t &mask, uint32_t &cell) {
    while (__atomic_load_n(&sh->mark_seq, __ATOMIC_RELAXED) != mark_expect) __builtin_amdgcn_s_sleep(1);
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
    mask = sh->mark_pend;
    cell = sh->mark_cell[lane];
    marked = false;
  }
  // this wave's share of `cnt` pending rows: contiguous ranks, an even number per wave so that only the list's last row
  // can be the odd one out (its spare entry sits behind the list)
  __device__ __forceinline__ void share(const SearchArgs &a, int cnt, int lane) {
    const int per = (((cnt + W - 1) / W) + 1) & ~1;
    const int first = wave * per;
    const int count = cnt - first < per ? cnt - first : per;
    if (count <= 0) return;
    uint32_t *s_slot = this->hs;
    float *s_res = reinterpret_cast<float *>(this->hs + Base::kHopSlots);
    if (a.tail) this->template rows_range<true, true>(a, s_slot, s_res, first, count, lane);
    else this->template rows_range<false, true>(a, s_slot, s_res, first, count, lane);
  }
  __device__ __forceinline__ float hop(const SearchArgs &a, uint32_t nb, uint64_t pend, int lane) {
    const int cnt = __popcll(pend);
    const bool mine = (pend >> lane) & 1ull;
    if (hit_cur) {  // this row's distances were computed while the last hop's points were inserted: by edge position
      hit_cur = false;
#ifdef SDB_STAMPS  // st[2]: from naming the row to needing its distances (the walker's own work); st[0]: waiting for them
      const unsigned long long w0 = __builtin_amdgcn_s_memtime();
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      this->st[2] += w0 - t_named;
#endif
      while (__atomic_load_n(&sh->ahead_done, __ATOMIC_RELAXED) != ahead_expect) __builtin_amdgcn_s_sleep(1);
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
      const float raw = sh->ahead_res[lane];
#ifdef SDB_STAMPS
      asm volatile("" ::"v"(raw));
      const unsigned long long w1 = __builtin_amdgcn_s_memtime();
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      this->st[0] += w1 - w0;
#endif
      return mine ? metric_finish(raw, a.metric) : 0.0f;
    }
    const uint32_t rank =
        __builtin_amdgcn_mbcnt_hi((uint32_t)(pend >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)pend, 0u));
    uint32_t *s_slot = this->hs;
    float *s_res = reinterpret_cast<float *>(this->hs + Base::kHopSlots);
    quiesce();  // the others may still be at a row the walk did not go to
    if (mine) {
      s_slot[rank] = nb;
      if ((int)rank == cnt - 1) s_slot[cnt] = nb;  // the spare entry
    }
    if (lane == 0) sh->cnt = (uint32_t)cnt;
    send(kWordShare, lane);
    share(a, cnt, lane);
    __syncthreads();  // every share has been written
    return mine ? metric_finish(s_res[rank], a.metric) : 0.0f;
  }
  __device__ __forceinline__ void skip(int) { hit_cur = false; }  // a chunk without a new neighbour: nothing to share
  __device__ __forceinline__ void finish(int lane) {
    quiesce();
    send(kWordDone, lane);
  }

  // ---- waves 1 .. W-1
  // a computing wave's share of the distances to the neighbours of the candidate ahead
  __device__ __forceinline__ void compute_ahead(const SearchArgs &a, const __attribute__((address_space(1))) uint32_t *rowp, int lane) {
    const uint32_t nb = rowp[lane];
    const uint64_t m = __ballot(nb != kNoSlot);
    const int deg = __popcll(m);  // rows are padded with kNoSlot behind their edges
    sh->ahead_slot[lane] = nb != kNoSlot ? nb : 0u;  // every computing wave writes the same words
    if (lane == deg - 1) sh->ahead_slot[deg] = nb;  // the spare entry behind the list
    wave_lds_sync();
    const int first = (wave - kFirstAhead) * kAheadPer;
    const int count = deg - first < kAheadPer ? deg - first : kAheadPer;
    if (count > 0) {
      if (a.tail) this->template rows_range<true, true>(a, sh->ahead_slot, sh->ahead_res, first, count, lane);
      else this->template rows_range<false, true>(a, sh->ahead_slot, sh->ahead_res, first, count, lane);
    }
    wave_lds_sync();  // the sums before the count
    if (lane == 0) {
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
      atomicAdd(&sh->ahead_done, 1u);
    }
  }
  template <class HV>  // HV: the walker's visited set (its table is `tab`)
  __device__ __forceinline__ void serve(const SearchArgs &a, int lane, uint32_t *tab) {
#ifdef SDB_STAMPS  // per wave: waiting for a word, the shares, the work ahead
    unsigned long long hs_word = 0, hs_share = 0, hs_work = 0, hs_n = 0;
#define SDB_HSTAMP(acc)                                         \
  {                                                             \
    unsigned long long _t = __builtin_amdgcn_s_memtime();       \
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory"); \
    acc += _t - hs_t0;                                          \
    hs_t0 = _t;                                                 \
  }
    unsigned long long hs_t0 = __builtin_amdgcn_s_memtime();
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#else
#define SDB_HSTAMP(acc)
#endif
    for (;;) {
      words++;
      while (__atomic_load_n(&sh->word, __ATOMIC_RELAXED) != words) __builtin_amdgcn_s_sleep(1);
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
      SDB_HSTAMP(hs_word)
      const uint32_t kind = sh->kind;
      if (kind == kWordDone) {
#ifdef SDB_STAMPS
        if (lane == 0 && a.tr_visit && a.visit_cap >= 44) a.tr_visit[(size_t)blockIdx.x * a.visit_cap + 28 + wave] = hs_work;
        if (lane == 0 && (wave == 1 || wave == 2) && a.tr_visit && a.visit_cap >= 24) {
          uint64_t *o = a.tr_visit + (size_t)blockIdx.x * a.visit_cap + (wave == 1 ? 12 : 18);
          o[0] = 0, o[1] = hs_share, o[2] = hs_word, o[3] = hs_work, o[4] = hs_n, o[5] = 0;
        }
#endif
        return;
      }
      if (kind == kWordShare) {
        share(a, (int)sh->cnt, lane);
        __syncthreads();
        SDB_HSTAMP(hs_share)
        continue;
      }
#ifdef SDB_STAMPS
      hs_n++;
#endif
      const auto *ahead = as_global(reinterpret_cast<const uint32_t *>(sh->ahead));  // (an adjacency row: device memory)
      if (kFirstAhead == 2 && wave == 1) {
        if (sh->mark_on) {
          const uint32_t nb = ahead[lane];
          uint32_t cell;
          const bool isnew = HV::claim(tab, nb != kNoSlot, nb, cell);
          const uint64_t pend = __ballot(isnew);
          sh->mark_cell[lane] = cell;
          if (lane == 0) sh->mark_pend = pend;
          wave_lds_sync();
        }
        n_ahead++;
        if (lane == 0) {
          __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
          __atomic_store_n(&sh->mark_seq, n_ahead, __ATOMIC_RELAXED);
        }
      } else {
        compute_ahead(a, ahead, lane);
      }
      SDB_HSTAMP(hs_work)
    }
  }
  uint32_t n_ahead = 0;  // marker: kWordAhead words it is through with
};

}  // namespace sdb
