// The walk's routing decision (semadb_amd/csrc/walk_plan.h) as plain C++, no HIP: tests/test_walk_plan.py builds this
// once plainly and once under AddressSanitizer + UBSan and runs it as a stand-alone program.
//
//   test_walk_plan plans FILE   one call per line of FILE as "key=value ..." (the routing-relevant fields that
//                               tools/walk_routes.py records beside every entry of tests/golden/walk_routes.json);
//                               prints the call's plan the same way, for the Python side to hold against the kernel
//                               that the GPU run recorded
//   test_walk_plan checks       what a tiny table cannot reach: the 2^24-row boundary of the 16-bit-cell visited set
//                               (expected policies stated by hand below) and a grid over ng x searchSize x filter x
//                               stage x knobs
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <map>
#include <sstream>
#include <string>

#include "../../semadb_amd/csrc/walk_args.h"
#include "../../semadb_amd/csrc/walk_plan.h"

using namespace sdb;

static int failures = 0;
#define CHECK(cond, ...)                          \
  do {                                            \
    if (!(cond)) {                                \
      failures++;                                 \
      std::printf("FAIL %s: ", #cond);            \
      std::printf(__VA_ARGS__);                   \
      std::printf("\n");                          \
    }                                             \
  } while (0)

// something for the pointer fields to point at: plan_walk only asks whether they are set
static uint64_t there[2];
template <class T>
static T *set() { return reinterpret_cast<T *>(there); }

struct Call {
  SearchArgs a{};
  uint32_t nq = 16;
};

static Call call_of(const std::map<std::string, long> &f) {
  auto get = [&](const char *k) { auto it = f.find(k); return it == f.end() ? 0L : it->second; };
  Call c;
  SearchArgs &a = c.a;
  c.nq = (uint32_t)get("nq");
  a.ng = (uint32_t)get("ng"), a.tail = (uint32_t)get("tail"), a.metric = (int)get("metric");
  a.search_size = (uint32_t)get("search_size"), a.words_per_query = (uint32_t)get("words_per_query");
  if (get("filt")) a.filt_off = set<const uint32_t>();
  a.stage = (Stage)get("stage");
  a.prefer_bitset = (uint32_t)get("prefer_bitset"), a.wide_hash = (uint32_t)get("wide_hash");
  a.wide_mode = (uint32_t)get("wide_mode"), a.hash_limit = (uint32_t)get("hash_limit");
  if (get("pq")) a.pq_codes = set<const uint8_t>();
  a.pq_M = (uint32_t)get("pq_M"), a.pq_K = (uint32_t)get("pq_K");
  a.pq_lut_in_lds = (uint32_t)get("pq_lut_in_lds"), a.pq_narrow = (uint32_t)get("pq_narrow");
  if (get("bq")) a.bq_codes = set<const uint64_t>();
  a.bq_metric = (uint32_t)get("bq_metric");
  if (get("vis")) a.vis_slots = set<uint32_t>();
  if (get("dcache")) a.dcache = set<uint2>();
  a.start_ext_n = (uint32_t)get("start_ext_n");
  return c;
}

static const char *family_name(WalkFamily f) {
  switch (f) {
    case WalkFamily::kPlain: return "plain";
    case WalkFamily::kStageHalf: return "stage_half";
    case WalkFamily::kStageInt8: return "stage_int8";
    case WalkFamily::kWide: return "wide";
    case WalkFamily::kPqLds: return "pq_lds";
    case WalkFamily::kPqGlobal: return "pq_global";
    case WalkFamily::kPqTwoWaves: return "pq_two_waves";
    case WalkFamily::kPqWide: return "pq_wide";
    case WalkFamily::kBits: return "bits";
  }
  return "?";
}
static const char *visited_name(WalkVisited v) {
  switch (v) {
    case WalkVisited::kBitset: return "bitset";
    case WalkVisited::kHash: return "hash";
    case WalkVisited::kHashPQ: return "hash_pq";
    case WalkVisited::kHash16: return "hash16";
  }
  return "?";
}

static int print_plans(const char *path) {
  std::ifstream in(path);
  if (!in) return std::printf("cannot read %s\n", path), 2;
  std::string line;
  while (std::getline(in, line)) {
    std::map<std::string, long> f;
    std::istringstream ss(line);
    std::string tok;
    while (ss >> tok) {
      const size_t eq = tok.find('=');
      if (eq == std::string::npos) return std::printf("bad token %s\n", tok.c_str()), 2;
      f[tok.substr(0, eq)] = std::strtol(tok.c_str() + eq + 1, nullptr, 10);
    }
    const Call c = call_of(f);
    const WalkPlan p = plan_walk(c.a, c.nq);
    std::printf("error=%d family=%s visited=%s clear=%d ng=%d l2=%d filt=%d jaccard=%d nreg=%d waves=%d nl=%d rt=%d nlw=%d split=%d "
                "hash_limit=%u wide_pull=%u\n",
                (int)p.bad_search_size, family_name(p.family), visited_name(p.visited), (int)p.clear_bitsets, p.ng, (int)p.l2, (int)p.filt,
                (int)p.jaccard, p.nreg, p.waves, p.nl, p.rt, p.nlw, (int)p.split, p.hash_limit, p.wide_pull);
  }
  return 0;
}

// words_per_query * 32 just below and just above 1 << 24: up to 2^24 rows a set beside a code table has 16-bit cells,
// beyond 32-bit ones; SDB_TUNE_WIDE_HASH keeps the latter everywhere.  Plain rows never take either.
static void check_boundary() {
  const uint32_t below = (1u << 24) / 32, above = below + 1;
  struct Shape { const char *what; uint32_t M, K, lut_in_lds; bool bq; WalkFamily family; };
  const Shape shapes[] = {
      {"quantized, one wave (SDB_TUNE_PQ_NARROW = 1)", 8, 256, 1, false, WalkFamily::kPqLds},
      {"quantized, two waves", 8, 256, 1, false, WalkFamily::kPqTwoWaves},
      {"quantized, multi-wave M = 192", 192, 256, 0, false, WalkFamily::kPqWide},
      {"quantized, multi-wave M = 384", 384, 256, 0, false, WalkFamily::kPqWide},
      {"bit codes", 0, 0, 0, true, WalkFamily::kBits},
  };
  for (const Shape &s : shapes)
    for (int wide_hash = 0; wide_hash < 2; wide_hash++)
      for (uint32_t words : {below, above}) {
        SearchArgs a{};
        a.search_size = 75, a.words_per_query = words, a.wide_hash = (uint32_t)wide_hash;
        if (s.bq) a.bq_codes = set<const uint64_t>();
        else a.pq_codes = set<const uint8_t>(), a.pq_M = s.M, a.pq_K = s.K, a.pq_lut_in_lds = s.lut_in_lds;
        if (s.family == WalkFamily::kPqLds) a.pq_narrow = 1;
        const WalkPlan p = plan_walk(a, 1024);
        const WalkVisited want = (words == below && !wide_hash) ? WalkVisited::kHash16 : WalkVisited::kHashPQ;
        CHECK(!p.bad_search_size && p.family == s.family, "%s: family %s", s.what, family_name(p.family));
        CHECK(p.visited == want, "%s, %u words, wide_hash %d: %s", s.what, words, wide_hash, visited_name(p.visited));
        CHECK(!p.clear_bitsets, "%s: an LDS set needs no clear", s.what);
      }
  for (uint32_t words : {below, above}) {  // plain rows: the 32-bit-cell set of 8192 cells whatever the table's size
    SearchArgs a{};
    a.search_size = 75, a.words_per_query = words, a.ng = 3;
    const WalkPlan p = plan_walk(a, 1024);
    CHECK(p.family == WalkFamily::kPlain && p.visited == WalkVisited::kHash, "plain rows, %u words: %s", words, visited_name(p.visited));
  }
}

static void check_grid() {
  long plans = 0, staged_above_96 = 0;
  for (uint32_t ng : {0u, 1u, 2u, 3u, 4u, 5u, 6u, 8u, 12u, 16u, 24u, 7u})
    for (uint32_t ss : {0u, 1u, 64u, 96u, 97u, 128u, 129u, 512u, 513u})
      for (int filt = 0; filt < 2; filt++)
        for (uint32_t stage = 0; stage < 3; stage++)
          for (uint32_t knobs = 0; knobs < 64; knobs++)
            for (uint32_t nq : {1u, 256u, 257u, 512u, 513u, 4096u}) {
              SearchArgs a{};
              a.ng = ng, a.search_size = ss, a.stage = (Stage)stage;
              if (filt) a.filt_off = set<const uint32_t>();
              a.prefer_bitset = knobs & 1, a.wide_mode = (knobs >> 1) & 3;
              if (a.wide_mode == 3) continue;
              if (filt && a.stage == Stage::kInt8) continue;  // no such call: search_batch.hip choose_stage gives a filtered call the float16 copy or none
              a.metric = (knobs & 8) ? SDB_METRIC_EUCLIDEAN : SDB_METRIC_COSINE;
              a.tail = (knobs & 16) ? 7 : 0;
              if (knobs & 32) a.vis_slots = set<uint32_t>();
              const WalkPlan p = plan_walk(a, nq);
              plans++;
              if (ss == 0 || ss == 513) {
                CHECK(p.bad_search_size && !p.clear_bitsets, "searchSize %u", ss);
                continue;
              }
              CHECK(!p.bad_search_size, "searchSize %u", ss);
              // the bitsets are cleared exactly for the kernels that walk on them ...
              CHECK(p.clear_bitsets == (p.visited == WalkVisited::kBitset), "ng %u L %u filt %d stage %u knobs %u nq %u", ng, ss, filt,
                    stage, knobs, nq);
              // ... and the staged filtered walk keeps its LDS sets at 97 .. 128, where every other walk is on the bitset
              const bool staged = p.family == WalkFamily::kStageHalf || p.family == WalkFamily::kStageInt8;
              if (ss > 96) {
                CHECK(staged ? (ss <= 128 && filt && !a.prefer_bitset && p.family == WalkFamily::kStageHalf && !p.clear_bitsets)
                             : p.visited == WalkVisited::kBitset,
                      "ng %u L %u filt %d stage %u knobs %u nq %u: %s / %s", ng, ss, filt, stage, knobs, nq, family_name(p.family),
                      visited_name(p.visited));
                staged_above_96 += staged;
              }
              CHECK(p.nreg == (ss <= 128 ? 2 : 8), "L %u: %d array registers", ss, p.nreg);
              CHECK(p.family == WalkFamily::kWide || p.wide_pull == 0, "wide_pull outside the workgroup-per-query walk");
            }
  CHECK(staged_above_96 > 0, "the grid never reached the staged filtered walk above searchSize 96");
  std::printf("grid: %ld plans, %ld staged above searchSize 96\n", plans, staged_above_96);
}

int main(int argc, char **argv) {
  if (argc == 3 && !std::strcmp(argv[1], "plans")) return print_plans(argv[2]);
  if (argc == 2 && !std::strcmp(argv[1], "checks")) {
    check_boundary();
    check_grid();
    std::printf("%d failures\n", failures);
    return failures ? 1 : 0;
  }
  std::printf("usage: %s plans FILE | checks\n", argv[0]);
  return 2;
}
