#!/usr/bin/env python3
"""Which walk kernel serves which call, recorded on the GPU: a fixed, ordered list of search calls (and three small builds)
on tiny tables, run under a kernel-trace-only profiler; per call the walk kernel's demangled name, grid, workgroup and
LDS size, and the fills (hipMemsetAsync; the bitset clear is one) that ran between the call's start and the walk.

    rocprofv3 --kernel-trace --output-format csv -d DIR -- python3 tools/walk_routes.py run DIR/calls.json
    python3 tools/walk_routes.py record DIR DIR/calls.json OUT.json     # fails if a leaf of the routing was not reached
    python3 tools/walk_routes.py compare A.json B.json OUT.json         # entry for entry; exit 1 on a difference

SEMADB_AMD_LIB selects the library, so the same list runs on a library built from another commit.  Beside every entry
stand the routing-relevant fields of the call's SearchArgs as this file's model of the search call fills them:
tests/test_walk_plan.py hands them to csrc/walk_plan.h's plan_walk() on the CPU and holds the plan against the kernel
recorded here (tests/golden/walk_routes.json is the record of the commit before walk_plan.h existed).

"lds" is the profiler's LDS_Block_Size column as it stands: it is not the dynamic LDS the launch asked for (a walk with
the 32 KB visited set shows 1024, filtered walks with LDS sets 0), so it only shows that two runs agree, not the size;
the sizes are walk_launch.hip's expressions.

A call starts at a marker kernel (torch's erfinv on a scratch tensor, which nothing else launches)."""
import csv
import glob
import hashlib
import json
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ROWS = 600
METRIC = {"euclidean": 0, "cosine": 1, "dot": 2, "hamming": 3, "jaccard": 4}
DIM_OF_NG = {0: 16, 1: 128, 2: 256, 3: 384, 4: 512, 6: 768, 8: 1024, 12: 1536, 16: 2048, 24: 3072, 17: 2176}


def layout(dim):
    """common.h RowLayout: (ng, tail)"""
    ng = (dim // 32 + 3) // 4
    for t in (1, 2, 3, 4, 6, 8, 12, 16, 24):
        if t >= ng:
            if 3 * t <= 4 * ng:
                ng = t
            break
    return ng, dim % 32


def call(desc, table, nq=16, L=75, filt=False, **knobs):
    return {"desc": desc, "table": list(table), "nq": nq, "L": L, "filt": filt, "knobs": knobs}


def plain(metric, dim):
    return ("plain", metric, dim)


def pq(M, K, dim=768):
    return ("pq", "cosine", dim, M, K)


def bq(bit_metric):
    return ("bq", "cosine", 384, bit_metric)


def calls():
    c = []
    one = {"wide_walk": 1}  # one wave per query for a call of 16 queries
    # plain tables: every group count with a kernel of its own, one without (no dimension lays out as ng = 5: 640 floats
    # are padded to 6 groups; 2 176 floats stay at 17), a tail, both metric classes
    for ng in (0, 1, 2, 3, 4, 6, 8, 12, 16, 24, 17):
        for metric in ("cosine", "euclidean"):
            c.append(call("plain ng=%d %s, float32 walk" % (ng, metric), plain(metric, DIM_OF_NG[ng]), sketch=0, **one))
    c.append(call("plain d=100 (ng=1, tail 4) cosine", plain("cosine", 100), **one))
    c.append(call("plain d=100 (ng=1, tail 4) cosine, workgroup per query", plain("cosine", 100)))
    # batch size, where the workgroup-per-query walk turns
    for nq in (256, 257):
        c.append(call("ng=4 cosine, %d queries" % nq, plain("cosine", 512), nq=nq))
    for nq in (512, 513):
        c.append(call("ng=3 cosine, %d queries" % nq, plain("cosine", 384), nq=nq))
    c.append(call("ng=3 cosine, 257 queries (eight waves per query)", plain("cosine", 384), nq=257))
    c.append(call("ng=8 cosine, 16 queries (the eight-wave form)", plain("cosine", 1024)))
    c.append(call("ng=8 cosine, 257 queries", plain("cosine", 1024), nq=257))
    c.append(call("ng=3 euclidean, 16 queries, filtered, workgroup per query", plain("euclidean", 384), filt=True))
    c.append(call("ng=3 cosine, 600 queries, SDB_TUNE_WIDE_WALK=2", plain("cosine", 384), nq=600, wide_walk=2))
    c.append(call("ng=12 cosine, 16 queries, SDB_TUNE_WIDE_WALK=2 (no such kernel beyond ng=8)", plain("cosine", 1536), wide_walk=2))
    # searchSize
    for L in (96, 97, 128, 129, 512):
        for filt in (False, True):
            c.append(call("ng=3 euclidean L=%d%s, float32 walk" % (L, " filtered" if filt else ""), plain("euclidean", 384), L=L,
                          filt=filt, sketch=0, **one))
    c.append(call("ng=17 cosine L=129 filtered (run-time length, eight array registers)", plain("cosine", 2176), L=129, filt=True, **one))
    # the two-precision stage
    c.append(call("ng=3 cosine, default stage (int8)", plain("cosine", 384), **one))
    c.append(call("ng=3 cosine, SDB_TUNE_SKETCH=1 (float16)", plain("cosine", 384), sketch=1, **one))
    c.append(call("ng=3 euclidean, SDB_TUNE_SKETCH=3 (falls to float16)", plain("euclidean", 384), sketch=3, **one))
    c.append(call("ng=6 cosine, default stage (float16: no int8 stage beyond ng=3)", plain("cosine", 768), **one))
    c.append(call("ng=3 cosine filtered, default (no stage for a filtered call)", plain("cosine", 384), filt=True, **one))
    for L in (75, 97, 128, 129):
        c.append(call("ng=3 cosine filtered L=%d, SDB_TUNE_SKETCH_FILTERED" % L, plain("cosine", 384), L=L, filt=True,
                      sketch_filtered=1, **one))
    c.append(call("ng=3 cosine L=97, default stage (plain calls above 96: the bitset)", plain("cosine", 384), L=97, **one))
    # bitset and hash knobs
    c.append(call("ng=3 cosine, SDB_TUNE_NO_HASH", plain("cosine", 384), no_hash=1, **one))
    c.append(call("ng=3 cosine filtered, SDB_TUNE_NO_HASH, SDB_TUNE_SKETCH_FILTERED", plain("cosine", 384), filt=True, no_hash=1,
                  sketch_filtered=1, **one))
    c.append(call("ng=3 cosine, SDB_TUNE_NO_HASH, 16 queries (no workgroup-per-query walk on the bitset)", plain("cosine", 384), no_hash=1))
    c.append(call("ng=3 cosine, SDB_TUNE_WIDE_HASH (plain rows: no effect)", plain("cosine", 384), wide_hash=1, **one))
    # bit codes: both metrics, each visited policy
    for m in ("hamming", "jaccard"):
        c.append(call("bit codes %s" % m, bq(m)))
        c.append(call("bit codes %s, SDB_TUNE_WIDE_HASH" % m, bq(m), wide_hash=1))
        c.append(call("bit codes %s, SDB_TUNE_NO_HASH" % m, bq(m), no_hash=1))
        c.append(call("bit codes %s filtered L=129" % m, bq(m), L=129, filt=True))
    # product quantizer
    c.append(call("pq M=8 K=256 (2 048 entries: two waves)", pq(8, 256)))
    c.append(call("pq M=8 K=256, SDB_TUNE_WIDE_HASH", pq(8, 256), wide_hash=1))
    c.append(call("pq M=8 K=256, SDB_TUNE_PQ_NARROW=1 (one wave)", pq(8, 256), pq_narrow=1))
    c.append(call("pq M=8 K=256, SDB_TUNE_PQ_NARROW=1, SDB_TUNE_WIDE_HASH", pq(8, 256), pq_narrow=1, wide_hash=1))
    c.append(call("pq M=8 K=256 filtered", pq(8, 256), filt=True))
    c.append(call("pq M=8 K=256 L=97", pq(8, 256), L=97))
    c.append(call("pq M=8 K=256, SDB_TUNE_NO_HASH", pq(8, 256), no_hash=1))
    c.append(call("pq M=32 K=256 (table in LDS above 2 048 entries)", pq(32, 256)))
    c.append(call("pq M=32 K=256 L=129 filtered", pq(32, 256), L=129, filt=True))
    c.append(call("pq M=96 K=256 (table over 64 KB)", pq(96, 256)))
    c.append(call("pq M=96 K=256 L=129", pq(96, 256), L=129))
    c.append(call("pq M=16 K=100 (K no multiple of 32)", pq(16, 100)))
    c.append(call("pq M=128 K=100 (K no multiple of 32: no multi-wave walk)", pq(128, 100)))
    for M in (128, 192, 256, 384):
        c.append(call("pq M=%d K=256" % M, pq(M, 256)))
    c.append(call("pq M=192 K=256, SDB_TUNE_WIDE_HASH", pq(192, 256), wide_hash=1))
    c.append(call("pq M=384 K=256, SDB_TUNE_WIDE_HASH", pq(384, 256), wide_hash=1))
    for M in (128, 192):
        for narrow in (2, 3):
            c.append(call("pq M=%d K=256, SDB_TUNE_PQ_NARROW=%d" % (M, narrow), pq(M, 256), pq_narrow=narrow))
    c.append(call("pq M=192 K=256, SDB_TUNE_PQ_NARROW=1", pq(192, 256), pq_narrow=1))
    c.append(call("pq M=192 K=256 filtered", pq(192, 256), filt=True))
    c.append(call("pq M=192 K=256 L=97", pq(192, 256), L=97))
    # the build's own searches: a visit log and a distance table per point, wide_mode from build.hip
    c.append({"desc": "build of 600 rows d=384 cosine", "table": list(plain("cosine", 384)), "build": True, "knobs": {}})
    c.append({"desc": "build of 600 rows d=384 cosine, SDB_TUNE_WIDE_WALK=1", "table": list(plain("cosine", 384)), "build": True,
              "knobs": {"wide_walk": 1}})
    c.append({"desc": "build of 600 rows d=2176 cosine (run-time length)", "table": list(plain("cosine", 2176)), "build": True, "knobs": {}})
    return c


def fields(c):
    """the routing-relevant fields of SearchArgs for a call: search_batch.hip fill_search_args / choose_stage /
    attach_quantizer, build.hip's round for a build"""
    t, k = c["table"], c["knobs"]
    ng, tail = layout(t[2])
    f = {"nq": c.get("nq", 0), "ng": ng, "tail": tail, "metric": METRIC[t[1]], "search_size": c.get("L", 0),
         "words_per_query": (ROWS + 1 + 31) // 32, "filt": int(c.get("filt", False)), "stage": 0,
         "prefer_bitset": k.get("no_hash", 0), "wide_hash": k.get("wide_hash", 0), "wide_mode": k.get("wide_walk", 0),
         "pq_narrow": k.get("pq_narrow", 0)}
    if t[0] == "pq":
        f.update(pq=1, pq_M=t[3], pq_K=t[4], pq_lut_in_lds=int(t[3] * t[4] * 4 <= 64 * 1024))
    elif t[0] == "bq":
        f.update(bq=1, bq_metric=METRIC[t[3]])
    elif "build" not in c:
        knob, for_filtered = k.get("sketch", 3), k.get("sketch_filtered", 0)
        if knob and tail == 0 and ng in (1, 2, 3, 4, 6):
            int8 = knob >= 3 and not for_filtered and ng <= 3 and t[1] != "euclidean"
            f["stage"] = (0 if c["filt"] else 2) if int8 else (1 if not c["filt"] or for_filtered else 0)
    if "build" in c:  # (nq and wide_mode are the round's: tests/test_walk_plan.py takes nq from the recorded grid)
        f.update(search_size=75, vis=1, dcache=1, build=1, wide_mode=1 if k.get("wide_walk", 0) == 1 else 0)
    return f


# ---- run: the calls, on the GPU -------------------------------------------------------------------------------------
def run(out):
    import numpy as np
    import torch
    from semadb_amd import vamana
    from semadb_amd import vectorstore as vs

    rng = np.random.default_rng(20261019)
    scratch = torch.zeros(4096, device="cuda")
    tables = {}

    def rows(n, d):
        v = rng.standard_normal((n, d)).astype(np.float32)
        return torch.from_numpy(v / np.linalg.norm(v, axis=1, keepdims=True)).cuda()

    def new_index(t):
        ix = vamana.NewIndexVamana("routes", vamana.IndexVectorVamanaParameters(t[2], t[1], 75, 32, 1.2), capacity=ROWS + 1, strict=False)  # (searchSize beyond the REST range)
        ix.set_start(rows(1, t[2])[0].cpu().numpy())
        return ix

    def table(t):
        if tuple(t) not in tables:
            ix = new_index(t)
            base = rows(ROWS, t[2])
            ix.insert_batch(None, base)
            if t[0] == "pq":
                q = vs.ProductQuantizer(t[1], vs.ProductQuantizerParameters(t[4], t[3], ROWS), t[2])
                q.Fit(base.cpu().numpy().copy(), np.arange(t[3]) * 7 % ROWS, alias=True)
                vs.attach(ix, q)
            elif t[0] == "bq":
                q = vs.BinaryQuantizer(vs.BinaryQuantizerParameters(None, 0, t[3]), t[2])
                vs.attach_binary(ix, q)
            tables[tuple(t)] = (ix, q if t[0] != "plain" else None)
        return tables[tuple(t)][0]

    def mark():
        torch.cuda.synchronize()
        scratch.erfinv_()
        torch.cuda.synchronize()

    todo = calls()
    for c in todo:
        c["fields"] = fields(c)
        if c.get("build"):
            ix, base = new_index(c["table"]), rows(ROWS, c["table"][2])
            for key, v in c["knobs"].items():
                ix.set_tuning(key, v)
            mark()
            ix.insert_batch(None, base)
            torch.cuda.synchronize()
            ix.close()
            continue
        ix = table(c["table"])
        for key, v in c["knobs"].items():
            ix.set_tuning(key, v)
        q = rows(c["nq"], c["table"][2])
        filters = [set(int(v) for v in rng.choice(ROWS, 200, replace=False) + 2) for _ in range(c["nq"])] if c["filt"] else None
        mark()
        ix.search_batch(q, 10, c["L"], filters=filters)
        torch.cuda.synchronize()
        for key in c["knobs"]:
            ix.set_tuning(key, {"sketch": 3}.get(key, 0))
    mark()
    with open(out, "w") as f:
        json.dump(todo, f)
    print("ran %d calls" % len(todo))


# ---- record: the trace, per call ------------------------------------------------------------------------------------
LEAVES = [  # every leaf of the routing that a table of 600 rows can reach: (label, pattern on the demangled name)
    ("plain, LDS set", r"k_greedy_search<sdb::PlainDist<3, false, true, 0, \(sdb::Stage\)0>, 2, false, 8192u>"),
    ("plain, LDS set, filtered", r"k_greedy_search<sdb::PlainDist<3, true, true, 0, \(sdb::Stage\)0>, 2, true, 8192u>"),
    ("plain, bitset, two registers", r"k_greedy_search<sdb::PlainDist<3, true, false, 0, \(sdb::Stage\)0>, 2, false, 0u>"),
    ("plain, bitset, eight registers", r"k_greedy_search<sdb::PlainDist<3, true, false, 0, \(sdb::Stage\)0>, 8, false, 0u>"),
    ("plain, bitset, filtered", r"k_greedy_search<sdb::PlainDist<3, true, false, 0, \(sdb::Stage\)0>, 8, true, 0u>"),
    ("run-time length", r"k_greedy_search<sdb::PlainDist<-1, false, false, 0, \(sdb::Stage\)0>, 2, false, 0u>"),
    ("run-time length, eight registers, filtered", r"k_greedy_search<sdb::PlainDist<-1, false, false, 0, \(sdb::Stage\)0>, 8, true, 0u>"),
    ("float16 stage", r"k_greedy_search<sdb::PlainDist<3, false, true, 4, \(sdb::Stage\)1>, 2, false, 8192u>"),
    ("float16 stage, euclidean", r"k_greedy_search<sdb::PlainDist<3, true, true, 4, \(sdb::Stage\)1>, 2, false, 8192u>"),
    ("float16 stage, filtered", r"k_greedy_search<sdb::PlainDist<3, false, true, 4, \(sdb::Stage\)1>, 2, true, 8192u>"),
    ("int8 stage", r"k_greedy_search<sdb::Int8Dist<3>, 2, false, 8192u>"),
    ("workgroup per query, sixteen waves", r"k_greedy_search_wide<3, false, 16, false>"),
    ("workgroup per query, eight waves", r"k_greedy_search_wide<3, false, 8, false>"),
    ("workgroup per query, ng=8", r"k_greedy_search_wide<8, false, 8, false>"),
    ("workgroup per query, filtered", r"k_greedy_search_wide<3, true, 16, true>"),
    ("bit codes, 16-bit cells", r"k_greedy_search<sdb::BitDist<false>, 2, false, 4294967295u>"),
    ("bit codes, 32-bit cells", r"k_greedy_search<sdb::BitDist<true>, 2, false, 7417u>"),
    ("bit codes, bitset", r"k_greedy_search<sdb::BitDist<true>, 2, false, 0u>"),
    ("bit codes, bitset, filtered", r"k_greedy_search<sdb::BitDist<false>, 8, true, 0u>"),
    ("quantized, two waves, 16-bit cells", r"k_greedy_search_pq2<4294967295u>"),
    ("quantized, two waves, 32-bit cells", r"k_greedy_search_pq2<7417u>"),
    ("quantized, one wave, LDS table, 16-bit cells", r"k_greedy_search<sdb::PQDistT<true, true>, 2, false, 4294967295u>"),
    ("quantized, one wave, LDS table, 32-bit cells", r"k_greedy_search<sdb::PQDistT<true, true>, 2, false, 7417u>"),
    ("quantized, one wave, LDS table, LDS sets, filtered", r"k_greedy_search<sdb::PQDistT<true, true>, 2, true, 4294967295u>"),
    ("quantized, one wave, LDS table, bitset", r"k_greedy_search<sdb::PQDistT<true, true>, 2, false, 0u>"),
    ("quantized, one wave, LDS table, bitset, eight registers, filtered", r"k_greedy_search<sdb::PQDistT<true, true>, 8, true, 0u>"),
    ("quantized, one wave, global table", r"k_greedy_search<sdb::PQDistT<false, false>, 2, false, 0u>"),
    ("quantized, one wave, global table, eight registers", r"k_greedy_search<sdb::PQDistT<false, false>, 8, false, 0u>"),
    ("multi-wave M=128", r"k_greedy_search_pqw<15, 17, 4294967295u, 4, 15, true>"),
    ("multi-wave M=128, one query per CU", r"k_greedy_search_pqw<32, 0, 4294967295u, 4, 32, false>"),
    ("multi-wave M=128, walker does everything", r"k_greedy_search_pqw<15, 17, 4294967295u, 4, 15, false>"),
    ("multi-wave M=192", r"k_greedy_search_pqw<15, 33, 4294967295u, 4, 15, true>"),
    ("multi-wave M=192, 32-bit cells", r"k_greedy_search_pqw<15, 33, 7417u, 4, 15, true>"),
    ("multi-wave M=192, one query per CU", r"k_greedy_search_pqw<32, 16, 4294967295u, 4, 32, false>"),
    ("multi-wave M=192, walker does everything", r"k_greedy_search_pqw<15, 33, 4294967295u, 4, 15, false>"),
    ("multi-wave M=256", r"k_greedy_search_pqw<32, 32, 4294967295u, 4, 32, false>"),
    ("multi-wave M=384", r"k_greedy_search_pqw<15, 33, 4294967295u, 8, 24, false>"),
    ("multi-wave M=384, 32-bit cells", r"k_greedy_search_pqw<15, 33, 7417u, 8, 24, false>"),
]


def record(trace_dir, calls_json, out):
    found = glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True)
    if len(found) != 1:
        sys.exit("expected one kernel trace under %s, found %d" % (trace_dir, len(found)))
    rows = sorted(csv.DictReader(open(found[0])), key=lambda r: int(r["Start_Timestamp"]))
    col = lambda r, *names: next(int(r[n]) for n in names if n in r)
    todo = json.load(open(calls_json))
    spans, cur = [], None
    for r in rows:
        if "erfinv" in r["Kernel_Name"]:
            cur = []
            spans.append(cur)
        elif cur is not None:
            cur.append(r)
    if len(spans) != len(todo) + 1:
        sys.exit("%d markers in the trace for %d calls" % (len(spans), len(todo)))
    entries = []
    for c, span in zip(todo, spans):
        fills, kernels = [], []
        for r in span:
            name = r["Kernel_Name"]
            if "fillBuffer" in name and not kernels:
                fills.append(col(r, "Grid_Size_X", "Grid_Size"))
            if "sdb::k_greedy_search" in name:
                k = {"kernel": re.sub(r"^void |\(sdb::SearchArgs\)$", "", name), "grid": col(r, "Grid_Size_X", "Grid_Size"),
                     "workgroup": col(r, "Workgroup_Size_X", "Workgroup_Size"), "lds": col(r, "LDS_Block_Size")}
                if k not in kernels:
                    kernels.append(k)
        e = {"desc": c["desc"], "fields": c["fields"]}
        if c.get("build"):  # every distinct launch of the build's rounds (their fills include the build's own tables)
            e["kernels"] = kernels
        else:  # the call is the first thing behind its marker (what follows in the span: the next call's table being built)
            if not kernels:
                sys.exit("%s: no walk kernel in the call's span" % c["desc"])
            e.update(kernels[0], fills_before_walk=len(fills))
        entries.append(e)
    names = [k["kernel"] for e in entries for k in e.get("kernels", [e])]
    missing = [label for label, pat in LEAVES if not any(re.search(pat, n) for n in names)]
    json.dump(entries, open(out, "w"), indent=0, separators=(",", ":"))
    print("%d entries, %d distinct kernels" % (len(entries), len(set(names))))
    if missing:
        sys.exit("leaves of the routing that no call reached: " + "; ".join(missing))


def compare(a, b, out):
    A, B = json.load(open(a)), json.load(open(b))
    diff = [{"desc": x["desc"], "a": x, "b": y} for x, y in zip(A, B) if x != y]
    sha = lambda path: hashlib.sha256(open(path, "rb").read()).hexdigest()
    # (the first record is named, not repeated: it is the committed tests/golden/walk_routes.json when the parent is compared)
    verdict = {"entries": [len(A), len(B)], "equal": len(A) == len(B) and not diff, "differences": diff,
               "a": {"file": os.path.basename(a), "sha256": sha(a)}, "b_sha256": sha(b), "b": B}
    json.dump(verdict, open(out, "w"), indent=0, separators=(",", ":"))
    print("equal" if verdict["equal"] else "%d entries differ" % len(diff))
    sys.exit(0 if verdict["equal"] else 1)


if __name__ == "__main__":
    mode = sys.argv[1] if len(sys.argv) > 1 else ""
    if mode == "run" and len(sys.argv) == 3:
        run(sys.argv[2])
    elif mode == "record" and len(sys.argv) == 5:
        record(*sys.argv[2:5])
    elif mode == "compare" and len(sys.argv) == 5:
        compare(*sys.argv[2:5])
    else:
        sys.exit(__doc__)
