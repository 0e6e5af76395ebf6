"""The walk's routing decision (semadb_amd/csrc/walk_plan.h plan_walk) on the CPU.

tests/golden/walk_routes.json is what tools/walk_routes.py recorded on one MI355X with the library of the commit
BEFORE walk_plan.h existed: per call of a fixed list, the walk kernel that ran (demangled name, grid, workgroup, LDS) and
how many fills preceded it, with the routing-relevant fields of the call's SearchArgs beside it.  Here
tests/host/test_walk_plan.cpp -- plain C++, the two HIP-free headers only -- plans every one of those calls, and the plan
must name exactly the recorded kernel and the recorded clear.  The program's own checks cover what a tiny table cannot
reach (the 2^24-row boundary of the 16-bit-cell visited set, a grid over shapes and knobs).  Both run once plainly and
once under AddressSanitizer + UBSan, as a stand-alone program."""
import json
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "semadb_amd", "csrc")
GOLDEN = os.path.join(ROOT, "tests", "golden", "walk_routes.json")
CLANG = shutil.which("clang++", path="/opt/rocm/lib/llvm/bin") or shutil.which("clang++")
BUILDS = {"plain": [], "sanitized": ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]}
VISITED = {"bitset": "0u", "hash": "8192u", "hash_pq": "7417u", "hash16": "4294967295u"}
PREDICATES = ("pq_wide_shape", "search_uses_hash", "pq_two_waves", "wide_walk", "sketch_walk")


@pytest.fixture(scope="module", params=sorted(BUILDS))
def program(request, tmp_path_factory):
    if CLANG is None:
        pytest.skip("no clang++ in this image")
    exe = str(tmp_path_factory.mktemp("walk_plan") / ("walk_plan_" + request.param))
    subprocess.check_call([CLANG, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror"] + BUILDS[request.param] +
                          [os.path.join(ROOT, "tests", "host", "test_walk_plan.cpp"), "-o", exe])
    return exe


def _run(args):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1")
    out = subprocess.run(args, capture_output=True, text=True, timeout=120, env=env)
    tail = out.stdout[-3000:] + "\n" + out.stderr[-3000:]
    assert out.returncode == 0, tail
    for word in ("AddressSanitizer", "LeakSanitizer", "runtime error"):
        assert word not in out.stderr, tail
    return out.stdout


def kernel_of(p):
    """the demangled instantiation a plan names (walk_launch.hip's mapping, stated once more)"""
    b = lambda key: "true" if p[key] == "1" else "false"
    v = VISITED[p["visited"]]
    fam = p["family"]
    if fam == "wide":
        return "sdb::k_greedy_search_wide<%s, %s, %s, %s>" % (p["ng"], b("l2"), p["waves"], b("filt"))
    if fam == "pq_two_waves":
        return "sdb::k_greedy_search_pq2<%s>" % v
    if fam == "pq_wide":
        return "sdb::k_greedy_search_pqw<%s, %s, %s, %s, %s, %s>" % (p["nl"], p["rt"], v, p["waves"], p["nlw"], b("split"))
    dist = {"plain": "sdb::PlainDist<%s, %s, %s, 0, (sdb::Stage)0>" % (p["ng"], b("l2"), "true" if p["visited"] == "hash" else "false"),
            "stage_half": "sdb::PlainDist<%s, %s, true, 4, (sdb::Stage)1>" % (p["ng"], b("l2")),
            "stage_int8": "sdb::Int8Dist<%s>" % p["ng"],
            "pq_lds": "sdb::PQDistT<true, true>", "pq_global": "sdb::PQDistT<false, false>",
            "bits": "sdb::BitDist<%s>" % b("jaccard")}[fam]
    return "sdb::k_greedy_search<%s, %s, %s, %s>" % (dist, p["nreg"], b("filt"), v)


def _line(fields, nq=None):
    f = dict(fields, nq=fields["nq"] if nq is None else nq)
    return " ".join("%s=%d" % kv for kv in sorted(f.items()))


def test_plan_names_the_recorded_kernel_of_every_call(program, tmp_path):
    golden = json.load(open(GOLDEN))
    launches = []  # (description, recorded launch, fields line)
    for e in golden:
        if "kernels" in e:  # a build: every distinct launch of its rounds; a round's points are the launch's queries
            for k in e["kernels"]:
                launches.append((e["desc"], k, _line(e["fields"], k["grid"] // k["workgroup"])))
        else:
            launches.append((e["desc"], e, _line(e["fields"])))
    assert len(golden) >= 90 and len(launches) > len(golden)
    path = tmp_path / "calls.txt"
    path.write_text("".join(line + "\n" for _, _, line in launches))
    plans = [dict(tok.split("=") for tok in ln.split()) for ln in _run([program, "plans", str(path)]).splitlines()]
    assert len(plans) == len(launches)
    # the fills ahead of a filtered call's walk that are not the bitset clear (the resolve step's flags): what the record
    # shows for the filtered call on the LDS sets
    flags = {e["desc"]: e for e in golden}["ng=3 cosine filtered, default (no stage for a filtered call)"]["fills_before_walk"]
    for (desc, rec, line), p in zip(launches, plans):
        assert p["error"] == "0", desc
        assert rec["kernel"] == kernel_of(p), "%s\n  %s" % (desc, line)
        assert rec["workgroup"] == 64 * int(p["waves"]), desc
        if "fills_before_walk" in rec:
            assert rec["grid"] == rec["workgroup"] * int(line.split(" nq=")[1].split()[0]), desc
            filtered = " filt=1 " in " " + line + " "
            assert rec["fills_before_walk"] == int(p["clear"]) + (flags if filtered else 0), desc
        assert p["hash_limit"] == "6000"
        assert p["wide_pull"] == ("2" if p["family"] == "wide" and (p["waves"] == "16" or p["ng"] == "8") and
                                  rec["grid"] // rec["workgroup"] <= 256 else "0"), desc


def test_plan_beyond_what_a_tiny_table_reaches(program):
    out = _run([program, "checks"])
    assert "\n0 failures" in out, out[-3000:]
    assert re.search(r"grid: \d{5,} plans, [1-9]\d* staged above searchSize 96", out), out[-3000:]


def test_dirty_buffer_settings_reach_every_result_copy(program, tmp_path):
    """tests/test_gpu_pq.py test_result_rows_into_dirty_buffers says which caller of write_results each of its five
    settings reaches; nothing a search call returns tells the callers apart, so the plan of each setting is held here:
    60 rows, limit = searchSize = 64, 8 queries, K = 32; the fields as search_batch.hip fills them for a quantized table
    (the table goes to LDS up to 64 KB)"""
    want = {(128, 0): "sdb::k_greedy_search_pqw<15, 17, 4294967295u, 4, 15, true>",   # the split form: PQWideDist::serve<true>
            (128, 3): "sdb::k_greedy_search_pqw<15, 17, 4294967295u, 4, 15, false>",  # the walker's own search_body
            (128, 1): "sdb::k_greedy_search<sdb::PQDistT<true, true>, 2, false, 0u>",        # one wave, on the bitset
            (8, 0): "sdb::k_greedy_search_pq2<4294967295u>",                           # pq2_merger
            (8, 1): "sdb::k_greedy_search<sdb::PQDistT<true, true>, 2, false, 4294967295u>"}
    keys = sorted(want)
    lines = [_line({"nq": 8, "ng": 1, "tail": 0, "metric": 1, "search_size": 64, "words_per_query": 2, "filt": 0, "stage": 0,
                    "prefer_bitset": 0, "wide_hash": 0, "wide_mode": 0, "pq_narrow": narrow, "pq": 1, "pq_M": M, "pq_K": 32,
                    "pq_lut_in_lds": int(M * 32 * 4 <= 64 * 1024)}) for M, narrow in keys]
    path = tmp_path / "dirty.txt"
    path.write_text("".join(line + "\n" for line in lines))
    plans = [dict(tok.split("=") for tok in ln.split()) for ln in _run([program, "plans", str(path)]).splitlines()]
    assert [kernel_of(p) for p in plans] == [want[k] for k in keys]


def test_golden_record_is_small():
    others = [os.path.getsize(os.path.join(os.path.dirname(GOLDEN), f)) for f in os.listdir(os.path.dirname(GOLDEN))
              if f.endswith(".npz")]
    assert os.path.getsize(GOLDEN) <= min(others)


def test_callers_and_launcher_read_one_plan():
    """the launcher and both callers take the decision from walk_plan.h; nothing under csrc/ keeps a copy of it"""
    src = {f: open(os.path.join(CSRC, f)).read() for f in os.listdir(CSRC) if f.endswith((".hip", ".h", ".inc"))}
    for f in ("walk_launch.hip", "search_batch.hip", "build.hip"):
        assert '#include "walk_plan.h"' in src[f] and "plan_walk(" in src[f], f
    for f in ("search_batch.hip", "build.hip"):
        assert "plan_walk(" in src[f] and "launch_walk_plan(plan, " in src[f] and "plan.clear_bitsets" in src[f], f
    for f, text in src.items():
        for gone in PREDICATES:
            assert not re.search(r"\b%s\b" % gone, text), "%s names %s" % (f, gone)
    assert src["walk_launch.hip"].count("hipLaunchKernelGGL") == 1
    assert 'fail(SDB_ERR_INVALID, "searchSize %u not supported on device (1..512)", a.search_size)' in src["walk_launch.hip"]
    assert [f for f, text in src.items() if '#include "search_kernel.h"' in text] == ["walk_launch.hip"]
    for part in ("walk_stage.h", "walk_dist_rows.h", "cand_array.h", "visited_set.h", "walk_dist_codes.h"):  # search_kernel.h's parts
        assert part in src and '#include "%s"' % part in src["search_kernel.h"], part
        assert not [f for f, text in src.items() if f.endswith(".hip") and '#include "%s"' % part in text], part
    for f in ("walk_args.h", "walk_plan.h"):  # HIP-free outside a HIP build
        assert not re.search(r"__device__|__global__|hipStream_t", src[f]), f
