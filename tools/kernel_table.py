#!/usr/bin/env python3
"""Register / scratch / LDS figures of every kernel in the built libsemadb_amd.so, read from the gfx950 code
objects' own metadata notes (.vgpr_count, .agpr_count, .sgpr_count, .vgpr_spill_count, .private_segment_fixed_size,
.group_segment_fixed_size, .max_flat_workgroup_size) -- the figures DESIGN.md quotes come from here, not from memory.

    python3 tools/kernel_table.py                       # markdown table of the walk / build kernels
    python3 tools/kernel_table.py --all                 # every kernel
    python3 tools/kernel_table.py --json out.json       # machine-readable
    python3 tools/kernel_table.py --check               # exit 1 if ANY kernel has scratch or spilled VGPRs, or a kernel
                                                        # spills more SGPRs than its class allows (tests use this)
    python3 tools/kernel_table.py --memory-ops          # the walk kernels' memory instructions by kind, from the
                                                        # disassembly, and the staged hop's load schedule (stage_span)

Needs only the ROCm LLVM tools (llvm-objdump --offloading, llvm-readelf; binutils c++filt); no GPU."""
import argparse
import json
import os
import re
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SO = os.path.join(ROOT, "semadb_amd", "libsemadb_amd.so")
LLVM = "/opt/rocm/lib/llvm/bin"

# Round 6: NO kernel of the library may carry scratch memory or spilled VGPRs (--check fails on any).
# Spilled SGPRs live in lanes of a VGPR, not in memory; they cost lane moves.  The kernels a BASELINE configuration
# launches inside a timed region (C2 walk and its small-call forms, the C4 quantized walks and their table / encode /
# k-means kernels, the C3 build's prunes and back-edges, the exact scan, the merge) may spill at most SGPR_TIMED of
# them; the filtered forms of the walk carry six more list pointers and get SGPR_FILTERED; everything else SGPR_ANY
# (the run-time-length fallbacks of the quantizer kernels sit at 112 .. 135).
# The C2 walk is the two-precision hop's (PlainDist<NG, L2, true, 4, Stage::kHalf> -- the demangled name spells the stage
# (sdb::Stage)1 --, the default since SDB_TUNE_SKETCH is on), with the float32 walk (PlainDist<NG, L2, true, 0, (sdb::Stage)0>,
# the opt-out) beside it; both metrics, both timed.  Cosine / dot rows of up to 384 floats walk with the int8 first stage
# by default (Int8Dist<NG>, SDB_TUNE_SKETCH = 3): timed too.
SGPR_TIMED, SGPR_FILTERED, SGPR_ANY = 64, 128, 160
TIMED = re.compile(
    r"^sdb::(k_greedy_search<sdb::PlainDist<(3|6), (false|true), true, (0, \(sdb::Stage\)0|4, \(sdb::Stage\)1)>, 2, (false|true), 8192u>"
    r"|k_greedy_search<sdb::Int8Dist<(1|2|3)>, 2, false, 8192u>"
    r"|k_greedy_search<sdb::BitDist<(false|true)>, "  # the bit-code walks (tools/bench_bq.py times the hamming one)
    r"|k_greedy_search_wide<(3|6), false, (8|16), (false|true)>"
    r"|k_greedy_search_pq2<|k_greedy_search_pqw<15, 33, 4294967295u, 4, 15, true>"
    r"|k_pq_lut_t<true, 3, 96>|k_pq_lut_t<true, 0, 4>|k_pq_lut_mfma<|k_pq_encode_t<true, 3, true>|k_pq_encode_pair<true, 4>"
    r"|k_km_assign_t<3, 96>|k_km_assign_t<0, 4>|k_km_(?!assign_t<)|k_backedges<(3|6), false>|k_prune_|k_flat_|k_topk_merge|k_k1_|k_index_distance"
    r"|k_adjcodes|k_filter_)")
FILTERED = re.compile(r"^sdb::(k_greedy_search<.*, true, \d+u>|k_greedy_search_wide<.*, true>)$")

FIELDS = [".vgpr_count", ".agpr_count", ".sgpr_count", ".vgpr_spill_count", ".sgpr_spill_count",
          ".private_segment_fixed_size", ".group_segment_fixed_size", ".max_flat_workgroup_size"]


def code_objects(so, tmp):
    dst = os.path.join(tmp, os.path.basename(so))
    shutil.copy(so, dst)
    subprocess.run([os.path.join(LLVM, "llvm-objdump"), "--offloading", dst], cwd=tmp, check=True,
                   stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    return sorted(os.path.join(tmp, f) for f in os.listdir(tmp) if "amdgcn" in f)


def kernels(so=SO):
    out = []
    with tempfile.TemporaryDirectory() as tmp:
        for co in code_objects(so, tmp):
            notes = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", co], check=True, capture_output=True,
                                   text=True).stdout
            cur = None
            for line in notes.splitlines():
                if line.startswith("  - ") and cur is not None and ".name" in cur:
                    out.append(cur)
                    cur = {}
                elif line.startswith("  - "):
                    cur = {}
                if cur is None:
                    continue
                m = re.match(r"^(?:  - |    )(\.[a-z_]+):\s+(\S.*)$", line)
                if m and m.group(1) in FIELDS + [".name"]:
                    cur[m.group(1)] = m.group(2).strip()
                if line.startswith("amdhsa.target") or line.startswith("amdhsa.version"):
                    if cur and ".name" in cur:
                        out.append(cur)
                    cur = None
            if cur and ".name" in cur:
                out.append(cur)
    rows = []
    for k, d in zip(out, demangled([k[".name"] for k in out])):  # (without the parameter list: a template argument may hold parentheses of its own)
        row = {"kernel": d}
        for f in FIELDS:
            row[f[1:]] = int(k.get(f, "0"))
        rows.append(row)
    rows.sort(key=lambda r: r["kernel"])
    return rows


def demangled(names):
    dem = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True).stdout.splitlines()
    out = []
    for d in dem:
        d = re.sub(r"\s*\[clone .*\]$", "", d)
        d = re.sub(r"^void ", "", d)
        out.append(re.sub(r"\([^()]*\)$", "", d))
    return out


def disassembly(so=SO, match=r"^sdb::k_greedy_search"):
    """{demangled kernel name: [(mnemonic, operands), ...] in program order} of the kernels whose name matches"""
    pat = re.compile(match)
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        for co in code_objects(so, tmp):
            text = subprocess.run([os.path.join(LLVM, "llvm-objdump"), "-d", "--no-show-raw-insn", co], check=True,
                                  capture_output=True, text=True).stdout
            syms, cur = [], None
            for line in text.splitlines():
                m = re.match(r"^[0-9a-f]+ <([^>]+)>:$", line)
                if m:
                    cur = []
                    syms.append((m.group(1), cur))
                    continue
                m = re.match(r"^\s+([a-z_][a-z0-9_]*)\s*(.*?)\s*(?://.*)?$", line)
                if m and cur is not None:
                    cur.append((m.group(1), m.group(2)))
            for name, (_, ins) in zip(demangled([n for n, _ in syms]), syms):
                if pat.match(name) and ins:
                    out[name] = ins
    return out


# the staged one-wave kernels whose hop asks for the copy rows of all 64 edges ahead (walk_stage.h stage_ahead)
AHEAD = re.compile(r"^sdb::k_greedy_search<sdb::(Int8Dist<(1|2|3)>|PlainDist<(1|2|3), (false|true), true, 4, \(sdb::Stage\)1>), ")


def is_vmem_load(mn):
    return mn.startswith(("global_load", "flat_load", "buffer_load"))


def copy_row_loads(name):
    """vector loads a hop of that kernel issues for its copy rows: 32 pairs of rows, one load per int8 row, NG per
    float16 row, and the euclidean walk's ||y16||^2 of the lane's edge"""
    m = AHEAD.match(name)
    if m.group(2):
        return 32
    return 32 * int(m.group(3)) + (1 if m.group(4) == "true" else 0)


def stage_span(ins, want=32):
    """The hop's run of copy-row loads and what lies between it and the visited-set test.  Candidates are the stretches
    of straight-line code (no branch inside) that hold at least `want` vector-memory loads; the hop's is the one whose
    last load lies nearest in front of a ds_cmpst_rtn_b32 -- the test follows the hop's loads at once, whatever else of
    the kernel (a prologue, a round of float32 rows) may load as many values.  The run is the last `want` loads of that
    stretch: it may begin with the load of the adjacency row, which the copy rows' addresses wait for and which is not
    part of the run.  Returns None when there is no such stretch with a ds_cmpst_rtn_b32 behind it, else a dict: first /
    last (index of the run's first and last load), cmpst (index of the first ds_cmpst_rtn_b32 behind the run), loads
    (vector loads in the stretch), vm_waits (the s_waitcnt with a vmcnt field from the run's first load to that
    ds_cmpst_rtn_b32), other_vmem (vector-memory instructions behind the run and before the ds_cmpst_rtn_b32)."""
    cmpsts = [j for j, (mn, _) in enumerate(ins) if mn == "ds_cmpst_rtn_b32"]
    start, best = 0, None
    for i, (mn, _) in enumerate(list(ins) + [("s_endpgm", "")]):
        if mn.startswith(("s_cbranch", "s_branch", "s_endpgm", "s_setpc", "s_swappc")):
            idx = [j for j in range(start, min(i, len(ins))) if is_vmem_load(ins[j][0])]
            if len(idx) >= want:
                nxt = next((c for c in cmpsts if c > idx[-1]), None)
                if nxt is not None and (best is None or nxt - idx[-1] < best[2] - best[1]):
                    best = (idx[-want], idx[-1], nxt, len(idx))
            start = i + 1
    if best is None:
        return None
    first, last, cmpst, n_loads = best
    vm = ("global_", "flat_", "buffer_", "scratch_")
    return {"first": first, "last": last, "cmpst": cmpst, "loads": n_loads,
            "vm_waits": [(j, ins[j][1]) for j in range(first, cmpst) if ins[j][0] == "s_waitcnt" and "vmcnt" in ins[j][1]],
            "other_vmem": [(j, ins[j][0]) for j in range(last + 1, cmpst) if ins[j][0].startswith(vm)]}


def memory_ops(so=SO):
    """rows of the --memory-ops report: per walk kernel the count of instructions by kind, and stage_span's findings"""
    rows = []
    for name, ins in sorted(disassembly(so).items()):
        row = {"kernel": name}
        for kind in ("flat_", "global_load", "global_store", "global_atomic", "s_load", "ds_"):
            row[kind] = sum(1 for mn, _ in ins if mn.startswith(kind))
        if AHEAD.match(name):
            sp = stage_span(ins, copy_row_loads(name))
            row["stage"] = None if sp is None else {"loads": sp["loads"], "vm_waits": [w for _, w in sp["vm_waits"]],
                                                    "instructions_to_cmpst": sp["cmpst"] - sp["first"]}
        rows.append(row)
    return rows


def waves_per_simd(r):
    # gfx950: 512 VGPRs per SIMD lane shared by arch + acc registers, allocation granule 8, at most 8 waves per SIMD.
    # .vgpr_count of a gfx90a+ code object is the unified total (arch registers up to the accumulation offset + AGPRs)
    regs = r["vgpr_count"]
    regs = max(8, (regs + 7) // 8 * 8)
    return min(8, 512 // regs)


def is_hot(name):
    return bool(TIMED.match(name))


def sgpr_limit(name):
    if FILTERED.match(name):
        return SGPR_FILTERED
    return SGPR_TIMED if is_hot(name) else SGPR_ANY


def offenders(rows):
    return [r for r in rows if r["vgpr_spill_count"] or r["private_segment_fixed_size"] or
            r["sgpr_spill_count"] > sgpr_limit(r["kernel"])]


def markdown(rows):
    lines = ["| kernel | VGPR (of which AGPR) | SGPR | spilled VGPR | spilled SGPR | scratch B | static LDS B | max WG | waves/SIMD by registers |",
             "|---|---|---|---|---|---|---|---|---|"]
    for r in rows:
        lines.append("| `%s` | %d (%d) | %d | %d | %d | %d | %d | %d | %d |" % (
            r["kernel"], r["vgpr_count"], r["agpr_count"], r["sgpr_count"], r["vgpr_spill_count"], r["sgpr_spill_count"],
            r["private_segment_fixed_size"], r["group_segment_fixed_size"], r["max_flat_workgroup_size"], waves_per_simd(r)))
    return "\n".join(lines)


# the kernels DESIGN.md's register table shows: what the BASELINE configurations launch in their timed regions
DESIGN = re.compile(
    r"^sdb::(k_greedy_search<sdb::PlainDist<(3|6), (false|true), true, (0, \(sdb::Stage\)0|4, \(sdb::Stage\)1)>, 2, false, 8192u>"
    r"|k_greedy_search<sdb::Int8Dist<3>, 2, false, 8192u>"
    r"|k_greedy_search_wide<3, false, (8|16), false>|k_greedy_search_pq2<4294967295u>"
    r"|k_greedy_search_pqw<15, 33, 4294967295u, 4, 15, true>|k_pq_lut_t<true, (3, 96|0, 4)>|k_pq_encode_t<true, 3, true>"
    r"|k_pq_encode_pair<true, 4>|k_km_assign_t<(3, 96|0, 4)>|k_backedges<3, false>|k_prune_new<3, false>"
    r"|k_prune_new_tiled<3, false, false, 8>|k_flat_scan_mfma<12, false>|k_flat_scan<false>|k_k1_stream_mfma<12>"
    r"|k_k1_tile_mfma<12, false>|k_topk_merge)")
BEGIN, END = "<!-- kernel_table:begin (python3 tools/kernel_table.py --design) -->", "<!-- kernel_table:end -->"


def design_block(rows):
    sel = [r for r in rows if DESIGN.match(r["kernel"])]
    worst_t = max([r["sgpr_spill_count"] for r in rows if is_hot(r["kernel"]) and not FILTERED.match(r["kernel"])] or [0])
    worst = max([r["sgpr_spill_count"] for r in rows] or [0])
    head = ("%d kernels in the library; %d with spilled VGPRs or scratch memory; most spilled SGPRs: %d on a timed path, "
            "%d anywhere.\n\n" % (len(rows), sum(1 for r in rows if r["vgpr_spill_count"] or r["private_segment_fixed_size"]),
                                  worst_t, worst))
    return BEGIN + "\n" + head + markdown(sel) + "\n" + END


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--so", default=SO)
    ap.add_argument("--all", action="store_true")
    ap.add_argument("--match", default=None, help="regular expression on the demangled name")
    ap.add_argument("--json", default=None)
    ap.add_argument("--check", action="store_true")
    ap.add_argument("--design", action="store_true", help="the block DESIGN.md carries between its kernel_table markers")
    ap.add_argument("--memory-ops", action="store_true", help="the walk kernels' memory instructions and the staged hop's load schedule")
    a = ap.parse_args()
    if a.memory_ops:
        rows = memory_ops(a.so)
        if a.json:
            with open(a.json, "w") as f:
                json.dump(rows, f, indent=1)
        print("| kernel | flat | global load | global store | global atomic | s_load | LDS | copy-row loads in the hop's run | vmcnt waits before the visited-set test |")
        print("|---|---|---|---|---|---|---|---|---|")
        for r in rows:
            st = r.get("stage", "")
            print("| `%s` | %d | %d | %d | %d | %d | %d | %s | %s |" % (
                r["kernel"], r["flat_"], r["global_load"], r["global_store"], r["global_atomic"], r["s_load"], r["ds_"],
                "" if st == "" else ("not found" if st is None else st["loads"]),
                "" if not st else (", ".join(st["vm_waits"]) or "none")))
        return 0
    rows = kernels(a.so)
    if a.design:
        print(design_block(rows))
        return 0
    if a.check:
        bad = offenders(rows)
        for r in bad:
            print("SPILL %s: %d VGPRs spilled, %d B scratch, %d SGPRs spilled (limit %d)" % (
                r["kernel"], r["vgpr_spill_count"], r["private_segment_fixed_size"], r["sgpr_spill_count"], sgpr_limit(r["kernel"])))
        print("%d kernels, %d on timed paths, %d with scratch, spilled VGPRs or too many spilled SGPRs; most SGPRs spilled: "
              "%d on a timed path, %d anywhere" % (
                  len(rows), sum(is_hot(r["kernel"]) for r in rows), len(bad),
                  max([r["sgpr_spill_count"] for r in rows if is_hot(r["kernel"]) and not FILTERED.match(r["kernel"])] or [0]),
                  max([r["sgpr_spill_count"] for r in rows] or [0])))
        return 1 if bad else 0
    sel = rows
    if a.match:
        sel = [r for r in rows if re.search(a.match, r["kernel"])]
    elif not a.all:
        sel = [r for r in rows if re.match(r"^sdb::(k_greedy_search|k_backedges|k_prune_new|k_pq_lut|k_flat_scan|k_k1_)", r["kernel"])]
    if a.json:
        with open(a.json, "w") as f:
            json.dump(sel, f, indent=1)
    print(markdown(sel))
    return 0


if __name__ == "__main__":
    sys.exit(main())
