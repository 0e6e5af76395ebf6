#!/usr/bin/env python3
"""Filtered search (search.go:33-51,93-95) at C2: 1M x 384 cosine, searchSize 75, batch 1024, filters of 10 / 1 000 /
100 000 ids per query.  Reports the K2 kernel time (HIP events around the launch) and the whole call (which includes the
host-side translation of the filter ids to slots -- filter arrays are host memory in the ABI, like the reference's
roaring bitmap).  BENCH_TUNE=no_hash=1 gives the bitset variant of round 2 for comparison.

--sketch: the two-precision hop on filtered calls against the float32 walk (SDB_TUNE_SKETCH 1 against 0) in ONE process,
the two alternating --reps times per filter size: per repetition the mean kernel and call time of three batches, their
minimum and median per knob, the spread (max - min) of the knob-0 repetitions -- the yardstick a difference has to beat --
and the neighbours discarded on their float16 distance over the distances the reference evaluates."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import bench

ap = argparse.ArgumentParser()
ap.add_argument("--rows", type=int, default=1_000_000)
ap.add_argument("--dim", type=int, default=384)
ap.add_argument("--sizes", default="10,1000,100000")
ap.add_argument("--holes", type=int, default=0, help="delete this many rows first: ids are no longer consecutive (id -> slot table on the device)")
ap.add_argument("--host-filters", action="store_true", help="the host's translation (tuning host_filters)")
ap.add_argument("--pinned", action="store_true", help="the filter arrays in page-locked host memory (what sdb_host_alloc gives a host program)")
ap.add_argument("--sketch", action="store_true", help="knob 0 against knob 1, alternating in this process (see above)")
ap.add_argument("--reps", type=int, default=5, help="--sketch: repetitions per knob and filter size")
a0 = ap.parse_args()


class A:
    metric, search_size, degree_bound, alpha = "cosine", 75, 64, 1.2


dev = "cuda:0"
base = bench.gen_rows(a0.rows, a0.dim, 20250620, "latent:24", dev)
queries = bench.gen_rows(4 * 1024, a0.dim, 20250621, "latent:24", dev).view(4, 1024, a0.dim)
ix, build_s = bench.build_index(A, base, 0)
out = {"rows": a0.rows, "dim": a0.dim, "build_s": round(build_s, 2), "tuning": os.environ.get("BENCH_TUNE", "")}
rng = np.random.default_rng(3)
if a0.holes:
    ix.delete_batch(np.sort(rng.choice(a0.rows, size=a0.holes, replace=False).astype(np.uint64) + 2))
    out["holes"] = a0.holes
if a0.host_filters:
    ix.set_tuning("host_filters", 1)
    out["host_filters"] = True
ix.set_profiling(True)
# unfiltered reference point
for b in range(2):
    ix.search_batch(queries[b], 10, 75)
torch.cuda.synchronize()
ix.profile_read()
for b in range(4):
    ix.search_batch(queries[b], 10, 75)
torch.cuda.synchronize()
out["unfiltered_kernel_ms"] = round(float(np.mean(ix.profile_read())), 4)
for size in [int(x) for x in a0.sizes.split(",")]:
    filt = [np.sort(rng.choice(a0.rows, size=size, replace=False).astype(np.uint64) + 2) for _ in range(1024)]
    off = np.zeros(1025, dtype=np.uint64)
    off[1:] = np.cumsum([len(f) for f in filt])
    flat = np.concatenate(filt)
    if a0.pinned:
        keep = torch.from_numpy(flat.view(np.int64)).pin_memory()  # `keep` owns the pages
        flat = keep.numpy().view(np.uint64)
        out["pinned"] = True
    if a0.sketch:
        try:
            ix.set_tuning("sketch_filtered", 1)  # (the filtered hop is an opt-in)
        except Exception:  # a library from before the knob (a comparison run): both knobs time its float32 filtered walk
            out["sketch_filtered_knob"] = False
        rec = {0: {"kernel_ms": [], "call_ms": []}, 1: {"kernel_ms": [], "call_ms": []}}
        for rep in range(a0.reps):
            for knob in (0, 1):
                ix.set_tuning("sketch", knob)  # (0 drops the float16 copy, 1 converts the rows again: outside the timed region)
                for _ in range(3 if rep == 0 else 1):
                    ix.search_batch(queries[0], 10, 75, filters=(off, flat))
                    torch.cuda.synchronize()
                ix.profile_read()
                dt = 0.0
                for b in range(1, 4):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    ix.search_batch(queries[b], 10, 75, filters=(off, flat))
                    torch.cuda.synchronize()
                    dt += time.perf_counter() - t0
                rec[knob]["kernel_ms"].append(round(float(np.mean(ix.profile_read())), 4))
                rec[knob]["call_ms"].append(round(dt / 3 * 1e3, 3))
        before = ix.sketch_stats()[0]  # (the knob is at 1)
        _, _, _, tr = ix.search_batch(queries[1], 10, 75, filters=(off, flat), trace=True)
        torch.cuda.synchronize()
        discarded, _, in_use = ix.sketch_stats()
        n_dist = int(tr.n_dist.sum().item())
        row = {"copy_in_use": bool(in_use), "discarded": int(discarded - before), "n_dist": n_dist,
               "discarded_over_n_dist": round((discarded - before) / max(n_dist, 1), 4)}
        for knob in (0, 1):
            k = rec[knob]["kernel_ms"]
            row["sketch_%d" % knob] = {"kernel_ms": k, "kernel_ms_min": min(k), "kernel_ms_median": round(float(np.median(k)), 4),
                                       "call_ms": rec[knob]["call_ms"], "call_ms_median": round(float(np.median(rec[knob]["call_ms"])), 3)}
        row["sketch_0_kernel_spread_ms"] = round(max(rec[0]["kernel_ms"]) - min(rec[0]["kernel_ms"]), 4)
        row["kernel_median_1_over_0"] = round(row["sketch_1"]["kernel_ms_median"] / row["sketch_0"]["kernel_ms_median"], 4)
        out["filter_%d" % size] = row
        continue
    for _ in range(3):  # the first filtered calls size their workspaces (bitsets for the spill path, filter arrays)
        ix.search_batch(queries[0], 10, 75, filters=(off, flat))
        torch.cuda.synchronize()
    ix.profile_read()
    hits, dt = 0, 0.0
    for b in range(1, 4):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ids, d, c, _ = ix.search_batch(queries[b], 10, 75, filters=(off, flat))
        torch.cuda.synchronize()
        dt += time.perf_counter() - t0
        # outside the timed region: torch loads the module of its reduction kernel on first use (~80 ms), which round 3's
        # version of this loop charged to the first filter size it measured (the "filter_10 outlier")
        hits += int(c.sum().item()) if hasattr(c, "sum") else 0
    dt /= 3
    kms = float(np.mean(ix.profile_read()))
    out["filter_%d" % size] = {"kernel_ms": round(kms, 4), "kernel_qps": round(1024 / kms * 1e3, 1),
                               "call_ms": round(dt * 1e3, 2), "call_qps": round(1024 / dt, 1),
                               "mean_results": round(hits / 3 / 1024, 2), "upload_MB": round(flat.nbytes / 1e6, 1)}
    # the same filters as bitmaps (sdb_index_search_batch_bitmap)
    from semadb_amd import vamana
    bm = vamana.FilterBitmaps.from_sets(filt)
    if a0.pinned:
        keep_w = torch.from_numpy(bm.words.view(np.int64)).pin_memory()
        bm = vamana.FilterBitmaps(bm.first_id, bm.word_offsets, keep_w.numpy().view(np.uint64))
    for _ in range(2):
        ix.search_batch(queries[0], 10, 75, filters=bm)
        torch.cuda.synchronize()
    ix.profile_read()
    dt = 0.0
    for b in range(1, 4):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ix.search_batch(queries[b], 10, 75, filters=bm)
        torch.cuda.synchronize()
        dt += time.perf_counter() - t0
    dt /= 3
    kms = float(np.mean(ix.profile_read()))
    out["filter_%d" % size]["as_bitmaps"] = {"kernel_ms": round(kms, 4), "call_ms": round(dt * 1e3, 2),
                                             "upload_MB": round(bm.words.nbytes / 1e6, 1)}
print(json.dumps(out, indent=1))
