#!/usr/bin/env python3
"""The binary quantizer's walk at the bench's shape: 1M x 384 cosine, searchSize 75, batches of 1 024 queries.

On ONE graph in ONE process: the kernel time per batch (HIP events around the launch, sdb_index_set_profiling) and
recall@10 against the exact float ground truth of the default float walk, then -- after sdb_index_attach_bq with an
unfitted quantizer (fit + encode of every row, timed) -- of the hamming walk.  Attaching is one-way, so the float
walk's --reps repetitions come first and the bit walk's after them; per walk the record keeps every repetition's mean
over its batches, the minimum, the median and the spread (max - min), which is what a difference has to beat.  The reference does not re-rank a binary store's
answers either, so its recall is the quantizer's, not the walk's: reported, not tuned.

    python3 tools/bench_bq.py --out profiles/bq_walk.json"""
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
ap.add_argument("--batches", type=int, default=8)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--metric", default="hamming", choices=["hamming", "jaccard"])
ap.add_argument("--out", default=None)
a0 = ap.parse_args()


class A:
    metric, search_size, degree_bound, alpha = "cosine", 75, 64, 1.2


dev = "cuda:0"
NQ = 1024
base = bench.gen_rows(a0.rows, a0.dim, 20250620, "latent:24", dev)
queries = bench.gen_rows(a0.batches * NQ, a0.dim, 20250621, "latent:24", dev).view(a0.batches, NQ, a0.dim)
ix, build_s = bench.build_index(A, base, 0)
_, truth = bench.exact_topk(queries.view(-1, a0.dim), base, 10)
truth = (truth + 2).cpu().numpy()  # row i has id i + 2
ix.set_profiling(True)


def measure():
    """(kernel ms per batch: mean over the batches, recall@10, mean distances evaluated per query)"""
    for b in range(2):
        ix.search_batch(queries[b], 10, 75)
    torch.cuda.synchronize()
    ix.profile_read()
    got = []
    for b in range(a0.batches):
        ids, _, _, _ = ix.search_batch(queries[b], 10, 75)
        got.append(ids)
    torch.cuda.synchronize()
    ms = float(np.mean(ix.profile_read()))
    ids = torch.cat(got).cpu().numpy().view(np.uint64)
    hits = sum(len(np.intersect1d(ids[i], truth[i])) for i in range(ids.shape[0]))
    _, _, _, tr = ix.search_batch(queries[0], 10, 75, trace=True)
    torch.cuda.synchronize()
    return ms, hits / (ids.shape[0] * 10), float(tr.n_dist.float().mean().item()), float(tr.n_hop.float().mean().item())


def summary(reps):
    ms = [r[0] for r in reps]
    return {"kernel_ms": [round(v, 4) for v in ms], "kernel_ms_min": round(min(ms), 4), "kernel_ms_median": round(float(np.median(ms)), 4),
            "kernel_ms_spread": round(max(ms) - min(ms), 4), "qps_at_median": round(NQ / float(np.median(ms)) * 1e3, 1),
            "recall_at_10": round(reps[0][1], 4), "mean_n_dist": round(reps[0][2], 1), "mean_n_hop": round(reps[0][3], 1)}


float_reps = [measure() for _ in range(a0.reps)]
from semadb_amd import vectorstore as vs
bq = vs.BinaryQuantizer(vs.BinaryQuantizerParameters(None, 0, a0.metric), a0.dim)
torch.cuda.synchronize()
t0 = time.perf_counter()
vs.attach_binary(ix, bq)  # fit over the 1M + 1 stored rows, then encode them
torch.cuda.synchronize()
attach_s = time.perf_counter() - t0
bit_reps = [measure() for _ in range(a0.reps)]
out = {"workload": "%d x %d cosine latent:24, searchSize 75, limit 10, %d batches of %d queries, %d repetitions" %
                   (a0.rows, a0.dim, a0.batches, NQ, a0.reps),
       "device": torch.cuda.get_device_name(0), "build_s": round(build_s, 2), "bit_metric": a0.metric,
       "words_per_code": bq.W, "bytes_per_code_row": bq.W * 8, "bytes_per_float_row": a0.dim * 4,
       "attach_s": round(attach_s, 4), "float_walk": summary(float_reps), "bit_walk": summary(bit_reps)}
out["bit_over_float_kernel_median"] = round(out["bit_walk"]["kernel_ms_median"] / out["float_walk"]["kernel_ms_median"], 4)
text = json.dumps(out, indent=1)
print(text)
if a0.out:
    with open(a0.out, "w") as f:
        f.write(text + "\n")
