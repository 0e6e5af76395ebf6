#!/usr/bin/env python3
"""Re-ranked quantized search (sdb_index_search_batch_rerank) against the un-re-ranked call and the full-precision walk,
on ONE graph per table in ONE run:

    bq: 1M x 384 cosine, binary quantizer (hamming)        -- tools/bench_bq.py's table
    pq: 1M x 768 cosine, product quantizer M = 192, K = 256  -- tools/bench_pq.py's table

searchSize 75, limit 10, batches of 1 024 device-resident queries.  Per table: the full-precision walk at searchSize
10 .. 75 (its recall / speed curve: the other end, and what "equal recall" is read from), then -- attaching is one-way --
the quantized walk un-re-ranked and with rerank 10 / 25 / 50 / 75, the variants taking turns inside every repetition
(the order rotates).  Per variant: queries/s of the whole call (torch events around the batches: table build, walk,
re-rank, nothing copied) and of the kernels alone (HIP events of sdb_index_set_profiling: a re-ranked call records the
walk and the re-rank kernel separately), every repetition's figure, the median and the spread; recall@10 against the
exact float top 10.  The re-rank kernel's bytes are nq * rerank * ld * 4 (the rows it has to read; the candidates of one
batch overlap, so HBM sees fewer) over its time, set against the best figure tools/gather_ceiling.py reaches for the same
row size on the same device (run first, as a process of its own).

    python3 tools/bench_rerank.py --out profiles/rerank.json"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

import bench
from semadb_amd import vectorstore as vs

ap = argparse.ArgumentParser()
ap.add_argument("--rows", type=int, default=1_000_000)
ap.add_argument("--tables", default="bq,pq")
ap.add_argument("--batches", type=int, default=8)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--no-ceiling", action="store_true", help="skip tools/gather_ceiling.py (fractions are left out)")
ap.add_argument("--out", default=None)
a0 = ap.parse_args()

NQ, LIMIT, SS = 1024, 10, 75
RERANKS = (10, 25, 50, 75)
FLOAT_SS = (10, 15, 25, 50, 75)
dev = "cuda:0"


class A:
    metric, search_size, degree_bound, alpha = "cosine", SS, 64, 1.2


def gather_ceiling():
    """{d: best GB/s of tools/gather_ceiling.py over its occupancies} for 1M-row slabs"""
    if a0.no_ceiling:
        return {}
    res = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gather_ceiling.py")], capture_output=True, text=True, check=True)
    rec = json.loads(res.stdout[res.stdout.index("{"):])
    out = {}
    for key, val in rec.items():
        d, n = int(key.split()[0][2:]), int(key.split()[1][2:])
        if n == 1000000:
            out[d] = max(v for k, v in val.items() if k.startswith("waves="))
    return out


def stats(v):
    v = [float(x) for x in v]
    return {"each": [round(x, 4) for x in v], "median": round(float(np.median(v)), 4), "min": round(min(v), 4),
            "spread": round(max(v) - min(v), 4)}


def run_variant(ix, queries, ss, rerank):
    """one pass over the batches: (call ms per batch, walk kernel ms per batch, re-rank kernel ms per batch or None, ids)"""
    ix.profile_read()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    got = []
    e0.record()
    for b in range(queries.shape[0]):
        got.append(ix.search_batch(queries[b], LIMIT, ss, rerank=rerank)[0])
    e1.record()
    torch.cuda.synchronize()
    ms = ix.profile_read()
    call = e0.elapsed_time(e1) / queries.shape[0]
    if rerank is None:
        assert len(ms) == queries.shape[0]
        return call, float(np.mean(ms)), None, got
    assert len(ms) == 2 * queries.shape[0]
    return call, float(np.mean(ms[0::2])), float(np.mean(ms[1::2])), got


def recall(got, truth):
    ids = torch.cat(got).to(torch.int64)
    return float((ids.unsqueeze(2) == truth.unsqueeze(1)).any(2).sum().item()) / (ids.shape[0] * LIMIT)


def measure(ix, queries, truth, variants, ld, ceiling):
    """variants: [(name, searchSize, rerank or None)], taking turns inside every repetition"""
    for name, ss, r in variants:  # warm-up: every shape the timed window uses
        for _ in range(2):
            run_variant(ix, queries[:2], ss, r)
    acc = {name: {"call": [], "walk": [], "rerank": [], "recall": None} for name, _, _ in variants}
    for rep in range(a0.reps):
        k = rep % len(variants)
        for name, ss, r in variants[k:] + variants[:k]:
            call, walk, rr, got = run_variant(ix, queries, ss, r)
            acc[name]["call"].append(call), acc[name]["walk"].append(walk)
            if rr is not None:
                acc[name]["rerank"].append(rr)
            if acc[name]["recall"] is None:
                acc[name]["recall"] = recall(got, truth)
    out = {}
    for name, ss, r in variants:
        v = acc[name]
        rec = {"search_size": ss, "rerank": r, "recall_at_10": round(v["recall"], 4), "call_ms": stats(v["call"]),
               "walk_kernel_ms": stats(v["walk"])}
        rec["call_qps_at_median"] = round(NQ / rec["call_ms"]["median"] * 1e3)
        kern = rec["walk_kernel_ms"]["median"]
        if r is not None:
            rec["rerank_kernel_ms"] = stats(v["rerank"])
            t = rec["rerank_kernel_ms"]["median"]
            kern += t
            rec["rerank_row_bytes"] = NQ * r * ld * 4
            rec["rerank_GBps"] = round(NQ * r * ld * 4 / t / 1e6, 1)
            if ceiling:
                rec["rerank_fraction_of_gather_ceiling"] = round(rec["rerank_GBps"] / ceiling, 4)
        rec["kernel_qps_at_median"] = round(NQ / kern * 1e3)
        out[name] = rec
    return out


def verdict(float_curve, quantized):
    """per re-ranked point: the fastest full-precision point (whole call) that reaches its recall, and who wins"""
    out = {}
    for name, p in quantized.items():
        if p["rerank"] is None:
            continue
        reach = [(f["call_qps_at_median"], n) for n, f in float_curve.items() if f["recall_at_10"] >= p["recall_at_10"]]
        best = max(reach) if reach else None
        out[name] = {"recall_at_10": p["recall_at_10"], "call_qps": p["call_qps_at_median"],
                     "fastest_full_precision_with_that_recall": None if best is None else
                     {"variant": best[1], "call_qps": best[0], "recall_at_10": float_curve[best[1]]["recall_at_10"]},
                     "reranked_quantized_wins": best is None or p["call_qps_at_median"] > best[0]}
    return out


def say(*what):
    print(*what, file=sys.stderr, flush=True)


def table(name, d, attach):
    say("table", name, "rows", a0.rows, "dim", d)
    base = bench.gen_rows(a0.rows, d, 20250620, "latent:24", dev)
    queries = bench.gen_rows(a0.batches * NQ, d, 20250621, "latent:24", dev).view(a0.batches, NQ, d)
    ix, build_s = bench.build_index(A, base, 0, strict=False)
    truth = bench.exact_topk(queries.view(-1, d), base, LIMIT)[1] + 2  # row i has id i + 2
    ix.set_profiling(True)
    ld = ((d // 32 + 3) // 4) * 128 + (32 if d % 32 else 0)  # floats of one slab row (d = 384, 768: no padding)
    ceiling = CEILING.get(d)
    rec = {"workload": "%d x %d cosine latent:24, searchSize %d, limit %d, %d batches of %d queries, %d repetitions" %
                       (a0.rows, d, SS, LIMIT, a0.batches, NQ, a0.reps),
           "build_s": round(build_s, 2), "gather_ceiling_GBps": ceiling}
    say("built in %.1f s; full-precision walk" % build_s)
    rec["full_precision"] = measure(ix, queries, truth, [("searchSize %d" % s, s, None) for s in FLOAT_SS], ld, ceiling)
    rec["full_precision_reranked"] = measure(ix, queries, truth, [("rerank 75", SS, 75)], ld, ceiling)  # (a plain store: the same answer)
    rec["quantizer"] = attach(ix, base, d)
    say("quantizer attached:", rec["quantizer"]["kind"])
    variants = [("un-re-ranked", SS, None)] + [("rerank %d" % r, SS, r) for r in RERANKS]
    rec["quantized"] = measure(ix, queries, truth, variants, ld, ceiling)
    rec["at_equal_recall"] = verdict(rec["full_precision"], rec["quantized"])
    rec["reranked_quantized_beats_full_precision_at_equal_recall"] = any(v["reranked_quantized_wins"] for v in rec["at_equal_recall"].values())
    ix.close()
    del base, queries
    torch.cuda.empty_cache()
    return rec


def attach_bq(ix, base, d):
    bq = vs.BinaryQuantizer(vs.BinaryQuantizerParameters(None, 0, "hamming"), d)
    vs.attach_binary(ix, bq)
    return {"kind": "binary, hamming", "bytes_per_code_row": bq.W * 8, "bytes_per_float_row": d * 4}


def attach_pq(ix, base, d, M=192, K=256, train_rows=10000):
    train = base[:train_rows].cpu().numpy().copy()
    pq = vs.ProductQuantizer("cosine", vs.ProductQuantizerParameters(K, M, train_rows), d)
    pq.Fit(train, np.arange(M) * 7 % train_rows, alias=True)
    vs.attach(ix, pq)
    return {"kind": "product, M = %d, K = %d, fitted on the first %d rows" % (M, K, train_rows), "bytes_per_code_row": M,
            "bytes_per_float_row": d * 4}


say("gather ceiling (tools/gather_ceiling.py)")
CEILING = gather_ceiling()
say(CEILING)
out = {"device": torch.cuda.get_device_name(0),
       "method": "full-precision walk first (attaching a quantizer is one-way), then the quantized variants taking turns "
                 "inside every repetition; medians over the repetitions, spread = max - min; call = torch events around "
                 "the batches of one pass, kernels = the library's HIP events (walk, re-rank kernel)"}
for t in a0.tables.split(","):
    out[t] = table(t, 384, attach_bq) if t == "bq" else table(t, 768, attach_pq)
text = json.dumps(out, indent=1)
print(text)
if a0.out:
    with open(a0.out, "w") as f:
        f.write(text + "\n")
