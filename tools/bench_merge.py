#!/usr/bin/env python3
"""Times the shard fan-out merge (cluster.topk_merge -> k_topk_merge) on device tensors, one process per run:

    python3 tools/bench_merge.py                                # the fan-out's own shape: 8 shards x 10 -> 10, 1 024 queries
    python3 tools/bench_merge.py --shards 64 --per 32 --calls 20   # the kernel's largest, 2 048 items per query: milliseconds per call
    SEMADB_AMD_LIB=/path/to/another/libsemadb_amd.so python3 tools/bench_merge.py   # the same on another build

Prints one JSON line: microseconds per call of `cluster.topk_merge` (the binding allocates its four outputs per call)
and of the bare `sdb_topk_merge` over outputs allocated once -- device events around `--calls` back-to-back calls,
`--reps` times, every repetition listed -- and a SHA-256 of the merged answer, so that two builds can be compared on
what they computed as well as on how long they took.  Inputs are finite (what a healthy fan-out merges)."""
import argparse
import ctypes as C
import hashlib
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shards", type=int, default=8)
    ap.add_argument("--per", type=int, default=10)
    ap.add_argument("--limit", type=int, default=10)
    ap.add_argument("--nq", type=int, default=1024)
    ap.add_argument("--calls", type=int, default=5000)
    ap.add_argument("--reps", type=int, default=7)
    a = ap.parse_args()
    import torch
    from semadb_amd import _buf, _lib, cluster
    from semadb_amd._lib import MEM_DEVICE, check, lib
    if _lib.device_count() < 1:
        sys.exit("bench_merge.py needs a GPU")
    rng = np.random.default_rng(8)
    d = np.sort(rng.random((a.shards, a.nq, a.per), dtype=np.float32), axis=2)
    d[:, ::3, :] = np.sort(rng.integers(0, 50, size=(a.shards, len(range(0, a.nq, 3)), a.per)).astype(np.float32) / 8, axis=2)  # ties
    ids = rng.integers(2, 10 ** 6, size=(a.shards, a.nq, a.per)).astype(np.int64)
    counts = np.full((a.shards, a.nq), a.per, dtype=np.int32)
    counts[:, 1::7] = rng.integers(0, a.per + 1, size=(a.shards, len(range(1, a.nq, 7))))
    t_ids, t_d, t_c = torch.from_numpy(ids).cuda(), torch.from_numpy(d).cuda(), torch.from_numpy(counts).cuda()
    outs = cluster.topk_merge(t_ids, t_d, t_c, a.limit)
    torch.cuda.synchronize()
    h = hashlib.sha256()
    n = outs[3].cpu().numpy()
    for o in outs[:3]:  # the slots below each query's count; what lies behind them is the caller's
        o = o.cpu().numpy()
        for q in range(a.nq):
            h.update(o[q, :n[q]].tobytes())
    h.update(n.tobytes())
    stream = _buf.current_stream(MEM_DEVICE)
    ptrs = [C.c_void_p(t.data_ptr()) for t in (t_ids, t_d, t_c)] + [C.c_void_p(o.data_ptr()) for o in outs]

    def bound():
        cluster.topk_merge(t_ids, t_d, t_c, a.limit)

    def bare():
        check(lib().sdb_topk_merge(a.shards, a.nq, a.per, ptrs[0], ptrs[1], ptrs[2], a.limit, ptrs[3], ptrs[4], ptrs[5],
                                   ptrs[6], MEM_DEVICE, 0, stream))

    def time_us(fn):
        for _ in range(min(200, a.calls)):
            fn()
        torch.cuda.synchronize()
        out = []
        for _ in range(a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.calls):
                fn()
            e1.record()
            e1.synchronize()
            out.append(round(e0.elapsed_time(e1) * 1e3 / a.calls, 4))
        return out

    res = {"lib": os.path.relpath(_lib.SO_PATH, os.path.dirname(os.path.dirname(os.path.abspath(__file__)))), "shards": a.shards, "per_shard": a.per, "limit": a.limit, "nq": a.nq, "calls": a.calls,
           "answer_sha256": h.hexdigest()}
    for name, fn in (("topk_merge_us", bound), ("bare_call_us", bare)):
        reps = time_us(fn)
        res[name] = float(np.median(reps))
        res[name + "_reps"] = reps
    print(json.dumps(res))


if __name__ == "__main__":
    main()
