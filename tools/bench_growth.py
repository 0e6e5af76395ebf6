"""One reserve doubling of a 2^20 x 128 table and one compaction of it with a tenth of its rows deleted; one JSON line.
usage: [SEMADB_AMD_LIB=<library of another commit>] python tools/bench_growth.py"""
import json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import bench
from semadb_amd import vamana
n, d = (1 << 20) - 1, 128  # with the start node exactly the 2^20 rows the tables are created with
base = bench.gen_rows(n + 8, d, 20250620, "latent:24", "cuda:0")
ix = vamana.NewIndexVamana("grow", vamana.IndexVectorVamanaParameters(d, "cosine", 75, 64, 1.2), capacity=n + 1, strict=True)
ix.set_start(bench.start_vector(d))
ix.insert_batch(None, base[:n])
torch.cuda.synchronize()
size0 = ix.SizeInMemory()
t0 = time.perf_counter()
ix.insert_batch(None, base[n:n + 8])  # one row more than the tables hold: they double
torch.cuda.synchronize()
t_grow = time.perf_counter() - t0
assert ix.SizeInMemory() > size0
t0 = time.perf_counter()
ix.insert_batch(None, base[:8].flip(0).contiguous())  # the same call without growth
torch.cuda.synchronize()
t_same = time.perf_counter() - t0
dels = np.random.default_rng(1).choice(np.arange(2, n + 2, dtype=np.uint64), n // 10, replace=False)
ix.delete_batch(dels)
torch.cuda.synchronize()
t0 = time.perf_counter()
ix.compact()
torch.cuda.synchronize()
t_compact = time.perf_counter() - t0
assert ix.row_usage()[1] == 0
print(json.dumps({"lib": os.environ.get("SEMADB_AMD_LIB", "this"), "grow_insert_ms": round(t_grow * 1e3, 2), "insert_without_growth_ms": round(t_same * 1e3, 2),
                  "compact_ms": round(t_compact * 1e3, 2)}))
ix.close()
