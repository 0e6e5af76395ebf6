"""bench.py's command line: a plain run prints the headline alone, --full adds everything else, --dump-outputs writes
the last timed step's answers as .npy files (float32 / float64) that two runs with the same arguments reproduce."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def test_dump_outputs_writes_float_arrays(tmp_path):
    import torch
    import bench
    rng = np.random.default_rng(5)
    ids = torch.from_numpy(rng.integers(2, 1 << 40, size=(64, 10)).astype(np.int64))
    dists = torch.from_numpy(rng.standard_normal((64, 10)).astype(np.float32))
    counts = torch.from_numpy(rng.integers(0, 11, size=64).astype(np.int32))
    bench.dump_outputs(str(tmp_path / "a"), (ids, dists, None, counts), merged=False)
    got = {n: np.load(tmp_path / "a" / (n + ".npy")) for n in ("ids", "dists", "counts")}
    assert sorted(os.listdir(tmp_path / "a")) == ["counts.npy", "dists.npy", "ids.npy"]
    assert got["ids"].dtype == np.float64 and np.array_equal(got["ids"].astype(np.int64), ids.numpy())
    assert got["dists"].dtype == np.float32 and np.array_equal(got["dists"].view(np.uint32), dists.numpy().view(np.uint32))
    assert got["counts"].dtype == np.float64 and np.array_equal(got["counts"], counts.numpy())
    # a merged N > 1 answer also names the shard of every id; the replicas' gathered form has three arrays
    shards = torch.zeros((64, 10), dtype=torch.int32)
    bench.dump_outputs(str(tmp_path / "b"), (ids, dists, shards, counts), merged=True)
    assert "shards.npy" in os.listdir(tmp_path / "b")
    bench.dump_outputs(str(tmp_path / "c"), [ids, dists, counts], merged=False)
    assert sorted(os.listdir(tmp_path / "c")) == ["counts.npy", "dists.npy", "ids.npy"]


def test_dump_outputs_samples_rows_above_the_limit(tmp_path, monkeypatch):
    import torch
    import bench
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 4096)
    n = 1000
    ids = torch.arange(n * 10, dtype=torch.int64).view(n, 10)
    dists = torch.arange(n * 10, dtype=torch.float32).view(n, 10)
    counts = torch.full((n,), 10, dtype=torch.int32)
    for sub in ("a", "b"):
        bench.dump_outputs(str(tmp_path / sub), (ids, dists, None, counts), merged=False)
    a = {n_: np.load(tmp_path / "a" / (n_ + ".npy")) for n_ in ("ids", "dists", "counts")}
    assert sum(x.nbytes for x in a.values()) <= 4096 and a["ids"].shape[0] > 0
    # the same rows of every array, and the same sample each time
    assert np.array_equal(a["ids"], a["dists"].astype(np.float64))
    assert np.array_equal(a["ids"], np.load(tmp_path / "b" / "ids.npy"))


def test_dump_outputs_is_for_the_search_configuration():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--config", "c3", "--dump-outputs", "x"],
                         capture_output=True, text=True, timeout=300)
    assert out.returncode == 2 and "--dump-outputs" in out.stderr


def _run(args, timeout=900):
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, capture_output=True, text=True,
                         timeout=timeout)
    assert out.returncode == 0, out.stderr[-3000:]
    return json.loads([line for line in out.stdout.splitlines() if line.startswith("{")][-1])


@pytest.mark.gpu
def test_plain_and_full_runs_and_their_outputs(tmp_path):
    """A plain run: the headline fields, --steps timed steps, none of the extras.  --full: the roofline and its counter
    pass as well.  The answers of the last timed step are the same bits in every run with the same arguments."""
    small = ["--gpus", "1", "--steps", "7", "--warmup", "2", "--rows", "60000", "--recall-batches", "2",
             "--timed-batches", "3"]
    runs = []
    for i, extra in enumerate(([], [], ["--full", "--no-cpu-baseline", "--no-secondary", "--no-host-rates", "--c4-rows", "0"])):
        d = str(tmp_path / ("run%d" % i))
        j = _run(small + extra + ["--dump-outputs", d])
        assert j["steps"] == 7 and j["warmup"] == 2 and j["ms_per_step"] > 0 and "invalid" not in j
        assert abs(j["value"] - 1024 / (j["ms_per_step"] * 1e-3)) / j["value"] < 2e-3
        for key in ("metric", "value", "unit", "higher_is_better", "dtype"):
            assert key in j, key
        assert j["config"]["recall_at_10"] >= 0.95
        if extra:
            assert j["roofline"]["kernel"] == "k_greedy_search" and j["config"]["mean_n_dist"] > 0
            assert "two_precision_hop" in j["config"]
        else:
            for key in ("roofline", "build_roofline", "cpu_baseline", "value_host", "value_two_precision"):
                assert key not in j, key
            for key in ("flat_scan_ms", "mean_n_dist", "two_batches_in_flight_qps", "value_second_pass", "c4"):
                assert key not in j["config"], key
        runs.append({n: np.load(os.path.join(d, n + ".npy")) for n in ("ids", "dists", "counts")})
    first = runs[0]
    assert first["ids"].dtype == np.float64 and first["ids"].shape == (1024, 10)
    assert first["dists"].dtype == np.float32 and first["counts"].dtype == np.float64
    assert (first["counts"] == 10).all() and (first["ids"] >= 2).all()
    for other in runs[1:]:
        assert np.array_equal(first["ids"], other["ids"]) and np.array_equal(first["counts"], other["counts"])
        assert np.array_equal(first["dists"].view(np.uint32), other["dists"].view(np.uint32))
