"""Multi-shard path: the exchange step on 2 ranks over gloo (CPU), and the device merge kernel against
the oracle's restatement of cluster/actions.go:357-376 (GPU)."""
import os
import sys
import socket

import numpy as np
import pytest


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _shard_results(rank, nq, per):
    """deterministic per-shard top-k lists: ascending distances, ids unique per shard"""
    rng = np.random.default_rng(100 + rank)
    d = np.sort(rng.random((nq, per)).astype(np.float32), axis=1)
    ids = (rng.permutation(nq * per).reshape(nq, per) + 2).astype(np.int64)
    counts = np.full(nq, per, dtype=np.int32)
    counts[rank] = per - 3  # one ragged query per shard
    return ids, d, counts


def _worker(rank, world, port, q):
    import torch
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from semadb_amd import cluster
    nq, per = 16, 10
    ids, d, c = _shard_results(rank, nq, per)
    g_ids, g_d, g_c = cluster.allgather_topk(torch.from_numpy(ids), torch.from_numpy(d), torch.from_numpy(c))
    # the packed form bench.py uses: one all-gather of (ids | dists | counts) per batch
    blk = cluster.PackedTopK(nq, per, "cpu")
    blk.ids.copy_(torch.from_numpy(ids)); blk.dists.copy_(torch.from_numpy(d)); blk.counts.copy_(torch.from_numpy(c))
    p_ids, p_d, p_c = blk.allgather()
    assert torch.equal(p_ids, g_ids) and torch.equal(p_d, g_d) and torch.equal(p_c, g_c)
    q.put((rank, g_ids.numpy(), g_d.numpy(), g_c.numpy()))
    dist.barrier()
    dist.destroy_process_group()


def test_allgather_exchange_two_ranks_gloo(oracle):
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    world, nq, per, limit = 2, 16, 10, 10
    procs = [ctx.Process(target=_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    got = [q.get(timeout=120) for _ in range(world)]
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    expect = [_shard_results(r, nq, per) for r in range(world)]
    for rank, g_ids, g_d, g_c in got:
        # shard-major layout [world, nq, per], identical on every rank
        for s in range(world):
            assert np.array_equal(g_ids[s], expect[s][0]) and np.array_equal(g_d[s], expect[s][1])
            assert np.array_equal(g_c[s], expect[s][2])
        # merging the gathered buffer with the reference's rule gives the global top-k
        for qi in range(nq):
            m_ids, m_d, m_s = oracle.cluster_merge(g_ids[:, qi, :].astype(np.uint64), g_d[:, qi, :], g_c[:, qi], limit)
            pool = sorted((float(expect[s][1][qi, j]), s, int(expect[s][0][qi, j]))
                          for s in range(world) for j in range(int(expect[s][2][qi])))[:limit]
            assert [p[2] for p in pool] == [int(v) for v in m_ids]
            assert [p[1] for p in pool] == [int(v) for v in m_s]


def test_shard_limit_rule():
    # cluster/actions.go:291-299 through the C ABI (pure host arithmetic, no GPU needed)
    from semadb_amd import cluster
    assert cluster.shard_limit(10, 8) == 10
    assert cluster.shard_limit(100, 5) == 38
    assert cluster.shard_limit(75, 1) == 75
    assert cluster.shard_limit(100, 1, 75) == 75


@pytest.mark.gpu
@pytest.mark.parametrize("n_shards,per,limit", [(1, 10, 10), (2, 10, 10), (8, 10, 10), (8, 75, 75), (5, 38, 100)])
def test_topk_merge_matches_reference_rule(oracle, n_shards, per, limit):
    from semadb_amd import cluster
    rng = np.random.default_rng(n_shards * 100 + per)
    nq = 37
    d = np.sort(rng.integers(0, 50, size=(n_shards, nq, per)).astype(np.float32) / 8, axis=2)  # many ties
    ids = rng.integers(2, 10 ** 6, size=(n_shards, nq, per)).astype(np.uint64)
    counts = rng.integers(0, per + 1, size=(n_shards, nq)).astype(np.uint32)
    o_ids, o_d, o_s, o_c = cluster.topk_merge(ids, d, counts, limit)
    for q in range(nq):
        w_ids, w_d, w_s = oracle.cluster_merge(ids[:, q, :], d[:, q, :], counts[:, q].astype(np.int32), limit)
        n = len(w_ids)
        assert int(o_c[q]) == n
        assert np.array_equal(o_ids[q, :n], w_ids) and np.array_equal(o_d[q, :n], w_d)
        assert np.array_equal(o_s[q, :n].astype(np.int32), w_s)


@pytest.mark.gpu
def test_sharded_search_equals_single_index_union(oracle):
    """Two shards on one GPU, merged with the cluster rule, against brute force over the union: the
    fan-out path end to end (device tensors, as bench.py drives it)."""
    import torch
    from semadb_amd import cluster, vamana
    from tests.helpers import start_vector, unit_rows
    rng = np.random.default_rng(2)
    d, n = 32, 2000
    lat = rng.standard_normal((8, d)).astype(np.float32)
    def rows(m):
        x = rng.standard_normal((m, 8)).astype(np.float32) @ lat
        return (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32)
    shards = [rows(n), rows(n)]
    q = rows(64)
    res = []
    for s, base in enumerate(shards):
        ix = vamana.NewIndexVamana("s%d" % s, vamana.IndexVectorVamanaParameters(d, "cosine", 75, 64, 1.2))
        ix.set_start(start_vector(rng, d))
        ix.insert_batch(None, base)
        ids, dist, cnt, _ = ix.search_batch(torch.from_numpy(q).cuda(), 10, 75)
        res.append((ids, dist, cnt))
        ix.close()
    g_ids = torch.stack([r[0] for r in res]); g_d = torch.stack([r[1] for r in res]); g_c = torch.stack([r[2] for r in res])
    m_ids, m_d, m_s, m_c = cluster.topk_merge(g_ids, g_d, g_c, 10)
    torch.cuda.synchronize()
    m_ids, m_s = m_ids.cpu().numpy(), m_s.cpu().numpy()
    hits = 0
    for i in range(64):
        sims = np.concatenate([q[i] @ shards[0].T, q[i] @ shards[1].T])
        top = np.argsort(-sims)[:10]
        truth = set((int(t // n), int(t % n) + 2) for t in top)
        hits += len(truth & set((int(m_s[i, j]), int(m_ids[i, j])) for j in range(10)))
    assert hits / 640 >= 0.95


@pytest.mark.gpu
def test_topk_merge_with_repeated_items(oracle):
    """a caller may hand in the same (distance, shard, id) twice (a shard's own search never does): every item
    still lands on a position of its own (found by tools/fuzz_parity.py, seed 301 trial 83)"""
    from semadb_amd import cluster
    n_shards, nq, per, limit = 3, 5, 8, 20
    d = np.zeros((n_shards, nq, per), dtype=np.float32)
    d[:, :, 4:] = -0.375
    d = np.sort(d, axis=2)
    ids = np.full((n_shards, nq, per), 7, dtype=np.uint64)
    ids[:, :, ::3] = 9
    counts = np.full((n_shards, nq), per, dtype=np.uint32)
    o_ids, o_d, o_s, o_c = cluster.topk_merge(ids, d, counts, limit)
    for q in range(nq):
        w_ids, w_d, w_s = oracle.cluster_merge(ids[:, q, :], d[:, q, :], counts[:, q].astype(np.int32), limit)
        assert int(o_c[q]) == len(w_ids) == limit
        assert np.array_equal(o_ids[q], w_ids) and np.array_equal(o_d[q], w_d)
        assert np.array_equal(o_s[q].astype(np.int32), w_s)


def test_bench_summary_keys_are_scalars_and_extras_are_single_gpu_only():
    """The driver's record keeps the scalars of `config`: bench.flatten_summary repeats the figures a reader needs as
    scalars in front; and every single-GPU extra of measure_mode is gated on world == 1 (the 8-GPU lease runs three
    modes, each a build of its own -- DESIGN 6 budgets its wall time from a one-rank rehearsal)."""
    import re
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, root)
    import bench
    res = {"value_host": 990000.0, "build_roofline": {"frac": 0.62, "frac_mixed": 0.82, "hbm_unique_bytes": 8, "build_s": 1.6},
           "config": {"workload": "w", "mode": "shards", "dataset": "d", "recall_at_10": 0.98, "x": {"nested": 1},
                      "secondary_datasets": {"gaussian": {"qps": 6.0, "recall_at_10": 0.03, "search_size_for_recall_0.95": "none <= 512"}},
                      "c4": {"M=8": {"call_qps": 2.0, "kernel_ms": 0.3, "recall_at_10": 0.1, "traffic_over_algorithmic": 1.26,
                                     "roofline": {"frac": 0.02}},
                             "M=192": {"call_qps": 9.0, "kernel_ms": 1.0, "lookups_per_s": 0.8, "bound_by": "latency"}},
                      "latency_ms": {"workgroup_per_query": {"1": 0.32, "256": 0.38}, "host_memory_call": {"1": 0.35}}}}
    bench.flatten_summary(res)
    keys = list(res["config"])
    assert keys[:4] == ["workload", "mode", "dataset", "recall_at_10"] and keys[4] == "value_host"
    cfg = res["config"]
    assert cfg["gaussian_search_size_for_recall_0.95"] == "none <= 512" and cfg["c4_M8_traffic_over_algorithmic"] == 1.26
    assert cfg["c4_M192_lookups_per_s"] == 0.8 and cfg["latency_ms_1_queries"] == 0.32 and cfg["build_roofline_frac"] == 0.62
    assert keys.index("c4_M8_call_qps") < keys.index("x")  # the scalars come before the nested objects
    src = open(os.path.join(root, "bench.py")).read()
    for guard in re.findall(r"if rank == 0 and world == 1 and primary[^\n]*", src):
        assert "rehearse" in guard
    assert len(re.findall(r"if rank == 0 and world == 1 and primary", src)) == 2


def test_bench_starts_its_own_ranks_when_no_launcher_did(monkeypatch, capsys):
    """`python3 bench.py --gpus N` (the shape of the driver's single-GPU command, with N > 1): bench.py builds the
    torch.distributed.run command line itself and runs it as a CHILD process before touching the GPU, relays the
    child's stdout line and returns its exit code -- instead of a usage message and rc 1."""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, root)
    import bench
    cmd = bench.torchrun_command(8, ["--gpus", "8", "--steps", "20", "--warmup", "3"], port=29511)
    assert cmd[:3] == [sys.executable, "-m", "torch.distributed.run"]
    assert "--nnodes=1" in cmd and cmd[cmd.index("--nproc-per-node") + 1] == "8"
    assert cmd[cmd.index("--master-addr") + 1] == "127.0.0.1" and cmd[cmd.index("--master-port") + 1] == "29511"
    i = cmd.index(os.path.join(root, "bench.py"))
    assert cmd[i + 1:] == ["--gpus", "8", "--steps", "20", "--warmup", "3"]
    # main() takes that path exactly when WORLD_SIZE is absent and --gpus > 1, and never imports a GPU call before it
    seen = {}

    class FakeProc:
        stdout = iter(['{"metric": "relayed"}\n'])

        def wait(self):
            return 7

    def fake_popen(cmd, **kw):
        seen["cmd"], seen["kw"] = cmd, kw
        return FakeProc()

    monkeypatch.delenv("WORLD_SIZE", raising=False)
    monkeypatch.setattr(subprocess, "Popen", fake_popen)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "4", "--steps", "2", "--warmup", "1"])
    import torch
    monkeypatch.setattr(torch.cuda, "set_device", lambda *a, **k: (_ for _ in ()).throw(AssertionError("GPU touched before the relaunch")))
    with pytest.raises(SystemExit) as ei:
        bench.main()
    assert ei.value.code == 7
    assert seen["cmd"][seen["cmd"].index("--nproc-per-node") + 1] == "4" and seen["cmd"][-6:] == sys.argv[1:]
    assert seen["kw"]["env"]["HSA_ENABLE_IPC_MODE_LEGACY"] == "0"
    assert '{"metric": "relayed"}' in capsys.readouterr().out
    # under a launcher (WORLD_SIZE set) nothing is relaunched
    monkeypatch.setenv("WORLD_SIZE", "4")
    seen.clear()
    with pytest.raises(AssertionError, match="GPU touched"):
        bench.main()
    assert not seen


def _identity_worker(rank, world, port, q):
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), LOCAL_RANK=str(rank), WORLD_SIZE=str(world))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    import bench
    infos = [None] * world
    dist.all_gather_object(infos, bench.rank_identity(rank))  # (no GPU here: ordinal only, no PCI id, no communicator)
    q.put((rank, bench.judge_ranks(infos, world, native=False)))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("world", [2, 8])
def test_n_gpu_line_diagnoses_its_ranks(world):
    """config.rccl of the N > 1 line (bench.rank_identity gathered over the process group, bench.judge_ranks): the keys
    the unattended 8-GPU run will carry, and the conditions that make the line invalid instead of plausible."""
    import torch.multiprocessing as mp
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, root)
    import bench
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_identity_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    got = dict(q.get(timeout=180) for _ in range(world))
    for p in procs:
        p.join(timeout=60)
    for r in range(world):
        rccl, bad = got[r]
        assert bad is None and [x["rank"] for x in rccl["ranks"]] == list(range(world))
        assert [x["device_ordinal"] for x in rccl["ranks"]] == list(range(world))
    # what a healthy RCCL run reports ...
    tr = "rccl 2.22.3 (/opt/rocm/lib/librccl.so.1): ncclAllGather, communicator of %d ranks, this is rank 0 on GPU 0" % world
    infos = [{"rank": r, "local_rank": r, "device_ordinal": r, "pci_bus_id": "0000:%02x:00" % (5 + r), "cluster_rank": r,
              "cluster_world": world, "cluster_device": r, "transport": tr} for r in range(world)]
    rccl, bad = bench.judge_ranks(infos, world, native=True)
    assert bad is None and rccl["nccl_version"] == "2.22.3" and rccl["ranks_seen_by_cluster_info"] == list(range(world))
    assert rccl["transport"] == tr
    # ... and what must not pass for a measurement: a rank missing from the communicator, a communicator of another size,
    # two ranks on one device
    dup = [dict(i) for i in infos]
    dup[1]["cluster_rank"] = 0
    assert "sdb_cluster_info" in bench.judge_ranks(dup, world, native=True)[1]
    small = [dict(i) for i in infos]
    small[0]["cluster_world"] = world - 1
    assert "communicator" in bench.judge_ranks(small, world, native=True)[1]
    same = [dict(i) for i in infos]
    same[1]["pci_bus_id"] = same[0]["pci_bus_id"]
    assert "same device" in bench.judge_ranks(same, world, native=True)[1]
    assert bench.judge_ranks(same, world, native=True, shared_device_ok=True)[1] is None
    assert "ranks gathered" in bench.judge_ranks(infos[1:], world, native=True)[1]


@pytest.mark.gpu
@pytest.mark.parametrize("world", [2, 8])
def test_bench_without_a_launcher_runs_all_its_ranks(world):
    """`python3 bench.py --gpus N` with NO torchrun on the command line, N ranks sharing this GPU over gloo: the line
    comes back through the self-started launcher, the merge saw every rank's block (ranks_seen == [0..N-1]) and at 8
    shards the per-shard limit is the reference's int(10/8*1.42+10) -> 10 (cluster/actions.go:291-299)."""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, BENCH_BACKEND="gloo")
    env.pop("WORLD_SIZE", None)
    rows = 60000 * world
    cmd = [sys.executable, os.path.join(root, "bench.py"), "--gpus", str(world), "--steps", "4", "--warmup", "1",
           "--rows", str(rows), "--mode", "shards", "--recall-batches", "2", "--timed-batches", "3", "--full"]
    out = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-3000:]
    line = [l for l in out.stdout.splitlines() if l.startswith("{")][-1]
    j = json.loads(line)
    assert j["n_gpus"] == world and j["config"]["mode"] == "shards" and "invalid" not in j
    assert j["config"]["ranks_seen"] == list(range(world)) and "tag check" in j["config"]["exchange"]
    assert j["config"]["recall_at_10"] >= 0.95
    assert j["config"]["per_shard_limit"] == min(10, int(10 / world * 1.42 + 10))
    # the line diagnoses itself: every rank's identity, what the exchange alone costs (round 6)
    rccl = j["config"]["rccl"]
    assert [r["rank"] for r in rccl["ranks"]] == list(range(world)) and rccl["shared_device_ok"] is True
    assert all(r["device_ordinal"] == 0 for r in rccl["ranks"]) and rccl["allgather_merge_us_per_batch"] > 0


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["all", "shards", "replicas"])
def test_bench_two_ranks_over_gloo(mode, tmp_path):
    """bench.py --gpus 2 end to end with two ranks sharing this GPU (BENCH_BACKEND=gloo; RCCL refuses two ranks on
    one device): the N > 1 modes of SURVEY 8e produce a valid line whose merged answers recall the exact top-k of
    the whole database, and `value` is the user-visible rate, not a per-shard sum."""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, BENCH_BACKEND="gloo")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr",
           "127.0.0.1", "--master-port", str(_free_port()), os.path.join(root, "bench.py"), "--gpus", "2", "--steps", "6",
           "--warmup", "2", "--rows", "120000", "--mode", mode, "--recall-batches", "3", "--timed-batches", "4",
           "--c5-rows", "60000"]
    out = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    line = [l for l in out.stdout.splitlines() if l.startswith("{")][-1]
    j = json.loads(line)
    assert j["n_gpus"] == 2 and j["scaling"] == "strong" and j["config"]["mode"] == ("shards" if mode == "all" else mode)
    assert j["config"]["recall_at_10"] >= 0.95 and "invalid" not in j
    assert abs(j["value"] - 1024 * j["steps"] / (j["ms_per_step"] * j["steps"] * 1e-3)) / j["value"] < 1e-3
    if mode != "replicas":
        assert j["config"]["per_shard_walk_qps"] == pytest.approx(2 * j["value"], rel=1e-3)
        assert j["config"]["ranks_seen"] == [0, 1] and "tag check" in j["config"]["exchange"]
    if mode == "all":  # the whole SURVEY 8e record in one line: shards (primary) + replicas + c5
        assert j["config"]["primary_mode"] == "shards" and sorted(j["config"]["modes"]) == ["c5", "replicas"]
        rep, c5 = j["config"]["modes"]["replicas"], j["config"]["modes"]["c5"]
        assert rep["recall_at_10"] >= 0.95 and rep["value"] > 0 and rep["scaling"] == "strong"
        assert c5["recall_at_10"] >= 0.95 and c5["value"] > 0 and c5["scaling"] == "weak" and c5["ranks_seen"] == [0, 1]
        assert "120000 rows in all" in c5["workload"] and "2 shard(s) x 60000" in c5["workload"]
        # the N > 1 line carries its wall time by phase and mode, and none of the single-GPU extras (they would put
        # the driver's 8-GPU lease at risk: secondary datasets, the 10M x 768 C4 point, side kernels, the CPU baseline)
        cfg = j["config"]
        assert all(m in cfg["wall_s_by_phase"] for m in ("shards:", "replicas:", "c5:")) and cfg["wall_s_total"] > 0
        for extra in ("c4", "secondary_datasets", "side_kernels", "latency_ms", "host_qps", "two_batches_in_flight_qps"):
            assert extra not in cfg, extra
        assert "cpu_baseline" not in j
        assert cfg["replicas_qps"] == rep["value"] and cfg["c5_qps"] == c5["value"]


def _gloo_exchange_worker(rank, world, port, q):
    """two processes share the GPU; gloo carries the blocks, the library stamps and checks the tags"""
    import torch
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from semadb_amd import cluster
    from semadb_amd._lib import SemaDBError
    torch.cuda.set_device(0)
    nq, per, limit, dim = 16, 10, 10, 24
    ids, d, c = _shard_results(rank, nq, per)
    blk = cluster.PackedTopK(nq, per, "cuda:0")
    blk.ids.copy_(torch.from_numpy(ids)); blk.dists.copy_(torch.from_numpy(d)); blk.counts.copy_(torch.from_numpy(c))
    same = torch.arange(nq * dim, dtype=torch.float32, device="cuda:0").view(nq, dim)
    out = {"rank": rank}
    m = blk.exchange(limit, seq=0, ticket=1, queries=same)  # every rank searched the same queries: merged
    torch.cuda.synchronize()
    out["ok_ids"], out["ok_counts"] = m[0].cpu().numpy(), m[3].cpu().numpy()
    mine = same + (1.0 if rank == 1 else 0.0)  # rank 1 was handed another request's queries
    try:
        blk.exchange(limit, seq=1, ticket=2, queries=mine)
        out["mismatch"] = None
    except SemaDBError as e:
        out["mismatch"] = (e.code, str(e))
    try:  # a shard that failed its search says so in its tag
        blk.exchange(limit, seq=2, ticket=3, queries=same, status=3 if rank == 0 else 0)
        out["failed"] = None
    except SemaDBError as e:
        out["failed"] = (e.code, str(e))
    try:  # out of step by one request
        blk.exchange(limit, seq=3 + rank, ticket=4 + rank, queries=same)
        out["seq"] = None
    except SemaDBError as e:
        out["seq"] = (e.code, str(e))
    q.put(out)
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.gpu
def test_tag_check_fires_across_two_gloo_ranks(oracle):
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    world, nq, per, limit = 2, 16, 10, 10
    procs = [ctx.Process(target=_gloo_exchange_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    got = [q.get(timeout=300) for _ in range(world)]
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    expect = [_shard_results(r, nq, per) for r in range(world)]
    g_ids = np.stack([e[0] for e in expect]).astype(np.uint64); g_d = np.stack([e[1] for e in expect]); g_c = np.stack([e[2] for e in expect])
    for o in got:
        for qi in range(nq):
            w_ids, w_d, w_s = oracle.cluster_merge(g_ids[:, qi, :], g_d[:, qi, :], g_c[:, qi], limit)
            assert int(o["ok_counts"][qi]) == len(w_ids)
            assert np.array_equal(o["ok_ids"][qi, :len(w_ids)].view(np.uint64), w_ids)
        assert o["mismatch"] is not None and o["mismatch"][0] == 3 and "query hash" in o["mismatch"][1]
        assert o["failed"] is not None and o["failed"][0] == 3 and "shard 0" in o["failed"][1]
        assert o["seq"] is not None and o["seq"][0] == 3 and "sequence number" in o["seq"][1] and "ticket" in o["seq"][1]
