"""The shard fan-out merge kernel (csrc/merge.hip: k_topk_merge) against the rule of tests/merge_model.py and the
oracle: non-finite distances, every output slot written exactly once, the shapes at the kernel's limits (2 048 items,
64 shards), the shape errors, and the fan-out end to end with queries that make every distance NaN or Inf.

The reference sorts with cmp.Compare (cluster/actions.go:362-364): NaN distances are one tie class behind +Inf, -0.0
ties with 0.0.  A rank-by-counting merge that compares with `<` / `==` alone gives every NaN item rank 0 and leaves
the slots behind the finite items unwritten; these tests are what notices."""
import ctypes as C

import numpy as np
import pytest

from tests import merge_model as mm
from tests.test_gpu_nonfinite import _poisoned_queries, same_bits_or_both_nan

pytestmark = pytest.mark.gpu

ID_SENTINEL = 0xA5A5A5A5A5A5A5A5
D_SENTINEL = 0xDEADBEEF  # a finite float32 (-6.26e18) no input below holds
U32_SENTINEL = 0xA5A5A5A5


# ---------------------------------------------------------------------------------------------------------------
# the three ways in
# ---------------------------------------------------------------------------------------------------------------
def _via_host(ids, d, counts, limit):
    from semadb_amd import cluster
    return cluster.topk_merge(ids, d, counts, limit)


def _to_numpy(o):
    return (o[0].cpu().numpy().view(np.uint64), o[1].cpu().numpy(), o[2].cpu().numpy().view(np.uint32),
            o[3].cpu().numpy().view(np.uint32))


def _via_device(ids, d, counts, limit):
    import torch
    from semadb_amd import cluster
    o = cluster.topk_merge(torch.from_numpy(ids.view(np.int64)).cuda(), torch.from_numpy(d).cuda(),
                           torch.from_numpy(counts.view(np.int32)).cuda(), limit)
    torch.cuda.synchronize()
    return _to_numpy(o)


def _via_gathered(ids, d, counts, limit):
    """the packed blocks an all-gather delivers back to back (ids | dists | counts | tag per shard), each stamped by
    sdb_cluster_stamp_block, through the tag check + merge of sdb_cluster_merge_gathered"""
    import torch
    from semadb_amd import _buf, cluster
    from semadb_amd._lib import MEM_DEVICE, check, lib
    n_shards, nq, per = ids.shape
    off_d, off_c, off_t, total = cluster.block_layout(nq, per)
    host = np.zeros((n_shards, total), dtype=np.uint8)
    for s in range(n_shards):
        host[s, :off_d] = ids[s].reshape(-1).view(np.uint8)
        host[s, off_d:off_c] = d[s].reshape(-1).view(np.uint8)
        host[s, off_c:off_c + nq * 4] = counts[s].view(np.uint8)
    g = torch.from_numpy(host).cuda()
    stream = _buf.current_stream(MEM_DEVICE)
    for s in range(n_shards):
        check(lib().sdb_cluster_stamp_block(C.c_void_p(g.data_ptr() + s * total), nq, per, limit, s, 5, 9, 0, None, 0, 0,
                                            stream))
    o = _device_outputs(nq, limit, sentinel=False)
    check(lib().sdb_cluster_merge_gathered(n_shards, nq, per, C.c_void_p(g.data_ptr()), limit, *_ptrs(o), 0, stream))
    torch.cuda.synchronize()
    return _to_numpy(o)


WAYS = {"host": _via_host, "device": _via_device, "gathered": _via_gathered}


def _device_outputs(nq, limit, sentinel=True):
    import torch
    if not sentinel:
        return (torch.zeros((nq, limit), dtype=torch.int64, device="cuda"), torch.zeros((nq, limit), dtype=torch.float32, device="cuda"),
                torch.zeros((nq, limit), dtype=torch.int32, device="cuda"), torch.zeros((nq,), dtype=torch.int32, device="cuda"))
    o_ids = torch.from_numpy(np.full((nq, limit), ID_SENTINEL, dtype=np.uint64).view(np.int64)).cuda()
    o_d = torch.from_numpy(np.full((nq, limit), D_SENTINEL, dtype=np.uint32).view(np.float32)).cuda()
    o_s = torch.from_numpy(np.full((nq, limit), U32_SENTINEL, dtype=np.uint32).view(np.int32)).cuda()
    o_c = torch.from_numpy(np.full((nq,), U32_SENTINEL, dtype=np.uint32).view(np.int32)).cuda()
    return o_ids, o_d, o_s, o_c


def _ptrs(o):
    return [C.c_void_p(t.data_ptr()) if t is not None else None for t in o]


def _raw_device_merge(ids, d, counts, limit, n_shards=None, per=None, with_shards=True):
    """sdb_topk_merge on device memory over outputs pre-filled with sentinels -> (return code, outputs as numpy);
    n_shards / per override what the arrays' shape says (the shape-error cases)"""
    import torch
    from semadb_amd import _buf
    from semadb_amd._lib import MEM_DEVICE, lib
    s_, nq, p_ = ids.shape
    t_ids = torch.from_numpy(ids.view(np.int64)).cuda()
    t_d = torch.from_numpy(d).cuda()
    t_c = torch.from_numpy(counts.view(np.int32)).cuda()
    o = _device_outputs(nq, max(limit, 1))
    ptrs = _ptrs(o)
    if not with_shards:
        ptrs[2] = None
    rc = lib().sdb_topk_merge(s_ if n_shards is None else n_shards, nq, p_ if per is None else per,
                              C.c_void_p(t_ids.data_ptr()), C.c_void_p(t_d.data_ptr()), C.c_void_p(t_c.data_ptr()), limit,
                              *ptrs, MEM_DEVICE, 0, _buf.current_stream(MEM_DEVICE))
    torch.cuda.synchronize()
    return rc, _to_numpy(o)


# ---------------------------------------------------------------------------------------------------------------
# comparison
# ---------------------------------------------------------------------------------------------------------------
def _check(got, ids, d, counts, limit, oracle=None, shards=True):
    """every query's answer is the model's: count, ids, shards, the same distance bits (NaN where the model has NaN).
    `counts` are the clipped ones.  With an oracle, the oracle has to give the model's answer too."""
    o_ids, o_d, o_s, o_c = got
    want = mm.merge_batch(ids, d, counts, limit)
    for q, (w_ids, w_d, w_s) in enumerate(want):
        n = len(w_ids)
        assert int(o_c[q]) == n, ("count", q, int(o_c[q]), n)
        assert np.array_equal(o_ids[q, :n], w_ids), ("ids", q, o_ids[q, :n], w_ids)
        assert same_bits_or_both_nan(o_d[q, :n], w_d), ("distances", q, o_d[q, :n], w_d)
        if shards:
            assert np.array_equal(o_s[q, :n].astype(np.int32), w_s), ("shards", q)
        if oracle is not None:
            r_ids, r_d, r_s = oracle.cluster_merge(ids[:, q, :], d[:, q, :], counts[:, q].astype(np.int32), limit)
            assert np.array_equal(r_ids, w_ids) and np.array_equal(r_s, w_s)
            assert np.array_equal(r_d.view(np.uint32), w_d.view(np.uint32))
    return want


def _item_multiset(ids, d, sh):
    """sorted (id, distance bits with every NaN folded to one value, shard)"""
    b = np.ascontiguousarray(d, dtype=np.float32).view(np.uint32).astype(np.uint64)
    b[np.isnan(d)] = 1 << 40
    return sorted(zip((int(v) for v in ids), (int(v) for v in b), (int(v) for v in sh)))


def _check_slots(got, ids, d, counts, limit):
    """[0, count) holds the model's items, each exactly once and none of them a sentinel; [count, limit) was left alone"""
    o_ids, o_d, o_s, o_c = got
    want = mm.merge_batch(ids, d, counts, limit)
    o_bits = o_d.view(np.uint32)
    for q, (w_ids, w_d, w_s) in enumerate(want):
        n = len(w_ids)
        assert int(o_c[q]) == n, ("count", q)
        assert not (o_ids[q, :n] == ID_SENTINEL).any(), ("id slot never written", q, np.flatnonzero(o_ids[q, :n] == ID_SENTINEL))
        assert not (o_bits[q, :n] == D_SENTINEL).any(), ("distance slot never written", q)
        assert not (o_s[q, :n] == U32_SENTINEL).any(), ("shard slot never written", q)
        assert _item_multiset(o_ids[q, :n], o_d[q, :n], o_s[q, :n]) == _item_multiset(w_ids, w_d, w_s), ("items", q)
        assert (o_ids[q, n:] == ID_SENTINEL).all() and (o_bits[q, n:] == D_SENTINEL).all(), ("written past count", q)
        assert (o_s[q, n:] == U32_SENTINEL).all(), ("shard written past count", q)


# ---------------------------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------------------------
def _special_queries(rng, n_shards, per):
    """16 queries, one class of trouble each -> ids [S, 16, per], d, counts (full lists; every shard's list ascending
    where that means anything, as a shard's own search leaves it -- the merge does not rely on it)"""
    nq = 16
    f = np.float32
    d = np.sort(rng.integers(0, 40, size=(n_shards, nq, per)).astype(f) / 8, axis=2)
    ids = rng.integers(2, 10 ** 6, size=(n_shards, nq, per)).astype(np.uint64)
    bits = d.view(np.uint32)
    s1 = min(1, n_shards - 1)  # "the second shard", where there is one
    d[:, 0, :] = np.nan                                     # 0: every item on every shard NaN (a NaN query component)
    bits[:, 1, :] = rng.choice(mm.NAN_BITS, size=(n_shards, per))  # 1: all NaN, distinct payloads and signs
    d[n_shards - 1, 2, per // 2:] = np.nan                  # 2: NaN on one shard only, behind its finite items
    d[:, 3, per - 3:] = np.nan                              # 3: NaN at the end of every shard's list
    d[:, 4, 0] = np.nan                                     # 4: NaN FIRST in every list
    d[0, 5, :] = np.nan                                     # 5: one shard all NaN, the first one
    bits[:, 5, 1::4] = mm.NAN_BITS[2]                       #    ... and NaN scattered through the others
    d[:, 6, per // 3:] = np.inf                             # 6: runs of +Inf ties across shards
    d[:, 7, per // 2:] = np.inf                             # 7: +Inf ties in front of NaN
    d[:, 7, per - 2:] = np.nan
    d[:, 8, 0] = -np.inf                                    # 8: -Inf present on every shard, twice on shard 1
    d[s1, 8, 1] = -np.inf
    d[:, 9, :] = np.sort(-d[:, 9, :], axis=1)               # 9: negative (dot-product) distances with -Inf and NaN
    d[0, 9, 0], d[s1, 9, per - 1] = -np.inf, np.nan
    d[:, 10, :] = np.where(rng.integers(0, 2, size=(n_shards, per)) == 1, f(-0.0), f(0.0))  # 10: only +-0.0
    d[:, 11, :3] = np.array([-0.0, 0.0, -0.0], dtype=f)     # 11: +-0.0 in front of positive distances
    d[s1, 11, :3] = np.array([0.0, -0.0, 0.0], dtype=f)
    den = np.array(mm.DENORMAL_BITS, dtype=np.uint32).view(f)
    d[:, 12, :] = np.sort(np.concatenate([den, [f(0.0), f(-0.0), f(1e-38)]])[rng.integers(0, 7, size=(n_shards, per))], axis=1)  # 12: denormals around zero
    d[:, 13, :] = mm.SPECIALS[rng.integers(0, len(mm.SPECIALS), size=(n_shards, per))]      # 13: everything at once, unsorted
    ids[:, 14, :] = rng.integers(2, 5, size=(n_shards, per))  # 14: NaN ties that only the id / the position breaks
    d[:, 14, per // 2:] = np.nan
    #                                                         15: an ordinary query
    counts = np.full((n_shards, nq), per, dtype=np.uint32)
    return ids, np.ascontiguousarray(d), counts


def _limit_shapes(rng, n_shards, per, nq, p_special):
    """tie-rich distances (integers / 8) with special values sprinkled in, ragged counts with zeros and with counts
    ABOVE per_shard (the kernel clips them) -> ids, d, raw counts, clipped counts"""
    d = np.sort(rng.integers(0, 50, size=(n_shards, nq, per)).astype(np.float32) / 8, axis=2)
    mm.sprinkle(rng, d, p_special)
    ids = rng.integers(2, 10 ** 6, size=(n_shards, nq, per)).astype(np.uint64)
    counts = rng.integers(0, per + 1, size=(n_shards, nq)).astype(np.uint32)
    counts[rng.random(counts.shape) < 0.15] = 0
    counts[rng.random(counts.shape) < 0.15] = per + int(rng.integers(1, 1000))
    counts[:, 0] = per  # the first query always has the full item count, one shard saying more than it has room for
    counts[0, 0] = per + 7
    d[n_shards - 1, 0, per // 2], d[0, 0, per - 1] = np.nan, np.inf  # and holds a NaN and a +Inf whatever was drawn
    return ids, d, counts, np.minimum(counts, per).astype(np.uint32)


# ---------------------------------------------------------------------------------------------------------------
# special values
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("way", sorted(WAYS))
@pytest.mark.parametrize("limit", [10, 30])
@pytest.mark.parametrize("n_shards", [2, 3, 8])
def test_special_values_merge_like_the_model(oracle, n_shards, limit, way):
    rng = np.random.default_rng(9000 + n_shards)
    ids, d, counts = _special_queries(rng, n_shards, 10)
    assert np.isnan(d).any() and np.isinf(d).any()
    _check(WAYS[way](ids, d, counts, limit), ids, d, counts, limit, oracle=oracle)
    # the same lists cut ragged: NaN items fall off the end of some lists, some shards bring nothing
    counts = rng.integers(0, 11, size=counts.shape).astype(np.uint32)
    _check(WAYS[way](ids, d, counts, limit), ids, d, counts, limit, oracle=oracle)


@pytest.mark.parametrize("way", sorted(WAYS))
def test_single_shard_with_nan_comes_back_unsorted(oracle, way):
    rng = np.random.default_rng(9100)
    ids, d, counts = _special_queries(rng, 1, 10)
    d[0, 15, :] = d[0, 15, ::-1]  # descending: a sort would turn it round
    d[0, 15, 4] = np.nan
    for limit in (10, 4, 30):
        want = _check(WAYS[way](ids, d, counts, limit), ids, d, counts, limit, oracle=oracle)
        n = min(10, limit)
        assert np.array_equal(want[15][0], ids[0, 15, :n]) and np.isnan(want[15][1][4 if n > 4 else 0]) == (n > 4)


# ---------------------------------------------------------------------------------------------------------------
# every slot written exactly once
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_shards,per,limit", [(2, 10, 10), (3, 10, 30), (8, 10, 30), (8, 10, 100), (3, 7, 21), (2, 10, 1)])
def test_every_slot_below_count_is_written_once_and_none_above(n_shards, per, limit):
    """outputs pre-filled with sentinels on the device-memory path (nothing clears them there): a NaN item that takes
    rank 0 leaves a hole behind the finite items and collides with the best one; limit > total must leave the tail
    alone"""
    rng = np.random.default_rng(9200 + n_shards * per + limit)
    ids, d, counts = _special_queries(rng, n_shards, per)
    rc, got = _raw_device_merge(ids, d, counts, limit)
    assert rc == 0
    _check_slots(got, ids, d, counts, limit)
    _check(got, ids, d, counts, limit)
    counts = rng.integers(0, per + 1, size=counts.shape).astype(np.uint32)
    counts[:, 3] = 0  # total = 0: count 0, nothing written
    counts[1:, 4] = 0  # one shard alone brings items (still sorted: n_shards > 1)
    rc, got = _raw_device_merge(ids, d, counts, limit)
    assert rc == 0 and int(got[3][3]) == 0
    _check_slots(got, ids, d, counts, limit)
    _check(got, ids, d, counts, limit)


def test_all_counts_zero_writes_nothing_but_the_counts():
    rng = np.random.default_rng(9300)
    ids, d, counts = _special_queries(rng, 3, 10)
    counts[:] = 0
    rc, got = _raw_device_merge(ids, d, counts, 10)
    assert rc == 0 and not got[3].any()
    _check_slots(got, ids, d, counts, 10)


# ---------------------------------------------------------------------------------------------------------------
# shapes at the kernel's limits
# ---------------------------------------------------------------------------------------------------------------
LIMIT_SHAPES = [(64, 32), (63, 32), (8, 256), (2, 1024), (1, 2048), (64, 1), (3, 21), (5, 13)]


@pytest.mark.parametrize("nq", [1, 37])
@pytest.mark.parametrize("n_shards,per", LIMIT_SHAPES)
def test_shapes_at_the_kernels_limits(oracle, n_shards, per, nq):
    """2 048 items exactly and just under, 64 shards, one item short of a wave and one over; limit 1, per, total and
    past total; ragged counts, zero counts, counts above per_shard; out_shards = NULL"""
    rng = np.random.default_rng(9400 + n_shards * 7 + per + nq)
    total = n_shards * per
    ids, d, raw, clipped = _limit_shapes(rng, n_shards, per, nq, 0.05)
    assert int(clipped[:, 0].sum()) == total and (raw > per).any() and np.isnan(d).any()
    for limit in sorted({1, per, total, total + 5}):
        rc, got = _raw_device_merge(ids, d, raw, limit)
        assert rc == 0
        _check_slots(got, ids, d, clipped, limit)
        _check(got, ids, d, clipped, limit, oracle=oracle if limit == total else None)
    # the host-memory path at the widest limit, and out_shards = NULL on the device path
    _check(_via_host(ids, d, raw, total), ids, d, clipped, total)
    rc, got = _raw_device_merge(ids, d, raw, per, with_shards=False)
    assert rc == 0 and (got[2] == U32_SENTINEL).all()
    _check(got, ids, d, clipped, per, shards=False)


def test_full_item_count_of_nan_and_of_ties(oracle):
    """2 048 items that are all NaN / all the same distance: every rank is decided by (shard, id, position) alone"""
    rng = np.random.default_rng(9500)
    for n_shards, per in [(64, 32), (2, 1024)]:
        ids = rng.integers(2, 40, size=(n_shards, 2, per)).astype(np.uint64)  # ids repeat inside a shard
        d = np.full((n_shards, 2, per), np.nan, dtype=np.float32)
        d[:, 1, :] = np.inf
        counts = np.full((n_shards, 2), per, dtype=np.uint32)
        for limit in (n_shards * per, 100):
            rc, got = _raw_device_merge(ids, d, counts, limit)
            assert rc == 0
            _check_slots(got, ids, d, counts, limit)
            _check(got, ids, d, counts, limit)


# ---------------------------------------------------------------------------------------------------------------
# shape errors
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("way", ["topk_merge", "gathered"])
def test_shape_errors_touch_nothing_and_the_next_call_is_served(way):
    import torch
    from semadb_amd import _buf
    from semadb_amd._lib import MEM_DEVICE, lib
    rng = np.random.default_rng(9600)
    ids, d, counts = _special_queries(rng, 3, 10)
    #      n_shards, per_shard, limit
    bad = [(0, 10, 10), (65, 10, 10), (1, 2049, 10), (7, 293, 10), (64, 33, 10), (3, 10, 0), (3, 0, 10)]
    assert 7 * 293 == 2051 and 2049 > 2048
    for n_shards, per, limit in bad:
        if way == "topk_merge":
            rc, got = _raw_device_merge(ids, d, counts, limit, n_shards=n_shards, per=per)
        else:
            g = torch.zeros(1 << 16, dtype=torch.uint8, device="cuda")  # never read: the shape is refused first
            o = _device_outputs(16, max(limit, 1))
            rc = lib().sdb_cluster_merge_gathered(n_shards, 16, per, C.c_void_p(g.data_ptr()), limit, *_ptrs(o), 0,
                                                  _buf.current_stream(MEM_DEVICE))
            torch.cuda.synchronize()
            got = _to_numpy(o)
        assert rc == 1, (n_shards, per, limit, rc)  # SDB_ERR_INVALID
        assert lib().sdb_last_error()  # and it says why
        assert (got[0] == ID_SENTINEL).all() and (got[1].view(np.uint32) == D_SENTINEL).all()
        assert (got[2] == U32_SENTINEL).all() and (got[3] == U32_SENTINEL).all()
        # the next good call is served
        fn = _via_device if way == "topk_merge" else _via_gathered
        _check(fn(ids, d, counts, 10), ids, d, counts, 10)


# ---------------------------------------------------------------------------------------------------------------
# end to end: the fan-out with poisoned queries
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", ["euclidean", "cosine"])
@pytest.mark.parametrize("d", [33, 96])
@pytest.mark.parametrize("world", [2, 4])
def test_fanout_with_nonfinite_queries_equals_the_merge_of_the_shards_answers(world, d, metric):
    """Fanout.search_points over `world` shards that share the GPU with queries that make every distance NaN (a NaN
    component), +-Inf (an Inf component, the 1e20 scale) or ordinary: the answer is the model's merge of the shards'
    own search_batch answers at the per-shard limit.  The single-index walk is tested to answer such queries like the
    reference (tests/test_gpu_nonfinite.py); this is the same query one level up."""
    from semadb_amd import cluster, vamana
    from tests.helpers import start_vector, unit_rows
    rng = np.random.default_rng(9700 + world * 1000 + d + len(metric))
    n, limit, L = 400, 10, 50
    ixs = []
    for s in range(world):
        base = unit_rows(rng, n, d)
        base[:, 0] = np.abs(base[:, 0]) + np.float32(1e-3)  # one sign in component 0: see the last query below
        ix = vamana.NewIndexVamana("mg%d" % s, vamana.IndexVectorVamanaParameters(d, metric, L, 32, 1.2), strict=False)
        ix.set_start(start_vector(rng, d))
        ix.insert_batch(None, base)
        ixs.append(ix)
    q = _poisoned_queries(rng, d, 13, 1.0)
    q[12, 0] = -np.inf  # (-Inf - x)^2 = +Inf; 1 - (-Inf * x) = +Inf for x > 0: every distance +Inf under both metrics
    per = cluster.shard_limit(limit, world, 75)
    res = [ix.search_batch(q, per, L) for ix in ixs]
    s_ids = np.stack([r[0] for r in res]); s_d = np.stack([r[1] for r in res]); s_c = np.stack([r[2] for r in res])
    ranks = cluster.Cluster.create_local([0] * world)
    fan = cluster.Fanout(ranks, ixs)
    got = fan.search_points(q, limit, L)
    want = _check(got, s_ids, s_d, np.minimum(s_c, per).astype(np.uint32), limit)
    merged = np.concatenate([w[1] for w in want])
    assert np.isnan(merged).any() and np.isposinf(merged).any(), "no NaN / +Inf reached the merge: the case is vacuous"
    assert np.isnan(want[0][1]).all() and len(want[0][1]) == limit  # the NaN-component query: a full answer of NaN
    # ... and a second request through the same ranks
    _check(fan.search_points(q[::-1].copy(), limit, L), s_ids[:, ::-1], s_d[:, ::-1],
           np.minimum(s_c, per).astype(np.uint32)[:, ::-1], limit)
    for r in ranks:
        r.close()
    for ix in ixs:
        ix.close()
