"""The shard fan-out merge (ClusterNode.SearchPoints, cluster/actions.go:357-376) for one query, restated in plain
Python: the rule the device merge (csrc/merge.hip), the oracle (orc_cluster_merge) and the ABI comment all follow.

The reference sorts the gathered items with cmp.Compare(b.HybridScore, a.HybridScore), HybridScore = -dist * weight.
cmp.Compare is a total order on floats: NaN is below every number and equal to NaN, -0.0 equals 0.0.  Read in
distances (weight > 0): -Inf first, ..., +Inf, then every NaN-distance item as ONE tie class at the very end.  The
reference's sort is unstable inside a tie class; here ties break by (shard, id, position in the shard's list), so every
item has one place.  A single shard is not sorted at all (actions.go:357: `if len(col.ShardIds) > 1`)."""
import numpy as np


def sort_key(dist, shard, ident, pos):
    """(isnan, dist, shard, id, position).  dist stays a numpy float32: float32 comparison, so -0.0 == 0.0; the
    distance of a NaN item is replaced by 0 so that the tuple never compares a NaN."""
    nan = bool(np.isnan(dist))
    return (nan, np.float32(0) if nan else np.float32(dist), int(shard), int(ident), int(pos))


def merge_one(ids, dists, counts, limit):
    """ids/dists [n_shards, per_shard], counts [n_shards] of ONE query -> (ids uint64, dists float32, shards int32)
    of min(total, limit) items; the distance bits (the sign of a zero, a NaN's payload) travel untouched."""
    ids = np.asarray(ids, dtype=np.uint64)
    dists = np.asarray(dists, dtype=np.float32)
    n_shards, per = ids.shape
    items = []
    for s in range(n_shards):
        for i in range(min(int(counts[s]), per)):
            items.append((dists[s, i], s, int(ids[s, i]), i))
    if n_shards > 1:
        items.sort(key=lambda it: sort_key(*it))
    items = items[:limit]
    sh = np.array([it[1] for it in items], dtype=np.int32)
    pos = np.array([it[3] for it in items], dtype=np.int64)
    return ids[sh, pos], dists[sh, pos], sh  # gathered, not rebuilt from scalars: the bits are the input's


def merge_batch(ids, dists, counts, limit):
    """ids/dists [n_shards, nq, per_shard], counts [n_shards, nq] -> a list of merge_one answers, one per query"""
    ids, dists, counts = np.asarray(ids), np.asarray(dists), np.asarray(counts)
    return [merge_one(ids[:, q, :], dists[:, q, :], counts[:, q], limit) for q in range(ids.shape[1])]


# the values a merge can go wrong on; two NaNs of different payload and sign
NAN_BITS = (0x7FC00000, 0x7FC00001, 0xFFC12345)
DENORMAL_BITS = (0x00000001, 0x80000001, 0x007FFFFF, 0x00000002)
#                              +Inf        -Inf        0.0         -0.0
SPECIAL_BITS = np.array(NAN_BITS + (0x7F800000, 0xFF800000, 0x00000000, 0x80000000) + DENORMAL_BITS, dtype=np.uint32)
SPECIALS = SPECIAL_BITS.view(np.float32)
NAN_A, NAN_B = SPECIALS[1], SPECIALS[2]


def sprinkle(rng, dists, p):
    """replace a fraction p of `dists` (C-contiguous float32, any shape) by values drawn from SPECIALS, in place"""
    assert dists.dtype == np.float32 and dists.flags.c_contiguous
    hit = (rng.random(dists.shape) < p).reshape(-1)
    dists.reshape(-1).view(np.uint32)[hit] = SPECIAL_BITS[rng.integers(0, len(SPECIAL_BITS), int(hit.sum()))]
    return dists
