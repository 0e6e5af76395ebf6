"""The merge rule itself (tests/merge_model.py), without a GPU: hand-written answers for the cases where Go's
cmp.Compare differs from the `<` / `>` pair (NaN, signed zeros, infinities), and the model against the oracle's
restatement (orc_cluster_merge) on random lists that hold those values -- the two judges the GPU tests rely on
(tests/test_gpu_merge.py) have to agree with each other first."""
import numpy as np
import pytest

from tests import merge_model as mm

NAN, INF = np.float32(np.nan), np.float32(np.inf)


def _lists(rows):
    """rows: per shard a list of (id, dist) -> ids [S, per], dists [S, per], counts [S] (short lists padded)"""
    per = max(len(r) for r in rows)
    ids = np.zeros((len(rows), per), dtype=np.uint64)
    d = np.zeros((len(rows), per), dtype=np.float32)
    for s, r in enumerate(rows):
        for i, (ident, dist) in enumerate(r):
            ids[s, i], d[s, i] = ident, dist
    return ids, d, np.array([len(r) for r in rows], dtype=np.int32)


def _answer(got):
    ids, d, sh = got
    return [(int(s), int(i)) for s, i in zip(sh, ids)]


def _bits(d):
    return np.ascontiguousarray(d, dtype=np.float32).view(np.uint32)


def _both(oracle, ids, d, c, limit):
    """the model's answer, after checking that the oracle gives the same one bit for bit (NaN payloads included: both
    only move the caller's floats)"""
    m = mm.merge_one(ids, d, c, limit)
    o = oracle.cluster_merge(ids, d, c, limit)
    assert np.array_equal(m[0], o[0]) and np.array_equal(m[2], o[2]), (_answer(m), _answer(o))
    assert np.array_equal(_bits(m[1]), _bits(o[1]))
    return m


def test_nan_sorts_after_plus_inf(oracle):
    ids, d, c = _lists([[(10, NAN), (11, 0.5)], [(20, INF), (21, 0.25)]])
    m = _both(oracle, ids, d, c, 10)
    assert _answer(m) == [(1, 21), (0, 11), (1, 20), (0, 10)]
    assert np.isnan(m[1][3]) and m[1][2] == INF


def test_nans_are_one_tie_class_broken_by_shard_then_id(oracle):
    # different payloads and signs: still equal to each other
    ids, d, c = _lists([[(7, mm.NAN_B), (3, 1.0)], [(9, NAN), (2, mm.NAN_A)], [(1, mm.NAN_A)]])
    m = _both(oracle, ids, d, c, 10)
    assert _answer(m) == [(0, 3), (0, 7), (1, 2), (1, 9), (2, 1)]
    assert _bits(m[1]).tolist()[1:] == [0xFFC12345, 0x7FC00001, 0x7FC00000, 0x7FC00001]  # payloads travel untouched
    # all NaN, truncated: the first `limit` by (shard, id)
    assert _answer(_both(oracle, ids[:, :1], d[:, :1], np.array([1, 1, 1], dtype=np.int32), 2)) == [(0, 7), (1, 9)]


def test_signed_zeros_tie_and_break_by_shard(oracle):
    ids, d, c = _lists([[(5, 0.0), (6, 0.5)], [(4, -0.0)], [(3, 0.0), (2, -0.0)]])
    m = _both(oracle, ids, d, c, 10)
    assert _answer(m) == [(0, 5), (1, 4), (2, 2), (2, 3), (0, 6)]
    assert _bits(m[1]).tolist() == [0, 0x80000000, 0x80000000, 0, 0x3F000000]  # an emitted -0.0 is still -0.0


def test_minus_inf_comes_first(oracle):
    ids, d, c = _lists([[(1, -3e38), (2, NAN)], [(3, -INF), (4, INF)], [(5, -INF)]])
    assert _answer(_both(oracle, ids, d, c, 10)) == [(1, 3), (2, 5), (0, 1), (1, 4), (0, 2)]
    assert _answer(_both(oracle, ids, d, c, 3)) == [(1, 3), (2, 5), (0, 1)]


def test_single_shard_is_not_sorted(oracle):
    ids, d, c = _lists([[(9, 0.5), (8, NAN), (7, 0.25), (6, -INF), (5, NAN)]])
    m = _both(oracle, ids, d, c, 4)
    assert _answer(m) == [(0, 9), (0, 8), (0, 7), (0, 6)]
    assert np.isnan(m[1][1]) and m[1][3] == -INF


def test_counts_are_clipped_and_position_is_the_last_tie_break(oracle):
    # the same (dist, shard, id) twice with different bits (0.0 / -0.0): the list's own order decides
    ids, d, c = _lists([[(4, -0.0), (4, 0.0), (4, -0.0)], [(1, 1.0), (1, NAN), (1, 1.0)]])
    m = mm.merge_one(ids, d, np.array([7, 2]), 10)  # 7 > per_shard: clipped to 3
    assert _answer(m) == [(0, 4)] * 3 + [(1, 1)] * 2
    assert _bits(m[1]).tolist()[:3] == [0x80000000, 0, 0x80000000] and np.isnan(m[1][4])
    _both(oracle, ids, d, np.array([3, 2], dtype=np.int32), 10)


@pytest.mark.parametrize("seed", range(6))
def test_model_equals_oracle_on_random_lists_with_special_values(oracle, seed):
    """ragged lists of tie-rich distances (integers / 8, both signs) with NaN / +-Inf / +-0 / denormals drawn in, in
    ARBITRARY order inside a shard (the merge does not assume sorted input) and with ids that repeat"""
    rng = np.random.default_rng(7100 + seed)
    seen_nan = 0
    for trial in range(60):
        n_shards = int(rng.integers(1, 10))
        per = int(rng.integers(1, 40))
        limit = int(rng.integers(1, n_shards * per + 6))
        d = (rng.integers(-20, 20, size=(n_shards, per)).astype(np.float32) / 8).astype(np.float32)
        mm.sprinkle(rng, d, float(rng.choice([0.0, 0.1, 0.5, 1.0])))
        ids = rng.integers(2, int(rng.choice([6, 10 ** 6])), size=(n_shards, per)).astype(np.uint64)
        c = rng.integers(0, per + 1, size=n_shards).astype(np.int32)
        _both(oracle, ids, d, c, limit)
        seen_nan += int(np.isnan(d).sum())
    assert seen_nan > 100
