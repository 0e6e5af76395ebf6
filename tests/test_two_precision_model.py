"""The float64 model of the two-precision hop (tests/two_precision_model.py), pinned without a GPU: its replay of
greedySearch equals the oracle's walk, its three counts are ordered (lower <= upper <= discardable), and on every input
that tests/test_gpu_two_precision_bound.py sends to the device the two sides of the sandwich are within 1 % of each
other (lower / upper >= 0.99; measured 0.9997 .. 1.0000), so that the device's count is pinned from both sides."""
import numpy as np
import pytest

from tests import two_precision_model as M
from tests.helpers import bits, build_oracle_index, unit_rows


def _same_walk(o, rep, q, limit, L):
    o_ids, o_d, o_vis, o_tr = o.search(q, limit, L)
    assert np.array_equal(rep.ids, o_ids) and np.array_equal(bits(rep.dists), bits(o_d))
    assert np.array_equal(rep.visit, o_vis), "visit order"
    assert (rep.n_hop, rep.n_dist, rep.n_edges) == (o_tr.n_hop, o_tr.n_dist, o_tr.n_edges)


def test_half_rows_round_like_the_copy():
    x = np.array([0.0, 1.0, 6.1e-5, 6.103515625e-5, -6.0e-5, 65504.0, 65519.9, 65520.0, 1e6, 1.0 + 2.0 ** -11,
                  1.0 + 3 * 2.0 ** -11, np.inf], dtype=np.float32)
    want = [0.0, 1.0, 0.0, 6.103515625e-5, 0.0, 65504.0, 65504.0, np.inf, np.inf, 1.0, 1.0 + 2.0 ** -9, np.inf]
    assert np.array_equal(M.half_rows(x), np.array(want))
    e, y = M.maxima(np.array([[3.0, 4.0], [1.0 + 2.0 ** -11, 0.0]], dtype=np.float32))
    assert y == 5.0 and e == 2.0 ** -11
    assert np.isnan(M.maxima(np.array([[np.nan, 1.0]], dtype=np.float32))[0])
    assert np.isinf(M.maxima(np.array([[1e6, 1.0]], dtype=np.float32))[1])


@pytest.mark.parametrize("metric", M.METRICS)
def test_replay_equals_the_oracle(oracle, metric):
    """on an oracle-built graph with short rows, ties (repeated points) and L below, at and above the degree"""
    rng = np.random.default_rng(3)
    base = unit_rows(rng, 900, 48)
    base[600:] = base[rng.integers(0, 300, 300)]
    o = build_oracle_index(oracle, base, metric, R=24, L=30)
    g = M.Graph(*o.export())
    q = np.vstack([unit_rows(rng, 24, 48), base[:4], np.zeros((1, 48), dtype=np.float32)])
    D = oracle.distance_matrix(q, g.vecs, metric, M.impl_of(oracle))
    for limit, L in ((1, 1), (1, 2), (5, 5), (10, 30), (10, 96), (10, 128)):
        for i in range(q.shape[0]):
            _same_walk(o, M.replay(g, D[i], limit, L), q[i], limit, L)


def _model_case(oracle, metric, d, ex, queries, limit, L, what, full_rows=True):
    g = M.Graph(*ex)
    o = M.load_oracle(oracle, metric, d, ex)
    reps, t, _ = M.run_model(oracle, g, metric, queries, limit, L)
    for i, rep in enumerate(reps):
        _same_walk(o, rep, queries[i], limit, L)
    M.check_tally(t, what)
    if full_rows:
        assert t.expanded_full_rows >= 0.9 * t.expanded, "%s: %d of %d expanded nodes have 64 edges" % (what, t.expanded_full_rows, t.expanded)
    return t


@pytest.mark.parametrize("metric", M.METRICS)
@pytest.mark.parametrize("d", M.WIDTHS)
def test_width_inputs(oracle, metric, d):
    ex, queries, limit, L = M.width_case(oracle, metric, d)
    t = _model_case(oracle, metric, d, ex, queries, limit, L, "%s d=%d" % (metric, d))
    assert t.lower > 10000 and t.discardable >= 0.7 * t.full, t  # most neighbours met with the array full are discardable


@pytest.mark.parametrize("metric", M.METRICS)
@pytest.mark.parametrize("d", [128, 512])
def test_l_and_hostile_inputs(oracle, metric, d):
    ex, queries = M.l_case(oracle, metric, d)
    for L, limit in M.L_CASES:
        if L < limit:
            continue  # (search.go:23-25 refuses them)
        t = _model_case(oracle, metric, d, ex, queries, limit, L, "%s d=%d L=%d limit=%d" % (metric, d, L, limit))
        assert t.lower > 0
    for L in M.L_BEYOND:
        _model_case(oracle, metric, d, ex, queries, 10, L, "%s d=%d L=%d" % (metric, d, L))
    for kind in M.HOSTILE_NO_DISCARD:
        t = _model_case(oracle, metric, d, ex, M.hostile_queries(d, kind), 10, 40, "%s d=%d %s" % (metric, d, kind))
        assert t.upper == 0 and t.lower == 0, (kind, t)
    for kind in M.HOSTILE_SANDWICH:
        _model_case(oracle, metric, d, ex, M.hostile_queries(d, kind), 10, 40, "%s d=%d %s" % (metric, d, kind))


@pytest.mark.parametrize("metric", M.METRICS)
def test_overflow_list_inputs(oracle, metric):
    ex, queries = M.overflow_case(oracle, metric)
    g = M.Graph(*ex)
    assert g.deg[g.start] > 64 + 64
    for L in (1, 2):
        t = _model_case(oracle, metric, 128, ex, queries, 1, L, "%s overflow list L=%d" % (metric, L), full_rows=False)
        assert t.lower > 0


@pytest.mark.parametrize("d", [128, 512])
def test_dispatch_inputs(oracle, d):
    ex, queries = M.dispatch_case(oracle, d)
    _model_case(oracle, "cosine", d, ex, queries, 10, 40, "dispatch d=%d" % d)
