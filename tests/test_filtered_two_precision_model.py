"""The float64 model of the two-precision hop on filtered walks (tests/filtered_two_precision_model.py), pinned without
a GPU on every input tests/test_gpu_filtered_two_precision.py sends to the device: its replay equals the oracle's
filtered search (ids, distance bits, visit order, counters); lower <= upper <= discardable; on the sandwich cases
lower / upper >= 0.99 and lower > 0, and at least one neighbour that the pure bound would discard against the array's
last distance as the chunk starts is KEPT by the reference -- the inputs catch a straight port of the plain walk's rule.

Deliberately exempt from those three sandwich conditions (Case.sandwich = False; replay == oracle and the order of the
counts are still asserted): the NaN-seed inputs, where the bound is NaN and upper == lower == 0 is what is asserted, and
the near-tie inputs, whose crowd of distances within the bound of B puts `lower` far below `upper` by construction (as
in test_gpu_sketch.py's near-tie test, answers and contradicted == 0 carry that case on the device).  L = 129 has no
stage: only the replay is held against the oracle there."""
import numpy as np
import pytest

from tests import filtered_two_precision_model as F
from tests.helpers import bits


def _same_walk(case, reps):
    for i, rep in enumerate(reps):
        o_ids, o_d, o_vis, o_tr = case.o.search(case.queries[i], case.limit, case.L, filter_ids=sorted(case.filters[i]))
        what = "%s query %d" % (case.what, i)
        assert np.array_equal(rep.ids, o_ids), what
        nan = np.isnan(o_d)
        assert np.array_equal(np.isnan(rep.dists), nan) and np.array_equal(bits(rep.dists)[~nan], bits(o_d)[~nan]), what
        assert np.array_equal(rep.visit, o_vis), what + ": visit order"
        assert (rep.n_hop, rep.n_dist, rep.n_edges) == (o_tr.n_hop, o_tr.n_dist, o_tr.n_edges), what + ": counters"


def _check(oracle, case):
    reps, t = case.model(oracle)
    _same_walk(case, reps)
    print("%s: %r" % (case.what, t))
    F.check_tally(t, case.what, case.sandwich)
    return t


@pytest.mark.parametrize("metric,d,full_rows", F.WIDTH_CASES)
def test_width_inputs(oracle, metric, d, full_rows):
    t = _check(oracle, F.width_case(oracle, metric, d, full_rows))
    assert t.risen > 0, "no chunk starts with the maximum of the array's last entries above its last one"


@pytest.mark.parametrize("metric", F.METRICS)
def test_search_size_inputs(oracle, metric):
    for L, limit in F.L_CASES:
        _check(oracle, F.width_case(oracle, metric, 128, False, limit, L))
    case = F.width_case(oracle, metric, 128, False, 10, F.L_NO_STAGE)
    _same_walk(case, case.model(oracle)[0])


@pytest.mark.parametrize("metric", F.METRICS)
def test_holes_inputs(oracle, metric):
    case = F.holes_case(oracle, metric)
    ids = case.ex[0]
    assert np.any(np.diff(ids.astype(np.int64)) < 0) and len(ids) < int(ids.max())  # out of id order, and holes
    _check(oracle, case)


@pytest.mark.parametrize("metric", ["cosine", "euclidean"])
def test_nan_seed_inputs(oracle, metric):
    case = F.nan_case(oracle, metric)
    t = _check(oracle, case)
    assert t.upper == 0 and t.lower == 0 and t.full > 0, t


@pytest.mark.parametrize("metric", ["cosine", "euclidean"])
@pytest.mark.parametrize("noise", F.NEAR_TIE_NOISE)
def test_near_tie_inputs(oracle, metric, noise):
    _check(oracle, F.near_tie_case(oracle, metric, noise))


def test_dispatch_inputs(oracle):
    """the GPU test compares the 513 answers with the oracle's own; here the replay is held against the oracle on the
    64 queries its small call shares with the large one"""
    case = F.dispatch_case(oracle)
    assert case.queries.shape[0] == 513 and len(case.filters) == 513
    first = F.Case(case.what, case.metric, case.d, case.ex, case.o, case.queries[:64], case.filters[:64], case.limit, case.L)
    _check(oracle, first)
