"""The float64 model of the two-precision hop on filtered walks (tests/filtered_two_precision_model.py), pinned without
a GPU on every input tests/test_gpu_filtered_two_precision.py sends to the device: its replay equals the oracle's
filtered search (ids, distance bits, visit order, counters); lower <= upper <= discardable; on the sandwich cases
lower / upper >= 0.99 and lower > 0, and at least one neighbour that the pure bound would discard against the array's
last distance as the chunk starts is KEPT by the reference -- the inputs catch a straight port of the plain walk's rule.

Deliberately exempt from those three sandwich conditions (Case.sandwich = False; replay == oracle and the order of the
counts are still asserted): the NaN-seed inputs, where the bound is NaN and upper == lower == 0 is what is asserted, and
the near-tie inputs, whose crowd of distances within the bound of B puts `lower` far below `upper` by construction (as
in test_gpu_sketch.py's near-tie test, answers and contradicted == 0 carry that case on the device).  L = 129 has no
stage: only the replay is held against the oracle there.

Further exemptions, each for the reason given:
* searchSize 1 (the L cases and the overflow-list cases) is exempt from naive_wrong > 0 and from risen > 0: an array of
  one entry is sorted, B is its only distance, and the chunk-start rule is the same rule.  naive_wrong == 0 and
  risen == 0 are asserted there instead (check_tally(naive=False)).
* the hostile-query inputs are exempt from all three sandwich conditions: a query that overflows float16, holds a NaN or
  an inf, is all zero or has every element below 2^-14 makes the bound infinite, NaN or wider than any distance, so
  upper == 0 -- which the GPU test turns into "0 discarded on the device".  Where the bound survives (norm 1e4 under
  cosine) the order of the counts still holds and the device's count is held between them.
* the write-path checkpoints behind the row with an element of 1e6 (until compact) have an infinite Emax: upper == 0
  is asserted."""
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
    case.check(t)
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


def test_dispatch_beyond_the_hash_set_inputs(oracle):
    """searchSize 100, calls of 8 / 64 / 513 queries: the CPU test replays the 64 the two small calls are made of (the
    GPU test replays all 513); both prefixes must prove something"""
    case = F.dispatch_beyond_hash_case(oracle)
    assert case.queries.shape[0] == 513 and len(case.filters) == 513 and case.L == 100
    first = F.Case(case.what, case.metric, case.d, case.ex, case.o, case.queries[:64], case.filters[:64], case.limit, case.L)
    _check(oracle, first)
    _, t8 = first.prefix(oracle, 8)
    first.check(t8)


@pytest.mark.parametrize("metric", F.METRICS)
def test_overflow_list_inputs(oracle, metric):
    for L, limit in F.OVERFLOW_L:
        case = F.overflow_case(oracle, metric, L, limit)
        assert case.g.deg[case.g.start] > 128
        t = _check(oracle, case)
        if L > 1:  # (L = 1: an array of one entry is sorted -- its last distance cannot rise)
            assert t.risen > 0, case.what


@pytest.mark.parametrize("metric,d", F.HOSTILE_TABLES)
def test_hostile_query_inputs(oracle, metric, d):
    none = []
    for kind in F.HOSTILE_KINDS:
        t = _check(oracle, F.hostile_case(oracle, metric, d, kind))
        assert t.full > 0, kind
        if t.upper == 0:
            none.append(kind)
    # the float16 query is infinite, NaN or all zero: nothing is provable, under any metric
    assert set(("overflow", "nan", "inf", "zero", "tiny")) <= set(none), none


@pytest.mark.parametrize("metric", ["cosine", "euclidean"])
def test_write_path_inputs(oracle, metric):
    steps = F.write_path_steps(oracle, metric)
    assert len(steps) == 6
    for st in steps:
        t = _check(oracle, st.case)
        if st.expect_none:
            assert t.upper == 0 and t.full > 0, st.what
    assert len(steps[1].case.ex[0]) <= F.WRITE_GROWS_PAST < len(steps[2].case.ex[0])  # the transaction grows the table


def test_reader_inputs(oracle):
    base, rows = F.reader_case(oracle)
    assert rows.shape == (10, 128) and base.L == 40
