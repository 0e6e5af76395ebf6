"""The conditions of tests/test_gpu_visited_spill.py, asserted without a GPU: on every batch that file sends to the
device, the limits of its sweep make the walks spill where the test means them to (tests/visited_spill_model.py
check_conditions), so that no GPU case can pass by never leaving the LDS table.  Each test prints, per case, the smallest
and the median number of marks of a query and how many queries pass each limit (pytest -s)."""
import numpy as np
import pytest

from tests import two_precision_model as M
from tests import visited_spill_model as S
from tests.helpers import bits


def _check(case):
    line = S.check_conditions(case)
    print(line)
    return line


def test_the_sweep_of_a_made_up_batch():
    """the conditions themselves, on marks written down here: they hold for a batch like the tests', and each one
    refuses the batch that breaks it"""
    class Stub(S.Case):
        def __init__(self, marks, L=40, fixed=None):
            super().__init__(None, "stub", "cosine", 8, None, None, 10, L, fixed=fixed)
            self._marks = np.asarray(marks, dtype=np.int64)

    ok = Stub(np.arange(1400, 1432))
    assert ok.sweep() == (0, 1, 63, 64, 700, 1398, 1415)
    assert "lo 1400 med 1415" in S.check_conditions(ok)
    with pytest.raises(AssertionError, match="median"):
        S.check_conditions(Stub([1400] * 30 + [1401, 1500]))      # nobody is past the median + 1 but one query
    with pytest.raises(AssertionError, match="searchSize"):
        S.check_conditions(Stub(np.arange(200, 232), L=40))       # lo // 2 = 100 <= 104: the array may not be full yet
    with pytest.raises(AssertionError, match="only"):
        S.check_conditions(Stub([60] + list(range(1400, 1431)), fixed=(0, 1, 64)))  # a query that never passes 64
    with pytest.raises(AssertionError, match="control"):
        S.check_conditions(Stub(np.arange(5990, 6022)))           # the control itself would spill


@pytest.mark.parametrize("metric,d,L", sorted(set(S.F32_CASES + S.F16_CASES + S.INT8_CASES + S.WIDE16_CASES)))
def test_one_wave_and_sixteen_wave_batches(oracle, metric, d, L):
    case = S.plain_case(oracle, metric, d, L)
    _check(case)
    # the replay the GPU test compares with is the oracle's walk, visit order included
    reps = case.replays()[0]
    for i, r in enumerate(reps):
        o_ids, o_d, o_vis, o_tr = case.o.search(case.queries[i], case.limit, case.L)
        assert np.array_equal(r.ids, o_ids) and np.array_equal(bits(r.dists), bits(o_d)) and np.array_equal(r.visit, o_vis)
        assert r.n_dist == o_tr.n_dist == case.marks()[i]
    if (metric, d, L) in S.F16_CASES:
        M.check_tally(case.replays()[1], case.what)


@pytest.mark.parametrize("L", sorted(set(S.OVERFLOW_L + S.WIDE16_OVERFLOW_L)))
def test_overflow_list_batches(oracle, L):
    case = S.overflow_case(oracle, L, 1 if L in S.OVERFLOW_L else S.LIMIT)
    assert case.g.deg[case.g.start] > 64 + 64 + 2   # T = 130 is reached inside the start node's third chunk
    _check(case)


@pytest.mark.parametrize("metric,d", S.WIDE8_CASES)
def test_eight_wave_batches(oracle, metric, d):
    case = S.wide8_case(oracle, metric, d)
    assert 256 < case.queries.shape[0] <= 512
    _check(case)


def test_filtered_batch(oracle):
    case = S.filtered_case(oracle)
    assert sorted(set(len(f) for f in case.filters)) == [5, case.L, (len(case.g.ids) - 1) // 2]
    _check(case)


def test_seam_batch(oracle):
    case = S.seam_case(oracle)
    assert case.queries.shape[0] == S.SEAM[1]
    _check(case)
    assert case.sweep()[1] > case.L + 64
