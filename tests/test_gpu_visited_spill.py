"""The visited set's spill from LDS to the HBM bitset, forced in the middle of the walk in every walk kernel that has one.

A query that has marked more than `hash_limit` ids clears its bitset, replays its LDS table into it and carries on there
(visited_set.h HashVisited::spill).  Test tables are too small to reach the default limit of 6000, so each batch here
runs at hash_limit = T for every T of a sweep (tests/visited_spill_model.py): 0 (the control: nothing spills), 1 (in the
start node's row), 63 and 64 (either side of one full chunk), lo // 2 (mid-walk, the candidate array full, a first stage
discarding), lo - 2 (every query within its last marks) and the batch's median (about half the waves of a launch spill),
with lo the smallest number of ids a query of the batch marks.  That the walks do spill at these limits is asserted from
the oracle alone, without a GPU, by tests/test_visited_spill_model.py; no kernel counts its spills.

Every run, at every T: ids, distance bits, counts, n_dist, n_hop, n_edges and the visit log equal the replay's, which
equals the oracle's walk; and the whole answer is bit-identical to the T = 0 run on the same index.  A spill that loses
or repeats a mark changes n_dist and the visit order of exactly the queries that cross the limit.  The staged walks
(float16 first stage: sketch 2 = audited, 1; int8: 4 = audited, 3) also report the copy in use, contradict no discard,
discard a count inside the float64 model's sandwich, and discard the SAME count at every T under both knobs: a discard
depends on the candidate array and the bound, never on where the visited set lives.

The kernels: the one-wave float32 hash walk (sketch 0) with a tail chain, NG 3 and NG 8, cosine and euclidean; the
one-wave walks with a float16 / int8 first stage, whose stage_begin() has a hop's copy rows in flight when
test_and_set() spills; either stage on a start node with an overflow list; the workgroup-per-query walk with sixteen
waves and helpers marking ahead of the walker (wide_walk 2: claim / credit / unmark, credit() itself spills), with eight
waves at NG 8, with eight waves and nobody ahead (300 queries on the default dispatch), on the overflow-list table (the
marker stays off while the list lasts) and in its filtered form (the result set's table spills too, at T / 8); and the
default dispatch either side of its seam at 512 / 513 queries.

Shown to bite on scratch builds (none kept; profiles/r10_visited_spill_mutants.txt): a spill that leaves the table's last
64 cells out of the replay (0.8 % of the marks lost) fails every sweep case, the seam, the filtered form and the build
case -- n_dist rises for the queries that meet a lost id again; a marker wave that keeps claiming in the LDS table after
the spill fails the overflow-list and the filtered workgroup-per-query cases, where the walker's own tests alternate
with the marker's.  Observed on an MI355X (profiles/r10_visited_spill_sweep.log): every case passes at every limit, each
staged case with one discarded count across its whole sweep, e.g. cosine d = 384 searchSize 40, float16 stage: 44 864 of a
sandwich 44 864 .. 44 868 at all seven limits under both knobs; int8 stage: 43 267 of 43 265 .. 43 271.
"""
import numpy as np
import pytest

from tests import int8_stage_model as M8
from tests import visited_spill_model as S
from tests.helpers import bits
from tests.test_gpu_filtered_two_precision import _walk as _walk_filtered
from tests.test_gpu_two_precision_bound import _equals_replay, _index, _oracle_equals_replay, _same_bits, _walk

pytestmark = pytest.mark.gpu


def _identical(a, b, what, n=None):
    """the first n queries of two calls: ids, distance bits, counts, counters, and the visit logs up to n_hop"""
    n = a[0].shape[0] if n is None else n
    assert np.array_equal(a[0][:n], b[0][:n]) and np.array_equal(a[2][:n], b[2][:n]), "%s: ids / counts" % what
    assert _same_bits(a[1][:n], b[1][:n]), "%s: distance bits" % what
    for x, y in ((a[3].n_dist, b[3].n_dist), (a[3].n_hop, b[3].n_hop), (a[3].n_edges, b[3].n_edges)):
        assert np.array_equal(x[:n], y[:n]), "%s: counters" % what
    for i in range(n):
        k = int(b[3].n_hop[i])
        assert np.array_equal(a[3].visit_ids[i, :k], b[3].visit_ids[i, :k]), "%s query %d: visit order" % (what, i)


def _sweep(ix, case, knobs, tally=None, checked=None):
    """the case's batch at every T of its sweep under each knob of `knobs` (None: the knob left alone).  tally: the
    model's counts of a staged walk; None: the kernel has no first stage and discards nothing.  checked: how many of
    the batch's first queries are compared with the oracle one by one (default: all)."""
    print(S.check_conditions(case))
    reps = case.replays(checked)[0]
    nrep = len(reps)
    if case.filters is None:
        _oracle_equals_replay(case.o, reps, case.queries[:nrep], case.limit, case.L)
    else:
        for i, r in enumerate(reps):
            o_ids, o_d, o_vis, _ = case.o.search(case.queries[i], case.limit, case.L, filter_ids=sorted(case.filters[i]))
            assert np.array_equal(r.ids, o_ids) and np.array_equal(bits(r.dists), bits(o_d)) and np.array_equal(r.visit, o_vis)
    control, seen = {}, []
    for T in case.sweep():
        ix.set_tuning("hash_limit", T)
        for knob in knobs:
            if case.filters is None:
                ans, discarded, contradicted, in_use = _walk(ix, case.queries, case.limit, case.L, knob)
            else:
                ans, discarded, contradicted, in_use = _walk_filtered(ix, case.queries, case.limit, case.L, case.filters, knob)
            what = "%s hash_limit=%d sketch=%s" % (case.what, T, knob)
            if tally is not None:
                what += ": lower %d / discarded on the device %d / upper %d (contradicted %d)" % (tally.lower, discarded, tally.upper, contradicted)
                print(what)
            _equals_replay(ans, reps, what)
            if T == 0:
                control[knob] = ans
            else:
                _identical(ans, control[knob], what + ": against the T = 0 run")
            assert contradicted == 0, what
            if tally is None:
                assert discarded == 0, "%s: %d discarded by a walk without a first stage" % (what, discarded)
            else:
                assert in_use, what
                assert 0 < tally.lower <= discarded <= tally.upper, what
            seen.append(discarded)
    ix.set_tuning("hash_limit", 0)
    assert len(set(seen)) == 1, "%s: the discarded count moves with the limit or the knob: %r over T = %r x sketch = %r" % (case.what, seen, case.sweep(), knobs)
    return control


@pytest.mark.parametrize("metric,d,L", S.F32_CASES)
def test_float32_hash_walk(oracle, metric, d, L):
    from semadb_amd import vamana
    case = S.plain_case(oracle, metric, d, L)
    ix = _index(vamana, metric, d, case.ex)
    _sweep(ix, case, (0,))
    assert not ix.sketch_stats()[2]
    ix.close()


@pytest.mark.parametrize("metric,d,L", S.F16_CASES)
def test_float16_first_stage(oracle, metric, d, L):
    from semadb_amd import vamana
    case = S.plain_case(oracle, metric, d, L)
    ix = _index(vamana, metric, d, case.ex)
    _sweep(ix, case, (2, 1), case.replays()[1])
    ix.close()


@pytest.mark.parametrize("metric,d,L", S.INT8_CASES)
def test_int8_first_stage(oracle, metric, d, L):
    from semadb_amd import vamana
    case = S.plain_case(oracle, metric, d, L)
    ix = _index(vamana, metric, d, case.ex)
    tally = M8.run_model8(oracle, case.g, metric, case.queries, case.limit, case.L)[1]
    M8.check_tally8(tally, case.what)
    control = _sweep(ix, case, (4, 3), tally)
    # the int8 walk's answers are the float32 walk's, at the default limit and mid-walk
    for T in (0, case.lo_med()[0] // 2):
        ix.set_tuning("hash_limit", T)
        _identical(_walk(ix, case.queries, case.limit, case.L, 0)[0], control[3], "%s hash_limit=%d: sketch 0 against 3" % (case.what, T))
    ix.close()


@pytest.mark.parametrize("L", S.OVERFLOW_L)
def test_either_stage_on_a_start_node_with_an_overflow_list(oracle, L):
    """the start node has more than 128 edges and the array is full from its first chunk on: at T = 1, 64 and 130 the
    spill lands inside the start node's first, second and third chunk"""
    from semadb_amd import vamana
    case = S.overflow_case(oracle, L)
    ix = _index(vamana, "cosine", 128, case.ex)
    _sweep(ix, case, (2, 1), case.replays()[1])
    _sweep(ix, case, (4, 3), M8.run_model8(oracle, case.g, "cosine", case.queries, case.limit, case.L)[1])
    ix.close()


@pytest.mark.parametrize("metric,d,L", S.WIDE16_CASES)
def test_workgroup_per_query_with_helpers_ahead(oracle, metric, d, L):
    """wide_walk 2, 32 queries: sixteen waves per query (eight at d = 1024) and the marker wave ahead of the walker.  The
    table holds a copy where its shape has one, and nothing is discarded: the kernel that ran has no first stage."""
    from semadb_amd import vamana
    case = S.plain_case(oracle, metric, d, L)
    ix = _index(vamana, metric, d, case.ex, wide_walk=2)
    _sweep(ix, case, (None,))
    assert ix.sketch_stats()[2] == (d != 1024)
    ix.close()


@pytest.mark.parametrize("L", S.WIDE16_OVERFLOW_L)
def test_workgroup_per_query_on_an_overflow_list(oracle, L):
    from semadb_amd import vamana
    case = S.overflow_case(oracle, L, S.LIMIT if L >= S.LIMIT else 1)
    ix = _index(vamana, "cosine", 128, case.ex, wide_walk=2)
    _sweep(ix, case, (None,))
    ix.close()


@pytest.mark.parametrize("metric,d", S.WIDE8_CASES)
def test_workgroup_per_query_with_eight_waves(oracle, metric, d):
    """300 queries on the default dispatch: eight waves per query, nobody ahead of the walker.  The first 32 queries are
    compared with the oracle one by one, all 300 with the T = 0 run."""
    from semadb_amd import vamana
    case = S.wide8_case(oracle, metric, d)
    ix = _index(vamana, metric, d, case.ex, wide_walk=None)
    _sweep(ix, case, (None,), checked=S.WIDE8_CHECKED)
    ix.close()


def test_workgroup_per_query_filtered(oracle):
    """filters of 5, L and n / 2 ids: the search set and the result set (a table of 1 024 cells: its limit is T / 8) both
    spill, into bitsets of their own"""
    from semadb_amd import vamana
    case = S.filtered_case(oracle)
    ix = _index(vamana, "cosine", 384, case.ex, wide_walk=2)
    _sweep(ix, case, (None,))
    ix.close()


def test_default_dispatch_at_the_seam(oracle):
    """wide_walk left alone, d = 128: 512 queries stay on the many-waves kernel (nothing discarded), 513 take the int8
    walk; at T = lo // 2 as at T = 0 the shared queries get the same answers from both, the oracle's for the first 32"""
    from semadb_amd import vamana
    case = S.seam_case(oracle)
    print(S.check_conditions(case))
    ix = _index(vamana, "cosine", 128, case.ex, wide_walk=None)
    reps = case.replays(32)[0]
    _oracle_equals_replay(case.o, reps, case.queries[:32], case.limit, case.L)
    small, big = S.SEAM
    for knob in (4, 3):
        control, seen = None, []
        for T in case.sweep():
            ix.set_tuning("hash_limit", T)
            what = "seam hash_limit=%d sketch=%d" % (T, knob)
            a, discarded, contradicted, in_use = _walk(ix, case.queries[:small], case.limit, case.L, knob)
            assert in_use and discarded == 0 and contradicted == 0, "%s: %d discarded by %d queries" % (what, discarded, small)
            b, discarded, contradicted, in_use = _walk(ix, case.queries[:big], case.limit, case.L, None)
            print("%s: %d discarded by %d queries" % (what, discarded, big))
            assert in_use and discarded > 0 and contradicted == 0, what
            _equals_replay(a, reps, what)
            _equals_replay(b, reps, what)
            _identical(a, b, what + ": %d against %d queries" % (small, big), small)
            if control is None:
                control = (a, b)
            else:
                _identical(a, control[0], what + ": against the T = 0 run")
                _identical(b, control[1], what + ": against the T = 0 run")
            seen.append(discarded)
        assert len(set(seen)) == 1, "sketch=%d: the discarded count moves with the limit: %r" % (knob, seen)
    ix.close()
