"""The two-precision hop on filtered batch searches, between two independent counts.

A filtered walk's candidate array is not sorted (its seeds are appended by Add), so its last distance can rise within
a chunk of neighbours; the kernel's threshold is B, the maximum of the array's last min(k, L) distances as a chunk with
k new neighbours starts (search_kernel.h list_tail_bound).  tests/filtered_two_precision_model.py restates the filtered
walk in numpy and counts, against B, the neighbours the pure float16 bound proves discardable (`upper`) and those it
still proves with every inflation the kernel documents charged generously (`lower`).  For sketch = 2 (audit) and then 1
every case asserts the oracle's answers per query (ids, distance bits, counts, n_dist / n_hop / n_edges, visit order),
the copy in use, contradicted == 0, lower <= discarded on the device <= upper, and the same count in both modes.

A walk that reads float32 rows only (the filtered walk before it had the stage) discards 0 and falls below `lower`; a
kernel that keeps the chunk-start last distance as its threshold lands above `upper` or returns other answers: the CPU
test (test_filtered_two_precision_model.py) asserts that every sandwich input holds neighbours that threshold would
discard and the reference keeps.

All cases run with wide_walk = 1 (one wave per query, the kernel that has the stage) except test_default_dispatch, and
with the opt-in SDB_TUNE_SKETCH_FILTERED set: without it (the default) a filtered call reads float32 rows only
(test_off_by_default).
"""
import numpy as np
import pytest

from tests import filtered_two_precision_model as F
from tests.helpers import bits

pytestmark = pytest.mark.gpu


def _index(case, wide_walk=1, R=64, filtered_hop=True):
    from semadb_amd import vamana
    ix = vamana.NewIndexVamana("t", vamana.IndexVectorVamanaParameters(case.d, case.metric, 75, R, 1.2), strict=False)
    if wide_walk is not None:
        ix.set_tuning("wide_walk", wide_walk)
    ix.set_tuning("sketch_filtered", 1 if filtered_hop else 0)
    ix.load(*case.ex)
    return ix


def _walk(ix, queries, limit, L, filters, mode):
    """answers and the (discarded, contradicted) the call added; setting the knob clears the counters"""
    if mode is not None:
        ix.set_tuning("sketch", mode)
    d0, c0, _ = ix.sketch_stats()
    ans = ix.search_batch(queries, limit, L, filters=filters, trace=True, visit_cap=1024)
    d1, c1, in_use = ix.sketch_stats()
    return ans, d1 - d0, c1 - c0, in_use


def _same_bits(a, b):
    """bit for bit, or a NaN where the reference has a NaN (a NaN's sign and payload differ between the machines)"""
    a, b = np.ascontiguousarray(a, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32)
    na, nb = np.isnan(a), np.isnan(b)
    return np.array_equal(na, nb) and np.array_equal(bits(a)[~na], bits(b)[~nb])


def _equals_replay(ans, reps, what):
    ids, d, c, tr = ans
    for i, r in enumerate(reps):
        k = len(r.ids)
        assert int(c[i]) == k, "%s query %d: count" % (what, i)
        assert np.array_equal(ids[i, :k], r.ids), "%s query %d: ids" % (what, i)
        assert _same_bits(d[i, :k], r.dists), "%s query %d: distance bits" % (what, i)
        assert (int(tr.n_dist[i]), int(tr.n_hop[i]), int(tr.n_edges[i])) == (r.n_dist, r.n_hop, r.n_edges), "%s query %d: counters" % (what, i)
        assert np.array_equal(tr.visit_ids[i, :r.n_hop], r.visit), "%s query %d: visit order" % (what, i)


def _oracle_equals_replay(case, reps):
    for i, r in enumerate(reps):
        o_ids, o_d, o_vis, o_tr = case.o.search(case.queries[i], case.limit, case.L, filter_ids=sorted(case.filters[i]))
        assert np.array_equal(r.ids, o_ids) and _same_bits(r.dists, o_d) and np.array_equal(r.visit, o_vis), case.what
        assert (r.n_hop, r.n_dist, r.n_edges) == (o_tr.n_hop, o_tr.n_dist, o_tr.n_edges), case.what


def _sandwich(ix, oracle, case, filters=None, expect_none=False):
    """audit run and plain run of the case's batch.  `filters`: the same filters in another form (bitmaps)"""
    reps, t = case.model(oracle)
    _oracle_equals_replay(case, reps)
    F.check_tally(t, case.what, case.sandwich)
    seen = []
    for mode in (2, 1):
        ans, discarded, contradicted, in_use = _walk(ix, case.queries, case.limit, case.L, case.filters if filters is None else filters, mode)
        msg = "%s sketch=%d: lower %d / discarded on the device %d / upper %d (discardable %d of %d; contradicted %d)" % (
            case.what, mode, t.lower, discarded, t.upper, t.discardable, t.full, contradicted)
        print(msg)
        assert in_use, msg
        _equals_replay(ans, reps, case.what)
        assert contradicted == 0, msg
        assert t.lower <= discarded <= t.upper, msg
        if expect_none:
            assert discarded == 0 and t.upper == 0, msg
        seen.append(discarded)
    assert seen[0] == seen[1], "%s: the audit run discarded %d, the plain run %d" % (case.what, seen[0], seen[1])
    return ans


@pytest.mark.parametrize("metric,d,full_rows", F.WIDTH_CASES)
def test_widths_metrics_and_filter_sizes(oracle, metric, d, full_rows):
    """filters of 5, L - 1, L, 3 L, n / 2 ids and mostly unknown ids in turn over the 32 queries"""
    case = F.width_case(oracle, metric, d, full_rows)
    ix = _index(case)
    _sandwich(ix, oracle, case)
    ix.close()


@pytest.mark.parametrize("metric", F.METRICS)
def test_search_sizes(oracle, metric):
    """L = 10 with limit 10, L = 128 (the last the kernel's two array registers hold); L = 129: the float32 walk"""
    first = F.width_case(oracle, metric, 128, False)
    ix = _index(first)
    for L, limit in F.L_CASES:
        _sandwich(ix, oracle, F.width_case(oracle, metric, 128, False, limit, L))
    # L = 128 once more with LDS visited sets that give up after 24 ids: at 97 .. 128 no bitset is cleared ahead of the
    # launch, both sets spill into bitsets they clear themselves (HashVisited::spill)
    ix.set_tuning("hash_limit", 24)
    _sandwich(ix, oracle, F.width_case(oracle, metric, 128, False, 10, 128))
    ix.set_tuning("hash_limit", 0)
    case = F.width_case(oracle, metric, 128, False, 10, F.L_NO_STAGE)
    reps, _ = case.model(oracle)
    _oracle_equals_replay(case, reps)
    for mode in (2, 1):
        ans, discarded, contradicted, _ = _walk(ix, case.queries, case.limit, case.L, case.filters, mode)
        _equals_replay(ans, reps, case.what)
        assert discarded == 0 and contradicted == 0, "%s sketch=%d: %d discarded" % (case.what, mode, discarded)
    ix.close()


@pytest.mark.parametrize("metric", F.METRICS)
def test_table_with_holes_and_rows_out_of_id_order(oracle, metric):
    """ids with holes resolve through the id -> slot table on the device; ascending ids are not ascending slots, so
    Contains is answered from the id lists (SearchArgs::filt_ids)"""
    case = F.holes_case(oracle, metric)
    ix = _index(case)
    _sandwich(ix, oracle, case)
    ix.close()


def test_off_by_default(oracle):
    """without SDB_TUNE_SKETCH_FILTERED a filtered call discards nothing and answers the same; a plain call on the same
    index keeps its stage"""
    case = F.width_case(oracle, "cosine", 128, False)
    reps, _ = case.model(oracle)
    ix = _index(case, filtered_hop=False)
    for mode in (2, 1):
        ans, discarded, contradicted, in_use = _walk(ix, case.queries, case.limit, case.L, case.filters, mode)
        assert in_use and discarded == 0 and contradicted == 0, "sketch=%d: %d discarded" % (mode, discarded)
        _equals_replay(ans, reps, case.what)
        _, plain, _, _ = _walk(ix, case.queries, case.limit, case.L, None, None)
        assert plain > 0
    ix.set_tuning("sketch_filtered", 1)
    _, discarded, _, _ = _walk(ix, case.queries, case.limit, case.L, case.filters, 1)
    assert discarded > 0
    ix.close()


def test_bitmap_entry_point(oracle):
    from semadb_amd import vamana
    case = F.width_case(oracle, "cosine", 128, False)
    ix = _index(case)
    got = _sandwich(ix, oracle, case, filters=vamana.FilterBitmaps.from_sets(case.filters, align=64))
    lists, _, _, _ = _walk(ix, case.queries, case.limit, case.L, case.filters, None)
    assert np.array_equal(got[0], lists[0]) and np.array_equal(bits(got[1]), bits(lists[1])) and np.array_equal(got[2], lists[2])
    ix.close()


@pytest.mark.parametrize("metric", ["cosine", "euclidean"])
def test_nan_row_among_the_seeds(oracle, metric):
    """the table-wide bound is NaN: nothing is discarded, and the answers are the float32 walk's"""
    case = F.nan_case(oracle, metric)
    ix = _index(case)
    got = _sandwich(ix, oracle, case, expect_none=True)
    ref, discarded, _, in_use = _walk(ix, case.queries, case.limit, case.L, case.filters, 0)
    assert not in_use and discarded == 0
    assert np.array_equal(got[0], ref[0]) and np.array_equal(got[2], ref[2]) and np.array_equal(got[3].n_dist, ref[3].n_dist)
    for i in range(case.queries.shape[0]):
        k = int(ref[2][i])
        assert _same_bits(got[1][i, :k], ref[1][i, :k]) and np.array_equal(got[3].visit_ids[i, :int(ref[3].n_hop[i])], ref[3].visit_ids[i, :int(ref[3].n_hop[i])])
    ix.close()


@pytest.mark.parametrize("metric", ["cosine", "euclidean"])
@pytest.mark.parametrize("noise", F.NEAR_TIE_NOISE)
def test_near_ties_around_the_threshold(oracle, metric, noise):
    """B sits inside a crowd of neighbours whose distances differ by less than the bound, or not at all: every such
    neighbour is left to the exact evaluation (the sandwich is wide here; answers and contradicted == 0 carry the case)"""
    case = F.near_tie_case(oracle, metric, noise)
    ix = _index(case)
    _sandwich(ix, oracle, case)
    ix.close()


def test_default_dispatch(oracle):
    """wide_walk at its default: a filtered call of 64 queries is the workgroup-per-query kernel's (no stage: 0
    discarded), one of 513 queries the one-wave kernel's (the stage); the same per-query answers from both, the oracle's"""
    case = F.dispatch_case(oracle)
    ix = _index(case, wide_walk=None)
    for mode in (2, 1):
        small, d_small, c_small, in_use = _walk(ix, case.queries[:64], case.limit, case.L, case.filters[:64], mode)
        assert in_use and d_small == 0 and c_small == 0, "sketch=%d: %d discarded by a call the many-waves kernel keeps" % (mode, d_small)
        big, d_big, c_big, in_use = _walk(ix, case.queries, case.limit, case.L, case.filters, None)
        assert in_use and d_big > 0 and c_big == 0, "sketch=%d: %d discarded by a call of 513 queries" % (mode, d_big)
        assert np.array_equal(small[0], big[0][:64]) and np.array_equal(bits(small[1]), bits(big[1][:64])) and np.array_equal(small[2], big[2][:64])
        for a, b in ((small[3].n_dist, big[3].n_dist), (small[3].n_hop, big[3].n_hop), (small[3].n_edges, big[3].n_edges)):
            assert np.array_equal(a, b[:64])
        for i in range(0, 513, 1 if mode == 2 else 8):
            o_ids, o_d, o_vis, o_tr = case.o.search(case.queries[i], case.limit, case.L, filter_ids=sorted(case.filters[i]))
            k = len(o_ids)
            assert int(big[2][i]) == k and np.array_equal(big[0][i, :k], o_ids) and np.array_equal(bits(big[1][i, :k]), bits(o_d)), i
            assert (int(big[3].n_dist[i]), int(big[3].n_hop[i]), int(big[3].n_edges[i])) == (o_tr.n_dist, o_tr.n_hop, o_tr.n_edges), i
            assert np.array_equal(big[3].visit_ids[i, :o_tr.n_hop], o_vis), i
    ix.close()
