"""The two-precision hop on filtered batch searches, between two independent counts.

A filtered walk's candidate array is not sorted (its seeds are appended by Add), so its last distance can rise within
a chunk of neighbours; the kernel's threshold is B, the maximum of the array's last min(k, L) distances as a chunk with
k new neighbours starts (cand_array.h list_tail_bound).  tests/filtered_two_precision_model.py restates the filtered
walk in numpy and counts, against B, the neighbours the pure float16 bound proves discardable (`upper`) and those it
still proves with every inflation the kernel documents charged generously (`lower`).  For sketch = 2 (audit) and then 1
every case asserts the oracle's answers per query (ids, distance bits, counts, n_dist / n_hop / n_edges, visit order),
the copy in use, contradicted == 0, lower <= discarded on the device <= upper, and the same count in both modes.

A walk that reads float32 rows only (the filtered walk before it had the stage) discards 0 and falls below `lower`; a
kernel that keeps the chunk-start last distance as its threshold lands above `upper` or returns other answers: the CPU
test (test_filtered_two_precision_model.py) asserts that every sandwich input holds neighbours that threshold would
discard and the reference keeps.

All cases run with wide_walk = 1 (one wave per query, the kernel that has the stage) except the two dispatch tests, and
with the opt-in SDB_TUNE_SKETCH_FILTERED set: without it (the default) a filtered call reads float32 rows only
(test_off_by_default).

The routing these tests state (csrc/walk_plan.h, not imported): a filtered call takes the stage at every batch
size when searchSize is 97 .. 128 (the many-waves kernel needs the LDS hash set, which ends at 96), at searchSize <= 96
when the many-waves kernel does not keep the call (wide_walk = 1, or more than 512 / 256 queries), never with
no_hash = 1, never inside an open transaction, never past searchSize 128.

The float64 model is what sees a wrong window in list_tail_bound: the audit compares a discarded neighbour with the
kernel's own threshold, so `first = cap - k + 1` contradicts nothing; it raises the device's count above `upper` or
changes answers only where the window's first entry is its maximum -- which the unsorted seeds of the filter kinds, the
searchSize 1 / 2 cases and the overflow-list cases supply.
"""
import threading

import numpy as np
import pytest

from tests import filtered_two_precision_model as F
from tests.helpers import assert_same_graph, bits

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
    case.check(t)
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
    """L = 1 and 2 (min(k, L) is the whole array), 5 = limit, 10, 64, 96 / 97 (either side of the plain calls' LDS set, csrc/walk_plan.h: a
    filtered call keeps the hop, and from 97 on no bitset is cleared ahead of the launch), 128 (the last the kernel's two
    array registers hold); L < limit: refused; L = 129: the float32 walk"""
    first = F.width_case(oracle, metric, 128, False)
    ix = _index(first)
    for L, limit in F.L_CASES:
        _sandwich(ix, oracle, F.width_case(oracle, metric, 128, False, limit, L))
    # L = 128 once more with LDS visited sets that give up after 24 ids: at 97 .. 128 no bitset is cleared ahead of the
    # launch, both sets spill into bitsets they clear themselves (HashVisited::spill)
    ix.set_tuning("hash_limit", 24)
    _sandwich(ix, oracle, F.width_case(oracle, metric, 128, False, 10, 128))
    ix.set_tuning("hash_limit", 0)
    # searchSize < limit (search.go:23-25): refused by both sides, nothing walked, the counters as they were
    from semadb_amd._lib import SemaDBError
    L, limit = F.L_REFUSED
    with pytest.raises(ValueError):
        first.o.search(first.queries[0], limit, L, filter_ids=sorted(first.filters[0]))
    before = ix.sketch_stats()[:2]
    with pytest.raises(SemaDBError):
        ix.search_batch(first.queries, limit, L, filters=first.filters)
    assert ix.sketch_stats()[:2] == before
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


def _same_answers(a, b, n, what):
    """the first n queries of two calls: ids, distance bits, counts, counters, visit order up to n_hop"""
    assert np.array_equal(a[0][:n], b[0][:n]) and np.array_equal(a[2][:n], b[2][:n]), what
    for i in range(n):
        k = int(b[2][i])
        assert _same_bits(a[1][i, :k], b[1][i, :k]), "%s query %d: distance bits" % (what, i)
        h = int(b[3].n_hop[i])
        assert np.array_equal(a[3].visit_ids[i, :h], b[3].visit_ids[i, :h]), "%s query %d: visit order" % (what, i)
    for x, y in ((a[3].n_dist, b[3].n_dist), (a[3].n_hop, b[3].n_hop), (a[3].n_edges, b[3].n_edges)):
        assert np.array_equal(x[:n], y[:n]), what


def test_default_dispatch_beyond_the_hash_set(oracle):
    """searchSize 100, wide_walk at its default: the many-waves kernel is out of the dispatch at every batch size, so
    calls of 8, 64 and 513 queries all take the stage -- each inside its own sandwich with lower > 0, the same per-query
    answers from the three.  Once more with LDS sets that give up after 24 ids: they spill into bitsets that nobody
    cleared ahead of the launch (csrc/walk_plan.h: the plan of such a call asks for no clear)."""
    case = F.dispatch_beyond_hash_case(oracle)
    reps, _ = case.model(oracle)
    _oracle_equals_replay(F.Case(case.what, case.metric, case.d, case.ex, case.o, case.queries[:64], case.filters[:64],
                                 case.limit, case.L), reps[:64])
    ix = _index(case, wide_walk=None)
    for hash_limit in (0, 24):
        ix.set_tuning("hash_limit", hash_limit)
        for mode in (2, 1):
            ix.set_tuning("sketch", mode)
            for nq in F.DISPATCH_SIZES:
                what = "L=100 %d queries sketch=%d hash_limit=%d" % (nq, mode, hash_limit)
                r, t = case.prefix(oracle, nq)
                case.check(t)
                ans, discarded, contradicted, in_use = _walk(ix, case.queries[:nq], case.limit, case.L, case.filters[:nq], None)
                msg = "%s: lower %d / discarded on the device %d / upper %d (contradicted %d)" % (what, t.lower, discarded, t.upper, contradicted)
                print(msg)
                assert in_use and contradicted == 0, msg
                _equals_replay(ans, r, what)
                assert 0 < t.lower <= discarded <= t.upper, msg
    ix.close()


@pytest.mark.parametrize("metric", F.METRICS)
def test_no_hash_has_no_stage(oracle, metric):
    """no_hash = 1 (SearchArgs::prefer_bitset): the bitset kernel walks, which has no stage"""
    case = F.width_case(oracle, metric, 256, False)
    reps, _ = case.model(oracle)
    ix = _index(case)
    ix.set_tuning("no_hash", 1)
    for mode in (2, 1):
        ans, discarded, contradicted, _ = _walk(ix, case.queries, case.limit, case.L, case.filters, mode)
        assert discarded == 0 and contradicted == 0, "%s no_hash sketch=%d: %d discarded" % (case.what, mode, discarded)
        _equals_replay(ans, reps, case.what + " no_hash")
    ix.set_tuning("no_hash", 0)
    ans, discarded, _, _ = _walk(ix, case.queries, case.limit, case.L, case.filters, 1)
    assert discarded > 0
    _equals_replay(ans, reps, case.what)
    ix.close()


@pytest.mark.parametrize("metric", F.METRICS)
def test_start_node_with_an_overflow_list(oracle, metric):
    """a start node of more than 64 + 64 edges: one expansion is several chunks, the array's last distance moves between
    them and, unsorted, can rise; at L = 1 and 2 the array is full from the first chunk on"""
    ix = None
    for L, limit in F.OVERFLOW_L:
        case = F.overflow_case(oracle, metric, L, limit)
        assert case.g.deg[case.g.start] > 128
        if ix is None:
            ix = _index(case)
        _sandwich(ix, oracle, case)
    ix.close()


@pytest.mark.parametrize("metric,d", F.HOSTILE_TABLES)
def test_hostile_queries(oracle, metric, d):
    """queries that break or strain the float16 copy of the query: nothing discarded wherever the model's bound proves
    nothing (upper == 0), the sandwich otherwise; the oracle's answers, NaN distances included"""
    ix = _index(F.width_case(oracle, metric, d, False))
    for kind in F.HOSTILE_KINDS:
        case = F.hostile_case(oracle, metric, d, kind)
        _sandwich(ix, oracle, case, expect_none=case.model(oracle)[1].upper == 0)
    ix.close()


def _write_index(vamana, case, filtered_hop):
    # (the parameters of the oracle that F.write_path_steps writes to)
    ix = vamana.NewIndexVamana("t", vamana.IndexVectorVamanaParameters(case.d, case.metric, 40, 64, 1.2), capacity=2048, strict=False)
    ix.set_tuning("wide_walk", 1)
    ix.set_tuning("sketch_filtered", 1 if filtered_hop else 0)
    ix.load(*case.ex)
    return ix


@pytest.mark.parametrize("metric", ["cosine", "euclidean"])
def test_write_paths(oracle, metric):
    """the filtered twin of test_maxima_through_every_write_path: after every write the device's count is inside the
    sandwich of the maxima carried since the last full conversion, the filters resolve through this version's id -> slot
    table (each names ids the write deleted, updated and added), and the answers are those of a twin index that never
    takes the hop on a filtered call, and the oracle's.  Inside the open transaction: no copy in use, 0 discarded, the
    committed version's answers."""
    from semadb_amd import vamana
    steps = F.write_path_steps(oracle, metric)
    ix = _write_index(vamana, steps[0].case, True)
    twin = _write_index(vamana, steps[0].case, False)
    prev = None
    for st in steps:
        case = st.case
        for op in st.ops:
            for t in (ix, twin):
                if op[0] == "iud":
                    t.InsertUpdateDelete([vamana.IndexVectorChange(int(i), None if r is None else r) for i, r in op[1]], round_size=1)
                elif op[0] == "delete":
                    t.delete_batch(np.array(op[1], dtype=np.uint64))
                elif op[0] == "compact":
                    t.compact()
                else:
                    before = t.SizeInMemory()
                    t.begin_write()
                    t.insert_batch(np.array(op[1], dtype=np.uint64), op[2], round_size=1)
                    if t is ix:  # inside the open transaction
                        for mode in (2, 1):
                            ans, discarded, contradicted, in_use = _walk(ix, prev.queries, prev.limit, prev.L, prev.filters, mode)
                            assert not in_use and discarded == 0 and contradicted == 0, "inside the transaction, sketch=%d: %d discarded" % (mode, discarded)
                            _equals_replay(ans, prev.model(oracle)[0], "inside the transaction")
                    t.commit()
                    assert t.SizeInMemory() > 1.5 * before, "the table did not grow"
        assert_same_graph(ix, case.o)
        got = _sandwich(ix, oracle, case, expect_none=st.expect_none)
        ref, discarded, _, _ = _walk(twin, case.queries, case.limit, case.L, case.filters, None)
        assert discarded == 0, "%s: the twin discarded %d" % (case.what, discarded)
        _same_answers(got, ref, case.queries.shape[0], case.what + ": differs from the float32 walk")
        prev = case
    ix.close()
    twin.close()


def test_reader_sees_one_committed_version_while_the_writer_commits(oracle):
    """a reader thread asks filtered searches, with the hop, while the writer commits one-point inserts; every answer
    it sees is the float32 answer of one committed version (a twin without the filtered hop receives the same writes)"""
    from semadb_amd import vamana
    case, rows = F.reader_case(oracle)
    ix, twin = _write_index(vamana, case, True), _write_index(vamana, case, False)

    def ask(t):
        ids, dd, c = t.search_batch(case.queries, case.limit, case.L, filters=case.filters)[:3]
        return ids.copy(), bits(dd).copy(), c.copy()

    versions = [ask(twin)]
    seen, stop, errors = [], threading.Event(), []

    def reader():
        try:
            while not stop.is_set():
                seen.append(ask(ix))
        except Exception as e:  # pragma: no cover - reported below
            errors.append(e)

    th = threading.Thread(target=reader)
    th.start()
    try:
        for i in range(rows.shape[0]):
            pid = np.array([9000 + i], dtype=np.uint64)
            ix.insert_batch(pid, rows[i:i + 1], round_size=1)
            twin.insert_batch(pid, rows[i:i + 1], round_size=1)
            versions.append(ask(twin))
    finally:
        stop.set()
        th.join()
    assert not errors, errors
    assert seen
    for got in seen:
        assert any(all(np.array_equal(x, y) for x, y in zip(got, v)) for v in versions), "an answer that no committed version gives"
    discarded, contradicted, in_use = ix.sketch_stats()
    assert in_use and discarded > 0 and contradicted == 0
    assert all(np.array_equal(x, y) for x, y in zip(ask(ix), versions[-1]))
    assert twin.sketch_stats()[0] == 0
    ix.close()
    twin.close()
