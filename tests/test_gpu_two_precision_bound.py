"""The two-precision hop between two independent counts.

tests/two_precision_model.py restates the stage in float64 and counts, over the oracle's walk, the neighbours that the
pure bound proves discardable (`upper`) and those it still proves with every inflation the kernel documents charged
generously (`lower`).  The kernel's derivation implies  lower <= discarded on the device <= upper:  a bound that is
looser than documented, a counter that counts something else, a float16 sum that is wrong for some edge position or
some chunk of pending rows (the answers stay right: the exact stage catches what a too small sum lets through, the audit
what a too large one discards) all leave this interval, which is within 0.03 % on these inputs
(test_two_precision_model.py asserts 1 %).  Adjacency rows are full (R = 64) so that every pair of the rows-ahead
path and every round of HalfRows::range carries live edges.  Every query's answer, counters and visit order are compared
with the oracle's.

Observed on an MI355X, 32 queries, L = 40, lower / discarded on the device / upper (discardable, met with the array
full): cosine d = 32: 38 447 / 38 449 / 38 449 (38 465, 43 120); euclidean d = 128: 42 296 / 42 298 / 42 303 (42 343,
47 035); dot d = 384: 45 237 / 45 237 / 45 241 (45 295, 50 171); euclidean d = 512: 39 825 / 39 829 / 39 833 (39 932,
44 671); cosine d = 640: 40 039 / 40 046 / 40 051 (40 117, 44 903); euclidean d = 768: 39 922 / 39 927 / 39 929
(40 024, 44 504); 513 queries at d = 512 on the default dispatch: 638 674 / 638 705 / 638 776.  Every assertion's
message carries its case's figures.

Shown to bite on scratch builds (none kept): the bound doubled (FirstStage::eps, HalfRows::delta x 2) leaves the sandwich below
`lower` in every case that has the stage; the float16 sums of pairs 16 .. 31 zeroed, or the second round of
HalfRows::range, fail every full-row case of the path they belong to (rows of up to 384 floats; wider rows) while
test_gpu_sketch.py and test_gpu_sketch_default.py (R <= 24) stay green; the carry of the maxima dropped from
build_sketch puts the device above `upper` in test_maxima_through_every_write_path at its first small-norm append.
"""
import numpy as np
import pytest

from tests import two_precision_model as M
from tests.helpers import bits, unit_rows

pytestmark = pytest.mark.gpu

# csrc/walk_plan.h: with the default dispatch a plain call of up to 512 queries (rows of up to 384 floats) or up
# to 256 queries (wider rows) runs on the many-waves-per-query kernel, which has no first stage; above, one wave per
# query walks, with the stage.  Stated here, not imported.
WIDE_UP_TO = {128: 512, 512: 256}


def _index(vamana, metric, d, ex, wide_walk=1):
    ix = vamana.NewIndexVamana("t", vamana.IndexVectorVamanaParameters(d, metric, M.L_BUILD, M.R_FULL, 1.2), strict=False)
    if wide_walk is not None:
        ix.set_tuning("wide_walk", wide_walk)  # 1: the one-wave-per-query walk, which has the stage, at any batch size
    ix.load(*ex)
    return ix


def _walk(ix, queries, limit, L, mode, visit_cap=1024):
    """answers and the (discarded, contradicted) the call added.  Setting the knob clears the counters
    (index.hip SDB_TUNE_SKETCH, index_sketch.hip); mode None leaves it."""
    if mode is not None:
        ix.set_tuning("sketch", mode)
    d0, c0, _ = ix.sketch_stats()
    ids, d, c, tr = ix.search_batch(queries, limit, L, trace=True, visit_cap=visit_cap)
    d1, c1, in_use = ix.sketch_stats()
    return (ids, d, c, tr), d1 - d0, c1 - c0, in_use


def _same_bits(a, b):
    """bit for bit, or a NaN where the reference has a NaN: a NaN's sign and payload are the one thing the two machines
    do not share (tests/test_gpu_nonfinite.py)"""
    a, b = np.ascontiguousarray(a, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32)
    na, nb = np.isnan(a), np.isnan(b)
    return np.array_equal(na, nb) and np.array_equal(bits(a)[~na], bits(b)[~nb])


def _equals_replay(ans, reps, what):
    """every query: ids, distance bits, counts, n_dist, n_hop, n_edges, visit order (the replays equal the oracle's
    walks: _oracle_equals_replay, and test_two_precision_model.py without a GPU)"""
    ids, d, c, tr = ans
    for i, r in enumerate(reps):
        k = len(r.ids)
        assert int(c[i]) == k, "%s query %d: count" % (what, i)
        assert np.array_equal(ids[i, :k], r.ids), "%s query %d: ids" % (what, i)
        assert _same_bits(d[i, :k], r.dists), "%s query %d: distance bits" % (what, i)
        assert (int(tr.n_dist[i]), int(tr.n_hop[i]), int(tr.n_edges[i])) == (r.n_dist, r.n_hop, r.n_edges), "%s query %d: counters" % (what, i)
        assert np.array_equal(tr.visit_ids[i, :r.n_hop], r.visit), "%s query %d: visit order" % (what, i)


def _oracle_equals_replay(o, reps, queries, limit, L):
    for i, r in enumerate(reps):
        o_ids, o_d, o_vis, o_tr = o.search(queries[i], limit, L)
        assert np.array_equal(r.ids, o_ids) and np.array_equal(bits(r.dists), bits(o_d)) and np.array_equal(r.visit, o_vis)
        assert (r.n_hop, r.n_dist, r.n_edges) == (o_tr.n_hop, o_tr.n_dist, o_tr.n_edges)


def _sandwich(ix, oracle, o, g, metric, queries, limit, L, what, emax_ymax=None, expect=None):
    """audit run and plain run of one batch: answers equal the oracle's, no discard contradicted, and the device's count
    between the model's two.  expect: "none" -- the bound is infinite, nothing may be discarded; "some" -- lower > 0."""
    reps, t, _ = M.run_model(oracle, g, metric, queries, limit, L, emax_ymax)
    _oracle_equals_replay(o, reps, queries, limit, L)
    M.check_tally(t, what)
    seen = []
    for mode in (2, 1):
        ans, discarded, contradicted, in_use = _walk(ix, queries, limit, L, mode)
        msg = "%s sketch=%d: lower %d / discarded on the device %d / upper %d (discardable %d of %d; contradicted %d)" % (
            what, mode, t.lower, discarded, t.upper, t.discardable, t.full, contradicted)
        print(msg)
        assert in_use, msg
        _equals_replay(ans, reps, what)
        assert contradicted == 0, msg
        assert t.lower <= discarded <= t.upper, msg
        if expect == "none":
            assert discarded == 0 and t.upper == 0, msg
        if expect == "some":
            assert t.lower > 0, msg
        seen.append(discarded)
    assert seen[0] == seen[1], "%s: the audit run discarded %d, the plain run %d" % (what, seen[0], seen[1])
    return t, seen[1]


@pytest.mark.parametrize("metric", M.METRICS)
@pytest.mark.parametrize("d", M.WIDTHS)
def test_full_rows_every_width(oracle, metric, d):
    from semadb_amd import vamana
    ex, queries, limit, L = M.width_case(oracle, metric, d)
    g = M.Graph(*ex)
    o = M.load_oracle(oracle, metric, d, ex)
    ix = _index(vamana, metric, d, ex)
    t, _ = _sandwich(ix, oracle, o, g, metric, queries, limit, L, "%s d=%d" % (metric, d), expect="some")
    # the condition of the case: the rows the walks expand are full
    assert t.expanded_full_rows >= 0.9 * t.expanded, "%d of %d expanded nodes have 64 edges" % (t.expanded_full_rows, t.expanded)
    ix.close()


@pytest.mark.parametrize("metric", M.METRICS)
@pytest.mark.parametrize("d", M.NO_STAGE_WIDTHS)
def test_widths_without_the_stage(oracle, metric, d):
    """a tail chain (d % 32 != 0) and a group count the stage is not built for: no copy, no discard, the oracle's answers"""
    from semadb_amd import vamana
    seed = 300 + d
    ex = M.full_row_export(oracle, metric, d, 1500, seed)
    queries = unit_rows(np.random.default_rng(seed + 7), M.N_QUERIES, d)
    g = M.Graph(*ex)
    o = M.load_oracle(oracle, metric, d, ex)
    ix = _index(vamana, metric, d, ex)
    reps, _, _ = M.run_model(oracle, g, metric, queries, 10, 40)
    _oracle_equals_replay(o, reps, queries, 10, 40)
    for mode in (2, 1):
        ans, discarded, contradicted, in_use = _walk(ix, queries, 10, 40, mode)
        assert not in_use and discarded == 0 and contradicted == 0
        _equals_replay(ans, reps, "%s d=%d" % (metric, d))
    ix.close()


@pytest.mark.parametrize("metric", M.METRICS)
@pytest.mark.parametrize("d", [128, 512])
def test_search_sizes_limits_and_hostile_queries(oracle, metric, d):
    """one graph per width and metric: L = 1, 2 (the tail is the head), L < limit, the last L with the hash set (96), the
    L beyond it, and queries that break or strain the float16 copy of the query"""
    from semadb_amd import vamana
    from semadb_amd._lib import SemaDBError
    ex, queries = M.l_case(oracle, metric, d)
    g = M.Graph(*ex)
    o = M.load_oracle(oracle, metric, d, ex)
    ix = _index(vamana, metric, d, ex)
    for L, limit in M.L_CASES:
        what = "%s d=%d L=%d limit=%d" % (metric, d, L, limit)
        if L < limit:  # search.go:23-25: refused by both, and nothing walked
            with pytest.raises(ValueError):
                o.search(queries[0], limit, L)
            before = ix.sketch_stats()[:2]
            with pytest.raises(SemaDBError):
                ix.search_batch(queries, limit, L)
            assert ix.sketch_stats()[:2] == before
            continue
        _sandwich(ix, oracle, o, g, metric, queries, limit, L, what, expect="some")
    for L in M.L_BEYOND:
        # Present routing: searchSize > 96 leaves the hash set (csrc/walk_plan.h) and with it the kernel that
        # has the stage, so nothing is discarded.  Should a later change let the stage run there, the sandwich applies.
        what = "%s d=%d L=%d" % (metric, d, L)
        reps, t, _ = M.run_model(oracle, g, metric, queries, 10, L)
        _oracle_equals_replay(o, reps, queries, 10, L)
        for mode in (2, 1):
            ans, discarded, contradicted, _ = _walk(ix, queries, 10, L, mode)
            _equals_replay(ans, reps, what)
            assert contradicted == 0
            assert discarded == 0 or t.lower <= discarded <= t.upper, \
                "%s: discarded %d is neither 0 (the stage does not run there today) nor within %d .. %d" % (what, discarded, t.lower, t.upper)
            assert discarded == 0, "%s: the stage ran (%d discarded, inside the sandwich): state the new routing here" % (what, discarded)
    for kind in M.HOSTILE_NO_DISCARD:
        _sandwich(ix, oracle, o, g, metric, M.hostile_queries(d, kind), 10, 40, "%s d=%d %s" % (metric, d, kind), expect="none")
    for kind in M.HOSTILE_SANDWICH:
        _sandwich(ix, oracle, o, g, metric, M.hostile_queries(d, kind), 10, 40, "%s d=%d %s" % (metric, d, kind))
    ix.close()


@pytest.mark.parametrize("metric", M.METRICS)
def test_start_node_with_an_overflow_list(oracle, metric):
    """L = 1 and 2 with a start node of more than 64 + 64 edges: the array is full from the first chunk on, and the tail
    moves between the chunks of one expansion"""
    from semadb_amd import vamana
    ex, queries = M.overflow_case(oracle, metric)
    g = M.Graph(*ex)
    assert g.deg[g.start] > 64 + 64
    o = M.load_oracle(oracle, metric, 128, ex)
    ix = _index(vamana, metric, 128, ex)
    for L in (1, 2):
        _sandwich(ix, oracle, o, g, metric, queries, 1, L, "%s overflow list L=%d" % (metric, L), expect="some")
    ix.close()


@pytest.mark.parametrize("d", [128, 512])
def test_default_dispatch(oracle, d):
    """wide_walk at its default: batches of 256, 257, 512, 513 queries that share their first 256.  Per-query answers
    are the same in the four calls; the calls the many-waves kernel keeps discard nothing, the others are inside the
    sandwich."""
    from semadb_amd import vamana
    ex, queries = M.dispatch_case(oracle, d)
    g = M.Graph(*ex)
    o = M.load_oracle(oracle, "cosine", d, ex)
    ix = _index(vamana, "cosine", d, ex, wide_walk=None)
    reps, _, D = M.run_model(oracle, g, "cosine", queries, 10, 40)
    _oracle_equals_replay(o, reps[:32], queries[:32], 10, 40)
    m = M.Model(g, "cosine")
    for mode in (2, 1):
        ix.set_tuning("sketch", mode)
        for nq in (256, 257, 512, 513):
            what = "d=%d %d queries sketch=%d" % (d, nq, mode)
            ans, discarded, contradicted, in_use = _walk(ix, queries[:nq], 10, 40, None)
            assert in_use and contradicted == 0, what
            _equals_replay(ans, reps[:nq], what)
            if nq <= WIDE_UP_TO[d]:
                assert discarded == 0, "%s: %d discarded by a call the many-waves kernel keeps" % (what, discarded)
                continue
            t = M.Tally()
            for i in range(nq):
                t.add(m.count(queries[i], D[i], reps[i]))
            M.check_tally(t, what)
            msg = "%s: lower %d / discarded on the device %d / upper %d" % (what, t.lower, discarded, t.upper)
            print(msg)
            assert t.lower > 0 and t.lower <= discarded <= t.upper, msg
    ix.close()


def _scaled(rng, n, d, norm):
    return (unit_rows(rng, n, d) * np.float32(norm)).astype(np.float32)


def _half_error_rows(rng, d):
    """rows whose float16 copy is far from them: every element just above 2^-14 (where a half has 10 bits left), and a
    few near the largest half, 65 504, where neighbouring halves are 32 apart"""
    r = np.full((2, d), 6.2e-5, dtype=np.float32) * rng.choice(np.array([-1, 1], dtype=np.float32), size=(2, d))
    r[0, :4] = [60000.7, -65503.0, 33333.3, 65519.0]
    r[1, 5] = 47000.9
    return r


@pytest.mark.parametrize("metric", ["cosine", "euclidean"])
def test_maxima_through_every_write_path(oracle, metric):
    """The table-wide maxima max ||y - y16|| and max ||y16|| are carried from commit to commit (index_sketch.hip build_sketch,
    `from` > 0) and restart only when every row is converted again (load, compact).  Rows that raise them, and small
    rows behind them (whose own maxima would lower them, were the carry lost), arrive through every write path; after
    each commit the device's count is inside the sandwich of the model's maxima over all rows converted since the last
    full conversion, deleted ones included.  A twin index with the copy switched off receives the same writes: its
    answers are the float32 walk's."""
    from semadb_amd import vamana
    d, L, limit = 128, 40, 10
    ex, queries = M.l_case(oracle, metric, d)
    rng = np.random.default_rng(61)
    params = vamana.IndexVectorVamanaParameters(d, metric, M.L_BUILD, M.R_FULL, 1.2)

    def make(sketch):
        ix = vamana.NewIndexVamana("t", params, capacity=2048, strict=False)
        ix.set_tuning("wide_walk", 1)
        ix.set_tuning("sketch", sketch)
        ix.load(*ex)
        return ix

    ix, twin = make(1), make(0)
    state = {"maxima": M.maxima(ex[1]), "next": 5000}

    def new_ids(k):
        first = state["next"]
        state["next"] += k
        return np.arange(first, first + k, dtype=np.uint64)

    def check(what, expect=None):
        cur = ix.export()
        g = M.Graph(*cur)
        o = M.load_oracle(oracle, metric, d, cur)
        _sandwich(ix, oracle, o, g, metric, queries, limit, L, "%s after %s" % (metric, what), state["maxima"], expect)
        ix.set_tuning("sketch", 1)
        got = ix.search_batch(queries, limit, L, trace=True, visit_cap=1024)
        ref = twin.search_batch(queries, limit, L, trace=True, visit_cap=1024)
        assert not twin.sketch_stats()[2]
        for a, b in ((got[0], ref[0]), (bits(got[1]), bits(ref[1])), (got[2], ref[2]), (got[3].n_dist, ref[3].n_dist),
                     (got[3].n_hop, ref[3].n_hop), (got[3].n_edges, ref[3].n_edges)):
            assert np.array_equal(a, b), "%s: differs from the float32 walk" % what
        for i in range(queries.shape[0]):  # (a visit log is defined up to its walk's n_hop)
            k = int(ref[3].n_hop[i])
            assert np.array_equal(got[3].visit_ids[i, :k], ref[3].visit_ids[i, :k]), "%s query %d: visit order differs from the float32 walk's" % (what, i)

    def appended(rows):
        state["maxima"] = M.join_maxima(state["maxima"], M.maxima(rows))

    def rounds(rows):
        ids = new_ids(len(rows))
        for t in (ix, twin):
            t.insert_batch(ids, rows)
        appended(rows)
        return ids

    def one_point(rows):
        ids = new_ids(1)
        for t in (ix, twin):
            t.insert_batch(ids, rows[:1], round_size=1)
        appended(rows[:1])
        return ids

    def insert_and_update(rows):  # rows[:-1] inserted, rows[-1] replaces a stored point (delete + insert: appended too)
        ids = new_ids(len(rows) - 1)
        target = state.setdefault("update", 100)
        state["update"] += 1
        changes = [vamana.IndexVectorChange(int(i), rows[k].tolist()) for k, i in enumerate(ids)]
        changes.append(vamana.IndexVectorChange(target, rows[-1].tolist()))
        for t in (ix, twin):
            t.InsertUpdateDelete(changes)
        appended(rows)
        return ids

    def explicit(rows):
        ids = new_ids(len(rows))
        for t in (ix, twin):
            t.begin_write()
            t.insert_batch(ids, rows)
            assert not t.sketch_stats()[2]
            t.commit()
        appended(rows)
        return ids

    check("load", expect="some")
    for what, path, rows in (
            ("insert_batch, rows of norm 2", rounds, _scaled(rng, 6, d, 2.0)),
            ("insert_batch, rows of norm 1e-3", rounds, _scaled(rng, 6, d, 1e-3)),
            ("a one-point commit, norm 4", one_point, _scaled(rng, 1, d, 4.0)),
            ("a one-point commit, norm 1e-3", one_point, _scaled(rng, 1, d, 1e-3)),
            ("InsertUpdateDelete, inserts of norm 8, update of norm 1e-3", insert_and_update,
             np.vstack([_scaled(rng, 2, d, 8.0), _scaled(rng, 1, d, 1e-3)])),
            ("InsertUpdateDelete, insert of norm 1e-3, update of norm 16", insert_and_update,
             np.vstack([_scaled(rng, 1, d, 1e-3), _scaled(rng, 1, d, 16.0)])),
            ("begin_write .. commit, norm 32", explicit, _scaled(rng, 4, d, 32.0))):
        path(rows)
        check(what, expect="some")
    before = ix.SizeInMemory()
    explicit(_scaled(rng, 80, d, 1e-3))  # 2 001 + 17 + 80 rows: past the 2 048 the table was created with
    assert ix.SizeInMemory() > 1.5 * before, "the table did not grow"
    check("begin_write .. commit that grows the table, norm 1e-3", expect="some")
    hostile = [int(v) for v in rounds(_half_error_rows(rng, d))]
    check("insert_batch, rows with a large float16 error")
    row = unit_rows(rng, 1, d)
    row[0, 17] = 1e6
    hostile += [int(v) for v in one_point(row)]
    check("a row with an element of 1e6", expect="none")
    row = unit_rows(rng, 2, d)
    row[0, 3] = np.nan
    hostile += [int(v) for v in insert_and_update(row)[:1]]
    check("a NaN row", expect="none")
    # the hostile rows deleted: the maxima still count them (upper bounds stay upper bounds) ...
    for t in (ix, twin):
        t.delete_batch(np.array(hostile, dtype=np.uint64))
    check("the hostile rows deleted", expect="none")
    # ... until every row is converted again: the maxima of the rows that remain
    for t in (ix, twin):
        t.compact()
    state["maxima"] = M.maxima(ix.export()[1])
    check("compact", expect="some")
    ix.close()
    twin.close()
