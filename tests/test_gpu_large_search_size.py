"""The walks above searchSize 96 and the quantizer tables of 2 049 .. 16 384 entries, against the oracle bit for bit.

Past searchSize 96 every search runs k_greedy_search<Dist, NREG, FILT, 0>: the query's HBM bitset as the visited set, a
candidate array of two registers per lane (128 entries) at 97 .. 128 and of eight (512 entries) at 129 .. 512, for every
distance policy, plain and filtered.  A product quantizer of 2 049 .. 16 384 table entries takes that kernel at every
searchSize, its table in up to 64 KB of dynamic LDS.  The cases (tests/large_search_model.py; that they fill, overfill,
tie across or never fill the array is proved without a GPU by tests/test_large_search_model.py):

  A  d = 32, 10 000 rows, three metrics: searchSize on and beside every register boundary, limit 1 .. searchSize;
     300 rows at searchSize 512 (the array never fills) and at limit = searchSize = 97 .. 200 (rows one short)
  B  an integer grid with ties across every register boundary, plain and filtered; non-finite queries
  C  six filter kinds at seven (searchSize, limit) pairs, resolved on the device, on the host and given as bitmaps
  D  thirteen row widths, one per kernel shape, plain and filtered
  E  one index through searchSize 512 / 512 filtered / 128 / 97 filtered / 512 / 50 / 129; 513 queries in one call; a
     start node with an overflow list
  F  five quantizer shapes from 128 to 18 432 table entries at searchSize 50 .. 512, and under the visited-set knobs

Every comparison: ids, distance bits, counts, n_hop, n_dist, n_edges, the visit order; and every output row is zero
behind its count.  That the KERNEL writes those zeros shows only where it writes into the caller's memory: a traced call
on host arrays is staged, and the library clears the staged rows ahead of the launch.  So the small table, the
limit = searchSize rows and the six filter kinds at all seven (searchSize, limit) pairs also run on device tensors that
hold a sentinel (_search(device=True)): both epilogues (search set, result set) at both array sizes.  wide_walk is left
at 0: above 96 the workgroup walk never takes the call.

Shown to bite on scratch builds (none kept; profiles/r12_large_search_mutants.txt): list_tail() reading one entry early
above 128 fails 55 of the then 109 cases -- the small tables and the ties rather than the sweep, where a point dropped
between the last two entries is nearly always pushed out again before the walk ends --, a result copy whose rank stops
advancing after the second register fails 90, and a zero fill that starts 64 entries late fails the twelve device-tensor
cases and no other.  Observed on an MI355X (profiles/r12_large_search_size.log): all 120 pass on the unchanged library,
the quantizer of 64 x 256 entries (64 KB of dynamic LDS beside the kernel's static 1 KB / 4 KB) included: that launch is
accepted as it is.
"""
import numpy as np
import pytest

from tests import large_search_model as LM
from tests import visited_spill_model as S
from tests.helpers import bits
from tests.test_gpu_nonfinite import same_bits_or_both_nan

pytestmark = pytest.mark.gpu

VISIT_CAP = 2048
SENTINEL_ID, SENTINEL_D, SENTINEL_C = 0xDEADBEEF, np.float32(-7.0), 99


def _load(t, R=32, L=50):
    from semadb_amd import vamana
    ix = vamana.NewIndexVamana("large", vamana.IndexVectorVamanaParameters(t.d, t.metric, L, R, 1.2), strict=False)
    ix.load(*t.ex)
    return ix


@pytest.fixture(scope="module")
def indexes(oracle):
    """device indexes over the model's tables, loaded once per module"""
    held = {}

    def get(key, make):
        if key not in held:
            held[key] = make()
        return held[key]

    yield get
    for v in held.values():
        for x in (v if isinstance(v, tuple) else (v,)):
            x.close()


def _search(ix, queries, limit, L, filters=None, device=False):
    """one traced call.  Host arrays (the default): the library stages the call and clears its staged output rows ahead
    of the launch, so what comes back behind a count is zero whatever the kernel does.  device: queries, outputs and
    trace are device tensors and the kernel writes straight into the caller's memory, which holds a sentinel -- what the
    kernel did not write shows.  Returns numpy arrays either way."""
    if not device:
        return ix.search_batch(queries, limit, L, filters=filters, trace=True, visit_cap=VISIT_CAP)
    import torch
    nq = queries.shape[0]
    out = (torch.full((nq, limit), SENTINEL_ID, dtype=torch.int64, device="cuda"),
           torch.full((nq, limit), float(SENTINEL_D), dtype=torch.float32, device="cuda"),
           torch.full((nq,), SENTINEL_C, dtype=torch.int32, device="cuda"))
    ids, d, c, tr = ix.search_batch(torch.from_numpy(np.ascontiguousarray(queries)).cuda(), limit, L, filters=filters,
                                    trace=True, visit_cap=VISIT_CAP, out=out)
    torch.cuda.synchronize()
    assert ids.data_ptr() == out[0].data_ptr() and d.data_ptr() == out[1].data_ptr() and c.data_ptr() == out[2].data_ptr()
    tr.n_dist, tr.n_hop, tr.n_edges = (x.cpu().numpy().astype(np.uint32) for x in (tr.n_dist, tr.n_hop, tr.n_edges))
    tr.visit_ids = tr.visit_ids.cpu().numpy().view(np.uint64)
    return ids.cpu().numpy().view(np.uint64), d.cpu().numpy(), c.cpu().numpy().astype(np.uint32), tr


def _check(what, ix, o, queries, limit, L, filters=None, picked=None, nonfinite=False, device=False):
    """the device's answers against the oracle's, everything the trace shows; returns the answers and prints the case's
    n_dist range"""
    g_ids, g_d, g_c, tr = ans = _search(ix, queries, limit, L, filters, device)
    lo, hi = 1 << 62, 0
    for q in (range(queries.shape[0]) if picked is None else picked):
        o_ids, o_d, o_vis, o_tr = o.search(queries[q], limit, L, filter_ids=None if filters is None else sorted(filters[q]))
        k = len(o_ids)
        w = "%s query %d" % (what, q)
        assert int(g_c[q]) == k, "%s: count %d, oracle %d" % (w, int(g_c[q]), k)
        assert np.array_equal(g_ids[q, :k], o_ids), "%s: ids" % w
        if nonfinite:
            assert same_bits_or_both_nan(g_d[q, :k], o_d), "%s: distances" % w
        else:
            assert np.array_equal(bits(g_d[q, :k]), bits(o_d)), "%s: distance bits" % w
        assert not g_ids[q, k:].any() and not bits(g_d[q, k:]).any(), "%s: the row behind its count is not zero" % w
        assert (int(tr.n_hop[q]), int(tr.n_dist[q]), int(tr.n_edges[q])) == (o_tr.n_hop, o_tr.n_dist, o_tr.n_edges), \
            "%s: n_hop / n_dist / n_edges %r, oracle %r" % (w, (int(tr.n_hop[q]), int(tr.n_dist[q]), int(tr.n_edges[q])),
                                                          (o_tr.n_hop, o_tr.n_dist, o_tr.n_edges))
        assert o_tr.n_hop <= VISIT_CAP
        same = np.array_equal(tr.visit_ids[q, :o_tr.n_hop], o_vis)
        assert same, "%s: visit order, first differing hop %d" % (w, int(np.argmax(tr.visit_ids[q, :o_tr.n_hop] != o_vis)))
        lo, hi = min(lo, o_tr.n_dist), max(hi, o_tr.n_dist)
    print("ok %s: n_dist %d .. %d" % (what, lo, hi))
    return ans


def _identical(a, b, what):
    """two calls: ids, distance bits, counts, counters, and the visit logs up to n_hop (behind n_hop a log row holds what
    the call's staging memory held before)"""
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[2], b[2]), "%s: ids / counts" % what
    assert np.array_equal(bits(a[1]), bits(b[1])), "%s: distance bits" % what
    for f in ("n_dist", "n_hop", "n_edges"):
        assert np.array_equal(getattr(a[3], f), getattr(b[3], f)), "%s: %s" % (what, f)
    for q in range(a[0].shape[0]):
        k = int(b[3].n_hop[q])
        assert np.array_equal(a[3].visit_ids[q, :k], b[3].visit_ids[q, :k]), "%s query %d: visit order" % (what, q)


# ---------------------------------------------------------------------------------------------- A
@pytest.mark.parametrize("L", LM.A_L)
@pytest.mark.parametrize("metric", LM.A_METRICS)
def test_candidate_array_sweep(oracle, indexes, metric, L):
    t = LM.a_table(oracle, metric)
    ix = indexes(("a", metric), lambda: _load(t))
    for limit in LM.limits_of(L):
        _check("A %s L=%d limit=%d" % (metric, L, limit), ix, t.o, t.queries, limit, L)


def test_a_table_smaller_than_the_array(oracle):
    """300 rows at searchSize 512, limit 512, into device tensors that hold a sentinel: every row comes back but the
    start node, and the kernel writes 212 zeros behind them"""
    t = LM.small_table(oracle)
    ix = _load(t)
    ids, d, c, _ = _check("A n=%d L=512 limit=512, device tensors" % t.n, ix, t.o, t.queries, 512, 512, device=True)
    assert (c == t.n).all()
    assert not ids[:, t.n:].any() and not bits(d[:, t.n:]).any()
    assert all(sorted(int(v) for v in row[:t.n]) == sorted(int(v) for v in t.ids) for row in ids)
    _check("A n=%d L=512 limit=512" % t.n, ix, t.o, t.queries, 512, 512)
    ix.close()


@pytest.mark.parametrize("L", LM.SHORT_ROW_L)
def test_plain_rows_are_zero_behind_their_count(oracle, L):
    """limit = searchSize on the small table, device tensors over a sentinel: a query whose final array holds the start
    node returns searchSize - 1 results and one zero behind them, written by the kernel (two array registers at 97 and
    128, eight at 129 and 200; that such queries exist: tests/test_large_search_model.py)"""
    t = LM.small_table(oracle)
    ix = _load(t)
    c = _check("A n=%d L=%d limit=%d, device tensors" % (t.n, L, L), ix, t.o, t.queries, L, L, device=True)[2]
    assert (c == L - 1).any()
    ix.close()


@pytest.mark.parametrize("L,limit", LM.FILTER_CASES)
def test_filtered_rows_are_zero_behind_their_count(oracle, indexes, L, limit):
    """the six filter kinds into device tensors over a sentinel: the "fewer than limit", "40 and unknown ids", "with the
    start id" and empty filters return short rows (the empty one nothing at all), filled with zeros by the result
    set's epilogue at both array sizes"""
    t = LM.a_table(oracle, "cosine")
    ix = indexes(("a", "cosine"), lambda: _load(t))
    filters = LM.filters_of(oracle, "cosine", L, limit)
    queries = np.vstack([t.queries, t.more_queries])[:LM.NQ_FILTERED]
    c = _check("C cosine L=%d limit=%d, device tensors" % (L, limit), ix, t.o, queries, limit, L, filters=filters, device=True)[2]
    assert (c[5::6] == 0).all() and (c[0::6] < limit).all() and (c[0::6] > 0).all()


# ---------------------------------------------------------------------------------------------- B
@pytest.mark.parametrize("L", LM.TIE_L)
@pytest.mark.parametrize("filtered", [False, True])
def test_ties_across_the_registers(oracle, indexes, filtered, L):
    t = LM.tie_table(oracle)
    ix = indexes("ties", lambda: _load(t))
    for limit in (L, 65):
        _check("B ties%s L=%d limit=%d" % (" filtered" if filtered else "", L, limit), ix, t.o, t.queries, limit, L,
               filters=t.filters if filtered else None)


@pytest.mark.parametrize("L", LM.NONFINITE_L)
def test_non_finite_queries(oracle, indexes, L):
    t = LM.a_table(oracle, "cosine")
    ix = indexes(("a", "cosine"), lambda: _load(t))
    qn = LM.nonfinite_queries(t.queries)
    with np.errstate(all="ignore"):
        for limit in (10, L):
            _check("B non-finite L=%d limit=%d" % (L, limit), ix, t.o, qn, limit, L, nonfinite=True)


# ---------------------------------------------------------------------------------------------- C
@pytest.mark.parametrize("L,limit", LM.FILTER_CASES)
@pytest.mark.parametrize("metric", LM.FILTER_METRICS)
def test_filtered_large_array(oracle, indexes, metric, L, limit):
    """(a filtered call takes no first stage unless sketch_filtered asks for one: at 97 and 128 this is the two-register
    bitset kernel, at 129 and beyond the eight-register one)"""
    from semadb_amd import vamana
    t = LM.a_table(oracle, metric)
    ix = indexes(("a", metric), lambda: _load(t))
    filters = LM.filters_of(oracle, metric, L, limit)
    queries = np.vstack([t.queries, t.more_queries])[:LM.NQ_FILTERED]
    what = "C %s L=%d limit=%d" % (metric, L, limit)
    ref = _check(what + " ids resolved on the device", ix, t.o, queries, limit, L, filters=filters)
    ix.set_tuning("host_filters", 1)
    try:
        _identical(_search(ix, queries, limit, L, filters), ref, what + " host_filters")
    finally:
        ix.set_tuning("host_filters", 0)
    _identical(_search(ix, queries, limit, L, vamana.FilterBitmaps.from_sets(filters)), ref, what + " bitmaps")


# ---------------------------------------------------------------------------------------------- D
@pytest.mark.parametrize("d", LM.WIDTHS)
@pytest.mark.parametrize("metric", LM.WIDTH_METRICS)
def test_every_row_width(oracle, metric, d):
    t = LM.width_table(oracle, metric, d)
    ix = _load(t)
    for L in LM.WIDTH_L:
        _check("D %s d=%d L=%d" % (metric, d, L), ix, t.o, t.queries, 10, L)
    _check("D %s d=%d filtered (129, 129)" % (metric, d), ix, t.o, t.queries, 129, 129, filters=t.filters)
    ix.close()


# ---------------------------------------------------------------------------------------------- E
def test_bitsets_are_reused_across_batches(oracle):
    """an index of its own: the workspaces are this test's alone from the first call on"""
    t = LM.a_table(oracle, "euclidean")
    ix = _load(t)
    filters = LM.make_filters(np.random.default_rng(9900), t.ids, LM.NQ, 97, 10)
    half = [set(int(v) for v in np.random.default_rng(9901 + i).choice(t.ids, size=t.n // 2, replace=False)) for i in range(LM.NQ)]
    answers = []
    for step, (which, L, filtered) in enumerate(LM.REUSE_STEPS):
        q = t.queries if which == 1 else t.more_queries
        f = None if not filtered else half if L == 512 else filters
        answers.append(_check("E step %d L=%d%s" % (step + 1, L, " filtered" if filtered else ""), ix, t.o, q, 10, L, filters=f))
    _identical(answers[0], answers[4], "E the first and the fifth batch")
    ix.close()


def test_many_queries_in_one_call(oracle, indexes):
    t = LM.a_table(oracle, "euclidean")
    ix = indexes(("a", "euclidean"), lambda: _load(t))
    q = LM.many_queries()
    a = _check("E %d queries L=%d" % (LM.MANY, LM.MANY_L), ix, t.o, q, 10, LM.MANY_L, picked=LM.many_checked())
    b = _search(ix, q, 10, LM.MANY_L)
    _identical(a, b, "E %d queries, the call repeated" % LM.MANY)


def test_overflow_list_into_the_large_array(oracle):
    from semadb_amd import vamana
    from tests.test_gpu_two_precision_bound import _index
    case = S.overflow_case(oracle, LM.OVERFLOW_L, 10)
    ix = _index(vamana, "cosine", 128, case.ex, wide_walk=None)
    for limit in (10, LM.OVERFLOW_L):
        _check("E overflow list L=%d limit=%d" % (LM.OVERFLOW_L, limit), ix, case.o, case.queries, limit, LM.OVERFLOW_L)
    ix.close()


# ---------------------------------------------------------------------------------------------- F
@pytest.mark.parametrize("d,M,K", LM.PQ_SHAPES)
@pytest.mark.parametrize("metric", LM.PQ_METRICS)
def test_quantized_store(oracle, metric, d, M, K):
    from semadb_amd import vectorstore as vs
    t = LM.pq_table(oracle, metric, d, M, K)
    ix = _load(t)
    gpq = vs.ProductQuantizer(metric, vs.ProductQuantizerParameters(K, M), d)
    gpq.Fit(t.train.copy(), t.first, alias=True)
    vs.attach(ix, gpq)
    what = "F %s M=%d K=%d (%s / %s)" % (metric, M, K, LM.pq_route(M, K, 50), LM.pq_route(M, K, 97))
    try:
        first = _check(what + " L=50", ix, t.o, t.queries, 10, 50)
        _check(what + " L=50 filtered", ix, t.o, t.queries, 10, 50, filters=t.filters40)
        for L in LM.PQ_L:
            _check(what + " L=%d" % L, ix, t.o, t.queries, 10, L)
        _check(what + " filtered (129, 129)", ix, t.o, t.queries, 129, 129, filters=t.filters_half)
        _identical(_search(ix, t.queries, 10, 50), first, what + " L=50 again")
        if (M, K) in ((32, 256), (64, 256)):  # the 32 KB and the 64 KB table
            for knob in ("wide_hash", "no_hash"):
                ix.set_tuning(knob, 1)
                got = _search(ix, t.queries, 10, 50)
                ix.set_tuning(knob, 0)
                _identical(got, first, what + " L=50 " + knob)
    finally:
        ix.close()
        gpq.close()
