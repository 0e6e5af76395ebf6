"""Re-ranked search (sdb_index_search_batch_rerank / _bitmap_rerank, IndexVamana.search_batch(rerank=)) on the device
against tests/rerank_model.py: ids, the EXACT distances' bits, counts and the zeroed unused entries of every query, and
the trace against the un-re-ranked call's (limit = rerank: the walk the definition names).  The tables and queries are
the ones tests/test_rerank_model.py states the model's conditions on."""
import numpy as np
import pytest

from tests import rerank_model as rm
from tests.helpers import assert_same_graph, bits, unit_rows

pytestmark = pytest.mark.gpu

VC = 1024  # visit ids kept per query (searchSize 512 makes 512+ hops; the comparison is device against device)


def same_bits_or_both_nan(a, b):
    from tests.test_gpu_nonfinite import same_bits_or_both_nan as f  # (a NaN's payload is the one thing the machines do not share)
    return f(a, b)


def assert_same_trace(a, b):
    """counters and the visit order (entries past a query's n_hop are not part of the trace: nobody writes them)"""
    for name in ("n_dist", "n_hop", "n_edges"):
        assert np.array_equal(getattr(a, name), getattr(b, name)), name
    for k, h in enumerate(np.asarray(a.n_hop)):
        assert np.array_equal(a.visit_ids[k, :min(int(h), VC)], b.visit_ids[k, :min(int(h), VC)]), k


def _gpu_index(fx, L=rm.L):
    """the fixture's graph in HBM, its quantizer attached: (index, quantizer or None)"""
    from semadb_amd import vamana, vectorstore as vs
    ix = vamana.NewIndexVamana("rr", vamana.IndexVectorVamanaParameters(fx.d, fx.metric, L, rm.R, 1.2), strict=False)
    ix.load(fx.ids, fx.vecs, fx.off, fx.edges)
    quant = None
    if fx.kind == "pq":
        quant = vs.ProductQuantizer(fx.metric, vs.ProductQuantizerParameters(fx.K, fx.M), fx.d)
        quant.Fit(fx.train.copy(), fx.first, alias=True)
        vs.attach(ix, quant)
    elif fx.kind in ("hamming", "jaccard"):
        quant = vs.BinaryQuantizer(vs.BinaryQuantizerParameters(None, 0, fx.kind), fx.d)
        vs.attach_binary(ix, quant)  # fitted from the rows, start node included
        assert np.array_equal(bits(quant.threshold()), bits(fx.thr))
        assert np.array_equal(vs.get_bit_codes(ix, fx.ids), fx.codes)
    return ix, quant


_OPEN = {}


@pytest.fixture(scope="module", autouse=True)
def _close_indexes():
    yield
    for ix, quant in _OPEN.values():
        ix.close()
        if quant is not None:
            quant.close()
    _OPEN.clear()


def shared_index(key, fx):
    if key not in _OPEN:
        _OPEN[key] = _gpu_index(fx)
    return _OPEN[key][0]


def check(oracle, fx, ix, q, limit, L, r, filters=None, bitmap=False, nonfinite=False, ids=None, vecs=None, **kw):
    """one re-ranked batch against the model; returns the device's (ids, dists, counts)"""
    from semadb_amd import vamana
    f = filters
    if filters is not None and bitmap:
        f = vamana.FilterBitmaps.from_sets(filters)
    ids = fx.ids if ids is None else ids
    vecs = fx.vecs if vecs is None else vecs
    with np.errstate(all="ignore"):
        w_ids, w_d, w_c, w_tr = ix.search_batch(q, r, L, filters=f, trace=True, visit_cap=VC, **kw)
        g_ids, g_d, g_c, g_tr = ix.search_batch(q, limit, L, filters=f, trace=True, visit_cap=VC, rerank=r, **kw)
    assert g_ids.shape == (q.shape[0], limit) and g_d.shape == (q.shape[0], limit)
    assert_same_trace(g_tr, w_tr)  # the walk's trace, untouched
    for k in range(q.shape[0]):
        with np.errstate(all="ignore"):
            m_ids, m_e, walk = rm.rerank(oracle, fx.o, ids, vecs, fx.metric, q[k], limit, L, r,
                                         None if filters is None else sorted(filters[k]))
        cn, m = len(walk[0]), len(m_ids)
        assert int(w_c[k]) == cn and np.array_equal(w_ids[k, :cn], walk[0]), (k, r)  # the candidates are the walk's
        assert int(g_c[k]) == m == min(limit, cn), (k, r)
        assert np.array_equal(g_ids[k, :m], m_ids), (k, r, g_ids[k], m_ids)
        if nonfinite:
            assert same_bits_or_both_nan(g_d[k, :m], m_e), (k, r)
        else:
            assert np.array_equal(bits(g_d[k, :m]), bits(m_e)), (k, r, g_d[k], m_e)
        assert not g_ids[k, m:].any() and not bits(g_d[k, m:]).any(), (k, r)  # unused entries: 0 / +0.0f
    return g_ids, g_d, g_c


# ---- product quantizer -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("metric", rm.METRICS)
@pytest.mark.parametrize("d,M,K,n", rm.PQ_SHAPES)
def test_product_quantizer(oracle, metric, d, M, K, n):
    fx = rm.pq_fixture(metric, d, M, K, n)
    ix = shared_index(("pq", metric, d, M, K, n), fx)
    ref = {r: check(oracle, fx, ix, fx.q, rm.LIMIT, rm.L, r) for r in rm.RERANKS}
    for key in ("pq_narrow", "wide_hash"):  # the one-wave kernel, the other visited set: same answers
        ix.set_tuning(key, 1)
        try:
            for r in rm.RERANKS:
                got = check(oracle, fx, ix, fx.q, rm.LIMIT, rm.L, r)
                assert np.array_equal(got[0], ref[r][0]) and np.array_equal(bits(got[1]), bits(ref[r][1])), (key, r)
        finally:
            ix.set_tuning(key, 0)


@pytest.mark.parametrize("metric", rm.METRICS)
@pytest.mark.parametrize("d,M,K,n", rm.PQ_TABLE)
def test_product_quantizer_nonfinite_queries(oracle, metric, d, M, K, n):
    """the NaN / Inf / overflow queries of tests/test_gpu_pq.py::test_pq_search_parity: NaNs last, in the walk's order"""
    fx = rm.pq_fixture(metric, d, M, K, n)
    ix = shared_index(("pq", metric, d, M, K, n), fx)
    qn = fx.q[:8].copy()
    qn[0, 3] = np.nan
    qn[1, :] = np.float32(3e38)
    qn[2, ::2] = np.float32(-3e38)
    qn[3, 0] = np.inf
    qn[4, : d // 2] = np.float32(2e38)
    for r in (10, 25):
        check(oracle, fx, ix, qn, rm.LIMIT, rm.L, r, nonfinite=True)


# ---- binary quantizer --------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind,d", rm.BQ_CASES)
def test_binary_quantizer(oracle, kind, d):
    fx = rm.bq_fixture(kind, d)
    ix = shared_index((kind, d), fx)
    for r in rm.RERANKS:
        check(oracle, fx, ix, fx.q, rm.LIMIT, rm.L, r)
    if kind == "hamming":  # many equal code distances: the walk's order among ties is part of the answer
        walk = fx.o.search(fx.q[0], 50, rm.L)[1]
        assert len(np.unique(walk)) < len(walk)


# ---- no quantizer: the plain search --------------------------------------------------------------------------------

@pytest.mark.parametrize("d", [100, 384])
@pytest.mark.parametrize("sketch", [0, 1, 3])
def test_plain_store_is_the_plain_search(oracle, d, sketch):
    fx = rm.plain_fixture("cosine", d)
    ix = shared_index(("plain", "cosine", d), fx)
    ix.set_tuning("sketch", sketch)
    try:
        for nq in (1, 256, 257, 513):  # every dispatch of the walk
            q = fx.q[:nq]
            want = ix.search_batch(q, rm.LIMIT, rm.L, trace=True, visit_cap=VC)
            for r in (10, 50):
                got = ix.search_batch(q, rm.LIMIT, rm.L, trace=True, visit_cap=VC, rerank=r)
                assert np.array_equal(got[0], want[0]) and np.array_equal(bits(got[1]), bits(want[1])), (nq, r)
                assert np.array_equal(got[2], want[2]), (nq, r)
                assert_same_trace(got[3], want[3])
        check(oracle, fx, ix, fx.q[:rm.NQ], rm.LIMIT, rm.L, 25)  # ... and the model's
    finally:
        ix.set_tuning("sketch", 3)


@pytest.mark.parametrize("metric", ["euclidean", "dot"])
def test_plain_store_other_metrics(oracle, metric):
    fx = rm.plain_fixture(metric, 100)
    ix = shared_index(("plain", metric, 100), fx)
    for r in rm.RERANKS:
        got = check(oracle, fx, ix, fx.q[:rm.NQ], rm.LIMIT, rm.L, r)
        want = ix.search_batch(fx.q[:rm.NQ], rm.LIMIT, rm.L)
        assert np.array_equal(got[0], want[0]) and np.array_equal(bits(got[1]), bits(want[1]))


# ---- exact ties --------------------------------------------------------------------------------------------------

def test_duplicated_rows_keep_the_walk_order(oracle):
    fx = rm.dup_fixture()
    ix, quant = _gpu_index(fx)
    try:
        tied = 0
        for k in range(rm.NQ):
            c = fx.o.search(fx.q[k], 50, rm.L)[0]
            e = oracle.distance_matrix(fx.q[k][None, :], rm.rows_of(fx.ids, fx.vecs, c), fx.metric)[0]
            tied += len(e) - len(np.unique(bits(e)))
        assert tied >= 40, tied  # exact distances that tie bit for bit among one query's candidates
        for r in rm.RERANKS:
            check(oracle, fx, ix, fx.q, rm.LIMIT, rm.L, r)
    finally:
        ix.close()
        quant.close()


# ---- boundaries --------------------------------------------------------------------------------------------------

def test_boundaries(oracle):
    from semadb_amd import SemaDBError
    fx = rm.pq_fixture("cosine", 32, 8, 16, 1500)
    ix = shared_index(("pq", "cosine", 32, 8, 16, 1500), fx)
    check(oracle, fx, ix, fx.q, 10, 50, 10)   # rerank == limit: the same ten, reordered
    check(oracle, fx, ix, fx.q, 10, 50, 50)   # rerank == search_size
    check(oracle, fx, ix, fx.q, 50, 50, 50)
    check(oracle, fx, ix, fx.q, 1, 1, 1)
    for ss in (96, 97, 128, 512):
        check(oracle, fx, ix, fx.q[:8], 10, ss, ss)
        check(oracle, fx, ix, fx.q[:8], ss, ss, ss)
    # a filter of 3 ids: count < limit
    filters = [set(int(v) for v in fx.rng.choice(fx.ids[1:], size=3, replace=False)) for _ in range(rm.NQ)]
    got = check(oracle, fx, ix, fx.q, 10, 50, 25, filters=filters)
    assert (got[2] == 3).all()
    check(oracle, fx, ix, fx.q, 10, 50, 25, filters=filters, bitmap=True)
    # invalid arguments: an error, and the output buffers as they were
    for limit, ss, r in ((10, 50, 9), (10, 50, 51), (10, 50, 0), (10, 600, 600)):
        out = (np.full((rm.NQ, limit), 77, np.uint64), np.full((rm.NQ, limit), 7.5, np.float32), np.full(rm.NQ, 7, np.uint32))
        with pytest.raises(SemaDBError):
            ix.search_batch(fx.q, limit, ss, rerank=r, out=out)
        assert (out[0] == 77).all() and (out[1] == 7.5).all() and (out[2] == 7).all(), (limit, ss, r)
        with pytest.raises(SemaDBError):
            ix.search_batch(fx.q, limit, ss, rerank=r, out=out, filters=filters)
        assert (out[0] == 77).all() and (out[1] == 7.5).all() and (out[2] == 7).all(), (limit, ss, r)


def test_strict_mode_checks_apply():
    from semadb_amd import SemaDBError, vamana
    fx = rm.plain_fixture("cosine", 100)
    ix = vamana.NewIndexVamana("rr", vamana.IndexVectorVamanaParameters(fx.d, fx.metric, rm.L, rm.R, 1.2), strict=True)
    try:
        with pytest.raises(SemaDBError):  # no start point
            ix.search_batch(fx.q[:4], 10, 50, rerank=25)
        ix.load(fx.ids, fx.vecs, fx.off, fx.edges)
        with pytest.raises(SemaDBError):  # searchSize outside 25 .. 75
            ix.search_batch(fx.q[:4], 10, 100, rerank=25)
        with pytest.raises(SemaDBError):
            ix.search_batch(fx.q[:4], 10, 20, rerank=15)
        got = ix.search_batch(fx.q[:4], 10, 75, rerank=75)
        want = ix.search_batch(fx.q[:4], 10, 75)
        assert np.array_equal(got[0], want[0]) and np.array_equal(bits(got[1]), bits(want[1]))
    finally:
        ix.close()


def test_fewer_live_rows_than_rerank(oracle):
    fx = rm.small_fixture()
    ix, quant = _gpu_index(fx)
    try:
        got = check(oracle, fx, ix, fx.q, 10, 50, 50)  # 30 rows: every query returns them all
        assert (got[2] == 10).all()
        got = check(oracle, fx, ix, fx.q, 40, 50, 45)
        assert (got[2] == 30).all()
    finally:
        ix.close()
        quant.close()


# ---- filters -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("which", ["pq", "hamming"])
@pytest.mark.parametrize("bitmap", [False, True])
def test_filters(oracle, which, bitmap):
    if which == "pq":
        fx = rm.pq_fixture("cosine", 96, 8, 256, 1500)
        ix = shared_index(("pq", "cosine", 96, 8, 256, 1500), fx)
    else:
        fx = rm.bq_fixture("hamming", 100)
        ix = shared_index(("hamming", 100), fx)
    rng = np.random.default_rng(41)
    filters = [set(int(v) for v in rng.choice(fx.ids[1:], size=40, replace=False)) for _ in range(rm.NQ)]
    for limit, r in ((5, 5), (5, 20), (10, 40), (10, 50)):
        check(oracle, fx, ix, fx.q, limit, rm.L, r, filters=filters, bitmap=bitmap)
    if not bitmap:  # the ABI's own form: (offsets, ascending ids)
        flat = np.concatenate([np.array(sorted(f), np.uint64) for f in filters])
        off = np.arange(0, 40 * rm.NQ + 1, 40, dtype=np.uint64)
        a = ix.search_batch(fx.q, 10, rm.L, filters=(off, flat), rerank=40)
        b = ix.search_batch(fx.q, 10, rm.L, filters=filters, rerank=40)
        assert np.array_equal(a[0], b[0]) and np.array_equal(bits(a[1]), bits(b[1])) and np.array_equal(a[2], b[2])


# ---- views -------------------------------------------------------------------------------------------------------

def test_views_deletes_compaction_and_a_reused_id(oracle):
    fx = rm.pq_fixture.__wrapped__("cosine", 32, 8, 16, 1500)  # a copy of its own: this test changes the graph
    ix, quant = _gpu_index(fx)
    try:
        rng = np.random.default_rng(5)
        extra = unit_rows(rng, 20, fx.d)
        new_ids = np.arange(5000, 5020, dtype=np.uint64)
        # inside an open write transaction: the answers of the committed view
        ix.begin_write()
        ix.insert_batch(new_ids, extra, round_size=1)
        ix.delete_batch(fx.ids[5:15])
        for r in (10, 50):
            check(oracle, fx, ix, fx.q, rm.LIMIT, rm.L, r)
        assert ix.abort_write()
        check(oracle, fx, ix, fx.q, rm.LIMIT, rm.L, 25)
        # 50 ids deleted: the ids are no longer consecutive (the view's id -> slot table resolves the candidates)
        dead = rng.choice(fx.ids[1:], size=50, replace=False).astype(np.uint64)
        assert fx.o.delete(dead) == 0
        ix.delete_batch(dead)
        assert_same_graph(ix, fx.o)
        ids, vecs, _, _ = fx.o.export()
        filters = [set(int(v) for v in rng.choice(ids[1:], size=40, replace=False)) for _ in range(rm.NQ)]
        for r in rm.RERANKS:
            check(oracle, fx, ix, fx.q, rm.LIMIT, rm.L, r, ids=ids, vecs=vecs)
        check(oracle, fx, ix, fx.q, rm.LIMIT, rm.L, 40, ids=ids, vecs=vecs, filters=filters)
        ix.compact()
        for r in rm.RERANKS:
            check(oracle, fx, ix, fx.q, rm.LIMIT, rm.L, r, ids=ids, vecs=vecs)
        # an id deleted and inserted again: it sits behind larger ids, the subtraction would name another row
        back = dead[:5]
        for i, v in enumerate(back):
            assert fx.o.insert(int(v), extra[i]) == 0
        ix.insert_batch(back, extra[:5], round_size=1)
        assert_same_graph(ix, fx.o)
        ids, vecs, _, _ = fx.o.export()
        q = np.concatenate([fx.q[:27], extra[:5] + np.float32(0.01)]).astype(np.float32)  # queries next to the rows that came back
        filters = [set(int(v) for v in rng.choice(ids[1:], size=40, replace=False)) | set(int(v) for v in back) for _ in range(rm.NQ)]
        seen = 0
        for r in rm.RERANKS:
            got = check(oracle, fx, ix, q, rm.LIMIT, rm.L, r, ids=ids, vecs=vecs)
            seen += int(np.isin(got[0], back).sum())
            check(oracle, fx, ix, q, rm.LIMIT, rm.L, r, ids=ids, vecs=vecs, filters=filters)
            check(oracle, fx, ix, q, rm.LIMIT, rm.L, r, ids=ids, vecs=vecs, filters=filters, bitmap=True)
        assert seen > 0  # the rows behind the reused ids are among the answers
    finally:
        ix.close()
        quant.close()


# ---- memory kinds ------------------------------------------------------------------------------------------------

def test_memory_kinds_and_reused_scratch(oracle):
    import torch
    from semadb_amd import _buf
    fx = rm.pq_fixture("cosine", 32, 8, 16, 1500)
    ix = shared_index(("pq", "cosine", 32, 8, 16, 1500), fx)
    pfx = rm.plain_fixture("cosine", 100)
    pix = shared_index(("plain", "cosine", 100), pfx)
    for f, x, q in ((fx, ix, fx.q), (pfx, pix, pfx.q[:rm.NQ])):  # (a plain store's pinned buffers are read and written in place)
        nq = q.shape[0]
        want = {r: check(oracle, f, x, q, rm.LIMIT, rm.L, r) for r in (25, 50)}  # numpy
        # page-locked host memory
        pq_ = _buf.pinned_empty(q.shape, np.float32)
        pq_[:] = q
        out = (_buf.pinned_empty((nq, rm.LIMIT), np.uint64), _buf.pinned_empty((nq, rm.LIMIT), np.float32),
               _buf.pinned_empty((nq,), np.uint32))
        for r in (25, 50, 25):
            for o in out:
                o[...] = 99
            x.search_batch(pq_, rm.LIMIT, rm.L, rerank=r, out=out)
            assert np.array_equal(out[0], want[r][0]) and np.array_equal(bits(out[1]), bits(want[r][1])), r
            assert np.array_equal(out[2], want[r][2]), r
        # device tensors with out=, two calls back to back on one stream: the second reuses the first's scratch
        tq = torch.from_numpy(q).cuda()
        outs = [(torch.full((nq, rm.LIMIT), -1, dtype=torch.int64, device="cuda"),
                 torch.full((nq, rm.LIMIT), -1.0, dtype=torch.float32, device="cuda"),
                 torch.full((nq,), -1, dtype=torch.int32, device="cuda")) for _ in range(2)]
        x.search_batch(tq, rm.LIMIT, rm.L, rerank=50, out=outs[0])
        x.search_batch(tq, rm.LIMIT, rm.L, rerank=25, out=outs[1])
        torch.cuda.synchronize()
        for o, r in zip(outs, (50, 25)):
            assert np.array_equal(o[0].cpu().numpy().astype(np.uint64), want[r][0]), r
            assert np.array_equal(bits(o[1].cpu().numpy()), bits(want[r][1])), r
            assert np.array_equal(o[2].cpu().numpy().astype(np.uint32), want[r][2]), r
        # ... and with a trace, in device memory
        t_ids, t_d, t_c, t_tr = x.search_batch(tq, rm.LIMIT, rm.L, rerank=25, trace=True, visit_cap=VC)
        w_tr = x.search_batch(tq, 25, rm.L, trace=True, visit_cap=VC)[3]
        torch.cuda.synchronize()
        assert np.array_equal(t_ids.cpu().numpy().astype(np.uint64), want[25][0])
        assert torch.equal(t_tr.n_dist, w_tr.n_dist) and torch.equal(t_tr.visit_ids, w_tr.visit_ids)
