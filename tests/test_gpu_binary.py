"""Binary quantizer parity (GPU): threshold fit, encode and the bit distances against the numpy model
(tests/binary_model.py); an index with the quantizer attached against the oracle -- hamming distance between codes IS
the squared euclidean distance between their 0.0 / 1.0 expansions, exactly, in float32 and in any summation order, so
oracle.Index(d, "euclidean") over the expanded code rows is the reference's hamming store: greedySearch, robustPrune,
insertSinglePoint, the delete path and the batched round schedule, ties broken by the reference's rules.  Jaccard has
no float twin: there the model's Python restatement (checked against the oracle in tests/test_binary_model.py) is the
oracle.  Every comparison is exact: ids, float bits, counters, graph edges."""
import numpy as np
import pytest

from tests import binary_model as bm
from tests.helpers import bits, start_vector, unit_rows

pytestmark = pytest.mark.gpu


def _new_gpu(d, metric, R, L, alpha=1.2):
    from semadb_amd import vamana
    return vamana.NewIndexVamana("bq", vamana.IndexVectorVamanaParameters(d, metric, L, R, alpha), strict=False)


def _bq(d, metric, thr=None):
    from semadb_amd import vectorstore as vs
    q = vs.BinaryQuantizer(vs.BinaryQuantizerParameters(None, 0, metric), d)
    if thr is not None:
        q.set_threshold(thr)
    return q


def _clustered(rng, n, d, unit=False):
    """rows around a few centres: codes that share most bits, so nearly every distance ties with others"""
    centers = rng.standard_normal((10, d)).astype(np.float32)
    rows = (centers[rng.integers(0, 10, n)] + 0.7 * rng.standard_normal((n, d))).astype(np.float32)
    if unit:
        rows /= np.linalg.norm(rows, axis=1, keepdims=True).astype(np.float32)
    return rows


def _codes_in_order(ix):
    from semadb_amd import vectorstore as vs
    ids, vecs, off, edges = ix.export()
    return ids, vecs, off, edges, vs.get_bit_codes(ix, ids)


def _oracle_of(oracle, ix, d, R, L, alpha=1.2):
    """the index's graph over the 0/1 expansion of its code rows, in the oracle"""
    ids, _, off, edges, codes = _codes_in_order(ix)
    o = oracle.Index(d, "euclidean", R, L, alpha)
    assert o.load(ids, bm.expand(codes, d), off, edges) == 0
    return o


def _same_graph(ix, o):
    g_ids, _, g_off, g_e = ix.export()
    o_ids, _, o_off, o_e = o.export(with_vectors=False)
    assert np.array_equal(g_ids, o_ids)
    assert np.array_equal(g_off, o_off), "degree sequence differs"
    assert np.array_equal(g_e, o_e), "edge lists differ"


def _check_walks(ix, o, thr, d, q, limit, ss, filters=None, bitmap=False):
    """device search of float queries == oracle search of their expanded codes: everything the trace shows"""
    from semadb_amd import vamana
    f = filters
    if filters is not None and bitmap:
        f = vamana.FilterBitmaps.from_sets(filters)
    g_ids, g_d, g_c, tr = ix.search_batch(q, limit, ss, filters=f, trace=True, visit_cap=2048)  # (searchSize 512: 512+ hops)
    qx = bm.expand(bm.encode(q, thr), d)
    for k in range(q.shape[0]):
        o_ids, o_d, o_vis, o_tr = o.search(qx[k], limit, ss, filter_ids=None if filters is None else filters[k])
        m = len(o_ids)
        assert int(g_c[k]) == m, (k, limit, ss)
        assert np.array_equal(g_ids[k, :m], o_ids), (k, limit, ss)
        assert np.array_equal(bits(g_d[k, :m]), bits(o_d)), (k, limit, ss)
        assert (int(tr.n_dist[k]), int(tr.n_hop[k]), int(tr.n_edges[k])) == (o_tr.n_dist, o_tr.n_hop, o_tr.n_edges), (k, limit, ss)
        assert np.array_equal(tr.visit_ids[k, :o_tr.n_hop], o_vis), (k, limit, ss)


# (searchSize 129 .. 512: the eight-register candidate array, k_greedy_search<BitDist, 8, *, 0>; limit > 64: a result row
# that crosses its registers -- and nearly every bit distance ties with others)
LARGE_CASES = [(10, 256), (129, 129), (512, 512)]
CASES = [(1, 1), (10, 10), (10, 64), (10, 65), (10, 75), (100, 100), (10, 128), (10, 129)] + LARGE_CASES


# ---- 1. the quantizer object ----------------------------------------------------------------------------------

@pytest.mark.parametrize("d", [1, 5, 63, 64, 65, 200, 384, 768, 4096])
def test_encode_fit_distance_against_the_model(d):
    import torch
    from semadb_amd import SemaDBError, vectorstore as vs
    rng = np.random.default_rng(d)
    X = _clustered(rng, 40, d)
    bq = _bq(d, "hamming")
    assert bq.threshold() is None and bq.W == bm.n_words(d)
    with pytest.raises(SemaDBError) as e:
        bq.encode(X)
    assert e.value.code == 3  # SDB_ERR_STATE without a threshold (encode returns nil, binary.go:104-106)
    thr = rng.standard_normal(d).astype(np.float32)
    thr[0] = 0.0
    bq.set_threshold(thr)
    assert np.array_equal(bits(bq.threshold()), bits(thr))
    # values equal to their threshold, +-0 around a 0 threshold, denormals, NaN and +-Inf
    X[0] = thr
    X[1] = np.nextafter(thr, np.float32(np.inf))
    X[2] = np.nextafter(thr, np.float32(-np.inf))
    X[3], X[4], X[5], X[6], X[7] = 0.0, -0.0, np.nan, np.inf, -np.inf
    X[8, ::2] = np.nan
    X[9, 0] = np.float32(1e-45)
    want = bm.encode(X, thr)
    assert int(want[0].sum()) == 0 and int(want[5].sum()) == 0
    got = bq.encode(X)
    assert got.dtype == np.uint64 and np.array_equal(got, want)
    got_dev = bq.encode(torch.from_numpy(X).cuda())
    torch.cuda.synchronize()
    assert np.array_equal(got_dev.cpu().numpy().view(np.uint64), want)
    # distances: random codes, the empty code and the full one, host and device memory
    Y = bm.encode(_clustered(rng, 70, d), thr)
    Y[0], Y[1] = 0, bm.encode(np.full((1, d), np.inf, np.float32), thr)[0]
    Q = np.concatenate([want[:12], Y[:2]])
    for metric in ("hamming", "jaccard"):
        ref = bm.distance_matrix(metric, Q, Y)
        assert np.array_equal(bits(vs.bit_distance(metric, Q, Y)), bits(ref)), metric
        qd, yd = torch.from_numpy(Q.view(np.int64)).cuda(), torch.from_numpy(Y.view(np.int64)).cuda()
        out = vs.bit_distance(metric, qd, yd)
        torch.cuda.synchronize()
        assert np.array_equal(bits(out.cpu().numpy()), bits(ref)), metric
        odd = torch.zeros(1 + Y.size, dtype=torch.int64, device="cuda")  # code rows 8 bytes off a 16-byte boundary
        odd[1:] = yd.flatten()
        out = vs.bit_distance(metric, qd, odd[1:].view(-1, bq.W))
        torch.cuda.synchronize()
        assert np.array_equal(bits(out.cpu().numpy()), bits(ref)), metric
    assert bm.distance_matrix("jaccard", Y[:1], Y[:1])[0, 0] == 0 and vs.bit_distance("jaccard", Y[:1], Y[:1])[0, 0] == 0
    bq.close()


@pytest.mark.parametrize("n,d", [(1, 5), (2, 65), (5000, 70), (5000, 384), (77, 4096)])
def test_fit_is_the_sequential_float32_mean(n, d):
    import torch
    rng = np.random.default_rng(n + d)
    X = (rng.standard_normal((n, d)) * 100 + 3).astype(np.float32)  # sums that round at every step
    want = bm.fit_threshold(X)
    for dev in (False, True):
        bq = _bq(d, "jaccard")
        bq.Fit(torch.from_numpy(X).cuda() if dev else X)
        if dev:
            torch.cuda.synchronize()
        assert np.array_equal(bits(bq.threshold()), bits(want)), dev
        bq.Fit(X[:1] + 1)  # a quantizer that has its threshold is not fitted again (binary.go:148)
        assert np.array_equal(bits(bq.threshold()), bits(want))
        bq.close()
    if n == 2 and d == 65:  # Fit of [1, 2], [3, 4] -> [2, 3] (binary_test.go)
        bq = _bq(2, "hamming")
        bq.Fit(np.array([[1, 2], [3, 4]], np.float32))
        assert np.array_equal(bq.threshold(), np.array([2, 3], np.float32))
        bq.close()


def test_known_answers_on_the_device():
    from semadb_amd import vectorstore as vs
    bq = vs.New(vs.Quantizer(vs.QuantizerBinary, Binary=vs.BinaryQuantizerParameters(0.5, 0, "hamming")), "euclidean", 5)
    assert isinstance(bq, vs.BinaryQuantizer)
    assert int(bq.encode(np.array([[1.0, 0.1, 0.6, 0.7, 0.4]], np.float32))[0, 0]) == 0b01101  # binary_test.go:11-24
    x, y = np.array([[0b1001, 0b1]], np.uint64), np.array([[0b1101, 0]], np.uint64)
    assert vs.bit_distance("hamming", x, y)[0, 0] == 2 and vs.bit_distance("jaccard", x, y)[0, 0] == 0.5
    assert bq.distance(x, y)[0, 0] == 2
    bq.close()
    # a collection whose own metric is a bit metric: 0/1 vectors cut at 0.5 (vectorstore.go:51-66)
    bq = vs.New(None, "jaccard", 3)
    assert np.array_equal(bq.threshold(), np.full(3, 0.5, np.float32)) and bq.params.DistanceMetric == "jaccard"
    bq.close()


# ---- 2. attach ------------------------------------------------------------------------------------------------

def test_attach_encodes_every_row_and_fits_over_live_rows():
    from semadb_amd import vectorstore as vs
    rng = np.random.default_rng(2)
    n, d = 900, 65
    base = _clustered(rng, n, d)
    ix = _new_gpu(d, "euclidean", 16, 30)
    ix.set_start(start_vector(rng, d))
    ids = np.arange(2, n + 2, dtype=np.uint64)
    ix.insert_batch(ids, base)
    ix.delete_batch(rng.choice(ids, 120, replace=False))  # tombstones in the slab
    ix.insert_batch(np.arange(5000, 5040, dtype=np.uint64), _clustered(rng, 40, d))
    rows, dead = ix.row_usage()
    assert dead == 120 and rows == n + 1 + 40
    size0 = ix.SizeInMemory()
    bq = _bq(d, "hamming")
    vs.attach_binary(ix, bq)
    l_ids, l_vecs, _, _ = ix.export()  # live rows in storage order, the start node first
    assert l_ids[0] == 1 and len(l_ids) == n + 1 - 120 + 40
    want = bm.fit_threshold(l_vecs)
    assert np.array_equal(bits(bq.threshold()), bits(want))
    codes = vs.get_bit_codes(ix, l_ids)
    got_vecs, found = ix.GetMany(l_ids)
    assert found.all() and np.array_equal(codes, bm.encode(got_vecs, want))
    assert ix.SizeInMemory() > size0  # the code array counts
    # codes as a bucket holds them: written and read back, unknown ids refused with nothing written
    mine = codes[5:9] ^ np.uint64(1)
    vs.set_bit_codes(ix, l_ids[5:9], mine)
    assert np.array_equal(vs.get_bit_codes(ix, l_ids[5:9]), mine)
    from semadb_amd import SemaDBError
    with pytest.raises(SemaDBError) as e:
        vs.set_bit_codes(ix, np.array([l_ids[3], 10**9], np.uint64), codes[:2] ^ np.uint64(2))
    assert e.value.code == 4 and np.array_equal(vs.get_bit_codes(ix, l_ids[3:4]), codes[3:4])
    ix.begin_write()
    with pytest.raises(SemaDBError) as e:
        vs.set_bit_codes(ix, l_ids[5:9], mine)
    assert e.value.code == 3
    ix.abort_write()
    ix.close()


def test_attach_error_paths():
    import ctypes as C
    from semadb_amd import SemaDBError, _lib, distance, vamana, vectorstore as vs
    rng = np.random.default_rng(3)
    d = 32
    base = unit_rows(rng, 300, d)
    ix = _new_gpu(d, "euclidean", 16, 30)
    ix.set_start(start_vector(rng, d))
    ix.insert_batch(None, base)
    bq = _bq(d, "hamming", np.zeros(d, np.float32))
    wrong = _bq(d + 1, "hamming", np.zeros(d + 1, np.float32))
    with pytest.raises(SemaDBError) as e:
        vs.attach_binary(ix, wrong)
    assert e.value.code == 1
    ix.begin_write()
    with pytest.raises(SemaDBError) as e:
        vs.attach_binary(ix, bq)
    assert e.value.code == 3
    ix.abort_write()
    with pytest.raises(SemaDBError) as e:
        vs.get_bit_codes(ix, [2])
    assert e.value.code == 3  # nothing attached
    pq = vs.ProductQuantizer("euclidean", vs.ProductQuantizerParameters(16, 4), d)
    pq.Fit(base.copy(), rng.integers(0, 300, 4))
    vs.attach(ix, pq)
    with pytest.raises(SemaDBError) as e:
        vs.attach_binary(ix, bq)
    assert e.value.code == 3  # a product quantizer is attached
    ix.close()
    ix = _new_gpu(d, "euclidean", 16, 30)
    empty = _bq(d, "hamming")
    with pytest.raises(SemaDBError) as e:
        vs.attach_binary(ix, empty)  # nothing to fit from
    assert e.value.code == 3
    ix.set_start(start_vector(rng, d))
    vs.attach_binary(ix, bq)
    with pytest.raises(SemaDBError) as e:
        vs.attach_binary(ix, _bq(d, "jaccard", np.zeros(d, np.float32)))
    assert e.value.code == 3  # another binary quantizer
    with pytest.raises(SemaDBError) as e:
        vs.attach(ix, pq)
    assert e.value.code == 3
    ix.close()
    # the bit metrics are no float metrics
    L = _lib.lib()
    x = np.zeros((1, d), np.float32)
    out = np.zeros((1, 1), np.float32)
    h = C.c_void_p()
    for m in (3, 4):
        assert L.sdb_distance_batch(m, d, x.ctypes.data, 1, x.ctypes.data, 1, out.ctypes.data, 0, 0, None) == 1
        p = _lib.IndexParams(d, m, 75, 64, 1.2, 0, 0, 0)
        assert L.sdb_index_create(C.byref(p), C.byref(h)) == 1
        assert L.sdb_pq_create(d, m, 4, 16, 0, C.byref(h)) == 1
    for m in (0, 1, 2, 5):
        assert L.sdb_bq_create(d, m, 0, C.byref(h)) == 1
        assert L.sdb_bit_distance_batch(m, 1, x.ctypes.data, 1, x.ctypes.data, 1, out.ctypes.data, 0, 0, None) == 1
    assert L.sdb_bq_create(0, 3, 0, C.byref(h)) == 1 and L.sdb_bq_create(4097, 3, 0, C.byref(h)) == 1
    with pytest.raises(SemaDBError):
        vamana.NewIndexVamana("x", vamana.IndexVectorVamanaParameters(d, "hamming"))
    with pytest.raises(SemaDBError):
        distance.distance_batch("jaccard", x, x)


# ---- 3. hamming search parity with the oracle -----------------------------------------------------------------

class _Table:
    pass


def _hamming_table(oracle, n, d, metric, seed, R=32, L=50):
    from semadb_amd import vectorstore as vs
    t = _Table()
    rng = np.random.default_rng(seed)
    t.rng, t.n, t.d, t.R, t.L = rng, n, d, R, L
    base = _clustered(rng, n, d, unit=metric == "cosine")
    t.ix = _new_gpu(d, metric, R, L)
    sv = start_vector(rng, d)
    t.ix.set_start(sv)
    t.ix.insert_batch(None, base)  # the float graph, built on the device
    t.bq = _bq(d, "hamming")
    vs.attach_binary(t.ix, t.bq)  # fitted from the rows
    t.thr = t.bq.threshold()
    assert np.array_equal(bits(t.thr), bits(bm.fit_threshold(np.concatenate([sv[None, :], base]))))
    t.o = _oracle_of(oracle, t.ix, d, R, L)
    t.q = (base[rng.integers(0, n, 64)] + 0.5 * rng.standard_normal((64, d))).astype(np.float32)
    t.q[0], t.q[1] = np.nan, 0.0
    t.base = base
    return t


@pytest.fixture(scope="module")
def cosine_table(oracle):
    t = _hamming_table(oracle, 2000, 128, "cosine", 11)
    yield t
    t.ix.close()


@pytest.fixture(scope="module")
def ragged_table(oracle):
    t = _hamming_table(oracle, 1500, 65, "euclidean", 12)
    yield t
    t.ix.close()


@pytest.mark.parametrize("limit,ss", CASES)
def test_hamming_search_equals_the_oracle(cosine_table, ragged_table, limit, ss):
    for t in (cosine_table, ragged_table):
        _check_walks(t.ix, t.o, t.thr, t.d, t.q, limit, ss)


@pytest.mark.parametrize("knob,value", [("no_hash", 1), ("hash_limit", 24), ("wide_walk", 2), ("wide_hash", 1)])
def test_hamming_search_under_every_setting(cosine_table, ragged_table, knob, value):
    for t in (cosine_table, ragged_table):
        t.ix.set_tuning(knob, value)
        try:
            for limit, ss in CASES:
                _check_walks(t.ix, t.o, t.thr, t.d, t.q, limit, ss)
        finally:
            t.ix.set_tuning(knob, 0)


@pytest.mark.parametrize("nq", [1, 257, 1024])
def test_hamming_search_batch_sizes(cosine_table, nq):
    import torch
    t = cosine_table
    rng = np.random.default_rng(nq)
    q = (t.base[rng.integers(0, t.n, nq)] + 0.5 * rng.standard_normal((nq, t.d))).astype(np.float32)
    qx = bm.expand(bm.encode(q, t.thr), t.d)
    for limit, ss in CASES:
        o_ids, o_d, o_c, o_nd, o_nh, o_ne = t.o.search_batch(qx, limit, ss)
        for dev in (False, True):
            g_ids, g_d, g_c, tr = t.ix.search_batch(torch.from_numpy(q).cuda() if dev else q, limit, ss, trace=True)
            if dev:
                torch.cuda.synchronize()
                g_ids, g_d, g_c = g_ids.cpu().numpy().view(np.uint64), g_d.cpu().numpy(), g_c.cpu().numpy()
                tr.n_dist, tr.n_hop, tr.n_edges = (x.cpu().numpy() for x in (tr.n_dist, tr.n_hop, tr.n_edges))
            assert np.array_equal(g_c.astype(np.int64), o_c.astype(np.int64))
            for k in range(nq):
                m = int(o_c[k])
                assert np.array_equal(g_ids[k, :m], o_ids[k, :m]) and np.array_equal(bits(g_d[k, :m]), bits(o_d[k, :m])), k
            assert np.array_equal(np.asarray(tr.n_dist, np.uint64), o_nd) and np.array_equal(np.asarray(tr.n_hop, np.uint64), o_nh)
            assert np.array_equal(np.asarray(tr.n_edges, np.uint64), o_ne)


def test_index_distance_batch_is_the_bit_distance(ragged_table):
    t = ragged_table
    ids, _, _, _, codes = _codes_in_order(t.ix)
    cand = np.stack([t.rng.choice(ids, 33, replace=False) for _ in range(8)])
    cand[0, 0], cand[3, 5] = 10**9, 0  # unknown ids -> math.MaxFloat32
    got = t.ix.distance_batch(t.q[:8], cand)
    pos = {int(v): i for i, v in enumerate(ids)}
    qc = bm.encode(t.q[:8], t.thr)
    for i in range(8):
        for j in range(33):
            want = np.float32(np.finfo(np.float32).max) if int(cand[i, j]) not in pos else bm.hamming(qc[i], codes[pos[int(cand[i, j])]])
            assert got[i, j] == want, (i, j)


def test_all_rows_one_code(oracle):
    """every row above the threshold everywhere: one code, every distance 0 -- the walk is decided by ties alone"""
    from semadb_amd import vectorstore as vs
    rng = np.random.default_rng(4)
    n, d = 400, 70
    base = rng.random((n, d), dtype=np.float32) + np.float32(0.5)
    ix = _new_gpu(d, "euclidean", 16, 30)
    ix.set_start(start_vector(rng, d) + np.float32(2))
    ix.insert_batch(None, base)
    thr = np.zeros(d, np.float32)
    vs.attach_binary(ix, _bq(d, "hamming", thr))
    o = _oracle_of(oracle, ix, d, 16, 30)
    q = np.concatenate([base[:4], -base[:4]])
    for limit, ss in ((1, 1), (10, 30), (10, 75)):
        _check_walks(ix, o, thr, d, q, limit, ss)
    ix.close()


def _overflowing(oracle, quant_first):
    """a start node with an overflow list, made by deletes as tests/test_gpu_delete.py makes it; `quant_first`: the
    deletes themselves run on the bit-code store (the delete path's bit distance), else on the float store"""
    from semadb_amd import vectorstore as vs
    rng = np.random.default_rng(1204)
    n, d, R, L = 1200, 48, 4, 20
    base = _clustered(rng, n, d)
    ix = _new_gpu(d, "euclidean", R, L, 1.5)
    ix.set_start(start_vector(rng, d))
    ids = np.arange(2, n + 2, dtype=np.uint64)
    ix.insert_batch(ids, base, round_size=1)
    thr = bm.fit_threshold(base)
    o = None
    if quant_first:
        vs.attach_binary(ix, _bq(d, "hamming", thr))
        o = _oracle_of(oracle, ix, d, R, L, 1.5)
    dels = rng.choice(ids, n // 8, replace=False).astype(np.uint64)
    ix.delete_batch(dels)
    if quant_first:
        assert o.delete(dels) == 0
        _same_graph(ix, o)
    else:
        vs.attach_binary(ix, _bq(d, "hamming", thr))
        o = _oracle_of(oracle, ix, d, R, L, 1.5)
    _, _, off, _ = ix.export()
    assert int(off[1] - off[0]) > 64 + 64, "the case must overflow the start node's row by more than one chunk"
    return ix, o, thr, d, rng, base


@pytest.mark.parametrize("quant_first", [False, True])
def test_start_node_with_an_overflow_list(oracle, quant_first):
    ix, o, thr, d, rng, base = _overflowing(oracle, quant_first)
    q = (base[rng.integers(0, len(base), 16)] + 0.3 * rng.standard_normal((16, d))).astype(np.float32)
    for limit, ss in ((5, 20), (10, 75), (1, 1)):
        _check_walks(ix, o, thr, d, q, limit, ss)
    filt = [list(range(2, 700, 3))] * 16
    _check_walks(ix, o, thr, d, q, 5, 20, filters=filt)
    # an insert whose back-edges meet the long start node (insert.go:47-58 over row + overflow + new point)
    new = _clustered(rng, 30, d)
    new_ids = np.arange(3000, 3030, dtype=np.uint64)
    ix.insert_batch(new_ids, new, round_size=1)
    nx = bm.expand(bm.encode(new, thr), d)
    for i in range(30):
        assert o.insert(int(new_ids[i]), nx[i]) == 0
    _same_graph(ix, o)
    _check_walks(ix, o, thr, d, q, 5, 20)
    ix.close()


# ---- 4. filtered parity ---------------------------------------------------------------------------------------

def _filters(rng, ids, nq, kind, ss):
    live = [int(v) for v in ids if int(v) != 1]
    out = []
    for k in range(nq):
        if kind == "one":
            f = [live[int(rng.integers(0, len(live)))]]
        elif kind == "few":
            f = [int(v) for v in rng.choice(live, max(1, ss // 3), replace=False)]
        elif kind == "half":
            f = [int(v) for v in rng.choice(live, len(live) // 2, replace=False)]
        else:  # unknown ids among known ones (skipped like GetMany does)
            f = [int(v) for v in rng.choice(live, 40, replace=False)] + [max(live) + 7, max(live) + 1000, 10**7 + k]
        out.append(sorted(set(f)))
    return out


@pytest.mark.parametrize("kind", ["one", "few", "half", "unknown"])
@pytest.mark.parametrize("bitmap", [False, True])
def test_filtered_hamming_search(cosine_table, ragged_table, kind, bitmap):
    for t in (cosine_table, ragged_table):
        ids = t.ix.export(with_vectors=False)[0]
        for limit, ss in ((1, 1), (10, 25), (10, 75), (10, 128)):
            f = _filters(np.random.default_rng(limit + ss), ids, 16, kind, ss)
            _check_walks(t.ix, t.o, t.thr, t.d, t.q[:16], limit, ss, filters=f, bitmap=bitmap)


def test_filtered_hamming_search_at_the_largest_array(cosine_table):
    """(512, 65): eight array registers and a result row of two, seeded by 170 ids, by half the table, by unknown ids;
    as id lists and as bitmaps"""
    t = cosine_table
    ids = t.ix.export(with_vectors=False)[0]
    for kind in ("few", "half", "unknown"):
        f = _filters(np.random.default_rng(512 + 65), ids, 16, kind, 512)
        for bitmap in (False, True):
            _check_walks(t.ix, t.o, t.thr, t.d, t.q[:16], 65, 512, filters=f, bitmap=bitmap)


@pytest.mark.parametrize("bitmap", [False, True])
def test_filtered_search_after_deletes(oracle, bitmap):
    """a table with deleted rows: filter ids go through the device's id -> slot table"""
    from semadb_amd import vectorstore as vs
    rng = np.random.default_rng(41)
    n, d, R, L = 1500, 65, 16, 30
    base = _clustered(rng, n, d)
    ix = _new_gpu(d, "euclidean", R, L)
    ix.set_start(start_vector(rng, d))
    ids = np.arange(2, n + 2, dtype=np.uint64)
    ix.insert_batch(ids, base)
    bq = _bq(d, "hamming")
    vs.attach_binary(ix, bq)
    thr = bq.threshold()
    o = _oracle_of(oracle, ix, d, R, L)
    dels = rng.choice(ids, 200, replace=False).astype(np.uint64)
    ix.delete_batch(dels)
    assert o.delete(dels) == 0
    _same_graph(ix, o)
    live = ix.export(with_vectors=False)[0]
    q = (base[rng.integers(0, n, 16)] + 0.5 * rng.standard_normal((16, d))).astype(np.float32)
    for kind in ("one", "few", "half", "unknown"):
        f = _filters(rng, live, 16, kind, 30)
        f[0] = sorted(set(f[0]) | set(int(v) for v in dels[:5]))  # deleted ids are unknown ids
        for limit, ss in ((10, 30), (5, 75)):
            _check_walks(ix, o, thr, d, q, limit, ss, filters=f, bitmap=bitmap)
    ix.close()


# ---- 5. / 7. jaccard: the Python restatement is the oracle ---------------------------------------------------------

def _model_of(ix, metric, R, L, alpha=1.2):
    ids, _, off, edges, codes = _codes_in_order(ix)
    g = bm.Graph(bm.PAIR[metric], R, L, alpha)
    g.load(ids, codes, off, edges)
    return g


def _check_walks_model(ix, g, thr, q, limit, ss, filters=None, bitmap=False):
    from semadb_amd import vamana
    f = filters
    if filters is not None and bitmap:
        f = vamana.FilterBitmaps.from_sets(filters)
    g_ids, g_d, g_c, tr = ix.search_batch(q, limit, ss, filters=f, trace=True, visit_cap=1024)
    qc = bm.encode(q, thr)
    for k in range(q.shape[0]):
        m = g.search(qc[k], limit, ss, None if filters is None else filters[k])
        assert int(g_c[k]) == len(m.ids), (k, limit, ss)
        assert np.array_equal(g_ids[k, :len(m.ids)], m.ids) and np.array_equal(bits(g_d[k, :len(m.ids)]), bits(m.dists)), (k, limit, ss)
        assert (int(tr.n_dist[k]), int(tr.n_hop[k]), int(tr.n_edges[k])) == (m.n_dist, m.n_hop, m.n_edges), (k, limit, ss)
        assert np.array_equal(tr.visit_ids[k, :m.n_hop], np.array(m.visit, np.uint64)), (k, limit, ss)


def test_jaccard_search_equals_the_restatement():
    from semadb_amd import vectorstore as vs
    rng = np.random.default_rng(5)
    n, d, R, L = 500, 70, 16, 30
    base = _clustered(rng, n, d)
    ix = _new_gpu(d, "euclidean", R, L)
    ix.set_start(start_vector(rng, d))
    ix.insert_batch(None, base)
    bq = _bq(d, "jaccard")
    vs.attach_binary(ix, bq)
    thr = bq.threshold()
    g = _model_of(ix, "jaccard", R, L)
    q = (base[rng.integers(0, n, 32)] + 0.5 * rng.standard_normal((32, d))).astype(np.float32)
    q[0], q[1] = np.nan, -1e9  # empty query codes: every union is the row's own bits, or empty
    ids = ix.export(with_vectors=False)[0]
    for ss in (1, 25, 75):
        limit = min(10, ss)
        _check_walks_model(ix, g, thr, q, limit, ss)
        for kind in ("few", "half", "unknown"):
            f = _filters(rng, ids, 32, kind, ss)
            _check_walks_model(ix, g, thr, q, limit, ss, filters=f)
            _check_walks_model(ix, g, thr, q, limit, ss, filters=f, bitmap=True)
    for limit, ss in LARGE_CASES:  # (500 rows: at 512 the array never fills)
        _check_walks_model(ix, g, thr, q[:12], limit, ss)
    _check_walks_model(ix, g, thr, q[:12], 129, 129, filters=_filters(rng, ids, 12, "half", 129))
    ix.set_tuning("no_hash", 1)
    _check_walks_model(ix, g, thr, q, 10, 75)
    # the exact scan and explicit distances under jaccard
    got = ix.distance_batch(q[:4], np.tile(ids[None, :50], (4, 1)))
    codes = vs.get_bit_codes(ix, ids[:50])
    assert np.array_equal(bits(got), bits(bm.distance_matrix("jaccard", bm.encode(q[:4], thr), codes)))
    ix.close()


@pytest.mark.parametrize("metric", ["jaccard", "hamming"])
def test_sequential_build_equals_the_restatement(metric):
    from semadb_amd import vectorstore as vs
    rng = np.random.default_rng(7)
    n, d, R, L = 300, 70, 8, 25
    base = _clustered(rng, n, d)
    sv = start_vector(rng, d)
    thr = bm.fit_threshold(base)
    ix = _new_gpu(d, "cosine", R, L)
    ix.set_start(sv)
    vs.attach_binary(ix, _bq(d, metric, thr))  # a store that encodes from the first Set on
    ids = np.arange(2, n + 2, dtype=np.uint64)
    ix.insert_batch(ids, base, round_size=1)
    g = bm.Graph(bm.PAIR[metric], R, L, 1.2)
    g.set_start(bm.encode(sv[None, :], thr)[0])
    codes = bm.encode(base, thr)
    for i in range(n):
        g.insert(int(ids[i]), codes[i])
    m_ids, m_off, m_e = g.export()
    g_ids, _, g_off, g_e = ix.export()
    assert np.array_equal(g_ids, m_ids) and np.array_equal(g_off, m_off), "degree sequence differs"
    assert np.array_equal(g_e, m_e), "edge lists differ"
    assert np.array_equal(vs.get_bit_codes(ix, ids), codes)
    ix.close()


# ---- 6. writes, hamming ---------------------------------------------------------------------------------------

def _write_table(oracle, seed, n=1500, d=65, R=16, L=30):
    from semadb_amd import vectorstore as vs
    t = _Table()
    rng = np.random.default_rng(seed)
    t.rng, t.n, t.d, t.R, t.L = rng, n, d, R, L
    t.base = _clustered(rng, n, d)
    t.ix = _new_gpu(d, "euclidean", R, L)
    t.ix.set_start(start_vector(rng, d))
    t.ids = np.arange(2, n + 2, dtype=np.uint64)
    t.ix.insert_batch(t.ids, t.base)
    t.bq = _bq(d, "hamming")
    vs.attach_binary(t.ix, t.bq)
    t.thr = t.bq.threshold()
    t.o = _oracle_of(oracle, t.ix, d, R, L)
    t.q = (t.base[rng.integers(0, n, 24)] + 0.5 * rng.standard_normal((24, d))).astype(np.float32)
    return t


def test_sequential_inserts_after_attach(oracle):
    t = _write_table(oracle, 61)
    new = _clustered(t.rng, 300, t.d)
    new_ids = np.arange(9000, 9300, dtype=np.uint64)
    t.ix.insert_batch(new_ids, new, round_size=1)
    nx = bm.expand(bm.encode(new, t.thr), t.d)
    for i in range(300):
        assert t.o.insert(int(new_ids[i]), nx[i]) == 0
    _same_graph(t.ix, t.o)
    from semadb_amd import vectorstore as vs
    assert np.array_equal(vs.get_bit_codes(t.ix, new_ids), bm.encode(new, t.thr))
    _check_walks(t.ix, t.o, t.thr, t.d, t.q, 10, 30)
    t.ix.close()


@pytest.mark.parametrize("round_size,big_min", [(0, 512), (0, 2), (64, 3)])
def test_batched_inserts_equal_the_oracle_schedule(oracle, round_size, big_min):
    t = _write_table(oracle, 62 + big_min, n=1200)
    new = _clustered(t.rng, 1500, t.d)
    new_ids = np.arange(9000, 10500, dtype=np.uint64)
    t.ix.set_tuning("hub_min", big_min)
    t.ix.insert_batch(new_ids, new, round_size=round_size)
    assert t.o.insert_rounds(new_ids, bm.expand(bm.encode(new, t.thr), t.d), round_size=round_size, big_min=big_min) == 0
    _same_graph(t.ix, t.o)
    if big_min < 512:
        assert t.ix.build_stats()["hubs"] > 0
    _check_walks(t.ix, t.o, t.thr, t.d, t.q, 10, 30)
    t.ix.close()


def test_delete_update_compact_abort(oracle):
    from semadb_amd import vectorstore as vs
    t = _write_table(oracle, 63)
    ix, o = t.ix, t.o
    dels = t.rng.choice(t.ids, 150, replace=False).astype(np.uint64)
    ix.delete_batch(dels)
    assert o.delete(dels) == 0
    _same_graph(ix, o)
    _check_walks(ix, o, t.thr, t.d, t.q, 10, 30)
    # an update: delete + insert of the same ids with new vectors, one transaction; a search issued while it is open
    # answers from the committed graph
    upd = np.array(sorted(set(int(v) for v in t.ids) - set(int(v) for v in dels)))[:40].astype(np.uint64)
    newv = _clustered(t.rng, 40, t.d)
    ix.begin_write()
    ix.delete_batch(upd)
    ix.insert_batch(upd, newv, round_size=1)
    _check_walks(ix, o, t.thr, t.d, t.q, 10, 30)  # `o` is still the committed state
    # a filter is strictly ascending: the updated ids, the deleted ones among 2..399 (unknown to the table) and the rest
    filt = [sorted(set(int(v) for v in upd) | set(range(2, 400)))] * len(t.q)
    _check_walks(ix, o, t.thr, t.d, t.q, 10, 30, filters=filt)
    ix.commit()
    assert o.delete(upd) == 0
    nx = bm.expand(bm.encode(newv, t.thr), t.d)
    for i in range(40):
        assert o.insert(int(upd[i]), nx[i]) == 0
    _same_graph(ix, o)
    _check_walks(ix, o, t.thr, t.d, t.q, 10, 30)
    assert np.array_equal(vs.get_bit_codes(ix, upd), bm.encode(newv, t.thr))
    # a transaction that inserted and is aborted leaves no trace
    ix.begin_write()
    ix.insert_batch(np.arange(20000, 20100, dtype=np.uint64), _clustered(t.rng, 100, t.d))
    ix.abort_write()
    _same_graph(ix, o)
    _check_walks(ix, o, t.thr, t.d, t.q, 10, 30)
    # compaction moves the code rows with their rows
    ids_before = ix.export(with_vectors=False)[0]
    codes_before = vs.get_bit_codes(ix, ids_before)
    assert ix.row_usage()[1] > 0
    ix.compact()
    assert ix.row_usage()[1] == 0
    assert np.array_equal(vs.get_bit_codes(ix, ids_before), codes_before)
    _same_graph(ix, o)
    _check_walks(ix, o, t.thr, t.d, t.q, 10, 30)
    _check_walks(ix, o, t.thr, t.d, t.q, 10, 30, filters=filt)
    # and the table keeps growing past its capacity with its codes
    more = _clustered(t.rng, 2500, t.d)
    more_ids = np.arange(30000, 32500, dtype=np.uint64)
    ix.insert_batch(more_ids, more)
    assert o.insert_rounds(more_ids, bm.expand(bm.encode(more, t.thr), t.d)) == 0
    _same_graph(ix, o)
    assert np.array_equal(vs.get_bit_codes(ix, ids_before), codes_before)
    ix.close()


def test_union_prune_on_bit_codes(oracle):
    t = _write_table(oracle, 64, n=900, R=8)
    extra = t.rng.choice(t.ids[100:], 200, replace=False).astype(np.uint64)
    for chip_wide in (False, True):
        node = int(t.ids[7 + chip_wide])
        t.ix.union_prune(node, extra, chip_wide=chip_wide)
        assert t.o.union_prune(node, extra) == 0
        _same_graph(t.ix, t.o)
    t.ix.close()


# ---- 8. flat scan ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("metric", ["hamming", "jaccard"])
def test_flat_scan_keeps_the_first_stored_row_of_a_tie(metric):
    """IndexFlat.Search over a binary store (flat.go:98-124): `dist >= tail -> skip`, so among equal distances -- under
    hamming nearly all of them -- the row stored first stays: a stable sort by distance over storage order"""
    from semadb_amd import flat, vectorstore as vs
    rng = np.random.default_rng(8)
    n, d = 3000, 65
    base = _clustered(rng, n, d)
    ix = _new_gpu(d, "euclidean", 16, 30)
    ix.set_start(start_vector(rng, d))
    ids = np.arange(2, n + 2, dtype=np.uint64)
    ix.insert_batch(ids, base)
    ix.delete_batch(ids[100:160])
    bq = _bq(d, metric)
    vs.attach_binary(ix, bq)
    thr = bq.threshold()
    l_ids, _, _, _, codes = _codes_in_order(ix)
    l_ids, codes = l_ids[1:], codes[1:]  # the start node is not a point
    q = (base[rng.integers(0, n, 20)] + 0.5 * rng.standard_normal((20, d))).astype(np.float32)
    q[0] = np.nan
    dm = bm.distance_matrix(metric, bm.encode(q, thr), codes)
    filters = [sorted(int(v) for v in rng.choice(l_ids, 500, replace=False)) + [10**8] for _ in range(20)]
    filters[1] = [int(l_ids[3])]
    for limit in (1, 10, 128):
        for filt in (None, filters):
            g_ids, g_d, g_c = flat.flat_search_batch(ix._h, d, q, limit, filt)
            for k in range(20):
                sel = np.arange(len(l_ids)) if filt is None else np.flatnonzero(np.isin(l_ids, np.array(filt[k], np.uint64)))
                order = sel[np.argsort(dm[k, sel], kind="stable")][:limit]
                assert int(g_c[k]) == len(order), (limit, k)
                assert np.array_equal(g_ids[k, :len(order)], l_ids[order]), (limit, k)
                assert np.array_equal(bits(g_d[k, :len(order)]), bits(dm[k, order])), (limit, k)
    ix.close()


def test_flat_store_sets_and_replaces_vectors():
    """an index without a graph (IndexFlat): vecStore.Set encodes (binary.go:131-139), a replaced id gets a new code row"""
    from semadb_amd import flat, vectorstore as vs
    rng = np.random.default_rng(9)
    d = 200
    fx = flat.NewIndexFlat(flat.IndexVectorFlatParameters(d, "euclidean"))
    base = _clustered(rng, 600, d)
    ids = np.arange(10, 610, dtype=np.uint64)
    fx.set_vectors(ids[:300], base[:300])
    bq = _bq(d, "hamming")
    vs.attach_binary(fx, bq)
    thr = bq.threshold()
    assert np.array_equal(bits(thr), bits(bm.fit_threshold(base[:300])))
    fx.set_vectors(ids[300:], base[300:])
    fx.set_vectors(ids[5:9], base[500:504])  # replaced
    want = bm.encode(base, thr)
    want[5:9] = want[500:504]
    assert np.array_equal(vs.get_bit_codes(fx, ids), want)
    q = base[:6] + 0.2
    g_ids, g_d, g_c = fx.search_batch(q.astype(np.float32), 10)
    stored = np.concatenate([ids[:5], ids[9:], ids[5:9]])  # storage order: the replaced rows were appended
    codes = np.concatenate([want[:5], want[9:], want[5:9]])
    dm = bm.distance_matrix("hamming", bm.encode(q, thr), codes)
    for k in range(6):
        order = np.argsort(dm[k], kind="stable")[:10]
        assert np.array_equal(g_ids[k], stored[order]) and np.array_equal(bits(g_d[k]), bits(dm[k, order]))
    fx.close()


# ---- the Python mirror's store policy (vamana.IndexVamana with Quantizer(Type="binary")) ------------------------

def _mirror_index(d, R, L, binary):
    from semadb_amd import vamana, vectorstore as vs
    p = vamana.IndexVectorVamanaParameters(d, "euclidean", L, R, 1.2, Quantizer=vs.Quantizer(vs.QuantizerBinary, Binary=binary))
    return vamana.NewIndexVamana("bq", p, strict=False)


def test_a_given_threshold_encodes_from_the_first_set_on(oracle):
    """binary.go:51-56, 131-139: with Threshold given the store encodes every Set, the start node's included, so the
    first batch's graph is already built on hamming distances: the oracle's sequential inserts over the 0/1 rows"""
    from semadb_amd import SemaDBError, vamana, vectorstore as vs
    rng = np.random.default_rng(71)
    d, R, L, n = 70, 8, 25, 300
    ix = _mirror_index(d, R, L, vs.BinaryQuantizerParameters(0.25, 0, "hamming"))
    thr = np.full(d, 0.25, np.float32)
    assert ix._bq is ix._store and np.array_equal(bits(ix._store.threshold()), bits(thr))
    with pytest.raises(SemaDBError) as e:  # stored codes and query codes are cut at one threshold
        ix._store.set_threshold(thr + 1)
    assert e.value.code == 3
    sv = start_vector(rng, d)
    ix.set_start(sv)
    base = _clustered(rng, n, d)
    ix.InsertUpdateDelete([vamana.IndexVectorChange(i + 2, base[i]) for i in range(n)], round_size=1)
    ids, _, _, _, codes = _codes_in_order(ix)
    assert np.array_equal(codes, bm.encode(np.concatenate([sv[None, :], base]), thr))
    o = oracle.Index(d, "euclidean", R, L, 1.2)
    o.set_start(bm.expand(codes[:1], d)[0])
    for i in range(n):
        assert o.insert(i + 2, bm.expand(codes[i + 1:i + 2], d)[0]) == 0
    _same_graph(ix, o)
    ix.close()


def test_without_a_threshold_the_store_is_fitted_at_the_trigger():
    """binary.go:145-185: no threshold -> float distances until TriggerThreshold points are stored (the start node is
    one), then the column means over the stored rows in storage order; later Sets are encoded with them"""
    from semadb_amd import SemaDBError, vamana, vectorstore as vs
    rng = np.random.default_rng(72)
    d, n = 70, 150
    ix = _mirror_index(d, 8, 25, vs.BinaryQuantizerParameters(None, 100, "jaccard"))
    sv = start_vector(rng, d)
    ix.set_start(sv)
    base = _clustered(rng, n, d)
    ch = [vamana.IndexVectorChange(i + 2, base[i]) for i in range(n)]
    ix.InsertUpdateDelete(ch[:50])
    assert ix._bq is None and ix._store.threshold() is None  # 51 stored points
    with pytest.raises(SemaDBError) as e:
        vs.get_bit_codes(ix, [2])
    assert e.value.code == 3
    ix.InsertUpdateDelete(ch[50:120])
    thr = ix._store.threshold()
    assert ix._bq is ix._store and np.array_equal(bits(thr), bits(bm.fit_threshold(np.concatenate([sv[None, :], base[:120]]))))
    ix.InsertUpdateDelete(ch[120:])
    ids, _, _, _, codes = _codes_in_order(ix)
    assert np.array_equal(ids, np.arange(1, n + 2, dtype=np.uint64))
    assert np.array_equal(codes, bm.encode(np.concatenate([sv[None, :], base]), thr))
    ix.close()
