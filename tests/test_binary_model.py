"""CPU-only: the binary quantizer's model (tests/binary_model.py) gives the reference's known answers, its hamming
distance IS the oracle's squared euclidean distance over 0/1 rows, and its restatement of the walk and of the build
agrees with oracle.Index over those rows -- which is what lets tests/test_gpu_binary.py use it as the jaccard oracle.
Also the parameter rules of models/quantizer.go and vectorstore.New for the `binary` kind."""
import numpy as np
import pytest

from tests import binary_model as bm
from tests.helpers import bits


def _impls(oracle):
    out = [oracle.IMPL_ASM]
    for name in ("IMPL_AVX2", "IMPL_PURE"):  # the oracle's three arithmetics
        if hasattr(oracle, name) and (name != "IMPL_AVX2" or oracle.has_avx2()):
            out.append(getattr(oracle, name))
    return out


def test_known_answers():
    """binary_test.go:11-39 and distance_test.go:41-57"""
    codes = bm.encode([[1.0, 0.1, 0.6, 0.7, 0.4]], np.full(5, 0.5, np.float32))
    assert codes.shape == (1, 1) and int(codes[0, 0]) == 0b01101
    assert np.array_equal(bits(bm.fit_threshold([[1, 2], [3, 4]])), bits([2, 3]))
    x, y = np.array([0b1001, 0b1], np.uint64), np.array([0b1101, 0], np.uint64)
    assert bm.hamming(x, y) == np.float32(2) and bm.hamming_int(bm.code_int(x), bm.code_int(y)) == np.float32(2)
    assert bm.jaccard(x, y) == np.float32(0.5) and bm.jaccard_int(bm.code_int(x), bm.code_int(y)) == np.float32(0.5)
    z = np.zeros(2, np.uint64)
    assert bm.jaccard(z, z) == np.float32(0) and bm.jaccard_int(0, 0) == np.float32(0)
    assert np.array_equal(bm.distance_matrix("jaccard", [x, z], [y, z]), np.array([[0.5, 1], [1, 0]], np.float32))


def test_encode_is_strict_and_nan_is_zero():
    thr = np.array([0.0, 0.0, 1.5, -np.inf, np.inf, 0.0, np.nan], np.float32)
    v = np.array([[0.0, -0.0, 1.5, -np.inf, np.inf, np.nan, 1.0],
                  [np.float32(1e-45), 1.0, np.nextafter(np.float32(1.5), np.float32(2)), 0.0, np.inf, np.inf, np.nan]], np.float32)
    codes = bm.encode(v, thr)
    assert int(codes[0, 0]) == 0 and int(codes[1, 0]) == 0b0101111
    assert np.array_equal(bm.expand(codes, 7)[1], np.array([1, 1, 1, 1, 0, 1, 0], np.float32))


@pytest.mark.parametrize("d", [1, 5, 63, 64, 65, 200, 384, 4096])
def test_hamming_is_the_oracles_euclidean_over_expanded_rows(oracle, d):
    rng = np.random.default_rng(d)
    x = bm.encode(rng.standard_normal((9, d)), np.zeros(d, np.float32))
    y = bm.encode(rng.standard_normal((11, d)), np.zeros(d, np.float32))
    x[0], y[0] = 0, bm.encode(np.ones((1, d)), np.zeros(d, np.float32))[0]  # the empty code against the full one
    want = bm.distance_matrix("hamming", x, y)
    assert want[0, 0] == np.float32(d)
    for impl in _impls(oracle):
        got = oracle.distance_matrix(bm.expand(x, d), bm.expand(y, d), "euclidean", impl=impl)
        assert np.array_equal(bits(got), bits(want))
    for i in range(3):
        for j in range(3):
            assert bm.hamming(x[i], y[j]) == want[i, j] == bm.hamming_int(bm.code_int(x[i]), bm.code_int(y[j]))


def _table(seed, n, d):
    """clustered rows so that codes share many bits (ties) and a threshold at the column means"""
    rng = np.random.default_rng(seed)
    centers = rng.standard_normal((12, d)).astype(np.float32)
    rows = (centers[rng.integers(0, 12, n)] + 0.6 * rng.standard_normal((n, d))).astype(np.float32)
    return rng, rows


def test_restatement_equals_the_oracle_search_and_build(oracle):
    """hamming as the pair function: the Python restatement and oracle.Index(d, "euclidean") over the expanded rows give
    the same sequential build, edge for edge, and on it the same searches -- ids, distance bits, visit order, counters"""
    n, d, R, L = 300, 70, 8, 25
    rng, rows = _table(5, n + 1, d)
    thr = bm.fit_threshold(rows)
    codes = bm.encode(rows, thr)
    ex = bm.expand(codes, d)
    o = oracle.Index(d, "euclidean", R, L, 1.2)
    g = bm.Graph(bm.PAIR["hamming"], R, L, 1.2)
    o.set_start(ex[0])
    g.set_start(codes[0])
    for i in range(1, n + 1):
        assert o.insert(i + 1, ex[i]) == 0
        g.insert(i + 1, codes[i])
    o_ids, _, o_off, o_edges = o.export()
    g_ids, g_off, g_edges = g.export()
    assert np.array_equal(g_ids, o_ids) and np.array_equal(g_off, o_off), "degree sequence differs"
    assert np.array_equal(g_edges, o_edges), "edge lists differ"
    q = bm.encode(rows[rng.integers(0, n, 12)] + 0.4 * rng.standard_normal((12, d)).astype(np.float32), thr)
    q[0] = 0
    filters = [None, [7], list(range(2, 12)), list(range(2, n + 2, 2)), [3, 9, 10**6, 10**6 + 5]]
    for limit, ss in ((1, 1), (1, 2), (2, 2), (10, 25), (10, 75), (75, 75)):
        for filt in filters:
            for k in range(q.shape[0]):
                o_i, o_d, o_vis, o_tr = o.search(bm.expand(q[k:k + 1], d)[0], limit, ss, filter_ids=filt)
                m = g.search(q[k], limit, ss, filt)
                assert np.array_equal(m.ids, o_i) and np.array_equal(bits(m.dists), bits(o_d)), (limit, ss, filt, k)
                assert np.array_equal(np.array(m.visit, np.uint64), o_vis)
                assert (m.n_dist, m.n_hop, m.n_edges) == (o_tr.n_dist, o_tr.n_hop, o_tr.n_edges)


def test_binary_quantizer_parameters_validate():
    """models/quantizer.go:41-49"""
    from semadb_amd import SemaDBError
    from semadb_amd.vectorstore import BinaryQuantizerParameters as P
    P(None, 0, "hamming").Validate()
    P(None, 50000, "jaccard").Validate()
    P(0.5, 10**9, "hamming").Validate()  # the trigger is not looked at when a threshold is given
    for bad in (P(None, -1, "hamming"), P(None, 50001, "hamming"), P(0.5, 0, "euclidean"), P(None, 0, "")):
        with pytest.raises(SemaDBError):
            bad.Validate()


def test_new_knows_the_binary_kind():
    """vectorstore.New (vectorstore.go:47-96): without a GPU the handle cannot be created, but the error must be the
    device's, not "unknown vector store type"; parameter errors come first either way"""
    from semadb_amd import SemaDBError, _lib, vectorstore as vs
    assert vs.QuantizerBinary == "binary"
    with pytest.raises(SemaDBError, match="binary quantizer parameters are nil"):
        vs.New(vs.Quantizer(vs.QuantizerBinary), "cosine", 8)
    with pytest.raises(SemaDBError, match="unknown bit distance function"):
        vs.New(vs.Quantizer(vs.QuantizerBinary, Binary=vs.BinaryQuantizerParameters(None, 0, "cosine")), "cosine", 8)
    with pytest.raises(SemaDBError, match="unknown float32 distance function"):
        vs.New(vs.Quantizer(vs.QuantizerBinary, Binary=vs.BinaryQuantizerParameters(None, 0, "hamming")), "manhattan", 8)
    params = vs.Quantizer(vs.QuantizerBinary, Binary=vs.BinaryQuantizerParameters(0.25, 0, "jaccard"))
    if _lib.device_count() == 0:
        with pytest.raises(SemaDBError) as e:
            vs.New(params, "cosine", 70)
        assert "unknown vector store type" not in str(e.value)
    else:
        bq = vs.New(params, "cosine", 70)
        assert isinstance(bq, vs.BinaryQuantizer) and bq.W == 2 and np.all(bq.threshold() == np.float32(0.25))
        bq.close()
    assert _lib.BIT_METRICS == {"hamming": 3, "jaccard": 4}
