"""The device tables grow while two graph versions differ.  Inside an open transaction `reserve` has to carry both copies
of the graph, the dirty-row flags, the code rows and the neighbours' code rows into the new tables and hand the searches
the committed copy's new pointers without ending the transaction: the searches go on answering from the committed
graph, an abort still finds what to restore, a commit still knows which rows it wrote.  The shapes are the smallest at
which that happens: an index created with 16 rows (the ABI's minimum) that a transaction takes to 128."""
import numpy as np
import pytest

from tests import binary_model as bm
from tests.helpers import assert_same_graph, bits, build_oracle_index, start_vector, unit_rows

pytestmark = pytest.mark.gpu

R, L, K, NQ = 8, 20, 5, 8


def _same_topology(g, o):
    g_ids, _, g_off, g_e = g.export()
    o_ids, _, o_off, o_e = o.export(with_vectors=False)
    assert np.array_equal(g_ids, o_ids)
    assert np.array_equal(g_off, o_off), "degree sequence differs"
    assert np.array_equal(g_e, o_e), "edge lists differ"


class _Pair:
    """a device index and the oracle that is given the same writes; orow / oq: what the oracle stores / is asked for a
    float row / query (a binary store's oracle holds the 0/1 expansion of the code rows)"""

    def __init__(self, ix, o, q, orow=lambda x: x, same_graph=assert_same_graph, walks=False):
        self.ix, self.o, self.q, self.orow, self.same_graph, self.walks = ix, o, q, orow, same_graph, walks
        self.oq = orow(q)

    def answers(self, tag, filters=None):
        """the device's answers are the oracle's: ids and distance bits; walks: hops, evaluations and visit order too"""
        g_ids, g_d, g_c, tr = self.ix.search_batch(self.q, K, L, filters=filters, trace=True, visit_cap=512)
        for i in range(len(self.q)):
            o_ids, o_d, o_vis, o_tr = self.o.search(self.oq[i], K, L, filter_ids=sorted(filters[i]) if filters else None)
            assert int(g_c[i]) == len(o_ids), tag
            assert np.array_equal(g_ids[i, :len(o_ids)], o_ids), tag
            assert np.array_equal(bits(g_d[i, :len(o_ids)]), bits(o_d)), tag
            if self.walks:
                assert int(tr.n_hop[i]) == o_tr.n_hop and int(tr.n_dist[i]) == o_tr.n_dist, tag
                assert np.array_equal(tr.visit_ids[i, :o_tr.n_hop], o_vis), tag
        return g_ids, g_d, g_c

    def insert(self, ids, rows):
        """the oracle-checked insert path: one point per round is the oracle's loop"""
        self.ix.insert_batch(ids, rows, round_size=1)

    def oracle_insert(self, ids, rows):
        orows = self.orow(rows)
        for i in range(len(ids)):
            assert self.o.insert(int(ids[i]), orows[i]) == 0


def _grow_inside_a_transaction(p, committed_ids, new_ids, new_rows, more_ids, more_rows, rng):
    """p: a committed table that is nearly full.  new_*: the 60 rows whose insert makes the tables grow inside the
    transaction; more_*: rows that make them grow again outside one."""
    ix, o = p.ix, p.o
    assert ix.version_diff() == 0
    p.same_graph(ix, o)
    snap, stats0, usage0, size0 = ix.export(), ix.stats(), ix.row_usage(), ix.SizeInMemory()
    pre = p.answers("committed")
    gone = rng.choice(committed_ids, 5, replace=False).astype(np.uint64)
    named = [set(int(v) for v in rng.choice(committed_ids, 6, replace=False)) | {int(gone[0]), int(new_ids[i])} for i in range(NQ)]

    def writes():
        ix.begin_write()
        p.insert(new_ids, new_rows)
        ix.delete_batch(gone)

    for attempt in range(2):  # twice: the second transaction starts from grown tables
        writes()
        if attempt == 0:
            assert ix.SizeInMemory() > size0, "the case must make the tables grow inside the transaction"
        assert ix.row_usage()[0] == usage0[0] + len(new_ids)
        assert ix.version_diff() > 0
        p.answers("inside the open transaction")  # the oracle still holds the committed graph
        p.answers("inside the open transaction, filtered", named)
        assert ix.abort_write() is True
        again = ix.export()
        for a, b in zip(snap, again):
            assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()
        assert ix.version_diff() == 0
        assert ix.stats() == stats0 and ix.row_usage() == usage0
        got = p.answers("after the abort")
        for a, b in zip(got, pre):
            assert a.tobytes() == b.tobytes()
        p.answers("after the abort, filtered", named)
    # the same writes for real, on both sides
    writes()
    ix.commit()
    p.oracle_insert(new_ids, new_rows)
    assert o.delete(gone) == 0
    assert ix.version_diff() == 0
    p.same_graph(ix, o)
    p.answers("committed after growth")
    p.answers("committed after growth, filtered", named)
    # and growth outside a transaction
    size1 = ix.SizeInMemory()
    p.insert(more_ids, more_rows)
    p.oracle_insert(more_ids, more_rows)
    assert ix.SizeInMemory() > size1, "the case must make the tables grow again"
    assert ix.version_diff() == 0
    p.same_graph(ix, o)
    p.answers("after the second growth")


def _impl(oracle):
    return oracle.IMPL_AVX2 if oracle.has_avx2() else oracle.IMPL_ASM


def _small_table(oracle, metric, d, rng, quantizer=None, orow=lambda x: x, **pair):
    """an index of 16 rows that holds the start node and 10 committed rows, and its oracle"""
    from semadb_amd import vamana
    sv = start_vector(np.random.default_rng(5), d)
    rows = unit_rows(rng, 10 + 60 + 70, d)
    ids = np.arange(2, 2 + len(rows), dtype=np.uint64)
    o = oracle.Index(d, metric, R, L, 1.2, impl=_impl(oracle))
    kw = {} if quantizer is None else {"Quantizer": quantizer}
    ix = vamana.NewIndexVamana("grow", vamana.IndexVectorVamanaParameters(d, metric, L, R, 1.2, **kw), strict=False, capacity=16)
    ix.set_start(sv)
    o.set_start(orow(sv[None, :])[0])
    p = _Pair(ix, o, unit_rows(rng, NQ, d), orow=orow, **pair)
    p.insert(ids[:10], rows[:10])
    p.oracle_insert(ids[:10], rows[:10])
    return p, ids, rows


def test_plain_rows_grow_inside_a_transaction(oracle):
    """cosine rows of 32 floats, the first-stage copy of the rows at its default: it follows the growth (a search of the
    committed graph must not read a copy that ends at the old capacity)"""
    rng = np.random.default_rng(1601)
    p, ids, rows = _small_table(oracle, "cosine", 32, rng)
    _grow_inside_a_transaction(p, ids[:10], ids[10:70], rows[10:70], ids[70:], rows[70:], rng)  # 16 -> 128 -> 256 rows
    p.ix.close()


def test_bit_codes_grow_inside_a_transaction(oracle):
    """a binary quantizer with a given threshold: the code rows of both old and new points travel with the tables; the
    oracle walks the 0/1 expansion of the code rows (hamming = squared euclidean there)"""
    from semadb_amd import vectorstore as vs
    d = 64
    rng = np.random.default_rng(1602)
    thr = np.full(d, 0.02, np.float32)
    p, ids, rows = _small_table(oracle, "euclidean", d, rng, orow=lambda x: bm.expand(bm.encode(x, thr), d), same_graph=_same_topology,
                                quantizer=vs.Quantizer(vs.QuantizerBinary, Binary=vs.BinaryQuantizerParameters(0.02, 0, "hamming")))
    assert p.ix._bq is p.ix._store and np.array_equal(bits(p.ix._store.threshold()), bits(thr))
    _grow_inside_a_transaction(p, ids[:10], ids[10:70], rows[10:70], ids[70:], rows[70:], rng)
    live = p.ix.export()[0]
    assert np.array_equal(vs.get_bit_codes(p.ix, live[1:]), bm.encode(rows[live[1:].astype(np.int64) - 2], thr))
    p.ix.close()


def test_neighbour_code_rows_grow_inside_a_transaction(oracle):
    """a product quantizer small enough (M = 32) for the neighbours' code rows behind both adjacency copies: fitted on a
    table large enough to train, loaded with four rows to spare, grown by the transaction.  The walks are the oracle's:
    ids, distance bits, hops, evaluations, visit order."""
    from semadb_amd import vamana, vectorstore as vs
    metric, d, M, Kc, n0 = "euclidean", 64, 32, 16, 200
    rng = np.random.default_rng(1603)
    base = unit_rows(rng, n0 + 60 + 220, d)
    o = build_oracle_index(oracle, base[:n0], metric, R=R, L=L)
    ids, vecs, off, edges = o.export()
    train = vecs[1:161].copy()
    first = rng.integers(0, 160, M)
    opq = oracle.PQ(d, metric, M, Kc)
    opq.fit(train.copy(), first, alias=True)
    assert o.attach_pq(opq, np.stack([opq.encode(v) for v in vecs])) == 0
    ix = vamana.NewIndexVamana("growpq", vamana.IndexVectorVamanaParameters(d, metric, L, R, 1.2), strict=False, capacity=len(ids) + 4)
    ix.load(ids, vecs, off, edges)
    gpq = vs.ProductQuantizer(metric, vs.ProductQuantizerParameters(Kc, M), d)
    gpq.Fit(train.copy(), first, alias=True)
    vs.attach(ix, gpq)
    p = _Pair(ix, o, unit_rows(rng, NQ, d), walks=True)
    all_ids = np.arange(2, 2 + len(base), dtype=np.uint64)
    _grow_inside_a_transaction(p, all_ids[:n0], all_ids[n0:n0 + 60], base[n0:n0 + 60], all_ids[n0 + 60:], base[n0 + 60:], rng)  # 205 -> 410 -> 820 rows
    live = ix.export()[0]
    assert np.array_equal(vs.get_codes(ix, live), np.stack([opq.encode(v) for v in ix.export()[1]]))
    ix.close()
    gpq.close()


def test_overflow_list_survives_growth_and_compaction(oracle):
    """the start node's overflow list (made as tests/test_gpu_delete.py::test_start_node_overflow_list makes it) while the
    tables grow inside a transaction, and through the compaction behind it: both copies of the list are carried, and
    the walks that expand it are the oracle's"""
    from semadb_amd import vamana
    metric, d, n, Rs = "euclidean", 16, 900, 5
    rng = np.random.default_rng(n + Rs)
    sv = start_vector(np.random.default_rng(5), d)
    base = unit_rows(rng, n, d)
    base = base[rng.integers(0, n // 3, n)].copy()  # repeated points: zero distances and ties on top
    o = oracle.Index(d, metric, Rs, L, 1.5, impl=_impl(oracle))
    o.set_start(sv)
    ids = np.arange(2, n + 2, dtype=np.uint64)
    for i in range(n):
        assert o.insert(int(ids[i]), base[i]) == 0
    e_ids, e_v, e_off, e_e = o.export()
    g = vamana.NewIndexVamana("ovfgrow", vamana.IndexVectorVamanaParameters(d, metric, L, Rs, 1.5), strict=False, capacity=n + 1 + 4)
    g.load(e_ids, e_v, e_off, e_e)
    p = _Pair(g, o, unit_rows(rng, 16, d), walks=True)

    def start_degree():
        x_ids, _, off, _ = o.export(with_vectors=False)
        assert x_ids[0] == 1
        return int(off[1] - off[0])

    dels = rng.choice(ids, size=n // 8, replace=False).astype(np.uint64)
    g.delete_batch(dels)
    assert o.delete(dels) == 0
    assert start_degree() > 64 + 64, "the case must overflow the row by more than one chunk (%d)" % start_degree()
    assert_same_graph(g, o)
    pre = p.answers("overflowing")
    # growth inside a transaction, the list in place: searches read the committed copy of it from the new tables' view
    size0 = g.SizeInMemory()
    far = (-base[:8] + 0.05 * unit_rows(rng, 8, d)).astype(np.float32)
    far_ids = np.arange(n + 2, n + 10, dtype=np.uint64)
    g.begin_write()
    p.insert(far_ids, far)
    assert g.SizeInMemory() > size0, "the case must make the tables grow"
    got = p.answers("inside the open transaction")
    for a, b in zip(got, pre):
        assert a.tobytes() == b.tobytes()
    g.commit()
    p.oracle_insert(far_ids, far)
    assert start_degree() > 64, "the list must outlive the inserts (%d)" % start_degree()
    assert g.version_diff() == 0
    assert_same_graph(g, o)
    p.answers("grown")
    g.compact()
    assert g.version_diff() == 0
    assert g.row_usage()[1] == 0
    assert_same_graph(g, o)
    p.answers("compacted")
    g.close()
