"""The staged hop after its copy-row loads became global loads issued for EVERY hop (walk_stage.h FirstStage::begin).

What that change makes newly reachable, each against the float32 walk (knob 0) on the same index and against the oracle,
bit for bit -- ids, distance bits, counts, n_dist / n_hop / n_edges, visit order:

* one-, two- and three-dword copy rows (d = 128, 256, 384), cosine and dot, the int8 stage (knob 3) and the float16
  stage (knob 1); d = 384 euclidean at knob 1, whose loads stay behind the copy's pointer test;
* 513 queries on the default dispatch (the one-wave walk) and small batches with wide_walk forcing it;
* an array that never fills (60 rows at searchSize 75): rows are requested in every hop and the stage never decides;
* sparse adjacency rows (degree bound 8): most edge positions are kNoSlot and ask for the start node's row instead;
* a table whose capacity is exactly its rows + 1 (the start node's slot): a walk that reaches the last slot reads the
  last copy row of the allocation;
* the audit (knob 4), whose flag is now read at the head of the hop: 0 contradicted decisions, the same answers.

Tables are the oracle's own R = 64 builds of 1 500 rows, built once per (metric, width) and shared."""
import numpy as np
import pytest

from tests import two_precision_model as M
from tests.helpers import bits, start_vector, unit_rows
from tests.test_gpu_two_precision_bound import _index, _same_bits, _walk

pytestmark = pytest.mark.gpu

N_ROWS = 1500
_tables = {}


def _table(oracle, metric, d):
    """(export, oracle index, queries) of one (metric, width), built once"""
    key = (metric, d)
    if key not in _tables:
        seed = 11000 + d * 3 + M.METRICS.index(metric)
        ex = M.full_row_export(oracle, metric, d, N_ROWS, seed)
        _tables[key] = (ex, M.load_oracle(oracle, metric, d, ex), unit_rows(np.random.default_rng(seed + 7), M.N_QUERIES, d))
    return _tables[key]


def _same_answers(a, b, what):
    assert np.array_equal(a[0], b[0]) and _same_bits(a[1], b[1]) and np.array_equal(a[2], b[2]), "%s: answers" % what
    for x, y in ((a[3].n_dist, b[3].n_dist), (a[3].n_hop, b[3].n_hop), (a[3].n_edges, b[3].n_edges)):
        assert np.array_equal(x, y), "%s: counters" % what
    for i in range(a[0].shape[0]):
        k = int(b[3].n_hop[i])
        assert np.array_equal(a[3].visit_ids[i, :k], b[3].visit_ids[i, :k]), "%s query %d: visit order" % (what, i)


def _equals_oracle(ans, o, queries, limit, L, what, first=None):
    ids, d, c, tr = ans
    for i in range(len(queries) if first is None else first):
        o_ids, o_d, o_vis, o_tr = o.search(queries[i], limit, L)
        k = len(o_ids)
        assert int(c[i]) == k, "%s query %d: count" % (what, i)
        assert np.array_equal(ids[i, :k], o_ids), "%s query %d: ids" % (what, i)
        assert np.array_equal(bits(d[i, :k]), bits(o_d)), "%s query %d: distance bits" % (what, i)
        assert (int(tr.n_dist[i]), int(tr.n_hop[i]), int(tr.n_edges[i])) == (o_tr.n_dist, o_tr.n_hop, o_tr.n_edges), "%s query %d: counters" % (what, i)
        assert np.array_equal(tr.visit_ids[i, :o_tr.n_hop], o_vis), "%s query %d: visit order" % (what, i)


def _check(ix, o, queries, limit, L, knobs, what, discards=True, oracle_first=None):
    """knob 0 equals the oracle; every knob of `knobs` equals knob 0, has the copy in use and no contradicted decision"""
    ref, discarded, _, in_use = _walk(ix, queries, limit, L, 0)
    assert not in_use and discarded == 0, what
    _equals_oracle(ref, o, queries, limit, L, what + " knob 0", oracle_first)
    seen = {}
    for knob in knobs:
        ans, discarded, contradicted, in_use = _walk(ix, queries, limit, L, knob)
        msg = "%s knob %d: discarded %d, contradicted %d" % (what, knob, discarded, contradicted)
        print(msg)
        assert in_use and contradicted == 0, msg
        assert (discarded > 0) == discards, msg
        _same_answers(ans, ref, msg)
        _equals_oracle(ans, o, queries, limit, L, msg, oracle_first)
        seen[knob] = (ans, discarded)
    return seen


@pytest.mark.parametrize("metric", ("cosine", "dot"))
@pytest.mark.parametrize("d", (128, 256, 384))
def test_copy_rows_of_one_two_and_three_dwords(oracle, metric, d):
    from semadb_amd import vamana
    ex, o, queries = _table(oracle, metric, d)
    ix = _index(vamana, metric, d, ex)  # (wide_walk = 1: a small batch on the one-wave walk)
    _check(ix, o, queries, 10, 40, (3, 1), "%s d=%d" % (metric, d))
    ix.close()


def test_the_guarded_euclidean_walk(oracle):
    from semadb_amd import vamana
    ex, o, queries = _table(oracle, "euclidean", 384)
    ix = _index(vamana, "euclidean", 384, ex)
    _check(ix, o, queries, 10, 40, (1,), "euclidean d=384")
    ix.close()


def test_513_queries_on_the_default_dispatch(oracle):
    from semadb_amd import vamana
    d = 128
    ex, o, _ = _table(oracle, "cosine", d)
    queries = unit_rows(np.random.default_rng(513), 513, d)
    ix = _index(vamana, "cosine", d, ex, wide_walk=None)
    _check(ix, o, queries, 10, 40, (3, 1), "513 queries", oracle_first=16)
    ix.close()


def test_the_audit_reads_its_flag_at_the_head_of_the_hop(oracle):
    from semadb_amd import vamana
    ex, o, queries = _table(oracle, "cosine", 384)
    ix = _index(vamana, "cosine", 384, ex)
    seen = _check(ix, o, queries, 10, 40, (4, 3, 2, 1), "audit d=384")
    assert seen[4][1] == seen[3][1] and seen[2][1] == seen[1][1], "an audited run discards what the plain run discards"
    ix.close()


def test_an_array_that_never_fills(oracle):
    """60 rows at searchSize 75: every hop asks for its copy rows and no hop's stage decides anything"""
    from semadb_amd import vamana
    d, n = 128, 60
    rng = np.random.default_rng(60)
    o = oracle.Index(d, "cosine", M.R_FULL, M.L_BUILD, 1.2, impl=M.impl_of(oracle))
    o.set_start(start_vector(np.random.default_rng(9), d))
    assert o.insert_rounds(np.arange(2, n + 2, dtype=np.uint64), unit_rows(rng, n, d)) == 0
    ix = _index(vamana, "cosine", d, o.export())
    _check(ix, o, unit_rows(rng, M.N_QUERIES, d), 10, 75, (3, 1, 4), "60 rows", discards=False)
    ix.close()


def test_sparse_adjacency_rows(oracle):
    """degree bound 8: most of a row's 64 positions hold no edge and ask for the start node's copy row"""
    from semadb_amd import vamana
    d, n = 256, N_ROWS
    rng = np.random.default_rng(8)
    o = oracle.Index(d, "cosine", 8, M.L_BUILD, 1.2, impl=M.impl_of(oracle))
    o.set_start(start_vector(np.random.default_rng(9), d))
    assert o.insert_rounds(np.arange(2, n + 2, dtype=np.uint64), unit_rows(rng, n, d)) == 0
    ex = o.export()
    assert np.diff(ex[2].astype(np.int64)).max() <= 8
    ix = _index(vamana, "cosine", d, ex)
    _check(ix, o, unit_rows(rng, M.N_QUERIES, d), 10, 40, (3, 1), "degree bound 8")
    ix.close()


@pytest.mark.parametrize("knob", (3, 1))
def test_the_last_copy_row_of_an_exact_allocation(oracle, knob):
    """capacity = rows + 1, i.e. exactly the slots the table holds: the export's len(ids) counts the start node (slot 0)
    beside the rows, and a table created with that capacity reserves nothing more, so the last slot's copy row ends where
    the copy's allocation ends.  The walk expands that slot and its answers are the oracle's.  (What this shows is that
    the last row is read and read right; a device allocation is rounded up, so a read past it would not fault here.)"""
    from semadb_amd import vamana
    d = 384
    ex, o, queries = _table(oracle, "cosine", d)
    ids, vecs = ex[0], ex[1]
    params = vamana.IndexVectorVamanaParameters(d, "cosine", M.L_BUILD, M.R_FULL, 1.2)
    ix = vamana.NewIndexVamana("t", params, capacity=len(ids), strict=False)
    ix.set_tuning("wide_walk", 1)
    ix.load(*ex)
    # (the last row itself and its neighbourhood as queries: the walk ends at the last slot)
    q = np.vstack([vecs[-1:], queries[:7]]).astype(np.float32)
    seen = _check(ix, o, q, 10, 40, (knob,), "capacity = rows + 1, knob %d" % knob)
    tr = seen[knob][0][3]
    assert int(ids[-1]) in tr.visit_ids[0, :int(tr.n_hop[0])].tolist(), "the walk never expanded the last slot"
    ix.close()
