"""The staged hop after its copy-row addresses and its transposing butterfly changed (walk_stage.h).

FirstStage::begin takes the slot of pair u with one ds_bpermute of the lane's edge (lane 2u in lanes 0..31, lane 2u + 1
in lanes 32..63) where it had two readlanes and a select; edge_sums exchanges through v_permlane16_swap and DPP adds
where it went through ds_swizzle.  Neither shows in an answer unless it is wrong: a wrong source lane reads another
edge's copy row, a wrong exchange adds another edge's partial sum, and either moves the first stage's distance of some
edge -- the discarded count leaves the model's sandwich (tests/int8_stage_model.py: lower <= device <= upper, within
2 % of each other), or a needed neighbour is discarded and the answers, counters or visit order differ from the float32
walk (knob 0) and the oracle, or the audit (knob 4) finds a contradicted decision.  Every case asserts all of these,
bit for bit, through test_gpu_int8_stage.py's _sandwich8 (int8 stage) or test_gpu_two_precision_bound.py's _sandwich
(float16 stage).

Shapes: 2 000 rows, d = 128 / 256 / 384 (one, two and three dwords per lane and copy row), cosine and dot, searchSize 75
and 96, 64 and 513 queries.  Then what the address change can get wrong -- edges that point at the table's last slot, a
capacity far above the rows, nodes with fewer than 64 edges (kNoSlot replaced by the start slot), a table of fewer than
64 rows -- and walks whose array holds no unvisited entry (searchSize 1 and 2), duplicate rows, NaN / Inf queries, a
start node with an overflow list, queries far from every row.  Tables are built once per (metric, width) and shared."""
import numpy as np
import pytest

from tests import int8_stage_model as M8
from tests import two_precision_model as M
from tests.helpers import start_vector, unit_rows
from tests.test_gpu_int8_stage import _sandwich8
from tests.test_gpu_two_precision_bound import _index, _sandwich

pytestmark = pytest.mark.gpu

N_ROWS = 2000
_tables = {}


def _table(oracle, metric, d):
    """(export, graph, oracle index, copy, 513 queries) of one (metric, width), built once"""
    key = (metric, d)
    if key not in _tables:
        seed = 21000 + d * 3 + M.METRICS.index(metric)
        ex = M.full_row_export(oracle, metric, d, N_ROWS, seed)
        g = M8.Graph(*ex)
        _tables[key] = (ex, g, M.load_oracle(oracle, metric, d, ex), M8.Copy8(g.vecs), unit_rows(np.random.default_rng(seed + 7), 513, d))
    return _tables[key]


def _built(oracle, metric, d, base, R=64, L=M.L_BUILD):
    """the oracle's own build over `base`: (export, graph, oracle index)"""
    o = oracle.Index(d, metric, R, L, 1.2, impl=M.impl_of(oracle))
    o.set_start(start_vector(np.random.default_rng(9), d))
    assert o.insert_rounds(np.arange(2, base.shape[0] + 2, dtype=np.uint64), base) == 0
    ex = o.export()
    return ex, M8.Graph(*ex), o


@pytest.mark.parametrize("metric", ("cosine", "dot"))
@pytest.mark.parametrize("d", (128, 256, 384))
def test_every_copy_row_width_both_search_sizes_64_queries(oracle, metric, d):
    from semadb_amd import vamana
    ex, g, o, copy, queries = _table(oracle, metric, d)
    ix = _index(vamana, metric, d, ex)
    for L in (75, 96):
        _sandwich8(ix, oracle, o, g, metric, queries[:64], 10, L, "%s d=%d L=%d" % (metric, d, L), copy, expect="some")
    ix.close()


@pytest.mark.parametrize("d", (128, 256, 384))
def test_513_queries_on_the_default_dispatch(oracle, d):
    from semadb_amd import vamana
    ex, g, o, copy, queries = _table(oracle, "cosine", d)
    ix = _index(vamana, "cosine", d, ex, wide_walk=None)
    t, discarded = _sandwich8(ix, oracle, None, g, "cosine", queries, 10, 75, "513 queries d=%d" % d, copy)
    assert t.lower > 0 and discarded > 0
    ix.close()


@pytest.mark.parametrize("metric", ("cosine", "euclidean"))
def test_the_float16_stage_takes_the_same_addresses_and_butterfly(oracle, metric):
    from semadb_amd import vamana
    d = 384
    seed = 21000 + d * 3 + M.METRICS.index(metric)
    if metric == "cosine":
        ex, _, o, _, queries = _table(oracle, metric, d)
    else:
        ex = M.full_row_export(oracle, metric, d, N_ROWS, seed)
        o, queries = M.load_oracle(oracle, metric, d, ex), unit_rows(np.random.default_rng(seed + 7), 64, d)
    ix = _index(vamana, metric, d, ex)
    _sandwich(ix, oracle, o, M.Graph(*ex), metric, queries[:64], 10, 75, "float16 stage %s" % metric, expect="some")
    ix.close()


def test_edges_that_point_at_the_last_slot_of_an_exact_allocation(oracle):
    """capacity = the table's slots exactly: the last slot's copy row ends where the copy ends.  Queries at and around
    the last row: its slot is an edge of many rows the walk expands (a pair's source lane read wrong would ask for
    another row; the count and the answers say so) and is expanded itself."""
    from semadb_amd import vamana
    d = 384
    ex, g, o, copy, queries = _table(oracle, "cosine", d)
    params = vamana.IndexVectorVamanaParameters(d, "cosine", M.L_BUILD, M.R_FULL, 1.2)
    ix = vamana.NewIndexVamana("t", params, capacity=len(ex[0]), strict=False)
    ix.set_tuning("wide_walk", 1)
    ix.load(*ex)
    near = ex[1][-1:] + np.float32(0.05) * unit_rows(np.random.default_rng(4), 15, d)
    q = np.vstack([ex[1][-1:], near, queries[:16]]).astype(np.float32)
    _sandwich8(ix, oracle, o, g, "cosine", q, 10, 75, "capacity = rows + 1", copy, expect="some")
    ans = ix.search_batch(q, 10, 75, trace=True, visit_cap=1024)
    assert int(ex[0][-1]) in ans[3].visit_ids[0, :int(ans[3].n_hop[0])].tolist(), "the walk never expanded the last slot"
    ix.close()


def test_a_capacity_far_above_the_rows(oracle):
    from semadb_amd import vamana
    d = 256
    ex, g, o, copy, queries = _table(oracle, "dot", d)
    params = vamana.IndexVectorVamanaParameters(d, "dot", M.L_BUILD, M.R_FULL, 1.2)
    ix = vamana.NewIndexVamana("t", params, capacity=1 << 20, strict=False)
    ix.set_tuning("wide_walk", 1)
    ix.load(*ex)
    _sandwich8(ix, oracle, o, g, "dot", queries[:32], 10, 75, "capacity 2^20", copy, expect="some")
    ix.close()


@pytest.mark.parametrize("R", (8, 33))
def test_rows_of_fewer_than_64_edges(oracle, R):
    """degree bound 8 / 33: the edge positions behind a row's edges hold kNoSlot and ask for the start slot's copy row;
    33 leaves pair 16 with an edge in its low half and none in its high half"""
    from semadb_amd import vamana
    d = 384
    rng = np.random.default_rng(80 + R)
    ex, g, o = _built(oracle, "cosine", d, unit_rows(rng, N_ROWS, d), R=R)
    assert np.diff(ex[2].astype(np.int64)).max() <= R
    ix = _index(vamana, "cosine", d, ex)
    t, discarded = _sandwich8(ix, oracle, o, g, "cosine", unit_rows(rng, 32, d), 10, 75, "degree bound %d" % R)
    assert t.lower > 0 and discarded > 0
    ix.close()


def test_a_table_of_fewer_than_64_rows(oracle):
    """40 rows at searchSize 75: copy rows are asked for in every hop, the array never fills, nothing is discarded"""
    from semadb_amd import vamana
    d = 128
    rng = np.random.default_rng(40)
    ex, g, o = _built(oracle, "cosine", d, unit_rows(rng, 40, d))
    ix = _index(vamana, "cosine", d, ex)
    _sandwich8(ix, oracle, o, g, "cosine", unit_rows(rng, 32, d), 10, 75, "40 rows", expect="none")
    ix.close()


def test_search_sizes_1_and_2(oracle):
    """the array is full from the first hop and mostly holds no unvisited entry; every hop's stage decides"""
    from semadb_amd import vamana
    d = 384
    ex, g, o, copy, queries = _table(oracle, "cosine", d)
    ix = _index(vamana, "cosine", d, ex)
    for L in (1, 2):
        _sandwich8(ix, oracle, o, g, "cosine", queries[:64], 1, L, "L=%d" % L, copy, expect="some")
    ix.close()


def test_duplicate_rows(oracle):
    """every row four times: new points tie with each other and with the entry first in line, in every hop"""
    from semadb_amd import vamana
    d = 128
    rng = np.random.default_rng(44)
    base = np.tile(unit_rows(rng, N_ROWS // 4, d), (4, 1))
    ex, g, o = _built(oracle, "cosine", d, base)
    ix = _index(vamana, "cosine", d, ex)
    q = np.vstack([unit_rows(rng, 24, d), base[:8]]).astype(np.float32)
    for L in (75, 96):
        _sandwich8(ix, oracle, o, g, "cosine", q, 10, L, "duplicate rows L=%d" % L)
    ix.close()


@pytest.mark.parametrize("metric", ("cosine", "dot"))
def test_nan_inf_and_far_queries(oracle, metric):
    from semadb_amd import vamana
    d = 384
    ex, g, o, copy, queries = _table(oracle, metric, d)
    ix = _index(vamana, metric, d, ex)
    for kind in ("nan", "inf"):
        _sandwich8(ix, oracle, o, g, metric, M.hostile_queries(d, kind), 10, 75, "%s %s queries" % (metric, kind), copy, expect="none")
    # far from every row: the negated mean direction of the rows, so every hop's nearest new point is a poor one
    far = -ex[1][1:].mean(axis=0, keepdims=True) + np.float32(0.02) * unit_rows(np.random.default_rng(5), 16, d)
    far = (far / np.linalg.norm(far, axis=1, keepdims=True)).astype(np.float32)
    _sandwich8(ix, oracle, o, g, metric, far, 10, 75, "%s far queries" % metric, copy)
    ix.close()


def test_a_start_node_with_an_overflow_list(oracle):
    from semadb_amd import vamana
    ex, queries = M.overflow_case(oracle, "cosine")
    g = M8.Graph(*ex)
    assert g.deg[g.start] > 64 + 64
    o = M.load_oracle(oracle, "cosine", 128, ex)
    ix = _index(vamana, "cosine", 128, ex)
    for L, limit in ((2, 1), (75, 10)):
        _sandwich8(ix, oracle, o, g, "cosine", queries, limit, L, "overflow list L=%d" % L)
    ix.close()
