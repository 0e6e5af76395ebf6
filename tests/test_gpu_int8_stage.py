"""The int8 first stage of the two-precision hop (SDB_TUNE_SKETCH = 3, audited: 4) between two independent counts.

tests/int8_stage_model.py restates the copy, the two-term query, the exact integer sum and the bound in float64 and
counts, over the oracle's walk, the neighbours the pure bound proves discardable (`upper`) and those it still proves with
every inflation the kernel documents charged generously (`lower`; test_int8_stage_model.py pins lower >= 0.98 upper,
measured 0.999+).  Every case asserts: answers, distance bits, counters and visit order equal the replay (which equals the
oracle), no discard contradicted, lower <= discarded on the device <= upper, and knob 3's answers equal knob 1's and
knob 0's bit for bit.  Adjacency rows are full (R = 64), so all 32 pairs of the butterfly carry an edge."""
import threading

import numpy as np
import pytest

from tests import int8_stage_model as M8
from tests import two_precision_model as M
from tests.helpers import bits, start_vector, unit_rows
from tests.test_gpu_two_precision_bound import _equals_replay, _index, _oracle_equals_replay, _same_bits, _walk

pytestmark = pytest.mark.gpu

METRICS8 = ("cosine", "dot")
WIDTHS8 = (32, 96, 128, 256, 352, 384)


def _ld(d):
    return (d + 127) // 128 * 128


def _same_answers(a, b, what):
    """(ids, dists, counts, trace) of two calls: bit for bit, visit logs up to n_hop"""
    assert np.array_equal(a[0], b[0]) and _same_bits(a[1], b[1]) and np.array_equal(a[2], b[2]), "%s: answers" % what
    for x, y in ((a[3].n_dist, b[3].n_dist), (a[3].n_hop, b[3].n_hop), (a[3].n_edges, b[3].n_edges)):
        assert np.array_equal(x, y), "%s: counters" % what
    for i in range(a[0].shape[0]):
        k = int(b[3].n_hop[i])
        assert np.array_equal(a[3].visit_ids[i, :k], b[3].visit_ids[i, :k]), "%s query %d: visit order" % (what, i)


def _sandwich8(ix, oracle, o, g, metric, queries, limit, L, what, copy=None, expect=None, model="int8"):
    """audit run (4) and plain run (3) of one batch against the model; then knobs 1 and 0 on the same index.
    expect: "none" -- nothing may be discarded; "some" -- lower > 0 and within 2 % of upper; "none or inside".
    model "float16": the table was refused the int8 copy, the sandwich is the float16 stage's."""
    if model == "int8":
        reps, t, _, _ = M8.run_model8(oracle, g, metric, queries, limit, L, copy)
    else:
        reps, t, _ = M.run_model(oracle, g, metric, queries, limit, L)
    if o is not None:
        _oracle_equals_replay(o, reps, queries, limit, L)
    seen, ans3 = [], None
    for mode in (4, 3):
        ans, discarded, contradicted, in_use = _walk(ix, queries, limit, L, mode)
        msg = "%s sketch=%d: lower %d / discarded on the device %d / upper %d (discardable %d of %d; contradicted %d)" % (
            what, mode, t.lower, discarded, t.upper, t.discardable, t.full, contradicted)
        print(msg)
        assert in_use, msg
        _equals_replay(ans, reps, what)
        assert contradicted == 0, msg
        if expect == "none or inside":  # a hostile input: the device may find its bound infinite where float64 does not
            assert discarded == 0 or t.lower <= discarded <= t.upper, msg
        else:
            assert t.lower <= discarded <= t.upper, msg
        if expect == "none":
            assert discarded == 0, msg
        if expect == "some":
            assert t.lower > 0 and t.lower >= 0.98 * t.upper, msg
        seen.append(discarded)
        ans3 = ans
    assert seen[0] == seen[1], "%s: the audit run discarded %d, the plain run %d" % (what, seen[0], seen[1])
    for mode in (1, 0):
        ans, _, contradicted, _ = _walk(ix, queries, limit, L, mode)
        assert contradicted == 0
        _same_answers(ans3, ans, "%s: knob 3 against knob %d" % (what, mode))
    ix.set_tuning("sketch", 3)
    return t, seen[1]


@pytest.mark.parametrize("metric", METRICS8)
@pytest.mark.parametrize("d", WIDTHS8)
def test_full_rows_every_width(oracle, metric, d):
    from semadb_amd import vamana
    ex, queries, limit, L = M.width_case(oracle, metric, d)
    g = M8.Graph(*ex)
    o = M.load_oracle(oracle, metric, d, ex)
    ix = _index(vamana, metric, d, ex)
    t, _ = _sandwich8(ix, oracle, o, g, metric, queries, limit, L, "%s d=%d" % (metric, d), expect="some")
    assert t.expanded_full_rows >= 0.9 * t.expanded, "%d of %d expanded nodes have 64 edges" % (t.expanded_full_rows, t.expanded)
    ix.close()


@pytest.mark.parametrize("metric", METRICS8)
def test_search_sizes_hostile_queries_and_a_query_equal_to_a_row(oracle, metric):
    from semadb_amd import vamana
    d = 384
    ex, queries = M.l_case(oracle, metric, d)
    g = M8.Graph(*ex)
    o = M.load_oracle(oracle, metric, d, ex)
    ix = _index(vamana, metric, d, ex)
    copy = M8.Copy8(g.vecs)
    for L, limit in ((1, 1), (2, 1), (10, 10), (75, 10), (96, 10)):
        _sandwich8(ix, oracle, o, g, metric, queries, limit, L, "%s L=%d limit=%d" % (metric, L, limit), copy, expect="some")
    for kind in ("nan", "inf"):
        _sandwich8(ix, oracle, o, g, metric, M.hostile_queries(d, kind), 10, 40, "%s %s queries" % (metric, kind), copy, expect="none")
    for kind in M.HOSTILE_SANDWICH + ("overflow",):
        _sandwich8(ix, oracle, o, g, metric, M.hostile_queries(d, kind), 10, 40, "%s %s queries" % (metric, kind), copy)
    big = unit_rows(np.random.default_rng(3), 8, d) * np.float32(1e30)
    # (||q||^2 overflows float32: the wave measures an infinite norm and discards nothing; the model's float64 does not)
    _sandwich8(ix, oracle, o, g, metric, big, 10, 40, "%s 1e30 queries" % metric, copy, expect="none or inside")
    _sandwich8(ix, oracle, o, g, metric, np.ascontiguousarray(g.vecs[5:37]), 10, 40, "%s queries equal to rows" % metric, copy, expect="some")
    ix.close()


@pytest.mark.parametrize("metric", METRICS8)
def test_start_node_with_an_overflow_list(oracle, metric):
    from semadb_amd import vamana
    ex, queries = M.overflow_case(oracle, metric)
    g = M8.Graph(*ex)
    assert g.deg[g.start] > 64 + 64
    o = M.load_oracle(oracle, metric, 128, ex)
    ix = _index(vamana, metric, 128, ex)
    for L in (1, 2):
        _sandwich8(ix, oracle, o, g, metric, queries, 1, L, "%s overflow list L=%d" % (metric, L), expect="some")
    ix.close()


def test_default_dispatch_513_queries(oracle):
    """wide_walk at its default: 512 queries stay on the many-waves kernel (no first stage), 513 take the one-wave walk"""
    from semadb_amd import vamana
    d = 128
    ex, queries = M.dispatch_case(oracle, d)
    g = M8.Graph(*ex)
    o = M.load_oracle(oracle, "cosine", d, ex)
    ix = _index(vamana, "cosine", d, ex, wide_walk=None)
    reps, t, _, _ = M8.run_model8(oracle, g, "cosine", queries, 10, 40)
    _oracle_equals_replay(o, reps[:32], queries[:32], 10, 40)
    for mode in (4, 3):
        ix.set_tuning("sketch", mode)
        ans, discarded, contradicted, in_use = _walk(ix, queries[:512], 10, 40, None)
        assert in_use and discarded == 0 and contradicted == 0
        _equals_replay(ans, reps[:512], "512 queries")
        ans, discarded, contradicted, in_use = _walk(ix, queries, 10, 40, None)
        msg = "513 queries sketch=%d: lower %d / discarded on the device %d / upper %d" % (mode, t.lower, discarded, t.upper)
        print(msg)
        _equals_replay(ans, reps, msg)
        assert in_use and contradicted == 0 and t.lower > 0 and t.lower <= discarded <= t.upper, msg
    ix.close()


def _loaded(vamana, oracle, metric, d, base, R=64, L=M.L_BUILD):
    """an oracle-built graph over `base` (any rows), loaded; (ix, o, g)"""
    o = oracle.Index(d, metric, R, L, 1.2, impl=M.impl_of(oracle))
    o.set_start(start_vector(np.random.default_rng(9), d))
    assert o.insert_rounds(np.arange(2, base.shape[0] + 2, dtype=np.uint64), base) == 0
    ex = o.export()
    return _index(vamana, metric, d, ex), o, M8.Graph(*ex)


@pytest.mark.parametrize("kind", ["zero row", "zeros only", "nan", "inf", "1e30", "norms 1e-3 .. 1e3", "near ties"])
def test_hostile_tables(oracle, kind):
    from semadb_amd import vamana
    d, n = 128, 1500
    rng = np.random.default_rng(40 + len(kind))
    base = unit_rows(rng, n, d)
    metric, expect, model = "cosine", "some", "int8"
    if kind == "zero row":
        base[7] = 0.0
    elif kind == "zeros only":
        base[:] = 0.0
        expect = None
    elif kind in ("nan", "inf", "1e30"):
        base[11, 5] = {"nan": np.nan, "inf": np.inf, "1e30": 1e30}[kind]
        expect = "none"
        model = "float16" if kind != "1e30" else "int8"  # (a NaN or Inf row: refused the int8 copy; the float16 bound is NaN / Inf too)
    elif kind == "norms 1e-3 .. 1e3":
        metric, expect, model = "dot", None, "float16"
        base *= (10.0 ** rng.uniform(-3, 3, (n, 1))).astype(np.float32)
    elif kind == "near ties":  # clusters of rows within 1e-3 of each other: distances crowd around the threshold
        centres = unit_rows(rng, 30, d)
        base = centres[rng.integers(0, 30, n)] + np.float32(1e-3) * unit_rows(rng, n, d)
        base = (base / np.linalg.norm(base, axis=1, keepdims=True)).astype(np.float32)
        expect = None
    ix, o, g = _loaded(vamana, oracle, metric, d, base)
    copy = M8.Copy8(g.vecs)
    assert copy.refused() == (model == "float16" or kind == "1e30"), kind
    if kind == "1e30":
        model = "float16"  # (every other row quantises to nothing: refused; the float16 copy overflows: nothing discarded)
    queries = np.vstack([unit_rows(rng, 28, d), base[:4]]).astype(np.float32)
    _sandwich8(ix, oracle, None if kind in ("nan", "inf") else o, g, metric, queries, 10, 40, kind, copy, expect=expect, model=model)
    # which copy the table holds: knob 0 frees it, rows of ld bytes (int8) or of 2 ld + 4 (float16)
    before = ix.SizeInMemory()
    ix.set_tuning("sketch", 0)
    freed, row = before - ix.SizeInMemory(), _ld(d) if model == "int8" else _ld(d) * 2 + 4
    assert freed == 2048 * row, (kind, freed)  # (1 501 rows: a capacity of 2 048)
    ix.close()


def _twins(vamana, metric, d, ex, capacity):
    params = vamana.IndexVectorVamanaParameters(d, metric, M.L_BUILD, M.R_FULL, 1.2)
    out = []
    for knob in (None, 0):  # the default (3) and the float32 walk
        ix = vamana.NewIndexVamana("t", params, capacity=capacity, strict=False)
        ix.set_tuning("wide_walk", 1)
        if knob is not None:
            ix.set_tuning("sketch", knob)
        ix.load(*ex)
        out.append(ix)
    return out


@pytest.mark.parametrize("metric", METRICS8)
def test_write_paths_against_a_twin_on_knob_0(oracle, metric):
    """after every step the copy is in use, the count is inside the sandwich of the model's copy (scale and maxima carried
    as the index carries them) and the answers equal the float32 twin's"""
    from semadb_amd import vamana
    d, L, limit = 128, 40, 10
    ex, queries = M.l_case(oracle, metric, d)
    ix, twin = _twins(vamana, metric, d, ex, 2048)
    rng = np.random.default_rng(62)
    state = {"next": 5000, "copy": M8.Copy8(ex[1]), "update": 100, "all": np.asarray(ex[1], dtype=np.float32)}

    def appended(rows):
        """the model of build_sketch_kind: rows inside the range take the scale and raise the maxima; beyond: all again"""
        c = state["copy"]
        state["all"] = np.vstack([state["all"], rows])  # (deleted rows keep their slots until compact)
        if M8.absmax(rows) <= c.amax:
            new = M8.Copy8(rows, scale=c.scale)
            c.emax, c.ymax, c.rel = max(c.emax, new.emax), max(c.ymax, new.ymax), max(c.rel, new.rel)
            state["scale_kept"] = True
        else:
            state["copy"] = M8.Copy8(state["all"])
            state["scale_kept"] = False

    def check(what):
        cur = ix.export()
        g = M8.Graph(*cur)
        c = state["copy"]
        full = M8.Copy8(g.vecs, scale=c.scale)  # every stored row under the index's scale, with the carried maxima
        full.emax, full.ymax = c.emax, c.ymax
        reps, t, _, _ = M8.run_model8(oracle, g, metric, queries, limit, L, full)
        _oracle_equals_replay(M.load_oracle(oracle, metric, d, cur), reps, queries, limit, L)
        for mode in (4, 3):
            ans, discarded, contradicted, in_use = _walk(ix, queries, limit, L, mode)
            msg = "%s after %s sketch=%d: lower %d / device %d / upper %d, contradicted %d" % (metric, what, mode, t.lower, discarded, t.upper, contradicted)
            print(msg)
            assert in_use and contradicted == 0 and t.lower > 0 and t.lower <= discarded <= t.upper, msg
            _equals_replay(ans, reps, msg)
        ref = twin.search_batch(queries, limit, L, trace=True, visit_cap=1024)
        assert not twin.sketch_stats()[2]
        _same_answers(ans, ref, "%s after %s: against the float32 twin" % (metric, what))

    def ids_for(k):
        first = state["next"]
        state["next"] += k
        return np.arange(first, first + k, dtype=np.uint64)

    def rounds(rows):
        ids = ids_for(len(rows))
        for t in (ix, twin):
            t.insert_batch(ids, rows)
        appended(rows)
        return ids

    def one_point(rows):
        ids = ids_for(1)
        for t in (ix, twin):
            t.insert_batch(ids, rows[:1], round_size=1)
        appended(rows[:1])

    def insert_update_delete(rows):
        ids = ids_for(len(rows) - 1)
        changes = [vamana.IndexVectorChange(int(i), rows[k].tolist()) for k, i in enumerate(ids)]
        changes.append(vamana.IndexVectorChange(state["update"], rows[-1].tolist()))
        changes.append(vamana.IndexVectorChange(state["update"] + 50, None))
        state["update"] += 1
        for t in (ix, twin):
            t.InsertUpdateDelete(changes)
        appended(rows)

    def explicit(rows):
        ids = ids_for(len(rows))
        for t in (ix, twin):
            t.begin_write()
            t.insert_batch(ids, rows)
            assert not t.sketch_stats()[2]
            t.commit()
        appended(rows)

    check("load")
    rounds(unit_rows(rng, 6, d))
    check("insert_batch")
    one_point(unit_rows(rng, 1, d))
    check("a one-point commit")
    insert_update_delete(unit_rows(rng, 3, d))
    check("InsertUpdateDelete")
    rounds(unit_rows(rng, 4, d) * np.float32(0.25))
    assert state["scale_kept"]
    check("an append of small-norm rows (the maxima are carried, not lowered)")
    scale0 = state["copy"].scale
    rounds(unit_rows(rng, 3, d) * np.float32(3.0))
    assert not state["scale_kept"] and state["copy"].scale > scale0
    check("an append beyond the table's range (every row converted again, the maxima follow)")
    for t in (ix, twin):
        t.delete_batch(np.arange(20, 60, dtype=np.uint64))
    check("delete_batch")
    before = ix.SizeInMemory()
    explicit(unit_rows(rng, 80, d))  # past the 2 048 rows the table was created with
    assert ix.SizeInMemory() > 1.5 * before, "the table did not grow"
    check("begin_write .. commit that grows the table")
    for t in (ix, twin):
        t.compact()
    state["all"] = ix.export()[1]
    state["copy"] = M8.Copy8(state["all"])
    check("compact")
    rounds(unit_rows(rng, 2100, d)[:2100])  # growth without an explicit transaction
    check("insert_batch that grows the table")
    ix.close()
    twin.close()


def test_a_reader_during_commits(oracle):
    from semadb_amd import vamana
    d = 128
    ex, queries = M.l_case(oracle, "cosine", d)
    ix, twin = _twins(vamana, "cosine", d, ex, 4096)
    rng = np.random.default_rng(8)
    stop, errors = threading.Event(), []

    def reader():
        try:
            while not stop.is_set():
                ids, dd, c = ix.search_batch(queries, 10, 40)[:3]
                assert (c == 10).all() and np.isfinite(dd).all()
        except Exception as e:  # noqa: BLE001
            errors.append(e)

    th = threading.Thread(target=reader)
    th.start()
    try:
        for step in range(6):
            ids = np.arange(9000 + 8 * step, 9008 + 8 * step, dtype=np.uint64)
            rows = unit_rows(rng, 8, d) * np.float32(1.0 if step % 2 == 0 else 1.0 + 0.3 * step)  # (odd steps: beyond the range)
            for t in (ix, twin):
                t.insert_batch(ids, rows)
    finally:
        stop.set()
        th.join()
    assert not errors, errors
    assert ix.sketch_stats()[2]
    a = ix.search_batch(queries, 10, 40, trace=True, visit_cap=1024)
    b = twin.search_batch(queries, 10, 40, trace=True, visit_cap=1024)
    _same_answers(a, b, "after the commits")
    ix.close()
    twin.close()


def test_knob_transitions(oracle):
    from semadb_amd import vamana
    d, cap = 384, 4096
    ex, queries = M.l_case(oracle, "cosine", d)
    params = vamana.IndexVectorVamanaParameters(d, "cosine", M.L_BUILD, M.R_FULL, 1.2)
    ix = vamana.NewIndexVamana("t", params, capacity=cap, strict=False)
    ix.set_tuning("wide_walk", 1)
    ix.load(*ex)
    ld = _ld(d)
    sizes, ref = {}, None
    for knob in (3, 1, 3, 0, 3):
        ix.set_tuning("sketch", knob)
        assert ix.sketch_stats() == (0, 0, knob != 0), "the counters are cleared at each set"
        sizes.setdefault(knob, ix.SizeInMemory())
        assert sizes[knob] == ix.SizeInMemory()
        ans = ix.search_batch(queries, 10, 40, trace=True, visit_cap=1024)
        assert (ix.sketch_stats()[0] > 0) == (knob != 0)
        if ref is not None:
            _same_answers(ans, ref, "knob %d" % knob)
        ref = ans
    assert sizes[3] - sizes[0] == cap * ld, "the int8 copy: cap x ld bytes"
    assert sizes[1] - sizes[0] == cap * (ld * 2 + 4), "the float16 copy: cap x (2 ld + 4) bytes"
    # an open transaction walks float32 rows
    ix.begin_write()
    assert not ix.sketch_stats()[2]
    before = ix.sketch_stats()[0]
    _same_answers(ix.search_batch(queries, 10, 40, trace=True, visit_cap=1024), ref, "inside a transaction")
    assert ix.sketch_stats()[0] == before
    ix.abort_write()
    assert ix.sketch_stats()[2]
    ix.close()


@pytest.mark.parametrize("metric,d", [("euclidean", 128), ("cosine", 512), ("cosine", 100)])
def test_tables_without_the_int8_stage_report_the_same_under_3_as_under_1(oracle, metric, d):
    from semadb_amd import vamana
    seed = 700 + d
    ex = M.full_row_export(oracle, metric, d, 1500, seed)
    queries = unit_rows(np.random.default_rng(seed + 7), M.N_QUERIES, d)
    ix = _index(vamana, metric, d, ex)
    seen = {}
    for knob in (1, 3, 2, 4):
        ans, discarded, contradicted, in_use = _walk(ix, queries, 10, 40, knob)
        seen[knob] = (discarded, contradicted, in_use, ix.SizeInMemory())
        if knob != 1:
            _same_answers(ans, ref, "%s d=%d knob %d" % (metric, d, knob))
        ref = ans
    assert seen[3] == seen[1] and seen[4] == seen[2] and seen[1][:3] == seen[2][:3], seen
    assert seen[1][2] == (d != 100)
    ix.close()
