"""The two-precision hop is the default walk (SDB_TUNE_SKETCH starts at 1): every write path leaves the float16 copy
current without being asked, the copy follows table growth, tables the walk cannot take it for hold no copy, and the
answers are the float32 walk's bit for bit."""
import threading

import numpy as np
import pytest

from tests.helpers import bits, build_oracle_index, unit_rows

pytestmark = pytest.mark.gpu


def _answers(ix, queries, limit, L, visit_cap=512):
    ids, d, c, tr = ix.search_batch(queries, limit, L, trace=True, visit_cap=visit_cap)
    return ids.copy(), bits(d).copy(), c.copy(), tr.n_dist.copy(), tr.n_hop.copy(), tr.n_edges.copy(), tr.visit_ids.copy()


def _same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


def _in_use(ix):
    return bool(ix.sketch_stats()[2])


def _float32_answers(ix, queries, L):
    """the float32 walk's answers, then the default back on (the copy is rebuilt from the committed rows)"""
    ix.set_tuning("sketch", 0)
    ref = _answers(ix, queries, 10, L)
    ix.set_tuning("sketch", 1)
    return ref


def _rows(rng, n, d):
    lat = rng.standard_normal((12, d)).astype(np.float32)
    base = rng.standard_normal((n, 12)).astype(np.float32) @ lat + 0.2 * rng.standard_normal((n, d)).astype(np.float32)
    return (base / np.linalg.norm(base, axis=1, keepdims=True)).astype(np.float32)


@pytest.mark.parametrize("metric", ["cosine", "dot", "euclidean"])
@pytest.mark.parametrize("d", [96, 384, 768])
def test_every_write_leaves_the_copy_current(oracle, metric, d):
    from semadb_amd import vamana
    rng = np.random.default_rng(d + len(metric))
    n, L = 700, 25
    base = _rows(rng, n + 40, d)
    queries = np.vstack([unit_rows(rng, 24, d), base[:4]])
    o = build_oracle_index(oracle, base[:n], metric, R=24, L=L)
    ids, vecs, offsets, edges = o.export()
    ix = vamana.NewIndexVamana("t", vamana.IndexVectorVamanaParameters(d, metric, L, 24, 1.2), strict=False)
    ix.set_tuning("wide_walk", 1)  # the batch walk (one wave per query) is the one that has the stage
    ix.load(ids, vecs, offsets, edges)
    assert _in_use(ix), "load"
    got = _answers(ix, queries, 10, L)
    assert ix.sketch_stats()[0] > 0, "the default walk never discarded a neighbour on its float16 distance"
    ref = _float32_answers(ix, queries, L)
    assert _same(ref, got)
    for q in range(0, queries.shape[0], 5):  # ... and the oracle's, for a sample
        o_ids, o_d, o_vis, o_tr = o.search(queries[q], 10, L)
        assert np.array_equal(got[0][q, :len(o_ids)], o_ids) and np.array_equal(got[1][q, :len(o_ids)], bits(o_d))
        assert int(got[3][q]) == o_tr.n_dist and int(got[4][q]) == o_tr.n_hop and np.array_equal(got[6][q, :o_tr.n_hop], o_vis)
    first = int(ids.max()) + 1
    steps = [
        ("insert_batch", lambda: ix.insert_batch(np.arange(first, first + 30, dtype=np.uint64), base[n:n + 30])),
        ("one-point commit", lambda: ix.insert_batch(np.array([first + 30], dtype=np.uint64), base[n + 30:n + 31], round_size=1)),
        ("InsertUpdateDelete", lambda: ix.InsertUpdateDelete([vamana.IndexVectorChange(first + 31, base[n + 31].tolist()),
                                                              vamana.IndexVectorChange(first + 1, base[n + 32].tolist()),
                                                              vamana.IndexVectorChange(first + 2, None)])),
        ("delete_batch", lambda: ix.delete_batch(np.ascontiguousarray(ids[10:60], dtype=np.uint64))),
        ("compact", lambda: ix.compact()),
    ]
    for name, step in steps:
        step()
        assert _in_use(ix), name
        got = _answers(ix, queries, 10, L)
        assert _same(_float32_answers(ix, queries, L), got), name
    # an open transaction: searches walk the committed view with float32 rows
    ix.begin_write()
    assert not _in_use(ix)
    ix.abort_write()
    assert _in_use(ix)
    # the opt-out frees the copy: rows of ld halves and one float norm each
    before = ix.SizeInMemory()
    ix.set_tuning("sketch", 0)
    assert not _in_use(ix)
    # plain = cap (ld 4 + 3 x 64 x 4 + 3 x 4 + 2 x 8) and the copy = cap (ld 2 + 4): cap and the row stride ld follow
    plain = ix.SizeInMemory()
    freed = before - plain
    cap = (plain - 2 * freed) // (3 * 64 * 4 + 3 * 4 + 2 * 8 - 8)
    ld = (freed // cap - 4) // 2
    assert cap >= ix.stats()[0] and ld >= d and ld % 32 == 0 and freed == cap * (ld * 2 + 4)
    ix.close()


def test_tables_without_the_stage_hold_no_copy(oracle):
    from semadb_amd import vamana, vectorstore as vs
    rng = np.random.default_rng(4)
    # rows with a tail chain (d % 32 != 0)
    ix = vamana.NewIndexVamana("t", vamana.IndexVectorVamanaParameters(100, "cosine", 25, 16, 1.2), strict=False)
    ix.set_start(unit_rows(rng, 1, 100)[0])
    ix.insert_batch(np.arange(2, 402, dtype=np.uint64), unit_rows(rng, 400, 100))
    assert not _in_use(ix)
    ix.close()
    # a quantizer attached after the copy was built: the copy goes, and with it its memory
    d, n = 64, 600
    base = unit_rows(rng, n, d)
    ix = vamana.NewIndexVamana("t", vamana.IndexVectorVamanaParameters(d, "euclidean", 25, 16, 1.2), strict=False)
    ix.set_start(unit_rows(rng, 1, d)[0])
    ix.insert_batch(np.arange(2, n + 2, dtype=np.uint64), base)
    assert _in_use(ix)
    with_copy = ix.SizeInMemory()
    ix.set_tuning("sketch", 0)
    plain = ix.SizeInMemory()
    ix.set_tuning("sketch", 1)
    assert ix.SizeInMemory() == with_copy > plain
    ids, vecs, _, _ = ix.export()
    gpq = vs.ProductQuantizer("euclidean", vs.ProductQuantizerParameters(16, 4), d)
    codes = gpq.Fit(vecs.copy(), rng.integers(0, len(ids), 4), alias=True)
    vs.attach(ix, gpq, ids, codes)
    assert not _in_use(ix)
    cap, M = (plain - 2 * (with_copy - plain)) // 788, 4  # (as in the test above)
    assert ix.SizeInMemory() == plain + cap * (M + 2 * 64 * M)  # code rows and the neighbours' code rows; no copy
    ix.close()


@pytest.mark.parametrize("explicit", [False, True])
def test_growth_keeps_the_copy_in_use(explicit):
    from semadb_amd import vamana
    rng = np.random.default_rng(21 + explicit)
    d, L = 128, 30
    base = _rows(rng, 2600, d)
    queries = unit_rows(rng, 48, d)
    ix = vamana.NewIndexVamana("t", vamana.IndexVectorVamanaParameters(d, "cosine", L, 24, 1.2), capacity=1024, strict=False)
    ix.set_tuning("wide_walk", 1)
    ix.set_start(unit_rows(rng, 1, d)[0])
    ix.insert_batch(np.arange(2, 1002, dtype=np.uint64), base[:1000])
    assert _in_use(ix)
    done = 1000
    for step in (300, 700, 600):  # 1 300 rows: past 1 024; 2 000; 2 600: past 2 048
        if explicit:
            ix.begin_write()
        ix.insert_batch(np.arange(2 + done, 2 + done + step, dtype=np.uint64), base[done:done + step])
        if explicit:
            assert not _in_use(ix)
            ix.commit()
        done += step
        assert _in_use(ix), "after the commit that followed growth to %d rows" % done
        got = _answers(ix, queries, 10, L)
        assert _same(_float32_answers(ix, queries, L), got)
    ix.set_tuning("sketch", 2)
    _answers(ix, queries, 10, L)
    discarded, contradicted, in_use = ix.sketch_stats()
    assert in_use and discarded > 0 and contradicted == 0
    ix.close()


def test_reader_sees_one_committed_version_while_the_writer_commits():
    """a reader thread searches while the writer commits one-point inserts; every answer is the float32 walk's answer
    of one committed version (a twin index with the copy switched off receives the same writes)"""
    from semadb_amd import vamana
    rng = np.random.default_rng(33)
    d, L, n0, steps = 96, 30, 1500, 12
    base = _rows(rng, n0 + steps, d)
    queries = unit_rows(rng, 32, d)
    start = unit_rows(rng, 1, d)[0]

    def make(sketch):
        ix = vamana.NewIndexVamana("t", vamana.IndexVectorVamanaParameters(d, "cosine", L, 24, 1.2), strict=False)
        ix.set_tuning("wide_walk", 1)
        ix.set_tuning("sketch", sketch)
        ix.set_start(start)
        ix.insert_batch(np.arange(2, n0 + 2, dtype=np.uint64), base[:n0])
        return ix

    ix, twin = make(1), make(0)
    versions = [_answers(twin, queries, 10, L)[:3]]
    seen, stop, errors = [], threading.Event(), []

    def reader():
        try:
            while not stop.is_set():
                ids, dd, c, _ = ix.search_batch(queries, 10, L)
                seen.append((ids.copy(), bits(dd).copy(), c.copy()))
        except Exception as e:  # pragma: no cover - reported below
            errors.append(e)

    t = threading.Thread(target=reader)
    t.start()
    try:
        for i in range(steps):
            pid = np.array([n0 + 2 + i], dtype=np.uint64)
            ix.insert_batch(pid, base[n0 + i:n0 + i + 1], round_size=1)
            twin.insert_batch(pid, base[n0 + i:n0 + i + 1], round_size=1)
            versions.append(_answers(twin, queries, 10, L)[:3])
    finally:
        stop.set()
        t.join()
    assert not errors, errors
    assert seen
    for got in seen:
        assert any(_same(got, v) for v in versions), "an answer that no committed version gives"
    assert _in_use(ix) and _same(_answers(ix, queries, 10, L)[:3], versions[-1])
    ix.close()
    twin.close()


def test_filtered_searches_on_a_table_with_the_copy_are_unchanged():
    """filtered walks read float32 rows: with the copy held (the default) they answer what they answer without it"""
    from semadb_amd import vamana
    rng = np.random.default_rng(41)
    d, L, n = 128, 40, 1500
    base = _rows(rng, n, d)
    ix = vamana.NewIndexVamana("t", vamana.IndexVectorVamanaParameters(d, "cosine", L, 24, 1.2), strict=False)
    ix.set_start(unit_rows(rng, 1, d)[0])
    ix.insert_batch(np.arange(2, n + 2, dtype=np.uint64), base)
    assert _in_use(ix)
    q = unit_rows(rng, 24, d)
    ids = np.arange(2, n + 2)
    filters = [set(int(v) for v in rng.choice(ids, size=(5, L, n // 2)[i % 3], replace=False)) for i in range(q.shape[0])]

    def ask():
        g_ids, g_d, g_c, tr = ix.search_batch(q, 10, L, filters=filters, trace=True, visit_cap=1024)
        return g_ids.copy(), bits(g_d).copy(), g_c.copy(), tr.n_dist.copy(), tr.n_hop.copy(), tr.visit_ids.copy()

    with_copy = ask()
    assert _in_use(ix)
    ix.set_tuning("sketch", 0)
    assert _same(with_copy, ask())
    ix.close()
