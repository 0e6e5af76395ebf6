"""CPU model of the re-ranked search (sdb_index_search_batch_rerank) and the inputs its tests share: numpy and the
oracle only, no GPU.

    rerank(oracle, o, ids, vecs, metric, q, limit, L, r, filter_ids)

is the definition in include/semadb_amd.h restated: the walk's first r candidates (o.search with limit = r), the
oracle's float32 distance between the query and each candidate's stored row, np.lexsort over (isnan, distance, walk
position), the first `limit`.  `o` is whatever walks the store: the oracle's index (plain store, product quantizer) or
one of the two adapters below for bit codes -- hamming through the oracle over the 0 / 1 expansion of the codes, jaccard
through tests/binary_model.py's restatement, as tests/test_gpu_binary.py does.

The fixture builders are cached: tests/test_rerank_model.py (CPU) states the model's own conditions on exactly the
tables and queries tests/test_gpu_rerank.py sends to the device."""
import atexit
import functools
import types

import numpy as np

from tests import binary_model as bm
from tests.helpers import build_oracle_index, unit_rows

R, L, NQ, LIMIT = 32, 50, 32, 10
RERANKS = (10, 25, 50)
# (d, M, K, n): the two-wave walk, a table of 8 KB, the slot-gathered walk, the multi-wave walk, a row with a tail
# chain, a wide row
PQ_SHAPES = [(32, 8, 16, 1500), (96, 8, 256, 1500), (128, 64, 32, 1500), (192, 192, 256, 1500), (90, 6, 16, 1500),
             (768, 8, 64, 700)]
PQ_TABLE = PQ_SHAPES[:3]  # the shapes of tests/test_gpu_pq.py::test_pq_search_parity among them (same seeds, same draws)
METRICS = ("euclidean", "cosine", "dot")
BQ_CASES = [(kind, d) for kind in ("hamming", "jaccard") for d in (64, 100, 384)]


def rows_of(ids, vecs, want):
    """the stored rows of the ids `want`, by id (ids need not be ascending)"""
    ids = np.asarray(ids, dtype=np.uint64)
    order = np.argsort(ids, kind="stable")
    pos = order[np.searchsorted(ids[order], np.asarray(want, dtype=np.uint64))]
    assert np.array_equal(ids[pos], np.asarray(want, dtype=np.uint64))
    return vecs[pos]


def rerank(oracle, o, ids, vecs, metric, q, limit, L, r, filter_ids=None):
    """(ids, exact distances) of the re-ranked search of one query, and the walk's own answer (ids, dists, visit, trace)"""
    walk = o.search(q, r, L, filter_ids)
    c_ids = np.asarray(walk[0], dtype=np.uint64)
    if c_ids.size == 0:
        return c_ids, np.zeros(0, np.float32), walk
    with np.errstate(all="ignore"):
        e = oracle.distance_matrix(np.asarray(q, np.float32)[None, :], rows_of(ids, vecs, c_ids), metric)[0]
    j = np.arange(c_ids.size)
    order = np.lexsort((j, e, np.isnan(e)))
    return c_ids[order][:limit], e[order][:limit], walk


class HammingWalk:
    """the walk over hamming codes: the oracle over the codes' 0.0 / 1.0 expansion (squared euclidean == hamming, exactly)"""

    def __init__(self, oracle, ids, codes, off, edges, thr, d, R=R, L=L):
        self.thr, self.d = thr, d
        self.o = oracle.Index(d, "euclidean", R, L, 1.2)
        assert self.o.load(ids, bm.expand(codes, d), off, edges) == 0

    def search(self, q, limit, L, filter_ids=None):
        return self.o.search(bm.expand(bm.encode(np.asarray(q, np.float32)[None, :], self.thr), self.d)[0], limit, L,
                             filter_ids=filter_ids)


class JaccardWalk:
    """the walk over jaccard codes: tests/binary_model.py's restatement of the reference"""

    def __init__(self, ids, codes, off, edges, thr, R=R, L=L):
        self.thr = thr
        self.g = bm.Graph(bm.PAIR["jaccard"], R, L, 1.2)
        self.g.load(ids, codes, off, edges)

    def search(self, q, limit, L, filter_ids=None):
        m = self.g.search(bm.encode(np.asarray(q, np.float32)[None, :], self.thr)[0], limit, L, filter_ids)
        tr = types.SimpleNamespace(n_dist=m.n_dist, n_hop=m.n_hop, n_edges=m.n_edges)
        return m.ids, m.dists, np.array(m.visit, dtype=np.uint64), tr


def _orc():
    from oracle import oracle as orc
    orc.lib()
    return orc


@functools.lru_cache(maxsize=None)
def pq_fixture(metric, d, M, K, n):
    """the table, quantizer and queries of tests/test_gpu_pq.py::test_pq_search_parity (seed d * M + K)"""
    oracle = _orc()
    rng = np.random.default_rng(d * M + K)
    base = unit_rows(rng, n, d)
    o = build_oracle_index(oracle, base, metric, R=R, L=L)
    ids, vecs, off, edges = o.export()
    n_train = min(700, n)
    train = vecs[1:1 + n_train].copy()
    first = rng.integers(0, n_train, M)
    opq = oracle.PQ(d, metric, M, K)
    opq.fit(train.copy(), first, alias=True)
    codes = np.stack([opq.encode(v) for v in vecs])
    assert o.attach_pq(opq, codes) == 0
    q = unit_rows(rng, NQ, d)
    return types.SimpleNamespace(kind="pq", o=o, opq=opq, ids=ids, vecs=vecs, off=off, edges=edges, train=train, first=first,
                                 q=q, metric=metric, d=d, M=M, K=K, rng=rng)


def clustered(rng, n, d, unit):
    """rows around a few centres (tests/test_gpu_binary.py): codes that share most bits, so nearly every bit distance ties"""
    centers = rng.standard_normal((10, d)).astype(np.float32)
    rows = (centers[rng.integers(0, 10, n)] + 0.7 * rng.standard_normal((n, d))).astype(np.float32)
    if unit:
        rows /= np.linalg.norm(rows, axis=1, keepdims=True).astype(np.float32)
    return rows


@functools.lru_cache(maxsize=None)
def bq_fixture(kind, d, n=1000):
    """a float graph built by the oracle, the threshold the quantizer fits from its rows (start node included, storage
    order), every row's code; float metric: cosine over unit rows at d = 384, euclidean otherwise"""
    oracle = _orc()
    metric = "cosine" if d == 384 else "euclidean"
    rng = np.random.default_rng(7000 + d + (1 if kind == "jaccard" else 0))
    base = clustered(rng, n, d, unit=metric == "cosine")
    fo = build_oracle_index(oracle, base, metric, R=R, L=L)
    ids, vecs, off, edges = fo.export()
    thr = bm.fit_threshold(vecs)
    codes = bm.encode(vecs, thr)
    if kind == "hamming":
        o = HammingWalk(oracle, ids, codes, off, edges, thr, d)
    else:
        o = JaccardWalk(ids, codes, off, edges, thr)
    q = (base[rng.integers(0, n, NQ)] + 0.5 * rng.standard_normal((NQ, d))).astype(np.float32)
    return types.SimpleNamespace(kind=kind, o=o, ids=ids, vecs=vecs, off=off, edges=edges, thr=thr, codes=codes, q=q,
                                 metric=metric, d=d, rng=rng)


def small_fixture():
    """fewer live rows (30) than candidates asked for"""
    return bq_fixture("hamming", 64, 30)


@functools.lru_cache(maxsize=None)
def dup_fixture(n=1200, d=32, M=8, K=16, metric="euclidean"):
    """40 rows stored twice under different ids, every query next to one such pair: the pair's codes, quantizer
    distances and exact distances tie bit for bit, so only the walk's order can place them"""
    oracle = _orc()
    rng = np.random.default_rng(4242)
    base = unit_rows(rng, n, d)
    base[n - 40:] = base[:40]
    o = build_oracle_index(oracle, base, metric, R=R, L=L)
    ids, vecs, off, edges = o.export()
    train = vecs[1:701].copy()
    first = rng.integers(0, 700, M)
    opq = oracle.PQ(d, metric, M, K)
    opq.fit(train.copy(), first, alias=True)
    codes = np.stack([opq.encode(v) for v in vecs])
    assert o.attach_pq(opq, codes) == 0
    q = (base[:NQ] + np.float32(0.05) * rng.standard_normal((NQ, d))).astype(np.float32)
    return types.SimpleNamespace(kind="pq", o=o, opq=opq, ids=ids, vecs=vecs, off=off, edges=edges, train=train, first=first,
                                 q=q, metric=metric, d=d, M=M, K=K, rng=rng)


@functools.lru_cache(maxsize=None)
def plain_fixture(metric, d, n=1200, nq=513):
    oracle = _orc()
    rng = np.random.default_rng(9000 + d)
    base = unit_rows(rng, n, d)
    o = build_oracle_index(oracle, base, metric, R=R, L=L)
    ids, vecs, off, edges = o.export()
    q = unit_rows(rng, nq, d)
    return types.SimpleNamespace(kind="plain", o=o, ids=ids, vecs=vecs, off=off, edges=edges, q=q, metric=metric, d=d, rng=rng)


def exact_top(oracle, fx, k=LIMIT):
    """ids of the k stored points nearest to each query by the float32 metric (the start node is no point)"""
    with np.errstate(all="ignore"):
        D = oracle.distance_matrix(fx.q, fx.vecs[1:], fx.metric)
    return [fx.ids[1:][np.argsort(D[i], kind="stable")[:k]] for i in range(fx.q.shape[0])]


def recall_and_changes(oracle, fx, nq=NQ):
    """{r: (mean recall@10 against the exact top 10, queries whose re-ranked top 10 differs from the walk's own)}"""
    truth = exact_top(oracle, fx)
    out = {}
    for r in RERANKS:
        hits, changed = 0, 0
        for k in range(nq):
            plain = fx.o.search(fx.q[k], LIMIT, L)[0]
            got = rerank(oracle, fx.o, fx.ids, fx.vecs, fx.metric, fx.q[k], LIMIT, L, r)[0]
            hits += len(set(int(v) for v in got) & set(int(v) for v in truth[k]))
            changed += 0 if np.array_equal(got, plain) else 1
        out[r] = (hits / (LIMIT * nq), changed)
    return out


@atexit.register
def _drop_fixtures():  # the oracle's handles are freed while its library is still loaded
    for f in (pq_fixture, bq_fixture, dup_fixture, plain_fixture):
        f.cache_clear()
