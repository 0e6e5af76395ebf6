"""The inputs of the large-searchSize tests (tests/test_gpu_large_search_size.py) and the conditions that make them
reach what they are meant to reach (tests/test_large_search_model.py, without a GPU).

Above searchSize 96 every search leaves the LDS visited sets for the query's HBM bitset and the one-wave kernel
k_greedy_search<Dist, NREG, FILT, 0>: two array registers (128 entries) at 97 .. 128, eight (512 entries) at 129 .. 512.
A product quantizer whose table has 2 049 .. 16 384 entries takes the same kernel at ANY searchSize, its table in up to
64 KB of dynamic LDS.  The cases below fill, overfill or never fill those arrays:

  A  one narrow table per metric (d = 32, N_A rows), searchSize on and beside every register boundary, limit up to
     searchSize; a table smaller than the array (N_SMALL rows at searchSize 512)
  B  an integer grid whose distances nearly all tie, so that equal distances straddle every register boundary; the
     non-finite queries of test_gpu_pq.py
  C  the six filter kinds of test_gpu_filter.py at (searchSize, limit) pairs either side of 128
  D  every row width that has a kernel of its own
  E  bitset reuse across batches of different searchSize on one index; 513 queries in one call; a start node with an
     overflow list
  F  product quantizers of 128 .. 18 432 table entries

Tables are built by the oracle once per process and shared by the CPU and the GPU tests.
"""
import atexit
import functools

import numpy as np

from tests.helpers import build_oracle_index, unit_rows

# ---------------------------------------------------------------------------------------------- A
D_A = 32
N_A = 10000        # 2 * L < n_dist < 0.8 * n for every query at every L below (test_large_search_model.py states the range)
N_SMALL = 300      # fewer rows than the array has entries
NQ = 16
A_METRICS = ("euclidean", "cosine", "dot")
A_L = (97, 127, 128, 129, 191, 192, 193, 256, 257, 320, 384, 385, 448, 511, 512)
BOUNDARIES = (64, 128, 192, 256, 320, 384, 448)   # entry b is lane 0 of register b / 64


SHORT_ROW_L = (97, 128, 129, 200)   # limit = searchSize on the small table: a final array that holds the start node


def limits_of(L):
    """limit 1, 10, either side of one register, and the whole array"""
    return (1, 10, 64, 65, L)


class Table:
    def __init__(self, metric, d, o, queries, n):
        self.metric, self.d, self.o, self.queries, self.n = metric, d, o, queries, n
        self.ex = o.export()
        self.ids = self.ex[0][self.ex[0] != 1].astype(np.int64)


def _table(orc, metric, d, n, seed, nq=NQ):
    rng = np.random.default_rng(seed)
    base = unit_rows(rng, n, d)
    o = build_oracle_index(orc, base, metric, R=32, L=50)
    return Table(metric, d, o, unit_rows(rng, nq, d), n)


@functools.lru_cache(maxsize=None)
def a_table(orc, metric):
    t = _table(orc, metric, D_A, N_A, 9100 + A_METRICS.index(metric))
    t.more_queries = unit_rows(np.random.default_rng(9200 + A_METRICS.index(metric)), NQ, D_A)  # E: "other queries"
    return t


@functools.lru_cache(maxsize=None)
def small_table(orc):
    return _table(orc, "euclidean", D_A, N_SMALL, 9300)


# ---------------------------------------------------------------------------------------------- B
N_TIES = 12000
TIE_L = (129, 192, 256, 512)


@functools.lru_cache(maxsize=None)
def tie_table(orc):
    """the integer grid of test_gpu_search.py::test_search_many_ties: squared distances are small integers"""
    rng = np.random.default_rng(3)
    base = rng.integers(0, 4, size=(N_TIES, 8)).astype(np.float32)
    o = build_oracle_index(orc, base, "euclidean", R=32, L=50)
    t = Table("euclidean", 8, o, rng.integers(0, 4, size=(NQ, 8)).astype(np.float32), N_TIES)
    t.filters = [set(int(v) for v in rng.choice(t.ids, size=N_TIES // 2, replace=False)) for _ in range(NQ)]
    return t


def nonfinite_queries(q):
    """the five query kinds of test_gpu_pq.py::test_pq_search_parity, and three finite ones behind them"""
    d = q.shape[1]
    qn = q[:8].copy()
    qn[0, 3] = np.nan
    qn[1, :] = np.float32(3e38)
    qn[2, ::2] = np.float32(-3e38)
    qn[3, 0] = np.inf
    qn[4, : d // 2] = np.float32(2e38)
    return qn


NONFINITE_L = (129, 512)

# ---------------------------------------------------------------------------------------------- C
FILTER_KINDS = ("fewer than limit", "exactly L", "n // 2", "40 and unknown ids", "with the start id", "empty")
FILTER_CASES = ((97, 65), (128, 128), (129, 129), (200, 10), (320, 200), (512, 65), (512, 512))
FILTER_METRICS = ("cosine", "euclidean")
NQ_FILTERED = 18   # three queries of every kind


def make_filters(rng, ids, nq, L, limit):
    """the six kinds of test_gpu_filter.py::test_filtered_batch_parity, query i of kind i % 6"""
    out, n = [], len(ids)
    for i in range(nq):
        kind = i % 6
        if kind == 0:
            f = rng.choice(ids, size=min(5, max(limit - 1, 0)), replace=False)
        elif kind == 1:
            f = rng.choice(ids, size=L, replace=False)
        elif kind == 2:
            f = rng.choice(ids, size=n // 2, replace=False)
        elif kind == 3:
            f = np.concatenate([rng.choice(ids, size=40, replace=False), [10 ** 7 + i, 10 ** 8]])
        elif kind == 4:
            f = np.concatenate([[1], rng.choice(ids, size=20, replace=False)])
        else:
            f = np.array([], dtype=np.int64)
        out.append(set(int(v) for v in f))
    return out


@functools.lru_cache(maxsize=None)
def filters_of(orc, metric, L, limit):
    t = a_table(orc, metric)
    return make_filters(np.random.default_rng(9400 + 7 * L + limit), t.ids, NQ_FILTERED, L, limit)


def seeds_of(t, f, L):
    """search.go:33-51: the first searchSize ids of the filter, ascending, those the table holds"""
    known = set(int(v) for v in t.ex[0])
    return sum(1 for v in sorted(f)[:L] if v in known)


# ---------------------------------------------------------------------------------------------- D
# a tail-only row; NG 1 with a tail; NG 1, 2, 3, 4, 6, 8; 1280: padded to NG 12; 1536: NG 12; 2048: NG 16; 2112: the
# generic kernel; 3072: NG 24
WIDTHS = (25, 100, 128, 256, 384, 512, 768, 1024, 1280, 1536, 2048, 2112, 3072)
WIDTH_METRICS = ("euclidean", "cosine")
WIDTH_L = (129, 256)
NQ_WIDTH = 12


def width_rows(d):
    return 800 if d <= 512 else 600 if d <= 1536 else 400


@functools.lru_cache(maxsize=None)
def width_table(orc, metric, d):
    t = _table(orc, metric, d, width_rows(d), 9500 + d + WIDTH_METRICS.index(metric), NQ_WIDTH)
    rng = np.random.default_rng(9600 + d)
    t.filters = [set(int(v) for v in rng.choice(t.ids, size=t.n // 2, replace=False)) for _ in range(NQ_WIDTH)]
    return t


# ---------------------------------------------------------------------------------------------- E
REUSE_STEPS = ((1, 512, False), (2, 512, True), (1, 128, False), (1, 97, True), (1, 512, False), (1, 50, False), (1, 129, False))
MANY = 513
MANY_L = 129


def many_checked():
    """the first 8 queries and every 16th: the per-query bitset stride, the grid's last block"""
    return sorted(set(range(8)) | set(range(0, MANY, 16)) | {MANY - 1})


@functools.lru_cache(maxsize=None)
def many_queries():
    return unit_rows(np.random.default_rng(9700), MANY, D_A)


OVERFLOW_L = 256

# ---------------------------------------------------------------------------------------------- F
# (d, M, K)
PQ_SHAPES = ((32, 8, 16), (128, 32, 256), (128, 64, 256), (192, 96, 192), (128, 128, 64))
PQ_METRICS = ("cosine", "euclidean")
PQ_ROWS = 1500
PQ_L = (97, 128, 129, 512)
NQ_PQ = 16
LDS_TABLE_BYTES = 64 * 1024   # the largest table the one-wave kernel copies into LDS
HASH_TABLE_ENTRIES = 2048     # the largest table that leaves room for an LDS visited set beside it
WIDE_M = (128, 192, 256, 384)  # the multi-wave walk's shapes, up to searchSize 96


def pq_route(M, K, L):
    """which walk serves a plain search of a table of M x K entries at searchSize L, from the shape alone:
    "multi-wave", "hash" (LDS visited set beside an LDS table), "bitset lds" (table in LDS, HBM bitset), "bitset global" """
    if M in WIDE_M and K <= 256 and K % 32 == 0 and L <= 96:
        return "multi-wave"
    in_lds = M * K * 4 <= LDS_TABLE_BYTES
    if in_lds and M * K <= HASH_TABLE_ENTRIES and L <= 96:
        return "hash"
    return "bitset lds" if in_lds else "bitset global"


@functools.lru_cache(maxsize=None)
def pq_table(orc, metric, d, M, K):
    """a latent-mixture table (test_gpu_pq.py::test_multi_wave_quantized_walk_parity) with a quantizer trained as
    test_pq_search_parity trains it: on the first 700 stored rows, first centroids drawn per sub-vector"""
    rng = np.random.default_rng(9800 + d + M + K + PQ_METRICS.index(metric))
    lat = rng.standard_normal((12, d)).astype(np.float32)
    base = rng.standard_normal((PQ_ROWS, 12)).astype(np.float32) @ lat + 0.3 * rng.standard_normal((PQ_ROWS, d)).astype(np.float32)
    base = (base / np.linalg.norm(base, axis=1, keepdims=True)).astype(np.float32)
    o = build_oracle_index(orc, base, metric, R=32, L=50)
    t = Table(metric, d, o, unit_rows(rng, NQ_PQ, d), PQ_ROWS)
    t.M, t.K = M, K
    t.train = t.ex[1][1:701].copy()
    t.first = rng.integers(0, 700, M)
    t.opq = orc.PQ(d, metric, M, K)
    t.opq.fit(t.train.copy(), t.first, alias=True)
    t.codes = np.stack([t.opq.encode(v) for v in t.ex[1]])
    assert o.attach_pq(t.opq, t.codes) == 0
    t.filters40 = [set(int(v) for v in rng.choice(t.ids, size=40, replace=False)) for _ in range(NQ_PQ)]
    t.filters_half = [set(int(v) for v in rng.choice(t.ids, size=PQ_ROWS // 2, replace=False)) for _ in range(NQ_PQ)]
    return t


def n_dist_range(t, limit, L, filters=None, queries=None):
    q = t.queries if queries is None else queries
    nd = [t.o.search(q[i], limit, L, filter_ids=None if filters is None else sorted(filters[i]))[3].n_dist for i in range(len(q))]
    return min(nd), max(nd)


@atexit.register
def _drop_the_tables():
    """the cached tables hold oracle indexes: freed while the oracle's library is still loaded"""
    for f in (a_table, small_table, tie_table, width_table, pq_table, filters_of):
        f.cache_clear()
