"""A float64 model of the two-precision hop, independent of the kernel's arithmetic.

The walk (search_kernel.h search_body) reads a float16 copy of a new neighbour's row first and its float32 row only
when the float16 distance does not PROVE that AddWithLimit discards the neighbour: with the array full and `tail` its
last distance as the hop (a chunk of 64 edges) starts, a neighbour whose reference distance is above `tail` is never
kept.  This module restates, in numpy and float64,

* the walk itself (`replay`): greedySearch over an exported graph with the oracle's float32 distances, recording for
  every chunk the tail as the chunk starts and the new neighbours in edge order;
* the copy (`half_rows`, `maxima`, `Bounds`): y16 = float16(y), round to nearest, magnitudes below 2^-14 -> 0;
* three counts over the neighbours met with the array full (`count`):
    discardable  reference distance > tail (what a perfect first stage could discard),
    upper        the pure bound proves it: cosine / dot  d16 - (qerr Ymax + ||q|| Emax) > tail,
                 euclidean  D16 - 2 (qerr + Emax) sqrt(D16) > tail,
    lower        the same with every inflation the kernel documents charged on top, each rounded up generously.

The kernel's derivation implies  lower <= discarded on the device <= upper <= discardable.  The constants of `lower`
are the kernel's documented charges (walk_stage.h HalfRows::query, stage_eps, FirstStage::out / HalfRows::out_l2, index_sketch.hip k_sketch_rows), not its output.

Also here: the inputs the GPU tests use (`width_case`, `l_case`, `hostile_queries`, `dispatch_case`), generated through one function so that the CPU
test (test_two_precision_model.py) checks the model's own conditions on exactly them.
"""
import numpy as np

from tests.helpers import start_vector, unit_rows

HALF_MIN_NORMAL = 6.103515625e-5  # 2^-14
METRICS = ("cosine", "dot", "euclidean")


def impl_of(orc):
    return orc.IMPL_AVX2 if orc.has_avx2() else orc.IMPL_ASM


# ---------------------------------------------------------------------------------------------- the float16 copy
def half_rows(x):
    """float16(x) as the copy stores it, returned in float64: round to nearest even, |x| < 2^-14 -> 0, overflow -> inf"""
    x = np.asarray(x, dtype=np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        h = x.astype(np.float16).astype(np.float64)
    h[np.abs(x) < np.float32(HALF_MIN_NORMAL)] = 0.0
    return h


def maxima(rows):
    """(Emax, Ymax) = (max ||y - y16||, max ||y16||) over `rows`, in float64.  A NaN row makes them NaN (on the device a
    NaN's bit pattern wins the atomicMax), an overflowing element makes them inf."""
    rows = np.asarray(rows, dtype=np.float32)
    if rows.shape[0] == 0:
        return 0.0, 0.0
    h = half_rows(rows)
    with np.errstate(over="ignore", invalid="ignore"):
        e = np.sqrt(((rows.astype(np.float64) - h) ** 2).sum(1))
        y = np.sqrt((h ** 2).sum(1))
    em = np.nan if np.isnan(e).any() else e.max()
    ym = np.nan if np.isnan(y).any() else y.max()
    return float(em), float(ym)


def join_maxima(a, b):
    """the maxima of two sets of rows (NaN wins)"""
    return tuple(np.nan if (np.isnan(x) or np.isnan(y)) else max(x, y) for x, y in zip(a, b))


# ---------------------------------------------------------------------------------------------- the graph
class Graph:
    """an exported graph by slot: ids, float32 vectors, adjacency lists as arrays of slots; the start node is id 1"""

    def __init__(self, ids, vecs, offsets, edges):
        self.ids = np.asarray(ids, dtype=np.uint64)
        self.vecs = np.ascontiguousarray(vecs, dtype=np.float32)
        pos = {int(v): k for k, v in enumerate(self.ids)}
        off = np.asarray(offsets, dtype=np.int64)
        slots = np.fromiter((pos[int(e)] for e in edges), dtype=np.int64, count=len(edges))
        self.adj = [slots[off[i]:off[i + 1]] for i in range(len(self.ids))]
        self.deg = np.diff(off)
        self.start = pos[1]


class Replay:
    __slots__ = ("ids", "dists", "visit", "n_hop", "n_dist", "n_edges", "chunks", "expanded")


def replay(g, D, limit, L):
    """greedySearch (search.go:9-102) over `g` with the float32 reference distances `D` ([slots], one query).

    AddWithLimit is restated comparison for comparison (distset.go:166-200: strict >, the evicted tail, the bubble
    with strict <), so that ties and NaNs fall as they do in the reference.  `chunks` gets, per chunk of 64 edges of an
    expanded node (only a start node with an overflow list has more than one), (tail, new) with `tail` the array's last
    distance AS THE CHUNK STARTS when the array is full then, else None, and `new` the unseen neighbours in edge order.
    """
    r = Replay()
    seen = np.zeros(len(g.ids), dtype=bool)
    arr_d, arr_s, arr_v = [], [], []  # distance, slot, visited

    def add(s):
        dist = D[s]
        if len(arr_d) == L:
            if dist > arr_d[-1]:
                return
            arr_d[-1], arr_s[-1], arr_v[-1] = dist, s, False
        else:
            arr_d.append(dist), arr_s.append(s), arr_v.append(False)
        i = len(arr_d) - 1
        while i > 0 and arr_d[i] < arr_d[i - 1]:
            arr_d[i], arr_d[i - 1] = arr_d[i - 1], arr_d[i]
            arr_s[i], arr_s[i - 1] = arr_s[i - 1], arr_s[i]
            arr_v[i], arr_v[i - 1] = arr_v[i - 1], arr_v[i]
            i -= 1

    seen[g.start] = True
    add(g.start)
    n_dist, n_edges = 1, 0
    visit, chunks, expanded = [], [], []
    while True:
        k = next((j for j in range(min(len(arr_d), L)) if not arr_v[j]), None)
        if k is None:
            break
        arr_v[k] = True
        p = arr_s[k]
        visit.append(int(g.ids[p]))
        expanded.append(p)
        row = g.adj[p]
        n_edges += len(row)
        for c0 in range(0, len(row), 64):
            chunk = row[c0:c0 + 64]
            new = chunk[~seen[chunk]]
            if len(new) != len(set(new.tolist())):  # a repeated edge: the second occurrence is seen already
                _, first = np.unique(new, return_index=True)
                new = new[np.sort(first)]
            seen[new] = True
            n_dist += len(new)
            chunks.append((arr_d[-1] if len(arr_d) == L else None, new))
            for s in new.tolist():
                add(s)
    keep = [j for j in range(len(arr_s)) if arr_s[j] != g.start][:limit]
    r.ids = np.array([g.ids[arr_s[j]] for j in keep], dtype=np.uint64)
    r.dists = np.array([arr_d[j] for j in keep], dtype=np.float32)
    r.visit = np.array(visit, dtype=np.uint64)
    r.n_hop, r.n_dist, r.n_edges = len(visit), n_dist, n_edges
    r.chunks, r.expanded = chunks, np.array(expanded, dtype=np.int64)
    return r


# ---------------------------------------------------------------------------------------------- the bounds
class Bounds:
    """per row of the table, for one query: the threshold a tail must be BELOW for the neighbour to be discarded,
    by the pure bound (`upper`) and by the pure bound with every documented inflation charged (`lower`)"""

    def __init__(self, metric, q, v16, yy16, emax, ymax):
        q = np.asarray(q, dtype=np.float32)
        q64 = q.astype(np.float64)
        q16 = half_rows(q)
        with np.errstate(all="ignore"):
            qerr = np.sqrt(((q64 - q16) ** 2).sum())
            qn = np.sqrt((q64 ** 2).sum())
            dot16 = v16 @ q16
            if metric == "euclidean":
                qq = (q16 ** 2).sum()
                D16 = ((v16 - q16) ** 2).sum(1)
                delta = qerr + emax
                self.upper = D16 - 2.0 * delta * np.sqrt(D16)
                # The kernel (HalfRows::out_l2) forms D16 as ||q16||^2 + ||y16||^2 - 2 q16.y16 from three rounded sums, "error
                # below 1e-5 S" with S = ||q16||^2 + ||y16||^2 + 2 |q16.y16|, and charges 1e-5 S itself (`err`): 2e-5 S
                # between the exact D16 and its `d16 - err`, the same above for `up`; charged here: 2.5e-5 S each way.
                # delta: qerr, Emax and their sum carry 1.0001 each at most twice (k_sketch_rows, HalfRows::query): 1.0003,
                # their float32 roundings on top; charged 1.001.  root: x 1.00001 and the sqrt's rounding; charged
                # 1.0001.  The product (1 - 2e-5); charged (1 - 4e-5).  The last line's 1e-6 (|d16| + err + delta root);
                # charged 2e-6 of the same terms taken at their upper values, + 1e-30 for `err`'s floor.
                S = qq + yy16 + 2.0 * np.abs(dot16)
                root = np.sqrt(D16 + 2.5e-5 * S) * 1.0001
                dl = 1.001 * delta
                low = ((D16 - 2.5e-5 * S) - 2.0 * dl * root) * (1.0 - 4e-5)
                self.lower = low - 2e-6 * (np.abs(D16) + 5e-5 * S + dl * root) - 1e-29
            else:
                d16 = (1.0 - dot16) if metric == "cosine" else -dot16
                eps = qerr * ymax + qn * emax
                self.upper = d16 - eps
                # HalfRows::query, stage_eps: qerr, ||q||, Emax, Ymax carry 1.0001 each and the sum another (1.0003 on every product),
                # float32 roundings on top; charged 1.001.  2e-5 ||q|| (Ymax + Emax) for the roundings of the two sums,
                # inflated the same way, and the float16 sum's own roundings (documented below 6.6e-6 ||q|| ||y||)
                # once more because d16 is exact here; charged 3e-5 x 1.001.  FirstStage::out: 4e-7 (1 + |d16| + eps) for
                # the roundings of 1 - dot / -dot and of the subtraction; charged 2e-6 of the same terms.
                slack = 1.001 * eps + 3e-5 * 1.001 * qn * (ymax + emax)
                self.lower = d16 - (slack + 2e-6 * (1.0 + np.abs(d16) + slack))


class Model:
    """the copy of a table and the counts of walks over it.  `emax_ymax`: the table-wide maxima to use (default: of
    all rows of the graph, which is what a full conversion measures)"""

    def __init__(self, g, metric, emax_ymax=None):
        self.g, self.metric = g, metric
        self.v16 = half_rows(g.vecs)
        with np.errstate(all="ignore"):
            self.yy16 = (self.v16 ** 2).sum(1)
        self.emax, self.ymax = maxima(g.vecs) if emax_ymax is None else emax_ymax

    def count(self, q, D, rep):
        """(met with the array full, discardable, upper, lower) over the chunks of one replayed walk"""
        b = Bounds(self.metric, q, self.v16, self.yy16, self.emax, self.ymax)
        full = disc = up = lo = 0
        with np.errstate(invalid="ignore"):
            for tail, new in rep.chunks:
                if tail is None or len(new) == 0:
                    continue
                full += len(new)
                disc += int((D[new] > tail).sum())
                up += int((b.upper[new] > tail).sum())
                lo += int((b.lower[new] > tail).sum())
        return full, disc, up, lo


class Tally:
    """sums over a batch"""

    def __init__(self):
        self.full = self.discardable = self.upper = self.lower = 0
        self.expanded = self.expanded_full_rows = 0

    def add(self, counts, rep=None, g=None):
        self.full += counts[0]
        self.discardable += counts[1]
        self.upper += counts[2]
        self.lower += counts[3]
        if rep is not None:
            self.expanded += len(rep.expanded)
            self.expanded_full_rows += int((g.deg[rep.expanded] >= 64).sum())

    def __repr__(self):
        return "full %d discardable %d upper %d lower %d" % (self.full, self.discardable, self.upper, self.lower)


def run_model(orc, g, metric, queries, limit, L, emax_ymax=None):
    """replays and counts of a batch: ([Replay], Tally, D [nq][slots])"""
    D = orc.distance_matrix(queries, g.vecs, metric, impl_of(orc))
    m = Model(g, metric, emax_ymax)
    t, reps = Tally(), []
    for i in range(queries.shape[0]):
        rep = replay(g, D[i], limit, L)
        t.add(m.count(queries[i], D[i], rep), rep, g)
        reps.append(rep)
    return reps, t, D


# ---------------------------------------------------------------------------------------------- the inputs
N_QUERIES = 32
R_FULL = 64
L_BUILD = 75


def regular_graph(orc, base, metric, start, seed):
    """a hand-made 64-regular graph for the widths at which the reference's prune leaves rows short: every node its 48
    nearest and 16 random other nodes, the start node (id 1, slot 0) 64 random ones.  Returns an export tuple."""
    rng = np.random.default_rng(seed)
    n = base.shape[0]
    Dm = orc.distance_matrix(base, base, metric, impl_of(orc)).astype(np.float64)
    np.fill_diagonal(Dm, np.inf)
    rows = [rng.choice(n, size=64, replace=False)]
    for i in range(n):
        near = np.argsort(Dm[i], kind="stable")[:48]
        rest = np.setdiff1d(np.arange(n), np.append(near, i), assume_unique=False)
        rows.append(np.concatenate([near, rng.choice(rest, size=16, replace=False)]))
    ids = np.arange(1, n + 2, dtype=np.uint64)
    vecs = np.vstack([start[None, :], base]).astype(np.float32)
    offsets = np.arange(0, (n + 1) * 64 + 1, 64, dtype=np.uint64)
    edges = (np.concatenate(rows) + 2).astype(np.uint64)  # row i of base is id i + 2
    return ids, vecs, offsets, edges


def full_row_export(orc, metric, d, n, seed, L=L_BUILD):
    """an export tuple (ids, vecs, offsets, edges) over n i.i.d. unit rows of width d whose adjacency rows are full:
    the oracle's own R = 64 build where at least 90 % of its nodes come out with 64 edges, else the hand-made graph"""
    rng = np.random.default_rng(seed)
    base = unit_rows(rng, n, d)
    start = start_vector(np.random.default_rng(seed), d)
    o = orc.Index(d, metric, R_FULL, L, 1.2, impl=impl_of(orc))
    o.set_start(start)
    # (the reference's round schedule: the same prune, many inserts per round -- a tenth of the one-by-one build's time)
    assert o.insert_rounds(np.arange(2, n + 2, dtype=np.uint64), base) == 0
    ex = o.export()
    deg = np.diff(ex[2].astype(np.int64))
    if (deg >= 64).mean() >= 0.9:
        return ex
    return regular_graph(orc, base, metric, start, seed + 1)


def load_oracle(orc, metric, d, ex, L=L_BUILD):
    o = orc.Index(d, metric, R_FULL, L, 1.2, impl=impl_of(orc))
    assert o.load(*ex) == 0
    return o


WIDTHS = (32, 64, 128, 160, 256, 320, 384, 448, 512, 640, 704, 768)  # NG 1 1 1 2 2 3 3 4 4 6(padded) 6 6
NO_STAGE_WIDTHS = (100, 1024)  # a tail chain; NG 8: no copy is held


def width_rows(d):
    # (the host cost is the oracle's build: fewer rows where they are wide)
    return 2500 if d <= 384 else 2000


def width_case(orc, metric, d):
    """(export, queries, limit, L) of the width cases of test_gpu_two_precision_bound.py"""
    seed = 1000 + d * 3 + METRICS.index(metric)
    ex = full_row_export(orc, metric, d, width_rows(d), seed)
    queries = unit_rows(np.random.default_rng(seed + 7), N_QUERIES, d)
    return ex, queries, 10, 40


L_CASES = ((1, 1), (2, 1), (5, 1), (10, 1), (64, 1), (96, 1), (1, 10), (2, 10), (5, 10), (10, 10), (64, 10), (96, 10))
L_BEYOND = (97, 128)  # the stage is behind the LDS visited set (csrc/walk_plan.h: searchSize <= 96): present routing discards nothing there


def l_case(orc, metric, d):
    """(export, queries) shared by the L / limit and the hostile-query cases of a width"""
    seed = 5000 + d * 3 + METRICS.index(metric)
    ex = full_row_export(orc, metric, d, 2000, seed)
    return ex, unit_rows(np.random.default_rng(seed + 7), N_QUERIES, d)


def hostile_queries(d, kind, seed=77):
    """8 queries of one hostile kind"""
    rng = np.random.default_rng(seed + len(kind))
    q = unit_rows(rng, 8, d)
    if kind == "overflow":
        q[np.arange(8), rng.integers(0, d, 8)] = 1e6
    elif kind == "nan":
        q[np.arange(8), rng.integers(0, d, 8)] = np.nan
    elif kind == "inf":
        q[np.arange(8), rng.integers(0, d, 8)] = np.inf
    elif kind == "zero":
        q[:] = 0.0
    elif kind == "tiny":  # every element below 2^-14: the float16 query is all zero
        q *= np.float32(3e-5) / np.abs(q).max(axis=1, keepdims=True)
    elif kind == "norm1e4":
        q *= np.float32(1e4)
    elif kind == "norm1e-4":
        q *= np.float32(1e-4)
    else:
        raise ValueError(kind)
    return q.astype(np.float32)


HOSTILE_NO_DISCARD = ("overflow", "nan", "inf")  # the bound is infinite or NaN: nothing is discarded
HOSTILE_SANDWICH = ("zero", "tiny", "norm1e4", "norm1e-4")


def dispatch_case(orc, d):
    """(export, 513 queries) of the default-dispatch test: batches of 256, 257, 512, 513 share their first 256"""
    seed = 9000 + d
    ex = full_row_export(orc, "cosine", d, 2000, seed)
    return ex, unit_rows(np.random.default_rng(seed + 7), 513, d)


def overflow_case(orc, metric):
    """(export, queries) of an index whose start node carries an overflow list (more than 64 + 64 edges), built as
    test_gpu_delete.py::test_start_node_overflow_list builds it: a small degree bound and a large delete, whose
    stragglers are appended to the start node without bound (prune.go:131-151)"""
    d, n, R, L = 128, 1500, 4, 20
    rng = np.random.default_rng(1504)
    base = unit_rows(rng, n, d)
    o = orc.Index(d, metric, R, L, 1.5, impl=impl_of(orc))
    o.set_start(start_vector(np.random.default_rng(5), d))
    ids = np.arange(2, n + 2, dtype=np.uint64)
    for i in range(n):
        assert o.insert(int(ids[i]), base[i]) == 0
    assert o.delete(rng.choice(ids, size=n // 8, replace=False).astype(np.uint64)) == 0
    return o.export(), unit_rows(rng, N_QUERIES, d)


def check_tally(t, what):
    """the model's own conditions: the three counts are ordered, and the two sides of the sandwich are within 1 % of
    each other -- else the sandwich would not say much about the device's count"""
    assert t.lower <= t.upper <= t.discardable <= t.full, "%s: %r" % (what, t)
    assert t.lower >= 0.99 * t.upper, "%s: lower / upper = %d / %d" % (what, t.lower, t.upper)
