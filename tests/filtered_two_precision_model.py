"""A float64 model of the two-precision hop on FILTERED walks (search.go:33-51,93-95), independent of the kernel.

A filtered walk seeds its search set with Add (distset.go:203-211: appended, not sorted), so the candidate array is not
sorted and its last distance can RISE while a chunk of neighbours is inserted: AddWithLimit overwrites the last entry
and bubbles it left only while it is `<` its neighbour (:193-198), and the new last entry is then the old second-to-last
one.  The plain walk's rule -- discard what is provably above the last distance as the chunk starts -- is wrong here.

The rule the kernel uses (cand_array.h list_tail_bound): with the array full as a chunk starts and k new neighbours
in the chunk, B = the maximum of the array's last min(k, L) distances; a neighbour whose reference distance is above B
is discarded at its turn whatever happens before it.  (One kept insertion puts x <= tail somewhere and shifts what is
behind it right by one, so the tail after j insertions is at most the maximum of the original last j + 1 entries, and
the i-th neighbour of the chunk meets the array after at most i <= k - 1 insertions.)  A NaN among those distances makes
B NaN: nothing is discarded in that chunk.

Here: the walk (`replay`) with seeds, result set and B per chunk; the three counts of tests/two_precision_model.py taken
against B (`count`); the number of neighbours the pure bound would discard against the chunk-start tail although the
reference KEEPS them (`naive_wrong`: what a straight port of the plain rule gets wrong); and the inputs of
tests/test_gpu_filtered_two_precision.py, generated through one function each and cached, so that the CPU test
(test_filtered_two_precision_model.py) checks the model's own conditions on exactly them.  The float16 copy, its maxima
and the bounds are two_precision_model's.
"""
import functools

import numpy as np

from tests.helpers import build_oracle_index, unit_rows
from tests.two_precision_model import METRICS, Bounds, Graph, half_rows, impl_of, maxima
from tests import two_precision_model as M

N_QUERIES = 32


class Replay:
    __slots__ = ("ids", "dists", "visit", "n_hop", "n_dist", "n_edges", "chunks")


def _add_with_limit(arr, cap, dist, s):
    """DistSet.AddWithLimit past CheckAndVisit (distset.go:184-198) on arr = [dists, slots, visited]; was it kept?"""
    d_, s_, v_ = arr
    if len(d_) == cap:
        if dist > d_[-1]:
            return False
        d_[-1], s_[-1], v_[-1] = dist, s, False
    else:
        d_.append(dist), s_.append(s), v_.append(False)
    i = len(d_) - 1
    while i > 0 and d_[i] < d_[i - 1]:
        d_[i], d_[i - 1] = d_[i - 1], d_[i]
        s_[i], s_[i - 1] = s_[i - 1], s_[i]
        v_[i], v_[i - 1] = v_[i - 1], v_[i]
        i -= 1
    return True


def replay(g, D, limit, L, filter_ids):
    """the filtered greedySearch over `g` with the float32 reference distances `D` ([slots], one query).

    `chunks` gets, per chunk of 64 edges of an expanded node, (tail, B, new, kept): the array's last distance and the
    maximum of its last min(len(new), L) distances AS THE CHUNK STARTS when the array is full then (else None, None),
    the unseen neighbours in edge order and whether AddWithLimit kept each."""
    r = Replay()
    pos = {int(v): k for k, v in enumerate(g.ids)}
    filt = sorted(int(v) for v in filter_ids)
    fset = set(filt)
    seen = np.zeros(len(g.ids), dtype=bool)
    rseen = np.zeros(len(g.ids), dtype=bool)
    arr = ([], [], [])   # the search set
    res = ([], [], [])   # the result set, capacity `limit`
    n_dist = n_edges = 0
    seeds = [pos[i] for i in filt[:L] if i in pos]  # :41-48 the first searchSize ids, those that exist
    for s in seeds:  # searchSet.Add :49 -- appended, not sorted
        if not seen[s]:
            seen[s] = True
            n_dist += 1
            arr[0].append(D[s]), arr[1].append(s), arr[2].append(False)
    for s in seeds:  # resultSet.AddWithLimit :50
        if not rseen[s]:
            rseen[s] = True
            n_dist += 1
            _add_with_limit(res, limit, D[s], s)
    if not seen[g.start]:  # :57-61
        seen[g.start] = True
        n_dist += 1
        _add_with_limit(arr, L, D[g.start], g.start)
    visit, chunks = [], []
    while True:
        k = next((j for j in range(min(len(arr[0]), L)) if not arr[2][j]), None)
        if k is None:
            break
        arr[2][k] = True
        p = arr[1][k]
        pd = arr[0][k]
        visit.append(int(g.ids[p]))
        row = g.adj[p]
        n_edges += len(row)
        for c0 in range(0, len(row), 64):
            chunk = row[c0:c0 + 64]
            new = chunk[~seen[chunk]]
            if len(new) != len(set(new.tolist())):
                _, first = np.unique(new, return_index=True)
                new = new[np.sort(first)]
            seen[new] = True
            n_dist += len(new)
            tail = B = None
            if len(arr[0]) == L and len(new):
                tail = arr[0][-1]
                B = np.max(np.asarray(arr[0][L - min(len(new), L):], dtype=np.float64))  # (a NaN wins)
            kept = np.array([_add_with_limit(arr, L, D[s], s) for s in new.tolist()], dtype=bool)
            chunks.append((tail, B, new, kept))
        if int(g.ids[p]) in fset and not rseen[p]:  # :93-95
            rseen[p] = True
            n_dist += 1
            _add_with_limit(res, limit, pd, p)
    keep = [j for j in range(len(res[1])) if res[1][j] != g.start][:limit]
    r.ids = np.array([g.ids[res[1][j]] for j in keep], dtype=np.uint64)
    r.dists = np.array([res[0][j] for j in keep], dtype=np.float32)
    r.visit = np.array(visit, dtype=np.uint64)
    r.n_hop, r.n_dist, r.n_edges = len(visit), n_dist, n_edges
    r.chunks = chunks
    return r


class Tally:
    def __init__(self):
        self.full = self.discardable = self.upper = self.lower = self.naive_wrong = self.risen = 0

    def __repr__(self):
        return "full %d discardable %d upper %d lower %d; the chunk-start tail would wrongly discard %d; chunks whose tail rose %d" % (
            self.full, self.discardable, self.upper, self.lower, self.naive_wrong, self.risen)


def count(t, b, D, rep):
    """adds one replayed walk's counts to `t`, with `b` the query's Bounds"""
    with np.errstate(invalid="ignore"):
        for tail, B, new, kept in rep.chunks:
            if B is None:
                continue
            t.full += len(new)
            t.discardable += int((D[new] > B).sum())
            t.upper += int((b.upper[new] > B).sum())
            t.lower += int((b.lower[new] > B).sum())
            t.naive_wrong += int(((b.upper[new] > tail) & kept).sum())
            t.risen += int(B > tail)


def run_model(orc, g, metric, queries, limit, L, filters, emax_ymax=None):
    """([Replay], Tally) of a batch; `emax_ymax`: the table-wide maxima (default: of all rows of the graph)"""
    D = orc.distance_matrix(queries, g.vecs, metric, impl_of(orc))
    v16 = half_rows(g.vecs)
    with np.errstate(all="ignore"):
        yy16 = (v16 ** 2).sum(1)
    emax, ymax = maxima(g.vecs) if emax_ymax is None else emax_ymax
    t, reps = Tally(), []
    for i in range(queries.shape[0]):
        rep = replay(g, D[i], limit, L, filters[i])
        count(t, Bounds(metric, queries[i], v16, yy16, emax, ymax), D[i], rep)
        reps.append(rep)
    return reps, t


def check_tally(t, what, sandwich=True, naive=True):
    """the model's own conditions.  sandwich: the two sides within 1 % of each other, something provably discarded, and
    -- unless naive is False -- the input catches the naive rule (a neighbour the chunk-start tail would discard and the
    reference keeps).  naive = False is for searchSize 1 alone: an array of one entry is sorted, B is its only distance,
    so the two rules are the same rule there and no input can tell them apart."""
    assert t.lower <= t.upper <= t.discardable <= t.full, "%s: %r" % (what, t)
    if sandwich:
        assert t.lower > 0 and t.lower >= 0.99 * t.upper, "%s: %r" % (what, t)
        if naive:
            assert t.naive_wrong > 0, "%s: the chunk-start tail discards nothing wrongly here: %r" % (what, t)
        else:
            assert t.naive_wrong == 0 and t.risen == 0, "%s: %r" % (what, t)


# ---------------------------------------------------------------------------------------------- the inputs
class Case:
    """one table and one batch: export tuple, the oracle that holds it, queries, filters (sets of ids), limit, L"""

    def __init__(self, what, metric, d, ex, o, queries, filters, limit, L, sandwich=True, maxima_rows=None):
        self.what, self.metric, self.d, self.ex, self.o = what, metric, d, ex, o
        self.queries, self.filters, self.limit, self.L, self.sandwich = queries, filters, limit, L, sandwich
        self.g = Graph(*ex)
        self.emax_ymax = None if maxima_rows is None else maxima(maxima_rows)
        self.naive = L != 1  # (check_tally: an array of one entry is sorted)
        self._model = None
        self._prefixes = {}

    def model(self, orc):
        """([Replay], Tally), computed once"""
        if self._model is None:
            self._model = run_model(orc, self.g, self.metric, self.queries, self.limit, self.L, self.filters, self.emax_ymax)
        return self._model

    def check(self, t):
        check_tally(t, self.what, self.sandwich, self.naive)

    def prefix(self, orc, nq):
        """([Replay], Tally) of the batch's first `nq` queries, from the same replays as the whole batch's"""
        if nq not in self._prefixes:
            D = orc.distance_matrix(self.queries[:nq], self.g.vecs, self.metric, impl_of(orc))
            v16 = half_rows(self.g.vecs)
            with np.errstate(all="ignore"):
                yy16 = (v16 ** 2).sum(1)
            emax, ymax = maxima(self.g.vecs) if self.emax_ymax is None else self.emax_ymax
            reps = self.model(orc)[0][:nq]
            t = Tally()
            for i in range(nq):
                count(t, Bounds(self.metric, self.queries[i], v16, yy16, emax, ymax), D[i], reps[i])
            self._prefixes[nq] = (reps, t)
        return self._prefixes[nq]


def latent_rows(rng, n, d):
    lat = rng.standard_normal((12, d)).astype(np.float32)
    base = rng.standard_normal((n, 12)).astype(np.float32) @ lat + 0.2 * rng.standard_normal((n, d)).astype(np.float32)
    return (base / np.linalg.norm(base, axis=1, keepdims=True)).astype(np.float32)


FILTER_KINDS = ("5", "L-1", "L", "3L", "n/2", "mostly unknown")


def make_filters(rng, ids, nq, L):
    """filters of 5, L - 1, L (the start node meets a full, unsorted array), 3 L and n / 2 known ids, and one of 30 known
    ids among 200 unknown ones, in turn; `ids`: the table's ids without the start node's"""
    n = len(ids)
    out = []
    for i in range(nq):
        kind = FILTER_KINDS[i % len(FILTER_KINDS)]
        if kind == "mostly unknown":
            known = rng.choice(ids, size=min(30, n), replace=False)
            top = int(ids.max())
            unknown = top + 1000 + rng.choice(100000, size=200, replace=False)  # (near the table: a bitmap of them stays small)
            f = np.concatenate([known, unknown])
        else:
            size = {"5": 5, "L-1": max(L - 1, 1), "L": L, "3L": 3 * L, "n/2": n // 2}[kind]
            f = rng.choice(ids, size=min(size, n), replace=False)
        out.append(set(int(v) for v in f))
    return out


def _seed(metric, d, extra=0):
    return 7000 + d * 3 + METRICS.index(metric) + 1000 * extra


@functools.lru_cache(maxsize=None)
def _graph(orc, metric, d, full_rows):
    """n = 1 500 latent-12 unit rows under the oracle's R = 24 build, or i.i.d. unit rows with full adjacency rows (R = 64)"""
    n = 1500
    if full_rows:
        ex = M.full_row_export(orc, metric, d, n, _seed(metric, d, 1))
        return ex, M.load_oracle(orc, metric, d, ex)
    o = build_oracle_index(orc, latent_rows(np.random.default_rng(_seed(metric, d)), n, d), metric, R=24, L=40)
    return o.export(), o


# NG 1 (32: short, 128), 2 (160: padded, 256), 3, 4, 6 (640: padded, 768); full rows at NG 3 and 4
WIDTH_CASES = [(m, d, False) for d in (128, 384, 768, 32, 160, 256, 512, 640) for m in METRICS] + \
              [(m, d, True) for d in (384, 512) for m in METRICS]


@functools.lru_cache(maxsize=None)
def width_case(orc, metric, d, full_rows, limit=10, L=40):
    """32 queries, the six filter kinds in turn.  (The L cases reuse the d = 128 graphs with their own filters.)"""
    ex, o = _graph(orc, metric, d, full_rows)
    rng = np.random.default_rng(_seed(metric, d, 2) + L)
    queries = unit_rows(rng, N_QUERIES, d)
    filters = make_filters(rng, ex[0][ex[0] != 1].astype(np.int64), N_QUERIES, L)
    what = "%s d=%d %s L=%d limit=%d" % (metric, d, "R=64 full rows" if full_rows else "R=24", L, limit)
    return Case(what, metric, d, ex, o, queries, filters, limit, L)


# (L, limit); L = 40 is the width cases'.  1 and 2: min(k, L) is the whole array; 96 / 97: the last searchSize with the
# LDS hash set by routing and the first without (csrc/walk_plan.h) -- a filtered call keeps the hop on both sides
L_CASES = ((1, 1), (2, 1), (5, 5), (10, 10), (64, 10), (96, 10), (97, 10), (128, 10))
L_NO_STAGE = 129                 # past the kernel's two array registers: the float32 walk
L_REFUSED = (5, 10)              # searchSize < limit: refused by both sides (search.go:23-25)


@functools.lru_cache(maxsize=None)
def holes_case(orc, metric):
    """a table with deleted rows whose rows are not stored in id order: the ids are not consecutive (the filter resolves
    through the id -> slot table) and ascending ids are not ascending slots (Contains is answered from the id lists)"""
    d, n, L = 128, 1500, 40
    rng = np.random.default_rng(_seed(metric, d, 3))
    o = build_oracle_index(orc, latent_rows(rng, n, d), metric, R=24, L=40)
    gone = np.sort(rng.choice(np.arange(2, n + 2), size=120, replace=False)).astype(np.uint64)
    assert o.delete(gone) == 0
    ids, vecs, off, edges = o.export()
    perm = np.concatenate([[0], 1 + rng.permutation(len(ids) - 1)])
    assert ids[0] == 1
    deg = np.diff(off.astype(np.int64))
    p_off = np.zeros(len(off), dtype=np.uint64)
    p_off[1:] = np.cumsum(deg[perm])
    p_edges = np.concatenate([edges[int(off[i]):int(off[i + 1])] for i in perm])
    ex = (ids[perm], vecs[perm], p_off, p_edges)
    queries = unit_rows(rng, N_QUERIES, d)
    filters = make_filters(rng, ids[ids != 1].astype(np.int64), N_QUERIES, L)
    filters = [f | set(int(v) for v in rng.choice(gone, size=5)) for f in filters]  # ids of deleted rows: unknown
    return Case("%s holes, rows out of id order" % metric, metric, d, ex, o, queries, filters, 10, L)


@functools.lru_cache(maxsize=None)
def nan_case(orc, metric):
    """a NaN row among every query's seeds: the table-wide bound is NaN, nothing is discarded"""
    d, n, L = 128, 1500, 40
    rng = np.random.default_rng(_seed(metric, d, 4))
    rows = latent_rows(rng, n, d)
    rows[11] = np.nan  # id 13
    o = build_oracle_index(orc, rows, metric, R=24, L=40)
    ex = o.export()
    queries = unit_rows(rng, N_QUERIES, d)
    ids = ex[0][ex[0] != 1].astype(np.int64)
    filters = [f | {13} for f in make_filters(rng, ids[ids > 13], N_QUERIES, L)]  # the smallest id of each filter: a seed
    return Case("%s NaN row among the seeds" % metric, metric, d, ex, o, queries, filters, 10, L, sandwich=False)


NEAR_TIE_NOISE = (1e-3, 1e-5, 0.0)


@functools.lru_cache(maxsize=None)
def near_tie_case(orc, metric, noise):
    """rows in tight clusters: B sits inside a crowd of neighbours whose distances differ by less than the bound or not at
    all.  The two sides of the sandwich are far apart by construction: only their order and the answers are asserted."""
    d, n, L = 128, 1500, 30
    rng = np.random.default_rng(int(noise * 1e6) + 23 + METRICS.index(metric))
    centers = unit_rows(rng, 12, d)
    base = centers[rng.integers(0, 12, n)] + np.float32(noise) * rng.standard_normal((n, d)).astype(np.float32)
    base = (base / np.linalg.norm(base, axis=1, keepdims=True)).astype(np.float32)
    o = build_oracle_index(orc, base, metric, R=24, L=L)
    ex = o.export()
    queries = np.vstack([centers, base[:8], unit_rows(rng, 12, d)])
    filters = make_filters(rng, ex[0][ex[0] != 1].astype(np.int64), queries.shape[0], L)
    return Case("%s near ties, noise %g" % (metric, noise), metric, d, ex, o, queries, filters, 10, L, sandwich=False)


@functools.lru_cache(maxsize=None)
def dispatch_case(orc):
    """513 queries on the d = 128 cosine table, the filter kinds in turn; a call of the first 64 shares their filters"""
    ex, o = _graph(orc, "cosine", 128, False)
    rng = np.random.default_rng(9128)
    queries = unit_rows(rng, 513, 128)
    filters = make_filters(rng, ex[0][ex[0] != 1].astype(np.int64), 513, 40)
    return Case("default dispatch", "cosine", 128, ex, o, queries, filters, 10, 40)


DISPATCH_SIZES = (8, 64, 513)


@functools.lru_cache(maxsize=None)
def dispatch_beyond_hash_case(orc):
    """513 queries at searchSize 100 on the d = 128 cosine table; calls of 8 and 64 queries share the first ones"""
    ex, o = _graph(orc, "cosine", 128, False)
    rng = np.random.default_rng(9228)
    queries = unit_rows(rng, 513, 128)
    filters = make_filters(rng, ex[0][ex[0] != 1].astype(np.int64), 513, 100)
    return Case("default dispatch, L = 100", "cosine", 128, ex, o, queries, filters, 10, 100)


@functools.lru_cache(maxsize=None)
def _overflow(orc, metric):
    ex, queries = M.overflow_case(orc, metric)
    return ex, queries, M.load_oracle(orc, metric, 128, ex)


OVERFLOW_L = ((1, 1), (2, 1), (20, 10), (40, 10))  # (L, limit)


@functools.lru_cache(maxsize=None)
def overflow_case(orc, metric, L, limit):
    """a start node with an overflow list (more than 64 + 64 edges; tests/two_precision_model.py overflow_case): one
    expansion is several chunks, between which the array's last distance moves -- and, unsorted, can rise"""
    ex, queries, o = _overflow(orc, metric)
    rng = np.random.default_rng(_seed(metric, 128, 5) + L)
    filters = make_filters(rng, ex[0][ex[0] != 1].astype(np.int64), N_QUERIES, L)
    return Case("%s overflow list L=%d limit=%d" % (metric, L, limit), metric, 128, ex, o, queries, filters, limit, L)


HOSTILE_KINDS = M.HOSTILE_NO_DISCARD + M.HOSTILE_SANDWICH
HOSTILE_TABLES = [(m, d) for d in (128, 512) for m in ("cosine", "euclidean")]


@functools.lru_cache(maxsize=None)
def hostile_case(orc, metric, d, kind):
    """8 queries that break or strain the float16 copy of the query (tests/two_precision_model.py hostile_queries) with
    the first 8 filters of the width case.  Only the order of the counts is asserted of the model (sandwich = False): a
    bound that is infinite, NaN or wider than the distances proves nothing, and upper == 0 then makes the device's 0."""
    base = width_case(orc, metric, d, False)
    q = M.hostile_queries(d, kind)
    return Case("%s d=%d hostile %s" % (metric, d, kind), metric, d, base.ex, base.o, q, base.filters[:q.shape[0]], 10, 40,
                sandwich=False)


# ---------------------------------------------------------------------------------------------- the write paths
class Step:
    """one write of the write-path schedule: `ops` for the device -- ("iud", [(id, row or None)]) applied through
    InsertUpdateDelete one point per round, ("tx", ids, rows) inserted inside begin_write .. commit, ("delete", ids),
    ("compact",) -- and the checkpoint behind it: a Case over the oracle's graph after the same write, the maxima the
    device carries, whether anything can be discarded"""

    def __init__(self, what, ops, case, expect_none):
        self.what, self.ops, self.case, self.expect_none = what, ops, case, expect_none


def _scaled(rng, n, d, norm):
    return (unit_rows(rng, n, d) * np.float32(norm)).astype(np.float32)


WRITE_GROWS_PAST = 2048  # the 1 501 rows loaded sit in a table of 2 048 (capacities double from 1 024): the transaction grows it


@functools.lru_cache(maxsize=None)
def write_path_steps(orc, metric):
    """The filtered twin of test_gpu_two_precision_bound.py::test_maxima_through_every_write_path, shorter.  The maxima
    are those of every row converted since the last full conversion (load, compact), deleted rows included.  Each
    checkpoint's filters are drawn over the live ids, and every one of them also names ids the last write deleted,
    updated and added."""
    d, L, limit = 128, 40, 10
    ex0, o_loaded = _graph(orc, metric, d, False)
    o = M.load_oracle(orc, metric, d, ex0, L=40)  # (this one is written to; R = 64 from here on, on both sides)
    rng = np.random.default_rng(_seed(metric, d, 6))
    queries = unit_rows(rng, N_QUERIES, d)
    state = {"maxima": maxima(ex0[1]), "next": 5000}
    steps = []

    def checkpoint(what, ops, deleted=(), updated=(), added=(), expect_none=False, full_conversion=False):
        ex = o.export()
        if full_conversion:
            state["maxima"] = maxima(ex[1])
        live = ex[0][ex[0] != 1].astype(np.int64)
        named = set(int(v) for v in list(deleted)[:3] + list(updated)[:3] + list(added)[:3])
        filters = [f | named for f in make_filters(rng, live, N_QUERIES, L)]
        c = Case("%s write path: %s" % (metric, what), metric, d, ex, M.load_oracle(orc, metric, d, ex), queries, filters,
                 limit, L, sandwich=not expect_none)
        c.emax_ymax = state["maxima"]
        steps.append(Step(what, ops, c, expect_none))

    def apply(changes):
        """InsertUpdateDelete's order (fuzz_parity.trial): inserts, then deletes and updates' old rows, then the updates"""
        have = set(int(v) for v in o.export(with_vectors=False)[0])
        for i, row in changes:
            if row is not None and i not in have:
                assert o.insert(i, row) == 0
        gone = [i for i, row in changes if i in have]
        if gone:
            assert o.delete(np.array(gone, dtype=np.uint64)) == 0
        for i, row in changes:
            if row is not None and i in have:
                assert o.insert(i, row) == 0
        rows = [row for _, row in changes if row is not None]
        if rows:
            state["maxima"] = M.join_maxima(state["maxima"], maxima(np.stack(rows)))

    def new_ids(k):
        first = state["next"]
        state["next"] += k
        return list(range(first, first + k))

    checkpoint("load", [])
    ins, upd, dele = new_ids(3), [100, 101], [200, 201, 202]
    changes = [(i, r) for i, r in zip(ins, _scaled(rng, 3, d, 8.0))] + [(i, None) for i in dele] + \
              [(i, r) for i, r in zip(upd, _scaled(rng, 2, d, 1e-3))]
    apply(changes)
    checkpoint("InsertUpdateDelete, inserts of norm 8, updates of norm 1e-3, deletes", [("iud", changes)], dele, upd, ins)
    ids, rows = new_ids(560), _scaled(rng, 560, d, 1e-3)
    apply(list(zip(ids, rows)))
    checkpoint("begin_write .. commit that grows the table, norm 1e-3", [("tx", ids, rows)], added=ids)
    big = new_ids(1)
    row = unit_rows(rng, 1, d)
    row[0, 17] = 1e6
    apply([(big[0], row[0])])
    checkpoint("a row with an element of 1e6", [("iud", [(big[0], row[0])])], added=big, expect_none=True)
    apply([(big[0], None)])
    checkpoint("that row deleted", [("delete", big)], deleted=big, expect_none=True)
    checkpoint("compact", [("compact",)], deleted=big, full_conversion=True)
    return steps


@functools.lru_cache(maxsize=None)
def reader_case(orc):
    """the table, queries and filters of the reader-during-commits test, and the rows the writer adds one by one"""
    base = width_case(orc, "cosine", 128, False)
    rng = np.random.default_rng(9333)
    return base, _scaled(rng, 10, 128, 1.0)
