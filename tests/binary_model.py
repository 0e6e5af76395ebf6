"""CPU model of the binary quantizer and of the Vamana walk over an arbitrary pair distance: numpy and plain Python
only, no GPU, no arithmetic shared with the kernels.

  * encode / fit_threshold / hamming / jaccard / expand restate shard/vectorstore/binary.go:103-129,152-173 and
    distance/distance.go:45-67;
  * Graph restates greedySearch (search.go:9-102, with filter), DistSet (distset.go:133-238), robustPrune
    (search.go:106-138) and insertSinglePoint (insert.go:16-68) literally, parameterised by the pair distance.  With
    hamming it must agree with oracle.Index(d, "euclidean") over the 0/1 expansion of the codes
    (tests/test_binary_model.py); for jaccard, which has no float-metric twin, it is the oracle."""
import numpy as np

STARTID = 1


def n_words(d):
    return (d + 63) // 64  # binary.go:107-111


def encode(vectors, thr):
    """codes [n][W] uint64: bit i % 64 of word i / 64 is set iff v[i] > thr[i] (binary.go:123-127; false for NaN)"""
    v = np.atleast_2d(np.asarray(vectors, dtype=np.float32))
    thr = np.asarray(thr, dtype=np.float32)
    n, d = v.shape
    with np.errstate(invalid="ignore"):
        bits = v > thr[None, :]
    codes = np.zeros((n, n_words(d)), dtype=np.uint64)
    for i in range(d):
        codes[:, i // 64] |= bits[:, i].astype(np.uint64) << np.uint64(i % 64)
    return codes


def fit_threshold(X):
    """binaryQuantizer.Fit, first pass (binary.go:152-173): one float32 add per row, in order, one float32 division"""
    X = np.asarray(X, dtype=np.float32)
    acc = np.zeros(X.shape[1], dtype=np.float32)
    with np.errstate(all="ignore"):
        for r in X:
            acc += r
        return acc / np.float32(X.shape[0])


def _popcount(a):
    a = np.ascontiguousarray(a, dtype=np.uint64)
    return np.unpackbits(a.view(np.uint8).reshape(a.shape + (8,)), axis=-1).sum(axis=(-1, -2)).astype(np.int64)


def hamming(x, y):
    """hammingDistance (distance.go:45-54) of two codes -> float32"""
    return np.float32(int(_popcount(np.bitwise_xor(np.asarray(x, np.uint64), np.asarray(y, np.uint64)))))


def jaccard(x, y):
    """jaccardDistance (distance.go:56-67)"""
    x, y = np.asarray(x, np.uint64), np.asarray(y, np.uint64)
    inter, union = int(_popcount(np.bitwise_and(x, y))), int(_popcount(np.bitwise_or(x, y)))
    if union == 0:
        return np.float32(0)
    return np.float32(np.float32(1) - np.float32(inter) / np.float32(union))


def distance_matrix(metric, q, c):
    """out[i, j] = metric(q[i], c[j]) for code arrays [nq][W], [nc][W]"""
    q, c = np.asarray(q, np.uint64), np.asarray(c, np.uint64)
    if metric == "hamming":
        return _popcount(np.bitwise_xor(q[:, None, :], c[None, :, :])).astype(np.float32)
    inter = _popcount(np.bitwise_and(q[:, None, :], c[None, :, :])).astype(np.float32)
    union = _popcount(np.bitwise_or(q[:, None, :], c[None, :, :])).astype(np.float32)
    with np.errstate(all="ignore"):
        out = np.float32(1) - inter / union
    out[union == 0] = np.float32(0)
    return out.astype(np.float32)


def expand(codes, d):
    """codes [n][W] -> 0.0 / 1.0 float32 rows [n][d]: hamming(x, y) == squared euclidean distance of the expansions"""
    codes = np.atleast_2d(np.asarray(codes, dtype=np.uint64))
    out = np.zeros((codes.shape[0], d), dtype=np.float32)
    for i in range(d):
        out[:, i] = ((codes[:, i // 64] >> np.uint64(i % 64)) & np.uint64(1)).astype(np.float32)
    return out


def code_int(code):
    """a code's words as one Python integer (word 0 lowest): the walk's pair functions work on these"""
    v = 0
    for w in reversed(np.asarray(code, dtype=np.uint64).tolist()):
        v = (v << 64) | int(w)
    return v


def _ones(v):
    return bin(v).count("1")


def hamming_int(x, y):
    return np.float32(_ones(x ^ y))


def jaccard_int(x, y):
    union = _ones(x | y)
    if union == 0:
        return np.float32(0)
    return np.float32(np.float32(1) - np.float32(_ones(x & y)) / np.float32(union))


PAIR = {"hamming": hamming_int, "jaccard": jaccard_int}  # pair functions over code_int() values


class _Elem:
    __slots__ = ("id", "dist", "visited", "removed")

    def __init__(self, pid, dist):
        self.id, self.dist, self.visited, self.removed = pid, dist, False, False


class DistSet:
    """distset.go:133-238; the visited set is a Python set (CheckAndVisit :174)"""

    def __init__(self, capacity, dist_fn, counter):
        self.items, self.cap, self.seen, self.dist_fn, self.sorted_until, self.counter = [], capacity, set(), dist_fn, 0, counter

    def add_with_limit(self, ids):  # :166-200
        for p in ids:
            if p in self.seen:
                continue
            self.seen.add(p)
            d = self.dist_fn(p)
            self.counter[0] += 1
            if len(self.items) == self.cap and d > self.items[self.cap - 1].dist:
                continue
            e = _Elem(p, d)
            if len(self.items) < self.cap:
                self.items.append(e)
                self.sorted_until += 1
            else:
                self.items[-1] = e
            i = len(self.items) - 1
            while i > 0 and self.items[i].dist < self.items[i - 1].dist:
                self.items[i], self.items[i - 1] = self.items[i - 1], self.items[i]
                i -= 1

    def add(self, ids):  # :203-211
        for p in ids:
            if p in self.seen:
                continue
            self.seen.add(p)
            self.items.append(_Elem(p, self.dist_fn(p)))
            self.counter[0] += 1

    def add_already_unique(self, elem):  # :219-221 (a copy, as Go copies the struct)
        self.items.append(_Elem(elem.id, elem.dist))

    def sort(self):  # :223-238
        for i in range(self.sorted_until, len(self.items)):
            j = i
            while j > 0 and self.items[j].dist < self.items[j - 1].dist:
                self.items[j], self.items[j - 1] = self.items[j - 1], self.items[j]
                j -= 1
        self.sorted_until = len(self.items)


class SearchOut:
    def __init__(self, ids, dists, visit, n_dist, n_hop, n_edges):
        self.ids, self.dists, self.visit, self.n_dist, self.n_hop, self.n_edges = ids, dists, visit, n_dist, n_hop, n_edges


class Graph:
    """IndexVamana over a store of bit codes with pair distance `pair(code_int, code_int) -> float32` (PAIR[...])"""

    def __init__(self, pair, degree_bound, search_size, alpha):
        self.pair, self.R, self.L, self.alpha = pair, degree_bound, search_size, np.float32(alpha)
        self.order, self.codes, self.edges = [], {}, {}  # ids in storage order, id -> code, id -> [neighbour ids]

    def set_start(self, code):
        self.order, self.codes, self.edges = [STARTID], {STARTID: code_int(code)}, {STARTID: []}

    def load(self, ids, codes, offsets, edges):
        self.order = [int(v) for v in ids]
        self.codes = {int(v): code_int(codes[i]) for i, v in enumerate(ids)}
        self.edges = {int(v): [int(e) for e in edges[int(offsets[i]):int(offsets[i + 1])] if int(e) in self.codes]
                      for i, v in enumerate(ids)}

    def export(self):
        offsets, edges = [0], []
        for v in self.order:
            edges.extend(self.edges[v])
            offsets.append(len(edges))
        return (np.array(self.order, dtype=np.uint64), np.array(offsets, dtype=np.uint64),
                np.array(edges, dtype=np.uint64))

    def greedy_search(self, qcode, k, search_size, filt=None):  # search.go:9-102
        qcode = qcode if isinstance(qcode, int) else code_int(qcode)
        counter = [0]
        dist_fn = lambda p: self.pair(qcode, self.codes[p])
        search_set = DistSet(search_size, dist_fn, counter)
        visited = DistSet(search_size * 2, dist_fn, counter)
        if search_size < k:
            raise ValueError("searchSize (%d) must be greater than k (%d)" % (search_size, k))
        result = search_set
        fset = None
        if filt is not None:
            fsorted = sorted(int(v) for v in filt)
            fset = set(fsorted)
            result = DistSet(k, dist_fn, counter)
            points = [p for p in fsorted[:search_size] if p in self.codes]  # :40-45, GetMany skips unknown ids
            search_set.add(points)
            result.add_with_limit(points)
        search_set.add_with_limit([STARTID])  # :61
        visit, n_edges = [], 0
        i = 0
        while i < min(len(search_set.items), search_size):  # :65
            e = search_set.items[i]
            if e.visited:
                i += 1
                continue
            visited.add_already_unique(e)
            e.visited = True
            visit.append(e.id)
            nbrs = self.edges[e.id]
            n_edges += len(nbrs)
            search_set.add_with_limit(nbrs)  # :90
            if fset is not None and e.id in fset:  # :93-95
                result.add_with_limit([e.id])
            i = 0
        visited.sort()  # :100
        return result, visited, SearchOut(None, None, visit, counter[0], len(visit), n_edges)

    def search(self, qcode, limit, search_size, filt=None):
        """IndexVamana.Search (vamana.go:278-310): start node removed, cut at limit"""
        result, _, out = self.greedy_search(qcode, limit, search_size, filt)
        items = [e for e in result.items if e.id != STARTID][:limit]
        out.ids = np.array([e.id for e in items], dtype=np.uint64)
        out.dists = np.array([e.dist for e in items], dtype=np.float32)
        return out

    def robust_prune(self, node, cand):  # search.go:106-138
        self.edges[node] = []
        items = cand.items
        for i in range(len(items)):
            c = items[i]
            if c.removed or c.id == node:
                continue
            self.edges[node].append(c.id)
            if len(self.edges[node]) >= self.R:
                break
            cc = self.codes[c.id]
            for j in range(i + 1, len(items)):
                nx = items[j]
                if nx.removed:
                    continue
                if np.float32(self.alpha * self.pair(cc, self.codes[nx.id])) < nx.dist:  # :132
                    nx.removed = True

    def insert(self, pid, code):  # insert.go:16-68
        pid = int(pid)
        code = code_int(code)
        self.codes[pid] = code
        self.order.append(pid)
        _, visited, _ = self.greedy_search(code, 1, self.L)
        self.edges[pid] = []
        self.robust_prune(pid, visited)
        for nb in list(self.edges[pid]):
            if len(self.edges[nb]) + 1 > self.R:
                cb = self.codes[nb]
                cand = DistSet(len(self.edges[nb]) + 1, lambda p, cb=cb: self.pair(cb, self.codes[p]), [0])
                cand.add(self.edges[nb])
                cand.add([pid])
                cand.sort()
                self.robust_prune(nb, cand)
            else:
                self.edges[nb].append(pid)
