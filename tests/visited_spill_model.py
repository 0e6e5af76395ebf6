"""The inputs of the forced visited-set spill tests, and the conditions that make them spill.

Every hash-set walk keeps its visited set in an LDS table (visited_set.h HashVisited) and, once a query has marked
more than `hash_limit` ids (default 6000 = kHashLimit), replays the table into the query's HBM bitset and carries on
there, in the middle of the walk.  A test table of a few thousand rows never marks 6000 ids, so the tests lower the
limit: tests/test_gpu_visited_spill.py runs each batch below at hash_limit = T for every T of `Case.sweep()` and asks for
the oracle's answers and for answers bit-identical to the T = 0 run.  With kHashCap = 8192 the table's limit equals T and
a query spills as soon as it has marked more than T ids; a walk's marks are the start node and every new neighbour,
which is what the oracle counts as n_dist.

What is stated here, from the oracle alone and without a GPU (tests/test_visited_spill_model.py), is that the spill
HAPPENS where the GPU tests mean it to: at every T but 0 and the median every query of the batch marks more than T + 1
ids, at the median between a quarter and three quarters do, and `lo // 2` lies past searchSize + 64, so the candidate
array is full (and a first stage is discarding) when the set moves.  No kernel counts its spills -- the timed walks do
not gain a register for a test's sake -- so these conditions are the proof that the path ran.

The tables and queries are the existing case makers' (tests/two_precision_model.py), built once per session.
"""
import atexit
import functools

import numpy as np

from tests import filtered_two_precision_model as F
from tests import two_precision_model as M
from tests.helpers import unit_rows

LIMIT = 10
FIXED_T = (0, 1, 63, 64)          # the control; a spill in the start node's row; either side of one full chunk
OVERFLOW_T = (0, 1, 64, 130)      # a start node of more than 128 edges: the spill lands inside its chunks


@functools.lru_cache(maxsize=None)
def _width(orc, metric, d):
    return M.width_case(orc, metric, d)


@functools.lru_cache(maxsize=None)
def _l(orc, metric, d):
    return M.l_case(orc, metric, d)


@functools.lru_cache(maxsize=None)
def _no_stage(orc, metric, d):
    """the tables of test_gpu_two_precision_bound.py::test_widths_without_the_stage: a tail chain (d = 100), NG = 8"""
    seed = 300 + d
    return M.full_row_export(orc, metric, d, 1500, seed), unit_rows(np.random.default_rng(seed + 7), M.N_QUERIES, d)


@functools.lru_cache(maxsize=None)
def _overflow(orc):
    return M.overflow_case(orc, "cosine")


@functools.lru_cache(maxsize=None)
def _dispatch(orc, d):
    return M.dispatch_case(orc, d)


class Case:
    """one table and one batch; the oracle, its per-query marks, the sweep and the replays are computed once"""

    def __init__(self, orc, what, metric, d, ex, queries, limit, L, fixed=None, filters=None):
        self.orc, self.what, self.metric, self.d, self.ex = orc, what, metric, d, ex
        self.queries, self.limit, self.L, self.fixed, self.filters = queries, limit, L, fixed, filters
        self._g = self._o = self._marks = None
        self._reps = {}

    @property
    def g(self):
        if self._g is None:
            self._g = M.Graph(*self.ex)
        return self._g

    @property
    def o(self):
        if self._o is None:
            self._o = M.load_oracle(self.orc, self.metric, self.d, self.ex)
        return self._o

    def marks(self):
        """ids each query's walk marks in its search set.  Plain: the oracle's n_dist.  Filtered: n_dist also counts the
        result set's distances, so the new neighbours of the replay's chunks are counted instead (seeds and start node
        left out: a lower bound), after the replay has been compared with the oracle's filtered walk."""
        if self._marks is None:
            if self.filters is None:
                self._marks = np.array([self.o.search(q, self.limit, self.L)[3].n_dist for q in self.queries], dtype=np.int64)
            else:
                reps = self.replays()[0]
                for i, r in enumerate(reps):
                    tr = self.o.search(self.queries[i], self.limit, self.L, filter_ids=sorted(self.filters[i]))[3]
                    assert (r.n_hop, r.n_dist, r.n_edges) == (tr.n_hop, tr.n_dist, tr.n_edges), "%s query %d" % (self.what, i)
                self._marks = np.array([sum(len(c[2]) for c in r.chunks) for r in reps], dtype=np.int64)
        return self._marks

    def lo_med(self):
        m = self.marks()
        return int(m.min()), int(np.median(m))

    def sweep(self):
        if self.fixed is not None:
            return self.fixed
        lo, med = self.lo_med()
        return FIXED_T + (lo // 2, lo - 2, med)

    def replays(self, nq=None):
        """([Replay], Tally of the float16 model, D) of the batch's first nq queries (plain), ([Replay], Tally) (filtered)"""
        nq = self.queries.shape[0] if nq is None else nq
        if nq not in self._reps:
            if self.filters is None:
                self._reps[nq] = M.run_model(self.orc, self.g, self.metric, self.queries[:nq], self.limit, self.L)
            else:
                self._reps[nq] = F.run_model(self.orc, self.g, self.metric, self.queries[:nq], self.limit, self.L, self.filters[:nq])
        return self._reps[nq]


def check_conditions(case):
    """the conditions of a GPU case, from the oracle alone; returns the line the CPU test prints"""
    m, sweep = case.marks(), case.sweep()
    lo, med = case.lo_med()
    shares = []
    for T in sweep:
        past = int((m > T + 1).sum())
        shares.append("T=%d: %d/%d" % (T, past, m.size) if T else "T=0 (the control): 0/%d past 6000" % m.size)
        if T == 0:
            assert m.max() <= 6000, "%s: the control spills (%d marks)" % (case.what, m.max())
        elif case.fixed is None and T == med:
            assert m.size / 4 <= past <= 3 * m.size / 4, "%s: %d of %d queries pass the median %d" % (case.what, past, m.size, T)
        else:
            assert past == m.size, "%s: only %d of %d queries mark more than T + 1 = %d ids" % (case.what, past, m.size, T + 1)
    if case.fixed is None:
        assert lo // 2 > case.L + 64, "%s: lo // 2 = %d is not past searchSize + 64 = %d" % (case.what, lo // 2, case.L + 64)
        assert len(set(sweep)) == len(sweep), "%s: the sweep repeats a limit: %r" % (case.what, sweep)
    return "%s: lo %d med %d; queries past T + 1: %s" % (case.what, lo, med, ", ".join(shares))


# ---------------------------------------------------------------------------------------------- the cases
# (metric, d, searchSize).  d = 100: a tail chain; 384: NG 3; 1024: NG 8
F32_CASES = [(m, d, L) for m in ("cosine", "euclidean") for d in (100, 384, 1024) for L in (40, 96)]
# M.width_case at searchSize 40; M.l_case at d = 384 and searchSize 96, the last with the hash set
F16_CASES = [(m, d, 40) for m in M.METRICS for d in (128, 384, 768)] + [(m, 384, 96) for m in M.METRICS]
INT8_CASES = [(m, d, 40) for m in ("cosine", "dot") for d in (128, 352, 384)]  # 352: a partial last group
OVERFLOW_L = (1, 2)
WIDE16_CASES = [(m, d, 40) for m in ("cosine", "euclidean") for d in (128, 384, 1024)]  # 1024: NG 8, eight waves
WIDE16_OVERFLOW_L = (2, 20)
WIDE8_QUERIES = 300               # 257 .. 512 queries: eight waves per query and nobody ahead of the walker
WIDE8_CHECKED = 32                # compared with the oracle one by one; the rest with the T = 0 run
WIDE8_CASES = [("cosine", 128), ("cosine", 384)]
FILTERED_QUERIES = 24
SEAM = (512, 513)                 # csrc/walk_plan.h: 512 queries stay on the many-waves kernel at d = 128


@functools.lru_cache(maxsize=None)
def plain_case(orc, metric, d, L):
    """the one-wave walks' batches: 32 queries, limit 10"""
    if d in M.NO_STAGE_WIDTHS:
        ex, queries = _no_stage(orc, metric, d)
    elif L == 96:
        ex, queries = _l(orc, metric, d)
    else:
        ex, queries = _width(orc, metric, d)[:2]
    return Case(orc, "%s d=%d L=%d" % (metric, d, L), metric, d, ex, queries, LIMIT, L)


@functools.lru_cache(maxsize=None)
def overflow_case(orc, L, limit=1):
    ex, queries = _overflow(orc)
    return Case(orc, "cosine overflow list L=%d" % L, "cosine", 128, ex, queries, limit, L, fixed=OVERFLOW_T)


@functools.lru_cache(maxsize=None)
def wide8_case(orc, metric, d):
    """300 queries: the width case's 32 and 268 more"""
    ex, queries = _width(orc, metric, d)[:2]
    more = unit_rows(np.random.default_rng(4100 + d), WIDE8_QUERIES - queries.shape[0], d)
    return Case(orc, "%s d=%d %d queries" % (metric, d, WIDE8_QUERIES), metric, d, ex, np.vstack([queries, more]), LIMIT, 40)


@functools.lru_cache(maxsize=None)
def filtered_case(orc):
    """cosine, d = 384, 24 queries with filters of 5, L and n / 2 ids in turn"""
    d, L = 384, 40
    ex, queries = _width(orc, "cosine", d)[:2]
    rng = np.random.default_rng(4200)
    ids = ex[0][ex[0] != 1].astype(np.int64)
    sizes = (5, L, len(ids) // 2)
    filters = [set(int(v) for v in rng.choice(ids, size=sizes[i % 3], replace=False)) for i in range(FILTERED_QUERIES)]
    return Case(orc, "cosine d=384 filtered", "cosine", d, ex, queries[:FILTERED_QUERIES], LIMIT, L, filters=filters)


@functools.lru_cache(maxsize=None)
def seam_case(orc):
    """M.dispatch_case at d = 128: 513 queries; the one limit of the seam test is lo // 2"""
    ex, queries = _dispatch(orc, 128)
    c = Case(orc, "cosine d=128 seam", "cosine", 128, ex, queries, LIMIT, 40)
    c.fixed = (0, c.lo_med()[0] // 2)
    return c


@atexit.register
def _drop_the_cases():
    """the cached cases hold oracle indexes: freed while the oracle's library is still loaded"""
    for f in (plain_case, overflow_case, wide8_case, filtered_case, seam_case):
        f.cache_clear()
