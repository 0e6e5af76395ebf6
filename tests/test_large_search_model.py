"""The large-searchSize cases (tests/large_search_model.py) reach what they are meant to reach -- from the oracle alone,
without a GPU.  The kernels count nothing for a test's sake, so these conditions are the proof that the GPU tests of
tests/test_gpu_large_search_size.py ran the candidate array full, overfull, tied across its registers, or never full.

A.  n = 10 000 rows of d = 32.  Every query at every searchSize L computes 2 * L < n_dist < 0.8 * n distances: the
    array is full for most of the walk and the walk is no exhaustive scan.  Measured (min .. max n_dist over the 16
    queries; euclidean / cosine / dot):
      L =  97: 1 953 .. 2 118 / 1 980 .. 2 139 / 1 316 .. 1 535      L = 257: 3 882 .. 4 055 / 3 814 .. 4 092 / 2 867 .. 3 065
      L = 127: 2 377 .. 2 559 / 2 387 .. 2 592 / 1 696 .. 1 864      L = 320: 4 412 .. 4 609 / 4 351 .. 4 647 / 3 365 .. 3 512
      L = 128: 2 390 .. 2 574 / 2 404 .. 2 592 / 1 703 .. 1 875      L = 384: 4 882 .. 5 082 / 4 819 .. 5 127 / 3 809 .. 3 936
      L = 129: 2 410 .. 2 586 / 2 419 .. 2 592 / 1 711 .. 1 883      L = 385: 4 892 .. 5 090 / 4 828 .. 5 133 / 3 814 .. 3 948
      L = 191: 3 193 .. 3 365 / 3 185 .. 3 391 / 2 314 .. 2 494      L = 448: 5 318 .. 5 500 / 5 264 .. 5 538 / 4 195 .. 4 352
      L = 192: 3 210 .. 3 380 / 3 195 .. 3 414 / 2 327 .. 2 500      L = 511: 5 715 .. 5 883 / 5 649 .. 5 916 / 4 545 .. 4 695
      L = 193: 3 217 .. 3 390 / 3 211 .. 3 414 / 2 334 .. 2 506      L = 512: 5 719 .. 5 888 / 5 661 .. 5 922 / 4 551 .. 4 703
      L = 256: 3 871 .. 4 044 / 3 804 .. 4 084 / 2 867 .. 3 065
    The small table (n = 300 < L = 512) is scanned whole: n_dist = 301 for every query, and 300 results; at
    limit = L = 97, 128, 129, 200 some of its queries return L - 1 results (the start node is in the final array).
B.  The integer grid at n = 12 000: 2 * L < n_dist < 0.8 * n holds too (plain: 752 .. 990 at L = 129, 1 064 .. 1 327
    at 192, 1 324 .. 1 578 at 256, 2 279 .. 2 560 at 512), at least 90 % of the returned distances repeat their
    predecessor (75 % of a filtered search's, whose result set takes single insertions), and for every L some query
    has equal distances on both sides of every register boundary (entries 63 | 64, 127 | 128, ... 447 | 448) -- plain
    and filtered.
C.  The "exactly L" and "n // 2" filters seed the array with exactly L entries, the others with fewer.
D.  Every width computes more than L distances at L = 129 and 256.
E.  The overflow-list table's start node has more than 128 edges; the 513-query sample holds the last query.
F.  The routing band of every quantizer shape, from M * K alone.
"""
import numpy as np
import pytest

from tests import large_search_model as LM
from tests import visited_spill_model as S


@pytest.mark.parametrize("metric", LM.A_METRICS)
def test_the_narrow_table_fills_the_array_without_a_scan(oracle, metric):
    t = LM.a_table(oracle, metric)
    for L in LM.A_L:
        lo, hi = LM.n_dist_range(t, L, L)
        print("A %s L=%d: n_dist %d .. %d of n = %d" % (metric, L, lo, hi, t.n))
        assert 2 * L < lo and hi < 0.8 * t.n, (metric, L, lo, hi)
        for q in t.queries:
            assert len(t.o.search(q, L, L)[0]) >= L - 1  # a full array: all of it comes back, the start node left out


def test_the_small_table_never_fills_the_array(oracle):
    t = LM.small_table(oracle)
    for q in t.queries:
        ids, _, _, tr = t.o.search(q, 512, 512)
        assert len(ids) == LM.N_SMALL and tr.n_dist == LM.N_SMALL + 1
        assert 1 not in set(int(v) for v in ids)
    # limit = searchSize < n: some final array holds the start node, and that query's row is one entry short
    for L in LM.SHORT_ROW_L:
        counts = [len(t.o.search(q, L, L)[0]) for q in t.queries]
        assert set(counts) <= {L - 1, L} and L - 1 in counts, (L, counts)


@pytest.mark.parametrize("filtered", [False, True])
def test_ties_straddle_every_register_boundary(oracle, filtered):
    t = LM.tie_table(oracle)
    for L in LM.TIE_L:
        if not filtered:
            lo, hi = LM.n_dist_range(t, L, L)
            print("B ties L=%d: n_dist %d .. %d of n = %d" % (L, lo, hi, t.n))
            assert 2 * L < lo and hi < 0.8 * t.n, (L, lo, hi)
        straddled = {b: False for b in LM.BOUNDARIES if b < L}
        for i, q in enumerate(t.queries):
            d = t.o.search(q, L, L, filter_ids=sorted(t.filters[i]) if filtered else None)[1]
            assert len(d) >= L - 1
            # (filtered: the result set is built by single insertions, fewer of its distances repeat)
            assert int((d[1:] == d[:-1]).sum()) >= (0.75 if filtered else 0.9) * len(d), (L, i)
            for b in straddled:
                straddled[b] = straddled[b] or bool(d[b - 1] == d[b])
        assert all(straddled.values()), (L, straddled)


@pytest.mark.parametrize("metric", LM.FILTER_METRICS)
def test_filters_seed_the_array_as_meant(oracle, metric):
    t = LM.a_table(oracle, metric)
    for L, limit in LM.FILTER_CASES:
        filters = LM.filters_of(oracle, metric, L, limit)
        for i, f in enumerate(filters):
            seeds, kind = LM.seeds_of(t, f, L), i % 6
            if kind in (1, 2):
                assert seeds == L, (L, limit, i, seeds)   # the array starts full and unsorted
            else:
                assert seeds < min(L, 64), (L, limit, i, seeds)
            if kind == 0:
                assert len(f) < limit
            if kind == 3:
                assert len(f) == 42 and seeds == 40
            if kind == 4:
                assert 1 in f
            n = len(t.o.search(t.queries[i % LM.NQ], limit, L, filter_ids=sorted(f))[0])
            assert n <= min(limit, len(f & set(int(v) for v in t.ids))), (L, limit, i, n)
            if kind in (1, 2):
                assert n == limit, (L, limit, i, n)   # a full result row: limit > 64 crosses a register of rid / rd


@pytest.mark.parametrize("d", LM.WIDTHS)
def test_every_width_overfills_the_array(oracle, d):
    for metric in LM.WIDTH_METRICS:
        t = LM.width_table(oracle, metric, d)
        for L in LM.WIDTH_L:
            lo, hi = LM.n_dist_range(t, 10, L)
            assert lo > L, (metric, d, L, lo)
        for f in t.filters:
            assert LM.seeds_of(t, f, 129) == 129


def test_the_reuse_and_overflow_cases(oracle):
    case = S.overflow_case(oracle, LM.OVERFLOW_L, 10)
    off = case.ex[2]
    assert int(off[1] - off[0]) > 64 + 64, "the start node must carry an overflow list"
    lo = min(case.o.search(q, 10, LM.OVERFLOW_L)[3].n_dist for q in case.queries)
    assert lo > LM.OVERFLOW_L
    picked = LM.many_checked()
    assert picked[:8] == list(range(8)) and picked[-1] == LM.MANY - 1 and 512 in picked
    assert [L for _, L, _ in LM.REUSE_STEPS] == [512, 512, 128, 97, 512, 50, 129]


def test_the_quantizer_shapes_lie_in_their_routing_bands():
    """from M * K alone: which searches of section F the bitset kernel with an LDS table serves"""
    want = {(8, 16): ("hash", "bitset lds"), (32, 256): ("bitset lds", "bitset lds"), (64, 256): ("bitset lds", "bitset lds"),
            (96, 192): ("bitset global", "bitset global"), (128, 64): ("multi-wave", "bitset lds")}
    for d, M, K in LM.PQ_SHAPES:
        assert d % M == 0
        assert (LM.pq_route(M, K, 50), LM.pq_route(M, K, 97)) == want[(M, K)], (M, K)
        for L in LM.PQ_L:
            assert LM.pq_route(M, K, L) == want[(M, K)][1]
    assert 8 * 16 <= 2048 < 32 * 256 < 64 * 256 == 16384 < 96 * 192
    assert 64 * 256 * 4 == LM.LDS_TABLE_BYTES and 128 * 64 * 4 == 32 * 1024
    assert 96 not in LM.WIDE_M and 96 * 192 * 4 > LM.LDS_TABLE_BYTES   # no multi-wave shape, too large for LDS


@pytest.mark.parametrize("d,M,K", LM.PQ_SHAPES)
def test_the_quantized_walks_overfill_the_array(oracle, d, M, K):
    for metric in LM.PQ_METRICS:
        t = LM.pq_table(oracle, metric, d, M, K)
        for L in (50,) + LM.PQ_L:
            lo, hi = LM.n_dist_range(t, 10, L)
            assert lo > L and (L > 129 or hi < 0.8 * t.n), (metric, M, K, L, lo, hi)
        for f in t.filters_half:
            assert LM.seeds_of(t, f, 129) == 129
