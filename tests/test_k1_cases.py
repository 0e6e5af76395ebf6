"""tests/k1_cases.py on the CPU: the shape table reaches what it says it reaches (by the restated dispatch), the
restatement carries the constants of semadb_amd/csrc/distance_tile.hip, and the special-value inputs make the oracle
itself produce every class of value the GPU tests mean to compare."""
import os
import re

import numpy as np
import pytest

from tests import k1_cases as k1

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TILE_SRC = os.path.join(ROOT, "semadb_amd", "csrc", "distance_tile.hip")

SWEEP_ROUTES = k1.routes([c for nblk in k1.SWEEP for c in k1.SWEEP[nblk]])
ALL_ROUTES = k1.routes(k1.all_cases())


def _reached(routes, family):
    return {r.nblk for r, _, _ in routes if r.family == family}


def test_constants_are_the_source_s():
    """the numbers k1_route carries are the ones the launcher is compiled with"""
    src = open(TILE_SRC).read()

    def const(pattern):
        m = re.search(pattern, src)
        assert m, pattern
        return int(m.group(1))

    assert const(r"constexpr uint32_t kK1Rows = (\d+);") == k1.K1_ROWS
    assert const(r"constexpr uint32_t kK1TailPitch = (\d+);") == k1.K1_TAIL_PITCH
    assert const(r"constexpr uint32_t kK1TailImgFloats = (\d+);") == k1.K1_TAIL_IMG_FLOATS
    assert const(r"#define SDB_K1_STREAM_MAX_NQ (\d+)") == k1.K1_STREAM_MAX_NQ
    assert const(r"uint32_t span = (\d+);") == k1.K1_STREAM_SPAN
    assert const(r"#define SDB_K1_WAVES (\d+)") == k1.K1_PK_WAVES
    assert const(r"#define SDB_K1_QPP (\d+)") == 1  # k1_route counts one query per pass of the packed kernel
    assert "(160 * 1024 - 16) / row_bytes" in src and "if (lds > 160 * 1024) return 0;" in src
    assert "if (tile_rows < 8) return 0;" in src and "if (nblk > 32) return 0;" in src
    # the launch bounds change between 12 and 13 blocks, in both matrix-core families
    assert "__launch_bounds__(256, (NBLK <= 12 && !TAIL) ? 2 : 1)" in src
    assert "__launch_bounds__(256, NBLK <= 12 ? 2 : 1)" in src


def test_route_examples():
    """the dispatch at the points the source's comments and the existing tests name"""
    r = k1.k1_route
    assert r("cosine", 384, 64, 4096).family == k1.STREAM and r("cosine", 384, 64, 4096).blocks == 8
    assert r("cosine", 384, 256, 513)[:2] == (k1.STREAM, 12) and r("cosine", 384, 257, 513)[:2] == (k1.TILE, 12)
    assert r("dot", 416, 300, 1030)[:3] == (k1.TILE, 13, 0)          # thirteen whole blocks: no tail
    assert r("dot", 416, 130, 1100)[:3] == (k1.STREAM, 13, 0)
    assert r("dot", 420, 130, 1100)[:3] == (k1.TILE_TAIL, 13, 4)     # a tail takes the tile kernel at any query count
    assert r("dot", 384, 4, 6).family == k1.STREAM and r("dot", 384, 1, 6).family == k1.FIRST
    assert r("cosine", 33, 5, 77).family == k1.FIRST and r("cosine", 31, 5, 77).family == k1.FIRST
    assert r("cosine", 1056, 5, 77).family == k1.FIRST and r("cosine", 4096, 2, 20).family == k1.FIRST
    assert r("euclidean", 4096, 2, 20).family == k1.PK and r("euclidean", 4096, 2, 20).tile_rows == 9
    assert r("cosine", 100, 35, 83, q_off=4).family == k1.FIRST and r("dot", 96, 18, 83, c_off=4).family == k1.FIRST
    assert r("dot", 96, 258, 84).vec_store == 1 and r("dot", 96, 258, 83).vec_store == 0
    assert [r("dot", 96, 258, 84, out_off=o).vec_store for o in (4, 8, 12)] == [0, 0, 0]
    assert r("cosine", 32, 65535, 3)[:4] == (k1.TILE, 1, 0, 4096) and r("euclidean", 32, 65535, 3).family == k1.PK
    # the largest image: <32, true> needs 146 432 bytes of LDS, under the 160 KB every instantiation is allowed
    assert k1.tile_lds_bytes(32, 28) == 146432 <= k1.K1_LDS_MAX
    # rows per tile of the packed kernel drop below 64 at d = 636
    assert [r("euclidean", d, 2, 9).tile_rows for d in (608, 632, 636, 640, 768, 1024)] == [64, 64, 63, 63, 53, 39]
    assert {d: r("euclidean", d, 2, 9).tile_rows for d in k1.PK_TILE_ROWS} == k1.PK_TILE_ROWS


def test_every_sweep_row_reaches_the_kernel_it_is_there_for():
    for nblk, rows in k1.SWEEP.items():
        got = [(c.d, r.family, r.nblk, r.tail) for r, c, _ in k1.routes(rows)]
        d, t = 32 * nblk, k1.sweep_tail(nblk)
        assert got == [(d, k1.STREAM, nblk, 0)] * 2 + [(d, k1.TILE, nblk, 0)] * 2 + [(d + t, k1.TILE_TAIL, nblk, t)] * 2 + \
            [(d, k1.PK, nblk, 0), (d + t, k1.PK, nblk, t)], nblk


def test_the_sweep_reaches_all_96_instantiations():
    """delete a row of k1_cases._sweep_rows (or a block count of SWEEP) and this fails"""
    every = set(range(1, 33))
    assert sorted(k1.SWEEP) == sorted(every)
    for family in (k1.STREAM, k1.TILE, k1.TILE_TAIL):
        assert _reached(SWEEP_ROUTES, family) == every, family
    # the packed kernel is one instantiation; the sweep gives it every block count with and without a tail
    assert {(r.nblk, r.tail != 0) for r, _, _ in SWEEP_ROUTES if r.family == k1.PK} == {(n, t) for n in every for t in (False, True)}
    # both matrix metrics reach each of them
    for family in (k1.STREAM, k1.TILE, k1.TILE_TAIL):
        for metric in k1.MATRIX:
            assert {r.nblk for r, _, m in SWEEP_ROUTES if r.family == family and m == metric} == every


def test_every_tail_length_on_four_block_counts():
    for tail in range(4, 32, 4):
        nblks = {r.nblk for r, _, _ in SWEEP_ROUTES if r.family == k1.TILE_TAIL and r.tail == tail}
        assert len(nblks) >= 4, (tail, sorted(nblks))


def test_the_tail_kernel_wraps_its_double_buffer():
    """at least 17 query groups (the two-slot query image used nine times and more) at 1, 13 and 32 blocks"""
    many = k1.routes(k1.MANY_GROUPS)
    for nblk in (1, 13, 32):
        groups = [r.groups for r, _, _ in many if r.family == k1.TILE_TAIL and r.nblk == nblk]
        assert groups and max(groups) >= 17 and len(groups) >= 4, (nblk, groups)  # two shapes, two metrics
    assert all(r.family == k1.TILE_TAIL and r.groups >= 17 for r, _, _ in many)
    assert {c.d for c in k1.MANY_GROUPS} >= {36, 412, 1052}


def test_the_packed_kernel_s_tiles():
    """64, 63, 40 and 9 rows per tile, with and without a tail -- except 40 without one: only d = 996 .. 1 016 give 40
    rows, and no multiple of 32 lies there (992 gives 41, 1 024 gives 39); the test states that instead"""
    pk = [(r, c) for r, c, _ in ALL_ROUTES if r.family == k1.PK]
    seen = {(r.tile_rows, r.tail != 0) for r, _ in pk}
    for rows in (64, 63, 40, 9):
        assert (rows, True) in seen, rows
    for rows in (64, 63, 9):
        assert (rows, False) in seen, rows
    assert [d for d in range(32, 4097, 4) if k1.k1_route("euclidean", d, 2, 9).tile_rows == 40 and d % 32 == 0] == []
    assert min(k1.k1_route("euclidean", d, 2, 9).tile_rows for d in range(32, 4097, 4)) == 9  # never under 8: always tiled
    # a tail together with a short tile, a tile larger than the whole block, more queries than the 16 waves take at once
    assert any(r.tail and r.tile_rows < 64 and c.nc % r.tile_rows for r, c in pk)
    assert any(c.nc < r.tile_rows for r, c in pk)
    assert any(r.groups > 2 * k1.K1_PK_WAVES and r.tail and r.tile_rows < 64 for r, c in pk)
    for d, rows in k1.PK_TILE_ROWS.items():
        ncs = {c.nc for c in k1.PK_TILES if c.d == d}
        assert ncs == set(k1.pk_ncs(rows)), d


def test_ragged_cases_meet_both_matrix_kernels():
    fam = {(c.d, c.nq): r.family for r, c, m in k1.routes(k1.RAGGED) if m == "cosine"}
    assert fam[(384, 255)] == fam[(384, 256)] == k1.STREAM and fam[(384, 257)] == k1.TILE
    assert fam[(32, 256)] == k1.STREAM and fam[(32, 257)] == k1.TILE
    assert fam[(100, 2)] == fam[(100, 257)] == fam[(1052, 2)] == fam[(1052, 257)] == k1.TILE_TAIL
    assert len(k1.RAGGED) == len(k1.RAGGED_DIMS) * len(k1.RAGGED_NQ) * len(k1.RAGGED_NC)
    spans = [r.blocks for r, c, m in k1.routes(k1.SPAN) if m == "dot"]
    assert spans == [1, 1, 2, 3]


def test_special_surround_and_limit_cases_reach_their_kernels():
    def fam(case, metric, **kw):
        r = k1.k1_route(metric, case.d, case.nq, case.nc, **kw)
        return (r.family, r.nblk, r.tail)

    sp = {(c.d, c.nq): c for c in k1.SPECIAL}
    assert fam(sp[(384, 258)], "dot") == (k1.TILE, 12, 0)
    assert fam(sp[(396, 35)], "dot") == fam(sp[(396, 258)], "cosine") == (k1.TILE_TAIL, 12, 12)
    assert fam(sp[(1052, 35)], "cosine") == (k1.TILE_TAIL, 32, 28)
    assert fam(sp[(384, 64)], "cosine") == (k1.STREAM, 12, 0)
    r = k1.k1_route("euclidean", 1000, 35, k1.SPECIAL_NC)
    assert (r.family, r.tile_rows, r.tail) == (k1.PK, 40, 8)
    assert [k1.k1_route(c.metrics[0], c.d, c.nq, c.nc).family for c in k1.SURROUND] == \
        [k1.STREAM, k1.TILE, k1.TILE_TAIL, k1.PK, k1.FIRST, k1.FIRST]
    pk = k1.SURROUND[3]
    r = k1.k1_route("euclidean", pk.d, pk.nq, pk.nc)
    assert r.tail == 8 and r.tile_rows == 40 and pk.nc % 40 == 3
    for c in k1.UNALIGNED_IN:  # tiled when aligned, the first kernel when either input is 4 bytes off
        assert fam(c, c.metrics[0])[0] != k1.FIRST
        assert fam(c, c.metrics[0], q_off=4)[0] == fam(c, c.metrics[0], c_off=4)[0] == k1.FIRST
    assert {fam(c, c.metrics[0])[0] for c in k1.UNALIGNED_IN} == {k1.TILE_TAIL, k1.STREAM, k1.PK}
    for c in k1.UNALIGNED_OUT:
        assert c.nc % 4 == 0 and k1.k1_route(c.metrics[0], c.d, c.nq, c.nc).vec_store == 1
        for off in (4, 8, 12):
            r = k1.k1_route(c.metrics[0], c.d, c.nq, c.nc, out_off=off)
            assert r.family in (k1.TILE, k1.TILE_TAIL) and r.vec_store == 0


@pytest.mark.parametrize("case", k1.SPECIAL, ids=lambda c: "d%d-nq%d" % (c.d, c.nq))
def test_special_inputs_make_the_oracle_produce_every_class(oracle, case):
    """per metric: a NaN, an Inf, an exact zero and a denormal among the oracle's own outputs, and at most a quarter of
    them NaN -- a comparison that excuses positions where both sides are NaN must not excuse most of the block.
    Cosine is 1 - dot: next to 1 the float32 grid is 6e-8 wide, so no cosine distance is denormal; there the dot
    product it is computed from (the dot metric's output on the same rows) has to hold the denormals."""
    q, c = k1.special_inputs(case.d, case.nq, case.nc)
    assert q.shape == (case.nq, case.d) and c.shape == (case.nc, case.d)
    for metric in case.metrics:
        want = oracle.distance_matrix(q, c, metric, oracle.IMPL_ASM)
        nan = np.isnan(want)
        assert nan.any() and np.isinf(want).any() and (want == 0).any(), metric
        assert nan.mean() <= 0.25, (metric, nan.mean())
        if metric != "cosine":
            assert k1.is_denormal(want).any(), metric
        # every class on both sides of zero where the metric has two sides
        if metric == "dot":
            assert (want == np.inf).any() and (want == -np.inf).any()
        # and most of the block is ordinary numbers
        assert np.isfinite(want).mean() >= 0.5
