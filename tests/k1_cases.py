"""The shapes tests/test_gpu_distance_sweep.py sends through sdb_distance_batch (K1), and which kernel each one reaches.

K1 has five kernels behind one entry point; three of them are compiled once per row length (NBLK = d / 32 = 1 .. 32),
96 instantiations in all.  A test cannot see which kernel ran, so the dispatch is restated here as a pure function,
k1_route, and the shape table below is built so that -- by that function -- every instantiation and every edge of the
dispatch is reached.  tests/test_k1_cases.py holds the table to that claim without a GPU; the GPU module runs it.

Line numbers cite semadb_amd/csrc/distance_tile.hip (launch_k1_tiles) unless they name another file.
"""
from collections import namedtuple

import numpy as np

METRICS = ("euclidean", "cosine", "dot")
MATRIX = ("cosine", "dot")

# ---- the dispatch, restated ------------------------------------------------------------------------------------------
K1_ROWS = 64                  # kK1Rows, :32
K1_TAIL_PITCH = 36            # kK1TailPitch, :33
K1_TAIL_IMG_FLOATS = 768      # kK1TailImgFloats, :34
K1_LDS_MAX = 160 * 1024       # the dynamic LDS every K1 kernel is allowed, :410, :445, :493
K1_STREAM_MAX_NQ = 256        # SDB_K1_STREAM_MAX_NQ, :460
K1_STREAM_SPAN = 512          # :463
K1_PK_WAVES = 16              # SDB_K1_WAVES, :305

FIRST, STREAM, TILE, TILE_TAIL, PK = "first", "stream", "tile", "tile_tail", "pk"

# family:    FIRST k_distance_batch | STREAM k_k1_stream_mfma<nblk> | TILE k_k1_tile_mfma<nblk, false> |
#            TILE_TAIL k_k1_tile_mfma<nblk, true> | PK k_k1_tile_pk<true>
# groups:    what the kernel's outer loop counts -- query groups of 16 (TILE, TILE_TAIL), queries handed out from the LDS
#            counter (PK), candidate groups of 16 in the longest span (STREAM); 0 for FIRST
# blocks:    workgroups launched (x * y)
# tile_rows: candidate rows per workgroup of the packed kernel; 0 elsewhere
# vec_store: TILE / TILE_TAIL only: 16-byte stores (1) or the scalar store path (0)
Route = namedtuple("Route", "family nblk tail groups blocks tile_rows vec_store")


def k1_route(metric, d, nq, nc, q_off=0, c_off=0, out_off=0):
    """launch_k1_tiles's decisions for one call.  q_off / c_off / out_off: the byte offset of each block's first element
    from a 16-byte boundary (the staging path and a fresh allocation give 0)."""
    assert metric in METRICS and 1 <= d <= 4096 and nq >= 1 and nc >= 1  # distance.hip:140-144
    nblk, tail = d // 32, d % 32                                          # :438
    first = Route(FIRST, nblk, tail, 0, -(-nc // K1_ROWS) * nq, 0, 0)     # distance.hip:179
    if nq < 2 or nblk < 1 or (d & 3):                                     # :439
        return first
    if (q_off | c_off) & 15:                                              # :440
        return first
    if metric == "euclidean":                                             # :442
        row_bytes = (d + 4) * 4                                           # :444
        tile_rows = min(K1_ROWS, (K1_LDS_MAX - 16) // row_bytes)          # :445
        if tile_rows < 8:                                                 # :446
            return first
        return Route(PK, nblk, tail, nq, -(-nc // tile_rows), tile_rows, 0)  # :453, groups :336 (one query per pass)
    if nblk > 32:                                                         # :458
        return first
    if tail == 0 and nq <= K1_STREAM_MAX_NQ:                              # :462
        span = K1_STREAM_SPAN                                             # :463
        while -(-nc // span) > 65535:                                     # :464
            span *= 2
        blocks = -(-nq // 64) * -(-nc // span)                            # :465
        return Route(STREAM, nblk, 0, -(-min(span, nc) // 16), blocks, 0, 0)  # groups :212
    ngroups = -(-nq // 16)                                                # :490
    grp_floats = nblk * 512 + (K1_TAIL_IMG_FLOATS if tail else 0)         # :491
    lds = 2 * grp_floats * 4 + (K1_ROWS * K1_TAIL_PITCH * 4 if tail else 0)  # :492
    if lds > K1_LDS_MAX:                                                  # :493
        return first
    if ngroups * grp_floats > 0xFFFFFFFF:                                 # :494-495
        return first
    vec_store = 1 if (nc & 3) == 0 and (out_off & 15) == 0 else 0         # :502
    return Route(TILE_TAIL if tail else TILE, nblk, tail, ngroups, -(-nc // K1_ROWS), 0, vec_store)  # :441, :503


def tile_lds_bytes(nblk, tail):
    """the dynamic LDS of k_k1_tile_mfma<nblk, tail != 0> (:491-492)"""
    grp_floats = nblk * 512 + (K1_TAIL_IMG_FLOATS if tail else 0)
    return 2 * grp_floats * 4 + (K1_ROWS * K1_TAIL_PITCH * 4 if tail else 0)


# ---- the shape table ---------------------------------------------------------------------------------------------
# One row = one call per metric: (d, metrics, nq, nc).
Case = namedtuple("Case", "d metrics nq nc")


def sweep_tail(nblk):
    """the tail length the sweep gives block count nblk: 4, 8, .., 28 in turn, each on four or five block counts"""
    return 4 * (1 + (nblk - 1) % 7)


def _sweep_rows(nblk):
    d, dt = 32 * nblk, 32 * nblk + sweep_tail(nblk)
    return [
        # stream<nblk>: one query block whose second wave holds 2 real queries and whose third and fourth hold none;
        # six candidate groups, the last with 3 rows
        Case(d, MATRIX, 18, 83),
        # tile<nblk, false>: 17 query groups, the last with 2 queries; two workgroups, the second with 19 rows (one full
        # wave, one with 3 rows, two idle)
        Case(d, MATRIX, 258, 83),
        # tile<nblk, true>: three query groups, the last with 3 queries
        Case(dt, MATRIX, 35, 83),
        # the packed kernel without and with a tail: more queries than waves, a ragged last tile
        Case(d, ("euclidean",), 18, 83),
        Case(dt, ("euclidean",), 18, 83),
    ]


# SWEEP[nblk]: the instantiation sweep's rows for one block count
SWEEP = {nblk: _sweep_rows(nblk) for nblk in range(1, 33)}

# many query groups through the tail kernel's double buffer (the tail rows sit behind it): 17 and 19 groups.  d = 36,
# 412 and 1 052 are 1, 12 and 32 blocks; 420 is 13 blocks and a tail of 4, the first block count past the change of
# __launch_bounds__ in the kernels without a tail
MANY_GROUPS_DIMS = (36, 412, 420, 1052)
MANY_GROUPS = [Case(d, MATRIX, nq, nc) for d in MANY_GROUPS_DIMS for nq, nc in ((258, 83), (300, 130))]

# ragged edges of each family: every pair of these counts, at each of these widths, all three metrics.  255 / 256 / 257
# queries are where the two matrix-core kernels meet
RAGGED_DIMS = (32, 100, 384, 1052)
RAGGED_NC = (1, 3, 15, 16, 17, 63, 64, 65)
RAGGED_NQ = (2, 15, 16, 17, 63, 64, 65, 255, 256, 257)
RAGGED = [Case(d, METRICS, nq, nc) for d in RAGGED_DIMS for nq in RAGGED_NQ for nc in RAGGED_NC]

# candidate counts around the streaming kernel's span of 512 (one span, a second of one row, a third of one row)
SPAN = [Case(32, METRICS, 64, nc) for nc in (511, 512, 513, 1025)]

# the packed kernel's tiles: 64, 63, 40, 9 and 9 rows, the first four with a tail; candidate counts one short of a tile,
# a tile, one more, two tiles and a row; 2, 17 and 33 queries for 16 waves
PK_TILE_ROWS = {632: 64, 636: 63, 1000: 40, 4092: 9, 4096: 9}
PK_NQ = (2, 17, 33)


def pk_ncs(tile_rows):
    return (tile_rows - 1, tile_rows, tile_rows + 1, 2 * tile_rows + 1)


PK_TILES = [Case(d, ("euclidean",), nq, nc) for d, tr in PK_TILE_ROWS.items() for nq in PK_NQ for nc in pk_ncs(tr)]

# special values in every family: (d, nq); nc = 83 everywhere, all three metrics
SPECIAL_NC = 83
SPECIAL = [Case(d, METRICS, nq, SPECIAL_NC) for d, nq in ((384, 258), (396, 35), (396, 258), (1052, 35), (1000, 35), (384, 64))]

# what surrounds the blocks: one ragged shape per family
SURROUND = [
    Case(96, ("cosine",), 18, 83),        # streaming
    Case(96, ("dot",), 258, 83),          # tile
    Case(100, ("cosine",), 35, 83),       # tile with a tail
    Case(1000, ("euclidean",), 17, 83),   # packed, tail 8, 40 rows per tile, the third tile with 3 rows
    Case(33, ("euclidean",), 5, 83),      # the first kernel (rows are not whole float4s)
    Case(40, ("dot",), 1, 83),            # the first kernel (one query)
]
# unaligned callers: queries, then candidates, 4 bytes off a 16-byte boundary -> the first kernel
UNALIGNED_IN = [Case(100, ("cosine",), 35, 83), Case(96, ("dot",), 18, 83), Case(1000, ("euclidean",), 17, 83)]
# out 4, 8 and 12 bytes off with nc % 4 == 0 -> the tile kernels' scalar stores
UNALIGNED_OUT = [Case(96, ("dot",), 258, 84), Case(100, ("cosine",), 35, 84)]

# argument limits that are accepted
LIMITS = [Case(32, ("cosine", "euclidean"), 65535, 3), Case(4096, METRICS, 2, 20)]


def all_cases():
    rows = [c for nblk in SWEEP for c in SWEEP[nblk]]
    return rows + MANY_GROUPS + RAGGED + SPAN + PK_TILES + SPECIAL + SURROUND + UNALIGNED_OUT + LIMITS


def routes(cases):
    """[(route, case, metric)] for every call the cases make"""
    return [(k1_route(m, c.d, c.nq, c.nc), c, m) for c in cases for m in c.metrics]


# ---- inputs ------------------------------------------------------------------------------------------------------
def normal_rows(rng, n, d):
    return (rng.standard_normal((n, d)) * 2).astype(np.float32)


def special_inputs(d, nq, nc, seed=77):
    """tests/test_gpu_distance.py's recipe (denormal products, overflow at the 1e18 scale, c = q and c = -q, alternating
    zeros and negative zeros) plus all-zero rows, rows whose squared differences are denormal, a unit vector on both
    sides (cosine distance exactly 0), and NaN / +Inf / -Inf planted in single elements: in the first block, in a middle
    block, and in the last positions of the row (the tail chain where d % 32 != 0).  Two NaN rows and two Inf rows on
    each side: at 35 x 83 about a tenth of the outputs are NaN."""
    assert nq >= 11 and nc >= 12 and d >= 64
    rng = np.random.default_rng(seed + d)
    q = rng.standard_normal((nq, d)).astype(np.float32)
    c = rng.standard_normal((nc, d)).astype(np.float32)
    q[0] *= np.float32(1e-38)
    c[0] *= np.float32(1e-3)       # denormal products
    q[1] *= np.float32(1e18)
    c[1] *= np.float32(1e18)       # overflow
    c[2] = q[2]
    c[3] = -q[2]                   # cancellation
    q[3, ::2] = 0.0
    c[4, 1::2] = -0.0              # signed zeros
    q[4] = 0.0
    c[5] = 0.0                     # all-zero rows
    q[5] *= np.float32(1e-21)
    c[6] *= np.float32(1e-21)      # denormal squares and sums of them
    q[6] = 0.0
    q[6, 0] = 1.0
    c[7] = 0.0
    c[7, 0] = 1.0                  # dot exactly 1
    mid = 32 * (d // 64) + 9       # an element of a middle block
    q[7, 5] = np.nan
    q[8, d - 1] = np.nan
    q[9, mid] = np.inf
    q[10, d - 2] = -np.inf
    c[8, 7] = np.nan
    c[9, d - 3] = np.nan
    c[10, mid + 1] = -np.inf
    c[11, d - 1] = np.inf
    return q, c


def is_denormal(a):
    a = np.abs(np.asarray(a, dtype=np.float32))
    return (a > 0) & (a < np.finfo(np.float32).tiny)
