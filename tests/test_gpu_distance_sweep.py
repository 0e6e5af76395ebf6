"""K1 parity (GPU), every instantiation and every edge of the dispatch: sdb_distance_batch against the oracle's
AVX2-order arithmetic, bit for bit, over the shape table of tests/k1_cases.py.

Behind the entry point sit the first kernel (k_distance_batch), k_k1_stream_mfma<NBLK>, k_k1_tile_mfma<NBLK, false>,
k_k1_tile_mfma<NBLK, true> and the packed euclidean kernel k_k1_tile_pk; the three matrix-core families are compiled
once per row length, NBLK = 1 .. 32.  Which of them a shape reaches is taken from k1_cases.k1_route, the dispatch
restated (tests/test_k1_cases.py holds the table to it on the CPU); nothing here observes it on the device."""
import ctypes as C

import numpy as np
import pytest

from tests import k1_cases as k1
from tests.helpers import bits

pytestmark = pytest.mark.gpu

GUARD = 1024           # floats before and after every guarded block: a multiple of 64, so blocks start 256-byte aligned
WORD = 0x5EDBC0DE      # what fills `out` and its surroundings before a call


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _run(metric, qd, cd):
    """device blocks in, the distance block back on the host (the copy waits for the kernels)"""
    from semadb_amd import distance
    return distance.distance_batch(metric, qd, cd).cpu().numpy()


def _assert_bits(got, want, what):
    assert got.shape == want.shape, what
    diff = bits(got) != bits(want)
    assert not diff.any(), (what, int(diff.sum()), np.argwhere(diff)[:4].tolist())


def _assert_bits_or_nan(got, want, what):
    """equal bits, or NaN on both sides (x86 and the device produce different default NaNs): so the NaN masks are
    identical.  How much of a block that may excuse is checked on the CPU (tests/test_k1_cases.py)."""
    assert got.shape == want.shape, what
    gn, wn = np.isnan(got), np.isnan(want)
    assert np.array_equal(gn, wn), (what, "NaN masks differ", np.argwhere(gn != wn)[:4].tolist())
    diff = (bits(got) != bits(want)) & ~wn
    assert not diff.any(), (what, int(diff.sum()), np.argwhere(diff)[:4].tolist())


class _Reference:
    """rows for one width, the largest counts any case of it needs, and the oracle's matrix per metric computed once:
    a pair's distance does not depend on the other rows, so every smaller case is a corner of it"""

    def __init__(self, oracle, d, nq, nc, seed):
        rng = np.random.default_rng(seed)
        self.oracle, self.q, self.c = oracle, k1.normal_rows(rng, nq, d), k1.normal_rows(rng, nc, d)
        self.qd, self.cd = _dev(self.q), _dev(self.c)
        self._want = {}

    def want(self, metric):
        if metric not in self._want:
            self._want[metric] = self.oracle.distance_matrix(self.q, self.c, metric, self.oracle.IMPL_ASM)
        return self._want[metric]

    def check(self, metric, nq, nc):
        got = _run(metric, self.qd[:nq], self.cd[:nc])
        _assert_bits(got, self.want(metric)[:nq, :nc], (metric, self.q.shape[1], nq, nc))


def _check_cases(oracle, cases, seed):
    refs = {}
    for d in sorted({c.d for c in cases}):
        mine = [c for c in cases if c.d == d]
        refs[d] = _Reference(oracle, d, max(c.nq for c in mine), max(c.nc for c in mine), seed + d)
    for c in cases:
        for metric in c.metrics:
            refs[c.d].check(metric, c.nq, c.nc)


# ---- 2. the instantiation sweep ----------------------------------------------------------------------------------
@pytest.mark.parametrize("nblk", range(1, 33))
def test_every_instantiation(oracle, nblk):
    """stream<nblk>, tile<nblk, false>, tile<nblk, true> (tail 4 .. 28 in turn) for cosine and dot, and the packed
    kernel at the same two row lengths: ragged query groups, ragged candidate groups, two workgroups"""
    _check_cases(oracle, k1.SWEEP[nblk], 1000 * nblk)


@pytest.mark.parametrize("d", k1.MANY_GROUPS_DIMS)
def test_tail_kernel_many_query_groups(oracle, d):
    """17 and 19 query groups through the tail kernel's double-buffered query image, the row tails behind it"""
    _check_cases(oracle, [c for c in k1.MANY_GROUPS if c.d == d], 31)


# ---- 3. ragged edges ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", k1.METRICS)
@pytest.mark.parametrize("d", k1.RAGGED_DIMS)
def test_ragged_counts(oracle, metric, d):
    """1 .. 65 candidates x 2 .. 257 queries: single rows, one short of / exactly / one past a wave's 16 and a
    workgroup's 64, and 255 / 256 / 257 queries where the streaming kernel hands over to the tile kernel"""
    _check_cases(oracle, [k1.Case(c.d, (metric,), c.nq, c.nc) for c in k1.RAGGED if c.d == d], 37)


@pytest.mark.parametrize("metric", k1.METRICS)
def test_candidates_around_the_stream_span(oracle, metric):
    _check_cases(oracle, [k1.Case(c.d, (metric,), c.nq, c.nc) for c in k1.SPAN], 41)


@pytest.mark.parametrize("d", sorted(k1.PK_TILE_ROWS))
def test_packed_kernel_tiles(oracle, d):
    """64, 63, 40, 9 and 9 rows per tile (the first four with a tail chain), candidate counts around one and two tiles,
    fewer and more queries than the workgroup has waves"""
    _check_cases(oracle, [c for c in k1.PK_TILES if c.d == d], 43)


# ---- 4. special values -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", k1.SPECIAL, ids=lambda c: "d%d-nq%d" % (c.d, c.nq))
def test_special_values_in_every_family(oracle, case):
    """denormals, overflow, cancellation, signed zeros, all-zero rows, planted NaN and +-Inf (first block, a middle
    block, the row's last positions = the tail chain) through the tile kernel with and without a tail, the packed
    kernel's short tile with a tail, and the streaming kernel"""
    q, c = k1.special_inputs(case.d, case.nq, case.nc)
    qd, cd = _dev(q), _dev(c)
    for metric in case.metrics:
        want = oracle.distance_matrix(q, c, metric, oracle.IMPL_ASM)
        _assert_bits_or_nan(_run(metric, qd, cd), want, (metric, case))


# ---- 5. what surrounds the blocks --------------------------------------------------------------------------------
def _guarded_input(block, off_floats, device):
    """the block inside a NaN-filled buffer, `off_floats` past a 256-byte boundary; returns (owner, address)"""
    n = block.size
    if device:
        import torch
        buf = torch.full((2 * GUARD + n + 64,), float("nan"), dtype=torch.float32, device="cuda")
        base = buf.data_ptr()
        buf[GUARD + off_floats:GUARD + off_floats + n] = torch.from_numpy(block.ravel()).cuda()
    else:
        buf = np.full(2 * GUARD + n + 64, np.nan, dtype=np.float32)
        base = buf.ctypes.data
        buf[GUARD + off_floats:GUARD + off_floats + n] = block.ravel()
    assert device is False or base % 256 == 0
    return buf, base + 4 * (GUARD + off_floats)


def _guarded_out(n, off_floats, device):
    if device:
        import torch
        buf = torch.full((2 * GUARD + n + 64,), WORD, dtype=torch.int32, device="cuda")
        base = buf.data_ptr()
        assert base % 256 == 0
    else:
        buf = np.full(2 * GUARD + n + 64, WORD, dtype=np.uint32)
        base = buf.ctypes.data
    return buf, base + 4 * (GUARD + off_floats)


def _raw_call(metric, d, qp, nq, cp, nc, op, device):
    from semadb_amd._lib import MEM_DEVICE, MEM_HOST, METRICS, lib
    stream = None
    if device:
        import torch
        stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    rc = lib().sdb_distance_batch(METRICS[metric], d, C.c_void_p(qp), nq, C.c_void_p(cp), nc, C.c_void_p(op),
                                  MEM_DEVICE if device else MEM_HOST, 0, stream)
    if device:
        import torch
        torch.cuda.synchronize()
    return rc


def _guarded_call(oracle, metric, d, nq, nc, q_off=0, c_off=0, out_off=0, device=True, seed=53):
    """one raw call on blocks with poisoned surroundings: the block is the oracle's, every guard word is untouched"""
    rng = np.random.default_rng(seed + d)
    q, c = k1.normal_rows(rng, nq, d), k1.normal_rows(rng, nc, d)
    qbuf, qp = _guarded_input(q, q_off, device)
    cbuf, cp = _guarded_input(c, c_off, device)
    obuf, op = _guarded_out(nq * nc, out_off, device)
    what = (metric, d, nq, nc, q_off, c_off, out_off, device)
    assert _raw_call(metric, d, qp, nq, cp, nc, op, device) == 0, what
    words = (obuf.cpu().numpy() if device else obuf).view(np.uint32)
    lo, hi = GUARD + out_off, GUARD + out_off + nq * nc
    touched = np.flatnonzero(np.concatenate([words[:lo], words[hi:]]) != WORD)
    assert touched.size == 0, (what, "stores outside out[nq][nc]", touched[:8].tolist())
    got = words[lo:hi].view(np.float32).reshape(nq, nc)
    _assert_bits(got, oracle.distance_matrix(q, c, metric, oracle.IMPL_ASM), what)
    del qbuf, cbuf


@pytest.mark.parametrize("case", k1.SURROUND, ids=lambda c: "%s-d%d-nq%d" % (c.metrics[0], c.d, c.nq))
def test_poisoned_surroundings(oracle, case):
    """NaN before and behind `queries` and `candidates`, a fixed word around `out`: a kernel that reads past a block's
    end or uses a clamped row's result turns outputs into NaN, one that stores past out[nq][nc] changes a guard word"""
    _guarded_call(oracle, case.metrics[0], case.d, case.nq, case.nc)


@pytest.mark.parametrize("case", k1.UNALIGNED_IN, ids=lambda c: "%s-d%d" % (c.metrics[0], c.d))
@pytest.mark.parametrize("which", ["queries", "candidates"])
def test_unaligned_inputs_take_the_first_kernel(oracle, case, which):
    """either input 4 bytes off a 16-byte boundary: the tile kernels' 16-byte loads would fault or read the wrong
    elements, so the launcher falls back; the bits are the oracle's either way"""
    off = {"queries": dict(q_off=1), "candidates": dict(c_off=1)}[which]
    _guarded_call(oracle, case.metrics[0], case.d, case.nq, case.nc, **off)


@pytest.mark.parametrize("case", k1.UNALIGNED_OUT, ids=lambda c: "%s-d%d" % (c.metrics[0], c.d))
@pytest.mark.parametrize("off", [1, 2, 3])
def test_unaligned_out_takes_scalar_stores(oracle, case, off):
    """nc % 4 == 0 but `out` 4, 8, 12 bytes off: the tile kernels must not use their 16-byte stores"""
    _guarded_call(oracle, case.metrics[0], case.d, case.nq, case.nc, out_off=off)


def test_host_memory_blocks(oracle):
    """the staging path lays the three blocks out itself (256-byte aligned parts of one allocation): host blocks at
    any address, NaN around the inputs, a guarded `out`; then the same through distance.distance_batch"""
    from semadb_amd import distance
    _guarded_call(oracle, "cosine", 100, 35, 83, q_off=1, c_off=3, out_off=1, device=False)
    _guarded_call(oracle, "euclidean", 1000, 17, 83, q_off=2, c_off=1, out_off=3, device=False)
    rng = np.random.default_rng(59)
    qbuf, cbuf = np.full((35 + 2, 100), np.nan, dtype=np.float32), np.full((83 + 2, 100), np.nan, dtype=np.float32)
    qbuf[1:36], cbuf[1:84] = k1.normal_rows(rng, 35, 100), k1.normal_rows(rng, 83, 100)
    for metric in k1.METRICS:
        got = distance.distance_batch(metric, qbuf[1:36], cbuf[1:84])
        _assert_bits(got, oracle.distance_matrix(qbuf[1:36], cbuf[1:84], metric, oracle.IMPL_ASM), metric)


# ---- 6. argument limits ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", k1.LIMITS, ids=lambda c: "d%d-nq%d" % (c.d, c.nq))
def test_largest_accepted_sizes(oracle, case):
    """65 535 queries (4 096 query groups through tile<1, false>; the packed kernel's counter up to 65 535) and the
    longest row, 4 096 floats (the first kernel for cosine / dot, 9 rows per tile for euclidean)"""
    _check_cases(oracle, [case], 61)


def test_refused_sizes_and_empty_calls():
    from semadb_amd import SemaDBError, distance
    with pytest.raises(SemaDBError) as e:
        distance.distance_batch("cosine", np.zeros((65536, 32), np.float32), np.zeros((3, 32), np.float32))
    assert e.value.code == 1
    for d in (0, 4097):
        with pytest.raises(SemaDBError) as e:
            distance.distance_batch("dot", np.zeros((2, d), np.float32), np.zeros((3, d), np.float32))
        assert e.value.code == 1
    assert distance.distance_batch("dot", np.zeros((0, 32), np.float32), np.zeros((3, 32), np.float32)).shape == (0, 3)
    assert distance.distance_batch("dot", np.zeros((2, 32), np.float32), np.zeros((0, 32), np.float32)).shape == (2, 0)
    # the raw call: invalid status for the refused sizes, OK for the empty ones, and `out` left alone by all of them
    for device in (True, False):
        qbuf, qp = _guarded_input(np.zeros((4, 4097), np.float32), 0, device)
        cbuf, cp = _guarded_input(np.zeros((4, 4097), np.float32), 0, device)
        obuf, op = _guarded_out(64, 0, device)
        for metric in k1.METRICS:
            assert _raw_call(metric, 32, qp, 65536, cp, 3, op, device) == 1
            assert _raw_call(metric, 0, qp, 2, cp, 3, op, device) == 1
            assert _raw_call(metric, 4097, qp, 2, cp, 3, op, device) == 1
            assert _raw_call(metric, 32, qp, 0, cp, 3, op, device) == 0
            assert _raw_call(metric, 32, qp, 2, cp, 0, op, device) == 0
            assert _raw_call(metric, 32, qp, 0, cp, 0, op, device) == 0
        words = (obuf.cpu().numpy() if device else obuf).view(np.uint32)
        assert (words == WORD).all(), device
        del qbuf, cbuf
