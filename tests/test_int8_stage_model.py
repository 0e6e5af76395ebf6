"""The float64 model of the int8 first stage (tests/int8_stage_model.py), pinned without a GPU: the copy's rules, the
two-term query, the exact integer sum, and -- on every input tests/test_gpu_int8_stage.py sends to the device -- a
replay that equals the oracle's walk and a sandwich that can see a half-broken stage: lower > 0 and lower >= 0.98 upper
(measured here: 0.99977 .. 0.99995, see test_width_inputs).  The last test replays the benchmark's own rows (100 000 of
them) and prints the shares that the choice of one scale per table and the refusal threshold rest on."""
import numpy as np
import pytest

import bench
from tests import int8_stage_model as M8
from tests import two_precision_model as M
from tests.helpers import bits, start_vector, unit_rows

METRICS8 = ("cosine", "dot")
WIDTHS8 = (32, 96, 128, 256, 352, 384)  # NG 1, 1, 1, 2, 3, 3: whole and partial last groups


def _same_walk(o, rep, q, limit, L):
    o_ids, o_d, o_vis, o_tr = o.search(q, limit, L)
    assert np.array_equal(rep.ids, o_ids) and np.array_equal(bits(rep.dists), bits(o_d))
    assert np.array_equal(rep.visit, o_vis), "visit order"
    assert (rep.n_hop, rep.n_dist, rep.n_edges) == (o_tr.n_hop, o_tr.n_dist, o_tr.n_edges)


def test_the_copy():
    f32 = np.float32
    rows = np.array([[1.0, -0.5, 0.25, 0.0], [0.003, 0.0041, -1.0, 0.5]], dtype=f32)
    c = M8.Copy8(rows)
    s = c.scale
    assert s > f32(1.0) / f32(127.0) and s == np.nextafter(f32(1.0) / f32(127.0), f32(1), dtype=f32)  # rounded up
    assert np.array_equal(c.y8, np.rint(rows / s).astype(np.int64)) and np.abs(c.y8).max() == 127
    # round to nearest EVEN, in float32: 2.5 -> 2, 3.5 -> 4; the clamp
    c2 = M8.Copy8(np.array([[2.5, 3.5, -2.5, 400.0, -400.0, 127.0]], dtype=f32), scale=1.0)
    assert c2.y8.tolist() == [[2, 4, -2, 127, -127, 127]]
    e = np.sqrt(0.5 ** 2 * 3 + 273.0 ** 2 * 2)
    assert abs(c2.emax - e) < 1e-12 and abs(c2.ymax - np.sqrt(4 + 16 + 4 + 3 * 127.0 ** 2)) < 1e-12
    # the maxima are maxima over rows; an all-zero row has no relative error
    c3 = M8.Copy8(np.vstack([rows, np.zeros((1, 4), dtype=f32)]))
    assert (c3.emax, c3.ymax, c3.rel) == (c.emax, c.ymax, c.rel) and not c3.refused()
    # a table of zeros: scale 0, nothing divided, nothing refused, bound 0
    z = M8.Copy8(np.zeros((3, 8), dtype=f32))
    assert z.scale == 0 and not z.y8.any() and (z.emax, z.ymax, z.rel) == (0.0, 0.0, 0.0) and not z.refused()
    # NaN, Inf: the maxima say so and the table is refused the copy; 1e30: finite, every other row becomes 0
    for bad in (np.nan, np.inf):
        r = rows.copy()
        r[1, 2] = bad
        cb = M8.Copy8(r)
        assert not np.isfinite(cb.emax) and cb.refused()
    r = rows.copy()
    r[1, 2] = 1e30
    cb = M8.Copy8(r)
    assert np.isfinite(cb.emax) and not cb.y8[0].any() and cb.refused()  # (row 0 is all error: rel = 1)
    # an appended row inside the range keeps the scale; its own maxima only ever raise the table's
    small = M8.Copy8(rows[:1] * f32(1e-3), scale=s)
    assert small.emax < c.emax and small.ymax < c.ymax


def test_the_refusal_rule():
    """unit rows are far inside; dot rows whose norms span 1e-3 .. 1e3 are refused through their small rows although the
    ratio of the two maxima -- both set by the largest rows -- stays small"""
    rng = np.random.default_rng(5)
    for d in WIDTHS8:
        c = M8.Copy8(unit_rows(rng, 500, d))
        assert not c.refused() and c.emax / c.ymax < 0.05 and c.rel < 0.05, (d, c.emax, c.ymax, c.rel)
    rows = unit_rows(rng, 600, 128) * (10.0 ** rng.uniform(-3, 3, (600, 1))).astype(np.float32)
    c = M8.Copy8(rows)
    assert c.emax / c.ymax < M8.MAX_RATIO and c.rel > 0.9 and c.refused(), (c.emax, c.ymax, c.rel)


def test_the_two_term_query():
    rng = np.random.default_rng(6)
    for d in WIDTHS8:
        for q in (unit_rows(rng, 4, d), unit_rows(rng, 4, d) * np.float32(1e4), unit_rows(rng, 4, d) * np.float32(1e-4)):
            for v in q:
                a, b, sq128 = M8.query8(v)
                assert np.abs(a).max() == 127 and np.abs(b).max() <= 65
                qhat = np.float64(sq128) * (128 * a + b)
                # the residual of b is at most half a step of s_q / 128 per element
                assert np.abs(v.astype(np.float64) - qhat).max() <= 0.51 * float(sq128)
    a, b, sq128 = M8.query8(np.zeros(32, dtype=np.float32))
    assert not a.any() and not b.any() and sq128 == 0
    # the integer sum stays below 2^31 for rows of up to 384 floats
    assert (128 * 127 + 64) * 127 * 384 < 2 ** 31


# lower / upper measured by this test (32 queries, L = 40): the sandwich is this tight on every input
MEASURED = {("cosine", 32): 0.99992, ("cosine", 96): 0.99995, ("cosine", 128): 0.99990, ("cosine", 256): 0.99993,
            ("cosine", 352): 0.99988, ("cosine", 384): 0.99986, ("dot", 32): 0.99990, ("dot", 96): 0.99993,
            ("dot", 128): 0.99988, ("dot", 256): 0.99989, ("dot", 352): 0.99986, ("dot", 384): 0.99977}


@pytest.mark.parametrize("metric", METRICS8)
@pytest.mark.parametrize("d", WIDTHS8)
def test_width_inputs(oracle, metric, d):
    ex, queries, limit, L = M.width_case(oracle, metric, d)
    g = M8.Graph(*ex)
    o = M.load_oracle(oracle, metric, d, ex)
    reps, t, _, copy = M8.run_model8(oracle, g, metric, queries, limit, L)
    for i, rep in enumerate(reps):
        _same_walk(o, rep, queries[i], limit, L)
    what = "%s d=%d" % (metric, d)
    M8.check_tally8(t, what)
    print("%s: %r lower / upper %.5f E8max %.5f Y8max %.5f" % (what, t, t.lower / t.upper, copy.emax, copy.ymax))
    assert not copy.refused()
    assert t.expanded_full_rows >= 0.9 * t.expanded
    assert t.lower > 10000 and t.discardable >= 0.7 * t.full, t
    assert t.lower / t.upper >= MEASURED[(metric, d)] - 0.0005, (what, t)


@pytest.mark.parametrize("metric", METRICS8)
def test_l_hostile_and_overflow_inputs(oracle, metric):
    d = 384
    ex, queries = M.l_case(oracle, metric, d)
    g = M8.Graph(*ex)
    o = M.load_oracle(oracle, metric, d, ex)
    copy = M8.Copy8(g.vecs)
    for L, limit in ((1, 1), (2, 1), (10, 10), (75, 10), (96, 10)):
        reps, t, _, _ = M8.run_model8(oracle, g, metric, queries, limit, L, copy)
        for i, rep in enumerate(reps):
            _same_walk(o, rep, queries[i], limit, L)
        M8.check_tally8(t, "%s L=%d" % (metric, L))
    for kind in M.HOSTILE_NO_DISCARD:
        if kind == "overflow":
            continue  # (1e6 overflows a float16, not an int8 query: the sandwich holds, below)
        _, t, _, _ = M8.run_model8(oracle, g, metric, M.hostile_queries(d, kind), 10, 40, copy)
        assert t.upper == 0 and t.lower == 0, (kind, t)
    for kind in M.HOSTILE_SANDWICH + ("overflow",):
        _, t, _, _ = M8.run_model8(oracle, g, metric, M.hostile_queries(d, kind), 10, 40, copy)
        assert t.lower <= t.upper <= t.discardable, (kind, t)
    ex, queries = M.overflow_case(oracle, metric)
    g = M8.Graph(*ex)
    for L in (1, 2):
        _, t, _, _ = M8.run_model8(oracle, g, metric, queries, 1, L)
        M8.check_tally8(t, "%s overflow list L=%d" % (metric, L))


def test_pricing_on_the_benchmark_rows(oracle):
    """bench.py's rows (latent:24, d = 384, cosine, R = 64, L = 75) at 100 000: shares of the neighbours met with the array
    full that are kept, decided by the int8 margin, and within it -- for one scale per table and for one per row.  The
    per-row scale does not pay for its 4-byte gather per edge: the bound is table-wide either way (E8max), so it
    moves the within-margin share by a fraction of a per cent.  The stage breaks even against the float16 stage while
    kept + within-margin < 0.41 (index.h kSketch8MaxRatio); the shares at inflated bounds give the ratio at which that is
    reached."""
    n, d, L, nq = 100000, 384, 75, 32
    base = bench.gen_rows(n, d, 20250620, "latent:24", "cpu").numpy()
    q = bench.gen_rows(nq, d, 20250621, "latent:24", "cpu").numpy()
    o = oracle.Index(d, "cosine", 64, L, 1.2, impl=M.impl_of(oracle))
    o.set_start(np.asarray(bench.start_vector(d), dtype=np.float32))
    assert o.insert_rounds(np.arange(2, n + 2, dtype=np.uint64), base) == 0
    g = M8.Graph(*o.export())
    reps, t, D, copy = M8.run_model8(oracle, g, "cosine", q, 10, L)
    M8.check_tally8(t, "bench rows")
    table = M8.price("cosine", copy, g.vecs, q, D, reps)
    per_row = M8.price("cosine", copy, g.vecs, q, D, reps, per_row=True)
    print("bench rows, one scale per table: %r" % (table,))
    print("bench rows, one scale per row:   %r" % (per_row,))
    assert not copy.refused() and copy.emax / copy.ymax < 0.03
    assert table["kept"] + table["within_margin"] < 0.2  # far below the 0.41 at which the stage stops paying
    assert abs(per_row["within_margin"] - table["within_margin"]) < 0.01
    # the same walk with the table's error inflated: where kept + within-margin crosses 0.41
    shares = {}
    for r in (0.05, 0.1, 0.16, 0.2, 0.3):
        c = M8.Copy8(g.vecs)
        c.emax = r * c.ymax
        p = M8.price("cosine", c, g.vecs, q, D, reps)
        shares[r] = round(p["kept"] + p["within_margin"], 4)
    print("kept + within-margin at E8max / Y8max = r: %r" % (shares,))
    assert shares[M8.MAX_RATIO] < 0.41 < shares[0.2]
