"""A float64 model of the int8 first stage of the two-precision hop (SDB_TUNE_SKETCH = 3, 4), independent of the
kernel's arithmetic.  The walk, the replay and the tally are tests/two_precision_model.py's; what is restated here is

* the copy (`Copy8`): one scale per table, s = the largest |element| / 127 rounded up (float32), y8 = clamp(rint(y / s),
  -127, 127) with the division in float32, the maxima E8max = max ||y - s y8||, Y8max = max ||s y8|| and the largest error
  of a row relative to its own norm, all in float64; the rule by which a table is refused the copy (`refused`);
* the two-term query (`query8`): s_q = max |q_i| / 127, a = clamp(rint(q / s_q)), b = clamp(rint((q - s_q a) 128 / s_q)),
  q^ = (s_q / 128)(128 a + b), in the kernel's float32 steps;
* the exact integer sum W = sum (128 a + b) y8 and d8 = metric(s (s_q / 128) W), exact in float64;
* the bound: upper  d8 - (||q - q^|| Y8max + ||q|| E8max) > tail,
             lower  the same with every inflation the kernel documents (walk_stage.h Int8Rows) charged generously.

The kernel's derivation implies  lower <= discarded on the device <= upper <= discardable.
"""
import numpy as np

from tests.two_precision_model import Graph, Tally, impl_of, run_model  # noqa: F401  (Graph: re-exported for the tests)

MAX_RATIO = 0.16  # index.h kSketch8MaxRatio


def scale_of(amax):
    """the table's scale from its largest |element| (float32): amax / 127 rounded up; 0, Inf and NaN stay"""
    s0 = np.float32(amax) / np.float32(127.0)
    if s0 > 0 and s0 < np.float32(3.0e38):
        return np.nextafter(s0, np.float32(3.4e38), dtype=np.float32)
    return np.float32(s0)


def absmax(rows):
    a = np.abs(np.asarray(rows, dtype=np.float32))
    return np.float32(np.nan) if np.isnan(a).any() else np.float32(a.max() if a.size else 0.0)


class Copy8:
    """the int8 copy of `rows` under `scale` (default: from their own largest |element|)"""

    def __init__(self, rows, scale=None):
        rows = np.asarray(rows, dtype=np.float32)
        self.amax = absmax(rows)
        self.scale = scale_of(self.amax) if scale is None else np.float32(scale)
        with np.errstate(all="ignore"):
            if self.scale != 0:
                f = np.rint(rows / self.scale)  # float32 division, round to nearest even
                f = np.where(np.isnan(f), np.float32(-127.0), np.clip(f, -127.0, 127.0))  # (fmaxf drops a NaN)
            else:
                f = np.zeros_like(rows)
            self.y8 = f.astype(np.int64)
            hv = np.float64(self.scale) * f.astype(np.float64)
            self.yhat = hv
            e = np.sqrt(((rows.astype(np.float64) - hv) ** 2).sum(1))
            y = np.sqrt((hv ** 2).sum(1))
            yn = np.sqrt((rows.astype(np.float64) ** 2).sum(1))
            rel = e[yn != 0] / yn[yn != 0]
        nanmax = lambda x: 0.0 if x.size == 0 else (np.nan if np.isnan(x).any() else float(x.max()))
        self.emax, self.ymax, self.rel = nanmax(e), nanmax(y), nanmax(rel)

    def refused(self):
        """the table keeps the float16 copy (index_sketch.hip build_sketch_kind)"""
        return not (self.emax <= MAX_RATIO * self.ymax) or not (self.rel <= MAX_RATIO)


def query8(q):
    """(a, b, s_q / 128) of one query, in the kernel's float32 steps"""
    q = np.asarray(q, dtype=np.float32)
    f32 = np.float32
    with np.errstate(all="ignore"):
        mx = f32(0.0) if np.isnan(np.abs(q)).all() else f32(np.nanmax(np.abs(q)))
        sq = f32(mx / f32(127.0))
        inv = f32(1.0) / sq if sq > 0 else f32(0.0)
        fa = np.rint(q * inv)
        fa = np.where(np.isnan(fa), f32(-127.0), np.clip(fa, -127.0, 127.0)).astype(f32)
        fb = np.rint(((q - sq * fa).astype(f32) * inv).astype(f32) * f32(128.0))
        fb = np.where(np.isnan(fb), f32(-127.0), np.clip(fb, -127.0, 127.0)).astype(f32)
    return fa.astype(np.int64), fb.astype(np.int64), f32(sq * f32(0.0078125))


class Bounds8:
    """per row, for one query: the threshold a tail must be BELOW for the neighbour to be discarded (`upper`: the pure
    bound; `lower`: with every documented inflation charged)"""

    def __init__(self, metric, q, copy):
        assert metric in ("cosine", "dot")
        q64 = np.asarray(q, dtype=np.float32).astype(np.float64)
        a, b, sq128 = query8(q)
        w = 128 * a + b
        with np.errstate(all="ignore"):
            qhat = np.float64(sq128) * w
            qerr = np.sqrt(((q64 - qhat) ** 2).sum())
            qn = np.sqrt((q64 ** 2).sum())
            W = copy.y8 @ w  # exact integers
            dot8 = np.float64(copy.scale) * np.float64(sq128) * W.astype(np.float64)
            d8 = (1.0 - dot8) if metric == "cosine" else -dot8
            eps = qerr * copy.ymax + qn * copy.emax
            self.upper = d8 - eps
            # Int8Rows::query, stage_eps: qerr, ||q||, E8max, Y8max carry 1.0001 each and the sum another, float32 roundings on top;
            # charged 1.001.  qerr gets 2e-7 ||q|| for the rounding of q^'s float32 value; charged 3e-7 x 1.001 ||q|| Y8max.
            # 2e-5 ||q|| (Y8max + E8max) for the reference's roundings and d8's three, inflated the same way, and d8's own
            # three once more because d8 is exact here; charged 3e-5 x 1.001.  FirstStage::out: 4e-7 (1 + |d8| + eps) for the
            # roundings of 1 - dot / -dot and of the subtraction; charged 2e-6 of the same terms.
            slack = 1.001 * eps + 3e-7 * 1.001 * qn * copy.ymax + 3e-5 * 1.001 * qn * (copy.ymax + copy.emax)
            self.lower = d8 - (slack + 2e-6 * (1.0 + np.abs(d8) + slack))


def count8(metric, copy, q, D, rep):
    """(met with the array full, discardable, upper, lower) over the chunks of one replayed walk"""
    b = Bounds8(metric, q, copy)
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


def run_model8(orc, g, metric, queries, limit, L, copy=None):
    """replays and int8 counts of a batch: ([Replay], Tally, D, Copy8).  The replays are two_precision_model.run_model's."""
    reps, _, D = run_model(orc, g, metric, queries, limit, L)
    copy = Copy8(g.vecs) if copy is None else copy
    t = Tally()
    for i in range(queries.shape[0]):
        t.add(count8(metric, copy, queries[i], D[i], reps[i]), reps[i], g)
    return reps, t, D, copy


def check_tally8(t, what):
    """the sandwich can see a half-broken stage: the counts are ordered, lower > 0 and within 2 % of upper"""
    assert t.lower <= t.upper <= t.discardable <= t.full, "%s: %r" % (what, t)
    assert t.lower > 0 and t.lower >= 0.98 * t.upper, "%s: lower / upper = %d / %d" % (what, t.lower, t.upper)


# ---------------------------------------------------------------------------------------------- pricing
def price(metric, copy, copy_rows, queries, D, reps, per_row=False):
    """kept / decided by the margin / within the margin, as shares of the neighbours evaluated with the array full.
    per_row: a scale per row (the row's own largest |element| / 127) in place of the table's"""
    if per_row:
        rows = np.asarray(copy_rows, dtype=np.float32)
        sc = np.array([scale_of(absmax(r)) for r in rows], dtype=np.float32)[:, None]
        with np.errstate(all="ignore"):
            f = np.clip(np.rint(rows / np.where(sc == 0, np.float32(1), sc)), -127, 127)
        yhat = sc.astype(np.float64) * f
        e = np.sqrt(((rows.astype(np.float64) - yhat) ** 2).sum(1))
        copy = Copy8(rows)
        copy.y8, copy.emax, copy.ymax = None, float(e.max()), float(np.sqrt((yhat ** 2).sum(1)).max())
        copy.yhat = yhat
    full = kept = decided = 0
    for i in range(queries.shape[0]):
        if per_row:
            a, b, sq128 = query8(queries[i])
            qhat = np.float64(sq128) * (128 * a + b)
            q64 = queries[i].astype(np.float64)
            dot8 = copy.yhat @ qhat
            d8 = (1.0 - dot8) if metric == "cosine" else -dot8
            upper = d8 - (np.sqrt(((q64 - qhat) ** 2).sum()) * copy.ymax + np.sqrt((q64 ** 2).sum()) * copy.emax)
        else:
            upper = Bounds8(metric, queries[i], copy).upper
        for tail, new in reps[i].chunks:
            if tail is None or len(new) == 0:
                continue
            full += len(new)
            kept += int((~(D[i][new] > tail)).sum())
            decided += int((upper[new] > tail).sum())
    return {"evaluated_full": full, "kept": round(kept / full, 4), "decided": round(decided / full, 4),
            "within_margin": round((full - kept - decided) / full, 4), "emax": copy.emax, "ymax": copy.ymax}
