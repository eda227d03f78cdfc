"""The yardstick of the trajectory envelopes (mpct_envelope, mpct_eval_robust_envelope; include/mpct.h): the
trajectories y [C, D, rows, nit], read as they lie in memory, are the table x [C, D, rows * nit] of mpct_draw_stats,
so the envelope is draw_stats_ref.stats_ref of the reshaped array -- no statistics code of its own -- and the spread
is a scalar restatement of the header's rule on the lo and hi that reference gives: d(t) = hi(t) - lo(t), lane
(t - t0) mod 64 adds its d in ascending t from 0.0, the 64 partials combine as a pairwise tree in lane order
(indices_ref.lane_sum); the maximum and the first t that attains it."""
import math

import numpy as np
from draw_stats_ref import FIELDS, INT_FIELDS, LEVEL, stats_ref
from indices_ref import lane_sum

NAN = math.nan
SPREAD = ("spread", "spread_max", "t_spread_max")


def spread_row(lo, hi, t0):
    """lo, hi: one row's nit samples -> (spread, spread_max, t_spread_max)"""
    lo, hi = [float(v) for v in lo], [float(v) for v in hi]
    if any(lo[t] != lo[t] for t in range(t0, len(lo))):
        return NAN, NAN, -1
    d = [hi[t] - lo[t] for t in range(t0, len(lo))]
    mx, tm = -1.0, -1
    for k, v in enumerate(d):
        if v > mx:
            mx, tm = v, t0 + k
    return lane_sum(d, 0), mx, tm


def spread_ref(lo, hi, t0):
    """lo, hi [C, rows, nit] -> dict of spread, spread_max float64 and t_spread_max int32, each [C, rows]"""
    Cn, rows, _ = lo.shape
    out = {"spread": np.empty((Cn, rows)), "spread_max": np.empty((Cn, rows)), "t_spread_max": np.empty((Cn, rows), np.int32)}
    for c in range(Cn):
        for i in range(rows):
            out["spread"][c, i], out["spread_max"][c, i], out["t_spread_max"][c, i] = spread_row(lo[c, i], hi[c, i], t0)
    return out


def spread_rows(nit=200, t0=3):
    """Three rows of a D = 2 table whose draw 0 is the band's lower and draw 1 its upper edge.  Row 0: d(t0) = 2^53
    and every other d = 1, so a sequential sum loses every 1 while the lanes keep theirs.  Row 1: the maximum
    2.0 at t = 10 and again two 64-sample blocks later, at t = 138: one lane holds both.  Row 2: the maximum at
    t = 20 and at t = 70, which from t0 = 3 belong to lanes 17 and 3: the later one sits in the lower lane, so the
    first maximum is a selection across lanes."""
    rng = np.random.default_rng(5)
    lo, hi = np.zeros((3, nit)), np.ones((3, nit))
    hi[0, t0] = 2.0 ** 53
    lo[1:] = rng.random((2, nit))
    hi[1:] = lo[1:] + rng.random((2, nit))             # every d below 1
    lo[1, 10] = lo[1, 138] = lo[2, 20] = lo[2, 70] = 0.25
    hi[1, 10] = hi[1, 138] = hi[2, 20] = hi[2, 70] = 2.25
    return lo, hi


def envelope_ref(x, alive=None, levels=(), t0=0, stats=stats_ref):
    """x [C, D, rows, nit] -> (record dict with arrays [C, rows, nit] / [C, rows, nit, nlev], spread dict).  `stats`:
    the statistics of the reshaped table, stats_ref or a planted variant of it."""
    x = np.ascontiguousarray(x, dtype=np.float64)
    Cn, D, rows, nit = x.shape
    st = stats(x.reshape(Cn, D, rows * nit), alive, levels)
    nlev = st["quantile"].shape[2]
    rec = {f: np.ascontiguousarray(st[f].reshape((Cn, rows, nit, nlev) if f in LEVEL else (Cn, rows, nit))) for f in FIELDS}
    return rec, spread_ref(rec["lo"], rec["hi"], t0)


def assert_same_spread(got, want, msg=""):
    from draw_stats_ref import assert_same_stats

    assert_same_stats(got, want, fields=SPREAD, msg=msg)


__all__ = ["envelope_ref", "spread_ref", "spread_row", "assert_same_spread", "spread_rows", "SPREAD", "FIELDS", "INT_FIELDS", "LEVEL"]
