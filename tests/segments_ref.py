"""Reference of the step-response indices per setpoint segment (include/mpct.h, "Step-response indices per
setpoint segment").

  * ``output_unit`` / ``input_unit`` / ``segments_scalar``: the contract restated sample by sample in Python
    floats (IEEE double, every product rounded before it is added: Python has no fused multiply-add), with the
    stated summation order -- lane l = (t - a) mod 64 accumulates in ascending t from 0.0, the 64 partials are
    combined as a pairwise tree in lane order (indices_ref.lane_sum);
  * ``segments_np``: the vectorised form, held to the first by tests/test_segments.py;
  * ``MISTAKES``: planted mistakes ``segments_scalar(.., mistake=name)`` commits on purpose; each must break the
    comparison on the committed cases (tests/test_segments.py);
  * ``generated``: seeded trajectories that carry the contract's edges.
"""
import math

import numpy as np

from indices_ref import _lane_tree, bits, lane_sum

Y_FIELDS = ("iae", "ise", "itae", "emax", "t_emax", "over", "under", "e_final", "settle", "rise")
U_FIELDS = ("tv", "du2", "dumax", "u_lo", "u_hi")
FIELDS = Y_FIELDS + U_FIELDS          # their positions are the MPCT_SX_* ids
INT_FIELDS = ("t_emax", "settle", "rise")
NAN = float("nan")
MISTAKES = ("base_from_y", "rg_at_a", "boundary_move_earlier", "rise_from_a", "itae_absolute_t", "settle_relative")


def _invalid(fields):
    return {f: (-1 if f in INT_FIELDS else NAN) for f in fields}


def output_unit(y, r, a, b, first, base, band_rel, band_abs, rise_lo, rise_hi, mistake=None):
    """one (output row, segment): the samples a <= t < b; ``first``: segment 0"""
    use_r = base == 1 and not first and mistake != "base_from_y"
    read = [float(y[t]) for t in range(a, b)] + [float(r[t]) for t in range(a, b)] + ([float(r[a - 1])] if use_r else [])
    if not all(math.isfinite(x) for x in read):
        return _invalid(Y_FIELDS)
    ys = [float(y[t]) for t in range(a, b)]
    e = [float(y[t]) - float(r[t]) for t in range(a, b)]
    ae = [abs(x) for x in e]
    k_of = (lambda k: float(a + k)) if mistake == "itae_absolute_t" else float
    emax, t_emax = -1.0, -1
    for k, x in enumerate(ae):
        if x > emax:                       # strict: the first of equal maxima
            emax, t_emax = x, a + k
    rg = float(r[a]) if mistake == "rg_at_a" else float(r[b - 1])
    c = float(r[a - 1]) if use_r else float(y[a])
    d = rg - c
    sg = 1.0 if d > 0 else (-1.0 if d < 0 else 0.0)
    p = [sg * (x - c) for x in ys]
    if sg == 0.0:
        over, under, rise = emax, 0.0, -1
    else:
        m = max(sg * x for x in e)
        over = m if m > 0 else 0.0
        w = max(-x for x in p)
        under = w if w > 0 else 0.0
        lvl_lo, lvl_hi = rise_lo * abs(d), rise_hi * abs(d)     # rounded products
        t_lo = next((a + k for k, x in enumerate(p) if x >= lvl_lo), None)
        t_hi = next((a + k for k, x in enumerate(p) if x >= lvl_hi), None)
        rise = b - a if t_hi is None else t_hi - (a if mistake == "rise_from_a" else t_lo)
    prod = band_rel * abs(d)               # rounded, then added
    band = prod + band_abs
    settle = a
    for t in range(a, b):
        if not abs(float(y[t]) - rg) <= band:
            settle = t + 1
    if mistake == "settle_relative":
        settle -= a
    return {"iae": lane_sum(ae), "ise": lane_sum([x * x for x in e]),
            "itae": lane_sum([k_of(k) * x for k, x in enumerate(ae)]), "emax": emax, "t_emax": t_emax, "over": over,
            "under": under, "e_final": float(y[b - 1]) - float(r[b - 1]), "settle": settle, "rise": rise}


def input_unit(u, a, b, first, mistake=None):
    """one (input row, segment): the moves du(t), t in [max(a, tseg[0] + 1), b), and the range over [a, b)"""
    lo_t, hi_t = (a + 1 if first else a), b
    if mistake == "boundary_move_earlier":   # the move across the boundary b counted here, not in the next one
        lo_t, hi_t = a + 1, min(b + 1, len(u))
    read = [float(u[t]) for t in range(a, b)] + ([] if first else [float(u[a - 1])])
    if not all(math.isfinite(x) for x in read):
        return _invalid(U_FIELDS)
    du = [float(u[t]) - float(u[t - 1]) for t in range(lo_t, hi_t)]
    us = [float(u[t]) for t in range(a, b)]
    lane0 = (lo_t - a) % 64                  # du(t) belongs to lane (t - a) mod 64
    return {"tv": lane_sum([abs(x) for x in du], lane0), "du2": lane_sum([x * x for x in du], lane0),
            "dumax": max((abs(x) for x in du), default=0.0), "u_lo": min(us) + 0.0, "u_hi": max(us) + 0.0}


def _empty(S, my, nu, nseg):
    out = {f: np.zeros((S, my, nseg), dtype=np.int32 if f in INT_FIELDS else np.float64) for f in Y_FIELDS}
    out.update({f: np.zeros((S, nu, nseg)) for f in U_FIELDS})
    return out


def segments_scalar(y, u, r, tseg, base=1, band_rel=0.02, band_abs=0.0, rise_lo=0.1, rise_hi=0.9, mistake=None):
    """y [S, my, nit], u [S, nu, nit], r [nref, my, nit] -> dict of [S, my, nseg] / [S, nu, nseg] arrays"""
    S, my = y.shape[:2]
    nu, nref, nseg = u.shape[1], r.shape[0], len(tseg) - 1
    out = _empty(S, my, nu, nseg)
    for g in range(nseg):
        a, b = int(tseg[g]), int(tseg[g + 1])
        for s in range(S):
            for i in range(my):
                unit = output_unit(y[s, i], r[s % nref, i], a, b, g == 0, base, band_rel, band_abs, rise_lo, rise_hi, mistake)
                for f, x in unit.items():
                    out[f][s, i, g] = x
            for j in range(nu):
                for f, x in input_unit(u[s, j], a, b, g == 0, mistake).items():
                    out[f][s, j, g] = x
    return out


def _first(mask, a, none):
    """the first true sample of mask [..., n] as an absolute time, ``none`` where there is none"""
    return np.where(mask.any(-1), a + mask.argmax(-1), none)


def segments_np(y, u, r, tseg, base=1, band_rel=0.02, band_abs=0.0, rise_lo=0.1, rise_hi=0.9):
    """the vectorised form of segments_scalar"""
    y, u, r = (np.asarray(x, dtype=np.float64) for x in (y, u, r))
    S, my, nit = y.shape
    nu, nref, nseg = u.shape[1], r.shape[0], len(tseg) - 1
    out = _empty(S, my, nu, nseg)
    rr = r[np.arange(S) % nref] if my else np.zeros((S, 0, nit))
    with np.errstate(all="ignore"):
        for g in range(nseg):
            a, b = int(tseg[g]), int(tseg[g + 1])
            n = b - a
            ys, rs = y[..., a:b], rr[..., a:b]
            use_r = base == 1 and g > 0
            c = rr[..., a - 1] if use_r else y[..., a]
            valid = np.isfinite(ys).all(-1) & np.isfinite(rs).all(-1) & np.isfinite(c)
            e = ys - rs
            ae = np.abs(e)
            k = np.arange(n, dtype=np.float64)
            o = {"iae": _lane_tree(ae), "ise": _lane_tree(e * e), "itae": _lane_tree(k * ae)}
            safe = np.where(valid[..., None], ae, 0.0)
            o["emax"] = safe.max(-1)
            o["t_emax"] = a + safe.argmax(-1)
            rg = rr[..., b - 1]
            d = rg - c
            sg = np.sign(d)
            sg = np.where(np.isnan(sg), 0.0, sg)
            m = np.where(valid[..., None], sg[..., None] * e, 0.0).max(-1)
            o["over"] = np.where(sg == 0, o["emax"], np.where(m > 0, m, 0.0))
            p = sg[..., None] * (ys - c[..., None])
            w = np.where(valid[..., None], -p, 0.0).max(-1)
            o["under"] = np.where((sg != 0) & (w > 0), w, 0.0)
            o["e_final"] = e[..., -1]
            band = band_rel * np.abs(d) + band_abs
            viol = ~(np.abs(ys - rg[..., None]) <= band[..., None])
            o["settle"] = a + np.where(viol.any(-1), n - 1 - viol[..., ::-1].argmax(-1), -1) + 1
            t_lo = _first(p >= (rise_lo * np.abs(d))[..., None], a, a)
            t_hi = _first(p >= (rise_hi * np.abs(d))[..., None], a, -1)
            o["rise"] = np.where(sg == 0, -1, np.where(t_hi < 0, n, t_hi - t_lo))
            for f in Y_FIELDS:
                out[f][..., g] = np.where(valid, o[f], -1 if f in INT_FIELDS else np.nan)
            us = u[..., a:b]
            z = np.zeros(us.shape[:-1] + (1,))
            prev = u[..., a - 1:a] if g > 0 else us[..., :1]
            du = us - np.concatenate([prev, us[..., :-1]], -1)
            if g == 0:
                du = np.concatenate([z, du[..., 1:]], -1)     # no move into the first sample: lane 0 adds +0.0
            uval = np.isfinite(us).all(-1) & (np.isfinite(prev[..., 0]) if g > 0 else True)
            o = {"tv": _lane_tree(np.abs(du)), "du2": _lane_tree(du * du),
                 "dumax": np.where(uval[..., None], np.abs(du), 0.0).max(-1),
                 "u_lo": np.where(uval[..., None], us, 0.0).min(-1) + 0.0,
                 "u_hi": np.where(uval[..., None], us, 0.0).max(-1) + 0.0}
            for f in U_FIELDS:
                out[f][..., g] = np.where(uval, o[f], np.nan)
    return out


def mismatches(got, want, fields=None):
    """[(field, index)] of the elements that differ bit for bit"""
    bad = []
    for f in (fields or FIELDS):
        g, w = np.asarray(got[f]), np.asarray(want[f])
        assert g.dtype == w.dtype and g.shape == w.shape, (f, g.dtype, w.dtype, g.shape, w.shape)
        bad += [(f, tuple(ix)) for ix in np.argwhere(bits(g) != bits(w)).tolist()]
    return bad


def assert_bitwise(got, want, fields=None, what=""):
    """every field equal bit for bit (NaN is the one quiet NaN 0x7ff8.., zeros keep their sign)"""
    bad = mismatches(got, want, fields)
    if bad:
        f, ix = bad[0]
        raise AssertionError("%s %s: %d elements differ, first %s: got %r want %r" % (
            what, f, len(bad), list(ix), np.asarray(got[f])[ix], np.asarray(want[f])[ix]))


def reference_segments(r, extra=()):
    """the boundaries mpct_reference_segments gives: {0} u {t >= 1: some row of r changes at t} u extra u {nit}"""
    r = np.asarray(r, dtype=np.float64)
    nit = r.shape[-1]
    flat = r.reshape(-1, nit)
    changes = np.nonzero((flat[:, 1:] != flat[:, :-1]).any(0))[0] + 1
    return sorted({0, nit} | set(int(t) for t in changes) | set(int(t) for t in extra))


def generated(S, nref, my, nu, nit, tseg, seed=0):
    """Trajectories y [S, my, nit], u [S, nu, nit] and references r [nref, my, nit] (piecewise constant, changing at
    the boundaries tseg[1:-1]) with what the contract's edges need, per segment [a, b):

    * even rows (s * my + i) are quantised to 1/16 (exact sums, ties of the peak: two samples of equal |e| are
      planted at a + 1 and a + 3 where the segment is long enough, simulation 2 excepted), odd rows
      full-precision responses whose sums round;
    * channel 0 approaches each new level first-order from the level before; channel 1 starts every segment the
      wrong way (inverse response: under > 0), and the last reference set's channel 1 ramps inside each segment,
      so that r(b-1) differs from r(a); channel 2, where present, has a reference that never moves
      (sigma = 0 with base = 1) and carries -0.0 samples;
    * simulation 2's channel 0 stops short of rise_hi (0.9) in every segment (rise = b - a);
    * in simulation 0, channel 0, a sample sits exactly on the rise levels 0.1 |d| and 0.9 |d| with |d| = 1 and
      exactly on the band edge band_abs = 0.125 at the last but one sample of each segment of length >= 6;
    * inputs: even rows a walk on the 1/8 grid, odd rows full precision; channel 1 of simulation 0 is +-0.0
      throughout.

    NaN and infinities are planted by the tests, which know which unit they spoil."""
    rng = np.random.default_rng(seed)
    nseg = len(tseg) - 1
    t = np.arange(nit)
    r = np.zeros((nref, my, nit))
    for k in range(nref):
        for i in range(my):
            for g in range(nseg):
                # channel 0: 0, 1 + k/2, 0, ..  (|d| = 1 for reference set 0); channel 1: +-(1 + k); channel 2: 0
                level = (g % 2) * (1.0 + 0.5 * k) if i == 0 else (float((-1) ** g) * (1 + k) if i == 1 else 0.0)
                r[k, i, int(tseg[g]):] = level
                if i == 1 and k == nref - 1:
                    # the last reference set's channel 1 ramps inside each segment: r(b-1) is not r(a)
                    a, b = int(tseg[g]), int(tseg[g + 1])
                    r[k, i, a:b] = level + np.arange(b - a) / 64.0
    y = np.zeros((S, my, nit))
    u = np.zeros((S, nu, nit))
    for s in range(S):
        for i in range(my):
            rr = r[s % nref, i]
            row = np.zeros(nit)
            lvl = 0.0
            for g in range(nseg):
                a, b = int(tseg[g]), int(tseg[g + 1])
                k = np.arange(b - a)
                target = rr[b - 1]
                reach = 0.8 if (s == 2 and i == 0) else 1.0
                resp = lvl + reach * (target - lvl) * (1.0 - np.exp(-(k + 1) / (2.0 + s)))
                if i == 1:
                    resp = resp - 0.4 * (target - lvl) * np.exp(-k / 1.5)      # starts the wrong way
                row[a:b] = resp + 0.02 * rng.standard_normal(b - a)
                lvl = target
            if (s * my + i) % 2 == 0:
                row = np.round(16.0 * row) / 16.0
                for g in range(nseg):
                    a, b = int(tseg[g]), int(tseg[g + 1])
                    if b - a >= 5 and s != 2:
                        row[a + 1] = rr[a + 1] + 8.0
                        row[a + 3] = rr[a + 3] - 8.0
            if i == 2:
                row = np.where(t % 5 == 0, -0.0, np.round(8.0 * 0.3 * np.sin(t / 3.0 + s)) / 8.0)
            if s == 0 and i == 0:
                for g in range(1, nseg):
                    a, b = int(tseg[g]), int(tseg[g + 1])
                    if b - a >= 6:
                        c, d = rr[a - 1], rr[b - 1] - rr[a - 1]
                        row[a:b] = c + d * np.minimum(1.0, 0.05 + 0.15 * np.arange(b - a))
                        row[a + 1] = c + 0.1 * d        # exactly on rise_lo |d| (|d| = 1: 0.1 * 1 = 0.1)
                        row[a + 2] = c + 0.5 * d
                        row[a + 3] = c + 0.9 * d        # exactly on rise_hi |d|
                        row[b - 2] = rr[b - 1] + 0.125  # exactly on the band edge band_abs
            y[s, i] = row
        for j in range(nu):
            walk = np.cumsum(0.2 * rng.standard_normal(nit))
            row = np.round(8.0 * walk) / 8.0 if (s + j) % 2 == 0 else walk
            if s == 0 and j == 1:
                row = np.where(t % 2 == 0, -0.0, 0.0)
            u[s, j] = row
    return y, u, r
