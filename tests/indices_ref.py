"""Reference of the closed-loop performance indices (include/mpct.h, "Closed-loop performance indices").

Three parts:
  * ``output_row`` / ``input_row`` / ``indices_scalar``: the contract restated sample by sample in Python
    floats (IEEE double, every product rounded before it is added: Python has no fused multiply-add), with
    the stated summation order -- lane l = (t - t0) mod 64 accumulates in ascending t from 0.0, the 64
    partials are combined as a pairwise tree in lane order;
  * ``indices_np``: the same, vectorised over the rows; tests/test_indices.py holds it to the scalar one
    bit for bit;
  * ``check_order_free``: every sum against math.fsum of the same rounded terms within n * 2^-53 * sum|term|,
    the bound of ANY summation order of n terms, so a reference that copied a mistake of the kernel's order
    (or a kernel that dropped or doubled a term) is caught without trusting the order above.
"""
import math

import numpy as np

Y_FIELDS = ("iae", "ise", "itae", "emax", "t_emax", "over", "e_final", "settle")
U_FIELDS = ("tv", "du2", "dumax", "u_lo", "u_hi")
INT_FIELDS = ("t_emax", "settle")
SUM_FIELDS = ("iae", "ise", "itae", "tv", "du2")
NAN = float("nan")


def tree64(p):
    """the 64 lane partials combined pairwise in lane order"""
    p = list(p)
    assert len(p) == 64
    while len(p) > 1:
        p = [p[i] + p[i + 1] for i in range(0, len(p), 2)]
    return p[0]


def lane_sum(terms, first_lane=0):
    """terms[j] belongs to lane (first_lane + j) mod 64; each lane adds its terms in order, from 0.0"""
    p = [0.0] * 64
    for j, x in enumerate(terms):
        p[(first_lane + j) % 64] += x
    return tree64(p)


def output_terms(y, r, t0):
    """the rounded terms of iae, ise and itae of one output row, in ascending t"""
    e = [float(y[t]) - float(r[t]) for t in range(t0, len(y))]
    return {"iae": [abs(x) for x in e], "ise": [x * x for x in e], "itae": [float(k) * abs(x) for k, x in enumerate(e)]}


def input_terms(u, t0):
    du = [float(u[t]) - float(u[t - 1]) for t in range(t0 + 1, len(u))]
    return {"tv": [abs(x) for x in du], "du2": [x * x for x in du]}


def output_row(y, r, t0, band_rel, band_abs):
    nit = len(y)
    if not all(math.isfinite(float(y[t])) and math.isfinite(float(r[t])) for t in range(t0, nit)):
        return {f: (-1 if f in INT_FIELDS else NAN) for f in Y_FIELDS}
    e = [float(y[t]) - float(r[t]) for t in range(t0, nit)]
    tm = output_terms(y, r, t0)
    emax, t_emax = -1.0, -1
    for k, x in enumerate(e):
        if abs(x) > emax:
            emax, t_emax = abs(x), t0 + k
    rf = float(r[nit - 1])
    d = rf - float(y[t0])
    sg = 1.0 if d > 0 else (-1.0 if d < 0 else 0.0)
    if sg == 0.0:
        over = emax
    else:
        m = max(sg * x for x in e)
        over = m if m > 0 else 0.0
    prod = band_rel * abs(d)          # rounded, then added
    band = prod + band_abs
    settle = t0
    for t in range(t0, nit):
        if not abs(float(y[t]) - rf) <= band:
            settle = t + 1
    return {"iae": lane_sum(tm["iae"]), "ise": lane_sum(tm["ise"]), "itae": lane_sum(tm["itae"]), "emax": emax,
            "t_emax": t_emax, "over": over, "e_final": e[-1], "settle": settle}


def input_row(u, t0):
    nit = len(u)
    if not all(math.isfinite(float(u[t])) for t in range(t0, nit)):
        return {f: NAN for f in U_FIELDS}
    tm = input_terms(u, t0)
    us = [float(u[t]) for t in range(t0, nit)]
    # du(t) belongs to lane (t - t0) mod 64: the first one, t = t0 + 1, to lane 1
    return {"tv": lane_sum(tm["tv"], 1), "du2": lane_sum(tm["du2"], 1), "dumax": max(tm["tv"], default=0.0),
            "u_lo": min(us) + 0.0, "u_hi": max(us) + 0.0}


def _empty(S, my, nu):
    out = {f: np.zeros((S, my), dtype=np.int32 if f in INT_FIELDS else np.float64) for f in Y_FIELDS}
    out.update({f: np.zeros((S, nu)) for f in U_FIELDS})
    return out


def indices_scalar(y, u, r, t0, band_rel, band_abs):
    """y [S, my, nit], u [S, nu, nit], r [nref, my, nit] -> dict of [S, my] / [S, nu] arrays"""
    S, my, _ = y.shape
    nu, nref = u.shape[1], r.shape[0]
    out = _empty(S, my, nu)
    for s in range(S):
        for i in range(my):
            for f, x in output_row(y[s, i], r[s % nref, i], t0, band_rel, band_abs).items():
                out[f][s, i] = x
        for j in range(nu):
            for f, x in input_row(u[s, j], t0).items():
                out[f][s, j] = x
    return out


def _lane_tree(terms):
    """terms [..., n], term k in lane k mod 64 -> the contract's sum"""
    n = terms.shape[-1]
    p = np.zeros(terms.shape[:-1] + (64,))
    for b in range(0, n, 64):
        blk = terms[..., b:b + 64]
        p[..., :blk.shape[-1]] += blk
    while p.shape[-1] > 1:
        p = p[..., 0::2] + p[..., 1::2]
    return p[..., 0]


def indices_np(y, u, r, t0, band_rel, band_abs):
    y, u, r = (np.asarray(a, dtype=np.float64) for a in (y, u, r))
    S, my, nit = y.shape
    nref = r.shape[0]
    out = {}
    with np.errstate(all="ignore"):
        rr = r[np.arange(S) % nref]
        ys, rs = y[..., t0:], rr[..., t0:]
        e = ys - rs
        ae = np.abs(e)
        k = np.arange(nit - t0, dtype=np.float64)
        out["iae"], out["ise"], out["itae"] = _lane_tree(ae), _lane_tree(e * e), _lane_tree(k * ae)
        valid = np.isfinite(ys).all(-1) & np.isfinite(rs).all(-1)
        safe = np.where(valid[..., None], ae, 0.0)
        out["emax"] = safe.max(-1)
        out["t_emax"] = (t0 + safe.argmax(-1)).astype(np.int32)       # argmax: the first of equal maxima
        rf = rr[..., -1]
        d = rf - y[..., t0]
        sg = np.sign(d)
        m = np.where(valid[..., None], sg[..., None] * e, 0.0).max(-1)
        out["over"] = np.where(sg == 0, out["emax"], np.where(m > 0, m, 0.0))
        out["e_final"] = e[..., -1]
        band = band_rel * np.abs(d) + band_abs
        viol = ~(np.abs(ys - rf[..., None]) <= band[..., None])
        n = nit - t0
        last = np.where(viol.any(-1), n - 1 - viol[..., ::-1].argmax(-1), -1)
        out["settle"] = (t0 + last + 1).astype(np.int32)
        for f in Y_FIELDS:
            out[f] = np.where(valid, out[f], -1 if f in INT_FIELDS else np.nan).astype(out[f].dtype)
        us = u[..., t0:]
        du = us[..., 1:] - us[..., :-1]
        z = np.zeros(us.shape[:-1] + (1,))
        out["tv"] = _lane_tree(np.concatenate([z, np.abs(du)], -1))
        out["du2"] = _lane_tree(np.concatenate([z, du * du], -1))
        uval = np.isfinite(us).all(-1)
        out["dumax"] = np.concatenate([z, np.where(uval[..., None], np.abs(du), 0.0)], -1).max(-1)
        out["u_lo"] = np.where(uval[..., None], us, 0.0).min(-1) + 0.0
        out["u_hi"] = np.where(uval[..., None], us, 0.0).max(-1) + 0.0
        for f in U_FIELDS:
            out[f] = np.where(uval, out[f], np.nan)
    return out


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int64) if a.dtype == np.float64 else a


def assert_bitwise(got, want, fields=None, what=""):
    """every field equal bit for bit (NaN is the one quiet NaN 0x7ff8.., zeros keep their sign)"""
    for f in (fields or Y_FIELDS + U_FIELDS):
        g, w = np.asarray(got[f]), np.asarray(want[f])
        assert g.dtype == w.dtype and g.shape == w.shape, (what, f, g.dtype, w.dtype, g.shape, w.shape)
        bad = np.argwhere(bits(g) != bits(w))
        assert bad.size == 0, "%s %s: %d rows differ, first %s: got %r want %r" % (
            what, f, len(bad), bad[0].tolist(), g[tuple(bad[0])], w[tuple(bad[0])])


def check_order_free(got, y, u, r, t0):
    """each sum of ``got`` against math.fsum of its rounded terms within n * 2^-53 * sum |term|"""
    S, my, _ = y.shape
    nu, nref = u.shape[1], r.shape[0]
    checked = 0
    for s in range(S):
        for i in range(my):
            if np.isnan(got["iae"][s, i]):
                continue
            for f, tm in output_terms(y[s, i], r[s % nref, i], t0).items():
                bound = len(tm) * 2.0 ** -53 * math.fsum(abs(x) for x in tm)
                assert abs(float(got[f][s, i]) - math.fsum(tm)) <= bound, (f, s, i, got[f][s, i], math.fsum(tm), bound)
                checked += 1
        for j in range(nu):
            if np.isnan(got["tv"][s, j]):
                continue
            for f, tm in input_terms(u[s, j], t0).items():
                bound = len(tm) * 2.0 ** -53 * math.fsum(abs(x) for x in tm)
                assert abs(float(got[f][s, j]) - math.fsum(tm)) <= bound, (f, s, j, got[f][s, j], math.fsum(tm), bound)
                checked += 1
    return checked


BAND_REL, BAND_ABS = 0.25, 0.125


def generated(S, nref, my, nu, nit, seed=0):
    """Trajectories with what the contract's edges need.  Even output rows are quantised to 1/16 (ties in
    |e|, samples exactly on the band edge of t0 = 0 with BAND_REL / BAND_ABS, one a single ulp outside it),
    odd rows are full-precision noise (sums that round, so the summation order shows).  The references
    are steps starting at an index > 0, one channel's is identically 0 (sigma = 0 where y(t0) = 0).
    Simulation 1 is all NaN (a slot that was not run), one y sample is +inf, one u sample -inf, one r
    sample at t = 0 is NaN (invalid for t0 = 0 only), and zeros of both signs appear in y and u."""
    rng = np.random.default_rng(seed)
    t = np.arange(nit)
    r = np.zeros((nref, my, nit))
    for k in range(nref):
        for i in range(my):
            if (k + i) % 3 != 2:        # (k + i) % 3 == 2: a regulated channel, r = 0
                r[k, i, min(2 + k + 2 * i, nit - 1):] = (1.0 + 0.5 * k) * (-1.0 if i == 1 else 1.0)
    y = np.zeros((S, my, nit))
    u = np.zeros((S, nu, nit))
    for s in range(S):
        for i in range(my):
            rf = r[s % nref, i, -1]
            resp = rf * (1.0 - np.exp(-t / 9.0) * np.cos(t / 3.0 + s))
            if (s * my + i) % 2 == 0:
                row = np.round(16.0 * (resp + 0.2 * rng.standard_normal(nit) * np.exp(-t / 40.0))) / 16.0
                if nit > 12:
                    # two equal peak errors of opposite sign, later than the reference's step
                    row[9] = r[s % nref, i, 9] + 4.5
                    row[11] = r[s % nref, i, 11] - 4.5
                if nit > 40:
                    band = BAND_REL * abs(rf - row[0]) + BAND_ABS     # exact: multiples of 1/64
                    row[nit - 7] = rf + band                          # on the edge: inside
                    row[nit - 5] = rf - band
                    if s % 2 == 1:
                        row[nit - 3] = np.nextafter(rf + band, np.inf)  # one ulp outside
            else:
                row = resp + 0.3 * rng.standard_normal(nit) * np.exp(-t / 25.0) + 1e-3 * rng.standard_normal(nit)
            y[s, i] = row
        for j in range(nu):
            mv = np.cumsum(rng.standard_normal(nit) * np.exp(-t / 30.0))
            u[s, j] = np.round(8.0 * mv) / 8.0 if (s + j) % 2 == 0 else mv
    # a regulated channel that starts at rest: y(0) = y(1) = r = 0, with a negative zero
    for s in range(S):
        for i in range(my):
            if not r[s % nref, i].any():
                y[s, i, :2] = (-0.0, 0.0)[:min(2, nit)]
    if S > 4:
        u[4, 0] = np.where(t % 2 == 0, -0.0, 0.0)     # zeros of both signs only: u_lo = u_hi = +0.0
    if S > 1:
        y[1], u[1] = np.nan, np.nan
    if S > 2:
        y[2, my - 1, nit // 2] = np.inf
    if S > 3:
        u[3, 0, nit - 1] = -np.inf
    if nit > 1 and nref > 1:
        r[nref - 1, my - 1, 0] = np.nan
    return y, u, r
