"""Reference of the limit indices (include/mpct.h, "Limit indices").

  * ``output_row`` / ``input_row`` / ``limits_scalar``: the contract restated sample by sample in Python floats
    (IEEE double, every subtraction and the product ex*ex rounded once: Python has no fused multiply-add), with
    the stated summation order -- lane l = (t - t0) mod 64 accumulates in ascending t from 0.0, the 64 partials
    are combined as a pairwise tree in lane order (indices_ref.lane_sum);
  * ``check_order_free``: every sum against math.fsum of the same rounded terms within n * 2^-53 * sum|term|, the
    bound of ANY summation order of n terms;
  * ``generated``: seeded trajectories and bounds that carry the contract's edges, by name (see its docstring).
"""
import math

import numpy as np

from indices_ref import bits, lane_sum

Y_FIELDS = ("viol", "viol2", "vmax", "t_vmax", "n_out", "t_in", "y_margin")
U_FIELDS = ("n_lo", "n_hi", "n_rate", "sat_run", "u_margin", "du_margin")
INT_FIELDS = ("t_vmax", "n_out", "t_in", "n_lo", "n_hi", "n_rate", "sat_run")
SUM_FIELDS = ("viol", "viol2")
BOUNDS = ("y_lo", "y_hi", "u_lo", "u_hi", "du_lo", "du_hi")
NAN, INF = float("nan"), float("inf")


def excess(yv, lo, hi):
    """ex = fmax(fmax(lo - y, y - hi), 0.0), a zero always +0.0"""
    m = max(lo - yv, yv - hi)
    return m if m > 0.0 else 0.0


def output_terms(y, lo, hi, t0):
    ex = [excess(float(y[t]), lo, hi) for t in range(t0, len(y))]
    return {"viol": ex, "viol2": [x * x for x in ex]}


def output_row(y, lo, hi, t0, out_tol):
    nit = len(y)
    lo, hi, out_tol = float(lo), float(hi), float(out_tol)
    if not all(math.isfinite(float(y[t])) for t in range(t0, nit)):
        return {f: (-1 if f in INT_FIELDS else NAN) for f in Y_FIELDS}
    tm = output_terms(y, lo, hi, t0)
    vmax, t_vmax, n_out, t_in, margin = -1.0, -1, 0, t0, INF
    for k, x in enumerate(tm["viol"]):
        if x > vmax:                       # strict: the first of equal maxima
            vmax, t_vmax = x, t0 + k
        if x > out_tol:
            n_out += 1
            t_in = t0 + k + 1
        yv = float(y[t0 + k])
        margin = min(margin, min(yv - lo, hi - yv))
    return {"viol": lane_sum(tm["viol"]), "viol2": lane_sum(tm["viol2"]), "vmax": vmax, "t_vmax": t_vmax,
            "n_out": n_out, "t_in": t_in, "y_margin": margin + 0.0}


def input_row(u, u_lo, u_hi, du_lo, du_hi, t0, sat_tol):
    nit = len(u)
    u_lo, u_hi, du_lo, du_hi, sat_tol = (float(x) for x in (u_lo, u_hi, du_lo, du_hi, sat_tol))
    if not all(math.isfinite(float(u[t])) for t in range(t0, nit)):
        return {f: (-1 if f in INT_FIELDS else NAN) for f in U_FIELDS}
    n_lo = n_hi = n_rate = run = sat_run = 0
    u_margin = du_margin = INF
    for t in range(t0, nit):
        uv = float(u[t])
        at_lo, at_hi = uv - u_lo <= sat_tol, u_hi - uv <= sat_tol
        n_lo += at_lo
        n_hi += at_hi
        run = run + 1 if (at_lo or at_hi) else 0
        sat_run = max(sat_run, run)
        u_margin = min(u_margin, min(uv - u_lo, u_hi - uv))
        if t >= t0 + 1:
            du = uv - float(u[t - 1])
            n_rate += (du - du_lo <= sat_tol) or (du_hi - du <= sat_tol)
            du_margin = min(du_margin, min(du - du_lo, du_hi - du))
    return {"n_lo": int(n_lo), "n_hi": int(n_hi), "n_rate": int(n_rate), "sat_run": sat_run, "u_margin": u_margin + 0.0,
            "du_margin": du_margin + 0.0}


def _bound(P, name, n):
    a = P.get(name)
    none = -INF if name.endswith("lo") else INF
    return np.full(n, none) if a is None else np.broadcast_to(np.asarray(a, dtype=np.float64), (n,))


def limits_scalar(y, u, P, t0):
    """y [S, my, nit], u [S, nu, nit], P: the bounds (absent / None: no bound), out_tol, sat_tol
    -> dict of [S, my] / [S, nu] arrays"""
    S, my = y.shape[:2]
    nu = u.shape[1]
    out = {f: np.zeros((S, my), dtype=np.int32 if f in INT_FIELDS else np.float64) for f in Y_FIELDS}
    out.update({f: np.zeros((S, nu), dtype=np.int32 if f in INT_FIELDS else np.float64) for f in U_FIELDS})
    b = {name: _bound(P, name, my if name[0] == "y" else nu) for name in BOUNDS}
    for s in range(S):
        for i in range(my):
            for f, x in output_row(y[s, i], b["y_lo"][i], b["y_hi"][i], t0, P["out_tol"]).items():
                out[f][s, i] = x
        for j in range(nu):
            row = input_row(u[s, j], b["u_lo"][j], b["u_hi"][j], b["du_lo"][j], b["du_hi"][j], t0, P["sat_tol"])
            for f, x in row.items():
                out[f][s, j] = x
    return out


def mismatches(got, want, fields=None):
    """[(field, index)] of the elements that differ bit for bit"""
    bad = []
    for f in (fields or Y_FIELDS + U_FIELDS):
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


def check_order_free(got, y, P, t0):
    """each sum of ``got`` against math.fsum of its rounded terms within n * 2^-53 * sum |term|"""
    S, my = y.shape[:2]
    lo, hi = _bound(P, "y_lo", my), _bound(P, "y_hi", my)
    checked = 0
    for s in range(S):
        for i in range(my):
            if np.isnan(got["viol"][s, i]):
                continue
            for f, tm in output_terms(y[s, i], float(lo[i]), float(hi[i]), t0).items():
                bound = len(tm) * 2.0 ** -53 * math.fsum(abs(x) for x in tm)
                assert abs(float(got[f][s, i]) - math.fsum(tm)) <= bound, (f, s, i, got[f][s, i], math.fsum(tm), bound)
                checked += 1
    return checked


OUT_TOL, SAT_TOL = 0.25, 0.125
LONG = 70      # nit - t0 from which the rows below that need two blocks are planted
# per channel, cycled: a finite band; lo == hi; a zero lower bound alone; both bounds infinite
_Y_LO, _Y_HI = (-0.5, 0.5, 0.0, -INF), (1.0, 0.5, INF, INF)
# a finite range with rate bounds; a zero upper bound alone
_U_LO, _U_HI, _DU_LO, _DU_HI = (-1.0, -INF), (0.5, 0.0), (-0.25, -INF), (0.25, INF)


def generated(S, my, nu, nit, t0, seed=0):
    """Trajectories y [S, my, nit], u [S, nu, nit] and the parameters P, with what the contract's edges need.
    Positions k are relative to t0, as the kernel's 64-sample blocks are.

    Outputs.  Channel i % 4: 0 the band [-0.5, 1], 1 lo == hi = 0.5, 2 [0, +inf) with rows of +-0.0 and positive
    values (ex and the margin against a zero bound), 3 no bound.  Even rows (s * my + i) are quantised to 1/16,
    odd rows are full-precision noise of amplitude 1.5 (sums that round).  With nit - t0 > 12, channel 0 of an
    even row (simulation 3 excepted) holds ex exactly at OUT_TOL (k = 5: inside), one ulp above it (k = 7: outside) and three equal peaks
    on both sides of the band (k = 8, 9, 10: t_vmax = t0 + 8).  Simulation 3's channel 0 stays inside the band
    (y_margin > 0, n_out = 0, t_in = t0); simulation 4's ends outside (t_in = nit).

    Inputs.  Channel j % 2: 0 the range [-1, 0.5] with the rate bounds +-0.25, 1 u <= 0 alone.  Channel 0 is a
    clipped random walk on the 1/8 grid (even s + j) or in full precision; with nit - t0 >= LONG simulations 0, 2,
    3 and 4 carry instead the named runs of RUNS on a quiet row, and simulation 0 three samples at u_lo + SAT_TOL
    and one ulp either side of it (k = 1, 2, 3).  Channel 1 of simulation 0 is +-0.0 throughout (one run over the
    whole row, at a zero bound); other rows of channel 1 are negative walks.

    Simulation 1 is all NaN, one y sample of simulation 2 is +inf and one u sample of its channel 1 is -inf."""
    rng = np.random.default_rng(seed)
    t = np.arange(nit)
    n = nit - t0
    P = {"y_lo": [_Y_LO[i % 4] for i in range(my)], "y_hi": [_Y_HI[i % 4] for i in range(my)],
         "u_lo": [_U_LO[j % 2] for j in range(nu)], "u_hi": [_U_HI[j % 2] for j in range(nu)],
         "du_lo": [_DU_LO[j % 2] for j in range(nu)], "du_hi": [_DU_HI[j % 2] for j in range(nu)],
         "out_tol": OUT_TOL, "sat_tol": SAT_TOL}
    y = np.zeros((S, my, nit))
    u = np.zeros((S, nu, nit))
    for s in range(S):
        for i in range(my):
            even = (s * my + i) % 2 == 0
            if i % 4 == 2:
                row = np.abs(np.round(4.0 * rng.standard_normal(nit)) / 4.0)
                row[t % 3 == 0] = 0.0
                row[t % 6 == 0] = -0.0
            elif even:
                row = np.round(16.0 * (0.6 + 0.8 * np.sin(t / 5.0 + s) + 0.2 * rng.standard_normal(nit))) / 16.0
            else:
                row = 1.5 * np.sin(t / 7.0 + s) + 0.3 * rng.standard_normal(nit)
            if i % 4 == 0 and s == 3:
                row = 0.25 + 0.5 * np.sin(t / 4.0)
            if i % 4 == 0 and even and n > 12 and s != 3:
                row[t0 + 5] = 1.0 + OUT_TOL
                row[t0 + 7] = np.nextafter(1.0 + OUT_TOL, 2.0)
                row[t0 + 8], row[t0 + 9], row[t0 + 10] = 3.0, -2.5, 3.0
            if i % 4 == 0 and s == 4:
                row[nit - 1] = 3.0
            y[s, i] = row
        for j in range(nu):
            walk = np.cumsum(0.2 * rng.standard_normal(nit))
            if j % 2 == 1:
                row = -np.abs(np.round(8.0 * walk) / 8.0) if s else np.where(t % 2 == 0, -0.0, 0.0)
            elif (s + j) % 2 == 0:
                row = np.clip(np.round(8.0 * walk) / 8.0, -1.0, 0.5)
            else:
                row = np.clip(walk, -1.125, 0.625)
            if j % 2 == 0 and n >= LONG and s in RUNS:
                row = 0.0625 * (np.arange(nit) % 3)
                for k0, k1, val in RUNS[s][1](n):
                    row[t0 + k0:t0 + k1] = val
                if s == 0:
                    row[t0 + 1:t0 + 4] = (-1.0 + SAT_TOL, np.nextafter(-1.0 + SAT_TOL, 0.0), np.nextafter(-1.0 + SAT_TOL, -1.0))
            u[s, j] = row
    if S > 1:
        y[1], u[1] = np.nan, np.nan
    if S > 2 and my:
        y[2, my - 1, nit // 2] = np.inf
    if S > 2 and nu > 1:
        u[2, 1, nit - 1] = -np.inf
    return y, u, P


# simulation -> (name, the saturated stretches [k0, k1) and their value as a function of n = nit - t0, sat_run)
RUNS = {0: ("a run ending at sample 63", lambda n: [(10, 13, 0.5), (59, 64, 0.5)], lambda n: 5),
        2: ("a run starting at sample 64", lambda n: [(20, 22, -1.0), (64, 68, 0.5)], lambda n: 4),
        3: ("a run crossing samples 63 and 64", lambda n: [(61, 67, -1.0), (30, 33, 0.5)], lambda n: 6),
        4: ("two equal runs, the second ending at the last sample", lambda n: [(5, 8, 0.5), (n - 3, n, 0.5)], lambda n: 3)}
