"""Reference of the oscillation indices per setpoint segment (include/mpct.h, "Oscillation indices per setpoint
segment").

  * ``output_unit`` / ``input_unit`` / ``osc_scalar``: the contract restated sample by sample in Python floats
    (IEEE double; band_rel*|d| is rounded before band_abs is added: Python has no fused multiply-add).  Every
    field is an exact integer, a maximum or one division: there is no sum and so no order of summation;
  * ``osc_np``: the vectorised form, held to the first by tests/test_osc.py;
  * ``MISTAKES``: planted mistakes ``osc_scalar(.., mistake=name)`` commits on purpose; each must break the
    comparison on the committed cases (tests/test_osc.py);
  * ``generated``: seeded damped, undamped and growing sinusoids around a stepped reference, with samples
    exactly on the band edges; ``edge_rows``: hand-placed rows for the order-dependent paths of the kernel.
"""
import math

import numpy as np

from indices_ref import bits

Y_FIELDS = ("ncross", "decay", "period", "a_last")
U_FIELDS = ("nmove", "nrev", "t_rev")
FIELDS = Y_FIELDS + U_FIELDS          # their positions are the MPCT_OX_* ids
INT_FIELDS = ("ncross", "period", "nmove", "nrev", "t_rev")
NAN = float("nan")
MISTAKES = ("edge_is_outside", "inside_resets_state", "k0_ignored", "last_attaining_peak", "boundary_move_earlier",
            "x_against_r_t")


def _invalid(fields):
    return {f: (-1 if f in INT_FIELDS else NAN) for f in fields}


def _state(x, h, mistake=None):
    if mistake == "edge_is_outside":
        return 1 if x >= h else (-1 if x <= -h else 0)
    return 1 if x > h else (-1 if x < -h else 0)


def output_unit(y, r, a, b, first, base, band_rel, band_abs, mistake=None):
    """one (output row, segment): the samples a <= t < b; ``first``: segment 0"""
    use_r = base == 1 and not first
    read = [float(y[t]) for t in range(a, b)] + [float(r[b - 1])] + ([float(r[a - 1])] if use_r else [])
    if not all(math.isfinite(v) for v in read):
        return _invalid(Y_FIELDS)
    rg = float(r[b - 1])
    c = float(r[a - 1]) if use_r else float(y[a])
    d = rg - c
    prod = band_rel * abs(d)               # rounded, then added
    h = prod + band_abs
    k0 = 1 if (d != 0 and mistake != "k0_ignored") else 0
    prev, ncross = 0, 0
    A, T = [], []                          # peak and first attaining sample of each lobe
    for t in range(a, b):
        x = float(y[t]) - (float(r[t]) if mistake == "x_against_r_t" else rg)
        st = _state(x, h, mistake)
        if st == 0:
            if mistake == "inside_resets_state":
                prev = 0
            continue
        if prev != 0 and st != prev:
            ncross += 1
        if len(A) <= ncross:
            A.append(-1.0)
            T.append(-1)
        ax = abs(x)
        if ax > A[ncross] or (mistake == "last_attaining_peak" and ax == A[ncross]):
            A[ncross], T[ncross] = ax, t
        prev = st
    two = ncross >= k0 + 2
    return {"ncross": ncross, "decay": A[k0 + 2] / A[k0] if two else 0.0, "period": T[k0 + 2] - T[k0] if two else -1,
            "a_last": A[ncross] if (A and ncross >= k0) else 0.0}


def input_unit(u, a, b, first, rev_tol, mistake=None):
    """one (input row, segment): the moves du(t), t in [max(a, tseg[0] + 1), b)"""
    lo_t, hi_t = (a + 1 if first else a), b
    if mistake == "boundary_move_earlier":   # the move across the boundary b counted here, not in the next one
        lo_t, hi_t = a + 1, min(b + 1, len(u))
    read = [float(u[t]) for t in range(a, b)] + ([] if first else [float(u[a - 1])])
    if not all(math.isfinite(v) for v in read):
        return _invalid(U_FIELDS)
    prev, nmove, nrev, t_rev = 0, 0, 0, -1
    for t in range(lo_t, hi_t):
        du = float(u[t]) - float(u[t - 1])
        st = _state(du, rev_tol)
        if st == 0:
            continue
        nmove += 1
        if prev != 0 and st != prev:
            nrev += 1
            t_rev = t
        prev = st
    return {"nmove": nmove, "nrev": nrev, "t_rev": t_rev}


def _empty(S, my, nu, nseg):
    out = {f: np.zeros((S, my, nseg), dtype=np.int32 if f in INT_FIELDS else np.float64) for f in Y_FIELDS}
    out.update({f: np.zeros((S, nu, nseg), dtype=np.int32) for f in U_FIELDS})
    return out


def osc_scalar(y, u, r, tseg, base=1, band_rel=0.02, band_abs=0.0, rev_tol=0.0, mistake=None):
    """y [S, my, nit], u [S, nu, nit], r [nref, my, nit] -> dict of [S, my, nseg] / [S, nu, nseg] arrays"""
    S, my = y.shape[:2]
    nu, nref, nseg = u.shape[1], r.shape[0], len(tseg) - 1
    out = _empty(S, my, nu, nseg)
    for g in range(nseg):
        a, b = int(tseg[g]), int(tseg[g + 1])
        for s in range(S):
            for i in range(my):
                for f, x in output_unit(y[s, i], r[s % nref, i], a, b, g == 0, base, band_rel, band_abs, mistake).items():
                    out[f][s, i, g] = x
            for j in range(nu):
                for f, x in input_unit(u[s, j], a, b, g == 0, rev_tol, mistake).items():
                    out[f][s, j, g] = x
    return out


def _order(st):
    """st [..., n] in {-1, 0, +1} -> (crossing mask, lobe index per sample): the walk over the outside samples"""
    n = st.shape[-1]
    idx = np.where(st != 0, np.arange(n), -1)
    last = np.maximum.accumulate(idx, axis=-1)                      # the last outside sample at or before t
    before = np.concatenate([np.full(st.shape[:-1] + (1,), -1), last[..., :-1]], -1)
    prev = np.where(before >= 0, np.take_along_axis(st, np.maximum(before, 0), -1), 0)
    cross = (st != 0) & (prev != 0) & (prev != st)
    return cross, np.cumsum(cross, -1)


def _peak(ax, sel, a):
    """the largest ax over sel [..., n] and the first sample attaining it; (-1.0, -1) where sel is empty"""
    v = np.where(sel, ax, -1.0)
    return v.max(-1), np.where(sel.any(-1), a + v.argmax(-1), -1)


def osc_np(y, u, r, tseg, base=1, band_rel=0.02, band_abs=0.0, rev_tol=0.0):
    """the vectorised form of osc_scalar"""
    y, u, r = (np.asarray(x, dtype=np.float64) for x in (y, u, r))
    S, my, nit = y.shape
    nu, nref, nseg = u.shape[1], r.shape[0], len(tseg) - 1
    out = _empty(S, my, nu, nseg)
    rr = r[np.arange(S) % nref] if my else np.zeros((S, 0, nit))
    with np.errstate(all="ignore"):
        for g in range(nseg):
            a, b = int(tseg[g]), int(tseg[g + 1])
            ys = y[..., a:b]
            use_r = base == 1 and g > 0
            c = rr[..., a - 1] if use_r else y[..., a]
            rg = rr[..., b - 1]
            valid = np.isfinite(ys).all(-1) & np.isfinite(c) & np.isfinite(rg)
            d = rg - c
            h = (band_rel * np.abs(d) + band_abs)[..., None]
            x = np.where(valid[..., None], ys - rg[..., None], 0.0)
            ax = np.abs(x)
            st = np.where(x > h, 1, np.where(x < -h, -1, 0))
            cross, lobe = _order(st)
            ncross = cross.sum(-1)
            k0 = np.where(d != 0, 1, 0)[..., None]
            outside = st != 0
            A0, T0 = _peak(ax, outside & (lobe == k0), a)
            A2, T2 = _peak(ax, outside & (lobe == k0 + 2), a)
            AL, _ = _peak(ax, outside & (lobe == ncross[..., None]), a)
            two = ncross >= k0[..., 0] + 2
            o = {"ncross": ncross, "decay": np.where(two, A2 / np.where(two, A0, 1.0), 0.0),
                 "period": np.where(two, T2 - T0, -1),
                 "a_last": np.where((ncross >= k0[..., 0]) & outside.any(-1), AL, 0.0)}
            for f in Y_FIELDS:
                out[f][..., g] = np.where(valid, o[f], -1 if f in INT_FIELDS else np.nan)
            us = u[..., a:b]
            prev = u[..., a - 1:a] if g > 0 else us[..., :1]
            uval = np.isfinite(us).all(-1) & (np.isfinite(prev[..., 0]) if g > 0 else True)
            du = np.where(uval[..., None], us - np.concatenate([prev, us[..., :-1]], -1), 0.0)
            st = np.where(du > rev_tol, 1, np.where(du < -rev_tol, -1, 0))
            if g == 0:
                st[..., 0] = 0                                      # no move into the first sample
            cross, _ = _order(st)
            n = b - a
            o = {"nmove": (st != 0).sum(-1), "nrev": cross.sum(-1),
                 "t_rev": np.where(cross.any(-1), a + n - 1 - cross[..., ::-1].argmax(-1), -1)}
            for f in U_FIELDS:
                out[f][..., g] = np.where(uval, o[f], -1)
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


H = 0.125          # the band of the committed cases: band_rel = 0, band_abs = 1/8, exact in binary
TOL = 0.125        # their dead zone of a move


def generated(S, nref, my, nu, nit, tseg, seed=0):
    """Trajectories y [S, my, nit], u [S, nu, nit] and references r [nref, my, nit] (piecewise constant, changing at
    the boundaries tseg[1:-1]) for the band H and the dead zone TOL, per segment [a, b):

    * the outputs are sinusoids around the segment's level, amplitude * rho^k * cos(w k + phase) with rho < 1
      (damped: rows with (s + i) % 3 == 0), rho = 1 (undamped) and rho > 1 (growing: a_last > A_k0), starting
      from the level before; even rows (s * my + i) are quantised to 1/32, so equal peaks occur and the first
      must win, odd rows keep full precision (a decay ratio that rounds);
    * channel 0 of every even simulation has samples exactly on +H and -H (at b - 3, b - 2 where the segment is
      long enough; in simulation 0, damped, the response has died by then): inside;
    * the last reference set's channel 1 ramps inside each segment, so that r(t) differs from r_g = r(b-1);
    * channel 2, where present, has a reference that never moves (sigma = 0 under base = 1: k0 = 0) and
      carries -0.0 samples;
    * inputs: even rows (s + j) a walk on the grid of TOL / 2 whose moves are -TOL, -TOL/2, 0, TOL/2, TOL, 2 TOL
      (moves of exactly +-TOL are inside), odd rows full precision; channel 1 of simulation 0 is +-0.0 throughout.

    NaN and infinities are planted by the tests, which know which unit they spoil."""
    rng = np.random.default_rng(seed)
    nseg = len(tseg) - 1
    t = np.arange(nit)
    r = np.zeros((nref, my, nit))
    for k in range(nref):
        for i in range(my):
            for g in range(nseg):
                level = (g % 2) * (1.0 + 0.5 * k) if i == 0 else (float((-1) ** g) * (1 + k) if i == 1 else 0.0)
                r[k, i, int(tseg[g]):] = level
                if i == 1 and k == nref - 1:
                    a, b = int(tseg[g]), int(tseg[g + 1])
                    r[k, i, a:b] = level + (np.arange(b - a) - (b - a - 1)) / 64.0
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
                rho = (0.93, 1.0, 1.02)[(s + i) % 3]
                amp = (lvl - target) if lvl != target else 0.75
                w = 2.0 * np.pi / (5.0 + 2.0 * ((s + g) % 4))
                row[a:b] = target + amp * rho ** k * np.cos(w * k) + 0.01 * rng.standard_normal(b - a)
                lvl = target
            if (s * my + i) % 2 == 0:
                row = np.round(32.0 * row) / 32.0
            if i == 2:
                row = np.where(t % 7 == 0, -0.0, row)
            if i == 0 and s % 2 == 0:
                for g in range(nseg):
                    a, b = int(tseg[g]), int(tseg[g + 1])
                    if b - a >= 4:
                        row[b - 3] = rr[b - 1] + H
                        row[b - 2] = rr[b - 1] - H
            y[s, i] = row
        for j in range(nu):
            if (s + j) % 2 == 0:
                moves = rng.choice(np.array([-TOL, -TOL / 2, 0.0, TOL / 2, TOL, 2 * TOL, -2 * TOL]), size=nit)
                row = np.cumsum(moves)
            else:
                row = np.cumsum(0.2 * rng.standard_normal(nit))
            if s == 0 and j == 1:
                row = np.where(t % 2 == 0, -0.0, 0.0)
            u[s, j] = row
    return y, u, r


# the hand-placed rows of edge_rows, by name, in row order
EDGE_ROWS = ("crossing between lane 63 and lane 0", "inside gap longer than 64 samples", "peak of lobe k0+2 tied across two blocks",
             "ncross exactly k0+1", "ncross exactly k0+2", "never leaves the band", "sigma = 0 disturbance",
             "growing oscillation")


def edge_rows(nit=330, a=1, b=326):
    """One simulation of len(EDGE_ROWS) output channels over one segment [a, b) (tseg = [a, b], so c = y(a)) with a
    reference of 0 throughout, band H, and as many input channels whose moves carry the same patterns around
    the dead zone TOL; the kernel's lane of sample t is (t - a) mod 64.  Returns y [1, m, nit], u [1, m, nit],
    r [1, m, nit], tseg."""
    m = len(EDGE_ROWS)
    y = np.zeros((1, m, nit))
    # every row but two starts at y(a) = -1: d = 1, sigma != 0, k0 = 1; lobe 0 is the approach from below
    y[0, :, a] = -1.0
    lane0 = lambda blk: a + 64 * blk                                        # noqa: E731
    # 0: + at lane 63 of block 0 is the first crossing, - at lane 0 of block 1 the second
    y[0, 0, lane0(0) + 63], y[0, 0, lane0(1)] = 0.5, -0.5
    # 1: + then nothing outside for more than a whole block (blocks 1 and 2 are empty), then -
    y[0, 1, lane0(0) + 5], y[0, 1, lane0(3) + 2] = 0.5, -0.25
    # 2: lobes +(k0), -, +(k0+2) with the third lobe's peak 0.375 in block 1 (lane 60) and again in block 2 (lane 3)
    y[0, 2, a + 3], y[0, 2, a + 9] = 0.75, -0.5
    y[0, 2, lane0(1) + 59: lane0(2) + 5] = 0.25
    y[0, 2, lane0(1) + 60], y[0, 2, lane0(2) + 3] = 0.375, 0.375
    # 3: ncross = 2 = k0 + 1: no second peak on the side of lobe k0
    y[0, 3, a + 3], y[0, 3, a + 70] = 0.5, -0.25
    # 4: ncross = 3 = k0 + 2
    y[0, 4, a + 3], y[0, 4, a + 70], y[0, 4, a + 140] = 0.5, -0.25, 0.1875
    # 5: never leaves the band: y(a) = 0, so d = 0 and k0 = 0; samples exactly on the edges are inside
    y[0, 5, a] = 0.0
    y[0, 5, a + 10], y[0, 5, a + 11], y[0, 5, a + 100] = H, -H, -0.0
    # 6: sigma = 0 (y(a) = 0): lobe 0 is the first excursion; + - + with peaks 0.5, 0.375, 0.25
    y[0, 6, a] = 0.0
    y[0, 6, a + 20], y[0, 6, a + 90], y[0, 6, a + 200] = 0.5, -0.375, 0.25
    # 7: a growing oscillation: the last lobe's peak exceeds A_k0
    for k, t in enumerate(range(a + 4, b, 37)):
        y[0, 7, t] = (-1.0) ** k * (0.25 + 0.125 * k)
    r = np.zeros((1, m, nit))
    # the inputs: u is the running sum of moves that are the outputs' excursions scaled to the dead zone
    du = np.where(np.abs(y[0]) > H, y[0], 0.0)
    du[:, a] = 0.0
    du[5, a + 10], du[5, a + 11] = TOL, -TOL                                # moves exactly on the dead zone: none
    u = np.cumsum(du, -1)[None]
    return y, u, r, [a, b]
