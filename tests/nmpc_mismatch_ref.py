"""Numpy reference of the Van de Vusse NMPC closed loop whose simulated plant is not the controller's
model (closedloop_toolbox_nmpc.m: `model` integrated at :71 and :91, the controller fed the measured
state at :69).  Test infrastructure for test_nmpc_variants.py / test_nmpc_variants_gpu.py.

The controller is oracle.nmpc_vdv.controller, unchanged: its module constants are the nominal model.
The plant is this file's own RK4 step on a variant's 16 parameters (mpct_nmpc_desc.params order), in
the closed loop and in the open-loop leg.  Nothing here knows of the device's speculation or of its
variant table: one plant, one loop."""
from dataclasses import dataclass

import numpy as np

import oracle.nmpc_vdv as nv

MODEL = np.array([nv.K10, nv.K20, nv.K30, nv.E1, nv.E2, nv.E3, nv.DHAB, nv.DHBC, nv.DHAD, nv.RHO, nv.CP, nv.KW,
                  nv.AR, nv.VR, nv.T0, nv.CA0])


def plant_rhs(x, u, p):
    """vandevusse_model.m on the parameters p (the arithmetic of oracle.nmpc_vdv.rhs, term by term)."""
    k10, k20, k30, e1, e2, e3, dab, dbc, dad, rho, cp, kw, ar, vr, t0, ca0 = p
    ca, cb, T = x
    fov, tk = u
    k1 = k10 * np.exp(e1 / (T + 273.15))
    k2 = k20 * np.exp(e2 / (T + 273.15))
    k3 = k30 * np.exp(e3 / (T + 273.15))
    return np.array([
        fov * (ca0 - ca) - k1 * ca - k3 * ca * ca,
        -fov * cb + k1 * ca - k2 * cb,
        (1.0 / (rho * cp)) * (k1 * ca * dab + k2 * cb * dbc + k3 * ca * ca * dad)
        + fov * (t0 - T) + (kw * ar / (rho * cp * vr)) * (tk - T),
    ])


def plant_rk4(x, u, p):
    """One Ts of the plant: classical RK4, nv.NSUB sub-steps."""
    h = nv.TS / nv.NSUB
    x = np.array(x, dtype=float)
    for _ in range(nv.NSUB):
        k1 = plant_rhs(x, u, p)
        k2 = plant_rhs(x + 0.5 * h * k1, u, p)
        k3 = plant_rhs(x + 0.5 * h * k2, u, p)
        k4 = plant_rhs(x + h * k3, u, p)
        x = x + (h / 6.0) * (k1 + 2 * k2 + 2 * k3 + k4)
    return x


@dataclass
class MismatchResult:
    y: np.ndarray
    u: np.ndarray
    yopt: np.ndarray
    uopt: np.ndarray
    x: np.ndarray       # 3 x nit plant states
    sqp_iters: int
    max_iters: int      # the most Gauss-Newton iterations any controller call took
    bounds_ok: bool


def closedloop_mismatch(r, N, Nu, delta, lam, params, x0, nit=nv.NIT, u0=nv.U0, open_loop=True,
                        xbounds=(nv.XMIN, nv.XMAX)):
    """closedloop_toolbox_nmpc with the plant `params` started at x0 (the variant's start state; the
    open-loop controller call starts there too)."""
    params = np.asarray(params, dtype=float)
    x0 = np.asarray(x0, dtype=float)
    u0 = np.asarray(u0, dtype=float)
    r = np.asarray(r, dtype=float).reshape(nv.NY, nit)
    X = np.zeros((3, nit))
    U = np.zeros((2, nit))
    X[:, 0] = x0
    U[:, 0] = u0
    Uw = np.tile(u0, (Nu, 1))
    iters = mx = 0
    for i in range(1, nit):
        Uw, it = nv.controller(X[:, i - 1], U[:, i - 1], r[:, i], N, Nu, delta, lam, Uw, xbounds, False)
        iters += it
        mx = max(mx, it)
        U[:, i] = Uw[0]
        X[:, i] = plant_rk4(X[:, i - 1], U[:, i], params)
        Uw = np.vstack([Uw[1:], Uw[-1:]])
    xmn, xmx = (np.asarray(b, dtype=float) for b in xbounds)
    ok = bool(np.all(X >= xmn[:, None] - 1e-9) and np.all(X <= xmx[:, None] + 1e-9))
    yopt = uopt = None
    if open_loop:
        Uo, it = nv.controller(x0, u0, r[:, -1], N, Nu, delta, lam, np.tile(u0, (Nu, 1)), xbounds, False)
        iters += it
        mx = max(mx, it)
        uopt = np.array([Uo[min(k, Nu - 1)] for k in range(nit)]).T.copy()
        Xo = np.zeros((3, nit))
        Xo[:, 0] = x0
        for i in range(1, nit):
            Xo[:, i] = plant_rk4(Xo[:, i - 1], uopt[:, i], params)
        yopt = Xo[1:].copy()
    return MismatchResult(X[1:].copy(), U, yopt, uopt, X, iters, mx, ok)


def costs(res, yref, ink0=9):
    """J1, j22, j21, Jnu of a loop, as the kernel defines them (tests/test_nmpc.py)."""
    e = res.y - yref
    out = dict(J1=(e ** 2).sum(1), j22=(e[:, ink0:] ** 2).sum(1))
    if res.yopt is not None:
        out["j21"] = ((res.y - res.yopt)[:, ink0:] ** 2).sum(1)
        du = np.abs(np.diff(res.uopt, axis=1))
        with np.errstate(divide="ignore", invalid="ignore"):
            xr = np.abs(res.uopt[:, :1]) / du
        xr[~np.isfinite(xr)] = 0.0
        out["Jnu"] = (xr ** 2).sum(1)
    return out


def scaled(params, k=(1.0, 1.0, 1.0), h=(1.0, 1.0, 1.0)):
    """params with k10, k20, k30 times k and dHab, dHbc, dHad times h."""
    p = np.array(params, dtype=float)
    p[0:3] *= np.asarray(k, dtype=float)
    p[6:9] *= np.asarray(h, dtype=float)
    return p
