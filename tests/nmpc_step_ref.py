"""Truth for nmpc_kernel.hip one Gauss-Newton step at a time (tests/test_nmpc_units.py on the CPU,
tests/test_nmpc_units_gpu.py on the device).  Every parameter is explicit (oracle/nmpc_vdv.py reads
module globals); `p` is the 16-entry parameter row in mpct.nmpc.VDV_PARAMS order.

  rhs, rk4       the Van de Vusse state derivative and the classical RK4 map of nmpc_model.h with
                 their exact directional derivatives, in mpmath (`MP`, 40 digits) or float64
  gn_step        one Gauss-Newton step of one controller call as oracle/nmpc_vdv.py controller states
                 it: residual rows w_y (y - r) and w_u du in the absolute moves, the box on the moves,
                 optional linearised state rows.  The active set comes from the float64 oracle's
                 solvers (scipy BVLS, oracle.toolbox_band.qp_dual_dense); the equality-constrained
                 least squares is solved in mpmath and CERTIFIED by its KKT conditions (every
                 inactive row feasible by more than KKT_MARGIN of its scale, every multiplier above
                 KKT_MARGIN of the largest gradient entry).  Then the convergence test, the Anderson
                 candidate test and the Armijo decision, each with its margin from a tie relative
                 to f0 (the convergence test: relative to sqp_tol)
  call_chain     a closed loop of such calls (plant step, warm-start shift, that step's reference,
                 a plant that may differ from the model) and the open-loop call
  f64_chain      the float64 restatement of the device's algorithm on the truth's active sets:
                 increments as variables, per-column forward tangents through the RK4 stages, the
                 streamed row-wise Givens QR of [rate rows; output rows | residual], the packed
                 triangular inverse, the step s = s_u + J J'C'mu on the active rows (what
                 Goldfarb-Idnani ends with), its own Armijo / Anderson decisions.  `mutate` plants
                 one error: ("tangent", row, col) scales one streamed tangent entry by 1 + 1e-6,
                 ("rotation", row, col) drops one Givens rotation

Bounds.  The measure is max |move - move_truth| / u_scale over the compared moves.  No bound is
derived (cond(R) differs per case and the v_rsq_f64 rotations have no published bound): per case
family the float64 restatement's own measure against the truth is taken on the CPU and the device
gets 8 x the family's largest value (FMA contraction, the summation order of the lane-parallel
solves, the two-Newton-step reciprocal square root); both planted errors move every case's step by
more than 100 x its family's bound (tests/test_nmpc_units.py).  Never tuned from device output.
Measured by tests/make_nmpc_step_fixture.py (stored in tests/golden/nmpc_step_truth.npz, which
tests/test_nmpc_units.py holds to this table):

BOUND_TABLE_BEGIN
family   restatement   device bound   planted / bound
a        2.58e-16      2.07e-15       9.74e+04
along    5.17e-16      4.13e-15       5.21e+03
b        3.88e-16      3.1e-15        2.88e+05
c        9.04e-16      7.23e-15       4.69e+03
d        1.42e-15      1.14e-14       2.6e+04
dlong    5.17e-16      4.13e-15       5.21e+03
e        1.16e-15      9.3e-15        9.43e+03
BOUND_TABLE_END

The probe of nmpc_model.h (probe_reference: per case the largest error over the largest entry, value and
tangents apart, the restatement against the truth over the probe's own cases; the device gets 8 x):

PROBE_TABLE_BEGIN
probe     restatement value   bound     restatement tangent   bound
rhs-own   7.55e-16            6.04e-15  1.78e-18              1.42e-17
rhs-xd    7.55e-16            6.04e-15  2.1e-16               1.68e-15
rk4-own   8.63e-14            6.9e-13   7.97e-14              6.38e-13
rk4-xd    8.63e-14            6.9e-13   7.41e-14              5.93e-13
PROBE_TABLE_END
"""
from __future__ import annotations

import math
import os

import mpmath
import numpy as np

MP = mpmath.mp.clone()
MP.dps = 40
mpf = MP.mpf

LS_MAX, LS_C1, LS_FLAT = 12, 1e-4, 1e-14      # oracle/nmpc_vdv.py, nmpc_model.h
KKT_MARGIN = 1e-9
TIE_MARGIN = 1e-6      # every Armijo / Anderson decision of a valid case is further than this from a tie
CONV_MARGIN = 1e-2     # |max|d|/s_u / sqp_tol - 1| of every convergence test
DEVICE_FACTOR = 8.0
MUTATION_FACTOR = 100.0
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "nmpc_step_truth.npz")

VDV_PARAMS = (1.287e12, 1.287e12, 9.043e9, -9758.3, -9758.3, -8560.0, -4.20, 11.00, 41.85,
              0.9342, 3.01, 4032.0, 0.215, 10.0, 130.00, 5.10)
U0 = (20.0, 130.0)
UMIN, UMAX = (0.0, 40.0), (150.0, 150.0)
XMIN, XMAX = (0.0, 0.0, 40.0), (6.0, 1.2, 150.0)
SU = (150.0, 110.0)
TS = 0.05
INF = float("inf")


# ------------------------------------------------------------------------------------------------
# the model: scalar code, generic over mpmath and float

def _exp(z):
    # MP is a clone of mpmath.mp with an mpf class of its own: dispatch on float, never on mpmath.mpf
    return math.exp(z) if isinstance(z, float) else MP.exp(z)


def _num(mp):
    return (lambda v: mpf(float(v))) if mp else float


def rhs(p, x, u, xd=None, ud=None):
    """f(x, u) (nmpc_vandevusse_state.m:64-82); with (xd, ud) also its directional derivative."""
    k10, k20, k30, e1, e2, e3, dab, dbc, dad, rho, cp, kw, ar, vr, t0, ca0 = p
    ca, cb, T = x
    fov, tk = u
    th = T + 273.15      # the double 273.15 in both arithmetics: the kernel's constant
    k1, k2, k3 = k10 * _exp(e1 / th), k20 * _exp(e2 / th), k30 * _exp(e3 / th)
    a, b = 1 / (rho * cp), kw * ar / (rho * cp * vr)
    f = [fov * (ca0 - ca) - k1 * ca - k3 * ca * ca,
         -fov * cb + k1 * ca - k2 * cb,
         a * (k1 * ca * dab + k2 * cb * dbc + k3 * ca * ca * dad) + fov * (t0 - T) + b * (tk - T)]
    if xd is None:
        return f
    cad, cbd, Td = xd
    k1d, k2d, k3d = -e1 / th ** 2 * k1 * Td, -e2 / th ** 2 * k2 * Td, -e3 / th ** 2 * k3 * Td
    fd = [ud[0] * (ca0 - ca) - fov * cad - k1d * ca - k1 * cad - k3d * ca * ca - 2 * k3 * ca * cad,
          -ud[0] * cb - fov * cbd + k1d * ca + k1 * cad - k2d * cb - k2 * cbd,
          a * (k1d * ca * dab + k1 * cad * dab + k2d * cb * dbc + k2 * cbd * dbc + k3d * ca * ca * dad
               + 2 * k3 * ca * cad * dad) + ud[0] * (t0 - T) - fov * Td + b * (ud[1] - Td)]
    return f, fd


def rk4(p, ts, nsub, x, u, xd=None, ud=None):
    """One sample ts of classical RK4 with nsub sub-steps (nmpc_model.h vdv_rk4).  xd: a list of
    tangent 3-vectors with their input tangents ud (2-vectors); returns x, or (x, tangents)."""
    h = ts / nsub
    x = list(x)
    tan = xd is not None
    X = [list(t) for t in xd] if tan else []
    for _ in range(nsub):
        ks, Ks = [], [[] for _ in X]
        for c in (None, 0.5, 0.5, 1.0):
            xs = x if c is None else [x[i] + c * h * ks[-1][i] for i in range(3)]
            Xs = X if c is None else [[X[k][i] + c * h * Ks[k][-1][i] for i in range(3)] for k in range(len(X))]
            if tan and X:
                fs = None
                for k in range(len(X)):
                    fs, fd = rhs(p, xs, u, Xs[k], ud[k])
                    Ks[k].append(fd)
                ks.append(fs)
            else:
                ks.append(rhs(p, xs, u))
        x = [x[i] + (h / 6) * (ks[0][i] + 2 * ks[1][i] + 2 * ks[2][i] + ks[3][i]) for i in range(3)]
        X = [[X[k][i] + (h / 6) * (Ks[k][0][i] + 2 * Ks[k][1][i] + 2 * Ks[k][2][i] + Ks[k][3][i]) for i in range(3)]
             for k in range(len(X))]
    return (x, X) if tan else x


def steady_state(p=VDV_PARAMS, u=U0, x=(5.1, 1.1163, 130.0)):
    """Newton on rhs(x, u) = 0 in float64 (VanDeVusse_NMPC.m:78)."""
    x = np.array(x, float)
    for _ in range(50):
        f = np.array(rhs(p, list(x), u))
        J = np.array([rhs(p, list(x), u, list(e), [0.0, 0.0])[1] for e in np.eye(3)]).T
        dx = np.linalg.solve(J, -f)
        x = x + dx
        if np.max(np.abs(dx) / np.maximum(1.0, np.abs(x))) < 1e-15:
            break
    return x


# ------------------------------------------------------------------------------------------------
# one controller problem

class Prob:
    """What one controller call depends on besides (x, u_last, r, warm start).  xc is 1-based."""

    def __init__(self, N, Nu, delta, lam, xc=(2, 3), params=VDV_PARAMS, ts=TS, nsub=2, u_min=UMIN, u_max=UMAX,
                 x_min=XMIN, x_max=XMAX, y_scale=None, u_scale=SU, sqp_tol=1e-8, sqp_max=1, plant=None):
        self.N, self.Nu, self.M = int(N), int(Nu), 2 * int(Nu)
        self.xc = [int(c) - 1 for c in xc]
        self.ny = len(self.xc)
        self.params, self.ts, self.nsub = tuple(float(v) for v in params), float(ts), int(nsub)
        self.plant = self.params if plant is None else tuple(float(v) for v in plant)
        ys = [XMAX[c] - XMIN[c] for c in self.xc] if y_scale is None else list(y_scale)
        self.delta, self.lam = [float(v) for v in delta], [float(v) for v in lam]
        self.wy = [abs(d) / s for d, s in zip(self.delta, ys)]
        self.wu = [abs(l) / s for l, s in zip(self.lam, u_scale)]
        self.y_scale, self.su = [float(v) for v in ys], [float(v) for v in u_scale]
        self.lb, self.ub = [float(v) for v in u_min], [float(v) for v in u_max]
        self.xmin, self.xmax = [float(v) for v in x_min], [float(v) for v in x_max]
        self.sqp_tol, self.sqp_max = float(sqp_tol), int(sqp_max)

    def has_xb(self):
        return any(math.isfinite(v) for v in self.xmin + self.xmax)


def _predict(P, x, U, mp, sens):
    """States x(k+1..k+N) for the absolute moves U [Nu][2] (held after Nu - 1) and, with sens,
    dx_i/dU (N x 3 x M, column n Nu + l) chained from the RK4 map's Jacobians [Fx | Fu]."""
    n_ = _num(mp)
    p = [n_(v) for v in P.params]
    one, zero = n_(1.0), n_(0.0)
    x = list(x)
    XP, SX = [], []
    S = [[zero] * P.M for _ in range(3)]
    seeds_x = [[one if i == k else zero for i in range(3)] for k in range(3)] + [[zero] * 3] * 2
    seeds_u = [[zero, zero]] * 3 + [[one, zero], [zero, one]]
    for i in range(P.N):
        li = min(i, P.Nu - 1)
        u = U[li]
        if sens:
            x, F = rk4(p, n_(P.ts), P.nsub, x, u, seeds_x, seeds_u)
            Sn = [[sum(F[k][a] * S[k][m] for k in range(3)) for m in range(P.M)] for a in range(3)]
            for n in range(2):
                for a in range(3):
                    Sn[a][n * P.Nu + li] += F[3 + n][a]
            S = Sn
            SX.append(S)
        else:
            x = rk4(p, n_(P.ts), P.nsub, x, u)
        XP.append(x)
    return XP, SX


def _cost(P, x, U, ul, r, mp):
    n_ = _num(mp)
    XP, _ = _predict(P, x, U, mp, False)
    f = n_(0.0)
    for xs in XP:
        for j in range(P.ny):
            f += (n_(P.wy[j]) * (xs[P.xc[j]] - r[j])) ** 2
    for n in range(2):
        for l in range(P.Nu):
            f += (n_(P.wu[n]) * (U[l][n] - (U[l - 1][n] if l else ul[n]))) ** 2
    inb = all(n_(P.xmin[s]) <= xs[s] <= n_(P.xmax[s]) for xs in XP for s in range(3))
    return f / 2, inb


def _armijo_gap(f1, f0, alpha, dd):
    """>= 0: the trial is accepted (either comparison of the oracle's test holds)."""
    return max(f0 + LS_C1 * alpha * dd - f1, LS_FLAT * f0 - (f1 - f0)) / f0


def _constraints(P, v, XP, SX, n_):
    """Rows C d >= b of the step d in the absolute moves: the box, then the finite state rows in
    the kernel's order (row i, state s, min before max).  Returns (C, b, scale, tag)."""
    M = P.M
    C, b, sc, tag = [], [], [], []
    zero, one = n_(0.0), n_(1.0)
    for sg in (1, -1):
        for m in range(M):
            n = m // P.Nu
            C.append([one * sg if k == m else zero for k in range(M)])
            b.append(min(n_(P.lb[n]) - v[m], zero) if sg > 0 else -max(n_(P.ub[n]) - v[m], zero))
            sc.append(P.su[n])
            tag.append(("lo" if sg > 0 else "hi", m))
    for i in range(P.N):
        for s in range(3):
            if math.isfinite(P.xmin[s]):
                C.append(list(SX[i][s]))
                b.append(n_(P.xmin[s]) - XP[i][s])
                sc.append(XMAX[s] - XMIN[s])
                tag.append(("xmin", i, s))
            if math.isfinite(P.xmax[s]):
                C.append([-t for t in SX[i][s]])
                b.append(XP[i][s] - n_(P.xmax[s]))
                sc.append(XMAX[s] - XMIN[s])
                tag.append(("xmax", i, s))
    return C, b, sc, tag


def _linearise(P, x, ul, r, U, mp):
    n_ = _num(mp)
    XP, SX = _predict(P, x, U, mp, True)
    A, res = [], []
    for i in range(P.N):
        for j in range(P.ny):
            if P.wy[j] > 0.0:
                w = n_(P.wy[j])
                A.append([w * t for t in SX[i][P.xc[j]]])
                res.append(w * (XP[i][P.xc[j]] - r[j]))
    zero = n_(0.0)
    for n in range(2):
        for l in range(P.Nu):
            m = n * P.Nu + l
            w = n_(P.wu[n])
            row = [zero] * P.M
            row[m] = w
            if l:
                row[m - 1] = -w
            A.append(row)
            res.append(w * (U[l][n] - (U[l - 1][n] if l else ul[n])))
    return XP, SX, A, res


def oracle_active_set(A, res, C, b, sc, nbox):
    """The float64 oracle's solution of the step QP and the rows active at it, with the number of
    rows Goldfarb-Idnani drops on the way (most-violated selection, as the kernel's)."""
    from scipy.optimize import lsq_linear

    from oracle.toolbox_band import qp_dual_dense

    A, C = (np.array([[float(t) for t in row] for row in a]) for a in (A, C))
    res, b = (np.array([float(t) for t in a]) for a in (res, b))
    M = A.shape[1]
    d = lsq_linear(A, -res, bounds=(b[:M], -b[M:2 * M]), method="bvls", tol=1e-14, lsmr_tol=None).x
    drops = 0
    if C.shape[0] > nbox and np.min(C[nbox:] @ d - b[nbox:]) < -1e-10 * max(1.0, float(np.max(np.abs(b[nbox:])))):
        d, it, act = qp_dual_dense(A, res, C, b, qr=True)
        drops = (it - len(act)) // 2
    s = (C @ d - b) / np.asarray(sc)
    return d, [int(k) for k in np.flatnonzero(s <= 1e-9)], drops


def gn_step(P, x, ul, r, U, hist=None):
    """One Gauss-Newton step in mpmath.  x, ul, r, U [Nu][2]: mpf.  hist: the previous iteration's
    (d, G(v)) for the Anderson candidate.  Returns a record:
      U          the next iterate (the iterate itself when converged)
      converged  max |d| / s_u <= sqp_tol
      d, active, tags, drops, slack, mult      the certified step and its certificate
      margins    [(name, margin)]: every decision's distance from a tie
      took       "converged" | "anderson" | "armijo<k halvings>"
    """
    M, Nu = P.M, P.Nu
    XP, SX, A, res = _linearise(P, x, ul, r, U, True)
    v = [U[m % Nu][m // Nu] for m in range(M)]
    C, b, sc, tag = _constraints(P, v, XP, SX, mpf)
    _, act, drops = oracle_active_set(A, res, C, b, sc, 2 * M)
    Am = MP.matrix(A)
    H = Am.T * Am
    g = Am.T * MP.matrix(res)
    na = len(act)
    K = MP.zeros(M + na, M + na)
    rh = MP.zeros(M + na, 1)
    for i in range(M):
        for k in range(M):
            K[i, k] = H[i, k]
        rh[i] = -g[i]
    for a_, q in enumerate(act):
        for k in range(M):
            K[M + a_, k] = C[q][k]
            K[k, M + a_] = -C[q][k]
        rh[M + a_] = b[q]
    sol = MP.lu_solve(K, rh)
    d = [sol[i] for i in range(M)]
    mu = [sol[M + a_] for a_ in range(na)]
    gmax = max([abs(t) for t in g] + [mpf(1e-300)])
    slack = min([(sum(C[q][k] * d[k] for k in range(M)) - b[q]) / sc[q]
                 for q in range(len(C)) if q not in act] + [mpf(INF)])
    mult = min([m_ / gmax for m_ in mu] + [mpf(INF)])
    rec = dict(d=d, active=[tag[q] for q in act], drops=drops, slack=float(slack), mult=float(mult), margins=[],
               certified=bool(slack > KKT_MARGIN and mult > KKT_MARGIN))
    chg = max(abs(d[m]) / P.su[m // Nu] for m in range(M))
    rec["margins"].append(("converged", float(abs(chg / P.sqp_tol - 1))))
    rec["converged"] = bool(chg <= P.sqp_tol)
    if rec["converged"]:
        rec.update(U=U, took="converged", hist=hist)
        return rec
    f0 = sum(t * t for t in res) / 2
    dd = sum(g[i] * d[i] for i in range(M))
    gv = [v[m] + d[m] for m in range(M)]
    rec.update(f0=float(f0), hist=(d, gv))
    toU = lambda w: [[w[n * Nu + l] for n in range(2)] for l in range(Nu)]  # noqa: E731
    if hist is not None:
        df = [(d[m] - hist[0][m]) / P.su[m // Nu] for m in range(M)]
        den = sum(t * t for t in df)
        if den > 0:
            gam = sum(df[m] * d[m] / P.su[m // Nu] for m in range(M)) / den
            vc = [min(max(gv[m] - gam * (gv[m] - hist[1][m]), mpf(P.lb[m // Nu])), mpf(P.ub[m // Nu])) for m in range(M)]
            fc, inb = _cost(P, x, toU(vc), ul, r, True)
            gap = (f0 + LS_C1 * dd - fc) / f0
            rec["margins"].append(("anderson", float(abs(gap))))
            if P.has_xb():
                edge = min(min(xs[s] - P.xmin[s], P.xmax[s] - xs[s]) / (XMAX[s] - XMIN[s])
                           for xs in _predict(P, x, toU(vc), True, False)[0] for s in range(3))
                rec["margins"].append(("anderson_states", float(abs(edge))))
            if inb and gap >= 0:
                rec.update(U=toU(vc), took="anderson")
                return rec
    alpha, k = mpf(1), 0
    for k in range(LS_MAX):
        f1, _ = _cost(P, x, toU([v[m] + alpha * d[m] for m in range(M)]), ul, r, True)
        gap = _armijo_gap(f1, f0, alpha, dd)
        rec["margins"].append(("armijo%d" % k, float(abs(gap))))
        if gap >= 0:
            break
        alpha /= 2
    rec.update(U=toU([v[m] + alpha * d[m] for m in range(M)]), took="armijo%d" % k)
    return rec


# ------------------------------------------------------------------------------------------------
# float64 restatement of the device's algorithm

def _rhs_v(p, x, u, xd, ud):
    """float64 rhs with K tangents at once (xd [3][K], ud [2][K]), the expressions of vdv_rhs."""
    f, fd = rhs(p, x, u, xd, ud)
    return f, [np.asarray(t, float) + np.zeros_like(xd[0]) for t in fd]


def _rk4_v(p, h, nsub, x, u, xd, ud):
    x = list(x)
    X = [np.array(t, float) for t in xd]
    for _ in range(nsub):
        k1, K1 = _rhs_v(p, x, u, X, ud)
        k2, K2 = _rhs_v(p, [x[i] + 0.5 * h * k1[i] for i in range(3)], u, [X[i] + 0.5 * h * K1[i] for i in range(3)], ud)
        k3, K3 = _rhs_v(p, [x[i] + 0.5 * h * k2[i] for i in range(3)], u, [X[i] + 0.5 * h * K2[i] for i in range(3)], ud)
        k4, K4 = _rhs_v(p, [x[i] + h * k3[i] for i in range(3)], u, [X[i] + h * K3[i] for i in range(3)], ud)
        x = [x[i] + (h / 6.0) * (k1[i] + 2.0 * k2[i] + 2.0 * k3[i] + k4[i]) for i in range(3)]
        X = [X[i] + (h / 6.0) * (K1[i] + 2.0 * K2[i] + 2.0 * K3[i] + K4[i]) for i in range(3)]
    return x, X


def nm_up(i, k, M):
    return i * M - ((i * (i - 1)) >> 1) + (k - i)


def _f64_pass(P, x, ul, r, v, mutate=None):
    """mpass for one point: increments v [M] -> (R packed, c, U, XP, SX in the increments, f)."""
    M, Nu = P.M, P.Nu
    wu = np.array([P.wu[m // Nu] for m in range(M)])
    U = np.array([ul[m // Nu] + v[(m // Nu) * Nu:m + 1].sum() for m in range(M)])
    R = np.diag(wu).astype(float)
    c = wu * v
    X = [np.zeros(M) for _ in range(3)]
    xs = [float(t) for t in x]
    XP, SX, fo = [], [], 0.0
    h = P.ts / P.nsub
    nrow = 0
    for i in range(P.N):
        li = min(i, Nu - 1)
        u = [U[li], U[Nu + li]]
        ud = [np.array([1.0 if m // Nu == n and m % Nu <= li else 0.0 for m in range(M)]) for n in range(2)]
        xs, X = _rk4_v(P.params, h, P.nsub, xs, u, X, ud)
        XP.append(list(xs))
        SX.append([t.copy() for t in X])
        for j in range(P.ny):
            if not P.wy[j] > 0.0:
                continue
            w = P.wy[j] * X[P.xc[j]]
            if mutate and mutate[0] == "tangent" and mutate[1] == nrow:
                w[mutate[2]] *= 1.0 + 1e-6
            e = P.wy[j] * (xs[P.xc[j]] - r[j])
            fo += e * e
            for k in range(M):
                a, bb = R[k, k], w[k]
                if bb != 0.0 and not (mutate and mutate[0] == "rotation" and mutate[1:] == (nrow, k)):
                    ri = 1.0 / math.sqrt(a * a + bb * bb)
                    cs, sn = a * ri, bb * ri
                    rk = R[k, k:].copy()
                    R[k, k:] = cs * rk + sn * w[k:]
                    w[k:] = -sn * rk + cs * w[k:]
                    ck = c[k]
                    c[k] = cs * ck + sn * e
                    e = -sn * ck + cs * e
            nrow += 1
    f = 0.5 * (fo + float(((wu * v) ** 2).sum()))
    return R, c, U, XP, SX, f


def _f64_cost(P, x, ul, r, v):
    M, Nu = P.M, P.Nu
    U = [ul[m // Nu] + v[(m // Nu) * Nu:m + 1].sum() for m in range(M)]
    xs = [float(t) for t in x]
    fa, inb = 0.0, True
    h = P.ts / P.nsub
    for i in range(P.N):
        li = min(i, Nu - 1)
        xs = _rk4_plain(P.params, h, P.nsub, xs, [U[li], U[Nu + li]])
        for j in range(P.ny):
            e = P.wy[j] * (xs[P.xc[j]] - r[j])
            fa += e * e
        inb = inb and all(P.xmin[s] <= xs[s] <= P.xmax[s] for s in range(3))
    wu = np.array([P.wu[m // Nu] for m in range(M)])
    return 0.5 * (fa + float(((wu * v) ** 2).sum())), inb


def _rk4_plain(p, h, nsub, x, u):
    x = list(x)
    for _ in range(nsub):
        k1 = rhs(p, x, u)
        k2 = rhs(p, [x[i] + 0.5 * h * k1[i] for i in range(3)], u)
        k3 = rhs(p, [x[i] + 0.5 * h * k2[i] for i in range(3)], u)
        k4 = rhs(p, [x[i] + h * k3[i] for i in range(3)], u)
        x = [x[i] + (h / 6.0) * (k1[i] + 2.0 * k2[i] + 2.0 * k3[i] + k4[i]) for i in range(3)]
    return x


def f64_step(P, x, ul, r, v, active, hist=None, mutate=None):
    """One iteration of the kernel's controller in float64 on the truth's active set (tags of
    gn_step).  v: increments [M].  Returns (v_next, converged, hist, took)."""
    M, Nu = P.M, P.Nu
    R, c, U, XP, SX, f0 = _f64_pass(P, x, ul, r, v, mutate)
    # R^-1, packed upper triangle, column by column (the kernel's lane-j solve of R x = e_j)
    Ri = np.zeros((M, M))
    for j in range(M):
        for kk in range(j, -1, -1):
            a = 1.0 if kk == j else 0.0
            for q in range(kk + 1, j + 1):
                a -= R[kk, q] * Ri[q, j]
            Ri[kk, j] = a / R[kk, kk]
    s = -Ri @ c
    if active:
        # rows C s >= b in the increments: cumulative box rows and the state rows
        C, b = [], []
        for t in active:
            if t[0] in ("lo", "hi"):
                m = t[1]
                row = np.array([1.0 if k // Nu == m // Nu and k <= m else 0.0 for k in range(M)])
                bound = (P.lb if t[0] == "lo" else P.ub)[m // Nu] - U[m]
                C.append(row if t[0] == "lo" else -row)
                b.append(bound if t[0] == "lo" else -bound)
            else:
                _, i, si = t
                row = np.array([SX[i][si][k] for k in range(M)])
                C.append(row if t[0] == "xmin" else -row)
                b.append(P.xmin[si] - XP[i][si] if t[0] == "xmin" else XP[i][si] - P.xmax[si])
        C, b = np.array(C), np.array(b)
        CJ = C @ Ri
        mu = np.linalg.solve(CJ @ CJ.T, b - C @ s)
        s = s + Ri @ (CJ.T @ mu)
    su = np.array([P.su[m // Nu] for m in range(M)])
    dpre = np.array([s[(m // Nu) * Nu:m + 1].sum() for m in range(M)])
    if np.max(np.abs(dpre) / su) <= P.sqp_tol:
        return v, True, hist, "converged"
    dd = float(c @ (np.triu(R) @ s))
    gv = v + s
    new_hist = (dpre, gv)
    if hist is not None:
        wdf = (dpre - hist[0]) / su
        den = float(wdf @ wdf)
        if den > 0.0:
            gam = float(wdf @ (dpre / su)) / den
            vc0 = gv - gam * (gv - hist[1])
            lbv = np.array([P.lb[m // Nu] for m in range(M)])
            ubv = np.array([P.ub[m // Nu] for m in range(M)])
            ucl = np.array([min(max(ul[m // Nu] + vc0[(m // Nu) * Nu:m + 1].sum(), lbv[m]), ubv[m]) for m in range(M)])
            vc = np.array([ucl[m] - (ul[m // Nu] if m % Nu == 0 else ucl[m - 1]) for m in range(M)])
            fc, inb = _f64_cost(P, x, ul, r, vc)
            if (inb or not P.has_xb()) and fc <= f0 + LS_C1 * dd:
                return vc, False, new_hist, "anderson"
    alpha, k = 1.0, 0
    for k in range(LS_MAX):
        f1, _ = _f64_cost(P, x, ul, r, v + alpha * s)
        if f1 <= f0 + LS_C1 * alpha * dd or f1 - f0 <= LS_FLAT * f0:
            break
        alpha *= 0.5
    return v + alpha * s, False, new_hist, "armijo%d" % k


# ------------------------------------------------------------------------------------------------
# closed loops of calls

def call_chain(P, x0, u0, r, open_loop=True, plant_x0=None, memo=None):
    """closedloop_toolbox_nmpc restated on gn_step, at most P.sqp_max iterations per call.  r
    [ny][nit] (float).  Returns dict(u [2][nit], uopt [Nu][2] (the open-loop call's moves), iters,
    maxiter, bounds_edge: the closed-loop states' smallest distance inside the bounds of MPCT_ST_BOUNDS
    (negative: outside), calls: per call (t, or -1 for the open-loop call) its step records)."""
    nit = len(r[0])
    Nu = P.Nu
    pl = [mpf(v) for v in P.plant]

    def controller(x, ul, rv, U):
        recs, hist = [], None
        for _ in range(P.sqp_max):
            key = repr((x, ul, rv, U, hist))
            rec = memo[key] if memo is not None and key in memo else gn_step(P, x, ul, rv, U, hist)
            if memo is not None:
                memo[key] = rec
            recs.append(rec)
            if rec["converged"]:
                return U, recs, True
            U, hist = rec["U"], rec["hist"]
        return U, recs, False

    x = [mpf(float(v)) for v in (x0 if plant_x0 is None else plant_x0)]
    ul = [mpf(float(v)) for v in u0]
    xstart = list(x)
    U = [list(ul) for _ in range(Nu)]
    u = [[float(v)] for v in u0]
    calls, iters, maxiter = [], 0, False
    # the kernel's MPCT_ST_BOUNDS test on every closed-loop state: x_min - 1e-9 <= x <= x_max + 1e-9
    edge = lambda z: min(min(z[s] - (P.xmin[s] - 1e-9), (P.xmax[s] + 1e-9) - z[s]) for s in range(3))  # noqa: E731
    bedge = edge(x)
    for t in range(1, nit):
        U, recs, conv = controller(x, ul, [mpf(float(r[j][t])) for j in range(P.ny)], U)
        calls.append((t, recs, [float(v) for v in x]))
        iters += len(recs)
        maxiter = maxiter or not conv
        ul = list(U[0])
        x = rk4(pl, mpf(P.ts), P.nsub, x, ul)
        bedge = min(bedge, edge(x))
        for n in range(2):
            u[n].append(float(ul[n]))
        U = U[1:] + [list(U[-1])]
    out = dict(u=np.array(u), iters=iters, maxiter=maxiter, calls=calls, bounds_edge=float(bedge))
    if open_loop:
        ul = [mpf(float(v)) for v in u0]
        Uo, recs, conv = controller(xstart, ul, [mpf(float(r[j][nit - 1])) for j in range(P.ny)],
                                    [list(ul) for _ in range(Nu)])
        out["calls"].append((-1, recs, [float(v) for v in xstart]))
        out["iters"] += len(recs)
        out["maxiter"] = out["maxiter"] or not conv
        out["uopt"] = np.array([[float(t) for t in row] for row in Uo])
    return out


def f64_chain(P, x0, u0, r, truth, open_loop=True, plant_x0=None, mutate=None):
    """The same loop on f64_step with the truth's active sets (truth: call_chain's result).
    Returns dict(u, uopt, iters, maxiter, took: per call the decisions taken)."""
    nit = len(r[0])
    M, Nu = P.M, P.Nu
    h = P.ts / P.nsub
    by_call = {t: recs for t, recs, _ in truth["calls"]}

    def controller(t, x, ul, rv, v):
        hist, took = None, []
        for it in range(P.sqp_max):
            recs = by_call[t]
            act = recs[min(it, len(recs) - 1)]["active"]
            v, conv, hist, tk = f64_step(P, x, ul, rv, v, act, hist, mutate)
            took.append(tk)
            if conv:
                return v, took, True
        return v, took, False

    x = [float(v) for v in (x0 if plant_x0 is None else plant_x0)]
    xstart = list(x)
    ul = [float(v) for v in u0]
    v = np.zeros(M)
    u = [[float(t)] for t in u0]
    took_all, iters, maxiter = {}, 0, False
    for t in range(1, nit):
        v, took, conv = controller(t, x, ul, [float(r[j][t]) for j in range(P.ny)], v)
        took_all[t] = took
        iters += len(took)
        maxiter = maxiter or not conv
        ul = [ul[0] + v[0], ul[1] + v[Nu]]
        x = _rk4_plain(P.plant, h, P.nsub, x, ul)
        for n in range(2):
            u[n].append(ul[n])
        v = np.array([v[m + 1] if m % Nu < Nu - 1 else 0.0 for m in range(M)])
    out = dict(u=np.array(u), iters=iters, maxiter=maxiter, took=took_all)
    if open_loop:
        ul = [float(t) for t in u0]
        vo, took, conv = controller(-1, xstart, ul, [float(r[j][nit - 1]) for j in range(P.ny)], np.zeros(M))
        out["took"][-1] = took
        out["iters"] += len(took)
        out["maxiter"] = out["maxiter"] or not conv
        out["uopt"] = np.array([[ul[n] + vo[n * Nu:n * Nu + l + 1].sum() for n in range(2)] for l in range(Nu)])
    return out


# ------------------------------------------------------------------------------------------------
# the cases and the truth of the nmpc_model.h probe

def probe_cases():
    """(p [16], x [3], u [2], nsub): the steady state, the corners of the state / input box, twelve seeded
    points inside it; the reference parameters (E1 == E2: the shared exp) and a vandevusse_mc_params row with
    E2 moved off E1 (the split); nsub 1 and 10."""
    from mpct.nmpc import vandevusse_mc_params

    rng = np.random.default_rng(20250321)
    pts = [(steady_state(), np.array(U0))]
    for k in range(32):
        b = [(k >> i) & 1 for i in range(5)]
        pts.append((np.where(b[:3], XMAX, XMIN).astype(float), np.where(b[3:], UMAX, UMIN).astype(float)))
    pts += [(rng.uniform(XMIN, XMAX), rng.uniform(UMIN, UMAX)) for _ in range(12)]
    p2 = vandevusse_mc_params(3)[2].copy()
    p2[4] *= 1.0 + 1e-3
    assert p2[3] != p2[4]
    # nsub = 10 on the steady state, the seeded points and four of the corners (the truth's cost)
    return [(np.array(p, float), x, u, nsub) for p in (VDV_PARAMS, p2)
            for nsub, sel in ((1, pts), (10, pts[:1] + pts[33:] + pts[1:33:9])) for x, u in sel]


def probe_seeds(kind, Nu=7):
    """[64][3], [64][2]: the kernel's own (lane m < 2 Nu: ud = e_n, xd = 0; the others zero) or four seeded
    nonzero (xd, ud) pairs, lane l carrying pair l % 4."""
    xd, ud = np.zeros((64, 3)), np.zeros((64, 2))
    for m in range(2 * Nu):
        ud[m, m // Nu] = 1.0
    if kind == "xd":
        rng = np.random.default_rng(5)
        xd, ud = np.tile(rng.standard_normal((4, 3)), (16, 1)), np.tile(rng.standard_normal((4, 2)), (16, 1))
    return xd, ud


def probe_truth(rk4_, c, xd, ud):
    """mpmath value and tangents (two distinct lanes suffice for the kernel's seeds: one per input), and the
    float64 restatement's, as ([3], [64][3]) pairs."""
    p, x, u, nsub = c
    mp_ = lambda v: [mpf(float(t)) for t in v]  # noqa: E731
    lanes = sorted({tuple(np.r_[xd[l], ud[l]]) for l in range(64)})
    tv, fv = {}, {}
    for s in lanes:
        if rk4_:
            # the sub-step is the double the device is given, h = fl(TS / nsub)
            xm, Xm = rk4(mp_(p), mpf(TS / nsub) * nsub, nsub, mp_(x), mp_(u), [mp_(s[:3])], [mp_(s[3:])])
            xf, Xf = _rk4_v(tuple(p), TS / nsub, nsub, list(x), list(u), [np.array([s[i]]) for i in range(3)],
                              [np.array([s[3 + i]]) for i in range(2)])
            Xm, Xf = Xm[0], [float(t[0]) for t in Xf]
        else:
            xm, Xm = rhs(mp_(p), mp_(x), mp_(u), mp_(s[:3]), mp_(s[3:]))
            xf, Xf = rhs(tuple(p), list(x), list(u), list(s[:3]), list(s[3:]))
        tv[s] = (xm, Xm)
        fv[s] = (np.array(xf, float), np.array(Xf, float))
    key = [tuple(np.r_[xd[l], ud[l]]) for l in range(64)]
    return (tv[key[0]][0], [tv[k][1] for k in key]), (fv[key[0]][0], np.array([fv[k][1] for k in key]))


def probe_dev(a, t, floor=0.0):
    """max |a - t| over the largest |t|, or over `floor` where that is larger: the size of the terms of a
    derivative that cancels (the truth t in mpmath, the difference taken there)."""
    a, t = np.asarray(a, float).reshape(-1), list(np.asarray(t, object).reshape(-1))
    scale = max([abs(v) for v in t] + [mpf(floor), mpf(1e-300)])
    return float(max(abs(mpf(float(x)) - v) for x, v in zip(a, t)) / scale)



PROBE_RUNS = [(r, k) for r in ("rhs", "rk4") for k in ("own", "xd")]


def probe_reference(which, kind):
    """The probe's cases with their truth, and the restatement's errors (value, tangent) that set the bounds:
    (cases, xd, ud, [(truth value, truth tangents, value floor, tangent floor)], rv, rd)."""
    rk4_ = which == "rk4"
    cases = probe_cases()
    xd, ud = probe_seeds(kind)
    rows, rv, rd = [], 0.0, 0.0
    for c in cases:
        (tx, tX), (fx, fX) = probe_truth(rk4_, c, xd, ud)
        # the derivative's terms u x and u xd, where its entries cancel (the corners); the RK4 state does not
        fl = 0.0 if rk4_ else float(np.abs(c[1]).max() * max(np.abs(c[2]).max(), 1.0))
        fld = 0.0 if rk4_ else fl * float(max(np.abs(xd).max(), np.abs(ud).max()))
        rv, rd = max(rv, probe_dev(fx, tx, fl)), max(rd, probe_dev(fX, tX, fld))
        rows.append((tx, tX, fl, fld))
    return cases, xd, ud, rows, rv, rd


# ------------------------------------------------------------------------------------------------
# LDS layout of nmpc_model.h restated

def _even(n):
    return (n + 1) & ~1


def nm_layout(M, N, G):
    """Pieces (name, offset, length in doubles) of nm_layout and the total."""
    o, pieces = 0, []

    def take(name, n):
        nonlocal o
        pieces.append((name, o, n))
        o += _even(n)

    take("ri", M * (M + 1) // 2)
    take("jt", M * M)
    take("ra", M * (M + 3) // 2)
    for nm in ("dv", "xc", "uo", "nv"):
        take(nm, M + 1)
    take("bits", (6 * N + 63) // 64)
    w = 16 if G > 1 else M + 1
    g, gp = 0, []
    for nm, n in (("g_rr", M * (M + 1) // 2), ("g_cv", w), ("g_u", w), ("g_v", w), ("g_rw", w), ("g_xp", 3 * N),
                  ("g_sx", 3 * N * M)):
        gp.append((nm, g, n))
        g += _even(n)
    for k in range(G):
        pieces += [("%s[%d]" % (nm, k), o + k * g + off, n) for nm, off, n in gp]
    return pieces, _even(o + G * g)


def nm_groups(M, N):
    if M > 15:
        return 1
    if nm_layout(M, N, 4)[1] * 8 <= 40 * 1024:
        return 4
    return 2 if nm_layout(M, N, 2)[1] * 8 <= 64 * 1024 else 1


def lds_bytes(M, N):
    return nm_layout(M, N, nm_groups(M, N))[1] * 8


# ------------------------------------------------------------------------------------------------
# the cases of tests/test_nmpc_units*.py

def measure(a, b, su=SU):
    """max |a - b| / u_scale over moves [..][2] (the last axis is the input)."""
    return float(np.max(np.abs(np.asarray(a, float) - np.asarray(b, float)) / np.asarray(su)))


def _case(name, family, N, Nu, delta, lam, rstep, n_max=31, nu_max=15, xc=(2, 3), sqp_max=1, tstars=None, nit=None,
          short=True, pre=None, **kw):
    nit = Nu + 1 if nit is None else nit
    return dict(name=name, family=family, N=N, Nu=Nu, delta=tuple(delta), lam=tuple(lam), rstep=tuple(rstep),
                n_max=n_max, nu_max=nu_max, xc=tuple(xc), sqp_max=sqp_max, nit=nit, short=short,
                tstars=tuple(tstars) if tstars else (nit - 1, None), pre=tuple(pre) if pre else None, kw=kw)


# reference steps (from the steady state's outputs): c_B to 1.0 and T down 4 K, the size of the
# driver's own setpoint changes
_R23 = (1.0, -4.0)
_PLANT = tuple(v * f for v, f in zip(VDV_PARAMS, (1 + 2e-3, 1 - 1e-3, 1 + 3e-3, 1, 1, 1, 1 - 2e-3, 1 + 1e-3, 1 + 2e-3,
                                                  1, 1, 1, 1, 1, 1, 1)))
CASES = [
    # a. the step vector, every class and tier (weights inside nmpc_candidate_grid's ranges)
    _case("a/3-1", "a", 3, 1, (1.0, 0.5), (0.05, 0.02), _R23),
    _case("a/4-2", "a", 4, 2, (0.093, 0.113), (0.246, 0.123), _R23),
    _case("a/3-3", "a", 3, 3, (3.0, 0.02), (0.001, 0.001), _R23),          # lambda at the small end
    _case("a/8-7", "a", 8, 7, (1.0, 0.5), (0.05, 0.02), _R23),              # M = 14
    _case("a/9-8", "a", 9, 8, (1.0, 0.5), (0.05, 0.02), _R23),              # M = 16: the other class
    _case("a/16-16", "a", 16, 16, (0.5, 2.0), (0.01, 0.3), _R23, nu_max=16, short=False),
    _case("a/70-7", "along", 70, 7, (0.7, 1.0), (0.05, 0.2), _R23, n_max=127, nu_max=8, short=False),     # G = 2
    _case("a/127-7", "along", 127, 7, (1.0, 0.5), (0.1, 0.1), _R23, n_max=127, nu_max=8, short=False),    # G = 1
    # b. output selection
    _case("b/x1", "b", 4, 2, (1.0,), (0.05, 0.02), (-0.2,), xc=(1,)),
    _case("b/x2", "b", 4, 2, (1.0,), (0.05, 0.02), (1.0,), xc=(2,)),
    _case("b/x3", "b", 4, 2, (1.0,), (0.05, 0.02), (-4.0,), xc=(3,)),
    _case("b/x31", "b", 4, 2, (0.5, 1.0), (0.05, 0.02), (-4.0, -0.2), xc=(3, 1)),
    _case("b/w0", "b", 4, 2, (1.0, 0.0), (0.05, 0.02), _R23),               # the wy == 0 row skip
    # e. the second iteration
    _case("e/4-2", "e", 4, 2, (0.093, 0.113), (0.246, 0.123), _R23, sqp_max=2),
    _case("e/8-7", "e", 8, 7, (1.0, 0.5), (0.05, 0.02), _R23, sqp_max=2),                     # Anderson taken
    _case("e/8-7-full", "e", 8, 7, (0.105, 0.0652), (0.718, 0.0215), (1.139, -5.64), sqp_max=2),  # the full step instead
    _case("e/4-2-halved", "e", 4, 2, (0.128, 0.0103), (0.309, 0.0029), (0.747, -8.92), sqp_max=2),  # and two halvings
    # c. constraints inside the one step (scales stay nominal: only the bounds move)
    _case("c/first", "c", 4, 2, (1.0, 0.5), (0.05, 0.02), _R23, u_max=(22.5, 150.0), u_min=(0.0, 124.2)),
    _case("c/cum", "c", 6, 3, (0.093, 0.113), (0.246, 0.123), _R23, u_max=(22.3, 150.0)),
    _case("c/state", "c", 6, 3, (1.0, 0.5), (0.05, 0.02), (0.95, 139.0), x_max=(6.0, 1.2, 135.5)),
    _case("c/state-drop", "c", 6, 3, (4.08, 0.24), (0.00153, 0.00109), (0.761, 140.4), x_max=(6.0, 1.2, 136.3)),
    # d. speculated passes: the reference steps at t* = 2, 3, 4 (the call there starts from a pass that the
    # call 1, 2, 3 steps earlier ran, G = 4; G = 2 speculates one call ahead, G = 1 none), the last one is held
    _case("d/4-2", "d", 4, 2, (1.0, 0.5), (0.05, 0.02), _R23, nit=6, tstars=(2, 3, 4, None)),
    _case("d/4-2-plant", "d", 4, 2, (1.0, 0.5), (0.05, 0.02), _R23, nit=6, tstars=(2, 3, 4, None), plant=_PLANT,
          sqp_tol=1e-3),
    # the same with a nonzero warm start: a first step at t = 1 (one Gauss-Newton step, sqp_max = 1), then calls
    # that return their shifted warm starts at once under sqp_tol = 0.03, so the pass the call at t = 2 speculates
    # 1, 2, 3 steps ahead shifts nonzero increments and applies nonzero first moves; a second step at t*
    _case("d/8-7-shift", "d", 8, 7, (1.0, 0.5), (0.05, 0.02), (0.9, -8.0), nit=7, tstars=(3, 4, 5, None), pre=_R23,
          sqp_tol=0.03),
    _case("d/70-7", "dlong", 70, 7, (0.7, 1.0), (0.05, 0.2), _R23, n_max=127, nu_max=8, nit=6, tstars=(2, 3, None),
          short=False),
    _case("d/127-7", "dlong", 127, 7, (1.0, 0.5), (0.1, 0.1), _R23, n_max=127, nu_max=8, nit=6, tstars=(2, 3, None),
          short=False),
]
BY_NAME = {c["name"]: c for c in CASES}
FAMILIES = sorted({c["family"] for c in CASES})
MUTATIONS = ("tangent", "rotation")      # planted at the last streamed row, column 1 (a move no case pins)


def case_key(c):
    """The case's parameters as the fixture stores them: an edited case needs a regenerated fixture."""
    return repr(sorted((k, sorted(v.items()) if isinstance(v, dict) else v) for k, v in c.items()))


def case_prob(c):
    return Prob(c["N"], c["Nu"], c["delta"], c["lam"], xc=c["xc"], sqp_max=c["sqp_max"], **c["kw"])


def case_refs(c, x0):
    """[nref][ny][nit]: the steady state's outputs, stepped from t* on (a positive rstep entry is the new
    value, a negative one an offset); t* = None: held throughout.  pre: a first step of every set at t = 1."""
    xc = [k - 1 for k in c["xc"]]
    out = []
    for ts_ in c["tstars"]:
        r = np.tile(np.asarray(x0, float)[xc][:, None], (1, c["nit"]))
        for j, v in enumerate(c["pre"] or ()):
            r[j, 1:] = v if v > 0 else x0[xc[j]] + v
        if ts_ is not None:
            for j, v in enumerate(c["rstep"]):
                r[j, ts_:] = v if v > 0 else x0[xc[j]] + v
        out.append(r)
    return np.array(out)


def run_case(c, mutations=True):
    """Truth, certificate, margins, the restatement's error and the planted errors' deviations of one
    case: a dict of arrays (what tests/golden/nmpc_step_truth.npz stores under "<name>/<field>")."""
    x0 = steady_state()
    P = case_prob(c)
    refs = case_refs(c, x0)
    memo = {}
    out = dict(x0=x0, refs=refs, u=[], uopt=[], iters=[], maxiter=[], early=[], bounds_edge=[])
    err, slack, mult, tie, conv, mut = 0.0, INF, INF, INF, INF, [INF] * len(MUTATIONS)
    for k, r in enumerate(refs):
        tr = call_chain(P, x0, U0, r, memo=memo)
        out["u"].append(tr["u"])
        out["uopt"].append(tr["uopt"])
        out["iters"].append(tr["iters"])
        out["maxiter"].append(tr["maxiter"])
        out["bounds_edge"].append(tr["bounds_edge"])
        ts_ = c["tstars"][k]
        out["early"].append(all(recs[0]["converged"] for t, recs, _ in tr["calls"] if (1 if c["pre"] else 0) < t < (ts_ or c["nit"])))
        for t, recs, _ in tr["calls"]:
            for rec in recs:
                if not rec["certified"]:
                    raise AssertionError("%s: KKT certificate failed at call %d: %r" % (c["name"], t, rec["active"]))
                slack, mult = min(slack, rec["slack"]), min(mult, rec["mult"])
                for n, m in rec["margins"]:
                    if n == "converged":
                        conv = min(conv, m)
                    else:
                        tie = min(tie, m)
        with np.errstate(all="ignore"):
            f = f64_chain(P, x0, U0, r, tr)
            err = max(err, measure(f["uopt"], tr["uopt"]), measure(f["u"].T, tr["u"].T))
            if mutations and ts_ is not None:
                for i, mu in enumerate(MUTATIONS):
                    fm = f64_chain(P, x0, U0, r, tr, mutate=(mu, P.N * sum(w > 0.0 for w in P.wy) - 1, 1))
                    dev = max(measure(fm["uopt"], tr["uopt"]), measure(fm["u"].T, tr["u"].T))
                    mut[i] = min(mut[i], dev if np.isfinite(dev) else 1e300)
        if k == 0:
            main = tr["calls"][-1][1]
            out.update(nactive=len(main[0]["active"]), drops=max(rec["drops"] for rec in main),
                       kinds=",".join(sorted({t[0] + ("0" if t[0] in ("lo", "hi") and t[1] % c["Nu"] == 0 else "")
                                              for t in main[0]["active"]})),
                       took=",".join(rec["took"] for rec in main))
    out.update(err=err, slack=slack, mult=mult, tie=tie, conv=conv, mut=np.array(mut), case=case_key(c))
    return {k: np.asarray(v) for k, v in out.items()}


def probe_table_text(store):
    lines = ["probe     restatement value   bound     restatement tangent   bound"]
    for which, kind in PROBE_RUNS:
        rv, rd = (float(t) for t in store["probe/%s-%s" % (which, kind)])
        lines.append("%-9s %-19.3g %-9.3g %-21.3g %.3g" % (which + "-" + kind, rv, DEVICE_FACTOR * rv, rd, DEVICE_FACTOR * rd))
    return "\n".join(lines)


def bound_table(results):
    """{family: (largest restatement error, bound = DEVICE_FACTOR x it, smallest planted deviation / bound)}
    from {name: run_case result}."""
    tab = {}
    for fam in FAMILIES:
        names = [c["name"] for c in CASES if c["family"] == fam]
        e = max(float(results[n]["err"]) for n in names)
        tab[fam] = (e, DEVICE_FACTOR * e, min(float(np.min(results[n]["mut"])) for n in names) / (DEVICE_FACTOR * e))
    return tab
