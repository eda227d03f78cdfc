"""The band kernel's free-response window update, restated in numpy (test helper).

mdband_kernel.hip carries the window F_t[k] = y(t+1+k | MVs held at u(t-1), MDs held at v(t)),
k = 0..N2-1, from step to step.  Every model entry (i, j) keeps a tail of the window, tl[l] = the
entry's own part of F[N2-1-l], l = 0..order-1, at stride ts = max(mz_maxa - 1, 1).  One step t does

    tail corrections   tl[l] += s_ij(N2 - l) du_j(t-1)         (MV)   where N2 - l >= 0
                       tl[l] += s_ij(N2 - 1 - l) dv_j(t)       (MD)   where N2 - 1 - l >= 0
    extension          ext = sum_l b[l] u_j(min(t + N2 - l, tcap)) - sum_{l>=1} a[l] tl[l-1],
                       tcap = t - 1 (MV) or t (MD), taps whose time is negative dropped
    tail shift         tl[l] = tl[l-1] for l = order-1..1, tl[0] = ext
    window             F[k] = F[k+1] + sum_n s_in(k+2) du_n(t-1) + sum_m s_im(k+1) dv_m(t),  k < N2-1
                       F[N2-1] = sum_j ext_ij

This module states exactly that, in any numpy float type (float64, numpy.longdouble), on the full
input history instead of the device's rings, plus the entry recursion of the plant (and, with the
output-bias estimator, of the parallel model).  closed_loop() feeds the window to the oracle's QP
(oracle.toolbox_band.band_qp, float64).  It is a yardstick, not a truth: the truth of the tests is the
oracle's forward simulation (oracle/toolbox_band.py), which shares none of this.

`fault` plants one index error of the kind the tests must be able to see (tests/test_band_family.py
negative controls):
    "no_shift"    the tail shift dropped
    "mv_index"    the MV correction reads s(N2 - 1 - l) instead of s(N2 - l)
    "md_as_mv"    the MD correction uses the MV index rule s(N2 - l)
    "own_stride"  the tails indexed with the entry's own order instead of the scenario's stride ts
    "md_tcap"     tcap of an MD taken as t - 1
"""
import numpy as np

FAULTS = ("no_shift", "mv_index", "md_as_mv", "own_stride", "md_tcap")


def entry_tables(P, dtype):
    """my x nin lists of (b, a, off): z^-1 taps with the delay folded into b, normalised by den[0];
    off is the first nonzero tap (len(b) for a zero entry).  P: rows of (num, den, delay), equal
    lengths of num and den."""
    out = []
    for row in P:
        r = []
        for num, den, delay in row:
            num = np.asarray(num, dtype=dtype)
            den = np.asarray(den, dtype=dtype)
            assert num.size == den.size
            b = np.concatenate([np.zeros(int(delay), dtype=dtype), num]) / den[0]
            nz = np.nonzero(b)[0]
            r.append((b, den / den[0], int(nz[0]) if nz.size else b.size))
        out.append(r)
    return out


def step_response(b, a, n, dtype):
    """s(0..n-1) of one entry by its difference equation."""
    s = np.zeros(n, dtype=dtype)
    for t in range(n):
        acc = dtype(0)
        for l in range(min(t + 1, b.size)):
            acc += b[l]
        for l in range(1, min(t, a.size - 1) + 1):
            acc -= a[l] * s[t - l]
        s[t] = acc
    return s


class Entries:
    """The entry recursion of mdband_kernel.hip's plant copies: y_e(t) = sum_l b[l] u_j(t-l)
    - sum_{l>=1} a[l] y_e(t-l), one history per entry."""

    def __init__(self, P, nit, dtype):
        self.T = entry_tables(P, dtype)
        self.my, self.nin = len(P), len(P[0])
        self.h = np.zeros((self.my, self.nin, nit), dtype=dtype)
        self.dtype = dtype

    def output(self, t, U):
        """y(t) from the inputs U[:, :t+1] (the MV rows are read up to t - 1 only when no entry has
        feedthrough from an MV)."""
        y = np.zeros(self.my, dtype=self.dtype)
        for i in range(self.my):
            for j in range(self.nin):
                b, a, off = self.T[i][j]
                a0 = self.dtype(0)
                a1 = self.dtype(0)
                for l in range(off, b.size):
                    if t - l >= 0:
                        a0 += b[l] * U[j, t - l]
                for l in range(1, a.size):
                    if t - l >= 0:
                        a1 -= a[l] * self.h[i, j, t - l]
                self.h[i, j, t] = a0 + a1
                y[i] += self.h[i, j, t]
        return y


class Window:
    """The carried window of one simulation."""

    def __init__(self, model, nu, N2, dtype=np.float64, fault=None):
        assert fault is None or fault in FAULTS
        self.T = entry_tables(model, dtype)
        self.my, self.nin, self.nu, self.N2 = len(model), len(model[0]), nu, N2
        self.dtype, self.fault = dtype, fault
        maxa = max(a.size for row in self.T for _, a, _ in row)
        self.ts = maxa - 1 if maxa > 2 else 1
        self.tail = np.zeros(self.my * self.nin * self.ts, dtype=dtype)   # flat, as the LDS block is
        self.F = np.zeros((self.my, N2), dtype=dtype)
        self.S = [[step_response(b, a, N2 + 2, dtype) for b, a, _ in row] for row in self.T]

    def advance(self, t, U, du_prev):
        """F_{t-1} -> F_t.  U (nin x >= t+1): MV rows valid up to t - 1, MD rows up to t;
        du_prev = u(t-1) - u(t-2).  Returns F_t (my x N2, a view)."""
        N2, nu, nin, dt, fault = self.N2, self.nu, self.nin, self.dtype, self.fault
        ext = np.zeros((self.my, nin), dtype=dt)
        dv = np.zeros(nin, dtype=dt)
        for j in range(nu, nin):
            dv[j] = U[j, t] - (U[j, t - 1] if t > 0 else dt(0))
        for i in range(self.my):
            for j in range(nin):
                b, a, off = self.T[i][j]
                na = a.size - 1
                e = i * nin + j
                base = e * (na if fault == "own_stride" else self.ts)
                tl = self.tail[base:base + max(na, 1)]
                sp = self.S[i][j]
                if j < nu:
                    dlt = du_prev[j]
                    if dlt != 0:
                        for l in range(na):
                            k = N2 - 1 - l if fault == "mv_index" else N2 - l
                            if k >= 0:
                                tl[l] += sp[k] * dlt
                else:
                    dlt = dv[j]
                    if dlt != 0:
                        for l in range(na):
                            k = N2 - l if fault == "md_as_mv" else N2 - 1 - l
                            if k >= 0:
                                tl[l] += sp[k] * dlt
                tcap = t - 1 if (j < nu or fault == "md_tcap") else t
                a0 = dt(0)
                a1 = dt(0)
                for l in range(off, b.size):
                    tau = min(t + N2 - l, tcap)
                    if tau >= 0:
                        a0 += b[l] * U[j, tau]
                for l in range(1, na + 1):
                    a1 -= a[l] * tl[l - 1]
                x = a0 + a1
                if fault != "no_shift":
                    for l in range(na - 1, 0, -1):
                        tl[l] = tl[l - 1]
                if na > 0:
                    tl[0] = x
                ext[i, j] = x
        F = self.F
        for i in range(self.my):
            for k in range(N2 - 1):
                f = F[i, k + 1]
                for n in range(nu):
                    f += self.S[i][n][k + 2] * du_prev[n]
                for m in range(nu, nin):
                    if dv[m] != 0:
                        f += self.S[i][m][k + 1] * dv[m]
                F[i, k] = f
            f = dt(0)
            for j in range(nin):
                f += ext[i, j]
            F[i, N2 - 1] = f
        return F


def windows_on(model, nu, N2, U, du, dtype=np.longdouble, fault=None):
    """The carried window at every step of a given input history: U (nin x nit, MVs applied and
    MDs measured), du (nu x nit, the applied moves).  Returns nit x my x N2."""
    nit = U.shape[1]
    Ud = np.asarray(U, dtype=dtype)
    dud = np.asarray(du, dtype=dtype)
    w = Window(model, nu, N2, dtype, fault)
    out = np.zeros((nit, len(model), N2), dtype=dtype)
    zero = np.zeros(nu, dtype=dtype)
    for t in range(nit):
        out[t] = w.advance(t, Ud, dud[:, t - 1] if t > 0 else zero)
    return out


class Loop:
    """What closed_loop returns: y (my x nit), u (nu x nit), du (nu x nit), f (nit x my*N2, the
    window the QP saw, bias included), x (nit x nu*Nu+1, the QP solutions), all float64."""

    def __init__(self, y, u, du, f, x):
        self.y, self.u, self.du_hist, self.f, self.x = y, u, du, f, x


def closed_loop(osc, model, r, v, N2, Nu, delta, lam, nit, dtype=np.float64, fault=None, plant=None):
    """The device's loop restated: plant entries -> y(t), carried window -> F_t, the oracle's QP on
    F_t (float64), u(t) = u(t-1) + du.  osc: the oracle's BandScenario (bounds, bands, scale factors
    and the QP's dynamic matrix); model: rows of (num, den, delay).  plant (rows of entries): the
    output-bias estimator's loop, the window plus b(t) = y(t) - y_model(t) on every row."""
    from oracle.toolbox_band import band_qp, dyn_matrix, step_table

    my, nu = len(model), osc.nu
    nin = len(model[0])
    r = np.asarray(r, dtype=float).reshape(my, nit)
    v = np.asarray(v, dtype=float).reshape(nin - nu, nit)
    d = np.abs(np.asarray(delta, dtype=float))
    lm = np.abs(np.asarray(lam, dtype=float))
    wq = (d / osc.sy) ** 2 if osc.weights_squared else d / osc.sy
    wl = (lm / osc.su) ** 2 if osc.weights_squared else lm / osc.su
    G = dyn_matrix(step_table(osc, N2 + 2), nu, N2, Nu)
    U = np.zeros((nin, nit), dtype=dtype)
    U[nu:] = v
    pl = Entries(model if plant is None else plant, nit, dtype)
    mdl = Entries(model, nit, dtype) if plant is not None else None
    w = Window(model, nu, N2, dtype, fault)
    Y = np.zeros((my, nit))
    Uo = np.zeros((nu, nit))
    DU = np.zeros((nu, nit))
    Fs = np.zeros((nit, my * N2))
    Xs = np.zeros((nit, nu * Nu + 1))
    u_prev = np.zeros(nu, dtype=dtype)
    du_prev = np.zeros(nu, dtype=dtype)
    for t in range(nit):
        y = pl.output(t, U)
        bias = y - mdl.output(t, U) if mdl is not None else np.zeros(my, dtype=dtype)
        F = w.advance(t, U, du_prev)
        f = np.asarray(F + bias[:, None], dtype=float).reshape(-1)
        x, _ = band_qp(osc, G, f, r[:, t], np.asarray(u_prev, dtype=float), N2, Nu, wq, wl)
        du_prev = np.array([x[n * Nu] for n in range(nu)], dtype=dtype)
        u_prev = u_prev + du_prev
        U[:nu, t] = u_prev
        Y[:, t], Uo[:, t], DU[:, t], Fs[t], Xs[t] = y, u_prev, du_prev, f, x
    return Loop(Y, Uo, DU, Fs, Xs)
