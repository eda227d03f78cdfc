"""Plain references for the device unit probes (tests/device_units/unit_probe.hip): numpy and python
only, nothing imported from the product package.

  * primitive references: exact sums (math.fsum), the argmin rule, the shifts, the block prefix sums,
    correctly rounded 1/x and 1/sqrt(x) from rational arithmetic;
  * the QP optimum from an independent algorithm (oracle.toolbox_gpc.qp_primal_active_set: primal
    active set with lstsq), accepted only with a passing KKT residual;
  * the seeded case generator shared by tests/test_qp_units.py (CPU: every case has the property it
    is named for) and tests/test_qp_units_gpu.py (GPU: the device against the reference).

The argmin contract (wave_ops.h row_argmin, wave_argmin64, qargmin): the lexicographic minimum of
(value, id) over the lanes whose value is not NaN; -0.0 == +0.0 (so the sign of a zero minimum is
not part of the contract); lanes that hold +INF carry id 0x7fffffff at every call site, so when
nothing is finite the result is (INF, 0x7fffffff)."""
import functools
import math
from fractions import Fraction

import numpy as np

EPS = float(np.finfo(np.float64).eps)  # 2^-52
NOID = 0x7FFFFFFF
TOL = 1e-10                            # the engine's default feasibility tolerance
ST_MAXITER, ST_INFEAS = 1, 2

# probe_prim op codes (unit_probe.hip)
OPS = ("bcast row_sum row_min row_min_i row_argmin pair_min16 pair_min32 pair_min_i16 pair_min_i32 "
       "pair_argmin16 pair_argmin32 wave_argmin64 row4_sum row4_sum2 row4_sum4 wave_sum64 qsum16 qsum64 "
       "qargmin16_m1 qargmin16_0 qargmin16_2 qargmin64 lane_next16 lane_next64 lane_prev16 lane_prev64 "
       "lane_next_i16 lane_next_i64 block_prefix16 block_prefix64 rcp_nr rsq_nr").split()
OP = {n: k for k, n in enumerate(OPS)}
OP_ROW_BCAST16 = 100


# ---------------------------------------------------------------------------------------------
# primitives
def argmin_ref(vals, ids):
    """(value, id): lexicographic minimum over the non-NaN entries (python compares -0.0 == 0.0)."""
    best = None
    for v, k in zip(vals, ids):
        v, k = float(v), int(k)
        if math.isnan(v):
            continue
        if best is None or (v, k) < best:
            best = (v, k)
    return best if best is not None else (math.inf, NOID)


def same_min_value(dev, ref):
    """Bitwise, except that a zero minimum may carry either sign."""
    dev, ref = float(dev), float(ref)
    if dev == 0.0 and ref == 0.0:
        return True
    return np.float64(dev).view(np.int64) == np.float64(ref).view(np.int64)


def argmin_matches(dev_v, dev_id, vals, ids):
    rv, rid = argmin_ref(vals, ids)
    return int(dev_id) == rid and same_min_value(dev_v, rv)


def sum_check(dev, vals, depth):
    """|dev - exact| <= depth * eps * sum|v|, the exact sums in rational arithmetic."""
    fr = [Fraction(float(v)) for v in vals]
    return abs(Fraction(float(dev)) - sum(fr)) <= depth * Fraction(EPS) * sum(abs(v) for v in fr)


def shift_ref(v, maxm, direction):
    """lane_next (direction +1: lane i receives lane i + 1) / lane_prev (-1).  MAXM <= 16: DPP row
    shifts, 0 at the 16-lane rows' edges.  MAXM > 16: __shfl_down / __shfl_up over the wave, whose
    edge lane keeps its own value."""
    v = np.asarray(v)
    out = np.zeros_like(v)
    for i in range(64):
        j = i + direction
        if maxm <= 16:
            out[i] = v[j] if 0 <= j < 64 and (j >> 4) == (i >> 4) else 0
        else:
            out[i] = v[j] if 0 <= j < 64 else v[i]
    return out


def block_prefix_terms(x, M, Nu):
    """lane -> the terms of its inclusive prefix sum within its MV block (lanes >= M: the lane alone)."""
    return [[float(x[j]) for j in range(i - (i % Nu), i + 1)] if i < M else [float(x[i])] for i in range(64)]


def ulp(x):
    return math.ulp(abs(float(x)))


def rcp_exact(x):
    return 1 / Fraction(float(x))


def rsq_exact(x):
    """1/sqrt(x) to 2^-100 relative as a Fraction: sqrt(d/n) = isqrt(d n 4^k) / (n 2^k)."""
    f = Fraction(float(x))
    n, d = f.numerator, f.denominator
    k = 120 + max(0, (n.bit_length() - d.bit_length()))
    return Fraction(math.isqrt(d * n << (2 * k)), n << k)


def ulps_off(dev, exact):
    """|dev - exact| in ulps of the correctly rounded result."""
    cr = float(exact)
    return float(abs(Fraction(float(dev)) - exact) / Fraction(ulp(cr)))


# ---------------------------------------------------------------------------------------------
# QP cases
SHAPES = {16: [(1, 1), (1, 2), (3, 1), (3, 5), (2, 8), (1, 9), (1, 16)],
          32: [(1, 17), (3, 10), (2, 16)],
          64: [(3, 11), (7, 9), (4, 16)]}
VARIANTS = {0: 16, 1: 32, 2: 64, 3: 16, 4: 16}   # probe_qp variant -> MAXM class
VARIANT_NAMES = {0: "gi_qp<16>", 1: "gi_qp<32>", 2: "gi_qp<64>", 3: "gi_qp16<false,void,false>",
                 4: "gi_qp16<true,void,true>"}
T_WARM = 12
REBUILD_WIDE = 8   # kGiRebuildWide (gpc_qp.h)


def default_maxit(M):
    return 8 * M + 16   # gpc_kernel.hip, gpc_small.hip


def make_R(M, seed):
    """Upper-triangular R with cond(R) <= 1e3 (singular values log-spaced over 10^0 .. 10^-2.5)."""
    rng = np.random.default_rng(seed)
    U, _ = np.linalg.qr(rng.standard_normal((M, M)))
    V, _ = np.linalg.qr(rng.standard_normal((M, M)))
    s = np.logspace(0.0, -2.5 * rng.uniform(0.3, 1.0), M) if M > 1 else np.ones(1)
    R = np.linalg.qr(U @ np.diag(s) @ V.T)[1]
    R = R * np.sign(np.diag(R))[:, None]
    return np.triu(R)


class Seq:
    """One sequence of T QPs sharing H = R'R and the bounds: min 1/2 (x - xu)'H(x - xu) subject to
    the rate / amplitude rows of oracle.toolbox_gpc.constraint_rows at u(t-1) = up[t]."""

    def __init__(self, name, nu, Nu, R, bnd, xu, up, maxit=None):
        self.name, self.nu, self.Nu, self.M = name, nu, Nu, nu * Nu
        self.R = R
        self.rinv = np.triu(np.linalg.inv(R))
        self.bnd = np.asarray(bnd, float).reshape(4, nu)       # dmin, dmax, umin, umax
        self.xu = np.asarray(xu, float).reshape(-1, self.M)
        self.up = np.asarray(up, float).reshape(-1, nu)
        self.T = self.xu.shape[0]
        self.maxit = default_maxit(self.M) if maxit is None else maxit
        self.cond = float(np.linalg.cond(R))

    def rows(self, t):
        from oracle.toolbox_gpc import constraint_rows

        return constraint_rows(self.nu, self.Nu, *self.bnd, self.up[t])

    def row_ids(self):
        """Device id 4 m + kind of every row of rows(t) (the l == 0 amplitude rows are merged into
        the rate box: kinds 2, 3 -> 0, 1)."""
        ids = []
        for n in range(self.nu):
            for l in range(self.Nu):
                m = n * self.Nu + l
                for kind, b in enumerate(self.bnd[:, n]):
                    if np.isfinite(b):
                        ids.append(4 * m + (kind & 1 if l == 0 else kind))
        return np.array(ids)

    @functools.lru_cache(maxsize=None)
    def solve(self, t):
        """The reference optimum of step t (cold), accepted only with the KKT check of
        tests/test_oracle_golden.py::test_primal_active_set_kkt.  Returns a dict."""
        from oracle.toolbox_gpc import qp_primal_active_set
        from scipy.optimize import nnls

        A, b = self.rows(t)
        x, it, W, mu = qp_primal_active_set(self.R, -self.R @ self.xu[t], A, b)
        s = A @ x - b
        assert s.min() > -1e-10, (self.name, t, s.min())
        H = self.R.T @ self.R
        g = H @ (x - self.xu[t])
        act = np.nonzero(s < 1e-9)[0]
        if len(act):
            lam, res = nnls(A[act].T, g)
            assert res < 1e-8 * max(1.0, np.abs(g).max()), (self.name, t, res)
        else:
            lam = np.zeros(0)
            assert np.abs(g).max() < 1e-8, (self.name, t)
        # spread of the optimum when every right-hand side moves by +-tol, on the active set found
        # (tol = 1e-10 does not change the set): dx = H^-1 N (N'H^-1 N)^+ (tol 1)
        spread = 0.0
        if len(act):
            N = A[act].T
            HiN = np.linalg.solve(H, N)
            dx = HiN @ np.linalg.lstsq(N.T @ HiN, TOL * np.ones(len(act)), rcond=None)[0]
            spread = float(np.abs(dx).max())
        scale = max(spread, self.cond * self.M * EPS * float(np.abs(x).max()))
        ids = self.row_ids()
        nondeg = bool(len(act) == 0 or (np.linalg.matrix_rank(A[act]) == len(act) and lam.min() > 1e-7 * max(1.0, lam.max())))
        return dict(x=x, slack=s, act=act, act_ids=frozenset(int(k) for k in ids[act]), lam=lam, scale=scale,
                    nondegenerate=nondeg, A=A, b=b)

    def min_slack(self, t, x):
        A, b = self.rows(t)
        return float((A @ x - b).min())


def _bounds(nu, dmax=1.0, umax=None, Nu=1):
    umax = 2.0 * Nu * dmax if umax is None else umax
    return np.array([[-dmax] * nu, [dmax] * nu, [-umax] * nu, [umax] * nu])


def _kkt_xu(R, xstar, normals, lam):
    """x_u that makes xstar the optimum with multipliers lam on `normals` (columns): H (x* - xu) = N lam."""
    H = R.T @ R
    return xstar - np.linalg.solve(H, normals @ lam)


def gen_feasible(nu, Nu, seed):
    """Step 0 puts constraints into the set; step 1's x_u is feasible (the retained set stays)."""
    M = nu * Nu
    rng = np.random.default_rng(seed)
    R = make_R(M, seed)
    xu0 = rng.uniform(1.5, 3.0, M) * rng.choice([-1.0, 1.0], M)
    xu1 = rng.uniform(-0.4, 0.4, M)
    return Seq("feasible", nu, Nu, R, _bounds(nu, Nu=Nu), [xu0, xu1], np.zeros((2, nu)))


def gen_cold(nu, Nu, k, seed):
    """Exactly k active rate bounds with strictly positive multipliers (strict complementarity)."""
    M = nu * Nu
    rng = np.random.default_rng(seed)
    R = make_R(M, seed)
    moves = rng.permutation(M)[:k]
    sg = rng.choice([-1.0, 1.0], k)              # +1: lower bound du >= -1 active, -1: upper
    xstar = rng.uniform(-0.6, 0.6, M)
    xstar[moves] = -sg
    N = np.zeros((M, k))
    N[moves, np.arange(k)] = sg
    xu = _kkt_xu(R, xstar, N, rng.uniform(0.5, 2.0, k))
    return Seq("cold%d" % k, nu, Nu, R, _bounds(nu, Nu=Nu), [xu], np.zeros((1, nu)))


def gen_warm(nu, Nu, seed, T=T_WARM):
    """x_u and u(t-1) drift so that rate and amplitude constraints enter and leave."""
    M = nu * Nu
    rng = np.random.default_rng(seed)
    R = make_R(M, seed)
    bnd = _bounds(nu, umax=1.5, Nu=Nu)
    ph = rng.uniform(0, 2 * np.pi, M)
    amp = rng.uniform(0.8, 2.5, M)
    xu = [amp * np.sin(ph + 0.9 * t) + 0.2 * rng.standard_normal(M) for t in range(T)]
    up = [np.clip(1.2 * np.sin(0.7 * t + np.arange(nu)), -1.5, 1.5) for t in range(T)]
    return Seq("warm", nu, Nu, R, bnd, xu, up)


def gen_rebuild_wide(nu, Nu, seed, T=None):
    """Small-M sequence whose active constraint flips every step: the set is never empty and every
    step adds (a rotation), so nrot passes kGiRebuildWide * M well inside T steps."""
    M = nu * Nu
    T = 4 * REBUILD_WIDE * M + 8 if T is None else T
    rng = np.random.default_rng(seed)
    R = make_R(M, seed)
    xu = [(2.0 + rng.uniform(0, 1, M)) * (1.0 if t % 2 == 0 else -1.0) * np.where(np.arange(M) % 2 == 0, 1.0, -1.0)
          for t in range(T)]
    return Seq("rebuild_wide", nu, Nu, R, _bounds(nu, Nu=Nu), xu, np.zeros((T, nu)))


def gen_degenerate(nu, Nu, seed):
    """Nu >= 2: u_max - u(t-1) = Nu * du_max exactly and the optimum has every move of block 0 on its
    upper rate bound: the block's last amplitude bound is active with them, and its normal is the sum
    of the rate normals (a dependent active normal; multipliers are not unique)."""
    assert Nu >= 2
    M = nu * Nu
    rng = np.random.default_rng(seed)
    R = make_R(M, seed)
    bnd = np.array([[-1.0] * nu, [1.0] * nu, [-4.0 * Nu] * nu, [float(Nu)] * nu])
    xstar = rng.uniform(-0.5, 0.5, M)
    xstar[:Nu] = 1.0
    N = np.zeros((M, Nu))
    N[np.arange(Nu), np.arange(Nu)] = -1.0
    xu = _kkt_xu(R, xstar, N, rng.uniform(0.5, 2.0, Nu))
    return Seq("degenerate", nu, Nu, R, bnd, [xu], np.zeros((1, nu)))


def gen_full(nu, Nu, seed):
    """Step 0: every move on its upper rate bound (q == M).  Step 1: the even moves' optimum is on the
    lower rate bound instead, so their upper bounds must be dropped from the full set."""
    M = nu * Nu
    rng = np.random.default_rng(seed)
    R = make_R(M, seed)
    xu0 = _kkt_xu(R, np.ones(M), -np.eye(M), rng.uniform(0.5, 2.0, M))
    sg = np.where(np.arange(M) % 2 == 0, 1.0, -1.0)     # +1: lower bound active, -1: upper
    xu1 = _kkt_xu(R, -sg, np.diag(sg), rng.uniform(0.5, 2.0, M))
    return Seq("full", nu, Nu, R, _bounds(nu, Nu=Nu), [xu0, xu1], np.zeros((2, nu)))


def gen_infeasible(nu, Nu, seed, kind):
    """kind 'amp': an amplitude bound out of reach of the rate bounds, u_min - u(t-1) > du_max (every
    amplitude row of the block carries the same bound, so the conflict shows in the merged l == 0 box
    first).  kind 'box': the l == 0 box of MV 0 has lo > hi from the rate bounds alone."""
    M = nu * Nu
    rng = np.random.default_rng(seed)
    R = make_R(M, seed)
    bnd = _bounds(nu, Nu=Nu)
    if kind == "amp":
        bnd[2, 0] = 1.5                           # u_min - 0 = 1.5 > du_max = 1
    else:
        bnd[0, 0], bnd[1, 0] = 0.5, -0.5          # du_min > du_max
    xu = rng.uniform(-0.5, 0.5, M)
    return Seq("infeasible_" + kind, nu, Nu, R, bnd, [xu], np.zeros((1, nu)))


def is_infeasible(seq, t=0):
    from scipy.optimize import linprog

    A, b = seq.rows(t)
    r = linprog(np.zeros(seq.M), A_ub=-A, b_ub=-b, bounds=[(None, None)] * seq.M, method="highs")
    return r.status == 2


@functools.lru_cache(maxsize=None)
def cases(maxm):
    """Every sequence of one MAXM class, by shape: {(nu, Nu): {kind: [Seq, ...]}}.  Seeds are fixed;
    a case the reference cannot solve is replaced by changing its seed here, never skipped."""
    out = {}
    for si, (nu, Nu) in enumerate(SHAPES[maxm]):
        M = nu * Nu
        base = 1000 * maxm + 100 * si
        d = dict(feasible=[gen_feasible(nu, Nu, base + 1)],
                 cold=[gen_cold(nu, Nu, k, base + 10 + k) for k in range(1, M)],
                 warm=[gen_warm(nu, Nu, base + 2), gen_warm(nu, Nu, base + 3)],
                 full=[gen_full(nu, Nu, base + 4)],
                 infeasible=[gen_infeasible(nu, Nu, base + 5, "box"), gen_infeasible(nu, Nu, base + 7, "amp")],
                 degenerate=[])
        if Nu >= 2:
            d["degenerate"].append(gen_degenerate(nu, Nu, base + 6))
        out[(nu, Nu)] = d
    return out


REBUILD_WIDE_SHAPES = [(1, 2), (3, 1)]


@functools.lru_cache(maxsize=None)
def rebuild_wide_cases():
    return {sh: gen_rebuild_wide(sh[0], sh[1], 7000 + k) for k, sh in enumerate(REBUILD_WIDE_SHAPES)}


def first_rebuild_step(seq, interval_M=1):
    """The first step at which a J rebuild must fire when the interval is interval_M * M rotations, or
    None: the step starts from a retained set, its x_u is infeasible, and at least interval_M * M adds
    have accumulated since J was last loaded from R^-1 (every id entering the reference's active set
    needs one add; an empty retained set reloads J at the next infeasible step)."""
    prev, cnt = frozenset(), 0
    for t in range(seq.T):
        infeasible = seq.min_slack(t, seq.xu[t]) < -TOL
        if infeasible and not prev:
            cnt = 0
        elif infeasible and cnt >= interval_M * seq.M:
            return t
        if infeasible:
            cur = seq.solve(t)["act_ids"]
            cnt += len(cur - prev)
            prev = cur
    return None


# ---------------------------------------------------------------------------------------------
# comparison helpers (their sensitivity is checked in tests/test_qp_units.py)
def x_ratio(seq, t, x_dev):
    """max|x_dev - x_ref| over the reference's scale (the device is allowed 8)."""
    r = seq.solve(t)
    return float(np.abs(np.asarray(x_dev) - r["x"]).max() / r["scale"])


def slack_floor(seq, x):
    return -TOL - seq.Nu * EPS * float(np.abs(x).sum())


# ---------------------------------------------------------------------------------------------
# factor updates (gi_core.h gi_add / gi_drop / gi_backsub, gpc_qp16.h gi16_add / gi16_drop)
FACTOR_SIZES = {16: [(4, 2), (15, 5), (16, 8)], 32: [(17, 17), (32, 16)], 64: [(33, 11), (64, 16)]}   # (M, Nu)
LD = np.longdouble


def normal_of(p, M, Nu):
    """Normal of constraint p = 4 m + kind (gi_core.h cinfo): kinds 0 / 1 the rate row +-e_m, kinds
    2 / 3 the amplitude row +-(sum of e_j over the MV block up to m)."""
    m, kind = p >> 2, p & 3
    n = np.zeros(M)
    n[(m if kind < 2 else (m // Nu) * Nu):m + 1] = -1.0 if kind & 1 else 1.0
    return n


class FactorRef:
    """float64 restatement of the J-form updates (gi_core.h's header comment): H^-1 = J J', J'N_A =
    [R_A; 0].  add: one Householder reflector on J(:, q:) mapping d(q:) = J(:, q:)'n_p onto alpha e_q,
    R_A gains the column [d(0:q); alpha].  drop: R_A loses column kd and is re-triangularised by
    Givens rotations of rows (jj, jj + 1), applied to J's columns (and B's, B = R_A^-1).  `flip`
    (negative control only): the index of one rotation whose sine is negated on J."""

    def __init__(self, rinv, Nu, flip=None):
        self.M, self.Nu = rinv.shape[0], Nu
        self.J = np.array(rinv, float)
        self.RA = np.zeros((0, 0))
        self.B = np.zeros((0, 0))
        self.ww, self.uw, self.nrot, self.nrotation, self.flip = [], [], 0, 0, flip

    def add(self, p, upm):
        q, J = len(self.ww), self.J
        d = J.T @ normal_of(p, self.M, self.Nu)
        beta = float(d[q:] @ d[q:])
        nrm = math.sqrt(beta)
        alpha = -nrm if d[q] > 0.0 else nrm
        v = d[q:].copy()
        v[0] -= alpha
        f = (J[:, q:] @ d[q:] - alpha * J[:, q]) / (beta - alpha * d[q])
        J[:, q:] -= np.outer(f, v)
        RA = np.zeros((q + 1, q + 1))
        RA[:q, :q] = self.RA
        RA[:q, q] = d[:q]
        RA[q, q] = alpha
        B = np.zeros((q + 1, q + 1))
        B[:q, :q] = self.B
        B[:q, q] = -(self.B @ d[:q]) / alpha
        B[q, q] = 1.0 / alpha
        self.RA, self.B = RA, B
        self.ww.append(p)
        self.uw.append(float(upm))
        self.nrot += 1
        return beta, float(d @ d)

    def drop(self, kd):
        q = len(self.ww)
        RA = np.delete(self.RA, kd, axis=1)
        B = np.delete(self.B, kd, axis=0)
        for jj in range(kd, q - 1):
            a, b = RA[jj, jj], RA[jj + 1, jj]
            rr = a * a + b * b
            if rr != 0.0:
                ri = 1.0 / math.sqrt(rr)
                cs, sn = a * ri, b * ri
                G = np.array([[cs, sn], [-sn, cs]])
                RA[jj:jj + 2, jj:] = G @ RA[jj:jj + 2, jj:]
                RA[jj + 1, jj] = 0.0
                B[:, jj:jj + 2] = B[:, jj:jj + 2] @ G.T
                if self.flip == self.nrotation:
                    G = np.array([[cs, -sn], [sn, cs]])
                self.J[:, jj:jj + 2] = self.J[:, jj:jj + 2] @ G.T
                self.nrot += 1
                self.nrotation += 1
        self.RA, self.B = RA[:q - 1], B[:, :q - 1]
        del self.ww[kd], self.uw[kd]

    def act(self):
        a = np.zeros(64, np.int64)
        for p in self.ww:
            a[p >> 2] |= 1 << (p & 3)
        return a


def factor_residuals(rinv, Nu, J, RA, ww, rdg=None, B=None, bs=None, rhs=None):
    """The invariants of one state, evaluated in numpy.longdouble, each as a relative residual:
    jj: |J J' - H^-1| / |H^-1|;  ra: |J'N_A - [R_A; 0]| / |R_A| with R_A's upper triangle (anything
    below it counts as residual);  rdg: max |rdg_i R_A(i, i) - 1|;  b: |B R_A - I|;  bs: |R_A r - c| /
    (|R_A| |r|) for r = gi_backsub(c).  Norms are Frobenius."""
    M, q = rinv.shape[0], len(ww)
    Jl, Ri = np.asarray(J, LD), np.asarray(rinv, LD)
    Hi = Ri @ Ri.T
    out = dict(jj=float(np.linalg.norm(Jl @ Jl.T - Hi) / np.linalg.norm(Hi)))
    if q:
        N = np.array([normal_of(p, M, Nu) for p in ww], LD).T
        Rl = np.asarray(RA, LD)[:q, :q]
        Ru = np.triu(Rl)
        full = np.zeros((M, q), LD)
        full[:q] = Ru
        nr = np.linalg.norm(Ru)
        out["ra"] = float(np.linalg.norm(Jl.T @ N - full) / nr)
        if rdg is not None:
            out["rdg"] = float(np.abs(np.asarray(rdg, LD)[:q] * np.diag(Ru) - 1).max())
        if B is not None:
            out["b"] = float(np.linalg.norm(np.asarray(B, LD)[:q, :q] @ Ru - np.eye(q, dtype=LD)))
        if bs is not None:
            r, c = np.asarray(bs, LD)[:q], np.asarray(rhs, LD)[:q]
            out["bs"] = float(np.linalg.norm(Ru @ r - c) / (nr * max(np.linalg.norm(r), LD(1e-300))))
    return out


def factor_script(M, Nu, seed):
    """[(kind, arg)]: kind 0 adds constraint id arg, kind 1 drops position arg.  One constraint per
    move at most (rate or amplitude kind at random), so every active set is independent.  Fill to
    q == M; drop position 0 and re-add the same id; drop q - 1 and re-add; drop positions 3, 7, 11, ..
    (the Givens chain then crosses columns 4b+3 -> 4b+4) and re-add each; then 2 M random adds and
    drops."""
    rng = np.random.default_rng(seed)
    script, ww, free = [], [], list(rng.permutation(M))

    def cid(m):
        kinds = [0, 1] + ([2, 3] if m % Nu else [])
        return 4 * int(m) + int(rng.choice(kinds))

    def add(p):
        script.append((0, p))
        ww.append(p)

    def drop(kd):
        script.append((1, kd))
        return ww.pop(kd)

    while free:
        add(cid(free.pop()))
    for kd in [0, M - 1] + list(range(3, M - 1, 4)):
        add(drop(kd))
    for _ in range(2 * M):
        if ww and (not free or rng.random() < 0.5):
            free.append(drop(int(rng.integers(len(ww)))) >> 2)
        else:
            add(cid(free.pop(int(rng.integers(len(free))))))
    return script


def crosses_block_boundary(kd, q):
    """The drop's chain jj = kd .. q - 2 rotates columns (4b + 3, 4b + 4) for some b."""
    return any(jj & 3 == 3 for jj in range(kd, q - 1))


@functools.lru_cache(maxsize=None)
def factor_case(M, Nu, seed, flip=None):
    """The script, R^-1, the right-hand side of gi_backsub and the restatement's state and residuals
    after every entry."""
    rinv = np.triu(np.linalg.inv(make_R(M, 9000 + seed)))
    rhs = np.random.default_rng(seed).standard_normal(64)
    script = factor_script(M, Nu, seed)
    ref, states = FactorRef(rinv, Nu, flip), []
    for e, (kind, arg) in enumerate(script):
        beta = ref.add(arg, e + 1)[0] if kind == 0 else (ref.drop(arg), 0.0)[1]
        q = len(ref.ww)
        rdg = 1.0 / np.diag(ref.RA) if q else np.zeros(0)
        bs = np.linalg.solve(ref.RA, rhs[:q]) if q else np.zeros(0)
        res = factor_residuals(rinv, Nu, ref.J, ref.RA, ref.ww, rdg, ref.B, bs, rhs)
        states.append(dict(ww=list(ref.ww), uw=list(ref.uw), act=ref.act(), q=q, nrot=ref.nrot, beta=beta,
                           res=res, J=ref.J.copy()))
    worst = {k: max(s["res"].get(k, 0.0) for s in states) for k in ("jj", "ra", "rdg", "b", "bs")}
    return dict(M=M, Nu=Nu, rinv=rinv, rhs=rhs, script=script, states=states, ref_worst=worst)


def factor_tolerance(case, key):
    """8 x the restatement's own worst residual over the script, never below M eps."""
    return max(8.0 * case["ref_worst"][key], case["M"] * EPS)
