"""A family of small band scenarios whose MODEL entries are of higher order, one per branch of the
band kernel's window update (mdband_kernel.hip, "free-response window F_{t-1} -> F_t").

Every band scenario the other GPU tests build has first-order model entries: one tail value per
entry, a tail stride of 1, two numerator taps.  The cases below reach the tail shift, the tail
corrections at depth, a tail stride that is not the entry's own order, compact taps with zeros inside
and differing offsets, horizons shorter than an entry's order or delay, an integrating entry, rich
disturbances, the output-bias estimator on a second-order model and the 32-row QP instance.
tests/test_band_family.py pins each case to its branch with the layout probe and holds every
candidate to its named properties by the oracle alone; tests/test_band_family_gpu.py runs them on the
device.

Each case is written out as discrete entries (num, den, delay) with len(num) == len(den), descending
powers of z (tfdata form).  From them: product() builds the mpct.engine.Scenario through
mpct.lti.Tf.make, oracle() the oracle.toolbox_band.BandScenario through oracle.matlab.DTF.  No product
table reaches the oracle.

Signals (all cases but md_rich): the disturbance ramps up over steps 5..25 until, left alone, the
outputs would sit at about twice their band, and steps up once more at step 45.  A band-mode candidate
(delta = 0) does nothing until an output reaches its band, rides it from there (a band row active for
tens of steps) and meets the second step at the edge of the band, where the move it needs saturates
the rate bound.  The gentle candidate tracks r with weights on every output and a large lambda: it
keeps the outputs near r, and the second step, seen from there, stays inside the band, so none of
its QPs has an active row.  The setpoint of output 0 moves at step 55.

This is a plain module: no fixture, no conftest.
"""
from __future__ import annotations

import functools
from dataclasses import dataclass

import numpy as np

NIT = 70
ACT_TOL = 1e-9   # a row counts as active when its slack is below this (relative to max(1, |bound|))

# second / third order denominators: poles 0.8 +- 0.3i (|p| = 0.854), 0.75 +- 0.312i (|p| = 0.812)
DA = (1.0, -1.6, 0.73)
DB = (1.0, -1.5, 0.66)
D3 = (1.0, -2.2, 1.69, -0.438)    # DA times (1 - 0.6 z^-1)
DI = (1.0, -1.7, 0.7)             # (1 - z^-1)(1 - 0.7 z^-1): an integrator times a lag


def E(num, den, delay):
    assert len(num) == len(den)
    return (tuple(float(x) for x in num), tuple(float(x) for x in den), int(delay))


@dataclass(frozen=True)
class Case:
    name: str
    model: tuple                 # my x (nu + nd) entries (num, den, delay)
    nu: int
    y_band: tuple                # per output (y_min, y_max)
    du_max: tuple
    u_max: tuple
    cands: tuple                 # (N2, Nu, delta, lambda); candidate 0 is the gentle one
    n2_max: int
    nu_max: int
    v: tuple                     # nd rows of nit samples
    ecr: tuple = None            # per output MinECR = MaxECR (None: 1)
    plants: tuple = None         # est_*: the plant variants (each my x nin entries)
    nit: int = NIT

    @property
    def my(self):
        return len(self.model)

    @property
    def nin(self):
        return len(self.model[0])

    @property
    def nd(self):
        return self.nin - self.nu

    @property
    def est(self):
        return self.plants is not None

    @property
    def nvar(self):
        return len(self.plants) if self.plants else 1


def _ramp_step(level, step, nit=NIT, t0=5, t1=25, t2=45):
    v = np.zeros(nit)
    v[t0:t1] = level * (np.arange(t0, t1) - t0 + 1) / (t1 - t0)
    v[t1:] = level
    v[t2:] += step
    return tuple(v.tolist())


def setpoint(case):
    """r [my][nit]: output 0 moves at step 55."""
    r = np.zeros((case.my, case.nit))
    r[0, 55:] = 0.1
    return r


def _cands(my, nu, n2_max, order, reach, gentle_lam, extra=(), lams=(0.05, 0.05, 0.1, 0.02, 0.01)):
    """The horizons every case runs: N2 = 1, 2, the highest entry order (mz_na - 1), one below the
    longest delay plus taps (`reach`), n2_max; Nu = 1 and Nu = N2 at N2 = 1, 2."""
    z = (0.0,) * my
    lam = lambda x: (float(x),) * nu
    track0 = (1.0,) + (0.0,) * (my - 1)
    return ((n2_max, 2, (1.0,) * my, lam(gentle_lam)),
            (1, 1, z, lam(lams[0])),
            (2, 2, z, lam(lams[1])),
            (order, 1, z, lam(lams[2])),
            (reach - 1, 2, z, lam(lams[3])),
            (n2_max, 3, z, lam(lams[4])),
            (10, 2, track0, lam(0.3))) + tuple(extra)


def _cases():
    cs = []
    fo_v0 = E((0.0, 0.1), (1.0, -0.85), 1)
    fo_v1 = E((0.0, 0.12), (1.0, -0.8), 0)
    # ---- so2: every MV entry second order and underdamped, delays 0..3; the MD entries first order
    so2 = ((E((0.0, 0.08, 0.05), DA, 0), E((0.0, 0.03, 0.02), DB, 2), fo_v0),
           (E((0.0, 0.02, 0.03), DA, 3), E((0.0, 0.09, 0.04), DB, 1), fo_v1))
    v = (_ramp_step(1.2, 0.45),)
    bands2 = ((-0.4, 0.4), (-0.4, 0.4))
    cs.append(Case("so2", so2, 2, bands2, (0.08, 0.08), (2.0, 2.0), _cands(2, 2, 16, 2, 6, 6.0), 16, 3, v))
    # ---- to3_mixed: a third-order entry, second- and first-order ones beside it, output 2 all first
    # order: own order below the stride, tail shifts of depth 2.  Output 2's band is hard (ECR 0): the
    # oracle solves it at +-0.3 (its rows are in every QP and never bind); at +-0.25 the disturbance's
    # free response alone leaves the band at N2 = 16 and band_qp refuses the QP as infeasible
    m = ((E((0.0, 0.02, 0.02, 0.012), D3, 1), E((0.0, 0.03, 0.02), DB, 0), fo_v0),
         (E((0.0, 0.06), (1.0, -0.8), 2), E((0.0, 0.09, 0.04), DB, 1), fo_v1),
         (E((0.0, 0.05), (1.0, -0.7), 0), E((0.0, 0.04), (1.0, -0.75), 1), E((0.0, 0.02), (1.0, -0.9), 0)))
    cs.append(Case("to3_mixed", m, 2, bands2 + ((-0.3, 0.3),), (0.08, 0.08), (2.0, 2.0),
                   _cands(3, 2, 16, 3, 5, 6.0, lams=(0.3, 0.05, 0.1, 0.02, 0.01)), 16, 3, v, ecr=(1.0, 1.0, 0.0)))
    # ---- taps: numerators of 3 and 4 taps with a zero inside, a delay of 4 beside delay 0, an MD
    # with feedthrough
    m = ((E((0.0, 0.06, 0.0, 0.04), (1.0, -0.8, 0.0, 0.0), 0), E((0.05, 0.0, 0.03, 0.02), (1.0, -0.85, 0.0, 0.0), 4),
          fo_v0),
         (E((0.0, 0.03, 0.0, 0.05), DB + (0.0,), 1), E((0.0, 0.12), (1.0, -0.8), 0),
          E((0.04, 0.0, 0.08), (1.0, -0.8, 0.0), 0)))
    cs.append(Case("taps", m, 2, bands2, (0.08, 0.08), (2.0, 2.0), _cands(2, 2, 16, 3, 8, 6.0), 16, 3, v))
    # ---- integrator: b z^-1 / (1 - z^-1) times a lag on entry (0, u0)
    m = ((E((0.0, 0.03, 0.0), DI, 0), E((0.0, 0.05), (1.0, -0.8), 1), fo_v0),
         (E((0.0, 0.02, 0.03), DA, 2), E((0.0, 0.09, 0.04), DB, 1), fo_v1))
    cs.append(Case("integrator", m, 2, bands2, (0.08, 0.08), (2.0, 2.0), _cands(2, 2, 16, 2, 5, 6.0), 16, 3, v))
    # ---- md_rich: two disturbances through second-order entries; v0 is nonzero at t = 0, ramps over
    # 10 steps and steps twice in a row while the transient runs; v1 is a square pulse
    m = ((so2[0][0], so2[0][1], E((0.0, 0.05, 0.03), DB, 1), E((0.0, 0.02, 0.02), DA, 0)),
         (so2[1][0], E((0.0, 0.09, 0.04), DB, 0), E((0.0, 0.04, 0.04), DA, 0), E((0.0, 0.03, 0.01), DB, 2)))
    t = np.arange(NIT)
    v0 = 0.2 + 1.0 * np.clip((t - 9) / 10.0, 0.0, 1.0) + 0.3 * (t >= 40) + 0.3 * (t >= 43)
    v1 = 0.5 * ((t >= 22) & (t < 36))
    cs.append(Case("md_rich", m, 2, bands2, (0.08, 0.08), (2.0, 2.0), _cands(2, 2, 16, 2, 6, 6.0), 16, 3,
                   (tuple(v0.tolist()), tuple(v1.tolist()))))
    # ---- est_so2: the so2 model under the output-bias estimator on three plants: gains x 1.3, one
    # delay longer than the model's longest, one entry of another order
    g13 = tuple(tuple(E([1.3 * x for x in num], den, d) for num, den, d in row) for row in so2)
    dly = ((so2[0][0], so2[0][1], so2[0][2]), (so2[1][0], E(so2[1][1][0], so2[1][1][1], 5), so2[1][2]))
    ordr = ((so2[0][0], E((0.0, 0.1), (1.0, -0.68), 2), so2[0][2]), so2[1])
    cs.append(Case("est_so2", so2, 2, bands2, (0.08, 0.08), (2.0, 2.0),
                   _cands(2, 2, 16, 2, 6, 6.0, lams=(0.3, 0.05, 0.4, 0.02, 0.01)), 16, 3, v,
                   plants=(g13, dly, ordr)))
    # ---- wide: Nu = 8 on two MVs (Mz = 17, the 32-row QP instance) beside Mz <= 16 candidates
    z2 = (0.0, 0.0)
    cs.append(Case("wide", so2, 2, bands2, (0.08, 0.08), (2.0, 2.0),
                   _cands(2, 2, 16, 2, 6, 6.0, extra=((16, 8, z2, (0.02, 0.02)),)), 16, 8, v))
    return {c.name: c for c in cs}


CASES = _cases()
NAMES = tuple(CASES)
NOMINAL = tuple(n for n in NAMES if not CASES[n].est)


def signals(case):
    """(r [my][nit], v [nd][nit], yref [my][nit] = 0)."""
    return setpoint(case), np.array(case.v), np.zeros((case.my, case.nit))


def arrays(case, idx=None):
    """The candidates as eval_batch takes them: (N2, Nu, delta, lambda)."""
    c = case.cands if idx is None else [case.cands[i] for i in idx]
    return (np.array([x[0] for x in c], np.int32), np.array([x[1] for x in c], np.int32),
            np.array([x[2] for x in c], dtype=float), np.array([x[3] for x in c], dtype=float))


def _bands(case):
    ecr = np.ones(case.my) if case.ecr is None else np.array(case.ecr, dtype=float)
    return dict(y_min=np.array([b[0] for b in case.y_band]), y_max=np.array([b[1] for b in case.y_band]),
                ecr_min=ecr, ecr_max=ecr.copy(), rho=1e4)


def product_tfs(entries):
    from mpct.lti import Tf

    return [[Tf.make(list(num), list(den), delay) for num, den, delay in row] for row in entries]


def product(case, plants="all"):
    """The mpct.engine.Scenario of the case.  plants: "all" (the case's variants, or the model where
    it has none), or a list of plants (entries) for an estimator scenario on just those."""
    from mpct.engine import Scenario

    M = product_tfs(case.model)
    du, um = np.array(case.du_max), np.array(case.u_max)
    P = None
    if plants == "all":
        P = [product_tfs(p) for p in case.plants] if case.est else None
    elif plants is not None:
        P = [product_tfs(p) for p in plants]
    return Scenario(P[0] if P else M, M, nu=case.nu, du_min=-du, du_max=du, u_min=-um, u_max=um,
                    yref=np.zeros((case.my, case.nit)), n2_max=case.n2_max, nu_max=case.nu_max, bands=_bands(case),
                    plant_variants=P if P and len(P) > 1 else None, estimator="output_bias" if P else None)


def oracle_dtfs(entries):
    from oracle.matlab import DTF

    return [[DTF(np.array(num), np.array(den), delay) for num, den, delay in row] for row in entries]


def oracle(case):
    """The oracle.toolbox_band.BandScenario of the case (its model; plant variants go to
    band_mismatch_ref.closedloop_band_bias as oracle_dtfs(plant))."""
    from oracle.toolbox_band import BandScenario

    b = _bands(case)
    du, um = np.array(case.du_max), np.array(case.u_max)
    return BandScenario(plant=oracle_dtfs(case.model), nu=case.nu, du_min=-du, du_max=du, u_min=-um, u_max=um,
                        y_min=b["y_min"], y_max=b["y_max"], ecr_min=b["ecr_min"], ecr_max=b["ecr_max"],
                        sy=np.ones(case.my), su=np.ones(case.nu), rho=b["rho"])


def descriptor_text(case):
    """The case as the layout probe reads a band scenario (tests/host_tables/text_descriptor.h)."""
    out = ["band %d" % case.nd, "%d %d %d %d %d" % (case.my, case.nu, case.nit, case.n2_max, case.nu_max),
           " ".join(["1"] * case.my)]
    for _ in range(2):   # plant == model
        for row in case.model:
            for num, den, delay in row:
                out.append(" ".join([str(len(num))] + [repr(x) for x in num + den] + [str(delay)]))
    du, um = [float(x) for x in case.du_max], [float(x) for x in case.u_max]
    b = _bands(case)
    for vec in ([-x for x in du], du, [-x for x in um], um, b["y_min"], b["y_max"], b["ecr_min"], b["ecr_max"]):
        out.append(" ".join(repr(float(x)) for x in vec))
    out.append(repr(b["rho"]))
    return "\n".join(out) + "\n"


# ------------------------------------------------------------------------------------------------
def _trel(a, b):
    return float(np.max(np.abs(a - b)) / max(float(np.max(np.abs(b))), 1e-300))


def traj_err(y, u, ref):
    """The comparison of the GPU tests: the worst of y and u against a reference loop, each relative
    to the reference trajectory's peak."""
    return max(_trel(y, ref.y), _trel(u, ref.u))


def active_rows(osc, G, f, x, u_prev, N2, Nu):
    """(band rows, MV bound rows) active at the QP solution x = [dU; eps], by slack."""
    my, nu = osc.my, osc.nu
    M = nu * Nu
    dU, eps = x[:M], x[M]
    pred = (f + G @ dU).reshape(my, N2)
    nb = 0
    for i in range(my):
        up = osc.y_max[i] + eps * osc.ecr_max[i] * osc.sy[i] - pred[i]
        lo = pred[i] - (osc.y_min[i] - eps * osc.ecr_min[i] * osc.sy[i])
        nb += int(np.sum(up <= ACT_TOL * max(1.0, abs(osc.y_max[i])))) + int(np.sum(lo <= ACT_TOL * max(1.0, abs(osc.y_min[i]))))
    nm = 0
    for n in range(nu):
        d = dU[n * Nu:(n + 1) * Nu]
        uc = u_prev[n] + np.cumsum(d)
        nm += int(np.sum(osc.du_max[n] - d <= ACT_TOL)) + int(np.sum(d - osc.du_min[n] <= ACT_TOL))
        nm += int(np.sum(osc.u_max[n] - uc <= ACT_TOL * max(1.0, abs(osc.u_max[n]))))
        nm += int(np.sum(uc - osc.u_min[n] <= ACT_TOL * max(1.0, abs(osc.u_min[n]))))
    return nb, nm


@dataclass
class OracleLoop:
    res: object          # CLResult: y, u, du_hist (ys, uopt on nominal cases)
    f: np.ndarray        # nit x my*N2: the forward-simulated window every QP saw (bias included)
    x: np.ndarray        # nit x Mz
    band_steps: int      # steps with an active band row
    mv_steps: int        # steps with an active MV bound


@functools.lru_cache(maxsize=None)
def oracle_loop(name, k, var=0, lam_scale=1.0):
    """Candidate k of a case (on plant variant var of an estimator case) by the oracle alone:
    oracle.toolbox_band.closedloop_band, or tests/band_mismatch_ref.closedloop_band_bias.  Every QP
    passes band_qp's KKT check or the call raises.  Computed once per process, read-only."""
    from oracle.toolbox_band import closedloop_band, dyn_matrix, step_table

    import band_mismatch_ref as bm

    case = CASES[name]
    osc = oracle(case)
    r, v, _ = signals(case)
    N2, Nu, d, lam = case.cands[k]
    d, lam = np.array(d), np.array(lam) * lam_scale
    ft, xt = [], []
    if case.est:
        res = bm.closedloop_band_bias(osc, oracle_dtfs(case.plants[var]), r, v, N2, Nu, d, lam, case.nit, trace=ft, xtrace=xt)
    else:
        res = closedloop_band(osc, r, v, N2, Nu, d, lam, case.nit, open_loop=True, trace=ft, xtrace=xt)
    G = dyn_matrix(step_table(osc, N2 + 2), case.nu, N2, Nu)
    nb = nm = 0
    for t in range(case.nit):
        u_prev = res.u[:, t - 1] if t > 0 else np.zeros(case.nu)
        b, m = active_rows(osc, G, ft[t], xt[t], u_prev, N2, Nu)
        nb += int(b > 0)
        nm += int(m > 0)
    out = OracleLoop(res, np.array(ft), np.array(xt), nb, nm)
    for a in (res.y, res.u, res.du_hist, out.f, out.x):
        a.setflags(write=False)
    return out


def sensitivity(name, k, var=0):
    """The oracle's own response to a 1e-13 relative change of lambda: the change of its y and u,
    relative to their peaks (traj_err).  A loop that rides its constraints and switches between them
    amplifies rounding; a candidate whose reference moves by more than 1e-9 (100 x below the GPU
    tests' TRAJ_RTOL) cannot be compared by its free run, and the cases hold none."""
    a, b = oracle_loop(name, k, var), oracle_loop(name, k, var, 1.0 + 1e-13)
    return traj_err(b.res.y, b.res.u, a.res)


# ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def restated_loop(name, k, var=0, dtype=np.float64, fault=None):
    case = CASES[name]
    r, v, _ = signals(case)
    N2, Nu, d, lam = case.cands[k]
    import band_window_ref as bw

    return bw.closed_loop(oracle(case), case.model, r, v, N2, Nu, np.array(d), np.array(lam), case.nit, dtype=dtype,
                          fault=fault, plant=case.plants[var] if case.est else None)


@functools.lru_cache(maxsize=None)
def gentle_bound(name, var=0):
    """(bound, measured): the tolerance of the gentle candidate's trajectories, relative to their
    peak.  measured = the float64 restatement's closed loop against the longdouble one; the bound is
    8 x that (the margin the factor and prologue tests give a float64 restatement: the device's QP
    arithmetic and FMA contraction differ), and never below nit * (max taps + max na) * 2^-53."""
    case = CASES[name]
    a = restated_loop(name, 0, var)
    b = restated_loop(name, 0, var, np.longdouble)
    measured = traj_err(a.y, a.u, b)
    taps = max(len(num) + delay for P in (case.model,) + (case.plants or ()) for row in P for num, _, delay in row)
    na = max(len(den) for P in (case.model,) + (case.plants or ()) for row in P for _, den, _ in row)
    floor = case.nit * (taps + na) * 2.0 ** -53
    return max(8.0 * measured, floor), measured
