"""A family of small synthetic plants, one per plant-layout branch of the GPC kernels.

Every GPU parity test of the GPC kernels used the Shell 3x3 plant: nine first-order entries, integer
delays, my = nu = 3, plant == model.  The cases below reach what that plant cannot: the fourth term
row and the four-slot entry ring of gpc_small.hip, its other plant shapes, the deeper taps of the
general kernel's packed / register / LDS plant paths, more than 16 plant entries, and a plant that
differs from the controller's model.  tests/test_plant_family.py pins each case to its branch with
the host-only layout probe (tests/host_tables/layout_probe.cpp) and compares the kernels with the two
CPU references.

Each case is one list of continuous-time entries (num(s), den(s), delay) and one Ts.  It is
discretised twice: with mpct.lti.c2d into a product mpct.engine.Scenario (product()), and with
oracle.matlab.c2d_zoh into an oracle.toolbox_gpc.Scenario (oracle()), the way mpct/scenarios.py and
oracle/scenarios.py build Shell 3x3.  No product table reaches the oracle.

This is a plain module: no fixture, no conftest.
"""
from __future__ import annotations

import functools
from dataclasses import dataclass

import numpy as np

# second / third order denominators (descending powers of s), all underdamped or mixed
D2A = (4.0, 2.0, 1.0)        # wn = 0.50, zeta = 0.50
D2B = (9.0, 2.4, 1.0)        # wn = 0.33, zeta = 0.40
D2C = (2.25, 1.2, 1.0)       # wn = 0.67, zeta = 0.40
D2D = (6.25, 3.0, 1.0)       # wn = 0.40, zeta = 0.60
D3A = tuple(np.convolve((3.0, 1.0), (4.0, 1.6, 1.0)).tolist())   # pole -1/3 and wn = 0.5, zeta = 0.4


def fo(k, tau, delay):
    """K e^{-delay s} / (tau s + 1)"""
    return ((float(k),), (float(tau), 1.0), float(delay))


@dataclass(frozen=True)
class Case:
    name: str
    model: tuple                 # my x nu continuous entries (num, den, delay)
    steps: tuple                 # per output: (sample, level) of its setpoint step
    du_max: tuple
    u_min: tuple
    u_max: tuple
    N2: tuple
    Nu: tuple
    n2_max: int
    nu_max: int
    nit: int = 80
    Ts: float = 1.0
    seed: int = 20250307
    log_delta: tuple = (-1.0, 0.5)
    log_lambda: tuple = (-2.0, 0.5)
    gentle: tuple = (1.0, 10.0)  # candidate 0's (delta, lambda) on every output / MV: it stays off the bounds
    tau_ref: float = 3.0         # Yref = the setpoint through 1 / (tau_ref s + 1)
    plant: tuple = None          # None: the plant is the model
    # the branch the case exists to reach (the layout probe's answer, the kernel instances)
    small: int = 0
    regpath: int = 1
    sm_ke: int = 2
    ne_over_16: bool = False
    nominal: str = None          # *_mismatch cases: the case with the same model and plant == model

    @property
    def my(self):
        return len(self.model)

    @property
    def nu(self):
        return len(self.model[0])

    @property
    def plant_entries(self):
        return self.model if self.plant is None else self.plant

    @property
    def instances(self):
        """(cost-only, trajectory) answers of mpct_kernel_instance"""
        top = 16 if self.nu * self.nu_max <= 16 else 32 if self.nu * self.nu_max <= 32 else 64

        def general(ext):
            tail = ",false,true>" if ext else ",false,false>"
            names = ["gpc_closed_loop_kernel<16" + tail]
            c = 32
            while c <= top:
                names.append("<%d%s" % (c, tail))
                c *= 2
            return " + ".join(names)

        if self.small:
            assert top == 16
            return "gpc_small_kernel", general(True)
        return general(False), general(True)


def _mismatch(model, gains, taus):
    """The plant of a *_mismatch case: entry (i, j)'s gain times gains[i][j], and the denominator of
    entry (i, taus[i][0]) stretched in time by taus[i][1] (den(s) -> den(f s): every time constant of
    that entry times f).  Delays stay."""
    out = []
    for i, row in enumerate(model):
        prow = []
        for j, (num, den, delay) in enumerate(row):
            num = tuple(gains[i][j] * c for c in num)
            if j == taus[i][0]:
                f, n = taus[i][1], len(den) - 1
                den = tuple(c * f ** (n - k) for k, c in enumerate(den))
            prow.append((num, den, delay))
        out.append(tuple(prow))
    return tuple(out)


def _cases():
    cs = []
    # ---- gpc_small.hip, four terms per entry (2 numerator + 2 denominator taps) and ke = 4
    m = ((((1.0,), D2A, 2.0), ((1.5, 0.6), D2A, 1.0)),
         (((0.4,), D2B, 3.0), ((1.2,), D2B, 1.0)))
    small4 = Case("small_4term_ke4", m, steps=((5, 1.0), (30, -0.6)), du_max=(0.12, 0.12), u_min=(-1.64, -1.64),
                  u_max=(1.64, 1.64), N2=(12, 8, 16, 10, 14, 16, 9, 12), Nu=(2, 1, 8, 3, 5, 8, 4, 6), n2_max=16,
                  nu_max=8, small=1, sm_ke=4)
    cs.append(small4)
    # ---- gpc_small.hip, quad i = 3 and three MVs: first order, two poles per row (nyh = 12), one
    # zero-delay and one fractional-delay entry
    m = ((fo(1.0, 4.0, 2.0), fo(0.5, 7.0, 1.0), fo(0.3, 4.0, 3.0)),
         (fo(0.4, 5.0, 1.0), fo(1.2, 5.0, 0.0), fo(-0.3, 9.0, 2.0)),
         (fo(0.2, 6.0, 4.0), fo(0.5, 3.0, 1.5), fo(1.1, 3.0, 1.0)),
         (fo(0.6, 8.0, 1.0), fo(-0.4, 8.0, 2.0), fo(0.7, 5.0, 5.0)))
    cs.append(Case("small_4x3", m, steps=((5, 0.5), (20, 0.4), (35, 0.5), (50, 0.3)), du_max=(0.1, 0.1, 0.1),
                   u_min=(-0.9,) * 3, u_max=(0.9,) * 3, N2=(12, 6, 16, 10, 15, 8, 14, 16),
                   Nu=(2, 1, 5, 3, 4, 2, 5, 1), n2_max=16, nu_max=5, small=1))
    # ---- gpc_small.hip, 1 x 1 with the longest delay small_plant() takes (dum = 8 = kSmR)
    m = ((fo(1.5, 6.0, 8.0),),)
    cs.append(Case("small_siso", m, steps=((5, 1.0),), du_max=(0.1,), u_min=(-0.9,), u_max=(0.9,),
                   N2=(12, 16, 16, 10, 14, 9, 16, 13), Nu=(2, 16, 8, 1, 5, 3, 12, 13), n2_max=16, nu_max=16,
                   small=1))
    # ---- gpc_small.hip, 2 x 3 with first and second order entries in one row
    m = ((((1.0,), D2A, 1.0), fo(0.5, 5.0, 2.0), ((0.8, 0.5), D2A, 0.0)),
         (fo(0.6, 4.0, 1.0), fo(-0.5, 4.0, 0.5), ((1.2,), D2D, 2.0)))
    cs.append(Case("small_2x3", m, steps=((5, 1.0), (30, 0.7)), du_max=(0.1, 0.1, 0.1), u_min=(-0.8,) * 3,
                   u_max=(0.8,) * 3, N2=(12, 6, 16, 10, 15, 8, 14, 16), Nu=(2, 1, 5, 3, 4, 2, 5, 1), n2_max=16,
                   nu_max=5, small=1, sm_ke=4))
    # ---- general kernel, register / packed paths at depth: third and second order, fractional delays
    m = ((((1.0,), D3A, 1.4), ((0.7, 0.5), D2C, 2.5)),
         (((0.5,), D2B, 0.6), ((2.0, 0.9), D2B, 1.0)))
    deep = Case("packed_deep", m, steps=((5, 1.0), (30, -0.5)), du_max=(0.12, 0.12), u_min=(-1.85, -1.85),
                u_max=(1.85, 1.85), N2=(12, 16, 18, 20, 20, 10, 14, 20), Nu=(2, 8, 9, 16, 17, 1, 5, 12), n2_max=20,
                nu_max=17)
    cs.append(deep)
    # ---- general kernel, LDS path: a row of three distinct second-order entries (nyhi = 7 > kRegY)
    m = ((((1.0,), D2A, 1.0), ((0.6,), D2B, 2.0), ((0.5, 0.4), D2C, 0.0)),
         (fo(0.4, 5.0, 0.0), fo(0.9, 5.0, 1.0), fo(-0.3, 5.0, 2.0)))
    lds = Case("lds_path", m, steps=((5, 1.0), (30, 0.5)), du_max=(0.1, 0.1, 0.1), u_min=(-0.9,) * 3,
               u_max=(0.9,) * 3, N2=(12, 15, 16, 18, 18, 8, 14, 16), Nu=(2, 5, 6, 10, 11, 1, 3, 8), n2_max=18,
               nu_max=11, regpath=0, log_lambda=(-0.7, 0.7))
    cs.append(lds)
    # ---- general kernel, 20 plant entries: the <16> class cannot pack them
    taus = ((4.0, 7.0), (5.0, 9.0), (3.0, 6.0), (8.0, 5.0), (6.0, 4.0))
    gain = ((1.0, 0.3, -0.2, 0.4), (0.3, 1.1, 0.4, -0.2), (-0.3, 0.2, 0.9, 0.3), (0.2, -0.4, 0.3, 1.2),
            (0.5, 0.4, 0.3, 0.6))
    dly = ((1, 2, 0, 3), (2, 0, 1, 2), (3, 1, 1, 0), (0, 2, 3, 1), (2, 2, 1, 1))
    m = tuple(tuple(fo(gain[i][j], taus[i][j & 1], dly[i][j]) for j in range(4)) for i in range(5))
    cs.append(Case("many_entries", m, steps=((5, 0.5), (15, 0.4), (25, 0.5), (35, 0.3), (45, 0.4)),
                   du_max=(0.1,) * 4, u_min=(-1.2,) * 4, u_max=(1.2,) * 4, N2=(12, 10, 12, 14, 16, 8, 16, 12),
                   Nu=(2, 4, 5, 8, 9, 1, 6, 3), n2_max=16, nu_max=9, ne_over_16=True))
    # ---- plant != model: every gain 10-12 % off, one entry per row 10 % slower or faster, delays kept
    g2 = ((1.1, 1.12), (0.9, 0.88))
    cs.append(_with_plant(small4, _mismatch(small4.model, g2, ((0, 1.1), (1, 0.9)))))
    cs.append(_with_plant(deep, _mismatch(deep.model, g2, ((1, 1.1), (0, 0.9)))))
    g3 = ((1.1, 0.9, 1.1), (0.9, 1.1, 0.9))
    cs.append(_with_plant(lds, _mismatch(lds.model, g3, ((2, 1.1), (1, 0.9)))))
    return {c.name: c for c in cs}


def _with_plant(nominal, plant):
    kw = {k: getattr(nominal, k) for k in nominal.__dataclass_fields__}
    kw.update(name=nominal.name + "_mismatch", plant=plant, nominal=nominal.name)
    return Case(**kw)


CASES = _cases()
NAMES = tuple(CASES)
SMALL = tuple(n for n in NAMES if CASES[n].small)
MISMATCH = tuple(n for n in NAMES if CASES[n].nominal)


# ------------------------------------------------------------------------------------------------
def setpoint(case):
    """r [my][nit]: one step per output, each at its own sample."""
    r = np.zeros((case.my, case.nit))
    for i, (t0, level) in enumerate(case.steps):
        r[i, t0:] = level
    return r


def candidates(case):
    """(N2, Nu, delta, lambda): the case's horizons (one batch reaches every QP-size class the
    scenario has) with log-uniform weights from the case's seed, as mpct.scenarios.candidate_grid
    draws them; candidate 0 is a fixed gentle point, as the tuned point is there."""
    rng = np.random.default_rng(case.seed)
    C = len(case.N2)
    delta = 10.0 ** rng.uniform(*case.log_delta, size=(C, case.my))
    lam = 10.0 ** rng.uniform(*case.log_lambda, size=(C, case.nu))
    delta[0], lam[0] = case.gentle
    return np.array(case.N2, dtype=np.int32), np.array(case.Nu, dtype=np.int32), delta, lam


def product_tfs(case):
    """(plant, model) as my x nu lists of mpct.lti.Tf."""
    from mpct.lti import c2d

    def disc(entries):
        return [[c2d(list(num), list(den), case.Ts, delay) for (num, den, delay) in row] for row in entries]

    model = disc(case.model)
    return (model if case.plant is None else disc(case.plant)), model


def product_signals(case):
    from mpct.lti import c2d, lsim

    r = setpoint(case)
    ref = c2d([1.0], [case.tau_ref, 1.0], case.Ts, 0.0)
    return r, np.stack([lsim(ref, r[i]) for i in range(case.my)])


def product(case):
    """(mpct.engine.Scenario, r, yref) of the case: the product's own discretisation."""
    from mpct.engine import Scenario

    plant, model = product_tfs(case)
    r, yref = product_signals(case)
    du = np.array(case.du_max)
    sc = Scenario(plant, model, nu=case.nu, du_min=-du, du_max=du, u_min=np.array(case.u_min),
                  u_max=np.array(case.u_max), yref=yref, n2_max=case.n2_max, nu_max=case.nu_max, Ts=case.Ts)
    return sc, r, yref


def oracle(case):
    """(oracle.toolbox_gpc.Scenario, r, yref) of the case: the oracle's own discretisation."""
    from oracle.matlab import c2d_zoh, lsim_dtf
    from oracle.toolbox_gpc import Scenario

    def disc(entries):
        return [[c2d_zoh(list(num), list(den), case.Ts, delay) for (num, den, delay) in row] for row in entries]

    model = disc(case.model)
    plant = model if case.plant is None else disc(case.plant)
    du = np.array(case.du_max)
    sc = Scenario(plant=plant, model=model, nu=case.nu, du_min=-du, du_max=du, u_min=np.array(case.u_min),
                  u_max=np.array(case.u_max))
    r = setpoint(case)
    ref = c2d_zoh([1.0], [case.tau_ref, 1.0], case.Ts, 0.0)
    return sc, r, np.stack([lsim_dtf(ref, r[i]) for i in range(case.my)])


def descriptor_text(case):
    """The case as the layout probe reads it (tests/host_tables/layout_probe.cpp): whitespace-
    separated numbers,
        my nu nit n2_max nu_max
        n1[my]
        my*nu plant entries, row-major, each `len num[len] den[len] delay`
        my*nu model entries, the same way
        du_min[nu] du_max[nu] u_min[nu] u_max[nu]
    from the product's discretisation.  No CARIMA table: the library derives them from the model, as it
    does for the MATLAB host."""
    plant, model = product_tfs(case)
    out = ["%d %d %d %d %d" % (case.my, case.nu, case.nit, case.n2_max, case.nu_max), " ".join(["1"] * case.my)]
    for P in (plant, model):
        for row in P:
            for t in row:
                out.append(" ".join([str(len(t.num))] + [repr(float(x)) for x in t.num + t.den] + [str(t.delay)]))
    du = [float(x) for x in case.du_max]
    for v in ([-x for x in du], du, case.u_min, case.u_max):
        out.append(" ".join(repr(float(x)) for x in v))
    return "\n".join(out) + "\n"


# ------------------------------------------------------------------------------------------------
# the references, each computed once per process and shared by the tests that need it
@functools.lru_cache(maxsize=None)
def cport(name):
    """(CPort, oracle scenario, r, yref) of a case."""
    from oracle.cport import CPort

    case = CASES[name]
    osc, r, yref = oracle(case)
    return CPort(osc, case.n2_max, case.nit, yref), osc, r, yref


@functools.lru_cache(maxsize=None)
def cport_ext(name):
    """The C port's open-loop + trajectory results of every candidate of a case (read-only)."""
    cp, _, r, _ = cport(name)
    ref = cp.eval(*candidates(CASES[name]), r[None], open_loop=True, want_traj=True)
    for v in ref.values():
        v.setflags(write=False)
    return ref


@functools.lru_cache(maxsize=None)
def cport_costs(name):
    """The C port's cost-only results of every candidate of a case (read-only)."""
    cp, _, r, _ = cport(name)
    ref = cp.eval(*candidates(CASES[name]), r[None])
    for v in ref.values():
        v.setflags(write=False)
    return ref


@functools.lru_cache(maxsize=None)
def numpy_oracle(name, k):
    """Candidate k of a case through the numpy oracle (primal active-set QP; no table code shared
    with the product or the C port): a CLResult, read-only."""
    from oracle.toolbox_gpc import closedloop_toolbox

    case = CASES[name]
    _, osc, r, _ = cport(name)
    N2, Nu, d, l = candidates(case)
    o = closedloop_toolbox(osc, r, None, int(N2[k]), int(Nu[k]), d[k], l[k], case.nit, open_loop=True)
    for a in (o.y, o.u, o.ys, o.uopt, o.du_hist):
        a.setflags(write=False)
    return o
