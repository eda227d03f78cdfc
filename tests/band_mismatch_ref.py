"""Reference closed loop of the band controller on a plant that is not its model (test helper).

A numpy loop built from the oracle's own pieces (oracle/toolbox_band.py simulate, step_table,
dyn_matrix, band_qp), with the output-bias estimator the device states: at each step
the plant and the controller's model are simulated on the full input history, b = y - y_model is
added to the model's explicit free response on every row of its output, and band_qp is solved
there.  Nothing is carried from step to step except the applied inputs, so the loop shares no
arithmetic with the device's shifted window, its parallel-model recursion or its shifted bounds.
With plant == model it is closedloop_band (b = 0 exactly: the two simulations are the same call).
"""
import numpy as np

from oracle.matlab import DTF
from oracle.toolbox_band import band_qp, dyn_matrix, simulate, step_table
from oracle.toolbox_gpc import CLResult


def to_dtf(P):
    """A plant of mpct.lti.Tf (or oracle DTF) entries as oracle DTF entries, coefficients unchanged."""
    return [[e if isinstance(e, DTF) else DTF(np.array(e.num), np.array(e.den), int(e.delay)) for e in row]
            for row in P]


def _ba(P):
    return [[e.zinv_form() for e in row] for row in to_dtf(P)]


def _weights(sc, delta, lam):
    delta = np.abs(np.asarray(delta, dtype=float))
    lam = np.abs(np.asarray(lam, dtype=float))
    wq = (delta / sc.sy) ** 2 if sc.weights_squared else delta / sc.sy
    wl = (lam / sc.su) ** 2 if sc.weights_squared else lam / sc.su
    return wq, wl


def _free(ba_m, nu, U, t, N2, u_hold, v_hold):
    """Model prediction y(t+1..t+N2) with MVs held at u_hold from t, MDs at v_hold after t."""
    Uf = np.zeros((U.shape[0], t + N2 + 1))
    Uf[:, :t] = U[:, :t]
    Uf[:nu, t:] = u_hold[:, None]
    Uf[nu:, t:] = v_hold[:, None]
    return simulate(ba_m, Uf, t + N2 + 1)[:, t + 1:]


def closedloop_band_bias(sc, plant, r, v, N2, Nu, delta, lam, nit, trace=None, xtrace=None):
    """The closed loop of sc's controller (model sc.plant) on `plant` (my x nin entries) with the
    output-bias estimator.  r: my x nit, v: nd x nit.  Returns a CLResult (y, u, du_hist) with
    .bias (my x nit).  trace / xtrace: lists that receive every step's biased free response and QP
    solution [dU; eps]."""
    my, nu, nd, nin = sc.my, sc.nu, sc.nd, sc.nin
    r = np.asarray(r, dtype=float).reshape(my, nit)
    v = np.asarray(v, dtype=float).reshape(nd, nit)
    wq, wl = _weights(sc, delta, lam)
    ba_m, ba_p = sc.ba(), _ba(plant)
    G = dyn_matrix(step_table(sc, N2 + 2), nu, N2, Nu)
    U = np.zeros((nin, nit + N2 + 1))
    U[nu:, :nit] = v
    Y = np.zeros((my, nit))
    B = np.zeros((my, nit))
    DU = np.zeros((nu, nit))
    u_prev = np.zeros(nu)
    iters = 0
    for t in range(nit):
        Y[:, t] = simulate(ba_p, U, t + 1)[:, t]
        B[:, t] = Y[:, t] - simulate(ba_m, U, t + 1)[:, t]
        f = (_free(ba_m, nu, U, t, N2, u_prev, v[:, t]) + B[:, t][:, None]).reshape(-1)
        x, it = band_qp(sc, G, f, r[:, t], u_prev, N2, Nu, wq, wl)
        iters += it
        if trace is not None:
            trace.append(f.copy())
            xtrace.append(x.copy())
        DU[:, t] = [x[n * Nu] for n in range(nu)]
        u_prev = u_prev + DU[:, t]
        U[:nu, t] = u_prev
    res = CLResult(Y, U[:nu, :nit].copy(), None, None, iters, DU)
    res.bias = B
    return res


def replay_moves_bias(sc, plant, r, v, N2, Nu, delta, lam, U, T=None):
    """Per-step optimality check of an applied MV trajectory U (nu x nit): at every step the plant
    and model outputs, the bias and the free response are rebuilt from U[:, :t] and v, and the QP is
    solved there.  Returns (du_oracle, du_applied), both nu x T."""
    my, nu, nd, nin = sc.my, sc.nu, sc.nd, sc.nin
    nit = U.shape[1]
    T = nit if T is None else T
    r = np.asarray(r, dtype=float).reshape(my, nit)
    v = np.asarray(v, dtype=float).reshape(nd, nit)
    wq, wl = _weights(sc, delta, lam)
    ba_m, ba_p = sc.ba(), _ba(plant)
    G = dyn_matrix(step_table(sc, N2 + 2), nu, N2, Nu)
    Uall = np.zeros((nin, nit + N2 + 1))
    Uall[:nu, :nit] = U
    Uall[nu:, :nit] = v
    # the outputs at t depend on the inputs before t only through U (no feedthrough from an MV) and
    # on v(0..t): one simulation of each system over the whole applied history gives every step's bias
    Bias = simulate(ba_p, Uall, nit) - simulate(ba_m, Uall, nit)
    du_o = np.zeros((nu, T))
    du_a = np.zeros((nu, T))
    for t in range(T):
        u_prev = U[:, t - 1] if t > 0 else np.zeros(nu)
        f = (_free(ba_m, nu, Uall, t, N2, u_prev, v[:, t]) + Bias[:, t][:, None]).reshape(-1)
        x, _ = band_qp(sc, G, f, r[:, t], u_prev, N2, Nu, wq, wl)
        du_o[:, t] = [x[n * Nu] for n in range(nu)]
        du_a[:, t] = U[:, t] - u_prev
    return du_o, du_a


# --------------------------------------------------------------------------------------------
# The synthetic 2 x (1 MV + 1 MD) band plant of tests/host_tables/band_variants_check.cpp: a model of
# four first-order entries and three plants: 0 gains x 1.3, 1 entry (1, u) with a delay of 5 (the
# model's longest is 2), 2 entry (0, u) of second order with three numerator taps.  nit = 60 with
# ring lengths 8 (inputs) and 4 (entry outputs) wraps both rings several times, N2 <= 12 extends the
# window past every delay, and the disturbance step (v = 2 from t = 5) drives both outputs through
# their +-0.3 bands.
SYN_NIT = 60
SYN_NUM = [[0.0, 0.2], [0.05, 0.03], [0.0, 0.15], [0.0, 0.1]]
SYN_DEN = [[1.0, -0.8], [1.0, -0.7], [1.0, -0.9], [1.0, -0.6]]
SYN_DELAY = [1, 0, 2, 0]
SYN_CANDS = [(12, 3, np.zeros(2), np.array([0.3])), (7, 2, np.array([0.5, 1.0]), np.array([0.05])),
             (10, 1, np.zeros(2), np.array([2.0]))]


def synthetic_plants():
    """(model, [plant 0, plant 1, plant 2]) as 2 x 2 lists of mpct.lti.Tf."""
    from mpct.lti import Tf

    def grid(entries):
        return [[entries[0], entries[1]], [entries[2], entries[3]]]

    M = [Tf.make(SYN_NUM[e], SYN_DEN[e], SYN_DELAY[e]) for e in range(4)]
    V0 = [Tf.make([1.3 * x for x in SYN_NUM[e]], SYN_DEN[e], SYN_DELAY[e]) for e in range(4)]
    V1 = list(M)
    V1[2] = Tf.make(SYN_NUM[2], SYN_DEN[2], 5)
    V2 = list(M)
    V2[0] = Tf.make([0.1, 0.2, 0.05], [1.0, -1.3, 0.4], SYN_DELAY[0])
    return grid(M), [grid(V0), grid(V1), grid(V2)]


def synthetic_signals(nit=SYN_NIT):
    """(r, v, yref): a small setpoint step on output 0, the disturbance step, a zero Yref."""
    r = np.zeros((2, nit))
    r[0, 20:] = 0.1
    v = np.zeros((1, nit))
    v[0, 5:] = 2.0
    return r, v, np.zeros((2, nit))


def synthetic_scenario(plants=None, estimator="output_bias", nit=SYN_NIT, n2_max=12, nu_max=3):
    """The band scenario of the synthetic model on `plants` (None: the model itself, one plant)."""
    from mpct.engine import Scenario

    M, _ = synthetic_plants()
    plants = [M] if plants is None else plants
    bands = dict(y_min=np.full(2, -0.3), y_max=np.full(2, 0.3), ecr_min=np.ones(2), ecr_max=np.ones(2), rho=1e4)
    return Scenario(plants[0], M, nu=1, du_min=[-0.2], du_max=[0.2], u_min=[-1.0], u_max=[1.0],
                    yref=synthetic_signals(nit)[2], n2_max=n2_max, nu_max=nu_max, bands=bands,
                    plant_variants=plants if len(plants) > 1 else None, estimator=estimator)
