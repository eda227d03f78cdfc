"""Scenario builders for the reference's driver scripts (product host code).

shell3x3(): MPC-Tuning/Shell3x3.m with caso = 2, nominal, rest = true — BASELINE config 2.
The CondMin scaling is taken from the committed tuning result (MPCTuning.m:155 CondMin's
fmincon optimum is not unique: cond() is scale invariant), transcribed below from
MPC-Tuning/Shell3x3_Tuning_25Jul2023_12_06.mat (Tuning_Parameters.scale.L / .R).
"""
from __future__ import annotations

import numpy as np

from .engine import Scenario
from .lti import c2d, fopdt_grid, lsim

# Shell3x3.m:52-57 nominal model, Ts, nit
SHELL3_K = np.array([[4.05, 1.77, 5.88], [5.39, 5.72, 6.9], [4.38, 4.42, 7.2]])
SHELL3_TAU = np.array([[50, 60, 50], [50, 60, 40], [33, 44, 19]], dtype=float)
SHELL3_DELAY = np.array([[27, 28, 27], [18, 14, 15], [20, 22, 0]], dtype=float)
SHELL3_TS, SHELL3_NIT = 4.0, 500
# Shell3x3_Tuning_25Jul2023_12_06.mat: Tuning_Parameters.scale (diagonals)
SHELL3_L = np.array([0.43577812475231503, 0.4205588479390135, 0.5932860051199568])
SHELL3_R = np.array([0.661867070834956, 0.2756082654542081, 0.41172304878568067])
# ... and the tuned point it stores (N=24, Nu=[6 2 2])
SHELL3_TUNED = dict(N=24, Nu=(6, 2, 2),
                    delta=(0.010659948215964849, 0.004019856475662751, 0.0007926546087416782),
                    lam=(9.247457388705409e-05, 0.0005523146971406108, 0.0015219790494510478))


def _shell_mc_plants(K, DK, TAU, DELAY, Ts, draws, seed, e_max, max_dshift, L, R):
    """The Shell model-error draws: gains K[i, j] + DK[i, j] * e_j, time constants and delays of the
    nominal model, scaled by L, R.  Draw 0 is the reference's case, e = e_max exactly and no delay
    shift; draws k >= 1 take e_j ~ U(-e_max_j, e_max_j) from numpy default_rng(seed), one number per
    column.  max_dshift > 0 adds U{0..max_dshift} * Ts to every entry's delay of the draws k >= 1, from
    a stream of its own (default_rng([seed, 1])), so the gains are the same for every max_dshift."""
    e_max = np.broadcast_to(np.asarray(e_max, dtype=float), (K.shape[1],))
    rng = np.random.default_rng(seed)
    rng_d = np.random.default_rng([seed, 1]) if max_dshift > 0 else None
    out = []
    for k in range(draws):
        e = e_max if k == 0 else rng.uniform(-e_max, e_max)
        sh = np.zeros(K.shape, dtype=int) if k == 0 or rng_d is None else rng_d.integers(0, max_dshift + 1, K.shape)
        out.append(fopdt_grid(K + DK * e[None, :], TAU, DELAY + sh * Ts, Ts, L, R))
    return out


def shell3x3_xsp(nit=SHELL3_NIT):
    """Setpoint of Shell3x3.m:89-92 (1-based inclusive ranges, later ones overwrite)."""
    X = np.zeros((3, max(nit, 500)))
    levels = [(0.2, 0.0, 0.1, 0.0), (0.2, 0.4, 0.3, 0.0), (0.2, 0.1, 0.0, 0.0)]
    for i, (a, b, c, d) in enumerate(levels):
        X[i, 9:80] = a
        X[i, 79:200] = b
        X[i, 199:400] = c
        X[i, 399:500] = d
    return X[:, :nit]


def shell3x3_yref(X, caso=2):
    """Yref = lsim(Pref, Xsp, t, 'zoh') (Shell3x3.m:71-76, 98-99)."""
    taus = (5.0, 9.0, 5.7) if caso == 1 else (30.0, 30.0, 30.0)
    delays = (27.0, 14.0, 0.0)
    return np.stack([lsim(c2d([1.0], [taus[i], 1.0], SHELL3_TS, delays[i]), X[i]) for i in range(3)])


def shell3x3_plant(L=SHELL3_L, R=SHELL3_R):
    """Pze = L * c2d(Ps, Ts, 'zoh') * R  (Shell3x3.m:65, MPCTuning.m:162)."""
    return fopdt_grid(SHELL3_K, SHELL3_TAU, SHELL3_DELAY, SHELL3_TS, L, R)


def _shell3x3_scenario(plant, n2_max, nu_max, nit, L, R, **kw):
    """What shell3x3 and shell3x3_mc share: the nominal model, bounds (Shell3x3.m:120-123 scaled by R,
    MPCTuning.m:170-178), r = L*Xsp and yref = L*Yref (MPCTuning.m:188-189).  plant None: the model."""
    P = shell3x3_plant(L, R)
    X = shell3x3_xsp(nit)
    yref = L[:, None] * shell3x3_yref(X)
    sc = Scenario(P if plant is None else plant, P, nu=3, du_min=-0.05 / R, du_max=0.05 / R, u_min=-1.0 / R,
                  u_max=0.5 / R, yref=yref, n2_max=n2_max, nu_max=nu_max, Ts=SHELL3_TS, **kw)
    return sc, L[:, None] * X, yref


def shell3x3(n2_max=30, nu_max=5, nit=SHELL3_NIT, L=SHELL3_L, R=SHELL3_R, window="toolbox",
             weights_squared=True, exact_carima=True):
    """Returns (Scenario, r, yref): r = L*Xsp, yref = L*Yref (MPCTuning.m:188-189) as row signals.
    Bounds: Shell3x3.m:120-123 scaled by R (MPCTuning.m:170-178)."""
    return _shell3x3_scenario(None, n2_max, nu_max, nit, L, R, window=window, weights_squared=weights_squared,
                              exact_carima=exact_carima)


# Shell3x3.m:43-45 "model error case": the simulated plant's gains are K + DK * e_j (column j)
SHELL3_DK = np.array([[2.11, 0.39, 0.59], [3.29, 0.57, 0.89], [3.11, 0.73, 1.33]])
SHELL3_EMAX = (0.2, 0.2, 0.3)   # Shell3x3.m:38 (nominal = false)


def shell3x3_mc_plants(draws, seed=20250307, e_max=SHELL3_EMAX, max_dshift=0, L=SHELL3_L, R=SHELL3_R):
    """Plant-mismatch draws around Shell3x3.m's model error case (:34-48), three e_j per draw
    (_shell_mc_plants).  e = 0 gives shell3x3_plant.  Returns a list of 3x3 plants (mpct.lti.Tf)."""
    return _shell_mc_plants(SHELL3_K, SHELL3_DK, SHELL3_TAU, SHELL3_DELAY, SHELL3_TS, draws, seed, e_max, max_dshift, L, R)


def shell3x3_mc(draws=8, n2_max=30, nu_max=5, nit=SHELL3_NIT, seed=20250307, e_max=SHELL3_EMAX, max_dshift=0,
                L=SHELL3_L, R=SHELL3_R):
    """The constrained Shell 3x3 loop of shell3x3() over `draws` mismatched plants (shell3x3_mc_plants;
    variant k runs with reference row k): the controller keeps the nominal model, bounds and Yref are
    those of shell3x3().  Returns (Scenario, refs [draws, 3, nit], plants)."""
    plants = shell3x3_mc_plants(draws, seed, e_max, max_dshift, L, R)
    sc, r, _ = _shell3x3_scenario(plants[0], n2_max, nu_max, nit, L, R, window="toolbox", plant_variants=plants)
    return sc, np.broadcast_to(r, (draws, 3, nit)).copy(), plants


def vns_step_refs(my, nit, inK=10):
    """VNS2.m:58-61 + 147-150: one simulation per output with a unit step on that output."""
    R = np.zeros((my, my, nit))
    for i in range(my):
        R[i, i, inK - 1:] = 1.0
    return R


def candidate_grid(C=4096, my=3, nu=3, N2=30, Nu=5, seed=20250307, tuned=SHELL3_TUNED):
    """BASELINE config 2 grid: log10 delta ~ U(-4,0), log10 lambda ~ U(-5,-1),
    numpy default_rng(20250307); candidate 0 is the fixture-tuned (delta, lambda) at N2, Nu."""
    rng = np.random.default_rng(seed)
    delta = 10.0 ** rng.uniform(-4, 0, size=(C, my))
    lam = 10.0 ** rng.uniform(-5, -1, size=(C, nu))
    if tuned is not None and C > 0:
        delta[0] = tuned["delta"]
        lam[0] = tuned["lam"]
    return (np.full(C, N2, dtype=np.int32), np.full(C, Nu, dtype=np.int32), delta, lam)


# ---------------------------------------------------------------------------------------------
# Shell 7x5 (config 3): MPC-Tuning/Shell7x5.m, nominal (e1..e5 = 0, :38-43).  [Gs Ds] of
# Shell7x5.m:73-91 (3 MVs, 2 measured disturbances), Ts = 4, nit = 200.  Scaling from the
# committed Shell7x5_Tuning_14Sep2024_14_22.mat (Tuning_Parameters.scale), which also holds the
# tuned point below.
SHELL7_K = np.array([[4.05, 1.77, 5.88, 1.20, 1.44], [5.39, 5.72, 6.9, 1.52, 1.83],
                     [3.66, 1.65, 5.53, 1.16, 1.27], [5.92, 2.54, 8.10, 1.73, 1.79],
                     [4.13, 2.38, 6.23, 1.31, 1.26], [4.06, 4.18, 6.53, 1.19, 1.17],
                     [4.38, 4.42, 7.2, 1.14, 1.26]])
SHELL7_TAU = np.array([[50, 60, 50, 45, 40], [50, 60, 40, 25, 20], [9, 30, 40, 11, 6],
                       [12, 27, 20, 5, 19], [8, 19, 10, 2, 22], [13, 33, 9, 19, 24],
                       [33, 44, 19, 24, 32]], dtype=float)
SHELL7_DELAY = np.array([[27, 28, 27, 27, 27], [18, 14, 15, 15, 15], [2, 20, 2, 0, 0], [11, 12, 2, 0, 0],
                         [5, 7, 2, 0, 0], [8, 4, 1, 0, 0], [20, 22, 0, 0, 0]], dtype=float)
SHELL7_TS, SHELL7_NIT = 4.0, 200
SHELL7_YMX = np.array([0.005, 0.005, 0.5, 0.5, 0.5, 0.5, 0.5])   # Shell7x5.m:106-107
SHELL7_ECR = np.array([0.1, 0.5, 1, 1, 1, 1, 1])                   # Shell7x5.m:143-152
SHELL7_L = np.array([0.4400615063022943, 0.2319273262887009, 0.6265090010777253, 0.5431290766409146,
                     0.6006058918173808, 0.20692945405215463, 0.39416907820719865])
SHELL7_R = np.array([0.2639712478155768, 0.1350971290956903, 0.1156440799331315, 0.781865375367461,
                     0.4665315477471682])
SHELL7_TUNED = dict(N=27, Nu=(2, 2, 2), delta=(0.0,) * 7,
                    lam=(0.055949075594369936, 0.016702486485524682, 1.6101890690935143))
SHELL7_W = np.array([1e-4, 1e-4, 1, 0.5, 1, 0.5, 1])               # Shell7x5.m:202 (GAM weights)


CONFIG3_N2 = (16, 24, 32, 48, 64, 96, 112, 127)
CONFIG3_NU = (2, 3, 4, 6, 8, 10, 12, 15)


def config3_grid(per=1024, seed=20250307):
    """BASELINE config 3 grid: N2 x Nu cells (N2-major, 64 cells) x ``per``
    lambda draws log10 U(-3, 1) (numpy default_rng(seed)), delta = 0 (band mode, Shell7x5.m:190).
    Candidate c sits in cell c // per: N2 = CONFIG3_N2[cell // 8], Nu = CONFIG3_NU[cell % 8]."""
    rng = np.random.default_rng(seed)
    N2 = np.repeat(np.array([n for n in CONFIG3_N2 for _ in CONFIG3_NU], np.int32), per)
    Nu = np.repeat(np.array([u for _ in CONFIG3_N2 for u in CONFIG3_NU], np.int32), per)
    lam = 10.0 ** rng.uniform(-3, 1, size=(N2.size, 3))
    return N2, Nu, np.zeros((N2.size, 7)), lam


def config3_stratified(per_cell=128, per=1024):
    """Indices of the first ``per_cell`` lambda draws of every config-3 cell (the parity sample)."""
    return (np.arange(64)[:, None] * per + np.arange(per_cell)[None, :]).ravel()


def shell7x5_plant(L=SHELL7_L, R=SHELL7_R):
    """Pze = L * c2d([Gs Ds], Ts, 'zoh') * R  (Shell7x5.m:93-98, MPCTuning.m:162)."""
    return fopdt_grid(SHELL7_K, SHELL7_TAU, SHELL7_DELAY, SHELL7_TS, L, R)


def shell7x5_signals(nit=SHELL7_NIT, tmd=20, L=SHELL7_L, R=SHELL7_R):
    """(r, v, yref): r = L*Xsp = 0 (Shell7x5.m:118), v = Rv\\mdv with mdv = 0.5 from tmd
    (:121-123, MPCTuning.m:191), yref = L*lsim(Pref, Xref) with Xref(i, tmd:tmd+5) = Ymx(i) and
    Pref = 1/(50s+1) delayed by min over row i of [Gs Ds].iodelay (:126-135, MPCTuning.m:188)."""
    X = np.zeros((7, nit))
    X[:, tmd - 1: tmd + 5] = SHELL7_YMX[:, None]
    dl = SHELL7_DELAY.min(axis=1)
    Yref = np.stack([lsim(c2d([1.0], [50.0, 1.0], SHELL7_TS, dl[i]), X[i]) for i in range(7)])
    mdv = np.zeros((2, nit))
    mdv[:, tmd - 1:] = 0.5
    return np.zeros((7, nit)), mdv / R[3:, None], L[:, None] * Yref


def _shell7x5_scenario(plant, n2_max, nu_max, nit, L, R, **kw):
    """What shell7x5 and shell7x5_mc share: the nominal model, signals, MV bounds and output bands
    (see shell7x5).  plant None: the model.  Returns (Scenario, r, v, yref)."""
    P = shell7x5_plant(L, R)
    r, v, yref = shell7x5_signals(nit, L=L, R=R)
    umx = 0.5 / R[:3]
    yr = 2 * SHELL7_YMX
    bands = dict(y_min=-L * SHELL7_YMX, y_max=L * SHELL7_YMX, ecr_min=SHELL7_ECR, ecr_max=SHELL7_ECR,
                 y_scale=np.where(yr != 1.0, L * yr, yr), u_scale=np.ones(3), rho=1e4)
    inf = np.full(3, np.inf)
    sc = Scenario(P if plant is None else plant, P, nu=3, du_min=-inf, du_max=inf, u_min=-umx, u_max=umx, yref=yref,
                  n2_max=n2_max, nu_max=nu_max, Ts=SHELL7_TS, window="toolbox", bands=bands, **kw)
    return sc, r, v, yref


def shell7x5(n2_max=127, nu_max=15, nit=SHELL7_NIT, L=SHELL7_L, R=SHELL7_R):
    """Returns (Scenario, r, v, yref) for the toolbox MPC of Shell7x5.m after MPCTuning's
    scaling: MV bounds +-0.5/R (:110-111, 135-138; no rate bounds), soft OV bands L*Ymn..L*Ymx
    with MinECR/MaxECR (:141-152), OV ScaleFactor = L*Yrange unless Yrange == 1 (:162-168,
    MPCTuning.m:182-184), MV ScaleFactor 1 (Urange = 1), Weights.ECR = 1e4 (:191)."""
    return _shell7x5_scenario(None, n2_max, nu_max, nit, L, R)


# Shell7x5.m:46-62 "model error case": the simulated plant's gains are K + DK * e_j (column j of
# [Gr Dr], the two disturbance columns included)
SHELL7_DK = np.array([[2.11, 0.39, 0.59, 0.12, 0.16], [3.29, 0.57, 0.89, 0.13, 0.13],
                      [2.29, 0.35, 0.67, 0.08, 0.08], [2.34, 0.24, 0.32, 0.02, 0.04],
                      [1.71, 0.93, 0.30, 0.03, 0.02], [2.39, 0.35, 0.72, 0.08, 0.01],
                      [3.11, 0.73, 1.33, 0.18, 0.10]])
SHELL7_EMAX = (0.2, 0.2, 0.3, 0.5, 0.5)   # Shell7x5.m:41 (nominal = false)


def shell7x5_mc_plants(draws, seed=20250307, e_max=SHELL7_EMAX, max_dshift=0, L=SHELL7_L, R=SHELL7_R):
    """Plant-mismatch draws around Shell7x5.m's model error case (:38-63), five e_j per draw over all
    columns of [Gr Dr] (_shell_mc_plants).  e = 0 gives shell7x5_plant.  Returns a list of 7x5 plants."""
    return _shell_mc_plants(SHELL7_K, SHELL7_DK, SHELL7_TAU, SHELL7_DELAY, SHELL7_TS, draws, seed, e_max, max_dshift, L, R)


def shell7x5_mc(draws=8, n2_max=127, nu_max=15, nit=SHELL7_NIT, seed=20250307, e_max=SHELL7_EMAX, max_dshift=0,
                L=SHELL7_L, R=SHELL7_R):
    """The Shell 7x5 band loop of shell7x5() over `draws` mismatched plants (shell7x5_mc_plants; variant
    k runs with signal row k): the controller keeps the nominal model [Gs Ds] and corrects its
    prediction by the output-bias estimator (Shell7x5.m:302-303 simulates with options.Model = plant;
    the toolbox's own estimator is not restated); bounds, bands and Yref are those of
    shell7x5().  Returns (Scenario, r [draws, 7, nit], v [draws, 2, nit], yref, plants)."""
    plants = shell7x5_mc_plants(draws, seed, e_max, max_dshift, L, R)
    sc, r, v, yref = _shell7x5_scenario(plants[0], n2_max, nu_max, nit, L, R, plant_variants=plants,
                                        estimator="output_bias")
    return sc, np.broadcast_to(r, (draws, 7, nit)).copy(), np.broadcast_to(v, (draws, 2, nit)).copy(), yref, plants


# ---------------------------------------------------------------------------------------------
# WoodBerry.m (toolbox MPC, caso = 1, nominal, rest = true): [Gs Ds] with one measured
# disturbance, Ts = 1, nit = 400.  The reference commits no WoodBerry tuning .mat, so CondMin's
# scaling is not pinned: L = R = I unless given.
WB_K = np.array([[12.8, -18.9, 3.8], [6.6, -19.4, 4.9]])          # WoodBerry.m:48-52
WB_TAU = np.array([[16.7, 21.0, 14.9], [10.9, 14.4, 13.2]])
WB_DELAY = np.array([[1.0, 2.0, 8.1], [2.0, 1.0, 3.4]])
WB_W = np.array([0.1, 0.5])                                        # WoodBerry.m:155


def _woodberry_scenario(plant, n2_max, nu_max, nit, caso, L, R, **kw):
    """What woodberry_toolbox and woodberry_toolbox_mc share: the nominal model, signals and bounds
    (see woodberry_toolbox).  plant None: the model.  Returns (Scenario, r, v, yref)."""
    P = fopdt_grid(WB_K, WB_TAU, WB_DELAY, 1.0, L, R)
    X = np.zeros((2, nit))
    X[0, 9:] = 0.8
    X[1, 199:] = 0.5
    taus = (10.0, 7.0) if caso == 1 else (15.0, 12.0)
    Yref = np.stack([lsim(c2d([1.0], [taus[i], 1.0], 1.0, 1.0), X[i]) for i in range(2)])
    mdv = np.zeros((1, nit))
    mdv[0, 299:] = -0.25
    Ru = R[:2]
    sc = Scenario(P if plant is None else plant, P, nu=2, du_min=-0.05 / Ru, du_max=0.05 / Ru, u_min=-0.5 / Ru,
                  u_max=0.5 / Ru, yref=L[:, None] * Yref, n2_max=n2_max, nu_max=nu_max, Ts=1.0, window="toolbox", **kw)
    return sc, L[:, None] * X, mdv / R[2:, None], L[:, None] * Yref


def woodberry_toolbox(n2_max=30, nu_max=10, nit=400, caso=1, L=np.ones(2), R=np.ones(3)):
    """Returns (Scenario, r, v, yref) of WoodBerry.m:43-148: rate bounds +-0.05, amplitude
    +-0.5 (:118-134, scaled by R), unbounded outputs; Xsp(1, 10:) = 0.8, Xsp(2, 200:) = 0.5
    (:87-89); mdv(300:) = -0.25 (:92-94); Yref = lsim(Pref, Xsp) with Pref diag(1/(10s+1),
    1/(7s+1)) (caso 1) or diag(1/(15s+1), 1/(12s+1)), delays [1, 1] (:69-75, :98)."""
    return _woodberry_scenario(None, n2_max, nu_max, nit, caso, L, R)


WB_DELTAK, WB_DELTAL = 0.2, 1.0   # WoodBerry.m:40-41 (nominal = false)


def woodberry_mc_plants(draws, seed=20250307, dk_max=WB_DELTAK, max_dshift=int(WB_DELTAL), L=np.ones(2), R=np.ones(3)):
    """Plant-mismatch draws around WoodBerry.m's model error case (:34-46): the MV gains of Gs times
    (1 + dk) and the MV delays plus dL samples, the disturbance column Ds unchanged.  Draw 0 is the
    reference's case (dk = dk_max, dL = max_dshift); draws k >= 1 take dk ~ U(-dk_max, dk_max) from
    numpy default_rng(seed) and dL ~ U{0..max_dshift} from default_rng([seed, 1]), one number each
    per draw.  dk_max = 0, max_dshift = 0 gives the nominal plant.  Returns a list of 2x3 plants.

    Not mpct.dtc.woodberry_mc_plants (config 4, DTC_GPC_WW.m): that one draws the 2x2 MV block alone,
    a gain factor and a delay shift per entry, both from one stream default_rng(seed), and has no
    reference draw 0; here one dk and one dL move the whole MV block and the streams are two."""
    rng = np.random.default_rng(seed)
    rng_d = np.random.default_rng([seed, 1])
    mv = np.array([1.0, 1.0, 0.0])[None, :]   # the MV columns of [Gs Ds]
    out = []
    for k in range(draws):
        dk = dk_max if k == 0 else rng.uniform(-dk_max, dk_max)
        dl = max_dshift if k == 0 else int(rng_d.integers(0, max_dshift + 1))
        out.append(fopdt_grid(WB_K * (1.0 + dk * mv), WB_TAU, WB_DELAY + dl * mv, 1.0, L, R))
    return out


def woodberry_toolbox_mc(draws=8, n2_max=30, nu_max=10, nit=400, caso=1, seed=20250307, dk_max=WB_DELTAK,
                         max_dshift=int(WB_DELTAL), L=np.ones(2), R=np.ones(3)):
    """WoodBerry.m's toolbox MPC of woodberry_toolbox() over `draws` mismatched plants
    (woodberry_mc_plants; WoodBerry.m:272-273 simulates with options.Model = plant): nominal model,
    output-bias estimator.  Returns (Scenario, r [draws, 2, nit], v [draws, 1, nit], yref, plants)."""
    plants = woodberry_mc_plants(draws, seed, dk_max, max_dshift, L, R)
    sc, r, v, yref = _woodberry_scenario(plants[0], n2_max, nu_max, nit, caso, L, R, plant_variants=plants,
                                         estimator="output_bias")
    return sc, np.broadcast_to(r, (draws, 2, nit)).copy(), np.broadcast_to(v, (draws, 1, nit)).copy(), yref, plants
