"""The band-scenario family of tests/band_family.py on the GPU (-m gpu): mdband_closed_loop_kernel on
model entries of second and third order, through engine.eval_batch(..., want_traj=True).

The truth is the oracle's forward-simulated loop (oracle/toolbox_band.py closedloop_band / replay_moves;
tests/band_mismatch_ref.py for the estimator case), computed once per process in band_family.oracle_loop.
No candidate and no step is left out: tests/test_band_family.py holds the inputs to what makes that
possible.  Tolerances: the band tests' own (tests/test_band.py) on the constrained candidates; on the
gentle candidate (a linear loop) band_family.gentle_bound, 8 x the float64 restatement's own distance
from its longdouble twin and never below nit * (taps + na) * 2^-53.
"""
import numpy as np
import pytest

import band_family as bf
import band_mismatch_ref as bm

TRAJ_RTOL = 1e-7      # free-run trajectories, relative to the trajectory's peak
REPLAY_RTOL = 1e-6    # per-step first moves at the device's own states, relative to max |du|
COST_RTOL = 1e-6      # BASELINE tolerance on the costs
INK0 = 9              # vns_ink - 1: j22 sums from here


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int64 if a.dtype == np.float64 else a.dtype)


@pytest.fixture(scope="module")
def gpu(built, has_gpu):
    if not has_gpu:
        pytest.skip("no GPU")
    return True


def _run(case, sc, idx=None, open_loop=False):
    from mpct.engine import eval_batch

    r, v, _ = bf.signals(case)
    n = sc.nplant
    return eval_batch(sc, *bf.arrays(case, idx), np.broadcast_to(r, (n,) + r.shape), v=np.broadcast_to(v, (n,) + v.shape),
                      open_loop=open_loop, want_traj=True)


@pytest.fixture(scope="module")
def runs(gpu):
    """One launch per case, all candidates (x plant variants), with trajectories; the open-loop leg
    on the cases without an estimator.  Shared by the tests below, never modified."""
    cache = {}

    def get(name):
        if name not in cache:
            case = bf.CASES[name]
            sc = bf.product(case)
            cache[name] = (sc, _run(case, sc, open_loop=not case.est))
        return cache[name]

    return get


@pytest.mark.gpu
@pytest.mark.parametrize("name", bf.NAMES)
def test_against_oracle(runs, name):
    """Every status 0; y and u of every candidate (on every plant variant) against the oracle's closed
    loop; J1 and j22 against its sums; the open-loop ys / uopt (one QP from rest) where there is no
    estimator."""
    case = bf.CASES[name]
    sc, res = runs(name)
    nv = case.nvar
    assert np.all(res.status == 0), res.status
    fails = []
    for k in range(len(case.cands)):
        for var in range(nv):
            s = k * nv + var
            o = bf.oracle_loop(name, k, var).res
            err = bf.traj_err(res.y[s], res.u[s], o)
            tol = TRAJ_RTOL
            if k == 0:
                tol, measured = bf.gentle_bound(name, var)
                print("%s variant %d gentle: device %.2e of the peak, bound %.2e (restatement %.2e): ratio %.3f"
                      % (name, var, err, tol, measured, err / tol))
            J1 = (o.y ** 2).sum(1)
            j22 = (o.y[:, INK0:] ** 2).sum(1)
            ej = float(np.max(np.abs(res.J1[s] - J1) / J1))
            e22 = float(np.max(np.abs(res.j22[s] - j22) / j22))
            line = "%s cand %d variant %d: y/u %.2e (tol %.2e), J1 %.2e, j22 %.2e" % (name, k, var, err, tol, ej, e22)
            if not case.est:
                eo = max(bf._trel(res.ys[s], o.ys), bf._trel(res.uopt[s], o.uopt)) if np.abs(o.uopt).max() > 0 else \
                    float(max(np.abs(res.uopt[s]).max(), bf._trel(res.ys[s], o.ys)))
                line += ", ys/uopt %.2e" % eo
                if not eo < TRAJ_RTOL:
                    fails.append(line)
            print(line)
            if not (err < tol and ej < COST_RTOL and e22 < COST_RTOL):
                fails.append(line)
    assert not fails, fails


@pytest.mark.gpu
@pytest.mark.parametrize("name", bf.NAMES)
def test_replay(runs, name):
    """Every applied first move over all nit steps is the oracle QP's optimum at the device's own
    state (the state rebuilt by forward simulation from the device's u)."""
    from oracle.toolbox_band import replay_moves

    case = bf.CASES[name]
    _, res = runs(name)
    osc = bf.oracle(case)
    r, v, _ = bf.signals(case)
    nv = case.nvar
    fails = []
    for k, c in enumerate(case.cands):
        for var in range(nv):
            s = k * nv + var
            d, lam = np.array(c[2]), np.array(c[3])
            if case.est:
                du_o, du_a = bm.replay_moves_bias(osc, bf.oracle_dtfs(case.plants[var]), r, v, c[0], c[1], d, lam, res.u[s])
            else:
                du_o, du_a = replay_moves(osc, r, v, c[0], c[1], d, lam, res.u[s])
            assert du_o.shape[1] == case.nit
            err = bf._trel(du_a, du_o)
            print("%s cand %d variant %d: replay %.2e of the largest move" % (name, k, var, err))
            if not err < REPLAY_RTOL:
                fails.append((k, var, err))
    assert not fails, fails


@pytest.mark.gpu
@pytest.mark.parametrize("name", bf.NAMES)
def test_deterministic_and_order_free(runs, name):
    """The reversed batch gives the same bits in every result."""
    case = bf.CASES[name]
    sc, a = runs(name)
    n, nv = len(case.cands), case.nvar
    b = _run(case, sc, idx=list(range(n))[::-1], open_loop=not case.est)
    fields = ("J1", "j22", "status", "qp_iters", "y", "u") + (() if case.est else ("j21", "Jnu", "ys", "uopt"))
    for f in fields:
        x, y = getattr(a, f), getattr(b, f)
        back = y.reshape((n, nv) + y.shape[1:])[::-1].reshape(y.shape)
        np.testing.assert_array_equal(bits(x), bits(back), err_msg=f)


@pytest.mark.gpu
def test_estimator_on_the_model_is_the_nominal_loop(gpu):
    """est_so2 with every plant variant equal to the model: b = +0.0 exactly, and each simulation has
    the bits of the nominal scenario on the so2 model (mdband_kernel.hip, the comment on EST)."""
    est = bf.CASES["est_so2"]
    assert est.model == bf.CASES["so2"].model
    a = _run(est, bf.product(est, plants=None))   # the same model, bands and candidates, no estimator
    b = _run(est, bf.product(est, plants=[est.model] * 3))
    assert np.all(a.status == 0), a.status
    for var in range(3):
        for f in ("J1", "j22", "status", "qp_iters", "y", "u"):
            np.testing.assert_array_equal(bits(getattr(b, f)[var::3]), bits(getattr(a, f)), err_msg="%s variant %d" % (f, var))


@pytest.mark.gpu
def test_wide_candidate_alone(runs):
    """wide: the Nu = 8 candidate (Mz = 17, the 32-row instance) has in the mixed batch the bits of
    its own single-candidate run, and so has an Mz <= 16 neighbour."""
    case = bf.CASES["wide"]
    sc, a = runs("wide")
    wide = [k for k, c in enumerate(case.cands) if case.nu * c[1] + 1 > 16]
    assert wide == [7]
    for k in (7, 5):
        b = _run(case, sc, idx=[k], open_loop=True)
        for f in ("J1", "j21", "j22", "Jnu", "status", "qp_iters", "y", "u", "ys", "uopt"):
            np.testing.assert_array_equal(bits(getattr(b, f)[0]), bits(getattr(a, f)[k]), err_msg="%s cand %d" % (f, k))
