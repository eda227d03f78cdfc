"""GPU: the Van de Vusse NMPC kernel one Gauss-Newton step at a time against the mpmath truth of
tests/nmpc_step_ref.py (tests/golden/nmpc_step_truth.npz), and nmpc_model.h's state derivative and RK4 map
through tests/device_units/libmpct_nmpc_probe.so.

One-step tests: NmpcScenario(..., sqp_max = 1 | 2), open-loop leg on, trajectories on, nit just long enough;
one tiny batch per case whose reference sets step at t* (or never: the last set, which proves that every
call before a step converges at once, so the call at the step starts from a speculated pass).  Compared:
every closed-loop move u (the move at t* is the first move of a call that starts from a pass run 0..3
calls earlier) and all 2 Nu open-loop moves uopt (a fresh call's whole step vector), by
max |device - truth| / u_scale against 8 x the float64 restatement's own error of the case's family;
qp_iters, the MPCT_ST_SQP_MAXITER bit and no other status bit exactly."""
import ctypes as C
import os

import numpy as np
import pytest

import nmpc_step_ref as S

pytestmark = pytest.mark.gpu

LIB = os.path.join(os.path.dirname(os.path.abspath(__file__)), "device_units", "libmpct_nmpc_probe.so")
ST_SQP_MAXITER = 32


@pytest.fixture(scope="module")
def gpu(built, has_gpu):
    if not has_gpu:
        pytest.skip("no GPU")
    return True


@pytest.fixture(scope="module")
def golden():
    z = np.load(S.GOLDEN)
    g = {c["name"]: {k.rsplit("/", 1)[1]: z[k] for k in z.files if k.rsplit("/", 1)[0] == c["name"]} for c in S.CASES}
    return g, S.bound_table(g)


def run_case(c, g):
    from mpct import nmpc
    from mpct.engine import eval_batch

    kw = c["kw"]
    xcz = [k - 1 for k in c["xc"]]
    yref = g["refs"][-1]
    sc = nmpc.NmpcScenario(g["x0"], S.U0, kw.get("u_min", S.UMIN), kw.get("u_max", S.UMAX), S.XMIN,
                           kw.get("x_max", S.XMAX), yref, c["n_max"], c["nu_max"], nsub=2, xc=c["xc"],
                           params=np.array(S.VDV_PARAMS), y_scale=[S.XMAX[k] - S.XMIN[k] for k in xcz], u_scale=S.SU,
                           sqp_max=c["sqp_max"], sqp_tol=kw.get("sqp_tol", 1e-8),
                           plant_params=np.array(kw["plant"])[None] if "plant" in kw else None)
    try:
        return eval_batch(sc, [c["N"]], [c["Nu"]], np.array([c["delta"]]), np.array([c["lam"]]), g["refs"],
                          open_loop=True, want_traj=True)
    finally:
        sc.close()


@pytest.mark.parametrize("name", [c["name"] for c in S.CASES])
def test_one_step_against_the_truth(gpu, golden, name, capsys):
    c = S.BY_NAME[name]
    g, tab = golden
    g = g[name]
    bound = tab[c["family"]][1]
    res = run_case(c, g)
    nref, Nu, nit = len(c["tstars"]), c["Nu"], c["nit"]
    nshow = min(nit, Nu)
    eu = max(S.measure(res.u[k].T, g["u"][k].T) for k in range(nref))
    eo = max(S.measure(res.uopt[k].T[:nshow], g["uopt"][k][:nshow]) for k in range(nref))
    with capsys.disabled():
        print("\n  %s: max |du| / s_u  closed loop %.3g, open-loop step %.3g, bound %.3g; qp_iters %s status %s"
              % (name, eu, eo, bound, res.qp_iters.tolist(), res.status.tolist()))
    np.testing.assert_array_equal(res.qp_iters, g["iters"])
    np.testing.assert_array_equal(res.status, np.where(g["maxiter"], ST_SQP_MAXITER, 0))      # and no other bit
    # the set that never steps: every call converged at once (the calls before a step are bitwise these); with a
    # first step at t = 1 (`pre`) that call alone did not
    assert g["early"].all() and res.qp_iters[-1] == nit and res.status[-1] == (ST_SQP_MAXITER if c["pre"] else 0)
    for k in range(nref):
        np.testing.assert_array_equal(res.uopt[k][:, nshow - 1:], np.repeat(res.uopt[k][:, nshow - 1:nshow], nit - nshow + 1, 1))
    assert eo <= bound, (name, eo, bound)
    assert eu <= bound, (name, eu, bound)


def test_speculated_first_move_is_the_fresh_calls(gpu, golden):
    """d/4-2 (G = 4): the call at t* = 2, 3, 4 starts from a pass that the call at t = 1 ran 1, 2, 3 steps
    ahead; its first move is the first move of the open-loop call, a fresh pass from (bitwise nearly) the same
    state, within the family's bound; with plant != model the speculation's plant steps are the plant's."""
    g, tab = golden
    for name in ("d/4-2", "d/4-2-plant"):
        c = S.BY_NAME[name]
        res = run_case(c, g[name])
        for k, ts_ in enumerate(c["tstars"][:-1]):
            assert np.all(res.u[k][:, :ts_] == np.array(S.U0)[:, None])          # held until the step
            assert S.measure(res.u[k][:, ts_], g[name]["u"][k][:, ts_]) <= tab["d"][1], (name, ts_)
    # the plant's steps matter at this tolerance: the truth that steps the model instead is further away
    c = S.BY_NAME["d/4-2-plant"]
    P = S.Prob(c["N"], c["Nu"], c["delta"], c["lam"], sqp_tol=1e-3)
    wrong = S.call_chain(P, g[c["name"]]["x0"], S.U0, g[c["name"]]["refs"][2], open_loop=False)["u"]
    assert S.measure(wrong[:, 4], g[c["name"]]["u"][2][:, 4]) > 100 * tab["d"][1]


# ---------------------------------------------------------------------------------------------
# nmpc_model.h through the probe

def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def call_probe(lib, rk4, tan, cases, xd, ud):
    n = len(cases)
    p = np.ascontiguousarray([c[0] for c in cases])
    x = np.ascontiguousarray([c[1] for c in cases])
    u = np.ascontiguousarray([c[2] for c in cases])
    h = np.ascontiguousarray([S.TS / c[3] for c in cases])
    ns = np.ascontiguousarray([c[3] for c in cases], dtype=np.int32)
    XD, UD = np.ascontiguousarray(np.tile(xd, (n, 1, 1))), np.ascontiguousarray(np.tile(ud, (n, 1, 1)))
    out, outd = np.full((n, 64, 3), np.nan), np.full((n, 64, 3), -7.0)
    if rk4:
        rc = lib.probe_vdv_rk4(C.c_int(tan), C.c_int(n), _p(p), _p(x), _p(u), _p(h), _p(ns), _p(XD), _p(UD), _p(out), _p(outd))
    else:
        rc = lib.probe_vdv_rhs(C.c_int(tan), C.c_int(n), _p(p), _p(x), _p(u), _p(XD), _p(UD), _p(out), _p(outd))
    assert rc == 0, rc
    return out, outd


@pytest.fixture(scope="module")
def probe(gpu):
    return C.CDLL(LIB)


@pytest.mark.parametrize("rk4", [False, True], ids=["rhs", "rk4"])
@pytest.mark.parametrize("kind", ["own", "xd"])
def test_model_against_the_truth(probe, rk4, kind, capsys):
    """vdv_rhs / vdv_rk4 with and without tangents: every lane returns bitwise the same value; value and
    tangents within 8 x the float64 restatement's own error (nmpc_step_ref's probe table: taken over the same
    cases on the CPU, value and tangents apart; per case: largest error over the largest entry)."""
    cases, xd, ud, rows, rv, rd = S.probe_reference("rk4" if rk4 else "rhs", kind)
    stored = np.load(S.GOLDEN)["probe/%s-%s" % ("rk4" if rk4 else "rhs", kind)]
    assert (rv, rd) == tuple(stored)        # the bounds are the fixture's, measured on the CPU
    out1, outd1 = call_probe(probe, rk4, 1, cases, xd, ud)
    out0, outd0 = call_probe(probe, rk4, 0, cases, xd, ud)
    assert np.all(outd0 == -7.0)                                   # TAN = false writes no tangent
    assert np.all(out1 == out1[:, :1]) and np.all(out0 == out0[:, :1])
    same = bool(np.all(out0 == out1))
    ev = ed = 0.0
    for k, (tx, tX, fl, fld) in enumerate(rows):
        ev = max(ev, S.probe_dev(out1[k, 0], tx, fl), S.probe_dev(out0[k, 0], tx, fl))
        ed = max(ed, S.probe_dev(outd1[k], tX, fld))
    with capsys.disabled():
        print("\n  %s/%s: value %.3g (restatement %.3g), tangent %.3g (restatement %.3g); TAN on/off bitwise equal: %s,"
              " max |difference| %.3g" % ("rk4" if rk4 else "rhs", kind, ev, rv, ed, rd, same, np.abs(out0 - out1).max()))
    assert ev <= S.DEVICE_FACTOR * rv, (ev, rv)
    assert ed <= S.DEVICE_FACTOR * rd, (ed, rd)
    assert same        # the Armijo test compares costs of both instances


def test_probe_refuses_bad_arguments(probe):
    cases = S.probe_cases()[:2]
    z = np.zeros((2, 64, 3))
    p = np.ascontiguousarray([c[0] for c in cases])
    args = [_p(p), _p(np.zeros((2, 3))), _p(np.zeros((2, 2)))]
    tail = [_p(np.zeros((2, 64, 3))), _p(np.zeros((2, 64, 2))), _p(z), _p(z)]
    h, ns = np.array([0.0, 0.1]), np.array([1, 1], np.int32)
    assert probe.probe_vdv_rk4(1, 2, *args, _p(h), _p(ns), *tail) == 1              # h = 0
    assert probe.probe_vdv_rk4(1, 2, *args, _p(np.array([0.1, 0.1])), _p(np.array([1, 0], np.int32)), *tail) == 1
    assert probe.probe_vdv_rhs(2, 2, *args, *tail) == 1 and probe.probe_vdv_rhs(1, 0, *args, *tail) == 1
    assert probe.probe_vdv_rhs(1, 2, None, *args[1:], *tail) == 1
    bad = p.copy()
    bad[1, 9] = 0.0                                                                   # rho = 0
    assert probe.probe_vdv_rhs(1, 2, _p(bad), *args[1:], *tail) == 1
