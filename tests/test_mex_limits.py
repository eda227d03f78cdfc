"""The MEX gateway's 'limit_indices', 'eval_limit_indices' and 'eval_robust_limit_indices' commands
(matlab/mpct_mex.c) through the MX stub, built and driven like tests/test_mex_indices.py: argument errors without
a device (the gateway's own and the library's messages), and on the GPU the struct's fields against
tests/limits_ref.py and the Python host, bit for bit, in MATLAB's layouts (my x nit x S signals in, S x my fields
out, 0-based t_vmax and t_in)."""
import subprocess

import numpy as np
import pytest

import limits_ref as R
from test_mex import _parse_out, mex, shell3x3_desc, spec

ALL = R.Y_FIELDS + R.U_FIELDS


def _pages(a):
    """[S, rows, nit] -> MATLAB rows x nit x S"""
    return np.ascontiguousarray(np.transpose(a, (1, 2, 0)))


def _par(P, t0, **more):
    par = {"t0": float(t0), "out_tol": P["out_tol"], "sat_tol": P["sat_tol"]}
    par.update({k: np.asarray(P[k], dtype=float) for k in R.BOUNDS if P.get(k) is not None})
    par.update(more)
    return par


def test_mex_limit_indices_argument_errors(built, has_gpu):
    y, u, P = R.generated(4, 2, 2, 30, 1)
    Y, U = _pages(y), _pages(u)
    res = mex([(1, ["limit_indices"]),
               (1, ["limit_indices", np.zeros((0, 0)), np.zeros((0, 0))]),
               (1, ["limit_indices", Y, _pages(u[:3])]),                             # S disagrees
               (1, ["limit_indices", Y, U, {"t0": 2.5}]),
               (1, ["limit_indices", Y, U, {"y_lo": np.zeros(3)}]),                  # one value per channel
               (1, ["limit_indices", Y, U, {"t0": 30.0}]),                           # the library's MPCT_EINVAL
               (1, ["limit_indices", Y, U, {"sat_tol": -1.0}]),
               (1, ["limit_indices", Y, U, {"u_lo": np.array([0.0, 1.0]), "u_hi": np.array([1.0, 0.5])}]),
               (1, ["eval_limit_indices", 0.0]),
               (1, ["eval_robust_limit_indices", 0.0])])
    assert not res[0][0] and res[0][1][0] == "mpct:arg" and "usage" in res[0][1][1]
    assert res[1] == (False, ("mpct:arg", "'y' and 'u' are both empty"))
    assert not res[2][0] and res[2][1][0] == "mpct:arg" and "agree" in res[2][1][1]
    assert res[3] == (False, ("mpct:arg", "'t0' must be an integer"))
    assert res[4] == (False, ("mpct:arg", "'y_lo' must hold 2 values, one per channel"))
    assert res[5] == (False, ("mpct:limit_indices", "t0 must be 0 .. nit-1"))
    assert not res[6][0] and res[6][1][0] == "mpct:limit_indices" and "sat_tol" in res[6][1][1]
    assert not res[7][0] and res[7][1][0] == "mpct:limit_indices" and "bad bound" in res[7][1][1]
    assert not res[8][0] and res[8][1][0] == "mpct:arg" and "usage" in res[8][1][1]
    assert not res[9][0] and res[9][1][0] == "mpct:arg" and "eval_robust_limit_indices" in res[9][1][1]
    if not has_gpu:
        res = mex([(1, ["limit_indices", Y, U, _par(P, 1)])])
        assert not res[0][0] and res[0][1][0] == "mpct:limit_indices" and "device" in res[0][1][1]


def _fields_of(lines, k, at):
    mine = lines[at[k]:at[k + 1] if k + 1 < len(at) else None]
    return {ln.split()[2]: _parse_out(ln.split()[3:]) for ln in mine if ln.startswith("FIELD 0 ")}


@pytest.mark.gpu
def test_mex_limit_indices_match_reference_and_python_host(built, has_gpu):
    if not has_gpu:
        pytest.skip("no GPU")
    from test_robust_gpu import _build_driver
    from mpct.engine import eval_limit_indices, eval_robust_limit_indices
    from mpct.scenarios import candidate_grid, vns_step_refs

    y, u, P = R.generated(5, 4, 2, 130, 1)
    sc, _, d = shell3x3_desc()
    N2, Nu, dl, lm = candidate_grid(4)
    N2[2] = 0                                             # a candidate that is not run: NaN / -1 rows
    refs = vns_step_refs(3, 500)
    u_hi = np.array([0.5, 0.25, 1.0])                     # the caller's bound beside the scenario's own
    batch = [("P", 2, 0), N2.astype(float), Nu.astype(float), dl, lm, _pages(refs), np.zeros((0, 0))]
    calls = [(1, ["limit_indices", _pages(y), _pages(u), _par(P, 1)]),
             (1, ["limit_indices", np.zeros((0, 0)), _pages(u), _par({k: v for k, v in P.items() if k[0] != "y"}, 1)]),
             (1, ["create", d]),
             (1, ["eval_limit_indices"] + batch + [{"t0": 10.0, "sat_tol": 1e-9, "u_hi": u_hi}]),
             (1, ["eval_robust_limit_indices"] + batch + [{"t0": 10.0, "sat_tol": 1e-9, "u_hi": u_hi, "levels": np.array([0.5, 1.0]),
                                                           "fields": np.array([10.0, 9.0, 0.0])}])]
    text = "\n".join("CALL %d %d\n%s" % (nl, len(args), "\n".join(spec(a) for a in args)) for nl, args in calls)
    out = subprocess.run([_build_driver()], input=text, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    lines = out.stdout.splitlines()
    assert all("CALL %d OK" % k in lines for k in range(5)), out.stdout[-2000:]
    at = [i for i, ln in enumerate(lines) if ln.startswith("CALL ")]
    want = R.limits_scalar(y, u, P, 1)
    got = _fields_of(lines, 0, at)
    assert set(got) == set(ALL)
    for f in ALL:                                         # S x my / S x nu, not transposed; integers 0-based
        assert got[f].shape == want[f].shape, f
        assert (R.bits(got[f].astype(np.float64)) == R.bits(want[f].astype(np.float64))).all(), f
    assert (got["t_in"][1] == -1).all() and got["sat_run"][3, 0] == 6 and got["t_vmax"][0, 0] == 9
    part = _fields_of(lines, 1, at)
    assert all(part[f].size == 0 for f in R.Y_FIELDS)
    for f in R.U_FIELDS:
        assert (R.bits(part[f].astype(np.float64)) == R.bits(want[f].astype(np.float64))).all(), f
    # the scored batch: the Python host's records of the same call
    ev = _fields_of(lines, 3, at)
    py = eval_limit_indices(sc, N2, Nu, dl, lm, refs, t0=10, sat_tol=1e-9, u_hi=u_hi, want_costs=True, device=0)
    assert set(ev) == set(ALL) | {"J1", "j22", "status", "iters"}
    for f in ALL:
        mine = getattr(py, f).reshape(12, -1)
        assert (R.bits(ev[f].astype(np.float64)) == R.bits(mine.astype(np.float64))).all(), f
    assert (R.bits(ev["J1"]) == R.bits(py.batch.J1)).all() and (ev["status"][:, 0] == py.batch.status).all()
    assert np.isnan(ev["u_margin"][6:9]).all() and (ev["sat_run"][6:9] == -1).all() and (ev["n_rate"][:6] >= 0).all()
    # the statistics over the three pages of r as draws: the Python host's table of the same call
    tab = _fields_of(lines, 4, at)
    rob = eval_robust_limit_indices(sc, N2, Nu, dl, lm, refs, fields=("sat_run", "n_rate", "viol"), levels=[0.5, 1.0], t0=10,
                                    sat_tol=1e-9, u_hi=u_hi, device=0)
    assert tab["field"].ravel().tolist() == [10.0] * 3 + [9.0] * 3 + [0.0] * 3
    assert tab["channel"].ravel().tolist() == [1.0, 2.0, 3.0] * 3
    for f in ("n", "mean", "lo", "hi", "lo_draw", "hi_draw"):
        assert (R.bits(tab[f].astype(np.float64)) == R.bits(getattr(rob, f).astype(np.float64))).all(), f
    assert (R.bits(tab["J1_mean"]) == R.bits(rob.base.mean)).all() and (tab["n_failed"][:, 0] == rob.base.n_failed).all()
