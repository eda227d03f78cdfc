"""The MEX gateway's 'envelope' and 'eval_robust_envelope' commands (matlab/mpct_mex.c) through the MX stub, built
and driven like tests/test_mex_draw_stats.py: argument errors without a device (the gateway's own and the library's
messages), and on the GPU the struct's fields against tests/envelope_ref.py and the Python host, bit for bit, in
MATLAB's layouts (y my x nit x C*D in, C x rows*nit (x nlev) and C x rows fields out, 0-based draws and samples)."""
import subprocess

import numpy as np
import pytest

import draw_stats_ref as R
import envelope_ref as E
from test_mex import _parse_out, mex, shell3x3_desc, spec

LEVELS = [0.95, 0.05, 0.5]
SIDE = R.FIELDS + E.SPREAD
NAMES = {p + f for p in ("y_", "u_") for f in SIDE} | {"levels"}


def _pages(x):
    """[C, D, rows, nit] -> MATLAB rows x nit x C*D"""
    Cn, D, rows, nit = x.shape
    return np.ascontiguousarray(np.transpose(x.reshape(Cn * D, rows, nit), (1, 2, 0)))


def _traj(Cn, D, rows, nit, seed):
    x, alive = R.table(Cn, D, rows * nit, seed)
    return x.reshape(Cn, D, rows, nit), alive


def test_mex_envelope_argument_errors(built, has_gpu):
    y, alive = _traj(3, 5, 2, 7, 11)
    u, _ = _traj(3, 5, 1, 7, 12)
    Y, U, A = _pages(y), _pages(u), np.ascontiguousarray(alive.T).astype(float)
    none = np.zeros((0, 0))
    _, r, d = shell3x3_desc()
    one = [[30.0], [5.0], np.ones((1, 3)), np.ones((1, 3)), r]
    res = mex([(1, ["envelope"]),
               (1, ["envelope", none, none, 5.0]),
               (1, ["envelope", Y, _pages(u[:2]), 5.0]),                          # another number of pages
               (1, ["envelope", Y, U, 4.0]),                                      # 15 pages are no multiple of 4
               (1, ["envelope", Y, U, 5.0, A[:4]]),                               # alive with another D
               (1, ["envelope", Y, U, 5.0, A, {"levels": np.full(9, 0.5)}]),      # nine levels
               (1, ["envelope", Y, U, 5.0, A, {"device": 0.5}]),
               (1, ["envelope", Y, U, 5.0, A, {"levels": [0.5, 1.5]}]),           # the library's MPCT_EINVAL
               (1, ["envelope", Y, U, 5.0, A, {"t0": 7.0}]),
               (1, ["envelope", _pages(np.zeros((1, 5000, 1, 2))), none, 5000.0, none, {"levels": [0.5]}]),   # MPCT_ERANGE
               (1, ["eval_robust_envelope", 0.0]),
               (1, ["create", d]),
               (1, ["eval_robust_envelope", ("P", 11, 0)] + one + [none, {"levels": [0.0]}]),
               (1, ["eval_robust_envelope", ("P", 11, 0)] + one + [none, {"j_bound": -1.0}]),
               (1, ["eval_robust_envelope", ("P", 11, 0)] + one + [none, {"t0": 500.0}])])
    assert not res[0][0] and res[0][1][0] == "mpct:arg" and "usage" in res[0][1][1]
    assert res[1] == (False, ("mpct:arg", "'y' and 'u' are both empty"))
    assert res[2] == (False, ("mpct:arg", "'y' and 'u' must agree on nit and S"))
    assert not res[3][0] and res[3][1][0] == "mpct:arg" and "'D' must be" in res[3][1][1]
    assert res[4] == (False, ("mpct:arg", "'alive' must be D x C"))
    assert not res[5][0] and res[5][1][0] == "mpct:arg" and "'levels' must hold" in res[5][1][1]
    assert res[6] == (False, ("mpct:arg", "'device' must be an integer"))
    assert not res[7][0] and res[7][1][0] == "mpct:envelope" and "every level" in res[7][1][1]
    assert not res[8][0] and res[8][1][0] == "mpct:envelope" and "t0 must lie" in res[8][1][1]
    assert not res[9][0] and res[9][1][0] == "mpct:envelope" and "MPCT_TAIL_MAX_DRAWS" in res[9][1][1]
    assert not res[10][0] and res[10][1][0] == "mpct:arg" and "usage" in res[10][1][1]
    assert res[11][0]
    assert not res[12][0] and res[12][1][0] == "mpct:eval_robust_envelope" and "every level" in res[12][1][1]
    assert not res[13][0] and res[13][1][0] == "mpct:eval_robust_envelope" and "j_bound" in res[13][1][1]
    assert not res[14][0] and res[14][1][0] == "mpct:eval_robust_envelope" and "t0 must lie" in res[14][1][1]
    if not has_gpu:
        res = mex([(1, ["envelope", Y, U, 5.0, A, {"levels": [0.5]}])])
        assert not res[0][0] and res[0][1][0] == "mpct:envelope" and "device" in res[0][1][1]


def _fields_of(lines, k, at):
    mine = lines[at[k]:at[k + 1] if k + 1 < len(at) else None]
    return {ln.split()[2]: _parse_out(ln.split()[3:]) for ln in mine if ln.startswith("FIELD 0 ")}


def _same(got, name, want, msg):
    """a MEX field (doubles; C x w x nlev loses trailing singleton pages) against the reference's [C, rows, nit(, nlev)]"""
    w = np.asarray(want, dtype=np.float64)
    flat = w.reshape((w.shape[0], w.shape[1] * w.shape[2]) + w.shape[3:]) if w.ndim >= 3 else w
    g = np.asarray(got[name], dtype=np.float64).reshape(flat.shape)
    assert (R.bits(g) == R.bits(flat)).all(), (name, msg)


@pytest.mark.gpu
def test_mex_envelope_match_reference_and_python_host(built, has_gpu):
    if not has_gpu:
        pytest.skip("no GPU")
    from test_robust_gpu import _build_driver
    from mpct.engine import eval_robust_envelope
    from mpct.scenarios import candidate_grid, vns_step_refs

    y, alive = _traj(4, 5, 2, 37, 21)
    u, _ = _traj(4, 5, 1, 37, 22)
    sc, _, d = shell3x3_desc()
    N2, Nu, dl, lm = candidate_grid(3)
    N2[1] = 0                                             # a candidate that is not run: n = 0, NaN / -1
    refs = vns_step_refs(3, 500)
    par = {"levels": np.array(LEVELS[:2]), "t0": 10.0}
    none = np.zeros((0, 0))
    calls = [(1, ["envelope", _pages(y), _pages(u), 5.0, np.ascontiguousarray(alive.T).astype(float),
                  {"levels": np.array(LEVELS), "t0": 4.0}]),
             (1, ["envelope", none, _pages(u), 5.0]),
             (1, ["create", d]),
             (1, ["eval_robust_envelope", ("P", 2, 0), N2.astype(float), Nu.astype(float), dl, lm,
                  np.ascontiguousarray(np.transpose(refs, (1, 2, 0))), none, par])]
    text = "\n".join("CALL %d %d\n%s" % (nl, len(args), "\n".join(spec(a) for a in args)) for nl, args in calls)
    out = subprocess.run([_build_driver()], input=text, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr
    lines = out.stdout.splitlines()
    assert all("CALL %d OK" % k in lines for k in range(4)), out.stdout[-2000:]
    at = [i for i, ln in enumerate(lines) if ln.startswith("CALL ")]
    got = _fields_of(lines, 0, at)
    assert set(got) == NAMES and got["y_hi"].shape == (4, 74) and got["u_cvar"].shape == (4, 37, 3)
    assert got["y_spread"].shape == (4, 2) and got["levels"].ravel().tolist() == LEVELS
    for p, tab in (("y_", y), ("u_", u)):
        want, wsp = E.envelope_ref(tab, alive, LEVELS, t0=4)
        for f in R.FIELDS:                                # C x rows*nit (x nlev); draws 0-based
            _same(got, p + f, want[f], "stored")
        for f in E.SPREAD:
            _same(got, p + f, wsp[f], "stored")
    bare = _fields_of(lines, 1, at)
    want, wsp = E.envelope_ref(u, None, [], t0=0)
    for f in R.BASE:
        _same(bare, "u_" + f, want[f], "u alone, no alive, no levels")
    for f in E.SPREAD:
        _same(bare, "u_" + f, wsp[f], "u alone")
    assert all(bare["y_" + f].size == 0 for f in SIDE) and all(bare["u_" + f].size == 0 for f in R.LEVEL) and bare["levels"].size == 0
    # the scored batch: the Python host's record of the same call
    ev = _fields_of(lines, 3, at)
    py = eval_robust_envelope(sc, N2, Nu, dl, lm, refs, levels=LEVELS[:2], t0=10, device=0)
    assert set(ev) == NAMES | {"J1_mean", "J1_worst", "n_failed", "worst_draw", "status"}
    for p, rec in (("y_", py.y), ("u_", py.u)):
        for f in R.FIELDS:
            _same(ev, p + f, rec[f], "eval_robust_envelope")
        for f in E.SPREAD:
            _same(ev, p + f, py.spread[p[0]][f], "eval_robust_envelope")
    assert (R.bits(ev["J1_mean"]) == R.bits(py.base.mean)).all() and (R.bits(ev["J1_worst"]) == R.bits(py.base.worst)).all()
    for f in ("n_failed", "worst_draw", "status"):
        assert (ev[f][:, 0] == getattr(py.base, f)).all(), f
    assert (ev["y_n"][1] == 0).all() and np.isnan(ev["u_hi"][1]).all() and ev["status"][1, 0] == 8
    assert (ev["y_n"][[0, 2]] == 3).all() and np.isfinite(ev["y_hi"][[0, 2]]).all() and (ev["u_t_spread_max"][[0, 2]] >= 10).all()
