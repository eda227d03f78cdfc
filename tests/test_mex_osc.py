"""The MEX gateway's 'osc_indices', 'eval_osc_indices' and 'eval_robust_osc_indices' commands (matlab/mpct_mex.c)
through the MX stub, built and driven like tests/test_mex_segments.py: argument errors without a device, and on the
GPU the struct's fields against tests/osc_ref.py and the Python host, bit for bit, in MATLAB's layouts (my x nit x S
signals in, S x (my * nseg) fields out with channel i, segment g in column (i - 1) * nseg + g, 0-based samples)."""
import subprocess

import numpy as np
import pytest

import osc_ref as R
from test_mex import _parse_out, mex, shell3x3_desc, spec

TSEG = [1, 2, 4, 67, 131, 196, 326]
PAR = {"tseg": np.array(TSEG, dtype=float), "base": 1.0, "band_rel": 0.0, "band_abs": R.H, "rev_tol": R.TOL}


def _pages(a):
    """[S, rows, nit] -> MATLAB rows x nit x S"""
    return np.ascontiguousarray(np.transpose(a, (1, 2, 0)))


def test_mex_osc_commands_without_a_device(built, has_gpu):
    y, u, r = R.generated(4, 2, 2, 2, 30, [0, 10, 30])
    Y, U, Rr = _pages(y), _pages(u), _pages(r)
    res = mex([(1, ["osc_indices"]),
               (1, ["osc_indices", np.zeros((0, 0)), np.zeros((0, 0)), Rr]),
               (1, ["osc_indices", Y, _pages(u[:3]), Rr]),                          # S disagrees
               (1, ["osc_indices", Y, U, _pages(r[:, :1])]),                        # r's rows disagree
               (1, ["osc_indices", Y, U, Rr, {"tseg": np.array([0.0])}]),
               (1, ["osc_indices", Y, U, Rr, {"tseg": np.array([0.0, 2.5])}]),
               (1, ["osc_indices", np.zeros((0, 0)), U, np.zeros((0, 0))]),         # no reference, no tseg
               (1, ["osc_indices", Y, U, Rr, {"tseg": np.array([0.0, 31.0])}]),     # the library's MPCT_EINVAL
               (1, ["osc_indices", Y, U, Rr, {"tseg": np.arange(18.0)}]),           # and its MPCT_ERANGE
               (1, ["osc_indices", Y, U, Rr, {"tseg": np.array([0.0, 30.0]), "rev_tol": -1.0}]),
               (1, ["eval_osc_indices", 0.0]),
               (1, ["eval_robust_osc_indices", 0.0])])
    assert not res[0][0] and res[0][1][0] == "mpct:arg" and "usage" in res[0][1][1]
    assert res[1] == (False, ("mpct:arg", "'y' and 'u' are both empty"))
    assert not res[2][0] and res[2][1][0] == "mpct:arg" and "agree" in res[2][1][1]
    assert not res[3][0] and res[3][1][0] == "mpct:arg" and "'r' must be" in res[3][1][1]
    assert res[4] == (False, ("mpct:arg", "'tseg' must hold at least two boundaries"))
    assert res[5] == (False, ("mpct:arg", "'tseg' must hold integers"))
    assert not res[6][0] and res[6][1][0] == "mpct:arg" and "'tseg' is needed" in res[6][1][1]
    assert not res[7][0] and res[7][1][0] == "mpct:osc_indices" and "strictly ascending" in res[7][1][1]
    assert not res[8][0] and res[8][1][0] == "mpct:osc_indices" and "MPCT_SEG_MAX" in res[8][1][1]
    assert not res[9][0] and res[9][1][0] == "mpct:osc_indices" and "rev_tol must be" in res[9][1][1]
    assert not res[10][0] and res[10][1][0] == "mpct:arg" and "usage" in res[10][1][1]
    assert not res[11][0] and res[11][1][0] == "mpct:arg" and "eval_robust_osc_indices" in res[11][1][1]
    if not has_gpu:
        res = mex([(1, ["osc_indices", Y, U, Rr, {"tseg": np.array([0.0, 10.0, 30.0])}])])
        assert not res[0][0] and res[0][1][0] == "mpct:osc_indices" and "device" in res[0][1][1]


def _fields_of(lines, k, at):
    mine = lines[at[k]:at[k + 1] if k + 1 < len(at) else None]
    return {ln.split()[2]: _parse_out(ln.split()[3:]) for ln in mine if ln.startswith("FIELD 0 ")}


@pytest.mark.gpu
def test_mex_osc_indices_match_reference_and_python_host(built, has_gpu):
    if not has_gpu:
        pytest.skip("no GPU")
    from test_robust_gpu import _build_driver
    from mpct.engine import eval_osc_indices, eval_robust_osc_indices
    from mpct.scenarios import candidate_grid, vns_step_refs

    y, u, r = R.generated(6, 3, 3, 2, 330, TSEG)
    nseg = len(TSEG) - 1
    sc, _, d = shell3x3_desc()
    N2, Nu, dl, lm = candidate_grid(4)
    N2[2] = 0                                             # a candidate that is not run: NaN / -1 units
    refs = vns_step_refs(3, 500)
    batch = [("P", 2, 0), N2.astype(float), Nu.astype(float), dl, lm, _pages(refs), np.zeros((0, 0))]
    epar = {"band_rel": 0.05, "rev_tol": 1e-4, "extra": np.array([250.0])}
    calls = [(1, ["osc_indices", _pages(y), _pages(u), _pages(r), PAR]),
             (1, ["osc_indices", np.zeros((0, 0)), _pages(u), np.zeros((0, 0)), PAR]),
             (1, ["create", d]),
             (1, ["eval_osc_indices"] + batch + [epar]),
             (1, ["eval_robust_osc_indices"] + batch + [dict(epar, levels=np.array([0.5, 1.0]), fields=np.array([2.0, 5.0, 1.0]))])]
    text = "\n".join("CALL %d %d\n%s" % (nl, len(args), "\n".join(spec(a) for a in args)) for nl, args in calls)
    out = subprocess.run([_build_driver()], input=text, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    lines = out.stdout.splitlines()
    assert all("CALL %d OK" % k in lines for k in range(5)), out.stdout[-2000:]
    at = [i for i, ln in enumerate(lines) if ln.startswith("CALL ")]
    want = R.osc_scalar(y, u, r, TSEG, base=1, band_rel=0.0, band_abs=R.H, rev_tol=R.TOL)
    got = _fields_of(lines, 0, at)
    assert set(got) == set(R.FIELDS) | {"tseg"} and got["tseg"].ravel().tolist() == [float(t) for t in TSEG]
    for f in R.FIELDS:                                    # S x (w * nseg), channel-major; integers 0-based
        w = want[f].reshape(6, -1)
        assert got[f].shape == w.shape, f
        assert (R.bits(got[f].astype(np.float64)) == R.bits(w.astype(np.float64))).all(), f
    part = _fields_of(lines, 1, at)
    assert all(part[f].size == 0 for f in R.Y_FIELDS)
    for f in R.U_FIELDS:
        assert (R.bits(part[f].astype(np.float64)) == R.bits(want[f].reshape(6, -1).astype(np.float64))).all(), f
    # the scored batch: the Python host's records of the same call, boundaries from the reference and the extra event
    ev = _fields_of(lines, 3, at)
    py = eval_osc_indices(sc, N2, Nu, dl, lm, refs, extra=(250,), band_rel=0.05, rev_tol=1e-4, want_costs=True, device=0)
    assert 250 in py.tseg.tolist() and ev["tseg"].ravel().tolist() == [float(t) for t in py.tseg]
    assert set(ev) == set(R.FIELDS) | {"tseg", "J1", "j22", "status", "iters"}
    for f in R.FIELDS:
        mine = getattr(py, f).reshape(12, -1)
        assert (R.bits(ev[f].astype(np.float64)) == R.bits(mine.astype(np.float64))).all(), f
    assert (R.bits(ev["J1"]) == R.bits(py.batch.J1)).all() and (ev["status"][:, 0] == py.batch.status).all()
    assert np.isnan(ev["decay"][6:9]).all() and (ev["ncross"][6:9] == -1).all() and (ev["ncross"][:6] >= 0).all()
    # the statistics over the three pages of r as draws: the Python host's table of the same call
    tab = _fields_of(lines, 4, at)
    rob = eval_robust_osc_indices(sc, N2, Nu, dl, lm, refs, extra=(250,), band_rel=0.05, rev_tol=1e-4,
                                  fields=("period", "nrev", "decay"), levels=[0.5, 1.0], device=0)
    ns = py.tseg.size - 1
    assert tab["field"].ravel().tolist() == [2.0] * 3 * ns + [5.0] * 3 * ns + [1.0] * 3 * ns
    assert tab["channel"].ravel().tolist() == [float(i + 1) for i in range(3) for _ in range(ns)] * 3
    assert tab["segment"].ravel().tolist() == [float(g + 1) for g in range(ns)] * 9
    for f in ("n", "mean", "lo", "hi", "lo_draw", "hi_draw"):
        assert (R.bits(tab[f].astype(np.float64)) == R.bits(getattr(rob, f).astype(np.float64))).all(), f
    assert (R.bits(tab["J1_mean"]) == R.bits(rob.base.mean)).all() and (tab["n_failed"][:, 0] == rob.base.n_failed).all()
    assert nseg == 6
