"""The MEX gateway's 'indices' and 'eval_indices' commands (matlab/mpct_mex.c) through the MX stub, built and
driven like tests/test_mex_pareto.py: argument errors without a device (the gateway's own and the library's
messages), and on the GPU the struct's fields against tests/indices_ref.py and the Python host, bit for
bit, in MATLAB's layouts (my x nit x S signals in, S x my fields out, 0-based t_emax and settle)."""
import subprocess

import numpy as np
import pytest

import indices_ref as R
from test_mex import _parse_out, mex, shell3x3_desc, spec

ALL = R.Y_FIELDS + R.U_FIELDS


def _pages(a):
    """[S, rows, nit] -> MATLAB rows x nit x S"""
    return np.ascontiguousarray(np.transpose(a, (1, 2, 0)))


def test_mex_indices_argument_errors(built, has_gpu):
    y, u, r = R.generated(4, 2, 2, 1, 30)
    Y, U, Rr = _pages(y), _pages(u), _pages(r)
    res = mex([(1, ["indices"]),
               (1, ["indices", np.zeros((0, 0)), np.zeros((0, 0)), Rr]),
               (1, ["indices", Y, U, _pages(r[:, :1])]),                       # r with another my
               (1, ["indices", Y, _pages(u[:3]), Rr]),                         # S disagrees
               (1, ["indices", Y, U, Rr, {"t0": 2.5}]),
               (1, ["indices", Y, U, Rr, {"t0": 30.0}]),                       # the library's MPCT_EINVAL
               (1, ["indices", Y, U, Rr, {"band_rel": -1.0}]),
               (1, ["indices", _pages(y[:3]), _pages(u[:3]), Rr]),             # S = 3 is no multiple of nref = 2
               (1, ["eval_indices", 0.0])])
    assert not res[0][0] and res[0][1][0] == "mpct:arg" and "usage" in res[0][1][1]
    assert res[1] == (False, ("mpct:arg", "'y' and 'u' are both empty"))
    assert not res[2][0] and res[2][1][0] == "mpct:arg" and "'r' must be" in res[2][1][1]
    assert not res[3][0] and res[3][1][0] == "mpct:arg" and "agree" in res[3][1][1]
    assert res[4] == (False, ("mpct:arg", "'t0' must be an integer"))
    assert res[5] == (False, ("mpct:indices", "t0 must be 0 .. nit-1"))
    assert not res[6][0] and res[6][1][0] == "mpct:indices" and "band_rel" in res[6][1][1]
    assert res[7] == (False, ("mpct:indices", "S must be a multiple of nref"))
    assert not res[8][0] and res[8][1][0] == "mpct:arg" and "usage" in res[8][1][1]
    if not has_gpu:
        res = mex([(1, ["indices", Y, U, Rr])])
        assert not res[0][0] and res[0][1][0] == "mpct:indices" and "device" in res[0][1][1]


def _fields_of(lines, k, at):
    mine = lines[at[k]:at[k + 1] if k + 1 < len(at) else None]
    return {ln.split()[2]: _parse_out(ln.split()[3:]) for ln in mine if ln.startswith("FIELD 0 ")}


@pytest.mark.gpu
def test_mex_indices_match_reference_and_python_host(built, has_gpu):
    if not has_gpu:
        pytest.skip("no GPU")
    from test_robust_gpu import _build_driver
    from mpct.engine import eval_indices
    from mpct.scenarios import candidate_grid, vns_step_refs

    y, u, r = R.generated(6, 3, 3, 2, 130)
    sc, _, d = shell3x3_desc()
    N2, Nu, dl, lm = candidate_grid(4)
    N2[2] = 0                                             # a candidate that is not run: NaN / -1 rows
    refs = vns_step_refs(3, 500)
    par = {"t0": 1.0, "band_rel": R.BAND_REL, "band_abs": R.BAND_ABS}
    calls = [(1, ["indices", _pages(y), _pages(u), _pages(r), par]),
             (1, ["indices", np.zeros((0, 0)), _pages(u), np.zeros((0, 0)), par]),
             (1, ["create", d]),
             (1, ["eval_indices", ("P", 2, 0), N2.astype(float), Nu.astype(float), dl, lm, _pages(refs), np.zeros((0, 0)),
                  {"t0": 10.0, "band_rel": 0.05}])]
    text = "\n".join("CALL %d %d\n%s" % (nl, len(args), "\n".join(spec(a) for a in args)) for nl, args in calls)
    out = subprocess.run([_build_driver()], input=text, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    lines = out.stdout.splitlines()
    assert all("CALL %d OK" % k in lines for k in range(4)), out.stdout[-2000:]
    at = [i for i, ln in enumerate(lines) if ln.startswith("CALL ")]
    want = R.indices_np(y, u, r, 1, R.BAND_REL, R.BAND_ABS)
    got = _fields_of(lines, 0, at)
    assert set(got) == set(ALL)
    for f in ALL:                                         # S x my / S x nu, not transposed; integers 0-based
        assert got[f].shape == want[f].shape, f
        assert (R.bits(got[f].astype(np.float64)) == R.bits(want[f].astype(np.float64))).all(), f
    assert (got["settle"][1] == -1).all() and got["t_emax"].max() > 1
    part = _fields_of(lines, 1, at)
    assert all(part[f].size == 0 for f in R.Y_FIELDS)
    for f in R.U_FIELDS:
        assert (R.bits(part[f]) == R.bits(want[f])).all(), f
    # the scored batch: the Python host's records of the same call
    ev = _fields_of(lines, 3, at)
    py = eval_indices(sc, N2, Nu, dl, lm, refs, t0=10, band_rel=0.05, want_costs=True, device=0)
    assert set(ev) == set(ALL) | {"J1", "j22", "status", "iters"}
    for f in ALL:
        mine = getattr(py, f).reshape(12, -1)
        assert (R.bits(ev[f].astype(np.float64)) == R.bits(mine.astype(np.float64))).all(), f
    assert (R.bits(ev["J1"]) == R.bits(py.batch.J1)).all() and (ev["status"][:, 0] == py.batch.status).all()
    assert np.isnan(ev["iae"][6:9]).all() and (ev["settle"][6:9] == -1).all() and np.isfinite(ev["iae"][:6]).all()
