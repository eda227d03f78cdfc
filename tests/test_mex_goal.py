"""The MEX gateway's 'goal_attain' command (matlab/mpct_mex.c) through the MX stub, built and driven like
tests/test_mex_pareto.py: argument errors without a device (the library's messages for 17 objectives and for an
invalid goal vector), and on the GPU the struct's fields against tests/goal_ref.py: 1-based best and active,
the column-major C x k and G x k inputs transposed in the gateway, a vector of k goals used for every g."""
import subprocess

import numpy as np
import pytest

import goal_ref as R
from test_mex import _parse_out, mex, spec


def test_mex_goal_argument_errors(built, has_gpu):
    A = R.generated(6, 3, 4)
    gl, w = np.zeros((2, 3)), np.ones((2, 3))
    bad = w.copy()
    bad[1, 2] = -1.0
    res = mex([(1, ["goal_attain", A, gl]),
               (1, ["goal_attain", np.ones((4, 17)), np.zeros((1, 17)), np.ones((1, 17))]),   # 17 objectives: the library's MPCT_EINVAL
               (1, ["goal_attain", A, gl, w, 17.0]),                                       # n_best above the cap
               (1, ["goal_attain", A, gl, w, 2.5]),
               (1, ["goal_attain", A, np.zeros((2, 2)), w]),
               (1, ["goal_attain", A, gl, bad, 2.0]),                                      # goal vector 1 (0-based) is invalid
               (1, ["goal_attain", A, gl, w, 1.0, 0.0, 1.0])])
    assert not res[0][0] and res[0][1][0] == "mpct:arg" and "usage" in res[0][1][1]
    assert res[1] == (False, ("mpct:goal_attain", "k must be 1 .. MPCT_PARETO_MAX_OBJ"))
    assert not res[2][0] and res[2][1][0] == "mpct:goal_attain" and "MPCT_GOAL_MAX_BEST" in res[2][1][1]
    assert not res[3][0] and res[3][1][0] == "mpct:arg" and "n_best" in res[3][1][1]
    assert not res[4][0] and res[4][1][0] == "mpct:arg" and "goals" in res[4][1][1]
    assert not res[5][0] and res[5][1][0] == "mpct:goal_attain" and "goal vector 1 is invalid" in res[5][1][1]
    assert not res[6][0] and res[6][1][0] == "mpct:arg" and "usage" in res[6][1][1]
    if not has_gpu:
        res = mex([(1, ["goal_attain", A, gl, w, 2.0])])
        assert not res[0][0] and res[0][1][0] == "mpct:goal_attain" and "device" in res[0][1][1]


@pytest.mark.gpu
def test_mex_goal_matches_reference(built, has_gpu):
    if not has_gpu:
        pytest.skip("no GPU")
    from test_robust_gpu import _build_driver

    A = R.generated(300, 3, 6)          # not symmetric in its columns: a transposition error would show
    A[:, 1] += np.arange(300) % 7
    A[11, 2] = np.nan
    goals, weights = R.goal_vectors(9, 3, 6)
    one = np.array([0.5, 2.0, 0.75])
    calls = [(1, ["goal_attain", A, goals, weights, 4.0, 0.0]), (1, ["goal_attain", A, one, weights])]
    text = "\n".join("CALL %d %d\n%s" % (nl, len(args), "\n".join(spec(a) for a in args)) for nl, args in calls)
    out = subprocess.run([_build_driver()], input=text, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    lines = out.stdout.splitlines()
    assert "CALL 0 OK" in lines and "CALL 1 OK" in lines, out.stdout[-2000:]
    at = [i for i, ln in enumerate(lines) if ln.startswith("CALL ")]
    wants = [R.goal_np(A, goals, weights, 4), R.goal_np(A, np.tile(one, (9, 1)), weights, 1)]
    assert (wants[0]["n_feasible"] >= 4).any()
    for k, want in enumerate(wants):
        mine = lines[at[k]:at[k + 1] if k + 1 < len(at) else None]
        fields = {ln.split()[2]: _parse_out(ln.split()[3:]) for ln in mine if ln.startswith("FIELD 0 ")}
        assert set(fields) == set(R.FIELDS)
        nb = 4 if k == 0 else 1
        assert fields["best"].shape == (9, nb) and fields["wins"].shape == (300, 1)
        np.testing.assert_array_equal(fields["best"], want["best"] + 1)          # 1-based, 0: none
        np.testing.assert_array_equal(fields["active"], want["active"] + 1)
        # bit for bit, the sign of a zero included; the NaN padding by position (the text protocol carries no payload)
        pad = np.isnan(want["gamma"])
        np.testing.assert_array_equal(np.isnan(fields["gamma"]), pad)
        np.testing.assert_array_equal(np.ascontiguousarray(fields["gamma"])[~pad].view(np.int64), want["gamma"][~pad].view(np.int64))
        np.testing.assert_array_equal(fields["n_feasible"][:, 0], want["n_feasible"])
        np.testing.assert_array_equal(fields["n_attained"][:, 0], want["n_attained"])
        np.testing.assert_array_equal(fields["wins"][:, 0], want["wins"])
        assert fields["wins"][11, 0] == 0 and 12 not in fields["best"]
