"""The MEX gateway's 'eval_robust_tail' command (matlab/mpct_mex.c) through the MX stub, the way
tests/test_mex.py drives 'eval' and tests/test_robust_gpu.py drives 'eval_robust': argument errors
without a device, and on the GPU the struct's fields against the Python wrapper, bit for bit, in
MATLAB's layouts."""
import subprocess

import numpy as np
import pytest

from test_mex import _parse_out, mex, shell3x3_desc, spec

LEVELS = np.array([0.5, 0.9, 1.0])
NOV = np.zeros((0, 0))


def test_mex_tail_argument_errors(built, has_gpu):
    """The usage and the number of levels are checked by the gateway before anything is sized by it;
    a bad level is the library's MPCT_EINVAL, surfaced as mpct:eval_robust_tail with its message --
    all before any device work, so the same with and without a GPU."""
    _, r, d = shell3x3_desc()
    one = ["eval_robust_tail", ("P", 0, 0), [30.0], [5.0], np.ones((1, 3)), np.ones((1, 3)), r, NOV, 0.0]
    res = mex([(1, ["create", d]),
               (1, one),                                    # no levels
               (1, one + [np.zeros((1, 0))]),               # none
               (1, one + [np.full(9, 0.5)]),                # nine
               (1, one + [np.array([0.5, 1.5])]),           # a level above 1
               (1, one + [np.array([0.0])]),
               (1, one[:5] + [np.ones((2, 3))] + one[6:] + [LEVELS])])
    assert res[0][0]
    assert not res[1][0] and res[1][1][0] == "mpct:arg" and "usage" in res[1][1][1]
    assert res[2] == (False, ("mpct:arg", "'levels' must hold 1 .. 8 values (has 0)"))
    assert res[3] == (False, ("mpct:arg", "'levels' must hold 1 .. 8 values (has 9)"))
    for k in (4, 5):
        assert not res[k][0] and res[k][1][0] == "mpct:eval_robust_tail" and "level" in res[k][1][1], res[k]
    assert res[6] == (False, ("mpct:arg", "'lambda' must be 1 x 3 (one candidate per row)"))
    if not has_gpu:
        res = mex([(1, ["create", d]), (1, one + [LEVELS])])
        assert not res[1][0] and res[1][1][0] == "mpct:eval_robust_tail"


@pytest.mark.gpu
def test_mex_eval_robust_tail_matches_python_host(built, has_gpu):
    """mpct_mex('eval_robust_tail', ...) on 4 candidates x 3 draws of Shell 3x3, at the default bound
    and at one inside the totals: every field equals the Python wrapper's, bit for bit."""
    if not has_gpu:
        pytest.skip("no GPU")
    from test_robust_gpu import _build_driver, bits
    from mpct.engine import eval_robust
    from mpct.scenarios import candidate_grid, vns_step_refs

    sc, r, d = shell3x3_desc()
    N2, Nu, dl, lm = candidate_grid(4)
    refs = vns_step_refs(3, 500)
    R3 = np.transpose(refs, (1, 2, 0))       # my x nit x nref, as a MATLAB caller stacks them
    base = eval_robust(sc, N2, Nu, dl, lm, refs, want_J1=True)
    jb = float(np.median(base.J1.reshape(4, 3, 3).sum(axis=2)))
    calls = [(1, ["create", d])]
    for bound in (0.0, jb):
        calls.append((1, ["eval_robust_tail", ("P", 0, 0), N2.astype(float), Nu.astype(float), dl, lm, R3, NOV, bound,
                          LEVELS]))
    text = "\n".join("CALL %d %d\n%s" % (nl, len(args), "\n".join(spec(a) for a in args)) for nl, args in calls)
    out = subprocess.run([_build_driver()], input=text, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    lines = out.stdout.splitlines()
    assert "CALL 1 OK" in lines and "CALL 2 OK" in lines, out.stdout[-2000:]
    at = [i for i, ln in enumerate(lines) if ln.startswith("CALL ")]
    for k, bound in ((1, 0.0), (2, jb)):
        mine = lines[at[k]:at[k + 1] if k + 1 < len(at) else None]
        fields = {ln.split()[2]: _parse_out(ln.split()[3:]) for ln in mine if ln.startswith("FIELD 0 ")}
        assert set(fields) == {"mean", "worst", "n_failed", "worst_draw", "status", "J1", "levels", "quantile", "cvar",
                               "q_draw"}
        a = eval_robust(sc, N2, Nu, dl, lm, refs, j_bound=bound, want_J1=True, levels=LEVELS)
        for f in ("mean", "worst", "J1", "quantile", "cvar"):
            np.testing.assert_array_equal(bits(fields[f]), bits(getattr(a, f)), err_msg=f)
        for f in ("n_failed", "worst_draw", "status"):
            np.testing.assert_array_equal(fields[f][:, 0], getattr(a, f), err_msg=f)
        np.testing.assert_array_equal(fields["q_draw"], a.q_draw)
        np.testing.assert_array_equal(fields["levels"], LEVELS.reshape(1, 3))
        assert fields["quantile"].shape == (4, 3)
        np.testing.assert_array_equal(fields["q_draw"][:, 2], a.worst_draw)
    assert (a.n_failed > 0).any()      # the second bound fails draws
