"""The MEX gateway's 'pareto' command (matlab/mpct_mex.c) through the MX stub, built and driven like
tests/test_mex_tail.py: argument errors without a device (the library's message for 17 objectives), and on
the GPU the struct's fields against tests/pareto_ref.py: a 1-based front, 0-based dom_count and layer, the
column-major C x k input transposed in the gateway."""
import subprocess

import numpy as np
import pytest

import pareto_ref as R
from test_mex import _parse_out, mex, spec


def test_mex_pareto_argument_errors(built, has_gpu):
    A = R.generated(6, 3, 4)
    res = mex([(1, ["pareto"]),
               (1, ["pareto", np.ones((4, 17))]),              # 17 objectives: the library's MPCT_EINVAL
               (1, ["pareto", A, 65.0]),                       # layers out of range
               (1, ["pareto", A, 2.5]),
               (1, ["pareto", A, 2.0, 0.0, 1.0])])
    assert not res[0][0] and res[0][1][0] == "mpct:arg" and "usage" in res[0][1][1]
    assert res[1] == (False, ("mpct:pareto", "k must be 1 .. MPCT_PARETO_MAX_OBJ"))
    assert not res[2][0] and res[2][1][0] == "mpct:pareto" and "max_layers" in res[2][1][1]
    assert res[3] == (False, ("mpct:arg", "'max_layers' must be an integer"))
    assert not res[4][0] and res[4][1][0] == "mpct:arg" and "usage" in res[4][1][1]
    if not has_gpu:
        res = mex([(1, ["pareto", A, 2.0])])
        assert not res[0][0] and res[0][1][0] == "mpct:pareto" and "device" in res[0][1][1]


@pytest.mark.gpu
def test_mex_pareto_matches_reference(built, has_gpu):
    if not has_gpu:
        pytest.skip("no GPU")
    from test_robust_gpu import _build_driver

    A = R.generated(300, 3, 6)          # not symmetric in its columns: a transposition error would show
    A[:, 1] += np.arange(300) % 7
    A[11, 2] = np.nan
    calls = [(1, ["pareto", A, 5.0, 0.0]), (1, ["pareto", A])]
    text = "\n".join("CALL %d %d\n%s" % (nl, len(args), "\n".join(spec(a) for a in args)) for nl, args in calls)
    out = subprocess.run([_build_driver()], input=text, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    lines = out.stdout.splitlines()
    assert "CALL 0 OK" in lines and "CALL 1 OK" in lines, out.stdout[-2000:]
    at = [i for i, ln in enumerate(lines) if ln.startswith("CALL ")]
    dom, layer, front, nf = R.pareto_np(A, 5)
    assert 1 <= nf < 299 and layer.max() == 5
    for k in (0, 1):
        mine = lines[at[k]:at[k + 1] if k + 1 < len(at) else None]
        fields = {ln.split()[2]: _parse_out(ln.split()[3:]) for ln in mine if ln.startswith("FIELD 0 ")}
        assert set(fields) == {"front", "dom_count", "layer"}
        assert fields["front"].shape == (nf, 1) and fields["dom_count"].shape == (300, 1)
        np.testing.assert_array_equal(fields["front"][:, 0], front[:nf] + 1)      # 1-based
        np.testing.assert_array_equal(fields["dom_count"][:, 0], dom)             # 0-based, -1 invalid
        assert fields["dom_count"][11, 0] == -1 and 12 not in fields["front"]
        if k == 0:
            np.testing.assert_array_equal(fields["layer"][:, 0], layer)
        else:
            assert fields["layer"].size == 0
