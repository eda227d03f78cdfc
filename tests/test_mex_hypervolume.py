"""The MEX gateway's 'hypervolume' command (matlab/mpct_mex.c) through the MX stub, built and driven like
tests/test_mex_pareto.py: argument errors without a device (the library's messages for 17 objectives and
for an empty box), the struct of an empty table (which needs no device), and on the GPU the struct's fields
against tests/hv_ref.py: 1-based members with 0 for a skipped entry, [] for all rows, the column-major
C x k input transposed in the gateway."""
import subprocess

import numpy as np
import pytest

import hv_ref as R
from test_mex import _parse_out, mex, spec

EMPTY = np.zeros((0, 0))


def _struct_calls(calls):
    """the calls through the driver that prints struct outputs: [{field: array}] per call"""
    from test_robust_gpu import _build_driver

    text = "\n".join("CALL %d %d\n%s" % (nl, len(args), "\n".join(spec(a) for a in args)) for nl, args in calls)
    out = subprocess.run([_build_driver()], input=text, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    lines = out.stdout.splitlines()
    at = [i for i, ln in enumerate(lines) if ln.startswith("CALL ")]
    res = []
    for n, i in enumerate(at):
        assert lines[i] == "CALL %d OK" % n, out.stdout[-2000:]
        mine = lines[i:at[n + 1] if n + 1 < len(at) else None]
        res.append({ln.split()[2]: _parse_out(ln.split()[3:]) for ln in mine if ln.startswith("FIELD 0 ")})
    return res


def test_mex_hypervolume_argument_errors(built, has_gpu):
    A = R.generated(6, 3)
    lo, ref = np.zeros(3), np.full(3, 9.5)
    res = mex([(1, ["hypervolume", A, EMPTY, lo]),
               (1, ["hypervolume", np.ones((4, 17)), EMPTY, np.zeros(17), np.ones(17)]),   # the library's MPCT_EINVAL
               (1, ["hypervolume", A, EMPTY, lo, lo, 100.0]),                               # an empty box
               (1, ["hypervolume", A, np.array([1.0, 2.5]), lo, ref]),
               (1, ["hypervolume", A, np.array([1.0, 7.0]), lo, ref, 100.0]),               # row 7 of 6
               (1, ["hypervolume", A, EMPTY, lo, ref, 0.0]),
               (1, ["hypervolume", A, EMPTY, lo, ref, 100.0, 1.5]),
               (1, ["hypervolume", A, EMPTY, lo[:2], ref]),
               (1, ["hypervolume", A, EMPTY, lo, ref, 100.0, 0.0, -1.0, 1.0])])
    assert not res[0][0] and res[0][1][0] == "mpct:arg" and "usage" in res[0][1][1]
    assert res[1] == (False, ("mpct:hypervolume", "k must be 1 .. MPCT_PARETO_MAX_OBJ"))
    assert not res[2][0] and res[2][1][0] == "mpct:hypervolume" and "lo[j] < ref[j]" in res[2][1][1]
    assert not res[3][0] and res[3][1][0] == "mpct:arg" and "1-based" in res[3][1][1]
    assert not res[4][0] and res[4][1][0] == "mpct:hypervolume" and "members" in res[4][1][1]
    assert not res[5][0] and res[5][1][0] == "mpct:hypervolume" and "n_samples < 1" in res[5][1][1]
    assert not res[6][0] and res[6][1][0] == "mpct:arg" and "'seed'" in res[6][1][1]
    assert not res[7][0] and res[7][1][0] == "mpct:arg" and "'lo'" in res[7][1][1]
    assert not res[8][0] and res[8][1][0] == "mpct:arg" and "usage" in res[8][1][1]
    if not has_gpu:
        res = mex([(1, ["hypervolume", A, EMPTY, lo, ref, 100.0])])
        assert not res[0][0] and res[0][1][0] == "mpct:hypervolume" and "device" in res[0][1][1]


def test_mex_hypervolume_of_an_empty_table(built):
    """C = 0, so M = 0: the library needs no device, and the struct has every field"""
    got = _struct_calls([(1, ["hypervolume", np.zeros((0, 2)), EMPTY, np.zeros(2), np.array([1.0, 2.0]), 50.0])])[0]
    assert set(got) == {"hv", "n_covered", "n_samples", "excl", "depth_hist", "contribution", "volume"}
    assert got["hv"].ravel().tolist() == [0.0] and got["n_covered"].ravel().tolist() == [0.0]
    assert got["n_samples"].ravel().tolist() == [50.0] and got["volume"].ravel().tolist() == [2.0]
    assert got["excl"].size == 0 and got["contribution"].size == 0
    assert got["depth_hist"].shape == (8, 1) and got["depth_hist"][:, 0].tolist() == [50.0] + [0.0] * 7


@pytest.mark.gpu
def test_mex_hypervolume_matches_reference(built, has_gpu):
    if not has_gpu:
        pytest.skip("no GPU")
    A = R.generated(300, 3)             # not symmetric in its columns: a transposition error would show
    A[:, 1] += np.arange(300) % 7
    A[11, 2] = np.nan
    lo, ref = np.zeros(3), np.array([9.5, 15.5, 9.5])
    mem0 = np.random.default_rng(5).permutation(300)[:120]
    mem0[7] = -1                        # skipped: 0 in MATLAB's 1-based vector
    N, seed = 4000, 77
    got = _struct_calls([(1, ["hypervolume", A, (mem0 + 1).astype(float), lo, ref, float(N), float(seed), 0.0]),
                         (1, ["hypervolume", A, EMPTY, lo, ref, float(N), float(seed)])])
    for g, members in zip(got, (mem0, None)):
        want = R.hv_np(A, members, lo, ref, N, seed)
        M = 120 if members is not None else 300
        assert g["excl"].shape == (M, 1) and g["contribution"].shape == (M, 1) and g["depth_hist"].shape == (8, 1)
        R.compare((int(g["n_covered"].ravel()[0]), g["excl"][:, 0].astype(np.int64), g["depth_hist"][:, 0].astype(np.int64),
                   float(g["hv"].ravel()[0])), want, "mex")
        assert 0 < want[0] < N and want[1].sum() > 0
        vol = R.volume(lo, ref)
        assert g["volume"].ravel()[0] == vol and g["n_samples"].ravel()[0] == N
        np.testing.assert_array_equal(g["contribution"][:, 0], want[1] / float(N) * vol)
    assert got[0]["excl"][7, 0] == 0
