"""The MEX gateway's 'hv_select' command (matlab/mpct_mex.c) through the MX stub, built and driven like
tests/test_mex_hypervolume.py: argument errors without a device (the library's messages for 17 objectives,
an empty box and n_pick out of range), the struct of an empty table (which needs no device), and on the GPU
the struct's fields against tests/hvsel_ref.py: 1-based members with 0 for a skipped entry, [] for all rows,
1-based pos and index with 0 after the end of the selection, the column-major C x k input transposed in
the gateway."""
import numpy as np
import pytest

import hv_ref as R
import hvsel_ref as S
from test_mex import mex
from test_mex_hypervolume import _struct_calls

EMPTY = np.zeros((0, 0))
NAMES = {"n_picked", "pos", "index", "gain", "covered", "hv", "ties", "n_covered_all", "share", "n_samples", "volume"}


def test_mex_hv_select_argument_errors(built, has_gpu):
    A = R.generated(6, 3)
    lo, ref = np.zeros(3), np.full(3, 9.5)
    res = mex([(1, ["hv_select", A, EMPTY, lo, ref]),
               (1, ["hv_select", np.ones((4, 17)), EMPTY, np.zeros(17), np.ones(17), 2.0]),   # the library's MPCT_EINVAL
               (1, ["hv_select", A, EMPTY, lo, lo, 2.0, 100.0]),                               # an empty box
               (1, ["hv_select", A, np.array([1.0, 2.5]), lo, ref, 2.0]),
               (1, ["hv_select", A, np.array([1.0, 7.0]), lo, ref, 2.0, 100.0]),               # row 7 of 6
               (1, ["hv_select", A, EMPTY, lo, ref, 2.0, 0.0]),
               (1, ["hv_select", A, EMPTY, lo, ref, 0.0, 100.0]),
               (1, ["hv_select", A, EMPTY, lo, ref, 1025.0, 100.0]),
               (1, ["hv_select", A, EMPTY, lo, ref, 2.5]),
               (1, ["hv_select", A, EMPTY, lo, ref, 2.0, 100.0, 1.5]),
               (1, ["hv_select", A, EMPTY, lo[:2], ref, 2.0]),
               (1, ["hv_select", A, EMPTY, lo, ref, 2.0, 100.0, 0.0, -1.0, 1.0])])
    assert not res[0][0] and res[0][1][0] == "mpct:arg" and "usage" in res[0][1][1]
    assert res[1] == (False, ("mpct:hv_select", "k must be 1 .. MPCT_PARETO_MAX_OBJ"))
    assert not res[2][0] and res[2][1][0] == "mpct:hv_select" and "lo[j] < ref[j]" in res[2][1][1]
    assert not res[3][0] and res[3][1][0] == "mpct:arg" and "1-based" in res[3][1][1]
    assert not res[4][0] and res[4][1][0] == "mpct:hv_select" and "members" in res[4][1][1]
    assert not res[5][0] and res[5][1][0] == "mpct:hv_select" and "n_samples < 1" in res[5][1][1]
    assert res[6] == (False, ("mpct:hv_select", "n_pick < 1"))
    assert not res[7][0] and res[7][1][0] == "mpct:hv_select" and "MPCT_HVSEL_MAX_PICKS" in res[7][1][1]
    assert not res[8][0] and res[8][1][0] == "mpct:arg" and "'n_pick'" in res[8][1][1]
    assert not res[9][0] and res[9][1][0] == "mpct:arg" and "'seed'" in res[9][1][1]
    assert not res[10][0] and res[10][1][0] == "mpct:arg" and "'lo'" in res[10][1][1]
    assert not res[11][0] and res[11][1][0] == "mpct:arg" and "usage" in res[11][1][1]
    if not has_gpu:
        res = mex([(1, ["hv_select", A, EMPTY, lo, ref, 2.0, 100.0])])
        assert not res[0][0] and res[0][1][0] == "mpct:hv_select" and "device" in res[0][1][1]


def test_mex_hv_select_of_an_empty_table(built):
    """C = 0, so M = 0: the library needs no device, and the struct has every field at its end-of-selection fill"""
    got = _struct_calls([(1, ["hv_select", np.zeros((0, 2)), EMPTY, np.zeros(2), np.array([1.0, 2.0]), 3.0, 50.0])])[0]
    assert set(got) == NAMES
    assert got["n_picked"].ravel().tolist() == [0.0] and got["n_covered_all"].ravel().tolist() == [0.0]
    assert got["n_samples"].ravel().tolist() == [50.0] and got["volume"].ravel().tolist() == [2.0]
    for f, fill in (("pos", 0.0), ("index", 0.0), ("gain", 0.0), ("covered", 0.0), ("hv", 0.0), ("ties", 0.0)):
        assert got[f].shape == (3, 1) and got[f][:, 0].tolist() == [fill] * 3, f
    assert got["share"].shape == (3, 1) and np.isnan(got["share"]).all()


@pytest.mark.gpu
def test_mex_hv_select_matches_reference(built, has_gpu):
    if not has_gpu:
        pytest.skip("no GPU")
    A = R.generated(300, 3, 30)         # not symmetric in its columns: a transposition error would show
    A[:, 1] += np.arange(300) % 7
    A[11, 2] = np.nan
    lo, ref = np.zeros(3), np.array([29.5, 35.5, 29.5])
    mem0 = np.random.default_rng(5).permutation(300)[:120]
    mem0[7] = -1                        # skipped: 0 in MATLAB's 1-based vector
    N, seed = 4000, 77
    got = _struct_calls([(1, ["hv_select", A, (mem0 + 1).astype(float), lo, ref, 12.0, float(N), float(seed), 0.0]),
                         (1, ["hv_select", A, EMPTY, lo, ref, 40.0, float(N), float(seed)])])
    for g, members, K in zip(got, (mem0, None), (12, 40)):
        want = S.select_np(A, members, lo, ref, N, seed, K)
        n = want["n_picked"]
        assert set(g) == NAMES and all(g[f].shape == (K, 1) for f in ("pos", "index", "gain", "covered", "hv", "ties", "share"))
        back = dict(n_picked=int(g["n_picked"].ravel()[0]), n_covered_all=int(g["n_covered_all"].ravel()[0]),
                    pos=(g["pos"][:, 0] - 1).astype(np.int32), index=(g["index"][:, 0] - 1).astype(np.int32),
                    gain=g["gain"][:, 0].astype(np.int64), covered=g["covered"][:, 0].astype(np.int64),
                    hv=g["hv"][:, 0], ties=g["ties"][:, 0].astype(np.int32))
        S.compare(back, want, "mex")
        assert n >= 8 and (g["pos"][:n, 0] >= 1).all() and (g["pos"][n:, 0] == 0).all() and (g["index"][n:, 0] == 0).all()
        assert g["volume"].ravel()[0] == R.volume(lo, ref) and g["n_samples"].ravel()[0] == N
        np.testing.assert_array_equal(g["share"][:, 0], want["covered"] / np.float64(want["n_covered_all"]))
    assert got[1]["n_picked"].ravel()[0] < 40           # the second call runs past the end of the selection
    assert 8 not in got[0]["pos"][:, 0]                 # the skipped entry (position 7, 1-based 8) is never picked
