"""The MEX gateway's 'hypervolume_exact' command (matlab/mpct_mex.c) through the MX stub, built and driven like
tests/test_mex_hypervolume.py: argument errors without a device (the library's messages for four objectives
and for an empty box), the struct of an empty table (which needs no device), and on the GPU the struct's
fields against tests/hvx_ref.py's exact rational values: 1-based members with 0 for a skipped entry, [] for
all rows, the column-major C x k input transposed in the gateway."""
from fractions import Fraction

import numpy as np
import pytest

import hvx_ref as R
from test_mex import mex
from test_mex_hypervolume import _struct_calls

EMPTY = np.zeros((0, 0))


def test_mex_hypervolume_exact_argument_errors(built, has_gpu):
    A = np.random.default_rng(3).random((6, 3))
    lo, ref = np.zeros(3), np.ones(3)
    res = mex([(1, ["hypervolume_exact", A, EMPTY, lo]),
               (1, ["hypervolume_exact", np.ones((4, 4)), EMPTY, np.zeros(4), np.ones(4)]),   # the library's MPCT_ERANGE
               (1, ["hypervolume_exact", A, EMPTY, lo, lo]),                                    # an empty box
               (1, ["hypervolume_exact", A, np.array([1.0, 2.5]), lo, ref]),
               (1, ["hypervolume_exact", A, np.array([1.0, 7.0]), lo, ref]),                    # row 7 of 6
               (1, ["hypervolume_exact", A, EMPTY, lo, ref, 0.5]),
               (1, ["hypervolume_exact", A, EMPTY, lo[:2], ref]),
               (1, ["hypervolume_exact", A, EMPTY, lo, ref, -1.0, 1.0])])
    assert not res[0][0] and res[0][1][0] == "mpct:arg" and "usage" in res[0][1][1]
    assert not res[1][0] and res[1][1][0] == "mpct:hypervolume_exact" and "MPCT_HVX_MAX_OBJ" in res[1][1][1]
    assert not res[2][0] and res[2][1][0] == "mpct:hypervolume_exact" and "lo[j] < ref[j]" in res[2][1][1]
    assert not res[3][0] and res[3][1][0] == "mpct:arg" and "1-based" in res[3][1][1]
    assert not res[4][0] and res[4][1][0] == "mpct:hypervolume_exact" and "members" in res[4][1][1]
    assert not res[5][0] and res[5][1][0] == "mpct:arg" and "'device'" in res[5][1][1]
    assert not res[6][0] and res[6][1][0] == "mpct:arg" and "'lo'" in res[6][1][1]
    assert not res[7][0] and res[7][1][0] == "mpct:arg" and "usage" in res[7][1][1]
    if not has_gpu:
        res = mex([(1, ["hypervolume_exact", A, EMPTY, lo, ref])])
        assert not res[0][0] and res[0][1][0] == "mpct:hypervolume_exact" and "device" in res[0][1][1]


def test_mex_hypervolume_exact_of_an_empty_table(built):
    """C = 0, so M = 0: the library needs no device, and the struct has every field"""
    got = _struct_calls([(1, ["hypervolume_exact", np.zeros((0, 2)), EMPTY, np.zeros(2), np.array([1.0, 2.0])])])[0]
    assert set(got) == {"hv", "excl", "n_active"}
    assert got["hv"].ravel().tolist() == [0.0] and got["n_active"].ravel().tolist() == [0.0]
    assert got["excl"].size == 0


@pytest.mark.gpu
def test_mex_hypervolume_exact_matches_reference(built, has_gpu):
    if not has_gpu:
        pytest.skip("no GPU")
    rng = np.random.default_rng(9)
    A = rng.random((60, 3)) * np.array([1.0, 3.0, 0.5])   # not symmetric in its columns: a transposition error would show
    A[11, 2] = np.nan
    lo, ref = np.array([0.0, 0.25, 0.0]), np.array([1.0, 2.5, 0.5])
    mem0 = rng.permutation(60)[:40]
    mem0[7] = -1                        # skipped: 0 in MATLAB's 1-based vector
    got = _struct_calls([(1, ["hypervolume_exact", A, (mem0 + 1).astype(float), lo, ref, 0.0]),
                         (1, ["hypervolume_exact", A[:45], EMPTY, lo, ref])])
    vol = 1.0 * 2.25 * 0.5
    for g, (table, members) in zip(got, ((A, mem0), (A[:45], None))):
        HV, EXCL, NA = R.exact_fraction(table, members, lo, ref)
        M = 40 if members is not None else 45
        bd = R.bound(M, vol)
        assert g["excl"].shape == (M, 1) and int(g["n_active"].ravel()[0]) == NA and NA > 5
        assert abs(Fraction(float(g["hv"].ravel()[0])) - HV) <= bd and HV > 0
        for e, E in zip(g["excl"][:, 0].tolist(), EXCL):
            assert abs(Fraction(e) - E) <= bd and (E != 0 or e == 0.0)
        assert sum(1 for E in EXCL if E > 0) > 3
    assert got[0]["excl"][7, 0] == 0
