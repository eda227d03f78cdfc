"""CPU, no device: the contract of the closed-loop performance indices (include/mpct.h).  The reference of
tests/indices_ref.py has the properties it should have on hand-made rows, its vectorised form equals the
scalar one bit for bit and passes the order-free bound; the header, the ctypes list and the library carry
the four exports; every argument error comes back with the documented code in the documented order without
a device; the host entries fail loudly without a GPU; IndexResult.costs folds as specified."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import indices_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXPORTS = ("mpct_indices_device", "mpct_indices", "mpct_eval_indices", "mpct_eval_indices_device")
EINVAL, EDEVICE, ERANGE = -1, -3, -4


def _row(y, r, t0=0, rel=0.0, ab=0.0):
    return R.output_row(np.asarray(y, dtype=float), np.asarray(r, dtype=float), t0, rel, ab)


def test_reference_on_hand_made_rows():
    # a constant error: iae = n |e|, ise = n e^2, itae = |e| n (n - 1) / 2
    n, t0 = 70, 3
    got = _row(np.full(n, 1.5), np.full(n, 2.0), t0)
    assert got["iae"] == (n - t0) * 0.5 and got["ise"] == (n - t0) * 0.25
    assert got["itae"] == 0.5 * (n - t0) * (n - t0 - 1) / 2 and got["emax"] == 0.5 and got["t_emax"] == t0
    assert got["e_final"] == -0.5
    # always inside the band: settle = t0 (d = 0 here, so the absolute band alone decides)
    assert _row(np.full(20, 1.0), np.full(20, 1.0), 4, 0.02, 0.0)["settle"] == 4
    y = np.array([0.0, 0.5, 1.3, 0.9, 1.05, 1.01, 1.0, 1.0])
    r = np.array([0.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0])
    got = _row(y, r, 0, 0.02, 0.0)                    # d = 1, band = 0.02
    assert got["settle"] == 5                         # the last violating index is 4 (1.05)
    assert got["over"] == pytest.approx(0.3) and got["over"] == 1.3 - 1.0 and got["t_emax"] == 1 and got["emax"] == 0.5
    # a last sample outside the band: nit
    y2 = y.copy()
    y2[-1] = 1.5
    assert _row(y2, r, 0, 0.02, 0.0)["settle"] == 8
    # a downward step: the overshoot is measured in the step's direction
    got = _row(-y, -r, 0, 0.02, 0.0)
    assert got["over"] == 1.3 - 1.0 and got["settle"] == 5
    # never past the reference: +0.0
    got = _row([0.0, 0.5, 0.75, 1.0], [1.0, 1.0, 1.0, 1.0])
    assert got["over"] == 0.0 and np.signbit(got["over"]) == False  # noqa: E712
    # sigma = 0 (y(t0) = r_f): over = emax
    got = _row([0.0, 0.25, -0.75, 0.0], [0.0, 0.0, 0.0, 0.0])
    assert got["over"] == got["emax"] == 0.75
    # t_emax: the first of equal maxima, also across the 64-sample blocks and of opposite signs
    y = np.zeros(200)
    y[[150, 70, 135]] = (2.0, -2.0, 2.0)
    got = _row(y, np.zeros(200), 5)
    assert got["t_emax"] == 70 and got["emax"] == 2.0
    # samples exactly on the band edge are inside; one ulp beyond is outside
    y = np.array([0.0, 2.0, 1.25, 1.0])
    r = np.ones(4)
    assert _row(y, r, 0, 0.25, 0.0)["settle"] == 2
    y[2] = np.nextafter(1.25, 2.0)
    assert _row(y, r, 0, 0.25, 0.0)["settle"] == 3


def test_reference_input_rows_and_validity():
    got = R.input_row(np.array([5.0, 1.0, 3.0, 2.0]), 1)
    assert (got["tv"], got["du2"], got["dumax"], got["u_lo"], got["u_hi"]) == (3.0, 5.0, 2.0, 1.0, 3.0)
    # nit - t0 = 1: the du range is empty
    got = R.input_row(np.array([5.0, 1.0, 3.0, 2.0]), 3)
    assert (got["tv"], got["du2"], got["dumax"], got["u_lo"], got["u_hi"]) == (0.0, 0.0, 0.0, 2.0, 2.0)
    got = R.input_row(np.array([-0.0, 0.0, -0.0]), 0)
    assert not np.signbit(got["u_lo"]) and not np.signbit(got["u_hi"])
    # one non-finite sample inside [t0, nit) invalidates its own row only; one before t0 nothing
    for badval in (np.nan, np.inf, -np.inf):
        y, u, r = R.generated(4, 2, 2, 2, 40, seed=3)
        y[1], u[1], y[2], u[3] = y[0], u[0], y[0], u[0]      # no planted invalid rows
        r[:] = np.nan_to_num(r)
        want = R.indices_np(y, u, r, 5, 0.1, 0.0)
        assert all(np.isfinite(want[f]).all() for f in R.Y_FIELDS + R.U_FIELDS)
        y1, u1, r1 = y.copy(), u.copy(), r.copy()
        y1[2, 1, 4], u1[0, 1, 0], r1[1, 0, 3] = badval, badval, badval       # all before t0 = 5
        R.assert_bitwise(R.indices_np(y1, u1, r1, 5, 0.1, 0.0), want, what="before t0")
        y1[2, 1, 5], u1[0, 1, 39] = badval, badval
        got = R.indices_np(y1, u1, r1, 5, 0.1, 0.0)
        for f in R.Y_FIELDS:
            bad = np.zeros((4, 2), dtype=bool)
            bad[2, 1] = True
            assert ((got[f] == -1) if f in R.INT_FIELDS else np.isnan(got[f]))[bad].all()
            assert (R.bits(got[f])[~bad] == R.bits(want[f])[~bad]).all()
        for f in R.U_FIELDS:
            assert np.isnan(got[f][0, 1]) and np.isnan(got[f]).sum() == 1
        r1[1, 0, 20] = badval                                  # a reference sample: every row that reads it
        got = R.indices_np(y1, u1, r1, 5, 0.1, 0.0)
        assert np.isnan(got["iae"]).tolist() == [[False, False], [True, False], [False, True], [True, False]]


CASES = [(S, nref, my, nu, nit, t0) for (S, nref, my, nu) in ((6, 3, 3, 2), (5, 1, 1, 1))
         for nit in (1, 2, 63, 64, 65, 130, 500) for t0 in sorted({0, 1, nit - 1}) if t0 < nit]


@pytest.mark.parametrize("S,nref,my,nu,nit,t0", CASES)
def test_vectorised_equals_scalar_and_order_free_bound(S, nref, my, nu, nit, t0):
    y, u, r = R.generated(S, nref, my, nu, nit)
    want = R.indices_scalar(y, u, r, t0, R.BAND_REL, R.BAND_ABS)
    got = R.indices_np(y, u, r, t0, R.BAND_REL, R.BAND_ABS)
    R.assert_bitwise(got, want, what="vectorised against scalar")
    assert R.check_order_free(got, y, u, r, t0) > 0
    assert np.isnan(got["iae"][1]).all() and (got["settle"][1] == -1).all() and np.isnan(got["tv"][1]).all()


def test_generated_data_has_the_edges():
    y, u, r = R.generated(6, 3, 3, 2, 130)
    got = R.indices_np(y, u, r, 0, R.BAND_REL, R.BAND_ABS)
    rz = np.nan_to_num(r)
    assert rz.any(axis=2).sum() >= 5 and (np.argmax(rz != 0, axis=2)[rz.any(axis=2)] > 0).all()   # steps start after 0
    e = np.abs(y - r[np.arange(6) % 3])
    assert e[0, 0, 9] == e[0, 0, 11] == got["emax"][0, 0] and got["t_emax"][0, 0] == 9      # a tie in |e|
    band = R.BAND_REL * abs(r[0, 0, -1] - y[0, 0, 0]) + R.BAND_ABS
    assert abs(y[0, 0, 123] - r[0, 0, -1]) == band and got["settle"][0, 0] <= 123           # on the edge: inside
    assert got["settle"][3, 1] == 128                                                        # one ulp outside at 127
    assert np.isnan(got["iae"][2, 2]) and np.isnan(got["tv"][3, 0]) and np.isnan(got["iae"][1]).all()
    assert np.isnan(got["iae"][2, 2]) and not np.isnan(R.indices_np(y, u, r, 1, 0.1, 0.1)["iae"][5, 2])  # NaN r(0)
    assert np.signbit(u[4, 0]).any() and not np.signbit(got["u_lo"][4, 0]) and got["u_hi"][4, 0] == 0
    reg = ~rz[np.arange(6) % 3].any(-1) & ~np.isnan(got["iae"])      # regulated channels from rest: sigma = 0
    assert np.signbit(y[reg][:, 0]).all() and reg.sum() >= 3 and (got["over"][reg] == got["emax"][reg]).all()
    # sums of the full-precision rows round: another order gives other bits somewhere
    naive = np.abs(y - r[np.arange(6) % 3]).sum(-1)
    assert (naive[np.isfinite(naive)] != got["iae"][np.isfinite(naive)]).any()


def test_header_declares_and_lib_exports(built):
    from mpct import _lib

    src = open(os.path.join(ROOT, "include", "mpct.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    so = C.CDLL(_lib.lib_path())
    for f in EXPORTS:
        assert re.search(r"\bint32_t %s\s*\(" % f, code), f
        assert f in _lib.EXPORTS
        assert C.cast(getattr(so, f), C.c_void_p).value
    m = re.search(r"typedef struct mpct_index_result \{(.*?)\} mpct_index_result;", code, flags=re.S)
    assert re.findall(r"(double|int32_t)\* (\w+);", m.group(1)) == [
        ("int32_t" if i else "double", n) for n, _, i in _lib.INDEX_FIELDS]
    assert [n for n, _, _ in _lib.INDEX_FIELDS] == list(R.Y_FIELDS + R.U_FIELDS)
    assert re.search(r"typedef struct mpct_index_params \{\s*int32_t t0;\s*double band_rel;\s*double band_abs;\s*\}", code)
    assert re.search(r"#define MPCT_INDEX_MAX_ROWS 2147483647\b", code) and _lib.INDEX_MAX_ROWS == 2147483647
    assert re.search(r"#define MPCT_INDEX_SCRATCH_BYTES 268435456\b", code) and _lib.INDEX_SCRATCH_BYTES == 1 << 28
    assert "mpct_internal_index_budget" not in src and C.cast(so.mpct_internal_index_budget, C.c_void_p).value
    assert _lib.load().mpct_abi_version() == 7
    # the contract's points are in the header
    for phrase in ("Row validity", "No contraction", "Summation order", "pairwise tree", "Argument errors"):
        assert phrase in src, phrase


def test_indices_argument_errors_in_documented_order(built):
    """Each call also carries every LATER error of the header's list, so the code that comes back shows the
    order of the checks.  Host pointers: nothing is dereferenced before the checks have passed."""
    from mpct import _lib

    lib = _lib.load()
    buf = np.zeros(64)
    ibuf = np.zeros(64, dtype=np.int32)
    d, i = buf.ctypes.data_as(_lib.c_double_p), ibuf.ctypes.data_as(_lib.c_int32_p)
    none = _lib.MpctIndexResult()
    both = _lib.MpctIndexResult(iae=d, settle=i, tv=d)
    only_y, only_u = _lib.MpctIndexResult(settle=i), _lib.MpctIndexResult(dumax=d)
    P = _lib.MpctIndexParams
    a = buf.ctypes.data
    big = 1 << 31
    #          y     u     r     S   nref my  nu  nit  params              out
    steps = [((None, None, None, -3, 0, 2, 1, 10, None, none), EINVAL, "null params"),
             ((None, None, None, -3, 0, 2, 1, 10, P(10, -1.0, 0.0), none), EINVAL, "bad shape"),
             ((None, None, None, 4, 0, -1, 1, 10, P(10, -1.0, 0.0), none), EINVAL, "bad shape"),
             ((None, None, None, 4, 0, 2, 1, 0, P(10, -1.0, 0.0), none), EINVAL, "bad shape"),
             ((None, None, None, 4, 0, 2, 1, 10, P(10, -1.0, 0.0), none), EINVAL, "nref < 1"),
             ((None, None, None, 4, 3, 2, 1, 10, P(10, -1.0, 0.0), none), EINVAL, "multiple of nref"),
             ((None, None, None, 4, 2, 2, 1, 10, P(10, -1.0, 0.0), none), EINVAL, "t0 must be"),
             ((None, None, None, 4, 2, 2, 1, 10, P(-1, -1.0, 0.0), none), EINVAL, "t0 must be"),
             ((None, None, None, 4, 2, 2, 1, 10, P(9, -1.0, 0.0), none), EINVAL, "band_rel and band_abs"),
             ((None, None, None, 4, 2, 2, 1, 10, P(9, 0.0, np.nan), none), EINVAL, "band_rel and band_abs"),
             ((None, None, None, 4, 2, 2, 1, 10, P(9, np.inf, 0.0), none), EINVAL, "band_rel and band_abs"),
             ((None, None, None, 4, 2, 2, 1, 10, P(9, 0.0, 0.0), none), EINVAL, "no output pointer"),
             ((None, None, None, 4, 2, 2, 1, 10, P(9, 0.0, 0.0), None), EINVAL, "no output pointer"),
             ((None, a, None, big, 2, 2, 1, 10, P(9, 0.0, 0.0), both), EINVAL, "output-row field"),
             ((a, a, None, big, 2, 2, 1, 10, P(9, 0.0, 0.0), both), EINVAL, "output-row field"),
             ((a, a, a, big, 2, 0, 1, 10, P(9, 0.0, 0.0), only_y), EINVAL, "output-row field"),
             ((a, None, a, big, 2, 2, 1, 10, P(9, 0.0, 0.0), both), EINVAL, "input-row field"),
             ((a, a, a, big, 2, 2, 0, 10, P(9, 0.0, 0.0), only_u), EINVAL, "input-row field"),
             ((a, a, a, big, 2, 2, 1, 10, P(9, 0.0, 0.0), both), ERANGE, "MPCT_INDEX_MAX_ROWS"),
             ((None, a, None, big, 2, 1, 1, 10, P(9, 0.0, 0.0), only_u), ERANGE, "MPCT_INDEX_MAX_ROWS")]
    for args, code, msg in steps:
        y, u, r, S, nref, my, nu, nit, p, out = args
        pp = C.byref(p) if p is not None else None
        oo = C.byref(out) if out is not None else None
        for rc in (lib.mpct_indices_device(y, u, r, S, nref, my, nu, nit, pp, oo, None),
                   lib.mpct_indices(y, u, r, S, nref, my, nu, nit, pp, -1, oo)):
            assert rc == code, (args[3:8], rc, _lib.last_error())
            assert msg in _lib.last_error(), (args[3:8], _lib.last_error())
    # S = 0 is fine without trajectories and without a device, and writes nothing
    p = P(0, 0.02, 0.0)
    assert lib.mpct_indices_device(None, None, None, 0, 1, 2, 1, 10, C.byref(p), C.byref(both), None) == 0
    assert lib.mpct_indices(None, None, None, 0, 1, 2, 1, 10, C.byref(p), -1, C.byref(both)) == 0
    assert (buf == 0).all() and (ibuf == 0).all()


@pytest.fixture(scope="module")
def small_scenario(built):
    from mpct.scenarios import shell3x3

    sc, r, _ = shell3x3(n2_max=10, nu_max=3, nit=40)
    yield sc, r
    sc.close()


def test_eval_indices_argument_errors_in_documented_order(small_scenario):
    from mpct import _lib

    sc, r = small_scenario
    lib = _lib.load()
    buf = np.zeros(4 * 3 * 40)
    d = buf.ctypes.data_as(_lib.c_double_p)
    N2, Nu = np.array([5, 6], dtype=np.int32), np.array([2, 2], dtype=np.int32)
    dl, lm = np.ones((2, 3)), np.ones((2, 3))
    refs = np.ascontiguousarray(r[None])
    P, O = _lib.MpctIndexParams, _lib.MpctOpts
    none, some = _lib.MpctIndexResult(), _lib.MpctIndexResult(iae=d)
    traj = _lib.MpctResult(y=d)
    ol = O(1, 0, 0, -1, 0.0)
    cl = O(0, 0, 0, -1, 0.0)

    def call(h, C_, nref, refs_p, opts, p, res, out):
        a = [h, C_, N2.ctypes.data, Nu.ctypes.data, dl.ctypes.data, lm.ctypes.data, nref, refs_p, None,
             C.byref(opts) if opts is not None else None, C.byref(p) if p is not None else None,
             C.byref(res) if res is not None else None, C.byref(out) if out is not None else None]
        return lib.mpct_eval_indices(*a), lib.mpct_eval_indices_device(*(a + [None]))

    rp = refs.ctypes.data
    steps = [((None, -1, 0, None, ol, None, traj, none), "null scenario"),
             ((sc.handle, -1, 0, None, ol, None, traj, none), "null params"),
             ((sc.handle, -1, 0, None, ol, P(40, -1.0, 0.0), traj, none), "open_loop must be 0"),
             ((sc.handle, -1, 0, None, cl, P(40, -1.0, 0.0), traj, none), "trajectory pointers of res"),
             ((sc.handle, -1, 0, None, cl, P(40, -1.0, 0.0), None, none), "C < 0 or nref < 1"),
             ((sc.handle, 2, 0, None, cl, P(40, -1.0, 0.0), None, none), "C < 0 or nref < 1"),
             ((sc.handle, 2, 1, None, cl, P(40, -1.0, 0.0), None, none), "null input pointer"),
             ((sc.handle, 2, 1, rp, cl, P(40, -1.0, 0.0), None, none), "t0 must be"),
             ((sc.handle, 2, 1, rp, cl, P(39, -1.0, 0.0), None, none), "band_rel and band_abs"),
             ((sc.handle, 2, 1, rp, None, P(39, 0.0, 0.0), None, none), "no output pointer"),
             ((sc.handle, 2, 1, rp, None, P(39, 0.0, 0.0), None, None), "no output pointer")]
    for args, msg in steps:
        for rc in call(*args):
            assert rc == EINVAL, (msg, rc, _lib.last_error())
            assert msg in _lib.last_error(), (msg, _lib.last_error())
    assert (buf == 0).all()


def test_no_device_is_reported(small_scenario, has_gpu):
    from mpct.engine import MpctError, eval_indices, indices

    if has_gpu:
        pytest.skip("a GPU is present: the no-device message cannot show")
    sc, r = small_scenario
    y, u, rr = R.generated(4, 2, 2, 1, 30)
    with pytest.raises(MpctError, match=r"\(-3\).*HIP device"):
        indices(y, u, rr)
    with pytest.raises(MpctError, match=r"\(-3\).*(GPU|HIP device)"):
        eval_indices(sc, [5, 6], [2, 2], np.ones((2, 3)), np.ones((2, 3)), r[None])
    # an empty batch needs no device
    res = eval_indices(sc, np.zeros(0, dtype=np.int32), np.zeros(0, dtype=np.int32), np.zeros((0, 3)), np.zeros((0, 3)),
                       r[None])
    assert res.iae.shape == (0, 1, 3) and res.tv.shape == (0, 1, 3)


def test_index_result_costs():
    from mpct.engine import IndexResult

    nit, t0 = 50, 5
    iae = np.arange(12.0).reshape(2, 2, 3)
    settle = np.array([[[10, 20, 5], [7, 8, 9]], [[10, 50, 5], [7, 8, 9]]], dtype=np.int32)     # 50 = nit: unsettled
    e_final = -iae
    tv = np.arange(8.0).reshape(2, 2, 2)
    tv[1, 0, 1] = np.nan
    res = IndexResult(iae=iae, settle=settle, e_final=e_final, tv=tv, nit=nit, t0=t0)
    got = res.costs(["iae", "settle", "e_final", "tv"], reduce="max")
    assert got.shape == (2, 4) and got.dtype == np.float64
    np.testing.assert_array_equal(got[0], [5.0, 15.0, 5.0, 3.0])
    np.testing.assert_array_equal(got[1], [11.0, np.nan, 11.0, np.nan])
    got = res.costs(["iae", "settle", "tv"], reduce="sum")
    np.testing.assert_array_equal(got[0], [15.0, 10 + 20 + 5 + 7 + 8 + 9 - 6 * t0, 6.0])
    assert np.isnan(got[1, 1]) and np.isnan(got[1, 2])
    inv = IndexResult(settle=np.full((1, 1, 2), -1, dtype=np.int32), nit=nit, t0=t0)
    assert np.isnan(inv.costs(["settle"])).all()
    with pytest.raises(ValueError):
        res.costs(["iae"], reduce="mean")
    with pytest.raises(ValueError):
        res.costs(["overshoot"])
    with pytest.raises(ValueError):
        res.costs(["du2"])                # not in this result
