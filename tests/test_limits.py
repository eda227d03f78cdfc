"""CPU, no device: the contract of the limit indices (include/mpct.h).  The reference of tests/limits_ref.py has
the properties it should have on hand-made rows; the generator's rows have the properties they are named for;
a copy of the reference with one planted mistake fails the bitwise comparison on the generated data; the
header, the ctypes list and the library carry the six exports; every argument error comes back with the
documented code in the documented order without a device; empty calls need no device; LimitResult.costs
folds as specified."""
import ctypes as C
import os
import re
import types

import numpy as np
import pytest

import limits_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXPORTS = ("mpct_limit_indices_device", "mpct_limit_indices", "mpct_eval_limit_indices", "mpct_eval_limit_indices_device",
           "mpct_eval_robust_limit_indices", "mpct_eval_robust_limit_indices_device")
EINVAL, EDEVICE, ERANGE = -1, -3, -4
INF = float("inf")

# the shapes of the GPU test: row counts 1 and 5 (partial workgroups), my = 0 and nu = 0, and a full one
SHAPES = [(5, 4, 2), (1, 1, 0), (5, 1, 0), (1, 0, 1), (5, 0, 1)]
CASES = [(S, my, nu, nit, t0) for (S, my, nu) in SHAPES for nit in (1, 2, 63, 64, 65, 128, 129, 130, 500)
         for t0 in sorted({0, 1, nit - 1}) if t0 < nit]


def test_reference_on_hand_made_output_rows():
    y = np.array([0.0, 1.5, 2.0, 0.5, -1.0, 0.25])
    got = R.output_row(y, -0.5, 1.0, 0, 0.25)
    assert got["viol"] == 0.5 + 1.0 + 0.5 and got["viol2"] == 0.25 + 1.0 + 0.25
    assert got["vmax"] == 1.0 and got["t_vmax"] == 2
    assert got["n_out"] == 3 and got["t_in"] == 5 and got["y_margin"] == -1.0
    # from t0 = 3 on: only the excursion below the band is left
    got = R.output_row(y, -0.5, 1.0, 3, 0.25)
    assert (got["viol"], got["vmax"], got["t_vmax"], got["n_out"], got["t_in"], got["y_margin"]) == (0.5, 0.5, 4, 1, 5, -0.5)
    # never outside: zeros, t_vmax = t_in = t0, a positive margin
    got = R.output_row(y, -2.0, 3.0, 2, 0.0)
    assert (got["viol"], got["viol2"], got["vmax"], got["t_vmax"], got["n_out"], got["t_in"]) == (0.0, 0.0, 0.0, 2, 0, 2)
    assert got["y_margin"] == 1.0
    # outside at the last sample: t_in = nit
    assert R.output_row(np.array([0.0, 0.0, 2.0]), -1.0, 1.0, 0, 0.0)["t_in"] == 3
    # ex exactly at out_tol is inside, one ulp above it is outside
    assert R.output_row(np.array([1.25]), 0.0, 1.0, 0, 0.25)["n_out"] == 0
    assert R.output_row(np.array([np.nextafter(1.25, 2.0)]), 0.0, 1.0, 0, 0.25)["n_out"] == 1
    # the first of equal maxima, whichever side of the band
    assert R.output_row(np.array([0.0, -2.0, 3.0, 3.0]), 0.0, 1.0, 0, 0.0)["t_vmax"] == 1
    # one-sided and no bounds
    got = R.output_row(y, -INF, 1.0, 0, 0.0)
    assert got["viol"] == 1.5 and got["y_margin"] == -1.0
    got = R.output_row(y, -INF, INF, 0, 0.0)
    assert got["viol"] == 0.0 and got["y_margin"] == INF and got["t_in"] == 0 and got["t_vmax"] == 0
    # lo == hi: ex = |y - lo|, the margin -max|y - lo|
    got = R.output_row(np.array([0.5, 0.75, 0.0]), 0.5, 0.5, 0, 0.0)
    assert (got["viol"], got["vmax"], got["n_out"], got["y_margin"]) == (0.75, 0.5, 2, -0.5)
    # -0.0 against a zero bound: ex and the margin are +0.0
    got = R.output_row(np.array([-0.0, 0.0, -0.0]), 0.0, INF, 0, 0.0)
    assert got["viol"] == 0.0 and got["vmax"] == 0.0 and got["y_margin"] == 0.0
    assert not np.signbit(got["vmax"]) and not np.signbit(got["y_margin"]) and not np.signbit(got["viol"])
    # a non-finite sample in [t0, nit) invalidates the row; one before t0 does not
    for bad in (np.nan, np.inf, -np.inf):
        got = R.output_row(np.array([0.0, bad, 0.0]), -1.0, 1.0, 0, 0.0)
        assert all(got[f] == -1 for f in R.Y_FIELDS if f in R.INT_FIELDS)
        assert all(np.isnan(got[f]) for f in R.Y_FIELDS if f not in R.INT_FIELDS)
        assert R.output_row(np.array([0.0, bad, 0.0]), -1.0, 1.0, 2, 0.0)["viol"] == 0.0


def test_reference_on_hand_made_input_rows():
    u = np.array([0.0, 0.5, 0.5, 0.25, -1.0, -1.0, -1.0, 0.0])
    got = R.input_row(u, -1.0, 0.5, -0.25, 0.25, 0, 0.0)
    assert (got["n_lo"], got["n_hi"], got["sat_run"]) == (3, 2, 3)
    assert got["n_rate"] == 4            # +0.5, -0.25, -1.25, +1
    assert got["u_margin"] == 0.0 and got["du_margin"] == -1.0
    # a run over both bounds counts as one; a tolerance widens it
    got = R.input_row(np.array([0.5, -1.0, -1.0, 0.5, 0.0]), -1.0, 0.5, -INF, INF, 0, 0.0)
    assert (got["sat_run"], got["n_rate"], got["du_margin"]) == (4, 0, INF)
    got = R.input_row(np.array([0.5, 0.375, 0.25, 0.0]), -1.0, 0.5, -INF, INF, 0, 0.125)
    assert (got["n_hi"], got["sat_run"]) == (2, 2)
    # exactly at lo + sat_tol: at the bound; one ulp above: not
    assert R.input_row(np.array([-0.875]), -1.0, 0.5, -1.0, 1.0, 0, 0.125)["n_lo"] == 1
    assert R.input_row(np.array([np.nextafter(-0.875, 0.0)]), -1.0, 0.5, -1.0, 1.0, 0, 0.125)["n_lo"] == 0
    assert R.input_row(np.array([np.nextafter(-0.875, -1.0)]), -1.0, 0.5, -1.0, 1.0, 0, 0.125)["n_lo"] == 1
    # nit - t0 = 1: the du range is empty
    got = R.input_row(u, -1.0, 0.5, -0.25, 0.25, 7, 0.0)
    assert (got["n_rate"], got["du_margin"], got["u_margin"], got["sat_run"]) == (0, INF, 0.5, 0)
    # the sample before t0 is never read
    assert R.input_row(np.array([np.nan, 0.0, 0.25]), -1.0, 0.5, -0.25, 0.25, 1, 0.0)["n_rate"] == 1
    # -0.0 against a zero bound
    got = R.input_row(np.array([-0.0, 0.0, -0.0]), -INF, 0.0, -INF, INF, 0, 0.0)
    assert (got["n_hi"], got["sat_run"], got["u_margin"]) == (3, 3, 0.0) and not np.signbit(got["u_margin"])
    # runs across the 64-sample blocks
    u = np.zeros(200)
    u[60:70] = 0.5
    assert R.input_row(u, -1.0, 0.5, -INF, INF, 0, 0.0)["sat_run"] == 10
    assert R.input_row(u, -1.0, 0.5, -INF, INF, 62, 0.0)["sat_run"] == 8
    got = R.input_row(np.array([0.0, np.inf]), -1.0, 0.5, -INF, INF, 0, 0.0)
    assert got["n_lo"] == -1 and got["sat_run"] == -1 and np.isnan(got["u_margin"]) and np.isnan(got["du_margin"])


def test_generated_data_has_the_edges():
    for nit, t0 in ((130, 0), (130, 1), (500, 1)):
        n = nit - t0
        y, u, P = R.generated(5, 4, 2, nit, t0)
        got = R.limits_scalar(y, u, P, t0)
        for s, (name, _, want) in R.RUNS.items():
            assert got["sat_run"][s, 0] == want(n), name
        assert got["sat_run"][0, 1] == n and got["n_hi"][0, 1] == n and got["u_margin"][0, 1] == 0.0   # the whole row
        assert np.signbit(u[0, 1]).any() and not np.signbit(got["u_margin"][0, 1])
        assert got["n_lo"][0, 0] == 2                         # at lo + tol and one ulp below; one ulp above is not
        assert got["n_hi"][4, 0] == 6 and u[4, 0, nit - 1] == 0.5
        # outputs: ex at out_tol is inside, one ulp above outside, the first of three equal peaks
        assert y[0, 0, t0 + 5] - 1.0 == R.OUT_TOL and got["t_vmax"][0, 0] == t0 + 8 and got["vmax"][0, 0] == 2.0
        yy = y[0, 0].copy()
        yy[t0 + 7] = 0.0
        assert R.output_row(yy, -0.5, 1.0, t0, R.OUT_TOL)["n_out"] == got["n_out"][0, 0] - 1
        yy[t0 + 5] = 0.0
        assert R.output_row(yy, -0.5, 1.0, t0, R.OUT_TOL)["n_out"] == got["n_out"][0, 0] - 1
        assert got["y_margin"][3, 0] > 0 and got["n_out"][3, 0] == 0 and got["t_in"][3, 0] == t0
        assert got["t_in"][4, 0] == nit
        assert got["viol"][0, 1] > 0 and got["y_margin"][0, 1] < 0                    # lo == hi
        assert got["viol"][0, 2] == 0 and got["y_margin"][0, 2] == 0 and not np.signbit(got["y_margin"][0, 2])
        assert np.signbit(y[0, 2]).any()
        assert got["viol"][0, 3] == 0 and got["y_margin"][0, 3] == INF and got["t_vmax"][0, 3] == t0
        assert np.isinf(got["du_margin"][0, 1]) and got["n_rate"][0, 1] == 0
        # invalid rows beside valid ones
        assert np.isnan(got["viol"][1]).all() and (got["n_out"][1] == -1).all() and (got["sat_run"][1] == -1).all()
        assert np.isnan(got["viol"][2, 3]) and np.isfinite(got["viol"][2, :3]).all()
        assert got["n_hi"][2, 1] == -1 and got["n_hi"][2, 0] >= 0
        # the sums of the full-precision rows round: another order gives other bits somewhere
        ex = np.array([[R.excess(float(v), 0.5, 0.5) for v in y[s, 1, t0:]] for s in (0, 2, 3, 4)])
        assert (np.array([sum(row) for row in ex.tolist()]) != got["viol"][[0, 2, 3, 4], 1]).any()   # one accumulator
        assert R.check_order_free(got, y, P, t0) > 0
    # rate saturation and amplitude saturation arise in the walks as well
    y, u, P = R.generated(5, 1, 1, 64, 0)
    got = R.limits_scalar(y, u, P, 0)
    assert (got["n_rate"][[0, 2, 3, 4]] > 0).all() and (got["sat_run"] >= 2).any()


MISTAKES = [("uv - u_lo <= sat_tol", "uv - u_lo < sat_tol", "< for <= at the tolerance"),
            ("run = run + 1 if (at_lo or at_hi) else 0",
             "run = 0 if (t - t0) % 64 == 0 and t > t0 else run\n        run = run + 1 if (at_lo or at_hi) else 0",
             "sat_run reset at a block edge"),
            ("return m if m > 0.0 else 0.0", "return m", "ex without the clamp"),
            ("if x > out_tol:", "if x >= out_tol:", ">= for > at out_tol"),
            ("if x > vmax:", "if x >= vmax:", "the last of equal maxima")]


@pytest.mark.parametrize("old,new,what", MISTAKES, ids=[m[2] for m in MISTAKES])
def test_planted_mistake_fails_the_comparison(old, new, what):
    src = open(R.__file__).read()
    assert src.count(old) == 1, old
    bad = types.ModuleType("limits_ref_mistaken")
    bad.__file__ = R.__file__
    exec(compile(src.replace(old, new), R.__file__, "exec"), bad.__dict__)
    y, u, P = R.generated(5, 4, 2, 130, 1)
    want = R.limits_scalar(y, u, P, 1)
    R.assert_bitwise(R.limits_scalar(y, u, P, 1), want, what="the reference repeats itself")
    assert R.mismatches(bad.limits_scalar(y, u, P, 1), want), what


def test_header_declares_and_lib_exports(built):
    from mpct import _lib

    src = open(os.path.join(ROOT, "include", "mpct.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    so = C.CDLL(_lib.lib_path())
    for f in EXPORTS:
        assert re.search(r"\bint32_t %s\s*\(" % f, code), f
        assert f in _lib.EXPORTS and f in src.split("#ifndef MPCT_H")[0]
        assert C.cast(getattr(so, f), C.c_void_p).value
    m = re.search(r"typedef struct mpct_limit_result \{(.*?)\} mpct_limit_result;", code, flags=re.S)
    assert re.findall(r"(double|int32_t)\* (\w+);", m.group(1)) == [
        ("int32_t" if i else "double", n) for n, _, i in _lib.LIMIT_FIELDS]
    assert [n for n, _, _ in _lib.LIMIT_FIELDS] == list(R.Y_FIELDS + R.U_FIELDS)
    assert [n for n, y, _ in _lib.LIMIT_FIELDS if y] == list(R.Y_FIELDS)
    assert tuple(n for n, _, i in _lib.LIMIT_FIELDS if i) == R.INT_FIELDS
    for k, (n, _, _) in enumerate(_lib.LIMIT_FIELDS):
        assert re.search(r"#define MPCT_LX_%s %d\b" % (n.upper(), k), code), n
    m = re.search(r"typedef struct mpct_limit_params \{(.*?)\} mpct_limit_params;", code, flags=re.S)
    assert re.findall(r"(int32_t|double|const double\*) (\w+);", m.group(1)) == [
        ("int32_t", "t0"), ("double", "out_tol"), ("double", "sat_tol")] + [("const double*", b) for b in R.BOUNDS]
    assert [n for n, _ in _lib.MpctLimitParams._fields_] == ["t0", "out_tol", "sat_tol"] + list(R.BOUNDS)
    assert re.search(r"#define MPCT_LIMIT_MAX_CH 32\b", code) and _lib.LIMIT_MAX_CH == 32
    assert _lib.load().mpct_abi_version() == 7
    for phrase in ("Row validity", "No contraction", "Summation order", "Argument errors", "HOST"):
        assert phrase in src.split("Limit indices per simulation")[1], phrase


def _params(t0, out_tol=0.0, sat_tol=0.0, keep=None, **bounds):
    from mpct import _lib

    p = _lib.MpctLimitParams(t0, out_tol, sat_tol)
    for k, v in bounds.items():
        a = np.ascontiguousarray(v, dtype=np.float64)
        keep.append(a)
        setattr(p, k, a.ctypes.data_as(_lib.c_double_p))
    return p


def test_limit_indices_argument_errors_in_documented_order(built):
    """Each call also carries every LATER error of the header's list, so the code that comes back shows the
    order of the checks.  Host pointers: nothing is dereferenced before the checks have passed."""
    from mpct import _lib

    lib = _lib.load()
    buf = np.zeros(64)
    ibuf = np.zeros(64, dtype=np.int32)
    d, i = buf.ctypes.data_as(_lib.c_double_p), ibuf.ctypes.data_as(_lib.c_int32_p)
    none = _lib.MpctLimitResult()
    both = _lib.MpctLimitResult(viol=d, t_in=i, sat_run=i)
    only_y, only_u = _lib.MpctLimitResult(n_out=i), _lib.MpctLimitResult(u_margin=d)
    keep = []
    a = buf.ctypes.data
    big = 1 << 31
    nan2, ok2 = [0.0, np.nan], [0.0, 1.0]
    badp = lambda t0, **kw: _params(t0, -1.0, 0.0, keep, y_lo=nan2, **kw)      # noqa: E731 -- bad tolerance and bound
    #          y     u     S   my  nu  nit  params   out
    steps = [((None, None, -3, 2, 1, 10, None, none), EINVAL, "null params"),
             ((None, None, -3, 2, 1, 10, badp(10), none), EINVAL, "bad shape"),
             ((None, None, 4, -1, 1, 10, badp(10), none), EINVAL, "bad shape"),
             ((None, None, 4, 2, 1, 0, badp(10), none), EINVAL, "bad shape"),
             ((None, None, 4, 33, 1, 10, badp(10), none), EINVAL, "t0 must be"),
             ((None, None, 4, 33, 1, 10, badp(-1), none), EINVAL, "t0 must be"),
             ((None, None, 4, 33, 1, 10, badp(9), none), ERANGE, "MPCT_LIMIT_MAX_CH"),
             ((None, None, 4, 2, 33, 10, badp(9), none), ERANGE, "MPCT_LIMIT_MAX_CH"),
             ((None, None, 4, 2, 1, 10, badp(9), none), EINVAL, "out_tol and sat_tol"),
             ((None, None, 4, 2, 1, 10, _params(9, 0.0, np.nan, keep, y_lo=nan2), none), EINVAL, "out_tol and sat_tol"),
             ((None, None, 4, 2, 1, 10, _params(9, np.inf, 0.0, keep, y_lo=nan2), none), EINVAL, "out_tol and sat_tol"),
             ((None, None, 4, 2, 1, 10, _params(9, 0.0, 0.0, keep, y_lo=nan2), none), EINVAL, "bad bound"),
             ((None, None, 4, 2, 1, 10, _params(9, 0.0, 0.0, keep, y_hi=nan2), none), EINVAL, "bad bound"),
             ((None, None, 4, 2, 1, 10, _params(9, 0.0, 0.0, keep, y_lo=ok2, y_hi=[0.0, 0.5]), none), EINVAL, "bad bound"),
             ((None, None, 4, 2, 1, 10, _params(9, 0.0, 0.0, keep, u_lo=[INF]), none), EINVAL, "bad bound"),
             ((None, None, 4, 2, 1, 10, _params(9, 0.0, 0.0, keep, u_hi=[-INF]), none), EINVAL, "bad bound"),
             ((None, None, 4, 2, 1, 10, _params(9, 0.0, 0.0, keep, du_lo=[0.5], du_hi=[0.25]), none), EINVAL, "bad bound"),
             ((None, None, 4, 2, 1, 10, _params(9, 0.0, 0.0, keep, du_lo=[np.nan]), none), EINVAL, "bad bound"),
             ((None, None, 4, 2, 1, 10, _params(9, 0.0, 0.0, keep, y_lo=ok2, y_hi=ok2), none), EINVAL, "no output pointer"),
             ((None, None, 4, 2, 1, 10, _params(9, 0.0, 0.0, keep), None), EINVAL, "no output pointer"),
             ((None, a, big, 2, 1, 10, _params(9, 0.0, 0.0, keep), both), EINVAL, "output-row field"),
             ((a, a, big, 0, 1, 10, _params(9, 0.0, 0.0, keep), only_y), EINVAL, "output-row field"),
             ((a, None, big, 2, 1, 10, _params(9, 0.0, 0.0, keep), both), EINVAL, "input-row field"),
             ((a, a, big, 2, 0, 10, _params(9, 0.0, 0.0, keep), only_u), EINVAL, "input-row field"),
             ((a, a, big, 2, 1, 10, _params(9, 0.0, 0.0, keep), both), ERANGE, "MPCT_INDEX_MAX_ROWS"),
             ((None, a, big, 1, 1, 10, _params(9, 0.0, 0.0, keep), only_u), ERANGE, "MPCT_INDEX_MAX_ROWS")]
    for args, code, msg in steps:
        y, u, S, my, nu, nit, p, out = args
        pp = C.byref(p) if p is not None else None
        oo = C.byref(out) if out is not None else None
        for rc in (lib.mpct_limit_indices_device(y, u, S, my, nu, nit, pp, oo, None),
                   lib.mpct_limit_indices(y, u, S, my, nu, nit, pp, -1, oo)):
            assert rc == code, (args[2:6], msg, rc, _lib.last_error())
            assert msg in _lib.last_error(), (args[2:6], _lib.last_error())
    # infinite bounds on the open side and lo == hi are fine; S = 0 needs neither trajectories nor a device
    p = _params(0, 0.25, 0.125, keep, y_lo=[-INF, 0.5], y_hi=[INF, 0.5], u_lo=[-INF], du_hi=[INF])
    assert lib.mpct_limit_indices_device(None, None, 0, 2, 1, 10, C.byref(p), C.byref(both), None) == 0
    assert lib.mpct_limit_indices(None, None, 0, 2, 1, 10, C.byref(p), -1, C.byref(both)) == 0
    assert (buf == 0).all() and (ibuf == 0).all()


@pytest.fixture(scope="module")
def small_scenario(built):
    from mpct.scenarios import shell3x3

    sc, r, _ = shell3x3(n2_max=10, nu_max=3, nit=40)
    yield sc, r
    sc.close()


def test_eval_entries_argument_errors_in_documented_order(small_scenario):
    from mpct import _lib

    sc, r = small_scenario
    lib = _lib.load()
    buf = np.zeros(4 * 3 * 40)
    ibuf = np.zeros(64, dtype=np.int32)
    d, ip = buf.ctypes.data_as(_lib.c_double_p), ibuf.ctypes.data_as(_lib.c_int32_p)
    N2, Nu = np.array([5, 6], dtype=np.int32), np.array([2, 2], dtype=np.int32)
    dl, lm = np.ones((2, 3)), np.ones((2, 3))
    refs = np.ascontiguousarray(r[None])
    O = _lib.MpctOpts
    none, some = _lib.MpctLimitResult(), _lib.MpctLimitResult(viol=d)
    traj = _lib.MpctResult(y=d)
    ol, cl = O(1, 0, 0, -1, 0.0), O(0, 0, 0, -1, 0.0)
    keep = []
    nan3 = [0.0, np.nan, 0.0]
    bad = lambda t0: _params(t0, -1.0, 0.0, keep, u_hi=nan3)          # noqa: E731
    ref = lambda x: C.byref(x) if x is not None else None               # noqa: E731

    def call(h, C_, nref, refs_p, opts, p, res, out):
        a = [h, C_, N2.ctypes.data, Nu.ctypes.data, dl.ctypes.data, lm.ctypes.data, nref, refs_p, None, ref(opts), ref(p),
             ref(res), ref(out)]
        return lib.mpct_eval_limit_indices(*a), lib.mpct_eval_limit_indices_device(*(a + [None]))

    rp = refs.ctypes.data
    steps = [((None, -1, 0, None, ol, None, traj, none), "null scenario"),
             ((sc.handle, -1, 0, None, ol, None, traj, none), "null params"),
             ((sc.handle, -1, 0, None, ol, bad(40), traj, none), "open_loop must be 0"),
             ((sc.handle, -1, 0, None, cl, bad(40), traj, none), "trajectory pointers of res"),
             ((sc.handle, -1, 0, None, cl, bad(40), None, none), "C < 0 or nref < 1"),
             ((sc.handle, 2, 0, None, cl, bad(40), None, none), "C < 0 or nref < 1"),
             ((sc.handle, 2, 1, None, cl, bad(40), None, none), "null input pointer"),
             ((sc.handle, 2, 1, rp, cl, bad(40), None, none), "t0 must be"),
             ((sc.handle, 2, 1, rp, cl, bad(39), None, none), "out_tol and sat_tol"),
             ((sc.handle, 2, 1, rp, None, _params(39, 0.0, 0.0, keep, u_hi=nan3), None, none), "bad bound"),
             # the caller's lower bound against the scenario's own upper bound (du_max = 0.05 / R)
             ((sc.handle, 2, 1, rp, None, _params(39, 0.0, 0.0, keep, du_lo=[1.0, 1.0, 1.0]), None, none), "bad bound"),
             ((sc.handle, 2, 1, rp, None, _params(39, 0.0, 0.0, keep), None, none), "no output pointer"),
             ((sc.handle, 2, 1, rp, None, _params(39, 0.0, 0.0, keep), None, None), "no output pointer")]
    for args, msg in steps:
        for rc in call(*args):
            assert rc == EINVAL, (msg, rc, _lib.last_error())
            assert msg in _lib.last_error(), (msg, _lib.last_error())
    # an empty batch is fine without a device
    p = _params(0, 0.0, 0.0, keep)
    assert call(sc.handle, 0, 1, rp, None, p, None, some) == (0, 0)

    # the robust entries: the list of mpct_eval_robust_indices, then t0, the tolerances and the bounds
    S = _lib.MpctDrawStats
    stats, lev_stats = S(hi=d), S(hi=d, quantile=d)
    base_j1 = _lib.MpctRobustResult(J1=d)
    ids = lambda *v: np.array(v, dtype=np.int32)                     # noqa: E731
    lv = np.array([0.5, 2.0])

    def rcall(h, C_, nref, refs_p, jb, opts, p, nsel, fields, nlev, levels, base, out):
        a = [h, C_, N2.ctypes.data, Nu.ctypes.data, dl.ctypes.data, lm.ctypes.data, nref, refs_p, None, jb, ref(opts), ref(p),
             nsel, fields.ctypes.data_as(_lib.c_int32_p) if fields is not None else None, nlev,
             levels.ctypes.data_as(_lib.c_double_p) if levels is not None else None, ref(base), ref(out)]
        return lib.mpct_eval_robust_limit_indices(*a), lib.mpct_eval_robust_limit_indices_device(*(a + [None]))

    h = sc.handle
    rsteps = [((None, 2, 0, None, -1.0, ol, None, 0, None, 9, None, base_j1, None), EINVAL, "null scenario"),
              ((h, 2, 0, None, -1.0, ol, None, 0, None, 9, None, base_j1, None), EINVAL, "null params"),
              ((h, 2, 0, None, -1.0, ol, bad(40), 0, None, 9, None, base_j1, None), EINVAL, "open_loop must be 0"),
              ((h, 2, 0, None, -1.0, cl, bad(40), 0, None, 9, None, base_j1, None), EINVAL, "nsel must be"),
              ((h, 2, 0, None, -1.0, cl, bad(40), 2, ids(0, 13), 9, None, base_j1, None), EINVAL, "field id out of range"),
              ((h, 2, 0, None, -1.0, cl, bad(40), 2, ids(4, 4), 9, None, base_j1, None), EINVAL, "field id repeated"),
              ((h, 2, 0, None, -1.0, cl, bad(40), 2, ids(4, 12), 9, None, base_j1, None), EINVAL, "nref < 1"),
              ((h, 2, 1, None, -1.0, cl, bad(40), 2, ids(4, 12), 9, None, base_j1, None), EINVAL, "j_bound must be"),
              ((h, 2, 1, None, 0.0, cl, bad(40), 2, ids(4, 12), 9, None, base_j1, None), EINVAL, "nlev must be"),
              ((h, 2, 1, None, 0.0, cl, bad(40), 2, ids(4, 12), 2, None, base_j1, None), EINVAL, "null levels"),
              ((h, 2, 1, None, 0.0, cl, bad(40), 2, ids(4, 12), 2, lv, base_j1, None), EINVAL, "every level"),
              ((h, 2, 1, None, 0.0, cl, bad(40), 2, ids(4, 12), 0, None, base_j1, None), EINVAL, "every output pointer"),
              ((h, 2, 1, None, 0.0, cl, bad(40), 2, ids(4, 12), 0, None, base_j1, lev_stats), EINVAL, "base->J1 must be NULL"),
              ((h, 2, 1, None, 0.0, cl, bad(40), 2, ids(4, 12), 0, None, None, lev_stats), EINVAL, "need nlev >= 1"),
              ((h, 2, 1, None, 0.0, cl, bad(40), 2, ids(4, 12), 0, None, None, stats), EINVAL, "null input pointer"),
              ((h, 2, 1, rp, 0.0, cl, bad(40), 2, ids(4, 12), 0, None, None, stats), EINVAL, "t0 must be"),
              ((h, 2, 1, rp, 0.0, cl, bad(39), 2, ids(4, 12), 0, None, None, stats), EINVAL, "out_tol and sat_tol"),
              ((h, 2, 1, rp, 0.0, cl, _params(39, 0.0, 0.0, keep, u_hi=nan3), 2, ids(4, 12), 0, None, None, stats), EINVAL, "bad bound"),
              ((h, 2, 4097, rp, 0.0, cl, _params(39, 0.0, 0.0, keep), 2, ids(4, 12), 0, None, None, stats), ERANGE,
               "MPCT_TAIL_MAX_DRAWS")]
    for args, code, msg in rsteps:
        for rc in rcall(*args):
            assert rc == code, (msg, rc, _lib.last_error())
            assert msg in _lib.last_error(), (msg, _lib.last_error())
    assert rcall(h, 0, 1, rp, 0.0, None, p, 2, ids(4, 12), 0, None, None, stats) == (0, 0)
    assert (buf == 0).all() and (ibuf == 0).all()
    _ = ip


def test_nmpc_scenario_default_bounds_are_the_descriptors(built):
    """A NULL u_lo / u_hi of the scoring entries is an NMPC descriptor's u_min / u_max (Van de Vusse: [0, 40] and
    [150, 150]), and it holds no rate bound: the caller's other bound is checked against exactly those values,
    before any device is touched."""
    from mpct import _lib
    from mpct.nmpc import VDV_UMAX, VDV_UMIN, vandevusse

    sc, r, _ = vandevusse(n_max=5, nu_max=2, nit=20)
    lib = _lib.load()
    assert VDV_UMIN.tolist() == [0.0, 40.0] and VDV_UMAX.tolist() == [150.0, 150.0]
    N2, Nu = np.array([3], dtype=np.int32), np.array([2], dtype=np.int32)
    dl, lm = np.ones((1, 2)), np.ones((1, 2))
    refs = np.ascontiguousarray(r[None])
    none = _lib.MpctLimitResult()
    keep = []

    def call(**bounds):
        p = _params(0, 0.0, 0.0, keep, **bounds)
        a = [sc.handle, 1, N2.ctypes.data, Nu.ctypes.data, dl.ctypes.data, lm.ctypes.data, 1, refs.ctypes.data, None, None,
             C.byref(p), None, C.byref(none)]
        rcs = lib.mpct_eval_limit_indices(*a), lib.mpct_eval_limit_indices_device(*(a + [None]))
        assert rcs == (EINVAL, EINVAL), rcs
        return _lib.last_error()

    # accepted bounds fall through to the next check of the list, refused ones stop at the bound check
    for ok in (dict(), dict(u_lo=[150.0, 150.0]), dict(u_hi=[0.0, 40.0]), dict(u_lo=[-INF, 149.0], u_hi=[1.0, INF]),
               dict(du_lo=[1e9, 1e9]), dict(du_hi=[-1e9, -1e9]), dict(y_lo=[1e9, 1e9]), dict(y_hi=[-1e9, -1e9])):
        assert "no output pointer" in call(**ok), ok
    for bad in (dict(u_lo=[151.0, 0.0]), dict(u_lo=[0.0, 151.0]), dict(u_hi=[-1.0, 150.0]), dict(u_hi=[150.0, 39.0]),
                dict(u_hi=[150.0, np.nextafter(40.0, 0.0)]), dict(u_lo=[np.nextafter(150.0, 200.0), 40.0])):
        assert "bad bound" in call(**bad), bad
    sc.close()


def test_no_device_is_reported_and_empty_calls_need_none(small_scenario, has_gpu):
    from mpct.engine import MpctError, eval_limit_indices, eval_robust_limit_indices, limit_indices

    sc, r = small_scenario
    z = np.zeros(0, dtype=np.int32)
    res = eval_limit_indices(sc, z, z, np.zeros((0, 3)), np.zeros((0, 3)), r[None])
    assert res.viol.shape == (0, 1, 3) and res.sat_run.shape == (0, 1, 3) and res.sat_run.dtype == np.int32
    rob = eval_robust_limit_indices(sc, z, z, np.zeros((0, 3)), np.zeros((0, 3)), r[None], fields=("n_out", "sat_run"))
    assert rob.hi.shape == (0, 6) and rob.columns[3] == ("sat_run", 0)
    res = limit_indices(np.zeros((0, 2, 10)), np.zeros((0, 1, 10)), y_hi=1.0)
    assert res.viol.shape == (0, 1, 2) and res.n_lo.shape == (0, 1, 1)
    if has_gpu:
        return
    y, u, P = R.generated(2, 2, 1, 30, 0)
    with pytest.raises(MpctError, match=r"\(-3\).*HIP device"):
        limit_indices(y, u, y_lo=P["y_lo"], y_hi=P["y_hi"])
    with pytest.raises(MpctError, match=r"\(-3\).*(GPU|HIP device)"):
        eval_limit_indices(sc, [5, 6], [2, 2], np.ones((2, 3)), np.ones((2, 3)), r[None])


def test_limit_result_costs():
    from mpct.engine import LimitResult

    nit, t0 = 50, 5
    viol = np.arange(12.0).reshape(2, 2, 3)
    t_in = np.array([[[10, 20, 5], [7, 8, 9]], [[10, 50, 5], [7, -1, 9]]], dtype=np.int32)
    sat_run = np.array([[[3, 0], [1, 2]], [[0, 0], [7, 1]]], dtype=np.int32)
    y_margin = np.array([[[0.5, INF, -0.25], [1.0, INF, 0.0]], [[INF, INF, INF], [INF, INF, INF]]])
    u_margin = np.full((2, 2, 2), 0.5)
    u_margin[1, 0, 1] = np.nan
    res = LimitResult(viol=viol, t_in=t_in, sat_run=sat_run, y_margin=y_margin, u_margin=u_margin, nit=nit, t0=t0)
    got = res.costs(["viol", "t_in", "sat_run", "y_margin", "u_margin"], reduce="max")
    assert got.shape == (2, 5) and got.dtype == np.float64
    np.testing.assert_array_equal(got[0], [5.0, 15.0, 3.0, 0.25, -0.5])
    np.testing.assert_array_equal(got[1], [11.0, np.nan, 7.0, np.nan, np.nan])
    got = res.costs(["viol", "sat_run", "y_margin"], reduce="sum")
    np.testing.assert_array_equal(got[0], [15.0, 6.0, -1.25])
    assert np.isnan(got[1, 2]) and got[1, 1] == 8.0
    with pytest.raises(ValueError):
        res.costs(["viol"], reduce="mean")
    with pytest.raises(ValueError):
        res.costs(["iae"])
    with pytest.raises(ValueError):
        res.costs(["n_lo"])               # not in this result
