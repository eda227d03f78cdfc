"""CPU: the robust-scoring entry points of the C ABI (include/mpct.h: mpct_eval_robust,
mpct_eval_robust_device, mpct_robust_instance) exist, name what they launch without a device,
validate their arguments before touching one, fail loudly without a GPU, and RobustResult.scores
masks and selects as documented.  No kernel runs here."""
import ctypes as C

import numpy as np
import pytest


def test_exports_exist(built):
    from mpct import _lib

    lib = _lib.load()
    so = C.CDLL(_lib.lib_path())
    for f in ("mpct_eval_robust", "mpct_eval_robust_device", "mpct_robust_instance"):
        assert f in _lib.EXPORTS
        assert hasattr(lib, f)
        assert C.cast(getattr(so, f), C.c_void_p).value
    assert lib.mpct_abi_version() == 7   # additions to ABI 7, no version change


def _bounded_dtc():
    """The bounded DTC scenario of tests/test_abi.py: a finite move bound takes it off dtc_small_kernel."""
    from mpct.dtc import woodberry_dtc
    from mpct.engine import Scenario

    scd, r, q = woodberry_dtc(n2_max=10, nu_max=5)
    b = np.array([0.5, 0.5])
    scb = Scenario(scd.plant, scd.model, nu=2, du_min=-b, du_max=b, u_min=-np.full(2, np.inf),
                   u_max=np.full(2, np.inf), yref=np.zeros((2, 200)), n2_max=10, nu_max=5, Ts=1.0, window="gpc",
                   weights_squared=False, exact_carima=False, dtc=True, dist=[[t] for t in (scd.plant[0][0],
                                                                                           scd.plant[1][0])])
    return scb, r, q


def test_robust_instance_names(built):
    from mpct import _lib
    from mpct.dtc import woodberry_dtc, woodberry_mc
    from mpct.engine import kernel_instance, robust_instance
    from mpct.scenarios import shell3x3

    scm, _, _, _ = woodberry_mc(draws=4)
    assert robust_instance(scm) == "dtc_robust_kernel<16> + dtc_robust_kernel<32>"
    scd, _, _ = woodberry_dtc(n2_max=10, nu_max=5)
    assert robust_instance(scd) == "dtc_robust_kernel<16>"
    sc3, _, _ = shell3x3(n2_max=30, nu_max=5)
    assert robust_instance(sc3) == "gpc_small_kernel + robust_reduce_kernel"
    scb, _, _ = _bounded_dtc()
    assert kernel_instance(scb) == "gpc_closed_loop_kernel<16,true,false>"
    assert robust_instance(scb) == "gpc_closed_loop_kernel<16,true,false> + robust_reduce_kernel"
    lib = _lib.load()
    assert lib.mpct_robust_instance(None, None, None, 0) < 0
    o = _lib.MpctOpts(0, 1, 0, -1, 0.0)
    assert lib.mpct_robust_instance(scm.handle, C.byref(o), None, 0) == -1   # cost-only


def _call(sc, refs, v, j_bound=0.0, nref=None, open_loop=0, want_traj=0, outputs=True):
    from mpct import _lib

    lib = _lib.load()
    N2 = np.array([10, 8], np.int32)
    Nu = np.array([3, 2], np.int32)
    d = np.ones((2, sc.my))
    lam = np.ones((2, sc.nu))
    refs = np.ascontiguousarray(refs, dtype=float)
    v = np.ascontiguousarray(v, dtype=float)
    mean = np.zeros((2, sc.my))
    nf = np.zeros(2, np.int32)
    r = _lib.MpctRobustResult()
    if outputs:
        r.mean = mean.ctypes.data_as(_lib.c_double_p)
        r.n_failed = nf.ctypes.data_as(_lib.c_int32_p)
    o = _lib.MpctOpts(open_loop, want_traj, 0, -1, 0.0)
    rc = lib.mpct_eval_robust(sc.handle, 2, N2.ctypes.data, Nu.ctypes.data, d.ctypes.data, lam.ctypes.data,
                              refs.shape[0] if nref is None else nref, refs.ctypes.data, v.ctypes.data,
                              float(j_bound), C.byref(o), C.byref(r))
    return rc, _lib.last_error()


def test_einval_cases(built):
    """Every argument error is MPCT_EINVAL (-1) with a message, decided before any device is touched
    (so it is the same with and without a GPU)."""
    from mpct.dtc import woodberry_mc

    sc, refs, v, _ = woodberry_mc(draws=3, n2_max=10, nu_max=5)
    for kw, word in ((dict(open_loop=1), "cost-only"), (dict(want_traj=1), "cost-only"), (dict(nref=0), "nref"),
                     (dict(j_bound=-1.0), "j_bound"), (dict(j_bound=float("nan")), "j_bound"),
                     (dict(outputs=False), "NULL")):
        rc, msg = _call(sc, refs, v, **kw)
        assert rc == -1 and word in msg, (kw, rc, msg)


def test_robust_without_gpu_fails_loudly(built, has_gpu):
    """No CPU fallback: without a device a valid call returns MPCT_EDEVICE (-3) with a message, and
    the Python wrapper raises MpctError.  +inf is a valid j_bound."""
    if has_gpu:
        pytest.skip("GPU present: covered by tests/test_robust_gpu.py")
    from mpct.dtc import woodberry_mc
    from mpct.engine import MpctError, eval_robust

    sc, refs, v, _ = woodberry_mc(draws=3, n2_max=10, nu_max=5)
    rc, msg = _call(sc, refs, v, j_bound=float("inf"))
    assert rc == -3 and msg
    with pytest.raises(MpctError, match=r"-3"):
        eval_robust(sc, [10, 8], [3, 2], np.ones((2, 2)), np.ones((2, 2)), refs, v=v)


def test_scores_masking_and_stat():
    from mpct.engine import RobustResult

    mean = np.array([[1.0, 2.0], [3.0, 4.0], [5.0, 6.0], [np.nan, np.nan]])
    worst = 10.0 * mean
    res = RobustResult(mean=mean, worst=worst, n_failed=np.array([0, 1, 2, 4], np.int32),
                       worst_draw=np.array([0, 1, 2, -1], np.int32), status=np.array([0, 4, 4, 4], np.int32), draws=4)
    s = res.scores()                                   # worst, no failed draw tolerated
    np.testing.assert_array_equal(s[0], worst[0])
    assert np.all(np.isnan(s[1:]))
    s = res.scores(max_failed=1, stat="mean")
    np.testing.assert_array_equal(s[:2], mean[:2])
    assert np.all(np.isnan(s[2:]))
    s = res.scores(max_failed=4)
    np.testing.assert_array_equal(s[:3], worst[:3])
    assert np.all(np.isnan(s[3]))                       # no survivor: the statistic itself is NaN
    assert s is not res.worst and np.array_equal(res.worst[:3], worst[:3])   # a copy: the record is untouched
    with pytest.raises(ValueError):
        res.scores(stat="median")
