"""Plant-parameter draws in the NMPC kernel, without a GPU: the mpct_nmpc_scenario_create_var entry
(what it accepts, every MPCT_EINVAL case, nplant = 0 == mpct_nmpc_scenario_create), the instance names,
the numpy reference of the GPU tests (tests/nmpc_mismatch_ref.py), the vandevusse_mc draws and their
default half-widths, and the variant table under the sanitizers
(tests/host_tables/nmpc_variants_check.cpp)."""
import ctypes as C
import os

import numpy as np
import pytest

import host_program
import nmpc_mismatch_ref as mr

ROOT = host_program.ROOT
NOMINAL = "nmpc_closed_loop_kernel (QP-size x LDS-tier class launches)"
VARIANT = "nmpc_closed_loop_kernel<..., plant variants> (QP-size x LDS-tier class launches)"


def _scenario(**kw):
    from mpct import nmpc

    x0 = nmpc.steady_state()
    _, yref = nmpc.vandevusse_signals(x0)
    return nmpc.NmpcScenario(x0, nmpc.VDV_U0, nmpc.VDV_UMIN, nmpc.VDV_UMAX, nmpc.VDV_XMIN, nmpc.VDV_XMAX, yref, 31, 15,
                             **kw)


def _create_var(nplant, pp, px0):
    """mpct_nmpc_scenario_create_var on the Van de Vusse descriptor: (rc, message, handle, lib)."""
    from mpct import _lib, nmpc

    x0 = nmpc.steady_state()
    _, yref = nmpc.vandevusse_signals(x0)
    keep = dict(x0=x0, u0=nmpc.VDV_U0, u_min=nmpc.VDV_UMIN, u_max=nmpc.VDV_UMAX, x_min=nmpc.VDV_XMIN,
                x_max=nmpc.VDV_XMAX, y_scale=np.array([1.2, 110.0]), u_scale=np.array([150.0, 110.0]))
    keep = {k: np.ascontiguousarray(v, dtype=float) for k, v in keep.items()}
    xc = np.array(nmpc.VDV_XC, dtype=np.int32)
    yref = np.ascontiguousarray(yref)
    d = _lib.MpctNmpcDesc()
    d.abi_version, d.model, d.nx, d.ny, d.nu = _lib.ABI_VERSION, _lib.NMPC_VANDEVUSSE, 3, 2, 2
    d.xc, d.ts, d.nsub = xc.ctypes.data_as(_lib.c_int32_p), 0.05, 10
    for k, v in keep.items():
        setattr(d, k, v.ctypes.data_as(_lib.c_double_p))
    d.n_max, d.nu_max, d.nit, d.yref = 31, 15, yref.shape[1], yref.ctypes.data_as(_lib.c_double_p)
    lib = _lib.load()
    h = C.c_void_p()
    pp = None if pp is None else np.ascontiguousarray(pp, dtype=float)
    px0 = None if px0 is None else np.ascontiguousarray(px0, dtype=float)
    rc = lib.mpct_nmpc_scenario_create_var(C.byref(d), nplant, None if pp is None else pp.ctypes.data_as(_lib.c_double_p),
                                           None if px0 is None else px0.ctypes.data_as(_lib.c_double_p), C.byref(h))
    return rc, _lib.last_error(), h, lib


def _name(lib, h, robust=False):
    buf = C.create_string_buffer(192)
    (lib.mpct_robust_instance if robust else lib.mpct_kernel_instance)(h, None, buf, len(buf))
    return buf.value.decode()


def test_export(built):
    from mpct import _lib

    lib = _lib.load()
    so = C.CDLL(_lib.lib_path())
    assert "mpct_nmpc_scenario_create_var" in _lib.EXPORTS and hasattr(lib, "mpct_nmpc_scenario_create_var")
    assert C.cast(so.mpct_nmpc_scenario_create_var, C.c_void_p).value
    assert lib.mpct_abi_version() == 7   # an addition to ABI 7, no version change
    hdr = open(os.path.join(ROOT, "include", "mpct.h")).read()
    assert "int32_t mpct_nmpc_scenario_create_var(const mpct_nmpc_desc* desc, int32_t nplant" in hdr


def test_creation_and_names(built):
    from mpct.engine import kernel_instance, robust_instance

    P = np.array([mr.MODEL, mr.scaled(mr.MODEL, (1.05, 1.0, 0.95)), mr.scaled(mr.MODEL, h=(0.95, 1.05, 1.0))])
    X0 = np.array([[1.2, 0.9, 134.0], [1.25, 0.91, 135.0], [1.3, 0.92, 133.0]])
    nom = _scenario()
    assert nom.nplant == 0 and kernel_instance(nom) == NOMINAL
    assert robust_instance(nom) == NOMINAL + " + robust_reduce_kernel"
    for px in (X0, None):
        sc = _scenario(plant_params=P, plant_x0=px)
        assert sc.nplant == 3
        assert kernel_instance(sc) == VARIANT and kernel_instance(sc, open_loop=True, want_traj=True) == VARIANT
        assert robust_instance(sc) == VARIANT + " + robust_reduce_kernel"
        # staging, LDS layout and tiers do not depend on the variants
        for n, nu in ((31, 15), (3, 2), (12, 7), (20, 8)):
            assert sc.lds_bytes(n, nu) == nom.lds_bytes(n, nu)
    one = _scenario(plant_params=mr.MODEL)   # one variant equal to the model is still the variant instance
    assert one.nplant == 1 and kernel_instance(one) == VARIANT
    with pytest.raises(ValueError):
        _scenario(plant_params=P, plant_x0=X0[:2])


def test_nplant_zero_is_scenario_create(built):
    rc, msg, h, lib = _create_var(0, None, None)
    assert rc == 0, msg
    try:
        nom = _scenario()
        assert _name(lib, h) == NOMINAL and _name(lib, h, robust=True) == NOMINAL + " + robust_reduce_kernel"
        for n, nu in ((31, 15), (3, 2), (12, 7)):
            assert lib.mpct_lds_bytes(h, n, nu) == nom.lds_bytes(n, nu)
    finally:
        lib.mpct_scenario_destroy(h)


def test_einval_cases(built):
    P = np.array([mr.MODEL, mr.scaled(mr.MODEL, (1.05, 1.0, 0.95))])
    X0 = np.array([[1.2, 0.9, 134.0], [1.25, 0.91, 135.0]])

    def rejected(nplant, pp, px0, text):
        rc, msg, h, _ = _create_var(nplant, pp, px0)
        assert rc == -1 and text in msg and not h.value, (rc, msg)

    rejected(0, P, None, "nplant = 0 takes no plant_params and no plant_x0")
    rejected(0, None, X0, "nplant = 0 takes no plant_params and no plant_x0")
    rejected(2, None, None, "nplant >= 1 needs plant_params")
    rejected(2, None, X0, "nplant >= 1 needs plant_params")
    rejected(-1, None, None, "nplant must be >= 0")
    for bad in (np.nan, np.inf, -np.inf):
        Q = P.copy()
        Q[1, 4] = bad
        rejected(2, Q, X0, "non-finite plant parameter")
    for i in (9, 10, 13):   # rho, cp, V
        Q = P.copy()
        Q[1, i] = 0.0
        rejected(2, Q, None, "rho*cp*V = 0")
    Y = X0.copy()
    Y[1, 2] = np.nan
    rejected(2, P, Y, "non-finite plant_x0")
    rc, msg, h, lib = _create_var(2, P, X0)
    assert rc == 0 and h.value, msg
    assert _name(lib, h) == VARIANT
    lib.mpct_scenario_destroy(h)
    # the Python mirror reports the entry's message
    from mpct.engine import MpctError

    with pytest.raises(MpctError, match=r"create_var failed \(-1\).*rho\*cp\*V = 0"):
        Q = P.copy()
        Q[0, 13] = 0.0
        _scenario(plant_params=Q)


def test_reference_reduces_to_nominal_oracle():
    """A variant equal to the model: the mismatch reference is oracle.nmpc_vdv.closedloop_nmpc, bit for bit
    (the tuned point, and a longer horizon with the open-loop leg)."""
    import oracle.nmpc_vdv as nv
    from mpct.nmpc import VDV_TUNED as T

    np.testing.assert_array_equal(mr.MODEL[:3], [nv.K10, nv.K20, nv.K30])
    x0 = nv.steady_state()
    r, _ = nv.references(x0)
    for N, Nu, d, lam in ((T["N"], 2, np.array(T["delta"]), np.array(T["lam"])),
                          (6, 4, np.array([0.7, 1.0]), np.array([0.05, 0.2]))):
        a = nv.closedloop_nmpc(r, N, Nu, d, lam, x0=x0)
        b = mr.closedloop_mismatch(r, N, Nu, d, lam, mr.MODEL, x0)
        for f in ("y", "u", "yopt", "uopt"):
            np.testing.assert_array_equal(getattr(a, f), getattr(b, f), err_msg=f)
        assert a.sqp_iters == b.sqp_iters and a.bounds_ok == b.bounds_ok


def test_reference_sees_the_mismatch():
    """+5 % on the rate constants: the plant rests elsewhere, the loop differs, and full state feedback
    without an estimator leaves a steady-state offset."""
    import oracle.nmpc_vdv as nv
    from mpct import nmpc
    from mpct.nmpc import VDV_TUNED as T

    x0 = nv.steady_state()
    r, yref = nv.references(x0)
    p = mr.scaled(mr.MODEL, (1.05, 1.05, 1.05))
    d, lam = np.array(T["delta"]), np.array(T["lam"])
    a = mr.closedloop_mismatch(r, 3, 2, d, lam, mr.MODEL, x0, open_loop=False)
    b = mr.closedloop_mismatch(r, 3, 2, d, lam, p, x0, open_loop=False)
    assert np.max(np.abs(a.y - b.y)) > 1e-2
    assert abs(b.y[0, -1] - r[0, -1]) > 10 * abs(a.y[0, -1] - r[0, -1])
    xs = nmpc.steady_state(params=p)
    assert np.max(np.abs(mr.plant_rhs(xs, nv.U0, p))) < 1e-9 and np.max(np.abs(xs - x0)) > 1e-2


def test_vandevusse_mc_draws(built):
    from mpct import nmpc

    P = nmpc.vandevusse_mc_params(8)
    assert P.shape == (8, 16) and np.array_equal(P[0], nmpc.VDV_PARAMS)
    f = P / nmpc.VDV_PARAMS
    untouched = [3, 4, 5, 9, 10, 11, 12, 13, 14, 15]
    assert np.all(f[:, untouched] == 1.0)
    assert np.all(np.abs(f[1:, :3] - 1.0) <= nmpc.VDV_MC_EK) and np.all(np.abs(f[1:, 6:9] - 1.0) <= nmpc.VDV_MC_EH)
    assert np.all(f[1:, [0, 1, 2, 6, 7, 8]] != 1.0)
    assert np.array_equal(nmpc.vandevusse_mc_params(3), P[:3])           # the draws do not depend on D
    assert not np.array_equal(nmpc.vandevusse_mc_params(3, seed=1)[1], P[1])
    assert np.array_equal(nmpc.vandevusse_mc_params(3, e_k=0.0, e_h=0.0), np.tile(nmpc.VDV_PARAMS, (3, 1)))
    sc, r, yref = nmpc.vandevusse_mc(3)
    nom, r1, yref1 = nmpc.vandevusse()
    assert sc.nplant == 3 and r.shape == (3, 2, 60) and np.array_equal(yref, yref1) and np.array_equal(r[0], r1)
    X0 = sc._keep["plant_x0"]
    assert np.array_equal(X0[0], nom.x0) and np.array_equal(sc.x0, nom.x0)
    for k in range(3):
        assert np.max(np.abs(nmpc._vdv_rhs_jac(X0[k], nmpc.VDV_U0, P[k])[0])) < 1e-9   # rests at u0
        assert np.array_equal(r[k], nmpc.vandevusse_signals(X0[k])[0])


def test_vandevusse_mc_defaults_keep_the_tuned_loop_inside_the_bounds():
    """The default half-widths (0.05, 0.05): on the CPU reference the committed tuning keeps every state
    inside x_min / x_max on all of 8 draws, each from its own steady state on its own reference."""
    import oracle.nmpc_vdv as nv
    from mpct import nmpc
    from mpct.nmpc import VDV_TUNED as T

    assert (nmpc.VDV_MC_EK, nmpc.VDV_MC_EH) == (0.05, 0.05)
    P = nmpc.vandevusse_mc_params(8)
    for k in range(8):
        xk = nmpc.steady_state(params=P[k])
        rk, _ = nmpc.vandevusse_signals(xk)
        res = mr.closedloop_mismatch(rk, T["N"], max(T["Nu"]), np.array(T["delta"]), np.array(T["lam"]), P[k], xk,
                                     open_loop=False)
        assert res.bounds_ok and res.max_iters < nv.SQP_MAX, k


def test_mex_plant_fields(built):
    """matlab/mpct_mex.c: the optional NMPC descriptor fields plant_params (16 x nplant) and plant_x0
    (3 x nplant) select mpct_nmpc_scenario_create_var; absent is today's call."""
    from mpct import nmpc
    from test_mex import mex

    x0 = nmpc.steady_state()
    _, yref = nmpc.vandevusse_signals(x0)
    d = {"nx": 3.0, "ny": 2.0, "nu": 2.0, "xc": np.array([2.0, 3.0]), "ts": 0.05, "x0": x0, "u0": nmpc.VDV_U0,
         "u_min": nmpc.VDV_UMIN, "u_max": nmpc.VDV_UMAX, "x_min": nmpc.VDV_XMIN, "x_max": nmpc.VDV_XMAX,
         "y_scale": np.array([1.2, 110.0]), "u_scale": np.array([150.0, 110.0]), "n_max": 31.0, "nu_max": 15.0,
         "nit": 60.0, "yref": yref}
    P = np.array([mr.MODEL, mr.scaled(mr.MODEL, (1.05, 1.0, 0.95))])
    X0 = np.array([[1.2, 0.9, 134.0], [1.25, 0.91, 135.0]])
    bad = P.copy()
    bad[1, 13] = 0.0
    res = mex([(1, ["create_nmpc", d]),
               (1, ["instance", ("P", 0, 0)]),
               (1, ["create_nmpc", dict(d, plant_params=P.T.copy())]),
               (1, ["instance", ("P", 2, 0)]),
               (1, ["create_nmpc", dict(d, plant_params=P.T.copy(), plant_x0=X0.T.copy())]),
               (1, ["instance", ("P", 4, 0)]),
               (1, ["create_nmpc", dict(d, plant_params=bad.T.copy())]),
               (1, ["create_nmpc", dict(d, plant_x0=X0.T.copy())])])
    assert res[0][0] and res[1][1][0] == NOMINAL
    assert res[2][0] and res[3][1][0] == VARIANT
    assert res[4][0] and res[5][1][0] == VARIANT
    assert not res[6][0] and "rho*cp*V = 0" in res[6][1][1]
    assert not res[7][0] and "plant_x0 needs plant_params" in res[7][1][1]


def test_nmpc_variant_table_under_sanitizers(tmp_path):
    """tests/host_tables/nmpc_variants_check.cpp, host-only, with ASan, LSan and UBSan."""
    stdout = host_program.run(host_program.build("nmpc_variants_check", tmp_path))
    assert "nmpc 3 variants: table [3][19], 456 bytes in the blob" in stdout
