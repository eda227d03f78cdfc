"""Plant mismatch on the band kernel, without a GPU: the mpct_scenario_create_est entry (what it
accepts, what stays rejected, estimator 0 == mpct_scenario_create), the instance names and LDS figure
of estimator scenarios, the Shell 7x5 / WoodBerry model-error draws (mpct.scenarios), the numpy
reference of the GPU tests (tests/band_mismatch_ref.py), the MEX descriptor's `estimator` field, and
the host tables over plant variants under the sanitizers (tests/host_tables/band_variants_check.cpp)."""
import ctypes as C
import os

import numpy as np
import pytest

import band_mismatch_ref as bm
import host_program

ROOT = host_program.ROOT
MARK = " + output-bias estimator"
BAND = "mdband_closed_loop_kernel (QP-size x LDS-tier class launches)"


def _create_est(sc, est, **change):
    """mpct_scenario_create_est on a copy of sc's descriptor with fields changed: (rc, message, handle)."""
    from mpct import _lib

    d = _lib.MpctScenarioDesc()
    C.pointer(d)[0] = sc._desc
    for k, val in change.items():
        setattr(d, k, val)
    h = C.c_void_p()
    rc = sc.lib.mpct_scenario_create_est(C.byref(d), est, C.byref(h))
    return rc, _lib.last_error(), h


def test_export_and_constant(built):
    from mpct import _lib

    lib = _lib.load()
    so = C.CDLL(_lib.lib_path())
    assert "mpct_scenario_create_est" in _lib.EXPORTS and hasattr(lib, "mpct_scenario_create_est")
    assert C.cast(so.mpct_scenario_create_est, C.c_void_p).value
    assert lib.mpct_abi_version() == 7   # an addition to ABI 7, no version change
    hdr = open(os.path.join(ROOT, "include", "mpct.h")).read()
    assert "#define MPCT_EST_OUTPUT_BIAS 1" in hdr and _lib.EST_OUTPUT_BIAS == 1


def test_accepts_mismatch_and_variants(built):
    from mpct.engine import MpctError, Scenario

    M, V = bm.synthetic_plants()
    sc = bm.synthetic_scenario(V)
    assert sc.nplant == 3 and sc.estimator == "output_bias" and sc.dims()["nd"] == 1
    one = bm.synthetic_scenario([V[1]])
    assert one.nplant == 1
    # the same descriptors through mpct_scenario_create: today's messages, unchanged
    with pytest.raises(MpctError, match="mdband excludes dtc, plant-only disturbances and plant variants"):
        bm.synthetic_scenario(V, estimator=None)
    with pytest.raises(MpctError, match=r"mdband: plant must equal the model \(the toolbox estimator is not restated\)"):
        bm.synthetic_scenario([V[1]], estimator=None)
    with pytest.raises(ValueError):
        bm.synthetic_scenario(V, estimator="kalman")
    assert isinstance(sc, Scenario)


def test_rejections(built):
    from mpct.engine import MpctError
    from mpct.scenarios import shell3x3_mc_plants, shell3x3_plant, shell3x3_xsp, shell3x3_yref, SHELL3_L as L, SHELL3_R as R
    from mpct.engine import Scenario

    _, V = bm.synthetic_plants()
    sc = bm.synthetic_scenario(V)
    for bad in (2, -1, 7):
        rc, msg, h = _create_est(sc, bad)
        assert rc == -1 and msg == "unknown estimator id" and not h.value
    rc, msg, h = _create_est(sc, 1, dtc=1)
    assert rc == -1 and msg == "mdband excludes dtc, plant-only disturbances and plant variants" and not h.value
    rc, msg, h = _create_est(sc, 1, nq=1)
    assert rc == -1 and msg == "mdband excludes dtc, plant-only disturbances and plant variants"
    # a GPC-mode (non-mdband) descriptor with a non-zero estimator
    P = shell3x3_plant()
    yref = L[:, None] * shell3x3_yref(shell3x3_xsp(50))
    kw = dict(nu=3, du_min=-0.05 / R, du_max=0.05 / R, u_min=-1.0 / R, u_max=0.5 / R, yref=yref, n2_max=10, nu_max=2)
    with pytest.raises(MpctError, match=r"\(-1\).*belongs to the band kernel"):
        Scenario(shell3x3_mc_plants(1)[0], P, estimator="output_bias", **kw)
    gpc = Scenario(P, P, **kw)
    rc, msg, h = _create_est(gpc, 0)   # estimator 0 on it is mpct_scenario_create
    assert rc == 0 and h.value
    gpc.lib.mpct_scenario_destroy(h)


def test_estimator_zero_is_scenario_create(built):
    """estimator = 0 builds what mpct_scenario_create builds: tables, dims, LDS figures, instance."""
    from mpct import _lib

    nom = bm.synthetic_scenario(None, estimator=None)
    rc, msg, h = _create_est(nom, 0)
    assert rc == 0, msg
    lib = nom.lib
    try:
        for which in (0, 2):
            n = lib.mpct_scenario_table(h, which, None, 0)
            buf = np.zeros(n)
            lib.mpct_scenario_table(h, which, buf.ctypes.data_as(_lib.c_double_p), n)
            np.testing.assert_array_equal(buf, nom.table(which))
        for n2, nu in ((12, 3), (5, 1)):
            assert lib.mpct_lds_bytes(h, n2, nu) == nom.lds_bytes(n2, nu)
            assert lib.mpct_lds_bytes_opts(h, None, n2, nu) == nom.lds_bytes(n2, nu, costs_only=True)
        buf = C.create_string_buffer(192)
        lib.mpct_kernel_instance(h, None, buf, len(buf))
        assert buf.value.decode() == BAND
        # and with variants it rejects what mpct_scenario_create rejects
        _, V = bm.synthetic_plants()
        rc, msg, h2 = _create_est(bm.synthetic_scenario(V), 0)
        assert rc == -1 and msg == "mdband excludes dtc, plant-only disturbances and plant variants"
    finally:
        lib.mpct_scenario_destroy(h)


def test_instance_names_and_lds(built):
    from mpct.engine import kernel_instance, robust_instance
    from mpct.scenarios import shell7x5, shell7x5_mc

    M, V = bm.synthetic_plants()
    nom = bm.synthetic_scenario(None, estimator=None)
    est = bm.synthetic_scenario([M, M, M])
    assert kernel_instance(nom) == BAND and robust_instance(nom) == BAND + " + robust_reduce_kernel"
    assert kernel_instance(est) == BAND + MARK
    assert kernel_instance(est, want_traj=True) == BAND + MARK
    assert robust_instance(est) == BAND + MARK + " + robust_reduce_kernel"
    # the two-copy layout: with every variant equal to the model, the nominal scenario's own figure
    # with the open-loop leg's second copy, for cost-only calls too
    for n2, nu in ((12, 3), (7, 2), (3, 1)):
        two = nom.lds_bytes(n2, nu)
        assert est.lds_bytes(n2, nu, costs_only=True) == two and est.lds_bytes(n2, nu) == two
        assert nom.lds_bytes(n2, nu, costs_only=True) < two
    # longer variants lengthen the rings
    assert bm.synthetic_scenario(V).lds_bytes(12, 3, costs_only=True) > est.lds_bytes(12, 3, costs_only=True)
    s7, s7e = shell7x5(n2_max=40, nu_max=8)[0], shell7x5_mc(draws=3, n2_max=40, nu_max=8)[0]
    assert kernel_instance(s7e) == BAND + MARK and s7e.nplant == 3
    assert s7e.lds_bytes(40, 8, costs_only=True) == s7.lds_bytes(40, 8)
    assert s7.lds_bytes(40, 8, costs_only=True) < s7.lds_bytes(40, 8)


def test_shell7x5_mc_plants():
    from mpct.scenarios import (SHELL7_DK, SHELL7_EMAX, SHELL7_K, SHELL7_L as L, SHELL7_R as R, shell7x5_mc_plants,
                                shell7x5_plant)

    assert SHELL7_EMAX == (0.2, 0.2, 0.3, 0.5, 0.5)
    A = shell7x5_mc_plants(5)
    # draw 0: the gains of Shell7x5.m:46-62 at e = (0.2, 0.2, 0.3, 0.5, 0.5), literally
    e1, e2, e3, e4, e5 = SHELL7_EMAX
    lit = np.array([[4.05 + 2.11 * e1, 1.77 + 0.39 * e2, 5.88 + 0.59 * e3, 1.20 + 0.12 * e4, 1.44 + 0.16 * e5],
                    [5.39 + 3.29 * e1, 5.72 + 0.57 * e2, 6.9 + 0.89 * e3, 1.52 + 0.13 * e4, 1.83 + 0.13 * e5],
                    [3.66 + 2.29 * e1, 1.65 + 0.35 * e2, 5.53 + 0.67 * e3, 1.16 + 0.08 * e4, 1.27 + 0.08 * e5],
                    [5.92 + 2.34 * e1, 2.54 + 0.24 * e2, 8.10 + 0.32 * e3, 1.73 + 0.02 * e4, 1.79 + 0.04 * e5],
                    [4.13 + 1.71 * e1, 2.38 + 0.93 * e2, 6.23 + 0.30 * e3, 1.31 + 0.03 * e4, 1.26 + 0.02 * e5],
                    [4.06 + 2.39 * e1, 4.18 + 0.35 * e2, 6.53 + 0.72 * e3, 1.19 + 0.08 * e4, 1.17 + 0.01 * e5],
                    [4.38 + 3.11 * e1, 4.42 + 0.73 * e2, 7.2 + 1.33 * e3, 1.14 + 0.18 * e4, 1.26 + 0.10 * e5]])
    assert np.array_equal(SHELL7_K + SHELL7_DK * np.array(SHELL7_EMAX)[None, :], lit)
    got = np.array([[A[0][i][j].dcgain for j in range(5)] for i in range(7)])
    want = L[:, None] * R[None, :] * lit
    assert np.max(np.abs(got - want) / np.abs(want)) <= 1e-13
    # e = 0 is the nominal plant, exactly
    assert shell7x5_mc_plants(3, e_max=0.0) == [shell7x5_plant()] * 3
    assert shell7x5_mc_plants(5) == A
    B = shell7x5_mc_plants(5, seed=1)
    assert B[0] == A[0] and B[1] != A[1]
    nominal = L[:, None] * R[None, :] * SHELL7_K
    for P in A[1:]:
        g = np.array([[P[i][j].dcgain for j in range(5)] for i in range(7)])
        e = (g - nominal) / (L[:, None] * R[None, :] * SHELL7_DK)
        assert np.all(np.abs(e) <= np.array(SHELL7_EMAX)[None, :] + 1e-10)
        assert np.max(np.abs(e - e[0][None, :])) < 1e-10   # whole columns move together
        assert all(P[i][j].delay == A[0][i][j].delay for i in range(7) for j in range(5))
    # the gains are independent of max_dshift; the delays alone change, and not on draw 0
    D = shell7x5_mc_plants(5, max_dshift=2)
    shift = np.zeros((5, 7, 5), dtype=int)
    for k in range(5):
        for i in range(7):
            for j in range(5):
                assert D[k][i][j].num == A[k][i][j].num and D[k][i][j].den == A[k][i][j].den
                shift[k, i, j] = D[k][i][j].delay - A[k][i][j].delay
    assert np.all(shift[0] == 0) and shift.min() == 0 and shift.max() == 2


def test_mc_scenarios(built):
    from mpct.scenarios import (shell7x5, shell7x5_mc, shell7x5_plant, woodberry_mc_plants, woodberry_toolbox,
                                woodberry_toolbox_mc)

    sc, r, v, yref, plants = shell7x5_mc(draws=3, n2_max=40, nu_max=8)
    one, r1, v1, yref1 = shell7x5(n2_max=40, nu_max=8)
    assert r.shape == (3, 7, 200) and v.shape == (3, 2, 200) and len(plants) == 3
    assert all(np.array_equal(r[k], r1) and np.array_equal(v[k], v1) for k in range(3))
    assert np.array_equal(yref, yref1) and sc.model == shell7x5_plant() and sc.dims() == one.dims()
    assert all(np.array_equal(a, b) for a, b in zip(sc.bounds, one.bounds))
    assert all(np.array_equal(sc.bands[k], one.bands[k]) for k in one.bands)
    # WoodBerry.m:40-46: draw 0 is MV gains x 1.2, MV delays + 1, the disturbance column unchanged
    wb, wr, wv, wy = woodberry_toolbox()
    W = woodberry_mc_plants(4)
    for i in range(2):
        for j in range(3):
            a, b = W[0][i][j], wb.model[i][j]
            if j < 2:
                assert a.delay == b.delay + 1 and a.den == b.den
                assert abs(a.dcgain / b.dcgain - 1.2) < 1e-13
            else:
                assert a == b
    assert woodberry_mc_plants(3, dk_max=0.0, max_dshift=0) == [wb.model] * 3
    ws, r, v, yref, plants = woodberry_toolbox_mc(draws=4)
    assert ws.nplant == 4 and r.shape == (4, 2, 400) and v.shape == (4, 1, 400) and ws.model == wb.model


def test_reference_reduces_to_nominal_oracle():
    """With plant == model the mismatch reference is closedloop_band: zero bias, the same trajectories
    bit for bit (band mode and tracking weights)."""
    from oracle.scenarios import shell7x5
    from oracle.toolbox_band import closedloop_band

    sc, r, v, yref, fx = shell7x5(nit=40)
    lam = np.array(fx["lambda"])
    for N2, Nu, delta in ((9, 2, np.zeros(7)), (6, 3, np.r_[np.zeros(2), np.full(5, 0.3)])):
        a = closedloop_band(sc, r, v, N2, Nu, delta, lam, 40, open_loop=False)
        b = bm.closedloop_band_bias(sc, sc.plant, r, v, N2, Nu, delta, lam, 40)
        assert np.all(b.bias == 0.0)
        np.testing.assert_array_equal(a.y, b.y)
        np.testing.assert_array_equal(a.u, b.u)
        du_o, du_a = bm.replay_moves_bias(sc, sc.plant, r, v, N2, Nu, delta, lam, a.u)
        np.testing.assert_array_equal(du_o, a.du_hist)


def test_reference_sees_the_mismatch():
    """On the synthetic plants the bias is what the definition says and the loop stays inside reach."""
    from oracle.toolbox_band import BandScenario, simulate

    M, V = bm.synthetic_plants()
    osc = BandScenario(plant=bm.to_dtf(M), nu=1, du_min=np.array([-0.2]), du_max=np.array([0.2]), u_min=np.array([-1.0]),
                       u_max=np.array([1.0]), y_min=np.full(2, -0.3), y_max=np.full(2, 0.3), ecr_min=np.ones(2),
                       ecr_max=np.ones(2), sy=np.ones(2), su=np.ones(1))
    r, v, _ = bm.synthetic_signals()
    N2, Nu, delta, lam = bm.SYN_CANDS[0]
    res = bm.closedloop_band_bias(osc, V[0], r, v, N2, Nu, delta, lam, bm.SYN_NIT)
    U = np.vstack([res.u, v])
    ym = simulate(osc.ba(), U, bm.SYN_NIT)
    np.testing.assert_allclose(res.bias, res.y - ym, rtol=0, atol=1e-15)
    assert np.max(np.abs(res.bias)) > 1e-2 and np.max(np.abs(res.y)) < 1.0


def test_mex_estimator_field(built):
    """matlab/mpct_mex.c: the optional scalar descriptor field `estimator` selects
    mpct_scenario_create_est; absent or 0 is today's call."""
    from test_mex import mex, shell7x5_desc, tf_struct
    from mpct.scenarios import shell7x5_mc_plants

    sc, r, v, d = shell7x5_desc()
    plants = shell7x5_mc_plants(3)
    var = dict(d, model=tf_struct(sc.model), plant=tf_struct(plants[0]), nplant=3.0,
               plant_var=np.vstack([tf_struct(P) for P in plants]))
    res = mex([(1, ["create", dict(var, estimator=1.0)]),
               (1, ["instance", ("P", 0, 0)]),
               (1, ["create", var]),
               (1, ["create", dict(var, estimator=0.0)]),
               (1, ["create", dict(var, estimator=7.0)]),
               (1, ["create", dict(d, estimator=0.0)]),
               (1, ["instance", ("P", 5, 0)]),
               (1, ["create", dict(d, estimator=1.0)]),
               (1, ["instance", ("P", 7, 0)])])
    assert res[0][0], res[0]
    assert res[1][1][0] == BAND + MARK
    msg = "mdband excludes dtc, plant-only disturbances and plant variants"
    assert not res[2][0] and res[2][1][0] == "mpct:create" and msg in res[2][1][1]
    assert not res[3][0] and msg in res[3][1][1]
    assert not res[4][0] and "unknown estimator id" in res[4][1][1]
    assert res[5][0] and res[6][1][0] == BAND
    assert res[7][0] and res[8][1][0] == BAND + MARK


def test_band_variant_tables_under_sanitizers(tmp_path):
    """tests/host_tables/band_variants_check.cpp, host-only, with ASan, LSan and UBSan."""
    stdout = host_program.run(host_program.build("band_variants_check", tmp_path))
    assert "band 2x(1+1) x 3 variants: pl_maxb 7, pl_maxa 3, compact taps 3" in stdout
    assert 'variant past the rings: rejected -4 "plant entry too long for the device history rings"' in stdout
    assert 'model past the rings: rejected -4 "plant entry too long for the device history rings"' in stdout
    # the estimator argument's own checks, which build_scenario makes (mpct_scenario_create_est only passes it on)
    assert 'unknown estimator id: rejected -1 "unknown estimator id"' in stdout
    for what in ("estimator without mdband", "estimator on an ABI-2 descriptor"):
        assert what + ': rejected -1 "the output-bias estimator belongs to the band kernel (mdband = 1)"' in stdout
