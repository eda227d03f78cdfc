"""The band-scenario family of tests/band_family.py on the CPU: every case pinned to its branch of
mdband_kernel.hip's window update by the layout probe, every candidate held to its named properties
by the oracle alone, the numpy restatement of the update (tests/band_window_ref.py) against the
oracle's forward simulation, and the negative controls of the comparison the GPU tests use.

Tolerances.  WINDOW_RTOL: the oracle's window is a float64 lfilter over the whole input history; a
sample collects (taps + na) <= 12 roundings of 2^-53 per step, over nit = 70 steps, passed on through
the entry's impulse response (sum |h| <= 1 / (1 - |p|) = 7 for the underdamped poles here, <= nit for
the integrator): 70 * 12 * 2^-53 * 70 = 6.5e-12 of the window's peak bounds it; the longdouble
restatement adds nothing at that scale.  The constrained candidates' closed loops are held to the band
tests' TRAJ_RTOL; the gentle ones to band_family.gentle_bound, which the GPU test shares.
"""
import numpy as np
import pytest

import band_family as bf
import band_window_ref as bw
import host_program

TRAJ_RTOL = 1e-7      # tests/test_band.py
WINDOW_RTOL = 70 * 12 * 2.0 ** -53 * 70


# ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    exe = host_program.build("layout_probe", tmp_path_factory.mktemp("band_layout_probe"))

    def run(case):
        stdout = host_program.run(exe, stdin=bf.descriptor_text(case), ends_ok=False)
        got = {}
        for kv in stdout.split():
            k, v = kv.split("=", 1)
            got[k] = [int(x) for x in v.split(",")] if k in ("mz_na", "mz_nb", "mz_off") else int(v)
        return got

    return run


@pytest.mark.parametrize("name", bf.NAMES)
def test_layout_pins(probe, name):
    """Each case reaches the branch it is named for: the row lengths and per-entry lengths of the
    model's z^-1 tables, as scenario_tables.h builds them."""
    case = bf.CASES[name]
    got = probe(case)
    print(name, got)
    ne = case.my * case.nin
    assert got["ne"] == ne and len(got["mz_na"]) == len(got["mz_nb"]) == len(got["mz_off"]) == ne
    assert got["mz_maxa"] == max(got["mz_na"]) and got["mz_maxb"] == max(got["mz_nb"])
    assert got["mz_maxbc"] == max(b - o for b, o in zip(got["mz_nb"], got["mz_off"]))
    na = np.array(got["mz_na"]).reshape(case.my, case.nin)
    if name in ("so2", "est_so2", "wide"):
        assert got["mz_maxa"] == 3                                 # tail stride 2
        assert np.all(na[:, :case.nu] == 3) and np.all(na[:, case.nu:] == 2)
        assert sorted(np.array(got["mz_off"]).reshape(2, 3)[:, :2].ravel().tolist()) == [1, 2, 3, 4]   # delays 0..3
    if name == "to3_mixed":
        assert got["mz_maxa"] == 4                                 # tail stride 3, shifts of depth 2
        assert sorted(set(got["mz_na"])) == [2, 3, 4]              # own order below the stride
        assert np.all(na[2] == 2)                                  # an output of first-order entries only
    if name == "taps":
        assert got["mz_maxb"] == 8 and got["mz_maxbc"] == 4       # compact rows shorter than the full ones
        assert sorted(set(got["mz_off"])) == [0, 1, 2, 4]          # a delay of 4 beside delay 0, an MD with feedthrough
        assert sorted(b - o for b, o in zip(got["mz_nb"], got["mz_off"])) == [1, 1, 3, 3, 3, 4]
    if name == "integrator":
        assert got["mz_maxa"] == 3
        assert sum(case.model[0][0][1]) == pytest.approx(0.0, abs=1e-15)   # a pole at z = 1
    if name == "md_rich":
        assert case.nd == 2 and got["mz_maxa"] == 3 and np.all(na == 3)   # second-order MD entries
        v = np.array(case.v)
        assert v[0, 0] != 0.0                                      # dv != 0 at t = 0
        assert np.count_nonzero(np.diff(v[0])) >= 12 and np.count_nonzero(np.diff(v[1])) == 2


@pytest.mark.parametrize("name", bf.NAMES)
def test_candidate_properties(name):
    """By the oracle alone: every QP of every candidate solves and passes band_qp's KKT check (the
    device's status would be 0), the gentle candidate never has an active row, at least two
    candidates have a band row active on >= 10 steps and an MV bound on >= 3, one candidate tracks a
    moving setpoint, the horizons reach every length the update distinguishes, and the disturbance
    drives the outputs into their bands."""
    case = bf.CASES[name]
    assert case.my <= 3 and case.nu <= 2 and case.nd <= 2 and 60 <= case.nit <= 80 and case.n2_max <= 16
    assert len(case.cands) <= 8
    assert np.all(np.isfinite(case.y_band)) and np.all(np.isfinite(case.du_max)) and np.all(np.isfinite(case.u_max))
    order = max(len(den) for row in case.model for _, den, _ in row) - 1
    reach = max(len(num) + delay for row in case.model for num, _, delay in row)
    n2 = {c[0] for c in case.cands}
    assert {1, 2, order, reach - 1, case.n2_max} <= n2
    assert any(c[1] == 1 for c in case.cands) and any(c[0] == c[1] == 2 for c in case.cands)
    assert any(0 < np.count_nonzero(c[2]) < case.my for c in case.cands) and np.ptp(bf.setpoint(case)) > 0
    for var in range(case.nvar):
        loops = [bf.oracle_loop(name, k, var) for k in range(len(case.cands))]
        for k, o in enumerate(loops):
            print("%s cand %d variant %d: band rows active on %d steps, MV bounds on %d" % (name, k, var, o.band_steps, o.mv_steps))
        assert loops[0].band_steps == 0 and loops[0].mv_steps == 0
        assert np.abs(loops[0].res.u).max() > 0.3                      # and it does move
        assert sum(o.band_steps >= 10 and o.mv_steps >= 3 for o in loops) >= 2
        hi = np.array([b[1] for b in case.y_band])[:, None]
        assert any(np.any(o.res.y[:2] > hi[:2]) for o in loops)


@pytest.mark.parametrize("name", bf.NAMES)
def test_reference_is_well_conditioned(name):
    """The GPU test compares every candidate's free run, so every reference loop must be one that a
    free run can be compared with: it moves its MVs (a relative error needs a peak), and a 1e-13
    relative change of lambda moves the oracle's own y and u by <= 1e-9 of their peaks, 100 x below
    TRAJ_RTOL (the criterion of tests/test_band_mismatch_gpu.py)."""
    case = bf.CASES[name]
    worst = 0.0
    for k in range(len(case.cands)):
        for var in range(case.nvar):
            assert np.abs(bf.oracle_loop(name, k, var).res.u).max() > 1e-2, (k, var)
            s = bf.sensitivity(name, k, var)
            worst = max(worst, s)
            assert s <= 1e-9, (k, var, s)
    print("%s: the oracle's loops move by at most %.2e under a 1e-13 change of lambda" % (name, worst))


@pytest.mark.parametrize("name", bf.NAMES)
def test_window_against_forward_simulation(name):
    """The longdouble restatement of the carried window, run on the oracle's own inputs, against the
    window the oracle forward-simulates, at every step of every candidate."""
    case = bf.CASES[name]
    _, v, _ = bf.signals(case)
    worst = 0.0
    for k, c in enumerate(case.cands):
        for var in range(case.nvar):
            o = bf.oracle_loop(name, k, var)
            U = np.vstack([o.res.u, v])
            W = bw.windows_on(case.model, case.nu, c[0], U, o.res.du_hist)
            if case.est:
                W = W + np.asarray(o.res.bias, dtype=np.longdouble).T[:, :, None]
            err = float(np.max(np.abs(W.reshape(case.nit, -1) - o.f)) / np.max(np.abs(o.f)))
            worst = max(worst, err)
            assert err < WINDOW_RTOL, (k, var, err)
    print("%s: window against forward simulation %.2e of its peak (bound %.2e)" % (name, worst, WINDOW_RTOL))


@pytest.mark.parametrize("name", bf.NAMES)
def test_restated_closed_loop(name):
    """The float64 restatement's closed loop against the oracle's: the comparison and the tolerances
    of the GPU test."""
    case = bf.CASES[name]
    for var in range(case.nvar):
        bound, measured = bf.gentle_bound(name, var)
        for k in range(len(case.cands)):
            o = bf.oracle_loop(name, k, var)
            a = bf.restated_loop(name, k, var)
            err = bf.traj_err(a.y, a.u, o.res)
            tol = bound if k == 0 else TRAJ_RTOL
            print("%s cand %d variant %d: restated loop %.2e (tolerance %.2e; gentle float64 against longdouble %.2e)"
                  % (name, k, var, err, tol, measured))
            assert err < tol, (k, var, err, tol)


CONTROLS = [("no_shift", "so2", 5), ("mv_index", "so2", 5), ("mv_index", "integrator", 0),
            ("md_as_mv", "md_rich", 5), ("md_as_mv", "so2", 0), ("own_stride", "so2", 5), ("own_stride", "so2", 0),
            ("md_tcap", "taps", 5), ("md_tcap", "md_rich", 0)]


@pytest.mark.parametrize("fault,name,k", CONTROLS)
def test_negative_controls(fault, name, k):
    """Each planted index error of the restatement is rejected by the GPU test's comparison by more
    than 1e3 x its tolerance, on a constrained candidate and on a gentle one."""
    tol = bf.gentle_bound(name)[0] if k == 0 else TRAJ_RTOL
    o = bf.oracle_loop(name, k)
    a = bf.restated_loop(name, k, 0, np.float64, fault)
    err = bf.traj_err(a.y, a.u, o.res)
    print("%s on %s cand %d: %.2e against a tolerance of %.2e" % (fault, name, k, err, tol))
    assert err > 1e3 * tol
    assert set(f for f, _, _ in CONTROLS) == set(bw.FAULTS)
