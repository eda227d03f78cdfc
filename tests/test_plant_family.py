"""The GPC kernels on the synthetic plant family (tests/plant_family.py): every plant-layout branch
that Shell 3x3 cannot reach, each against the C port (oracle/cgpc.c) and the independent numpy
oracle (oracle/toolbox_gpc.py: primal active-set QP, no shared table code).

CPU tests: the host-only layout probe (tests/host_tables/layout_probe.cpp) pins every case to the
branch it exists for, and the two references must agree on every candidate, with rate and amplitude
bounds active in some candidate and one candidate that never touches a bound.

GPU tests, per case: the kernel instances, the cost-only batch and the open-loop + trajectory batch
against the C port, the first four candidates against the numpy oracle, the small kernel against the
general kernel, and for the plant != model cases a check that the reference itself tells the two plants
apart before the GPU is held to the mismatched one.

Tolerances are the project's own (BASELINE.json north_star: <= 1e-6 relative on du / closed-loop cost;
tests/test_gpu_parity.py holds trajectories to 1e-7 of their peak): TRAJ_RTOL = 1e-7, COST_RTOL = 1e-6,
Jnu 1e-5 under test_vns_objective's < 1e6 mask.

Measured worst errors (MI355X; trajectories: max |a - b| / max |b| over y, u, ys, uopt; costs: max
relative over J1, j21, j22):

  case                      cost-only vs C port   EXT vs C port            EXT vs numpy oracle    C port vs numpy
                            J1 (kernel)           traj      costs    Jnu     traj      costs        oracle, traj (CPU)
  small_4term_ke4           7.0e-14 (small)       1.0e-13   5.8e-14  2.0e-13 1.3e-14   1.8e-14      1.3e-13
  small_4x3                 8.9e-14 (small)       1.7e-13   8.9e-14  2.0e-13 3.3e-14   4.1e-14      3.0e-14
  small_siso                2.4e-15 (small)       1.2e-14   3.5e-14  3.5e-14 8.9e-15   1.3e-14      1.2e-14
  small_2x3                 7.9e-13 (small)       1.4e-12   1.1e-12  2.2e-13 1.8e-13   2.0e-13      1.9e-13
  packed_deep               2.2e-13 (general)     6.5e-13   1.8e-13  4.1e-13 5.6e-13   1.0e-13      6.7e-13
  lds_path                  3.9e-13 (general)     5.7e-13   3.9e-13  3.4e-14 4.1e-13   6.3e-13      4.3e-13
  many_entries              5.0e-14 (general)     3.9e-14   6.5e-14  8.8e-12 3.8e-14   5.1e-14      2.1e-14
  small_4term_ke4_mismatch  3.4e-14 (small)       1.3e-13   2.7e-14  2.0e-13 2.3e-14   2.0e-14      2.0e-13
  packed_deep_mismatch      3.2e-13 (general)     1.1e-12   8.0e-13  4.1e-13 7.1e-13   8.8e-13      1.1e-12
  lds_path_mismatch         6.0e-11 (general)     1.4e-11   2.4e-11  3.4e-14 1.8e-12   1.1e-12      7.5e-13

gpc_small_kernel against the general kernel on the same candidates (J1): at most 8.3e-14 (small_2x3).
The reference's J1 on the mismatched plant differs from its J1 on the nominal plant by at least 1.5e-2
(small_4term_ke4), 2.3e-3 (packed_deep) and 2.9e-3 (lds_path) on every candidate and output.
Every case is some four orders of magnitude inside its tolerance: no kernel or table defect turned up.
"""
import numpy as np
import pytest

import host_program
import plant_family as pf

TRAJ_RTOL = 1e-7   # tests/test_gpu_parity.py: max |a-b| / max |b| per trajectory
COST_RTOL = 1e-6   # BASELINE.json north_star
JNU_RTOL = 1e-5    # tests/test_gpu_parity.py::test_vns_objective, where the reference's Jnu < 1e6
TRAJ = ("y", "u", "ys", "uopt")


def _trel(a, b):
    return float(np.max(np.abs(a - b)) / max(float(np.max(np.abs(b))), 1e-300))


def _rel(a, b):
    return float(np.max(np.abs(a - b) / np.maximum(np.abs(b), 1e-12)))


def _traj_err(get, ref, idx=None):
    """Worst _trel over the four trajectories, each simulation on its own."""
    worst = {}
    for k in TRAJ:
        a, b = get(k), ref[k]
        worst[k] = max(_trel(a[s], b[s]) for s in (range(len(b)) if idx is None else idx))
    return worst


# ------------------------------------------------------------------------------------------------
# CPU
@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    """The layout probe, built and run by the recipe of the stand-alone check programs."""
    exe = host_program.build("layout_probe", tmp_path_factory.mktemp("layout_probe"))

    def run(case):
        stdout = host_program.run(exe, stdin=pf.descriptor_text(case), ends_ok=False)  # one line of fields, no "ok"
        fields = dict(kv.split("=", 1) for kv in stdout.split())
        coef = fields.pop("sm_coef", None)
        got = {k: int(v) for k, v in fields.items()}
        got["sm_coef"] = None if coef is None else np.array([float(x) for x in coef.split(",")])
        return got

    return run


@pytest.mark.parametrize("name", pf.NAMES)
def test_layout_pins(probe, name):
    """(i) scenario_tables.h puts the case in the class it was built for; should a limit there move,
    this fails instead of the GPU tests silently leaving their branch."""
    case = pf.CASES[name]
    got = probe(case)
    print(name, {k: v for k, v in got.items() if k != "sm_coef"})
    assert got["small"] == case.small and got["small_dtc"] == 0
    assert got["regpath"] == case.regpath
    assert got["ne"] == case.my * case.nu
    assert (got["ne"] > 16) == case.ne_over_16
    if case.small:
        assert got["sm_ke"] == case.sm_ke
        coef = got["sm_coef"]
        assert coef.shape == (64,)
        rows = [int(np.count_nonzero(coef[16 * k:16 * k + 16])) for k in range(4)]
        print(name, "nonzero plant terms per lane row", rows)
        if name.startswith("small_4term_ke4"):
            assert rows == [4, 4, 4, 4]  # every entry fills all four term rows, lanes 48..63 included
            assert np.count_nonzero(coef[48:]) >= 1
    if name == "small_siso":
        assert got["dum_max"] == 8   # kSmR: one more sample of delay and small_plant() says no
    if name.startswith("packed_deep"):
        # 4 numerator taps (kRegB), a_1..a_3 (of kRegA = 4), y history 6 (kRegY)
        assert got["pl_maxbc"] == 4 and got["pl_maxa"] == 4 and got["nyhi_max"] == 6
    if name.startswith("lds_path"):
        assert got["nyhi_max"] == 7  # > kRegY: what turns regpath off
    if case.nominal:
        nom = probe(pf.CASES[case.nominal])
        assert {k: v for k, v in got.items() if k != "sm_coef"} == {k: v for k, v in nom.items() if k != "sm_coef"}
        if case.small:  # the lane tables hold the plant, not the model: every gain differs (lane row 0)
            used = nom["sm_coef"] != 0
            assert np.array_equal(got["sm_coef"] != 0, used)
            assert np.all(got["sm_coef"][:16][used[:16]] != nom["sm_coef"][:16][used[:16]])


def test_siso_delay_is_the_longest_small_plant_takes(probe):
    """One more sample of delay and the case leaves gpc_small_kernel (dum = 9 > kSmR)."""
    case = pf.CASES["small_siso"]
    (num, den, delay), = case.model[0]
    longer = pf.Case(**dict({k: getattr(case, k) for k in case.__dataclass_fields__},
                            model=(((num, den, delay + case.Ts),),)))
    assert probe(longer)["small"] == 0


def _bound_activity(case, u):
    """Per candidate: fraction of steps with some MV's move on its rate bound, and steps with some MV
    on an amplitude bound.  u [C][nu][nit]."""
    du = np.diff(np.concatenate([np.zeros(u.shape[:2] + (1,)), u], axis=2), axis=2)
    dmax = np.array(case.du_max)[None, :, None]
    umin, umax = np.array(case.u_min)[None, :, None], np.array(case.u_max)[None, :, None]
    on_rate = np.any(np.abs(du) >= dmax * (1 - 1e-9), axis=1)
    on_amp = np.any((u >= umax - 1e-9 * np.abs(umax)) | (u <= umin + 1e-9 * np.abs(umin)), axis=1)
    # strictly inside: not within 1e-6 of a bound
    near = np.any(np.abs(du) >= dmax * (1 - 1e-6), axis=1) | \
        np.any((u >= umax - 1e-6 * np.abs(umax)) | (u <= umin + 1e-6 * np.abs(umin)), axis=1)
    return on_rate.mean(axis=1), on_amp.sum(axis=1), ~np.any(near, axis=1)


@pytest.mark.parametrize("name", pf.NAMES)
def test_references_agree_and_inputs_fit(built, name):
    """(ii) the C port and the numpy oracle agree on every candidate of the case, and the case's
    inputs do what they are for: rate and amplitude bounds active, one candidate never on a bound."""
    case = pf.CASES[name]
    N2, Nu, d, l = pf.candidates(case)
    C = len(N2)
    assert C <= 16 and 60 <= case.nit <= 120
    assert len({t0 for t0, _ in case.steps}) == case.my and all(lv != 0.0 for _, lv in case.steps)
    ref = pf.cport_ext(name)
    assert np.all(ref["status"] == 0), ref["status"]
    assert np.all(pf.cport_costs(name)["status"] == 0)
    worst = dict.fromkeys(TRAJ, 0.0)
    for k in range(C):
        o = pf.numpy_oracle(name, k)  # raises when its QP does not converge: its status 0 is returning
        for q in TRAJ:
            worst[q] = max(worst[q], _trel(getattr(o, q), ref[q][k]))
    print("%s: C port vs numpy oracle, worst over %d candidates: %s" % (
        name, C, ", ".join("%s %.1e" % kv for kv in worst.items())))
    assert max(worst.values()) < TRAJ_RTOL, worst
    rate, amp, never = _bound_activity(case, ref["u"])
    print("%s: steps on a rate bound %s, steps on an amplitude bound %s, never on a bound %s" % (
        name, np.round(rate, 2).tolist(), amp.tolist(), np.nonzero(never)[0].tolist()))
    assert rate.max() >= 0.05
    assert amp.max() >= 1
    assert never.any()
    # one batch reaches every QP-size class the scenario has, on both sides of each class edge
    M = case.nu * Nu
    top = case.nu * case.nu_max
    assert M.max() == top and np.all(Nu <= N2) and N2.max() == case.n2_max
    for edge in (16, 32):
        if top > edge:
            below, above = edge - edge % case.nu, edge - edge % case.nu + case.nu
            assert below in M and above in M, (edge, M)


# ------------------------------------------------------------------------------------------------
# GPU
@pytest.fixture(scope="module")
def gpu(built, has_gpu):
    if not has_gpu:
        pytest.skip("no GPU")
    return True


_RUNS = {}


def _runs(name):
    """The case's product scenario with its cost-only and EXT batches (one GPU run each per session)."""
    if name not in _RUNS:
        from mpct.engine import eval_batch

        case = pf.CASES[name]
        sc, r, yref = pf.product(case)
        _, _, orr, oyref = pf.cport(name)
        assert np.array_equal(r, orr) and np.allclose(yref, oyref, rtol=0, atol=1e-14)
        N2, Nu, d, l = pf.candidates(case)
        cost = eval_batch(sc, N2, Nu, d, l, r[None])
        ext = eval_batch(sc, N2, Nu, d, l, r[None], open_loop=True, want_traj=True)
        _RUNS[name] = dict(sc=sc, cost=cost, ext=ext)
    return _RUNS[name]


@pytest.mark.gpu
@pytest.mark.parametrize("name", pf.NAMES)
def test_gpu_case(gpu, name):
    from mpct.engine import kernel_instance
    from mpct.objectives import rank

    case = pf.CASES[name]
    run = _runs(name)
    sc, cost, ext = run["sc"], run["cost"], run["ext"]
    # (iii) the kernels the case is for
    assert (kernel_instance(sc), kernel_instance(sc, want_traj=True)) == case.instances
    assert kernel_instance(sc, open_loop=True, want_traj=True) == case.instances[1]
    # (iv) cost-only batch against the C port
    cref = pf.cport_costs(name)
    kern = "small kernel" if case.small else "general kernel"
    e_j1, e_j22 = _rel(cost.J1, cref["J1"]), _rel(cost.j22, cref["j22"])
    print("%s: cost-only (%s) vs C port: J1 %.1e, j22 %.1e" % (name, kern, e_j1, e_j22))
    assert np.all(cost.status == 0), cost.status
    assert e_j1 < COST_RTOL and e_j22 < COST_RTOL
    assert np.array_equal(rank(cost.J1.sum(1)), rank(cref["J1"].sum(1)))
    # (v) open-loop + trajectory batch against the C port
    ref = pf.cport_ext(name)
    te = _traj_err(lambda k: getattr(ext, k), ref)
    ce = {k: _rel(getattr(ext, k), ref[k]) for k in ("J1", "j21", "j22")}
    ok = ref["Jnu"] < 1e6
    e_jnu = _rel(ext.Jnu[ok], ref["Jnu"][ok])
    print("%s: EXT (general kernel) vs C port: %s; %s; Jnu %.1e" % (
        name, ", ".join("%s %.1e" % kv for kv in te.items()), ", ".join("%s %.1e" % kv for kv in ce.items()), e_jnu))
    assert np.all(ext.status == 0), ext.status
    assert max(te.values()) < TRAJ_RTOL, te
    assert max(ce.values()) < COST_RTOL, ce
    assert e_jnu < JNU_RTOL
    # (vi) the first four candidates against the numpy oracle
    _, _, _, oyref = pf.cport(name)
    tn = dict.fromkeys(TRAJ, 0.0)
    e_np = 0.0
    for k in range(4):
        o = pf.numpy_oracle(name, k)
        for q in TRAJ:
            tn[q] = max(tn[q], _trel(getattr(ext, q)[k], getattr(o, q)))
        J1 = ((o.y - oyref) ** 2).sum(axis=1)
        j21 = ((o.y - o.ys)[:, 9:] ** 2).sum(axis=1)      # VNS2.m:172-177 from inK = 10 on
        j22 = ((o.y - oyref)[:, 9:] ** 2).sum(axis=1)
        e_np = max(e_np, _rel(ext.J1[k], J1), _rel(ext.j21[k], j21), _rel(ext.j22[k], j22), _rel(cost.J1[k], J1))
    print("%s: EXT vs numpy oracle (4 candidates): %s; costs %.1e" % (
        name, ", ".join("%s %.1e" % kv for kv in tn.items()), e_np))
    assert max(tn.values()) < TRAJ_RTOL, tn
    assert e_np < COST_RTOL
    # (vii) two kernels on one problem
    if case.small:
        e_two = _rel(cost.J1, ext.J1)
        print("%s: gpc_small_kernel vs general kernel J1 %.1e" % (name, e_two))
        assert e_two < COST_RTOL


@pytest.mark.gpu
@pytest.mark.parametrize("name", pf.MISMATCH)
def test_gpu_follows_the_plant_not_the_model(gpu, name):
    """(viii) the reference tells the mismatched plant from the nominal one by far more than the
    tolerance on every candidate, so the GPU cannot match it while reading the model for the plant
    (or the plant for the model)."""
    case = pf.CASES[name]
    assert pf.candidates(case)[2].tobytes() == pf.candidates(pf.CASES[case.nominal])[2].tobytes()
    ref, nom = pf.cport_costs(name), pf.cport_costs(case.nominal)
    diff = np.abs(ref["J1"] - nom["J1"]) / np.abs(nom["J1"])
    print("%s: reference J1, mismatched vs nominal plant: least relative difference %.1e" % (name, diff.min()))
    assert diff.min() >= 1000 * COST_RTOL  # every candidate, every output
    for kind in ("cost", "ext"):
        assert _rel(_runs(name)[kind].J1, ref["J1"]) < COST_RTOL, kind
