"""GPU: plant variants on gpc_small_kernel (Shell 3x3 model-error draws, mpct.scenarios.shell3x3_mc).

Everything runs at nit = 200 (two setpoint jumps, the move and amplitude bounds active).  The
yardsticks are the single-plant scenarios on the same kernel (bitwise), the general kernel, the
oracle's C port and numpy closed loop with the draw as the simulated plant, and include/mpct.h's
reduction restated in numpy.  The oracle's plants are built here from the oracle's own helpers
(oracle.matlab.c2d_zoh) and Shell3x3.m's numbers, not from the product's constructor."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

NIT = 200
SEED = 20250307
COST_RTOL = 1e-6   # BASELINE cost tolerance (tests/test_gpu_parity.py)
E_MAX = np.array([0.2, 0.2, 0.3])                                      # Shell3x3.m:38
DK = np.array([[2.11, 0.39, 0.59], [3.29, 0.57, 0.89], [3.11, 0.73, 1.33]])   # Shell3x3.m:43-45
REF_SCALE = (1.0, 0.8, 0.6, 1.1, 0.9)   # five different reference sets: k = 3, 4 wrap to variants 0, 1


@pytest.fixture(scope="module")
def gpu(built, has_gpu):
    if not has_gpu:
        pytest.skip("no GPU")
    return True


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int64 if a.dtype == np.float64 else a.dtype)


def same_record(a, b, rows_a=slice(None), rows_b=slice(None), msg=""):
    for f in ("J1", "j22", "status", "qp_iters"):
        np.testing.assert_array_equal(bits(getattr(a, f)[rows_a]), bits(getattr(b, f)[rows_b]), err_msg="%s %s" % (f, msg))


def make(plants, nu_max=5, n2_max=30):
    """The Shell 3x3 loop of shell3x3() on `plants`: one plant -> a single-plant scenario."""
    from mpct.engine import Scenario
    from mpct.scenarios import SHELL3_L as L, SHELL3_R as R, SHELL3_TS, shell3x3_plant, shell3x3_xsp, shell3x3_yref

    X = shell3x3_xsp(NIT)
    sc = Scenario(plants[0], shell3x3_plant(), nu=3, du_min=-0.05 / R, du_max=0.05 / R, u_min=-1.0 / R, u_max=0.5 / R,
                  yref=L[:, None] * shell3x3_yref(X), n2_max=n2_max, nu_max=nu_max, Ts=SHELL3_TS,
                  plant_variants=plants if len(plants) > 1 else None)
    return sc, L[:, None] * X


def refs5(r):
    return np.stack([s * r for s in REF_SCALE])


# Candidates for the comparisons between different implementations.  A loop whose plant gains exceed
# the model's by up to 30 % is, for most of the metric grid's candidates, a bounded oscillation against
# the move bounds that amplifies a rounding error to O(1) in the cost: on the oracle's C port alone,
# perturbing delta or lambda by 1e-13 relative changes J1 by 1e-4 .. 1 for 13 of candidate_grid(16)'s
# candidates on draw 0.  No two implementations agree to 1e-6 on such a simulation, and none is wrong.
# So the parity tests take the first 16 of candidate_grid(1024)'s candidates for which the C port's
# J1 moves by <= 3e-11 relative under both perturbations on every one of the simulations used here
# (3 draws x 5 reference sets for max_dshift = 0 and 2; 3 draws x the setpoint itself); 54 of the 1024
# qualify.  The choice was made on the CPU with the C port alone, and each test repeats that check on
# the simulations it compares before it compares anything (status 0, finite, J1 moving by <= 1e-10),
# so no simulation is left out of a comparison.  The bitwise tests need no such care and use candidate_grid(16).
SEL = (4, 19, 43, 70, 83, 91, 169, 188, 194, 195, 198, 205, 207, 212, 222, 270)
COND_EPS, COND_MAX = 1e-13, 1e-10


def selected(n=16):
    from mpct.scenarios import candidate_grid

    return tuple(np.ascontiguousarray(a[list(SEL[:n])]) for a in candidate_grid(1024))


_cache = {}


def batch(dshift, sel=False):
    """16 candidates x 5 reference sets on 3 variants: the variant scenario's cost-only records."""
    from mpct.engine import eval_batch, kernel_instance
    from mpct.scenarios import candidate_grid, shell3x3_mc_plants

    if (dshift, sel) not in _cache:
        plants = shell3x3_mc_plants(3, max_dshift=dshift)
        sc, r = make(plants)
        assert sc.nplant == 3 and kernel_instance(sc) == "gpc_small_kernel"
        cand = selected() if sel else candidate_grid(16)
        _cache[(dshift, sel)] = dict(plants=plants, sc=sc, r=r, cand=cand, res=eval_batch(sc, *cand, refs5(r)))
    return _cache[(dshift, sel)]


def oracle_plants(draws, dshift):
    """The draws restated with the oracle's helpers: gains K + DK e (draw 0: e = e_max; then U(-e_max,
    e_max) from default_rng(SEED)), delay shifts from default_rng([SEED, 1])."""
    from oracle.matlab import c2d_zoh
    from oracle.scenarios import SHELL3_K, SHELL3_L as DELAY, SHELL3_TAU, SHELL3_TS, load_fixture

    fx = load_fixture()
    L, R = np.array(fx["scale"]["L"]), np.array(fx["scale"]["R"])
    rng, rng_d = np.random.default_rng(SEED), np.random.default_rng([SEED, 1])
    out = []
    for k in range(draws):
        e = E_MAX if k == 0 else rng.uniform(-E_MAX, E_MAX)
        sh = np.zeros((3, 3), dtype=int) if k == 0 or dshift == 0 else rng_d.integers(0, dshift + 1, (3, 3))
        out.append([[c2d_zoh([SHELL3_K[i, j] + DK[i, j] * e[j]], [SHELL3_TAU[i, j], 1.0], SHELL3_TS,
                             DELAY[i, j] + SHELL3_TS * sh[i, j]).scaled(L[i] * R[j]) for j in range(3)]
                    for i in range(3)])
    return out


def oracle_scenario(Pv):
    from oracle.scenarios import shell3x3 as o_shell3x3
    from oracle.toolbox_gpc import Scenario as OScenario

    osc, orr, oyref, _ = o_shell3x3()
    o = OScenario(plant=Pv, model=osc.model, nu=3, du_min=osc.du_min, du_max=osc.du_max, u_min=osc.u_min,
                  u_max=osc.u_max)
    return o, orr[:, :NIT], oyref[:, :NIT]


def cport_J1(dshift, cand, nvar, scales):
    """C-port records of simulation (c, k) = candidate c, reference set k, plant k % nvar: J1 [C, K, 3],
    status [C, K], and the largest relative change of J1 [C, K] when delta or lambda moves by COND_EPS."""
    from oracle.cport import CPort

    op = oracle_plants(nvar, dshift)
    N2, Nu, d, l = cand
    J1 = np.zeros((len(N2), len(scales), 3))
    st = np.zeros((len(N2), len(scales)), dtype=np.int32)
    cond = np.zeros((len(N2), len(scales)))
    for k, s in enumerate(scales):
        o, orr, oyref = oracle_scenario(op[k % nvar])
        cp = CPort(o, 30, NIT, oyref)
        ref = cp.eval(N2, Nu, d, l, (s * orr)[None])
        J1[:, k], st[:, k] = ref["J1"], ref["status"]
        for dd, ll in ((d * (1 + COND_EPS), l), (d, l * (1 - COND_EPS))):
            alt = cp.eval(N2, Nu, dd, ll, (s * orr)[None])["J1"]
            cond[:, k] = np.maximum(cond[:, k], np.max(np.abs(alt - ref["J1"]) / np.abs(ref["J1"]), axis=1))
    return J1, st, cond


# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dshift", [0, 2])
def test_variant_identity_bitwise(gpu, dshift):
    """Simulation (c, k) of the 3-variant scenario is the single-plant scenario of plant k % 3 on
    reference k, bit for bit (both on gpc_small_kernel): J1, j22, status, qp_iters.  With
    max_dshift = 2 the variants' ring delays (the hc table) differ as well."""
    from mpct.engine import eval_batch, kernel_instance

    b = batch(dshift)
    res, refs = b["res"], refs5(b["r"])
    assert res.status.shape == (16 * 5,) and not np.any(res.status & 128)
    if dshift:
        assert any(b["plants"][v][i][j].delay != b["plants"][0][i][j].delay for v in (1, 2) for i in range(3) for j in range(3))
    seen = set()
    for k in range(5):
        one, _ = make([b["plants"][k % 3]])
        assert one.nplant == 1 and kernel_instance(one) == "gpc_small_kernel"
        alone = eval_batch(one, *b["cand"], refs[k][None])
        same_record(res, alone, slice(k, None, 5), msg="k = %d" % k)
        seen.add(bits(alone.J1).tobytes())
        one.close()
    assert len(seen) == 5   # five different simulations per candidate: the identity is not vacuous


@pytest.mark.parametrize("dshift", [0, 2])
def test_against_general_kernel_and_cport(gpu, dshift):
    """The batch of the identity test on the selected candidates (SEL above: how they were chosen),
    cost-only on gpc_small_kernel and with trajectories on the general kernel
    (gpc_closed_loop_kernel<16,false,true>, which has honoured k % nvar since plant variants exist):
    identical statuses, J1 within 1e-6 relative.  The C port's own records come first: all 80
    simulations finite with status 0 and well conditioned.  Its parity figures are printed."""
    from mpct.engine import eval_batch, kernel_instance

    b = batch(dshift, sel=True)
    J1c, stc, cond = cport_J1(dshift, b["cand"], 3, REF_SCALE)
    assert np.all(stc == 0) and np.all(np.isfinite(J1c)) and cond.max() <= COND_MAX, cond.max()
    assert kernel_instance(b["sc"], want_traj=True) == "gpc_closed_loop_kernel<16,false,true>"
    gen = eval_batch(b["sc"], *b["cand"], refs5(b["r"]), want_traj=True)
    np.testing.assert_array_equal(gen.status, b["res"].status)
    assert np.all(gen.status == 0)
    assert np.any(b["res"].qp_iters > 0)   # the bounds are active
    rel = np.max(np.abs(b["res"].J1 - gen.J1) / np.abs(gen.J1))
    rel_c = np.max(np.abs(b["res"].J1.reshape(16, 5, 3) - J1c) / np.abs(J1c))
    rel_g = np.max(np.abs(gen.J1.reshape(16, 5, 3) - J1c) / np.abs(J1c))
    print("max_dshift %d: small vs general %.2e, small vs C port %.2e, general vs C port %.2e; C port conditioning %.1e"
          % (dshift, rel, rel_c, rel_g, cond.max()))
    assert rel < COST_RTOL


def test_against_oracle(gpu):
    """8 selected candidates x 3 draws of shell3x3_mc against oracle.cport.CPort on
    oracle.toolbox_gpc.Scenario(plant = the draw, model = the nominal model): J1 within 1e-6 relative
    (the C port's records finite, status 0 and well conditioned first); two of the simulations (draw 0,
    the reference's error case, of the first candidate and draw 1 of the sixth) against the numpy
    closed loop (primal active-set QP) as well."""
    from mpct.engine import eval_batch, kernel_instance
    from mpct.scenarios import shell3x3_mc
    from oracle.toolbox_gpc import closedloop_toolbox as o_cl

    sc, refs, _ = shell3x3_mc(draws=3, nit=NIT)
    assert kernel_instance(sc) == "gpc_small_kernel"
    cand = selected(8)
    res = eval_batch(sc, *cand, refs)
    assert np.all(res.status == 0) and np.any(res.qp_iters > 0)
    J1c, stc, cond = cport_J1(0, cand, 3, (1.0, 1.0, 1.0))
    assert np.all(stc == 0) and np.all(np.isfinite(J1c)) and cond.max() <= COND_MAX, cond.max()
    got = res.J1.reshape(8, 3, 3)
    rel = np.max(np.abs(got - J1c) / np.abs(J1c))
    print("8 x 3 vs C port: J1 max rel %.2e (C port conditioning %.1e)" % (rel, cond.max()))
    assert rel < COST_RTOL
    op = oracle_plants(3, 0)
    for c, k in ((0, 0), (5, 1)):
        o, orr, oyref = oracle_scenario(op[k])
        cl = o_cl(o, orr, None, 30, 5, cand[2][c], cand[3][c], NIT, open_loop=False)
        J = ((cl.y - oyref) ** 2).sum(axis=1)
        rel = np.max(np.abs(got[c, k] - J) / np.abs(J))
        print("candidate %d draw %d vs numpy oracle: J1 max rel %.2e" % (SEL[c], k, rel))
        assert rel < COST_RTOL
    sc.close()


def test_mixed_classes(gpu):
    """nu_max = 6, candidates at Nu = 5 (M = 15: gpc_small_kernel) and Nu = 6 (M = 18: the general
    kernel's wider class) over 3 variants x 5 reference sets: no slot keeps MPCT_ST_NOT_RUN, and every
    simulation matches its single-plant evaluation, bitwise in the small class, 1e-9 relative in the
    general class (two launches of one kernel on the same data)."""
    from mpct.engine import eval_batch, kernel_instance
    from mpct.scenarios import candidate_grid, shell3x3_mc_plants

    plants = shell3x3_mc_plants(3, max_dshift=2)
    sc, r = make(plants, nu_max=6)
    assert kernel_instance(sc) == "gpc_small_kernel + gpc_closed_loop_kernel<32,false,false>"
    N2, Nu, d, l = candidate_grid(12)
    Nu = np.where(np.arange(12) % 3 == 1, 6, 5).astype(np.int32)
    refs = refs5(r)
    res = eval_batch(sc, N2, Nu, d, l, refs)
    assert not np.any(res.status & 128), res.status
    small = np.repeat(Nu == 5, 5)
    assert small.sum() == 40 and (~small).sum() == 20
    for k in range(5):
        one, _ = make([plants[k % 3]], nu_max=6)
        alone = eval_batch(one, N2, Nu, d, l, refs[k][None])
        rows = np.arange(12) * 5 + k
        sm, ge = rows[Nu == 5], rows[Nu == 6]
        same_record(res, alone, sm, np.flatnonzero(Nu == 5), msg="k = %d" % k)
        np.testing.assert_array_equal(res.status[ge], alone.status[Nu == 6])
        ok = alone.status[Nu == 6] == 0
        assert ok.any()
        np.testing.assert_allclose(res.J1[ge][ok], alone.J1[Nu == 6][ok], rtol=1e-9, atol=0)
        np.testing.assert_allclose(res.j22[ge][ok], alone.j22[Nu == 6][ok], rtol=1e-9, atol=0)
        one.close()
    sc.close()


# ---------------------------------------------------------------------------------------------
def reduce_np(J1, st, jb):
    """include/mpct.h's record from J1 [C, D, my] and status [C, D], in robust_reduce.h's order: J(k)
    summed over the outputs in order, one accumulator per output over the surviving draws in order."""
    Cn, D, my = J1.shape
    out = dict(mean=np.full((Cn, my), np.nan), worst=np.full((Cn, my), np.nan), n_failed=np.zeros(Cn, np.int32),
               worst_draw=np.full(Cn, -1, np.int32), status=np.bitwise_or.reduce(st, axis=1).astype(np.int32))
    for c in range(Cn):
        s, mx, jw, n = np.zeros(my), np.zeros(my), 0.0, 0
        for k in range(D):
            J = 0.0
            for i in range(my):
                J = J + J1[c, k, i]
            if st[c, k] == 0 and np.isfinite(J) and J <= jb:
                s = s + J1[c, k]
                mx = J1[c, k].copy() if n == 0 else np.maximum(mx, J1[c, k])
                if n == 0 or J > jw:
                    jw, out["worst_draw"][c] = J, k
                n += 1
            else:
                out["n_failed"][c] += 1
        if n:
            out["mean"][c], out["worst"][c] = s / float(n), mx
    return out


def check_record(res, ref):
    for f in ("mean", "worst", "n_failed", "worst_draw", "status"):
        np.testing.assert_array_equal(bits(getattr(res, f)), bits(ref[f]), err_msg=f)


def test_robust_entry(gpu):
    """eval_robust on shell3x3_mc(draws = 4) (gpc_small_kernel + robust_reduce_kernel) with the
    per-simulation J1: the record is include/mpct.h's reduction of that J1 (statuses from eval_batch,
    whose J1 is bitwise the same), bit for bit, at the default bound; a repeated call is bitwise
    identical.

    A fifth variant with every gain negated: the loop's inputs are bounded and the plant is stable,
    so it does not overflow; it runs into the amplitude bounds with status 0 and a total cost of 132
    .. 8542 over these candidates, against at most 24 for the four mismatch draws (C port on the
    CPU).  A draw like that is failed by the documented cost bound: with j_bound = 56, a factor two
    from either group (asserted on the records first), it counts in n_failed for every candidate and is
    never the worst draw; at the default bound it survives and is the worst draw of every candidate."""
    from mpct.engine import eval_batch, eval_robust, robust_instance
    from mpct.lti import Tf
    from mpct.scenarios import candidate_grid, shell3x3_mc

    sc, refs, plants = shell3x3_mc(draws=4, nit=NIT)
    assert robust_instance(sc) == "gpc_small_kernel + robust_reduce_kernel"
    cand = candidate_grid(16)
    a = eval_robust(sc, *cand, refs, want_J1=True)
    per = eval_batch(sc, *cand, refs)
    np.testing.assert_array_equal(bits(a.J1), bits(per.J1))
    assert np.all(per.status == 0)
    check_record(a, reduce_np(a.J1.reshape(16, 4, 3), per.status.reshape(16, 4), 1e100))
    assert np.all(a.n_failed == 0)
    b = eval_robust(sc, *cand, refs, want_J1=True)
    for f in ("mean", "worst", "n_failed", "worst_draw", "status", "J1"):
        np.testing.assert_array_equal(bits(getattr(a, f)), bits(getattr(b, f)), err_msg=f)
    sc.close()

    neg = [[Tf(tuple(-x for x in t.num), t.den, t.delay) for t in row] for row in plants[0]]
    sc5, r = make(plants + [neg])
    assert sc5.nplant == 5 and robust_instance(sc5) == "gpc_small_kernel + robust_reduce_kernel"
    refs = np.broadcast_to(r, (5, 3, NIT)).copy()
    jb = 56.0
    per = eval_batch(sc5, *cand, refs)
    J = per.J1.reshape(16, 5, 3).sum(axis=2)
    print("negated draw: status %s, J %.4g .. %.4g; the other draws' J up to %.4g" % (
        np.unique(per.status.reshape(16, 5)[:, 4]).tolist(), J[:, 4].min(), J[:, 4].max(), J[:, :4].max()))
    assert np.all(per.status == 0) and np.all(J[:, :4] < jb / 2) and np.all(J[:, 4] > 2 * jb)
    c = eval_robust(sc5, *cand, refs, j_bound=jb, want_J1=True)
    np.testing.assert_array_equal(bits(c.J1), bits(per.J1))
    np.testing.assert_array_equal(bits(c.J1.reshape(16, 5, 3)[:, :4]), bits(a.J1.reshape(16, 4, 3)))
    check_record(c, reduce_np(c.J1.reshape(16, 5, 3), per.status.reshape(16, 5), jb))
    assert np.all(c.n_failed == 1) and np.all(c.worst_draw != 4) and np.all(c.worst_draw >= 0)
    np.testing.assert_array_equal(bits(c.worst), bits(a.worst))
    np.testing.assert_array_equal(c.worst_draw, a.worst_draw)
    d = eval_robust(sc5, *cand, refs, want_J1=True)
    check_record(d, reduce_np(d.J1.reshape(16, 5, 3), per.status.reshape(16, 5), 1e100))
    assert np.all(d.n_failed == 0) and np.all(d.worst_draw == 4)
    sc5.close()
