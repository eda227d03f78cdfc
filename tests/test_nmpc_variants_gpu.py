"""Plant-parameter draws in the NMPC kernel on the GPU (nmpc_closed_loop_kernel<MAXM, VAR = true>,
mpct_nmpc_scenario_create_var): variants equal to the model are bitwise the nominal kernel, simulation
(c, k) runs variant k % nplant, mismatched loops equal the numpy reference (tests/nmpc_mismatch_ref.py)
and eval_robust is eval_batch plus the reduction rule.  nit = 60 throughout."""
import numpy as np
import pytest

import nmpc_mismatch_ref as mr

TRAJ_RTOL = 1e-7     # tests/test_nmpc.py's tolerances
COST_RTOL = 1e-6
VARIANT = "nmpc_closed_loop_kernel<..., plant variants> (QP-size x LDS-tier class launches)"
FIELDS = ("status", "qp_iters", "J1", "j21", "j22", "Jnu", "y", "u", "ys", "uopt")


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int64) if a.dtype == np.float64 else a


def _trel(a, b):
    return float(np.max(np.abs(a - b)) / max(float(np.max(np.abs(b))), 1e-300))


def _same(a, b, rows_a=None, rows_b=None, what=""):
    for f in FIELDS:
        x, y = getattr(a, f), getattr(b, f)
        if rows_a is not None:
            x, y = x[rows_a], y[rows_b]
        np.testing.assert_array_equal(bits(x), bits(y), err_msg="%s %s" % (what, f))


@pytest.fixture(scope="module")
def gpu(built, has_gpu):
    if not has_gpu:
        pytest.skip("no GPU")
    return True


def _scenario(n_max=31, nu_max=15, **kw):
    from mpct import nmpc

    x0 = nmpc.steady_state()
    r, yref = nmpc.vandevusse_signals(x0)
    sc = nmpc.NmpcScenario(x0, nmpc.VDV_U0, nmpc.VDV_UMIN, nmpc.VDV_UMAX, nmpc.VDV_XMIN, nmpc.VDV_XMAX, yref, n_max,
                           nu_max, **kw)
    return sc, x0, r, yref


def _run(sc, cands, refs):
    from mpct.engine import eval_batch

    N, Nu, d, lam = cands
    return eval_batch(sc, N, Nu, d, lam, refs, open_loop=True, want_traj=True)


# ---- candidates and draws of the parity test.  (N, Nu, delta, lambda): M = 2 Nu = 4 (the tuned point),
# 6, 8, 10, 12, 14 (the M <= 15 class) and 16; short horizons, so each holds four point buffers
def _parity_cands():
    from mpct.nmpc import VDV_TUNED as T

    c = [(T["N"], max(T["Nu"]), T["delta"], T["lam"]),
         (5, 3, (1.0, 0.5), (0.05, 0.02)),
         (6, 4, (0.7, 1.0), (0.05, 0.2)),
         (7, 5, (1.0, 1.0), (0.1, 0.1)),
         (6, 6, (0.3, 0.2), (0.3, 0.1)),
         (8, 7, (1.0, 0.5), (0.1, 0.1)),
         (9, 8, (0.5, 1.0), (0.2, 0.05))]
    return (np.array([x[0] for x in c], np.int32), np.array([x[1] for x in c], np.int32),
            np.array([x[2] for x in c], float), np.array([x[3] for x in c], float))


# factors on (k10, k20, k30) and on (dHab, dHbc, dHad): the corners of +-5 %
DRAWS = [((1.05, 1.05, 1.05), (1.05, 1.05, 1.05)),
         ((0.95, 0.95, 0.95), (0.95, 0.95, 0.95)),
         ((1.05, 0.95, 1.05), (0.95, 1.05, 0.95)),
         ((0.95, 1.05, 0.95), (1.05, 0.95, 1.05))]
# (candidate, draw, plant_x0 given): a fixed spread of twelve over every candidate, draw and start state,
# out of the 56 pairs that met the conditioning rule (all 56 did, see test_matches_reference)
PAIRS = [(0, 0, True), (0, 3, False), (1, 1, True), (1, 2, False), (2, 0, False), (3, 1, False), (3, 2, True),
         (4, 3, True), (5, 0, True), (5, 2, False), (6, 1, True), (6, 3, False)]


def _nm_total(M, N, G):
    """nmpc_model.h nm_layout(M, N, G).total, restated (doubles)."""
    ev = lambda n: (n + 1) & ~1
    o = ev(M * (M + 1) // 2) + ev(M * M) + ev(M * (M + 3) // 2) + 4 * ev(M + 1) + ev((6 * N + 63) // 64)
    w = 16 if G > 1 else M + 1
    g = ev(M * (M + 1) // 2) + 4 * ev(w) + ev(3 * N) + ev(3 * N * M)
    return ev(o + G * g)


def _four_buffers(M, N):
    return M <= 15 and _nm_total(M, N, 4) * 8 <= 40 * 1024


@pytest.mark.gpu
def test_nominal_bitwise(gpu):
    """1. Three variants equal to the model, plant_x0 = x0: every result field of the VAR = true
    instances is bitwise the nominal kernel's, on test_nmpc's seven candidates and, on an n_max = 127,
    nu_max = 8 scenario, on (31, 8) (M = 16), (70, 7) (two point buffers) and (127, 7) (one)."""
    from mpct.engine import kernel_instance
    from test_nmpc import _cands

    long_c = (np.array([31, 70, 127], np.int32), np.array([8, 7, 7], np.int32),
              np.array([[1.0, 1.0], [0.7, 1.0], [1.0, 0.5]]), np.array([[0.1, 0.1], [0.05, 0.2], [0.1, 0.1]]))
    assert not _four_buffers(14, 70) and _nm_total(14, 70, 2) * 8 <= 64 * 1024 < _nm_total(14, 127, 2) * 8
    for (n_max, nu_max), cands in (((31, 15), _cands()), ((127, 8), long_c)):
        nom, x0, r, _ = _scenario(n_max, nu_max)
        var = _scenario(n_max, nu_max, plant_params=np.tile(mr.MODEL, (3, 1)), plant_x0=np.tile(x0, (3, 1)))[0]
        assert kernel_instance(var) == VARIANT and kernel_instance(nom) != VARIANT
        refs = np.stack([r, r, r])
        a, b = _run(nom, cands, refs), _run(var, cands, refs)
        assert np.all(a.status == 0), a.status
        _same(a, b, what="n_max %d" % n_max)


@pytest.mark.gpu
def test_variant_indexing(gpu):
    """2. nref = 5 over nplant = 3: simulation (c, k) is bitwise the single-variant scenario of plant
    k % 3 on reference k."""
    from mpct import nmpc

    P = np.array([mr.scaled(mr.MODEL, *DRAWS[0]), mr.MODEL, mr.scaled(mr.MODEL, *DRAWS[3])])
    X0 = np.array([nmpc.steady_state(params=p) for p in P])
    sc = _scenario(plant_params=P, plant_x0=X0)[0]
    # five distinct reference sets: each plant's own, then two with shifted setpoints
    refs = np.stack([nmpc.vandevusse_signals(X0[k % 3])[0] for k in range(5)])
    refs[3, 0, 9:] = 0.98
    refs[4, 1, 40:] = 131.0
    N, Nu, d, lam = _parity_cands()
    pick = [0, 3, 6]   # M = 4, 10 and 16
    cands = (N[pick], Nu[pick], d[pick], lam[pick])
    full = _run(sc, cands, refs)
    assert full.y.shape[0] == 15
    differ = 0
    for v in range(3):
        ks = [k for k in range(5) if k % 3 == v]
        one = _run(_scenario(plant_params=P[v], plant_x0=X0[v])[0], cands, refs[ks])
        rows_full = [c * 5 + k for c in range(3) for k in ks]
        _same(full, one, rows_full, list(range(3 * len(ks))), what="variant %d" % v)
        differ += int(not np.array_equal(full.y[0 * 5 + ks[0]], full.y[0 * 5 + (ks[0] + 1) % 5]))
    assert differ == 3   # neighbouring draws are different loops


@pytest.fixture(scope="module")
def parity(gpu):
    """The device results of every candidate x draw of both scenarios (plant_x0 given / NULL), and the
    reference loops of PAIRS, computed once."""
    from mpct import nmpc

    x0 = nmpc.steady_state()
    r0, yref = nmpc.vandevusse_signals(x0)
    P = np.array([mr.scaled(mr.MODEL, k, h) for k, h in DRAWS])
    X0 = np.array([nmpc.steady_state(params=p) for p in P])
    cands = _parity_cands()
    dev, start, refs = {}, {}, {}
    for given in (True, False):
        sc = _scenario(plant_params=P, plant_x0=X0 if given else None)[0]
        start[given] = X0 if given else np.tile(x0, (4, 1))
        refs[given] = np.stack([nmpc.vandevusse_signals(xs)[0] for xs in start[given]])
        dev[given] = _run(sc, cands, refs[given])
    ref = {}
    for ci, di, given in PAIRS:
        ref[ci, di, given] = mr.closedloop_mismatch(refs[given][di], int(cands[0][ci]), int(cands[1][ci]), cands[2][ci],
                                                    cands[3][ci], P[di], start[given][di])
    return dict(dev=dev, ref=ref, yref=yref, cands=cands)


@pytest.mark.gpu
def test_matches_reference(parity):
    """3. Twelve candidate x draw pairs at the corners of +-5 % on the rate constants and the reaction
    enthalpies, plant_x0 given (each plant's own steady state and its references) and NULL (the model's
    x0), open_loop = 1 and want_traj = 1: y, u, ys, uopt within 1e-7 of their peak, J1 / j22 / j21 / Jnu
    within 1e-6.

    The pairs were picked on the CPU by the rule: a 1e-13 relative change of lambda moves the reference's
    own J1 by less than 1e-9 relative.  Tried: all 56 pairs of 7 candidates x 4 draws x 2 start states.
    Rejected: none (the largest change was 1.6e-13: these mismatched loops are as well conditioned as the
    nominal one).  PAIRS is a fixed spread of twelve of them over every candidate; ten are in the M <= 15
    class with four point buffers, where the speculation runs."""
    N, Nu = parity["cands"][0], parity["cands"][1]
    assert len(PAIRS) == 12 and len(set(PAIRS)) == 12
    assert sum(_four_buffers(2 * int(Nu[c]), int(N[c])) for c, _, _ in PAIRS) >= 6
    assert {2 * int(Nu[c]) for c, _, _ in PAIRS} == {4, 6, 8, 10, 12, 14, 16}
    assert {g for _, _, g in PAIRS} == {True, False} and {d for _, d, _ in PAIRS} == {0, 1, 2, 3}
    yref = parity["yref"]
    for ci, di, given in PAIRS:
        res, o = parity["dev"][given], parity["ref"][ci, di, given]
        s = ci * 4 + di
        assert res.status[s] == 0 and o.bounds_ok, (ci, di, given, res.status[s])
        errs = [_trel(a, b) for a, b in ((res.y[s], o.y), (res.u[s], o.u), (res.ys[s], o.yopt), (res.uopt[s], o.uopt))]
        J = mr.costs(o, yref)
        cerr = [float(np.max(np.abs(getattr(res, f)[s] - J[f]) / np.maximum(np.abs(J[f]), 1e-300)))
                for f in ("J1", "j22", "j21", "Jnu")]
        print("pair", (ci, di, given), "traj", ["%.1e" % e for e in errs], "cost", ["%.1e" % e for e in cerr])
        assert max(errs) < TRAJ_RTOL, (ci, di, given, errs)
        for f in ("J1", "j22", "Jnu"):
            np.testing.assert_allclose(getattr(res, f)[s], J[f], rtol=COST_RTOL, err_msg=str((ci, di, given, f)))
        np.testing.assert_allclose(res.j21[s], J["j21"], rtol=COST_RTOL, atol=1e-12)


def _reduce_np(J1, st, jb):
    """include/mpct.h's robust record in csrc/robust_reduce.h's order, strictly sequential: per output one
    accumulator over the draws k = 0.., J(k) summed over the outputs i = 0.., the worst draw the first
    strict maximum."""
    Cn, D, my = J1.shape
    out = dict(mean=np.full((Cn, my), np.nan), worst=np.full((Cn, my), np.nan), n_failed=np.zeros(Cn, np.int32),
               worst_draw=np.full(Cn, -1, np.int32), status=np.zeros(Cn, np.int32))
    for c in range(Cn):
        acc, mx, n, nf, jw, wd, sor = np.zeros(my), np.zeros(my), 0, 0, 0.0, -1, 0
        for k in range(D):
            sor |= int(st[c, k])
            J = 0.0
            for i in range(my):
                J = J + J1[c, k, i]
            if st[c, k] == 0 and np.isfinite(J) and J <= jb:
                acc = acc + J1[c, k]
                mx = J1[c, k].copy() if n == 0 else np.where(J1[c, k] > mx, J1[c, k], mx)
                if n == 0 or J > jw:
                    jw, wd = J, k
                n += 1
            else:
                nf += 1
        if sor & (8 | 16):
            n, nf, wd = 0, 0, -1
        if n:
            out["mean"][c], out["worst"][c] = acc / float(n), mx
        out["n_failed"][c], out["worst_draw"][c], out["status"][c] = nf, wd, sor
    return out


ROBUST = ("mean", "worst", "n_failed", "worst_draw", "status")


@pytest.mark.gpu
def test_robust_route(gpu):
    """4. eval_robust on vandevusse_mc(D = 5) over twelve grid candidates is eval_batch plus the numpy
    restatement of the rule, bitwise, at the default bound and at one that fails some draws."""
    from mpct.engine import eval_batch, eval_robust, robust_instance
    from mpct.nmpc import nmpc_candidate_grid, vandevusse_mc

    sc, r, _ = vandevusse_mc(5)
    assert robust_instance(sc) == VARIANT + " + robust_reduce_kernel"
    N, Nu, d, lam = nmpc_candidate_grid(12)
    per = eval_batch(sc, N, Nu, d, lam, r)
    a = eval_robust(sc, N, Nu, d, lam, r, want_J1=True)
    np.testing.assert_array_equal(bits(a.J1), bits(per.J1))
    ref = _reduce_np(a.J1.reshape(12, 5, 2), per.status.reshape(12, 5), 1e100)
    for f in ROBUST:
        np.testing.assert_array_equal(bits(getattr(a, f)), bits(ref[f]), err_msg=f)
    assert a.n_failed[0] == 0 and a.status[0] == 0   # the committed tuning survives every default draw
    J = a.J1.reshape(12, 5, 2).sum(axis=2)
    jb = float(np.median(J[np.isfinite(J)]))
    b = eval_robust(sc, N, Nu, d, lam, r, j_bound=jb, want_J1=True)
    refb = _reduce_np(b.J1.reshape(12, 5, 2), per.status.reshape(12, 5), jb)
    for f in ROBUST:
        np.testing.assert_array_equal(bits(getattr(b, f)), bits(refb[f]), err_msg=f)
    assert 0 < b.n_failed.sum() < 60


@pytest.mark.gpu
def test_robust_bounds_draw_fails(gpu):
    """4, last item.  k10 x 1.5 from the model's steady state: on the CPU reference the tuned loop's c_B
    reaches 1.227 against x_max = 1.2.  The draw comes back with status 64 (a result, not an error),
    counts as failed and is never the worst draw."""
    from mpct.engine import eval_batch, eval_robust
    from mpct.nmpc import VDV_TUNED as T

    hot = mr.scaled(mr.MODEL, (1.5, 1.0, 1.0))
    P = np.array([mr.MODEL, hot, mr.scaled(mr.MODEL, *DRAWS[1])])
    sc, x0, r, yref = _scenario(plant_params=P)
    o = mr.closedloop_mismatch(r, T["N"], max(T["Nu"]), np.array(T["delta"]), np.array(T["lam"]), hot, x0, open_loop=False)
    assert not o.bounds_ok and o.x[1].max() > 1.22
    cands = ([T["N"]], [max(T["Nu"])], np.array([T["delta"]]), np.array([T["lam"]]))
    refs = np.stack([r, r, r])
    per = eval_batch(sc, *cands, refs, want_traj=True)
    assert per.status.tolist() == [0, 64, 0]
    assert np.all(np.isfinite(per.J1)) and _trel(per.y[1], o.y) < TRAJ_RTOL   # the loop itself is the reference's
    a = eval_robust(sc, *cands, refs, want_J1=True)
    assert a.n_failed.tolist() == [1] and a.status.tolist() == [64] and a.worst_draw[0] in (0, 2)
    assert per.J1[1].sum() > max(per.J1[0].sum(), per.J1[2].sum())   # it would have been the worst
    ref = _reduce_np(a.J1.reshape(1, 3, 2), per.status.reshape(1, 3), 1e100)
    for f in ROBUST:
        np.testing.assert_array_equal(bits(getattr(a, f)), bits(ref[f]), err_msg=f)
