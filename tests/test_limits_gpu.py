"""GPU: the limit indices (limit_indices.hip; include/mpct.h) against tests/limits_ref.py, bit for
bit on every field.

  * mpct_limit_indices_device on generated trajectories (limits_ref.generated: runs ending at sample 63, starting
    at 64, crossing both, over the whole row, ending at the last sample, two equal runs; samples at lo + sat_tol
    and one ulp either side; ex at out_tol; -0.0 against a zero bound; lo == hi; no bound; a NaN row and +-inf
    samples beside valid rows) at nit 1, 2, 63, 64, 65, 128, 129, 130, 500, t0 0, 1, nit - 1, row counts 1 and 5,
    my = 0 and nu = 0;
  * NULL-pointer subsets between guard words; mpct_limit_indices (host pointers) equal to the device route;
  * eval_limit_indices against the reference applied to the trajectories of eval_batch(want_traj=True) of the
    same batch, with the scenario's own bounds: Shell 3x3 driven to its rate and amplitude bounds, a band
    scenario with candidates inside and outside their bands; chunk independence; a second stream;
  * eval_robust_limit_indices on shell3x3_mc against tests/draw_stats_ref.py applied to the per-simulation
    limit records; its base record against mpct_eval_robust's: bit for bit where both run one kernel (the band
    scenario), within the suite's bound on the two kernels where they do not (Shell 3x3)."""
import ctypes as C

import numpy as np
import pytest

import band_family as bf
import draw_stats_ref as DS
import limits_ref as R
from test_limits import CASES

pytestmark = pytest.mark.gpu
ALL = R.Y_FIELDS + R.U_FIELDS
GUARD = 32
CANARY = {np.dtype(np.float64): 0x7FF85A5A5A5A5A5A, np.dtype(np.int32): 0x5A5A5A5A}


@pytest.fixture(scope="module")
def gpu(built, has_gpu):
    if not has_gpu:
        pytest.skip("no GPU")
    return True


def _dtype(f):
    return np.dtype(np.int32 if f in R.INT_FIELDS else np.float64)


def _bounds(P):
    return {k: P[k] for k in R.BOUNDS if P.get(k) is not None}


def device_call(y, u, P, t0, fields=None, drop=()):
    """mpct_limit_indices_device through engine.limit_indices_device with exactly `fields` requested, each buffer
    between GUARD canary words on both sides; the trajectories named in `drop` are passed as NULL.  Returns
    {field: [S, w]} after checking the guards and that every element was written."""
    import torch
    from mpct.engine import limit_indices_device

    dev = torch.device("cuda", 0)
    S, my, nu = y.shape[0], y.shape[1], u.shape[1]
    if fields is None:
        fields = (R.Y_FIELDS if my else ()) + (R.U_FIELDS if nu else ())
    ty = None if "y" in drop or not my else torch.tensor(y, device=dev)
    tu = None if "u" in drop or not nu else torch.tensor(u, device=dev)
    bufs, out = {}, {}
    for f in fields:
        dt, w = _dtype(f), (my if f in R.Y_FIELDS else nu)
        t = torch.full((S * w + 2 * GUARD,), CANARY[dt], dtype=torch.int32 if dt == np.int32 else torch.int64, device=dev)
        bufs[f] = t
        out[f] = t[GUARD:GUARD + S * w]
    if ty is None or tu is None:      # the shapes the binding cannot read off a missing tensor
        from mpct import _lib
        from mpct.engine import _limit_params, _limit_struct

        p, keep = _limit_params(my, nu, t0, P["out_tol"], P["sat_tol"], _bounds(P))
        o = _limit_struct(out)
        ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None          # noqa: E731
        code = _lib.load().mpct_limit_indices_device(ptr(ty), ptr(tu), S, my, nu, y.shape[2], C.byref(p), C.byref(o),
                                                     C.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
        assert code == 0, _lib.last_error()
    else:
        limit_indices_device(ty, tu, out, t0=t0, out_tol=P["out_tol"], sat_tol=P["sat_tol"], **_bounds(P))
    torch.cuda.synchronize(dev)
    got = {}
    for f, t in bufs.items():
        a = t.cpu().numpy()
        dt, w = _dtype(f), (my if f in R.Y_FIELDS else nu)
        can = a.dtype.type(CANARY[dt])
        assert np.all(a[:GUARD] == can) and np.all(a[GUARD + S * w:] == can), "guard of %s overwritten" % f
        rows = a[GUARD:GUARD + S * w]
        assert not np.any(rows == can), "%s: elements never written" % f
        got[f] = rows.view(dt).reshape(S, w).copy()
    return got


@pytest.mark.parametrize("S,my,nu,nit,t0", CASES)
def test_limit_indices_device_bitwise(gpu, S, my, nu, nit, t0):
    y, u, P = R.generated(S, my, nu, nit, t0)
    want = R.limits_scalar(y, u, P, t0)
    got = device_call(y, u, P, t0)
    fields = tuple(got)
    assert fields == (R.Y_FIELDS if my else ()) + (R.U_FIELDS if nu else ())
    R.assert_bitwise(got, want, fields=fields, what="mpct_limit_indices_device")
    if my:
        assert R.check_order_free(got, y, P, t0) > 0
    if nu and nit - t0 >= R.LONG and S == 5:
        for s, (name, _, run) in R.RUNS.items():
            assert got["sat_run"][s, 0] == run(nit - t0), name
    # a repeated call is bitwise identical, and a record does not depend on the row's place in the batch
    R.assert_bitwise(device_call(y, u, P, t0), got, fields=fields, what="repeat")
    if S > 1:
        back = device_call(y[::-1].copy(), u[::-1].copy(), P, t0)
        R.assert_bitwise({f: a[::-1] for f, a in back.items()}, got, fields=fields, what="reversed batch")


def test_null_pointer_subsets(gpu):
    y, u, P = R.generated(5, 4, 2, 130, 1)
    full = device_call(y, u, P, 1)
    for fields, drop in [(("t_in",), ()), (("viol2",), ()), (("sat_run",), ()), (R.Y_FIELDS, ("u",)), (R.U_FIELDS, ("y",)),
                         (("t_vmax", "du_margin"), ()), (("n_out", "y_margin", "n_rate"), ())]:
        got = device_call(y, u, P, 1, fields=fields, drop=drop)
        assert set(got) == set(fields)
        R.assert_bitwise(got, full, fields=fields, what="subset %s without %s" % (fields, drop))
    # no bound at all: NULL arrays
    none = {"out_tol": 0.0, "sat_tol": 0.0}
    got = device_call(y, u, none, 1)
    R.assert_bitwise(got, R.limits_scalar(y, u, none, 1), what="no bounds")
    ok = np.isfinite(y[:, :, 1:]).all(-1)
    assert (got["viol"][ok] == 0).all() and np.isinf(got["y_margin"][ok]).all() and (got["sat_run"][[0, 3, 4]] == 0).all()


def test_host_entry_equals_device_entry(gpu):
    import torch
    from mpct.engine import limit_indices

    y, u, P = R.generated(5, 4, 2, 130, 1)
    want = device_call(y, u, P, 1)
    before = torch.cuda.current_device()
    res = limit_indices(y, u, t0=1, out_tol=P["out_tol"], sat_tol=P["sat_tol"], device=0, **_bounds(P))
    assert torch.cuda.current_device() == before
    assert res.viol.shape == (5, 1, 4) and res.sat_run.shape == (5, 1, 2) and res.t_in.dtype == np.int32
    R.assert_bitwise({f: getattr(res, f).reshape(5, -1) for f in ALL}, want, what="mpct_limit_indices")
    part = limit_indices(None, u, t0=1, sat_tol=P["sat_tol"], fields=("sat_run", "u_margin"), device=-1,
                         u_lo=P["u_lo"], u_hi=P["u_hi"])
    assert part.viol is None and part.n_lo is None and part.sat_run.shape == (5, 1, 2)
    R.assert_bitwise({f: getattr(part, f).reshape(5, -1) for f in ("sat_run", "u_margin")}, want, fields=("sat_run", "u_margin"))


# ---------------------------------------------------------------------------------------------
# eval_limit_indices: the records of a scored batch against the reference on eval_batch's trajectories, with
# the scenario's own bounds
T0, OUT_TOL, SAT_TOL = 4, 0.0, 1e-9
_scen, _ref = {}, {}


def scen(name):
    """dict(sc, cands of 5 candidates, refs [1, my, nit], v, P: the scenario's own bounds for the reference)"""
    if name not in _scen:
        if name == "shell":
            from mpct.scenarios import SHELL3_R, shell3x3

            # eight times the setpoint of the scenario: the moves ride the rate bound and three candidates hold
            # u_0 at its upper bound for 9 to 13 samples on the oracle's trajectories (oracle.cport, nit = 60)
            sc, r, _ = shell3x3(n2_max=10, nu_max=3, nit=60)
            refs, v = 8.0 * r[None], None
            N2, Nu = np.array([10, 8, 5, 10, 6], np.int32), np.array([3, 2, 1, 1, 3], np.int32)
            d = np.array([[1, 1, 1], [10, 10, 10], [1, 10, 1], [10, 1, 1], [1, 1, 10.0]])
            l = np.array([[1e-4] * 3, [1e-3] * 3, [1e-4, 1e-2, 1e-4], [1e-2, 1e-4, 1e-4], [1e-1] * 3])
            P = dict(u_lo=-1.0 / SHELL3_R, u_hi=0.5 / SHELL3_R, du_lo=-0.05 / SHELL3_R, du_hi=0.05 / SHELL3_R)
        else:
            # so2 of the band family: candidates 0 and 6 keep both outputs inside their bands on the oracle's
            # trajectories (oracle.toolbox_band), candidates 1, 2 and 5 ride or leave them
            case = bf.CASES["so2"]
            sc = bf.product(case)
            r, vv, _ = bf.signals(case)
            refs, v = r[None], vv[None]
            N2, Nu, d, l = bf.arrays(case, [0, 1, 2, 5, 6])
            du, um = np.array(case.du_max), np.array(case.u_max)
            P = dict(y_lo=[b[0] for b in case.y_band], y_hi=[b[1] for b in case.y_band], u_lo=-um, u_hi=um, du_lo=-du, du_hi=du)
        P.update(out_tol=OUT_TOL, sat_tol=SAT_TOL)
        _scen[name] = dict(sc=sc, cands=(N2, Nu, d, l), refs=np.ascontiguousarray(refs), v=v, P=P)
    return _scen[name]


def reference(name):
    """eval_batch with trajectories for the batch, once, and the reference's records of them"""
    from mpct.engine import eval_batch

    if name not in _ref:
        q = scen(name)
        res = eval_batch(q["sc"], *q["cands"], q["refs"], v=q["v"], want_traj=True, device=0)
        want = R.limits_scalar(res.y, res.u, q["P"], T0)
        for a in want.values():
            a.setflags(write=False)
        _ref[name] = (res, want)
    return _ref[name]


def flat(res):
    return {f: getattr(res, f).reshape(-1, getattr(res, f).shape[-1]) for f in ALL}


def run_eval(name, budget=0, **kw):
    from mpct import _lib
    from mpct.engine import eval_limit_indices

    q = scen(name)
    lib = _lib.load()
    assert lib.mpct_internal_index_budget(int(budget)) == 0
    try:
        return eval_limit_indices(q["sc"], *q["cands"], q["refs"], v=q["v"], t0=T0, out_tol=OUT_TOL, sat_tol=SAT_TOL,
                                  device=0, **kw)
    finally:
        lib.mpct_internal_index_budget(0)


@pytest.mark.parametrize("name", ["shell", "band"])
def test_eval_limit_indices_against_reference(gpu, name):
    q = scen(name)
    ev, want = reference(name)
    sc = q["sc"]
    res = run_eval(name, want_costs=True)
    assert res.viol.shape == (5, 1, sc.my) and res.sat_run.shape == (5, 1, sc.nu)
    got = flat(res)
    print("status", ev.status.tolist(), {f: got[f].tolist() for f in ("n_out", "y_margin", "n_rate", "sat_run")})
    R.assert_bitwise(got, want, what=name)
    if name == "shell":      # the records are not all zero: moves at the rate bound, a run at the amplitude bound
        assert (got["n_rate"] > 0).any() and (got["sat_run"] >= 2).any()
        assert (got["viol"] == 0).all() and np.isinf(got["y_margin"]).all()         # no output bound in this scenario
    else:
        assert (got["n_out"] > 0).any() and (got["y_margin"] > 0).any()
        assert (got["n_out"][0] == 0).all() and (got["y_margin"][0] > 0).all() and (got["t_in"][0] == T0).all()
    # the costs of the same launch are eval_batch's
    for f in ("J1", "j22", "status", "qp_iters"):
        assert (DS.bits(getattr(res.batch, f)) == DS.bits(getattr(ev, f))).all(), f
    # the caller's bounds in place of the scenario's: the same values give the same bits, others other records
    same = run_eval(name, **_bounds(q["P"]))
    R.assert_bitwise(flat(same), want, what=name + " with the bounds passed")
    wide = dict(q["P"], u_hi=np.full(sc.nu, 100.0), du_lo=None, du_hi=None)
    other = run_eval(name, u_hi=wide["u_hi"], du_lo=np.full(sc.nu, -np.inf), du_hi=np.full(sc.nu, np.inf))
    R.assert_bitwise(flat(other), R.limits_scalar(ev.y, ev.u, wide, T0), what=name + " with other bounds")
    assert (other.n_rate == 0).all() and (other.n_hi == 0).all()
    # a single field: that one alone, the same bits; a repeated call
    one = run_eval(name, fields=("sat_run",))
    assert one.viol is None and one.n_lo is None and (one.sat_run.reshape(-1, sc.nu) == want["sat_run"]).all()
    R.assert_bitwise(flat(run_eval(name)), want, what=name + " repeated")


@pytest.mark.parametrize("per_chunk", [2, 1])
def test_chunks_of_whole_candidates(gpu, per_chunk):
    q = scen("shell")
    ev, want = reference("shell")
    sc = q["sc"]
    per = (sc.my + sc.nu) * sc.nit * 8
    res = run_eval("shell", budget=per_chunk * per + 8, want_costs=True)     # ragged against 5 candidates
    R.assert_bitwise(flat(res), want, what="%d candidates per chunk" % per_chunk)
    for f in ("J1", "j22", "status", "qp_iters"):
        assert (DS.bits(getattr(res.batch, f)) == DS.bits(getattr(ev, f))).all(), f


def test_eval_limit_indices_device_on_a_stream(gpu):
    import torch
    from mpct.engine import _batch_args, eval_limit_indices_device

    q = scen("shell")
    ev, want = reference("shell")
    sc = q["sc"]
    N2, Nu, d, l, refs, Cn, nref, _ = _batch_args(sc, *q["cands"], q["refs"], None)
    S = Cn * nref
    dev = torch.device("cuda", 0)
    ins = [torch.tensor(a, device=dev) for a in (N2, Nu, d, l, refs)]
    out = {f: torch.full((S, sc.my if f in R.Y_FIELDS else sc.nu), -7, dtype=torch.int32 if f in R.INT_FIELDS else torch.float64,
                         device=dev) for f in ALL}
    out["J1"] = torch.zeros((S, sc.my), dtype=torch.float64, device=dev)
    out["status"] = torch.full((S,), -7, dtype=torch.int32, device=dev)
    torch.cuda.synchronize(dev)
    st = torch.cuda.Stream(dev)
    for _ in range(2):          # back to back on one scenario: the second waits for the scratch of the first
        eval_limit_indices_device(sc, *ins, out, t0=T0, out_tol=OUT_TOL, sat_tol=SAT_TOL, device=0, stream=st)
    st.synchronize()
    R.assert_bitwise({f: out[f].cpu().numpy() for f in ALL}, want, what="device entry on a stream")
    assert (DS.bits(out["J1"].cpu().numpy()) == DS.bits(ev.J1)).all()
    assert (out["status"].cpu().numpy() == ev.status).all()


# ---------------------------------------------------------------------------------------------
# eval_robust_limit_indices: the statistics over the draws against draw_stats_ref on the per-simulation records
LEVELS = [0.9, 1.0, 0.5]
_mc = {}


def mc():
    """shell3x3_mc, 5 candidates (the fourth with a bad horizon) x 3 draws, nit = 60, the reference of `shell`"""
    if not _mc:
        from mpct.engine import eval_limit_indices
        from mpct.scenarios import shell3x3_mc

        sc, refs, _ = shell3x3_mc(draws=3, n2_max=10, nu_max=3, nit=60)
        q = scen("shell")
        N2, Nu, d, l = (a.copy() for a in q["cands"])
        N2[3] = 11                          # above n2_max: MPCT_ST_BADHORIZON on every draw
        kw = dict(t0=T0, out_tol=OUT_TOL, sat_tol=SAT_TOL, device=0)
        refs = 8.0 * refs
        res = eval_limit_indices(sc, N2, Nu, d, l, refs, want_costs=True, **kw)
        rec = {f: getattr(res, f) for f in ALL}
        J1, st = res.batch.J1.reshape(5, 3, -1), res.batch.status.reshape(5, 3)
        for a in list(rec.values()) + [J1, st]:
            a.setflags(write=False)
        _mc.update(sc=sc, cands=(N2, Nu, d, l), refs=refs, kw=kw, rec=rec, J1=J1, st=st)
    return _mc


def run_robust(fields, levels, j_bound=0.0, budget=0):
    from mpct import _lib
    from mpct.engine import eval_robust_limit_indices

    q = mc()
    lib = _lib.load()
    assert lib.mpct_internal_index_budget(int(budget)) == 0
    try:
        return eval_robust_limit_indices(q["sc"], *q["cands"], q["refs"], fields=fields, levels=levels, j_bound=j_bound, **q["kw"])
    finally:
        lib.mpct_internal_index_budget(0)


def assert_robust(res, fields, levels, j_bound, msg):
    q = mc()
    want, wbase = DS.robust_indices_ref(q["rec"], q["J1"], q["st"], j_bound, fields, levels)
    use = DS.FIELDS if len(levels) else DS.BASE
    DS.assert_same_stats({f: getattr(res, f) for f in use}, want, fields=use, msg=msg)
    for f in ("mean", "worst", "n_failed", "worst_draw", "status"):
        assert (DS.bits(getattr(res.base, f)) == DS.bits(wbase[f])).all(), (f, msg)
    return want


def test_eval_robust_limit_indices_against_composition(gpu):
    from mpct.engine import eval_robust

    q = mc()
    sc = q["sc"]
    alive = DS.alive_ref(q["J1"], q["st"], 0.0).sum(axis=1)
    print("status", q["st"].tolist(), "alive", alive.tolist(), "sat_run", q["rec"]["sat_run"].tolist())
    assert q["st"][3].tolist() == [16] * 3 and alive[3] == 0 and alive.max() >= 2
    # the draws differ and the records are not all zero
    assert (q["rec"]["n_rate"] > 0).any() and (q["rec"]["sat_run"] >= 2).any()
    assert (q["rec"]["u_margin"][0, 0] != q["rec"]["u_margin"][0, 1]).any()
    res = run_robust(ALL, LEVELS)
    W = 7 * sc.my + 6 * sc.nu
    assert res.hi.shape == (5, W) and res.cvar.shape == (5, W, 3) and len(res.columns) == W
    want = assert_robust(res, ALL, LEVELS, 0.0, "all fields")
    col = {c: k for k, c in enumerate(res.columns)}
    # an infinite margin is a draw without a value: the scenario has no output bound
    assert (res.n[:, col[("y_margin", 0)]] == 0).all() and np.isnan(res.hi[:, col[("y_margin", 0)]]).all()
    assert (res.n[:, col[("sat_run", 0)]] == alive).all() and (res.n[3] == 0).all()
    full = alive == 3
    assert (res.hi[full, col[("sat_run", 0)]] == q["rec"]["sat_run"][full, :, 0].max(axis=1)).all()
    # base against mpct_eval_robust's record of the same batch.  Both calls end in the same robust_reduce_kernel; bit
    # for bit base is that reduction of this launch's own per-simulation J1 (assert_robust above).  The closed loops
    # are not the same kernel on this scenario: the cost-only batch of mpct_eval_robust runs gpc_small_kernel, the
    # trajectory batch of this entry gpc_closed_loop_kernel<16,false,true> (pinned below).  tests/test_gpu_parity.py
    # holds each of the two to the C port within COST_RTOL, so their J1 agree within 2 * COST_RTOL and so do the
    # means and maxima over the draws.  Counts and statuses are exact (every simulated draw has status 0 on both),
    # the worst draw is the same where the two largest totals lie further apart than that bound.  Measured on an
    # MI355X: mean 4.0e-11, worst 1.2e-10.  The same comparison where both calls run one kernel is bitwise:
    # test_robust_base_is_eval_robusts_record_bitwise_on_one_kernel
    from mpct.engine import kernel_instance
    from test_gpu_parity import COST_RTOL

    assert kernel_instance(sc) == "gpc_small_kernel"
    assert kernel_instance(sc, want_traj=True) == "gpc_closed_loop_kernel<16,false,true>"
    rob = eval_robust(sc, *q["cands"], q["refs"], device=0)
    for f in ("n_failed", "status"):
        assert (getattr(res.base, f) == getattr(rob, f)).all(), f
    tot = np.sort(q["J1"].sum(axis=2), axis=1)
    apart = (tot[:, -1] - tot[:, -2]) > 2 * COST_RTOL * tot[:, -1]
    assert apart[[0, 1, 2, 4]].all() and (res.base.worst_draw[apart] == rob.worst_draw[apart]).all()
    for f in ("mean", "worst"):
        got, ref = getattr(res.base, f), getattr(rob, f)
        print(f, "max rel difference to mpct_eval_robust", np.nanmax(np.abs(got - ref) / np.abs(ref)))
        assert (np.isnan(got) == np.isnan(ref)).all()
        np.testing.assert_allclose(got, ref, rtol=2 * COST_RTOL, atol=0, err_msg=f)
    # a subset in a non-struct order, without levels; a bound that fails draws; a repeated call
    sub = ("sat_run", "viol", "n_rate", "du_margin")
    part = run_robust(sub, None)
    assert part.quantile is None and part.columns[0] == ("sat_run", 0) and part.columns[sc.nu] == ("viol", 0)
    assert_robust(part, sub, [], 0.0, "subset")
    c = int(np.argmax(alive))
    J = np.sort(q["J1"][c].sum(axis=1)[DS.alive_ref(q["J1"], q["st"], 0.0)[c] != 0])
    bound = float(0.5 * (J[-2] + J[-1]))
    assert J[-2] < bound < J[-1]
    cut = run_robust(sub, LEVELS, j_bound=bound)
    assert_robust(cut, sub, LEVELS, bound, "with j_bound")
    assert cut.base.n_failed[c] == res.base.n_failed[c] + 1 and cut.n[c, 0] == alive[c] - 1
    assert_robust(run_robust(ALL, LEVELS), ALL, LEVELS, 0.0, "repeated")
    tab = res.costs("hi", names=("sat_run", "n_rate"), max_failed=3)
    assert tab.shape == (5, 2 * sc.nu) and np.isnan(tab[3]).all() and np.isfinite(tab[c]).all()
    assert want["hi"].shape == (5, W)


@pytest.mark.parametrize("per_chunk", [2, 1])
def test_robust_chunks_of_whole_candidates(gpu, per_chunk):
    sc = mc()["sc"]
    per = 3 * (sc.my + sc.nu) * sc.nit * 8
    sub = ("t_in", "sat_run", "u_margin", "n_rate")
    res = run_robust(sub, LEVELS, budget=per_chunk * per + 8)
    assert_robust(res, sub, LEVELS, 0.0, "%d candidates per chunk" % per_chunk)


def test_eval_robust_limit_indices_device_on_a_stream(gpu):
    import torch
    from mpct.engine import _batch_args, eval_robust_limit_indices_device

    q = mc()
    sc = q["sc"]
    sub = ("sat_run", "u_margin")
    want, wbase = DS.robust_indices_ref(q["rec"], q["J1"], q["st"], 0.0, sub, LEVELS)
    N2, Nu, d, l, refs, Cn, D, _ = _batch_args(sc, *q["cands"], q["refs"], None)
    dev = torch.device("cuda", 0)
    ins = [torch.tensor(a, device=dev) for a in (N2, Nu, d, l, refs)]
    W = 2 * sc.nu
    out = {f: torch.full((Cn, W, 3) if f in DS.LEVEL else (Cn, W), -7, dtype=torch.int32 if f in DS.INT_FIELDS else torch.float64,
                         device=dev) for f in DS.FIELDS}
    base = {"mean": torch.zeros((Cn, sc.my), dtype=torch.float64, device=dev),
            "n_failed": torch.full((Cn,), -7, dtype=torch.int32, device=dev)}
    torch.cuda.synchronize(dev)
    st = torch.cuda.Stream(dev)
    for _ in range(2):
        eval_robust_limit_indices_device(sc, *ins, out, base=base, fields=sub, levels=LEVELS, stream=st, **q["kw"])
    st.synchronize()
    DS.assert_same_stats({f: out[f].cpu().numpy() for f in DS.FIELDS}, want, msg="device entry on a stream")
    assert (DS.bits(base["mean"].cpu().numpy()) == DS.bits(wbase["mean"])).all()
    assert (base["n_failed"].cpu().numpy() == wbase["n_failed"]).all()


def test_robust_base_is_eval_robusts_record_bitwise_on_one_kernel(gpu):
    """The band kernel is one instance for cost-only and trajectory batches (want_traj is a run-time flag that only
    gates its stores), so mpct_eval_robust and mpct_eval_robust_limit_indices run the same closed loops and the same
    robust_reduce_kernel: base equals mpct_eval_robust's record bit for bit, every field."""
    from mpct.engine import eval_robust, eval_robust_limit_indices, kernel_instance

    q = scen("band")
    sc = q["sc"]
    assert "mdband_closed_loop_kernel" in kernel_instance(sc) and kernel_instance(sc) == kernel_instance(sc, want_traj=True)
    scale = np.array([1.0, 0.5, 1.5])[:, None, None]
    refs, v = np.ascontiguousarray(scale * q["refs"]), np.ascontiguousarray(scale * q["v"])     # three draws
    res = eval_robust_limit_indices(sc, *q["cands"], refs, v=v, fields=("n_out", "vmax", "sat_run"), t0=T0, out_tol=OUT_TOL,
                                    sat_tol=SAT_TOL, device=0)
    rob = eval_robust(sc, *q["cands"], refs, v=v, device=0)
    print("n_failed", rob.n_failed.tolist(), "worst_draw", rob.worst_draw.tolist(), "n_out hi", res.hi[:, :sc.my].tolist())
    for f in ("mean", "worst", "n_failed", "worst_draw", "status"):
        assert (DS.bits(getattr(res.base, f)) == DS.bits(getattr(rob, f))).all(), f
    assert (rob.n_failed < 3).any() and np.isfinite(rob.mean[rob.n_failed < 3]).all()    # not a comparison of NaNs alone
