"""GPU: the step-response indices per setpoint segment (segment_indices.hip; include/mpct.h)
against tests/segments_ref.py, bit for bit on every field.

  * mpct_segment_indices_device on generated trajectories (segments_ref.generated: ties of the peak, samples
    exactly on the band edge and on the rise levels, inverse responses, a step that never reaches rise_hi,
    sigma = 0, -0.0) at the boundary lists of tests/test_segments.py (segment lengths 1, 2, 63, 64, 65, 130, starts
    0, 1, 63, 64, 65, nseg 1, 2, 16, tseg[0] > 0 and tseg[nseg] < nit), S of 1 and 5, nref 1 and 3, my = 0 and
    nu = 0, both base rules; NaN outside the covered range does not matter, NaN and +-inf inside one segment
    spoil that unit only;
  * NULL-pointer subsets between guard words; mpct_segment_indices (host pointers) equal to the device route;
  * nseg = 1, base = 0 equal to mpct_indices_device bit for bit;
  * eval_segment_indices against the reference applied to the trajectories of eval_batch(want_traj=True) of the
    same batch: a short Shell 3x3, a band scenario with an extra event, the NMPC scenario; chunk independence; a
    second stream;
  * eval_robust_segment_indices against tests/draw_stats_ref.py applied to the per-simulation records; its base
    against mpct_eval_robust's record: bit for bit where both run one kernel (the band scenario), within the
    suite's bound on the two kernels where they do not (Shell 3x3: the rule of tests/test_limits_gpu.py)."""
import ctypes as C

import numpy as np
import pytest

import band_family as bf
import draw_stats_ref as DS
import indices_ref as IR
import segments_ref as R
from test_segments import CASES, PAR

pytestmark = pytest.mark.gpu
GUARD = 32
CANARY = {np.dtype(np.float64): 0x7FF85A5A5A5A5A5A, np.dtype(np.int32): 0x5A5A5A5A}


@pytest.fixture(scope="module")
def gpu(built, has_gpu):
    if not has_gpu:
        pytest.skip("no GPU")
    return True


def _dtype(f):
    return np.dtype(np.int32 if f in R.INT_FIELDS else np.float64)


def device_call(y, u, r, tseg, base=1, fields=None, drop=(), par=PAR):
    """mpct_segment_indices_device with exactly `fields` requested, each buffer between GUARD canary words on both
    sides; the trajectories named in `drop` are passed as NULL.  Returns {field: [S, w, nseg]} after checking the
    guards and that every element was written."""
    import torch
    from mpct import _lib
    from mpct.engine import _segment_params, _segment_struct

    dev = torch.device("cuda", 0)
    S, my, nu, nref, nseg = y.shape[0], y.shape[1], u.shape[1], r.shape[0], len(tseg) - 1
    if fields is None:
        fields = (R.Y_FIELDS if my else ()) + (R.U_FIELDS if nu else ())
    ty = None if "y" in drop or not my else torch.tensor(y, device=dev)
    tr = None if "y" in drop or not my else torch.tensor(r, device=dev)
    tu = None if "u" in drop or not nu else torch.tensor(u, device=dev)
    bufs, out = {}, {}
    for f in fields:
        dt, n = _dtype(f), S * (my if f in R.Y_FIELDS else nu) * nseg
        t = torch.full((n + 2 * GUARD,), CANARY[dt], dtype=torch.int32 if dt == np.int32 else torch.int64, device=dev)
        bufs[f] = t
        out[f] = t[GUARD:GUARD + n]
    p, keep = _segment_params(tseg, base, par["band_rel"], par["band_abs"], par["rise_lo"], par["rise_hi"])
    o = _segment_struct(out)
    ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None          # noqa: E731
    code = _lib.load().mpct_segment_indices_device(ptr(ty), ptr(tu), ptr(tr), S, nref, my, nu, y.shape[2], C.byref(p),
                                                   C.byref(o), C.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
    assert code == 0, _lib.last_error()
    torch.cuda.synchronize(dev)
    del keep
    got = {}
    for f, t in bufs.items():
        a = t.cpu().numpy()
        dt, w = _dtype(f), (my if f in R.Y_FIELDS else nu)
        can = a.dtype.type(CANARY[dt])
        assert np.all(a[:GUARD] == can) and np.all(a[GUARD + S * w * nseg:] == can), "guard of %s overwritten" % f
        rows = a[GUARD:GUARD + S * w * nseg]
        assert not np.any(rows == can), "%s: elements never written" % f
        got[f] = rows.view(dt).reshape(S, w, nseg).copy()
    return got


def spoiled(y, u, r, tseg, nit):
    """copies with non-finite samples: NaN everywhere outside [tseg[0], tseg[nseg]) (must not matter), and inside
    the covered range a NaN, a +inf and a -inf in the middle segment of single rows (that unit only)"""
    y, u, r = y.copy(), u.copy(), r.copy()
    a0, b0 = tseg[0], tseg[-1]
    for x in (y, u, r):
        x[..., :a0] = np.nan
        x[..., b0:] = np.nan
    g = (len(tseg) - 1) // 2
    t = (tseg[g] + tseg[g + 1]) // 2
    S = y.shape[0]
    if y.shape[1]:
        y[S - 1, 0, t] = np.nan
        if S > 1:
            y[1, y.shape[1] - 1, tseg[g + 1] - 1] = np.inf
    if u.shape[1]:
        u[S - 1, 0, t] = -np.inf
    return y, u, r


@pytest.mark.parametrize("name,nit,tseg,shape", CASES, ids=["%s S%d nref%d my%d nu%d" % ((c[0],) + c[3]) for c in CASES])
def test_segment_indices_device_bitwise(gpu, name, nit, tseg, shape):
    S, nref, my, nu = shape
    y, u, r = R.generated(S, nref, my, nu, nit, tseg)
    nseg = len(tseg) - 1
    for base in (0, 1):
        want = R.segments_scalar(y, u, r, tseg, base=base, **PAR)
        got = device_call(y, u, r, tseg, base)
        fields = tuple(got)
        assert fields == (R.Y_FIELDS if my else ()) + (R.U_FIELDS if nu else ())
        R.assert_bitwise(got, want, fields=fields, what="%s base %d" % (name, base))
    # base = 1 from here on.  Non-finite samples: outside the covered range they are never read; inside they spoil
    # their own unit and leave the neighbours as they were
    ys, us, rs = spoiled(y, u, r, tseg, nit)
    want_s = R.segments_scalar(ys, us, rs, tseg, base=1, **PAR)
    got_s = device_call(ys, us, rs, tseg, 1)
    R.assert_bitwise(got_s, want_s, fields=fields, what=name + " with non-finite samples")
    g = nseg // 2
    for f in fields:
        w = np.asarray(want_s[f])
        bad = (w == -1) if f in R.INT_FIELDS and f != "rise" else np.isnan(w) if f not in R.INT_FIELDS else np.zeros(w.shape, bool)
        assert not bad[..., :g].any(), (f, "a segment before the spoiled one is invalid")
        if f not in ("rise",):
            assert bad[S - 1, 0, g], (f, "the spoiled unit is valid")
    other = [f for f in fields]
    keep = np.ones((S, 1, nseg), dtype=bool)
    keep[:, :, g:g + 2] = False              # the spoiled segment and the one whose u(a-1) / r(a-1) it holds
    for f in other:
        assert (IR.bits(np.asarray(got_s[f]))[np.broadcast_to(keep, got_s[f].shape)] ==
                IR.bits(np.asarray(got[f]))[np.broadcast_to(keep, got[f].shape)]).all(), (f, "a neighbour moved")
    # a repeated call is bitwise identical, and a record does not depend on the row's place in the batch
    R.assert_bitwise(device_call(y, u, r, tseg, 1), got, fields=fields, what="repeat")
    if S > 1 and nref == 1:
        back = device_call(y[::-1].copy(), u[::-1].copy(), r, tseg, 1)
        R.assert_bitwise({f: a[::-1] for f, a in back.items()}, got, fields=fields, what="reversed batch")


def test_null_pointer_subsets(gpu):
    name, nit, tseg, _ = CASES[12]
    y, u, r = R.generated(5, 1, 3, 2, nit, tseg)
    full = device_call(y, u, r, tseg)
    for fields, drop in [(("rise",), ()), (("under",), ()), (("tv",), ()), (R.Y_FIELDS, ("u",)), (R.U_FIELDS, ("y",)),
                         (("t_emax", "u_hi"), ()), (("settle", "ise", "dumax"), ())]:
        got = device_call(y, u, r, tseg, fields=fields, drop=drop)
        assert set(got) == set(fields)
        R.assert_bitwise(got, full, fields=fields, what="subset %s without %s" % (fields, drop))


def test_host_entry_equals_device_entry(gpu):
    import torch
    from mpct.engine import segment_indices

    name, nit, tseg, _ = CASES[12]
    y, u, r = R.generated(6, 3, 3, 2, nit, tseg)
    want = device_call(y, u, r, tseg)
    nseg = len(tseg) - 1
    before = torch.cuda.current_device()
    res = segment_indices(y, u, r, tseg, device=0, **PAR)
    assert torch.cuda.current_device() == before
    assert res.iae.shape == (2, 3, 3, nseg) and res.tv.shape == (2, 3, 2, nseg) and res.rise.dtype == np.int32
    R.assert_bitwise({f: getattr(res, f).reshape(6, -1, nseg) for f in R.FIELDS}, want, what="mpct_segment_indices")
    part = segment_indices(None, u, None, tseg, fields=("tv", "u_lo"), device=-1)
    assert part.iae is None and part.du2 is None and part.tv.shape == (6, 1, 2, nseg)
    R.assert_bitwise({f: getattr(part, f).reshape(6, -1, nseg) for f in ("tv", "u_lo")}, want, fields=("tv", "u_lo"))


@pytest.mark.parametrize("nit", [1, 65, 130])
def test_one_segment_equals_the_index_kernel(gpu, nit):
    """the consequence the header states: nseg = 1, base = 0, tseg = {t0, nit} against mpct_indices_device"""
    import torch
    from mpct.engine import indices_device

    dev = torch.device("cuda", 0)
    y, u, r = IR.generated(5, 1, 3, 2, nit)[:3]
    par = dict(band_rel=0.02, band_abs=0.01, rise_lo=0.1, rise_hi=0.9)
    for t0 in sorted({0, 1, nit - 1} & set(range(nit))):
        out = {f: torch.zeros((5, 3 if f in IR.Y_FIELDS else 2), dtype=torch.int32 if f in IR.INT_FIELDS else torch.float64,
                              device=dev) for f in IR.Y_FIELDS + IR.U_FIELDS}
        indices_device(torch.tensor(y, device=dev), torch.tensor(u, device=dev), torch.tensor(r, device=dev), out, t0=t0,
                       band_rel=0.02, band_abs=0.01)
        torch.cuda.synchronize(dev)
        seg = device_call(y, u, r, [t0, nit], base=0, par=par)
        IR.assert_bitwise({f: seg[f][..., 0] for f in out}, {f: t.cpu().numpy() for f, t in out.items()},
                          what="nit %d t0 %d" % (nit, t0))


# ---------------------------------------------------------------------------------------------
# eval_segment_indices: the records of a scored batch against the reference on eval_batch's trajectories
_scen, _ref = {}, {}
EPAR = dict(base=1, band_rel=0.05, band_abs=1e-3, rise_lo=0.1, rise_hi=0.9)


def scen(name):
    """dict(sc, cands, refs [1, my, nit], v, tseg)"""
    if name not in _scen:
        from mpct.engine import reference_segments

        if name == "shell":
            from mpct.scenarios import shell3x3

            # the scenario's own setpoints, compressed: changes at 9, 29, 59 and 89, back to 0
            sc, r, _ = shell3x3(n2_max=10, nu_max=3, nit=120)
            refs = np.zeros((1, 3, 120))
            for a, lv in ((9, r[:, 20]), (29, -r[:, 20]), (59, 0.5 * r[:, 20]), (89, 0.0 * r[:, 20])):
                refs[0, :, a:] = lv[:, None]
            v = None
            N2, Nu = np.array([10, 8, 5, 10, 6], np.int32), np.array([3, 2, 1, 1, 3], np.int32)
            d = np.array([[1, 1, 1], [10, 10, 10], [1, 10, 1], [10, 1, 1], [1, 1, 10.0]])
            l = np.array([[1e-4] * 3, [1e-3] * 3, [1e-4, 1e-2, 1e-4], [1e-2, 1e-4, 1e-4], [1e-1] * 3])
            tseg = reference_segments(refs)
            assert tseg.tolist() == [0, 9, 29, 59, 89, 120]
        elif name == "band":
            case = bf.CASES["so2"]
            sc = bf.product(case)
            r, vv, _ = bf.signals(case)
            refs, v = r[None], vv[None]
            N2, Nu, d, l = bf.arrays(case, [0, 1, 2, 5, 6])
            # the measured disturbance's first move is an event the reference does not show
            ev = int(np.nonzero(np.any(vv[:, 1:] != vv[:, :-1], axis=0))[0][0]) + 1
            tseg = reference_segments(refs, extra=(ev,))
            assert ev in tseg.tolist()
        else:
            import record_calls as rc

            # the Van de Vusse batch of tests/test_indices_gpu.py
            n = rc.scenario("nmpc")
            sc, refs, v = n["sc"], n["refs"], None
            N2, Nu, d, l = rc.take(n["pool"], np.array([2, 15]))
            tseg = reference_segments(refs)
        _scen[name] = dict(sc=sc, cands=(N2, Nu, d, l), refs=np.ascontiguousarray(refs), v=v, tseg=tseg)
    return _scen[name]


def reference(name):
    """eval_batch with trajectories for the batch, once, and the reference's records of them"""
    from mpct.engine import eval_batch

    if name not in _ref:
        q = scen(name)
        res = eval_batch(q["sc"], *q["cands"], q["refs"], v=q["v"], want_traj=True, device=0)
        want = R.segments_np(res.y, res.u, q["refs"], q["tseg"], **EPAR)
        for a in want.values():
            a.setflags(write=False)
        _ref[name] = (res, want)
    return _ref[name]


def flat(res):
    return {f: getattr(res, f).reshape((-1,) + getattr(res, f).shape[2:]) for f in R.FIELDS}


def run_eval(name, budget=0, **kw):
    from mpct import _lib
    from mpct.engine import eval_segment_indices

    q = scen(name)
    lib = _lib.load()
    assert lib.mpct_internal_index_budget(int(budget)) == 0
    try:
        return eval_segment_indices(q["sc"], *q["cands"], q["refs"], v=q["v"], tseg=q["tseg"], device=0, **EPAR, **kw)
    finally:
        lib.mpct_internal_index_budget(0)


@pytest.mark.parametrize("name", ["shell", "band", "nmpc"])
def test_eval_segment_indices_against_reference(gpu, name):
    q = scen(name)
    ev, want = reference(name)
    sc = q["sc"]
    nseg = len(q["tseg"]) - 1
    Cn = q["cands"][0].size
    res = run_eval(name, want_costs=True)
    assert res.iae.shape == (Cn, 1, sc.my, nseg) and res.tv.shape == (Cn, 1, sc.nu, nseg) and res.tseg.tolist() == q["tseg"].tolist()
    got = flat(res)
    print("tseg", q["tseg"].tolist(), "status", ev.status.tolist(), {f: got[f][0].tolist() for f in ("over", "settle", "rise", "under")})
    R.assert_bitwise(got, want, what=name)
    ok = ev.status == 0
    assert ok.any() and np.isfinite(got["iae"][ok]).all()
    if name == "shell":      # what the whole-run indices cannot see: every later segment is a step of its own
        assert (got["rise"][ok][:, :, 1:] >= 0).all()
    for f in ("J1", "j22", "status", "qp_iters"):
        assert (DS.bits(getattr(res.batch, f)) == DS.bits(getattr(ev, f))).all(), f
    # the default boundaries are the reference's; a single field; a repeated call
    if name == "shell":
        from mpct.engine import eval_segment_indices

        auto = eval_segment_indices(sc, *q["cands"], q["refs"], device=0, **EPAR)
        R.assert_bitwise(flat(auto), want, what="default tseg")
    one = run_eval(name, fields=("rise",))
    assert one.iae is None and one.tv is None and (one.rise.reshape(want["rise"].shape) == want["rise"]).all()
    R.assert_bitwise(flat(run_eval(name)), want, what=name + " repeated")
    tab = res.costs(("over", "tv", "itae"))
    assert tab.shape == (Cn, 3) and np.isfinite(tab[ok]).all()


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


def test_eval_segment_indices_device_on_a_stream(gpu):
    import torch
    from mpct.engine import _batch_args, eval_segment_indices_device

    q = scen("shell")
    ev, want = reference("shell")
    sc = q["sc"]
    nseg = len(q["tseg"]) - 1
    N2, Nu, d, l, refs, Cn, nref, _ = _batch_args(sc, *q["cands"], q["refs"], None)
    S = Cn * nref
    dev = torch.device("cuda", 0)
    ins = [torch.tensor(a, device=dev) for a in (N2, Nu, d, l, refs)]
    out = {f: torch.full((S, sc.my if f in R.Y_FIELDS else sc.nu, nseg), -7,
                         dtype=torch.int32 if f in R.INT_FIELDS else torch.float64, device=dev) for f in R.FIELDS}
    out["J1"] = torch.zeros((S, sc.my), dtype=torch.float64, device=dev)
    out["status"] = torch.full((S,), -7, dtype=torch.int32, device=dev)
    torch.cuda.synchronize(dev)
    st = torch.cuda.Stream(dev)
    for _ in range(2):          # back to back on one scenario: the second waits for the scratch of the first
        eval_segment_indices_device(sc, *ins, out, q["tseg"], device=0, stream=st, **EPAR)
    st.synchronize()
    R.assert_bitwise({f: out[f].cpu().numpy() for f in R.FIELDS}, want, what="device entry on a stream")
    assert (DS.bits(out["J1"].cpu().numpy()) == DS.bits(ev.J1)).all()
    assert (out["status"].cpu().numpy() == ev.status).all()


# ---------------------------------------------------------------------------------------------
# eval_robust_segment_indices: the statistics over the draws against draw_stats_ref on the per-simulation records
LEVELS = [0.9, 1.0, 0.5]
_mc = {}


def mc():
    """shell3x3_mc, 5 candidates (the fourth with a bad horizon) x 3 draws, nit = 120, the references of `shell`"""
    if not _mc:
        from mpct.engine import eval_segment_indices
        from mpct.scenarios import shell3x3_mc

        sc, refs, _ = shell3x3_mc(draws=3, n2_max=10, nu_max=3, nit=120)
        q = scen("shell")
        N2, Nu, d, l = (a.copy() for a in q["cands"])
        N2[3] = 11                          # above n2_max: MPCT_ST_BADHORIZON on every draw
        refs = np.ascontiguousarray(np.broadcast_to(q["refs"], refs.shape))
        kw = dict(tseg=q["tseg"], device=0, **EPAR)
        res = eval_segment_indices(sc, N2, Nu, d, l, refs, want_costs=True, **kw)
        # [C, D, w, nseg] -> the [C, D, w * nseg] tables the statistics see
        rec = {f: getattr(res, f).reshape(5, 3, -1) for f in R.FIELDS}
        J1, st = res.batch.J1.reshape(5, 3, -1), res.batch.status.reshape(5, 3)
        for a in list(rec.values()) + [J1, st]:
            a.setflags(write=False)
        _mc.update(sc=sc, cands=(N2, Nu, d, l), refs=refs, kw=kw, rec=rec, J1=J1, st=st, nseg=len(q["tseg"]) - 1)
    return _mc


def run_robust(fields, levels, j_bound=0.0, budget=0):
    from mpct import _lib
    from mpct.engine import eval_robust_segment_indices

    q = mc()
    lib = _lib.load()
    assert lib.mpct_internal_index_budget(int(budget)) == 0
    try:
        return eval_robust_segment_indices(q["sc"], *q["cands"], q["refs"], fields=fields, levels=levels, j_bound=j_bound, **q["kw"])
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


def test_eval_robust_segment_indices_against_composition(gpu):
    from mpct.engine import eval_robust, kernel_instance
    from test_gpu_parity import COST_RTOL

    q = mc()
    sc, nseg = q["sc"], q["nseg"]
    alive = DS.alive_ref(q["J1"], q["st"], 0.0).sum(axis=1)
    print("status", q["st"].tolist(), "alive", alive.tolist(), "rise", q["rec"]["rise"][0].tolist())
    assert q["st"][3].tolist() == [16] * 3 and alive[3] == 0 and alive.max() >= 2
    assert (q["rec"]["over"][0, 0] != q["rec"]["over"][0, 1]).any(), "the draws do not differ"
    res = run_robust(R.FIELDS, LEVELS)
    W = (10 * sc.my + 5 * sc.nu) * nseg
    assert res.hi.shape == (5, W) and res.cvar.shape == (5, W, 3) and len(res.columns) == W
    assert res.columns[0] == ("iae", 0, 0) and res.columns[nseg] == ("iae", 1, 0) and res.columns[-1] == ("u_hi", sc.nu - 1, nseg - 1)
    assert_robust(res, R.FIELDS, LEVELS, 0.0, "all fields")
    col = {c: k for k, c in enumerate(res.columns)}
    # a rise of -1 beside a valid unit (no step) is a draw without a value: MPCT_STAT_I32's rule
    rise = q["rec"]["rise"].reshape(5, 3, sc.my, nseg)
    st = q["rec"]["settle"].reshape(5, 3, sc.my, nseg)
    c = int(np.argmax(alive))
    for i in range(sc.my):
        for g in range(nseg):
            live = DS.alive_ref(q["J1"], q["st"], 0.0)[c] != 0
            assert res.n[c, col[("rise", i, g)]] == int(((rise[c, :, i, g] >= 0) & live).sum())
            assert res.n[c, col[("settle", i, g)]] == int(((st[c, :, i, g] >= 0) & live).sum())
    assert (res.n[3] == 0).all()
    # base against mpct_eval_robust's record of the same batch: the rule of tests/test_limits_gpu.py, for the same
    # reason.  Both calls end in robust_reduce_kernel and base is bit for bit that reduction of this launch's own
    # J1 (assert_robust above); the closed loops are two kernels on this scenario (pinned below), each held to the C
    # port within COST_RTOL by tests/test_gpu_parity.py, so J1, and with it the mean and the maximum over the draws,
    # agree within 2 * COST_RTOL; counts and statuses are exact
    assert kernel_instance(sc) == "gpc_small_kernel"
    assert kernel_instance(sc, want_traj=True) == "gpc_closed_loop_kernel<16,false,true>"
    rob = eval_robust(sc, *q["cands"], q["refs"], device=0)
    for f in ("n_failed", "status"):
        assert (getattr(res.base, f) == getattr(rob, f)).all(), f
    for f in ("mean", "worst"):
        got, ref = getattr(res.base, f), getattr(rob, f)
        print(f, "max rel difference to mpct_eval_robust", np.nanmax(np.abs(got - ref) / np.abs(ref)))
        assert (np.isnan(got) == np.isnan(ref)).all()
        np.testing.assert_allclose(got, ref, rtol=2 * COST_RTOL, atol=0, err_msg=f)
    # a subset in a non-struct order, without levels; a bound that fails draws; costs
    sub = ("rise", "over", "tv", "settle")
    part = run_robust(sub, None)
    assert part.quantile is None and part.columns[0] == ("rise", 0, 0) and part.columns[sc.my * nseg] == ("over", 0, 0)
    assert_robust(part, sub, [], 0.0, "subset")
    J = np.sort(q["J1"][c].sum(axis=1)[DS.alive_ref(q["J1"], q["st"], 0.0)[c] != 0])
    bound = float(0.5 * (J[-2] + J[-1]))
    assert J[-2] < bound < J[-1]
    cut = run_robust(sub, LEVELS, j_bound=bound)
    assert_robust(cut, sub, LEVELS, bound, "with j_bound")
    assert cut.base.n_failed[c] == res.base.n_failed[c] + 1
    tab = res.costs("hi", names=("over", "tv"), segments=(1, 2), max_failed=3)
    assert tab.shape == (5, 2 * (sc.my + sc.nu)) and np.isnan(tab[3]).all() and np.isfinite(tab[c]).all()


@pytest.mark.parametrize("per_chunk", [2, 1])
def test_robust_chunks_of_whole_candidates(gpu, per_chunk):
    sc = mc()["sc"]
    per = 3 * (sc.my + sc.nu) * sc.nit * 8
    sub = ("rise", "under", "u_lo", "settle")
    res = run_robust(sub, LEVELS, budget=per_chunk * per + 8)
    assert_robust(res, sub, LEVELS, 0.0, "%d candidates per chunk" % per_chunk)


def test_eval_robust_segment_indices_device_on_a_stream(gpu):
    import torch
    from mpct.engine import _batch_args, eval_robust_segment_indices_device

    q = mc()
    sc, nseg = q["sc"], q["nseg"]
    sub = ("rise", "tv")
    want, wbase = DS.robust_indices_ref(q["rec"], q["J1"], q["st"], 0.0, sub, LEVELS)
    N2, Nu, d, l, refs, Cn, D, _ = _batch_args(sc, *q["cands"], q["refs"], None)
    dev = torch.device("cuda", 0)
    ins = [torch.tensor(a, device=dev) for a in (N2, Nu, d, l, refs)]
    W = (sc.my + sc.nu) * nseg
    out = {f: torch.full((Cn, W, 3) if f in DS.LEVEL else (Cn, W), -7, dtype=torch.int32 if f in DS.INT_FIELDS else torch.float64,
                         device=dev) for f in DS.FIELDS}
    base = {"mean": torch.zeros((Cn, sc.my), dtype=torch.float64, device=dev),
            "n_failed": torch.full((Cn,), -7, dtype=torch.int32, device=dev)}
    torch.cuda.synchronize(dev)
    st = torch.cuda.Stream(dev)
    kw = {k: v for k, v in q["kw"].items() if k != "tseg"}
    for _ in range(2):
        eval_robust_segment_indices_device(sc, *ins, out, q["kw"]["tseg"], base_out=base, fields=sub, levels=LEVELS, stream=st, **kw)
    st.synchronize()
    DS.assert_same_stats({f: out[f].cpu().numpy() for f in DS.FIELDS}, want, msg="device entry on a stream")
    assert (DS.bits(base["mean"].cpu().numpy()) == DS.bits(wbase["mean"])).all()
    assert (base["n_failed"].cpu().numpy() == wbase["n_failed"]).all()


def test_robust_base_is_eval_robusts_record_bitwise_on_one_kernel(gpu):
    """The band kernel is one instance for cost-only and trajectory batches, so mpct_eval_robust and
    mpct_eval_robust_segment_indices run the same closed loops and the same robust_reduce_kernel: base equals
    mpct_eval_robust's record bit for bit, every field."""
    from mpct.engine import eval_robust, eval_robust_segment_indices, kernel_instance

    q = scen("band")
    sc = q["sc"]
    assert "mdband_closed_loop_kernel" in kernel_instance(sc) and kernel_instance(sc) == kernel_instance(sc, want_traj=True)
    scale = np.array([1.0, 0.5, 1.5])[:, None, None]
    refs, v = np.ascontiguousarray(scale * q["refs"]), np.ascontiguousarray(scale * q["v"])     # three draws
    res = eval_robust_segment_indices(sc, *q["cands"], refs, v=v, tseg=q["tseg"], fields=("over", "rise", "tv"), device=0, **EPAR)
    rob = eval_robust(sc, *q["cands"], refs, v=v, device=0)
    print("n_failed", rob.n_failed.tolist(), "worst_draw", rob.worst_draw.tolist())
    for f in ("mean", "worst", "n_failed", "worst_draw", "status"):
        assert (DS.bits(getattr(res.base, f)) == DS.bits(getattr(rob, f))).all(), f
    assert (rob.n_failed < 3).any() and np.isfinite(rob.mean[rob.n_failed < 3]).all()    # not a comparison of NaNs alone
