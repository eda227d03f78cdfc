"""GPU: the oscillation indices per setpoint segment (osc_indices.hip; include/mpct.h) against
tests/osc_ref.py, bit for bit on every field.

  * mpct_osc_indices_device on generated trajectories (osc_ref.generated: damped, undamped and growing
    sinusoids, equal peaks, samples exactly on the band edges, moves exactly on the dead zone, sigma = 0, -0.0) at
    the boundary lists of tests/test_osc.py (segment lengths 1, 2, 63, 64, 65, 130, starts 0, 1, 63, 64, 65, nseg
    1, 2, 16, tseg[0] > 0 and tseg[nseg] < nit), S of 1 and 5, nref 1 and 3, my = 0 and nu = 0, both base rules;
    NaN outside the covered range does not matter, NaN and +-inf inside one segment spoil that unit only;
  * the hand-placed rows of osc_ref.edge_rows: a crossing between lane 63 and lane 0 of the next block, an
    inside-band gap longer than 64 samples between two outside samples of opposite sign (the carry through empty
    blocks), the peak of lobe k0 + 2 tied across two blocks, ncross exactly k0 + 1 and k0 + 2; rev_tol = 0 with
    moves of +-0.0;
  * NULL-pointer subsets between guard words; mpct_osc_indices (host pointers) equal to the device route;
  * eval_osc_indices against the reference applied to the trajectories of eval_batch(want_traj=True) of the same
    batch (the batches of tests/test_segments_gpu.py): a short Shell 3x3, a band scenario, the NMPC scenario;
    chunk independence; a second stream;
  * eval_robust_osc_indices against tests/draw_stats_ref.py applied to the per-simulation records; its base
    against mpct_eval_robust's record bit for bit where both run one kernel (the band scenario)."""
import ctypes as C

import numpy as np
import pytest

import draw_stats_ref as DS
import indices_ref as IR
import osc_ref as R
import test_segments_gpu as SG
from test_osc import CASES, PAR

pytestmark = pytest.mark.gpu
GUARD, CANARY = SG.GUARD, SG.CANARY


@pytest.fixture(scope="module")
def gpu(built, has_gpu):
    if not has_gpu:
        pytest.skip("no GPU")
    return True


def _dtype(f):
    return np.dtype(np.int32 if f in R.INT_FIELDS else np.float64)


def device_call(y, u, r, tseg, base=1, fields=None, drop=(), par=PAR):
    """mpct_osc_indices_device with exactly `fields` requested, each buffer between GUARD canary words on both
    sides; the trajectories named in `drop` are passed as NULL.  Returns {field: [S, w, nseg]} after checking the
    guards and that every element was written."""
    import torch
    from mpct import _lib
    from mpct.engine import _osc_params, _osc_struct

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
    p, keep = _osc_params(tseg, base, par["band_rel"], par["band_abs"], par["rev_tol"])
    o = _osc_struct(out)
    ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None          # noqa: E731
    code = _lib.load().mpct_osc_indices_device(ptr(ty), ptr(tu), ptr(tr), S, nref, my, nu, y.shape[2], C.byref(p),
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


@pytest.mark.parametrize("name,nit,tseg,shape", CASES, ids=["%s S%d nref%d my%d nu%d" % ((c[0],) + c[3]) for c in CASES])
def test_osc_indices_device_bitwise(gpu, name, nit, tseg, shape):
    S, nref, my, nu = shape
    y, u, r = R.generated(S, nref, my, nu, nit, tseg)
    nseg = len(tseg) - 1
    for base in (0, 1):
        want = R.osc_scalar(y, u, r, tseg, base=base, **PAR)
        got = device_call(y, u, r, tseg, base)
        fields = tuple(got)
        assert fields == (R.Y_FIELDS if my else ()) + (R.U_FIELDS if nu else ())
        R.assert_bitwise(got, want, fields=fields, what="%s base %d" % (name, base))
    # base = 1 from here on.  Non-finite samples: outside the covered range they are never read; inside they spoil
    # their own unit and leave the neighbours as they were
    ys, us, rs = SG.spoiled(y, u, r, tseg, nit)
    want_s = R.osc_scalar(ys, us, rs, tseg, base=1, **PAR)
    got_s = device_call(ys, us, rs, tseg, 1)
    R.assert_bitwise(got_s, want_s, fields=fields, what=name + " with non-finite samples")
    g = nseg // 2
    for f in fields:
        w = np.asarray(want_s[f])
        if f in ("period", "t_rev"):
            continue                         # -1 is a value of theirs
        bad = (w == -1) if f in R.INT_FIELDS else np.isnan(w)
        assert not bad[..., :g].any(), (f, "a segment before the spoiled one is invalid")
        assert bad[S - 1, 0, g], (f, "the spoiled unit is valid")
    keep = np.ones((S, 1, nseg), dtype=bool)
    keep[:, :, g:g + 2] = False              # the spoiled segment and the one whose u(a-1) it holds
    for f in fields:
        assert (IR.bits(np.asarray(got_s[f]))[np.broadcast_to(keep, got_s[f].shape)] ==
                IR.bits(np.asarray(got[f]))[np.broadcast_to(keep, got[f].shape)]).all(), (f, "a neighbour moved")
    # a repeated call is bitwise identical, and a record does not depend on the row's place in the batch
    R.assert_bitwise(device_call(y, u, r, tseg, 1), got, fields=fields, what="repeat")
    if S > 1 and nref == 1:
        back = device_call(y[::-1].copy(), u[::-1].copy(), r, tseg, 1)
        R.assert_bitwise({f: a[::-1] for f, a in back.items()}, got, fields=fields, what="reversed batch")


def test_order_dependent_paths_on_hand_placed_rows(gpu):
    y, u, r, tseg = R.edge_rows()
    want = R.osc_scalar(y, u, r, tseg, base=1, **PAR)
    got = device_call(y, u, r, tseg, 1)
    print({f: got[f][0, :, 0].tolist() for f in R.FIELDS})
    R.assert_bitwise(got, want, what="edge rows")
    a = tseg[0]
    row = {n: k for k, n in enumerate(R.EDGE_ROWS)}
    k = row["crossing between lane 63 and lane 0"]
    assert got["ncross"][0, k, 0] == 2 and got["t_rev"][0, k, 0] == a + 64
    k = row["inside gap longer than 64 samples"]
    assert got["ncross"][0, k, 0] == 2 and got["a_last"][0, k, 0] == 0.25 and got["t_rev"][0, k, 0] == a + 3 * 64 + 2
    k = row["peak of lobe k0+2 tied across two blocks"]
    assert got["period"][0, k, 0] == (a + 64 + 60) - (a + 3) and got["decay"][0, k, 0] == 0.5
    k = row["ncross exactly k0+1"]
    assert (got["ncross"][0, k, 0], got["decay"][0, k, 0], got["period"][0, k, 0]) == (2, 0.0, -1)
    k = row["ncross exactly k0+2"]
    assert (got["ncross"][0, k, 0], got["decay"][0, k, 0], got["period"][0, k, 0]) == (3, 0.375, 137)
    k = row["never leaves the band"]
    assert (got["ncross"][0, k, 0], got["a_last"][0, k, 0], got["nmove"][0, k, 0]) == (0, 0.0, 0)
    # the same rows in several segments of other alignment, both base rules, and shifted by one sample
    for ts in ([1, 70, 140, 326], [0, 63, 64, 65, 195, 330], [2, 130, 131, 329]):
        for base in (0, 1):
            R.assert_bitwise(device_call(y, u, r, ts, base), R.osc_scalar(y, u, r, ts, base=base, **PAR), what=str(ts))
    # rev_tol = 0 and a band of 0: moves of +-0.0 are no moves, samples of +-0.0 are inside
    z = np.where(np.arange(130) % 2 == 0, -0.0, 0.0)[None, None] * np.ones((2, 2, 1))
    z[1, 1, 5], z[1, 1, 70] = 1.0, -1.0
    par = dict(band_rel=0.0, band_abs=0.0, rev_tol=0.0)
    got = device_call(z, z, np.zeros((1, 2, 130)), [0, 66, 130], 1, par=par)
    R.assert_bitwise(got, R.osc_scalar(z, z, np.zeros((1, 2, 130)), [0, 66, 130], base=1, **par), what="zeros")
    assert (got["nmove"][0] == 0).all() and (got["ncross"][0] == 0).all() and got["nmove"][1, 1].tolist() == [2, 2]


def test_null_pointer_subsets(gpu):
    name, nit, tseg, _ = CASES[12]
    y, u, r = R.generated(5, 1, 3, 2, nit, tseg)
    full = device_call(y, u, r, tseg)
    for fields, drop in [(("ncross",), ()), (("decay",), ()), (("t_rev",), ()), (R.Y_FIELDS, ("u",)), (R.U_FIELDS, ("y",)),
                         (("period", "nrev"), ()), (("a_last", "ncross", "nmove"), ())]:
        got = device_call(y, u, r, tseg, fields=fields, drop=drop)
        assert set(got) == set(fields)
        R.assert_bitwise(got, full, fields=fields, what="subset %s without %s" % (fields, drop))


def test_host_entry_equals_device_entry(gpu):
    import torch
    from mpct.engine import osc_indices

    name, nit, tseg, _ = CASES[12]
    y, u, r = R.generated(6, 3, 3, 2, nit, tseg)
    want = device_call(y, u, r, tseg)
    nseg = len(tseg) - 1
    before = torch.cuda.current_device()
    res = osc_indices(y, u, r, tseg, device=0, **PAR)
    assert torch.cuda.current_device() == before
    assert res.decay.shape == (2, 3, 3, nseg) and res.nrev.shape == (2, 3, 2, nseg) and res.ncross.dtype == np.int32
    R.assert_bitwise({f: getattr(res, f).reshape(6, -1, nseg) for f in R.FIELDS}, want, what="mpct_osc_indices")
    part = osc_indices(None, u, None, tseg, fields=("nrev", "t_rev"), rev_tol=R.TOL, device=-1)
    assert part.decay is None and part.nmove is None and part.nrev.shape == (6, 1, 2, nseg)
    R.assert_bitwise({f: getattr(part, f).reshape(6, -1, nseg) for f in ("nrev", "t_rev")}, want, fields=("nrev", "t_rev"))


# ---------------------------------------------------------------------------------------------
# eval_osc_indices: the records of a scored batch against the reference on eval_batch's trajectories (the batches
# and the trajectories of tests/test_segments_gpu.py, computed once for both files)
_ref = {}
EPAR = dict(base=1, band_rel=0.05, band_abs=1e-3, rev_tol=1e-4)


def reference(name):
    if name not in _ref:
        q = SG.scen(name)
        res, _ = SG.reference(name)
        want = R.osc_np(res.y, res.u, q["refs"], q["tseg"], **EPAR)
        for a in want.values():
            a.setflags(write=False)
        _ref[name] = (res, want)
    return _ref[name]


def flat(res):
    return {f: getattr(res, f).reshape((-1,) + getattr(res, f).shape[2:]) for f in R.FIELDS}


def run_eval(name, budget=0, **kw):
    from mpct import _lib
    from mpct.engine import eval_osc_indices

    q = SG.scen(name)
    lib = _lib.load()
    assert lib.mpct_internal_index_budget(int(budget)) == 0
    try:
        return eval_osc_indices(q["sc"], *q["cands"], q["refs"], v=q["v"], tseg=q["tseg"], device=0, **EPAR, **kw)
    finally:
        lib.mpct_internal_index_budget(0)


@pytest.mark.parametrize("name", ["shell", "band", "nmpc"])
def test_eval_osc_indices_against_reference(gpu, name):
    q = SG.scen(name)
    ev, want = reference(name)
    sc = q["sc"]
    nseg = len(q["tseg"]) - 1
    Cn = q["cands"][0].size
    res = run_eval(name, want_costs=True)
    assert res.decay.shape == (Cn, 1, sc.my, nseg) and res.nrev.shape == (Cn, 1, sc.nu, nseg) and res.tseg.tolist() == q["tseg"].tolist()
    got = flat(res)
    print("tseg", q["tseg"].tolist(), "status", ev.status.tolist(), {f: got[f][0].tolist() for f in R.FIELDS})
    R.assert_bitwise(got, want, what=name)
    # the vectorised reference against the sample-by-sample one on these trajectories
    R.assert_bitwise(R.osc_scalar(ev.y[:2], ev.u[:2], q["refs"], q["tseg"], **EPAR), {f: a[:2] for f, a in want.items()})
    ok = ev.status == 0
    assert ok.any() and (got["ncross"][ok] >= 0).all() and np.isfinite(got["decay"][ok]).all()
    for f in ("J1", "j22", "status", "qp_iters"):
        assert (DS.bits(getattr(res.batch, f)) == DS.bits(getattr(ev, f))).all(), f
    if name == "shell":
        from mpct.engine import eval_osc_indices

        auto = eval_osc_indices(sc, *q["cands"], q["refs"], device=0, **EPAR)
        R.assert_bitwise(flat(auto), want, what="default tseg")
    one = run_eval(name, fields=("nrev",))
    assert one.decay is None and one.nmove is None and (one.nrev.reshape(want["nrev"].shape) == want["nrev"]).all()
    R.assert_bitwise(flat(run_eval(name)), want, what=name + " repeated")
    tab = res.costs(("ncross", "decay", "nrev"))
    assert tab.shape == (Cn, 3) and np.isfinite(tab[ok]).all()


@pytest.mark.parametrize("per_chunk", [2, 1])
def test_chunks_of_whole_candidates(gpu, per_chunk):
    q = SG.scen("shell")
    ev, want = reference("shell")
    sc = q["sc"]
    per = (sc.my + sc.nu) * sc.nit * 8
    res = run_eval("shell", budget=per_chunk * per + 8, want_costs=True)     # ragged against 5 candidates
    R.assert_bitwise(flat(res), want, what="%d candidates per chunk" % per_chunk)
    for f in ("J1", "j22", "status", "qp_iters"):
        assert (DS.bits(getattr(res.batch, f)) == DS.bits(getattr(ev, f))).all(), f


def test_eval_osc_indices_device_on_a_stream(gpu):
    import torch
    from mpct.engine import _batch_args, eval_osc_indices_device

    q = SG.scen("shell")
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
        eval_osc_indices_device(sc, *ins, out, q["tseg"], device=0, stream=st, **EPAR)
    st.synchronize()
    R.assert_bitwise({f: out[f].cpu().numpy() for f in R.FIELDS}, want, what="device entry on a stream")
    assert (DS.bits(out["J1"].cpu().numpy()) == DS.bits(ev.J1)).all()
    assert (out["status"].cpu().numpy() == ev.status).all()


# ---------------------------------------------------------------------------------------------
# eval_robust_osc_indices: the statistics over the draws against draw_stats_ref on the per-simulation records
LEVELS = [0.9, 1.0, 0.5]
_mc = {}


def mc():
    """shell3x3_mc, 5 candidates (the fourth with a bad horizon) x 3 draws, nit = 120, the references of `shell`"""
    if not _mc:
        from mpct.engine import eval_osc_indices
        from mpct.scenarios import shell3x3_mc

        sc, refs, _ = shell3x3_mc(draws=3, n2_max=10, nu_max=3, nit=120)
        q = SG.scen("shell")
        N2, Nu, d, l = (a.copy() for a in q["cands"])
        N2[3] = 11                          # above n2_max: MPCT_ST_BADHORIZON on every draw
        refs = np.ascontiguousarray(np.broadcast_to(q["refs"], refs.shape))
        kw = dict(tseg=q["tseg"], device=0, **EPAR)
        res = eval_osc_indices(sc, N2, Nu, d, l, refs, want_costs=True, **kw)
        # [C, D, w, nseg] -> the [C, D, w * nseg] tables the statistics see
        rec = {f: getattr(res, f).reshape(5, 3, -1) for f in R.FIELDS}
        J1, st = res.batch.J1.reshape(5, 3, -1), res.batch.status.reshape(5, 3)
        for a in list(rec.values()) + [J1, st]:
            a.setflags(write=False)
        _mc.update(sc=sc, cands=(N2, Nu, d, l), refs=refs, kw=kw, rec=rec, J1=J1, st=st, nseg=len(q["tseg"]) - 1)
    return _mc


def run_robust(fields, levels, j_bound=0.0, budget=0):
    from mpct import _lib
    from mpct.engine import eval_robust_osc_indices

    q = mc()
    lib = _lib.load()
    assert lib.mpct_internal_index_budget(int(budget)) == 0
    try:
        return eval_robust_osc_indices(q["sc"], *q["cands"], q["refs"], fields=fields, levels=levels, j_bound=j_bound, **q["kw"])
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


def test_eval_robust_osc_indices_against_composition(gpu):
    q = mc()
    sc, nseg = q["sc"], q["nseg"]
    live = DS.alive_ref(q["J1"], q["st"], 0.0)
    alive = live.sum(axis=1)
    print("status", q["st"].tolist(), "alive", alive.tolist(), "ncross", q["rec"]["ncross"][0].tolist())
    assert q["st"][3].tolist() == [16] * 3 and alive[3] == 0 and alive.max() >= 2
    res = run_robust(R.FIELDS, LEVELS)
    W = (4 * sc.my + 3 * sc.nu) * nseg
    assert res.hi.shape == (5, W) and res.cvar.shape == (5, W, 3) and len(res.columns) == W
    assert res.columns[0] == ("ncross", 0, 0) and res.columns[nseg] == ("ncross", 1, 0) and res.columns[-1] == ("t_rev", sc.nu - 1, nseg - 1)
    assert_robust(res, R.FIELDS, LEVELS, 0.0, "all fields")
    col = {c: k for k, c in enumerate(res.columns)}
    # a period or a t_rev of -1 beside a valid unit is a draw without a value: MPCT_STAT_I32's rule
    c = int(np.argmax(alive))
    per = q["rec"]["period"].reshape(5, 3, sc.my, nseg)
    trv = q["rec"]["t_rev"].reshape(5, 3, sc.nu, nseg)
    for g in range(nseg):
        for i in range(sc.my):
            assert res.n[c, col[("period", i, g)]] == int(((per[c, :, i, g] >= 0) & (live[c] != 0)).sum())
            assert res.n[c, col[("ncross", i, g)]] == alive[c]
        for j in range(sc.nu):
            assert res.n[c, col[("t_rev", j, g)]] == int(((trv[c, :, j, g] >= 0) & (live[c] != 0)).sum())
    assert (res.n[3] == 0).all()
    # a subset in a non-struct order, without levels; a bound that fails draws; costs
    sub = ("nrev", "decay", "ncross", "period")
    part = run_robust(sub, None)
    assert part.quantile is None and part.columns[0] == ("nrev", 0, 0) and part.columns[sc.nu * nseg] == ("decay", 0, 0)
    assert_robust(part, sub, [], 0.0, "subset")
    J = np.sort(q["J1"][c].sum(axis=1)[live[c] != 0])
    bound = float(0.5 * (J[-2] + J[-1]))
    assert J[-2] < bound < J[-1]
    cut = run_robust(sub, LEVELS, j_bound=bound)
    assert_robust(cut, sub, LEVELS, bound, "with j_bound")
    assert cut.base.n_failed[c] == res.base.n_failed[c] + 1
    tab = res.costs("hi", names=("decay", "ncross"), segments=(1, 2), max_failed=3)
    assert tab.shape == (5, 2 * 2 * sc.my) and np.isnan(tab[3]).all() and np.isfinite(tab[c]).all()


@pytest.mark.parametrize("per_chunk", [2, 1])
def test_robust_chunks_of_whole_candidates(gpu, per_chunk):
    sc = mc()["sc"]
    per = 3 * (sc.my + sc.nu) * sc.nit * 8
    sub = ("a_last", "t_rev", "ncross")
    res = run_robust(sub, LEVELS, budget=per_chunk * per + 8)
    assert_robust(res, sub, LEVELS, 0.0, "%d candidates per chunk" % per_chunk)


def test_eval_robust_osc_indices_device_on_a_stream(gpu):
    import torch
    from mpct.engine import _batch_args, eval_robust_osc_indices_device

    q = mc()
    sc, nseg = q["sc"], q["nseg"]
    sub = ("decay", "nrev")
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
        eval_robust_osc_indices_device(sc, *ins, out, q["kw"]["tseg"], base_out=base, fields=sub, levels=LEVELS, stream=st, **kw)
    st.synchronize()
    DS.assert_same_stats({f: out[f].cpu().numpy() for f in DS.FIELDS}, want, msg="device entry on a stream")
    assert (DS.bits(base["mean"].cpu().numpy()) == DS.bits(wbase["mean"])).all()
    assert (base["n_failed"].cpu().numpy() == wbase["n_failed"]).all()


def test_robust_base_is_eval_robusts_record_bitwise_on_one_kernel(gpu):
    """The band kernel is one instance for cost-only and trajectory batches, so mpct_eval_robust and
    mpct_eval_robust_osc_indices run the same closed loops and the same robust_reduce_kernel: base equals
    mpct_eval_robust's record bit for bit, every field."""
    from mpct.engine import eval_robust, eval_robust_osc_indices, kernel_instance

    q = SG.scen("band")
    sc = q["sc"]
    assert "mdband_closed_loop_kernel" in kernel_instance(sc) and kernel_instance(sc) == kernel_instance(sc, want_traj=True)
    scale = np.array([1.0, 0.5, 1.5])[:, None, None]
    refs, v = np.ascontiguousarray(scale * q["refs"]), np.ascontiguousarray(scale * q["v"])     # three draws
    res = eval_robust_osc_indices(sc, *q["cands"], refs, v=v, tseg=q["tseg"], fields=("decay", "ncross", "nrev"), device=0, **EPAR)
    rob = eval_robust(sc, *q["cands"], refs, v=v, device=0)
    print("n_failed", rob.n_failed.tolist(), "worst_draw", rob.worst_draw.tolist())
    for f in ("mean", "worst", "n_failed", "worst_draw", "status"):
        assert (DS.bits(getattr(res.base, f)) == DS.bits(getattr(rob, f))).all(), f
    assert (rob.n_failed < 3).any() and np.isfinite(rob.mean[rob.n_failed < 3]).all()    # not a comparison of NaNs alone
