"""GPU: the trajectory envelopes (envelope.hip; include/mpct.h) against tests/envelope_ref.py, bit
for bit on all nine fields and on the spread, NaN payloads included.

  * mpct_envelope_device on stored trajectories made of draw_stats_ref.table reshaped (NaN, +-inf, zeros of both
    signs in ties, dead draws, a dead candidate, an all-dead sample) at (my, nit) = (1, 1), (1, 63), (1, 65),
    (3, 37) -- columns cross a row boundary inside a wave -- and (2, 130); D = 1, 2, 3, 5, 8, 33 and D_lane,
    D_lane + 1 (the lane kernel's last draw count and draw_stats_kernel's first); no levels, {1.0}, and
    {0.05, 0.5, 0.5, 0.95}; C = 1, 3, and 7 with a grid of two workgroups so that they stride; the other side NULL;
  * both kernels on one shape through the dlane hook, against each other and against engine.draw_stats of the
    reshaped table; the tile widths 256, 128, 64 and 32;
  * the spread at t0 = 0 and t0 = nit - 1, a maximum tied across two 64-sample blocks in one lane and one tied
    across lanes with the later sample in the lower lane, a row with one all-dead sample;
  * eval_robust_envelope on shell3x3_mc and woodberry_toolbox_mc (5 candidates x 8 draws, nit = 80, one bad-horizon
    candidate) against the reference applied to eval_batch(want_traj=True) with alive_ref; base against eval_robust;
    chunks of 2 and 1 candidates; two calls on two streams."""
import numpy as np
import pytest

import draw_stats_ref as R
import envelope_ref as E

pytestmark = pytest.mark.gpu
GUARD = 32
CANARY = {np.dtype(np.float64): 0x7FF85A5A5A5A5A5A, np.dtype(np.int32): 0x5A5A5A5A}
L1, L4 = [1.0], [0.05, 0.5, 0.5, 0.95]


@pytest.fixture(scope="module")
def gpu(built, has_gpu):
    if not has_gpu:
        pytest.skip("no GPU")
    return True


def _dtype(f):
    return np.dtype(np.int32 if f in R.INT_FIELDS or f == "t_spread_max" else np.float64)


class Hooks:
    """the grid and dlane hooks, reset on exit"""
    def __init__(self, grid=0, dlane=0):
        self.grid, self.dlane = grid, dlane

    def __enter__(self):
        from mpct import _lib

        self.lib = _lib.load()
        assert self.lib.mpct_internal_envelope_grid(int(self.grid)) == 0
        assert self.lib.mpct_internal_envelope_dlane(int(self.dlane)) == 0

    def __exit__(self, *exc):
        self.lib.mpct_internal_envelope_grid(0)
        self.lib.mpct_internal_envelope_dlane(0)


def device_call(y, u, alive, levels, t0=0, fields=None, spread=True, grid=0, dlane=0, stream=None):
    """mpct_envelope_device through engine.envelope_device with `fields` (default: all the levels allow) of every
    side given, each buffer between GUARD canary words on both sides.  Returns {'y': (records, spread), 'u': ..}
    after checking the guards and that every element was written."""
    import torch
    from mpct.engine import envelope_device

    dev = torch.device("cuda", 0)
    nlev = len(levels)
    fields = fields if fields is not None else (R.FIELDS if nlev else R.BASE)
    t = {k: (torch.tensor(a, device=dev) if a is not None else None) for k, a in (("y", y), ("u", u), ("alive", alive))}
    bufs, out = {}, {}
    for side, a in (("y", y), ("u", u)):
        if a is None:
            continue
        Cn, _, rows, nit = a.shape
        out[side], out["spread_" + side] = {}, {}
        for f in tuple(fields) + (E.SPREAD if spread else ()):
            dt = _dtype(f)
            shape = (Cn, rows) if f in E.SPREAD else ((Cn, rows, nit, nlev) if f in R.LEVEL else (Cn, rows, nit))
            n = int(np.prod(shape))
            b = torch.full((n + 2 * GUARD,), CANARY[dt], dtype=torch.int32 if dt == np.int32 else torch.int64, device=dev)
            bufs[(side, f)] = (b, n, shape)
            out["spread_" + side if f in E.SPREAD else side][f] = b[GUARD:GUARD + n]
    torch.cuda.synchronize(dev)
    with Hooks(grid, dlane):
        if stream is None:
            envelope_device(t["y"], t["u"], out, t["alive"], levels if nlev else None, t0)
        else:
            with torch.cuda.stream(stream):
                envelope_device(t["y"], t["u"], out, t["alive"], levels if nlev else None, t0)
    (stream or torch.cuda.current_stream(dev)).synchronize()
    got = {}
    for (side, f), (b, n, shape) in bufs.items():
        a = b.cpu().numpy()
        dt = _dtype(f)
        can = a.dtype.type(CANARY[dt])
        assert np.all(a[:GUARD] == can) and np.all(a[GUARD + n:] == can), "guard of %s.%s overwritten" % (side, f)
        vals = a[GUARD:GUARD + n]
        assert not np.any(vals == can), "%s.%s: elements never written" % (side, f)
        got.setdefault(side, ({}, {}))[1 if f in E.SPREAD else 0][f] = vals.view(dt).reshape(shape).copy()
    return got


def traj(Cn, D, rows, nit, seed):
    x, alive = R.table(Cn, D, rows * nit, seed)
    return x.reshape(Cn, D, rows, nit), alive


def check(got, want, wsp, fields, msg, rows=slice(None)):
    R.assert_same_stats(got[0], {f: want[f][rows] for f in fields}, fields=fields, msg=msg)
    E.assert_same_spread(got[1], {f: wsp[f][rows] for f in E.SPREAD}, msg=msg)


def _dlane():
    from mpct import _lib

    return _lib.ENVELOPE_DLANE


@pytest.mark.parametrize("my,nit", [(1, 1), (1, 63), (1, 65), (3, 37), (2, 130)])
@pytest.mark.parametrize("D", [1, 2, 3, 5, 8, 33, "dlane", "dlane+1"])
def test_envelope_device_bitwise(gpu, D, my, nit):
    D = {"dlane": _dlane(), "dlane+1": _dlane() + 1}.get(D, D)
    y, alive = traj(7, D, my, nit, 1000 * D + 10 * my + nit)
    for t0 in (0, nit - 1):
        want4, wsp = E.envelope_ref(y, alive, L4, t0=t0)
        want1, _ = E.envelope_ref(y, alive, L1, t0=t0) if t0 == 0 else (None, None)
        for Cn, grid in ((1, 0), (3, 0), (7, 2)):
            ys, al = np.ascontiguousarray(y[:Cn]), np.ascontiguousarray(alive[:Cn])
            msg = "C=%d D=%d my=%d nit=%d t0=%d" % (Cn, D, my, nit, t0)
            got = device_call(ys, None, al, L4, t0, grid=grid)
            assert set(got) == {"y"}
            check(got["y"], want4, wsp, R.FIELDS, msg + " four levels", slice(0, Cn))
            if t0 == 0:
                check(device_call(ys, None, al, [], t0, grid=grid)["y"], want4, wsp, R.BASE, msg + " no levels", slice(0, Cn))
                g1 = device_call(ys, None, al, L1, t0, grid=grid)["y"]
                check(g1, want1, wsp, R.FIELDS, msg + " level 1.0", slice(0, Cn))
                assert (R.bits(g1[0]["quantile"][..., 0]) == R.bits(g1[0]["hi"])).all()
                assert (g1[0]["q_draw"][..., 0] == g1[0]["hi_draw"]).all()
    # alive NULL; the same table as the u side with y NULL
    want, wsp = E.envelope_ref(y, None, L4, t0=0)
    check(device_call(y, None, None, L4)["y"], want, wsp, R.FIELDS, "alive NULL")
    got = device_call(None, y, None, L4)
    assert set(got) == {"u"}
    check(got["u"], want, wsp, R.FIELDS, "y NULL")


def test_both_sides_and_pointer_subsets(gpu):
    y, alive = traj(3, 8, 3, 37, 21)
    u, _ = traj(3, 8, 2, 37, 22)
    wy, sy = E.envelope_ref(y, alive, L4, t0=5)
    wu, su = E.envelope_ref(u, alive, L4, t0=5)
    got = device_call(y, u, alive, L4, 5)
    check(got["y"], wy, sy, R.FIELDS, "y of both")
    check(got["u"], wu, su, R.FIELDS, "u of both")
    for fields in [("n",), ("mean",), ("lo_draw", "hi"), ("cvar",), ("q_draw", "n"), ("quantile", "lo", "hi_draw")]:
        part = device_call(y, u, alive, L4, 5, fields=fields, spread=False)
        for side, w in (("y", wy), ("u", wu)):
            assert set(part[side][0]) == set(fields) and not part[side][1]
            R.assert_same_stats(part[side][0], w, fields=fields, msg="subset %s" % (fields,))
    part = device_call(y, u, alive, [], 5, fields=("lo", "hi"))
    check(part["u"], wu, su, ("lo", "hi"), "lo, hi and the spread alone")


@pytest.mark.parametrize("D", [5, 28, 29, 56, 57, 113, 114, 150, 227])
def test_both_kernels_on_one_shape(gpu, D):
    """The tile is 256 columns up to D = 14, 128 up to 28, 64 up to 56, 32 above (kEnvLdsBytes = 32 KiB at 9 B per
    draw and column; 113 is the last D whose 32 columns fit it).  dlane = 227, the hook's limit and with 65,376 B
    the largest tile, sends every D here to the lane kernel,
    dlane = 1 to draw_stats_kernel; the yardstick is engine.draw_stats of the reshaped table, which is the
    contract's own kernel and older than this one."""
    from mpct import _lib
    from mpct.engine import draw_stats

    rng = np.random.default_rng(D)
    Cn, rows, nit = 2, 3, 70
    y = rng.integers(0, 12, (Cn, D, rows, nit)).astype(np.float64) / 4.0 - 1.0        # many ties, zeros
    y[rng.random(y.shape) < 0.05] = np.nan
    y[y == 0.0] *= rng.choice([1.0, -1.0], size=int((y == 0.0).sum()))                # zeros of both signs
    y[1, :, 2, 7] = np.inf                                                            # an all-dead sample
    alive = (rng.random((Cn, D)) > 0.1).astype(np.int32)
    st = draw_stats(y.reshape(Cn, D, rows * nit), alive, L4, device=0)
    want = {f: getattr(st, f).reshape((Cn, rows, nit, 4) if f in R.LEVEL else (Cn, rows, nit)) for f in R.FIELDS}
    wsp = E.spread_ref(want["lo"], want["hi"], 3)
    lane = device_call(y, None, alive, L4, 3, dlane=_lib.ENVELOPE_LANE_MAX_DRAWS)["y"]
    prim = device_call(y, None, alive, L4, 3, dlane=1)["y"]
    check(lane, want, wsp, R.FIELDS, "lane kernel, D = %d" % D)
    check(prim, want, wsp, R.FIELDS, "draw_stats_kernel, D = %d" % D)
    R.assert_same_stats(lane[0], prim[0], msg="lane against primitive")
    assert np.isnan(wsp["spread"][1, 2]) and wsp["t_spread_max"][1, 2] == -1 and np.isfinite(wsp["spread"][0]).all()
    if D == 5:
        ref, _ = E.envelope_ref(y, alive, L4, t0=3)
        R.assert_same_stats(want, ref, msg="the yardstick against the Python reference")


def test_spread_tie_across_blocks_and_host_entry(gpu):
    import torch
    from mpct.engine import envelope

    t0 = 3
    lo, hi = E.spread_rows(200, t0)
    y = np.ascontiguousarray(np.stack([lo, hi])[None])                               # C = 1, D = 2, rows = 3, nit = 200
    want, wsp = E.envelope_ref(y, None, [], t0=t0)
    assert wsp["t_spread_max"][0].tolist() == [t0, 10, 20]       # rows 1 and 2: a tie within a lane and across lanes
    got = device_call(y, None, None, [], t0)["y"]
    check(got, want, wsp, R.BASE, "designed rows")
    for t in (0, 11, 199):
        _, w = E.envelope_ref(y, None, [], t0=t)
        E.assert_same_spread(device_call(y, None, None, [], t)["y"][1], w, msg="t0 = %d" % t)
    # the host entry equals the device entry; the current device is left alone; a second stream
    yy, alive = traj(3, 8, 2, 130, 31)
    uu, _ = traj(3, 8, 1, 130, 32)
    before = torch.cuda.current_device()
    res = envelope(yy, uu, alive, levels=L4, t0=7, device=0)
    assert torch.cuda.current_device() == before
    wy, sy = E.envelope_ref(yy, alive, L4, t0=7)
    wu, su = E.envelope_ref(uu, alive, L4, t0=7)
    check((res.y, res.spread["y"]), wy, sy, R.FIELDS, "mpct_envelope y")
    check((res.u, res.spread["u"]), wu, su, R.FIELDS, "mpct_envelope u")
    lo_, hi_ = res.band(1, 0, 0.05, 0.95)
    assert (R.bits(lo_) == R.bits(wy["quantile"][1, 0, :, 0])).all() and (R.bits(hi_) == R.bits(wy["quantile"][1, 0, :, 3])).all()
    assert res.costs(("spread", "spread_max")).shape == (3, 6)
    bare = envelope(None, uu, device=-1)
    assert bare.y is None and "quantile" not in bare.u
    wb, sb = E.envelope_ref(uu, None, [], t0=0)
    check((bare.u, bare.spread["u"]), wb, sb, R.BASE, "u alone, no alive, no levels")
    s2 = torch.cuda.Stream(torch.device("cuda", 0))
    got = device_call(yy, uu, alive, L4, 7, stream=s2)
    check(got["y"], wy, sy, R.FIELDS, "second stream y")
    check(got["u"], wu, su, R.FIELDS, "second stream u")


# ---------------------------------------------------------------------------------------------
# the scoring entry against the reference applied to eval_batch's trajectories
T0, DRAWS, NIT = 6, 8, 80
_scen = {}


def scen(name):
    """dict(sc, cands of 5 candidates (the fourth with a bad horizon), refs [8, my, nit], v)"""
    if name not in _scen:
        rng = np.random.default_rng(20261021)
        if name == "shell":
            from mpct.scenarios import shell3x3_mc

            sc, refs, _ = shell3x3_mc(draws=DRAWS, n2_max=10, nu_max=3, nit=NIT)
            v = None
            N2, Nu = np.array([10, 6, 8, 11, 4], np.int32), np.array([3, 2, 3, 2, 1], np.int32)
            d, l = 10.0 ** rng.uniform(-3, -1, (5, 3)), 10.0 ** rng.uniform(-3, -1, (5, 3))
        else:
            from mpct.scenarios import woodberry_toolbox_mc

            sc, refs, v, _, _ = woodberry_toolbox_mc(draws=DRAWS, nit=NIT)
            N2, Nu = np.array([30, 12, 20, 31, 8], np.int32), np.array([10, 2, 9, 6, 1], np.int32)
            d, l = 10.0 ** rng.uniform(-1, 1, (5, sc.my)), 10.0 ** rng.uniform(-1, 1, (5, sc.nu))
        _scen[name] = dict(sc=sc, cands=(N2, Nu, d, l), refs=np.ascontiguousarray(refs), v=v)
    return _scen[name]


_truth = {}


def truth(name, levels, j_bound=0.0):
    """the reference applied to eval_batch(want_traj=True), once per (scenario, levels, bound)"""
    from mpct.engine import eval_batch

    key = (name, tuple(levels), j_bound)
    if key not in _truth:
        q = scen(name)
        sc = q["sc"]
        if name not in _truth:
            res = eval_batch(sc, *q["cands"], q["refs"], v=q["v"], want_traj=True, device=0)
            _truth[name] = (res.y.reshape(5, DRAWS, sc.my, NIT), res.u.reshape(5, DRAWS, sc.nu, NIT),
                            res.J1.reshape(5, DRAWS, sc.my), res.status.reshape(5, DRAWS))
        y, u, J1, st = _truth[name]
        alive = R.alive_ref(J1, st, j_bound)
        _truth[key] = (E.envelope_ref(y, alive, levels, t0=T0), E.envelope_ref(u, alive, levels, t0=T0),
                       R.base_ref(J1, st, j_bound), alive)
    return _truth[key]


def run_entry(name, levels, j_bound=0.0, budget=0):
    from mpct import _lib
    from mpct.engine import eval_robust_envelope

    q = scen(name)
    lib = _lib.load()
    assert lib.mpct_internal_index_budget(int(budget)) == 0
    try:
        return eval_robust_envelope(q["sc"], *q["cands"], q["refs"], v=q["v"], levels=levels, j_bound=j_bound, t0=T0, device=0)
    finally:
        lib.mpct_internal_index_budget(0)


def assert_entry(res, name, levels, j_bound, msg):
    (wy, sy), (wu, su), wbase, alive = truth(name, levels or [], j_bound)
    use = R.FIELDS if levels else R.BASE
    check((res.y, res.spread["y"]), wy, sy, use, msg + " y")
    check((res.u, res.spread["u"]), wu, su, use, msg + " u")
    for f in ("mean", "worst", "n_failed", "worst_draw", "status"):
        assert (R.bits(getattr(res.base, f)) == R.bits(wbase[f])).all(), (f, msg)
    return alive


@pytest.mark.parametrize("name", ["shell", "woodberry"])
def test_eval_robust_envelope_against_composition(gpu, name):
    from mpct.engine import eval_robust

    q = scen(name)
    sc = q["sc"]
    res = run_entry(name, L4)
    assert res.y["lo"].shape == (5, sc.my, NIT) and res.u["cvar"].shape == (5, sc.nu, NIT, 4)
    alive = assert_entry(res, name, L4, 0.0, name)
    _, _, J1, st = _truth[name]
    assert st[3].tolist() == [16] * DRAWS and alive[[0, 1, 2, 4]].any()
    # the bad-horizon candidate: n = 0, NaN, -1 throughout, no failed draw
    assert (res.y["n"][3] == 0).all() and np.isnan(res.u["mean"][3]).all() and (res.y["q_draw"][3] == -1).all()
    assert np.isnan(res.spread["y"]["spread"][3]).all() and (res.spread["u"]["t_spread_max"][3] == -1).all()
    assert res.base.n_failed[3] == 0
    # a live draw's trajectory is finite, so every sample of a candidate has its live draws
    assert (res.y["n"] == alive.sum(axis=1)[:, None, None]).all()
    # base against mpct_eval_robust's record of the same batch.  Both calls end in robust_reduce_kernel; bit for
    # bit base is that reduction of this launch's own per-simulation J1 (assert_entry above).  Where the cost-only
    # batch of mpct_eval_robust and the trajectory batch of this entry run one kernel the two records are bitwise
    # equal.  On Shell 3x3 they do not (gpc_small_kernel against gpc_closed_loop_kernel<16,false,true>):
    # tests/test_gpu_parity.py holds each of the two to the C port within COST_RTOL, so their J1 agree within
    # 2 * COST_RTOL and so do the means and maxima over the draws; counts and statuses are exact, the worst draw is
    # the same where the two largest totals lie further apart than that bound (the rule of tests/test_limits_gpu.py)
    from mpct.engine import kernel_instance
    from test_gpu_parity import COST_RTOL

    rob = eval_robust(sc, *q["cands"], q["refs"], v=q["v"], device=0)
    one_kernel = kernel_instance(sc) == kernel_instance(sc, want_traj=True)
    print(name, kernel_instance(sc), "|", kernel_instance(sc, want_traj=True))
    assert one_kernel or name == "shell"
    if one_kernel:
        for f in ("mean", "worst", "n_failed", "worst_draw", "status"):
            assert (R.bits(getattr(res.base, f)) == R.bits(getattr(rob, f))).all(), f
    else:
        for f in ("n_failed", "status"):
            assert (getattr(res.base, f) == getattr(rob, f)).all(), f
        sim = [0, 1, 2, 4]
        assert (alive[sim].sum(axis=1) >= 2).all()
        tot = np.sort(np.where(alive[sim] != 0, J1[sim].sum(axis=2), -np.inf), axis=1)
        assert ((tot[:, -1] - tot[:, -2]) > 2 * COST_RTOL * tot[:, -1]).all()
        assert (res.base.worst_draw == rob.worst_draw).all()
        for f in ("mean", "worst"):
            got, ref = getattr(res.base, f), getattr(rob, f)
            print(f, "max rel difference to mpct_eval_robust", np.nanmax(np.abs(got - ref) / np.abs(ref)))
            assert (np.isnan(got) == np.isnan(ref)).all()
            np.testing.assert_allclose(got, ref, rtol=2 * COST_RTOL, atol=0, err_msg=f)
    # a bound between the two largest surviving totals of the candidate with the most live draws fails that draw
    c = int(np.argmax(alive.sum(axis=1)))
    J = np.sort(J1[c].sum(axis=1)[alive[c] != 0])
    assert J.size >= 2 and J[-2] < J[-1]
    bound = float(0.5 * (J[-2] + J[-1]))
    cut = run_entry(name, L4, j_bound=bound)
    assert_entry(cut, name, L4, bound, name + " with j_bound")
    assert cut.base.n_failed[c] == res.base.n_failed[c] + 1 and (cut.y["n"][c] == res.y["n"][c] - 1).all()
    # without levels; a repeated call; the table for pareto
    bare = run_entry(name, None)
    assert "quantile" not in bare.y
    assert_entry(bare, name, None, 0.0, name + " no levels")
    assert_entry(run_entry(name, L4), name, L4, 0.0, name + " repeated")
    tab = res.costs(("spread", "spread_max"), max_failed=DRAWS)
    assert tab.shape == (5, 2 * (sc.my + sc.nu)) and np.isnan(tab[3]).all() and np.isfinite(tab[c]).all()


@pytest.mark.parametrize("per_chunk", [2, 1])
def test_chunks_of_whole_candidates(gpu, per_chunk):
    sc = scen("shell")["sc"]
    per = DRAWS * (sc.my + sc.nu) * NIT * 8
    res = run_entry("shell", L4, budget=per_chunk * per + 8)        # ragged against 5
    assert_entry(res, "shell", L4, 0.0, "%d candidates per chunk" % per_chunk)


def test_two_calls_on_two_streams(gpu):
    import torch
    from mpct.engine import _batch_args, eval_robust_envelope_device

    q = scen("woodberry")
    sc = q["sc"]
    (wy, sy), (wu, su), wbase, _ = truth("woodberry", L4)
    N2, Nu, d, l, refs, Cn, nref, vv = _batch_args(sc, *q["cands"], q["refs"], q["v"])
    dev = torch.device("cuda", 0)
    ins = [torch.tensor(a, device=dev) for a in (N2, Nu, d, l, refs)]
    tv = torch.tensor(vv, device=dev)

    def outputs():
        out = {}
        for side, rows in (("y", sc.my), ("u", sc.nu)):
            out[side] = {f: torch.full((Cn, rows, NIT, 4) if f in R.LEVEL else (Cn, rows, NIT), -7,
                                       dtype=torch.int32 if f in R.INT_FIELDS else torch.float64, device=dev) for f in R.FIELDS}
            out["spread_" + side] = {f: torch.full((Cn, rows), -7, dtype=torch.int32 if f == "t_spread_max" else torch.float64,
                                                   device=dev) for f in E.SPREAD}
        base = {"mean": torch.zeros((Cn, sc.my), dtype=torch.float64, device=dev),
                "n_failed": torch.full((Cn,), -7, dtype=torch.int32, device=dev)}
        return out, base

    calls = [(torch.cuda.Stream(dev),) + outputs() for _ in range(2)]
    torch.cuda.synchronize(dev)
    for s, out, base in calls:      # back to back on one scenario: the second waits for the scratch of the first
        eval_robust_envelope_device(sc, *ins, out, base, v=tv, levels=L4, t0=T0, device=0, stream=s)
    for s, out, base in calls:
        s.synchronize()
        for side, w, ws in (("y", wy, sy), ("u", wu, su)):
            check(({f: t.cpu().numpy() for f, t in out[side].items()}, {f: t.cpu().numpy() for f, t in out["spread_" + side].items()}),
                  w, ws, R.FIELDS, "device entry, " + side)
        assert (R.bits(base["mean"].cpu().numpy()) == R.bits(wbase["mean"])).all()
        assert (base["n_failed"].cpu().numpy() == wbase["n_failed"]).all()
