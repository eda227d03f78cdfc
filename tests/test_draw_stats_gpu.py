"""GPU: the draw statistics (draw_stats.hip; include/mpct.h) against tests/draw_stats_ref.py, bit
for bit on all nine fields.

  * mpct_draw_stats_device on generated tables (draw_stats_ref.table: ties at both ends, zeros of both signs, NaN
    and +-inf, an all-dead column beside a live one, alive zeros; int32 with -1) at D = 1, 2, 63, 64, 65, 130
    (lane ownership wraps at 64), m = 1, 3, 7 (the two staging maps and ragged groups of four columns), C = 1
    and 5, with a forced grid of two workgroups so that they stride, D = 1365 / 1366 / 2730 / 2731 (where the
    waves per workgroup change: 4, 3, 2, 1) and D = 4096 (one wave per workgroup, the LDS ceiling); levels 1.0,
    one that clamps to rank 1, duplicates, unsorted; nlev = 0;
  * NULL-pointer subsets between guard words; the host entry equal to the device entry; a second stream;
  * the identity with the shipped robust scoring: mean / hi of J1 equal eval_robust's mean / worst, and on the
    totals the tail record equals the call's own;
  * eval_robust_indices against the composition eval_indices -> reference, on shell3x3_mc and woodberry_mc
    (5 candidates x 4 draws, one bad-horizon candidate), with a j_bound that fails exactly one draw, chunks of 2
    and 1 candidates, a field subset in a non-struct order, and the device entry on a stream."""
import ctypes as C

import numpy as np
import pytest

import draw_stats_ref as R

pytestmark = pytest.mark.gpu
GUARD = 32
CANARY = {np.dtype(np.float64): 0x7FF85A5A5A5A5A5A, np.dtype(np.int32): 0x5A5A5A5A}
LEVELS = [0.9, 1.0, 1e-9, 0.5, 0.9, 0.25]     # unsorted, a duplicate, level 1.0, one that clamps to rank 1


@pytest.fixture(scope="module")
def gpu(built, has_gpu):
    if not has_gpu:
        pytest.skip("no GPU")
    return True


def _dtype(f):
    return np.dtype(np.int32 if f in R.INT_FIELDS else np.float64)


def device_call(x, alive, levels, fields=R.FIELDS, grid=0, stream=None):
    """mpct_draw_stats_device through engine.draw_stats_device with exactly `fields` requested, each buffer
    between GUARD canary words on both sides.  Returns {field: array} after checking the guards and that every
    element was written."""
    import torch
    from mpct import _lib
    from mpct.engine import draw_stats_device

    dev = torch.device("cuda", 0)
    Cn, D, m = x.shape
    nlev = len(levels)
    tx = torch.tensor(x, device=dev)
    ta = torch.tensor(alive, device=dev) if alive is not None else None
    bufs, out = {}, {}
    for f in fields:
        dt, n = _dtype(f), Cn * m * (nlev if f in R.LEVEL else 1)
        t = torch.full((n + 2 * GUARD,), CANARY[dt], dtype=torch.int32 if dt == np.int32 else torch.int64, device=dev)
        bufs[f] = (t, n)
        out[f] = t[GUARD:GUARD + n]
    torch.cuda.synchronize(dev)
    lib = _lib.load()
    assert lib.mpct_internal_draw_stats_grid(int(grid)) == 0
    try:
        if stream is None:
            draw_stats_device(tx, out, ta, levels if nlev else None)
        else:
            with torch.cuda.stream(stream):
                draw_stats_device(tx, out, ta, levels if nlev else None)
    finally:
        lib.mpct_internal_draw_stats_grid(0)
    (stream or torch.cuda.current_stream(dev)).synchronize()
    got = {}
    for f, (t, n) in bufs.items():
        a = t.cpu().numpy()
        dt = _dtype(f)
        can = a.dtype.type(CANARY[dt])
        assert np.all(a[:GUARD] == can) and np.all(a[GUARD + n:] == can), "guard of %s overwritten" % f
        rows = a[GUARD:GUARD + n]
        assert not np.any(rows == can), "%s: elements never written" % f
        got[f] = rows.view(dt).reshape((Cn, m, nlev) if f in R.LEVEL else (Cn, m)).copy()
    return got


@pytest.mark.parametrize("m", [1, 3, 7])
@pytest.mark.parametrize("D", [1, 2, 63, 64, 65, 130])
def test_draw_stats_device_bitwise(gpu, D, m):
    for Cn in (1, 5):
        for as_int in (False, True):
            x, alive = R.table(Cn, D, m, 1000 * D + 10 * m + Cn, as_int)
            want = R.stats_ref(x, alive, LEVELS)
            got = device_call(x, alive, LEVELS)
            R.assert_same_stats(got, want, msg="C=%d D=%d m=%d int=%s" % (Cn, D, m, as_int))
            # level 1.0 is hi / hi_draw, duplicate levels give equal columns
            live = got["n"] > 0
            assert (R.bits(got["quantile"][..., 1]) == R.bits(got["hi"])).all() and (got["q_draw"][..., 1] == got["hi_draw"]).all()
            assert (got["cvar"][..., 1][live] == got["hi"][live]).all()              # 0.0 + hi: equal in value
            assert (R.bits(got["cvar"][..., 0]) == R.bits(got["cvar"][..., 4])).all()
            # rank 1 is the minimum, at the HIGHEST draw that holds it
            assert (got["quantile"][..., 2][live] == got["lo"][live]).all()
            assert (got["q_draw"][..., 2][live] >= got["lo_draw"][live]).all()
    # alive = NULL, no levels; the workgroups stride over the column groups; a record does not depend on C
    x, alive = R.table(5, D, m, 77 + D + m)
    want = R.stats_ref(x, None, [])
    R.assert_same_stats(device_call(x, None, [], fields=R.BASE), want, fields=R.BASE, msg="alive NULL, nlev 0")
    full = R.stats_ref(x, alive, LEVELS)
    R.assert_same_stats(device_call(x, alive, LEVELS, grid=2), full, msg="grid of 2 workgroups")
    one = device_call(np.ascontiguousarray(x[3:4]), np.ascontiguousarray(alive[3:4]), LEVELS)
    R.assert_same_stats(one, {f: a[3:4] for f, a in full.items()}, msg="candidate 3 alone")


def test_draw_stats_at_the_lds_ceiling(gpu):
    """D = 4096: one 48 KB slice, one wave per workgroup."""
    rng = np.random.default_rng(4096)
    x = rng.integers(0, 200, (1, 4096, 1)).astype(np.float64) / 8.0       # many ties
    x[0, rng.integers(0, 4096, 300), 0] = np.nan
    alive = (rng.random((1, 4096)) > 0.1).astype(np.int32)
    levels = [0.95, 1.0, 1e-9]
    R.assert_same_stats(device_call(x, alive, levels), R.stats_ref(x, alive, levels), msg="D = 4096")


@pytest.mark.parametrize("D", [1365, 1366, 2730, 2731])
def test_draw_stats_at_the_wave_count_switches(gpu, D):
    """D = 1,365 is the last size with four waves per workgroup (65,520 B of the 64 KiB of dynamic LDS, the slice
    offsets at their largest), 1,366 the first with three; 2,730 the last with two, 2,731 the first with one.
    m = 3 and C = 2: six columns, so the last group of columns is ragged at four and at three waves."""
    rng = np.random.default_rng(D)
    x = rng.integers(0, 60, (2, D, 3)).astype(np.float64) / 4.0          # many ties
    x[rng.random((2, D, 3)) < 0.05] = np.nan
    x[1, :, 2] = np.inf                                                   # an all-dead column in the ragged group
    alive = (rng.random((2, D)) > 0.1).astype(np.int32)
    levels = [0.95, 1.0, 1e-9]
    R.assert_same_stats(device_call(x, alive, levels), R.stats_ref(x, alive, levels), msg="D = %d" % D)


def test_null_pointer_subsets(gpu):
    x, alive = R.table(5, 65, 3, 5)
    full = device_call(x, alive, LEVELS)
    for fields in [("n",), ("mean",), ("lo_draw", "hi"), ("cvar",), ("q_draw", "n"), ("quantile", "lo", "hi_draw"), R.BASE]:
        got = device_call(x, alive, LEVELS, fields=fields)
        assert set(got) == set(fields)
        R.assert_same_stats(got, full, fields=fields, msg="subset %s" % (fields,))


def test_host_entry_and_second_stream(gpu):
    import torch
    from mpct.engine import draw_stats

    x, alive = R.table(5, 130, 3, 9)
    xi, _ = R.table(5, 130, 3, 10, True)
    want, wanti = device_call(x, alive, LEVELS), device_call(xi, alive, LEVELS)
    before = torch.cuda.current_device()
    res, resi = draw_stats(x, alive, LEVELS, device=0), draw_stats(xi, alive, LEVELS, device=-1)
    assert torch.cuda.current_device() == before
    assert res.n.shape == (5, 3) and res.cvar.shape == (5, 3, len(LEVELS)) and res.q_draw.dtype == np.int32
    R.assert_same_stats({f: getattr(res, f) for f in R.FIELDS}, want, msg="mpct_draw_stats")
    R.assert_same_stats({f: getattr(resi, f) for f in R.FIELDS}, wanti, msg="mpct_draw_stats int32")
    bare = draw_stats(x)
    assert bare.quantile is None
    R.assert_same_stats({f: getattr(bare, f) for f in R.BASE}, R.stats_ref(x, None, []), fields=R.BASE)
    st = torch.cuda.Stream(torch.device("cuda", 0))
    R.assert_same_stats(device_call(x, alive, LEVELS, stream=st), want, msg="second stream")


# ---------------------------------------------------------------------------------------------
# the identity with the shipped robust scoring, and the scoring entry against the composition
T0, REL, AB = 4, 0.05, 1e-3
TAIL = [0.9, 1.0, 0.5]
_scen = {}


def scen(name):
    """dict(sc, cands of 5 candidates (the fourth with a bad horizon), refs [4, my, nit], v) at the scenario's own nit"""
    if name not in _scen:
        rng = np.random.default_rng(20251020)
        if name == "shell":
            from mpct.scenarios import shell3x3_mc

            sc, refs, _ = shell3x3_mc(draws=4)
            v = None
            N2, Nu = np.array([30, 12, 20, 31, 8], np.int32), np.array([5, 2, 3, 2, 1], np.int32)
            d, l = 10.0 ** rng.uniform(-3, -1, (5, 3)), 10.0 ** rng.uniform(-3, -1, (5, 3))
        else:
            from mpct.dtc import woodberry_mc

            sc, refs, v, _ = woodberry_mc(draws=4)
            N2, Nu = np.array([30, 12, 20, 5, 8], np.int32), np.array([10, 2, 9, 6, 1], np.int32)
            d, l = 10.0 ** rng.uniform(-1, 1, (5, 2)), 10.0 ** rng.uniform(-1, 1, (5, 2))
        _scen[name] = dict(sc=sc, cands=(N2, Nu, d, l), refs=refs, v=v)
    return _scen[name]


_comp = {}


def composition(name):
    """eval_indices with the costs of the same launch, once: the per-simulation records [C, D, w], J1 [C, D, my]
    and status [C, D]"""
    from mpct.engine import eval_indices

    if name not in _comp:
        q = scen(name)
        res = eval_indices(q["sc"], *q["cands"], q["refs"], v=q["v"], t0=T0, band_rel=REL, band_abs=AB, want_costs=True, device=0)
        rec = {f: getattr(res, f) for f in R.INDEX_FIELDS}
        J1 = res.batch.J1.reshape(5, 4, -1)
        st = res.batch.status.reshape(5, 4)
        for a in list(rec.values()) + [J1, st]:
            a.setflags(write=False)
        _comp[name] = (rec, J1, st)
    return _comp[name]


def run_entry(name, fields, levels, j_bound=0.0, budget=0):
    from mpct import _lib
    from mpct.engine import eval_robust_indices

    q = scen(name)
    lib = _lib.load()
    assert lib.mpct_internal_index_budget(int(budget)) == 0
    try:
        return eval_robust_indices(q["sc"], *q["cands"], q["refs"], v=q["v"], fields=fields, levels=levels, j_bound=j_bound,
                                   t0=T0, band_rel=REL, band_abs=AB, device=0)
    finally:
        lib.mpct_internal_index_budget(0)


def assert_entry(res, name, fields, levels, j_bound, msg):
    rec, J1, st = composition(name)
    want, wbase = R.robust_indices_ref(rec, J1, st, j_bound, fields, levels)
    use = R.FIELDS if len(levels) else R.BASE
    R.assert_same_stats({f: getattr(res, f) for f in use}, want, fields=use, msg=msg)
    for f in ("mean", "worst", "n_failed", "worst_draw", "status"):
        assert (R.bits(getattr(res.base, f)) == R.bits(wbase[f])).all(), (f, msg)
    return want, wbase


def test_draw_stats_identity_with_eval_robust(gpu):
    from mpct.engine import draw_stats, eval_robust

    q = scen("shell")
    res = eval_robust(q["sc"], *q["cands"], q["refs"], want_J1=True, levels=TAIL, device=0)
    J1 = res.J1.reshape(5, 4, 3)
    # the survivors of the call: every draw of a simulated candidate is clean here, the bad horizon has none
    alive = np.repeat((res.status == 0)[:, None], 4, axis=1).astype(np.int32)
    print("status", res.status.tolist(), "n_failed", res.n_failed.tolist())
    assert res.n_failed.tolist() == [0] * 5 and res.status.tolist() == [0, 0, 0, 16, 0]
    per = draw_stats(J1, alive, device=0)
    assert (R.bits(per.mean) == R.bits(res.mean)).all() and (R.bits(per.hi) == R.bits(res.worst)).all()
    J = np.zeros((5, 4, 1))
    for i in range(3):
        J[:, :, 0] += J1[:, :, i]
    tot = draw_stats(J, alive, levels=TAIL, device=0)
    for f in R.LEVEL:
        assert (R.bits(getattr(tot, f)[:, 0]) == R.bits(getattr(res, f))).all(), f
    assert (tot.hi_draw[:, 0] == res.worst_draw).all()


@pytest.mark.parametrize("name", ["shell", "dtc"])
def test_eval_robust_indices_against_composition(gpu, name):
    q = scen(name)
    sc = q["sc"]
    rec, J1, st = composition(name)
    assert st[3].tolist() == [16] * 4 and (st[[0, 1, 2, 4]] == 0).all()
    res = run_entry(name, R.INDEX_FIELDS, TAIL)
    W = 8 * sc.my + 5 * sc.nu
    assert res.hi.shape == (5, W) and res.cvar.shape == (5, W, 3) and len(res.columns) == W
    want, wbase = assert_entry(res, name, R.INDEX_FIELDS, TAIL, 0.0, name)
    # the bad-horizon candidate: n = 0, NaN, -1 throughout, no failed draw
    assert (res.n[3] == 0).all() and np.isnan(res.mean[3]).all() and np.isnan(res.cvar[3]).all()
    assert (res.lo_draw[3] == -1).all() and (res.q_draw[3] == -1).all() and res.base.n_failed[3] == 0
    # every record of a live draw is valid here, so a column's n is its candidate's live draws (the shell draws
    # all survive; some of the DTC mismatch draws destabilise past the default bound with status 0)
    alive = R.alive_ref(J1, st, 0.0)
    assert (res.n == alive.sum(axis=1)[:, None]).all() and (res.base.n_failed[[0, 1, 2, 4]] == 4 - alive.sum(axis=1)[[0, 1, 2, 4]]).all()
    if name == "shell":
        assert (res.n[[0, 1, 2, 4]] == 4).all() and np.isfinite(res.hi[[0, 1, 2, 4]]).all()
    # a bound between the two largest surviving totals of the candidate with the most live draws fails exactly
    # that one draw more
    c = int(np.argmax(alive.sum(axis=1)))
    J = np.sort(J1[c].sum(axis=1)[alive[c] != 0])
    assert J.size >= 2 and J[-2] < J[-1]
    bound = float(0.5 * (J[-2] + J[-1]))
    assert J[-2] < bound < J[-1]
    cut = run_entry(name, R.INDEX_FIELDS, TAIL, j_bound=bound)
    assert_entry(cut, name, R.INDEX_FIELDS, TAIL, bound, name + " with j_bound")
    assert cut.base.n_failed[c] == res.base.n_failed[c] + 1 and (cut.n[c] == res.n[c] - 1).all()
    # a subset in a non-struct order, without levels; a repeated call
    sub = ("tv", "over", "settle")
    part = run_entry(name, sub, None)
    assert part.quantile is None and part.columns[0] == ("tv", 0) and part.columns[sc.nu] == ("over", 0)
    assert_entry(part, name, sub, [], 0.0, name + " subset")
    assert_entry(run_entry(name, R.INDEX_FIELDS, TAIL), name, R.INDEX_FIELDS, TAIL, 0.0, name + " repeated")
    # the table for pareto: hi of the named columns; the candidate that was never simulated has no failed draw,
    # its NaN is the statistic's own
    tab = res.costs("hi", names=("over", "tv"), max_failed=4)
    assert tab.shape == (5, sc.my + sc.nu) and np.isnan(tab[3]).all() and np.isfinite(tab[c]).all()
    assert np.isnan(cut.costs("hi")[c]).all() and np.isfinite(cut.costs("hi", max_failed=4)[c]).all()


@pytest.mark.parametrize("per_chunk", [2, 1])
def test_chunks_of_whole_candidates(gpu, per_chunk):
    q = scen("shell")
    sc = q["sc"]
    per = 4 * (sc.my + sc.nu) * sc.nit * 8
    res = run_entry("shell", ("settle", "iae", "u_hi", "t_emax"), TAIL, budget=per_chunk * per + 8)    # ragged against 5
    assert_entry(res, "shell", ("settle", "iae", "u_hi", "t_emax"), TAIL, 0.0, "%d candidates per chunk" % per_chunk)


def test_eval_robust_indices_device_on_a_stream(gpu):
    import torch
    from mpct.engine import _batch_args, eval_robust_indices_device

    q = scen("dtc")
    sc = q["sc"]
    fields = ("dumax", "e_final", "t_emax")
    rec, J1, st = composition("dtc")
    want, wbase = R.robust_indices_ref(rec, J1, st, 0.0, fields, TAIL)
    N2, Nu, d, l, refs, Cn, nref, vv = _batch_args(sc, *q["cands"], q["refs"], q["v"])
    dev = torch.device("cuda", 0)
    ins = [torch.tensor(a, device=dev) for a in (N2, Nu, d, l, refs)]
    W = sc.nu + 2 * sc.my
    out = {f: torch.full((Cn, W, 3) if f in R.LEVEL else (Cn, W), -7, dtype=torch.int32 if f in R.INT_FIELDS else torch.float64,
                         device=dev) for f in R.FIELDS}
    base = {"mean": torch.zeros((Cn, sc.my), dtype=torch.float64, device=dev),
            "n_failed": torch.full((Cn,), -7, dtype=torch.int32, device=dev)}
    tv = torch.tensor(vv, device=dev)
    torch.cuda.synchronize(dev)
    s = torch.cuda.Stream(dev)
    for _ in range(2):          # back to back on one scenario: the second waits for the scratch of the first
        eval_robust_indices_device(sc, *ins, out, base, v=tv, fields=fields, levels=TAIL, t0=T0, band_rel=REL, band_abs=AB,
                                   device=0, stream=s)
    s.synchronize()
    R.assert_same_stats({f: out[f].cpu().numpy() for f in R.FIELDS}, want, msg="device entry on a stream")
    assert (R.bits(base["mean"].cpu().numpy()) == R.bits(wbase["mean"])).all()
    assert (base["n_failed"].cpu().numpy() == wbase["n_failed"]).all()
