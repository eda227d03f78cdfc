"""GPU: the closed-loop performance indices (traj_indices.hip; include/mpct.h) against tests/indices_ref.py,
bit for bit on every field.

  * mpct_indices_device on generated trajectories at the block edges of the 64-lane stride (nit 1, 2, 63, 64,
    65, 130, 500; t0 0, 1, nit - 1), with a step reference, ties in |e|, samples on the band edge, NaN rows,
    +-inf samples and zeros of both signs (indices_ref.generated); the same sums against the order-free
    bound n * 2^-53 * sum|term|;
  * NULL-pointer subsets between guard words; mpct_indices (host pointers) equal to the device route, the
    current device unchanged;
  * eval_indices against the reference applied to the trajectories of eval_batch(want_traj=True) of the
    same batch: a linear GPC batch with an N2 = 0 and a bad-horizon candidate, a DTC batch, the Van de Vusse
    NMPC batch; the optional costs equal to eval_batch's;
  * chunk independence (2 of 5, 1 of 5, 256 + 44 of 300), repeated calls, a non-default stream."""
import ctypes as C

import numpy as np
import pytest

import indices_ref as R
import record_calls as rc
from test_indices import CASES

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


def device_call(y, u, r, t0, fields=ALL, rel=R.BAND_REL, ab=R.BAND_ABS, drop=()):
    """mpct_indices_device through engine.indices_device with exactly `fields` requested, each buffer between
    GUARD canary words on both sides; the trajectories named in `drop` are passed as NULL.  Returns
    {field: [S, w]} after checking the guards and that every element was written."""
    import torch
    from mpct.engine import indices_device

    dev = torch.device("cuda", 0)
    S, my, nu = y.shape[0], y.shape[1], u.shape[1]
    ty, tu, tr = (None if n in drop else torch.tensor(a, device=dev) for n, a in (("y", y), ("u", u), ("r", r)))
    bufs, out = {}, {}
    for f in fields:
        dt, w = _dtype(f), (my if f in R.Y_FIELDS else nu)
        t = torch.full((S * w + 2 * GUARD,), CANARY[dt], dtype=torch.int32 if dt == np.int32 else torch.int64, device=dev)
        bufs[f] = t
        out[f] = t[GUARD:GUARD + S * w]
    if "y" in drop:      # the shapes the binding cannot read off a missing tensor
        from mpct import _lib

        p = _lib.MpctIndexParams(int(t0), rel, ab)
        o = _lib.MpctIndexResult()
        for f in fields:
            setattr(o, f, C.cast(C.c_void_p(out[f].data_ptr()), _lib.c_int32_p if f in R.INT_FIELDS else _lib.c_double_p))
        code = _lib.load().mpct_indices_device(None, C.c_void_p(tu.data_ptr()), None, S, r.shape[0], my, nu, y.shape[2],
                                               C.byref(p), C.byref(o), C.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
        assert code == 0, _lib.last_error()
    else:
        indices_device(ty, tu, tr, out, t0=t0, band_rel=rel, band_abs=ab)
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


@pytest.mark.parametrize("S,nref,my,nu,nit,t0", CASES)
def test_indices_device_bitwise(gpu, S, nref, my, nu, nit, t0):
    y, u, r = R.generated(S, nref, my, nu, nit)
    want = R.indices_np(y, u, r, t0, R.BAND_REL, R.BAND_ABS)
    got = device_call(y, u, r, t0)
    R.assert_bitwise(got, want, what="mpct_indices_device")
    assert R.check_order_free(got, y, u, r, t0) > 0
    # a repeated call is bitwise identical, and a record does not depend on the row's place in the batch
    R.assert_bitwise(device_call(y, u, r, t0), got, what="repeat")
    if S % (2 * nref) == 0:
        h = S // 2
        back = device_call(np.concatenate([y[h:], y[:h]]), np.concatenate([u[h:], u[:h]]), r, t0)
        R.assert_bitwise({f: np.concatenate([a[h:], a[:h]]) for f, a in back.items()}, got, what="rotated batch")


def test_null_pointer_subsets(gpu):
    y, u, r = R.generated(6, 3, 3, 2, 130)
    full = device_call(y, u, r, 1)
    for fields, drop in [(("settle",), ()), (("itae",), ()), (("dumax",), ()), (R.Y_FIELDS, ("u",)),
                         (R.U_FIELDS, ("y", "r")), (("t_emax", "u_hi"), ())]:
        got = device_call(y, u, r, 1, fields=fields, drop=drop)
        assert set(got) == set(fields)
        R.assert_bitwise(got, full, fields=fields, what="subset %s without %s" % (fields, drop))


def test_host_entry_equals_device_entry(gpu):
    import torch
    from mpct.engine import indices

    y, u, r = R.generated(6, 3, 3, 2, 130)
    want = device_call(y, u, r, 1)
    before = torch.cuda.current_device()
    res = indices(y, u, r, t0=1, band_rel=R.BAND_REL, band_abs=R.BAND_ABS, device=0)
    assert torch.cuda.current_device() == before
    assert res.iae.shape == (2, 3, 3) and res.tv.shape == (2, 3, 2) and res.settle.dtype == np.int32
    R.assert_bitwise({f: getattr(res, f).reshape(6, -1) for f in ALL}, want, what="mpct_indices")
    part = indices(None, u, None, t0=1, fields=("tv", "u_lo"), device=-1)
    assert part.iae is None and part.tv.shape == (6, 1, 2)
    R.assert_bitwise({f: getattr(part, f).reshape(6, -1) for f in ("tv", "u_lo")}, want, fields=("tv", "u_lo"))


# ---------------------------------------------------------------------------------------------
# eval_indices: the records of a scored batch against the reference on eval_batch's trajectories
BATCHES = {"shell5": [0, 16, 3, 17, 9], "dtc": [1, 9, 16, 12], "nmpc": [2, 15]}
T0, REL, AB = 4, 0.05, 1e-3
_scen, _ref = {}, {}


def batch(name):
    if name not in _scen:
        q = rc.scenario(name)
        _scen[name] = (q, rc.take(q["pool"], np.array(BATCHES[name])))
    return _scen[name]


def reference(name):
    """eval_batch with trajectories for the batch, once, and the reference's records of them"""
    from mpct.engine import eval_batch

    if name not in _ref:
        q, cands = batch(name)
        res = eval_batch(q["sc"], *cands, q["refs"], v=q["v"], want_traj=True, device=0)
        want = R.indices_np(res.y, res.u, q["refs"], T0, REL, AB)
        for a in want.values():
            a.setflags(write=False)
        _ref[name] = (res, want)
    return _ref[name]


def flat(res):
    return {f: getattr(res, f).reshape(-1, getattr(res, f).shape[-1]) for f in ALL}


def run_eval(name, budget=0, **kw):
    from mpct import _lib
    from mpct.engine import eval_indices

    q, cands = batch(name)
    lib = _lib.load()
    assert lib.mpct_internal_index_budget(int(budget)) == 0
    try:
        return eval_indices(q["sc"], *cands, q["refs"], v=q["v"], t0=T0, band_rel=REL, band_abs=AB, device=0, **kw)
    finally:
        lib.mpct_internal_index_budget(0)


@pytest.mark.parametrize("name", list(BATCHES))
def test_eval_indices_against_reference(gpu, name):
    q, cands = batch(name)
    ev, want = reference(name)
    sc, nref = q["sc"], q["refs"].shape[0]
    Cn = len(BATCHES[name])
    res = run_eval(name, want_costs=True)
    assert res.iae.shape == (Cn, nref, sc.my) and res.tv.shape == (Cn, nref, sc.nu)
    R.assert_bitwise(flat(res), want, what=name)
    st = ev.status.reshape(Cn, nref)
    run = st[:, 0] & 24 == 0
    assert run.any() and np.isfinite(res.iae[run]).all() and (res.settle[run] >= T0).all()
    if name == "shell5":
        assert st[1, 0] == 8 and st[3, 0] == 16          # N2 = 0 and a bad horizon: NaN / -1 rows
        for c in (1, 3):
            assert np.isnan(res.iae[c]).all() and (res.settle[c] == -1).all() and (res.t_emax[c] == -1).all()
            assert np.isnan(res.tv[c]).all() and np.isnan(res.u_hi[c]).all()
    # the costs of the same launch are eval_batch's
    for f in ("J1", "j22", "status", "qp_iters"):
        assert (rc.bits(getattr(res.batch, f)) == rc.bits(getattr(ev, f))).all(), f
    assert np.isnan(res.batch.j21).all() and np.isnan(res.batch.Jnu).all()
    # a single field: that one alone, the same bits
    one = run_eval(name, fields=("ise",))
    assert one.tv is None and one.iae is None and (R.bits(one.ise.reshape(-1, sc.my)) == R.bits(want["ise"])).all()
    # a repeated call is bitwise identical
    R.assert_bitwise(flat(run_eval(name)), want, what=name + " repeated")


@pytest.mark.parametrize("per_chunk", [2, 1])
def test_chunks_of_whole_candidates(gpu, per_chunk):
    q, cands = batch("shell5")
    _, want = reference("shell5")
    sc, nref = q["sc"], q["refs"].shape[0]
    per = nref * (sc.my + sc.nu) * sc.nit * 8
    res = run_eval("shell5", budget=per_chunk * per + 8, want_costs=True)     # ragged against 5 candidates
    R.assert_bitwise(flat(res), want, what="%d candidates per chunk" % per_chunk)
    ev, _ = reference("shell5")
    for f in ("J1", "j22", "status", "qp_iters"):
        assert (rc.bits(getattr(res.batch, f)) == rc.bits(getattr(ev, f))).all(), f


def test_chunk_on_the_sorted_dispatch_path(gpu):
    """C = 300 as 256 + 44: the first chunk is dispatched heaviest-first (kOrderMinC = 256), the second is
    not; both equal the unchunked call, which sorts all 300"""
    from mpct import _lib
    from mpct.engine import eval_indices

    q = rc.scenario("shell5")
    sc = q["sc"]
    idx = rc.tiled(300)
    cands = rc.take(q["pool"], idx)
    refs = q["refs"][:1]
    per = (sc.my + sc.nu) * sc.nit * 8
    lib = _lib.load()
    one = eval_indices(sc, *cands, refs, t0=T0, band_rel=REL, band_abs=AB, device=0)
    assert lib.mpct_internal_index_budget(256 * per) == 0
    try:
        two = eval_indices(sc, *cands, refs, t0=T0, band_rel=REL, band_abs=AB, device=0)
    finally:
        lib.mpct_internal_index_budget(0)
    R.assert_bitwise(flat(two), flat(one), what="256 + 44 against 300")
    # and both are the records of the pool's candidates
    _, want = reference("shell5")
    pool_of = {c: k for k, c in enumerate(BATCHES["shell5"])}
    hits = [c for c in range(300) if int(idx[c]) in pool_of]
    assert len(hits) > 50
    for c in hits:
        for f in ALL:
            assert (R.bits(flat(one)[f][c]) == R.bits(want[f][3 * pool_of[int(idx[c])]])).all(), (f, c)
    assert np.isfinite(one.iae[idx < 16]).all() and np.isnan(one.iae[idx >= 16]).all()


def test_eval_indices_device_on_a_stream(gpu):
    import torch
    from mpct.engine import _batch_args, eval_indices_device

    q, cands = batch("shell5")
    ev, want = reference("shell5")
    sc = q["sc"]
    N2, Nu, d, l, refs, Cn, nref, _ = _batch_args(sc, *cands, q["refs"], None)
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
        eval_indices_device(sc, *ins, out, t0=T0, band_rel=REL, band_abs=AB, device=0, stream=st)
    st.synchronize()
    R.assert_bitwise({f: out[f].cpu().numpy() for f in ALL}, want, what="device entry on a stream")
    assert (rc.bits(out["J1"].cpu().numpy()) == rc.bits(ev.J1)).all()
    assert (out["status"].cpu().numpy() == ev.status).all()
