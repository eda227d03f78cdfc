"""GPU: the tail statistics end to end (mpct_eval_robust_tail, mpct_eval_robust_tail_device;
include/mpct.h).

The yardstick is tests/tail_ref.py applied to the J1 sample and the statuses of the EXISTING
per-simulation path (eval_batch, cost-only) on the same batch -- never the new code's own output.
Fused route (dtc_robust_kernel, then robust_tail_kernel on its sample): config 4, twelve candidates
at D = 5, 32, 128; the fall-through at D = 129; generic route: the Shell 3x3 model-error scenario,
twelve candidates x 4 draws.  Every case: the tail record is the yardstick's, the base record is
eval_robust's, host and device entries agree, a repeated and a reversed call agree, and the record
is the same with and without a J1 of the caller's (the scenario's robust scratch).  Then batches
with a dispatch order and strided workgroups, and tail / robust / batch calls interleaved on one
scenario across a regrow of the staging blob.  Every comparison is bitwise; no tolerance appears."""
import numpy as np
import pytest

from tail_ref import FIELDS, assert_same_tail, tail_ref
from test_robust_gpu import (RECORD, _device_inputs, bits, large_config4_batch, per_sim, rows, same_bits, shell_large,
                             totals)

pytestmark = [pytest.mark.gpu, pytest.mark.filterwarnings("error::RuntimeWarning")]

LEVELS = (0.5, 0.9, 1.0, 0.25, 0.9)    # unsorted, one duplicate
BASE = RECORD + ("J1",)


@pytest.fixture(scope="module")
def gpu(built, has_gpu):
    if not has_gpu:
        pytest.skip("no GPU")
    return True


def tail_of(res):
    return {f: getattr(res, f) for f in FIELDS}


def call(sc, q, refs, v, jb, levels=LEVELS, want_J1=True):
    from mpct.engine import eval_robust

    return eval_robust(sc, q["N2"], q["Nu"], q["d"], q["l"], refs, v=v, j_bound=jb, want_J1=want_J1, levels=levels)


def device_call(sc, q, refs, v, jb, levels=LEVELS, with_J1=True, base=True, stream=None, sync=True, inputs=None):
    """eval_robust_device(levels=...) into fresh output tensors."""
    import torch
    from mpct.engine import eval_robust_device

    dev = torch.device("cuda", 0)
    t, tr, tv = inputs if inputs is not None else _device_inputs(q, refs, v)
    Cn, D, my, nlev = t[0].numel(), tr.shape[0], sc.my, len(levels)
    out = dict(quantile=torch.empty((Cn, nlev), dtype=torch.float64, device=dev),
               cvar=torch.empty((Cn, nlev), dtype=torch.float64, device=dev),
               q_draw=torch.empty((Cn, nlev), dtype=torch.int32, device=dev))
    if base:
        out.update(mean=torch.empty((Cn, my), dtype=torch.float64, device=dev),
                   worst=torch.empty((Cn, my), dtype=torch.float64, device=dev),
                   n_failed=torch.empty(Cn, dtype=torch.int32, device=dev),
                   worst_draw=torch.empty(Cn, dtype=torch.int32, device=dev),
                   status=torch.empty(Cn, dtype=torch.int32, device=dev))
    if with_J1:
        out["J1"] = torch.empty((Cn * D, my), dtype=torch.float64, device=dev)
    eval_robust_device(sc, *t, tr, out, v=tv, j_bound=jb, stream=stream, levels=levels)
    if sync:
        torch.cuda.synchronize(dev)
    return out


def choose(sc, pool, refs, v, want=12):
    """Twelve candidates of the pool and a bound, chosen on the per-simulation yardstick: the bound is
    the median of the finite totals; up to six candidates with some but not all draws failed, up to
    three without a failed draw, the rest in index order."""
    D = refs.shape[0]
    J1, st = per_sim(sc, pool["N2"], pool["Nu"], pool["d"], pool["l"], refs, v)
    J = totals(J1, st)
    jb = float(np.median(J[np.isfinite(J)]))
    n = tail_ref(J1, st, jb, (1.0,))["n"]
    partial, clean = np.flatnonzero((n > 0) & (n < D)), np.flatnonzero(n == D)
    pick = partial[:6].tolist() + clean[:3].tolist()
    pick += [c for c in range(len(n)) if c not in pick][:want - len(pick)]
    return rows(pool, np.array(sorted(pick))), jb


def check_case(sc, q, refs, v, jb, min_partial=3):
    """Everything the module docstring promises of one case; returns the host call's result."""
    from mpct.engine import eval_robust

    Cn, D = len(q["N2"]), refs.shape[0]
    J1, st = per_sim(sc, q["N2"], q["Nu"], q["d"], q["l"], refs, v)
    want = tail_ref(J1, st, jb, LEVELS)
    nf = np.where(want["n"] == 0, 0, D - want["n"])
    partial = int(((want["n"] > 0) & (want["n"] < D)).sum())
    print("D = %d, j_bound %.6g: survivors %s" % (D, jb, want["n"].tolist()))
    assert partial >= min_partial, "fewer than %d candidates with 0 < n_failed < D" % min_partial
    if D >= 3:
        assert any(len(set(want["q_draw"][c].tolist())) >= 2 for c in range(Cn))
    base = eval_robust(sc, q["N2"], q["Nu"], q["d"], q["l"], refs, v=v, j_bound=jb, want_J1=True)
    a = call(sc, q, refs, v, jb)
    print("the J1 sample is bitwise eval_batch's: %s" % bool(np.array_equal(bits(a.J1.reshape(J1.shape)), bits(J1))))
    np.testing.assert_array_equal(bits(a.J1.reshape(J1.shape)), bits(J1))
    assert_same_tail(tail_of(a), want, msg="host entry")
    same_bits(a, base, BASE)                                   # the base record is eval_robust's
    np.testing.assert_array_equal(a.n_failed[want["n"] > 0], nf[want["n"] > 0])
    np.testing.assert_array_equal(a.q_draw[:, 2], a.worst_draw)  # level 1.0
    np.testing.assert_array_equal(bits(a.quantile[:, 2]), bits(a.cvar[:, 2]))
    np.testing.assert_array_equal(bits(a.quantile[:, 1]), bits(a.quantile[:, 4]))   # duplicate levels
    # without a J1 of the caller's: the scenario's scratch
    b = call(sc, q, refs, v, jb, want_J1=False)
    assert_same_tail(tail_of(b), want, msg="scratch")
    same_bits(b, base)
    # repeated, reversed
    assert_same_tail(tail_of(call(sc, q, refs, v, jb)), want, msg="repeated")
    r = call(sc, rows(q, np.arange(Cn)[::-1]), refs, v, jb, want_J1=False)
    assert_same_tail({f: getattr(r, f)[::-1] for f in FIELDS}, want, msg="reversed")
    for f in RECORD:
        np.testing.assert_array_equal(bits(getattr(r, f)[::-1]), bits(getattr(base, f)), err_msg=f)
    # the device entry: everything, the tail alone with and without a sample
    dv = device_call(sc, q, refs, v, jb)
    assert_same_tail({f: dv[f].cpu().numpy() for f in FIELDS}, want, msg="device entry")
    for f in BASE:
        np.testing.assert_array_equal(bits(dv[f].cpu().numpy()), bits(getattr(base, f)), err_msg=f)
    for with_J1 in (False, True):
        dt = device_call(sc, q, refs, v, jb, with_J1=with_J1, base=False)
        assert_same_tail({f: dt[f].cpu().numpy() for f in FIELDS}, want, msg="device entry, tail alone")
    # one level alone gives its column
    one = call(sc, q, refs, v, jb, levels=(0.9,), want_J1=False)
    assert_same_tail({f: getattr(one, f)[:, 0] for f in FIELDS}, {f: want[f][:, 1] for f in FIELDS})
    return a


# ---------------------------------------------------------------------------------------------
_c4 = {}


def config4_case(D):
    """The config-4 scenario at D draws and twelve of its first 512 candidates (module cache)."""
    from mpct.dtc import config4_candidates, woodberry_mc

    if D not in _c4:
        sc, refs, v, _ = woodberry_mc(draws=D, n2_max=30, nu_max=10, nit=200)
        pool = dict(zip(("N2", "Nu", "d", "l"), (a[:512] for a in config4_candidates(10000))))
        q, jb = choose(sc, pool, refs, v)
        _c4[D] = (sc, refs, v, q, jb)
    return _c4[D]


@pytest.mark.parametrize("D", [5, 32, 128, 129])
def test_config4(gpu, D):
    """Fused route at D = 5, 32 and 128 (the record array at its cap), the generic route's
    fall-through at D = 129."""
    from mpct.engine import robust_instance

    sc, refs, v, q, jb = config4_case(D)
    assert robust_instance(sc) == "dtc_robust_kernel<16> + dtc_robust_kernel<32>"
    assert (2 * q["Nu"] > 16).any() and (2 * q["Nu"] <= 16).any()     # both QP-size classes
    check_case(sc, q, refs, v, jb)


def test_config4_sentinels(gpu):
    """A sentinel (N2 = 0) and a bad horizon in the batch: NaN, NaN, -1 on both routes' records, the
    neighbours' bits unchanged."""
    from test_robust_gpu import with_invalid

    for D in (5, 129):
        sc, refs, v, q, jb = config4_case(D)
        a = call(sc, q, refs, v, jb, want_J1=False)
        qs = with_invalid(q["N2"], q["Nu"], q["d"], q["l"], (3, 7))
        s = call(sc, qs, refs, v, jb, want_J1=False)
        keep = np.array([k for k in range(14) if k not in (3, 7)])
        for k in (3, 7):
            assert np.all(np.isnan(s.quantile[k])) and np.all(np.isnan(s.cvar[k])) and np.all(s.q_draw[k] == -1)
        assert s.status[3] == 8 and s.status[7] == 16
        assert_same_tail({f: getattr(s, f)[keep] for f in FIELDS}, tail_of(a))


def test_shell3x3_mc_generic(gpu):
    """Generic route: gpc_small_kernel's plant-variant instance + robust_reduce_kernel +
    robust_tail_kernel, twelve of 64 grid candidates x 4 model-error draws at nit = 120."""
    from mpct.engine import robust_instance
    from mpct.scenarios import candidate_grid, shell3x3_mc

    made = shell3x3_mc(draws=4, nit=120)
    sc, refs = made[0], np.ascontiguousarray(made[1])
    assert refs.shape[0] == 4
    assert "robust_reduce_kernel" in robust_instance(sc)
    pool = dict(zip(("N2", "Nu", "d", "l"), candidate_grid(64)))
    q, jb = choose(sc, pool, refs, None)
    check_case(sc, q, refs, None, jb)


# ---------------------------------------------------------------------------------------------
def test_generic_batch_in_dispatch_order(gpu):
    """Shell 3x3, 320 grid candidates and two invalid ones x 3 step references: the per-simulation
    kernel runs in dispatch order into the caller's sample or the robust scratch; the tail record is
    the yardstick's on eval_batch's sample either way, and the same reversed."""
    sc, q, refs = shell_large(320, (100, 301))
    Cn = len(q["N2"])
    assert Cn == 322
    J1, st = per_sim(sc, q["N2"], q["Nu"], q["d"], q["l"], refs, None)
    J = totals(J1, st)
    jb = float(np.median(J[np.isfinite(J)]))
    want = tail_ref(J1, st, jb, LEVELS)
    assert want["n"][100] == 0 and want["n"][301] == 0
    assert ((want["n"] > 0) & (want["n"] < 3)).sum() >= 3
    a = call(sc, q, refs, None, jb)
    np.testing.assert_array_equal(bits(a.J1.reshape(J1.shape)), bits(J1))
    assert_same_tail(tail_of(a), want)
    assert_same_tail(tail_of(call(sc, q, refs, None, jb, want_J1=False)), want, msg="scratch")
    r = call(sc, rows(q, np.arange(Cn)[::-1]), refs, None, jb, want_J1=False)
    assert_same_tail({f: getattr(r, f)[::-1] for f in FIELDS}, want, msg="reversed")
    np.testing.assert_array_equal(a.q_draw[:, 2], a.worst_draw)


def test_fused_batch_where_workgroups_stride(gpu):
    """Config 4 at D = 5 with more than 2 * 4 * CUs candidates in the lower class and more than
    2 * 3 * CUs above (tests/test_robust_gpu.py large_config4_batch): the fused kernels stride, the
    classifier runs several passes, a dispatch order exists.  The tail record is the yardstick's on
    eval_batch's sample; the base record is eval_robust's; with and without a caller's J1; 24
    candidates in two twelve-candidate calls carry the large call's bits."""
    import torch
    from mpct.dtc import woodberry_mc
    from mpct.engine import eval_robust

    ncu = torch.cuda.get_device_properties(0).multi_processor_count
    sc, refs, v, _ = woodberry_mc(draws=5, n2_max=30, nu_max=10, nit=200)
    q, g16, g32 = large_config4_batch(ncu)
    Cn, D = len(q["N2"]), 5
    assert Cn > 2 * 4 * ncu
    J1, st = per_sim(sc, q["N2"], q["Nu"], q["d"], q["l"], refs, v)
    J = totals(J1, st)
    jb = float(np.median(J[np.isfinite(J)]))
    want = tail_ref(J1, st, jb, LEVELS)
    assert ((want["n"] > 0) & (want["n"] < D)).sum() >= 3
    a = call(sc, q, refs, v, jb)
    print("C = %d: the J1 sample is bitwise eval_batch's: %s" % (
        Cn, bool(np.array_equal(bits(a.J1.reshape(J1.shape)), bits(J1)))))
    np.testing.assert_array_equal(bits(a.J1.reshape(J1.shape)), bits(J1))
    assert_same_tail(tail_of(a), want)
    same_bits(a, eval_robust(sc, q["N2"], q["Nu"], q["d"], q["l"], refs, v=v, j_bound=jb, want_J1=True), BASE)
    assert_same_tail(tail_of(call(sc, q, refs, v, jb, want_J1=False)), want, msg="scratch")
    dv = device_call(sc, q, refs, v, jb, with_J1=False)
    assert_same_tail({f: dv[f].cpu().numpy() for f in FIELDS}, want, msg="device entry")
    pick = np.sort(np.random.default_rng(24).choice(Cn, 24, replace=False))
    for part in range(2):
        sel = pick[part::2]
        s = call(sc, rows(q, sel), refs, v, jb, want_J1=False)
        assert_same_tail(tail_of(s), {f: want[f][sel] for f in FIELDS}, msg="twelve-candidate call")


def test_entries_interleaved_across_a_regrow(gpu):
    """Tail, eval_robust and eval_batch calls alternate on one scenario (one staging blob, one signal
    cache, one robust scratch, one stream): 5 candidates, then 40 (the blob regrows), then 5 again;
    each call is held to a fresh scenario's bits."""
    import band_mismatch_ref as bm
    from mpct.engine import eval_batch, eval_robust

    _, V = bm.synthetic_plants()
    r, v, _ = bm.synthetic_signals()
    sig = np.stack([2.0 * r, -r]), np.stack([0.25 * v, v])
    cands = list(bm.SYN_CANDS) + [(9, 2, np.array([0.2, 0.0]), np.array([0.7])), (12, 1, np.array([1.0, 1.0]), np.array([0.01]))]

    def args(rep):
        c = cands[:5] * rep
        return ([x[0] for x in c], [x[1] for x in c], np.array([x[2] for x in c]), np.array([x[3] for x in c]))

    def tail(sc, rep, want_J1):
        return eval_robust(sc, *args(rep), sig[0].copy(), v=sig[1].copy(), want_J1=want_J1, levels=LEVELS)

    def robust(sc, rep):
        return eval_robust(sc, *args(rep), sig[0].copy(), v=sig[1].copy(), want_J1=True)

    def batch(sc, rep):
        return eval_batch(sc, *args(rep), sig[0].copy(), v=sig[1].copy())

    sc = bm.synthetic_scenario(V)
    got = [tail(sc, 1, False), batch(sc, 1), robust(sc, 1), tail(sc, 8, True), batch(sc, 8), tail(sc, 1, True),
           robust(sc, 8), tail(sc, 8, False)]
    fresh = [tail(bm.synthetic_scenario(V), 1, True), batch(bm.synthetic_scenario(V), 1),
             robust(bm.synthetic_scenario(V), 1), tail(bm.synthetic_scenario(V), 8, True),
             batch(bm.synthetic_scenario(V), 8)]
    J1 = fresh[1].J1.reshape(5, 2, -1)
    want = tail_ref(J1, fresh[1].status.reshape(5, 2), 0.0, LEVELS)
    assert_same_tail(tail_of(fresh[0]), want)
    assert len(set(want["q_draw"].ravel().tolist())) == 2      # both draws are selected somewhere
    for k, f in ((0, 0), (5, 0), (3, 3), (7, 3)):
        assert_same_tail(tail_of(got[k]), tail_of(fresh[f]), msg="call %d" % k)
        same_bits(got[k], fresh[f], RECORD)
    same_bits(got[5], fresh[0], BASE)
    same_bits(got[3], fresh[3], BASE)
    for k, f in ((2, 2), (6, 3)):
        same_bits(got[k], fresh[f], BASE)
    for k, f in ((1, 1), (4, 4)):
        same_bits(got[k], fresh[f], ("J1", "j21", "j22", "Jnu", "status", "qp_iters"))
