"""CPU: the tail statistics of robust scoring (include/mpct.h: mpct_eval_robust_tail,
mpct_eval_robust_tail_device).  The yardstick tests/tail_ref.py keeps the contract's identities on
seeded records, the comparison helper tells a tail summed out of order and a q_draw moved to a tied
neighbour from the record, both entries return their argument errors in the header's order before
any device is touched, and the exports exist.  No kernel runs here."""
import ctypes as C
import math
import os

import numpy as np
import pytest

from tail_ref import assert_same_tail, tail_ref

EINVAL, EDEVICE, ERANGE = -1, -3, -4


def _records(seed, Cn, D, my):
    """Seeded records with ties (totals on a coarse grid), failed draws of every kind and a
    never-simulated candidate."""
    rng = np.random.default_rng(seed)
    J1 = rng.integers(1, 6, (Cn, D, my)).astype(np.float64) / 4.0
    st = np.where(rng.random((Cn, D)) < 1 / 8, rng.choice([1, 2, 4, 128], (Cn, D)), 0).astype(np.int32)
    bad = rng.random((Cn, D)) < 1 / 16
    J1[bad, 0] = rng.choice([math.nan, math.inf, 1e6], int(bad.sum()))
    st[Cn - 1, D // 2] |= 8
    return J1, st


def test_level_one_is_the_maximum_and_worst_draw():
    """At level 1.0 quantile = cvar = the largest surviving J and q_draw = robust_reduce's worst_draw
    (lowest index among equal maxima: the reason for the descending tie-break)."""
    from test_robust_reduce_gpu import reduce_ref

    ties = 0
    for seed, (Cn, D, my) in enumerate([(9, 1, 1), (9, 7, 2), (9, 64, 3), (9, 130, 7)]):
        J1, st = _records(seed, Cn, D, my)
        t = tail_ref(J1, st, 100.0, [1.0])
        r = reduce_ref(J1, st, 100.0)
        np.testing.assert_array_equal(t["q_draw"][:, 0], r["worst_draw"])
        np.testing.assert_array_equal(t["n"], np.where(r["status"] & 24, 0, D - r["n_failed"]))
        for c in range(Cn):
            Js = [sum(J1[c, k].tolist()) for k in range(D)]
            surv = [k for k in range(D) if st[c, k] == 0 and math.isfinite(Js[k]) and Js[k] <= 100.0]
            if np.bitwise_or.reduce(st[c]) & 24:
                surv = []
            if not surv:
                assert math.isnan(t["quantile"][c, 0]) and math.isnan(t["cvar"][c, 0]) and t["q_draw"][c, 0] == -1
                continue
            top = max(Js[k] for k in surv)
            assert t["quantile"][c, 0] == top and t["cvar"][c, 0] == top
            ties += sum(Js[k] == top for k in surv) > 1
    assert ties > 0   # the tie-break was exercised


def test_duplicate_and_unsorted_levels():
    J1, st = _records(5, 6, 33, 2)
    lv = [0.9, 0.5, 0.9, 1.0, 0.1, 0.5]
    t = tail_ref(J1, st, 0.0, lv)
    for f in ("quantile", "cvar", "q_draw"):
        np.testing.assert_array_equal(t[f][:, 0].view(np.int64 if f != "q_draw" else np.int32),
                                      t[f][:, 2].view(np.int64 if f != "q_draw" else np.int32))
        np.testing.assert_array_equal(t[f][:-1, 1], t[f][:-1, 5])
    for j, a in enumerate(lv):   # a column depends on its own level only
        one = tail_ref(J1, st, 0.0, [a])
        assert_same_tail({f: one[f][:, 0] for f in ("quantile", "cvar", "q_draw")},
                         {f: t[f][:, j] for f in ("quantile", "cvar", "q_draw")})
    assert np.all(t["quantile"][:-1, 4] <= t["quantile"][:-1, 1]) and np.all(t["quantile"][:-1, 1] <= t["quantile"][:-1, 3])
    assert np.all(t["cvar"][:-1] >= t["quantile"][:-1])


def test_rank_is_ceil_of_the_double_product():
    """m = ceil(a * (double)n): a * n exact at 0.5 and even n (the quantile is J_(n/2), not the next),
    one above for nextafter(0.5, 1); 1e-300 clamps to rank 1; k / 7 at n = 7 follows the double
    product, whatever it rounds to."""
    J1 = np.arange(1.0, 9.0).reshape(1, 8, 1)
    t = tail_ref(J1, None, 0.0, [0.5, math.nextafter(0.5, 1.0), 1e-300, 1.0])
    assert t["quantile"][0].tolist() == [4.0, 5.0, 1.0, 8.0]
    assert t["q_draw"][0].tolist() == [3, 4, 0, 7]
    assert t["cvar"][0].tolist() == [(4.0 + 5 + 6 + 7 + 8) / 5, (5.0 + 6 + 7 + 8) / 4, 36.0 / 8, 8.0]
    J7 = np.arange(1.0, 8.0).reshape(1, 7, 1)
    for k in range(1, 8):
        t = tail_ref(J7, None, 0.0, [k / 7])
        assert t["quantile"][0, 0] == float(math.ceil((k / 7) * 7.0))


def test_helper_rejects_a_tail_summed_out_of_order_and_a_tied_neighbour():
    """One large term among small ones: adding it first instead of last changes the sum's bits, and
    the helper sees it; draws 1 and 2 tie at the median, the contract picks the HIGHER index (the
    lower rank goes to the higher index), and the helper rejects the neighbour."""
    rows = [0.1, 0.3, 0.3, 0.7, 1e16, 2.0, 3.0]
    J1 = np.array(rows).reshape(1, 7, 1)
    want = tail_ref(J1, None, 0.0, [0.4, 0.1])          # ranks ceil(2.8) = 3 and ceil(0.7) = 1 of n = 7
    assert want["q_draw"][0].tolist() == [1, 0]       # ranks: 0.1 (k0), 0.3 (k2), 0.3 (k1), ..
    assert want["quantile"][0, 0] == 0.3
    assert_same_tail(want, {f: want[f].copy() for f in want})
    seq = 0.0
    for x in (0.3, 0.7, 2.0, 3.0, 1e16):
        seq += x
    other = 1e16
    for x in (0.3, 0.7, 2.0, 3.0):
        other += x
    assert want["cvar"][0, 0] == seq / 5 and other / 5 != seq / 5
    wrong = {f: want[f].copy() for f in want}
    wrong["cvar"][0, 0] = other / 5
    with pytest.raises(AssertionError):
        assert_same_tail(wrong, want)
    wrong = {f: want[f].copy() for f in want}
    wrong["q_draw"][0, 0] = 2                          # the tied neighbour: the same J, another draw
    with pytest.raises(AssertionError):
        assert_same_tail(wrong, want)
    wrong = {f: want[f].copy() for f in want}
    wrong["quantile"][0, 1] = math.nextafter(0.1, 1.0)   # one ulp off
    with pytest.raises(AssertionError):
        assert_same_tail(wrong, want)


def test_exports_exist(built):
    from mpct import _lib

    lib = _lib.load()
    so = C.CDLL(_lib.lib_path())
    for f in ("mpct_eval_robust_tail", "mpct_eval_robust_tail_device"):
        assert f in _lib.EXPORTS
        assert hasattr(lib, f)
        assert C.cast(getattr(so, f), C.c_void_p).value
    assert C.cast(so.mpct_internal_robust_tail, C.c_void_p).value and "mpct_internal_robust_tail" not in _lib.EXPORTS
    assert lib.mpct_abi_version() == 7   # additions to ABI 7, no version change
    assert (_lib.TAIL_MAX_LEVELS, _lib.TAIL_MAX_DRAWS) == (8, 4096)
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "mpct.h")).read()
    assert "#define MPCT_TAIL_MAX_LEVELS 8" in hdr and "#define MPCT_TAIL_MAX_DRAWS 4096" in hdr


def _call(sc, refs, v, entry="host", nlev=2, levels=(0.5, 1.0), j_bound=0.0, nref=None, open_loop=0, want_traj=0,
          base=True, tail=True, null_out=False, null_tail=False, null_levels=False, null_scenario=False):
    """One call of a tail entry with host buffers (nothing valid reaches a device here: either an
    argument error returns first, or there is no device)."""
    from mpct import _lib

    lib = _lib.load()
    N2 = np.array([10, 8], np.int32)
    Nu = np.array([3, 2], np.int32)
    d = np.ones((2, sc.my))
    lam = np.ones((2, sc.nu))
    refs = np.ascontiguousarray(refs, dtype=float)
    v = np.ascontiguousarray(v, dtype=float)
    mean = np.zeros((2, sc.my))
    q = np.zeros((2, 8))
    qd = np.zeros((2, 8), np.int32)
    r = _lib.MpctRobustResult()
    if base:
        r.mean = mean.ctypes.data_as(_lib.c_double_p)
    t = _lib.MpctRobustTail()
    if tail:
        t.quantile = q.ctypes.data_as(_lib.c_double_p)
        t.q_draw = qd.ctypes.data_as(_lib.c_int32_p)
    lv = np.ascontiguousarray(levels, dtype=np.float64)
    o = _lib.MpctOpts(open_loop, want_traj, 0, -1, 0.0)
    args = [None if null_scenario else sc.handle, 2, N2.ctypes.data, Nu.ctypes.data, d.ctypes.data, lam.ctypes.data,
            refs.shape[0] if nref is None else nref, refs.ctypes.data, v.ctypes.data, float(j_bound), C.byref(o), nlev,
            None if null_levels else lv.ctypes.data_as(_lib.c_double_p), None if null_out else C.byref(r),
            None if null_tail else C.byref(t)]
    if entry == "host":
        rc = lib.mpct_eval_robust_tail(*args)
    else:
        rc = lib.mpct_eval_robust_tail_device(*(args + [None]))
    return rc, _lib.last_error()


@pytest.fixture(scope="module")
def mc3(built):
    from mpct.dtc import woodberry_mc

    return woodberry_mc(draws=3, n2_max=10, nu_max=5)[:3]


@pytest.mark.parametrize("entry", ["host", "device"])
def test_einval_cases_in_order(mc3, entry):
    """Every argument error is MPCT_EINVAL with a message, the same with and without a GPU.  Each
    case also carries every error that the header lists AFTER its own, so the message shows the
    order: nlev, levels NULL, a bad level, no result pointer, then mpct_eval_robust's checks."""
    sc, refs, v = mc3
    later = [dict(open_loop=1, j_bound=-1.0), dict(base=False, tail=False), dict(levels=(0.5, math.nan)),
             dict(null_levels=True)]
    cases = [(dict(nlev=0), "nlev", 4), (dict(nlev=-1), "nlev", 4), (dict(nlev=9, levels=(0.5,) * 9), "nlev", 3),
             (dict(null_levels=True), "null levels", 3),
             (dict(levels=(0.5, math.nan)), "level", 2), (dict(levels=(0.0, 1.0)), "level", 2),
             (dict(levels=(-0.5, 1.0)), "level", 2), (dict(levels=(1.0, math.nextafter(1.0, 2.0))), "level", 2),
             (dict(levels=(math.inf, 1.0)), "level", 2),
             (dict(base=False, tail=False), "NULL", 1), (dict(null_out=True, null_tail=True), "NULL", 1),
             (dict(null_out=True, tail=False), "NULL", 1), (dict(base=False, null_tail=True), "NULL", 1),
             (dict(open_loop=1), "cost-only", 0), (dict(want_traj=1), "cost-only", 0), (dict(nref=0), "nref", 0),
             (dict(j_bound=-1.0), "j_bound", 0), (dict(j_bound=math.nan), "j_bound", 0),
             (dict(null_scenario=True), "scenario", 0)]
    for kw, word, nlater in cases:
        rc, msg = _call(sc, refs, v, entry=entry, **kw)
        assert rc == EINVAL and word in msg, (kw, rc, msg)
        for extra in later[:nlater]:   # a later error beside it does not change the verdict
            both = dict(extra)
            both.update(kw)
            rc, msg = _call(sc, refs, v, entry=entry, **both)
            assert rc == EINVAL and word in msg, (both, rc, msg)


@pytest.mark.parametrize("entry", ["host", "device"])
def test_too_many_draws_is_erange(mc3, entry, has_gpu):
    """D = 4097 is MPCT_ERANGE, after the argument errors and before any device is touched; D = 4096
    passes every check (without a device the call then fails loudly with MPCT_EDEVICE)."""
    sc, refs, v = mc3
    refs_big = np.zeros((4097,) + refs.shape[1:])
    v_big = np.zeros((4097,) + v.shape[1:])
    rc, msg = _call(sc, refs_big, v_big, entry=entry)
    assert rc == ERANGE and "MPCT_TAIL_MAX_DRAWS" in msg, (rc, msg)
    rc, msg = _call(sc, refs_big, v_big, entry=entry, levels=(0.5, 2.0))   # an argument error comes first
    assert rc == EINVAL and "level" in msg
    if not has_gpu:
        rc, msg = _call(sc, refs_big, v_big, entry=entry, nref=4096)
        assert rc == EDEVICE and msg
        rc, msg = _call(sc, refs, v, entry=entry, null_out=True)            # the tail alone is a valid request
        assert rc == EDEVICE and msg
        rc, msg = _call(sc, refs, v, entry=entry, tail=False)               # and so is the base record alone
        assert rc == EDEVICE and msg


def test_python_entries_take_levels(mc3, has_gpu):
    """engine.eval_robust(levels=...) reaches the tail entry: a bad level raises MpctError with the
    library's message; without a GPU a valid call fails loudly (no CPU fallback)."""
    from mpct.engine import MpctError, eval_robust

    sc, refs, v = mc3
    with pytest.raises(MpctError, match=r"mpct_eval_robust_tail failed \(-1\).*level"):
        eval_robust(sc, [10, 8], [3, 2], np.ones((2, 2)), np.ones((2, 2)), refs, v=v, levels=[0.5, 1.5])
    with pytest.raises(MpctError, match=r"nlev"):
        eval_robust(sc, [10, 8], [3, 2], np.ones((2, 2)), np.ones((2, 2)), refs, v=v, levels=[0.5] * 9)
    if not has_gpu:
        with pytest.raises(MpctError, match=r"-3"):
            eval_robust(sc, [10, 8], [3, 2], np.ones((2, 2)), np.ones((2, 2)), refs, v=v, levels=[0.5, 1.0])
