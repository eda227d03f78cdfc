"""CPU: the trajectory envelopes (mpct_envelope, mpct_eval_robust_envelope; include/mpct.h).  The
reference of tests/envelope_ref.py on hand-made columns, and the mistakes it must catch; the exports and the
header; every argument error of the four entries in the header's order (each call also carries every LATER error,
so the message that comes back shows the order of the checks); C = 0; no device; EnvelopeResult.costs and .band.
No kernel runs here."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import draw_stats_ref as R
import envelope_ref as E
from indices_ref import tree64

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, EDEVICE, ERANGE = -1, -3, -4
EXPORTS = ("mpct_envelope_device", "mpct_envelope", "mpct_eval_robust_envelope", "mpct_eval_robust_envelope_device")


def test_reference_on_hand_made_columns():
    nan, inf = math.nan, math.inf
    # one candidate, D = 4 draws, one row, nit = 3 samples: y[0, k, 0, t]
    y = np.array([[[[1.0, 0.0, nan]], [[3.0, -0.0, nan]], [[1.0, 5.0, inf]], [[3.0, 5.0, nan]]]])
    rec, sp = E.envelope_ref(y, None, [0.5, 1.0], t0=0)
    assert rec["n"].shape == (1, 1, 3) and rec["quantile"].shape == (1, 1, 3, 2)
    assert rec["n"][0, 0].tolist() == [4, 4, 0]
    assert rec["lo"][0, 0, :2].tolist() == [1.0, 0.0] and rec["lo_draw"][0, 0].tolist() == [0, 0, -1]
    assert not np.signbit(rec["lo"][0, 0, 1])                       # +0.0 of draw 0, not the -0.0 of draw 1
    assert rec["hi"][0, 0, :2].tolist() == [3.0, 5.0] and rec["hi_draw"][0, 0].tolist() == [1, 2, -1]
    assert rec["mean"][0, 0, 0] == 8.0 / 4.0 and np.isnan(rec["mean"][0, 0, 2])
    # sample 0 in order: (1, k=2) (1, k=0) (3, k=3) (3, k=1): level 0.5 -> rank 2 = draw 0, cvar = (1 + 3 + 3) / 3
    assert rec["q_draw"][0, 0, 0].tolist() == [0, 1] and rec["cvar"][0, 0, 0, 0] == 7.0 / 3.0
    # sample 1: the zeros tie, the higher draw first: rank 2 is draw 0
    assert rec["q_draw"][0, 0, 1].tolist() == [0, 2] and not np.signbit(rec["quantile"][0, 0, 1, 0])
    # the all-dead sample 2 makes the row's spread NaN / -1 from t0 = 0 and leaves it alone from t0 = ... nothing later
    assert np.isnan(sp["spread"][0, 0]) and np.isnan(sp["spread_max"][0, 0]) and sp["t_spread_max"][0, 0] == -1
    rec2, sp2 = E.envelope_ref(y[..., :2], None, [], t0=0)
    assert sp2["spread"][0, 0] == 2.0 + 5.0 and sp2["spread_max"][0, 0] == 5.0 and sp2["t_spread_max"][0, 0] == 1
    _, sp3 = E.envelope_ref(y[..., :2], None, [], t0=1)
    assert sp3["spread"][0, 0] == 5.0 and sp3["t_spread_max"][0, 0] == 1
    # a dead draw leaves every sample of its candidate
    rec4, _ = E.envelope_ref(y[..., :2], np.array([[1, 1, 0, 1]], np.int32), [], t0=0)
    assert rec4["n"][0, 0].tolist() == [3, 3] and rec4["hi_draw"][0, 0].tolist() == [1, 3]
    # the reshape: sample (row, t) is column row * nit + t of the table
    x, alive = R.table(2, 5, 6, 4)
    rec5, _ = E.envelope_ref(x.reshape(2, 5, 2, 3), alive, [0.5])
    st = R.stats_ref(x, alive, [0.5])
    assert (R.bits(rec5["mean"][:, 1, 2]) == R.bits(st["mean"][:, 5])).all()
    assert (rec5["q_draw"][:, 1, 0, 0] == st["q_draw"][:, 3, 0]).all()


def test_spread_order_and_first_maximum():
    """The spread is the lane tree, not a sequential sum, and t_spread_max is the FIRST maximum -- also when the
    two maxima lie in different 64-sample blocks."""
    nit, t0 = 200, 3
    lo, hi = E.spread_rows(nit, t0)
    s, mx, tm = E.spread_row(lo[0], hi[0], t0)
    d = [float(hi[0, t]) - float(lo[0, t]) for t in range(t0, nit)]
    lanes = [0.0] * 64
    for k, v in enumerate(d):
        lanes[k % 64] += v
    assert s == tree64(lanes) and (mx, tm) == (2.0 ** 53, t0)
    seq = 0.0
    for v in d:
        seq += v
    assert seq == 2.0 ** 53 and s > seq                # a sequential sum is another number here
    assert hi[1, 10] - lo[1, 10] == hi[1, 138] - lo[1, 138] == 2.0
    s, mx, tm = E.spread_row(lo[1], hi[1], t0)
    assert mx == 2.0 and tm == 10                       # not 138
    assert E.spread_row(lo[1], hi[1], 11)[2] == 138
    assert (20 - t0) % 64 > (70 - t0) % 64 and E.spread_row(lo[2], hi[2], t0)[1:] == (2.0, 20)   # across lanes


def _planted(kind):
    """draw_stats_ref.stats_ref with one mistake planted"""
    def stats(x, alive, levels):
        g = R.stats_ref(x, alive, levels)
        Cn, D, m = x.shape
        for c in range(Cn):
            for i in range(m):
                live = [k for k in range(D) if (alive is None or alive[c, k]) and math.isfinite(x[c, k, i])]
                if kind == "mean_over_D" and live:
                    acc = 0.0
                    for k in live:
                        acc += float(x[c, k, i])
                    g["mean"][c, i] = acc / float(D)
                if kind == "ties_ascending" and live:
                    order = sorted(live, key=lambda k: (float(x[c, k, i]), k))
                    for j, a in enumerate(levels):
                        r = min(max(math.ceil(a * float(len(live))), 1), len(live))
                        g["q_draw"][c, i, j] = order[r - 1]
                        g["quantile"][c, i, j] = x[c, order[r - 1], i]
        return g
    return stats


def test_planted_mistakes_are_caught():
    x, alive = R.table(3, 6, 2 * 9, 11)
    y = x.reshape(3, 6, 2, 9)
    levels = [0.05, 0.5, 0.95]
    want, wsp = E.envelope_ref(y, alive, levels, t0=2)
    same, ssp = E.envelope_ref(y, alive, levels, t0=2)
    R.assert_same_stats(same, want)
    E.assert_same_spread(ssp, wsp)
    for kind in ("mean_over_D", "ties_ascending"):
        got, _ = E.envelope_ref(y, alive, levels, t0=2, stats=_planted(kind))
        with pytest.raises(AssertionError):
            R.assert_same_stats(got, want)
    # the spread summed sequentially, and the last maximum instead of the first
    t0 = 3
    lo, hi = E.spread_rows(200, t0)
    want, wsp = E.envelope_ref(np.stack([lo, hi])[None], None, [], t0=t0)
    assert (want["lo"][0] == lo).all() and (want["hi"][0] == hi).all() and (wsp["t_spread_max"][0] == [t0, 10, 20]).all()
    seq = {k: v.copy() for k, v in wsp.items()}
    last = {k: v.copy() for k, v in wsp.items()}
    for i in range(3):
        d = [float(hi[i, t]) - float(lo[i, t]) for t in range(t0, 200)]
        acc = 0.0
        for v in d:
            acc += v
        seq["spread"][0, i] = acc
        last["t_spread_max"][0, i] = t0 + max(k for k, v in enumerate(d) if v == max(d))
    assert last["t_spread_max"][0, 1] == 138 and last["t_spread_max"][0, 2] == 70
    for bad in (seq, last):
        with pytest.raises(AssertionError):
            E.assert_same_spread(bad, wsp)


def test_header_declares_and_lib_exports(built):
    from mpct import _lib

    src = open(os.path.join(ROOT, "include", "mpct.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    so = C.CDLL(_lib.lib_path())
    for f in EXPORTS:
        assert re.search(r"\bint32_t %s\s*\(" % f, code), f
        assert f in _lib.EXPORTS
        assert C.cast(getattr(so, f), C.c_void_p).value
    m = re.search(r"typedef struct mpct_envelope_spread \{(.*?)\} mpct_envelope_spread;", code, flags=re.S)
    assert re.findall(r"(double|int32_t)\* (\w+);", m.group(1)) == [
        ("double", "spread"), ("double", "spread_max"), ("int32_t", "t_spread_max")]
    assert [n for n, _ in _lib.MpctEnvelopeSpread._fields_] == list(E.SPREAD)
    for hook in ("mpct_internal_envelope_grid", "mpct_internal_envelope_dlane"):
        assert hook not in src and C.cast(getattr(so, hook), C.c_void_p).value
    assert _lib.load().mpct_abi_version() == 7
    hdr = open(os.path.join(ROOT, "model-predictive-control-tuning_amd", "csrc", "envelope.h")).read()
    assert re.search(r"kEnvDefaultDlane = %d;" % _lib.ENVELOPE_DLANE, hdr)
    for phrase in ("IS mpct_draw_stats", "pairwise tree", "the first t that attains it", "Argument errors",
                   "bitwise independent"):
        assert phrase in src, phrase
    lib = _lib.load()
    assert lib.mpct_internal_envelope_grid(-1) == EINVAL and lib.mpct_internal_envelope_dlane(-1) == EINVAL
    assert lib.mpct_internal_envelope_dlane(_lib.ENVELOPE_LANE_MAX_DRAWS + 1) == EINVAL
    assert lib.mpct_internal_envelope_dlane(_lib.ENVELOPE_LANE_MAX_DRAWS) == 0 and lib.mpct_internal_envelope_dlane(0) == 0


def _bufs(n=4096):
    from mpct import _lib

    buf, ibuf = np.zeros(n), np.zeros(n, dtype=np.int32)
    return buf, ibuf, buf.ctypes.data_as(_lib.c_double_p), ibuf.ctypes.data_as(_lib.c_int32_p)


def test_envelope_argument_errors_in_documented_order(built):
    from mpct import _lib

    lib = _lib.load()
    buf, ibuf, d, i = _bufs(64)
    S, P = _lib.MpctDrawStats, _lib.MpctEnvelopeSpread
    none, band, nolo, lev = S(), S(lo=d, hi=d), S(hi=d, n=i), S(lo=d, hi=d, q_draw=i)
    pnone, psome = P(), P(t_spread_max=i)
    a = buf.ctypes.data
    nanlev, badlev, oklev = np.array([0.5, np.nan]), np.array([0.5, 1.5]), np.array([0.5, 1.0])
    L = lambda v: v.ctypes.data_as(_lib.c_double_p)  # noqa: E731
    big = 1 << 30
    #          y     u     C    D     my  nu nit t0  nlev levels     out_y out_u sp_y   sp_u
    steps = [((None, None, -1, 5000, 4, 4, 4, -1, 9, None, none, None, psome, psome), EINVAL, "bad shape"),
             ((None, None, big, 0, 4, 4, 4, -1, 9, None, none, None, psome, psome), EINVAL, "bad shape"),
             ((None, None, big, 5000, -1, 4, 4, -1, 9, None, none, None, psome, psome), EINVAL, "bad shape"),
             ((None, None, big, 5000, 4, -1, 4, -1, 9, None, none, None, psome, psome), EINVAL, "bad shape"),
             ((None, None, big, 5000, 4, 4, 0, -1, 9, None, none, None, psome, psome), EINVAL, "bad shape"),
             ((None, None, big, 5000, 4, 4, 4, -1, 9, None, none, None, psome, psome), EINVAL, "t0 must lie"),
             ((None, None, big, 5000, 4, 4, 4, 4, 9, None, none, None, psome, psome), EINVAL, "t0 must lie"),
             ((None, None, big, 5000, 4, 4, 4, 3, 9, None, none, None, psome, psome), EINVAL, "nlev must be"),
             ((None, None, big, 5000, 4, 4, 4, 3, -1, None, none, None, psome, psome), EINVAL, "nlev must be"),
             ((None, None, big, 5000, 4, 4, 4, 3, 2, None, none, None, psome, psome), EINVAL, "null levels"),
             ((None, None, big, 5000, 4, 4, 4, 3, 2, L(nanlev), none, None, psome, psome), EINVAL, "every level"),
             ((None, None, big, 5000, 4, 4, 4, 3, 2, L(badlev), none, None, psome, psome), EINVAL, "every level"),
             ((None, None, big, 5000, 4, 4, 4, 3, 2, L(oklev), none, None, psome, psome), EINVAL, "a spread pointer needs"),
             ((None, None, big, 5000, 4, 4, 4, 3, 2, L(oklev), nolo, None, psome, None), EINVAL, "a spread pointer needs"),
             ((None, None, big, 5000, 4, 4, 4, 3, 2, L(oklev), band, None, psome, psome), EINVAL, "a spread pointer needs"),
             ((None, None, big, 5000, 4, 4, 4, 3, 2, L(oklev), none, None, pnone, None), EINVAL, "every output pointer"),
             ((None, None, big, 5000, 4, 4, 4, 3, 2, L(oklev), None, None, None, None), EINVAL, "every output pointer"),
             ((None, None, big, 5000, 4, 4, 4, 3, 0, None, lev, None, psome, None), EINVAL, "need nlev >= 1"),
             ((None, None, big, 5000, 4, 4, 4, 3, 0, None, band, lev, psome, psome), EINVAL, "need nlev >= 1"),
             ((None, None, big, 5000, 4, 4, 4, 3, 2, L(oklev), lev, None, psome, None), EINVAL, "out_y needs"),
             ((a, None, big, 5000, 0, 4, 4, 3, 2, L(oklev), lev, None, psome, None), EINVAL, "out_y needs"),
             ((a, None, big, 5000, 4, 4, 4, 3, 2, L(oklev), lev, band, psome, psome), EINVAL, "out_u needs"),
             ((a, a, big, 5000, 4, 0, 4, 3, 2, L(oklev), lev, band, psome, psome), EINVAL, "out_u needs"),
             ((a, a, big, 5000, 4, 4, 4, 3, 2, L(oklev), lev, band, psome, psome), ERANGE, "MPCT_TAIL_MAX_DRAWS"),
             ((a, a, big, 4097, 4, 4, 4, 3, 1, L(oklev), band, None, None, None), ERANGE, "MPCT_TAIL_MAX_DRAWS"),
             ((a, a, big, 5000, 4, 4, 4, 3, 0, None, band, band, psome, psome), ERANGE, "MPCT_INDEX_MAX_ROWS"),
             ((a, a, big, 4096, 1, 4, 4, 3, 2, L(oklev), lev, band, psome, psome), ERANGE, "MPCT_INDEX_MAX_ROWS"),
             ((a, None, 1 << 28, 1, 2, 0, 4, 0, 0, None, band, None, None, None), ERANGE, "MPCT_INDEX_MAX_ROWS")]
    ref = lambda s: C.byref(s) if s is not None else None  # noqa: E731
    for args, code, msg in steps:
        y, u, C_, D, my, nu, nit, t0, nlev, lv, oy, ou, sy, su = args
        for rc in (lib.mpct_envelope_device(y, u, None, C_, D, my, nu, nit, t0, nlev, lv, ref(oy), ref(ou), ref(sy), ref(su), None),
                   lib.mpct_envelope(y, u, None, C_, D, my, nu, nit, t0, nlev, lv, -1, ref(oy), ref(ou), ref(sy), ref(su))):
            assert rc == code, (args[2:9], msg, rc, _lib.last_error())
            assert msg in _lib.last_error(), (args[2:9], msg, _lib.last_error())
    # C = 0 is fine without trajectories and without a device, and writes nothing
    assert lib.mpct_envelope_device(None, None, None, 0, 4, 2, 2, 5, 0, 2, L(oklev), ref(lev), ref(band), ref(psome), None, None) == 0
    assert lib.mpct_envelope(None, None, None, 0, 4, 2, 0, 5, 4, 0, None, -1, ref(band), None, ref(psome), None) == 0
    assert (buf == 0).all() and (ibuf == 0).all()


@pytest.fixture(scope="module")
def small_scenario(built):
    from mpct.scenarios import shell3x3

    sc, r, _ = shell3x3(n2_max=10, nu_max=3, nit=40)
    yield sc, r
    sc.close()


def test_eval_robust_envelope_argument_errors_in_documented_order(small_scenario):
    from mpct import _lib

    sc, r = small_scenario
    lib = _lib.load()
    buf, ibuf, d, i = _bufs()
    N2, Nu = np.array([5, 6], dtype=np.int32), np.array([2, 2], dtype=np.int32)
    dl, lm = np.ones((2, 3)), np.ones((2, 3))
    refs = np.ascontiguousarray(r[None])
    O, S, B, P = _lib.MpctOpts, _lib.MpctDrawStats, _lib.MpctRobustResult, _lib.MpctEnvelopeSpread
    ol, cl = O(1, 0, 0, -1, 0.0), O(0, 0, 0, -1, 0.0)
    none, band, nohi, lev = S(), S(lo=d, hi=d), S(lo=d, mean=d), S(lo=d, hi=d, cvar=d)
    bnone, bj1, bsome = B(), B(J1=d), B(n_failed=i)
    pnone, psome = P(), P(spread=d)
    nanlev, oklev = np.array([0.5, np.nan]), np.array([0.5, 1.0])
    manyrefs = 5000
    ref = lambda s: C.byref(s) if s is not None else None  # noqa: E731

    def call(h, C_, nref, refs_p, jb, opts, t0, nlev, lv, base, oy, ou, sy, su):
        a = [h, C_, N2.ctypes.data, Nu.ctypes.data, dl.ctypes.data, lm.ctypes.data, nref, refs_p, None, jb, ref(opts), t0, nlev,
             lv.ctypes.data_as(_lib.c_double_p) if lv is not None else None, ref(base), ref(oy), ref(ou), ref(sy), ref(su)]
        return lib.mpct_eval_robust_envelope(*a), lib.mpct_eval_robust_envelope_device(*(a + [None]))

    rp = refs.ctypes.data
    h = sc.handle
    #         h     C  nref  refs  j_bound opts t0 nlev lv     base  out_y out_u sp_y  sp_u
    steps = [((None, -1, 0, None, -1.0, ol, 40, 9, None, bj1, none, None, psome, None), EINVAL, "null scenario"),
             ((h, -1, 0, None, -1.0, ol, 40, 9, None, bj1, none, None, psome, None), EINVAL, "open_loop must be 0"),
             ((h, -1, 0, None, -1.0, cl, 40, 9, None, bj1, none, None, psome, None), EINVAL, "nref < 1"),
             ((h, -1, manyrefs, None, -1.0, cl, 40, 9, None, bj1, none, None, psome, None), EINVAL, "j_bound must be"),
             ((h, -1, manyrefs, None, np.nan, None, 40, 9, None, bj1, none, None, psome, None), EINVAL, "j_bound must be"),
             ((h, -1, manyrefs, None, 0.0, cl, 40, 9, None, bj1, none, None, psome, None), EINVAL, "t0 must lie"),
             ((h, -1, manyrefs, None, np.inf, cl, -1, 9, None, bj1, none, None, psome, None), EINVAL, "t0 must lie"),
             ((h, -1, manyrefs, None, 0.0, cl, 39, 9, None, bj1, none, None, psome, None), EINVAL, "nlev must be"),
             ((h, -1, manyrefs, None, 0.0, cl, 39, 2, None, bj1, none, None, psome, None), EINVAL, "null levels"),
             ((h, -1, manyrefs, None, 0.0, cl, 39, 2, nanlev, bj1, none, None, psome, None), EINVAL, "every level"),
             ((h, -1, manyrefs, None, 0.0, cl, 39, 2, oklev, bj1, none, None, psome, None), EINVAL, "a spread pointer needs"),
             ((h, -1, manyrefs, None, 0.0, cl, 39, 2, oklev, bj1, band, nohi, None, psome), EINVAL, "a spread pointer needs"),
             ((h, -1, manyrefs, None, 0.0, cl, 39, 2, oklev, bnone, none, None, pnone, None), EINVAL, "every output pointer"),
             ((h, -1, manyrefs, None, 0.0, cl, 39, 2, oklev, None, None, None, None, None), EINVAL, "every output pointer"),
             ((h, -1, manyrefs, None, 0.0, cl, 39, 0, None, bj1, lev, None, psome, None), EINVAL, "base->J1 must be NULL"),
             ((h, -1, manyrefs, None, 0.0, cl, 39, 0, None, bsome, lev, None, psome, None), EINVAL, "need nlev >= 1"),
             ((h, -1, manyrefs, None, 0.0, cl, 39, 2, oklev, bsome, lev, None, psome, None), EINVAL, "C < 0 or nref < 1"),
             ((h, 2, manyrefs, None, 0.0, cl, 39, 2, oklev, None, lev, band, psome, psome), EINVAL, "null input pointer"),
             ((h, 2, manyrefs, rp, 0.0, cl, 39, 2, oklev, bsome, None, None, None, None), ERANGE, "MPCT_TAIL_MAX_DRAWS"),
             ((h, 1 << 25, 1, rp, 0.0, None, 0, 0, None, bsome, band, None, None, None), ERANGE, "MPCT_INDEX_MAX_ROWS")]
    for args, code, msg in steps:
        for rc in call(*args):
            assert rc == code, (msg, rc, _lib.last_error())
            assert msg in _lib.last_error(), (msg, _lib.last_error())
    # C = 0 needs no device and writes nothing
    for rc in call(h, 0, 1, rp, 0.0, cl, 0, 2, oklev, bsome, lev, band, psome, psome):
        assert rc == 0, _lib.last_error()
    assert (buf == 0).all() and (ibuf == 0).all()


def test_empty_batch_and_no_device(small_scenario, has_gpu):
    from mpct.engine import MpctError, envelope, eval_robust_envelope

    sc, r = small_scenario
    # an empty batch and empty trajectories need no device
    res = eval_robust_envelope(sc, np.zeros(0, dtype=np.int32), np.zeros(0, dtype=np.int32), np.zeros((0, 3)),
                               np.zeros((0, 3)), np.stack([r, r]), levels=[0.05, 0.95], t0=3)
    assert res.y["lo"].shape == (0, 3, 40) and res.u["cvar"].shape == (0, 3, 40, 2) and res.y["n"].dtype == np.int32
    assert res.spread["u"]["t_spread_max"].shape == (0, 3) and res.base.n_failed.shape == (0,) and res.t0 == 3
    empty = envelope(np.zeros((0, 4, 2, 7)), None)
    assert empty.u is None and "u" not in empty.spread and empty.y["hi_draw"].shape == (0, 2, 7) and "quantile" not in empty.y
    with pytest.raises(ValueError):
        envelope(None, None)
    with pytest.raises(ValueError):
        envelope(np.zeros((1, 4, 2, 7)), np.zeros((1, 4, 2, 8)))
    if not has_gpu:
        x, alive = R.table(2, 5, 6, 3)
        with pytest.raises(MpctError, match=r"\(-3\).*HIP device"):
            envelope(x.reshape(2, 5, 2, 3), None, alive, levels=[0.5])
        with pytest.raises(MpctError, match=r"\(-3\).*(GPU|HIP device)"):
            eval_robust_envelope(sc, [5, 6], [2, 2], np.ones((2, 3)), np.ones((2, 3)), np.stack([r, r]))


def test_envelope_result_costs_and_band():
    from mpct.engine import EnvelopeResult, RobustResult

    Cn, nit = 3, 5
    line = np.arange(Cn * 2 * nit, dtype=float).reshape(Cn, 2, nit)
    q = np.stack([line + 0.25, line + 0.75], axis=3)
    y = {"lo": line, "hi": line + 1.0, "quantile": q}
    sp = {"y": {"spread": np.arange(6.0).reshape(Cn, 2), "spread_max": np.ones((Cn, 2)), "t_spread_max": np.full((Cn, 2), 4, np.int32)},
          "u": {"spread": 10.0 + np.arange(3.0).reshape(Cn, 1), "spread_max": np.ones((Cn, 1)), "t_spread_max": np.zeros((Cn, 1), np.int32)}}
    base = RobustResult(mean=np.zeros((Cn, 2)), worst=np.zeros((Cn, 2)), n_failed=np.array([0, 2, 1], np.int32),
                        worst_draw=np.zeros(Cn, np.int32), status=np.zeros(Cn, np.int32), draws=4)
    res = EnvelopeResult(y=y, u=None, spread=sp, levels=np.array([0.05, 0.95]), base=base)
    got = res.costs(("spread", "t_spread_max"))
    assert got.shape == (3, 6) and got.dtype == np.float64
    np.testing.assert_array_equal(got[1], [2.0, 3.0, 11.0, 4.0, 4.0, 0.0])
    np.testing.assert_array_equal(res.costs(("spread",), sides=("u",))[:, 0], [10.0, 11.0, 12.0])
    masked = res.costs(("spread",), max_failed=1)
    assert np.isnan(masked[1]).all() and not np.isnan(masked[[0, 2]]).any()
    got[0, 0] = -1.0
    assert sp["y"]["spread"][0, 0] == 0.0              # a copy, not a view
    with pytest.raises(ValueError):
        res.costs(("width",))
    lo, hi = res.band(2, 1)
    np.testing.assert_array_equal(lo, line[2, 1])
    np.testing.assert_array_equal(hi, line[2, 1] + 1.0)
    lo, hi = res.band(2, 1, 0.05, 0.95)
    np.testing.assert_array_equal(lo, line[2, 1] + 0.25)
    np.testing.assert_array_equal(hi, line[2, 1] + 0.75)
    with pytest.raises(ValueError):
        res.band(0, 0, 0.5, None)
    with pytest.raises(ValueError):
        res.band(0, 0, side="u")
