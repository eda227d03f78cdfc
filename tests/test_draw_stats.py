"""CPU: the draw statistics (mpct_draw_stats, mpct_eval_robust_indices; include/mpct.h).  The
reference of tests/draw_stats_ref.py on hand-made columns and against the existing yardstick tail_ref.py; the
exports and the header; every argument error of the four entries in the header's order (each call also carries
every LATER error, so the message that comes back shows the order of the checks); C = 0; no device; the
masking of RobustIndexResult.costs.  No kernel runs here."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import draw_stats_ref as R
import tail_ref as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, EDEVICE, ERANGE = -1, -3, -4
EXPORTS = ("mpct_draw_stats_device", "mpct_draw_stats", "mpct_eval_robust_indices", "mpct_eval_robust_indices_device")


def test_reference_on_hand_made_columns():
    nan, inf = math.nan, math.inf
    #            k:  0     1     2     3     4     5
    x = np.array([[[3.0, nan, 1.0, 1.0, 3.0, inf],       # column 0: ties at both ends, a NaN and an inf
                   [0.0, -0.0, 5.0, 5.0, -0.0, 2.0]]]).transpose(0, 2, 1).copy()
    alive = np.array([[1, 1, 1, 1, 1, 1]], np.int32)
    g = R.stats_ref(x, alive, [1.0, 0.5, 0.01, 0.5])
    assert g["n"].tolist() == [[4, 6]]
    assert g["mean"][0, 0] == (3.0 + 1.0 + 1.0 + 3.0) / 4.0 and g["mean"][0, 1] == 12.0 / 6.0
    assert g["lo"][0].tolist() == [1.0, 0.0] and g["lo_draw"][0].tolist() == [2, 0]
    assert not np.signbit(g["lo"][0, 1])                 # +0.0 at draw 0 keeps its bits against -0.0 at 1 and 4
    assert g["hi"][0].tolist() == [3.0, 5.0] and g["hi_draw"][0].tolist() == [0, 2]
    # order of column 0: (1, k=3) (1, k=2) (3, k=4) (3, k=0); level 0.5 -> rank 2, level 0.01 -> rank 1
    assert g["q_draw"][0, 0].tolist() == [0, 2, 3, 2]
    assert g["quantile"][0, 0].tolist() == [3.0, 1.0, 1.0, 1.0]
    assert g["cvar"][0, 0].tolist() == [3.0, (1.0 + 3.0 + 3.0) / 3.0, 8.0 / 4.0, (1.0 + 3.0 + 3.0) / 3.0]
    # level 1.0 is hi / hi_draw; duplicate levels give equal columns
    assert (g["quantile"][..., 0] == g["hi"]).all() and (g["cvar"][..., 0] == g["hi"]).all()
    assert (g["q_draw"][..., 0] == g["hi_draw"]).all()
    for f in R.LEVEL:
        assert (R.bits(g[f][..., 1]) == R.bits(g[f][..., 3])).all()
    # the zeros: rank 1 of column 1 is the highest draw among the equal zeros, -0.0 at draw 4
    assert g["q_draw"][0, 1, 2] == 4 and np.signbit(g["quantile"][0, 1, 2])
    # a dead draw leaves every column of its candidate; an all-dead column is NaN / -1 beside a live one
    alive[0, 2] = 0
    x[0, :, 1] = nan
    h = R.stats_ref(x, alive, [0.5])
    assert h["n"].tolist() == [[3, 0]] and h["lo_draw"][0].tolist() == [3, -1] and h["hi_draw"][0].tolist() == [0, -1]
    assert np.isnan(h["mean"][0, 1]) and np.isnan(h["quantile"][0, 1, 0]) and h["q_draw"][0, 1, 0] == -1
    # int32: exact conversion, a negative value is no value; no levels: empty level arrays
    xi = np.array([[[4], [-1], [0], [7], [-1]]], np.int32)
    q = R.stats_ref(xi, None, [])
    assert q["n"][0, 0] == 3 and q["mean"][0, 0] == 11.0 / 3.0 and q["lo_draw"][0, 0] == 2 and q["hi"][0, 0] == 7.0
    assert q["quantile"].shape == (1, 1, 0)


@pytest.mark.parametrize("D,my,seed", [(1, 1, 0), (7, 3, 1), (65, 2, 2)])
def test_reference_equals_tail_ref_on_the_totals(D, my, seed):
    """m = 1, x = the totals J (summed over i in order) and alive = tail_ref's survivors: quantile, cvar and
    q_draw are tail_ref's, bit for bit; alive_ref is that classification."""
    rng = np.random.default_rng(seed)
    Cn = 6
    J1 = rng.integers(0, 5, (Cn, D, my)).astype(float) + rng.random((Cn, D, my)) * (rng.random((Cn, D, my)) < 0.5)
    J1[rng.random((Cn, D, my)) < 0.05] = np.inf
    st = (rng.random((Cn, D)) < 0.15).astype(np.int32) * 4
    st[2, 0] = 16
    st[3] = 0
    J1[3, :, 0] = 2e100 if D > 1 else 1.0          # over the default bound
    levels = [0.9, 1.0, 1e-9, 0.5, 0.9]
    for bound in (0.0, 6.5, math.inf):
        want = T.tail_ref(J1, st, bound, levels)
        alive = R.alive_ref(J1, st, bound)
        J = np.zeros((Cn, D, 1))
        for i in range(my):
            J[:, :, 0] += J1[:, :, i]
        got = R.stats_ref(J, alive, levels)
        assert (got["n"][:, 0] == want["n"]).all() and (alive.sum(1) == want["n"]).all()
        T.assert_same_tail({f: got[f][:, 0] for f in T.FIELDS}, want, msg="bound %r" % bound)
        b = R.base_ref(J1, st, bound)
        assert (b["worst_draw"] == got["hi_draw"][:, 0]).all()
        assert (b["n_failed"] == np.where(st.any(1) & ((st & 24).any(1)), 0, D - want["n"])).all()
    assert (R.alive_ref(J1, st, 0.0)[2] == 0).all() and R.alive_ref(J1, st, 0.0).any()


def test_header_declares_and_lib_exports(built):
    from mpct import _lib

    src = open(os.path.join(ROOT, "include", "mpct.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    so = C.CDLL(_lib.lib_path())
    for f in EXPORTS:
        assert re.search(r"\bint32_t %s\s*\(" % f, code), f
        assert f in _lib.EXPORTS
        assert C.cast(getattr(so, f), C.c_void_p).value
    m = re.search(r"typedef struct mpct_draw_stats_result \{(.*?)\} mpct_draw_stats_result;", code, flags=re.S)
    assert re.findall(r"(double|int32_t)\* (\w+);", m.group(1)) == [
        ("int32_t" if i else "double", n) for n, i, _ in _lib.STATS_FIELDS]
    assert [n for n, _, _ in _lib.STATS_FIELDS] == list(R.FIELDS)
    assert re.search(r"#define MPCT_STAT_F64 0\b", code) and re.search(r"#define MPCT_STAT_I32 1\b", code)
    assert (_lib.STAT_F64, _lib.STAT_I32) == (0, 1)
    ids = re.findall(r"#define MPCT_IX_(\w+) (\d+)\b", code)
    assert [(n.lower(), int(v)) for n, v in ids] == [(n, k) for k, n in enumerate(R.INDEX_FIELDS)]
    assert [n for n, _, _ in _lib.INDEX_FIELDS] == list(R.INDEX_FIELDS)
    assert "mpct_internal_draw_stats_grid" not in src and C.cast(so.mpct_internal_draw_stats_grid, C.c_void_p).value
    assert _lib.load().mpct_abi_version() == 7
    for phrase in ("SURVIVES", "lowest draw index", "DESCENDING", "Argument errors", "bitwise independent"):
        assert phrase in src, phrase


def test_draw_stats_argument_errors_in_documented_order(built):
    from mpct import _lib

    lib = _lib.load()
    buf, ibuf = np.zeros(64), np.zeros(64, dtype=np.int32)
    d, i = buf.ctypes.data_as(_lib.c_double_p), ibuf.ctypes.data_as(_lib.c_int32_p)
    S = _lib.MpctDrawStats
    none, base, lev = S(), S(n=i, hi=d), S(mean=d, q_draw=i)
    a = buf.ctypes.data
    nanlev, badlev, oklev = np.array([0.5, np.nan]), np.array([0.5, 1.5]), np.array([0.5, 1.0])
    zero = np.array([0.0])
    L = lambda v: v.ctypes.data_as(_lib.c_double_p)  # noqa: E731
    big = 1 << 31
    #          x     type C   D     m  nlev levels      out
    steps = [((None, 7, -1, 5000, 1, 9, None, none), EINVAL, "bad shape"),
             ((None, 7, big, 0, 1, 9, None, none), EINVAL, "bad shape"),
             ((None, 7, big, 5000, 0, 9, None, none), EINVAL, "bad shape"),
             ((None, 7, big, 5000, 1, 9, None, none), EINVAL, "x_type"),
             ((None, -1, big, 5000, 1, 9, None, none), EINVAL, "x_type"),
             ((None, 0, big, 5000, 1, 9, None, none), EINVAL, "nlev must be"),
             ((None, 1, big, 5000, 1, -1, None, none), EINVAL, "nlev must be"),
             ((None, 1, big, 5000, 1, 2, None, none), EINVAL, "null levels"),
             ((None, 1, big, 5000, 1, 2, L(nanlev), none), EINVAL, "every level"),
             ((None, 1, big, 5000, 1, 2, L(badlev), none), EINVAL, "every level"),
             ((None, 1, big, 5000, 1, 1, L(zero), none), EINVAL, "every level"),
             ((None, 1, big, 5000, 1, 2, L(oklev), none), EINVAL, "no output pointer"),
             ((None, 1, big, 5000, 1, 2, L(oklev), None), EINVAL, "no output pointer"),
             ((None, 1, big, 5000, 1, 0, None, lev), EINVAL, "need nlev >= 1"),
             ((None, 1, big, 5000, 1, 0, L(oklev), lev), EINVAL, "need nlev >= 1"),
             ((None, 1, big, 5000, 1, 2, L(oklev), lev), EINVAL, "x is NULL"),
             ((None, 0, big, 5000, 1, 0, None, base), EINVAL, "x is NULL"),
             ((a, 0, big, 5000, 1, 0, None, base), ERANGE, "MPCT_TAIL_MAX_DRAWS"),
             ((a, 0, big, 4097, 1, 2, L(oklev), lev), ERANGE, "MPCT_TAIL_MAX_DRAWS"),
             ((a, 0, big, 4096, 1, 0, None, base), ERANGE, "MPCT_INDEX_MAX_ROWS"),
             ((a, 1, 1 << 29, 1, 4, 0, None, base), ERANGE, "MPCT_INDEX_MAX_ROWS")]
    for args, code, msg in steps:
        x, ty, C_, D, m, nlev, lv, out = args
        oo = C.byref(out) if out is not None else None
        for rc in (lib.mpct_draw_stats_device(x, ty, None, C_, D, m, nlev, lv, oo, None),
                   lib.mpct_draw_stats(x, ty, None, C_, D, m, nlev, lv, -1, oo)):
            assert rc == code, (args[1:6], msg, rc, _lib.last_error())
            assert msg in _lib.last_error(), (args[1:6], msg, _lib.last_error())
    # C = 0 is fine without a table and without a device, and writes nothing
    assert lib.mpct_draw_stats_device(None, 0, None, 0, 4, 2, 2, L(oklev), C.byref(lev), None) == 0
    assert lib.mpct_draw_stats(None, 1, None, 0, 4, 2, 0, None, -1, C.byref(base)) == 0
    assert (buf == 0).all() and (ibuf == 0).all()


@pytest.fixture(scope="module")
def small_scenario(built):
    from mpct.scenarios import shell3x3

    sc, r, _ = shell3x3(n2_max=10, nu_max=3, nit=40)
    yield sc, r
    sc.close()


def test_eval_robust_indices_argument_errors_in_documented_order(small_scenario):
    from mpct import _lib

    sc, r = small_scenario
    lib = _lib.load()
    buf, ibuf = np.zeros(4096), np.zeros(4096, dtype=np.int32)
    d, i = buf.ctypes.data_as(_lib.c_double_p), ibuf.ctypes.data_as(_lib.c_int32_p)
    N2, Nu = np.array([5, 6], dtype=np.int32), np.array([2, 2], dtype=np.int32)
    dl, lm = np.ones((2, 3)), np.ones((2, 3))
    refs = np.ascontiguousarray(r[None])
    P, O, S, B = _lib.MpctIndexParams, _lib.MpctOpts, _lib.MpctDrawStats, _lib.MpctRobustResult
    ol, cl = O(1, 0, 0, -1, 0.0), O(0, 0, 0, -1, 0.0)
    badp = P(40, -1.0, 0.0)
    none, some, lev = S(), S(hi=d), S(hi=d, cvar=d)
    bnone, bj1, bsome = B(), B(J1=d), B(n_failed=i)
    F = lambda *ids: np.array(ids, dtype=np.int32)  # noqa: E731
    ok_f, rep_f, out_f = F(8, 5, 7), F(8, 5, 8), F(8, 13)
    nanlev, oklev = np.array([0.5, np.nan]), np.array([0.5, 1.0])
    manyrefs = 5000

    def call(h, C_, nref, refs_p, jb, opts, p, nsel, f, nlev, lv, base, out):
        a = [h, C_, N2.ctypes.data, Nu.ctypes.data, dl.ctypes.data, lm.ctypes.data, nref, refs_p, None, jb,
             C.byref(opts) if opts is not None else None, C.byref(p) if p is not None else None, nsel,
             f.ctypes.data_as(_lib.c_int32_p) if f is not None else None, nlev,
             lv.ctypes.data_as(_lib.c_double_p) if lv is not None else None,
             C.byref(base) if base is not None else None, C.byref(out) if out is not None else None]
        return lib.mpct_eval_robust_indices(*a), lib.mpct_eval_robust_indices_device(*(a + [None]))

    rp = refs.ctypes.data
    h = sc.handle
    #         h     C  nref  refs  j_bound opts p     nsel f     nlev lv     base   out
    steps = [((None, -1, 0, None, -1.0, ol, None, 0, None, 9, None, bj1, none), EINVAL, "null scenario"),
             ((h, -1, 0, None, -1.0, ol, None, 0, None, 9, None, bj1, none), EINVAL, "null params"),
             ((h, -1, 0, None, -1.0, ol, badp, 0, None, 9, None, bj1, none), EINVAL, "open_loop must be 0"),
             ((h, -1, 0, None, -1.0, cl, badp, 0, None, 9, None, bj1, none), EINVAL, "nsel must be"),
             ((h, -1, 0, None, -1.0, cl, badp, 14, ok_f, 9, None, bj1, none), EINVAL, "nsel must be"),
             ((h, -1, 0, None, -1.0, cl, badp, 3, None, 9, None, bj1, none), EINVAL, "nsel must be"),
             ((h, -1, 0, None, -1.0, cl, badp, 2, out_f, 9, None, bj1, none), EINVAL, "field id out of range"),
             ((h, -1, 0, None, -1.0, cl, badp, 3, rep_f, 9, None, bj1, none), EINVAL, "field id repeated"),
             ((h, -1, 0, None, -1.0, cl, badp, 3, ok_f, 9, None, bj1, none), EINVAL, "nref < 1"),
             ((h, -1, manyrefs, None, -1.0, cl, badp, 3, ok_f, 9, None, bj1, none), EINVAL, "j_bound must be"),
             ((h, -1, manyrefs, None, np.nan, cl, badp, 3, ok_f, 9, None, bj1, none), EINVAL, "j_bound must be"),
             ((h, -1, manyrefs, None, 0.0, cl, badp, 3, ok_f, 9, None, bj1, none), EINVAL, "nlev must be"),
             ((h, -1, manyrefs, None, np.inf, cl, badp, 3, ok_f, -1, None, bj1, none), EINVAL, "nlev must be"),
             ((h, -1, manyrefs, None, 0.0, cl, badp, 3, ok_f, 2, None, bj1, none), EINVAL, "null levels"),
             ((h, -1, manyrefs, None, 0.0, cl, badp, 3, ok_f, 2, nanlev, bj1, none), EINVAL, "every level"),
             ((h, -1, manyrefs, None, 0.0, cl, badp, 3, ok_f, 2, oklev, bnone, none), EINVAL, "every output pointer"),
             ((h, -1, manyrefs, None, 0.0, cl, badp, 3, ok_f, 2, oklev, None, None), EINVAL, "every output pointer"),
             ((h, -1, manyrefs, None, 0.0, cl, badp, 3, ok_f, 2, oklev, bj1, some), EINVAL, "base->J1 must be NULL"),
             ((h, -1, manyrefs, None, 0.0, cl, badp, 3, ok_f, 0, None, bsome, lev), EINVAL, "need nlev >= 1"),
             ((h, -1, manyrefs, None, 0.0, cl, badp, 3, ok_f, 2, oklev, bsome, lev), EINVAL, "C < 0 or nref < 1"),
             ((h, 2, manyrefs, None, 0.0, cl, badp, 3, ok_f, 2, oklev, bsome, lev), EINVAL, "null input pointer"),
             ((h, 2, manyrefs, rp, 0.0, cl, badp, 3, ok_f, 2, oklev, None, lev), EINVAL, "t0 must be"),
             ((h, 2, manyrefs, rp, 0.0, cl, P(39, -1.0, 0.0), 3, ok_f, 2, oklev, bsome, None), EINVAL, "band_rel and band_abs"),
             ((h, 2, manyrefs, rp, 0.0, None, P(39, 0.0, 0.0), 3, ok_f, 0, None, bsome, some), ERANGE, "MPCT_TAIL_MAX_DRAWS")]
    for args, code, msg in steps:
        for rc in call(*args):
            assert rc == code, (msg, rc, _lib.last_error())
            assert msg in _lib.last_error(), (msg, _lib.last_error())
    # C = 0 needs no device and writes nothing
    for rc in call(h, 0, 1, rp, 0.0, cl, P(0, 0.02, 0.0), 3, ok_f, 2, oklev, bsome, lev):
        assert rc == 0, _lib.last_error()
    assert (buf == 0).all() and (ibuf == 0).all()


def test_no_device_is_reported(small_scenario, has_gpu):
    from mpct.engine import MpctError, draw_stats, eval_robust_indices

    if has_gpu:
        pytest.skip("a GPU is present: the no-device message cannot show")
    sc, r = small_scenario
    x, alive = R.table(2, 5, 3, 3)
    with pytest.raises(MpctError, match=r"\(-3\).*HIP device"):
        draw_stats(x, alive, levels=[0.5])
    with pytest.raises(MpctError, match=r"\(-3\).*(GPU|HIP device)"):
        eval_robust_indices(sc, [5, 6], [2, 2], np.ones((2, 3)), np.ones((2, 3)), np.stack([r, r]), fields=("tv", "over"))
    # an empty batch and an empty table need no device
    res = eval_robust_indices(sc, np.zeros(0, dtype=np.int32), np.zeros(0, dtype=np.int32), np.zeros((0, 3)),
                              np.zeros((0, 3)), np.stack([r, r]), fields=("tv", "over", "settle"), levels=[0.9])
    assert res.hi.shape == (0, 9) and res.cvar.shape == (0, 9, 1) and len(res.columns) == 9
    assert res.columns[0] == ("tv", 0) and res.columns[3] == ("over", 0) and res.columns[8] == ("settle", 2)
    empty = draw_stats(np.zeros((0, 4, 2)), levels=[0.5])
    assert empty.n.shape == (0, 2) and empty.q_draw.shape == (0, 2, 1) and empty.n.dtype == np.int32


def test_robust_index_result_costs_masking():
    from mpct.engine import RobustIndexResult, RobustResult

    Cn = 3
    cols = [("tv", 0), ("tv", 1), ("over", 0), ("settle", 0)]
    hi = np.arange(12.0).reshape(Cn, 4)
    base = RobustResult(mean=np.zeros((Cn, 1)), worst=np.zeros((Cn, 1)), n_failed=np.array([0, 2, 1], np.int32),
                        worst_draw=np.zeros(Cn, np.int32), status=np.zeros(Cn, np.int32), draws=4)
    q = np.stack([hi, hi + 100.0], axis=2)
    res = RobustIndexResult(columns=cols, n=np.full((Cn, 4), 4, np.int32), mean=hi / 2, lo=-hi, lo_draw=np.zeros((Cn, 4), np.int32),
                            hi=hi, hi_draw=np.zeros((Cn, 4), np.int32), levels=np.array([0.5, 0.9]), quantile=q, cvar=q + 1,
                            q_draw=np.zeros((Cn, 4, 2), np.int32), base=base)
    got = res.costs("hi")
    assert got.shape == (3, 4) and got.dtype == np.float64
    np.testing.assert_array_equal(got[0], hi[0])
    assert np.isnan(got[1:]).all()                                  # more than max_failed = 0 failed draws
    got = res.costs(("cvar", 1), names=("over", "tv"), max_failed=1)
    np.testing.assert_array_equal(got[2], [111.0, 109.0, 110.0])    # the named fields' columns, in the order named
    assert np.isnan(got[1]).all() and not np.isnan(got[0]).any()
    np.testing.assert_array_equal(res.costs("mean", max_failed=2), hi / 2)
    got[0, 0] = -1.0
    assert res.cvar[0, 2, 1] == 103.0                               # a copy, not a view
    for bad in ("worst", ("median", 0)):
        with pytest.raises(ValueError):
            res.costs(bad)
    with pytest.raises(ValueError):
        res.costs("hi", names=("iae",))
    res.quantile = None
    with pytest.raises(ValueError):
        res.costs(("quantile", 0))
