"""CPU, no device: the contract of the oscillation indices per setpoint segment (include/mpct.h).  The reference
of tests/osc_ref.py gives the known answers on hand-made rows; its vectorised form equals it bit for bit; each
planted mistake fails the comparison on the committed cases; the header, the ctypes list and the library carry
the exports; every argument error comes back with the documented code in the documented order without a device;
empty calls need no device; OscResult.costs folds as specified."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import osc_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXPORTS = ("mpct_osc_indices_device", "mpct_osc_indices", "mpct_eval_osc_indices", "mpct_eval_osc_indices_device",
           "mpct_eval_robust_osc_indices", "mpct_eval_robust_osc_indices_device")
EINVAL, EDEVICE, ERANGE = -1, -3, -4
PAR = dict(band_rel=0.0, band_abs=R.H, rev_tol=R.TOL)

# the boundary lists of the GPU test: segment lengths 1, 2, 63, 64, 65 and 130, starts 0, 1, 63, 64 and 65, nseg 1,
# 2 and 16, tseg[0] > 0 and tseg[nseg] < nit; (name, nit, tseg)
TSEGS = [("one segment, the whole run", 65, [0, 65]),
         ("one sample", 3, [1, 2]),
         ("lengths 1 2 63 64 65 130", 330, [1, 2, 4, 67, 131, 196, 326]),
         ("starts 0 63 64 65", 200, [0, 63, 64, 65, 195]),
         ("two segments from 64", 200, [64, 129, 199]),
         ("sixteen segments", 140, [2, 3, 5, 8, 12, 17, 23, 30, 38, 47, 57, 68, 80, 93, 107, 122, 138])]
# (S, nref, my, nu): row counts 1 and 5 against four waves per workgroup, nref 1 and 3, my = 0 and nu = 0
SHAPES = [(5, 1, 3, 2), (6, 3, 3, 2), (1, 1, 1, 0), (5, 1, 1, 0), (1, 1, 0, 1), (5, 1, 0, 1)]
CASES = [(name, nit, tseg, shape) for name, nit, tseg in TSEGS for shape in SHAPES]


def test_boundary_lists_cover_the_shapes_named():
    lens = {b - a for _, _, t in TSEGS for a, b in zip(t, t[1:])}
    starts = {a for _, _, t in TSEGS for a in t[:-1]}
    assert {1, 2, 63, 64, 65, 130} <= lens and {0, 1, 63, 64, 65} <= starts
    assert {len(t) - 1 for _, _, t in TSEGS} >= {1, 2, 16}
    assert any(t[0] > 0 and t[-1] < nit for _, nit, t in TSEGS)


def test_reference_on_hand_made_output_rows():
    # a 3-lobe response to a step from 0 to 1: approach (lobe 0), overshoot, undershoot, second overshoot
    #             0    1    2    3     4    5     6    7     8      9    10   11
    y = np.array([0.0, 0.0, 0.5, 1.5, 1.25, 1.0, 0.75, 0.75, 1.0, 1.125, 1.0, 1.0])
    r = np.array([0.0, 0.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0])
    # segment [2, 12), base 1: c = r(1) = 0, d = 1, h = 0.0625: x = -0.5 | 0.5 0.25 | (0) | -0.25 -0.25 | (0) | 0.125
    g = R.output_unit(y, r, 2, 12, False, 1, 0.0625, 0.0)
    assert g == {"ncross": 3, "decay": 0.25, "period": 6, "a_last": 0.125}
    # the band at 0.125: the last peak is exactly on the edge, so inside: two crossings, no second peak
    g = R.output_unit(y, r, 2, 12, False, 1, 0.0, 0.125)
    assert g == {"ncross": 2, "decay": 0.0, "period": -1, "a_last": 0.25}
    assert not np.signbit(g["decay"])
    # base 0 in the same segment: c = y(2) = 0.5, d = 0.5: the relative band halves, the same three crossings
    assert R.output_unit(y, r, 2, 12, False, 0, 0.125, 0.0)["ncross"] == 3
    # segment 0 takes y(a) whatever the base
    assert R.output_unit(y, r, 2, 12, True, 1, 0.0625, 0.0) == R.output_unit(y, r, 2, 12, True, 0, 0.0625, 0.0)
    # the first of equal peaks: lobe k0 attains 0.5 at t = 3 and t = 4; T_k0 = 3
    ye = np.array([0.0, 0.0, 0.5, 1.5, 1.5, 1.0, 0.5, 1.0, 1.25, 1.25, 1.0, 1.0])
    g = R.output_unit(ye, r, 2, 12, False, 1, 0.0, 0.125)
    assert g == {"ncross": 3, "decay": 0.5, "period": 5, "a_last": 0.25}
    # a row that never leaves the band (the approach starts inside it): nothing to count, and no peak
    yq = np.array([0.0, 0.0, 0.9375, 1.0, 1.0625, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0])
    g = R.output_unit(yq, r, 2, 12, False, 1, 0.0625, 0.0)
    assert g == {"ncross": 0, "decay": 0.0, "period": -1, "a_last": 0.0} and not np.signbit(g["a_last"])
    # only the approach leaves the band: ncross = 0 < k0, so a_last is +0.0 although lobe 0 has a peak
    assert R.output_unit(np.array([0.0, 0.0, 0.5, 1.0, 1.0]), r[:5], 2, 5, False, 1, 0.0, 0.125)["a_last"] == 0.0
    # sigma = 0 (a disturbance on a level that does not move): k0 = 0, lobe 0 is the first excursion
    yd = np.array([1.0, 1.0, 1.5, 1.25, 0.75, 1.0, 1.125, 1.25, 1.0])
    rd = np.ones(9)
    g = R.output_unit(yd, rd, 1, 9, False, 1, 0.5, 0.0625)        # d = 0: the relative band vanishes
    assert g == {"ncross": 2, "decay": 0.5, "period": 5, "a_last": 0.25}
    # a growing oscillation: the last lobe's peak exceeds A_k0
    yg = np.array([0.0, 1.25, 0.5, 1.75, 0.0, 2.5])
    g = R.output_unit(yg, np.ones(6), 0, 6, True, 1, 0.0, 0.125)  # c = y(0) = 0: lobe 0 = {t = 0}
    assert g == {"ncross": 5, "decay": 3.0, "period": 2, "a_last": 1.5} and g["a_last"] > 0.25
    # inside samples between two outside samples of one sign are no crossing; -0.0 is inside a band of 0
    yz = np.array([1.0, 0.5, -0.0, 0.0, 0.25, -0.0, -0.5])
    g = R.output_unit(yz, np.zeros(7), 0, 7, True, 1, 0.0, 0.0)   # d = -1: k0 = 1
    assert g == {"ncross": 1, "decay": 0.0, "period": -1, "a_last": 0.5}
    # a NaN outside [a, b) does not matter, nor does one in r(t) before b - 1; inside y, or in r(a-1) under base 1,
    # it spoils the unit
    yn, rn = y.copy(), r.copy()
    yn[1], rn[5] = np.nan, np.nan
    assert R.output_unit(yn, rn, 2, 12, False, 1, 0.0625, 0.0) == R.output_unit(y, r, 2, 12, False, 1, 0.0625, 0.0)
    rn[1] = np.inf
    assert R.output_unit(y, rn, 2, 12, False, 0, 0.0625, 0.0)["ncross"] == 3
    bad = R.output_unit(y, rn, 2, 12, False, 1, 0.0625, 0.0)
    assert bad["ncross"] == -1 and bad["period"] == -1 and np.isnan(bad["decay"]) and np.isnan(bad["a_last"])


def test_reference_on_hand_made_input_rows():
    #             0    1    2    3    4    5    6     7    8
    u = np.array([0.0, 1.0, 3.0, 2.0, 2.0, 2.5, 2.25, 2.5, 2.5])
    g = R.input_unit(u, 1, 8, True, 0.0)         # the first segment: no move into sample a; moves + - 0 + - +
    assert g == {"nmove": 5, "nrev": 4, "t_rev": 7}
    g = R.input_unit(u, 1, 8, True, 0.25)        # |du| == rev_tol is no move: + - (0 0 0) +... the 0.5 is a move
    assert g == {"nmove": 3, "nrev": 2, "t_rev": 5}
    g = R.input_unit(u, 3, 8, False, 0.0)        # a later one starts with the move across its boundary, u(3) - u(2)
    assert g == {"nmove": 4, "nrev": 3, "t_rev": 7}
    assert R.input_unit(u, 3, 4, True, 0.0) == {"nmove": 0, "nrev": 0, "t_rev": -1}      # one sample, first segment
    z = np.array([0.0, -0.0, 0.0, -0.0])
    assert R.input_unit(z, 0, 4, True, 0.0) == {"nmove": 0, "nrev": 0, "t_rev": -1}      # moves of +-0.0 are none
    un = u.copy()
    un[2] = np.nan                               # u(a-1) of the segment [3, 8) is read
    assert R.input_unit(un, 3, 8, False, 0.0) == {"nmove": -1, "nrev": -1, "t_rev": -1}
    assert R.input_unit(un, 3, 8, True, 0.0)["nmove"] == 3


@pytest.mark.parametrize("name,nit,tseg,shape", CASES, ids=["%s S%d nref%d my%d nu%d" % ((c[0],) + c[3]) for c in CASES])
def test_vectorised_form_equals_the_scalar_one(name, nit, tseg, shape):
    S, nref, my, nu = shape
    y, u, r = R.generated(S, nref, my, nu, nit, tseg)
    for base in (0, 1):
        R.assert_bitwise(R.osc_np(y, u, r, tseg, base=base, **PAR), R.osc_scalar(y, u, r, tseg, base=base, **PAR),
                         what="%s base %d" % (name, base))


def test_edge_rows_have_the_known_answers():
    y, u, r, tseg = R.edge_rows()
    w = R.osc_scalar(y, u, r, tseg, base=1, **PAR)
    R.assert_bitwise(R.osc_np(y, u, r, tseg, base=1, **PAR), w)
    a = tseg[0]
    assert w["ncross"][0, :, 0].tolist() == [2, 2, 3, 2, 3, 0, 2, 9]
    assert w["decay"][0, :, 0].tolist() == [0.0, 0.0, 0.5, 0.0, 0.375, 0.0, 0.5, 2.0]
    # the tied peak of lobe k0 + 2 is taken where it comes first, in the earlier block
    assert w["period"][0, :, 0].tolist() == [-1, -1, (a + 64 + 60) - (a + 3), -1, 137, -1, 180, 74]
    assert w["a_last"][0, :, 0].tolist() == [0.5, 0.25, 0.375, 0.25, 0.1875, 0.0, 0.25, 1.25]
    assert w["a_last"][0, 7, 0] > 0.25                     # the growing row: above A_k0
    assert w["nrev"][0, :, 0].tolist() == [1, 1, 2, 1, 2, 0, 2, 8]
    assert w["t_rev"][0, :2, 0].tolist() == [a + 64, a + 3 * 64 + 2] and w["t_rev"][0, 5, 0] == -1


def test_generated_data_has_the_edges():
    name, nit, tseg = TSEGS[2]
    y, u, r = R.generated(6, 3, 3, 2, nit, tseg)
    w = R.osc_scalar(y, u, r, tseg, base=1, **PAR)
    long = np.diff(tseg) >= 63
    assert (w["ncross"][..., long] >= 3).all(), "every long segment rings"
    assert (w["decay"][..., long] < 0.9).any() and (w["decay"][..., long] > 1.1).any() and (w["decay"] == 1.0).any()
    assert (w["a_last"][..., long] > 2.0).any(), "a growing row"
    # the samples planted exactly on the band edges decide: one ulp more and the records move
    for g in (3, 4, 5):
        b = tseg[g + 1]
        assert y[0, 0, b - 3] == r[0, 0, b - 1] + R.H and y[0, 0, b - 2] == r[0, 0, b - 1] - R.H
        y2 = y.copy()
        y2[0, 0, b - 3], y2[0, 0, b - 2] = np.nextafter(y[0, 0, b - 3], np.inf), np.nextafter(y[0, 0, b - 2], -np.inf)
        got = R.osc_scalar(y2, u, r, tseg, base=1, **PAR)
        assert got["ncross"][0, 0, g] > w["ncross"][0, 0, g], "two more outside samples of opposite sign"
    assert np.signbit(y[:, 2]).any() and np.signbit(u[0, 1]).any()
    assert (w["nmove"][0, 1] == 0).all() and (w["nrev"][:, 0, -1] > 0).all()
    assert (np.diff(u[0, 0]) == R.TOL).any() and (np.diff(u[0, 0]) == -R.TOL).any()


@pytest.mark.parametrize("mistake", R.MISTAKES)
def test_planted_mistake_fails_the_comparison(mistake):
    """each planted mistake moves at least one record of the committed cases"""
    hit = 0
    for name, nit, tseg in TSEGS:
        y, u, r = R.generated(6, 3, 3, 2, nit, tseg)
        want = R.osc_scalar(y, u, r, tseg, base=1, **PAR)
        hit += len(R.mismatches(R.osc_scalar(y, u, r, tseg, base=1, mistake=mistake, **PAR), want))
    assert hit > 0, mistake


def test_header_declares_and_lib_exports(built):
    from mpct import _lib

    src = open(os.path.join(ROOT, "include", "mpct.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    so = C.CDLL(_lib.lib_path())
    for f in EXPORTS:
        assert re.search(r"\bint32_t %s\s*\(" % f, code), f
        assert f in _lib.EXPORTS and f in src.split("#ifndef MPCT_H")[0]
        assert C.cast(getattr(so, f), C.c_void_p).value
    m = re.search(r"typedef struct mpct_osc_result \{(.*?)\} mpct_osc_result;", code, flags=re.S)
    assert re.findall(r"(double|int32_t)\* (\w+);", m.group(1)) == [
        ("int32_t" if i else "double", n) for n, _, i in _lib.OSC_FIELDS]
    assert [n for n, _, _ in _lib.OSC_FIELDS] == list(R.FIELDS)
    assert [n for n, y, _ in _lib.OSC_FIELDS if y] == list(R.Y_FIELDS)
    assert tuple(n for n, _, i in _lib.OSC_FIELDS if i) == R.INT_FIELDS
    for k, (n, _, _) in enumerate(_lib.OSC_FIELDS):
        assert re.search(r"#define MPCT_OX_%s %d\b" % (n.upper(), k), code), n
    m = re.search(r"typedef struct mpct_osc_params \{(.*?)\} mpct_osc_params;", code, flags=re.S)
    assert re.findall(r"(int32_t|double|const int32_t\*) (\w+);", m.group(1)) == [
        ("int32_t", "nseg"), ("const int32_t*", "tseg"), ("int32_t", "base"), ("double", "band_rel"), ("double", "band_abs"),
        ("double", "rev_tol")]
    assert [n for n, _ in _lib.MpctOscParams._fields_] == ["nseg", "tseg", "base", "band_rel", "band_abs", "rev_tol"]
    assert _lib.load().mpct_abi_version() == 7
    for phrase in ("Segments.", "Validity.", "Exact; no contraction.", "Argument errors", "Layout."):
        assert phrase in src.split("Oscillation indices per setpoint segment")[1], phrase


def _params(tseg, base=1, band_rel=0.0, band_abs=0.0, rev_tol=0.0, keep=None, nseg=None):
    from mpct import _lib

    t = np.ascontiguousarray(tseg, dtype=np.int32) if tseg is not None else None
    keep.append(t)
    return _lib.MpctOscParams(len(t) - 1 if nseg is None else nseg, t.ctypes.data_as(_lib.c_int32_p) if t is not None else None,
                              base, band_rel, band_abs, rev_tol)


def test_osc_indices_argument_errors_in_documented_order(built):
    """Each call also carries every LATER error of the header's list, so the code that comes back shows the
    order of the checks.  Host pointers: nothing is dereferenced before the checks have passed."""
    from mpct import _lib

    lib = _lib.load()
    buf = np.zeros(64)
    ibuf = np.zeros(64, dtype=np.int32)
    d, i = buf.ctypes.data_as(_lib.c_double_p), ibuf.ctypes.data_as(_lib.c_int32_p)
    none = _lib.MpctOscResult()
    both = _lib.MpctOscResult(ncross=i, decay=d, nrev=i)
    only_y, only_u = _lib.MpctOscResult(a_last=d), _lib.MpctOscResult(t_rev=i)
    keep = []
    a = buf.ctypes.data
    big = 1 << 31
    long17 = list(range(18))
    # everything after the boundaries bad as well: base 2, a negative band, a negative dead zone
    bad = lambda tseg, nseg=None: _params(tseg, 2, -1.0, 0.0, -1.0, keep, nseg)          # noqa: E731
    ok = lambda **kw: _params([1, 5, 10], keep=keep, **kw)                               # noqa: E731
    #          y     u     r     S  nref my  nu  nit  params   out
    steps = [((None, None, None, -3, 0, 2, 1, 10, None, none), EINVAL, "null params"),
             ((None, None, None, -3, 0, 2, 1, 10, bad(None, 0), none), EINVAL, "bad shape"),
             ((None, None, None, 4, 0, -1, 1, 10, bad(None, 0), none), EINVAL, "bad shape"),
             ((None, None, None, 4, 0, 2, 1, 0, bad(None, 0), none), EINVAL, "bad shape"),
             ((None, None, None, 4, 0, 2, 1, 10, bad(None, 0), none), EINVAL, "nref < 1"),
             ((None, None, None, 4, 3, 2, 1, 10, bad(None, 0), none), EINVAL, "multiple of nref"),
             ((None, None, None, 4, 2, 2, 1, 10, bad(None, 0), none), EINVAL, "nseg must be"),
             ((None, None, None, 4, 2, 2, 1, 10, bad(None, 17), none), EINVAL, "nseg must be"),
             ((None, None, None, 4, 2, 2, 1, 10, bad([0, 5], 0), none), EINVAL, "nseg must be"),
             ((None, None, None, 4, 2, 2, 1, 10, bad(long17), none), ERANGE, "MPCT_SEG_MAX"),
             ((None, None, None, 4, 2, 2, 1, 10, bad([-1, 5, 10]), none), EINVAL, "strictly ascending"),
             ((None, None, None, 4, 2, 2, 1, 10, bad([0, 5, 11]), none), EINVAL, "strictly ascending"),
             ((None, None, None, 4, 2, 2, 1, 10, bad([0, 5, 5]), none), EINVAL, "strictly ascending"),
             ((None, None, None, 4, 2, 2, 1, 10, bad([0, 6, 5, 10]), none), EINVAL, "strictly ascending"),
             ((None, None, None, 4, 2, 2, 1, 10, bad([0, 5, 10]), none), EINVAL, "base must be"),
             ((None, None, None, 4, 2, 2, 1, 10, _params([0, 10], -1, -1.0, 0.0, -1.0, keep), none), EINVAL, "base must be"),
             ((None, None, None, 4, 2, 2, 1, 10, _params([0, 10], 1, -1.0, 0.0, -1.0, keep), none), EINVAL, "band_rel and band_abs"),
             ((None, None, None, 4, 2, 2, 1, 10, _params([0, 10], 0, 0.0, np.nan, -1.0, keep), none), EINVAL, "band_rel and band_abs"),
             ((None, None, None, 4, 2, 2, 1, 10, _params([0, 10], 0, np.inf, 0.0, -1.0, keep), none), EINVAL, "band_rel and band_abs"),
             ((None, None, None, 4, 2, 2, 1, 10, ok(rev_tol=-1.0), none), EINVAL, "rev_tol must be"),
             ((None, None, None, 4, 2, 2, 1, 10, ok(rev_tol=np.inf), none), EINVAL, "rev_tol must be"),
             ((None, None, None, 4, 2, 2, 1, 10, ok(rev_tol=np.nan), none), EINVAL, "rev_tol must be"),
             ((None, None, None, 4, 2, 2, 1, 10, ok(), none), EINVAL, "no output pointer"),
             ((None, None, None, 4, 2, 2, 1, 10, ok(), None), EINVAL, "no output pointer"),
             ((None, a, a, big, 2, 2, 1, 10, ok(), both), EINVAL, "output-row field"),
             ((a, a, None, big, 2, 2, 1, 10, ok(), both), EINVAL, "output-row field"),
             ((a, a, a, big, 2, 0, 1, 10, ok(), only_y), EINVAL, "output-row field"),
             ((a, None, a, big, 2, 2, 1, 10, ok(), both), EINVAL, "input-row field"),
             ((a, a, a, big, 2, 2, 0, 10, ok(), only_u), EINVAL, "input-row field"),
             ((a, a, a, big, 2, 2, 1, 10, ok(), both), ERANGE, "MPCT_INDEX_MAX_ROWS"),
             # the cap is on S * nu * nseg: 2^30 rows of one channel pass with one segment, not with two
             ((None, a, None, 1 << 30, 2, 1, 1, 10, ok(), only_u), ERANGE, "MPCT_INDEX_MAX_ROWS")]
    for args, code, msg in steps:
        y, u, r, S, nref, my, nu, nit, p, out = args
        pp = C.byref(p) if p is not None else None
        oo = C.byref(out) if out is not None else None
        for rc in (lib.mpct_osc_indices_device(y, u, r, S, nref, my, nu, nit, pp, oo, None),
                   lib.mpct_osc_indices(y, u, r, S, nref, my, nu, nit, pp, -1, oo)):
            assert rc == code, (args[3:8], msg, rc, _lib.last_error())
            assert msg in _lib.last_error(), (args[3:8], _lib.last_error())
    # a dead zone of 0, sixteen segments and S = 0 are fine, without trajectories or a device
    p = _params(list(range(17)), 0, 0.02, 0.0, 0.0, keep)
    q = _params([0, 10], 1, 0.0, 0.0, 1e300, keep)
    for pr in (p, q):
        assert lib.mpct_osc_indices_device(None, None, None, 0, 1, 2, 1, 16, C.byref(pr), C.byref(both), None) == 0
        assert lib.mpct_osc_indices(None, None, None, 0, 1, 2, 1, 16, C.byref(pr), -1, C.byref(both)) == 0
    assert (buf == 0).all() and (ibuf == 0).all()


@pytest.fixture(scope="module")
def small_scenario(built):
    from mpct.scenarios import shell3x3

    sc, r, _ = shell3x3(n2_max=10, nu_max=3, nit=40)
    yield sc, r
    sc.close()


def test_eval_entries_argument_errors_in_documented_order(small_scenario):
    from mpct import _lib

    sc, r = small_scenario
    lib = _lib.load()
    buf = np.zeros(4 * 3 * 40)
    ibuf = np.zeros(64, dtype=np.int32)
    d = buf.ctypes.data_as(_lib.c_double_p)
    N2, Nu = np.array([5, 6], dtype=np.int32), np.array([2, 2], dtype=np.int32)
    dl, lm = np.ones((2, 3)), np.ones((2, 3))
    refs = np.ascontiguousarray(r[None])
    O = _lib.MpctOpts
    none, some = _lib.MpctOscResult(), _lib.MpctOscResult(decay=d)
    traj = _lib.MpctResult(y=d)
    ol, cl = O(1, 0, 0, -1, 0.0), O(0, 0, 0, -1, 0.0)
    keep = []
    bad = lambda tseg, nseg=None: _params(tseg, 2, -1.0, 0.0, -1.0, keep, nseg)          # noqa: E731
    ref = lambda x: C.byref(x) if x is not None else None                                # noqa: E731

    def call(h, C_, nref, refs_p, opts, p, res, out):
        a = [h, C_, N2.ctypes.data, Nu.ctypes.data, dl.ctypes.data, lm.ctypes.data, nref, refs_p, None, ref(opts), ref(p),
             ref(res), ref(out)]
        return lib.mpct_eval_osc_indices(*a), lib.mpct_eval_osc_indices_device(*(a + [None]))

    rp = refs.ctypes.data
    E = EINVAL
    steps = [((None, -1, 0, None, ol, None, traj, none), E, "null scenario"),
             ((sc.handle, -1, 0, None, ol, None, traj, none), E, "null params"),
             ((sc.handle, -1, 0, None, ol, bad(None, 0), traj, none), E, "open_loop must be 0"),
             ((sc.handle, -1, 0, None, cl, bad(None, 0), traj, none), E, "trajectory pointers of res"),
             ((sc.handle, -1, 0, None, cl, bad(None, 0), None, none), E, "C < 0 or nref < 1"),
             ((sc.handle, 2, 0, None, cl, bad(None, 0), None, none), E, "C < 0 or nref < 1"),
             ((sc.handle, 2, 1, None, cl, bad(None, 0), None, none), E, "null input pointer"),
             ((sc.handle, 2, 1, rp, cl, bad(None, 0), None, none), E, "nseg must be"),
             ((sc.handle, 2, 1, rp, cl, bad(list(range(18))), None, none), ERANGE, "MPCT_SEG_MAX"),
             ((sc.handle, 2, 1, rp, cl, bad([0, 9, 41]), None, none), E, "strictly ascending"),      # nit is the scenario's 40
             ((sc.handle, 2, 1, rp, cl, bad([0, 9, 40]), None, none), E, "base must be"),
             ((sc.handle, 2, 1, rp, None, _params([0, 9, 40], 1, -1.0, 0.0, -1.0, keep), None, none), E, "band_rel and band_abs"),
             ((sc.handle, 2, 1, rp, None, _params([0, 9, 40], 1, 0.0, 0.0, -1.0, keep), None, none), E, "rev_tol must be"),
             ((sc.handle, 2, 1, rp, None, _params([0, 9, 40], keep=keep), None, none), E, "no output pointer"),
             ((sc.handle, 2, 1, rp, None, _params([0, 9, 40], keep=keep), None, None), E, "no output pointer")]
    for args, code, msg in steps:
        for rc in call(*args):
            assert rc == code, (msg, rc, _lib.last_error())
            assert msg in _lib.last_error(), (msg, _lib.last_error())
    # an empty batch is fine without a device
    p = _params([0, 9, 40], keep=keep)
    assert call(sc.handle, 0, 1, rp, None, p, None, some) == (0, 0)

    # the robust entries: the list of mpct_eval_robust_indices, then the oscillation parameters
    S = _lib.MpctDrawStats
    stats, lev_stats = S(hi=d), S(hi=d, quantile=d)
    base_j1 = _lib.MpctRobustResult(J1=d)
    ids = lambda *v: np.array(v, dtype=np.int32)                     # noqa: E731
    lv = np.array([0.5, 2.0])

    def rcall(h, C_, nref, refs_p, jb, opts, p, nsel, fields, nlev, levels, base, out):
        a = [h, C_, N2.ctypes.data, Nu.ctypes.data, dl.ctypes.data, lm.ctypes.data, nref, refs_p, None, jb, ref(opts), ref(p),
             nsel, fields.ctypes.data_as(_lib.c_int32_p) if fields is not None else None, nlev,
             levels.ctypes.data_as(_lib.c_double_p) if levels is not None else None, ref(base), ref(out)]
        return lib.mpct_eval_robust_osc_indices(*a), lib.mpct_eval_robust_osc_indices_device(*(a + [None]))

    h = sc.handle
    b0 = lambda: bad(None, 0)                                        # noqa: E731
    rsteps = [((None, 2, 0, None, -1.0, ol, None, 0, None, 9, None, base_j1, None), E, "null scenario"),
              ((h, 2, 0, None, -1.0, ol, None, 0, None, 9, None, base_j1, None), E, "null params"),
              ((h, 2, 0, None, -1.0, ol, b0(), 0, None, 9, None, base_j1, None), E, "open_loop must be 0"),
              ((h, 2, 0, None, -1.0, cl, b0(), 0, None, 9, None, base_j1, None), E, "nsel must be"),
              ((h, 2, 0, None, -1.0, cl, b0(), 8, ids(*range(8)), 9, None, base_j1, None), E, "nsel must be"),
              ((h, 2, 0, None, -1.0, cl, b0(), 2, ids(0, 7), 9, None, base_j1, None), E, "field id out of range"),
              ((h, 2, 0, None, -1.0, cl, b0(), 2, ids(1, 1), 9, None, base_j1, None), E, "field id repeated"),
              ((h, 2, 0, None, -1.0, cl, b0(), 2, ids(1, 6), 9, None, base_j1, None), E, "nref < 1"),
              ((h, 2, 1, None, -1.0, cl, b0(), 2, ids(1, 6), 9, None, base_j1, None), E, "j_bound must be"),
              ((h, 2, 1, None, 0.0, cl, b0(), 2, ids(1, 6), 9, None, base_j1, None), E, "nlev must be"),
              ((h, 2, 1, None, 0.0, cl, b0(), 2, ids(1, 6), 2, None, base_j1, None), E, "null levels"),
              ((h, 2, 1, None, 0.0, cl, b0(), 2, ids(1, 6), 2, lv, base_j1, None), E, "every level"),
              ((h, 2, 1, None, 0.0, cl, b0(), 2, ids(1, 6), 0, None, base_j1, None), E, "every output pointer"),
              ((h, 2, 1, None, 0.0, cl, b0(), 2, ids(1, 6), 0, None, base_j1, lev_stats), E, "base->J1 must be NULL"),
              ((h, 2, 1, None, 0.0, cl, b0(), 2, ids(1, 6), 0, None, None, lev_stats), E, "need nlev >= 1"),
              ((h, 2, 1, None, 0.0, cl, b0(), 2, ids(1, 6), 0, None, None, stats), E, "null input pointer"),
              ((h, 2, 1, rp, 0.0, cl, b0(), 2, ids(1, 6), 0, None, None, stats), E, "nseg must be"),
              ((h, 2, 1, rp, 0.0, cl, bad(list(range(18))), 2, ids(1, 6), 0, None, None, stats), ERANGE, "MPCT_SEG_MAX"),
              ((h, 2, 1, rp, 0.0, cl, bad([0, 9, 41]), 2, ids(1, 6), 0, None, None, stats), E, "strictly ascending"),
              ((h, 2, 1, rp, 0.0, cl, bad([0, 9, 40]), 2, ids(1, 6), 0, None, None, stats), E, "base must be"),
              ((h, 2, 1, rp, 0.0, cl, _params([0, 40], 0, 0.0, -1.0, -1.0, keep), 2, ids(1, 6), 0, None, None, stats), E,
               "band_rel and band_abs"),
              ((h, 2, 1, rp, 0.0, cl, _params([0, 40], 0, 0.0, 0.0, -1.0, keep), 2, ids(1, 6), 0, None, None, stats), E,
               "rev_tol must be"),
              ((h, 2, 4097, rp, 0.0, cl, _params([0, 40], keep=keep), 2, ids(1, 6), 0, None, None, stats), ERANGE,
               "MPCT_TAIL_MAX_DRAWS")]
    for args, code, msg in rsteps:
        for rc in rcall(*args):
            assert rc == code, (msg, rc, _lib.last_error())
            assert msg in _lib.last_error(), (msg, _lib.last_error())
    assert rcall(h, 0, 1, rp, 0.0, None, p, 2, ids(1, 6), 0, None, None, stats) == (0, 0)
    assert (buf == 0).all() and (ibuf == 0).all()


def test_no_device_is_reported_and_empty_calls_need_none(small_scenario, has_gpu):
    from mpct.engine import MpctError, eval_osc_indices, osc_indices

    sc, r = small_scenario
    e = np.zeros((0,), dtype=np.int32)
    res = eval_osc_indices(sc, e, e, np.zeros((0, 3)), np.zeros((0, 3)), r[None])
    assert res.decay.shape == (0, 1, 3, 2) and res.nrev.shape == (0, 1, 3, 2) and res.tseg.tolist() == [0, 9, 40]
    res = osc_indices(np.zeros((0, 2, 8)), np.zeros((0, 1, 8)), np.zeros((1, 2, 8)), [0, 4, 8])
    assert res.ncross.shape == (0, 1, 2, 2) and res.ncross.dtype == np.int32 and res.t_rev.shape == (0, 1, 1, 2)
    assert res.decay.dtype == np.float64
    if has_gpu:
        return
    with pytest.raises(MpctError, match=r"\(-3\)"):
        osc_indices(np.zeros((1, 2, 8)), np.zeros((1, 1, 8)), np.zeros((1, 2, 8)), [0, 4, 8])
    with pytest.raises(MpctError, match=r"\(-3\)"):
        eval_osc_indices(sc, [5], [2], np.ones((1, 3)), np.ones((1, 3)), r[None])


def test_osc_result_costs():
    from mpct.engine import OscResult, RobustResult, RobustSegmentResult

    tseg = np.array([2, 10, 30], dtype=np.int32)
    z = lambda *v: np.array(v, dtype=float).reshape(3, 1, 2, 2)           # noqa: E731 -- (C, nref, my | nu, nseg)
    res = OscResult(
        tseg=tseg,
        ncross=z(1, 2, 0, 6,   3, 1, 1, 1,   -1, 1, 1, 1).astype(np.int32),
        decay=z(0.0, 0.25, 0.0, 0.8,   0.5, 0.0, 0.0, 0.0,   np.nan, 0.0, 0.0, 0.0),
        period=z(4, 6, 3, 9,   5, -1, 4, 4,   -1, 3, 3, 3).astype(np.int32),
        t_rev=z(4, 15, 2, 10,   -1, 12, 3, 11,   -1, -1, -1, -1).astype(np.int32))
    c = res.costs(("ncross", "decay"))
    assert c.dtype == np.float64 and c.shape == (3, 2)
    assert c[0].tolist() == [6.0, 0.8] and c[1].tolist() == [3.0, 0.5] and np.isnan(c[2]).all()
    assert res.costs(("ncross",), reduce="sum")[0, 0] == 9.0
    assert res.costs(("decay",), segments=(0,))[:2, 0].tolist() == [0.0, 0.5]
    # period: -1 is no value, whether the unit is invalid or has no second peak
    p = res.costs(("period",))
    assert p[0, 0] == 9.0 and np.isnan(p[1, 0]) and np.isnan(p[2, 0])
    assert res.costs(("period",), segments=(0,))[:2, 0].tolist() == [4.0, 5.0]
    # t_rev: samples after the segment's start; -1 is no value
    t = res.costs(("t_rev",))
    assert t[0, 0] == 5.0 and np.isnan(t[1, 0]) and np.isnan(t[2, 0])
    assert res.costs(("t_rev",), segments=(1,))[:2, 0].tolist() == [5.0, 2.0]
    with pytest.raises(ValueError):
        res.costs(("nmove",))
    with pytest.raises(ValueError):
        res.costs(("nope",))
    with pytest.raises(ValueError):
        res.costs(("decay",), segments=(2,))
    with pytest.raises(ValueError):
        res.costs(("decay",), reduce="mean")
    # the robust record is the segment family's: columns (field, channel, segment)
    cols = [(f, ch, g) for f in ("decay", "ncross") for ch in range(2) for g in range(2)]
    tab = np.arange(3 * 8, dtype=float).reshape(3, 8)
    rb = RobustResult(mean=np.zeros((3, 2)), worst=np.zeros((3, 2)), n_failed=np.array([0, 1, 0], dtype=np.int32),
                      worst_draw=np.zeros(3, dtype=np.int32), status=np.zeros(3, dtype=np.int32), draws=2)
    rr = RobustSegmentResult(columns=cols, n=tab, mean=tab, lo=tab, lo_draw=tab, hi=tab, hi_draw=tab, base=rb, tseg=tseg)
    assert rr.costs("hi", names=("ncross",), segments=(1,), max_failed=1).tolist() == [[5.0, 7.0], [13.0, 15.0], [21.0, 23.0]]
