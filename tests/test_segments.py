"""CPU, no device: the contract of the step-response indices per setpoint segment (include/mpct.h).  The
reference of tests/segments_ref.py gives the known answers on hand-made rows; its vectorised form equals it bit
for bit; each planted mistake fails the comparison on the committed cases; over integer-valued inputs the
segments' tv add up to the whole run's exactly; mpct_reference_segments finds the boundaries of the scenarios'
references; the header, the ctypes list and the library carry the exports; every argument error comes back with
the documented code in the documented order without a device; empty calls need no device; SegmentResult.costs
folds as specified."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import indices_ref as IR
import segments_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXPORTS = ("mpct_reference_segments", "mpct_segment_indices_device", "mpct_segment_indices", "mpct_eval_segment_indices",
           "mpct_eval_segment_indices_device", "mpct_eval_robust_segment_indices", "mpct_eval_robust_segment_indices_device")
EINVAL, EDEVICE, ERANGE = -1, -3, -4
PAR = dict(band_rel=0.0, band_abs=0.125, rise_lo=0.1, rise_hi=0.9)

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
    #            0    1    2    3    4    5     6     7    8    9
    y = np.array([0.0, 0.0, 0.5, 1.0, 1.25, 1.0, 1.0, 0.5, 0.0, 0.0])
    r = np.array([0.0, 0.0, 1.0, 1.0, 1.0, 1.0, 1.0, 0.0, 0.0, 0.0])
    # segment [2, 7), base 1: c = r(1) = 0, d = 1; the step up with an overshoot of 0.25 at t = 4
    g = R.output_unit(y, r, 2, 7, False, 1, 0.0, 0.125, 0.1, 0.9)
    assert g["iae"] == 0.75 and g["ise"] == 0.3125 and g["itae"] == 2 * 0.25
    assert (g["emax"], g["t_emax"], g["over"], g["under"], g["e_final"]) == (0.5, 2, 0.25, 0.0, 0.0)
    assert g["settle"] == 5          # |1.25 - 1| > 0.125 at t = 4, inside the band from t = 5
    assert g["rise"] == 1            # p(2) = 0.5 >= 0.1, p(3) = 1.0 >= 0.9
    # segment [7, 10): the step back down, c = r(6) = 1, d = -1, sigma = -1
    g = R.output_unit(y, r, 7, 10, False, 1, 0.0, 0.125, 0.1, 0.9)
    assert (g["iae"], g["emax"], g["t_emax"], g["over"], g["under"], g["settle"], g["rise"]) == (0.5, 0.5, 7, 0.0, 0.0, 8, 1)
    # base 0 in the same segment: c = y(7) = 0.5, d = -0.5: the band is the same, the rise levels are not
    # (p(7) = 0, p(8) = 0.5 is past both 0.05 and 0.45: t_lo = t_hi = 8)
    g0 = R.output_unit(y, r, 7, 10, False, 0, 0.0, 0.125, 0.1, 0.9)
    assert g0["rise"] == 0 and g0["settle"] == 8 and g0["iae"] == 0.5
    # segment 0 takes y(a) whatever the base
    assert R.output_unit(y, r, 2, 7, True, 1, 0.0, 0.125, 0.1, 0.9) == R.output_unit(y, r, 2, 7, True, 0, 0.0, 0.125, 0.1, 0.9)
    # inverse response: the output first goes the wrong way from the base level
    yi = np.array([0.0, 0.0, -0.5, -0.25, 0.5, 1.0, 1.0])
    ri = np.array([0.0, 0.0, 1.0, 1.0, 1.0, 1.0, 1.0])
    g = R.output_unit(yi, ri, 2, 7, False, 1, 0.02, 0.0, 0.1, 0.9)
    assert g["under"] == 0.5 and g["over"] == 0.0 and g["rise"] == 1 and g["settle"] == 5
    # a row that never reaches rise_hi: rise = b - a; and it never settles: settle = b
    ys = np.array([0.0, 0.0, 0.25, 0.5, 0.75, 0.75, 0.75])
    g = R.output_unit(ys, ri, 2, 7, False, 1, 0.02, 0.0, 0.1, 0.9)
    assert g["rise"] == 5 and g["settle"] == 7 and g["e_final"] == -0.25
    # sigma = 0: over is emax, under +0.0, rise -1
    g = R.output_unit(np.array([0.0, 0.5, -0.25]), np.zeros(3), 1, 3, False, 1, 0.0, 0.125, 0.1, 0.9)
    assert (g["over"], g["under"], g["rise"], g["emax"], g["settle"]) == (0.5, 0.0, -1, 0.5, 3)
    assert not np.signbit(g["under"])
    # samples exactly on the rise levels and on the band edge count
    yl = np.array([0.0, 0.125, 0.875, 1.125, 1.0])
    g = R.output_unit(yl, np.ones(5), 0, 5, True, 1, 0.0, 0.125, 0.125, 0.875)
    assert g["rise"] == 1 and g["settle"] == 2
    # the first of equal peaks
    assert R.output_unit(np.array([0.0, 2.0, -2.0, 2.0]), np.zeros(4), 0, 4, True, 0, 0.0, 0.0, 0.1, 0.9)["t_emax"] == 1
    # a NaN outside [a, b) does not matter; inside, or in r(a-1) under base 1, it spoils the unit
    yn, rn = y.copy(), r.copy()
    yn[1] = np.nan
    assert R.output_unit(yn, rn, 2, 7, False, 1, **PAR) == R.output_unit(y, r, 2, 7, False, 1, **PAR)
    rn[1] = np.inf
    assert R.output_unit(y, rn, 2, 7, False, 0, **PAR)["rise"] >= 0
    bad = R.output_unit(y, rn, 2, 7, False, 1, **PAR)
    assert bad["rise"] == -1 and bad["settle"] == -1 and np.isnan(bad["iae"]) and np.isnan(bad["under"])


def test_reference_on_hand_made_input_rows():
    u = np.array([0.0, 1.0, 3.0, 2.0, 2.0, -0.0, 0.0])
    g = R.input_unit(u, 1, 4, True)              # the first segment: no move into sample a
    assert (g["tv"], g["du2"], g["dumax"], g["u_lo"], g["u_hi"]) == (3.0, 5.0, 2.0, 1.0, 3.0)
    g = R.input_unit(u, 4, 7, False)             # a later one starts with the move across its boundary, u(4) - u(3)
    assert (g["tv"], g["du2"], g["dumax"], g["u_lo"], g["u_hi"]) == (2.0, 4.0, 2.0, 0.0, 2.0)
    z = R.input_unit(u, 5, 7, False)
    assert z["u_lo"] == 0.0 and not np.signbit(z["u_lo"]) and not np.signbit(z["u_hi"])
    one = R.input_unit(u, 2, 3, True)            # one sample, first segment: an empty range of moves
    assert (one["tv"], one["du2"], one["dumax"], one["u_lo"], one["u_hi"]) == (0.0, 0.0, 0.0, 3.0, 3.0)
    un = u.copy()
    un[3] = np.nan                               # u(a-1) of the segment [4, 7) is read
    assert np.isnan(R.input_unit(un, 4, 7, False)["tv"]) and np.isnan(R.input_unit(un, 4, 7, False)["u_lo"])
    assert R.input_unit(un, 4, 7, True)["tv"] == 0.0 + 2.0 + 0.0


def test_segment_tv_adds_up_to_the_whole_runs():
    rng = np.random.default_rng(5)
    u = rng.integers(-40, 40, size=(4, 2, 300)).astype(np.float64)
    y, r = np.zeros((4, 0, 300)), np.zeros((1, 0, 300))
    tseg = [3, 4, 70, 134, 199, 300]
    seg = R.segments_scalar(y, u, r, tseg)
    whole = IR.indices_scalar(y, u, r, 3, 0.0, 0.0)
    assert (seg["tv"].sum(-1) == whole["tv"]).all() and (seg["du2"].sum(-1) == whole["du2"]).all()
    assert (seg["dumax"].max(-1) == whole["dumax"]).all()
    assert (seg["u_lo"].min(-1) == whole["u_lo"]).all() and (seg["u_hi"].max(-1) == whole["u_hi"]).all()


def test_one_segment_is_the_index_reference():
    """the consequence the header states, on the references: nseg = 1, base = 0, tseg = {t0, nit}"""
    y, u, r = IR.generated(5, 1, 3, 2, 130)[:3]
    for t0 in (0, 1, 129):
        seg = R.segments_scalar(y, u, r, [t0, 130], base=0, band_rel=0.02, band_abs=0.01)
        want = IR.indices_scalar(y, u, r, t0, 0.02, 0.01)
        IR.assert_bitwise({f: seg[f][..., 0] for f in IR.Y_FIELDS + IR.U_FIELDS}, want, what="t0 = %d" % t0)


@pytest.mark.parametrize("name,nit,tseg,shape", CASES, ids=["%s S%d nref%d my%d nu%d" % ((c[0],) + c[3]) for c in CASES])
def test_vectorised_form_equals_the_scalar_one(name, nit, tseg, shape):
    S, nref, my, nu = shape
    y, u, r = R.generated(S, nref, my, nu, nit, tseg)
    for base in (0, 1):
        R.assert_bitwise(R.segments_np(y, u, r, tseg, base=base, **PAR), R.segments_scalar(y, u, r, tseg, base=base, **PAR),
                         what="%s base %d" % (name, base))


def test_generated_data_has_the_edges():
    name, nit, tseg = TSEGS[2]
    y, u, r = R.generated(6, 3, 3, 2, nit, tseg)
    w = R.segments_scalar(y, u, r, tseg, base=1, **PAR)
    assert (w["under"][:, 1, 1:] > 0).all(), "channel 1 starts every segment the wrong way"
    long = np.diff(tseg) >= 63
    assert (w["rise"][2, 0][long] == np.diff(tseg)[long]).all(), "simulation 2 never reaches rise_hi"
    assert (w["rise"][:, 2, 1:] == -1).all() and (w["under"][:, 2, 1:] == 0).all(), "channel 2: sigma = 0 under base 1"
    assert (w["rise"][0, 0][long] >= 1).all()
    # the samples planted exactly on the levels decide: one ulp less and the records move
    g = 3                            # 64 samples, a step up from c = 0 with |d| = 1: p(t) = y(t) exactly
    a = tseg[g]
    assert r[0, 0, a - 1] == 0.0 and r[0, 0, a] == 1.0 and y[0, 0, a + 1] == 0.1 and y[0, 0, a + 3] == 0.9
    y2 = y.copy()
    y2[0, 0, a + 3] = np.nextafter(y[0, 0, a + 3], r[0, 0, a - 1])
    assert R.segments_scalar(y2, u, r, tseg, base=1, **PAR)["rise"][0, 0, g] != w["rise"][0, 0, g]
    b = tseg[g + 1]
    y2 = y.copy()
    y2[0, 0, b - 2] = np.nextafter(y[0, 0, b - 2], np.inf)
    assert R.segments_scalar(y2, u, r, tseg, base=1, **PAR)["settle"][0, 0, g] == b - 1 != w["settle"][0, 0, g]
    assert (w["t_emax"][1, 1] == np.array(tseg[:-1]) + 1)[np.diff(tseg) >= 5].all(), "the first of two equal peaks"
    assert np.signbit(y[:, 2]).any() and np.signbit(u[0, 1]).any()


@pytest.mark.parametrize("mistake", R.MISTAKES)
def test_planted_mistake_fails_the_comparison(mistake):
    """each planted mistake moves at least one record of the committed cases"""
    hit = 0
    for name, nit, tseg in TSEGS:
        y, u, r = R.generated(6, 3, 3, 2, nit, tseg)
        want = R.segments_scalar(y, u, r, tseg, base=1, **PAR)
        hit += len(R.mismatches(R.segments_scalar(y, u, r, tseg, base=1, mistake=mistake, **PAR), want))
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
    m = re.search(r"typedef struct mpct_segment_result \{(.*?)\} mpct_segment_result;", code, flags=re.S)
    assert re.findall(r"(double|int32_t)\* (\w+);", m.group(1)) == [
        ("int32_t" if i else "double", n) for n, _, i in _lib.SEGMENT_FIELDS]
    assert [n for n, _, _ in _lib.SEGMENT_FIELDS] == list(R.FIELDS)
    assert [n for n, y, _ in _lib.SEGMENT_FIELDS if y] == list(R.Y_FIELDS)
    assert tuple(n for n, _, i in _lib.SEGMENT_FIELDS if i) == R.INT_FIELDS
    for k, (n, _, _) in enumerate(_lib.SEGMENT_FIELDS):
        assert re.search(r"#define MPCT_SX_%s %d\b" % (n.upper(), k), code), n
    m = re.search(r"typedef struct mpct_segment_params \{(.*?)\} mpct_segment_params;", code, flags=re.S)
    assert re.findall(r"(int32_t|double|const int32_t\*) (\w+);", m.group(1)) == [
        ("int32_t", "nseg"), ("const int32_t*", "tseg"), ("int32_t", "base"), ("double", "band_rel"), ("double", "band_abs"),
        ("double", "rise_lo"), ("double", "rise_hi")]
    assert [n for n, _ in _lib.MpctSegmentParams._fields_] == ["nseg", "tseg", "base", "band_rel", "band_abs", "rise_lo", "rise_hi"]
    assert re.search(r"#define MPCT_SEG_MAX 16\b", code) and _lib.SEG_MAX == 16
    assert _lib.load().mpct_abi_version() == 7
    for phrase in ("Segments.", "Validity.", "No contraction; fixed order.", "Consequence.", "Argument errors", "Layout."):
        assert phrase in src.split("Step-response indices per setpoint segment")[1], phrase


def test_reference_segments_of_the_scenarios(built):
    from mpct.engine import MpctError, reference_segments
    from mpct.scenarios import shell3x3, woodberry_toolbox

    sc, r, _ = shell3x3(n2_max=10, nu_max=3, nit=500)
    sc.close()
    assert reference_segments(r).tolist() == [0, 9, 79, 199, 399, 500] == R.reference_segments(r)
    assert reference_segments(r).dtype == np.int32
    sc, rw = woodberry_toolbox()[:2]
    sc.close()
    tw = reference_segments(rw, extra=(299,)).tolist()
    assert {9, 199, 299} <= set(tw) and tw == R.reference_segments(rw, (299,)) and tw[0] == 0 and tw[-1] == rw.shape[-1]
    assert 299 not in reference_segments(rw).tolist()
    # several reference sets: the union; extras are deduplicated against the changes and the ends
    r3 = np.zeros((3, 2, 20))
    r3[0, 0, 5:], r3[1, 1, 7:], r3[2, 0, 5:] = 1.0, -1.0, 2.0
    assert reference_segments(r3, extra=(7, 0, 20, 12, 12)).tolist() == [0, 5, 7, 12, 20]
    assert reference_segments(np.zeros((1, 4))).tolist() == [0, 4]
    # more than max_seg segments; a non-finite reference; an extra sample out of range
    with pytest.raises(MpctError, match=r"\(-4\).*max_seg"):
        reference_segments(r3, extra=(12,), max_seg=3)
    assert reference_segments(r3, extra=(12,), max_seg=4).size == 5
    r3[1, 0, 19] = np.nan
    with pytest.raises(MpctError, match=r"\(-1\).*non-finite"):
        reference_segments(r3)
    with pytest.raises(MpctError, match=r"\(-1\).*outside"):
        reference_segments(np.zeros((1, 4)), extra=(5,))


def test_reference_segments_argument_errors_in_documented_order(built):
    from mpct import _lib

    lib = _lib.load()
    r = np.zeros(12)
    r[3] = np.nan
    out = np.full(8, -7, dtype=np.int32)
    n = C.c_int32(-7)
    ex = np.array([99], dtype=np.int32)
    ip = lambda a: a.ctypes.data_as(_lib.c_int32_p)       # noqa: E731
    rp, op, np_ = r.ctypes.data, ip(out), C.byref(n)
    #          r    nref my nit extra nextra max_seg tseg_out nseg
    steps = [((None, 0, 1, 12, None, -1, 0, op, np_), EINVAL, "null pointer"),
             ((rp, 0, 1, 12, None, -1, 0, None, np_), EINVAL, "null pointer"),
             ((rp, 0, 1, 12, None, -1, 0, op, None), EINVAL, "null pointer"),
             ((rp, 0, 1, 12, None, -1, 0, op, np_), EINVAL, "bad shape"),
             ((rp, 1, 0, 12, None, -1, 0, op, np_), EINVAL, "bad shape"),
             ((rp, 1, 1, 0, None, -1, 0, op, np_), EINVAL, "bad shape"),
             ((rp, 1, 1, 12, None, -1, 0, op, np_), EINVAL, "max_seg < 1"),
             ((rp, 1, 1, 12, None, -1, 1, op, np_), EINVAL, "nextra < 0"),
             ((rp, 1, 1, 12, None, 1, 1, op, np_), EINVAL, "nextra < 0"),
             ((rp, 1, 1, 12, ip(ex), 1, 1, op, np_), EINVAL, "outside [0, nit]"),
             ((rp, 1, 1, 12, None, 0, 1, op, np_), EINVAL, "non-finite")]
    for args, code, msg in steps:
        assert lib.mpct_reference_segments(*args) == code, (msg, _lib.last_error())
        assert msg in _lib.last_error(), (msg, _lib.last_error())
    r[3] = 1.0                       # changes at 3 and 4: three segments
    assert lib.mpct_reference_segments(rp, 1, 1, 12, None, 0, 2, op, np_) == ERANGE and "max_seg" in _lib.last_error()
    assert (out == -7).all() and n.value == -7, "nothing is written on an error"
    assert lib.mpct_reference_segments(rp, 1, 1, 12, None, 0, 3, op, np_) == 0
    assert n.value == 3 and out[:4].tolist() == [0, 3, 4, 12] and (out[4:] == -7).all()


def _params(tseg, base=1, band_rel=0.0, band_abs=0.0, rise_lo=0.1, rise_hi=0.9, keep=None, nseg=None):
    from mpct import _lib

    t = np.ascontiguousarray(tseg, dtype=np.int32) if tseg is not None else None
    keep.append(t)
    return _lib.MpctSegmentParams(len(t) - 1 if nseg is None else nseg, t.ctypes.data_as(_lib.c_int32_p) if t is not None else None,
                                  base, band_rel, band_abs, rise_lo, rise_hi)


def test_segment_indices_argument_errors_in_documented_order(built):
    """Each call also carries every LATER error of the header's list, so the code that comes back shows the
    order of the checks.  Host pointers: nothing is dereferenced before the checks have passed."""
    from mpct import _lib

    lib = _lib.load()
    buf = np.zeros(64)
    ibuf = np.zeros(64, dtype=np.int32)
    d, i = buf.ctypes.data_as(_lib.c_double_p), ibuf.ctypes.data_as(_lib.c_int32_p)
    none = _lib.MpctSegmentResult()
    both = _lib.MpctSegmentResult(iae=d, rise=i, tv=d)
    only_y, only_u = _lib.MpctSegmentResult(under=d), _lib.MpctSegmentResult(u_hi=d)
    keep = []
    a = buf.ctypes.data
    big = 1 << 31
    long17 = list(range(18))
    # everything after the boundaries bad as well: base 2, a negative band, rise_lo > rise_hi
    bad = lambda tseg, nseg=None: _params(tseg, 2, -1.0, 0.0, 0.9, 0.1, keep, nseg)      # noqa: E731
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
             ((None, None, None, 4, 2, 2, 1, 10, _params([0, 10], -1, -1.0, 0.0, 0.9, 0.1, keep), none), EINVAL, "base must be"),
             ((None, None, None, 4, 2, 2, 1, 10, _params([0, 10], 1, -1.0, 0.0, 0.9, 0.1, keep), none), EINVAL, "band_rel and band_abs"),
             ((None, None, None, 4, 2, 2, 1, 10, _params([0, 10], 0, 0.0, np.nan, 0.9, 0.1, keep), none), EINVAL, "band_rel and band_abs"),
             ((None, None, None, 4, 2, 2, 1, 10, _params([0, 10], 0, np.inf, 0.0, 0.9, 0.1, keep), none), EINVAL, "band_rel and band_abs"),
             ((None, None, None, 4, 2, 2, 1, 10, ok(rise_lo=0.9, rise_hi=0.1), none), EINVAL, "rise_lo and rise_hi"),
             ((None, None, None, 4, 2, 2, 1, 10, ok(rise_lo=-0.1), none), EINVAL, "rise_lo and rise_hi"),
             ((None, None, None, 4, 2, 2, 1, 10, ok(rise_hi=1.5), none), EINVAL, "rise_lo and rise_hi"),
             ((None, None, None, 4, 2, 2, 1, 10, ok(rise_lo=np.nan), none), EINVAL, "rise_lo and rise_hi"),
             ((None, None, None, 4, 2, 2, 1, 10, ok(rise_hi=np.nan), none), EINVAL, "rise_lo and rise_hi"),
             ((None, None, None, 4, 2, 2, 1, 10, ok(), none), EINVAL, "no output pointer"),
             ((None, None, None, 4, 2, 2, 1, 10, ok(), None), EINVAL, "no output pointer"),
             ((None, a, a, big, 2, 2, 1, 10, ok(), both), EINVAL, "output-row field"),
             ((a, a, None, big, 2, 2, 1, 10, ok(), both), EINVAL, "output-row field"),
             ((a, a, a, big, 2, 0, 1, 10, ok(), only_y), EINVAL, "output-row field"),
             ((a, None, a, big, 2, 2, 1, 10, ok(), both), EINVAL, "input-row field"),
             ((a, a, a, big, 2, 2, 0, 10, ok(), only_u), EINVAL, "input-row field"),
             ((a, a, a, big, 2, 2, 1, 10, ok(), both), ERANGE, "MPCT_INDEX_MAX_ROWS"),
             # the cap is on S * my * nseg: 2^30 rows of one channel pass with one segment, not with two
             ((None, a, None, 1 << 30, 2, 1, 1, 10, ok(), only_u), ERANGE, "MPCT_INDEX_MAX_ROWS")]
    for args, code, msg in steps:
        y, u, r, S, nref, my, nu, nit, p, out = args
        pp = C.byref(p) if p is not None else None
        oo = C.byref(out) if out is not None else None
        for rc in (lib.mpct_segment_indices_device(y, u, r, S, nref, my, nu, nit, pp, oo, None),
                   lib.mpct_segment_indices(y, u, r, S, nref, my, nu, nit, pp, -1, oo)):
            assert rc == code, (args[3:8], msg, rc, _lib.last_error())
            assert msg in _lib.last_error(), (args[3:8], _lib.last_error())
    # rise_lo = rise_hi, the ends 0 and 1, sixteen segments and S = 0 are fine, without trajectories or a device
    p = _params(list(range(17)), 0, 0.02, 0.0, 0.0, 0.0, keep)
    q = _params([0, 10], 1, 0.0, 0.0, 1.0, 1.0, keep)
    for pr in (p, q):
        assert lib.mpct_segment_indices_device(None, None, None, 0, 1, 2, 1, 16, C.byref(pr), C.byref(both), None) == 0
        assert lib.mpct_segment_indices(None, None, None, 0, 1, 2, 1, 16, C.byref(pr), -1, C.byref(both)) == 0
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
    none, some = _lib.MpctSegmentResult(), _lib.MpctSegmentResult(iae=d)
    traj = _lib.MpctResult(y=d)
    ol, cl = O(1, 0, 0, -1, 0.0), O(0, 0, 0, -1, 0.0)
    keep = []
    bad = lambda tseg, nseg=None: _params(tseg, 2, -1.0, 0.0, 0.9, 0.1, keep, nseg)      # noqa: E731
    ref = lambda x: C.byref(x) if x is not None else None                                # noqa: E731

    def call(h, C_, nref, refs_p, opts, p, res, out):
        a = [h, C_, N2.ctypes.data, Nu.ctypes.data, dl.ctypes.data, lm.ctypes.data, nref, refs_p, None, ref(opts), ref(p),
             ref(res), ref(out)]
        return lib.mpct_eval_segment_indices(*a), lib.mpct_eval_segment_indices_device(*(a + [None]))

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
             ((sc.handle, 2, 1, rp, None, _params([0, 9, 40], 1, -1.0, 0.0, 0.9, 0.1, keep), None, none), E, "band_rel and band_abs"),
             ((sc.handle, 2, 1, rp, None, _params([0, 9, 40], 1, 0.0, 0.0, 0.9, 0.1, keep), None, none), E, "rise_lo and rise_hi"),
             ((sc.handle, 2, 1, rp, None, _params([0, 9, 40], keep=keep), None, none), E, "no output pointer"),
             ((sc.handle, 2, 1, rp, None, _params([0, 9, 40], keep=keep), None, None), E, "no output pointer")]
    for args, code, msg in steps:
        for rc in call(*args):
            assert rc == code, (msg, rc, _lib.last_error())
            assert msg in _lib.last_error(), (msg, _lib.last_error())
    # an empty batch is fine without a device
    p = _params([0, 9, 40], keep=keep)
    assert call(sc.handle, 0, 1, rp, None, p, None, some) == (0, 0)

    # the robust entries: the list of mpct_eval_robust_indices, then the segment parameters
    S = _lib.MpctDrawStats
    stats, lev_stats = S(hi=d), S(hi=d, quantile=d)
    base_j1 = _lib.MpctRobustResult(J1=d)
    ids = lambda *v: np.array(v, dtype=np.int32)                     # noqa: E731
    lv = np.array([0.5, 2.0])

    def rcall(h, C_, nref, refs_p, jb, opts, p, nsel, fields, nlev, levels, base, out):
        a = [h, C_, N2.ctypes.data, Nu.ctypes.data, dl.ctypes.data, lm.ctypes.data, nref, refs_p, None, jb, ref(opts), ref(p),
             nsel, fields.ctypes.data_as(_lib.c_int32_p) if fields is not None else None, nlev,
             levels.ctypes.data_as(_lib.c_double_p) if levels is not None else None, ref(base), ref(out)]
        return lib.mpct_eval_robust_segment_indices(*a), lib.mpct_eval_robust_segment_indices_device(*(a + [None]))

    h = sc.handle
    b0 = lambda: bad(None, 0)                                        # noqa: E731
    rsteps = [((None, 2, 0, None, -1.0, ol, None, 0, None, 9, None, base_j1, None), E, "null scenario"),
              ((h, 2, 0, None, -1.0, ol, None, 0, None, 9, None, base_j1, None), E, "null params"),
              ((h, 2, 0, None, -1.0, ol, b0(), 0, None, 9, None, base_j1, None), E, "open_loop must be 0"),
              ((h, 2, 0, None, -1.0, cl, b0(), 0, None, 9, None, base_j1, None), E, "nsel must be"),
              ((h, 2, 0, None, -1.0, cl, b0(), 16, ids(*range(16)), 9, None, base_j1, None), E, "nsel must be"),
              ((h, 2, 0, None, -1.0, cl, b0(), 2, ids(0, 15), 9, None, base_j1, None), E, "field id out of range"),
              ((h, 2, 0, None, -1.0, cl, b0(), 2, ids(9, 9), 9, None, base_j1, None), E, "field id repeated"),
              ((h, 2, 0, None, -1.0, cl, b0(), 2, ids(9, 14), 9, None, base_j1, None), E, "nref < 1"),
              ((h, 2, 1, None, -1.0, cl, b0(), 2, ids(9, 14), 9, None, base_j1, None), E, "j_bound must be"),
              ((h, 2, 1, None, 0.0, cl, b0(), 2, ids(9, 14), 9, None, base_j1, None), E, "nlev must be"),
              ((h, 2, 1, None, 0.0, cl, b0(), 2, ids(9, 14), 2, None, base_j1, None), E, "null levels"),
              ((h, 2, 1, None, 0.0, cl, b0(), 2, ids(9, 14), 2, lv, base_j1, None), E, "every level"),
              ((h, 2, 1, None, 0.0, cl, b0(), 2, ids(9, 14), 0, None, base_j1, None), E, "every output pointer"),
              ((h, 2, 1, None, 0.0, cl, b0(), 2, ids(9, 14), 0, None, base_j1, lev_stats), E, "base->J1 must be NULL"),
              ((h, 2, 1, None, 0.0, cl, b0(), 2, ids(9, 14), 0, None, None, lev_stats), E, "need nlev >= 1"),
              ((h, 2, 1, None, 0.0, cl, b0(), 2, ids(9, 14), 0, None, None, stats), E, "null input pointer"),
              ((h, 2, 1, rp, 0.0, cl, b0(), 2, ids(9, 14), 0, None, None, stats), E, "nseg must be"),
              ((h, 2, 1, rp, 0.0, cl, bad(list(range(18))), 2, ids(9, 14), 0, None, None, stats), ERANGE, "MPCT_SEG_MAX"),
              ((h, 2, 1, rp, 0.0, cl, bad([0, 9, 41]), 2, ids(9, 14), 0, None, None, stats), E, "strictly ascending"),
              ((h, 2, 1, rp, 0.0, cl, bad([0, 9, 40]), 2, ids(9, 14), 0, None, None, stats), E, "base must be"),
              ((h, 2, 1, rp, 0.0, cl, _params([0, 40], 0, 0.0, -1.0, 0.9, 0.1, keep), 2, ids(9, 14), 0, None, None, stats), E,
               "band_rel and band_abs"),
              ((h, 2, 1, rp, 0.0, cl, _params([0, 40], 0, 0.0, 0.0, 0.9, 0.1, keep), 2, ids(9, 14), 0, None, None, stats), E,
               "rise_lo and rise_hi"),
              ((h, 2, 4097, rp, 0.0, cl, _params([0, 40], keep=keep), 2, ids(9, 14), 0, None, None, stats), ERANGE,
               "MPCT_TAIL_MAX_DRAWS")]
    for args, code, msg in rsteps:
        for rc in rcall(*args):
            assert rc == code, (msg, rc, _lib.last_error())
            assert msg in _lib.last_error(), (msg, _lib.last_error())
    assert rcall(h, 0, 1, rp, 0.0, None, p, 2, ids(9, 14), 0, None, None, stats) == (0, 0)
    assert (buf == 0).all() and (ibuf == 0).all()


def test_no_device_is_reported_and_empty_calls_need_none(small_scenario, has_gpu):
    from mpct.engine import MpctError, eval_segment_indices, segment_indices

    sc, r = small_scenario
    e = np.zeros((0,), dtype=np.int32)
    res = eval_segment_indices(sc, e, e, np.zeros((0, 3)), np.zeros((0, 3)), r[None])
    assert res.iae.shape == (0, 1, 3, 2) and res.tv.shape == (0, 1, 3, 2) and res.tseg.tolist() == [0, 9, 40]
    res = segment_indices(np.zeros((0, 2, 8)), np.zeros((0, 1, 8)), np.zeros((1, 2, 8)), [0, 4, 8])
    assert res.rise.shape == (0, 1, 2, 2) and res.rise.dtype == np.int32 and res.u_hi.shape == (0, 1, 1, 2)
    if has_gpu:
        return
    with pytest.raises(MpctError, match=r"\(-3\)"):
        segment_indices(np.zeros((1, 2, 8)), np.zeros((1, 1, 8)), np.zeros((1, 2, 8)), [0, 4, 8])
    with pytest.raises(MpctError, match=r"\(-3\)"):
        eval_segment_indices(sc, [5], [2], np.ones((1, 3)), np.ones((1, 3)), r[None])


def test_segment_result_costs():
    from mpct.engine import RobustResult, RobustSegmentResult, SegmentResult

    tseg = np.array([2, 10, 30], dtype=np.int32)
    z = lambda *v: np.array(v, dtype=float).reshape(3, 1, 2, 2)           # noqa: E731 -- (C, nref, my, nseg)
    res = SegmentResult(
        tseg=tseg,
        over=z(0.1, 0.2, 0.0, 0.4,   0.5, 0.1, 0.1, 0.1,   np.nan, 0.1, 0.1, 0.1),
        e_final=z(-0.5, 0.1, 0.2, 0.0,   0.0, 0.0, 0.0, -0.25,   np.nan, 0.0, 0.0, 0.0),
        settle=z(4, 15, 2, 10,   10, 12, 3, 11,   -1, 12, 3, 11).astype(np.int32),
        rise=z(2, 3, -1, 5,   -1, -1, -1, -1,   -1, 20, 1, 1).astype(np.int32))
    c = res.costs(("over", "e_final"))
    assert c.shape == (3, 2) and c[0].tolist() == [0.4, 0.5] and c[1].tolist() == [0.5, 0.25] and np.isnan(c[2]).all()
    assert res.costs(("over",), reduce="sum")[0, 0] == 0.1 + 0.2 + 0.0 + 0.4
    assert res.costs(("over",), segments=(0,))[:2, 0].tolist() == [0.1, 0.5]
    # settle: samples after the segment's start; the segment's end is "not settled"; -1 is invalid
    s = res.costs(("settle",))
    assert s[0, 0] == 5.0 and np.isnan(s[1, 0]) and np.isnan(s[2, 0])      # candidate 1: settle = 10 = tseg[1] in segment 0
    assert res.costs(("settle",), segments=(1,))[:2, 0].tolist() == [5.0, 2.0]
    # rise: -1 beside a valid settle is "no step" and neutral; no step anywhere is NaN; the segment's length is NaN;
    # -1 beside an invalid settle is an invalid unit
    ri = res.costs(("rise",))
    assert ri[0, 0] == 5.0 and np.isnan(ri[1, 0]) and np.isnan(ri[2, 0])
    assert res.costs(("rise",), reduce="sum")[0, 0] == 10.0
    assert res.costs(("rise",), segments=(0,))[0, 0] == 2.0
    with pytest.raises(ValueError):
        res.costs(("tv",))
    with pytest.raises(ValueError):
        res.costs(("nope",))
    with pytest.raises(ValueError):
        res.costs(("over",), segments=(2,))
    with pytest.raises(ValueError):
        res.costs(("over",), reduce="mean")
    # the robust counterpart: columns (field, channel, segment)
    cols = [(f, ch, g) for f in ("over", "rise") for ch in range(2) for g in range(2)]
    tab = np.arange(3 * 8, dtype=float).reshape(3, 8)
    rb = RobustResult(mean=np.zeros((3, 2)), worst=np.zeros((3, 2)), n_failed=np.array([0, 1, 0], dtype=np.int32),
                      worst_draw=np.zeros(3, dtype=np.int32), status=np.zeros(3, dtype=np.int32), draws=2)
    rr = RobustSegmentResult(columns=cols, n=tab, mean=tab, lo=tab, lo_draw=tab, hi=tab, hi_draw=tab, base=rb, tseg=tseg)
    assert rr.costs("hi").shape == (3, 8) and np.isnan(rr.costs("hi")[1]).all()
    assert rr.costs("hi", names=("rise",), segments=(1,), max_failed=1).tolist() == [[5.0, 7.0], [13.0, 15.0], [21.0, 23.0]]
    assert rr.costs("mean", names=("rise", "over"), segments=(0,))[0].tolist() == [4.0, 6.0, 0.0, 2.0]
    assert rr.columns == cols
    with pytest.raises(ValueError):
        rr.costs("hi", names=("tv",))
