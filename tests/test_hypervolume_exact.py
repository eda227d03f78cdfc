"""CPU: the contract of mpct_hypervolume_exact (include/mpct.h) without a device: the header and
the exports, the argument errors in their documented order against both entries, the empty call, and the
references of tests/hvx_ref.py against each other, against tests/hv_ref.py's 2-D sweep and inclusion-exclusion,
and against the torch path of dist.hypervolume_exact_candidates, within (M^2 + 8) 2^-53 vol."""
import ctypes as C
import os
import re
from fractions import Fraction

import numpy as np
import pytest

import hv_ref
import hvx_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_declares_and_lib_exports(built):
    from mpct import _lib

    src = open(os.path.join(ROOT, "include", "mpct.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    so = C.CDLL(_lib.lib_path())
    for f in ("mpct_hypervolume_exact_device", "mpct_hypervolume_exact"):
        assert re.search(r"\bint32_t %s\s*\(" % f, code), f
        assert f in _lib.EXPORTS and f in src.split("#ifndef MPCT_H")[0]      # named in the opening comment
        assert C.cast(getattr(so, f), C.c_void_p).value
    assert re.search(r"typedef struct mpct_hvx_result \{\s*double\*\s+hv;.*?double\*\s+excl;.*?int64_t\*\s+n_active;"
                     r".*?\} mpct_hvx_result;", src, flags=re.S)
    for name, val in (("MPCT_HVX_MAX_OBJ", 3), ("MPCT_HVX_MAX_M", 65536)):
        assert re.search(r"#define %s\s+%d\b" % (name, val), code)
    assert (_lib.HVX_MAX_OBJ, _lib.HVX_MAX_M) == (3, 65536)
    assert [n for n, _ in _lib.MpctHvxResult._fields_] == ["hv", "excl", "n_active"]
    assert _lib.load().mpct_abi_version() == 7


def test_argument_errors_in_documented_order(built):
    """Each call also carries every LATER error of the header's list, so the code that comes back shows the
    order of the checks: k < 1, k > 3, C or M < 0, C above its cap, M above its cap, NULL costs, NULL members
    with M != C, NULL box, no output; then, in the host entry alone, the box's values and the members' range."""
    from mpct import _lib

    lib = _lib.load()
    EINVAL, ERANGE = -1, -4
    buf = np.zeros(16, dtype=np.float64)
    p = buf.ctypes.data_as(_lib.c_double_p)
    A = np.zeros((4, 3))
    a = A.ctypes.data
    mem = np.array([0, 7, -2, 1], dtype=np.int32)          # out of range at both ends
    m = mem.ctypes.data
    bad = np.array([0.0, np.inf, 1.0])                     # a box that is not finite, and empty in column 0
    b = bad.ctypes.data
    lo, ref = np.zeros(3), np.ones(3)
    none = _lib.MpctHvxResult(None, None, None)
    some = _lib.MpctHvxResult(p, None, None)
    steps = [  # (costs, C, k, members, M, lo, ref, out)
        ((None, -1, 0, None, -1, None, None, none), EINVAL, "k < 1"),
        ((None, -1, 4, None, -1, None, None, none), ERANGE, "MPCT_HVX_MAX_OBJ"),
        ((None, -1, 16, None, -1, None, None, none), ERANGE, "MPCT_HVX_MAX_OBJ"),
        ((None, -1, 3, None, 65537, None, None, none), EINVAL, "C < 0 or M < 0"),
        ((None, 1048577, 3, None, -1, None, None, none), EINVAL, "C < 0 or M < 0"),
        ((None, 1048577, 3, None, 65537, None, None, none), ERANGE, "MPCT_PARETO_MAX_C"),
        ((None, 5, 3, None, 65537, None, None, none), ERANGE, "MPCT_HVX_MAX_M"),
        ((None, 5, 3, None, 4, None, None, none), EINVAL, "costs is NULL"),
        ((a, 5, 3, None, 4, None, None, none), EINVAL, "members is NULL"),
        ((a, 4, 3, m, 4, None, b, none), EINVAL, "lo or ref is NULL"),
        ((a, 4, 3, m, 4, b, None, none), EINVAL, "lo or ref is NULL"),
        ((a, 4, 3, m, 4, b, b, none), EINVAL, "no output pointer"),
        ((a, 4, 3, m, 4, b, b, None), EINVAL, "no output pointer"),
    ]
    for args, code, msg in steps:
        o = C.byref(args[7]) if args[7] is not None else None
        for rc in (lib.mpct_hypervolume_exact_device(*args[:7], o, None), lib.mpct_hypervolume_exact(*args[:7], -1, o)):
            assert rc == code, (args[1:5], rc)
            assert msg in _lib.last_error(), (args[1:5], _lib.last_error())
    host_only = [
        ((a, 4, 3, m, 4, b, b, some), "finite lo and ref"),                     # lo == ref
        ((a, 4, 3, m, 4, lo.ctypes.data, b, some), "finite lo and ref"),        # ref = +inf in column 1
        ((a, 4, 3, m, 4, ref.ctypes.data, lo.ctypes.data, some), "finite lo and ref"),   # lo > ref
        ((a, 4, 3, m, 4, lo.ctypes.data, ref.ctypes.data, some), "entry of members"),
    ]
    for args, msg in host_only:
        assert lib.mpct_hypervolume_exact(*args[:7], -1, C.byref(args[7])) == EINVAL
        assert msg in _lib.last_error(), _lib.last_error()
    assert (buf == 0).all()                                # nothing was written


def test_empty_members_and_no_device(built, has_gpu):
    from mpct.engine import MpctError, hypervolume_exact

    res = hypervolume_exact(np.zeros((0, 2)), lo=[0.0, 0.0], ref=[1.0, 2.0])     # M = 0 needs no device
    assert (res.hv, res.n_active, res.vol) == (0.0, 0, 2.0) and not np.signbit(res.hv)
    assert res.excl.size == 0 and res.contribution().size == 0
    res = hypervolume_exact(np.random.default_rng(1).random((5, 2)), members=[], lo=[0.0, 0.0], ref=[1.0, 2.0])
    assert res.hv == 0.0 and res.n_active == 0 and res.members.size == 0
    with pytest.raises(MpctError, match=r"\(-4\).*MPCT_HVX_MAX_OBJ"):             # never the estimator instead
        hypervolume_exact(np.zeros((0, 4)), lo=np.zeros(4), ref=np.ones(4))
    if not has_gpu:
        with pytest.raises(MpctError, match=r"\(-3\).*HIP device"):
            hypervolume_exact(np.random.default_rng(1).random((10, 3)))


# ---- the references against each other and the torch path --------------------------------------
BOXES = {1: (np.array([-2.5]), np.array([0.75])),
         2: (np.array([0.125, -1e-3]), np.array([3.0, 1e3])),
         3: (np.array([-3.0, 2.0, 1e-4]), np.array([-3.0 + 1e-3, 2.0 + 1e3, 7.0]))}


def _case(k, M, seed):
    lo, ref = BOXES[k]
    rng = np.random.default_rng(seed)
    A = lo + (rng.random((M + 4, k)) * 1.25 - 0.1) * (ref - lo)
    A[1, k - 1] = np.nan
    mem = rng.integers(-1, M + 4, M)
    if M > 2:
        mem[2] = mem[0]                                    # a duplicated index
    return A, mem, lo, ref


def _close(got, want, M, vol, what):
    hv, excl, na = got
    HV, EXCL, NA = want
    bd = R.bound(M, vol)
    assert na == NA, what
    assert abs(Fraction(float(hv)) - HV) <= bd, what
    for e, E in zip(np.asarray(excl).tolist(), EXCL):
        assert abs(Fraction(e) - E) <= bd, what
        assert E != 0 or (e == 0.0 and not np.signbit(e)), what


@pytest.mark.parametrize("k,M", [(1, 1), (1, 33), (2, 2), (2, 48), (3, 1), (3, 17), (3, 48)])
def test_sweep_and_torch_path_against_exact_fractions(k, M):
    import torch
    from mpct.dist import hypervolume_exact_candidates

    A, mem, lo, ref = _case(k, M, 10 * k + M)
    want = R.exact_fraction(A, mem, lo, ref)
    vol = hv_ref.volume(lo, ref)
    _close(R.sweep_numpy(A, mem, lo, ref), want, M, vol, "numpy sweep")
    d = hypervolume_exact_candidates(torch.from_numpy(A), torch.from_numpy(mem), lo=lo, ref=ref)
    _close((d["hv"], d["excl"].numpy(), d["n_active"]), want, M, vol, "torch path")
    assert d["excl"].dtype == torch.float64 and d["excl"].shape == (M,)
    if k == 2:
        assert abs(hv_ref.exact_2d(A, mem, lo, ref) - float(want[0])) <= 1e-12 * vol
    if want[2] <= 12:
        assert abs(hv_ref.exact_ie(A, mem, lo, ref) - float(want[0])) <= 1e-12 * vol


def test_lattice_reference_against_fractions_and_sweep():
    rng = np.random.default_rng(4)
    for k, hi in ((1, (40,)), (2, (9, 7)), (3, (6, 5, 7))):
        I = np.stack([rng.integers(-1, h + 1, 40) for h in hi], axis=1)     # some below lo, some on the face
        mem = rng.integers(-1, 40, 36)
        ilo, iref = np.zeros(k, dtype=np.int64), np.array(hi)
        hv, excl, na = R.exact_lattice(I, mem, ilo, iref)
        HV, EXCL, NA = R.exact_fraction(I.astype(float), mem, ilo.astype(float), iref.astype(float))
        assert (hv, na) == (HV, NA) and excl.tolist() == EXCL
        s = R.sweep_numpy(I.astype(float), mem, ilo.astype(float), iref.astype(float))
        assert s[0] == hv and s[1].tolist() == excl.tolist() and s[2] == na   # integers: the sweep is exact


def test_dist_rejects_what_the_library_rejects():
    import torch
    from mpct.dist import hypervolume_exact_candidates

    with pytest.raises(ValueError, match="three objectives"):
        hypervolume_exact_candidates(torch.zeros(5, 4, dtype=torch.float64), lo=np.zeros(4), ref=np.ones(4))
    with pytest.raises(ValueError, match="lo < ref"):
        hypervolume_exact_candidates(torch.zeros(5, 2, dtype=torch.float64), lo=np.ones(2), ref=np.ones(2))


def test_result_methods_feed_the_front(built, monkeypatch):
    """ParetoResult / RobustResult / RobustIndexResult.hypervolume_exact pass the front on as the members"""
    from mpct import engine

    seen = {}

    def fake(costs, members=None, **kw):
        seen["members"], seen["kw"], seen["shape"] = np.asarray(members), kw, np.asarray(costs).shape
        return "result"

    monkeypatch.setattr(engine, "hypervolume_exact", fake)
    pr = engine.ParetoResult(dom_count=np.zeros(4, dtype=np.int32), layer=None, front=np.array([0, 2], dtype=np.int32))
    assert pr.hypervolume_exact(np.zeros((4, 3)), lo=[0, 0, 0], device=1) == "result"
    assert seen["members"].tolist() == [0, 2] and seen["kw"] == dict(lo=[0, 0, 0], device=1) and seen["shape"] == (4, 3)
