"""CPU, no device: the Pareto contract of include/mpct.h.  The reference of tests/pareto_ref.py has the
properties it should have; the comparison helper notices a single count off by one; the header and the
ctypes list carry the exports; every argument error comes back in the documented order without a device;
the host entry fails loudly without a GPU; the CPU path of mpct.dist.pareto_candidates equals the reference."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import pareto_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = [(40, 1, 4), (60, 2, 5), (90, 3, 4), (70, 7, 3), (33, 16, 2)]


def _with_nan(Cn, k, hi):
    A = R.generated(Cn, k, hi)
    A[3, k - 1] = np.nan
    A[Cn - 1, 0] = np.nan
    return A


@pytest.mark.parametrize("Cn,k,hi", CASES)
def test_reference_properties(Cn, k, hi):
    A = _with_nan(Cn, k, hi)
    dom, layer, front, nf = R.pareto_scalar(A, 64)
    R.compare(R.pareto_np(A, 64), (dom, layer, front, nf), "vectorised against scalar")
    members = front[:nf].tolist()
    assert members == sorted(members) and (front[nf:] == -1).all() and nf >= 1
    assert dom[3] == -1 and layer[3] == -1 and 3 not in members
    # the front is an antichain
    assert not any(R.dominates(A[a], A[b]) for a in members for b in members)
    # every valid candidate off the front is dominated by a member of the front
    for c in range(Cn):
        if dom[c] > 0:
            assert any(R.dominates(A[a], A[c]) for a in members)
    # layers from peeling equal the recursion 1 + max over the dominators
    np.testing.assert_array_equal(layer, R.layers_by_recursion(A))
    for L in (1, 2):
        clamped = R.pareto_scalar(A, L)[1]
        np.testing.assert_array_equal(clamped, np.where(layer < 0, -1, np.minimum(layer, L)))
    if k == 1:   # one objective: the front is all the minima
        lo = np.nanmin(A)
        assert members == [c for c in range(Cn) if A[c, 0] == lo]
    # equivariance under a permutation of the candidates
    perm = np.random.default_rng(1).permutation(Cn)
    pd, pl, pf, pn = R.pareto_np(A[perm], 64)
    np.testing.assert_array_equal(pd, dom[perm])
    np.testing.assert_array_equal(pl, layer[perm])
    assert set(perm[pf[:pn]].tolist()) == set(members)


def test_reference_special_values():
    dom, layer, front, nf = R.pareto_scalar(np.array([[0.0, -0.0], [-0.0, 0.0], [np.inf, np.inf], [-np.inf, 5.0],
                                                      [np.nan, -np.inf]]), 3)
    assert dom.tolist() == [0, 0, 3, 0, -1] and layer.tolist() == [0, 0, 1, 0, -1] and front.tolist() == [0, 1, 3, -1, -1]
    dom, layer, front, nf = R.pareto_scalar(np.full((5, 2), 1.0), 1)
    assert dom.tolist() == [0] * 5 and nf == 5          # duplicates of a front point are all on the front
    assert R.pareto_scalar(np.zeros((0, 3)), 2)[3] == 0


def test_compare_rejects_one_count_off_by_one():
    A = R.generated(50, 3, 4)
    want = R.pareto_np(A, 4)
    R.compare(want, want)
    for f in range(3):
        got = [np.array(x, copy=True) for x in want[:3]] + [want[3]]
        got[f][17] += 1
        with pytest.raises(AssertionError):
            R.compare(tuple(got), want)
    with pytest.raises(AssertionError):
        R.compare(want[:3] + (want[3] + 1,), want)


def test_header_declares_and_lib_exports(built):
    from mpct import _lib

    src = open(os.path.join(ROOT, "include", "mpct.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for f in ("mpct_pareto_device", "mpct_pareto"):
        assert re.search(r"\bint32_t %s\s*\(" % f, code), f
        assert f in _lib.EXPORTS
        assert C.cast(getattr(C.CDLL(_lib.lib_path()), f), C.c_void_p).value
    assert re.search(r"typedef struct mpct_pareto_result \{\s*int32_t\* dom_count;.*?int32_t\* layer;.*?int32_t\* front;"
                     r".*?int32_t\* n_front;.*?\} mpct_pareto_result;", code, flags=re.S)
    for name, val in (("MPCT_PARETO_MAX_OBJ", 16), ("MPCT_PARETO_MAX_C", 1048576), ("MPCT_PARETO_MAX_LAYERS", 64)):
        assert re.search(r"#define %s %d\b" % (name, val), code)
    assert (_lib.PARETO_MAX_OBJ, _lib.PARETO_MAX_C, _lib.PARETO_MAX_LAYERS) == (16, 1048576, 64)
    assert _lib.load().mpct_abi_version() == 7


def _both_entries(costs, Cn, k, L, out):
    """return codes of the two entries for one set of arguments (host pointers: nothing is dereferenced
    before the checks have passed)"""
    from mpct import _lib

    lib = _lib.load()
    o = C.byref(out) if out is not None else None
    return (lib.mpct_pareto_device(costs, Cn, k, L, o, None), lib.mpct_pareto(costs, Cn, k, L, -1, o))


def test_argument_errors_in_documented_order(built):
    """Each call also carries every LATER error of the header's list, so the code that comes back shows
    the order of the checks: k, C < 0, C above the cap, NULL costs, no output, front without n_front, layers."""
    from mpct import _lib

    EINVAL, ERANGE = -1, -4
    buf = np.zeros(8, dtype=np.int32)
    p = buf.ctypes.data_as(_lib.c_int32_p)
    A = np.zeros((4, 3))
    none = _lib.MpctParetoResult(None, None, None, None)
    front_only = _lib.MpctParetoResult(None, p, p, None)        # front without n_front, layer asked for
    layer_only = _lib.MpctParetoResult(None, p, None, None)
    steps = [
        ((None, -1, 0, 65, none), EINVAL, "k must be"),
        ((None, -1, 17, 65, none), EINVAL, "k must be"),
        ((None, -1, 3, 65, none), EINVAL, "C < 0"),
        ((None, 1048577, 3, 65, none), ERANGE, "MPCT_PARETO_MAX_C"),
        ((None, 4, 3, 65, none), EINVAL, "costs is NULL"),
        ((A.ctypes.data, 4, 3, 65, none), EINVAL, "no output pointer"),
        ((A.ctypes.data, 4, 3, 65, None), EINVAL, "no output pointer"),
        ((A.ctypes.data, 4, 3, 65, front_only), EINVAL, "front needs n_front"),
        ((A.ctypes.data, 4, 3, 0, layer_only), EINVAL, "max_layers"),
        ((A.ctypes.data, 4, 3, 65, layer_only), EINVAL, "max_layers"),
        ((A.ctypes.data, 4, 3, -1, _lib.MpctParetoResult(p, None, None, None)), EINVAL, "max_layers"),
    ]
    for args, code, msg in steps:
        for rc in _both_entries(*args):
            assert rc == code, (args[1:4], rc)
            assert msg in _lib.last_error(), (args[1:4], _lib.last_error())
    assert (buf == 0).all()                                     # nothing was written


def test_empty_batch_and_no_device(built, has_gpu):
    from mpct import _lib
    from mpct.engine import MpctError, pareto

    nf = np.full(1, 99, dtype=np.int32)
    out = _lib.MpctParetoResult(None, None, None, nf.ctypes.data_as(_lib.c_int32_p))
    assert _lib.load().mpct_pareto(None, 0, 3, 0, -1, C.byref(out)) == 0 and nf[0] == 0     # C = 0 needs no device
    res = pareto(np.zeros((0, 2)), max_layers=3)
    assert res.front.size == 0 and res.dom_count.size == 0
    if not has_gpu:
        with pytest.raises(MpctError, match=r"\(-3\).*HIP device"):
            pareto(R.generated(10, 3, 4), max_layers=2)


@pytest.mark.parametrize("Cn,k,hi,L", [(257, 3, 6, 8), (300, 7, 6, 0), (1025, 1, 6, 64), (130, 16, 3, 2), (0, 3, 6, 2)])
def test_dist_cpu_fallback_equals_reference(Cn, k, hi, L):
    import torch
    from mpct.dist import pareto_candidates

    A = R.generated(Cn, k, hi)
    if Cn:
        A[5, 0] = np.nan
        A[6] = np.inf
    dom, layer, front, nf = R.pareto_np(A, L)
    got = pareto_candidates(torch.from_numpy(A), max_layers=L)
    np.testing.assert_array_equal(got["dom_count"].numpy(), dom)
    np.testing.assert_array_equal(got["front"].numpy(), front[:nf])
    if L:
        np.testing.assert_array_equal(got["layer"].numpy(), layer)
    else:
        assert "layer" not in got
    # the C argument cuts the sentinel padding of a gathered tensor
    if Cn > 10:
        cut = pareto_candidates(torch.from_numpy(A), C=Cn - 7, max_layers=L)
        np.testing.assert_array_equal(cut["dom_count"].numpy(), R.pareto_np(A[:Cn - 7], L)[0])
    with pytest.raises(ValueError):
        pareto_candidates(torch.zeros((3, 17), dtype=torch.float64))


def test_robust_result_pareto_masks_like_scores(built, monkeypatch):
    """RobustResult.pareto feeds the statistic with the NaN masking of scores, plus the tail columns asked
    for (the device call itself is replaced: no GPU here)."""
    from mpct import engine

    seen = {}

    def fake(costs, max_layers=0, device=-1):
        seen["costs"], seen["L"] = np.array(costs), max_layers
        return "result"

    monkeypatch.setattr(engine, "pareto", fake)
    res = engine.RobustResult(mean=np.arange(6.0).reshape(3, 2), worst=10 + np.arange(6.0).reshape(3, 2),
                              n_failed=np.array([0, 2, 1], dtype=np.int32), worst_draw=np.zeros(3, dtype=np.int32),
                              status=np.zeros(3, dtype=np.int32), draws=4, levels=np.array([0.5, 1.0]),
                              quantile=np.arange(6.0).reshape(3, 2) + 100, cvar=np.arange(6.0).reshape(3, 2) + 200)
    assert res.pareto(stat="mean", max_failed=1, max_layers=3) == "result"
    np.testing.assert_array_equal(seen["costs"], res.scores(1, "mean"))
    assert seen["L"] == 3 and np.isnan(seen["costs"][1]).all()
    res.pareto(columns=(("cvar", 1), ("quantile", 0)))
    assert seen["costs"].shape == (3, 4) and np.isnan(seen["costs"][1:]).all()
    assert seen["costs"][0].tolist() == [10.0, 11.0, 201.0, 100.0]
    with pytest.raises(ValueError):
        res.pareto(columns=(("mean", 0),))
