"""CPU, no device: the hypervolume contract of include/mpct.h.  The reference of tests/hv_ref.py has the
properties it should have and its estimate lies within four binomial standard deviations of an exact
hypervolume (a sweep at k = 2, inclusion-exclusion at k = 3, 5); the header and the ctypes list carry the
exports; every argument error comes back in the documented order without a device; the host entry fails
loudly without a GPU; the CPU path of mpct.dist.hypervolume_candidates equals the reference; the default box."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import hv_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def front_2d(n=40):
    """n points on a convex trade-off curve: an antichain"""
    x = np.linspace(0.05, 0.95, n)
    return np.stack([x, (1.0 - np.sqrt(x)) ** 2], axis=1)


def _case(k=3, Cn=60, N=3000, seed=5):
    A = R.generated(Cn, k, 10)
    lo, ref = np.zeros(k), np.full(k, 9.5)
    return A, lo, ref, N, seed


# ---- the reference's own properties -----------------------------------------------------------
def test_vectorised_equals_scalar():
    A, lo, ref, _, seed = _case(3, 20, 0)
    A[3, 1] = np.nan
    mem = np.array([4, -1, 3, 7, 7, 19, 0, 2], dtype=np.int32)
    R.compare(R.hv_np(A, mem, lo, ref, 400, seed), R.hv_scalar(A, mem, lo, ref, 400, seed), "subset")
    R.compare(R.hv_np(A, None, lo, ref, 300, seed, budget=1000), R.hv_scalar(A, None, lo, ref, 300, seed), "all, chunked")
    u = R.unit(123456789, 5, 9, 4)
    assert u.tolist() == [[R.unit_scalar(123456789, i, j) for j in range(4)] for i in range(5, 9)]
    assert R.unit_scalar(0, 0, 0) == float(0xE220A8397B1DCDAF >> 11) * 2.0 ** -53    # splitmix64's first output for seed 0


@pytest.mark.parametrize("k", [1, 2, 3, 7])
def test_reference_properties(k):
    A, lo, ref, N, seed = _case(k)
    mem = np.random.default_rng(1).permutation(60)[:35].astype(np.int32)
    ncov, excl, hist, hv = R.hv_np(A, mem, lo, ref, N, seed)
    assert excl.sum() == hist[1] and hist.sum() == N and ncov == N - hist[0] and 0 < ncov < N
    assert hv == (ncov / N) * R.volume(lo, ref)
    # permuting the members permutes excl and changes nothing else
    perm = np.random.default_rng(2).permutation(mem.size)
    got = R.hv_np(A, mem[perm], lo, ref, N, seed)
    R.compare(got, (ncov, excl[perm], hist, hv), "permuted")
    # a dominated member covers only what its dominators cover: n_covered stays, its own excl is 0, and
    # every excl stays but those of its dominators, which lose the points it now shares with them (depth 2)
    top = int(mem[np.argmax(excl)])
    B = np.vstack([A, A[top] + 1.0])
    got = R.hv_np(B, np.append(mem, 60).astype(np.int32), lo, ref, N, seed)
    above = (A[mem] <= B[60]).all(axis=1)
    assert above[np.argmax(excl)] and got[0] == ncov and got[1][-1] == 0
    assert (got[1][:-1][~above] == excl[~above]).all() and (got[1][:-1][above] <= excl[above]).all()
    # dominated and outside the box: it covers no point, so neither n_covered nor any excl changes
    B[60] = A[top] + 10.0
    R.compare(R.hv_np(B, np.append(mem, 60).astype(np.int32), lo, ref, N, seed), (ncov, np.append(excl, 0), hist, hv), "outside")
    # a duplicated member: both copies get 0, the others keep theirs
    m = int(np.argmax(excl))
    assert excl[m] > 0
    got = R.hv_np(A, np.append(mem, mem[m]).astype(np.int32), lo, ref, N, seed)
    assert got[0] == ncov and got[1][m] == 0 and got[1][-1] == 0
    keep = np.arange(mem.size) != m
    assert (got[1][:-1][keep] == excl[keep]).all()
    # a NaN member and a -1 entry cover nothing
    B = A.copy()
    B[mem[m], k - 1] = np.nan
    skipped = mem.copy()
    skipped[m] = -1
    R.compare(R.hv_np(B, mem, lo, ref, N, seed), R.hv_np(A, skipped, lo, ref, N, seed), "NaN against -1")
    assert R.hv_np(B, mem, lo, ref, N, seed)[1][m] == 0
    assert R.hv_np(A, np.full(5, -1, dtype=np.int32), lo, ref, N, seed)[2].tolist() == [N] + [0] * 7


def test_signed_zero_and_box_edges():
    lo, ref = np.array([0.0, 0.0]), np.array([1.0, 2.0])
    a = R.hv_np(np.array([[-0.0, 0.0]]), None, lo, ref, 500, 3)
    b = R.hv_np(np.array([[0.0, -0.0]]), None, lo, ref, 500, 3)
    R.compare(a, b, "signed zeros")
    assert a[0] == 500 and a[1].tolist() == [500]          # the corner lo covers every point, p == lo included
    assert R.hv_np(np.array([[-np.inf, -5.0]]), None, lo, ref, 500, 3)[0] == 500
    assert R.hv_np(np.array([[0.5, np.inf], [1.0, 0.0], [0.0, 2.0]]), None, lo, ref, 500, 3)[0] == 0   # p < ref
    for seed in (0, 1, 2 ** 64 - 1):
        P = R.points([-3.0, 1e-3, 5.0], [-1.0, 1e3, 5.5], seed, 0, 20000)
        assert (P >= [-3.0, 1e-3, 5.0]).all() and (P <= [-1.0, 1e3, 5.5]).all()
        u = R.unit(seed, 0, 20000, 3)
        assert 0.0 <= u.min() and u.max() < 1.0 and abs(u.mean() - 0.5) < 0.01


# ---- the estimator against exact hypervolumes -------------------------------------------------
def _sigmas(A, mem, lo, ref, N, seed, exact):
    p = exact / R.volume(lo, ref)
    assert 0.05 < p < 0.95
    z = (R.hv_np(A, mem, lo, ref, N, seed)[0] / N - p) / math.sqrt(p * (1.0 - p) / N)
    print("seed %d: p = %.6f, %+.2f standard deviations" % (seed, p, z))
    return z


@pytest.mark.parametrize("seed", [0, 1, 2, 3])
def test_estimator_2d_against_sweep(seed):
    A = front_2d(40)
    lo, ref = np.zeros(2), np.ones(2)
    exact = R.exact_2d(A, None, lo, ref)
    assert abs(exact - R.exact_ie(A[::4], None, lo, ref)) < 0.1 and exact > R.exact_ie(A[::4], None, lo, ref)
    assert abs(_sigmas(A, None, lo, ref, 1 << 16, seed, exact)) <= 4.0


@pytest.mark.parametrize("k,seed", [(3, 0), (3, 1), (5, 0), (5, 1)])
def test_estimator_against_inclusion_exclusion(k, seed):
    A = np.random.default_rng(11).uniform(0.0, 0.8, (10, k))
    A[9] = A[0] + 0.05                                       # a dominated member
    A[8, 0] = -0.3                                           # one below lo: clipped
    lo, ref = np.zeros(k), np.ones(k)
    exact = R.exact_ie(A, None, lo, ref)
    assert abs(_sigmas(A, None, lo, ref, 1 << 16, seed, exact)) <= 4.0


def test_exact_references_agree():
    A = np.random.default_rng(4).uniform(-0.2, 1.1, (12, 2))
    lo, ref = np.zeros(2), np.ones(2)
    assert abs(R.exact_2d(A, None, lo, ref) - R.exact_ie(A, None, lo, ref)) < 1e-12
    assert R.exact_2d(np.array([[0.25, 0.5]]), None, lo, ref) == 0.375
    assert R.exact_ie(np.array([[0.5, 0.5, 0.5], [0.5, 0.5, 0.5]]), None, np.zeros(3), np.ones(3)) == 0.125


# ---- the library without a device -------------------------------------------------------------
def test_header_declares_and_lib_exports(built):
    from mpct import _lib

    src = open(os.path.join(ROOT, "include", "mpct.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    so = C.CDLL(_lib.lib_path())
    for f in ("mpct_hypervolume_device", "mpct_hypervolume"):
        assert re.search(r"\bint32_t %s\s*\(" % f, code), f
        assert f in _lib.EXPORTS
        assert C.cast(getattr(so, f), C.c_void_p).value
    assert re.search(r"typedef struct mpct_hv_result \{\s*int64_t\* n_covered;.*?int64_t\* excl;.*?int64_t\* depth_hist;"
                     r".*?double\* hv;.*?\} mpct_hv_result;", code, flags=re.S)
    for name, val in (("MPCT_HV_MAX_SAMPLES", 1 << 30), ("MPCT_HV_BINS", 8)):
        assert re.search(r"#define %s %d\b" % (name, val), code)
    assert (_lib.HV_MAX_SAMPLES, _lib.HV_BINS) == (1 << 30, 8)
    assert [n for n, _ in _lib.MpctHvResult._fields_] == ["n_covered", "excl", "depth_hist", "hv"]
    assert "mpct_internal_hv_tuned" not in src and C.cast(so.mpct_internal_hv_tuned, C.c_void_p).value
    assert "mpct_internal_hv_tuned" not in _lib.EXPORTS
    assert _lib.load().mpct_abi_version() == 7


def test_argument_errors_in_documented_order(built):
    """Each call also carries every LATER error of the header's list, so the code that comes back shows the
    order of the checks: k, C or M < 0, the caps, N above its cap, N < 1, NULL costs, NULL members with
    M != C, NULL box, no output; then, in the host entry alone, the box's values and the members' range."""
    from mpct import _lib

    lib = _lib.load()
    EINVAL, ERANGE = -1, -4
    buf = np.zeros(16, dtype=np.int64)
    p = buf.ctypes.data_as(_lib.c_int64_p)
    A = np.zeros((4, 3))
    a = A.ctypes.data
    mem = np.array([0, 7, -2, 1], dtype=np.int32)          # out of range at both ends
    m = mem.ctypes.data
    bad = np.array([0.0, np.inf, 1.0])                     # a box that is not finite, and empty in column 0
    b = bad.ctypes.data
    lo, ref = np.zeros(3), np.ones(3)
    none = _lib.MpctHvResult(None, None, None, None)
    some = _lib.MpctHvResult(p, None, None, None)
    big = (1 << 30) + 1
    steps = [  # (costs, C, k, members, M, lo, ref, N, out)
        ((None, -1, 0, None, -1, None, None, big, none), EINVAL, "k must be"),
        ((None, -1, 17, None, -1, None, None, big, none), EINVAL, "k must be"),
        ((None, -1, 3, None, 5, None, None, big, none), EINVAL, "C < 0 or M < 0"),
        ((None, 5, 3, None, -1, None, None, big, none), EINVAL, "C < 0 or M < 0"),
        ((None, 1048577, 3, None, 5, None, None, big, none), ERANGE, "MPCT_PARETO_MAX_C"),
        ((None, 5, 3, None, 1048577, None, None, big, none), ERANGE, "MPCT_PARETO_MAX_C"),
        ((None, 5, 3, None, 4, None, None, big, none), ERANGE, "MPCT_HV_MAX_SAMPLES"),
        ((None, 5, 3, None, 4, None, None, 0, none), EINVAL, "n_samples < 1"),
        ((None, 5, 3, None, 4, None, None, 10, none), EINVAL, "costs is NULL"),
        ((a, 5, 3, None, 4, None, None, 10, none), EINVAL, "members is NULL"),
        ((a, 4, 3, m, 4, None, b, 10, none), EINVAL, "lo or ref is NULL"),
        ((a, 4, 3, m, 4, b, None, 10, none), EINVAL, "lo or ref is NULL"),
        ((a, 4, 3, m, 4, b, b, 10, none), EINVAL, "no output pointer"),
        ((a, 4, 3, m, 4, b, b, 10, None), EINVAL, "no output pointer"),
    ]
    for args, code, msg in steps:
        o = C.byref(args[8]) if args[8] is not None else None
        for rc in (lib.mpct_hypervolume_device(*args[:8], 0, o, None), lib.mpct_hypervolume(*args[:8], 0, -1, o)):
            assert rc == code, (args[1:5], args[7], rc)
            assert msg in _lib.last_error(), (args[1:5], _lib.last_error())
    host_only = [
        ((a, 4, 3, m, 4, b, b, 10, some), "finite lo and ref"),                     # lo == ref
        ((a, 4, 3, m, 4, lo.ctypes.data, b, 10, some), "finite lo and ref"),        # ref = +inf in column 1
        ((a, 4, 3, m, 4, ref.ctypes.data, lo.ctypes.data, 10, some), "finite lo and ref"),   # lo > ref
        ((a, 4, 3, m, 4, lo.ctypes.data, ref.ctypes.data, 10, some), "entry of members"),
    ]
    for args, msg in host_only:
        assert lib.mpct_hypervolume(*args[:8], 0, -1, C.byref(args[8])) == EINVAL
        assert msg in _lib.last_error(), _lib.last_error()
    for tile, blocks in ((64, 0), (0, -1)):
        assert lib.mpct_internal_hv_tuned(tile, blocks) == EINVAL
    assert lib.mpct_internal_hv_tuned(0, 0) == 0
    assert (buf == 0).all()                                # nothing was written


def test_empty_members_and_no_device(built, has_gpu):
    from mpct import _lib
    from mpct.engine import MpctError, hypervolume

    res = hypervolume(np.zeros((0, 2)), lo=[0.0, 0.0], ref=[1.0, 2.0], n_samples=77)     # M = 0 needs no device
    assert (res.hv, res.n_covered, res.n_samples, res.volume) == (0.0, 0, 77, 2.0)
    assert res.excl.size == 0 and res.depth_hist.tolist() == [77] + [0] * 7 and res.contribution.size == 0
    res = hypervolume(R.generated(5, 2), members=[], lo=[0.0, 0.0], ref=[1.0, 2.0], n_samples=9)
    assert res.depth_hist.tolist() == [9] + [0] * 7 and res.members.size == 0
    if not has_gpu:
        with pytest.raises(MpctError, match=r"\(-3\).*HIP device"):
            hypervolume(R.generated(10, 3), n_samples=100)
    assert _lib.HV_BINS == 8


# ---- the bindings -----------------------------------------------------------------------------
@pytest.mark.parametrize("Cn,k,N,seed", [(130, 3, 5000, 0), (300, 7, 4100, 9), (40, 1, 1000, 2 ** 64 - 1), (70, 16, 3000, 1)])
def test_dist_cpu_path_equals_reference(Cn, k, N, seed):
    import torch
    from mpct.dist import hypervolume_candidates

    A = R.generated(Cn, k, 10)
    A[5, 0] = np.nan
    A[6] = np.inf
    A[7] = -np.inf if k > 1 else A[7]
    lo, ref = np.zeros(k), np.full(k, 9.5)
    mem = np.random.default_rng(3).permutation(Cn)[:Cn // 2].astype(np.int32)
    mem[4], mem[9] = -1, mem[8]                             # a skipped entry and a duplicate
    for members in (None, mem):
        want = R.hv_np(A, members, lo, ref, N, seed)
        got = hypervolume_candidates(torch.from_numpy(A), None if members is None else torch.from_numpy(members),
                                     lo=lo, ref=ref, n_samples=N, seed=seed)
        R.compare((got["n_covered"], got["excl"].numpy(), got["depth_hist"].numpy(), got["hv"]), want, "dist")
        assert got["n_samples"] == N
    # the C argument cuts the sentinel padding of a gathered tensor; the default box is the engine's
    from mpct.engine import default_box

    sub = A[8:Cn - 7]
    got = hypervolume_candidates(torch.from_numpy(A[8:]), C=Cn - 15, n_samples=500, seed=4)
    dlo, dref = default_box(sub)
    R.compare((got["n_covered"], got["excl"].numpy(), got["depth_hist"].numpy(), got["hv"]),
              R.hv_np(sub, None, dlo, dref, 500, 4), "dist, default box")
    with pytest.raises(ValueError):
        hypervolume_candidates(torch.zeros((3, 17), dtype=torch.float64), lo=np.zeros(17), ref=np.ones(17))
    with pytest.raises(ValueError):
        hypervolume_candidates(torch.zeros((3, 2), dtype=torch.float64), lo=np.ones(2), ref=np.ones(2))


def test_default_box(built):
    from mpct.engine import HypervolumeResult, box_volume, default_box, hypervolume

    A = np.array([[1.0, 5.0, -2.0, 0.0], [3.0, 5.0, -2.0, 0.0], [2.0, 5.0, -2.0, 0.0], [np.nan, 100.0, 100.0, 100.0],
                  [50.0, 50.0, 50.0, 50.0]])
    lo, ref = default_box(A, members=[0, 1, -1, 2, 3])
    assert lo.tolist() == [1.0, 5.0, -2.0, 0.0]            # the NaN row and the non-member do not count
    assert ref.tolist() == [3.0 + 0.1 * 2.0, 5.0 + 0.1 * 5.0, -2.0 + 0.1 * 2.0, 0.0 + 0.1 * 1.0]
    lo, ref = default_box(A, members=[0, 1], ref=[9.0, 9.0, 9.0, 9.0])
    assert lo.tolist() == [1.0, 5.0, -2.0, 0.0] and ref.tolist() == [9.0] * 4
    lo, ref = default_box(A, lo=0.0, ref=[4.0, 6.0, 1.0, 1.0])      # nothing to compute: NaN rows do not matter
    assert lo.tolist() == [0.0] * 4
    assert box_volume(lo, ref) == ((((1.0 * 4.0) * 6.0) * 1.0) * 1.0)
    for bad in (np.array([[1.0, np.inf], [2.0, 3.0]]), np.array([[1.0, -np.inf], [2.0, 3.0]])):
        with pytest.raises(ValueError, match="explicit"):
            hypervolume(bad, n_samples=10)
    with pytest.raises(ValueError, match="explicit"):
        hypervolume(np.full((3, 2), np.nan), n_samples=10)
    with pytest.raises(ValueError, match="explicit"):
        default_box(A, lo=[0.0, 0.0, 0.0, -np.inf], ref=[1.0] * 4)
    r = HypervolumeResult(hv=1.0, n_covered=5, n_samples=10, excl=np.array([2, 0, 3]), depth_hist=np.zeros(8, dtype=np.int64),
                          lo=np.zeros(2), ref=np.array([2.0, 4.0]), volume=8.0)
    assert r.contribution.tolist() == [1.6, 0.0, 2.4]


def test_result_methods_feed_the_front(built, monkeypatch):
    """ParetoResult.hypervolume passes its front as the members; RobustResult.hypervolume builds the table
    of its pareto, takes the front and passes both on (the device calls are replaced: no GPU here)."""
    from mpct import engine

    seen = []

    def fake_hv(costs, members=None, **kw):
        seen.append((np.array(costs), np.array(members), kw))
        return "hv"

    def fake_pareto(costs, max_layers=0, device=-1):
        return engine.ParetoResult(dom_count=np.zeros(3, dtype=np.int32), layer=None, front=np.array([2, 0], dtype=np.int32))

    monkeypatch.setattr(engine, "hypervolume", fake_hv)
    monkeypatch.setattr(engine, "pareto", fake_pareto)
    T = np.arange(6.0).reshape(3, 2)
    assert fake_pareto(T).hypervolume(T, n_samples=64, seed=3) == "hv"
    assert seen[-1][1].tolist() == [2, 0] and seen[-1][2] == dict(n_samples=64, seed=3)
    res = engine.RobustResult(mean=T, worst=10 + T, n_failed=np.array([0, 2, 1], dtype=np.int32),
                              worst_draw=np.zeros(3, dtype=np.int32), status=np.zeros(3, dtype=np.int32), draws=4,
                              levels=np.array([0.5, 1.0]), quantile=T + 100, cvar=T + 200)
    assert res.hypervolume(stat="mean", max_failed=1, columns=(("cvar", 1),), n_samples=32) == "hv"
    costs, members, kw = seen[-1]
    assert costs.shape == (3, 3) and np.isnan(costs[1]).all() and costs[0].tolist() == [0.0, 1.0, 201.0]
    assert members.tolist() == [2, 0] and kw == dict(device=-1, n_samples=32)
