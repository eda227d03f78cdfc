"""CPU, no device: the hypervolume subset selection contract of include/mpct.h.  The two forms of
tests/hvsel_ref.py agree and have the properties the header states; greedy reaches 1 - (1 - 1/n)^n of the
best n-subset's coverage of the same sample set (brute force at M <= 10); the header and the ctypes list
carry the exports; every argument error comes back in the documented order without a device; the host
entry fails loudly without a GPU and needs none for M = 0; the CPU path of mpct.dist.hv_select_candidates
equals the reference."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import hv_ref as R
import hvsel_ref as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _case(k=3, Cn=40, hi=10):
    return R.generated(Cn, k, hi), np.zeros(k), np.full(k, hi - 0.5)


# ---- the reference's own properties -----------------------------------------------------------
def test_vectorised_equals_scalar():
    A, lo, ref = _case(3, 20)
    A[3, 1] = np.nan
    mem = np.array([4, -1, 3, 7, 7, 19, 0, 2, 25], dtype=np.int32)     # skipped, NaN, duplicate, out of range
    for members, N, K in ((mem, 300, 12), (None, 250, 4), (mem, 1, 3), (np.zeros(0, dtype=np.int32), 50, 2)):
        a, b = S.select_np(A, members, lo, ref, N, 5, K), S.select_scalar(A, members, lo, ref, N, 5, K)
        S.compare(a, b, "np against scalar")
        assert set(a) == set(S.FIELDS) and a["ties"].dtype == np.int32


@pytest.mark.parametrize("k", [1, 2, 3, 7])
def test_reference_properties(k):
    A, lo, ref = _case(k, 60)
    N, seed = 3000, 5
    mem = np.random.default_rng(1).permutation(60)[:35].astype(np.int32)
    want = R.hv_np(A, mem, lo, ref, N, seed)
    got = S.select_np(A, mem, lo, ref, N, seed, mem.size + 5)          # K >= M: the selection ends
    n = got["n_picked"]
    assert 0 < n <= mem.size and (np.diff(got["gain"]) <= 0).all()     # gain is non-increasing
    assert got["covered"][-1] == got["n_covered_all"] == want[0]
    assert got["covered"][n - 1] == want[0] and (got["gain"][:n] > 0).all()
    assert (got["pos"][n:] == -1).all() and (got["index"][n:] == -1).all() and (got["gain"][n:] == 0).all()
    assert (got["ties"][n:] == 0).all() and (got["ties"][:n] >= 1).all() and (got["covered"][n:] == want[0]).all()
    np.testing.assert_array_equal(got["index"][:n], mem[got["pos"][:n]])
    assert len(set(got["pos"][:n].tolist())) == n                      # no member twice
    assert got["hv"][-1] == want[3] and got["hv"][0] == (float(got["gain"][0]) / N) * R.volume(lo, ref)
    # the first pick is the member with the largest coverage of its own
    alone = [R.hv_np(A, mem[m:m + 1], lo, ref, N, seed)[0] for m in range(mem.size)]
    assert got["gain"][0] == max(alone) and got["pos"][0] == int(np.argmax(alone))
    # a shorter call is a prefix
    short = S.select_np(A, mem, lo, ref, N, seed, 3)
    for f in ("pos", "index", "gain", "covered", "ties"):
        np.testing.assert_array_equal(short[f], got[f][:3])
    # permuting the members where every pick was forced permutes pos and changes nothing else
    if (got["ties"][:n] == 1).all():
        perm = np.random.default_rng(2).permutation(mem.size)
        p = S.select_np(A, mem[perm], lo, ref, N, seed, mem.size + 5)
        S.compare(p, got, "permuted", fields=("n_picked", "index", "gain", "covered", "hv", "ties", "n_covered_all"))
        np.testing.assert_array_equal(perm[p["pos"][:n]], got["pos"][:n])


def test_ties_take_the_lowest_position():
    A, lo, ref = _case(3, 30)
    A[7] = A[21] = -1.0                                                # two rows that cover every point
    got = S.select_np(A, None, lo, ref, 500, 3, 4)
    assert got["ties"][0] == 2 and got["pos"][0] == 7 and got["gain"].tolist() == [500, 0, 0, 0] and got["n_picked"] == 1


@pytest.mark.parametrize("seed", [0, 1, 2, 3, 4])
@pytest.mark.parametrize("k", [2, 3, 5])
def test_greedy_bound_against_brute_force(k, seed):
    """M = 10: covered[n - 1] >= (1 - (1 - 1/n)^n) x the best n-subset's coverage, n = 1, 2, 3"""
    A = np.random.default_rng(100 * k + seed).uniform(0.0, 0.8, (10, k))
    lo, ref = np.zeros(k), np.ones(k)
    got = S.select_np(A, None, lo, ref, 2000, seed, 3)
    for n in (1, 2, 3):
        best = S.best_subset(A, None, lo, ref, 2000, seed, n)
        assert best > 0 and got["covered"][n - 1] <= best
        assert got["covered"][n - 1] >= (1.0 - (1.0 - 1.0 / n) ** n) * best, (n, got["covered"], best)
    assert got["covered"][0] == S.best_subset(A, None, lo, ref, 2000, seed, 1)


# ---- the library without a device -------------------------------------------------------------
def test_header_declares_and_lib_exports(built):
    from mpct import _lib

    src = open(os.path.join(ROOT, "include", "mpct.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    so = C.CDLL(_lib.lib_path())
    for f in ("mpct_hv_select_device", "mpct_hv_select"):
        assert re.search(r"\bint32_t %s\s*\(" % f, code), f
        assert f in _lib.EXPORTS
        assert C.cast(getattr(so, f), C.c_void_p).value
    m = re.search(r"typedef struct mpct_hv_select_result \{(.*?)\} mpct_hv_select_result;", code, flags=re.S)
    fields = re.findall(r"(int64_t|int32_t|double)\s*\*\s*(\w+);", m.group(1))
    assert [n for _, n in fields] == list(S.FIELDS) == [n for n, _ in _lib.MpctHvSelectResult._fields_]
    ctype = {"int64_t": _lib.c_int64_p, "int32_t": _lib.c_int32_p, "double": _lib.c_double_p}
    assert [ctype[t] for t, _ in fields] == [t for _, t in _lib.MpctHvSelectResult._fields_]
    assert re.search(r"#define MPCT_HVSEL_MAX_PICKS 1024\b", code) and _lib.HVSEL_MAX_PICKS == 1024
    for hook in ("mpct_internal_hvsel_tuned", "mpct_internal_hvsel_round_ms"):
        assert hook not in src and hook not in _lib.EXPORTS and C.cast(getattr(so, hook), C.c_void_p).value
    assert code.index("} mpct_hv_result;") < code.index("struct mpct_hv_select_result {") < code.index("struct mpct_index_params")
    assert _lib.load().mpct_abi_version() == 7


def test_argument_errors_in_documented_order(built):
    """Each call also carries every LATER error of the header's list, so the code that comes back shows the
    order of the checks: hypervolume's list down to N < 1, n_pick < 1, n_pick above its cap, NULL costs, NULL
    members with M != C, NULL box, no output; then, in the host entry alone, the box's values and the members'
    range."""
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
    none = _lib.MpctHvSelectResult()
    some = _lib.MpctHvSelectResult(n_picked=p)
    big = (1 << 30) + 1
    steps = [  # (costs, C, k, members, M, lo, ref, N, n_pick, out)
        ((None, -1, 0, None, -1, None, None, big, 0, none), EINVAL, "k must be"),
        ((None, -1, 17, None, -1, None, None, big, 0, none), EINVAL, "k must be"),
        ((None, -1, 3, None, 5, None, None, big, 0, none), EINVAL, "C < 0 or M < 0"),
        ((None, 5, 3, None, -1, None, None, big, 0, none), EINVAL, "C < 0 or M < 0"),
        ((None, 1048577, 3, None, 5, None, None, big, 0, none), ERANGE, "MPCT_PARETO_MAX_C"),
        ((None, 5, 3, None, 1048577, None, None, big, 0, none), ERANGE, "MPCT_PARETO_MAX_C"),
        ((None, 5, 3, None, 4, None, None, big, 0, none), ERANGE, "MPCT_HV_MAX_SAMPLES"),
        ((None, 5, 3, None, 4, None, None, 0, 0, none), EINVAL, "n_samples < 1"),
        ((None, 5, 3, None, 4, None, None, 10, 0, none), EINVAL, "n_pick < 1"),
        ((None, 5, 3, None, 4, None, None, 10, -3, none), EINVAL, "n_pick < 1"),
        ((None, 5, 3, None, 4, None, None, 10, 1025, none), ERANGE, "MPCT_HVSEL_MAX_PICKS"),
        ((None, 5, 3, None, 4, None, None, 10, 1024, none), EINVAL, "costs is NULL"),
        ((a, 5, 3, None, 4, None, None, 10, 2, none), EINVAL, "members is NULL"),
        ((a, 4, 3, m, 4, None, b, 10, 2, none), EINVAL, "lo or ref is NULL"),
        ((a, 4, 3, m, 4, b, None, 10, 2, none), EINVAL, "lo or ref is NULL"),
        ((a, 4, 3, m, 4, b, b, 10, 2, none), EINVAL, "no output pointer"),
        ((a, 4, 3, m, 4, b, b, 10, 2, None), EINVAL, "no output pointer"),
    ]
    for args, code, msg in steps:
        o = C.byref(args[9]) if args[9] is not None else None
        for rc in (lib.mpct_hv_select_device(*args[:8], 0, args[8], o, None),
                   lib.mpct_hv_select(*args[:8], 0, args[8], -1, o)):
            assert rc == code, (args[1:5], args[7:9], rc)
            assert msg in _lib.last_error(), (args[1:5], _lib.last_error())
    host_only = [
        ((a, 4, 3, m, 4, b, b, 10, 2, some), "finite lo and ref"),                     # lo == ref
        ((a, 4, 3, m, 4, lo.ctypes.data, b, 10, 2, some), "finite lo and ref"),        # ref = +inf in column 1
        ((a, 4, 3, m, 4, ref.ctypes.data, lo.ctypes.data, 10, 2, some), "finite lo and ref"),   # lo > ref
        ((a, 4, 3, m, 4, lo.ctypes.data, ref.ctypes.data, 10, 2, some), "entry of members"),
    ]
    for args, msg in host_only:
        assert lib.mpct_hv_select(*args[:8], 0, args[8], -1, C.byref(args[9])) == EINVAL
        assert msg in _lib.last_error(), _lib.last_error()
    for tile, blocks in ((64, 0), (0, -1)):
        assert lib.mpct_internal_hvsel_tuned(tile, blocks) == EINVAL
    assert lib.mpct_internal_hvsel_tuned(0, 0) == 0
    assert (buf == 0).all()                                # nothing was written


def test_empty_members_and_no_device(built, has_gpu):
    from mpct.engine import MpctError, hv_select

    res = hv_select(np.zeros((0, 2)), 5, lo=[0.0, 0.0], ref=[1.0, 2.0], n_samples=77)     # M = 0 needs no device
    assert (res.n_picked, res.n_covered_all, res.n_samples, res.volume) == (0, 0, 77, 2.0)
    S.compare(res, S.select_np(np.zeros((0, 2)), None, [0.0, 0.0], [1.0, 2.0], 77, 0, 5), "C = 0")
    assert res.pos.tolist() == [-1] * 5 and res.hv.tolist() == [0.0] * 5 and res.picked.size == 0
    assert res.cut("gain").size == 0 and np.isnan(res.share).all()
    res = hv_select(R.generated(5, 2), 3, members=[], lo=[0.0, 0.0], ref=[1.0, 2.0], n_samples=9)
    assert res.n_picked == 0 and res.index.tolist() == [-1] * 3 and res.ties.tolist() == [0] * 3
    if not has_gpu:
        with pytest.raises(MpctError, match=r"\(-3\).*HIP device"):
            hv_select(R.generated(10, 3), 2, n_samples=100)
    with pytest.raises(MpctError, match=r"\(-1\).*n_pick < 1"):
        hv_select(R.generated(10, 3), 0, n_samples=100)


# ---- the bindings -----------------------------------------------------------------------------
@pytest.mark.parametrize("Cn,k,N,seed,K", [(130, 3, 5000, 0, 12), (90, 7, 4100, 9, 30), (40, 1, 1000, 2 ** 64 - 1, 3),
                                           (70, 16, 3000, 1, 8)])
def test_dist_cpu_path_equals_reference(Cn, k, N, seed, K):
    import torch
    from mpct.dist import hv_select_candidates

    A = R.generated(Cn, k, 10)
    A[5, 0] = np.nan
    A[6] = np.inf
    lo, ref = np.zeros(k), np.full(k, 9.5)
    mem = np.random.default_rng(3).permutation(Cn)[:Cn // 2].astype(np.int32)
    mem[4], mem[9] = -1, mem[8]                             # a skipped entry and a duplicate
    for members in (None, mem):
        want = S.select_np(A, members, lo, ref, N, seed, K)
        got = hv_select_candidates(torch.from_numpy(A), K, None if members is None else torch.from_numpy(members),
                                   lo=lo, ref=ref, n_samples=N, seed=seed)
        S.compare({f: v.numpy() if torch.is_tensor(v) else v for f, v in got.items()}, want, "dist")
        assert got["n_samples"] == N and want["n_picked"] >= 1
    # the C argument cuts the sentinel padding of a gathered tensor; the default box is the engine's
    from mpct.engine import default_box

    sub = A[8:Cn - 7]
    got = hv_select_candidates(torch.from_numpy(A[8:]), 4, C=Cn - 15, n_samples=500, seed=4)
    dlo, dref = default_box(sub)
    S.compare({f: v.numpy() if torch.is_tensor(v) else v for f, v in got.items()},
              S.select_np(sub, None, dlo, dref, 500, 4, 4), "dist, default box")
    with pytest.raises(ValueError):
        hv_select_candidates(torch.zeros((3, 2), dtype=torch.float64), 0, lo=np.zeros(2), ref=np.ones(2))
    with pytest.raises(ValueError):
        hv_select_candidates(torch.zeros((3, 2), dtype=torch.float64), 2, lo=np.ones(2), ref=np.ones(2))


def test_result_methods_feed_the_front(built, monkeypatch):
    """ParetoResult.select passes its front as the members and returns the picked candidates;
    RobustResult.select builds the table of its pareto and goes through the front (no GPU here)."""
    from mpct import engine

    seen = []

    def fake_select(costs, n_pick, members=None, **kw):
        seen.append((np.array(costs), n_pick, np.array(members), kw))
        z = np.zeros(n_pick, dtype=np.int64)
        return engine.HvSelectResult(n_picked=1, pos=z.astype(np.int32), index=np.array([2] + [-1] * (n_pick - 1), dtype=np.int32),
                                     gain=z, covered=z + 4, hv=z * 1.0, ties=z.astype(np.int32), n_covered_all=8,
                                     n_samples=16, lo=np.zeros(2), ref=np.ones(2), volume=1.0)

    def fake_pareto(costs, max_layers=0, device=-1):
        return engine.ParetoResult(dom_count=np.zeros(3, dtype=np.int32), layer=None, front=np.array([2, 0], dtype=np.int32))

    monkeypatch.setattr(engine, "hv_select", fake_select)
    monkeypatch.setattr(engine, "pareto", fake_pareto)
    T = np.arange(6.0).reshape(3, 2)
    assert fake_pareto(T).select(T, 3, n_samples=64, seed=3).tolist() == [2]
    assert seen[-1][1] == 3 and seen[-1][2].tolist() == [2, 0] and seen[-1][3] == dict(n_samples=64, seed=3)
    assert fake_select(T, 2).share.tolist() == [0.5, 0.5]
    res = engine.RobustResult(mean=T, worst=10 + T, n_failed=np.array([0, 2, 1], dtype=np.int32),
                              worst_draw=np.zeros(3, dtype=np.int32), status=np.zeros(3, dtype=np.int32), draws=4,
                              levels=np.array([0.5, 1.0]), quantile=T + 100, cvar=T + 200)
    assert res.select(2, stat="mean", max_failed=1, columns=(("cvar", 1),), n_samples=32).tolist() == [2]
    costs, n_pick, members, kw = seen[-1]
    assert costs.shape == (3, 3) and np.isnan(costs[1]).all() and n_pick == 2
    assert members.tolist() == [2, 0] and kw == dict(device=-1, n_samples=32)
