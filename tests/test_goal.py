"""CPU, no device: the goal-attainment contract of include/mpct.h.  The two forms of tests/goal_ref.py agree on
generated cases and give the written-out answers of hand-made tables; the header and the ctypes list carry the
exports; every argument error comes back in the documented order without a device; the host entry fails loudly
without a GPU; GoalResult.winners; the CPU path of mpct.dist.goal_attain_candidates equals the reference; and
best[g][0] is weakly Pareto optimal."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import goal_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
nan, inf = np.nan, np.inf

# (name, costs, goals, weights, n_best, the expected fields written out)
HAND = [
    # A = (0, 1), B = (0.6, 0.6), C = (1, 0): B lies above the segment A-C, a non-convex front.  gamma = max of the
    # two costs: 1, 0.6, 1 -- goal attainment picks B; both costs attain B's maximum, so active is 0
    ("non-convex front", [[0.0, 1.0], [0.6, 0.6], [1.0, 0.0]], [0.0, 0.0], [1.0, 1.0], 3,
     dict(best=[[1, 0, 2]], gamma=[[0.6, 1.0, 1.0]], active=[[0, 1, 0]], n_feasible=[3], n_attained=[0], wins=[0, 1, 0])),
    # column 0 soft with goal 0, column 1 hard at 2: candidate 0 minimises gamma (1) but costs 5 > 2 in column 1
    ("hard constraint excludes the minimiser", [[1.0, 5.0], [2.0, 1.0], [3.0, 0.5]], [0.0, 2.0], [1.0, 0.0], 2,
     dict(best=[[1, 2]], gamma=[[2.0, 3.0]], active=[[0, 0]], n_feasible=[2], n_attained=[0], wins=[0, 1, 0])),
    # a hard bound below every cost
    ("all infeasible", [[1.0, 1.0], [2.0, 0.5]], [0.0, 0.25], [1.0, 0.0], 2,
     dict(best=[[-1, -1]], gamma=[[nan, nan]], active=[[-1, -1]], n_feasible=[0], n_attained=[0], wins=[0, 0])),
    # candidates 1 and 3 are duplicates with the smallest gamma, 0 and 2 tie behind them: ascending index
    ("tie by index", [[2.0], [1.0], [2.0], [1.0], [5.0]], [1.0], [0.5], 4,
     dict(best=[[1, 3, 0, 2]], gamma=[[0.0, 0.0, 2.0, 2.0]], active=[[0, 0, 0, 0]], n_feasible=[5], n_attained=[2],
          wins=[0, 1, 0, 0, 0])),
    # terms (2 - 0) / 1 = 2, (4 - 0) / 2 = 2, (1 - 0) / 0.5 = 2: columns 0, 1 and 2 all attain the maximum -> 0;
    # second candidate: terms 1, 3, 3 -> column 1
    ("active is the smallest attaining j", [[2.0, 4.0, 1.0], [1.0, 6.0, 1.5]], [0.0, 0.0, 0.0], [1.0, 2.0, 0.5], 2,
     dict(best=[[0, 1]], gamma=[[2.0, 3.0]], active=[[0, 1]], n_feasible=[2], n_attained=[0], wins=[1, 0])),
    # two goal vectors over one table: the first meets its goals (gamma <= 0), the second is invalid (negative weight)
    ("attained and invalid", [[1.0, 2.0], [0.5, 4.0]], [[1.0, 4.0], [1.0, 4.0]], [[1.0, 2.0], [1.0, -2.0]], 1,
     dict(best=[[0], [-1]], gamma=[[0.0], [nan]], active=[[0], [-1]], n_feasible=[2, -1], n_attained=[2, -1], wins=[1, 0])),
    # -INFINITY in the only soft column: gamma stays -INFINITY and active the first soft j; +INFINITY passes no
    # finite hard goal but passes an infinite one
    ("infinities", [[-inf, 1.0], [0.0, inf], [inf, 0.0]], [[0.0, 2.0], [0.0, inf]], [[1.0, 0.0], [1.0, 0.0]], 3,
     dict(best=[[0, 2, -1], [0, 1, 2]], gamma=[[-inf, inf, nan], [-inf, 0.0, inf]], active=[[0, 0, -1], [0, 0, 0]],
          n_feasible=[2, 3], n_attained=[1, 2], wins=[2, 0, 0])),
]


def expected(want):
    out = {f: np.asarray(v, dtype=np.float64 if f == "gamma" else np.int32) for f, v in want.items()}
    return out


@pytest.mark.parametrize("case", HAND, ids=[c[0] for c in HAND])
def test_hand_made_tables(case):
    name, A, goals, weights, nb, want = case
    for form in (R.goal_scalar, R.goal_np):
        R.compare(form(np.array(A), goals, weights, nb), expected(want), "%s (%s)" % (name, form.__name__))


def test_weighted_sum_never_reaches_the_non_convex_point():
    """mpct_rank_device's rule (ascending sum_j costs * w, ties by index) picks an end point of the non-convex
    front for every weight vector; goal attainment with the same weights picks the middle one."""
    A = np.array(HAND[0][1])
    for w1 in np.linspace(0.01, 0.99, 99):
        w = np.array([w1, 1.0 - w1])
        first = int(np.argsort(A @ w, kind="stable")[0])
        assert first in (0, 2)
    for w in ([1.0, 1.0], [1.0, 0.8], [0.7, 1.0]):
        assert R.goal_scalar(A, [0.0, 0.0], w, 1)["best"][0, 0] == 1


CASES = [(40, 1, 4, 9, 1), (60, 2, 5, 17, 4), (90, 3, 4, 12, 5), (70, 7, 3, 20, 16), (33, 16, 2, 8, 2), (5, 3, 3, 6, 16), (0, 2, 3, 4, 2)]


def special_case(Cn, k, hi, G, seed=0):
    """a generated table with NaN rows, infinities, signed zeros and duplicates, and G goal vectors of which
    every fifth is invalid in turn"""
    A = R.generated(Cn, k, hi, seed)
    if Cn > 12:
        A[3, k - 1] = nan
        A[Cn - 1, 0] = nan
        A[5] = inf
        A[6, 0] = -inf
        A[7] = -inf
        A[8] = A[9]
        A[10, :] = -0.0
    goals, weights = R.goal_vectors(G, k, hi, seed)
    for n, g in enumerate(range(2, G, 5)):
        R.spoil(goals, weights, g, R.INVALID[n % len(R.INVALID)])
    return A, goals, weights


@pytest.mark.parametrize("Cn,k,hi,G,nb", CASES)
def test_the_two_forms_agree(Cn, k, hi, G, nb):
    A, goals, weights = special_case(Cn, k, hi, G)
    a, b = R.goal_scalar(A, goals, weights, nb), R.goal_np(A, goals, weights, nb)
    R.compare(a, b, "scalar against vectorised")
    valid = np.array([R.valid_goal(goals[g], weights[g]) for g in range(G)])
    assert (~valid).sum() >= 1 and valid.sum() >= G // 2
    assert (a["n_feasible"][~valid] == -1).all() and (a["best"][~valid] == -1).all() and np.isnan(a["gamma"][~valid]).all()
    assert a["wins"].sum() == (a["n_feasible"] > 0).sum()
    for g in np.flatnonzero(valid):
        n = min(nb, a["n_feasible"][g])
        assert (a["best"][g, :n] >= 0).all() and (a["best"][g, n:] == -1).all() and np.isnan(a["gamma"][g, n:]).all()
        gm = a["gamma"][g, :n]
        assert (np.diff(gm) >= 0).all() or np.isinf(gm).any()
        assert a["n_attained"][g] <= a["n_feasible"][g]


def test_compare_rejects_a_single_difference():
    A, goals, weights = special_case(50, 3, 4, 11)
    want = R.goal_np(A, goals, weights, 4)
    R.compare(want, want)
    for f in R.FIELDS:
        got = {x: np.array(v, copy=True) for x, v in want.items()}
        flat = got[f].reshape(-1)
        if f == "gamma":
            i = int(np.flatnonzero(flat == 0.0)[0]) if (flat == 0.0).any() else 0
            flat[i] = -flat[i] if flat[i] == 0.0 else flat[i] + 1.0        # the sign of a zero counts
        else:
            flat[0] += 1
        with pytest.raises(AssertionError):
            R.compare(got, want)


def test_best_is_weakly_pareto_optimal():
    """no feasible candidate is strictly smaller than best[g][0] in every soft objective"""
    for Cn, k, hi, G, nb in CASES[:5]:
        A, goals, weights = special_case(Cn, k, hi, G, seed=3)
        res = R.goal_np(A, goals, weights, 1)
        checked = 0
        for g in range(G):
            b = res["best"][g, 0]
            if b < 0:
                continue
            soft = weights[g] > 0
            feas = ~np.isnan(A).any(axis=1) & (A[:, ~soft] <= goals[g, ~soft]).all(axis=1)
            assert feas[b]
            assert not (A[feas][:, soft] < A[b, soft]).all(axis=1).any(), (Cn, k, g)
            checked += 1
        assert checked >= G // 3


def test_header_declares_and_lib_exports(built):
    from mpct import _lib

    src = open(os.path.join(ROOT, "include", "mpct.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for f in ("mpct_goal_attain_device", "mpct_goal_attain"):
        assert re.search(r"\bint32_t %s\s*\(" % f, code), f
        assert f in _lib.EXPORTS
        assert C.cast(getattr(C.CDLL(_lib.lib_path()), f), C.c_void_p).value
    assert re.search(r"typedef struct mpct_goal_result \{\s*int32_t\* best;.*?double\* gamma;.*?int32_t\* active;"
                     r".*?int32_t\* n_feasible;.*?int32_t\* n_attained;.*?int32_t\* wins;.*?\} mpct_goal_result;", code, flags=re.S)
    for name, val in (("MPCT_GOAL_MAX_G", 1048576), ("MPCT_GOAL_MAX_BEST", 16)):
        assert re.search(r"#define %s %d\b" % (name, val), code)
    assert (_lib.GOAL_MAX_G, _lib.GOAL_MAX_BEST) == (1048576, 16)
    assert [n for n, _ in _lib.MpctGoalResult._fields_] == list(R.FIELDS)
    assert "Goal attainment" in src
    assert _lib.load().mpct_abi_version() == 7


def _both_entries(costs, Cn, k, goals, weights, G, nb, out):
    """return codes of the two entries for one set of arguments (host pointers: the device entry dereferences
    nothing, and here no call gets past its checks)"""
    from mpct import _lib

    lib = _lib.load()
    o = C.byref(out) if out is not None else None
    return (lib.mpct_goal_attain_device(costs, Cn, k, goals, weights, G, nb, o, None),
            lib.mpct_goal_attain(costs, Cn, k, goals, weights, G, nb, -1, o))


def test_argument_errors_in_documented_order(built):
    """Each call also carries every LATER error of the header's list, so the code that comes back shows the
    order of the checks."""
    from mpct import _lib

    EINVAL, ERANGE = -1, -4
    buf = np.zeros(64, dtype=np.int32)
    p = buf.ctypes.data_as(_lib.c_int32_p)
    dbuf = np.zeros(64)
    dp = dbuf.ctypes.data_as(_lib.c_double_p)
    A = np.zeros((4, 3))
    gl = np.zeros((5, 3))
    w = np.ones((5, 3))
    w[2, 1] = -1.0                                               # goal vector 2 is invalid: the host entry's last check
    a, g_, w_ = A.ctypes.data, gl.ctypes.data, w.ctypes.data
    none = _lib.MpctGoalResult(None, None, None, None, None, None)
    rows = _lib.MpctGoalResult(p, dp, p, None, None, None)       # rows asked for: an error with n_best = 0
    steps = [
        ((None, -1, 0, None, None, -1, 17, none), EINVAL, "k must be"),
        ((None, -1, 17, None, None, -1, 17, none), EINVAL, "k must be"),
        ((None, -1, 3, None, None, 1048577, 17, none), EINVAL, "C < 0 or G < 0"),
        ((None, 1048577, 3, None, None, -1, 17, none), EINVAL, "C < 0 or G < 0"),
        ((None, 1048577, 3, None, None, 5, -1, none), ERANGE, "MPCT_PARETO_MAX_C"),
        ((None, 4, 3, None, None, 1048577, -1, none), ERANGE, "MPCT_GOAL_MAX_G"),
        ((None, 4, 3, None, None, 5, -1, none), EINVAL, "n_best < 0"),
        ((None, 4, 3, None, None, 5, 17, none), ERANGE, "MPCT_GOAL_MAX_BEST"),
        ((None, 4, 3, None, None, 5, 0, none), EINVAL, "costs is NULL"),
        ((a, 4, 3, None, w_, 5, 0, none), EINVAL, "goals or weights is NULL"),
        ((a, 4, 3, g_, None, 5, 0, none), EINVAL, "goals or weights is NULL"),
        ((a, 4, 3, g_, w_, 5, 0, none), EINVAL, "no output pointer"),
        ((a, 4, 3, g_, w_, 5, 0, None), EINVAL, "no output pointer"),
        ((a, 4, 3, g_, w_, 5, 0, rows), EINVAL, "need n_best >= 1"),
        ((a, 4, 3, g_, w_, 5, 0, _lib.MpctGoalResult(None, dp, None, p, None, None)), EINVAL, "need n_best >= 1"),
        ((a, 4, 3, g_, w_, 5, 0, _lib.MpctGoalResult(None, None, p, None, None, p)), EINVAL, "need n_best >= 1"),
    ]
    for args, code, msg in steps:
        for rc in _both_entries(*args):
            assert rc == code, (args[1:3], args[5:7], rc)
            assert msg in _lib.last_error(), (args[1:3], args[5:7], _lib.last_error())
    # the host entry alone reads the arrays: the invalid goal vector, named by its row, before any device
    lib = _lib.load()
    assert lib.mpct_goal_attain(a, 4, 3, g_, w_, 5, 2, -1, C.byref(rows)) == EINVAL
    assert "goal vector 2 is invalid" in _lib.last_error()
    for how in R.INVALID:
        gl2, w2 = np.zeros((5, 3)), np.ones((5, 3))
        R.spoil(gl2, w2, 4, how)
        assert lib.mpct_goal_attain(a, 4, 3, gl2.ctypes.data, w2.ctypes.data, 5, 2, -1, C.byref(rows)) == EINVAL, how
        assert "goal vector 4 is invalid" in _lib.last_error(), how
    assert (buf == 0).all() and (dbuf == 0).all()                # nothing was written


def test_degenerate_sizes_and_no_device(built, has_gpu):
    from mpct.engine import MpctError, goal_attain

    # G = 0: wins zeroed, no device needed
    res = goal_attain(np.ones((4, 2)), np.zeros((0, 2)), np.zeros((0, 2)), n_best=3)
    assert res.best.shape == (0, 3) and res.wins.tolist() == [0, 0, 0, 0] and res.winners().size == 0
    # C = 0: every count 0 and the rows padded, no device needed
    res = goal_attain(np.zeros((0, 2)), [0.0, 1.0], [[1.0, 0.0], [2.0, 1.0]], n_best=2)
    assert (res.best == -1).all() and np.isnan(res.gamma).all() and (res.active == -1).all()
    assert res.n_feasible.tolist() == [0, 0] and res.n_attained.tolist() == [0, 0] and res.wins.size == 0
    with pytest.raises(ValueError):
        goal_attain(np.ones((4, 2)), [0.0, 0.0, 0.0], [1.0, 1.0])
    with pytest.raises(MpctError, match=r"\(-1\).*goal vector 0 is invalid"):
        goal_attain(np.ones((4, 2)), [0.0, 0.0], [0.0, 0.0])
    if not has_gpu:
        with pytest.raises(MpctError, match=r"\(-3\).*HIP device"):
            goal_attain(R.generated(10, 3, 4), [0.0, 0.0, 0.0], [1.0, 1.0, 0.0])
    # a call that cannot open its device (none here, or an ordinal out of range) leaves wins as it was
    from mpct import _lib

    A, gl, w = R.generated(10, 3, 4), np.zeros((2, 3)), np.ones((2, 3))
    wins = np.full(10, 77, dtype=np.int32)
    nf = np.full(2, 77, dtype=np.int32)
    out = _lib.MpctGoalResult(None, None, None, nf.ctypes.data_as(_lib.c_int32_p), None, wins.ctypes.data_as(_lib.c_int32_p))
    rc = _lib.load().mpct_goal_attain(A.ctypes.data, 10, 3, gl.ctypes.data, w.ctypes.data, 2, 0, 9999, C.byref(out))
    assert rc == (-1 if has_gpu else -3), _lib.last_error()
    assert (wins == 77).all() and (nf == 77).all()


def test_goal_result_winners():
    from mpct.engine import GoalResult

    wins = np.array([0, 3, 0, 5, 3, 1, 0], dtype=np.int32)
    res = GoalResult(best=None, gamma=None, active=None, n_feasible=np.zeros(12, dtype=np.int32),
                     n_attained=np.zeros(12, dtype=np.int32), wins=wins)
    assert res.winners().tolist() == [3, 1, 4, 5]               # descending wins, ties by index
    assert res.winners().dtype == np.int32


@pytest.mark.parametrize("Cn,k,hi,G,nb", CASES + [(300, 7, 3, 140, 4), (12, 2, 3, 5, 0)])
def test_dist_cpu_path_equals_reference(Cn, k, hi, G, nb):
    import torch
    from mpct.dist import goal_attain_candidates

    A, goals, weights = special_case(Cn, k, hi, G)
    want = R.goal_np(A, goals, weights, nb)
    got = goal_attain_candidates(torch.from_numpy(A), goals, weights, n_best=nb)
    R.compare({f: v.numpy() for f, v in got.items()}, want, "dist CPU path")
    if Cn > 10:      # the C argument cuts the sentinel padding of a gathered tensor; a (k,) vector is broadcast
        cut = goal_attain_candidates(torch.from_numpy(A), goals[0], weights, n_best=nb, C=Cn - 7)
        R.compare({f: v.numpy() for f, v in cut.items()}, R.goal_np(A[:Cn - 7], np.tile(goals[0], (G, 1)), weights, nb), "cut")
    with pytest.raises(ValueError):
        goal_attain_candidates(torch.zeros((3, 17), dtype=torch.float64), np.zeros(17), np.ones(17))


def test_result_methods_feed_the_cost_table(built, monkeypatch):
    """RobustResult.goal_attain, the index results' and the robust-index result's goal_attain hand the table their
    pareto / costs build to goal_attain (the device call itself is replaced: no GPU here)."""
    from mpct import engine

    seen = {}

    def fake(costs, goals, weights, n_best=1, device=-1):
        seen.update(costs=np.array(costs), goals=goals, weights=weights, n_best=n_best, device=device)
        return "result"

    monkeypatch.setattr(engine, "goal_attain", fake)
    res = engine.RobustResult(mean=np.arange(6.0).reshape(3, 2), worst=10 + np.arange(6.0).reshape(3, 2),
                              n_failed=np.array([0, 2, 1], dtype=np.int32), worst_draw=np.zeros(3, dtype=np.int32),
                              status=np.zeros(3, dtype=np.int32), draws=4, levels=np.array([0.5, 1.0]),
                              quantile=np.arange(6.0).reshape(3, 2) + 100, cvar=np.arange(6.0).reshape(3, 2) + 200)
    assert res.goal_attain([0, 0], [1, 1], n_best=3, stat="mean", max_failed=1, device=2) == "result"
    np.testing.assert_array_equal(seen["costs"], res.scores(1, "mean"))
    assert (seen["n_best"], seen["device"]) == (3, 2)
    res.goal_attain([0, 0, 0], [1, 1, 0], columns=(("cvar", 1),))
    assert seen["costs"].shape == (3, 3) and np.isnan(seen["costs"][1:]).all()
    idx = engine.IndexResult(iae=np.arange(12.0).reshape(3, 2, 2), over=np.ones((3, 2, 2)), nit=50)
    assert idx.goal_attain(("iae", "over"), [0, 0.5], [1, 0], n_best=2, reduce="sum") == "result"
    np.testing.assert_array_equal(seen["costs"], idx.costs(("iae", "over"), reduce="sum"))
    rob = engine.RobustIndexResult(columns=[("iae", 0), ("over", 0)], n=np.ones((3, 2)), mean=np.ones((3, 2)), lo=np.ones((3, 2)),
                                   lo_draw=np.zeros((3, 2)), hi=np.arange(6.0).reshape(3, 2), hi_draw=np.zeros((3, 2)), base=res)
    assert rob.goal_attain("hi", ("over",), [0.5], [1.0], max_failed=1) == "result"
    np.testing.assert_array_equal(seen["costs"], rob.costs("hi", ("over",), 1))
