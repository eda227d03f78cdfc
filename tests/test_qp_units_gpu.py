"""GPU: the wave primitives (wave_ops.h) and the QP drivers (gpc_qp.h gi_qp<16|32|64>, gpc_qp16.h
gi_qp16) one call at a time, through tests/device_units/libmpct_unit_probe.so, against the plain
references of tests/qp_unit_ref.py.  One launch per op or per (variant, shape, case kind).

Bounds, all derived (measured maxima are recorded in DESIGN.md, not here):
  * integer, argmin, shift and broadcast ops: bit for bit (a zero minimum may carry either sign:
    the rule is -0.0 == +0.0);
  * floating sums: exact on integer-valued inputs, elsewhere |s - exact| <= depth * eps * sum|v|,
    the pairwise-summation bound (each value passes through `depth` rounded additions, each with
    relative error <= eps / 2): depth 4 for a 16-lane row (four DPP stages), 2 for row4_sum (two
    permlane stages), 6 for the wave (4 + 2); block_prefix<16> is a four-stage scan (depth 4),
    block_prefix<64> a sequential sum of at most Nu terms (depth Nu - 1);
  * rcp_nr, rsq_nr: see test_rcp_rsq_ulps;
  * QP optimum: ||x_dev - x_ref||inf <= 8 * max(spread of x_ref under a +-tol move of the right-hand
    sides, cond(R) * M * eps * ||x_ref||inf); minimum slack >= -tol - Nu * eps * sum|x|.
"""
import ctypes as C
import math
import os

import numpy as np
import pytest

import qp_unit_ref as Q

pytestmark = pytest.mark.gpu

LIB = os.path.join(os.path.dirname(os.path.abspath(__file__)), "device_units", "libmpct_unit_probe.so")
INF, NAN = math.inf, math.nan


@pytest.fixture(scope="module")
def gpu(built, has_gpu):
    if not has_gpu:
        pytest.skip("no GPU")
    return True


@pytest.fixture(scope="module")
def probe(gpu):
    return C.CDLL(LIB)


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def prim(lib, op, a, b=None, k=None):
    """probe_prim: a, b [ncase, 64] doubles, k [ncase, 64] ints -> (out_d [ncase, 4, 64], out_i [ncase, 64])."""
    a = np.ascontiguousarray(a, np.float64).reshape(-1, 64)
    n = a.shape[0]
    b = np.zeros_like(a) if b is None else np.ascontiguousarray(b, np.float64).reshape(n, 64)
    k = np.zeros((n, 64), np.int32) if k is None else np.ascontiguousarray(k, np.int32).reshape(n, 64)
    od, oi = np.full((n, 4, 64), NAN), np.full((n, 64), -12345, np.int32)
    code = Q.OP[op] if isinstance(op, str) else op
    rc = lib.probe_prim(C.c_int(code), C.c_int(n), _p(a), _p(b), _p(k), _p(od), _p(oi))
    assert rc == 0, (op, rc)
    return od, oi


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.int64)


def same_bits(a, b):
    return np.array_equal(bits(a), bits(b))


# ---------------------------------------------------------------------------------------------
# input families, one wave (row of 64) each
def families():
    rng = np.random.default_rng(11)
    fam = {}
    fam["normal"] = rng.standard_normal((4, 64))
    fam["integer"] = rng.integers(-2 ** 20, 2 ** 20, (4, 64)).astype(float)
    big = rng.standard_normal((2, 64)) * 1e12
    big[:, 1::2] = -big[:, ::2] + rng.standard_normal((2, 32))
    fam["cancel"] = big
    fam["ties"] = rng.integers(-2, 3, (4, 64)).astype(float)
    nanv = rng.standard_normal((3, 64))
    nanv[0, ::3] = NAN
    nanv[1, :40] = NAN
    nanv[2, 5] = NAN
    fam["nan"] = nanv
    infv = rng.standard_normal((3, 64))
    infv[0, ::5] = INF
    infv[1, 7::9] = -INF
    infv[2, :] = INF
    infv[2, 33] = 4.0
    fam["inf"] = infv
    fam["all_inf"] = np.full((1, 64), INF)
    z = np.zeros((3, 64))
    z[0, 1::2] = -0.0
    z[1, :] = -0.0
    z[1, 40] = 0.0
    z[2] = rng.integers(0, 2, 64) * 1.0
    z[2, 9] = -0.0
    fam["zeros"] = z
    fam["denormal"] = rng.integers(-50, 50, (2, 64)) * 5e-324
    each = rng.uniform(1.0, 2.0, (64, 64))
    each[np.arange(64), np.arange(64)] = -1.0
    fam["each_lane"] = each
    return fam


def family_ids(name, v, rng):
    """ids != lane: a permutation-free many-to-one map with repeats; INF lanes carry 0x7fffffff as
    at every call site."""
    ids = rng.integers(0, 200, v.shape).astype(np.int32)
    if name == "each_lane":
        ids = (4 * np.arange(64)[None, :] + rng.integers(0, 4, v.shape)).astype(np.int32)
    ids[v == INF] = Q.NOID
    return ids


ROWS = [range(16 * r, 16 * r + 16) for r in range(4)]
FINITE_SUM_FAMILIES = ("normal", "integer", "cancel", "ties", "zeros", "denormal", "each_lane")


# ---------------------------------------------------------------------------------------------
def test_broadcasts_and_shifts(probe):
    rng = np.random.default_rng(3)
    v = rng.standard_normal((64, 64))
    v[0, :] = NAN
    v[1, ::2] = -0.0
    src = np.repeat(np.arange(64, dtype=np.int32)[:, None], 64, axis=1)
    od, _ = prim(probe, "bcast", v, k=src)
    for c in range(64):
        assert same_bits(od[c, 0], np.full(64, v[c, c])), c
    for k in range(16):
        od, _ = prim(probe, Q.OP_ROW_BCAST16 + k, v[:8])
        for c in range(8):
            want = np.concatenate([np.full(16, v[c, 16 * r + k]) for r in range(4)])
            assert same_bits(od[c, 0], want), (k, c)
    ki = rng.integers(-2 ** 31, 2 ** 31 - 1, (8, 64)).astype(np.int32)
    for maxm in (16, 64):
        od, _ = prim(probe, "lane_next%d" % maxm, v[:8])
        pd, _ = prim(probe, "lane_prev%d" % maxm, v[:8])
        _, oi = prim(probe, "lane_next_i%d" % maxm, v[:8], k=ki)
        for c in range(8):
            assert same_bits(od[c, 0], Q.shift_ref(v[c], maxm, +1)), (maxm, c)   # 0 (+0.0) at row edges
            assert same_bits(pd[c, 0], Q.shift_ref(v[c], maxm, -1)), (maxm, c)
            assert np.array_equal(oi[c], Q.shift_ref(ki[c], maxm, +1)), (maxm, c)


def test_min_and_argmin(probe):
    """row / pair / wave minima and argmins on every family: the value and id bit for bit on every
    lane that should hold them (smallest id among equal values, NaN never the minimum, all-INF with
    the call sites' ids gives 0x7fffffff).  A row that holds nothing but NaN is outside the contract's
    "nothing finite -> (INF, 0x7fffffff)": the id is 0x7fffffff, the value stays NaN (v_min_f64 of
    NaNs), and the drivers read such a result as "not below the threshold" either way; asserted as
    that.  The wave-wide forms are given at least one non-NaN lane."""
    rng = np.random.default_rng(5)
    for name, v in families().items():
        ids = family_ids(name, v, rng)
        n = v.shape[0]
        rm, _ = prim(probe, "row_min", v)
        _, rmi = prim(probe, "row_min_i", v, k=ids)
        ra, rai = prim(probe, "row_argmin", v, k=ids)
        wa, wai = prim(probe, "wave_argmin64", v, k=ids)
        q64, q64i = prim(probe, "qargmin64", v, k=ids)
        q16 = {s: prim(probe, "qargmin16_" + s, v, k=ids) for s in ("m1", "0", "2")}
        pm = {w: prim(probe, "pair_min%d" % w, v)[0] for w in (16, 32)}
        pmi = {w: prim(probe, "pair_min_i%d" % w, v, k=ids)[1] for w in (16, 32)}
        pa = {w: prim(probe, "pair_argmin%d" % w, v, k=ids) for w in (16, 32)}
        for c in range(n):
            tag = (name, c)
            for r in ROWS:
                lanes = list(r)
                rv, rid = Q.argmin_ref(v[c, lanes], ids[c, lanes])
                allnan = np.all(np.isnan(v[c, lanes]))
                for l in lanes:
                    if not allnan:
                        assert Q.same_min_value(rm[c, 0, l], rv), tag
                        assert Q.argmin_matches(ra[c, 0, l], rai[c, l], v[c, lanes], ids[c, lanes]), tag
                    else:   # nothing to compare with: the value stays NaN and no lane attains it
                        assert math.isnan(rm[c, 0, l]) and math.isnan(ra[c, 0, l]) and rai[c, l] == Q.NOID, tag
                    assert rmi[c, l] == ids[c, lanes].min(), tag
            for l in range(64):
                assert Q.argmin_matches(wa[c, 0, l], wai[c, l], v[c], ids[c]), tag
                assert Q.argmin_matches(q64[c, 0, l], q64i[c, l], v[c], ids[c]), tag
                for s in q16:   # row 0's result on every lane of the wave
                    if not np.all(np.isnan(v[c, :16])):
                        assert Q.argmin_matches(q16[s][0][c, 0, l], q16[s][1][c, l], v[c, :16], ids[c, :16]), tag + (s,)
                    else:
                        assert math.isnan(q16[s][0][c, 0, l]) and q16[s][1][c, l] == Q.NOID, tag + (s,)
                for w in (16, 32):
                    pair = [l, l ^ w]
                    if not np.all(np.isnan(v[c, pair])):
                        assert Q.same_min_value(pm[w][c, 0, l], Q.argmin_ref(v[c, pair], [0, 0])[0]), tag
                    # pair_argmin compares with `<` and makes no NaN promise (row_argmin and
                    # wave_argmin64 reduce the value with pair_min): checked on NaN-free pairs
                    if not np.any(np.isnan(v[c, pair])):
                        assert Q.argmin_matches(pa[w][0][c, 0, l], pa[w][1][c, l], v[c, pair], ids[c, pair]), tag
                    assert pmi[w][c, l] == min(ids[c, l], ids[c, l ^ w]), tag


def test_sums(probe):
    """Exact on integer-valued inputs; elsewhere within depth * eps * sum|v| of the exact sum (module
    docstring).  Every lane that holds a result holds the same bits; row4_sum2 / row4_sum4 are bitwise
    row4_sum of each operand."""
    fam = families()
    for name in FINITE_SUM_FAMILIES:
        v = fam[name]
        n = v.shape[0]
        w = np.roll(v, 17, axis=1) * 0.75
        rs, _ = prim(probe, "row_sum", v)
        r4, _ = prim(probe, "row4_sum", v, w)
        r42, _ = prim(probe, "row4_sum2", v, w)
        r44, _ = prim(probe, "row4_sum4", v, w)
        ws, _ = prim(probe, "wave_sum64", v)
        q16, _ = prim(probe, "qsum16", v)
        q64, _ = prim(probe, "qsum64", v)
        exact_all = name in ("integer", "ties", "zeros", "denormal")
        for c in range(n):
            tag = (name, c)
            for r in ROWS:
                lanes = list(r)
                assert len(set(bits(rs[c, 0, lanes]).tolist())) == 1, tag
                assert Q.sum_check(rs[c, 0, lanes[0]], v[c, lanes], 4), tag
                if exact_all:
                    assert rs[c, 0, lanes[0]] == math.fsum(v[c, lanes]), tag
            for l in range(16):
                col = [l, l + 16, l + 32, l + 48]
                for k, src in enumerate((v[c], w[c], v[(c + 1) % n], w[(c + 1) % n])):
                    assert len(set(bits(r4[c, k, col]).tolist())) == 1, tag
                    assert Q.sum_check(r4[c, k, l], src[col], 2), tag
            assert same_bits(r42[c, :2], r4[c, :2]), tag
            assert same_bits(r44[c], r4[c]), tag
            for out, lanes in ((ws, range(64)), (q64, range(64)), (q16, range(16))):
                assert len(set(bits(out[c, 0]).tolist())) == 1, tag
                depth = 6 if len(lanes) == 64 else 4
                assert Q.sum_check(out[c, 0, 0], v[c, list(lanes)], depth), tag
                if exact_all:
                    assert out[c, 0, 0] == math.fsum(v[c, list(lanes)]), tag


def test_block_prefix(probe):
    """block_prefix<16>: every (nu, Nu) with nu * Nu <= 16 (Nu = 1, 8, 9, 16 among them: the Nu > 8
    stage), garbage in the lanes >= M; block_prefix<64>: M = 17, 33, 64."""
    rng = np.random.default_rng(9)

    def run(op, shapes, depth_of):
        xs, ks = [], []
        for nu, Nu in shapes:
            for integer in (True, False):
                M = nu * Nu
                x = rng.integers(-1000, 1000, 64).astype(float) if integer else rng.standard_normal(64)
                x[M:] = rng.choice([NAN, INF, 1e300, -7.0], 64 - M) if op.endswith("16") else x[M:]
                l = np.where(np.arange(64) < M, np.arange(64) % Nu, 0)
                xs.append(x)
                ks.append(l | (Nu << 8) | (M << 16))
        od, _ = prim(probe, op, np.array(xs), k=np.array(ks, np.int32))
        c = 0
        for nu, Nu in shapes:
            for integer in (True, False):
                M = nu * Nu
                terms = Q.block_prefix_terms(xs[c], M, Nu)
                for i in range(M):
                    if integer:
                        assert od[c, 0, i] == math.fsum(terms[i]), (op, nu, Nu, i)
                    assert Q.sum_check(od[c, 0, i], terms[i], depth_of(Nu)), (op, nu, Nu, i)
                c += 1

    run("block_prefix16", [(nu, Nu) for Nu in range(1, 17) for nu in range(1, 16 // Nu + 1)], lambda Nu: 4)
    run("block_prefix64", [(1, 17), (17, 1), (3, 11), (33, 1), (4, 16), (64, 1), (8, 8)], lambda Nu: max(Nu - 1, 1))


def test_rcp_rsq_ulps(probe, capsys):
    """rcp_nr / rsq_nr against the exact rational result, in ulps of its correct rounding.

    rcp_nr: the last Newton step is r' = fma(r, e, r) with e = fma(-x, r, 1).  v_rcp_f64 and one step
    leave r = (1/x)(1 + d), |d| <= 2^-40 (a step squares the error and adds one rounding; 2^-40
    assumes a seed good to 2^-20, which a double-precision v_rcp_f64 / v_rsq_f64 is taken to be.  The
    bounds below need far less: the last step leaves d^2 2^53 ulp, under 1/2 ulp as soon as
    |d| <= 2^-27, i.e. a seed good to 14 bits).  e is one rounding of -d (error 2^-40 * 2^-53, nothing),
    r + r e = (1/x)(1 - d^2), and the fma rounds once: |r' - 1/x| <= 1/2 ulp + 2^-80 / x < 1 ulp.
    Bound: 1 ulp.

    rsq_nr: the last step is r' = fl(r * g), g = fma(-t, r, 1.5), t = fl(h r), h = x / 2 exact.  With
    r = x^-1/2 (1 + d), |d| <= 2^-40: t has relative error <= u = 2^-53, which enters g ~ 1 as
    0.5 u; the fma adds u; so g = (1 - d + O(d^2))(1 + 1.5 u) and r g = x^-1/2 (1 + 1.5 u + O(d^2)).
    A relative error of 1.5 u is at most 1.5 ulp of the result (ulp / value >= 2^-53), and the last
    multiplication rounds by 1/2 ulp more: 2 ulp + O(2^-27).  Bound: 2.5 ulp.

    Denormal inputs and results are printed, not asserted."""
    rng = np.random.default_rng(21)
    xs = list(rng.uniform(1.0, 2.0, 300) * 2.0 ** rng.integers(-300, 301, 300))
    for e in range(-8, 9):
        p = 2.0 ** e
        xs += [p, math.nextafter(p, 0.0), math.nextafter(p, INF)]
    # what the solvers feed them: |d|^2 of J-columns, Givens a^2 + b^2, Householder scalars
    d = rng.standard_normal((120, 16)) * 10.0 ** rng.uniform(-3, 1, (120, 1))
    xs += list((d * d).sum(1)) + list(d[:, 0] ** 2 + d[:, 1] ** 2) + list(np.abs(d[:, 2]) + 1e-3)
    x = np.array(xs)
    x = np.concatenate([x, np.full(-len(x) % 64, 1.0)]).reshape(-1, 64)
    worst = {}
    for op, exact, bound in (("rcp_nr", Q.rcp_exact, 1.0), ("rsq_nr", Q.rsq_exact, 2.5)):
        inp = x if op == "rsq_nr" else x * np.where(np.arange(64) % 2 == 0, 1.0, -1.0)
        od, _ = prim(probe, op, inp)
        errs = [Q.ulps_off(o, exact(v)) for o, v in zip(od[:, 0].ravel(), inp.ravel())]
        worst[op] = max(errs)
        print("%s: max error %.3f ulp over %d inputs (bound %.1f)" % (op, worst[op], len(errs), bound))
        assert worst[op] <= bound, (op, worst[op])
    den = np.array([5e-324, 1e-310, 2.2250738585072014e-308, 1.7e308, 8.9e307] + [1.0] * 59).reshape(1, 64)
    for op in ("rcp_nr", "rsq_nr"):
        od, _ = prim(probe, op, den)
        print(op, "on denormal inputs / results:", list(zip(den[0, :5].tolist(), od[0, 0, :5].tolist())))


# ---------------------------------------------------------------------------------------------
# QP drivers
def run_qp(lib, variant, seqs, rebuild=128, maxit=None):
    """One launch: sequences of equal shape and length -> dict of arrays [nseq, T, ...]."""
    s0 = seqs[0]
    n, T, M, nu = len(seqs), s0.T, s0.M, s0.nu
    assert all((s.T, s.M, s.Nu) == (T, M, s0.Nu) for s in seqs)
    rinv = np.ascontiguousarray([s.rinv for s in seqs])
    bnd = np.ascontiguousarray([s.bnd for s in seqs])
    xu = np.ascontiguousarray([s.xu for s in seqs])
    up = np.ascontiguousarray([s.up for s in seqs])
    out = dict(x=np.full((n, T, M), NAN), it=np.full((n, T), -1, np.int32), st=np.full((n, T), -1, np.int32),
               q=np.full((n, T), -1, np.int32), ids=np.full((n, T, 64), -7, np.int32),
               nrot=np.full((n, T), -1, np.int32))
    rc = lib.probe_qp(C.c_int(variant), C.c_int(n), C.c_int(T), C.c_int(M), C.c_int(s0.Nu), _p(rinv), _p(bnd),
                      _p(xu), _p(up), C.c_double(Q.TOL), C.c_int(s0.maxit if maxit is None else maxit),
                      C.c_int(rebuild), _p(out["x"]), _p(out["it"]), _p(out["st"]), _p(out["q"]), _p(out["ids"]),
                      _p(out["nrot"]))
    assert rc == 0, (variant, rc)
    return out


def active_ids(out, k, t):
    q = int(out["q"][k, t])
    return frozenset(int(i) for i in out["ids"][k, t, :q])


RATIOS = {}


def check_solved(variant, seqs, out, steps=None):
    """Status 0, minimum slack, x against the reference (8 x its scale); returns the largest ratio."""
    worst = 0.0
    for k, s in enumerate(seqs):
        for t in (range(s.T) if steps is None else steps):
            tag = (Q.VARIANT_NAMES[variant], s.nu, s.Nu, s.name, t)
            x = out["x"][k, t]
            assert out["st"][k, t] == 0, tag
            assert 0 <= out["it"][k, t] <= s.maxit, tag
            assert s.min_slack(t, x) >= Q.slack_floor(s, x), tag + (s.min_slack(t, x),)
            r = Q.x_ratio(s, t, x)
            worst = max(worst, r)
            assert r <= 8.0, tag + (r,)
            assert len(active_ids(out, k, t)) == out["q"][k, t], tag   # no id twice
    RATIOS[variant] = max(RATIOS.get(variant, 0.0), worst)
    return worst


VARIANT_SHAPES = [(v, sh) for v, maxm in Q.VARIANTS.items() for sh in Q.SHAPES[maxm]]


@pytest.mark.parametrize("variant,shape", VARIANT_SHAPES, ids=lambda p: str(p).replace(" ", ""))
def test_qp_cases(probe, variant, shape, capsys):
    """Cases 1-3 and 5-7 of one variant at one shape (module docstring for the bounds; case 4 and
    case 8 have tests of their own below)."""
    d = Q.cases(Q.VARIANTS[variant])[shape]
    M = shape[0] * shape[1]
    # 1. x_u feasible at step 1: zero iterations, x bitwise x_u, status 0, the retained set untouched
    seqs = d["feasible"]
    o = run_qp(probe, variant, seqs)
    check_solved(variant, seqs, o)
    assert o["it"][0, 1] == 0 and o["st"][0, 1] == 0
    assert same_bits(o["x"][0, 1], seqs[0].xu[1])
    assert o["q"][0, 0] > 0 and o["q"][0, 1] == o["q"][0, 0]
    assert np.array_equal(o["ids"][0, 1], o["ids"][0, 0]) and o["nrot"][0, 1] == o["nrot"][0, 0]
    # 2. cold solves with 1 .. M - 1 active constraints (none at M = 1)
    seqs = d["cold"]
    if seqs:
        o = run_qp(probe, variant, seqs)
        check_solved(variant, seqs, o)
        for k, s in enumerate(seqs):
            assert active_ids(o, k, 0) == s.solve(0)["act_ids"], (shape, s.name)
    # 3. warm sequences: each step equals the cold reference of the same QP; the same set of ids after
    # every step the reference calls non-degenerate (a step whose x_u is feasible keeps the retained
    # set by design, case 1, so the sets are compared after the steps that solve)
    seqs = d["warm"]
    o = run_qp(probe, variant, seqs)
    check_solved(variant, seqs, o)
    for k, s in enumerate(seqs):
        solved = [t for t in range(s.T) if s.min_slack(t, s.xu[t]) < -Q.TOL]
        assert len(solved) >= 2   # (a retained set that is already optimal solves with 0 iterations)
        assert all(o["it"][k, t] == 0 for t in range(s.T) if s.min_slack(t, s.xu[t]) >= 0.0)
        for t in solved:
            if s.solve(t)["nondegenerate"]:
                assert active_ids(o, k, t) == s.solve(t)["act_ids"], (shape, s.name, t)
    # 5. degenerate: x is still the unique optimum
    if d["degenerate"]:
        o = run_qp(probe, variant, d["degenerate"])
        check_solved(variant, d["degenerate"], o)
    # 6. full active set, then a step that must drop from it
    o = run_qp(probe, variant, d["full"])
    check_solved(variant, d["full"], o)
    assert o["q"][0, 0] == M and o["q"][0, 1] == M
    assert active_ids(o, 0, 0) == d["full"][0].solve(0)["act_ids"]
    assert active_ids(o, 0, 1) == d["full"][0].solve(1)["act_ids"]
    # 7. infeasible: flagged, within the cap, and the call returns
    for s in d["infeasible"]:
        o = run_qp(probe, variant, [s])
        assert o["st"][0, 0] & Q.ST_INFEAS, (shape, s.name, o["st"][0, 0])
        assert 0 <= o["it"][0, 0] <= s.maxit
    with capsys.disabled():
        print("\n  %s %s: worst |x - x_ref| / scale so far %.3f" % (Q.VARIANT_NAMES[variant], shape, RATIOS[variant]))


@pytest.mark.parametrize("variant,shape", VARIANT_SHAPES, ids=lambda p: str(p).replace(" ", ""))
def test_qp_maxiter_after_add(probe, variant, shape):
    """Case 8, and the regression case of the cap fix: a QP that still has violated constraints when
    an add lands exactly on the iteration cap must come back with MPCT_ST_QP_MAXITER (it came back
    with status 0 before the main loops re-checked after such an add).
      * maxit = 2 on every cold case with at least three active bounds: flagged, at most 2 + 1 iterations;
      * maxit = 1 on the full-set sequence, which exists at every shape: at M >= 2 step 0 needs M adds,
        so it is flagged after at most 1 + 1 iterations; at M = 1 step 0 is solved by its one add (no
        flag: the cap alone is no error) and step 1, which must drop before it adds, is flagged."""
    d = Q.cases(Q.VARIANTS[variant])[shape]
    M = shape[0] * shape[1]
    seqs = [s for s in d["cold"] if int(s.name[4:]) >= 3]
    assert bool(seqs) == (M >= 4)
    if seqs:
        o = run_qp(probe, variant, seqs, maxit=2)
        for k, s in enumerate(seqs):
            assert o["st"][k, 0] & Q.ST_MAXITER, (shape, s.name, o["st"][k, 0], o["it"][k, 0])
            assert o["it"][k, 0] <= 3
    o = run_qp(probe, variant, d["full"], maxit=1)
    t = 0 if M >= 2 else 1
    assert o["st"][0, t] & Q.ST_MAXITER, (shape, o["st"][0].tolist(), o["it"][0].tolist())
    assert np.all(o["it"][0] <= 2)
    if M == 1:
        assert o["st"][0, 0] == 0 and o["it"][0, 0] == 1


@pytest.mark.parametrize("shape", Q.SHAPES[16], ids=str)
def test_qp16_rebuild_and_layouts(probe, shape):
    """gi_qp16: the warm sequences with rebuild = 1 (x M rotations) and 128 both meet the tolerance,
    and nrot shows that the rebuild fired; gi_qp16<false,void,false> and <true,void,true> (packed
    R^-1, bounds in LDS) agree bit for bit in x, iterations and active ids."""
    d = Q.cases(16)[shape]
    seqs = d["warm"]
    res = {}
    for variant in (3, 4):
        for rebuild in (1, 128):
            o = run_qp(probe, variant, seqs, rebuild=rebuild)
            check_solved(variant, seqs, o)
            res[variant, rebuild] = o
    for rebuild in (1, 128):
        a, b = res[3, rebuild], res[4, rebuild]
        assert same_bits(a["x"], b["x"]) and np.array_equal(a["it"], b["it"])
        assert np.array_equal(a["ids"], b["ids"]) and np.array_equal(a["q"], b["q"])
    for k, s in enumerate(seqs):
        for variant in (3, 4):
            n1, n128 = res[variant, 1]["nrot"][k], res[variant, 128]["nrot"][k]
            q1, q128 = res[variant, 1]["q"][k], res[variant, 128]["q"][k]
            # with a retained set J is reloaded by the rebuild alone, so nrot falls only there
            fell1 = [t for t in range(1, s.T) if q1[t - 1] > 0 and n1[t] < n1[t - 1]]
            fell128 = [t for t in range(1, s.T) if q128[t - 1] > 0 and n128[t] < n128[t - 1]]
            # both runs take the same path, so their counters differ only once a rebuild has reset one
            if Q.first_rebuild_step(s) is not None:
                assert np.any(n1 < n128), (shape, n1.tolist(), n128.tolist())
                assert fell1 or s.M == 1, (shape, n1.tolist())
            assert not fell128, (shape, n128.tolist())   # 128 M rotations are never reached in 12 steps


@pytest.mark.parametrize("variant", (0, 1, 2))
def test_qp_wide_rebuild(probe, variant):
    """gi_qp: small-M sequences whose active constraints flip every step pass kGiRebuildWide * M
    rotations; nrot falls back (the J rebuild re-added the retained set) and every step still meets
    the tolerance."""
    for shape, s in Q.rebuild_wide_cases().items():
        o = run_qp(probe, variant, [s])
        check_solved(variant, [s], o)
        nrot = o["nrot"][0]
        assert Q.first_rebuild_step(s, Q.REBUILD_WIDE) is not None
        assert nrot.max() >= Q.REBUILD_WIDE * s.M, (shape, nrot.tolist())
        assert np.all(o["q"][0] > 0) and np.any(np.diff(nrot) < 0), (shape, nrot.tolist())


# ---------------------------------------------------------------------------------------------
# factor updates
def run_factors(lib, maxm, layout, case):
    """probe_factors on one script: per entry J [M, M] (J(i, k)), R_A [M, M] (upper triangle; unpacked
    from the packed layout), B [16, 16] (register variant), the lane fields and scalars."""
    M, Nu, script = case["M"], case["Nu"], np.ascontiguousarray(case["script"], np.int32)
    ns = len(script)
    reg = layout == 2
    rasz = M * (M + 3) // 2 if layout == 1 else M * M
    jsz = 256 if reg else M * M
    J, RA, B = np.full((ns, jsz), NAN), np.full((ns, rasz), NAN), np.full((ns, 256), NAN)
    ld, li = np.full((ns, 3, 64), NAN), np.full((ns, 2, 64), -9, np.int32)
    sc, bt = np.full((ns, 2), -9, np.int32), np.full((ns, 2), NAN)
    rinv, rhs = np.ascontiguousarray(case["rinv"]), np.ascontiguousarray(case["rhs"])
    rc = lib.probe_factors(C.c_int(maxm), C.c_int(layout), C.c_int(M), C.c_int(Nu), _p(rinv), _p(script),
                           C.c_int(ns), _p(rhs), _p(J), _p(RA), _p(B), _p(ld), _p(li), _p(sc), _p(bt))
    assert rc == 0, (maxm, layout, M, rc)
    if reg:
        Jm = J.reshape(ns, 16, 16)[:, :M, :M]
    else:
        Jm = J.reshape(ns, M, M).transpose(0, 2, 1)      # the dump is J' (sJT[k * M + i] = J(i, k))
    if layout == 1:
        Rm = np.zeros((ns, M, M))
        for j in range(M):
            for i in range(j + 1):
                Rm[:, i, j] = RA[:, j * (j + 3) // 2 + i]
    else:
        Rm = RA.reshape(ns, M, M)
    return dict(J=Jm, RA=Rm, B=B.reshape(ns, 16, 16), rdg=ld[:, 0], uw=ld[:, 1], bs=ld[:, 2], ww=li[:, 0],
                act=li[:, 1], q=sc[:, 0], nrot=sc[:, 1], beta=bt[:, 0])


FACTOR_RATIOS = {}


def check_factors(name, case, o, reg):
    """After every script entry: exact bookkeeping, and every invariant within 8 x the float64
    restatement's own worst residual over the script, never below M eps (Q.factor_tolerance)."""
    M = case["M"]
    tol = {k: Q.factor_tolerance(case, k) for k in ("jj", "ra", "rdg", "b", "bs")}
    rows = 4 if reg else 1
    for e, st in enumerate(case["states"]):
        tag = (name, M, e, case["script"][e])
        q = st["q"]
        assert o["q"][e] == q and o["nrot"][e] == st["nrot"], tag + (o["q"][e], o["nrot"][e], st["nrot"])
        span = 16 if reg else 64
        for r in range(rows):       # the register variant replicates the row vectors over the 16-lane rows
            ww, uw, act = (o[k][e, span * r:span * (r + 1)] for k in ("ww", "uw", "act"))
            assert ww[:q].tolist() == st["ww"] and np.all(ww[q:] == -1), tag
            assert uw[:q].tolist() == st["uw"] and np.all(uw[q:] == 0.0), tag
            assert np.array_equal(act, st["act"][:span]), tag
        res = Q.factor_residuals(case["rinv"], case["Nu"], o["J"][e], np.triu(o["RA"][e]), st["ww"],
                                 None if reg else o["rdg"][e], o["B"][e] if reg else None,
                                 None if reg else o["bs"][e], case["rhs"])
        for k, v in res.items():
            assert v <= tol[k], tag + (k, v, tol[k])
            key = (name, k)
            FACTOR_RATIOS[key] = max(FACTOR_RATIOS.get(key, 0.0), v / max(case["ref_worst"][k], 1e-300))
        if q and case["script"][e][0] == 0:
            assert abs(o["beta"][e] - st["beta"]) <= 64 * M * Q.EPS * max(st["beta"], o["beta"][e]), tag
        if not reg:
            assert np.all(o["bs"][e, q:] == 0.0), tag


@pytest.mark.parametrize("maxm,size", [(m, s) for m, ss in Q.FACTOR_SIZES.items() for s in ss], ids=str)
def test_factor_updates(probe, maxm, size, capsys):
    """gi_add / gi_drop / gi_backsub in both R_A layouts (and gi16_add / gi16_drop at M <= 16) on two
    scripts per size: fill to q == M, drops at 0, q - 1 and across every register-block boundary,
    re-adds of the dropped id, rate and amplitude rows (Q.factor_script).  RAPacked is bitwise
    RAFull."""
    M, Nu = size
    for seed in (1, 2):
        case = Q.factor_case(M, Nu, seed)
        full = run_factors(probe, maxm, 0, case)
        packed = run_factors(probe, maxm, 1, case)
        check_factors("gi_core<%d>" % maxm, case, full, False)
        check_factors("gi_core<%d>" % maxm, case, packed, False)
        for e, st in enumerate(case["states"]):
            q = st["q"]
            assert same_bits(full["J"][e], packed["J"][e]), e
            assert same_bits(np.triu(full["RA"][e])[:q, :q], np.triu(packed["RA"][e])[:q, :q]), e
            for k in ("rdg", "uw"):
                assert same_bits(full[k][e, :q], packed[k][e, :q]), (k, e)
            assert same_bits(full["bs"][e], packed["bs"][e]) and same_bits(full["beta"][e], packed["beta"][e]), e
            assert np.array_equal(full["ww"][e], packed["ww"][e]) and np.array_equal(full["act"][e], packed["act"][e])
        if maxm == 16:
            check_factors("gi16", case, run_factors(probe, 16, 2, case), True)
    with capsys.disabled():
        print("\n  factor ratios (device / restatement) so far:",
              {"%s %s" % k: round(v, 2) for k, v in sorted(FACTOR_RATIOS.items())})
