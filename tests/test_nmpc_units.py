"""CPU: the truth of the NMPC kernel's one-step tests (tests/nmpc_step_ref.py) against the project's float64
oracle (oracle/nmpc_vdv.py), the KKT certificate and the decision margins of every case of
tests/test_nmpc_units_gpu.py, the bound table, the mutation check that shows those tests can fail, and the
LDS layout of nmpc_model.h restated against mpct_lds_bytes."""
import re

import numpy as np
import pytest

import nmpc_step_ref as S


def _mp(v):
    return [S.mpf(float(t)) for t in v]


def _fl(v):
    return np.array([float(t) for t in v])


@pytest.fixture(scope="module")
def golden():
    z = np.load(S.GOLDEN)
    return {c["name"]: {k.rsplit("/", 1)[1]: z[k] for k in z.files if k.rsplit("/", 1)[0] == c["name"]} for c in S.CASES}


def test_rhs_and_rk4_match_the_oracle():
    import oracle.nmpc_vdv as nv

    np.testing.assert_array_equal(S.VDV_PARAMS, [nv.K10, nv.K20, nv.K30, nv.E1, nv.E2, nv.E3, nv.DHAB, nv.DHBC, nv.DHAD,
                                                 nv.RHO, nv.CP, nv.KW, nv.AR, nv.VR, nv.T0, nv.CA0])
    np.testing.assert_allclose(S.steady_state(), nv.steady_state(), rtol=1e-14)
    rng = np.random.default_rng(3)
    p = _mp(S.VDV_PARAMS)
    for _ in range(4):
        x = rng.uniform(S.XMIN, S.XMAX)
        u = rng.uniform(S.UMIN, S.UMAX)
        xd, ud = rng.standard_normal(3), rng.standard_normal(2)
        f, fd = S.rhs(p, _mp(x), _mp(u), _mp(xd), _mp(ud))
        J = nv.jac(x, u)
        np.testing.assert_allclose(_fl(f), nv.rhs(x, u), rtol=1e-12, atol=1e-12 * np.abs(nv.rhs(x, u)).max())
        np.testing.assert_allclose(_fl(fd), J[:, :3] @ xd + J[:, 3:] @ ud, rtol=1e-11, atol=1e-11 * np.abs(J).max())
        xe, X = nv.rk4(x, u, (np.eye(3, 5), np.eye(5)[3:]))
        seeds = [list(e) for e in np.eye(5)]
        xm, Xm = S.rk4(p, S.mpf(nv.TS), nv.NSUB, _mp(x), _mp(u), [_mp(e[:3]) for e in seeds], [_mp(e[3:]) for e in seeds])
        np.testing.assert_allclose(_fl(xm), xe, rtol=1e-13)
        np.testing.assert_allclose(np.array([_fl(t) for t in Xm]).T, X, rtol=1e-11, atol=1e-13)
        xf = S._rk4_v(S.VDV_PARAMS, nv.TS / nv.NSUB, nv.NSUB, list(x), list(u), [np.eye(3, 5)[i] for i in range(3)],
                      [np.eye(5)[3 + i] for i in range(2)])
        np.testing.assert_allclose(np.array(xf[1]), X, rtol=1e-11, atol=1e-13)


def test_the_truth_is_multiprecision():
    """rhs of mpf input is mpmath throughout, the Arrhenius exponentials included (MP is a clone of mpmath.mp with
    an mpf class of its own): the 40-digit value and tangent equal a 60-digit evaluation to 1e-30 relative, and
    differ from the float64 evaluation by rounding."""
    rng = np.random.default_rng(4)
    for _ in range(6):
        x, u = rng.uniform(S.XMIN, S.XMAX), rng.uniform(S.UMIN, S.UMAX)
        xd, ud = rng.standard_normal(3), rng.standard_normal(2)
        f40 = S.rhs(_mp(S.VDV_PARAMS), _mp(x), _mp(u), _mp(xd), _mp(ud))
        assert all(isinstance(t, S.mpf) for part in f40 for t in part)
        with S.MP.workdps(60):
            f60 = S.rhs(_mp(S.VDV_PARAMS), _mp(x), _mp(u), _mp(xd), _mp(ud))
            for a, b in zip(f40[0] + f40[1], f60[0] + f60[1]):
                assert abs(a - b) < S.mpf(10) ** -30 * max(abs(t) for t in f60[0] + f60[1])
        f64 = S.rhs(S.VDV_PARAMS, list(x), list(u), list(xd), list(ud))
        d = max(abs(S.mpf(a) - b) for a, b in zip(f64[0] + f64[1], f40[0] + f40[1])) / max(abs(t) for t in f40[0] + f40[1])
        assert 0 < d < 1e-13
    x = S.rk4(_mp(S.VDV_PARAMS), S.mpf(S.TS), 2, _mp(S.steady_state()), _mp(S.U0))
    assert all(isinstance(t, S.mpf) for t in x) and isinstance(S._exp(S.mpf(1) / 3), S.mpf)


@pytest.mark.parametrize("xmax", [S.XMAX, (6.0, 1.2, 136.5)], ids=["box", "state-rows"])
def test_one_step_matches_the_oracle_controller(monkeypatch, xmax):
    """oracle.nmpc_vdv.controller with SQP_MAX = 1 (and the kernel's nsub = 10): the truth's step is the
    oracle's to the oracle's own accuracy, box-only and with active state rows."""
    import oracle.nmpc_vdv as nv

    monkeypatch.setattr(nv, "SQP_MAX", 1)
    x0 = nv.steady_state()
    N, Nu, delta, lam = 6, 3, (1.0, 0.5), (0.05, 0.02)
    rvec = np.array([0.95, 139.0])
    U, it = nv.controller(x0, nv.U0, rvec, N, Nu, np.array(delta), np.array(lam), np.tile(nv.U0, (Nu, 1)),
                          (nv.XMIN, np.array(xmax)))
    P = S.Prob(N, Nu, delta, lam, nsub=nv.NSUB, x_max=xmax)
    rec = S.gn_step(P, _mp(x0), _mp(nv.U0), _mp(rvec), [_mp(nv.U0) for _ in range(Nu)])
    assert rec["certified"] and not rec["converged"] and it == 1
    assert bool(rec["active"]) == (xmax != S.XMAX)
    assert S.measure([_fl(r) for r in rec["U"]], U) < 1e-9


def test_fixture_is_what_the_truth_gives(golden):
    """The short cases regenerated (mpmath truth, restatement, planted errors) equal the committed fixture;
    the long-horizon ones are held to the fixture's own certificate below."""
    for c in S.CASES:
        if not c["short"]:
            continue
        got = S.run_case(c)
        for k in ("x0", "refs", "u", "uopt"):
            np.testing.assert_allclose(got[k], golden[c["name"]][k], rtol=0, atol=1e-13, err_msg=c["name"] + "/" + k)
        np.testing.assert_allclose(got["bounds_edge"], golden[c["name"]]["bounds_edge"], rtol=1e-9, atol=1e-13)
        for k in ("iters", "maxiter", "early", "nactive", "drops", "took", "kinds"):
            np.testing.assert_array_equal(got[k], golden[c["name"]][k], err_msg=c["name"] + "/" + k)
        assert float(got["err"]) <= float(golden[c["name"]]["err"]) * (1 + 1e-12), c["name"]
        # and what the regenerated case itself shows: certificate, margins, both planted errors
        bound = S.bound_table(golden)[c["family"]][1]
        assert float(got["slack"]) > S.KKT_MARGIN and float(got["mult"]) > S.KKT_MARGIN, c["name"]
        assert float(got["tie"]) > S.TIE_MARGIN and float(got["conv"]) > S.CONV_MARGIN, c["name"]
        assert float(np.min(got["mut"])) >= S.MUTATION_FACTOR * bound, (c["name"], got["mut"], bound)


def test_every_case_is_certified_and_clear_of_ties(golden):
    for c in S.CASES:
        g = golden[c["name"]]
        assert str(g["case"]) == S.case_key(c), c["name"] + ": the case changed, regenerate the fixture"
        assert float(g["slack"]) > S.KKT_MARGIN and float(g["mult"]) > S.KKT_MARGIN, c["name"]
        assert float(g["tie"]) > S.TIE_MARGIN, (c["name"], float(g["tie"]))
        assert float(g["conv"]) > S.CONV_MARGIN, (c["name"], float(g["conv"]))
        assert g["u"].shape == (len(c["tstars"]), 2, c["nit"]) and g["uopt"].shape == (len(c["tstars"]), c["Nu"], 2)
        # the held reference converges at once at every call; so does every call before the step
        # (with a first step at t = 1, `pre`, that call alone does not)
        assert g["early"].all() and bool(g["maxiter"][-1]) == bool(c["pre"]) and g["maxiter"][:-1].all(), c["name"]
        assert g["iters"][-1] == c["nit"]
        # no loop sets MPCT_ST_BOUNDS: every closed-loop state is inside the bounds by more than 1e-6 K (or mol/l)
        assert np.all(g["bounds_edge"] > 1e-6), (c["name"], g["bounds_edge"])
    g = golden
    assert "hi0" in str(g["c/first"]["kinds"]) and "lo0" in str(g["c/first"]["kinds"])
    assert str(g["c/cum"]["kinds"]) == "hi"                      # a cumulative bound alone
    assert str(g["c/state"]["kinds"]) == "xmax" and int(g["c/state"]["nactive"]) >= 2
    assert int(g["c/state-drop"]["drops"]) >= 1 and int(g["c/state-drop"]["nactive"]) >= 1   # added and dropped
    assert all(int(g[n]["nactive"]) > 0 for n in g if n.startswith("c/"))
    assert str(g["e/4-2"]["took"]).endswith("anderson") and str(g["e/8-7"]["took"]).endswith("anderson")
    assert str(g["e/8-7-full"]["took"]) == "armijo0,armijo0" and str(g["e/4-2-halved"]["took"]) == "armijo0,armijo2"
    assert all(int(g[n]["iters"][0]) == BY_ITERS[n] for n in BY_ITERS)


# closed-loop calls before the step (one iteration each) + two calls at the step of two iterations
BY_ITERS = {"e/4-2": 1 + 2 + 2, "e/8-7": 6 + 2 + 2, "a/4-2": 3, "a/127-7": 8}


def test_bound_table_and_mutations(golden):
    """Every bound is 8 x a CPU-measured restatement error; a tangent entry off by 1e-6 and a dropped rotation
    each move every family's step by more than 100 x its bound; the docstring's table is the fixture's."""
    tab = S.bound_table(golden)
    rows = re.search(r"BOUND_TABLE_BEGIN\n(.*?)BOUND_TABLE_END", S.__doc__, re.S).group(1).strip().splitlines()[1:]
    doc = {r.split()[0]: [float(t) for t in r.split()[1:]] for r in rows}
    assert sorted(doc) == sorted(tab) == S.FAMILIES
    for fam, (e, b, m) in tab.items():
        assert b == S.DEVICE_FACTOR * e and e > 0.0
        assert m >= S.MUTATION_FACTOR, (fam, m)
        np.testing.assert_allclose(doc[fam], [e, b, m], rtol=5e-3, err_msg=fam)
    for c in S.CASES:       # and case by case
        assert float(np.min(golden[c["name"]]["mut"])) >= S.MUTATION_FACTOR * tab[c["family"]][1], c["name"]


def test_probe_bounds_are_the_restatements(built):
    """The probe's bounds: the restatement's errors over the probe's cases, recomputed, are the fixture's and the
    docstring's; every one is positive (the truth is not the restatement)."""
    z = np.load(S.GOLDEN)
    rows = re.search(r"PROBE_TABLE_BEGIN\n(.*?)PROBE_TABLE_END", S.__doc__, re.S).group(1).strip().splitlines()[1:]
    doc = {r.split()[0]: [float(t) for t in r.split()[1:]] for r in rows}
    for which, kind in S.PROBE_RUNS:
        rv, rd = S.probe_reference(which, kind)[4:]
        assert (rv, rd) == tuple(z["probe/%s-%s" % (which, kind)]) and rv > 0 and rd > 0
        np.testing.assert_allclose(doc[which + "-" + kind], [rv, S.DEVICE_FACTOR * rv, rd, S.DEVICE_FACTOR * rd], rtol=5e-3)


def test_lds_layout_restated(built):
    """nm_layout / nm_groups restated equal mpct_lds_bytes for every even M in 2..32 and every N in 1..127 that a
    scenario accepts (64 KiB), and the pieces of a layout do not overlap."""
    from mpct import nmpc
    from mpct.engine import MpctError

    x0 = nmpc.steady_state()
    yref = nmpc.vandevusse_signals(x0, 4)[1]
    seen = set()
    worst = np.array([[S.lds_bytes(m, n) for n in range(1, 128)] for m in range(1, 33)])    # [m - 1][n - 1]
    for nu_max in range(1, 17):
        M = 2 * nu_max
        fits = np.maximum.accumulate(worst[:M].max(axis=0)) <= 64 * 1024      # every m <= M, every n' <= n
        n_max = int(np.flatnonzero(fits).max()) + 1
        if n_max < 127:
            with pytest.raises(MpctError, match="64 KiB"):
                nmpc.NmpcScenario(x0, nmpc.VDV_U0, nmpc.VDV_UMIN, nmpc.VDV_UMAX, nmpc.VDV_XMIN, nmpc.VDV_XMAX, yref,
                                  n_max + 1, nu_max)
        sc = nmpc.NmpcScenario(x0, nmpc.VDV_U0, nmpc.VDV_UMIN, nmpc.VDV_UMAX, nmpc.VDV_XMIN, nmpc.VDV_XMAX, yref,
                               n_max, nu_max)
        for N in range(1, n_max + 1):
            assert sc.lds_bytes(N, nu_max) == S.lds_bytes(M, N), (M, N)
            G = S.nm_groups(M, N)
            seen.add(G)
            pieces, total = S.nm_layout(M, N, G)
            spans = sorted((o, o + n) for _, o, n in pieces)
            assert all(a[1] <= b[0] for a, b in zip(spans, spans[1:])) and spans[-1][1] <= total, (M, N)
        sc.close()
    assert seen == {1, 2, 4}
    assert S.nm_groups(14, 70) == 2 and S.nm_groups(14, 127) == 1 and S.nm_groups(14, 8) == 4
    assert S.nm_groups(16, 9) == 1 and S.nm_groups(4, 4) == 4
