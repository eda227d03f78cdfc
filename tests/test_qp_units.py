"""CPU side of the device unit tests (tests/test_qp_units_gpu.py): the probe library is built and
exports its entry points, every generated case has the property it is named for (by the reference
alone, tests/qp_unit_ref.py), the reference converges on every case, and the comparison helpers
fail when the reference is perturbed (the negative control)."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import qp_unit_ref as Q

HERE = os.path.dirname(os.path.abspath(__file__))
PROBE = os.path.join(HERE, "device_units", "libmpct_unit_probe.so")
ENTRIES = ("probe_prim", "probe_factors", "probe_qp")


def _exports(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], check=True, capture_output=True, text=True).stdout
    return {ln.split()[-1] for ln in out.splitlines() if ln.strip()}


def test_probe_library_is_built_and_separate(built):
    import __graft_entry__ as g

    assert g.UNIT_PROBE_LIB == PROBE and os.path.exists(PROBE)
    sym = _exports(PROBE)
    assert all(e in sym for e in ENTRIES), sym
    lib = _exports(os.path.join(g.CSRC, "libmpct.so"))
    assert not [e for e in lib if e.startswith("probe_")]
    src = open(g.UNIT_PROBE_SRC).read()
    inc = [ln.split('"')[1] for ln in src.splitlines() if ln.startswith('#include "')]
    assert inc == ["wave_ops.h", "gi_core.h", "gpc_qp.h", "gpc_qp16.h"], inc


@pytest.mark.parametrize("maxm", (16, 32, 64))
def test_generated_cases_have_their_properties(maxm):
    """No case is skipped or filtered: Seq.solve asserts the reference's own KKT residual, and every
    property below is an assertion."""
    for (nu, Nu), d in Q.cases(maxm).items():
        M = nu * Nu
        assert len(d["cold"]) == M - 1
        for s in d["feasible"] + d["cold"] + d["warm"] + d["full"] + d["degenerate"]:
            assert s.cond <= 1e3, (s.name, s.cond)
            for t in range(s.T):
                s.solve(t)
        s = d["feasible"][0]
        assert s.min_slack(1, s.xu[1]) >= 0.0 and len(s.solve(0)["act"]) > 0
        assert s.min_slack(0, s.xu[0]) < -Q.TOL
        for s in d["cold"]:
            r = s.solve(0)
            assert len(r["act"]) == int(s.name[4:]) and r["nondegenerate"], (nu, Nu, s.name)
        for s in d["warm"]:
            counts = [len(s.solve(t)["act"]) for t in range(s.T)]
            sets = [s.solve(t)["act_ids"] for t in range(s.T)]
            assert any(a - b for a, b in zip(sets[1:], sets)) and any(b - a for a, b in zip(sets[1:], sets)), counts
            if maxm == 16 and M >= 2:
                assert Q.first_rebuild_step(s) is not None, (nu, Nu)
        for s in d["degenerate"]:
            r = s.solve(0)
            assert np.linalg.matrix_rank(r["A"][r["act"]]) < len(r["act"]), (nu, Nu)
        assert bool(d["degenerate"]) == (Nu >= 2)
        s = d["full"][0]
        assert len(s.solve(0)["act_ids"]) == M and len(s.solve(1)["act_ids"]) == M
        assert s.solve(0)["act_ids"] != s.solve(1)["act_ids"] and s.min_slack(1, s.xu[1]) < -Q.TOL
        assert {x.name for x in d["infeasible"]} == {"infeasible_box", "infeasible_amp"}
        for s in d["infeasible"]:
            assert Q.is_infeasible(s), (nu, Nu, s.name)


def test_wide_rebuild_sequences_accumulate_their_rotations():
    for shape, s in Q.rebuild_wide_cases().items():
        assert all(len(s.solve(t)["act"]) > 0 for t in range(s.T))
        assert Q.first_rebuild_step(s, Q.REBUILD_WIDE) is not None, shape


def test_primitive_references():
    assert Q.argmin_ref([3.0, 1.0, 1.0, math.nan], [0, 9, 4, 1]) == (1.0, 4)
    assert Q.argmin_ref([0.0, -0.0], [7, 8]) == (0.0, 7)
    assert Q.argmin_ref([math.inf] * 3, [Q.NOID] * 3) == (math.inf, Q.NOID)
    assert Q.argmin_ref([math.nan], [3]) == (math.inf, Q.NOID)
    v = np.arange(64.0) + 1
    assert Q.shift_ref(v, 16, +1)[15] == 0 and Q.shift_ref(v, 16, +1)[14] == 16 and Q.shift_ref(v, 16, -1)[16] == 0
    assert Q.shift_ref(v, 64, +1)[63] == 64 and Q.shift_ref(v, 64, -1)[0] == 1 and Q.shift_ref(v, 64, +1)[15] == 17
    assert Q.block_prefix_terms(v, 6, 3)[4] == [4.0, 5.0] and Q.block_prefix_terms(v, 6, 3)[7] == [8.0]
    assert Q.ulps_off(1.0 / 3.0, Q.rcp_exact(3.0)) < 0.5
    assert Q.ulps_off(1.0 / math.sqrt(2.0), Q.rsq_exact(2.0)) <= 1.0
    assert Q.ulps_off(0.25, Q.rsq_exact(16.0)) == 0.0


def test_negative_control_comparisons_fail_on_a_perturbed_reference():
    """The helpers the GPU tests assert with reject a subtly wrong answer: a tie broken to the largest
    id, a sum off by a few ulps, an optimum moved by 1e-8 or with one active bound released."""
    vals, ids = [2.0, 1.0, 1.0, 5.0], [3, 8, 6, 1]
    assert Q.argmin_matches(1.0, 6, vals, ids)
    assert not Q.argmin_matches(1.0, 8, vals, ids)          # largest id among the ties
    assert not Q.argmin_matches(math.nextafter(1.0, 2.0), 6, vals, ids)
    assert not Q.argmin_matches(math.nan, 6, vals + [math.nan], ids + [0])
    row = [0.1 * k for k in range(16)]
    good = math.fsum(row)
    assert Q.sum_check(good, row, 4)
    assert not Q.sum_check(good * (1 + 8 * Q.EPS), row, 4)
    assert not Q.sum_check(good - row[15], row, 4)           # one lane dropped
    s = Q.cases(16)[(3, 5)]["cold"][6]
    r = s.solve(0)
    assert Q.x_ratio(s, 0, r["x"]) == 0.0
    bad = r["x"].copy()
    bad[0] += 1e-8
    assert Q.x_ratio(s, 0, bad) > 8.0
    m = int(min(r["act_ids"])) >> 2
    off = r["x"].copy()
    off[m] *= 1.0 + 1e-6                                     # pushed through its active bound
    assert s.min_slack(0, off) < Q.slack_floor(s, off)
    assert Q.ulps_off(math.nextafter(math.nextafter(0.5, 1), 1), Q.rcp_exact(2.0)) == 2.0


@pytest.mark.parametrize("maxm", (16, 32, 64))
def test_factor_scripts_have_their_properties(maxm):
    """Every script fills the set (q == M), drops at position 0 and at q - 1, re-adds a dropped id,
    crosses every register-block boundary that M has, adds rate and amplitude rows, and agrees with
    its own bookkeeping; the float64 restatement keeps every invariant to a few M eps (longdouble)."""
    for M, Nu in Q.FACTOR_SIZES[maxm]:
        for seed in (1, 2):
            c = Q.factor_case(M, Nu, seed)
            q, qs, last_drop, seen = 0, [], None, dict(first=False, last=False, readd=False, cross=set())
            for (kind, arg), st in zip(c["script"], c["states"]):
                if kind == 0:
                    seen["readd"] |= last_drop == arg
                    q += 1
                else:
                    assert 0 <= arg < q
                    seen["first"] |= arg == 0 and q > 1
                    seen["last"] |= arg == q - 1 and q > 1
                    seen["cross"] |= {jj >> 2 for jj in range(arg, q - 1) if jj & 3 == 3}
                    assert Q.crosses_block_boundary(arg, q) == any(jj & 3 == 3 for jj in range(arg, q - 1))
                    last_drop = c["states"][len(qs) - 1]["ww"][arg]
                    q -= 1
                qs.append(q)
                assert st["q"] == q and len(set(p >> 2 for p in st["ww"])) == q
                assert sum(bin(int(a)).count("1") for a in st["act"]) == q
            assert max(qs) == M and seen["first"] and seen["last"] and seen["readd"], (M, seen)
            assert seen["cross"] == set(range((M - 1) // 4)), (M, seen["cross"])
            kinds = {p & 3 for k, p in c["script"] if k == 0}
            assert kinds & {0, 1} and kinds & {2, 3}, (M, kinds)
            assert all(v <= 64 * M * Q.EPS for k, v in c["ref_worst"].items() if k != "b"), c["ref_worst"]
            assert c["ref_worst"]["b"] <= 1e3 * 64 * M * Q.EPS     # |B R_A - I| scales with cond(R_A) <= cond(R)


def test_negative_control_one_rotation_sign():
    """One Givens rotation applied to J with the wrong sign: J J' stays H^-1 (the flipped rotation is
    still orthogonal), but J'N_A = [R_A; 0] breaks far beyond the tolerance, and only from the entry
    of that rotation on."""
    good, bad = Q.factor_case(15, 5, 1), Q.factor_case(15, 5, 1, flip=2)
    tol = Q.factor_tolerance(good, "ra")
    assert good["ref_worst"]["ra"] <= tol and bad["ref_worst"]["ra"] > 1e6 * tol
    assert bad["ref_worst"]["jj"] <= Q.factor_tolerance(good, "jj")
    first = next(e for e, s in enumerate(bad["states"]) if s["res"].get("ra", 0.0) > tol)
    assert good["script"][first][0] == 1     # it shows at a drop
    assert all(np.array_equal(a["J"], b["J"]) for a, b in zip(good["states"][:first], bad["states"][:first]))
