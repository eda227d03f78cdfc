"""CPU side of the prologue's unit tests (tests/test_prologue_units_gpu.py): the probe library is built,
separate from libmpct.so and includes the three headers only; every generated case has the properties it
is named for, by the reference alone (tests/prologue_ref.py); the float64 restatement stays within half of
every bound and passes the checking function the GPU test uses; and that function rejects the restatement
with each of the six planted errors (the negative controls)."""
import os
import re
import subprocess

import numpy as np
import pytest

import prologue_ref as P

HERE = os.path.dirname(os.path.abspath(__file__))
PROBE = os.path.join(HERE, "device_units", "libmpct_prologue_probe.so")
RUNS = [(name, inst) for name, f in P.FAMILIES.items() for inst in f["insts"]]


def _exports(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], check=True, capture_output=True, text=True).stdout
    return {ln.split()[-1] for ln in out.splitlines() if ln.strip()}


def test_prologue_probe_library_is_built_and_separate(built):
    import __graft_entry__ as g

    assert g.PROLOGUE_PROBE_LIB == PROBE and os.path.exists(PROBE)
    assert "probe_prologue" in _exports(PROBE)
    assert not [e for e in _exports(os.path.join(g.CSRC, "libmpct.so")) if e.startswith("probe_")]
    src = open(g.PROLOGUE_PROBE_SRC).read()
    inc = [ln.split('"')[1] for ln in src.splitlines() if ln.startswith('#include "')]
    assert inc == ["mpct_dev.h", "wave_ops.h", "gpc_prologue.h"], inc
    assert "prologue_probe.hip" in open(g.__file__).read().split("def kernel_isa")[1].split("def build")[0]


def test_probe_instances_are_the_trees(built):
    """Every gpc_prologue<...> the kernels instantiate is an instance of the probe with the same template
    arguments, and the reference's table of instances agrees with the probe's launch switch."""
    import __graft_entry__ as g

    def args_of(text):
        out = set()
        for m in re.finditer(r"gpc_prologue<([^>]*)>\(", text):
            a = [x.strip() for x in m.group(1).split(",")]
            a += ["false", "true", "false", "8", "false"][len(a) - 1:]
            out.add(tuple(a))
        return out

    used = set()
    for k in ("gpc_kernel.hip", "gpc_small.hip", "dtc_small.hip", "dtc_robust.hip"):
        used |= args_of(open(os.path.join(g.CSRC, k)).read())
    assert "#define MPCT_DTC_HB 4" in open(os.path.join(g.CSRC, "dtc_small.hip")).read()
    want = set()
    for a in used:
        a = tuple("4" if x == "MPCT_DTC_HB" else x for x in a)
        want |= {(m,) + a[1:] for m in (("16", "32", "64") if a[0] == "MAXM" and a[3] == "false" else
                                        ("16", "32") if a[0] == "MAXM" else (a[0],))}
    src = open(g.PROLOGUE_PROBE_SRC).read()
    launched = {}
    for m in re.finditer(r"(case \d+|default): MPCT_LAUNCH\(([^)]*)\)", src):
        k = 9 if m.group(1) == "default" else int(m.group(1).split()[1])
        launched[k] = tuple(x.strip() for x in m.group(2).split(","))
    assert sorted(launched) == sorted(P.INSTANCES)
    b = lambda v: "true" if v else "false"
    for k, I in P.INSTANCES.items():
        assert launched[k] == (str(I["maxm"]), b(I["packed"]), b(I["rinv"]), b(I["first"]), str(I["khb"]), b(I["tables"])), k
    assert want == {launched[k] for k in P.PRODUCTION}, (want, launched)
    assert "%#x" % P.SENTINEL in src.lower() and "kGuard = %d" % P.GUARD in src


def test_cell_offsets_are_the_host_builders():
    """cell_offsets against the figures tests/test_qr_tables.py holds qr_tables to on Shell 3x3."""
    off, total = P.cell_offsets(3, 3, 35, 30, 5)
    assert total == 151440 and int((off >= 0).sum()) == 140 and off[0] == 0 and off[1] == -1
    assert off[(2 - 1) * 5 + 0] == 3 * 1 * 38 and off[(2 - 1) * 5 + 1] == 3 * 38 + 3 * 2 * 38


def test_the_sizes_cover_what_they_are_chosen_for():
    seen = dict(M=set(), passes=set(), total=set(), first_short=False, tab_my=set(), straddle=False)
    for name, inst in RUNS:
        I = P.INSTANCES[inst]
        for c in P.family_cases(name, inst):
            M, khb, my, N2, nx, Nu = c["M"], I["khb"], c["my"], c["N2"], c["nx"], c["Nu"]
            assert M <= I["maxm"] and M < 64 and M == c["nu"] * Nu
            seen["M"].add((I["maxm"], M))
            seen["passes"].add((M, -(-nx // (64 - M))))
            seen["total"].add((I["maxm"], M + nx))
            rem = (my * N2) % khb
            seen.setdefault("rows%d" % khb, set()).add("multiple" if rem == 0 and my * N2 else "short" if rem == khb - 1 else
                                                       "sub" if my * N2 < khb else "other")
            seen.setdefault("shape", set()).update({"Nu1"} if Nu == 1 else set(), {"NuM"} if Nu == M else set(),
                                                   {"N2<M"} if N2 < M else set(), {"N2=1"} if N2 == 1 else set())
            if P.table_in_use(c, inst):
                seen["tab_my"].add(my)
                seen["straddle"] |= khb % my != 0
    assert {(16, 1), (16, 16), (32, 32), (64, 63)} <= seen["M"]
    assert {(63, 1), (63, 2), (63, 3), (63, 4), (16, 3), (32, 3)} <= seen["passes"]
    assert {(16, 63), (16, 64), (16, 65), (32, 63), (32, 64), (32, 65), (64, 63), (64, 64), (64, 65)} <= seen["total"]
    for khb in (4, 8, 12):
        assert {"multiple", "short", "sub"} <= seen["rows%d" % khb], (khb, seen["rows%d" % khb])
    assert seen["shape"] == {"Nu1", "NuM", "N2<M", "N2=1"} and seen["tab_my"] >= {1, 2, 3, 5} and seen["straddle"]
    assert {c["wsq"] for c in P.CASES.values()} == {0, 1}
    assert set(np.unique(np.concatenate([c["n1"] for c in P.CASES.values()])).tolist()) == {0, 1, 3}


@pytest.mark.parametrize("name,inst", RUNS, ids=["%s-%d" % r for r in RUNS])
def test_generated_cases_and_restatement(name, inst):
    """No case is filtered out or skipped.  By the truth: cond(W) <= 1e6 (the stiff family: 5e5 .. 1e6),
    weights of both signs spanning 1e-5 .. 1, the named zero columns.  The restatement, handed to
    check_case in the form the probe dumps, passes with every ratio <= 1/2."""
    for c in P.family_cases(name, inst):
        W, _ = P.build_W(c["step"], c["phi"], c["n1"], c["delta"], c["lam"], c["wsq"], c["N2"], c["Nu"])
        G = W[:c["my"] * c["N2"]]
        res = P.restate(c, inst)
        lds, flags = P.image_of(c, inst, res)
        if not c["expect_ok"]:
            zero = np.nonzero(~W.any(axis=0))[0]
            assert len(zero) or np.isnan(c["delta"]).any(), c["key"]
            assert not res["ok"] and P.check_case(c, inst, lds, flags) == {}
            continue
        tr = P.truth_of(c)
        assert tr["ok"] and tr["cond"] <= P.COND_CAP, (c["key"], tr["cond"])
        if c.get("stiff"):
            assert tr["cond"] >= 0.5 * P.COND_CAP, (c["key"], tr["cond"])
        else:
            w = np.abs(np.concatenate([c["delta"], c["lam"]])) ** (2 if c["wsq"] else 1)
            assert w.max() == 1.0 and abs(w.min() - 1e-5) < 1e-18 and (c["delta"] > 0).any() and (c["lam"] < 0).any()
        if c["key"] in ("stream16/5", "stream16/6", "tables/5"):
            assert (~G.any(axis=0)).any(), c["key"]          # columns of G that are exactly zero
        assert res["ok"] and res["nrefl"] == P.reflections(c, inst)
        out = P.check_case(c, inst, lds, flags)
        assert out and max(out.values()) <= 0.5, (c["key"], out)
    if name == "tables" and inst == 3:
        pairs = [(P.reflections(c, 3), P.reflections(c, 4)) for c in P.family_cases(name, 3)]
        assert all(a <= b for a, b in pairs) and sum(a < b for a, b in pairs) >= 4, pairs


# ---------------------------------------------------------------------------------------------
# the negative controls: check_case must reject each
def _rejected(case, inst, res=None, **image):
    res = P.restate(case, inst) if res is None else res
    with pytest.raises(AssertionError):
        P.check_case(case, inst, *P.image_of(case, inst, res, **image))


CONTROL = [("stream16/1", 0), ("stream16/2", 4), ("tables/6", 3), ("tables/3", 3), ("first16/1", 5), ("stream64/1", 2)]


@pytest.mark.parametrize("key,inst", CONTROL)
def test_negative_controls_on_the_rows(key, inst):
    """A dropped last row of the padded block, delta_0 (the largest weight) scaled by 1 + 1e-9, n1 off by
    one.  The table cases have N2 < M, where the last table row is a full trapezoid row; with N2 >= M it is
    row M - 1 of a smooth plant's R_i, a single entry too small for any bound to see."""
    c = P.CASES[key]
    P.check_case(c, inst, *P.image_of(c, inst, P.restate(c, inst)))
    _rejected(c, inst, P.restate(c, inst, drop_last_row=True))
    if not P.table_in_use(c, inst):
        _rejected(c, inst, P.restate(c, inst, n1=c["n1"] + 1))
    d = c["delta"].copy()
    d[0] *= 1.0 + 1e-9
    _rejected(c, inst, P.restate(c, inst, delta=d))


@pytest.mark.parametrize("key", ["tables/1", "tables/2", "tables/3", "tables/6"])
def test_negative_control_block_starts_one_level_too_high(key):
    """k0 one level too high skips a reflection a block needs: R'R = W'W breaks."""
    c = P.CASES[key]
    _rejected(c, 3, P.restate(c, 3, k0_bump=1))


def test_negative_control_column_from_the_wrong_pass():
    c = P.CASES["pass16/nx49"]
    _rejected(c, 0, a_swap=(0, 48))          # state column 0's gain taken from pass 1's lane
    c = P.CASES["stream64/nx2"]
    _rejected(c, 2, a_swap=(0, 1))


@pytest.mark.parametrize("key,inst", [("tables/1", 3), ("stream16/1", 4)])
def test_negative_control_packed_index_off_by_one(key, inst):
    c = P.CASES[key]
    _rejected(c, inst, pack_shift=1)
    _rejected(c, inst, pack_shift=-1)


def test_negative_controls_on_the_image():
    """A word written outside the three arrays, a lane that disagrees on the flag, a nonzero below the
    diagonal of the full R^-1, a flag that claims success for a singular R."""
    c, inst = P.CASES["stream16/1"], 0
    lds, flags = P.image_of(c, inst, P.restate(c, inst))
    L = P.layout_of(inst, c["M"], c["Nu"], c["astride"])
    P.check_case(c, inst, lds, flags)

    def bad(change):
        l2, f2 = lds.copy(), flags.copy()
        change(l2, f2)
        with pytest.raises(AssertionError):
            P.check_case(c, inst, l2, f2)

    bad(lambda l, f: l.__setitem__(L["end"], 0.0))                    # the closing guard
    bad(lambda l, f: l.__setitem__(L["a"] + c["nx"], 0.0))            # a column of sA past nx (astride 7, nx 5)
    bad(lambda l, f: f.__setitem__(63, 0))
    bad(lambda l, f: l.__setitem__(L["ri"] + 5 * c["M"] + 2, 1e-300))
    bad(lambda l, f: l.__setitem__(L["ri"] + 5 * c["M"] + 2, -0.0))
    c, inst = P.CASES["first16/1"], 5
    lds, flags = P.image_of(c, inst, P.restate(c, inst))
    L = P.layout_of(inst, c["M"], c["Nu"], c["astride"])
    lds[L["ri"] + 3] = 1.0                                            # RINV = false touched its region
    with pytest.raises(AssertionError):
        P.check_case(c, inst, lds, flags)
    c = P.CASES["notpd/0"]
    good = dict(c, expect_ok=True, lam=np.abs(c["lam"]) + 0.1, key="notpd/0+")
    with pytest.raises(AssertionError):
        P.check_case(c, 0, *P.image_of(good, 0, P.restate(good, 0)))
