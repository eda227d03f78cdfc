"""CPU side of the band kernel's factor unit tests (tests/test_band_factors_gpu.py): the probe library
is built, separate from libmpct.so and includes the three headers only; every generated case has the
properties it is named for, by the reference alone (tests/band_factor_ref.py); the float64 restatement
passes the checking function the GPU test uses; and that function rejects the restatement with one
rotation's sine negated on J, and with one row of B written one slot off (the negative controls)."""
import os
import re
import subprocess

import numpy as np
import pytest

import band_factor_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))
PROBE = os.path.join(HERE, "device_units", "libmpct_band_probe.so")
ENTRIES = ("probe_band_prefix", "probe_band_factors")
RUN_IDS = ["%d-%d-%s" % (m, z, "full" if f else "diag") for m, z, f in R.RUNS]


def _exports(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], check=True, capture_output=True, text=True).stdout
    return {ln.split()[-1] for ln in out.splitlines() if ln.strip()}


def test_band_probe_library_is_built_and_separate(built):
    import __graft_entry__ as g

    assert g.BAND_PROBE_LIB == PROBE and os.path.exists(PROBE)
    sym = _exports(PROBE)
    assert all(e in sym for e in ENTRIES), sym
    lib = _exports(os.path.join(g.CSRC, "libmpct.so"))
    assert not [e for e in lib if e.startswith("probe_")]
    src = open(g.BAND_PROBE_SRC).read()
    inc = [ln.split('"')[1] for ln in src.splitlines() if ln.startswith('#include "')]
    assert inc == ["wave_ops.h", "gi_core.h", "band_b.h"], inc
    assert "band_b.h" in g.HEADERS and "band_b.h" in g.BAND_PROBE_HEADERS


def test_the_band_kernel_takes_its_factor_code_from_the_header():
    """band_b.h holds the seven pieces and mdband_kernel.hip includes it and defines none of them."""
    import __graft_entry__ as g

    hdr = open(os.path.join(g.CSRC, "band_b.h")).read()
    kern = open(os.path.join(g.CSRC, "mdband_kernel.hip")).read()
    assert '#include "band_b.h"' in kern and '#include "gi_core.h"' in hdr
    for name in ("bt_idx", "bt_mul", "bt_tmul", "wave_prefix_sum", "band_drop_b"):
        assert re.search(r"__forceinline__ \w+ %s\(" % name, hdr), name
        assert not re.search(r"__forceinline__ \w+ %s\(" % name, kern), name
    for name in ("BandBAdd", "BandMark"):
        assert "struct %s {" % name in hdr and "struct %s {" % name not in kern, name


def test_packed_index_agrees_with_the_header():
    """bt_idx and packed_size against gi_core.h's ra_packed_size (its expression, read from the header):
    the columns tile the array exactly, column k holding rows 0 .. k + 1."""
    import __graft_entry__ as g

    src = open(os.path.join(g.CSRC, "gi_core.h")).read()
    m = re.search(r"constexpr int ra_packed_size\(int M\) \{ return (.*?); \}", src)
    assert m, "ra_packed_size not found"
    for Mz in range(1, 65):
        assert R.packed_size(Mz) == eval(m.group(1).replace("/", "//"), {"M": Mz}), Mz
        idx = [R.bt_idx(w, k) for k in range(Mz) for w in range(k + 2)]
        assert idx == list(range(R.packed_size(Mz))), Mz
    B = np.triu(np.arange(1.0, 26.0).reshape(5, 5))
    packed = R.pack_b(B, 7)
    assert np.array_equal(R.unpack_b(packed, 5), B)
    assert all(packed[R.bt_idx(k + 1, k)] == 0.0 for k in range(5)) and np.isnan(packed[R.bt_idx(0, 5):]).all()


@pytest.mark.parametrize("maxm,Mz,full_ri", R.RUNS, ids=RUN_IDS)
def test_generated_cases_have_their_properties(maxm, Mz, full_ri):
    """No case is filtered out or skipped: band_script raises when it cannot go on, and every property
    below is an assertion."""
    assert Mz <= maxm and (maxm == 16 or Mz > maxm // 2) and (Mz - 1) % R.NU[Mz] == 0
    for seed in R.SEEDS:
        c = R.band_case(Mz, full_ri, seed)
        ids, base, normals = c["ids"], c["base"], c["normals"]
        assert base == 4 * Mz and len(ids) == 3 * Mz == len(set(ids.tolist())) and normals.shape == (3 * Mz, Mz)
        assert ids.max() < base + 32 * R.BIT_WORDS
        out = np.nonzero(ids >= base)[0]
        assert len(out) == 2 * Mz and np.all(normals[out, -1] > 0.0)                  # v > 0
        for a, b in zip(out[::2], out[1::2]):                                          # pairs sharing g
            assert ids[b] == ids[a] + 1 and (ids[a] - base) % 2 == 0
            assert np.array_equal(normals[a, :-1], -normals[b, :-1]) and np.all(normals[a, :-1] != 0.0)
        assert int(ids[Mz - 1]) == 4 * (Mz - 1) and np.array_equal(normals[Mz - 1], np.eye(Mz)[Mz - 1])   # eps
        q, qs, seen = 0, [], dict(first=False, last=False, q1=False, readd=False, kds=set())
        last_drop = None
        for e, ((kind, arg), st) in enumerate(zip(c["script"], c["states"])):
            if kind == 0:
                seen["readd"] |= last_drop == arg
                q += 1
            else:
                assert 0 <= arg < q
                seen["first"] |= arg == 0 and q > 1
                seen["last"] |= arg == q - 1 and q > 1
                seen["q1"] |= q == 1
                if arg < q - 1:
                    seen["kds"].add(arg)
                last_drop = c["states"][e - 1]["rows"][arg]
                q -= 1
            qs.append(q)
            assert st["q"] == q == len(set(st["rows"])) and st["cond"] <= R.COND_CAP, (Mz, seed, e, st["cond"])
            assert st["amp"] <= R.AMP_PER_MZ * Mz, (Mz, seed, e, st["amp"])
            assert [int(ids[r]) for r in st["rows"]] == st["ww"]
            nbits = sum(bin(int(a)).count("1") for a in st["act"]) + sum(bin(int(b)).count("1") for b in st["bits"])
            assert nbits == q
        assert max(qs) == Mz and all(seen[k] for k in ("first", "last", "q1", "readd")), (Mz, seed, seen)
        assert seen["kds"] >= {k for k in R.BOUNDARY_DROPS if k < Mz - 1}, (Mz, seed, seen["kds"])
        added = {int(ids[arg]) for kind, arg in c["script"] if kind == 0}
        bits = {p - base for p in added if p >= base}
        assert any(p < base for p in added) and {31, 32} <= bits, (Mz, seed, sorted(added))
        if Mz >= 5:
            assert {63, 64} <= bits and 4 * (Mz - 1) in ids
        assert c["beta_margin"] <= 0.5, (Mz, seed, c["beta_margin"])


@pytest.mark.parametrize("maxm,Mz,full_ri", R.RUNS, ids=RUN_IDS)
def test_restatement_meets_its_own_invariants(maxm, Mz, full_ri):
    """The float64 restatement, handed to check_entry in the form the probe dumps, passes after every
    entry, and its residuals are a few Mz eps (|B R_A - I| scales with cond(R_A) <= 1e4)."""
    for seed in R.SEEDS:
        c = R.band_case(Mz, full_ri, seed)
        for e in range(len(c["script"])):
            R.check_entry(c, e, R.restated_entry(c, e))
        assert c["ref_worst"]["jj"] <= 64 * Mz * R.EPS and c["ref_worst"]["ra"] <= 64 * Mz * R.EPS, c["ref_worst"]
        assert c["ref_worst"]["b"] <= R.COND_CAP * 64 * Mz * R.EPS, c["ref_worst"]


def _first_rejected(case, ref_case):
    """The first entry at which check_entry, with ref_case's states and tolerances, rejects case's."""
    for e in range(len(case["script"])):
        try:
            R.check_entry(ref_case, e, R.restated_entry(case, e))
        except AssertionError as err:
            return e, err
    return None, None


@pytest.mark.parametrize("Mz,full_ri", [(5, 1), (17, 0), (46, 1)])
def test_negative_control_one_rotation_sign(Mz, full_ri):
    """One rotation applied to J with its sine negated: J J' stays H^-1, and check_entry rejects the
    state at the drop that holds that rotation, on J'N_A, and no earlier."""
    good = R.band_case(Mz, full_ri, 1)
    bad = R.band_case(Mz, full_ri, 1, flip=2)
    e, err = _first_rejected(bad, good)
    assert e is not None and good["script"][e][0] == 1 and "'ra'" in str(err), (e, err)
    assert all(np.array_equal(a["J"], b["J"]) for a, b in zip(good["states"][:e], bad["states"][:e]))
    assert bad["ref_worst"]["jj"] <= R.tolerance(good, "jj") and bad["ref_worst"]["ra"] > 1e6 * R.tolerance(good, "ra")


@pytest.mark.parametrize("Mz,full_ri", [(5, 1), (17, 0), (46, 1)])
def test_negative_control_one_row_of_b_one_slot_off(Mz, full_ri):
    """After one rotating drop the row of B that moved up is written one slot to the right: J is
    untouched, and check_entry rejects the state at that drop, on B R_A = I."""
    good = R.band_case(Mz, full_ri, 1)
    bad = R.band_case(Mz, full_ri, 1, slot=1)
    e, err = _first_rejected(bad, good)
    assert e is not None and good["script"][e][0] == 1 and "'b'" in str(err), (e, err)
    assert all(np.array_equal(a["J"], b["J"]) for a, b in zip(good["states"][:e + 1], bad["states"][:e + 1]))


def test_negative_control_poison_and_products():
    """check_entry rejects a NaN inside the active block of B, a nonzero stored subdiagonal, a product off
    by 1e-9 of the vector's largest entry, a nonzero product lane past q, and a bitmap bit in the wrong word."""
    c = R.band_case(17, 1, 1)
    e = next(k for k, s in enumerate(c["states"]) if s["q"] == 17)
    good = R.restated_entry(c, e)
    R.check_entry(c, e, good)

    def rejected(change):
        d = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in good.items()}
        change(d)
        with pytest.raises(AssertionError):
            R.check_entry(c, e, d)

    rejected(lambda d: d["B"].__setitem__(R.bt_idx(3, 9), np.nan))
    rejected(lambda d: d["B"].__setitem__(R.bt_idx(10, 9), 1e-300))
    rejected(lambda d: d["w"].__setitem__(4, d["w"][4] + 1e-9 * abs(d["w"]).max()))
    rejected(lambda d: d["lam"].__setitem__(0, d["lam"][0] + 1e-9 * abs(d["lam"]).max()))
    rejected(lambda d: d["w"].__setitem__(40, 1e-300))
    rejected(lambda d: d["bits"].__setitem__(slice(0, 2), d["bits"][:2][::-1].copy()) if d["bits"][0] != d["bits"][1]
             else d["bits"].__setitem__(0, d["bits"][0] ^ 1))
    rejected(lambda d: d.__setitem__("nrot", d["nrot"] + 1))
    rejected(lambda d: d["uw"].__setitem__(16, d["uw"][15]))


def test_prefix_reference():
    v = np.arange(1.0, 65.0)
    assert R.prefix_exact(v)[63] == 2080.0 and R.prefix_check(np.cumsum(v), v)
    bad = np.cumsum(v)
    bad[16] -= v[15]                          # the carry of row 0 dropped at the row boundary
    assert not R.prefix_check(bad, v)
    w = np.full(64, 0.1)
    assert R.prefix_check(np.cumsum(w), w) and not R.prefix_check(np.cumsum(w) * (1 + 16 * R.EPS), w)
