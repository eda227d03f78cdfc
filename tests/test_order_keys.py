"""CPU side of the dispatch-order key tests (tests/test_order_keys_gpu.py): the probe library is built
and separate, every batch reaches the path it is named for (from the header constants and the
scenario's dims alone), the reference's rounding windows meet the cap of the comparison rule
(tests/order_key_ref.py: at most 2 % two-integer windows, none wider, kappa_2(H) <= 1e6, float64 against
longdouble below 1/4 of the window), perturbed references fail the comparison (negative controls), and
gram_tables on the host equals the reference's G'G and G'1."""
import os
import subprocess

import numpy as np
import pytest

import host_program
import order_key_ref as R

GPC_BATCHES = [n for n, b in R.BATCHES.items() if n != "costly"]


def _exports(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], check=True, capture_output=True, text=True).stdout
    return {ln.split()[-1] for ln in out.splitlines() if ln.strip()}


def test_order_probe_library_is_built_and_separate(built):
    import __graft_entry__ as g

    assert g.ORDER_PROBE_LIB == R.PROBE_LIB and os.path.exists(R.PROBE_LIB)
    assert "probe_order" in _exports(R.PROBE_LIB)
    assert not [e for e in _exports(os.path.join(g.CSRC, "libmpct.so")) if e.startswith("probe_")]
    src = open(g.ORDER_PROBE_SRC).read()
    inc = [ln.split('"')[1] for ln in src.splitlines() if ln.startswith('#include "')]
    assert inc == ["scenario_tables.h", "work_order.hip"], inc      # both as they are: no copy, no patch


def test_header_constants():
    k = R.constants()
    assert k["kOrderMinC"] == 256 and k["kWave"] == 64 and k["kGramM"] == 16 and k["kCountRankMaxC"] == 8192
    assert all(c >= k["kOrderMinC"] for c in [b.C for b in R.BATCHES.values()])
    assert min(R.LARGE_C) < k["kCountRankMaxC"] < max(R.LARGE_C) and k["kCountRankMaxC"] in R.LARGE_C


def test_batches_reach_their_paths(built):
    k = R.constants()
    for name, b in R.BATCHES.items():
        p = b.plant
        N2, Nu, delta, lam = b.candidates()
        assert b.C in (256, 257) and len(N2) == b.C and b.r.shape[2] <= 160 or b.refs == "long", name
        assert R.scenario_path(p) == ("ratio:cost" if name == "costly" else "gpc"), name
        paths = R.candidate_paths(p, N2, Nu, b.tables)
        for path, least in b.needs:
            assert int((paths == path).sum()) >= least, (name, path, int((paths == path).sum()))
        # the mix every batch carries
        ok = R.valid_horizons(p, N2, Nu)
        assert (ok & (Nu == 1)).any() and (ok & (Nu == N2) & (Nu > 1)).any() and (ok & (Nu == p.numax)).any(), name
        assert (N2 <= 0).any() and (N2 > p.n2max).any() and (Nu < 1).any() and (Nu > p.numax).any() and \
            ((Nu > N2) & (Nu <= p.numax) & (N2 > 0)).any(), name
        rows = [tuple(r) for r in np.column_stack([N2, Nu, delta, lam])]
        assert len(set(rows)) <= b.C - 20, name                                 # exact duplicates: ties
        assert (delta < 0).any() and (lam < 0).any(), name
        zero = np.flatnonzero(ok & np.all(delta == 0, axis=1) & np.all(lam == 0, axis=1))
        assert zero.size == 1, name
        if name != "costly":
            ref = b.reference()
            assert ref.fixed[zero[0]] and (~ref.key[zero[0]] & R.FIELD_MAX) == R.FIELD_MAX, name   # H = 0: not SPD
            assert ((~ref.fixed).sum() == 0) == (b.refs == "const"), name         # no jump: every field is 0
        assert (b.free_mv is not None) == (not np.all(np.isfinite(p.bnd))), name
    B = R.BATCHES
    # the Gram tables exist exactly for my <= 4 (all of these are far below kGramMaxBytes)
    for name, b in B.items():
        assert R.has_gram(b.plant) == (b.plant.my <= 4), name
        assert b.plant.n2max * b.plant.numax * b.plant.my * k["kGramOut"] * 8 <= k["kGramMaxBytes"]
    assert B["shell-steps"].plant.my == 3 and B["4x3"].plant.my == 4 and B["many-steps"].plant.my == 5
    # M = 16 exactly with nu = 1; my M = 64 exactly on the lanes path; M = 24 and M = 33, 34 one lane per output
    N2, Nu, _, _ = B["siso"].candidates()
    assert B["siso"].plant.nu == 1 and (R.valid_horizons(B["siso"].plant, N2, Nu) & (Nu == 16)).sum() >= 5
    for name, nuc, path in (("deep-steps", 16, "chol_lanes"), ("deep-steps", 17, "chol_serial"),
                            ("shell-steps", 8, "chol_serial"), ("lds_path", 11, "chol_serial"),
                            ("wide60", 15, "chol_serial")):
        p = B[name].plant
        N2, Nu, _, _ = B[name].candidates()
        sel = R.valid_horizons(p, N2, Nu) & (Nu == nuc)
        assert sel.sum() >= 5 and set(R.candidate_paths(p, N2, Nu)[sel]) == {path}, (name, nuc)
    assert B["deep-steps"].plant.my * B["deep-steps"].plant.nu * 16 == k["kWave"]
    assert B["wide60"].plant.nu * 15 == 60
    # how the jumps are collected
    for scen, my in (("shell", 3), ("deep", 2), ("many", 5)):
        want = "pass" if my > 4 else "block"
        assert R.jump_paths(my, B[scen + "-steps"].r) == {want} and R.jump_paths(my, B[scen + "-vns3"].r) == {want}
        assert B[scen + "-vns3"].r.shape[0] == 3
        assert R.jump_paths(my, B[scen + "-every"].r) == {"pass"} and len(R.jumps(B[scen + "-every"].r)) == 149
        assert R.jump_paths(my, B[scen + "-const"].r) == {"none"}
        r = B[scen + "-long"].r
        assert r.shape[2] == 600 and R.jump_paths(my, r) == {want}
        assert list(np.flatnonzero(np.any(np.diff(r[0], axis=1) != 0, axis=0)) + 1) == list(R.LONG_JUMPS)
        assert max(R.LONG_JUMPS) == 599 and {512, 513} <= set(R.LONG_JUMPS)     # both 512-step blocks


def test_the_library_admits_no_qp_of_64_rows(built):
    """M = 64 and Mp > 64 cannot be reached through a descriptor: build_scenario wants nu nu_max < 64.
    wide60 (M = 60) is the largest H, and the fall-back to order_keys is reached by its cost bound."""
    from mpct.engine import MpctError

    for nu_max in (16, 17):
        with pytest.raises(MpctError, match="nu\\*nu_max"):
            R._family("many_entries", n2_max=17, nu_max=nu_max)
    p = R.BATCHES["costly"].plant
    assert p.nu * p.numax <= 64 and R.key_lds_bytes(p) <= 64 * 1024
    assert 0.5 * (p.nu * p.numax) ** 2 * p.my * p.n2max > R.constants()["kOrderEstMaxCost"]


@pytest.mark.parametrize("name", list(R.BATCHES))
def test_windows_meet_the_cap(built, name):
    ref = R.BATCHES[name].reference()
    share, widest = ref.two()
    print(name, "two-integer windows %.4f, widest %d, kappa max %s" % (share, widest, np.nanmax(ref.kappa)
                                                                         if np.isfinite(ref.kappa).any() else None))
    assert share <= R.CAP_TWO and widest <= 1
    assert not (ref.kappa > R.KAPPA_MAX).any()
    assert not R.compare(ref.key, ref).any()          # the reference passes its own rule


@pytest.mark.parametrize("kind", (R.K_GPC, R.K_NMPC))
def test_windows_of_the_ratio_key_meet_the_cap(kind):
    for my, nu in ((3, 3), (2, 1), (1, 2)):
        cand = R.null_candidates(my, nu, C=256 + (my & 1), seed=70 + my)
        ref = R.ratio_reference(kind, my, nu, *cand)
        share, widest = ref.two()
        assert share <= R.CAP_TWO and widest <= 1
        N2, Nu, delta, lam = cand
        assert (Nu == 64).any() and (Nu == 65).any() and np.all(lam == 0, axis=1).any() and np.all(delta == 0, axis=1).any()
        assert ref.key[np.flatnonzero(Nu == 65)[0]] == R.INVALID and ref.key[np.flatnonzero(Nu == 64)[0]] != R.INVALID
        if kind == R.K_GPC:
            f = ~ref.key & R.FIELD_MAX
            assert f[7] == R.FIELD_MAX and f[9] == 0      # lambda = 0 and delta = 0 clamp at the ends


def test_float64_against_longdouble(built):
    worst = 0.0
    for name in GPC_BATCHES:
        b = R.BATCHES[name]
        r64, rld = b.reference(), b.reference(dtype=np.longdouble)
        assert np.array_equal(r64.fixed, rld.fixed), name
        m = ~r64.fixed
        if m.any():
            worst = max(worst, float(np.max(np.abs(r64.x[m].astype(np.longdouble) - rld.x[m]) / r64.dx[m])))
    print("largest |x_64 - x_ld| / dx: %.3f" % worst)
    assert worst < R.LD_RATIO_MAX


@pytest.mark.parametrize("variant", R.NEGATIVE_CONTROLS)
def test_negative_controls_fail_the_comparison(built, variant):
    """A reference with one planted mistake, passed through compare() as if it were the device, must
    disagree with the true reference on at least half of the valid candidates of the Shell 3x3 batch (the
    one without squared weights, where q_unsquared differs)."""
    b = R.BATCHES["shell-wsq0"]
    true, wrong = b.reference(), b.reference(variant=variant)
    bad = R.compare(wrong.key, true)
    print(variant, int(bad.sum()), "of", int(true.valid.sum()))
    assert not bad[~true.valid].any()
    assert bad[true.valid].sum() >= 0.5 * true.valid.sum()


# ------------------------------------------------------------------------------------------------
# gram_tables on the host
GRAM_BLOCKS = {"shell": ((30, 5), (5, 5), (17, 2)), "gpc_window": ((16, 8), (5, 5), (12, 3))}


@pytest.fixture(scope="module")
def gram_program(tmp_path_factory):
    return host_program.build("gram_tables_check", tmp_path_factory.mktemp("gram_tables"))


def _gram_run(exe, scen, blocks):
    sc = R.scenario(scen)
    text = R.descriptor_text(sc) + "%d\n" % len(blocks) + "".join("%d %d\n" % b for b in blocks)
    out = host_program.run(exe, stdin=text)
    fields = dict(ln.split("=") for ln in out.splitlines() if "=" in ln)
    rows = {}
    for ln in out.splitlines():
        if ln.startswith("block "):
            t = ln.split()
            rows[(int(t[1]), int(t[2]), int(t[3]))] = np.array([float(x) for x in t[4:]])
    return sc, int(fields["gram_doubles"]), int(fields["nonzero_uncovered"]), rows


@pytest.mark.parametrize("scen", list(GRAM_BLOCKS))
def test_gram_tables_on_the_host(built, gram_program, scen):
    """G_o'G_o and G_o'1 of three (N2, Nu) blocks against the reference's G in longdouble, to 1e-13
    relative.  Every entry is a sum of at most N2 <= 127 terms of one sign (the step responses of these
    two plants are non-negative, asserted), accumulated in sequence in float64: each product rounds once
    and each of the n - 1 additions once, so the relative error is at most n eps = 127 * 2.2e-16 = 2.8e-14."""
    k = R.constants()
    sc, size, uncovered, rows = _gram_run(gram_program, scen, GRAM_BLOCKS[scen])
    p = R.plant_of(sc)
    assert (scen == "gpc_window") == bool((p.n1 > 1).all()) and p.n2max <= 127 and np.all(p.step >= 0.0)
    assert size == p.n2max * p.numax * p.my * k["kGramOut"]
    assert p.nu * p.numax > k["kGramM"] and uncovered == 0      # the blocks with nu Nu > 16 stay zero
    Ms = set()
    for N2, Nu in GRAM_BLOCKS[scen]:
        M = p.nu * Nu
        Ms.add((M, Nu == N2))
        nonzero = 0
        for o in range(p.my):
            got = rows[(N2, Nu, o)]
            G = R.forced_response(p, o, N2, Nu, dtype=np.longdouble)
            want = np.zeros((k["kGramM"] + 1, k["kGramM"]), dtype=np.longdouble)
            want[:M, :M] = G.T @ G
            want[k["kGramM"], :M] = G.sum(axis=0)
            want = want.ravel()
            err = np.abs(got.astype(np.longdouble) - want)
            assert np.all(err <= 1e-13 * np.abs(want)), (scen, N2, Nu, o, float(err.max()))
            nonzero += int(np.count_nonzero(want))
        assert nonzero >= M      # within the delays an output's G is zero; not all of the block is
    assert any(eq for _, eq in Ms)
    if scen == "gpc_window":
        assert any(M == k["kGramM"] for M, _ in Ms)


def test_no_gram_table_for_more_than_four_outputs(built, gram_program):
    sc, size, _, _ = _gram_run(gram_program, "many_entries", ())
    assert sc.my == 5 and size == 0
