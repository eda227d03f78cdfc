"""GPU: gpc_prologue.h (the QR of W = [Q^1/2 G; Lambda^1/2] carrying V, the gain A = -R^-1 Q1'V and R^-1)
in every instance the tree uses, one call at a time through tests/device_units/libmpct_prologue_probe.so,
against tests/prologue_ref.py.  One launch per (instance, family), its cases as workgroups; the whole
dynamic LDS starts filled with a NaN sentinel and comes back whole.

Per case (prologue_ref.check_case, the function the CPU negative controls use; the bounds and the
derivation of g are in prologue_ref's docstring):
  * the flag is uniform over the lanes; every LDS word outside sR, sRi and the mapped sA entries still
    holds the sentinel, every word inside was written (RINV = false: the region passed as sRi untouched);
  * R is finite on and above its diagonal, which is positive (the strict lower triangle is not asserted);
  * in numpy.longdouble on what the device returned: |R'R - W'W|_ij <= g |W_:i| |W_:j|,
    |R'(R A) + W'V|_ij <= g (|W_:i| |V_:j| + (|R'||R||A|)_ij), |R Rinv - I| <= gamma_{M+1} |R||Rinv|;
  * against the mpmath truth: R column-wise within cond(W) g; A and Rinv within 8 x the larger of the
    restatement's own forward error and the derived bound (not in the stiff family); cond(W) from the truth.
Across cases, bitwise: R does not depend on nx or the pass count; an A column is the one its Phi column
gives alone in pass 0, and permuted Phi columns give permuted A columns; TABLES = true without tables, or
with this cell's offset -1, is the TABLES = false twin; the first-move rows are rows n Nu of the run that
stores every row; packed and full R^-1 carry the same bits; acol scatters to the mapped columns.
lambda = 0 on an input with an all-zero step response, and a NaN weight, return false with sA and sRi
untouched.  Measured maxima are recorded in DESIGN.md, not here."""
import ctypes as C
import os

import numpy as np
import pytest

import prologue_ref as P

pytestmark = pytest.mark.gpu

LIB = os.path.join(os.path.dirname(os.path.abspath(__file__)), "device_units", "libmpct_prologue_probe.so")
RUNS = [(name, inst) for name, f in P.FAMILIES.items() for inst in f["insts"]]
RATIOS = {}


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


def call(lib, inst, cases, launch=True, edit=None):
    """probe_prologue on one launch: (rc, [(lds, flags)] per case)."""
    hdr, dp, ip = P.pack_launch(inst, cases)
    if edit:
        edit(hdr, dp, ip)
    n = C.c_int(0)
    args = [C.c_int(inst), C.c_int(len(cases)), _p(hdr), _p(dp), C.c_longlong(dp.size), _p(ip), C.c_longlong(ip.size)]
    rc = lib.probe_prologue(*args, None, None, C.byref(n))
    if rc != 0 or not launch:
        return rc, n.value
    lds = P.sentinel_image(len(cases) * n.value).reshape(len(cases), n.value)
    lds[:] = 0.0
    flags = np.full((len(cases), 64), -9, np.int32)
    rc = lib.probe_prologue(*args, _p(lds), _p(flags), C.byref(n))
    return rc, [(lds[k], flags[k]) for k in range(len(cases))]


_DUMPS = {}


def dumps(lib, name, inst):
    """The launch of (family, instance), once per module: {key: (lds, flags)}."""
    if (name, inst) not in _DUMPS:
        cases = P.family_cases(name, inst)
        rc, out = call(lib, inst, cases)
        assert rc == 0, (name, inst, rc)
        _DUMPS[name, inst] = {c["key"]: o for c, o in zip(cases, out)}
    return _DUMPS[name, inst]


def parsed(lib, name, inst, key):
    return P.parse_image(P.CASES[key], inst, *dumps(lib, name, inst)[key])


def upper(R):
    return R[np.triu_indices(R.shape[0])]


@pytest.mark.parametrize("name,inst", RUNS, ids=["%s-%d" % r for r in RUNS])
def test_prologue_against_the_reference(probe, name, inst, capsys):
    out = dumps(probe, name, inst)
    tag = P.INSTANCES[inst]["name"] + ("/stiff" if name == "stiff" else "")
    ratios = RATIOS.setdefault(tag, {})
    for c in P.family_cases(name, inst):
        P.check_case(c, inst, *out[c["key"]], ratios)
    with capsys.disabled():
        print("\n  %s ratios to the bounds so far:" % tag, {n: float("%.3g" % v) for n, v in sorted(ratios.items())})


def test_r_does_not_depend_on_nx_or_the_pass_count(probe):
    for name, inst, base, others in (("pass16", 0, "pass16/0", ["pass16/nx47", "pass16/nx48", "pass16/nx49", "pass16/col48"]),
                                     ("stream32", 1, "stream32/0", ["stream32/nx31", "stream32/nx32", "stream32/nx33"]),
                                     ("stream64", 2, "stream64/0", ["stream64/nx1", "stream64/nx2", "stream64/nx3"]),
                                     ("stream64", 2, "stream64/1", ["stream64/b_nx30", "stream64/b_nx31"])):
        ref = parsed(probe, name, inst, base)
        for k in others:
            got = parsed(probe, name, inst, k)
            assert P.same_bits(upper(got["R"]), upper(ref["R"])), k
            assert P.same_bits(got["Rinv"], ref["Rinv"]), k
            nx = P.CASES[k]["nx"]
            if "col" not in k:
                assert P.same_bits(got["A"], ref["A"][:, :nx]), k      # the same Phi columns, other passes


def test_a_columns_do_not_depend_on_their_pass(probe):
    ref = parsed(probe, "pass16", 0, "pass16/nx49")
    perm = P.CASES["pass16/perm"]["perm"]
    assert P.same_bits(parsed(probe, "pass16", 0, "pass16/perm")["A"], ref["A"][:, perm])
    assert sorted(perm.tolist()) == list(range(49)) and (perm[:48] >= 48).any()    # a column changed pass
    for j in (0, 47, 48):
        got = parsed(probe, "pass16", 0, "pass16/col%d" % j)
        assert P.same_bits(got["A"][:, 0], ref["A"][:, j]), j


def test_tables_absent_or_cell_missing_is_the_twin(probe):
    cases = P.family_cases("tables", 3)
    twin = dumps(probe, "tables", 4)
    rc, none = call(probe, 3, [dict(c, qrt=None, qoff=None) for c in cases])
    assert rc == 0
    rc, hole = call(probe, 3, [P.with_tables(c, cell=np.zeros(0), hole=True) for c in cases])
    assert rc == 0
    used = dumps(probe, "tables", 3)
    for c, a, b in zip(cases, none, hole):
        assert P.same_bits(a[0], twin[c["key"]][0]) and np.array_equal(a[1], twin[c["key"]][1]), c["key"]
        assert P.same_bits(b[0], twin[c["key"]][0]) and np.array_equal(b[1], twin[c["key"]][1]), c["key"]
        if c["M"] > 1:
            assert not P.same_bits(used[c["key"]][0], twin[c["key"]][0]), c["key"]     # the tables were read


def test_first_move_rows_are_rows_of_the_full_gain(probe):
    for name, first, full in (("first16", 5, 7), ("first32", 6, 8)):
        for c in P.family_cases(name, first):
            a, b = parsed(probe, name, first, c["key"]), parsed(probe, name, full, c["key"])
            rows = np.arange(0, c["M"], c["Nu"])
            assert P.same_bits(a["A"][rows], b["A"][rows]) and P.same_bits(upper(a["R"]), upper(b["R"])), c["key"]
            assert np.isnan(a["A"][np.setdiff1d(np.arange(c["M"]), rows)]).all()


def test_packed_and_full_rinv_carry_the_same_bits(probe):
    for name in ("stream16", "tables"):
        for c in P.family_cases(name, 4):
            a, b = parsed(probe, name, 4, c["key"]), parsed(probe, name, 9, c["key"])
            assert P.same_bits(a["Rinv"], b["Rinv"]) and P.same_bits(upper(a["R"]), upper(b["R"])), c["key"]
            assert P.same_bits(a["A"], b["A"]), c["key"]


def test_acol_scatters_to_the_mapped_columns(probe):
    """The same case with the identity map: the same A bits, found at the mapped columns."""
    cases = P.family_cases("tables", 3)
    rc, out = call(probe, 3, [dict(c, acol=None) for c in cases])
    assert rc == 0
    for c, o in zip(cases, out):
        ident = P.parse_image(dict(c, acol=None), 3, *o)
        assert (c["acol"] != np.arange(c["nx"])).any()
        assert P.same_bits(ident["A"], parsed(probe, "tables", 3, c["key"])["A"]), c["key"]


def test_probe_refuses_what_does_not_fit(probe):
    """Arguments are validated on the host before any launch: hipErrorInvalidValue (1), no kernel run."""
    c = P.CASES["tables/1"]
    H = {k: i for i, k in enumerate(P.HDR)}
    assert call(probe, 3, [c], launch=False)[0] == 0

    def refused(inst=3, case=c, **fields):
        def edit(hdr, dp, ip):
            for k, v in fields.items():
                hdr[0, H[k]] = v
        return call(probe, inst, [case], launch=False, edit=edit)[0] == 1

    assert refused(M=64, Nu=64 // c["nu"]) and refused(M=63, Nu=21)          # M >= 64; M > MAXM
    assert refused(inst=1, case=P.CASES["stream64/1"])                       # M = 33 > MAXM = 32
    assert refused(my=17) and refused(nu=2) and refused(N2=c["N2"] + 1) and refused(inst=10)
    assert refused(case=dict(c, acol=np.where(np.arange(c["nx"]) == 2, c["astride"], c["acol"]).astype(np.int32)))
    assert refused(case=dict(c, acol=None, astride=c["nx"] - 1))
    assert refused(qrt_len=c["qrt"].size - 1)                                # the cell runs past the table
    assert refused(case=dict(c, qoff=np.where(c["qoff"] == c["qoff"].max(), c["qoff"].max() + 1, c["qoff"]).astype(np.int32)))
    assert refused(tlen=c["step"].shape[2] - 2)                              # a step index past the table
    assert refused(case=dict(c, n1=np.array([0, -1], np.int32)))
    assert refused(step_off=-1) and refused(phi_off=1 << 30)
    big = P.make_case("big", 1, 1, 63, 63, 250, seed=1, astride=256)         # 24 k doubles: over the LDS a block gets
    rc, n = call(probe, 2, [big], launch=False)
    assert rc == 0 and n * 8 > 160 * 1024
    assert call(probe, 2, [big])[0] == 1


# ---------------------------------------------------------------------------------------------
# the production case
CELLS = ((30, 5), (13, 1), (4, 4), (1, 1))


@pytest.fixture(scope="module")
def shell(gpu):
    from mpct.scenarios import candidate_grid, shell3x3

    sc = shell3x3(n2_max=30, nu_max=5)[0]
    d = sc.dims()
    my, nu, nx, tlen = d["my"], d["nu"], d["nx"], d["tlen"]
    step = sc.table(0).reshape(my, nu, tlen)
    phid = sc.table(3).reshape(my, 30, nx)
    qrt = sc.table(4)
    off, total = P.cell_offsets(my, nu, nx, 30, 5)
    assert qrt.size == total == 151440
    _, _, dl, lm = candidate_grid(4096)
    corners = [(dl.min(axis=0), lm.max(axis=0)), (dl.max(axis=0), lm.min(axis=0))]
    cases = []
    for N2, Nu in CELLS:
        for k, (delta, lam) in enumerate(corners):
            cases.append(dict(key="shell/%d-%d-%d" % (N2, Nu, k), my=my, nu=nu, Nu=Nu, N2=N2, M=nu * Nu, nx=nx, wsq=0,
                              n2max=30, numax=5, n1=np.asarray(sc.n1, np.int32), step=step, phi=phid,
                              delta=np.asarray(delta, float), lam=np.asarray(lam, float), astride=36,
                              acol=np.random.default_rng(5).permutation(36)[:nx].astype(np.int32), qrt=qrt, qoff=off,
                              table_stage=min(N2, nu * Nu) * P.gamma_ref(N2), expect_ok=True))
    return cases


def test_shell3x3_rows_as_the_host_built_them(probe, shell, capsys):
    """Shell 3x3 (n2_max 30, nu_max 5) at cells (30, 5), (13, 1), (4, 4), (1, 1) and the grid's two extreme
    weight corners: the small instance reading the library's own rows, and <16> streaming, against mpmath."""
    worst = {}
    for inst in (3, 0):
        rc, out = call(probe, inst, shell)
        assert rc == 0
        for c, o in zip(shell, out):
            P.check_case(c, inst, *o, RATIOS.setdefault(P.INSTANCES[inst]["name"] + "/shell", {}))
            got, tr = P.parse_image(c, inst, *o), P.truth_of(c)
            w = worst.setdefault(inst, dict(R=0.0, A=0.0, Rinv=0.0, cond=0.0))
            for k in ("R", "A", "Rinv"):
                ref = np.triu(tr[k]) if k != "A" else tr[k]
                dev = np.triu(got[k]) if k != "A" else got[k]
                w[k] = max(w[k], float(np.abs(np.asarray(dev, P.LD) - ref).max() / np.abs(ref).max()))
            w["cond"] = max(w["cond"], tr["cond"])
    with capsys.disabled():
        print("\n  Shell 3x3 forward errors (max |dev - truth| / max |truth|):",
              {P.INSTANCES[k]["name"]: {n: float("%.3g" % v) for n, v in w.items()} for k, w in worst.items()})
