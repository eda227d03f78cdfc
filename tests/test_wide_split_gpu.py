"""GPU: the wide split of an ordered metric launch (launch_closed_loop).  The first H ordered
slots run on gpc_small_wide_kernel, the rest on gpc_small_kernel on an auxiliary stream; both instances
are one body and must give, bit for bit, what the single launch gives.

Every case scores one batch with the split forced to H slots (MPCT_WIDE_SLOTS=H when the scenario is
created) and compares every requested field with the same call on a scenario created with
MPCT_WIDE_SLOTS=0, the single launch.  The calls go through tests/record_calls.py: canary-filled buffers
with guards on both sides, every row written, no status NOT_RUN.  nit = 60 steps keep a case well under a
second; the candidates are slices of the Shell 3x3 metric grid (candidate_grid), whose weights drive the
loop into its MV bounds within the first setpoint jump (QP iterations are asserted non-zero)."""
import os

import numpy as np
import pytest

import record_calls as rc
from record_calls import COST, bits

pytestmark = pytest.mark.gpu

NIT = rc.NIT


@pytest.fixture(scope="module")
def gpu(built, has_gpu):
    if not has_gpu:
        pytest.skip("no GPU")
    return True


_scen, _ref = {}, {}


def scen(kind, n):
    """Scenario `kind` created with MPCT_WIDE_SLOTS=n (the option is read at creation)."""
    from mpct.scenarios import shell3x3, shell3x3_mc

    if (kind, n) not in _scen:
        old = os.environ.get("MPCT_WIDE_SLOTS")
        os.environ["MPCT_WIDE_SLOTS"] = str(n)
        try:
            if kind == "mc3":
                sc, refs, _ = shell3x3_mc(draws=3, n2_max=30, nu_max=5, nit=NIT)
            else:
                sc, r, _ = shell3x3(n2_max=30, nu_max=6 if kind == "nu6" else 5, nit=NIT)
                refs = r[None]
        finally:
            if old is None:
                del os.environ["MPCT_WIDE_SLOTS"]
            else:
                os.environ["MPCT_WIDE_SLOTS"] = old
        _scen[(kind, n)] = (sc, np.ascontiguousarray(refs))
    return _scen[(kind, n)]


def grid(C):
    """C candidates spread over the 4096 metric grid (every 15th, so light and heavy ones)."""
    from mpct.scenarios import candidate_grid

    N2, Nu, d, l = candidate_grid(4096)
    idx = (np.arange(C) * 15) % 4096
    return [np.ascontiguousarray(a[idx]) for a in (N2, Nu, d, l)]


def mixed300():
    """300 candidates over the horizon cells (30,5), (13,1), (4,4), (1,1), one skipped (N2 = 0) and one
    bad-horizon (Nu > N2) candidate; invalid candidates are ordered last (slots 298, 299)."""
    N2, Nu, d, l = grid(300)
    cells = np.array([(30, 5), (13, 1), (4, 4), (1, 1)], dtype=np.int32)
    N2[:], Nu[:] = cells[np.arange(300) % 4, 0], cells[np.arange(300) % 4, 1]
    N2[41], Nu[41] = 0, 3
    N2[177], Nu[177] = 3, 5
    return [N2, Nu, d, l]


def nu6():
    N2, Nu, d, l = grid(257)
    Nu[:] = np.where(np.arange(257) % 3 == 0, 6, 5)
    return [N2, Nu, d, l]


CASES = {"c257": ("shell5", grid, 257), "mixed300": ("shell5", mixed300, None), "mc3": ("mc3", grid, 257),
         "nu6": ("nu6", nu6, None)}


def run(case, n, fields=COST):
    kind, make, C = CASES[case]
    sc, refs = scen(kind, n)
    return rc.call("device", sc, make(C) if C else make(), refs, fields=fields)


def reference(case):
    """The single launch (split off), all six fields, computed once per case."""
    if case not in _ref:
        _ref[case] = run(case, 0)
    return _ref[case]


def same(got, ref, fields):
    for f in fields:
        assert np.array_equal(bits(got[f]), bits(ref[f])), "%s differs in %d rows" % (
            f, int(np.any(bits(got[f]) != bits(ref[f]), axis=1).sum()))


def test_instances(gpu):
    from mpct.engine import kernel_instance

    assert kernel_instance(scen("shell5", 37)[0]) == "gpc_small_kernel"
    assert kernel_instance(scen("nu6", 37)[0]) == "gpc_small_kernel + gpc_closed_loop_kernel<32,false,false>"


@pytest.mark.parametrize("H", [1, 37, 256, 257])
def test_c257(gpu, H):
    ref = reference("c257")
    assert ref["qp_iters"].max() > 0   # constrained loops
    same(run("c257", H), ref, COST)


@pytest.mark.parametrize("H", [150, 298, 299, 300])
def test_mixed_horizons_and_invalid_candidates(gpu, H):
    """The skipped and the bad-horizon candidate sit in the last two ordered slots: both outside the
    wide range at H = 150 and 298, one on each side at 299, both inside at 300.  Their status has
    exactly one writer each time (a missing one leaves NOT_RUN, which record_calls refuses)."""
    ref = reference("mixed300")
    assert ref["status"][41, 0] == 8 and ref["status"][177, 0] == 16
    assert not np.any(np.delete(ref["status"][:, 0], [41, 177]) & (8 | 16))
    same(run("mixed300", H), ref, COST)


@pytest.mark.parametrize("H", [100, 257, 770])
def test_three_reference_sets(gpu, H):
    """nref = 3 plant variants, S = 771 slots, H no multiple of 3: a candidate's three simulations fall
    on both sides of the boundary, and slot -> (candidate, reference) must hold across it."""
    ref = reference("mc3")
    assert ref["J1"].shape == (771, 3)
    # the variants differ, so a wrong reference index would show
    assert not np.array_equal(ref["J1"][0::3], ref["J1"][1::3])
    same(run("mc3", H), ref, COST)


@pytest.mark.parametrize("H", [37, 171])
def test_three_concurrent_launches(gpu, H):
    """nu_max = 6: Nu = 6 (M = 18) runs on the general kernel's <32> class beside the wide and the thin
    launch of the Nu = 5 candidates (171 of 257)."""
    ref = reference("nu6")
    same(run("nu6", H), ref, COST)


@pytest.mark.parametrize("fields", [("J1",), COST], ids=["J1", "all"])
def test_field_subsets(gpu, fields):
    same(run("c257", 37, fields), reference("c257"), fields)


def test_rule_is_the_default(gpu):
    """Without the option the rule decides (C = 257: every slot wide): the same records."""
    same(run("c257", -1), reference("c257"), COST)
