"""Plant variants on the small-plant GPC kernel, without a GPU: which kernel instance a Shell 3x3
model-error scenario (mpct.scenarios.shell3x3_mc) reports, the draws themselves, the metric
kernel's register budget, and the host lane tables under the sanitizers
(tests/host_tables/small_variants_check.cpp)."""
import os
import re

import numpy as np
import pytest

import host_program

NIT = 200


def test_instance_names(built):
    """A GPC-mode scenario with plant variants that is otherwise small runs the small kernel for
    cost-only batches, alone or (nu * nu_max > 16) with the general kernel's wider class; with
    trajectories it runs what the single-plant scenario runs."""
    from mpct.engine import kernel_instance, robust_instance
    from mpct.scenarios import shell3x3, shell3x3_mc

    sc = shell3x3_mc(draws=4, nit=NIT)[0]
    assert sc.nplant == 4
    assert kernel_instance(sc) == "gpc_small_kernel"
    assert robust_instance(sc) == "gpc_small_kernel + robust_reduce_kernel"
    sc6 = shell3x3_mc(draws=4, nu_max=6, nit=NIT)[0]
    assert kernel_instance(sc6) == "gpc_small_kernel + gpc_closed_loop_kernel<32,false,false>"
    one = shell3x3(nit=NIT)[0]
    assert kernel_instance(sc, want_traj=True) == kernel_instance(one, want_traj=True)
    assert kernel_instance(sc, open_loop=True, want_traj=True) == kernel_instance(one, open_loop=True, want_traj=True)
    assert kernel_instance(sc) == kernel_instance(one)


def _mc_with(plants, nit=NIT):
    from mpct.engine import Scenario
    from mpct.scenarios import SHELL3_L as L, SHELL3_R as R, SHELL3_TS, shell3x3_plant, shell3x3_xsp, shell3x3_yref

    P = shell3x3_plant()
    yref = L[:, None] * shell3x3_yref(shell3x3_xsp(nit))
    return Scenario(plants[0], P, nu=3, du_min=-0.05 / R, du_max=0.05 / R, u_min=-1.0 / R, u_max=0.5 / R,
                    yref=yref, n2_max=30, nu_max=5, Ts=SHELL3_TS, plant_variants=plants)


def test_ineligible_variant_falls_back(built):
    """One entry of one variant beyond 4 plant terms (three numerator taps, two denominator taps):
    the whole scenario runs the general kernel.  The delay limit: an entry whose taps end exactly at
    the input ring's length (16) is still small; one sample more cannot fall back, because the
    general kernel's history rings have the same length and the library refuses the scenario."""
    from mpct.engine import MpctError, kernel_instance
    from mpct.lti import Tf
    from mpct.scenarios import shell3x3_mc_plants

    plants = shell3x3_mc_plants(3)
    assert kernel_instance(_mc_with(plants)) == "gpc_small_kernel"
    t = plants[1][0][0]
    a = t.den[1]
    fat = [[e for e in row] for row in plants[1]]
    fat[0][0] = Tf.make([t.num[1], 0.5 * t.num[1], 0.25 * t.num[1]], [1.0, a - 0.5, -0.5 * a], t.delay)
    assert kernel_instance(_mc_with([plants[0], fat, plants[2]])) == "gpc_closed_loop_kernel<16,false,false>"
    # four terms (the first numerator tap zero) are still small
    fat[0][0] = Tf.make([0.0, t.num[1], 0.25 * t.num[1]], [1.0, a - 0.5, -0.5 * a], t.delay)
    assert kernel_instance(_mc_with([plants[0], fat, plants[2]])) == "gpc_small_kernel"
    late = [[e for e in row] for row in plants[2]]
    late[1][1] = Tf(late[1][1].num, late[1][1].den, 16 - len(late[1][1].num))
    assert kernel_instance(_mc_with([plants[0], plants[1], late])) == "gpc_small_kernel"
    late[1][1] = Tf(late[1][1].num, late[1][1].den, 17 - len(late[1][1].num))
    with pytest.raises(MpctError, match="history rings"):
        _mc_with([plants[0], plants[1], late])


def test_shell3x3_mc_plants():
    from mpct.scenarios import (SHELL3_DK, SHELL3_K, SHELL3_L as L, SHELL3_R as R, shell3x3_mc_plants,
                                shell3x3_plant)

    e_max = np.array([0.2, 0.2, 0.3])
    A = shell3x3_mc_plants(6)
    # draw 0: Shell3x3.m:38, 43-45
    assert SHELL3_DK.tolist() == [[2.11, 0.39, 0.59], [3.29, 0.57, 0.89], [3.11, 0.73, 1.33]]
    want = L[:, None] * R[None, :] * (SHELL3_K + SHELL3_DK * e_max[None, :])
    got = np.array([[A[0][i][j].dcgain for j in range(3)] for i in range(3)])
    assert np.max(np.abs(got - want)) <= 1e-14, np.max(np.abs(got - want))
    # e = 0 is the nominal plant, exactly
    assert shell3x3_mc_plants(3, e_max=0.0) == [shell3x3_plant()] * 3
    # the same seed, the same plants; another seed, other plants after draw 0
    assert shell3x3_mc_plants(6) == A
    B = shell3x3_mc_plants(6, seed=1)
    assert B[0] == A[0] and B[1] != A[1]
    # draws k >= 1 lie within the error box and move whole columns
    nominal = L[:, None] * R[None, :] * SHELL3_K
    for P in A[1:]:
        g = np.array([[P[i][j].dcgain for j in range(3)] for i in range(3)])
        e = (g - nominal) / (L[:, None] * R[None, :] * SHELL3_DK)
        assert np.all(np.abs(e) <= e_max[None, :] + 1e-12)
        assert np.max(np.abs(e - e[0][None, :])) < 1e-12
    # delay shifts leave the gains alone and change the delays only
    D = shell3x3_mc_plants(6, max_dshift=2)
    shift = np.zeros((6, 3, 3), dtype=int)
    for k in range(6):
        for i in range(3):
            for j in range(3):
                assert D[k][i][j].num == A[k][i][j].num and D[k][i][j].den == A[k][i][j].den
                shift[k, i, j] = D[k][i][j].delay - A[k][i][j].delay
    assert np.all(shift[0] == 0) and shift.min() == 0 and shift.max() == 2


def test_shell3x3_mc_scenario(built):
    from mpct.scenarios import shell3x3, shell3x3_mc, shell3x3_plant

    sc, refs, plants = shell3x3_mc(draws=3, nit=NIT)
    one, r, yref = shell3x3(nit=NIT)
    assert refs.shape == (3, 3, NIT) and all(np.array_equal(refs[k], r) for k in range(3))
    assert np.array_equal(sc.yref, one.yref) and sc.model == shell3x3_plant() and len(plants) == 3
    assert all(np.array_equal(a, b) for a, b in zip(sc.bounds, one.bounds))
    assert sc.dims() == one.dims()


def test_small_kernel_listing_budget(built):
    """The metric kernel still fits four waves per SIMD: at most 128 VGPRs, no private segment."""
    import __graft_entry__ as g

    path = [p for p in g.kernel_isa(force=True) if os.path.basename(p) == "gpc_small.gfx950.s"][0]
    text = open(path).read()
    blocks = [m.group(2) for m in re.finditer(r"\.amdhsa_kernel (\S+)(.*?)\.end_amdhsa_kernel", text, flags=re.S)
              if "gpc_small_kernel" in m.group(1)]
    assert len(blocks) == 1
    vgpr = int(re.search(r"\.amdhsa_next_free_vgpr (\d+)", blocks[0]).group(1))
    scratch = int(re.search(r"\.amdhsa_private_segment_fixed_size (\d+)", blocks[0]).group(1))
    print("gpc_small_kernel: next_free_vgpr %d, private segment %d" % (vgpr, scratch))
    assert vgpr <= 128 and scratch == 0


def test_small_variant_tables_under_sanitizers(tmp_path):
    """tests/host_tables/small_variants_check.cpp, host-only, with ASan, LSan and UBSan."""
    stdout = host_program.run(host_program.build("small_variants_check", tmp_path))
    assert "valid shell3x3 x 3 variants: ke 4, 192 lane rows" in stdout
    assert "five-term variant entry: small 0" in stdout
    assert 'delay past the rings: rejected -4 "plant entry too long for the device history rings"' in stdout
