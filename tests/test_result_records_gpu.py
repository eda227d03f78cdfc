"""GPU: the path of a finished simulation's record from the wavefront to the caller's arrays
(include/mpct.h: "any pointer may be NULL to skip that output"), with explicit field subsets, guarded
buffers and ragged batch sizes (tests/record_calls.py makes the calls).

From kOrderMinC = 256 candidates on the linear kernels write no caller array themselves: stage_row lays
out a row of the requested fields only, the dispatch-key launch prefills those rows, the class launches
(up to three, on fanned streams) write them through put_record at xcd_row(slot, S), and
unpermute_kernel scatters them through the permutation, turning status and qp_iters back from doubles.
The band and NMPC launches write the caller's arrays directly, field by field.  Trajectories always go
straight to the caller's index; those of a simulation that is not run (skipped, bad horizon) are NaN.

Reference: records do not depend on the batch position, bitwise (tests/test_gpu_parity.py), so every
scenario has a pool of 16 distinct valid candidates and three invalid ones (record_calls.pool), scored
once in a 19-candidate call with all fields (unordered, direct path), and every large batch is that pool
tiled and permuted with a fixed seed: every requested field of every row of a large call must equal the
pool's record of the same candidate bit for bit, NaNs included.  The pools were chosen on the CPU
(Shell 3x3: status 0 on the C port on all three reference sets; WoodBerry: finite costs in
oracle.dtcgpc.dtc_gpc_ww on all three draws; Van de Vusse: at most 8 Gauss-Newton iterations a step and
every state inside its bounds in tests/nmpc_mismatch_ref.py), and test_pool asserts status 0 on the
device and, for Shell 3x3, agreement with the C port within COST_RTOL before anything else is compared.

Sizes: C = 255 is the last direct size, 256 the first staged one, 257 and 261 give S mod 8 = 1 and 5,
257 x 3 reference sets S = 771, S mod 8 = 3."""
import numpy as np
import pytest

import record_calls as rc
from record_calls import BENCH, COST, FULL_SET, SINGLES, bits, subset_id
from test_gpu_parity import COST_RTOL

pytestmark = pytest.mark.gpu

LINEAR = ("shell5", "shell8", "shell8-ol", "dtc")
SIZES = [(255, 1), (256, 1), (257, 1), (261, 1), (257, 3)]
EXT8 = "gpc_closed_loop_kernel<16,false,true> + <32,false,true>"   # shell8 with trajectories / open loop


@pytest.fixture(scope="module")
def gpu(built, has_gpu):
    if not has_gpu:
        pytest.skip("no GPU")
    return True


_scen, _pool = {}, {}


def scen(name):
    """The scenario, its kernel instance pinned (a routing change must not silently empty a test)."""
    from mpct.engine import kernel_instance

    if name not in _scen:
        q = rc.scenario(name)
        assert kernel_instance(q["sc"], open_loop=q["open_loop"]) == q["instance"]
        _scen[name] = q
    return _scen[name]


def signals(q, nref):
    return q["refs"][:nref], None if q["v"] is None else q["v"][:nref]


def pool_records(name, nref, traj=()):
    """The pool's records: one 19-candidate host call with all fields (and the trajectories `traj`),
    C < kOrderMinC: no order, no staging.  Computed once per (scenario, nref) and left unchanged."""
    key = (name, nref, tuple(traj))
    if key not in _pool:
        q = scen(name)
        refs, v = signals(q, nref)
        rec = rc.call("host", q["sc"], q["pool"], refs, v, COST + tuple(traj), open_loop=q["open_loop"],
                      want_traj=bool(traj))
        st = rec["status"].reshape(19, nref)
        assert np.all(st[:16] == 0), st[:16]
        assert np.all(st[16:] == np.array(rc.INVALID_STATUS)[:, None]), st[16:]
        for f in ("J1", "j21", "j22", "Jnu") + tuple(traj):   # a simulation that is not run: NaN throughout
            assert np.all(np.isnan(rec[f].reshape(19, nref, -1)[16:])), f
        for a in rec.values():
            a.setflags(write=False)
        _pool[key] = rec
    return _pool[key]


def check_batch(name, got, idx, nref, fields, traj=()):
    """Every requested field of every row of a large call against the pool's record of its candidate."""
    S = len(idx) * nref
    assert np.any(idx < 16) and np.any(idx >= 16)   # valid and invalid candidates are compared
    assert set(got) == set(fields)
    ref = pool_records(name, nref, traj)
    for f in fields:
        want = rc.expect(ref[f], idx, nref)
        assert got[f].shape == want.shape and got[f].shape[0] == S, (f, got[f].shape, S)
        bad = np.flatnonzero(np.any(bits(got[f]) != bits(want), axis=1))
        assert bad.size == 0, "%s: %d of %d rows differ from the pool's record, first rows %s (pool candidates %s)" % (
            f, bad.size, S, bad[:6], idx[bad[:6] // nref])


# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", LINEAR + ("band", "nmpc"))
def test_pool(gpu, name):
    """Before anything else: the pool's valid records have status 0, the invalid three 8 / 16 / 16 with
    NaN costs, the candidates span the QP-size classes the scenario's instance string names, j21 and
    Jnu are NaN in a cost-only call and live with open_loop, and the Shell 3x3 costs are the C port's
    within COST_RTOL (the bitwise chain of every other test hangs on an independent number)."""
    q = scen(name)
    sc = q["sc"]
    N2, Nu, d, l = q["pool"]
    M = sc.nu * Nu[:16].astype(int)
    if name in ("shell8", "shell8-ol", "dtc"):
        assert np.any(M <= 16) and np.any(M > 16), M
    if name == "nmpc":
        assert np.any(M <= 15) and np.any(M > 15), M
    for nref in sorted({1, q["refs"].shape[0]}):
        rec = pool_records(name, nref)
        assert np.all(np.isfinite(rec["J1"][:16 * nref])) and np.all(np.isfinite(rec["j22"][:16 * nref]))
        live = np.isfinite(rec["j21"][:16 * nref]).all() and np.isfinite(rec["Jnu"][:16 * nref]).all()
        dead = np.isnan(rec["j21"]).all() and np.isnan(rec["Jnu"]).all()
        assert live if q["open_loop"] else dead
        # distinct candidates have distinct records: a row from the wrong candidate cannot pass
        assert len(np.unique(bits(rec["J1"][:16 * nref]), axis=0)) == 16 * nref
    if not name.startswith("shell"):
        return
    from oracle.cport import CPort
    from oracle.scenarios import shell3x3 as o_shell3x3

    osc, orr, oyref, _ = o_shell3x3()
    assert np.array_equal(rc.shell_refs(orr[:, :rc.NIT]), q["refs"])
    cp = CPort(osc, 30, rc.NIT, np.ascontiguousarray(oyref[:, :rc.NIT]))
    ref = cp.eval(N2[:16], Nu[:16], d[:16], l[:16], q["refs"], open_loop=q["open_loop"])
    assert np.all(ref["status"] == 0)
    rec = pool_records(name, 3)
    for f in ("J1", "j22") + (("j21",) if q["open_loop"] else ()):
        rel = float(np.max(np.abs(rec[f][:48] - ref[f]) / np.abs(ref[f])))
        print("%s pool %s against the C port: max rel %.2e" % (name, f, rel))
        assert rel < COST_RTOL, (f, rel)
    if q["open_loop"]:
        # Jnu divides by |diff(uopt)| (VNS2.m:185): compared where the oracle's moves are not tiny, by
        # the rule and the tolerance of tests/test_gpu_parity.py::test_vns_objective
        ok = ref["Jnu"] < 1e6
        assert ok.sum() > ok.size // 2
        rel = float(np.max(np.abs(rec["Jnu"][:48][ok] - ref["Jnu"][ok]) / np.maximum(np.abs(ref["Jnu"][ok]), 1e-12)))
        print("%s pool Jnu against the C port: max rel %.2e on %d of %d entries" % (name, rel, ok.sum(), ok.size))
        assert rel < 1e-5, rel


@pytest.mark.parametrize("fields", FULL_SET, ids=subset_id)
@pytest.mark.parametrize("C,nref", SIZES)
@pytest.mark.parametrize("name", LINEAR)
def test_linear_field_subsets(gpu, name, C, nref, fields):
    """The linear kernels through the device entry: the six single fields, the six leave-one-out sets,
    the benchmark's request and all six put every field at every staging offset it can have, on both
    sides of kOrderMinC and at ragged S."""
    q = scen(name)
    refs, v = signals(q, nref)
    idx = rc.tiled(C)
    got = rc.call("device", q["sc"], rc.take(q["pool"], idx), refs, v, fields, open_loop=q["open_loop"])
    check_batch(name, got, idx, nref, fields)


@pytest.mark.parametrize("fields", SINGLES, ids=subset_id)
@pytest.mark.parametrize("name", ("band", "nmpc"))
def test_band_and_nmpc_field_subsets(gpu, name, fields):
    """The band and NMPC launches (prefill_results plus their own record writes, no staging) with every
    single field and all six, C = 257 (NMPC: behind its dispatch order)."""
    q = scen(name)
    refs, v = signals(q, 1)
    idx = rc.tiled(257)
    got = rc.call("device", q["sc"], rc.take(q["pool"], idx), refs, v, fields)
    check_batch(name, got, idx, 1, fields)


def test_stale_staging_rows(gpu):
    """One scenario, one stream: a wide staged call, a narrower row in a smaller blob, a regrow, the
    direct path, a one-double row.  No call may see a row, an offset or a permutation of the one before."""
    import torch

    q = scen("shell8")
    stream = torch.cuda.Stream(torch.device("cuda", 0))
    for C, nref, fields in ((257, 3, COST), (256, 1, ("J1",)), (2056, 1, COST), (255, 1, COST), (257, 1, ("status",))):
        refs, v = signals(q, nref)
        idx = rc.tiled(C, seed=C + nref)
        got = rc.call("device", q["sc"], rc.take(q["pool"], idx), refs, v, fields, stream=stream)
        check_batch("shell8", got, idx, nref, fields)


@pytest.mark.parametrize("open_loop", [False, True])
@pytest.mark.parametrize("entry", ["host", "device"])
def test_trajectories_behind_an_ordered_launch(gpu, entry, open_loop):
    """want_traj at C = 257 through the host and the device entry: the cost records go through the
    staging rows, the trajectories straight to the caller's index, so y, u (ys, uopt) of every row must
    be the pool call's rows of the same candidate and their guards intact (a trajectory written at the
    slot would land on another candidate's row).  The rows of the skipped and bad-horizon candidates are
    NaN like their costs (fill_unrun_trajectories, work_order.hip): no canary survives in the device
    entry's buffers and no scratch of an earlier call comes back through the host entry's."""
    from mpct.engine import kernel_instance

    name = "shell8-ol" if open_loop else "shell8"
    q = scen(name)
    assert kernel_instance(q["sc"], open_loop=open_loop, want_traj=True) == EXT8
    traj = ("y", "u") + (("ys", "uopt") if open_loop else ())
    refs, v = signals(q, 1)
    idx = rc.tiled(257)
    got = rc.call(entry, q["sc"], rc.take(q["pool"], idx), refs, v, COST + traj, open_loop=open_loop, want_traj=True)
    ref = pool_records(name, 1, traj)
    for f in traj:   # the candidates' trajectories differ, so a misplaced row cannot pass
        assert len(np.unique(bits(ref[f][:16]), axis=0)) == 16, f
        assert np.all(np.isnan(got[f][idx >= 16])) and np.all(np.isfinite(got[f][idx < 16])), f
    check_batch(name, got, idx, 1, COST + traj, traj)


@pytest.mark.parametrize("name", ("band", "nmpc"))
def test_band_and_nmpc_trajectories(gpu, name):
    """The same through the band and NMPC launches (device entry, C = 257, y and u beside the status)."""
    from mpct.engine import kernel_instance

    q = scen(name)
    assert kernel_instance(q["sc"], want_traj=True) == q["instance"]
    refs, v = signals(q, 1)
    idx = rc.tiled(257)
    fields = ("status", "y", "u")
    got = rc.call("device", q["sc"], rc.take(q["pool"], idx), refs, v, fields, want_traj=True)
    for f in ("y", "u"):
        assert np.all(np.isnan(got[f][idx >= 16])) and np.all(np.isfinite(got[f][idx < 16])), f
    check_batch(name, got, idx, 1, fields, ("y", "u"))


@pytest.mark.parametrize("fields", FULL_SET, ids=subset_id)
def test_host_entry_field_subsets(gpu, fields):
    """mpct_eval_batch at C = 257: the device side stages all six fields, HostStage copies back only
    what was asked, and the numpy guards stay intact."""
    q = scen("shell5")
    refs, v = signals(q, 1)
    idx = rc.tiled(257)
    got = rc.call("host", q["sc"], rc.take(q["pool"], idx), refs, v, fields)
    check_batch("shell5", got, idx, 1, fields)


@pytest.mark.parametrize("fields", [BENCH, ("status",)], ids=subset_id)
@pytest.mark.parametrize("C", [257, 600])
def test_multi_entry_field_subsets(gpu, C, fields):
    """mpct_eval_batch_multi with device 0 listed twice against the single-device call: 257 candidates
    are shards of 129 and 128 (both direct, while the single-device call is staged), 600 are two
    staged shards of 300."""
    from mpct.engine import shard_candidates

    q = scen("shell5")
    assert [len(shard_candidates(C, 2, k)) for k in (0, 1)] == {257: [129, 128], 600: [300, 300]}[C]
    refs, v = signals(q, 1)
    idx = rc.tiled(C)
    cands = rc.take(q["pool"], idx)
    one = rc.call("host", q["sc"], cands, refs, v, fields)
    two = rc.call("multi", q["sc"], cands, refs, v, fields, devices=(0, 0))
    for f in fields:
        np.testing.assert_array_equal(bits(two[f]), bits(one[f]), err_msg=f)
    check_batch("shell5", two, idx, 1, fields)


@pytest.mark.parametrize("entry,C", [("device", 19), ("device", 257), ("host", 257), ("multi", 257)])
def test_no_field_requested(gpu, entry, C):
    """All ten result pointers NULL (include/mpct.h): stage_row gives w = 0, no stage is allocated,
    put_record and the prefill write nothing, and the call returns MPCT_OK.  The next call on the same
    scenario is unaffected."""
    q = scen("shell8")
    refs, v = signals(q, 1)
    idx = rc.tiled(C)
    pending = rc.launch(entry, q["sc"], rc.take(q["pool"], idx), refs, v, ())
    assert pending.rc == 0
    assert pending.finish() == {}
    got = rc.call(entry, q["sc"], rc.take(q["pool"], idx), refs, v, ("status",))
    check_batch("shell8", got, idx, 1, ("status",))
