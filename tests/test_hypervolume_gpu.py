"""GPU: mpct_hypervolume_device and mpct_hypervolume against tests/hv_ref.py, exactly: integer for integer
and hv bit for bit.  The device entry writes into a guard-filled arena.  The shapes are the smallest at
which the kernel can go wrong: the wave (64 points), the workgroup (256), workgroups that stride with a
partial last block, the LDS tile at T - 1, T, T + 1 and 2T + 3, and both sides of every padded instance
K = 2, 4, 8, 16."""
import contextlib
import ctypes as C
import itertools

import numpy as np
import pytest

import hv_ref as R

pytestmark = pytest.mark.gpu
GUARD = 0x5A5A5A5A5A5A5A5A
PAD = 32
FIELDS = ("n_covered", "excl", "depth_hist", "hv")


@pytest.fixture(scope="module")
def gpu(built, has_gpu):
    if not has_gpu:
        pytest.skip("no GPU")
    return True


@contextlib.contextmanager
def tuned(tile=0, blocks=0):
    """the tile length and the largest grid of hv_count_kernel forced for the calls inside"""
    from mpct import _lib

    lib = _lib.load()
    assert lib.mpct_internal_hv_tuned(int(tile), int(blocks)) == 0
    try:
        yield
    finally:
        lib.mpct_internal_hv_tuned(0, 0)


def device_call(A, members, lo, ref, N, seed, fields=FIELDS, stream=None, sync=True, dev_members=None):
    """The device entry into one int64 arena [guard | n_covered | guard | excl | guard | depth_hist | guard |
    hv | guard]; returns (n_covered, excl, depth_hist, hv) with None for the fields not asked for, after
    checking that nothing outside the asked-for fields was written."""
    import torch
    from mpct import _lib

    dev = torch.device("cuda", 0)
    A = np.ascontiguousarray(A, dtype=np.float64)
    A = A if A.ndim == 2 else A.reshape(-1, 1)
    Cn, k = A.shape
    t = torch.from_numpy(A).to(dev) if Cn else torch.zeros((1, k), dtype=torch.float64, device=dev)
    if dev_members is not None:
        tm, M = dev_members, int(dev_members.numel())
    elif members is None:
        tm, M = None, Cn
    else:
        mem = np.ascontiguousarray(members, dtype=np.int32)
        M = mem.size
        tm = torch.from_numpy(mem).to(dev) if M else torch.zeros(1, dtype=torch.int32, device=dev)
    tlo = torch.from_numpy(np.ascontiguousarray(lo, dtype=np.float64)).to(dev)
    tref = torch.from_numpy(np.ascontiguousarray(ref, dtype=np.float64)).to(dev)
    sizes = dict(n_covered=1, excl=M, depth_hist=8, hv=1)
    off, o = {}, PAD
    for f in FIELDS:
        off[f] = o
        o += sizes[f] + PAD
    arena = torch.full((o,), GUARD, dtype=torch.int64, device=dev)
    ptr = {f: C.c_void_p(arena.data_ptr() + 8 * off[f]) if f in fields else None for f in FIELDS}
    r = _lib.MpctHvResult(*[C.cast(ptr[f], _lib.c_double_p if f == "hv" else _lib.c_int64_p) if ptr[f] else None
                            for f in FIELDS])
    st = (stream or torch.cuda.current_stream(dev)).cuda_stream
    rc = _lib.load().mpct_hypervolume_device(C.c_void_p(t.data_ptr()), Cn, k, C.c_void_p(tm.data_ptr()) if tm is not None else None,
                                             M, C.c_void_p(tlo.data_ptr()), C.c_void_p(tref.data_ptr()), int(N),
                                             int(seed), C.byref(r), C.c_void_p(st))
    assert rc == 0, _lib.last_error()

    def collect():
        a = arena.cpu().numpy()
        mask = np.ones(a.size, dtype=bool)
        for f in fields:
            mask[off[f]:off[f] + sizes[f]] = False
        assert (a[mask] == GUARD).all(), "the call wrote outside its outputs"
        got = [a[off[f]:off[f] + sizes[f]].copy() if f in fields else None for f in FIELDS]
        if got[0] is not None:
            got[0] = int(got[0][0])
        if got[3] is not None:
            got[3] = float(got[3].view(np.float64)[0])
        return tuple(got)

    if not sync:
        return collect, (t, tm, tlo, tref, arena)   # keep the tensors alive until the caller has synchronised
    torch.cuda.synchronize(dev)
    return collect()


def host_call(A, members, lo, ref, N, seed):
    from mpct.engine import hypervolume

    res = hypervolume(A, members=members, lo=lo, ref=ref, n_samples=N, seed=seed, device=0)
    assert res.n_samples == N and res.volume == R.volume(lo, ref)
    return res.n_covered, res.excl, res.depth_hist, res.hv


def check(A, members, lo, ref, N, seed, what="", host=True):
    """both entries against the reference; returns the reference"""
    want = R.hv_np(A, members, lo, ref, N, seed)
    R.compare(device_call(A, members, lo, ref, N, seed), want, what + " device entry")
    if host:
        R.compare(host_call(A, members, lo, ref, N, seed), want, what + " host entry")
    return want


def box(k, hi=9.5):
    return np.zeros(k), np.full(k, hi)


# ---- sizes at every place the code branches ---------------------------------------------------
@pytest.mark.parametrize("N", [1, 63, 64, 65, 255, 256, 257])
def test_sample_counts(gpu, N):
    """one point, the wave and the workgroup at n - 1, n, n + 1"""
    A = R.generated(150, 3)
    want = check(A, None, *box(3), N, 11, "N = %d" % N)
    assert want[2].sum() == N


def test_striding_workgroups_with_a_partial_last_block(gpu):
    """1,000 points = 3 blocks of 256 and one of 232, on a grid forced to 2 workgroups (each makes two
    trips) and to 1 and 3 (one workgroup idles on the second trip); the default grid gives the same."""
    A = R.generated(300, 3)
    lo, ref = box(3)
    want = check(A, None, lo, ref, 1000, 5, "default grid")
    assert 0 < want[0] < 1000 and want[2][7] > 0 and want[1].sum() > 0
    for blocks in (2, 1, 3):
        for tile in (128, 256):
            with tuned(tile, blocks):
                R.compare(device_call(A, None, lo, ref, 1000, 5), want, "grid %d, tile %d" % (blocks, tile))


@pytest.mark.parametrize("M", [0, 1, 127, 128, 129, 259])
def test_member_counts_at_tile_128(gpu, M):
    """T - 1, T, T + 1 and 2T + 3 members at the forced tile T = 128, none and one"""
    A = R.generated(400, 4)
    mem = np.random.default_rng(M).permutation(400)[:M].astype(np.int32)
    lo, ref = box(4)
    want = R.hv_np(A, mem, lo, ref, 700, 2)
    with tuned(128, 0):
        R.compare(device_call(A, mem, lo, ref, 700, 2), want, "M = %d" % M)
        if M:
            R.compare(host_call(A, mem, lo, ref, 700, 2), want, "M = %d host" % M)
    if M == 0:
        assert want[2].tolist() == [700] + [0] * 7 and want[3] == 0.0
        R.compare(host_call(A, mem, lo, ref, 700, 2), want, "M = 0 host")
        R.compare(device_call(np.zeros((0, 4)), None, lo, ref, 700, 2), want, "C = 0")


@pytest.mark.parametrize("M", [255, 256, 257, 515])
def test_member_counts_at_tile_256(gpu, M):
    """the other tile instance at T - 1, T, T + 1 and 2T + 3, and the default tile at the same counts"""
    A = R.generated(M, 3)
    lo, ref = box(3)
    want = check(A, None, lo, ref, 600, 8, "M = %d" % M)
    assert want[0] > 0
    with tuned(256, 0):
        R.compare(device_call(A, None, lo, ref, 600, 8), want, "M = %d, T = 256" % M)
        R.compare(host_call(A, None, lo, ref, 600, 8), want, "M = %d, T = 256, host" % M)


@pytest.mark.parametrize("k", [1, 2, 3, 4, 5, 8, 9, 16])
def test_objective_counts(gpu, k):
    """both sides of every padded instance"""
    A = R.generated(140, k, 4 if k > 8 else 10)
    want = check(A, None, *box(k, 3.5 if k > 8 else 9.5), 900, 3, "k = %d" % k)
    assert want[0] > 0 and want[2].sum() == 900


# ---- the members vector -----------------------------------------------------------------------
def test_members_variants(gpu):
    A = R.generated(500, 3)
    lo, ref = box(3)
    rng = np.random.default_rng(4)
    with tuned(128, 0):
        sub = rng.permutation(500)[:300].astype(np.int32)
        want = check(A, sub, lo, ref, 800, 1, "shuffled subset")
        assert want[1].sum() > 0
        holes = sub.copy()
        holes[[0, 60, 127, 128, 255, 256, 299]] = -1            # the ends and the middle of tiles of 128
        check(A, holes, lo, ref, 800, 1, "-1 entries")
        tile = sub.copy()
        tile[128:256] = -1                                      # a whole tile skipped
        check(A, tile, lo, ref, 800, 1, "a tile of -1")
        check(A, np.full(130, -1, dtype=np.int32), lo, ref, 800, 1, "all skipped")
        # a duplicate: both copies get 0, across tiles too
        m = int(np.argmax(want[1]))
        dup = np.append(sub, sub[m]).astype(np.int32)
        got = check(A, dup, lo, ref, 800, 1, "duplicate")
        assert want[1][m] > 0 and got[1][m] == 0 and got[1][-1] == 0 and got[0] == want[0]
        # the permutation guarantee
        perm = rng.permutation(300)
        got = device_call(A, sub[perm], lo, ref, 800, 1)
        R.compare(got, (want[0], want[1][perm], want[2], want[3]), "permuted")
    # out of range is skipped by the device entry (the host entry refuses it: tests/test_hypervolume.py)
    wild = np.array([3, 500, -2, 7, 2 ** 31 - 1, -2 ** 31], dtype=np.int32)
    R.compare(device_call(A, wild, lo, ref, 800, 1), R.hv_np(A, np.array([3, -1, -1, 7, -1, -1]), lo, ref, 800, 1), "wild")


def test_front_buffer_of_a_pareto_call(gpu):
    """the -1-padded front of mpct_pareto_device passed as it is with M = C, without leaving the device"""
    import torch
    from mpct.engine import pareto_device

    import pareto_ref

    A = R.generated(700, 3, 30)
    A[9, 1] = np.nan
    t = torch.from_numpy(A).cuda()
    out = dict(front=torch.empty(700, dtype=torch.int32, device="cuda"), n_front=torch.empty(1, dtype=torch.int32, device="cuda"))
    pareto_device(t, out)
    lo, ref = box(3, 29.5)
    got = device_call(A, None, lo, ref, 2000, 6, dev_members=out["front"])
    front = out["front"].cpu().numpy()
    nf = int(out["n_front"].item())
    want_front = pareto_ref.pareto_np(A, 0)
    np.testing.assert_array_equal(front, want_front[2])
    assert 3 < nf < 200 and (front[nf:] == -1).all()
    R.compare(got, R.hv_np(A, front, lo, ref, 2000, 6), "front buffer")
    # the members off the front add no volume: the same n_covered from all candidates, other depths
    every = device_call(A, None, lo, ref, 2000, 6)
    assert every[0] == got[0] and every[2][0] == got[2][0] and every[2][1] < got[2][1]


# ---- values -----------------------------------------------------------------------------------
def test_special_values(gpu):
    nan, inf = np.nan, np.inf
    A = R.generated(270, 5)                 # k = 5 in the K = 8 instance: column 4 is beside the padding
    A[3, 0] = nan
    A[64, 4] = nan                          # the last column, next to the padded ones
    A[65, 2] = nan
    A[100] = nan
    A[7] = inf
    A[8, 1] = -inf
    A[10, 3] = inf
    A[11] = [-3.0, -1.0, 0.0, -0.0, 2.0]    # below lo in two columns
    A[12] = [12.0, 0.0, 0.0, 0.0, 0.0]      # above ref in one
    lo, ref = box(5)
    want = check(A, None, lo, ref, 3000, 9, "special")
    assert all(want[1][c] == 0 for c in (3, 64, 65, 100, 7, 10, 12)) and want[0] > 0
    only = check(A, [3, 64, 65, 100, 7, 10, 12], lo, ref, 500, 9, "members that cover nothing")
    assert only[0] == 0
    # -0.0 against a lo of +0.0, and the reverse: the corner covers every point
    for a, l in ((-0.0, 0.0), (0.0, -0.0)):
        want = check(np.array([[a, a]]), None, np.array([l, l]), np.array([1.0, 2.0]), 300, 1, "signed zeros")
        assert want[0] == 300 and want[1].tolist() == [300] and want[3] == 2.0
    # -inf covers every point, +inf none
    want = check(np.array([[-inf, -inf], [inf, 0.0]]), None, np.array([-5.0, 1e-3]), np.array([-1.0, 1e3]), 300, 1, "inf")
    assert want[1].tolist() == [300, 0]
    # NaN in the first and last column at each padded instance's edge
    for k in (2, 4, 8, 16):
        D = R.generated(130, k, 4)
        D[1, 0] = nan
        D[2, k - 1] = nan
        check(D, None, *box(k, 3.5), 500, 2, "k = %d with NaN" % k)


@pytest.mark.parametrize("seed", [0, 0xDEADBEEFCAFEF00D])
def test_ties_and_seeds(gpu, seed):
    """integer costs with many ties and a box with integer edges and a power-of-two width: points land on
    member coordinates (a_j == p_j happens for u = 0 only, equal vectors happen often)"""
    A = np.random.default_rng(7).integers(0, 10, (600, 3)).astype(float)
    assert len({tuple(r) for r in A.tolist()}) < 550                 # equal vectors
    want = check(A, None, np.zeros(3), np.full(3, 8.0), 4000, seed, "ties")
    assert want[0] > 0 and want[2][7] > 0 and want[2][1] > 0
    other = R.hv_np(A, None, np.zeros(3), np.full(3, 8.0), 4000, seed + 1)
    assert other[2].tolist() != want[2].tolist()                     # the seed matters


# ---- call variants ----------------------------------------------------------------------------
def test_output_subsets(gpu):
    A = R.generated(300, 3)
    mem = np.random.default_rng(2).permutation(300)[:200].astype(np.int32)
    lo, ref = box(3)
    want = R.hv_np(A, mem, lo, ref, 1000, 4)
    n = 0
    for m in range(1, 5):
        for fields in itertools.combinations(FIELDS, m):
            R.compare(device_call(A, mem, lo, ref, 1000, 4, fields=fields), want, "+".join(fields))
            n += 1
    assert n == 15


def test_repeated_and_streams_and_host(gpu):
    import torch

    A, B = R.generated(600, 3), R.generated(450, 7)
    la, ra = box(3)
    lb, rb = box(7)
    first = device_call(A, None, la, ra, 3000, 1)
    again = device_call(A, None, la, ra, 3000, 1)
    assert first[0] == again[0] and first[1].tobytes() == again[1].tobytes() and first[2].tobytes() == again[2].tobytes()
    assert np.float64(first[3]).tobytes() == np.float64(again[3]).tobytes()
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    ca, keep_a = device_call(A, None, la, ra, 3000, 1, stream=s1, sync=False)
    cb, keep_b = device_call(B, None, lb, rb, 2500, 2, stream=s2, sync=False)
    s1.synchronize()
    s2.synchronize()
    R.compare(ca(), first, "stream 1")
    R.compare(first, R.hv_np(A, None, la, ra, 3000, 1), "first")
    R.compare(cb(), R.hv_np(B, None, lb, rb, 2500, 2), "stream 2")
    # the host entry right after a device entry that has not been waited for
    cc, keep_c = device_call(A, None, la, ra, 3000, 1, sync=False)
    R.compare(host_call(B, None, lb, rb, 2500, 2), R.hv_np(B, None, lb, rb, 2500, 2), "host after device")
    torch.cuda.synchronize()
    R.compare(cc(), first, "device before host")


def test_dist_gpu_path(gpu):
    import torch
    from mpct.dist import hypervolume_candidates, pareto_candidates

    A = R.generated(700, 3, 30)
    A[4, 1] = np.nan
    t = torch.from_numpy(A).cuda()
    front = pareto_candidates(t)["front"]
    lo, ref = box(3, 29.5)
    got = hypervolume_candidates(t, front, lo=lo, ref=ref, n_samples=3000, seed=12)
    want = R.hv_np(A, front.cpu().numpy(), lo, ref, 3000, 12)
    R.compare((got["n_covered"], got["excl"].cpu().numpy(), got["depth_hist"].cpu().numpy(), got["hv"]), want, "dist")
    cpu = hypervolume_candidates(t.cpu(), front.cpu(), lo=lo, ref=ref, n_samples=3000, seed=12)
    R.compare((cpu["n_covered"], cpu["excl"].numpy(), cpu["depth_hist"].numpy(), cpu["hv"]), want, "dist on the CPU")


# ---- end to end -------------------------------------------------------------------------------
def test_shell3x3_front_hypervolume(gpu):
    """Shell 3x3 at 64 candidates: eval_batch -> pareto -> ParetoResult.hypervolume with the default box."""
    from mpct.engine import default_box, eval_batch, pareto
    from mpct.scenarios import candidate_grid, shell3x3

    sc, r, yref = shell3x3(n2_max=30, nu_max=5, nit=200)
    N2, Nu, d, l = candidate_grid(64)
    N2[5] = 0                                   # a sentinel: NaN costs
    res = eval_batch(sc, N2, Nu, d, l, r[None], device=0)
    J = res.J1.reshape(64, 3)
    front = pareto(J, device=0)
    assert 2 <= front.front.size < 63 and 5 not in front.front
    got = front.hypervolume(J, n_samples=1 << 14, seed=3, device=0)
    lo, ref = default_box(J, front.front)
    np.testing.assert_array_equal(got.lo, lo)
    np.testing.assert_array_equal(got.ref, ref)
    np.testing.assert_array_equal(got.members, front.front)
    want = R.hv_np(J, front.front, lo, ref, 1 << 14, 3)
    print("Shell 3x3, 64 candidates: front %d, covered %d of %d, hv %.6g, depth histogram %s"
          % (front.front.size, want[0], 1 << 14, want[3], want[2].tolist()))
    R.compare((got.n_covered, got.excl, got.depth_hist, got.hv), want, "Shell 3x3")
    assert 0 < got.n_covered < 1 << 14 and got.volume == R.volume(lo, ref)
    np.testing.assert_array_equal(got.contribution, want[1] / (1 << 14) * got.volume)


def test_robust_result_hypervolume(gpu):
    """RobustResult.hypervolume on 12 candidates x 4 model-error draws of shell3x3_mc: the front of the
    worst-case table, then its hypervolume."""
    import pareto_ref
    from mpct.engine import default_box, eval_robust
    from mpct.scenarios import candidate_grid, shell3x3_mc

    made = shell3x3_mc(draws=4, nit=120)
    sc, refs = made[0], np.ascontiguousarray(made[1])
    N2, Nu, d, l = (x[::5][:12] for x in candidate_grid(64))
    res = eval_robust(sc, N2, Nu, d, l, refs, device=0)
    S = res.scores(0, "worst")
    assert (~np.isnan(S).any(axis=1)).sum() >= 6
    pf = pareto_ref.pareto_np(S, 0)
    front = pf[2][:pf[3]]
    got = res.hypervolume(stat="worst", n_samples=1 << 13, seed=8, device=0)
    lo, ref = default_box(S, front)
    np.testing.assert_array_equal(got.members, front)
    R.compare((got.n_covered, got.excl, got.depth_hist, got.hv), R.hv_np(S, front, lo, ref, 1 << 13, 8), "robust")
    assert got.n_covered > 0
