"""GPU: mpct_hv_select_device and mpct_hv_select against tests/hvsel_ref.py, exactly: integer for integer and
hv bit for bit.  The device entry writes into a guard-filled arena.  The shapes are the smallest at which
the kernels can go wrong: the bitmask's word (64 points) and block (256) edges on grids forced to 1, 2 and
3 workgroups, the LDS tile at T - 1, T, T + 1 and 2T + 3, both sides of every padded instance K = 2, 4, 8,
16, and n_pick at 1, 2, n_picked, past the end of the selection, past M and at its cap."""
import contextlib
import ctypes as C

import numpy as np
import pytest

import hv_ref as R
import hvsel_ref as S

pytestmark = pytest.mark.gpu
GUARD = 0x5A5A5A5A5A5A5A5A
PAD = 32
FIELDS = S.FIELDS
I32 = ("pos", "index", "ties")


@pytest.fixture(scope="module")
def gpu(built, has_gpu):
    if not has_gpu:
        pytest.skip("no GPU")
    return True


@contextlib.contextmanager
def tuned(tile=0, blocks=0):
    """the tile length and the largest grid of hvsel_gain_kernel forced for the calls inside"""
    from mpct import _lib

    lib = _lib.load()
    assert lib.mpct_internal_hvsel_tuned(int(tile), int(blocks)) == 0
    try:
        yield
    finally:
        lib.mpct_internal_hvsel_tuned(0, 0)


def device_call(A, members, lo, ref, N, seed, K, fields=FIELDS, stream=None, sync=True):
    """The device entry into one int64 arena, every output between guards (an int32 output [K] takes
    ceil(K / 2) words; an odd K leaves half a word of guard); returns a dict of the asked-for fields after
    checking that nothing outside them was written."""
    import torch
    from mpct import _lib

    dev = torch.device("cuda", 0)
    A = np.ascontiguousarray(A, dtype=np.float64)
    A = A if A.ndim == 2 else A.reshape(-1, 1)
    Cn, k = A.shape
    t = torch.from_numpy(A).to(dev) if Cn else torch.zeros((1, k), dtype=torch.float64, device=dev)
    if members is None:
        tm, M = None, Cn
    else:
        mem = np.ascontiguousarray(members, dtype=np.int32)
        M = mem.size
        tm = torch.from_numpy(mem).to(dev) if M else torch.zeros(1, dtype=torch.int32, device=dev)
    tlo = torch.from_numpy(np.ascontiguousarray(lo, dtype=np.float64)).to(dev)
    tref = torch.from_numpy(np.ascontiguousarray(ref, dtype=np.float64)).to(dev)
    words = {f: 1 if f in ("n_picked", "n_covered_all") else (K + 1) // 2 if f in I32 else K for f in FIELDS}
    off, o = {}, PAD
    for f in FIELDS:
        off[f] = o
        o += words[f] + PAD
    arena = torch.full((o,), GUARD, dtype=torch.int64, device=dev)
    ctype = {f: _lib.c_int32_p if f in I32 else _lib.c_double_p if f == "hv" else _lib.c_int64_p for f in FIELDS}
    r = _lib.MpctHvSelectResult(*[C.cast(C.c_void_p(arena.data_ptr() + 8 * off[f]), ctype[f]) if f in fields else None
                                  for f in FIELDS])
    st = (stream or torch.cuda.current_stream(dev)).cuda_stream
    rc = _lib.load().mpct_hv_select_device(C.c_void_p(t.data_ptr()), Cn, k, C.c_void_p(tm.data_ptr()) if tm is not None else None,
                                           M, C.c_void_p(tlo.data_ptr()), C.c_void_p(tref.data_ptr()), int(N), int(seed),
                                           int(K), C.byref(r), C.c_void_p(st))
    assert rc == 0, _lib.last_error()

    def collect():
        a = arena.cpu().numpy()
        g32 = np.full(2, GUARD, dtype=np.int64).view(np.int32)
        written = np.zeros(a.size, dtype=bool)
        got = {}
        for f in fields:
            w = a[off[f]:off[f] + words[f]].copy()
            written[off[f]:off[f] + words[f]] = True
            if f in I32:
                w = w.view(np.int32)
                assert K % 2 == 0 or w[K] == g32[1], "the call wrote past %s[K - 1]" % f
                got[f] = w[:K].copy()
            elif f == "hv":
                got[f] = w.view(np.float64)
            else:
                got[f] = int(w[0]) if words[f] == 1 and f in ("n_picked", "n_covered_all") else w
        assert (a[~written] == GUARD).all(), "the call wrote outside its outputs"
        return got

    if not sync:
        return collect, (t, tm, tlo, tref, arena)   # keep the tensors alive until the caller has synchronised
    torch.cuda.synchronize(dev)
    return collect()


def host_call(A, members, lo, ref, N, seed, K):
    from mpct.engine import hv_select

    res = hv_select(A, K, members=members, lo=lo, ref=ref, n_samples=N, seed=seed, device=0)
    assert res.n_samples == N and res.volume == R.volume(lo, ref)
    return res


def check(A, members, lo, ref, N, seed, K, what="", host=True, want=None):
    """both entries against the reference; returns the reference"""
    want = want or S.select_np(A, members, lo, ref, N, seed, K)
    S.compare(device_call(A, members, lo, ref, N, seed, K), want, what + " device entry")
    if host:
        S.compare(host_call(A, members, lo, ref, N, seed, K), want, what + " host entry")
    return want


def box(k, hi=9.5):
    return np.zeros(k), np.full(k, hi)


# ---- sizes at every place the code branches ---------------------------------------------------
@pytest.mark.parametrize("N", [1, 63, 64, 65, 255, 256, 257, 1000])
def test_sample_counts_on_small_grids(gpu, N):
    """word and block edges of the bitmask: one point, the wave and the workgroup at n - 1, n, n + 1, and
    1,000 points = 3 blocks and one of 232; on grids forced to 1, 2 and 3 workgroups and the default"""
    A = R.generated(150, 3, 30)
    lo, ref = box(3, 29.5)
    want = check(A, None, lo, ref, N, 11, 12, "N = %d" % N)
    assert want["n_picked"] >= (8 if N >= 255 else 1)
    for blocks in (1, 2, 3):
        with tuned(0, blocks):
            S.compare(device_call(A, None, lo, ref, N, 11, 12), want, "N = %d, grid %d" % (N, blocks))
    if N == 1000:
        with tuned(256, 2):
            S.compare(device_call(A, None, lo, ref, N, 11, 12), want, "tile 256, grid 2")


@pytest.mark.parametrize("M", [0, 1, 127, 128, 129, 259])
def test_member_counts_at_tile_128(gpu, M):
    """T - 1, T, T + 1 and 2T + 3 members at the forced tile T = 128, none and one"""
    A = R.generated(400, 4, 30)
    mem = np.random.default_rng(M).permutation(400)[:M].astype(np.int32)
    lo, ref = box(4, 29.5)
    with tuned(128, 0):
        want = check(A, mem, lo, ref, 700, 2, 10, "M = %d" % M)
    assert want["n_picked"] >= min(M, 8)
    if M == 0:
        assert want["pos"].tolist() == [-1] * 10 and want["hv"].tolist() == [0.0] * 10
        S.compare(device_call(np.zeros((0, 4)), None, lo, ref, 700, 2, 10), want, "C = 0")


@pytest.mark.parametrize("M", [255, 256, 257, 515])
def test_member_counts_at_tile_256(gpu, M):
    """the other tile instance at T - 1, T, T + 1 and 2T + 3, on a grid of 2"""
    A = R.generated(M, 3, 30)
    lo, ref = box(3, 29.5)
    want = S.select_np(A, None, lo, ref, 600, 8, 10)
    assert want["n_picked"] >= 8
    with tuned(256, 2):
        check(A, None, lo, ref, 600, 8, 10, "M = %d, T = 256" % M, want=want)


@pytest.mark.parametrize("k", [1, 2, 3, 4, 5, 8, 9, 16])
def test_objective_counts(gpu, k):
    """both sides of every padded instance"""
    hi = 400 if k <= 2 else 30 if k <= 5 else 6 if k <= 9 else 2
    A = R.generated(140, k, hi)
    want = check(A, None, *box(k, hi - 0.5), 900, 3, 10, "k = %d" % k)
    # one member carries a 1-D front and few a 2-D one, whatever hi
    assert want["n_picked"] >= (8 if k > 2 else 5 if k == 2 else 1) and want["n_covered_all"] > 0


def test_pick_counts(gpu):
    """K = 1, 2, n_picked, n_picked + 5 (the end-of-selection fill), M + 5, and the cap once at a small N"""
    A = R.generated(60, 3, 12)
    lo, ref = box(3, 11.5)
    full = S.select_np(A, None, lo, ref, 500, 4, 65)
    n = full["n_picked"]
    assert 8 <= n < 60 and full["covered"][n - 1] == full["n_covered_all"] == R.hv_np(A, None, lo, ref, 500, 4)[0]
    for K in (1, 2, n, n + 5, 65):
        want = check(A, None, lo, ref, 500, 4, K, "K = %d" % K)
        for f in ("pos", "index", "gain", "covered", "ties"):
            np.testing.assert_array_equal(want[f], full[f][:K])
    want = check(A, None, lo, ref, 200, 4, 1024, "K = 1024", host=False)
    assert want["n_picked"] < 60 and (want["pos"][60:] == -1).all()


# ---- the members vector and the values --------------------------------------------------------
def test_members_variants(gpu):
    A = R.generated(500, 3, 30)
    lo, ref = box(3, 29.5)
    rng = np.random.default_rng(4)
    with tuned(128, 2):
        sub = rng.permutation(500)[:300].astype(np.int32)
        want = check(A, sub, lo, ref, 800, 1, 12, "shuffled subset")
        assert want["n_picked"] >= 8
        holes = sub.copy()
        holes[[0, 60, 127, 128, 255, 256, 299]] = -1            # the ends and the middle of tiles of 128
        check(A, holes, lo, ref, 800, 1, 12, "-1 entries")
        tile = sub.copy()
        tile[128:256] = -1                                      # a whole tile skipped
        check(A, tile, lo, ref, 800, 1, 12, "a tile of -1")
        none = check(A, np.full(130, -1, dtype=np.int32), lo, ref, 800, 1, 3, "all skipped")
        assert none["n_picked"] == 0 and none["n_covered_all"] == 0
        # a duplicate of the first pick: a separate entry that ties with it, and is never picked after it
        dup = np.append(sub, sub[want["pos"][0]]).astype(np.int32)
        got = check(A, dup, lo, ref, 800, 1, 12, "duplicate")
        assert got["ties"][0] == want["ties"][0] + 1 and got["pos"][0] == want["pos"][0] and 300 not in got["pos"]
    # out of range is skipped by the device entry (the host entry refuses it: tests/test_hv_select.py)
    wild = np.array([3, 500, -2, 7, 2 ** 31 - 1, -2 ** 31], dtype=np.int32)
    S.compare(device_call(A, wild, lo, ref, 800, 1, 4), S.select_np(A, np.array([3, -1, -1, 7, -1, -1]), lo, ref, 800, 1, 4), "wild")


def test_special_values(gpu):
    nan, inf = np.nan, np.inf
    A = R.generated(270, 5, 12)             # k = 5 in the K = 8 instance: column 4 is beside the padding
    A[3, 0] = nan
    A[64, 4] = nan                          # the last column, next to the padded ones
    A[65, 2] = nan
    A[100] = nan
    A[7] = inf
    A[8, 1] = -inf
    A[10, 3] = inf
    A[11] = [-3.0, -1.0, 0.0, -0.0, 5.0]    # below lo in two columns, a signed zero
    A[12] = [12.0, 0.0, 0.0, 0.0, 0.0]      # above ref in one
    lo, ref = box(5, 11.5)
    want = check(A, None, lo, ref, 3000, 9, 14, "special")
    assert want["n_picked"] >= 8 and not set(want["index"].tolist()) & {3, 64, 65, 100, 7, 10, 12}
    only = check(A, [3, 64, 65, 100, 7, 10, 12], lo, ref, 500, 9, 3, "members that cover nothing")
    assert only["n_picked"] == 0
    # -0.0 against a lo of +0.0, and the reverse: the corner covers every point
    for a, l in ((-0.0, 0.0), (0.0, -0.0)):
        want = check(np.array([[a, a]]), None, np.array([l, l]), np.array([1.0, 2.0]), 300, 1, 2, "signed zeros")
        assert want["gain"].tolist() == [300, 0] and want["hv"].tolist() == [2.0, 2.0]
    # -inf covers every point, +inf none
    want = check(np.array([[inf, 0.0], [-inf, -inf]]), None, np.array([-5.0, 1e-3]), np.array([-1.0, 1e3]), 300, 1, 2, "inf")
    assert want["pos"].tolist() == [1, -1]


def test_ties(gpu):
    """an all-covering row at two positions: ties[0] == 2 and the lower position wins; and a generated input
    with a tied round after round 0"""
    A = R.generated(200, 3, 30)
    A[150] = A[37] = -1.0
    lo, ref = box(3, 29.5)
    want = check(A, None, lo, ref, 700, 3, 3, "two all-covering rows")
    assert want["ties"][0] == 2 and want["pos"][0] == 37 and want["n_picked"] == 1
    B = R.generated(90, 3, 1000)
    lo, ref = box(3, 999.5)
    with tuned(128, 3):
        want = check(B, None, lo, ref, 2000, 13, 12, "generated ties")
    assert want["n_picked"] >= 8 and want["ties"][0] == 1 and (want["ties"][1:want["n_picked"]] > 1).any()


# ---- properties -------------------------------------------------------------------------------
def test_properties_against_hypervolume(gpu):
    """the permutation property where every pick was forced; n_covered_all is mpct_hypervolume's n_covered;
    gain[0] is the largest single-member n_covered"""
    from mpct.engine import hypervolume

    A = R.generated(90, 3, 20000)
    lo, ref = box(3, 19999.5)
    N, seed, K = 3001, 13, 10
    want = S.select_np(A, None, lo, ref, N, seed, K)
    n = want["n_picked"]
    assert n >= 8 and (want["ties"][:n] == 1).all()
    got = device_call(A, None, lo, ref, N, seed, K)
    S.compare(got, want, "unpermuted")
    perm = np.random.default_rng(10).permutation(90).astype(np.int32)
    p = device_call(A, perm, lo, ref, N, seed, K)
    for f in ("n_picked", "gain", "covered", "ties", "n_covered_all"):
        np.testing.assert_array_equal(p[f], got[f])
    assert p["hv"].tobytes() == got["hv"].tobytes()
    np.testing.assert_array_equal(p["index"], got["index"])
    np.testing.assert_array_equal(perm[p["pos"][:n]], got["pos"][:n])
    assert got["n_covered_all"] == hypervolume(A, lo=lo, ref=ref, n_samples=N, seed=seed, device=0).n_covered
    single = max(hypervolume(A, members=[m], lo=lo, ref=ref, n_samples=N, seed=seed, device=0).n_covered for m in range(0, 90))
    assert got["gain"][0] == single


# ---- call variants ----------------------------------------------------------------------------
def test_output_subsets(gpu):
    """each pointer alone, each pointer missing, all, and a few mixed subsets of the 255"""
    A = R.generated(300, 3, 100)
    mem = np.random.default_rng(2).permutation(300)[:200].astype(np.int32)
    lo, ref = box(3, 99.5)
    want = S.select_np(A, mem, lo, ref, 1000, 4, 11)               # an odd K: the int32 outputs end mid-word
    assert want["n_picked"] >= 8
    subsets = [(f,) for f in FIELDS] + [tuple(g for g in FIELDS if g != f) for f in FIELDS]
    subsets += [FIELDS, ("pos", "hv"), ("gain", "ties", "n_covered_all"), ("n_picked", "index", "covered")]
    assert len(set(subsets)) == 20
    for fields in subsets:
        got = device_call(A, mem, lo, ref, 1000, 4, 11, fields=fields)
        assert set(got) == set(fields)
        S.compare(got, want, "+".join(fields))


def test_repeated_and_streams_and_host(gpu):
    import torch

    A, B = R.generated(600, 3, 30), R.generated(450, 7, 6)
    la, ra = box(3, 29.5)
    lb, rb = box(7, 5.5)
    first = device_call(A, None, la, ra, 3000, 1, 12)
    again = device_call(A, None, la, ra, 3000, 1, 12)
    for f in FIELDS:
        assert np.asarray(first[f]).tobytes() == np.asarray(again[f]).tobytes(), f
    wa, wb = S.select_np(A, None, la, ra, 3000, 1, 12), S.select_np(B, None, lb, rb, 2500, 2, 9)
    S.compare(first, wa, "first")
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    ca, keep_a = device_call(A, None, la, ra, 3000, 1, 12, stream=s1, sync=False)
    cb, keep_b = device_call(B, None, lb, rb, 2500, 2, 9, stream=s2, sync=False)
    s1.synchronize()
    s2.synchronize()
    S.compare(ca(), wa, "stream 1")
    S.compare(cb(), wb, "stream 2")
    # the host entry right after a device entry that has not been waited for
    cc, keep_c = device_call(A, None, la, ra, 3000, 1, 12, sync=False)
    S.compare(host_call(B, None, lb, rb, 2500, 2, 9), wb, "host after device")
    torch.cuda.synchronize()
    S.compare(cc(), wa, "device before host")


def test_bad_box_through_the_device_entry(gpu):
    """the device entry cannot read the box before it enqueues: hv is NaN, the counts whatever the
    comparisons give (here the box is empty in column 1: every point has p_1 = lo_1)"""
    A = R.generated(100, 3, 30)
    lo, ref = np.zeros(3), np.array([29.5, 0.0, 29.5])
    got = device_call(A, None, lo, ref, 500, 2, 6)
    assert np.isnan(got["hv"]).all()
    want = S.select_np(A, None, lo, ref, 500, 2, 6)
    S.compare(got, want, "empty box", fields=tuple(f for f in FIELDS if f != "hv"))
    got = device_call(A, None, lo, np.array([29.5, np.inf, 29.5]), 500, 2, 6, fields=("hv", "n_picked"))
    assert np.isnan(got["hv"]).all()


def test_dist_gpu_path(gpu):
    import torch
    from mpct.dist import hv_select_candidates, pareto_candidates

    A = R.generated(700, 3, 30)
    A[4, 1] = np.nan
    t = torch.from_numpy(A).cuda()
    front = pareto_candidates(t)["front"]
    lo, ref = box(3, 29.5)
    want = S.select_np(A, front.cpu().numpy(), lo, ref, 3000, 12, 10)
    assert want["n_picked"] >= 8
    for tensor, fr in ((t, front), (t.cpu(), front.cpu())):
        got = hv_select_candidates(tensor, 10, fr, lo=lo, ref=ref, n_samples=3000, seed=12)
        S.compare({f: v.cpu().numpy() if torch.is_tensor(v) else v for f, v in got.items()}, want, "dist on %s" % tensor.device)


# ---- end to end -------------------------------------------------------------------------------
def test_shell3x3_front_select(gpu):
    """Shell 3x3 at 64 candidates: eval_batch -> pareto -> ParetoResult.select with the default box."""
    from mpct.engine import default_box, eval_batch, hv_select, pareto
    from mpct.scenarios import candidate_grid, shell3x3

    sc, r, yref = shell3x3(n2_max=30, nu_max=5, nit=200)
    N2, Nu, d, l = candidate_grid(64)
    N2[5] = 0                                   # a sentinel: NaN costs
    res = eval_batch(sc, N2, Nu, d, l, r[None], device=0)
    J = res.J1.reshape(64, 3)
    front = pareto(J, device=0)
    assert 2 <= front.front.size < 63 and 5 not in front.front
    picked = front.select(J, 6, n_samples=1 << 14, seed=3, device=0)
    lo, ref = default_box(J, front.front)
    want = S.select_np(J, front.front, lo, ref, 1 << 14, 3, 6)
    print("Shell 3x3, 64 candidates: front %d, picks %s, gains %s, covered %d of %d"
          % (front.front.size, want["index"].tolist(), want["gain"].tolist(), want["covered"][-1], want["n_covered_all"]))
    np.testing.assert_array_equal(picked, want["index"][:want["n_picked"]])
    assert want["n_picked"] >= 2 and set(picked.tolist()) <= set(front.front.tolist())
    full = hv_select(J, 6, members=front.front, n_samples=1 << 14, seed=3, device=0)
    S.compare(full, want, "Shell 3x3")
    np.testing.assert_array_equal(full.share, want["covered"] / np.float64(want["n_covered_all"]))
    np.testing.assert_array_equal(full.lo, lo)


def test_robust_result_select(gpu):
    """RobustResult.select on 12 candidates x 4 model-error draws of shell3x3_mc: the front of the worst-case
    table, then the selection over it."""
    import pareto_ref
    from mpct.engine import default_box, eval_robust
    from mpct.scenarios import candidate_grid, shell3x3_mc

    made = shell3x3_mc(draws=4, nit=120)
    sc, refs = made[0], np.ascontiguousarray(made[1])
    N2, Nu, d, l = (x[::5][:12] for x in candidate_grid(64))
    res = eval_robust(sc, N2, Nu, d, l, refs, device=0)
    T = res.scores(0, "worst")
    assert (~np.isnan(T).any(axis=1)).sum() >= 6
    pf = pareto_ref.pareto_np(T, 0)
    front = pf[2][:pf[3]]
    picked = res.select(4, stat="worst", n_samples=1 << 13, seed=8, device=0)
    lo, ref = default_box(T, front)
    want = S.select_np(T, front, lo, ref, 1 << 13, 8, 4)
    np.testing.assert_array_equal(picked, want["index"][:want["n_picked"]])
    assert want["n_picked"] >= 1
