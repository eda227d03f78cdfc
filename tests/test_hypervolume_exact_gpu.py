"""GPU: mpct_hypervolume_exact_device and mpct_hypervolume_exact against tests/hvx_ref.py.  Real-valued members
within the contract's bound (M^2 + 8) 2^-53 vol of the values in exact rational arithmetic, lattice members with
`==` (every operation of the sweep is then exact).  The device entry writes into a guard-filled arena.  The
shapes are the smallest at which the kernel can go wrong: the 64-lane chunk at 63, 64, 65 columns, more slabs
than slab groups (group wrap), thousands of columns (chunk carry) and one holder over every column (the
longest run)."""
import ctypes as C
import itertools
from fractions import Fraction

import numpy as np
import pytest

import hv_ref
import hvx_ref as R

pytestmark = pytest.mark.gpu
GUARD = 0x5A5A5A5A5A5A5A5A
PAD = 32
FIELDS = ("hv", "excl", "n_active")


@pytest.fixture(scope="module")
def gpu(built, has_gpu):
    if not has_gpu:
        pytest.skip("no GPU")
    return True


def device_call(A, members, lo, ref, fields=FIELDS, stream=None, sync=True, dev_members=None, want_rc=0):
    """The device entry into one int64 arena [guard | hv | guard | excl | guard | n_active | guard]; returns
    (hv, excl, n_active) with None for the fields not asked for, after checking that nothing outside the
    asked-for fields was written."""
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
    sizes = dict(hv=1, excl=M, n_active=1)
    off, o = {}, PAD
    for f in FIELDS:
        off[f] = o
        o += sizes[f] + PAD
    arena = torch.full((o,), GUARD, dtype=torch.int64, device=dev)
    ptr = {f: C.c_void_p(arena.data_ptr() + 8 * off[f]) if f in fields else None for f in FIELDS}
    r = _lib.MpctHvxResult(*[C.cast(ptr[f], _lib.c_int64_p if f == "n_active" else _lib.c_double_p) if ptr[f] else None
                             for f in FIELDS])
    st = (stream or torch.cuda.current_stream(dev)).cuda_stream
    rc = _lib.load().mpct_hypervolume_exact_device(C.c_void_p(t.data_ptr()), Cn, k,
                                                   C.c_void_p(tm.data_ptr()) if tm is not None else None, M,
                                                   C.c_void_p(tlo.data_ptr()), C.c_void_p(tref.data_ptr()), C.byref(r),
                                                   C.c_void_p(st))
    assert rc == want_rc, _lib.last_error()

    def collect():
        a = arena.cpu().numpy()
        mask = np.ones(a.size, dtype=bool)
        for f in fields:
            mask[off[f]:off[f] + sizes[f]] = False
        assert (a[mask] == GUARD).all(), "the call wrote outside its outputs"
        hv = float(a[off["hv"]:off["hv"] + 1].view(np.float64)[0]) if "hv" in fields else None
        excl = a[off["excl"]:off["excl"] + M].view(np.float64).copy() if "excl" in fields else None
        na = int(a[off["n_active"]]) if "n_active" in fields else None
        return hv, excl, na

    if not sync:
        return collect, (t, tm, tlo, tref, arena)   # keep the tensors alive until the caller has synchronised
    torch.cuda.synchronize(dev)
    return collect()


def host_call(A, members, lo, ref):
    from mpct.engine import hypervolume_exact

    res = hypervolume_exact(A, members=members, lo=lo, ref=ref, device=0)
    assert res.vol == hv_ref.volume(lo, ref)
    return res.hv, res.excl, res.n_active


def same_bits(a, b):
    return np.asarray(a, dtype=np.float64).tobytes() == np.asarray(b, dtype=np.float64).tobytes()


def within_bound(got, want, M, vol, what):
    """|hv - HV| and every |excl[m] - EXCL_m| at most (M^2 + 8) 2^-53 vol; an exact zero is +0.0 bit for bit"""
    hv, excl, na = got
    HV, EXCL, NA = want
    bd = R.bound(M, vol)
    err = [abs(Fraction(hv) - HV)] + [abs(Fraction(float(e)) - E) for e, E in zip(excl, EXCL)]
    print("%s: M = %d, n_active = %d, largest error %.3g of the bound's %d units of 2^-53 vol"
          % (what, M, NA, float(max(err) / (R.EPS * Fraction(float(vol)))), M * M + 8))
    assert na == NA, what
    assert max(err) <= bd, what
    for e, E in zip(excl, EXCL):
        if E == 0:
            assert same_bits(e, 0.0), what
    if HV == 0:
        assert same_bits(hv, 0.0), what


def check_real(A, members, lo, ref, what, host=True):
    want = R.exact_fraction(A, members, lo, ref)
    M = len(A) if members is None else len(members)
    vol = hv_ref.volume(lo, ref)
    got = device_call(A, members, lo, ref)
    within_bound(got, want, M, vol, what + " device entry")
    if host:
        h = host_call(A, members, lo, ref)
        assert same_bits(h[0], got[0]) and same_bits(h[1], got[1]) and h[2] == got[2], what + " host entry"
    return got, want


BOXES = {1: (np.array([-2.5]), np.array([0.75])),
         2: (np.array([0.125, -1e-3]), np.array([3.0, 1e3])),
         3: (np.array([-3.0, 2.0, 1e-4]), np.array([-3.0 + 1e-3, 2.0 + 1e3, 7.0]))}   # lo != 0, widths 1e6 apart


def members_in(k, M, seed):
    """M rows inside and a little outside the box of BOXES[k]: some clip, some are inactive"""
    lo, ref = BOXES[k]
    u = np.random.default_rng(seed).random((M, k)) * 1.25 - 0.1
    u[0] = 0.25 + 0.5 * (u[0] + 0.1) / 1.25      # the first row strictly inside: something is always active
    return lo + u * (ref - lo)


# ---- real-valued members against exact rational arithmetic ------------------------------------
@pytest.mark.parametrize("k,M", [(k, M) for k in (1, 2) for M in (1, 2, 3, 63, 64, 65)] + [(3, M) for M in (1, 2, 17, 48)])
def test_real_members(gpu, k, M):
    lo, ref = BOXES[k]
    # M <= 48 for the Fraction grid in three axes; one and two axes stay cheap at 65
    got, want = check_real(members_in(k, M, 100 * k + M), None, lo, ref, "k = %d, M = %d" % (k, M))
    assert 0 < got[0] <= hv_ref.volume(lo, ref)


def test_real_members_unit_cube_and_against_the_2d_and_ie_references(gpu):
    rng = np.random.default_rng(5)
    A = rng.random((40, 2))
    got, want = check_real(A, None, np.zeros(2), np.ones(2), "unit square")
    assert abs(hv_ref.exact_2d(A, None, np.zeros(2), np.ones(2)) - got[0]) <= 1e-13
    B = rng.random((10, 3))
    got, want = check_real(B, None, np.zeros(3), np.ones(3), "unit cube")
    assert abs(hv_ref.exact_ie(B, None, np.zeros(3), np.ones(3)) - got[0]) <= 1e-13


# ---- lattice members: every operation is exact, so there is no tolerance ----------------------
@pytest.fixture(scope="module")
def lattice3():
    rng = np.random.default_rng(11)
    I = np.stack([rng.integers(0, 32, 5000), rng.integers(0, 32, 5000), rng.integers(0, 512, 5000)], axis=1)
    return I, R.exact_lattice(I, None, [0, 0, 0], [32, 32, 512])


def check_lattice(I, members, ilo, iref, want, scale=1.0, shift=0.0, what=""):
    k = I.shape[1]
    A = I.astype(np.float64) * scale + shift
    lo, ref = np.asarray(ilo, dtype=np.float64) * scale + shift, np.asarray(iref, dtype=np.float64) * scale + shift
    hv, excl, na = device_call(A, members, lo, ref)
    cell = scale ** k
    assert na == want[2], what
    assert hv == want[0] * cell, what
    np.testing.assert_array_equal(excl, want[1].astype(np.float64) * cell, what)
    return hv, excl, na


def test_lattice_3d_group_wrap_and_chunk_carry(gpu, lattice3):
    I, want = lattice3
    assert len(np.unique(I[:, 2])) == 512 and want[2] == 5000 and (want[1] > 0).sum() > 10
    check_lattice(I, None, [0, 0, 0], [32, 32, 512], want, what="lattice")
    # scaled by 2^-9 with lo = -3: still exact
    check_lattice(I, None, [0, 0, 0], [32, 32, 512], want, scale=2.0 ** -9, shift=-3.0, what="scaled lattice")


def test_lattice_2d_runs_across_many_chunks(gpu):
    rng = np.random.default_rng(12)
    x = rng.permutation(4000)
    # a staircase that descends slowly with noise: holders keep their columns over several 64-lane chunks
    y = np.clip(1000 - x // 4 + rng.integers(0, 200, 4000), 0, 1023)
    I = np.stack([x, y], axis=1)
    want = R.exact_lattice(I, None, [0, 0], [4000, 1024])
    assert (want[1] > 0).sum() > 20
    check_lattice(I, None, [0, 0], [4000, 1024], want, what="k = 2 lattice")
    mem = rng.permutation(4000)[:3000]
    check_lattice(I, mem, [0, 0], [4000, 1024], R.exact_lattice(I, mem, [0, 0], [4000, 1024]), what="k = 2 lattice, members")


def test_lattice_one_holder_of_every_column(gpu):
    """a single dominating point plus dominated ones: the longest run, over every chunk of every slab"""
    rng = np.random.default_rng(13)
    I = np.stack([rng.integers(1, 32, 3000), rng.integers(1, 32, 3000), rng.integers(1, 300, 3000)], axis=1)
    I[1234] = 0
    want = R.exact_lattice(I, None, [0, 0, 0], [32, 32, 300])
    assert want[0] == 32 * 32 * 300 and want[1][1234] > 0
    hv, excl, na = check_lattice(I, None, [0, 0, 0], [32, 32, 300], want, what="one holder")
    assert np.count_nonzero(excl) == 1


# ---- values -----------------------------------------------------------------------------------
def test_special_values(gpu):
    from mpct import _lib
    from mpct.engine import MpctError, hypervolume_exact

    nan, inf = np.nan, np.inf
    lo, ref = np.array([0.0, -1.0, 2.0]), np.array([4.0, 1.0, 4.0])   # dyadic: every operation below is exact
    A = np.array([[1.0, 0.0, 3.0],        # 0 ordinary
                  [nan, 0.0, 2.5],        # 1 a NaN row
                  [2.0, -0.5, 2.5],       # 2 ordinary
                  [inf, 0.0, 2.5],        # 3 +inf: inactive
                  [-inf, 0.5, 3.5],       # 4 -inf clips to lo
                  [-0.0, 0.75, 3.75],     # 5 -0.0 equals lo's +0.0
                  [3.0, 1.0, 2.0],        # 6 exactly on a reference face: inactive
                  [0.5, -0.75, 3.5],      # 7 one of two equal vectors
                  [0.5, -0.75, 3.5],      # 8 the other
                  [3.5, 0.5, 3.875]])     # 9 dominated by 0
    mem = np.array([0, 1, -1, 2, 3, 4, 5, 6, 7, 8, 9, 2, -1], dtype=np.int32)   # -1 entries, index 2 twice
    want = R.exact_fraction(A, mem, lo, ref)
    got = device_call(A, mem, lo, ref)
    assert got[2] == want[2] == 8
    assert Fraction(got[0]) == want[0]
    assert [Fraction(float(e)) for e in got[1]] == want[1]
    assert all(same_bits(got[1][m], 0.0) for m in (1, 2, 4, 7, 8, 9, 10, 12))
    assert all(same_bits(got[1][m], 0.0) for m in (3, 11))           # the duplicated index: each copy owns nothing
    h = host_call(A, mem, lo, ref)
    assert same_bits(h[0], got[0]) and same_bits(h[1], got[1]) and h[2] == got[2]
    # an entry outside [0, C): skipped by the device entry, MPCT_EINVAL for the host entry
    bad = mem.copy()
    bad[2] = 10
    again = device_call(A, bad, lo, ref)
    assert same_bits(again[0], got[0]) and same_bits(again[1], got[1]) and again[2] == got[2]
    with pytest.raises(MpctError, match="members"):
        hypervolume_exact(A, members=bad, lo=lo, ref=ref, device=0)
    # a member below lo in every axis owns the whole box: hv = vol bit for bit, whatever else is there
    B = np.vstack([A, [[-5.0, -7.0, 1.0]]])
    hv, excl, na = device_call(B, None, lo, ref)
    assert same_bits(hv, hv_ref.volume(lo, ref)) and na == 8 and np.count_nonzero(excl) == 1 and excl[10] > 0
    for k in (1, 2, 3):     # and alone in a box of any widths
        l, r = BOXES[k]
        hv, excl, na = device_call(np.full((1, k), -1e300), None, l, r)
        assert same_bits(hv, hv_ref.volume(l, r)) and same_bits(excl, [hv]) and na == 1
    # signed zeros in lo: the corner covers the whole box
    for a, l in ((-0.0, 0.0), (0.0, -0.0)):
        hv, excl, na = device_call(np.array([[a, a]]), None, np.array([l, l]), np.array([1.0, 2.0]))
        assert same_bits(hv, 2.0) and same_bits(excl, [2.0]) and na == 1
    # nothing active: +0.0 and 0; the bad box: NaN
    hv, excl, na = device_call(A, [1, 3, 6, -1], lo, ref)
    assert same_bits(hv, 0.0) and same_bits(excl, np.zeros(4)) and na == 0
    for l, r in ((np.array([0.0, 1.0, 2.0]), ref), (np.array([0.0, nan, 2.0]), ref), (lo, np.array([4.0, inf, 4.0]))):
        hv, excl, na = device_call(A, mem, l, r)
        assert np.isnan(hv) and np.isnan(excl).all() and na == 0
    # four columns are MPCT_ERANGE, never the estimator
    device_call(np.zeros((4, 4)), None, np.zeros(4), np.ones(4), want_rc=-4)
    assert "MPCT_HVX_MAX_OBJ" in _lib.last_error()


def test_front_buffer_of_a_pareto_call(gpu):
    """the -1-padded front of mpct_pareto_device passed as it is with M = C, without leaving the device"""
    import torch
    from mpct.engine import pareto_device

    A = np.random.default_rng(21).random((700, 3))
    A[9, 1] = np.nan
    t = torch.from_numpy(A).cuda()
    out = dict(front=torch.empty(700, dtype=torch.int32, device="cuda"), n_front=torch.empty(1, dtype=torch.int32, device="cuda"))
    pareto_device(t, out)
    lo, ref = np.zeros(3), np.ones(3)
    got = device_call(A, None, lo, ref, dev_members=out["front"])
    front = out["front"].cpu().numpy()
    nf = int(out["n_front"].item())
    assert 3 < nf < 200 and (front[nf:] == -1).all() and got[2] == nf
    assert same_bits(got[1][nf:], np.zeros(700 - nf)) and (got[1][:nf] > 0).all()
    every = device_call(A, None, lo, ref)
    off = np.setdiff1d(np.arange(700), front[:nf])
    assert every[2] == 699 and same_bits(every[1][off], np.zeros(off.size))   # off the front: exactly +0.0
    bd = float(R.bound(700, 1.0))
    assert abs(every[0] - got[0]) <= 2 * bd                                   # each within the bound of HV
    # a dominated candidate takes from the exclusive volume of the one member that dominates it, never adds to one
    assert (every[1][front[:nf]] <= got[1][:nf] + 2 * bd).all()
    sw = R.sweep_numpy(A, front, lo, ref)
    assert abs(sw[0] - got[0]) <= 2 * bd and sw[2] == nf


# ---- call variants ----------------------------------------------------------------------------
def test_output_subsets(gpu):
    A = members_in(3, 150, 31)
    lo, ref = BOXES[3]
    mem = np.random.default_rng(2).permutation(150)[:100].astype(np.int32)
    full = device_call(A, mem, lo, ref)
    n = 0
    for m in range(1, 4):
        for fields in itertools.combinations(FIELDS, m):
            got = device_call(A, mem, lo, ref, fields=fields)
            for f, g, w in zip(FIELDS, got, full):
                assert (g is None) == (f not in fields)
                if g is not None:
                    assert same_bits(g, w) if f != "n_active" else g == w
            n += 1
    assert n == 7


def test_repeat_rows_permutation_streams_and_host(gpu):
    import torch

    rng = np.random.default_rng(41)
    lo, ref = BOXES[3]
    A = members_in(3, 300, 41)
    g = np.abs(rng.standard_normal((150, 3)))             # half of them on a front: many members with a contribution
    A[100:250] = lo + 0.5 * (1.0 - g / np.linalg.norm(g, axis=1, keepdims=True)) * (ref - lo)
    A[7] = A[200]                                         # equal vectors
    assert np.count_nonzero(R.sweep_numpy(A, None, lo, ref)[1]) > 15
    first = device_call(A, None, lo, ref)
    again = device_call(A, None, lo, ref)
    assert same_bits(first[0], again[0]) and same_bits(first[1], again[1]) and first[2] == again[2]
    assert first[2] > 100 and np.count_nonzero(first[1]) > 15
    # the same members at other rows of a larger table
    where = rng.permutation(1000)[:300]
    big = rng.random((1000, 3))
    big[where] = A
    moved = device_call(big, where, lo, ref)
    assert same_bits(moved[0], first[0]) and same_bits(moved[1], first[1]) and moved[2] == first[2]
    # a permutation of members permutes excl bit for bit and leaves hv as it is
    p = rng.permutation(300)
    perm = device_call(A, p, lo, ref)
    assert same_bits(perm[0], first[0]) and same_bits(perm[1], first[1][p]) and perm[2] == first[2]
    # two streams at once
    B = members_in(2, 500, 42)
    lb, rb = BOXES[2]
    want_b = device_call(B, None, lb, rb)
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    ca, keep_a = device_call(A, None, lo, ref, stream=s1, sync=False)
    cb, keep_b = device_call(B, None, lb, rb, stream=s2, sync=False)
    s1.synchronize()
    s2.synchronize()
    for got, want in ((ca(), first), (cb(), want_b)):
        assert same_bits(got[0], want[0]) and same_bits(got[1], want[1]) and got[2] == want[2]
    # the host entry right after a device entry that has not been waited for
    cc, keep_c = device_call(A, None, lo, ref, sync=False)
    h = host_call(B, None, lb, rb)
    assert same_bits(h[0], want_b[0]) and same_bits(h[1], want_b[1]) and h[2] == want_b[2]
    torch.cuda.synchronize()
    got = cc()
    assert same_bits(got[0], first[0]) and same_bits(got[1], first[1])


def test_dist_gpu_path(gpu):
    import torch
    from mpct.dist import hypervolume_exact_candidates, pareto_candidates

    A = np.random.default_rng(51).random((400, 3))
    A[4, 1] = np.nan
    t = torch.from_numpy(A).cuda()
    front = pareto_candidates(t)["front"]
    lo, ref = np.zeros(3), np.ones(3)
    got = hypervolume_exact_candidates(t, front, lo=lo, ref=ref)
    cpu = hypervolume_exact_candidates(t.cpu(), front.cpu(), lo=lo, ref=ref)
    bd = 2 * float(R.bound(front.numel(), 1.0))
    assert got["n_active"] == cpu["n_active"] > 3 and abs(got["hv"] - cpu["hv"]) <= bd
    np.testing.assert_allclose(got["excl"].cpu().numpy(), cpu["excl"].numpy(), rtol=0, atol=bd)


# ---- the estimator against the exact value ----------------------------------------------------
def test_estimator_against_the_exact_value(gpu):
    """the first check of mpct_hypervolume that does not share its sample points: n_covered / N and every
    excl[m] / N within 6 sigma of the binomial (plus 1 / N) of the exact fractions"""
    from mpct.engine import hypervolume, hypervolume_exact

    A = np.random.default_rng(61).random((200, 3))
    lo, ref = np.zeros(3), np.array([1.0, 1.25, 1.5])
    N = 1 << 20
    ex = hypervolume_exact(A, lo=lo, ref=ref, device=0)
    mc = hypervolume(A, lo=lo, ref=ref, n_samples=N, seed=17, device=0)
    assert ex.vol == mc.volume

    def ok(count, exact):
        p = exact / ex.vol
        return abs(count / N - p) <= 6.0 * np.sqrt(p * (1.0 - p) / N) + 1.0 / N

    print("exact hv %.9g, estimate %.9g; %d members with a contribution" % (ex.hv, mc.hv, np.count_nonzero(ex.excl)))
    assert ok(mc.n_covered, ex.hv)
    bad = [m for m in range(200) if not ok(int(mc.excl[m]), float(ex.excl[m]))]
    assert not bad, bad


# ---- end to end -------------------------------------------------------------------------------
def test_shell3x3_front_hypervolume_exact(gpu):
    """Shell 3x3 at 64 candidates: eval_batch -> pareto -> ParetoResult.hypervolume_exact with the default box."""
    from mpct.engine import MpctError, default_box, eval_batch, hypervolume_exact, pareto
    from mpct.scenarios import candidate_grid, shell3x3

    sc, r, yref = shell3x3(n2_max=30, nu_max=5, nit=200)
    N2, Nu, d, l = candidate_grid(64)
    N2[5] = 0                                   # a sentinel: NaN costs
    res = eval_batch(sc, N2, Nu, d, l, r[None], device=0)
    J = res.J1.reshape(64, 3)
    front = pareto(J, device=0)
    got = front.hypervolume_exact(J, device=0)
    lo, ref = default_box(J, front.front)
    np.testing.assert_array_equal(got.lo, lo)
    np.testing.assert_array_equal(got.ref, ref)
    np.testing.assert_array_equal(got.members, front.front)
    b, act, _ = R.clipped(J, front.front, lo, ref)
    M = front.front.size
    assert got.n_active == int(act.sum()) and got.vol == hv_ref.volume(lo, ref)
    rel = (M * M + 8) * 2.0 ** -53
    print("Shell 3x3, 64 candidates: front %d, hv %.9g of a box of %.9g, sum of contributions %.9g"
          % (M, got.hv, got.vol, got.excl.sum()))
    assert 0 < got.hv <= got.vol and got.excl.sum() <= got.hv * (1 + rel) + rel * got.vol
    within_bound((got.hv, got.excl, got.n_active), R.exact_fraction(J, front.front, lo, ref), M, got.vol, "Shell 3x3")
    np.testing.assert_array_equal(got.contribution(), got.excl / got.hv)
    with pytest.raises(MpctError, match="MPCT_HVX_MAX_OBJ"):
        hypervolume_exact(np.hstack([J, J[:, :1]]), members=front.front, device=0)


def test_robust_result_hypervolume_exact(gpu):
    """RobustResult.hypervolume_exact on 12 candidates x 4 model-error draws of shell3x3_mc"""
    import pareto_ref
    from mpct.engine import default_box, eval_robust
    from mpct.scenarios import candidate_grid, shell3x3_mc

    made = shell3x3_mc(draws=4, nit=120)
    sc, refs = made[0], np.ascontiguousarray(made[1])
    N2, Nu, d, l = (x[::5][:12] for x in candidate_grid(64))
    res = eval_robust(sc, N2, Nu, d, l, refs, device=0)
    S = res.scores(0, "worst")
    pf = pareto_ref.pareto_np(S, 0)
    front = pf[2][:pf[3]]
    got = res.hypervolume_exact(stat="worst", device=0)
    lo, ref = default_box(S, front)
    np.testing.assert_array_equal(got.members, front)
    b, act, _ = R.clipped(S, front, lo, ref)
    M = front.size
    assert got.n_active == int(act.sum()) and 0 < got.hv <= got.vol
    assert got.excl.sum() <= got.hv * (1 + (M * M + 8) * 2.0 ** -53) + (M * M + 8) * 2.0 ** -53 * got.vol
    within_bound((got.hv, got.excl, got.n_active), R.exact_fraction(S, front, lo, ref), M, got.vol, "robust")
