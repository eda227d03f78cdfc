"""GPU: mpct_pareto_device and mpct_pareto against tests/pareto_ref.py, exactly (every result is an
integer).  Every case runs both entries, the device entry into a guard-filled arena, at the sizes where
the code branches: the workgroup (256 candidates), the LDS tile, the chunks of the split competitor range
and both sides of every padded instance K = 2, 4, 8, 16."""
import ctypes as C
import itertools

import numpy as np
import pytest

import pareto_ref as R

pytestmark = pytest.mark.gpu
GUARD = 0x5A5A5A5A
PAD = 64
FIELDS = ("dom_count", "layer", "front", "n_front")


@pytest.fixture(scope="module")
def gpu(built, has_gpu):
    if not has_gpu:
        pytest.skip("no GPU")
    return True


def grid_of(Cn):
    """(tile, chunks, competitors per chunk) of the device entry's launch for Cn candidates"""
    from mpct import _lib

    g = np.zeros(3, dtype=np.int32)
    assert _lib.load().mpct_internal_pareto_grid(int(Cn), g.ctypes.data_as(_lib.c_int32_p)) == 0
    return int(g[0]), int(g[1]), int(g[2])


def device_call(A, L, fields=FIELDS, stream=None, sync=True, tuned=None):
    """The device entry into one int32 arena [guard | dom_count | guard | layer | guard | front | guard |
    n_front | guard]; returns (dom_count, layer, front, n_front) with None for the fields not asked for,
    after checking that nothing outside the asked-for fields was written."""
    import torch
    from mpct import _lib

    dev = torch.device("cuda", 0)
    A = np.ascontiguousarray(A, dtype=np.float64)
    A = A if A.ndim == 2 else A.reshape(-1, 1)
    Cn, k = A.shape
    t = torch.from_numpy(A).to(dev) if Cn else torch.zeros((1, k), dtype=torch.float64, device=dev)
    sizes = dict(dom_count=Cn, layer=Cn, front=Cn, n_front=1)
    off, o = {}, PAD
    for f in FIELDS:
        off[f] = o
        o += sizes[f] + PAD
    arena = torch.full((o,), GUARD, dtype=torch.int32, device=dev)
    ptr = {f: C.cast(C.c_void_p(arena.data_ptr() + 4 * off[f]), _lib.c_int32_p) if f in fields else None for f in FIELDS}
    r = _lib.MpctParetoResult(*[ptr[f] for f in FIELDS])
    st = (stream or torch.cuda.current_stream(dev)).cuda_stream
    lib = _lib.load()
    if tuned is None:
        rc = lib.mpct_pareto_device(C.c_void_p(t.data_ptr()), Cn, k, L, C.byref(r), C.c_void_p(st))
    else:
        rc = lib.mpct_internal_pareto_tuned(C.c_void_p(t.data_ptr()), Cn, k, L, C.byref(r), C.c_void_p(st), *tuned)
    assert rc == 0, _lib.last_error()

    def collect():
        a = arena.cpu().numpy()
        mask = np.ones(a.size, dtype=bool)
        for f in fields:
            mask[off[f]:off[f] + sizes[f]] = False
        assert (a[mask] == GUARD).all(), "the call wrote outside its outputs"
        got = [a[off[f]:off[f] + sizes[f]].copy() if f in fields else None for f in FIELDS]
        if got[3] is not None:
            got[3] = int(got[3][0])
        return tuple(got)

    if not sync:
        return collect, (t, arena)   # keep the tensors alive until the caller has synchronised
    torch.cuda.synchronize(dev)
    return collect()


def host_call(A, L):
    from mpct.engine import pareto

    A = np.asarray(A, dtype=float)
    A = A if A.ndim == 2 else A.reshape(-1, 1)
    res = pareto(A, max_layers=L, device=0)
    front = np.full(len(A), -1, dtype=np.int32)
    front[:res.front.size] = res.front
    return res.dom_count, res.layer, front, int(res.front.size)


def check(A, L, what=""):
    """both entries against the reference; returns the reference"""
    want = R.pareto_np(A, L)
    R.compare(device_call(A, L), want, what + " device entry")
    R.compare(host_call(A, L), want, what + " host entry")
    return want


# ---- sizes at every place the code branches ---------------------------------------------------
def test_grid_and_tile(gpu):
    T, split, chunk = grid_of(513)
    assert T == 256                                  # the sizes below straddle this tile
    assert (split, chunk) == (3, 256) and 513 % chunk == 1   # the last chunk is partial
    assert grid_of(12001) == (256, 47, 256)          # 47 workgroups of b times 47 chunks of a
    T, split, chunk = grid_of(65536)
    assert chunk == 8 * T and split * chunk == 65536  # config 3's grid: several tiles per chunk


@pytest.mark.parametrize("Cn", [0, 1, 2, 63, 64, 65, 255, 256, 257, 511, 512, 513])
def test_sizes(gpu, Cn):
    """0, 1, 2, the wave, the workgroup and the tile T = 256 at T - 1, T, T + 1 and 2T + 1 (513: the
    competitor range in three chunks, the last one partial), and 2T - 1, 2T."""
    want = check(R.generated(Cn, 3, 4), 4, "C = %d" % Cn)
    if Cn >= 63:
        assert 1 <= want[3] < Cn and want[1].max() == 4      # a front, and candidates beyond the layers asked for


def test_many_workgroups(gpu):
    """12,001 candidates: 47 workgroups of b times 47 chunks of a, the last of each partial."""
    A = R.generated(12001, 2, 50)
    want = check(A, 1, "C = 12001")
    assert want[0].max() > 10000


def test_empty_and_partial_chunks_of_a_forced_split(gpu):
    """600 candidates with five chunks forced: 256, 256, 88 and two empty ones; two chunks of two tiles and
    one of three (the shape of a large grid's chunks); and tile 128."""
    A = R.generated(600, 3, 4)
    want = R.pareto_np(A, 6)
    R.compare(device_call(A, 6, tuned=(256, 5)), want, "split 5")
    R.compare(device_call(A, 6, tuned=(256, 2)), want, "split 2")
    R.compare(device_call(A, 6, tuned=(256, 1)), want, "split 1")
    R.compare(device_call(A, 6, tuned=(128, 3)), want, "tile 128, split 3")
    R.compare(device_call(A, 6, tuned=(128, 0)), want, "tile 128")


@pytest.mark.parametrize("k", [1, 2, 3, 4, 5, 7, 8, 9, 16])
def test_objective_counts(gpu, k):
    """both sides of every padded instance"""
    want = check(R.generated(257, k, 3), 8, "k = %d" % k)
    assert want[3] >= 1


# ---- generated inputs -------------------------------------------------------------------------
@pytest.mark.parametrize("Cn,k,hi,front,layers", [(257, 3, 6, 1, 15), (257, 7, 6, 64, 5), (4097, 7, 6, 83, 14),
                                                  (1025, 1, 6, 158, 6), (1025, 16, 3, 648, 3)])
def test_generated(gpu, Cn, k, hi, front, layers):
    A = R.generated(Cn, k, hi)
    assert R.n_layers(A) == layers           # the case is what it is meant to be
    want = check(A, 16, "%d x %d" % (Cn, k))
    assert want[3] == front
    if (Cn, k) == (4097, 7):
        assert want[0].max() == 2846
    if k == 1:
        assert (A[want[2][:front], 0] == A.min()).all()     # the front is all the minima


@pytest.mark.parametrize("L", [64, 1])
def test_deep_layers(gpu, L):
    """4,097 x 2 with 99 layers: at L = 64 the 'beyond' value is exercised, and at L = 1"""
    A = R.generated(4097, 2, 50)
    assert R.n_layers(A) == 99
    want = check(A, L, "L = %d" % L)
    assert want[3] == 2 and (want[1] == L).any() and want[1].max() == L


# ---- structured inputs ------------------------------------------------------------------------
def test_structured(gpu):
    Cn = 300
    want = check(np.full((Cn, 3), 2.5), 4, "all equal")
    assert want[3] == Cn and (want[0] == 0).all() and (want[1] == 0).all()
    x = np.arange(Cn, dtype=float)
    want = check(np.stack([x, 2 * x, x + 1], axis=1), 7, "total order")
    np.testing.assert_array_equal(want[0], np.arange(Cn))
    np.testing.assert_array_equal(want[1], np.minimum(np.arange(Cn), 7))
    want = check(np.stack([x, Cn - x], axis=1), 3, "antichain")
    assert want[3] == Cn


def test_continuous(gpu):
    A = np.random.default_rng(7).lognormal(size=(4097, 3))
    want = check(A, 40, "lognormal")
    assert want[3] == 39 and want[1].max() == 32 and R.n_layers(A) == 33


# ---- special values ---------------------------------------------------------------------------
def test_special_values(gpu):
    nan, inf = np.nan, np.inf
    A = R.generated(270, 5, 4)              # k = 5 in the K = 8 instance: column 4 is beside the padding
    A[3, 0] = nan
    A[64, 4] = nan                          # the last column, next to the padded ones
    A[65, 2] = nan
    A[100] = nan
    A[7] = inf
    A[8] = -inf                             # dominates every valid row but itself
    A[9] = -inf                             # a duplicate of the front point
    A[10, 1] = inf
    want = check(A, 5, "special")
    for c in (3, 64, 65, 100):
        assert want[0][c] == -1 and want[1][c] == -1 and c not in want[2][:want[3]]
    assert want[2][:want[3]].tolist() == [8, 9] and want[0][7] >= 2
    # -0.0 against +0.0: equal, so neither dominates
    want = check(np.array([[0.0, -0.0], [-0.0, 0.0], [0.0, 1.0]]), 2, "signed zeros")
    assert want[0].tolist() == [0, 0, 2] and want[3] == 2
    # every row invalid
    B = R.generated(257, 3, 4)
    B[:, 1] = nan
    want = check(B, 3, "all invalid")
    assert want[3] == 0 and (want[2] == -1).all() and (want[0] == -1).all() and (want[1] == -1).all()
    # NaN in the first and last column of each padded instance's edge
    for k in (2, 4, 8, 16):
        D = R.generated(130, k, 3)
        D[1, 0] = nan
        D[2, k - 1] = nan
        check(D, 3, "k = %d with NaN" % k)


# ---- call variants ----------------------------------------------------------------------------
def test_output_subsets(gpu):
    from mpct import _lib

    A = R.generated(513, 3, 5)
    want = R.pareto_np(A, 6)
    n = 0
    for m in range(1, 5):
        for fields in itertools.combinations(FIELDS, m):
            if "front" in fields and "n_front" not in fields:
                continue                     # MPCT_EINVAL: tests/test_pareto.py
            R.compare(device_call(A, 6 if "layer" in fields else 0, fields=fields), want, "+".join(fields))
            n += 1
    assert n == 11
    assert _lib.PARETO_MAX_LAYERS == 64


def test_repeated_and_permuted(gpu):
    A = R.generated(1025, 4, 5)
    A[17, 2] = np.nan
    first = device_call(A, 9)
    R.compare(first, R.pareto_np(A, 9), "first")
    again = device_call(A, 9)
    for a, b in zip(first[:3], again[:3]):
        assert a.tobytes() == b.tobytes()
    assert first[3] == again[3]
    for perm in (np.arange(1025)[::-1].copy(), np.random.default_rng(3).permutation(1025)):
        got = device_call(A[perm], 9)
        np.testing.assert_array_equal(got[0], first[0][perm])
        np.testing.assert_array_equal(got[1], first[1][perm])
        assert got[3] == first[3]
        assert set(perm[got[2][:got[3]]].tolist()) == set(first[2][:first[3]].tolist())
        assert (np.diff(got[2][:got[3]]) > 0).all() and (got[2][got[3]:] == -1).all()


def test_two_streams_then_host(gpu):
    import torch

    A, B = R.generated(2049, 3, 6), R.generated(1500, 7, 4)
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    ca, keep_a = device_call(A, 8, stream=s1, sync=False)
    cb, keep_b = device_call(B, 8, stream=s2, sync=False)
    s1.synchronize()
    s2.synchronize()
    R.compare(ca(), R.pareto_np(A, 8), "stream 1")
    R.compare(cb(), R.pareto_np(B, 8), "stream 2")
    # the host entry right after a device entry that has not been waited for
    cc, keep_c = device_call(A, 8, sync=False)
    R.compare(host_call(B, 8), R.pareto_np(B, 8), "host after device")
    torch.cuda.synchronize()
    R.compare(cc(), R.pareto_np(A, 8), "device before host")


def test_dist_gpu_path(gpu):
    import torch
    from mpct.dist import pareto_candidates

    A = R.generated(700, 3, 5)
    A[4, 1] = np.nan
    want = R.pareto_np(A, 5)
    got = pareto_candidates(torch.from_numpy(A).cuda(), max_layers=5)
    np.testing.assert_array_equal(got["dom_count"].cpu().numpy(), want[0])
    np.testing.assert_array_equal(got["layer"].cpu().numpy(), want[1])
    np.testing.assert_array_equal(got["front"].cpu().numpy(), want[2][:want[3]])


# ---- end to end -------------------------------------------------------------------------------
def test_shell3x3_grid_front(gpu):
    """Shell 3x3 at 322 candidates through eval_batch, J1 per output fed to pareto."""
    from mpct.engine import eval_batch, pareto
    from mpct.scenarios import candidate_grid, shell3x3

    sc, r, yref = shell3x3(n2_max=30, nu_max=5, nit=200)
    N2, Nu, d, l = candidate_grid(322)
    N2[5] = 0                                   # a sentinel: NaN costs, an invalid candidate
    res = eval_batch(sc, N2, Nu, d, l, r[None], device=0)
    J = res.J1.reshape(322, 3)
    nvalid = int((~np.isnan(J).any(axis=1)).sum())
    assert np.isnan(J[5]).all() and nvalid >= 300
    want = R.pareto_np(J, 8)
    got = pareto(J, max_layers=8, device=0)
    print("Shell 3x3, 322 candidates: %d valid, front %d, deepest layer asked %d" % (nvalid, want[3], want[1].max()))
    assert 1 <= want[3] < nvalid                 # J1 alone gives a proper front: no need for the (J1, j22) columns
    np.testing.assert_array_equal(got.dom_count, want[0])
    np.testing.assert_array_equal(got.layer, want[1])
    np.testing.assert_array_equal(got.front, want[2][:want[3]])
    assert got.dom_count[5] == -1 and 5 not in got.front


def test_robust_result_pareto(gpu):
    """RobustResult.pareto on config 4 at 12 candidates x 5 draws with a bound that fails some draws:
    candidates over max_failed come back -1; the tail columns join as further objectives."""
    from test_robust_tail_gpu import call, config4_case

    sc, refs, v, q, jb = config4_case(5)
    res = call(sc, q, refs, v, jb, levels=(0.5, 1.0), want_J1=False)
    assert (res.n_failed > 0).any() and (res.n_failed == 0).any()
    for stat, mf in (("worst", 0), ("mean", 2)):
        over = res.n_failed > mf
        assert over.any() and not over.all()
        S = res.scores(mf, stat)
        want = R.pareto_np(S, 4)
        got = res.pareto(stat=stat, max_failed=mf, max_layers=4, device=0)
        np.testing.assert_array_equal(got.dom_count, want[0])
        np.testing.assert_array_equal(got.layer, want[1])
        np.testing.assert_array_equal(got.front, want[2][:want[3]])
        assert (got.dom_count[over] == -1).all() and (got.layer[over] == -1).all()
        assert not set(got.front.tolist()) & set(np.flatnonzero(over).tolist())
    S = np.hstack([res.scores(0, "worst"), res.cvar[:, :1], res.quantile[:, 1:2]])
    S[res.n_failed > 0] = np.nan
    want = R.pareto_np(S, 0)
    got = res.pareto(columns=(("cvar", 0), ("quantile", 1)), device=0)
    np.testing.assert_array_equal(got.dom_count, want[0])
    assert got.layer is None
