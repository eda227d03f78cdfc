"""GPU: mpct_goal_attain_device and mpct_goal_attain against tests/goal_ref.py, every field bit for bit.  The
device entry writes into a guard-filled arena.  Sizes at every place the code branches: the wave, the workgroup
of 256 goal vectors, the LDS tile T, the padded instances K = 4, 8, 16 and the list lengths NB = 1, 4, 16; forced
splits of the candidate range reach the merge stage, partial and empty chunks."""
import ctypes as C
import itertools

import numpy as np
import pytest

import goal_ref as R
from test_goal import HAND, expected, special_case

pytestmark = pytest.mark.gpu
GUARD = 0x5A5A5A5A
PAD = 64
nan, inf = np.nan, np.inf


@pytest.fixture(scope="module")
def gpu(built, has_gpu):
    if not has_gpu:
        pytest.skip("no GPU")
    return True


@pytest.fixture
def grid(gpu):
    """force the split of the candidate range and the tile; the defaults come back afterwards"""
    from mpct import _lib

    lib = _lib.load()

    def force(split, tile=0):
        assert lib.mpct_internal_goal_grid(split, tile) == 0, _lib.last_error()

    yield force
    assert lib.mpct_internal_goal_grid(0, 0) == 0


def geometry(G, Cn):
    """(tile, chunks, candidates per chunk) of the device entry's launch under the current setting"""
    from mpct import _lib

    g = np.zeros(3, dtype=np.int32)
    assert _lib.load().mpct_internal_goal_geometry(int(G), int(Cn), g.ctypes.data_as(_lib.c_int32_p)) == 0
    return int(g[0]), int(g[1]), int(g[2])


def device_call(A, goals, weights, nb, fields=R.FIELDS, stream=None, sync=True):
    """The device entry into one int32 arena [guard | best | guard | gamma | guard | ...]; returns the dict of the
    fields asked for (the others None), after checking that nothing outside them was written."""
    import torch
    from mpct import _lib

    dev = torch.device("cuda", 0)
    A, goals, weights = R._tables(A, goals, weights)
    Cn, k = A.shape
    G = goals.shape[0]
    up = lambda x, rows: torch.from_numpy(np.ascontiguousarray(x)).to(dev) if rows else torch.zeros((1, k), dtype=torch.float64, device=dev)
    t, tg, tw = up(A, Cn), up(goals, G), up(weights, G)
    sizes = dict(best=G * nb, gamma=2 * G * nb, active=G * nb, n_feasible=G, n_attained=G, wins=Cn)
    off, o = {}, PAD
    for f in R.FIELDS:
        off[f] = o
        o += sizes[f] + sizes[f] % 2 + PAD           # even offsets: gamma's doubles stay 8-byte aligned
    arena = torch.full((o,), GUARD, dtype=torch.int32, device=dev)
    ptr = {f: C.c_void_p(arena.data_ptr() + 4 * off[f]) if f in fields else None for f in R.FIELDS}
    r = _lib.MpctGoalResult(*[C.cast(ptr[f], _lib.c_double_p if f == "gamma" else _lib.c_int32_p) if ptr[f] else None
                              for f in R.FIELDS])
    st = (stream or torch.cuda.current_stream(dev)).cuda_stream
    rc = _lib.load().mpct_goal_attain_device(C.c_void_p(t.data_ptr()) if Cn else None, Cn, k, C.c_void_p(tg.data_ptr()) if G else None,
                                             C.c_void_p(tw.data_ptr()) if G else None, G, nb, C.byref(r), C.c_void_p(st))
    assert rc == 0, _lib.last_error()

    def collect():
        a = arena.cpu().numpy()
        mask = np.ones(a.size, dtype=bool)
        for f in fields:
            mask[off[f]:off[f] + sizes[f]] = False
        assert (a[mask] == GUARD).all(), "the call wrote outside its outputs"
        got = {f: None for f in R.FIELDS}
        for f in fields:
            x = a[off[f]:off[f] + sizes[f]].copy()
            if f == "gamma":
                x = x.view(np.float64)
            got[f] = x.reshape(G, nb) if f in ("best", "gamma", "active") else x
        return got

    if not sync:
        return collect, (t, tg, tw, arena)   # keep the tensors alive until the caller has synchronised
    torch.cuda.synchronize(dev)
    return collect()


def host_call(A, goals, weights, nb):
    from mpct.engine import goal_attain

    A, goals, weights = R._tables(A, goals, weights)
    res = goal_attain(A, goals, weights, n_best=nb, device=0)
    return {f: getattr(res, f) for f in R.FIELDS}


def valid_only(goals, weights):
    keep = np.array([R.valid_goal(goals[g], weights[g]) for g in range(len(goals))], dtype=bool)
    return goals[keep], weights[keep], keep


def check(A, goals, weights, nb, what=""):
    """the device entry on every goal vector, the host entry on the valid ones (it rejects the others), against
    the reference; returns the reference"""
    want = R.goal_np(A, goals, weights, nb)
    got = device_call(A, goals, weights, nb, fields=R.FIELDS if nb else R.FIELDS[3:])
    R.compare(got, want, what + " device entry")
    gv, wv, keep = valid_only(*R._tables(A, goals, weights)[1:])
    wh = {f: (v if f == "wins" else v[keep]) for f, v in want.items()}
    R.compare(host_call(A, gv, wv, nb), wh, what + " host entry")
    return want


# ---- hand-made tables -------------------------------------------------------------------------
@pytest.mark.parametrize("case", HAND, ids=[c[0] for c in HAND])
def test_hand_made_tables(gpu, case):
    name, A, goals, weights, nb, want = case
    R.compare(device_call(np.array(A), goals, weights, nb), expected(want), name)


# ---- sizes at every place the code branches ---------------------------------------------------
def test_geometry(gpu, grid):
    T, split, chunk = geometry(1, 65536)
    assert T == 256 and chunk % T == 0 and split * chunk >= 65536 and split > 1     # one goal vector still fills the machine
    assert geometry(1 << 20, 65536)[1] == 1                                          # many goal vectors: no split, no merge
    assert geometry(300, 0)[1:] == (1, T) and geometry(300, 100)[1:] == (1, T)
    grid(7)
    assert geometry(300, 600) == (256, 7, 256)                                       # 256, 256, 88 and four empty chunks
    grid(2, 128)
    assert geometry(300, 600) == (128, 2, 384)


@pytest.mark.parametrize("Cn", [0, 1, 2, 63, 64, 65, 255, 256, 257, 1000])
def test_candidate_counts(gpu, Cn):
    """0, 1, 2, the wave and the tile T = 256 at T - 1, T, T + 1; 1,000: four tiles, the last partial"""
    assert geometry(1, 1000)[0] == 256
    A, goals, weights = special_case(Cn, 3, 4, 70)
    want = check(A, goals, weights, 5, "C = %d" % Cn)
    if Cn >= 63:
        assert (want["n_feasible"] > 5).any()        # full rows
    assert (want["best"] == -1).any()                # and padded ones


@pytest.mark.parametrize("G", [0, 1, 2, 63, 64, 65, 255, 256, 257, 300])
def test_goal_vector_counts(gpu, G):
    """0, 1, 2, the wave and the workgroup of 256 goal vectors at 255, 256, 257; 300: two workgroups"""
    A, goals, weights = special_case(130, 3, 4, G)
    want = check(A, goals, weights, 2, "G = %d" % G)
    assert want["wins"].sum() == (want["n_feasible"] > 0).sum()


@pytest.mark.parametrize("k", [1, 2, 3, 7, 8, 9, 16])
def test_objective_counts(gpu, k):
    """both sides of every padded instance K = 4, 8, 16"""
    A, goals, weights = special_case(270, k, 3, 40)
    check(A, goals, weights, 4, "k = %d" % k)


@pytest.mark.parametrize("nb", [0, 1, 2, 4, 5, 16])
def test_list_lengths(gpu, nb, grid):
    """both sides of every list instance NB = 1, 4, 16, with n_best above n_feasible for the padding, in one chunk
    and through the merge"""
    A, goals, weights = special_case(300, 3, 4, 66)
    check(A, goals, weights, nb, "n_best = %d" % nb)
    grid(3)
    check(A, goals, weights, nb, "n_best = %d, split 3" % nb)
    few = A[:7]                                      # fewer candidates than n_best for every goal vector
    check(few, goals, weights, nb, "n_best = %d, C = 7" % nb)


# ---- ties and special values ------------------------------------------------------------------
def test_ties_and_special_values(gpu, grid):
    """costs on two levels so that nearly every key ties, duplicate rows, NaN rows, +-INFINITY, -INFINITY in a soft
    column, signed zeros, +INFINITY goals on hard columns and the weights 3, 7, 0.1, 1e-300, 1e300"""
    A = R.generated(700, 4, 2)
    A[3, 0] = nan
    A[64, 3] = nan
    A[100] = nan
    A[7] = inf
    A[8] = -inf
    A[9] = -inf
    A[10, 1] = inf
    A[11, 2] = -inf
    A[300:320] = A[20:40]
    A[400:410] = -0.0
    A[410:420] = 0.0
    goals, weights = R.goal_vectors(96, 4, 2, seed=5)
    goals[0], weights[0] = [0.0, -0.0, 0.0, 0.25], [3.0, 7.0, 0.1, 1e-300]
    goals[1], weights[1] = [0.25, 0.0, inf, inf], [1e300, 1e-300, 0.0, 0.0]
    goals[2], weights[2] = [-0.0, 0.0, 0.0, 0.0], [1.0, 1.0, 1.0, 1.0]          # gamma = +-0.0 for the zero rows
    goals[3], weights[3] = [0.0, 0.0, 0.0, -inf], [1.0, 0.0, 0.0, 0.0]          # only -INFINITY passes the hard column
    want = check(A, goals, weights, 16, "special values")
    assert want["n_feasible"].max() <= 700 - 3 and want["n_feasible"][3] == 2 and want["best"][3, :3].tolist() == [8, 9, -1]
    assert np.isinf(want["gamma"]).any() and (want["gamma"] == 0.0).any()
    assert (want["n_feasible"][:3] > 100).all()                                 # the ties are many
    grid(5)
    R.compare(device_call(A, goals, weights, 16), want, "special values, split 5")
    B = R.generated(257, 3, 4)
    B[:, 1] = nan                                                               # every candidate invalid
    g2, w2 = R.goal_vectors(10, 3, 4)
    want = check(B, g2, w2, 2, "all invalid")
    assert (want["n_feasible"] == 0).all() and want["wins"].sum() == 0 and (want["best"] == -1).all()


def test_division_is_correctly_rounded(gpu):
    """one candidate, one objective: gamma = (F - goal) * (1 / w) for weights whose reciprocal is inexact"""
    w = np.array([3.0, 7.0, 0.1, 1e-300, 1e300, 1.1, 1e-308, 1.7976931348623157e308, 2.2250738585072014e-308, 49.0, 1 / 3])
    A = np.array([[1.5]])
    goals = np.full((w.size, 1), 0.25)
    want = check(A, goals, w.reshape(-1, 1), 1, "division")
    np.testing.assert_array_equal(want["gamma"][:, 0], 1.25 * (1.0 / w))


def test_invalid_goal_vectors_interleaved(gpu, grid):
    """negative, NaN, subnormal, all-zero and infinite weights and bad goals between valid vectors: -1 / NaN rows,
    -1 counts, no win; the valid rows as without them"""
    A = R.generated(300, 3, 4)
    goals, weights = R.goal_vectors(70, 3, 4, seed=2)
    clean = R.goal_np(A, goals, weights, 4)
    bad = list(range(1, 70, 3))
    for n, g in enumerate(bad):
        R.spoil(goals, weights, g, R.INVALID[n % len(R.INVALID)])
    for split in (0, 2):
        grid(split)
        got = device_call(A, goals, weights, 4)
        R.compare(got, R.goal_np(A, goals, weights, 4), "interleaved, split %d" % split)
        ok = np.setdiff1d(np.arange(70), bad)
        for f in R.FIELDS[:5]:
            assert got[f][ok].tobytes() == clean[f][ok].tobytes(), f
        assert (got["n_feasible"][bad] == -1).all() and (got["n_attained"][bad] == -1).all()
        assert (got["best"][bad] == -1).all() and np.isnan(got["gamma"][bad]).all() and (got["active"][bad] == -1).all()
        assert got["wins"].sum() == (clean["n_feasible"][ok] > 0).sum()


# ---- geometry ---------------------------------------------------------------------------------
def test_every_geometry_equals_split_1(gpu, grid):
    """splits 1, 2 and 7 of 600 candidates and 9 (more chunks than tiles: empty chunks), tile 128 as well: bitwise
    what one chunk gives"""
    A, goals, weights = special_case(600, 7, 3, 300)
    grid(1)
    one = device_call(A, goals, weights, 16)
    R.compare(one, R.goal_np(A, goals, weights, 16), "split 1")
    for split, tile in ((2, 0), (7, 0), (9, 0), (1, 128), (3, 128), (9, 128), (0, 0)):
        grid(split, tile)
        got = device_call(A, goals, weights, 16)
        for f in R.FIELDS:
            assert got[f].tobytes() == one[f].tobytes(), (split, tile, f)


# ---- call variants ----------------------------------------------------------------------------
def test_output_subsets(gpu, grid):
    A, goals, weights = special_case(513, 3, 4, 40)
    want = R.goal_np(A, goals, weights, 4)
    subsets = [s for m in (1, 2, 5) for s in itertools.combinations(R.FIELDS, m)]
    assert len(subsets) == 6 + 15 + 6
    for n, fields in enumerate(subsets):
        grid(n % 3)                                  # default, one chunk, two chunks in turn
        R.compare(device_call(A, goals, weights, 4, fields=fields), want, "+".join(fields))
    grid(0)
    for fields in (("n_feasible",), ("wins",), ("n_attained", "wins")):
        R.compare(device_call(A, goals, weights, 0, fields=fields), want, "n_best 0: " + "+".join(fields), fields=fields)


def test_repeated_and_permuted(gpu):
    A, goals, weights = special_case(1025, 4, 3, 200)
    first = device_call(A, goals, weights, 5)
    R.compare(first, R.goal_np(A, goals, weights, 5), "first")
    again = device_call(A, goals, weights, 5)
    for f in R.FIELDS:
        assert first[f].tobytes() == again[f].tobytes(), f
    for perm in (np.arange(200)[::-1].copy(), np.random.default_rng(3).permutation(200)):
        got = device_call(A, goals[perm], weights[perm], 5)
        for f in R.FIELDS[:5]:
            assert got[f].tobytes() == first[f][perm].tobytes(), f
        assert got["wins"].tobytes() == first["wins"].tobytes()
    assert first["wins"].sum() == (first["n_feasible"] > 0).sum()


def test_two_streams_then_host(gpu):
    import torch

    A, ga, wa = special_case(2049, 3, 4, 150)
    B, gb, wb = special_case(1500, 7, 3, 300)
    gbv, wbv, _ = valid_only(gb, wb)
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    ca, keep_a = device_call(A, ga, wa, 4, stream=s1, sync=False)
    cb, keep_b = device_call(B, gb, wb, 16, stream=s2, sync=False)
    s1.synchronize()
    s2.synchronize()
    R.compare(ca(), R.goal_np(A, ga, wa, 4), "stream 1")
    R.compare(cb(), R.goal_np(B, gb, wb, 16), "stream 2")
    # the host entry right after a device entry that has not been waited for
    cc, keep_c = device_call(A, ga, wa, 4, sync=False)
    R.compare(host_call(B, gbv, wbv, 16), R.goal_np(B, gbv, wbv, 16), "host after device")
    torch.cuda.synchronize()
    R.compare(cc(), R.goal_np(A, ga, wa, 4), "device before host")


def test_host_entry_broadcasts_one_vector(gpu):
    from mpct.engine import goal_attain

    A = R.generated(400, 3, 5)
    w = np.array([[1.0, 2.0, 0.0], [3.0, 0.0, 0.0], [0.1, 7.0, 1.0]])
    res = goal_attain(A, [0.25, 0.5, 0.75], w, n_best=3, device=0)
    R.compare({f: getattr(res, f) for f in R.FIELDS}, R.goal_np(A, np.tile([0.25, 0.5, 0.75], (3, 1)), w, 3), "broadcast goals")
    assert res.winners().tolist() == sorted(set(res.best[:, 0].tolist()) - {-1}, key=lambda c: (-res.wins[c], c))


def test_dist_gpu_path(gpu):
    import torch
    from mpct.dist import goal_attain_candidates

    A, goals, weights = special_case(700, 3, 4, 90)
    for nb in (3, 0):
        want = R.goal_np(A, goals, weights, nb)
        got = goal_attain_candidates(torch.from_numpy(A).cuda(), goals, weights, n_best=nb)
        R.compare({f: v.cpu().numpy() for f, v in got.items()}, want, "dist GPU path, n_best %d" % nb)
        cpu = goal_attain_candidates(torch.from_numpy(A), goals, weights, n_best=nb)
        for f in R.FIELDS:
            assert cpu[f].numpy().tobytes() == got[f].cpu().numpy().tobytes(), f


# ---- end to end -------------------------------------------------------------------------------
def test_shell3x3_indices_goal_attain(gpu):
    """eval_indices on Shell 3x3 at 64 candidates, then goal_attain with one hard overshoot bound: IAE against
    valve travel among the candidates whose overshoot stays under the bound."""
    from mpct.engine import eval_indices
    from mpct.scenarios import candidate_grid, shell3x3

    sc, r, yref = shell3x3(n2_max=30, nu_max=5, nit=200)
    N2, Nu, d, l = candidate_grid(64)
    idx = eval_indices(sc, N2, Nu, d, l, r[None], fields=("iae", "over", "tv"), device=0)
    names = ("iae", "tv", "over")
    T = idx.costs(names)
    assert T.shape == (64, 3) and np.isfinite(T).all(axis=1).sum() >= 32
    bound = float(np.nanmedian(T[:, 2]))
    goals = np.array([[np.nanmin(T[:, 0]), np.nanmin(T[:, 1]), bound]] * 3)
    weights = np.array([[1.0, 1.0, 0.0], [1.0, 0.1, 0.0], [0.1, 1.0, 0.0]]) * np.array([np.nanmax(T[:, 0]), np.nanmax(T[:, 1]), 1.0])
    want = R.goal_np(T, goals, weights, 4)
    got = idx.goal_attain(names, goals, weights, n_best=4, device=0)
    R.compare({f: getattr(got, f) for f in R.FIELDS}, want, "Shell 3x3 indices")
    print("Shell 3x3, 64 candidates, overshoot <= %.4g: %d feasible, best %s" % (bound, want["n_feasible"][0], want["best"][:, 0]))
    assert 1 <= want["n_feasible"][0] < 64 and (T[want["best"][:, 0], 2] <= bound).all()


def test_robust_result_goal_attain_shell3x3_mc(gpu):
    """RobustResult.goal_attain on shell3x3_mc at 12 candidates x 4 draws with a cost bound that fails some draws:
    the table RobustResult builds, selected on the device, against the reference on the same table; a candidate
    over max_failed is feasible for no goal vector."""
    from mpct.engine import eval_robust
    from mpct.scenarios import candidate_grid, shell3x3_mc

    made = shell3x3_mc(draws=4, nit=120)
    sc, refs = made[0], np.ascontiguousarray(made[1])
    N2, Nu, d, l = (x[::5][:12] for x in candidate_grid(64))
    free = eval_robust(sc, N2, Nu, d, l, refs, want_J1=True, device=0)
    J = free.J1.reshape(12, 4, -1).sum(axis=2)
    worst = np.where(np.isfinite(J), J, np.inf).max(axis=1)
    assert np.isfinite(worst).sum() >= 6
    jb = float(np.median(worst[np.isfinite(worst)]))     # about half of the candidates lose a draw to this bound
    res = eval_robust(sc, N2, Nu, d, l, refs, j_bound=jb, device=0)
    assert (res.n_failed > 0).sum() >= 3 and (res.n_failed == 0).sum() >= 3
    for stat, mf in (("worst", 0), ("mean", 1)):
        S = res.scores(mf, stat)
        k = S.shape[1]
        over = np.flatnonzero(res.n_failed > mf)
        assert over.size and np.isnan(S[over]).all()
        goals = np.tile(np.nanmin(S, axis=0), (3, 1))
        weights = np.ones((3, k)) * np.nanmax(S, axis=0)
        weights[1, 0], goals[1, 0] = 0.0, np.nanmedian(S[:, 0])          # a hard bound on the first output
        weights[2, 1:] = 0.0
        goals[2, 1:] = np.inf                                            # no constraint: the best first output
        want = R.goal_np(S, goals, weights, 3)
        got = res.goal_attain(goals, weights, n_best=3, stat=stat, max_failed=mf, device=0)
        R.compare({f: getattr(got, f) for f in R.FIELDS}, want, "shell3x3_mc %s" % stat)
        assert not set(got.best.ravel().tolist()) & set(over.tolist())
        assert got.n_feasible[0] == (~np.isnan(S).any(axis=1)).sum() and 1 <= got.n_feasible[1] < got.n_feasible[0]
        assert got.best[2, 0] == np.nanargmin(S[:, 0])


def test_robust_result_goal_attain(gpu):
    """RobustResult.goal_attain on config 4 at 12 candidates x 5 draws with a bound that fails some draws: a
    candidate over max_failed is feasible for no goal vector."""
    from test_robust_tail_gpu import call, config4_case

    sc, refs, v, q, jb = config4_case(5)
    res = call(sc, q, refs, v, jb, levels=(0.5, 1.0), want_J1=False)
    assert (res.n_failed > 0).any() and (res.n_failed == 0).any()
    for stat, mf in (("worst", 0), ("mean", 2)):
        S = res.scores(mf, stat)
        k = S.shape[1]
        goals = np.tile(np.nanmin(S, axis=0), (2, 1))
        weights = np.ones((2, k))
        weights[1, 0] = 0.0
        goals[1, 0] = np.nanmedian(S[:, 0])
        want = R.goal_np(S, goals, weights, 3)
        got = res.goal_attain(goals, weights, n_best=3, stat=stat, max_failed=mf, device=0)
        R.compare({f: getattr(got, f) for f in R.FIELDS}, want, "RobustResult %s" % stat)
        over = np.flatnonzero(res.n_failed > mf)
        assert over.size and not set(got.best.ravel().tolist()) & set(over.tolist())
        assert got.n_feasible[0] == (res.n_failed <= mf).sum()
