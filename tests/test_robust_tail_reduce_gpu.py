"""GPU: robust_tail_kernel alone on synthetic draw records (robust_tail.h; include/mpct.h,
mpct_eval_robust_tail), driven through the library's undeclared hook mpct_internal_robust_tail.

The yardstick is tests/tail_ref.py, a scalar Python restatement of the header's contract.  Every
comparison is bitwise, NaN matched by position; no tolerance appears in this file.  The outputs lie
in one arena of guard bytes, with guard bytes before, between and after the fields, and every byte
outside the fields asked for must stay as it was filled."""
import ctypes as C
import math

import numpy as np
import pytest

from tail_ref import FIELDS, assert_same_tail, bits, tail_ref

pytestmark = [pytest.mark.gpu, pytest.mark.filterwarnings("error::RuntimeWarning")]

MYS = (1, 2, 3, 7)
DS = (1, 2, 3, 63, 64, 65, 127, 128, 129, 1000, 4096)
CS = (1, 3, 4, 5)
EINVAL, ERANGE = -1, -4
INF, NAN = math.inf, math.nan
GUARD = 0xA5
PAD = 256
# eight levels, unsorted, one pair of duplicates: the maximum, a * n an exact integer for even n, the
# next double above it, the lowest rank by clamping
LEVELS8 = (1.0, 0.5, math.nextafter(0.5, 1.0), 0.95, 1e-300, 0.25, 0.95, 0.75)


@pytest.fixture(scope="module")
def gpu(built, has_gpu):
    if not has_gpu:
        pytest.skip("no GPU")
    return True


def _call_hook(Cn, D, my, j_bound, J1_ptr, st_ptr, levels, ptrs, nlev=None):
    import torch
    from mpct import _lib

    lv = None if levels is None else np.ascontiguousarray(levels, dtype=np.float64)
    return _lib.load().mpct_internal_robust_tail(
        Cn, D, my, float(j_bound), C.c_void_p(J1_ptr), C.c_void_p(st_ptr), len(lv) if nlev is None else nlev,
        None if lv is None else lv.ctypes.data_as(_lib.c_double_p), C.c_void_p(ptrs.get("quantile")),
        C.c_void_p(ptrs.get("cvar")), C.c_void_p(ptrs.get("q_draw")), C.c_void_p(torch.cuda.current_stream().cuda_stream))


def tail_on_device(J1, status, j_bound, levels, fields=FIELDS):
    """robust_tail_kernel on records J1 [C, D, my], status [C, D] or None (a NULL pointer).  Returns
    the fields named and asserts that every other byte of the arena still holds GUARD."""
    import torch
    from mpct import _lib

    J1 = np.ascontiguousarray(J1, dtype=np.float64)
    Cn, D, my = J1.shape
    nlev = len(levels)
    dev = torch.device("cuda", 0)
    size = {f: Cn * nlev * (4 if f == "q_draw" else 8) for f in FIELDS}
    off, o = {}, PAD
    for f in FIELDS:
        off[f] = o
        o += (size[f] + 255) // 256 * 256 + PAD
    arena = torch.full((o,), GUARD, dtype=torch.uint8, device=dev)
    tJ = torch.from_numpy(J1).to(dev)
    ts = None
    if status is not None:
        status = np.ascontiguousarray(status, dtype=np.int32)
        assert status.shape == (Cn, D)
        ts = torch.from_numpy(status).to(dev)
    rc = _call_hook(Cn, D, my, j_bound, tJ.data_ptr(), ts.data_ptr() if ts is not None else None, levels,
                    {f: arena.data_ptr() + off[f] for f in fields})
    assert rc == 0, _lib.last_error()
    torch.cuda.synchronize(dev)
    host = arena.cpu().numpy()
    untouched = np.ones(o, bool)
    out = {}
    for f in fields:
        untouched[off[f]:off[f] + size[f]] = False
        raw = host[off[f]:off[f] + size[f]].copy()
        out[f] = raw.view(np.int32 if f == "q_draw" else np.float64).reshape(Cn, nlev)
    assert np.all(host[untouched] == GUARD), "bytes outside the requested fields were written"
    return out


def check(J1, st, j_bound, levels):
    """The device's record is the yardstick's, bit for bit; returns the yardstick's."""
    J1 = np.asarray(J1, dtype=np.float64)
    st = None if st is None else np.asarray(st, dtype=np.int32)
    want = tail_ref(J1, st, j_bound, levels)
    assert_same_tail(tail_on_device(J1, st, j_bound, levels), want)
    return want


def spread(total, my, at=None):
    """A draw's row of my outputs whose sequential sum is exactly `total`: everything on one output."""
    row = [0.0] * my
    row[my - 1 if at is None else at] = total
    return row


def _mixed_records(rng, Cn, D, my):
    """Positive costs over 12 decades in the even candidates, totals on a grid of quarters (many
    ties) in the odd ones; about one draw in eight fails by status, one in sixteen holds a non-finite
    or huge cost, some exceed the bound 1e4; one candidate in 64 was never simulated."""
    J1 = 10.0 ** rng.uniform(-8.0, 4.0, (Cn, D, my))
    grid = rng.integers(0, 9, (Cn, D, my)).astype(np.float64) / 4.0
    J1[1::2] = grid[1::2]
    bad = rng.random((Cn, D)) < 1 / 16
    J1[bad, rng.integers(0, my, int(bad.sum()))] = rng.choice([NAN, INF, -INF, 1e308], int(bad.sum()))
    st = np.where(rng.random((Cn, D)) < 1 / 8, rng.choice([1, 2, 4, 128, 5], (Cn, D)), 0).astype(np.int32)
    never = rng.random(Cn) < 1 / 64
    st[never, rng.integers(0, D, int(never.sum()))] |= rng.choice([8, 16], int(never.sum())).astype(np.int32)
    return J1, st


# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Cn", CS)
@pytest.mark.parametrize("D", DS)
def test_shapes(gpu, D, Cn):
    """Every D at and around the wave width (a lane's second draw starts at 64, its third at 128), the
    cap 4096 and a D in between, x C = 1, 3, 4, 5, my cycling through 1, 2, 3, 7; eight levels and
    one; status given and NULL.  Asserted on the generated inputs: from D = 3 on some candidate has
    two levels that select different draws, so the ordering is exercised."""
    my = MYS[(DS.index(D) + CS.index(Cn)) % 4]
    rng = np.random.default_rng(1000 * D + Cn)
    J1, st = _mixed_records(rng, Cn, D, my)
    if D >= 3:                       # candidate 0 keeps at least three clean, distinct draws
        J1[0, :3] = [spread(float(k + 1), my) for k in range(3)]
        st[0, :] &= ~np.int32(8 | 16)
        st[0, :3] = 0
    for status in (st, None):
        want = check(J1, status, 1e4, LEVELS8)
        if D >= 3:
            assert any(len(set(want["q_draw"][c].tolist())) >= 2 for c in range(Cn)), "every level selects one draw"
            assert want["n"][0] >= 3
        one = check(J1, status, 1e4, (0.9,))
        assert one["quantile"].shape == (Cn, 1)
        np.testing.assert_array_equal(bits(want["quantile"][:, 3]), bits(want["quantile"][:, 6]))   # duplicates


def test_many_candidates(gpu):
    """C = 4,097 at D = 5: more candidates than one pass of anything, my = 2."""
    rng = np.random.default_rng(4097)
    J1, st = _mixed_records(rng, 4097, 5, 2)
    want = check(J1, st, 1e4, LEVELS8)
    assert (want["n"] == 0).any() and (want["n"] == 5).any() and ((want["n"] > 0) & (want["n"] < 5)).any()
    assert sum(len(set(want["q_draw"][c].tolist())) >= 2 for c in range(4097)) > 1000


def test_repeated_and_reversed(gpu):
    """A repeated call is bitwise identical; a record does not depend on the candidate's place."""
    rng = np.random.default_rng(77)
    J1, st = _mixed_records(rng, 37, 70, 3)
    a = tail_on_device(J1, st, 1e4, LEVELS8)
    assert_same_tail(tail_on_device(J1, st, 1e4, LEVELS8), a)
    r = tail_on_device(J1[::-1], st[::-1], 1e4, LEVELS8)
    assert_same_tail({f: r[f][::-1] for f in FIELDS}, a)
    assert_same_tail(a, tail_ref(J1, st, 1e4, LEVELS8))


def test_any_subset_of_the_outputs(gpu):
    """Any of the three output pointers may be NULL, all of them too: the fields asked for keep the
    bits of the full call and the arena around them (the NULL fields' places included) stays."""
    rng = np.random.default_rng(7)
    J1, st = _mixed_records(rng, 261, 9, 3)
    full = tail_on_device(J1, st, 1e4, LEVELS8)
    assert_same_tail(full, tail_ref(J1, st, 1e4, LEVELS8))
    for mask in range(8):
        sub = tuple(f for b, f in enumerate(FIELDS) if mask >> b & 1)
        got = tail_on_device(J1, st, 1e4, LEVELS8, fields=sub)
        assert set(got) == set(sub)
        assert_same_tail(got, full, fields=sub, msg=str(sub))


@pytest.mark.parametrize("my", MYS)
def test_all_totals_equal(gpu, my):
    """D equal totals, each on another output: rank m is draw D - m (index descending), whatever the
    lane and the pass; level 1 is draw 0, robust_reduce's worst_draw."""
    D = 130
    rows = [spread(4.0, my, k % my) for k in range(D)]
    want = check([rows], np.zeros((1, D), np.int32), 0.0, LEVELS8)
    for j, a in enumerate(LEVELS8):
        m = min(max(math.ceil(a * float(D)), 1), D)
        assert want["q_draw"][0, j] == D - m and want["quantile"][0, j] == 4.0 and want["cvar"][0, j] == 4.0
    assert want["q_draw"][0, 0] == 0 and want["q_draw"][0, 4] == D - 1


def test_equal_pairs_across_lanes_and_passes(gpu):
    """Equal pairs at draws 63 | 64 (the last lane's first draw and lane 0's second) and at 5 | 69
    (lane 5's first and second draw); -0.0 and +0.0 tie as well.  Among equals the higher index takes
    the lower rank."""
    D = 129
    J = np.arange(10.0, 10.0 + D)
    J[63] = J[64] = 5.0       # ranks 3, 4 -> draws 64, 63
    J[5] = J[69] = 7.0        # ranks 5, 6 -> draws 69, 5
    J[100], J[20] = 0.0, -0.0  # ranks 1, 2 -> draws 100, 20
    levels = [k / D for k in (1, 2, 3, 4, 5, 6)] + [1.0]
    want = check(J.reshape(1, D, 1), None, 0.0, levels)
    ms = [min(max(math.ceil(a * float(D)), 1), D) for a in levels]
    order = {1: 100, 2: 20, 3: 64, 4: 63, 5: 69, 6: 5, 7: 0}
    for j, m in enumerate(ms[:-1]):
        assert want["q_draw"][0, j] == order[m], (j, m)
    assert len({int(x) for x in want["q_draw"][0]}) >= 4
    # a total starts from the accumulator 0.0, so the -0.0 record totals +0.0: both zeros carry +0.0's bits
    z = check(J.reshape(1, D, 1), None, 0.0, [1e-300, 1.5 / D])
    assert z["q_draw"][0].tolist() == [100, 20]
    assert math.copysign(1.0, z["quantile"][0, 0]) == 1.0 and math.copysign(1.0, z["quantile"][0, 1]) == 1.0


@pytest.mark.parametrize("my", MYS)
def test_bound_is_inclusive(gpu, my):
    """J == j_bound survives and is the level-1 quantile, the next double above fails; the total is
    a genuine sum of my terms.  j_bound = 0 is 1e100."""
    row = [2.0 ** i for i in range(my)]
    jb = 0.0
    for x in row:
        jb += x
    over = row[:-1] + [math.nextafter(row[-1], INF)]
    small = [0.25] * my
    J1 = [[row, small, small], [over, small, small], [small, over, row]]
    want = check(J1, np.zeros((3, 3), np.int32), jb, (1.0, 0.5))
    assert want["n"].tolist() == [3, 2, 2]
    assert want["quantile"][:, 0].tolist() == [jb, 0.25 * my, jb] and want["q_draw"][:, 0].tolist() == [0, 1, 2]
    nxt = math.nextafter(1e100, INF)
    J1 = [[spread(1e100, my), spread(1.0, my)], [spread(nxt, my), spread(1.0, my)]]
    want = check(J1, None, 0.0, (1.0,))
    assert want["quantile"][:, 0].tolist() == [1e100, 1.0] and want["n"].tolist() == [2, 1]
    check(J1, None, 1e100, (1.0,))


@pytest.mark.parametrize("my", MYS)
def test_infinite_bound(gpu, my):
    """j_bound = +inf: finite totals near 1e308 survive, their tail sum rounds to +inf and the tail
    mean is +inf, never NaN; the quantile stays finite; a total that overflows fails."""
    big = spread(1e308, my)
    J1 = [[big, [1.0] * my, big, big], [big, big, [2.0] * my, [1e308] * my]]
    want = check(J1, np.zeros((2, 4), np.int32), INF, (1.0, 0.5, 0.25))
    assert want["n"].tolist() == ([4, 4] if my == 1 else [4, 3])
    assert want["cvar"][0].tolist() == [1e308, INF, INF] and not np.isnan(want["cvar"]).any()
    assert want["quantile"][0].tolist() == [1e308, 1e308, float(my)] and want["q_draw"][0].tolist() == [0, 3, 1]
    check(J1, np.zeros((2, 4), np.int32), 1.7e308, (1.0, 0.5, 0.25))


@pytest.mark.parametrize("my", MYS)
def test_status_bits_and_failed_draws(gpu, my):
    """Every status bit fails its draw though the total is small; bits 8 and 16 on any draw leave the
    candidate without a survivor; all draws failed (by status, by the bound, by NaN): NaN, NaN, -1;
    one survivor: every level selects it."""
    row = [0.5] * my
    J1 = np.array([[[(k + 1.0)] * my for k in range(7)]] * 9)
    st = np.zeros((9, 7), np.int32)
    st[0] = [0, 1, 2, 4, 32, 64, 128]        # one survivor: draw 0
    st[1] = [1, 2, 4, 32, 64, 128, 1 | 4]    # all failed
    st[2, 3] = 8                             # never simulated
    st[3, 6] = 16
    st[4] = [4, 16, 0, 0, 8 | 4, 0, 0]
    J1[5] = 1e9                              # all over the bound
    J1[6] = NAN
    st[7, [1, 3, 5]] = [1, 2, 128]           # four survivors: draws 0, 2, 4, 6
    J1[8, :, 0] = [NAN, INF, -INF, 1.0, 2.0, NAN, 3.0]   # status 0, non-finite totals fail
    want = check(J1, st, 1e6, LEVELS8)
    assert want["n"].tolist() == [1, 0, 0, 0, 0, 0, 0, 4, 3]
    assert np.all(want["q_draw"][0] == 0) and np.all(want["quantile"][0] == my * 1.0)
    for c in (1, 2, 3, 4, 5, 6):
        assert np.all(np.isnan(want["quantile"][c])) and np.all(np.isnan(want["cvar"][c]))
        assert np.all(want["q_draw"][c] == -1)
    assert want["q_draw"][7].tolist() == [6, 2, 4, 6, 0, 0, 6, 4]
    assert row == [0.5] * my
    # the same records without a status array: only the totals decide
    nost = check(J1, None, 1e6, LEVELS8)
    assert nost["n"].tolist() == [7, 7, 7, 7, 7, 0, 0, 7, 3]


def test_levels_k_over_n(gpu):
    """k / n for every k at n = 7 (nine draws, two failed) and 1.0: the rank is ceil of the double
    product as written; 0.5 at n = 8, where a * n is the integer 4, and the next double above 0.5."""
    J = np.array([[3.0, 9.0, 1.0, 1e9, 4.0, 7.0, 2.0, NAN, 5.0]]).reshape(1, 9, 1)
    levels = [k / 7 for k in range(1, 8)] + [1.0]
    want = check(J, None, 1e6, levels)
    assert want["n"][0] == 7
    srt = [1.0, 2.0, 3.0, 4.0, 5.0, 7.0, 9.0]
    assert want["quantile"][0].tolist() == [srt[min(math.ceil(a * 7.0), 7) - 1] for a in levels]
    assert len(set(want["q_draw"][0].tolist())) >= 6
    J8 = np.array([8.0, 3.0, 6.0, 1.0, 7.0, 2.0, 5.0, 4.0]).reshape(1, 8, 1)
    w8 = check(J8, None, 0.0, (0.5, math.nextafter(0.5, 1.0), 0.95, 1e-300))
    assert w8["quantile"][0].tolist() == [4.0, 5.0, 8.0, 1.0] and w8["q_draw"][0].tolist() == [7, 6, 0, 3]
    assert w8["cvar"][0, 0] == (4.0 + 5.0 + 6.0 + 7.0 + 8.0) / 5


def test_tail_sum_is_sequential_in_rank_order(gpu):
    """Terms spread over 16 decades: the ascending sequential sum and the descending one differ in the
    yardstick's own arithmetic (asserted), and the device gives the ascending bits."""
    rng = np.random.default_rng(20251020)
    D = 1000
    for _ in range(64):
        col = (10.0 ** rng.uniform(-8.0, 8.0, D)).tolist()
        up = 0.0
        for x in sorted(col):
            up += x
        down = 0.0
        for x in sorted(col, reverse=True):
            down += x
        if up != down:
            break
    assert up != down
    want = check(np.array(col).reshape(1, D, 1), None, 0.0, (1e-300, 0.5, 0.999))
    assert want["cvar"][0, 0] == up / D


def test_bad_arguments(gpu):
    """nlev outside 1 .. 8, levels NULL, a bad level, j_bound negative or NaN, D < 1, my < 1:
    MPCT_EINVAL; D = 4097: MPCT_ERANGE; nothing launched."""
    import torch
    from mpct import _lib

    dev = torch.device("cuda", 0)
    J1 = torch.ones((2, 3, 2), dtype=torch.float64, device=dev)
    st = torch.zeros((2, 3), dtype=torch.int32, device=dev)
    out = torch.full((64,), -7, dtype=torch.int32, device=dev)
    ptrs = {"q_draw": out.data_ptr()}
    ok = (0.5, 1.0)
    for D, my, jb, lv, nlev in ((3, 2, -1.0, ok, None), (3, 2, NAN, ok, None), (0, 2, 0.0, ok, None),
                                (3, 0, 0.0, ok, None), (3, 2, 0.0, ok, 0), (3, 2, 0.0, (0.5,) * 9, None),
                                (3, 2, 0.0, None, 2), (3, 2, 0.0, (0.5, NAN), None), (3, 2, 0.0, (0.0, 1.0), None),
                                (3, 2, 0.0, (0.5, 1.0000000000000002), None), (3, 2, 0.0, (-1.0,), None)):
        rc = _call_hook(2, D, my, jb, J1.data_ptr(), st.data_ptr(), lv, ptrs, nlev=nlev)
        assert rc == EINVAL, (D, my, jb, lv, nlev, rc)
        assert _lib.last_error()
    assert _call_hook(2, 4097, 2, 0.0, J1.data_ptr(), st.data_ptr(), ok, ptrs) == ERANGE
    torch.cuda.synchronize(dev)
    assert torch.all(out == -7).item()
    assert _call_hook(2, 3, 2, 0.0, J1.data_ptr(), st.data_ptr(), ok, ptrs) == 0   # and the same call, valid
    torch.cuda.synchronize(dev)
    # three equal totals: ranks 1, 2, 3 are draws 2, 1, 0; level 0.5 is rank ceil(1.5) = 2, level 1 rank 3
    assert out[:4].tolist() == [1, 0, 1, 0] and torch.all(out[4:] == -7).item()
