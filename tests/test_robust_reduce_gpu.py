"""GPU: robust_reduce_kernel on synthetic draw records (robust_reduce.h, "the single definition of
the semantics and of the summation order"; include/mpct.h).

The kernel is driven directly through the library's undeclared hook mpct_internal_robust_reduce, so
the records are whatever a case needs: a total exactly on the bound, an overflowing total, ties,
every status bit.  The yardstick is reduce_ref below, a scalar Python restatement of the header's
rule: one float accumulator per output over the draws k = 0 .. D - 1, J summed over i = 0 .. my - 1,
in that order (a Python float is an IEEE double and the loop is sequential; numpy.sum is pairwise
and is not used).  Every comparison is bitwise, NaN matched by position; no tolerance appears in
this file."""
import ctypes as C
import math

import numpy as np
import pytest

pytestmark = [pytest.mark.gpu, pytest.mark.filterwarnings("error::RuntimeWarning")]

FIELDS = ("mean", "worst", "n_failed", "worst_draw", "status")
MYS = (1, 2, 3, 7)
EINVAL = -1
INF, NAN = math.inf, math.nan
GUARD = 0xA5     # fill byte of the output arena
PAD = 256        # guard bytes around every output field


@pytest.fixture(scope="module")
def gpu(built, has_gpu):
    if not has_gpu:
        pytest.skip("no GPU")
    return True


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int64 if a.dtype == np.float64 else a.dtype)


# ---------------------------------------------------------------------------------------------
# the yardstick
def reduce_ref(J1, st, j_bound):
    """include/mpct.h's record, one candidate at a time in plain Python floats.  J1 [C, D, my],
    st [C, D]; j_bound = 0 means 1e100."""
    Cn, D, my = J1.shape
    bound = 1e100 if j_bound == 0.0 else float(j_bound)
    out = dict(mean=np.empty((Cn, my)), worst=np.empty((Cn, my)), n_failed=np.empty(Cn, np.int32),
               worst_draw=np.empty(Cn, np.int32), status=np.empty(Cn, np.int32))
    for c in range(Cn):
        rows, sts = J1[c].tolist(), st[c].tolist()
        acc, mx = [0.0] * my, [0.0] * my
        sor, nfail, nsurv, wd, jw = 0, 0, 0, -1, 0.0
        for k in range(D):
            sor |= sts[k]
            J = 0.0
            for i in range(my):
                J += rows[k][i]
            if sts[k] == 0 and math.isfinite(J) and J <= bound:
                for i in range(my):
                    v = rows[k][i]
                    acc[i] += v
                    if nsurv == 0 or v > mx[i]:
                        mx[i] = v
                if nsurv == 0 or J > jw:    # the first draw above every earlier surviving one
                    jw, wd = J, k
                nsurv += 1
            else:
                nfail += 1
        if sor & (8 | 16):                  # never simulated: not a failed draw
            nfail, nsurv, wd = 0, 0, -1
        for i in range(my):
            out["mean"][c, i] = acc[i] / nsurv if nsurv else NAN
            out["worst"][c, i] = mx[i] if nsurv else NAN
        out["n_failed"][c], out["worst_draw"][c], out["status"][c] = nfail, wd, sor
    return out


def reduce_ref_rows(J1, st, j_bound):
    """reduce_ref with the candidates side by side: the same walk over k and i with one numpy array of
    C doubles where reduce_ref holds one float.  Every operation is elementwise (no numpy reduction),
    so each candidate sees reduce_ref's additions in reduce_ref's order; for the large-C shapes, where
    the scalar loop would take minutes.  test_shapes holds it to reduce_ref's bits on a sample."""
    Cn, D, my = J1.shape
    bound = 1e100 if j_bound == 0.0 else float(j_bound)
    acc, mx = np.zeros((my, Cn)), np.zeros((my, Cn))
    sor, nfail, nsurv = np.zeros(Cn, np.int32), np.zeros(Cn, np.int32), np.zeros(Cn, np.int32)
    wd, jw = np.full(Cn, -1, np.int32), np.zeros(Cn)
    with np.errstate(all="ignore"):
        for k in range(D):
            sor |= st[:, k]
            J = np.zeros(Cn)
            for i in range(my):
                J = J + J1[:, k, i]
            ok = (st[:, k] == 0) & np.isfinite(J) & (J <= bound)
            first = nsurv == 0
            for i in range(my):
                v = J1[:, k, i]
                acc[i] = np.where(ok, acc[i] + v, acc[i])
                mx[i] = np.where(ok & (first | (v > mx[i])), v, mx[i])
            top = ok & (first | (J > jw))
            jw, wd = np.where(top, J, jw), np.where(top, k, wd).astype(np.int32)
            nsurv += ok
            nfail += ~ok
        never = (sor & (8 | 16)) != 0
        nfail[never], nsurv[never], wd[never] = 0, 0, -1
        some = nsurv > 0
        mean = np.where(some, acc / np.where(some, nsurv, 1), NAN).T
        worst = np.where(some, mx, NAN).T
    return dict(mean=np.ascontiguousarray(mean), worst=np.ascontiguousarray(worst), n_failed=nfail, worst_draw=wd,
                status=sor)


# ---------------------------------------------------------------------------------------------
# the kernel, launched directly
def _call_hook(Cn, D, my, j_bound, J1_ptr, st_ptr, ptrs):
    import torch
    from mpct import _lib

    r = _lib.MpctRobustResult()
    for f in FIELDS:
        ty = _lib.c_double_p if f in ("mean", "worst") else _lib.c_int32_p
        setattr(r, f, C.cast(C.c_void_p(ptrs.get(f)), ty))
    return _lib.load().mpct_internal_robust_reduce(Cn, D, my, float(j_bound), C.c_void_p(J1_ptr), C.c_void_p(st_ptr),
                                                   C.byref(r), C.c_void_p(torch.cuda.current_stream().cuda_stream))


def reduce_on_device(J1, status, j_bound, fields=FIELDS):
    """robust_reduce_kernel on records J1 [C, D, my], status [C, D] (host arrays).  The five output
    fields lie in one arena of GUARD bytes, PAD of them before, between and after; only the fields
    named get a pointer, the others are passed NULL.  Returns the named fields and asserts that every
    other byte of the arena still holds GUARD."""
    import torch
    from mpct import _lib

    J1 = np.ascontiguousarray(J1, dtype=np.float64)
    status = np.ascontiguousarray(status, dtype=np.int32)
    Cn, D, my = J1.shape
    assert status.shape == (Cn, D)
    dev = torch.device("cuda", 0)
    size = {f: Cn * my * 8 if f in ("mean", "worst") else Cn * 4 for f in FIELDS}
    off, o = {}, PAD
    for f in FIELDS:
        off[f] = o
        o += (size[f] + 255) // 256 * 256 + PAD
    arena = torch.full((o,), GUARD, dtype=torch.uint8, device=dev)
    tJ, ts = torch.from_numpy(J1).to(dev), torch.from_numpy(status).to(dev)
    rc = _call_hook(Cn, D, my, j_bound, tJ.data_ptr(), ts.data_ptr(), {f: arena.data_ptr() + off[f] for f in fields})
    assert rc == 0, _lib.last_error()
    torch.cuda.synchronize(dev)
    host = arena.cpu().numpy()
    untouched = np.ones(o, bool)
    out = {}
    for f in fields:
        untouched[off[f]:off[f] + size[f]] = False
        raw = host[off[f]:off[f] + size[f]].copy()
        out[f] = raw.view(np.float64).reshape(Cn, my) if f in ("mean", "worst") else raw.view(np.int32)
    assert np.all(host[untouched] == GUARD), "bytes outside the requested fields were written"
    return out


def check(J1, st, j_bound, ref=reduce_ref):
    """The device's record is the yardstick's, bit for bit; returns the yardstick's."""
    J1, st = np.asarray(J1, dtype=np.float64), np.asarray(st, dtype=np.int32)
    want = ref(J1, st, j_bound)
    got = reduce_on_device(J1, st, j_bound)
    for f in FIELDS:
        np.testing.assert_array_equal(bits(got[f]), bits(want[f]), err_msg=f)
    return want


def spread(total, my, at=None):
    """A draw's row of my outputs whose sequential sum is exactly `total`: everything on one output."""
    row = [0.0] * my
    row[my - 1 if at is None else at] = total
    return row


def seq_sum(xs):
    s = 0.0
    for x in xs:
        s += x
    return s


def tree_sum(xs):
    """pairwise (halving) summation in Python floats"""
    return xs[0] if len(xs) == 1 else tree_sum(xs[:len(xs) // 2]) + tree_sum(xs[len(xs) // 2:])


# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("my", MYS)
def test_bound_is_inclusive(gpu, my):
    """J == j_bound survives, the next double above fails; the total is a genuine sum of my terms
    (1 + 2 + .. + 2^(my-1), exact), and the failing one differs in its last term's last bit."""
    row = [2.0 ** i for i in range(my)]
    jb = seq_sum(row)
    over = row[:-1] + [math.nextafter(row[-1], INF)]
    assert jb == 2.0 ** my - 1 and seq_sum(over) == math.nextafter(jb, INF)
    small = [0.25] * my
    J1 = [[row, small], [over, small], [small, over]]
    want = check(J1, np.zeros((3, 2), np.int32), jb)
    assert want["n_failed"].tolist() == [0, 1, 1]
    assert want["worst_draw"].tolist() == [0, 1, 0]
    assert want["worst"][0].tolist() == row and want["worst"][1].tolist() == small
    assert want["mean"][0].tolist() == [(a + 0.25) / 2 for a in row] and want["mean"][2].tolist() == small


@pytest.mark.parametrize("my", MYS)
def test_default_bound_is_1e100(gpu, my):
    """j_bound = 0 means 1e100: a total of 1e100 survives, the next double fails."""
    nxt = math.nextafter(1e100, INF)
    J1 = [[spread(1e100, my)], [spread(nxt, my)], [spread(1e100, my, 0)], [spread(nxt, my, 0)]]
    want = check(J1, np.zeros((4, 1), np.int32), 0.0)
    assert want["n_failed"].tolist() == [0, 1, 0, 1] and want["worst_draw"].tolist() == [0, -1, 0, -1]
    assert want["worst"][0, my - 1] == 1e100 and np.all(np.isnan(want["mean"][1]))
    # and 0 is exactly the explicit 1e100
    check(J1, np.zeros((4, 1), np.int32), 1e100)


@pytest.mark.parametrize("my", MYS)
def test_infinite_bound(gpu, my):
    """j_bound = +inf: any finite total survives (1e308); two such draws sum to +inf, so the mean is
    +inf and not NaN; a draw whose outputs are finite but whose total overflows fails."""
    big = spread(1e308, my)
    J1 = [[big, [1.0] * my], [big, big]]
    if my > 1:
        J1.append([[1e308] * my, [1.0] * my])   # every output finite, the total +inf
    want = check(J1, np.zeros((len(J1), 2), np.int32), INF)
    assert want["n_failed"][:2].tolist() == [0, 0]
    assert want["mean"][1, my - 1] == INF and not np.isnan(want["mean"][1]).any()
    assert want["worst"][1, my - 1] == 1e308 and want["worst_draw"][1] == 0
    if my > 1:
        assert want["n_failed"][2] == 1 and want["worst_draw"][2] == 1 and want["worst"][2].tolist() == [1.0] * my
    # a finite bound at the top of the range fails nothing more than the overflow does
    check(J1, np.zeros((len(J1), 2), np.int32), 1.7e308)


@pytest.mark.parametrize("my", MYS)
def test_nonfinite_record_with_status_zero_fails(gpu, my):
    """A status-0 draw whose J1 holds NaN, +inf or -inf fails, wherever the value stands; +inf and
    -inf in one draw (a NaN total) too."""
    good = [float(i + 1) for i in range(my)]
    J1, expect, worst_draw = [], [], []
    for bad in (NAN, INF, -INF):
        for at in sorted({0, my // 2, my - 1}):
            row = list(good)
            row[at] = bad
            J1.append([good, row, [2 * g for g in good]])
            expect.append(1)
            worst_draw.append(2)
    if my > 1:
        J1.append([[INF, -INF] + good[2:], good, good])
        expect.append(1)
        worst_draw.append(1)
    J1.append([[NAN] * my, [INF] * my, [-INF] * my])
    expect.append(3)
    worst_draw.append(-1)
    st = np.zeros((len(J1), 3), np.int32)
    for jb in (0.0, INF, 1e6):
        want = check(J1, st, jb)
        assert want["n_failed"].tolist() == expect and np.all(want["status"] == 0)
        assert want["worst_draw"].tolist() == worst_draw
        assert np.all(np.isnan(want["mean"][-1])) and np.all(np.isnan(want["worst"][-1]))
        assert want["mean"][0].tolist() == [1.5 * g for g in good]


@pytest.mark.parametrize("my", MYS)
def test_nonzero_status_fails_and_is_ored(gpu, my):
    """A draw with status 1, 2, 4 or 128 fails though its total is small and finite; status is the
    OR over all draws; every draw failed: NaN statistics, worst_draw = -1, n_failed = D."""
    row = [0.5] * my
    J1 = [[row] * 5] * 4
    st = [[0, 1, 0, 2, 0], [4, 0, 128, 0, 1], [1, 2, 4, 128, 64 | 32], [0, 0, 0, 0, 0]]
    want = check(J1, st, 0.0)
    assert want["n_failed"].tolist() == [2, 3, 5, 0]
    assert want["status"].tolist() == [3, 133, 1 | 2 | 4 | 128 | 64 | 32, 0]
    assert want["worst_draw"].tolist() == [0, 1, -1, 0]
    assert np.all(np.isnan(want["mean"][2])) and np.all(np.isnan(want["worst"][2]))
    assert want["mean"][0].tolist() == row and want["worst"][1].tolist() == row
    # all failed by the bound alone, and by a NaN alone
    want = check([[[3.0] * my] * 4, [[NAN] * my] * 4], np.zeros((2, 4), np.int32), 1.0)
    assert want["n_failed"].tolist() == [4, 4] and want["worst_draw"].tolist() == [-1, -1]
    assert np.all(np.isnan(want["mean"])) and np.all(np.isnan(want["worst"])) and np.all(want["status"] == 0)


def test_ties_and_worst_per_output(gpu):
    """Equal totals: the lowest index is the worst draw.  worst is the maximum per output over the
    survivors, not the worst draw's row: rows (3, 1) and (1, 3) give worst = (3, 3), worst_draw = 0.
    A failed draw with the largest total is never worst_draw and adds nothing to worst."""
    J1 = [[[3.0, 1.0], [1.0, 3.0], [2.0, 2.0], [0.5, 0.5]],     # three equal totals
          [[0.5, 0.5], [1.0, 3.0], [3.0, 1.0], [2.0, 2.0]],     # the tie starts at draw 1
          [[9.0, 9.0], [1.0, 3.0], [3.0, 1.0], [50.0, 0.0]],    # draw 0 fails by status, draw 3 by the bound
          [[1.0, 2.0], [7.0, 0.0], [0.0, 7.5], [7.0, 0.5]]]     # worst draw 2, worst row (7, 7.5) of draws 1 and 2
    st = [[0, 0, 0, 0], [0, 0, 0, 0], [1, 0, 0, 0], [0, 0, 0, 0]]
    want = check(J1, st, 10.0)
    assert want["worst_draw"].tolist() == [0, 1, 1, 2]
    assert want["worst"].tolist() == [[3.0, 3.0], [3.0, 3.0], [3.0, 3.0], [7.0, 7.5]]
    assert want["n_failed"].tolist() == [0, 0, 2, 0]
    assert want["mean"][2].tolist() == [2.0, 2.0]
    for my in (1, 3, 7):   # the same tie with my outputs: D equal totals, each on another output
        rows = [spread(4.0, my, k % my) for k in range(2 * my + 1)]
        want = check([rows], np.zeros((1, 2 * my + 1), np.int32), 0.0)
        assert want["worst_draw"].tolist() == [0] and want["worst"][0].tolist() == [4.0] * my


@pytest.mark.parametrize("my", MYS)
def test_never_simulated(gpu, my):
    """Status 8 (skipped) or 16 (bad horizon) on any draw, alone or mixed with 4: NaN statistics,
    n_failed = 0, worst_draw = -1, status the OR, though other draws carry good records."""
    row = [1.0] * my
    J1 = [[row] * 3] * 6
    st = [[8, 8, 8], [16, 16, 16], [0, 8, 0], [4, 16, 0], [8 | 4, 0, 0], [0, 0, 16 | 8]]
    want = check(J1, st, 0.0)
    assert want["status"].tolist() == [8, 16, 8, 20, 12, 24]
    assert np.all(want["n_failed"] == 0) and np.all(want["worst_draw"] == -1)
    assert np.all(np.isnan(want["mean"])) and np.all(np.isnan(want["worst"]))
    nan_rows = [[[NAN] * my] * 3] * 2    # the records robust_classify_kernel's candidates would carry
    want = check(nan_rows, [[8] * 3, [16] * 3], INF)
    assert np.all(want["n_failed"] == 0) and want["status"].tolist() == [8, 16]


@pytest.mark.parametrize("D", [64, 1000])
def test_summation_order_is_sequential(gpu, D):
    """Terms spread over 16 decades: the sequential sum and a pairwise one differ in the yardstick's
    own arithmetic (asserted first, per output), and the device gives the sequential bits.  A column
    of D terms whose two sums happen to agree (the few largest terms dominate both) is drawn again
    from the same seeded stream: the choice looks at the yardstick's arithmetic only."""
    rng = np.random.default_rng(20250307 + D)
    for my in MYS:
        J1 = np.empty((3, D, my))
        for c in range(3):
            for i in range(my):
                for _ in range(64):
                    col = (10.0 ** rng.uniform(-8.0, 8.0, D)).tolist()
                    if seq_sum(col) != tree_sum(col):
                        break
                J1[c, :, i] = col
                assert seq_sum(col) != tree_sum(col), (my, c, i)
        want = check(J1, np.zeros((3, D), np.int32), 0.0)
        assert np.all(want["n_failed"] == 0)
        assert want["mean"][0, 0] == seq_sum(J1[0, :, 0].tolist()) / D
        # with every third draw failed the survivors' sum is sequential too
        st = np.zeros((3, D), np.int32)
        st[:, ::3] = 1
        check(J1, st, 0.0)


def _mixed_records(rng, Cn, D, my):
    """Positive costs over 12 decades; about one draw in eight fails by status, one in sixteen holds a
    non-finite cost, some exceed the bound 1e4; one candidate in 64 was never simulated."""
    J1 = 10.0 ** rng.uniform(-8.0, 4.0, (Cn, D, my))
    bad = rng.random((Cn, D)) < 1 / 16
    J1[bad, rng.integers(0, my, int(bad.sum()))] = rng.choice([NAN, INF, -INF, 1e308], int(bad.sum()))
    st = np.where(rng.random((Cn, D)) < 1 / 8, rng.choice([1, 2, 4, 128, 5], (Cn, D)), 0).astype(np.int32)
    never = rng.random(Cn) < 1 / 64
    st[never, rng.integers(0, D, int(never.sum()))] |= rng.choice([8, 16], int(never.sum())).astype(np.int32)
    return J1, st


@pytest.mark.parametrize("Cn", [1, 5, 4097])
@pytest.mark.parametrize("D", [1, 2, 129, 1000])
def test_shapes(gpu, D, Cn):
    """D = 1, 2, 129 (past the fused kernel's cap), 1000 x C = 1, 5, 4097 (the last four-wave block
    holds one candidate), my cycling through 1, 2, 3, 7.  The yardstick is reduce_ref where the scalar
    loop is quick and reduce_ref_rows beyond, held to reduce_ref's bits on the first, a middle and the
    last candidates."""
    my = MYS[([1, 2, 129, 1000].index(D) + [1, 5, 4097].index(Cn)) % 4]
    rng = np.random.default_rng(1000 * D + Cn)
    J1, st = _mixed_records(rng, Cn, D, my)
    want = check(J1, st, 1e4, ref=reduce_ref if Cn * D <= 10000 else reduce_ref_rows)
    pick = sorted({0, Cn // 2, Cn - 1} | set(range(max(0, Cn - 5), Cn)))
    scalar = reduce_ref(J1[pick], st[pick], 1e4)
    for f in FIELDS:
        np.testing.assert_array_equal(bits(want[f][pick]), bits(scalar[f]), err_msg=f)
    if Cn * D >= 129:   # the records are a real mix
        assert (want["n_failed"] > 0).any() and (want["worst_draw"] >= 0).any()


def test_any_subset_of_the_outputs(gpu):
    """Any output pointer may be NULL: the fields asked for keep the bits of the full call, and the
    arena around and between them (the NULL fields' places included) stays as it was filled."""
    rng = np.random.default_rng(7)
    J1, st = _mixed_records(rng, 261, 9, 3)
    full = reduce_on_device(J1, st, 1e4)
    want = reduce_ref(J1, st, 1e4)
    for f in FIELDS:
        np.testing.assert_array_equal(bits(full[f]), bits(want[f]), err_msg=f)
    subsets = [(f,) for f in FIELDS] + [("n_failed", "worst_draw"), ("mean", "worst"), ("mean", "status"),
                                        ("worst", "n_failed", "worst_draw", "status"), ()]
    for sub in subsets:
        got = reduce_on_device(J1, st, 1e4, fields=sub)
        assert set(got) == set(sub)
        for f in sub:
            np.testing.assert_array_equal(bits(got[f]), bits(full[f]), err_msg="%s of %s" % (f, sub))


def test_bad_arguments(gpu):
    """j_bound negative or NaN, D < 1, my < 1: MPCT_EINVAL, nothing launched."""
    import torch
    from mpct import _lib

    dev = torch.device("cuda", 0)
    J1 = torch.ones((2, 3, 2), dtype=torch.float64, device=dev)
    st = torch.zeros((2, 3), dtype=torch.int32, device=dev)
    out = torch.full((64,), -7, dtype=torch.int32, device=dev)
    ptrs = {"n_failed": out.data_ptr()}
    for D, my, jb in ((3, 2, -1.0), (3, 2, -0.5e-300), (3, 2, -INF), (3, 2, NAN), (0, 2, 0.0), (-1, 2, 0.0),
                      (3, 0, 0.0), (3, -2, 0.0)):
        rc = _call_hook(2, D, my, jb, J1.data_ptr(), st.data_ptr(), ptrs)
        assert rc == EINVAL, (D, my, jb, rc)
        assert _lib.last_error()
    torch.cuda.synchronize(dev)
    assert torch.all(out == -7).item()
    assert _call_hook(2, 3, 2, 0.0, J1.data_ptr(), st.data_ptr(), ptrs) == 0   # and the same call, valid
    torch.cuda.synchronize(dev)
    assert out[:2].tolist() == [0, 0] and torch.all(out[2:] == -7).item()
