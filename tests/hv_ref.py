"""The hypervolume contract of include/mpct.h in numpy: the counter-based sample points in wrapping
uint64 arithmetic, the coverage test, depth, excl, depth_hist and hv (hv_np; hv_scalar is the same in plain
loops, for small cases); and two exact hypervolumes to judge the estimator by: a sweep for k = 2 and
inclusion-exclusion over the clipped boxes for any k at M <= 12."""
import itertools

import numpy as np

BINS = 8
GOLDEN, MIX1, MIX2 = 0x9E3779B97F4A7C15, 0xBF58476D1CE4E5B9, 0x94D049BB133111EB
MASK = (1 << 64) - 1


def generated(Cn, k, hi=10, seed=7):
    """integer-valued costs with many ties, as tests/pareto_ref.py generates them"""
    return np.random.default_rng(seed).integers(0, hi, (Cn, k)).astype(float)


def unit(seed, i0, i1, k):
    """u[i - i0, j] in [0, 1) for the points i0 <= i < i1: uint64 arrays wrap silently"""
    i = np.arange(i0, i1, dtype=np.uint64)[:, None]
    j = np.arange(k, dtype=np.uint64)[None, :]
    x = np.uint64(seed & MASK) + np.uint64(GOLDEN) * (np.uint64(16) * i + j + np.uint64(1))
    x ^= x >> np.uint64(30)
    x *= np.uint64(MIX1)
    x ^= x >> np.uint64(27)
    x *= np.uint64(MIX2)
    x ^= x >> np.uint64(31)
    return (x >> np.uint64(11)).astype(np.float64) * 2.0 ** -53


def unit_scalar(seed, i, j):
    """the same for one coordinate in Python integers"""
    x = (seed + GOLDEN * (16 * i + j + 1)) & MASK
    x ^= x >> 30
    x = (x * MIX1) & MASK
    x ^= x >> 27
    x = (x * MIX2) & MASK
    x ^= x >> 31
    return float(x >> 11) * 2.0 ** -53


def points(lo, ref, seed, i0, i1):
    lo, ref = np.asarray(lo, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    w = ref - lo                      # rounded
    s = unit(seed, i0, i1, lo.size) * w   # rounded
    return lo + s                     # rounded: numpy never contracts


def volume(lo, ref):
    vol = 1.0
    for l, r in zip(np.asarray(lo, dtype=np.float64).tolist(), np.asarray(ref, dtype=np.float64).tolist()):
        vol *= r - l
    return vol


def _members(costs, members):
    costs = np.asarray(costs, dtype=np.float64)
    costs = costs if costs.ndim == 2 else costs.reshape(-1, 1)
    Cn = costs.shape[0]
    mem = np.arange(Cn, dtype=np.int64) if members is None else np.asarray(members, dtype=np.int64).reshape(-1)
    return costs, mem, np.flatnonzero((mem >= 0) & (mem < Cn))   # an entry outside [0, C) is skipped


def hv_np(costs, members, lo, ref, N, seed, budget=1 << 24):
    """(n_covered, excl[M], depth_hist[8], hv) of the contract, in chunks of points"""
    costs, mem, pos = _members(costs, members)
    A = costs[mem[pos]]                                   # a NaN row covers nothing: NaN <= p is false
    k = len(np.atleast_1d(lo))
    excl = np.zeros(mem.size, dtype=np.int64)
    hist = np.zeros(BINS, dtype=np.int64)
    step = max(1, budget // (A.shape[0] * k + 1))
    for i0 in range(0, N, step):
        P = points(lo, ref, seed, i0, min(N, i0 + step))
        le = (A[None, :, :k] <= P[:, None, :]).all(axis=2)
        depth = le.sum(axis=1)
        hist += np.bincount(np.minimum(depth, BINS - 1), minlength=BINS)
        one = depth == 1
        if one.any():
            np.add.at(excl, pos[le[one].argmax(axis=1)], 1)
    n_cov = int(N - hist[0])
    return n_cov, excl, hist, (float(n_cov) / float(N)) * volume(lo, ref)


def hv_scalar(costs, members, lo, ref, N, seed):
    """the contract in plain loops"""
    costs, mem, _ = _members(costs, members)
    k = len(lo)
    excl = np.zeros(mem.size, dtype=np.int64)
    hist = np.zeros(BINS, dtype=np.int64)
    for i in range(N):
        p = [float(np.float64(lo[j]) + np.float64(unit_scalar(seed, i, j)) * (np.float64(ref[j]) - np.float64(lo[j])))
             for j in range(k)]
        cover = [m for m, c in enumerate(mem) if 0 <= c < costs.shape[0] and all(costs[c, j] <= p[j] for j in range(k))]
        hist[min(len(cover), BINS - 1)] += 1
        if len(cover) == 1:
            excl[cover[0]] += 1
    n_cov = int(N - hist[0])
    return n_cov, excl, hist, (float(n_cov) / float(N)) * volume(lo, ref)


def compare(got, want, what=""):
    """exact: integers for integers, hv bit for bit; a field of `got` that is None was not asked for"""
    names = ("n_covered", "excl", "depth_hist", "hv")
    for n, g, w in zip(names, got, want):
        if g is None:
            continue
        if n == "hv":
            assert np.float64(g).tobytes() == np.float64(w).tobytes(), "%s hv: %r != %r" % (what, g, w)
        elif n == "n_covered":
            assert int(g) == int(w), "%s n_covered: %d != %d" % (what, g, w)
        else:
            np.testing.assert_array_equal(np.asarray(g), w, err_msg="%s %s" % (what, n))


# ---- exact hypervolumes ------------------------------------------------------------------------
def _corners(costs, members, lo, ref):
    """lower corners of the members' boxes clipped to [lo, ref]; a box of no volume is dropped"""
    costs, mem, pos = _members(costs, members)
    A = costs[mem[pos]]
    A = A[~np.isnan(A).any(axis=1)]
    A = np.maximum(A, np.asarray(lo, dtype=float))
    return A[(A < np.asarray(ref, dtype=float)).all(axis=1)]


def exact_2d(costs, members, lo, ref):
    """area of the union of [a, ref] inside the box, by a sweep over the first coordinate"""
    A = _corners(costs, members, lo, ref)
    if A.shape[0] == 0:
        return 0.0
    A = A[np.argsort(A[:, 0], kind="stable")]
    xs = np.append(A[:, 0], ref[0])
    ymin = np.minimum.accumulate(A[:, 1])
    return float(np.sum((xs[1:] - xs[:-1]) * (ref[1] - ymin)))


def exact_ie(costs, members, lo, ref):
    """volume of the union of [a, ref] inside the box by inclusion-exclusion (M <= 12)"""
    A = _corners(costs, members, lo, ref)
    assert A.shape[0] <= 12
    total = 0.0
    for n in range(1, A.shape[0] + 1):
        for S in itertools.combinations(range(A.shape[0]), n):
            corner = A[list(S)].max(axis=0)
            total += (-1.0) ** (n + 1) * float(np.prod(np.asarray(ref, dtype=float) - corner))
    return total
