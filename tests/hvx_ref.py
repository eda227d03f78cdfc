"""References for the exact hypervolume of mpct_hypervolume_exact (include/mpct.h): two that
share nothing with the device's sweep, and the sweep itself in numpy.

exact_fraction   any doubles, exact rational arithmetic over the coordinate-compressed grid (M <= 48)
exact_lattice    integer coordinates, occupancy grid and cumulative sums in int64 (thousands of members)
sweep_numpy      the sweep of the kernel in numpy: the same terms in another order of summation
"""
from fractions import Fraction

import numpy as np

EPS = Fraction(1, 2 ** 53)


def bound(M, vol):
    """the contract's error bound as a Fraction: (M^2 + 8) 2^-53 vol"""
    return (M * M + 8) * EPS * Fraction(float(vol))


def clipped(costs, members, lo, ref):
    """(b, act, mem): the entries' clipped vectors [M, k] (garbage where inactive) and which are active"""
    costs = np.asarray(costs, dtype=np.float64)
    costs = costs if costs.ndim == 2 else costs.reshape(-1, 1)
    Cn, k = costs.shape
    lo, ref = np.asarray(lo, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    mem = np.arange(Cn, dtype=np.int64) if members is None else np.asarray(members, dtype=np.int64).reshape(-1)
    ok = (mem >= 0) & (mem < Cn)
    rows = np.full((mem.size, k), np.nan)
    rows[ok] = costs[mem[ok]]
    with np.errstate(invalid="ignore"):
        b = np.where(rows > lo, rows, lo) + 0.0
        act = ok & ~np.isnan(rows).any(axis=1) & (b < ref).all(axis=1)
    return b, act, mem


def exact_fraction(costs, members, lo, ref):
    """(HV, EXCL[M], n_active) as Fractions: cells of the grid through every clipped coordinate, hv = the
    cells of depth >= 1, excl[m] = the cells of depth 1 that entry m covers"""
    b, act, mem = clipped(costs, members, lo, ref)
    M, k = b.shape
    ref = np.asarray(ref, dtype=np.float64)
    pos = np.flatnonzero(act)
    excl = [Fraction(0)] * M
    if pos.size == 0:
        return Fraction(0), excl, 0
    A = b[pos]
    cover, widths, den = [], [], 1
    for j in range(k):
        g = np.unique(A[:, j])                                       # cell lower corners, ascending
        edges = [Fraction(float(v)) for v in g] + [Fraction(float(ref[j]))]
        w = [edges[i + 1] - edges[i] for i in range(g.size)]
        d = max(x.denominator for x in w)                            # powers of two: the largest is the common one
        widths.append(np.array([int(x * d) for x in w], dtype=object))
        den *= d
        cover.append((A[:, j][:, None] <= g[None, :]).astype(np.int64))   # [n, cells_j]
    while len(cover) < 3:
        cover.append(np.ones((pos.size, 1), dtype=np.int64))
        widths.append(np.array([1], dtype=object))
    depth = np.einsum("mi,mj,ml->ijl", *cover)
    holder = np.einsum("m,mi,mj,ml->ijl", np.arange(1, pos.size + 1), *cover)
    W = widths[0][:, None, None] * widths[1][None, :, None] * widths[2][None, None, :]
    hv = Fraction(int(W[depth >= 1].sum()), den)
    one = depth == 1
    for t, m in enumerate(pos):
        sel = one & (holder == t + 1)
        if sel.any():
            excl[m] = Fraction(int(W[sel].sum()), den)
    return hv, excl, int(pos.size)


def exact_lattice(icosts, members, ilo, iref):
    """(hv, excl[M], n_active) in unit cells, all int64, for integer coordinates: depth per unit cell by 3-D
    cumulative sums of the occupancy grid, the holder of a depth-1 cell by those of (entry + 1)"""
    icosts = np.asarray(icosts, dtype=np.int64)
    icosts = icosts if icosts.ndim == 2 else icosts.reshape(-1, 1)
    Cn, k = icosts.shape
    ilo, iref = np.asarray(ilo, dtype=np.int64), np.asarray(iref, dtype=np.int64)
    mem = np.arange(Cn, dtype=np.int64) if members is None else np.asarray(members, dtype=np.int64).reshape(-1)
    ok = (mem >= 0) & (mem < Cn)
    b = np.zeros((mem.size, k), dtype=np.int64)
    b[ok] = np.maximum(icosts[mem[ok]], ilo)
    act = ok & (b < iref).all(axis=1)
    pos = np.flatnonzero(act)
    excl = np.zeros(mem.size, dtype=np.int64)
    if pos.size == 0:
        return 0, excl, 0
    shape = tuple(int(v) for v in (iref - ilo)) + (1,) * (3 - k)
    at = tuple((b[pos, j] - ilo[j]) if j < k else np.zeros(pos.size, dtype=np.int64) for j in range(3))
    depth = np.zeros(shape, dtype=np.int64)
    holder = np.zeros(shape, dtype=np.int64)
    np.add.at(depth, at, 1)
    np.add.at(holder, at, np.arange(1, pos.size + 1))
    for ax in range(3):
        depth = np.cumsum(depth, axis=ax)
        holder = np.cumsum(holder, axis=ax)
    cnt = np.bincount(holder[depth == 1], minlength=pos.size + 1)
    excl[pos] = cnt[1:pos.size + 1]
    return int(np.count_nonzero(depth >= 1)), excl, int(pos.size)


def sweep_numpy(costs, members, lo, ref):
    """(hv, excl[M], n_active) in doubles by the kernel's sweep: slabs in z order, columns in x order, a prefix
    scan of (smallest y, its holder, second smallest y); within the contract's bound of the exact values"""
    b, act, mem = clipped(costs, members, lo, ref)
    M, k = b.shape
    excl = np.zeros(M)
    pos = np.flatnonzero(act)
    n = pos.size
    if n == 0:
        return 0.0, excl, 0
    R = np.concatenate([np.asarray(ref, dtype=np.float64), np.ones(3 - k)])
    A = np.concatenate([b[pos], np.zeros((n, 3 - k))], axis=1)
    ox = np.lexsort((A[:, 2], A[:, 1], A[:, 0]))     # stable: (x, y, z, entry)
    oz = np.lexsort((A[:, 1], A[:, 0], A[:, 2]))     # (z, x, y, entry)
    zrank = np.empty(n, dtype=np.int64)
    zrank[oz] = np.arange(n)
    xs, yx, zrx, zs = A[ox, 0], A[ox, 1], zrank[ox], A[oz, 2]
    dx = np.append(xs[1:], R[0]) - xs
    z1 = np.append(zs[1:], R[2])
    part = np.zeros(n)
    hv = 0.0
    inf, none = np.full(n, np.inf), np.full(n, -1, dtype=np.int64)
    for s in np.flatnonzero(z1 > zs):
        dz = z1[s] - zs[s]
        on = zrx <= s
        m1, h, m2 = np.where(on, yx, np.inf), np.where(on, np.arange(n), -1), inf.copy()
        d = 1
        while d < n:
            a1 = np.concatenate([inf[:d], m1[:-d]])
            ha = np.concatenate([none[:d], h[:-d]])
            a2 = np.concatenate([inf[:d], m2[:-d]])
            left = a1 <= m1
            m2 = np.where(left, np.minimum(a2, m1), np.minimum(m2, a1))
            m1, h = np.where(left, a1, m1), np.where(left, ha, h)
            d *= 2
        seen = m1 < np.inf
        with np.errstate(invalid="ignore"):
            ta = np.where(seen, dx * (R[1] - m1), 0.0)
            te = np.where(seen, dx * (np.minimum(m2, R[1]) - m1), 0.0)
        hv += dz * ta.sum()
        np.add.at(part, np.maximum(h, 0), dz * te)
    excl[pos[ox]] = part
    return float(hv), excl, int(n)
