"""The hypervolume subset selection contract of include/mpct.h in numpy, on the sample points of
tests/hv_ref.py: greedy forward selection on the coverage count (select_np, vectorised over a coverage
matrix; select_scalar, the same in plain loops), the best n-subset by brute force for small cases, and an
exact comparison."""
import itertools

import numpy as np

import hv_ref as R

FIELDS = ("n_picked", "pos", "index", "gain", "covered", "hv", "ties", "n_covered_all")


def coverage(costs, members, lo, ref, N, seed, budget=1 << 24):
    """(cover [M, N] bool, mem [M]): cover[m, i] = entry m covers point i; a skipped or NaN entry covers nothing"""
    costs, mem, pos = R._members(costs, members)
    A = costs[mem[pos]]
    k = len(np.atleast_1d(lo))
    cover = np.zeros((mem.size, N), dtype=bool)
    step = max(1, budget // (A.shape[0] * k + 1))
    for i0 in range(0, N, step):
        P = R.points(lo, ref, seed, i0, min(N, i0 + step))
        cover[pos, i0:i0 + P.shape[0]] = (A[:, None, :k] <= P[None, :, :]).all(axis=2)
    return cover, mem


def _result(K, N, lo, ref, picks, n_all):
    """the eight outputs from the list of (m, index, gain, ties) per picking round"""
    out = dict(n_picked=len(picks), pos=np.full(K, -1, dtype=np.int32), index=np.full(K, -1, dtype=np.int32),
               gain=np.zeros(K, dtype=np.int64), covered=np.zeros(K, dtype=np.int64), ties=np.zeros(K, dtype=np.int32),
               n_covered_all=int(n_all))
    total = 0
    for r, (m, c, g, t) in enumerate(picks):
        total += g
        out["pos"][r], out["index"][r], out["gain"][r], out["covered"][r], out["ties"][r] = m, c, g, total, t
    out["covered"][len(picks):] = total
    vol = R.volume(lo, ref)
    out["hv"] = np.array([(float(c) / float(N)) * vol for c in out["covered"].tolist()], dtype=np.float64)
    return out


def select_np(costs, members, lo, ref, N, seed, K):
    """the contract, vectorised: a dict of the eight outputs"""
    cover, mem = coverage(costs, members, lo, ref, N, seed)
    alive = np.ones(N, dtype=bool)
    n_all = int(cover.any(axis=0).sum()) if mem.size else 0
    picks = []
    for _ in range(K if mem.size else 0):
        gains = (cover & alive[None, :]).sum(axis=1, dtype=np.int64)
        g = int(gains.max())
        if g == 0:
            break
        m = int(np.argmax(gains))                      # the first maximum: the smallest m
        picks.append((m, int(mem[m]), g, int((gains == g).sum())))
        alive &= ~cover[m]
    return _result(K, N, lo, ref, picks, n_all)


def select_scalar(costs, members, lo, ref, N, seed, K):
    """the contract in plain loops"""
    costs, mem, _ = R._members(costs, members)
    k = len(lo)
    pts = [[float(np.float64(lo[j]) + np.float64(R.unit_scalar(seed, i, j)) * (np.float64(ref[j]) - np.float64(lo[j])))
            for j in range(k)] for i in range(N)]
    covers = [set(i for i, p in enumerate(pts) if 0 <= c < costs.shape[0] and all(costs[c, j] <= p[j] for j in range(k)))
              for c in mem.tolist()]
    n_all = len(set().union(*covers)) if covers else 0
    left = set(range(N))
    picks = []
    for _ in range(K):
        gains = [len(s & left) for s in covers]
        g = max(gains) if gains else 0
        if g == 0:
            break
        m = gains.index(g)
        picks.append((m, int(mem[m]), g, sum(1 for x in gains if x == g)))
        left -= covers[m]
    return _result(K, N, lo, ref, picks, n_all)


def best_subset(costs, members, lo, ref, N, seed, n):
    """the largest coverage any n-subset of the entries reaches on the same sample set, by brute force"""
    cover, mem = coverage(costs, members, lo, ref, N, seed)
    best = 0
    for S in itertools.combinations(range(mem.size), min(n, mem.size)):
        best = max(best, int(cover[list(S)].any(axis=0).sum()))
    return best


def compare(got, want, what="", fields=FIELDS):
    """exact: integers for integers, hv bit for bit (NaN payload included); a field that `got` lacks or holds
    as None was not asked for"""
    for f in fields:
        g = got.get(f) if isinstance(got, dict) else getattr(got, f, None)
        if g is None:
            continue
        w = want[f]
        if f in ("n_picked", "n_covered_all"):
            assert int(g) == int(w), "%s %s: %d != %d" % (what, f, int(g), int(w))
        elif f == "hv":
            g = np.ascontiguousarray(g, dtype=np.float64)
            assert g.shape == w.shape and g.tobytes() == w.tobytes(), "%s hv: %r != %r" % (what, g, w)
        else:
            np.testing.assert_array_equal(np.asarray(g), w, err_msg="%s %s" % (what, f))
