"""Scalar restatement of the Pareto contract of include/mpct.h (mpct_pareto_device / mpct_pareto): two
nested loops for dominance, peeling for the layers.  `pareto_np` is the same contract with the inner
loop vectorised, for the cases too large for the scalar loops; tests/test_pareto.py holds the two equal.
All results are integers, so every comparison against this file is exact."""
import math

import numpy as np


def generated(C, k, hi):
    """The seeded costs of the tests and of tools/pareto_bench.py: small integers, so ties and duplicates."""
    return np.random.default_rng(7).integers(0, hi, (C, k)).astype(float)


def valid_row(row):
    return not any(math.isnan(x) for x in row)


def dominates(a, b):
    """a dominates b: both valid, a_j <= b_j for every j, a_j < b_j for at least one j."""
    if not (valid_row(a) and valid_row(b)):
        return False
    le, lt = True, False
    for x, y in zip(a, b):
        le = le and (x <= y)
        lt = lt or (x < y)
    return le and lt


def pareto_scalar(costs, max_layers=0):
    """(dom_count [C], layer [C] or None, front [C], n_front) as the library writes them."""
    M = np.asarray(costs, dtype=float)
    A = [[float(x) for x in row] for row in (M if M.ndim == 2 else M.reshape(-1, 1))]
    C = len(A)
    valid = [valid_row(r) for r in A]
    dom = [-1] * C
    for b in range(C):
        if valid[b]:
            dom[b] = sum(1 for a in range(C) if dominates(A[a], A[b]))
    members = [c for c in range(C) if valid[c] and dom[c] == 0]
    front = members + [-1] * (C - len(members))
    layer = None
    if max_layers > 0:
        layer = [-1 if not valid[c] else max_layers for c in range(C)]
        alive = [c for c in range(C) if valid[c]]
        for p in range(max_layers):  # peel the front of what is left
            top = [b for b in alive if not any(dominates(A[a], A[b]) for a in alive)]
            for b in top:
                layer[b] = p
            alive = [c for c in alive if layer[c] == max_layers]
    return (np.array(dom, dtype=np.int32), None if layer is None else np.array(layer, dtype=np.int32),
            np.array(front, dtype=np.int32), len(members))


def dominance_matrix(costs):
    """D[a, b] = a dominates b (bool [C, C]); rows and columns of invalid candidates are False."""
    A = np.asarray(costs, dtype=float)
    A = A if A.ndim == 2 else A.reshape(-1, 1)
    C, k = A.shape
    le = np.ones((C, C), dtype=bool)
    lt = np.zeros((C, C), dtype=bool)
    with np.errstate(invalid="ignore"):
        for j in range(k):
            le &= A[:, None, j] <= A[None, :, j]
            lt |= A[:, None, j] < A[None, :, j]
    valid = ~np.isnan(A).any(axis=1)
    return le & lt & valid[:, None] & valid[None, :], valid


def pareto_np(costs, max_layers=0):
    """The contract again, vectorised over the competitors (same return as pareto_scalar)."""
    A = np.asarray(costs, dtype=float)
    C = A.shape[0]
    if C == 0:
        z = np.zeros(0, dtype=np.int32)
        return z, (z.copy() if max_layers > 0 else None), z.copy(), 0
    D, valid = dominance_matrix(A)
    dom = np.where(valid, D.sum(axis=0), -1).astype(np.int32)
    members = np.nonzero(valid & (dom == 0))[0]
    front = np.full(C, -1, dtype=np.int32)
    front[:members.size] = members
    layer = None
    if max_layers > 0:
        layer = np.where(valid, max_layers, -1).astype(np.int32)
        alive = valid.copy()
        for p in range(max_layers):
            top = alive & (D[alive].sum(axis=0) == 0)
            layer[top] = p
            alive &= ~top
            if not alive.any():
                break
    return dom, layer, front, int(members.size)


def layers_by_recursion(costs):
    """layer[c] = 0 without a dominator, else 1 + the largest layer among c's dominators (unclamped);
    -1 for invalid candidates.  Dominance is a strict partial order, so the recursion ends."""
    D, valid = dominance_matrix(costs)
    C = D.shape[0]
    layer = np.full(C, -1, dtype=np.int64)
    order = np.argsort(D.sum(axis=0), kind="stable")  # a dominator has strictly fewer dominators
    for c in order:
        if valid[c]:
            doms = np.nonzero(D[:, c])[0]
            layer[c] = 0 if doms.size == 0 else 1 + layer[doms].max()
    return layer


def n_layers(costs):
    """number of non-empty layers of the full peeling"""
    lay = layers_by_recursion(costs)
    return int(lay.max()) + 1 if (lay >= 0).any() else 0


def compare(got, want, what=""):
    """Exact comparison of a (dom_count, layer, front, n_front) result with a reference's; fields that are
    None on either side are not compared.  Raises AssertionError naming the first field that differs."""
    names = ("dom_count", "layer", "front")
    for name, g, w in zip(names, got[:3], want[:3]):
        if g is None or w is None:
            continue
        g, w = np.asarray(g), np.asarray(w)
        assert g.shape == w.shape, "%s %s: shape %s != %s" % (what, name, g.shape, w.shape)
        bad = np.nonzero(g != w)[0]
        assert bad.size == 0, "%s %s differs at %d of %d entries, first c = %d: got %d, want %d" % (
            what, name, bad.size, g.size, bad[0], g[bad[0]], w[bad[0]])
    if got[3] is not None and want[3] is not None:
        assert int(got[3]) == int(want[3]), "%s n_front: got %d, want %d" % (what, int(got[3]), int(want[3]))
