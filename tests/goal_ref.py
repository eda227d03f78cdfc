"""The goal-attainment contract of include/mpct.h restated in numpy, twice: goal_scalar, a loop that follows the
contract statement by statement in the stated rounding order (Python floats: IEEE doubles, one rounding per
operation, no fused multiply-add), and goal_np, vectorised over the candidates.  Both return a dict with the
fields of mpct_goal_result.  Also the generators of the test cases and the bitwise comparison."""
import numpy as np

FIELDS = ("best", "gamma", "active", "n_feasible", "n_attained", "wins")
WEIGHTS = (3.0, 7.0, 0.1, 1e-300, 1e300, 1.0)      # they exercise the division 1 / w


def valid_goal(goal, w):
    """the validity rule of one goal / weight vector"""
    soft = False
    for gj, wj in zip(goal, w):
        gj, wj = float(gj), float(wj)
        if wj == 0.0:
            if gj != gj:
                return False
        elif wj > 0.0 and wj < np.inf:
            with np.errstate(over="ignore"):
                iw = float(np.float64(1.0) / np.float64(wj))
            if not np.isfinite(iw) or not np.isfinite(gj):
                return False
            soft = True
        else:
            return False                      # negative, NaN or infinite
    return soft


def _empty(G, Cn, nb):
    return dict(best=np.full((G, nb), -1, dtype=np.int32), gamma=np.full((G, nb), np.nan), active=np.full((G, nb), -1, dtype=np.int32),
                n_feasible=np.full(G, -1, dtype=np.int32), n_attained=np.full(G, -1, dtype=np.int32),
                wins=np.zeros(Cn, dtype=np.int32))


def _tables(A, goals, weights):
    A = np.asarray(A, dtype=np.float64)
    A = A if A.ndim == 2 else A.reshape(-1, 1)
    k = A.shape[1]
    goals = np.asarray(goals, dtype=np.float64).reshape(-1, k)
    weights = np.asarray(weights, dtype=np.float64).reshape(-1, k)
    assert goals.shape == weights.shape
    return A, goals, weights


def goal_scalar(A, goals, weights, n_best):
    """the contract as a loop over (g, c, j)"""
    A, goals, weights = _tables(A, goals, weights)
    Cn, k = A.shape
    G = goals.shape[0]
    out = _empty(G, Cn, n_best)
    for g in range(G):
        if not valid_goal(goals[g], weights[g]):
            continue
        w = [float(x) for x in weights[g]]
        gl = [float(x) for x in goals[g]]
        with np.errstate(divide="ignore"):
            iw = [float(np.float64(1.0) / np.float64(x)) if x > 0.0 else 0.0 for x in w]
        softs = [j for j in range(k) if w[j] > 0.0]
        keys, nf, na = [], 0, 0
        for c in range(Cn):
            F = [float(x) for x in A[c]]
            feas = not any(x != x for x in F)                      # 1. valid: no NaN cost
            for j in range(k):                                     # 2. hard objectives
                if w[j] == 0.0 and not F[j] <= gl[j]:
                    feas = False
            gam, act = -np.inf, softs[0]                           # 4.
            for j in softs:                                        # 3. soft objectives in ascending j
                d = F[j] - gl[j]
                term = d * iw[j]
                if term != term:                                   # 6. no NaN term
                    feas = False
                if term > gam:                                     # 5.
                    gam, act = term, j
            if feas:
                nf += 1
                na += 1 if gam <= 0.0 else 0
                keys.append((gam, c, act))
        keys.sort(key=lambda t: t[0])                              # 7. stable: ties (-0.0 == +0.0) stay in ascending c
        for i, (gam, c, act) in enumerate(keys[:n_best]):
            out["best"][g, i], out["gamma"][g, i], out["active"][g, i] = c, gam, act
        out["n_feasible"][g], out["n_attained"][g] = nf, na
        if keys:
            out["wins"][keys[0][1]] += 1
    return out


def goal_np(A, goals, weights, n_best):
    """the same, vectorised over the candidates"""
    A, goals, weights = _tables(A, goals, weights)
    Cn, k = A.shape
    G = goals.shape[0]
    out = _empty(G, Cn, n_best)
    cvalid = ~np.isnan(A).any(axis=1)
    for g in range(G):
        if not valid_goal(goals[g], weights[g]):
            continue
        soft = weights[g] > 0
        js = np.flatnonzero(soft)
        with np.errstate(invalid="ignore", over="ignore"):
            term = (A[:, js] - goals[g, js]) * (1.0 / weights[g, js])          # two roundings per element
            feas = cvalid & (A[:, ~soft] <= goals[g, ~soft]).all(axis=1) & ~np.isnan(term).any(axis=1)
        t = np.where(np.isnan(term), -np.inf, term)
        a = np.argmax(t == t.max(axis=1, keepdims=True), axis=1) if Cn else np.zeros(0, dtype=np.int64)   # first j at the maximum
        gam = t[np.arange(Cn), a]                                              # its term, the sign of a zero included
        idx = np.flatnonzero(feas)
        idx = idx[np.argsort(gam[idx], kind="stable")]
        n = min(n_best, idx.size)
        out["best"][g, :n], out["gamma"][g, :n], out["active"][g, :n] = idx[:n], gam[idx[:n]], js[a[idx[:n]]]
        out["n_feasible"][g] = idx.size
        out["n_attained"][g] = int((gam[idx] <= 0).sum())
        if idx.size:
            out["wins"][idx[0]] += 1
    return out


def compare(got, want, what="", fields=FIELDS):
    """every field bit for bit (gamma by its bit pattern: NaN padding and the sign of a zero included); a field
    that `got` holds as None was not asked for"""
    for f in fields:
        if got.get(f) is None:
            continue
        a, b = np.ascontiguousarray(got[f]), np.ascontiguousarray(want[f])
        assert a.shape == b.shape, "%s %s: shape %s against %s" % (what, f, a.shape, b.shape)
        if f == "gamma":
            a, b = a.view(np.int64), b.view(np.int64)
        bad = np.argwhere(a != b)
        assert bad.size == 0, "%s %s: %d entries differ, first at %s: %r against %r" % (
            what, f, len(bad), tuple(bad[0]), got[f][tuple(bad[0])], want[f][tuple(bad[0])])


def generated(Cn, k, hi, seed=0):
    """(Cn, k) costs quantised to the levels 0 .. hi - 1 scaled by 0.25, so that most attainment factors tie"""
    return np.random.default_rng(1000 + seed + 7 * Cn + k).integers(0, hi, size=(Cn, k)).astype(np.float64) * 0.25


def goal_vectors(G, k, hi, seed=0, hard=0.3):
    """G valid goal / weight vectors for a table of generated(., k, hi): goals on the costs' levels, weights drawn
    from WEIGHTS, a column hard with probability `hard` (its goal then in the upper levels or +INFINITY); at
    least one soft column per vector"""
    rng = np.random.default_rng(2000 + seed + 13 * G + k)
    goals = rng.integers(0, hi, size=(G, k)).astype(np.float64) * 0.25
    weights = rng.choice(np.array(WEIGHTS), size=(G, k))
    hd = rng.random((G, k)) < hard
    hd[np.arange(G), rng.integers(0, k, size=G)] = False
    weights[hd] = 0.0
    loose = rng.random((G, k))
    goals[hd & (loose < 0.5)] = (hi - 1) * 0.25
    goals[hd & (loose < 0.2)] = np.inf
    return goals, weights


INVALID = ("negative weight", "NaN weight", "subnormal weight", "all weights zero", "infinite soft goal", "NaN hard goal",
           "infinite weight")


def spoil(goals, weights, g, how):
    """make goal vector g invalid in the named way (in place)"""
    k = goals.shape[1]
    j = g % k
    if how == "negative weight":
        weights[g, j] = -1.0
    elif how == "NaN weight":
        weights[g, j] = np.nan
    elif how == "subnormal weight":
        weights[g, j] = 5e-324                 # its reciprocal overflows
    elif how == "all weights zero":
        weights[g] = 0.0
        goals[g] = np.where(np.isnan(goals[g]), 0.0, goals[g])
    elif how == "infinite soft goal":
        weights[g, j] = 2.0
        goals[g, j] = np.inf if g % 2 else -np.inf
    elif how == "NaN hard goal":
        weights[g] = 1.0
        weights[g, j] = 0.0
        goals[g, j] = np.nan
        if k == 1:
            weights[g, j] = np.nan
    elif how == "infinite weight":
        weights[g, j] = np.inf
    else:
        raise ValueError(how)
