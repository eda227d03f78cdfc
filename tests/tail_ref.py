"""The yardstick of the tail statistics (mpct_eval_robust_tail, include/mpct.h): a scalar Python
restatement of the header's contract.  A Python float is an IEEE double; every sum is a sequential
loop with one accumulator (numpy.sum is pairwise and is never used for a tail); the level's rank is
math.ceil(a * float(n)); the survivors are ordered by `sorted` on (J, -k), which is exact (and -0.0
== 0.0 in a tuple comparison, as the contract asks)."""
import math

import numpy as np

NAN = math.nan
FIELDS = ("quantile", "cvar", "q_draw")


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int64 if a.dtype == np.float64 else a.dtype)


def tail_ref(J1, st, j_bound, levels):
    """J1 [C, D, my], st [C, D] or None (read as 0), j_bound (0 = 1e100), levels [nlev] ->
    dict(quantile, cvar [C, nlev] float64, q_draw [C, nlev] int32, n [C])."""
    J1 = np.asarray(J1, dtype=np.float64)
    Cn, D, my = J1.shape
    bound = 1e100 if j_bound == 0.0 else float(j_bound)
    levels = [float(a) for a in np.atleast_1d(levels)]
    nlev = len(levels)
    out = dict(quantile=np.empty((Cn, nlev)), cvar=np.empty((Cn, nlev)), q_draw=np.empty((Cn, nlev), np.int32),
               n=np.empty(Cn, np.int32))
    for c in range(Cn):
        rows = J1[c].tolist()
        sts = [0] * D if st is None else np.asarray(st[c]).tolist()
        surv, sor = [], 0
        for k in range(D):
            sor |= sts[k]
            J = 0.0
            for i in range(my):
                J += rows[k][i]
            if sts[k] == 0 and math.isfinite(J) and J <= bound:
                surv.append((J, -k))
        if sor & (8 | 16):      # never simulated
            surv = []
        surv.sort()             # J ascending, among equal J the draw index descending
        n = len(surv)
        out["n"][c] = n
        for j, a in enumerate(levels):
            if n == 0:
                out["quantile"][c, j], out["cvar"][c, j], out["q_draw"][c, j] = NAN, NAN, -1
                continue
            m = min(max(math.ceil(a * float(n)), 1), n)
            acc = 0.0
            for r in range(m - 1, n):
                acc += surv[r][0]
            out["quantile"][c, j] = surv[m - 1][0]
            out["q_draw"][c, j] = -surv[m - 1][1]
            out["cvar"][c, j] = acc / (n - m + 1)
    return out


def assert_same_tail(got, want, fields=FIELDS, msg=""):
    """Bit for bit, NaN matched by position (a NaN's payload included); shapes too."""
    for f in fields:
        g, w = np.asarray(got[f]), np.asarray(want[f])
        assert g.shape == w.shape and g.dtype == w.dtype, (f, g.shape, w.shape, g.dtype, w.dtype, msg)
        np.testing.assert_array_equal(bits(g), bits(w), err_msg="%s %s" % (f, msg))
