"""The yardstick of the draw statistics (mpct_draw_stats, mpct_eval_robust_indices; include/mpct.h): a scalar
Python restatement of the header's contract, in the manner of tail_ref.py.  A Python float is an IEEE double;
every sum is a sequential loop with one accumulator; the level's rank is math.ceil(a * float(n)); the
survivors are ordered by `sorted` on (value, -k), which is exact (and -0.0 == 0.0 in a tuple comparison)."""
import math

import numpy as np

NAN = math.nan
BASE = ("n", "mean", "lo", "lo_draw", "hi", "hi_draw")
LEVEL = ("quantile", "cvar", "q_draw")
FIELDS = BASE + LEVEL
INT_FIELDS = ("n", "lo_draw", "hi_draw", "q_draw")
INDEX_FIELDS = ("iae", "ise", "itae", "emax", "t_emax", "over", "e_final", "settle", "tv", "du2", "dumax", "u_lo", "u_hi")
INDEX_INT = ("t_emax", "settle")


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int64) if a.dtype == np.float64 else a


def stats_ref(x, alive=None, levels=()):
    """x [C, D, m] float64 or int32, alive [C, D] or None, levels [nlev] -> dict of the nine fields:
    n, lo_draw, hi_draw int32 [C, m]; mean, lo, hi float64 [C, m]; quantile, cvar float64 and q_draw int32
    [C, m, nlev]."""
    x = np.asarray(x)
    is_int = np.issubdtype(x.dtype, np.integer)
    Cn, D, m = x.shape
    levels = [float(a) for a in np.atleast_1d(levels)] if np.size(levels) else []
    nlev = len(levels)
    out = {f: np.empty((Cn, m, nlev) if f in LEVEL else (Cn, m), np.int32 if f in INT_FIELDS else np.float64)
           for f in FIELDS}
    for c in range(Cn):
        live = [True] * D if alive is None else [int(a) != 0 for a in np.asarray(alive[c]).tolist()]
        for i in range(m):
            col = x[c, :, i]
            vals = col.tolist()
            surv = []
            n, acc, lo, hi, lod, hid = 0, 0.0, NAN, NAN, -1, -1
            for k in range(D):
                ok = live[k] and (vals[k] >= 0 if is_int else math.isfinite(vals[k]))
                if not ok:
                    continue
                v = float(vals[k])
                acc += v
                if n == 0 or v < lo:
                    lo, lod = v, k
                if n == 0 or v > hi:
                    hi, hid = v, k
                n += 1
                surv.append((v, -k))
            out["n"][c, i] = n
            out["mean"][c, i] = acc / float(n) if n else NAN
            out["lo"][c, i], out["lo_draw"][c, i] = lo, lod
            out["hi"][c, i], out["hi_draw"][c, i] = hi, hid
            surv.sort()     # value ascending, among equal values the draw index descending
            for j, a in enumerate(levels):
                if n == 0:
                    out["quantile"][c, i, j], out["cvar"][c, i, j], out["q_draw"][c, i, j] = NAN, NAN, -1
                    continue
                r = min(max(math.ceil(a * float(n)), 1), n)
                t = 0.0
                for q in range(r - 1, n):
                    t += surv[q][0]
                out["quantile"][c, i, j] = surv[r - 1][0]
                out["q_draw"][c, i, j] = -surv[r - 1][1]
                out["cvar"][c, i, j] = t / (n - r + 1)
    return out


def alive_ref(J1, status, j_bound):
    """The classification of mpct_eval_robust: J1 [C, D, my], status [C, D], j_bound (0 = 1e100) -> alive [C, D]
    int32.  Status 0, J = sum_i J1_i finite (summed over i in ascending order) and J <= bound; a candidate carrying
    MPCT_ST_SKIPPED (8) or MPCT_ST_BADHORIZON (16) on any draw has no live draw."""
    J1 = np.asarray(J1, dtype=np.float64)
    Cn, D, my = J1.shape
    bound = 1e100 if j_bound == 0.0 else float(j_bound)
    alive = np.zeros((Cn, D), np.int32)
    for c in range(Cn):
        rows, sts = J1[c].tolist(), np.asarray(status[c]).tolist()
        sor = 0
        for k in range(D):
            sor |= sts[k]
            J = 0.0
            for i in range(my):
                J += rows[k][i]
            alive[c, k] = 1 if (sts[k] == 0 and math.isfinite(J) and J <= bound) else 0
        if sor & (8 | 16):
            alive[c] = 0
    return alive


def base_ref(J1, status, j_bound):
    """mpct_eval_robust's record by the rule of robust_reduce.h: dict(mean, worst [C, my], n_failed, worst_draw,
    status [C])."""
    J1 = np.asarray(J1, dtype=np.float64)
    Cn, D, my = J1.shape
    bound = 1e100 if j_bound == 0.0 else float(j_bound)
    out = dict(mean=np.empty((Cn, my)), worst=np.empty((Cn, my)), n_failed=np.empty(Cn, np.int32),
               worst_draw=np.empty(Cn, np.int32), status=np.empty(Cn, np.int32))
    for c in range(Cn):
        rows, sts = J1[c].tolist(), np.asarray(status[c]).tolist()
        sor, nfail, nsurv, wd, jw = 0, 0, 0, -1, 0.0
        acc, mx = [0.0] * my, [0.0] * my
        for k in range(D):
            sor |= sts[k]
            J = 0.0
            for i in range(my):
                J += rows[k][i]
            if sts[k] == 0 and math.isfinite(J) and J <= bound:
                for i in range(my):
                    acc[i] += rows[k][i]
                    mx[i] = rows[k][i] if (nsurv == 0 or rows[k][i] > mx[i]) else mx[i]
                if nsurv == 0 or J > jw:
                    jw, wd = J, k
                nsurv += 1
            else:
                nfail += 1
        if sor & (8 | 16):
            nfail, nsurv, wd = 0, 0, -1
        for i in range(my):
            out["mean"][c, i] = acc[i] / float(nsurv) if nsurv else NAN
            out["worst"][c, i] = mx[i] if nsurv else NAN
        out["n_failed"][c], out["worst_draw"][c], out["status"][c] = nfail, wd, sor
    return out


def robust_indices_ref(records, J1, status, j_bound, fields, levels=()):
    """The composition mpct_eval_robust_indices stands for: records {field: [C, D, width]} of eval_indices, J1
    [C, D, my] and status [C, D] of the same launch -> (stats dict with arrays [C, W] / [C, W, nlev], the selected
    fields side by side in selection order; base dict)."""
    alive = alive_ref(J1, status, j_bound)
    parts = [stats_ref(records[f], alive, levels) for f in fields]
    stats = {f: np.concatenate([p[f] for p in parts], axis=1) for f in FIELDS}
    return stats, base_ref(J1, status, j_bound)


def assert_same_stats(got, want, fields=FIELDS, msg=""):
    """Bit for bit, NaN matched by position (a NaN's payload included); shapes and dtypes too."""
    for f in fields:
        g, w = np.asarray(got[f]), np.asarray(want[f])
        assert g.shape == w.shape and g.dtype == w.dtype, (f, g.shape, w.shape, g.dtype, w.dtype, msg)
        np.testing.assert_array_equal(bits(g), bits(w), err_msg="%s %s" % (f, msg))


def table(C, D, m, seed, as_int=False):
    """A [C, D, m] table with everything the contract names: ties at the minimum and the maximum (values from a
    small set), -0.0 against +0.0, NaN and +-inf entries, an all-dead column next to a live one, and an alive
    mask with zeros.  as_int: int32 with -1 entries instead.  Returns (x, alive)."""
    rng = np.random.default_rng(seed)
    if as_int:
        x = rng.integers(0, 6, (C, D, m)).astype(np.int32)
        x[rng.random((C, D, m)) < 0.15] = -1
    else:
        pool = np.array([-0.0, 0.0, 0.5, 0.5, 1.25, -3.0, 7.0, 1e-310, 2.0 ** -30])
        x = pool[rng.integers(0, len(pool), (C, D, m))] + np.where(rng.random((C, D, m)) < 0.3, rng.random((C, D, m)), 0.0)
        bad = rng.random((C, D, m))
        x[bad < 0.05] = np.nan
        x[(bad >= 0.05) & (bad < 0.08)] = np.inf
        x[(bad >= 0.08) & (bad < 0.11)] = -np.inf
    alive = (rng.random((C, D)) > 0.2).astype(np.int32)
    if C > 1:
        alive[C - 1] = 0                            # and a candidate without a live draw
    if D >= 3 and not as_int:
        # column (0, 0): finite values >= 1, then a tie at the minimum between zeros of both signs (lo carries the
        # -0.0 of draw 0) and, from D = 5, a tie at the maximum; those draws are alive
        col = np.abs(np.nan_to_num(x[0, :, 0], nan=1.0, posinf=2.0, neginf=3.0)) + 1.0
        col[0], col[1], col[D - 1] = -0.0, 0.0, -0.0
        alive[0, [0, 1, D - 1]] = 1
        if D >= 5:
            col[2] = col[D - 2] = 50.0
            alive[0, [2, D - 2]] = 1
        x[0, :, 0] = col
    if m > 1:
        x[0, :, m - 1] = -1 if as_int else np.nan   # an all-dead column; its neighbours stay live
    return x, alive
