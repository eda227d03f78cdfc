"""The MEX gateway's 'draw_stats' and 'eval_robust_indices' commands (matlab/mpct_mex.c) through the MX stub, built
and driven like tests/test_mex_indices.py: argument errors without a device (the gateway's own and the library's
messages), and on the GPU the struct's fields against tests/draw_stats_ref.py and the Python host, bit for bit, in
MATLAB's layouts (x D x m x C in, C x m and C x m x nlev fields out, 0-based draws)."""
import subprocess

import numpy as np
import pytest

import draw_stats_ref as R
from test_mex import _parse_out, mex, shell3x3_desc, spec

LEVELS = [0.9, 1.0, 1e-9, 0.5]
NAMES = set(R.FIELDS) | {"levels"}


def _pages(x):
    """[C, D, m] -> MATLAB D x m x C"""
    return np.ascontiguousarray(np.transpose(x, (1, 2, 0)))


def test_mex_draw_stats_argument_errors(built, has_gpu):
    x, alive = R.table(3, 5, 2, 11)
    X, A = _pages(x), np.ascontiguousarray(alive.T)
    _, r, d = shell3x3_desc()
    one = [[30.0], [5.0], np.ones((1, 3)), np.ones((1, 3)), r]
    res = mex([(1, ["draw_stats"]),
               (1, ["draw_stats", X, A[:4]]),                                  # alive with another D
               (1, ["draw_stats", X, A, np.full(9, 0.5)]),                     # nine levels
               (1, ["draw_stats", X, A, [0.5, 1.5]]),                          # the library's MPCT_EINVAL
               (1, ["draw_stats", X, A, [0.5], 0.5]),
               (1, ["draw_stats", np.zeros((5000, 1, 2)), np.zeros((0, 0)), [0.5]]),   # the library's MPCT_ERANGE
               (1, ["eval_robust_indices", 0.0]),
               (1, ["create", d]),
               (1, ["eval_robust_indices", ("P", 7, 0)] + one + [np.zeros((0, 0)), {"fields": np.arange(14.0)}]),
               (1, ["eval_robust_indices", ("P", 7, 0)] + one + [np.zeros((0, 0)), {"fields": [8.0, 13.0]}]),
               (1, ["eval_robust_indices", ("P", 7, 0)] + one + [np.zeros((0, 0)), {"fields": [8.0, 5.0, 8.0]}]),
               (1, ["eval_robust_indices", ("P", 7, 0)] + one + [np.zeros((0, 0)), {"levels": [0.0]}]),
               (1, ["eval_robust_indices", ("P", 7, 0)] + one + [np.zeros((0, 0)), {"j_bound": -1.0}]),
               (1, ["eval_robust_indices", ("P", 7, 0)] + one + [np.zeros((0, 0)), {"t0": 500.0}])])
    assert not res[0][0] and res[0][1][0] == "mpct:arg" and "usage" in res[0][1][1]
    assert res[1] == (False, ("mpct:arg", "'alive' must be D x C like 'x'"))
    assert not res[2][0] and res[2][1][0] == "mpct:arg" and "'levels' must hold" in res[2][1][1]
    assert not res[3][0] and res[3][1][0] == "mpct:draw_stats" and "every level" in res[3][1][1]
    assert res[4] == (False, ("mpct:arg", "'device' must be an integer"))
    assert not res[5][0] and res[5][1][0] == "mpct:draw_stats" and "MPCT_TAIL_MAX_DRAWS" in res[5][1][1]
    assert not res[6][0] and res[6][1][0] == "mpct:arg" and "usage" in res[6][1][1]
    assert res[7][0]
    assert not res[8][0] and res[8][1][0] == "mpct:arg" and "'fields' must hold" in res[8][1][1]
    assert res[9] == (False, ("mpct:eval_robust_indices", "field id out of range"))
    assert res[10] == (False, ("mpct:eval_robust_indices", "field id repeated"))
    assert not res[11][0] and res[11][1][0] == "mpct:eval_robust_indices" and "every level" in res[11][1][1]
    assert not res[12][0] and res[12][1][0] == "mpct:eval_robust_indices" and "j_bound" in res[12][1][1]
    assert res[13] == (False, ("mpct:eval_robust_indices", "t0 must be 0 .. nit-1"))
    if not has_gpu:
        res = mex([(1, ["draw_stats", X, A, [0.5]])])
        assert not res[0][0] and res[0][1][0] == "mpct:draw_stats" and "device" in res[0][1][1]


def _fields_of(lines, k, at):
    mine = lines[at[k]:at[k + 1] if k + 1 < len(at) else None]
    return {ln.split()[2]: _parse_out(ln.split()[3:]) for ln in mine if ln.startswith("FIELD 0 ")}


def _same(got, want, f, msg):
    """a MEX field (doubles; C x w x nlev loses trailing singleton pages) against the reference's array"""
    g = np.asarray(got[f], dtype=np.float64).reshape(want[f].shape)
    assert (R.bits(g) == R.bits(want[f].astype(np.float64))).all(), (f, msg)


@pytest.mark.gpu
def test_mex_draw_stats_match_reference_and_python_host(built, has_gpu):
    if not has_gpu:
        pytest.skip("no GPU")
    from test_robust_gpu import _build_driver
    from mpct.engine import eval_robust_indices
    from mpct.scenarios import candidate_grid, vns_step_refs

    x, alive = R.table(5, 65, 3, 21)
    xi, _ = R.table(5, 65, 3, 22, True)
    sc, _, d = shell3x3_desc()
    N2, Nu, dl, lm = candidate_grid(4)
    N2[2] = 0                                             # a candidate that is not run: n = 0, NaN / -1
    refs = vns_step_refs(3, 500)
    ids = [8, 5, 7]                                       # tv, over, settle
    par = {"fields": np.array(ids, dtype=float), "levels": np.array(LEVELS[:3]), "t0": 10.0, "band_rel": 0.05}
    calls = [(1, ["draw_stats", _pages(x), np.ascontiguousarray(alive.T).astype(float), np.array(LEVELS)]),
             (1, ["draw_stats", _pages(xi), np.ascontiguousarray(alive.T).astype(float), np.array(LEVELS)]),
             (1, ["draw_stats", _pages(x)]),
             (1, ["create", d]),
             (1, ["eval_robust_indices", ("P", 3, 0), N2.astype(float), Nu.astype(float), dl, lm,
                  np.ascontiguousarray(np.transpose(refs, (1, 2, 0))), np.zeros((0, 0)), par])]
    text = "\n".join("CALL %d %d\n%s" % (nl, len(args), "\n".join(spec(a) for a in args)) for nl, args in calls)
    out = subprocess.run([_build_driver()], input=text, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    lines = out.stdout.splitlines()
    assert all("CALL %d OK" % k in lines for k in range(5)), out.stdout[-2000:]
    at = [i for i, ln in enumerate(lines) if ln.startswith("CALL ")]
    for k, (tab, msg) in enumerate([(x, "double"), (xi, "int32")]):
        want = R.stats_ref(tab, alive, LEVELS)
        got = _fields_of(lines, k, at)
        assert set(got) == NAMES and got["hi"].shape == (5, 3) and got["cvar"].shape == (5, 3, 4)
        for f in R.FIELDS:                                # C x m (x nlev), not transposed; draws 0-based
            _same(got, want, f, msg)
        assert got["levels"].ravel().tolist() == LEVELS
    bare = _fields_of(lines, 2, at)
    want = R.stats_ref(x, None, [])
    for f in R.BASE:
        _same(bare, want, f, "no alive, no levels")
    assert all(bare[f].size == 0 for f in R.LEVEL + ("levels",))
    # the scored batch: the Python host's record of the same call
    ev = _fields_of(lines, 4, at)
    names = [R.INDEX_FIELDS[i] for i in ids]
    py = eval_robust_indices(sc, N2, Nu, dl, lm, refs, fields=names, levels=LEVELS[:3], t0=10, band_rel=0.05, device=0)
    assert set(ev) == NAMES | {"field", "channel", "J1_mean", "J1_worst", "n_failed", "worst_draw", "status"}
    assert ev["field"].ravel().tolist() == [8] * 3 + [5] * 3 + [7] * 3 and ev["channel"].ravel().tolist() == [1, 2, 3] * 3
    assert [(R.INDEX_FIELDS[int(f)], int(c) - 1) for f, c in zip(ev["field"].ravel(), ev["channel"].ravel())] == py.columns
    for f in R.FIELDS:
        _same(ev, {f: getattr(py, f)}, f, "eval_robust_indices")
    assert (R.bits(ev["J1_mean"]) == R.bits(py.base.mean)).all() and (R.bits(ev["J1_worst"]) == R.bits(py.base.worst)).all()
    for f in ("n_failed", "worst_draw", "status"):
        assert (ev[f][:, 0] == getattr(py.base, f)).all(), f
    assert (ev["n"][2] == 0).all() and np.isnan(ev["hi"][2]).all() and ev["status"][2, 0] == 8
    assert (ev["n"][[0, 1, 3]] == 3).all() and np.isfinite(ev["hi"][[0, 1, 3]]).all()
