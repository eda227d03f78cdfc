"""Goal-attainment selection on the device (mpct_goal_attain_device), timed on one GPU at the Shell 7x5
grid: C = 65,536 candidates x k = 7 objectives, and at the largest table, C = 2^20.

  device entry   mpct_goal_attain_device on resident tensors (preparation, pair and merge kernels and the scratch
                 of one call), HIP events, for G = 1, 4,096 and 65,536 goal / weight vectors at n_best 1 and 16, and
                 for C = 2^20 with G = 1 -- the shape a lane-per-goal layout serves worst.  The term rate G C k / t
                 is set against the FP64 vector peak of DESIGN §6 at two operations (F - goal, * 1/w) per term; the
                 compares and selects of a term are not counted.
  numpy          goal_np of tests/goal_ref.py (vectorised over the candidates, a Python loop over the goal vectors),
                 wall clock, on at most --np-goals goal vectors of each shape; reported per goal vector.
  check          inside the run: the rows of up to --check goal vectors of every shape equal goal_np bit for bit
                 (and wins where every goal vector was checked).

--warmup runs first, then --reps repetitions, the shapes interleaved repetition by repetition; median, min, max and
spread are reported.  The file's bench_ab block is not measured here: it records bench.py --gpus 1 --steps 20
--warmup 3 of the parent commit and of this one, run alternately from their own trees, and a rerun of this tool
keeps it.

    python tools/goal_bench.py [--reps 9] [--warmup 3] [--out profiles/r019_goal.json]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "model-predictive-control-tuning_amd"), ROOT, os.path.join(ROOT, "tests")]
import numpy as np
import torch
import goal_ref as R
from mpct import _lib, engine

ap = argparse.ArgumentParser()
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--reps", type=int, default=9)
ap.add_argument("--check", type=int, default=24)
ap.add_argument("--np-goals", type=int, default=64)
ap.add_argument("--out", default=None)
a = ap.parse_args()
DEV = torch.device("cuda", 0)
K = 7
PEAK_TFLOPS = 78.6     # MI355X FP64 vector dense peak
SHAPES = [(65536, 1, 1), (65536, 1, 16), (65536, 4096, 1), (65536, 4096, 16), (65536, 65536, 1), (65536, 65536, 16),
          (1 << 20, 1, 1), (1 << 20, 1, 16)]


def stats(t):
    t = np.sort(np.asarray(t))
    return {"median_ms": float(np.median(t)), "min_ms": float(t[0]), "max_ms": float(t[-1]),
            "spread_pct": float(100.0 * (t[-1] - t[0]) / np.median(t)), "all_ms": [float(x) for x in t]}


def table(Cn):
    """a cost table with the spread of an index table: lognormal columns, a few NaN rows and infinities"""
    A = np.random.default_rng(Cn).lognormal(size=(Cn, K))
    A[::997, 3] = np.nan
    A[5::1999, 1] = np.inf
    return A


def vectors(G, A):
    """weight directions on the simplex, goals at the column minima; columns 5 and 6 hard at their medians for
    every other goal vector"""
    rng = np.random.default_rng(G)
    w = rng.dirichlet(np.ones(K), size=G) + 1e-3
    goals = np.tile(np.nanmin(np.where(np.isfinite(A), A, np.nan), axis=0), (G, 1))
    w[1::2, 5:] = 0.0
    goals[1::2, 5:] = np.nanmedian(A[:, 5:], axis=0)
    return goals, w


def geometry(G, Cn):
    g = np.zeros(3, dtype=np.int32)
    assert _lib.load().mpct_internal_goal_geometry(G, Cn, g.ctypes.data_as(_lib.c_int32_p)) == 0
    return {"tile": int(g[0]), "chunks": int(g[1]), "chunk": int(g[2])}


tables = {Cn: table(Cn) for Cn in sorted({s[0] for s in SHAPES})}
dev_tables = {Cn: torch.from_numpy(A).to(DEV) for Cn, A in tables.items()}
cases = []
for Cn, G, nb in SHAPES:
    goals, w = vectors(G, tables[Cn])
    out = dict(best=torch.empty((G, nb), dtype=torch.int32, device=DEV), gamma=torch.empty((G, nb), dtype=torch.float64, device=DEV),
               active=torch.empty((G, nb), dtype=torch.int32, device=DEV), n_feasible=torch.empty(G, dtype=torch.int32, device=DEV),
               n_attained=torch.empty(G, dtype=torch.int32, device=DEV), wins=torch.empty(Cn, dtype=torch.int32, device=DEV))
    cases.append(dict(C=Cn, G=G, n_best=nb, goals=goals, w=w, tg=torch.from_numpy(goals).to(DEV), tw=torch.from_numpy(w).to(DEV),
                      out=out, t=[]))


def run(c):
    engine.goal_attain_device(dev_tables[c["C"]], c["tg"], c["tw"], c["out"], n_best=c["n_best"])


for c in cases:
    for _ in range(a.warmup):
        run(c)
torch.cuda.synchronize()
for _ in range(a.reps):
    for c in cases:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        run(c)
        e1.record()
        e1.synchronize()
        c["t"].append(e0.elapsed_time(e1))

res = {"tool": "tools/goal_bench.py", "device": torch.cuda.get_device_name(0), "k": K, "warmup": a.warmup, "reps": a.reps,
       "peak_fp64_tflops": PEAK_TFLOPS, "shapes": []}
for c in cases:
    Cn, G, nb = c["C"], c["G"], c["n_best"]
    s = stats(c["t"])
    terms = float(G) * Cn * K
    rate = terms / (s["median_ms"] * 1e-3)
    # the check: a sub-sample of the goal vectors against the vectorised reference, bit for bit
    n = min(G, a.check)
    rows = np.unique(np.linspace(0, G - 1, n).astype(np.int64))
    want = R.goal_np(tables[Cn], c["goals"][rows], c["w"][rows], nb)
    got = {f: v.cpu().numpy() for f, v in c["out"].items()}
    sub = {f: (got[f] if f == "wins" else got[f][rows]) for f in R.FIELDS}
    R.compare(sub, want, "C %d G %d n_best %d" % (Cn, G, nb), fields=R.FIELDS if rows.size == G else R.FIELDS[:5])
    rec = {"C": Cn, "G": G, "n_best": nb, **geometry(G, Cn), "device_entry": s, "terms": terms,
           "terms_per_s": rate, "fp64_fraction_of_peak": 2.0 * rate / (PEAK_TFLOPS * 1e12), "checked_goal_vectors": int(rows.size),
           "bitwise": True, "winners": int((got["wins"] > 0).sum())}
    if nb == 1:
        m = min(G, a.np_goals)
        t0 = time.perf_counter()
        R.goal_np(tables[Cn], c["goals"][:m], c["w"][:m], nb)
        rec["numpy"] = {"goal_vectors": m, "ms_per_goal_vector": 1e3 * (time.perf_counter() - t0) / m}
        rec["numpy"]["ms_for_G_extrapolated"] = rec["numpy"]["ms_per_goal_vector"] * G
    res["shapes"].append(rec)
    print(json.dumps({k_: (round(v, 4) if isinstance(v, float) else v) for k_, v in rec.items() if k_ not in ("device_entry", "numpy")}
                     | {"median_ms": round(s["median_ms"], 4), "min_ms": round(s["min_ms"], 4), "max_ms": round(s["max_ms"], 4)}
                     | ({"numpy_ms_per_g": round(rec["numpy"]["ms_per_goal_vector"], 3)} if "numpy" in rec else {})), flush=True)

if a.out:
    if os.path.exists(a.out):
        with open(a.out) as f:
            old = json.load(f)
        if "bench_ab" in old:
            res["bench_ab"] = old["bench_ab"]
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
