"""Hypervolume of a front and per-member contributions (mpct_hypervolume_device), timed on one
GPU against the same contract written two other ways:

  (a) mpct_hypervolume_device: all four outputs, at the default tile and with T = 128 and T = 256 forced
      (mpct_internal_hv_tuned), and once with the -1-padded front buffer of mpct_pareto_device as it is (M = C);
  (b) the contract as chunked torch expressions on the device (mpct.dist._hypervolume_torch);
  (c) the contract as chunked numpy on the CPU (wall clock), at --numpy-samples points, scaled to N and
      labelled as scaled.

Shapes: the fronts of the 4,096 x 3 and the 65,536 x 7 table of tools/pareto_bench.py (costs numpy.random
.default_rng(7).integers(0, 1000, (C, k))), computed in the run by mpct_pareto_device; box [0, 1000]^k;
N = 2^20 points.  HIP-event timings, --warmup launches and --reps repetitions per route, interleaved a, b, a,
b, .. so that clock drift hits all alike; median, min, max and spread are reported, and the routes' results
are compared (all integers, hv bit for bit).

python tools/hv_bench.py [--reps N] [--out profiles/r014_hypervolume.json]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "model-predictive-control-tuning_amd"), ROOT]
import numpy as np
import torch
from mpct import _lib
from mpct.dist import _hypervolume_torch
from mpct.engine import hypervolume_device, pareto_device

ap = argparse.ArgumentParser()
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--reps", type=int, default=11)
ap.add_argument("--torch-reps", type=int, default=5)
ap.add_argument("--samples", type=int, default=1 << 20)
ap.add_argument("--numpy-samples", type=int, default=1 << 14)
ap.add_argument("--seed", type=int, default=1)
ap.add_argument("--hi", type=int, default=1000)
ap.add_argument("--out", default=None)
a = ap.parse_args()
DEV = torch.device("cuda", 0)
SHAPES = ((4096, 3), (65536, 7))


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def stats(t):
    t = np.sort(np.asarray(t))
    return {"median_ms": float(np.median(t)), "min_ms": float(t[0]), "max_ms": float(t[-1]),
            "spread_pct": float(100.0 * (t[-1] - t[0]) / np.median(t)), "all_ms": [float(x) for x in t]}


def interleaved(routes, warmup, reps):
    """{name: stats} of the (callable, reps) in `routes`, run warm-ups first and then a, b, .., a, b, .."""
    for fn, _ in routes.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    t = {n: [] for n in routes}
    for r in range(max(n for _, n in routes.values())):
        for name, (fn, n) in routes.items():
            if r < n:
                t[name].append(timed(fn))
    return {n: stats(v) for n, v in t.items()}


def device_route(costs, members, lo, ref, N, tile=0):
    """(callable, output tensors) of one device-entry call into fresh tensors, with the tile forced or not"""
    M = costs.shape[0] if members is None else members.numel()
    out = dict(n_covered=torch.empty(1, dtype=torch.int64, device=DEV), excl=torch.empty(M, dtype=torch.int64, device=DEV),
               depth_hist=torch.empty(8, dtype=torch.int64, device=DEV), hv=torch.empty(1, dtype=torch.float64, device=DEV))
    lib = _lib.load()

    def run():
        lib.mpct_internal_hv_tuned(tile, 0)
        try:
            hypervolume_device(costs, out, lo, ref, members=members, n_samples=N, seed=a.seed)
        finally:
            lib.mpct_internal_hv_tuned(0, 0)

    return run, out


def hv_numpy(A, mem, lo, ref, N, seed, budget=1 << 25):
    """the contract on the CPU: wrapping uint64 sample points, chunked broadcasting"""
    rows = A[mem]
    k = A.shape[1]
    excl = np.zeros(mem.size, dtype=np.int64)
    hist = np.zeros(8, dtype=np.int64)
    step = max(1, budget // (rows.shape[0] * k + 1))
    for i0 in range(0, N, step):
        i = np.arange(i0, min(N, i0 + step), dtype=np.uint64)[:, None]
        x = np.uint64(seed) + np.uint64(0x9E3779B97F4A7C15) * (np.uint64(16) * i + np.arange(k, dtype=np.uint64)[None, :] + np.uint64(1))
        x ^= x >> np.uint64(30)
        x *= np.uint64(0xBF58476D1CE4E5B9)
        x ^= x >> np.uint64(27)
        x *= np.uint64(0x94D049BB133111EB)
        x ^= x >> np.uint64(31)
        P = lo + ((x >> np.uint64(11)).astype(np.float64) * 2.0 ** -53) * (ref - lo)
        le = (rows[None, :, :] <= P[:, None, :]).all(axis=2)
        depth = le.sum(axis=1)
        hist += np.bincount(np.minimum(depth, 7), minlength=8)
        one = depth == 1
        if one.any():
            np.add.at(excl, le[one].argmax(axis=1), 1)
    return int(N - hist[0]), excl, hist


def same(out, want):
    n_cov, excl, hist, hv = want
    return bool(int(out["n_covered"].item()) == n_cov and torch.equal(out["excl"], excl) and torch.equal(out["depth_hist"], hist)
                and np.float64(out["hv"].item()).tobytes() == np.float64(hv).tobytes())


N = a.samples
res = {"device": torch.cuda.get_device_name(0), "warmup": a.warmup, "reps": a.reps, "torch_reps": a.torch_reps, "samples": N,
       "numpy_samples": a.numpy_samples, "seed": a.seed, "hi": a.hi, "box": "[0, hi]^k",
       "generator": "numpy.random.default_rng(7).integers(0, hi, (C, k)).astype(float)", "shapes": {}}
for Cn, k in SHAPES:
    A = np.random.default_rng(7).integers(0, a.hi, (Cn, k)).astype(float)
    t = torch.from_numpy(A).to(DEV)
    pf = dict(front=torch.empty(Cn, dtype=torch.int32, device=DEV), n_front=torch.empty(1, dtype=torch.int32, device=DEV))
    pareto_device(t, pf)
    M = int(pf["n_front"].item())
    front = pf["front"][:M].contiguous()
    lo = torch.zeros(k, dtype=torch.float64, device=DEV)
    ref = torch.full((k,), float(a.hi), dtype=torch.float64, device=DEV)
    dflt, dflt_out = device_route(t, front, lo, ref, N)
    t128, t128_out = device_route(t, front, lo, ref, N, 128)
    t256, t256_out = device_route(t, front, lo, ref, N, 256)
    padded, padded_out = device_route(t, pf["front"], lo, ref, N)
    keep = {}

    def torch_run():
        keep["torch"] = _hypervolume_torch(t, front, lo, ref, N, a.seed)

    routes = {"device": (dflt, a.reps), "device_T128": (t128, a.reps), "device_T256": (t256, a.reps),
              "device_padded_front": (padded, a.reps), "torch": (torch_run, a.torch_reps)}
    st = interleaved(routes, a.warmup, a.reps)
    torch.cuda.synchronize()
    agree = bool(same(dflt_out, keep["torch"]) and same(t128_out, keep["torch"]) and same(t256_out, keep["torch"]) and
                 int(padded_out["n_covered"].item()) == keep["torch"][0] and torch.equal(padded_out["excl"][:M], keep["torch"][1]) and
                 int(padded_out["excl"][M:].sum().item()) == 0)
    # numpy on the CPU at fewer points, against the device at the same count
    Nn = min(a.numpy_samples, N)
    small, small_out = device_route(t, front, lo, ref, Nn)
    small()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    ncov, nexcl, nhist = hv_numpy(A, front.cpu().numpy().astype(np.int64), np.zeros(k), np.full(k, float(a.hi)), Nn, a.seed)
    tn = 1e3 * (time.perf_counter() - t0)
    agree_np = bool(ncov == int(small_out["n_covered"].item()) and np.array_equal(nexcl, small_out["excl"].cpu().numpy()) and
                    np.array_equal(nhist, small_out["depth_hist"].cpu().numpy()))
    st["numpy_scaled"] = {"measured_ms": tn, "measured_samples": Nn, "scaled_to_samples": N, "median_ms": tn * N / Nn,
                          "note": "one run at measured_samples points, scaled linearly to scaled_to_samples"}
    K = 2 if k <= 2 else 4 if k <= 4 else 8 if k <= 8 else 16
    d = st["device"]["median_ms"]
    hist = dflt_out["depth_hist"].cpu().numpy()
    excl = dflt_out["excl"].cpu().numpy()
    entry = {"C": Cn, "k": k, "K": K, "members": M, "n_covered": int(dflt_out["n_covered"].item()), "hv": float(dflt_out["hv"].item()),
             "depth_hist": [int(x) for x in hist], "members_with_excl_0": int((excl == 0).sum()),
             "share_of_excl_in_top_20": float(np.sort(excl)[::-1][:20].sum() / max(1, excl.sum())),
             "routes_agree": agree, "numpy_agrees": agree_np, "times": st,
             "column_tests_per_s": float(N) * M * K / (d * 1e-3),
             "ratios": {"torch_over_device": st["torch"]["median_ms"] / d,
                        "numpy_scaled_over_device": st["numpy_scaled"]["median_ms"] / d,
                        "T128_over_T256": st["device_T128"]["median_ms"] / st["device_T256"]["median_ms"],
                        "padded_front_over_device": st["device_padded_front"]["median_ms"] / d}}
    res["shapes"]["%dx%d" % (Cn, k)] = entry
    print(json.dumps({"shape": [Cn, k], "members": M, "agree": [agree, agree_np],
                      **{n: round(v["median_ms"], 4) for n, v in st.items()},
                      "column_tests_per_s": entry["column_tests_per_s"]}), flush=True)

out = a.out or os.path.join(ROOT, "profiles", "r014_hypervolume.json")
os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
with open(out, "w") as f:
    json.dump(res, f, indent=1)
    f.write("\n")
print("wrote", out)
