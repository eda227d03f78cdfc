"""Pareto front, domination counts and layers of a scored grid (mpct_pareto_device), timed on
one GPU against the same contract written two other ways:

  (a) mpct_pareto_device: dom_count, front and n_front, and the same with layer at L = 8;
  (b) the contract as chunked torch expressions on the device (mpct.dist._pareto_torch);
  (c) the contract as chunked numpy on the CPU (wall clock).

Shapes: 4,096 x 3 (the metric's grid) and 65,536 x 7 (config 3's), costs numpy.random.default_rng(7)
.integers(0, hi, (C, k)) as in tests/pareto_ref.py, hi = 1000.  HIP-event timings, --warmup launches and
--reps repetitions per route, interleaved a, b, a, b, .. so that clock drift hits both alike; median, min,
max and spread are reported, and the routes' results are compared (all integers: exactly).  The numpy
route at 65,536 x 7 runs --numpy-reps times, without layers (one pass of 4.3e9 pairs on one core).

The A/B that chose the tile length T and the split of the competitor range: the device entry with both
forced (mpct_internal_pareto_tuned), T in {128, 256} x split in {1, 2, 4, 8, 16, 32}, interleaved.

python tools/pareto_bench.py [--reps N] [--out profiles/r012_pareto.json]"""
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
from mpct.dist import _pareto_torch

ap = argparse.ArgumentParser()
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--reps", type=int, default=11)
ap.add_argument("--numpy-reps", type=int, default=1)
ap.add_argument("--layers", type=int, default=8)
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
    """{name: stats} of the callables in `routes`, run warm-ups first and then a, b, .., a, b, .."""
    for fn in routes.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    t = {n: [] for n in routes}
    for _ in range(reps):
        for n, fn in routes.items():
            t[n].append(timed(fn))
    return {n: stats(v) for n, v in t.items()}


def device_route(costs, L, tile=0, split=0):
    """(callable, output tensors) of one device-entry call into fresh tensors"""
    n = costs.shape[0]
    out = dict(dom_count=torch.empty(n, dtype=torch.int32, device=DEV), front=torch.empty(n, dtype=torch.int32, device=DEV),
               n_front=torch.empty(1, dtype=torch.int32, device=DEV))
    if L:
        out["layer"] = torch.empty(n, dtype=torch.int32, device=DEV)
    r = _lib.MpctParetoResult(*[C.cast(C.c_void_p(out[f].data_ptr()), _lib.c_int32_p) if f in out else None
                                for f in ("dom_count", "layer", "front", "n_front")])
    lib = _lib.load()

    def run():
        st = C.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)
        if tile or split:
            rc = lib.mpct_internal_pareto_tuned(C.c_void_p(costs.data_ptr()), n, costs.shape[1], L, C.byref(r), st, tile, split)
        else:
            rc = lib.mpct_pareto_device(C.c_void_p(costs.data_ptr()), n, costs.shape[1], L, C.byref(r), st)
        if rc != 0:
            raise RuntimeError(_lib.last_error())

    return run, out


def pareto_numpy(A, L, chunk=1024):
    """the contract on the CPU: chunked broadcasting, peeling for the layers"""
    n = A.shape[0]
    valid = ~np.isnan(A).any(axis=1)

    def count(alive, todo):
        out = np.zeros(todo.size, dtype=np.int64)
        ai = np.flatnonzero(alive)
        for b0 in range(0, todo.size, chunk):
            b = A[todo[b0:b0 + chunk]]
            for a0 in range(0, ai.size, chunk):
                x = A[ai[a0:a0 + chunk]]
                le = (x[:, None, :] <= b[None, :, :]).all(axis=2)
                lt = (x[:, None, :] < b[None, :, :]).any(axis=2)
                out[b0:b0 + chunk] += (le & lt).sum(axis=0)
        return out

    dom = np.full(n, -1, dtype=np.int32)
    vi = np.flatnonzero(valid)
    dom[vi] = count(valid, vi)
    layer = None
    if L:
        layer = np.where(valid, L, -1).astype(np.int32)
        alive = valid.copy()
        for p in range(L):
            todo = np.flatnonzero(alive)
            if todo.size == 0:
                break
            top = todo[(dom[todo] == 0) if p == 0 else (count(alive, todo) == 0)]
            layer[top] = p
            alive[top] = False
    return dom, layer, np.flatnonzero(valid & (dom == 0))


res = {"device": torch.cuda.get_device_name(0), "warmup": a.warmup, "reps": a.reps, "layers": a.layers, "hi": a.hi,
       "generator": "numpy.random.default_rng(7).integers(0, hi, (C, k)).astype(float)", "shapes": {}, "ab": {}}
for Cn, k in SHAPES:
    A = np.random.default_rng(7).integers(0, a.hi, (Cn, k)).astype(float)
    t = torch.from_numpy(A).to(DEV)
    g = np.zeros(3, dtype=np.int32)
    _lib.load().mpct_internal_pareto_grid(Cn, g.ctypes.data_as(_lib.c_int32_p))
    count_run, count_out = device_route(t, 0)
    layer_run, layer_out = device_route(t, a.layers)
    keep = {}

    def torch_run(L=a.layers):
        keep["torch"] = _pareto_torch(t, L, chunk=2048)

    def torch_count():
        keep["torch0"] = _pareto_torch(t, 0, chunk=2048)

    routes = {"device_count": count_run, "device_layers": layer_run, "torch_count": torch_count, "torch_layers": torch_run}
    st = interleaved(routes, a.warmup, a.reps)
    torch.cuda.synchronize()
    dom, layer, front, nf = keep["torch"]
    same = bool(torch.equal(dom, layer_out["dom_count"]) and torch.equal(layer, layer_out["layer"]) and
                torch.equal(front, layer_out["front"]) and nf == int(layer_out["n_front"].item()) and
                torch.equal(count_out["dom_count"], layer_out["dom_count"]))
    lay = layer_out["layer"].cpu().numpy()
    # numpy on the CPU
    nl = a.layers if Cn <= 8192 else 0
    nreps = a.reps if Cn <= 8192 else a.numpy_reps
    tn = []
    for _ in range(nreps):
        t0 = time.perf_counter()
        ndom, nlay, nfront = pareto_numpy(A, nl)
        tn.append(1e3 * (time.perf_counter() - t0))
    same_np = bool(np.array_equal(ndom, layer_out["dom_count"].cpu().numpy()) and
                   (nlay is None or np.array_equal(nlay, lay)) and
                   np.array_equal(nfront, layer_out["front"].cpu().numpy()[:nf]))
    st["numpy_layers" if nl else "numpy_count"] = stats(tn)
    entry = {"C": Cn, "k": k, "grid": {"tile": int(g[0]), "split": int(g[1]), "chunk": int(g[2])},
             "n_front": nf, "candidates_per_layer": [int((lay == p).sum()) for p in range(a.layers + 1)],
             "routes_agree": same, "numpy_agrees": same_np, "times": st}
    d = st["device_layers"]["median_ms"]
    entry["ratios"] = {"torch_layers_over_device_layers": st["torch_layers"]["median_ms"] / d,
                       "torch_count_over_device_count": st["torch_count"]["median_ms"] / st["device_count"]["median_ms"],
                       "device_layers_over_device_count": d / st["device_count"]["median_ms"]}
    if nl:
        entry["ratios"]["numpy_layers_over_device_layers"] = st["numpy_layers"]["median_ms"] / d
    else:
        entry["ratios"]["numpy_count_over_device_count"] = st["numpy_count"]["median_ms"] / st["device_count"]["median_ms"]
    res["shapes"]["%dx%d" % (Cn, k)] = entry
    print(json.dumps({"shape": [Cn, k], "agree": [same, same_np],
                      **{n: round(v["median_ms"], 4) for n, v in st.items()}}), flush=True)
    # the A/B of tile length and split, counting pass only (dom_count, front, n_front)
    ab = {}
    for tile in (128, 256):
        for split in (1, 2, 4, 8, 16, 32):
            ab["T%d_split%d" % (tile, split)] = device_route(t, 0, tile, split)[0]
    ab["default"] = count_run
    sa = interleaved(ab, 2, 7)
    res["ab"]["%dx%d" % (Cn, k)] = {n: {"median_ms": v["median_ms"], "min_ms": v["min_ms"], "max_ms": v["max_ms"]}
                                     for n, v in sa.items()}
    print(json.dumps({"ab": [Cn, k], **{n: round(v["median_ms"], 4) for n, v in sa.items()}}), flush=True)

out = a.out or os.path.join(ROOT, "profiles", "r012_pareto.json")
os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
with open(out, "w") as f:
    json.dump(res, f, indent=1)
    f.write("\n")
print("wrote", out)
