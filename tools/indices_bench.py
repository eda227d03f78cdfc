"""Closed-loop performance indices on the device (mpct_indices_device, mpct_eval_indices), timed on
one GPU at the Shell 3x3 tuning grid: 4,096 candidates x 3 reference sets = 12,288 simulations x (3 + 3) rows
x 500 steps.

  kernel alone   traj_indices_kernel on resident trajectories against a hipMemcpyAsync device-to-device copy
                 of the same trajectory bytes (y and u), same device, same run.  The copy reads and writes, so
                 it moves twice the kernel's traffic.  HIP events.
  end to end     engine.eval_indices (host arrays in, records out) against the only route without it:
                 engine.eval_batch(want_traj=True), the trajectories copied to the host, and the numpy
                 reference of tests/indices_ref.py on them.  Wall clock (the calls are synchronous); the two
                 parts of the old route are reported apart.  The records of both routes are compared.
  trajectory     engine.eval_batch cost-only for the same batch (gpc_small_kernel), wall clock, and the device
  penalty        entries alone by HIP events: mpct_eval_batch_device cost-only against mpct_eval_indices_device.

--warmup runs first, then --reps repetitions, the routes of a group interleaved a, b, a, b, ..; median, min, max
and spread are reported.

python tools/indices_bench.py [--reps N] [--out profiles/r013_indices.json]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "model-predictive-control-tuning_amd"), ROOT, os.path.join(ROOT, "tests")]
import numpy as np
import torch
import indices_ref as R
from mpct import _lib, engine
from mpct.scenarios import candidate_grid, shell3x3, vns_step_refs

ap = argparse.ArgumentParser()
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--candidates", type=int, default=4096)
ap.add_argument("--out", default=None)
a = ap.parse_args()
DEV = torch.device("cuda", 0)
T0, REL, AB = 0, 0.02, 0.0


def stats(t):
    t = np.sort(np.asarray(t))
    return {"median_ms": float(np.median(t)), "min_ms": float(t[0]), "max_ms": float(t[-1]),
            "spread_pct": float(100.0 * (t[-1] - t[0]) / np.median(t)), "all_ms": [float(x) for x in t]}


def timed_events(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def timed_wall(fn):
    t0 = time.perf_counter()
    fn()
    return 1e3 * (time.perf_counter() - t0)


def interleaved(routes, timer):
    for fn in routes.values():
        for _ in range(a.warmup):
            fn()
    torch.cuda.synchronize()
    t = {n: [] for n in routes}
    for _ in range(a.reps):
        for n, fn in routes.items():
            t[n].append(timer(fn))
    return {n: stats(v) for n, v in t.items()}


def hip_runtime():
    """the HIP runtime this process already uses (torch's), by the path it was loaded from"""
    with open("/proc/self/maps") as f:
        for ln in f:
            if "libamdhip64" in ln:
                return C.CDLL(ln.split()[-1])
    raise RuntimeError("no HIP runtime loaded")


sc, r, _ = shell3x3(n2_max=30, nu_max=5, nit=500)
N2, Nu, dl, lm = candidate_grid(a.candidates)
refs = vns_step_refs(3, 500)
Cn, nref, my, nu, nit = len(N2), refs.shape[0], sc.my, sc.nu, sc.nit
S = Cn * nref
res = {"device": torch.cuda.get_device_name(0), "warmup": a.warmup, "reps": a.reps,
       "shape": {"C": Cn, "nref": nref, "S": S, "my": my, "nu": nu, "nit": nit},
       "params": {"t0": T0, "band_rel": REL, "band_abs": AB}}

# ---- the trajectories of the grid itself, once (also the old route's first warm-up)
ev = engine.eval_batch(sc, N2, Nu, dl, lm, refs, want_traj=True, device=0)
traj_bytes = ev.y.nbytes + ev.u.nbytes
res["trajectory_bytes"] = traj_bytes

# ---- kernel alone against a device-to-device copy of the same bytes
ty, tu, tr = (torch.from_numpy(x).to(DEV) for x in (ev.y, ev.u, refs))
out = {f: torch.empty((S, my if f in R.Y_FIELDS else nu), dtype=torch.int32 if f in R.INT_FIELDS else torch.float64,
                      device=DEV) for f in R.Y_FIELDS + R.U_FIELDS}
cy, cu = torch.empty_like(ty), torch.empty_like(tu)
hip = hip_runtime()
hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
hip.hipMemcpyAsync.restype = C.c_int
D2D = 3  # hipMemcpyDeviceToDevice


def kernel():
    engine.indices_device(ty, tu, tr, out, t0=T0, band_rel=REL, band_abs=AB)


def copy():
    st = C.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)
    for dst, src in ((cy, ty), (cu, tu)):
        rc = hip.hipMemcpyAsync(C.c_void_p(dst.data_ptr()), C.c_void_p(src.data_ptr()), src.numel() * 8, D2D, st)
        if rc != 0:
            raise RuntimeError("hipMemcpyAsync failed (%d)" % rc)


k = interleaved({"index_kernel": kernel, "d2d_copy": copy}, timed_events)
torch.cuda.synchronize()
assert torch.equal(cy.view(torch.int64), ty.view(torch.int64)) and torch.equal(cu.view(torch.int64), tu.view(torch.int64))
want = R.indices_np(ev.y, ev.u, refs, T0, REL, AB)
kernel_ok = all(bool((R.bits(out[f].cpu().numpy()) == R.bits(want[f])).all()) for f in out)
km, cm = k["index_kernel"]["median_ms"], k["d2d_copy"]["median_ms"]
res["kernel_alone"] = {"times": k, "kernel_read_bytes": traj_bytes + refs.nbytes, "copy_moved_bytes": 2 * traj_bytes,
                       "kernel_GBps_read": (traj_bytes + refs.nbytes) / km / 1e6, "copy_GBps_moved": 2 * traj_bytes / cm / 1e6,
                       "kernel_over_copy": km / cm, "kernel_equals_reference_bitwise": kernel_ok}
print(json.dumps({"kernel_ms": round(km, 4), "copy_ms": round(cm, 4), "bitwise": kernel_ok}), flush=True)
del cy, cu

# ---- end to end on host arrays
keep = {}


def new_route():
    keep["new"] = engine.eval_indices(sc, N2, Nu, dl, lm, refs, t0=T0, band_rel=REL, band_abs=AB, device=0)


def old_eval():
    keep["ev"] = engine.eval_batch(sc, N2, Nu, dl, lm, refs, want_traj=True, device=0)


def old_numpy():
    keep["old"] = R.indices_np(keep["ev"].y, keep["ev"].u, refs, T0, REL, AB)


def cost_only():
    keep["cost"] = engine.eval_batch(sc, N2, Nu, dl, lm, refs, device=0)


e = interleaved({"eval_indices": new_route, "eval_batch_traj_to_host": old_eval, "numpy_reference": old_numpy,
                 "eval_batch_cost_only": cost_only}, timed_wall)
same = all(bool((R.bits(getattr(keep["new"], f).reshape(S, -1)) == R.bits(keep["old"][f])).all()) for f in out)
old_ms = e["eval_batch_traj_to_host"]["median_ms"] + e["numpy_reference"]["median_ms"]
res["end_to_end"] = {"times": e, "old_route_ms": old_ms, "old_over_new": old_ms / e["eval_indices"]["median_ms"],
                     "new_over_cost_only": e["eval_indices"]["median_ms"] / e["eval_batch_cost_only"]["median_ms"],
                     "routes_agree_bitwise": same}
print(json.dumps({"eval_indices_ms": round(e["eval_indices"]["median_ms"], 2), "old_route_ms": round(old_ms, 2),
                  "cost_only_ms": round(e["eval_batch_cost_only"]["median_ms"], 2), "agree": same}), flush=True)

# ---- the device entries alone: what the general trajectory kernel costs over the cost-only one
ins = [torch.from_numpy(np.ascontiguousarray(x)).to(DEV) for x in
       (N2.astype(np.int32), Nu.astype(np.int32), dl.reshape(Cn, my), lm.reshape(Cn, nu), refs)]
costs = {"J1": torch.empty((S, my), dtype=torch.float64, device=DEV), "j22": torch.empty((S, my), dtype=torch.float64, device=DEV),
         "status": torch.empty(S, dtype=torch.int32, device=DEV), "qp_iters": torch.empty(S, dtype=torch.int64, device=DEV)}


def dev_cost():
    engine.eval_batch_device(sc, *ins, costs, device=0)


def dev_indices():
    engine.eval_indices_device(sc, *ins, dict(out, **costs), t0=T0, band_rel=REL, band_abs=AB, device=0)


d = interleaved({"eval_batch_device_cost_only": dev_cost, "eval_indices_device": dev_indices}, timed_events)
res["device_entries"] = {"times": d, "instance_cost_only": engine.kernel_instance(sc),
                         "instance_trajectories": engine.kernel_instance(sc, want_traj=True),
                         "indices_over_cost_only": d["eval_indices_device"]["median_ms"] /
                         d["eval_batch_device_cost_only"]["median_ms"],
                         "scratch_chunks": int(np.ceil(traj_bytes / _lib.INDEX_SCRATCH_BYTES))}
print(json.dumps({n: round(v["median_ms"], 3) for n, v in d.items()}), flush=True)

path = a.out or os.path.join(ROOT, "profiles", "r013_indices.json")
os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
with open(path, "w") as f:
    json.dump(res, f, indent=1)
    f.write("\n")
print("wrote", path)
