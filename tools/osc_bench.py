"""Oscillation indices per setpoint segment on the device (mpct_osc_indices_device, mpct_eval_osc_indices;
DESIGN §22), timed on one GPU at the Shell 3x3 tuning grid of tools/segments_bench.py: 4,096 candidates x 3
reference sets = 12,288 simulations x (3 + 3) rows x 500 steps, the reference sets the scenario's own setpoint
sequence (changes at samples 9, 79, 199 and 399) at three scales: five segments.

  kernel alone   osc_indices_kernel on resident trajectories against segment_indices_kernel on the same tensors
                 and a hipMemcpyAsync device-to-device copy of the same trajectory bytes (y and u), same device,
                 same run, interleaved.  The copy reads and writes, so it moves twice the kernels' traffic.  HIP
                 events.
  end to end     engine.eval_osc_indices (host arrays in, records out) against the only route without it:
                 engine.eval_batch(want_traj=True), the trajectories copied to the host, and the vectorised numpy
                 reference over them (tests/osc_ref.osc_np).  Wall clock; the records of both routes are compared
                 bit for bit.
  records        how many output units have a second peak on the same side (ncross >= k0 + 2), and the
                 distribution of their decay ratio.

--warmup runs first, then --reps repetitions, the routes of a group interleaved a, b, c, a, b, c, ..; median, min,
max and spread are reported.

python tools/osc_bench.py [--reps N] [--out profiles/r018_osc.json]"""
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
import osc_ref as R
import segments_ref as SR
from mpct import engine
from mpct.scenarios import candidate_grid, shell3x3

ap = argparse.ArgumentParser()
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--candidates", type=int, default=4096)
ap.add_argument("--out", default=None)
a = ap.parse_args()
DEV = torch.device("cuda", 0)
PAR = dict(base=1, band_rel=0.02, band_abs=0.0, rev_tol=0.0)
SPAR = dict(base=1, band_rel=0.02, band_abs=0.0, rise_lo=0.1, rise_hi=0.9)


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
refs = np.ascontiguousarray(np.stack([r, 0.5 * r, -0.75 * r]))
tseg = engine.reference_segments(refs)
Cn, nref, my, nu, nit, nseg = len(N2), refs.shape[0], sc.my, sc.nu, sc.nit, tseg.size - 1
S = Cn * nref
res = {"device": torch.cuda.get_device_name(0), "warmup": a.warmup, "reps": a.reps,
       "shape": {"C": Cn, "nref": nref, "S": S, "my": my, "nu": nu, "nit": nit, "nseg": nseg},
       "params": dict(PAR, tseg=tseg.tolist())}

ev = engine.eval_batch(sc, N2, Nu, dl, lm, refs, want_traj=True, device=0)
traj_bytes = ev.y.nbytes + ev.u.nbytes
res["trajectory_bytes"] = traj_bytes

# ---- kernel alone against the segment kernel and a device-to-device copy of the same bytes
ty, tu, tr = (torch.from_numpy(x).to(DEV) for x in (ev.y, ev.u, refs))
out = {f: torch.empty((S, my if f in R.Y_FIELDS else nu, nseg), dtype=torch.int32 if f in R.INT_FIELDS else torch.float64,
                      device=DEV) for f in R.FIELDS}
sout = {f: torch.empty((S, my if f in SR.Y_FIELDS else nu, nseg), dtype=torch.int32 if f in SR.INT_FIELDS else torch.float64,
                       device=DEV) for f in SR.FIELDS}
cy, cu = torch.empty_like(ty), torch.empty_like(tu)
hip = hip_runtime()
hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
hip.hipMemcpyAsync.restype = C.c_int
D2D = 3  # hipMemcpyDeviceToDevice


def osc_kernel():
    engine.osc_indices_device(ty, tu, tr, out, tseg, **PAR)


def segment_kernel():
    engine.segment_indices_device(ty, tu, tr, sout, tseg, **SPAR)


def copy():
    st = C.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)
    for dst, src in ((cy, ty), (cu, tu)):
        rc = hip.hipMemcpyAsync(C.c_void_p(dst.data_ptr()), C.c_void_p(src.data_ptr()), src.numel() * 8, D2D, st)
        if rc != 0:
            raise RuntimeError("hipMemcpyAsync failed (%d)" % rc)


k = interleaved({"osc_kernel": osc_kernel, "segment_kernel": segment_kernel, "d2d_copy": copy}, timed_events)
torch.cuda.synchronize()
want = R.osc_np(ev.y, ev.u, refs, tseg, **PAR)
got = {f: out[f].cpu().numpy() for f in R.FIELDS}
kernel_ok = not R.mismatches(got, want)
# a sample of simulations against the scalar reference of the tests as well
rows = np.arange(0, S, max(1, S // 16)) // nref * nref          # whole candidates' first simulations: reference set 0
ref = R.osc_scalar(ev.y[rows], ev.u[rows], refs[:1], tseg, **PAR)
sample_ok = not R.mismatches({f: got[f][rows] for f in R.FIELDS}, ref)
om_, sm_, cm_ = (k[n]["median_ms"] for n in ("osc_kernel", "segment_kernel", "d2d_copy"))
# the osc kernel reads y, u and two samples of r per unit; the segment kernel reads r over the segments as well
res["kernel_alone"] = {"times": k, "osc_read_bytes": traj_bytes, "segment_read_bytes": traj_bytes + refs.nbytes,
                       "copy_moved_bytes": 2 * traj_bytes, "osc_GBps_read": traj_bytes / om_ / 1e6,
                       "segment_GBps_read": (traj_bytes + refs.nbytes) / sm_ / 1e6, "copy_GBps_moved": 2 * traj_bytes / cm_ / 1e6,
                       "osc_over_segment": om_ / sm_, "osc_over_copy": om_ / cm_,
                       "kernel_equals_numpy_bitwise": bool(kernel_ok), "sampled_rows_equal_scalar_reference": bool(sample_ok)}
valid = got["ncross"] >= 0
two = got["period"] >= 0                                        # ncross >= k0 + 2
dec = got["decay"][two]
q = [0.0, 0.1, 0.25, 0.5, 0.75, 0.9, 0.99, 1.0]
res["records"] = {"valid_output_units": int(valid.sum()), "units_with_a_crossing": int((got["ncross"][valid] > 0).sum()),
                  "units_with_second_peak": int(two.sum()),
                  "decay_quantiles": {str(p): float(np.quantile(dec, p)) for p in q} if dec.size else {},
                  "units_with_decay_at_least_1": int((dec >= 1.0).sum()),
                  "ncross_max": int(got["ncross"].max()), "ncross_mean_of_valid": float(got["ncross"][valid].mean()),
                  "valid_input_units": int((got["nmove"] >= 0).sum()), "nrev_max": int(got["nrev"].max()),
                  "nrev_mean_of_valid": float(got["nrev"][got["nrev"] >= 0].mean())}
print(json.dumps({"osc_ms": round(om_, 4), "segment_ms": round(sm_, 4), "copy_ms": round(cm_, 4), "bitwise": bool(kernel_ok),
                  "sample": bool(sample_ok), "second_peak_units": int(two.sum())}), flush=True)
del cy, cu

# ---- end to end on host arrays
keep = {}


def new_route():
    keep["new"] = engine.eval_osc_indices(sc, N2, Nu, dl, lm, refs, tseg=tseg, device=0, **PAR)


def old_eval():
    keep["ev"] = engine.eval_batch(sc, N2, Nu, dl, lm, refs, want_traj=True, device=0)


def old_numpy():
    keep["old"] = R.osc_np(keep["ev"].y, keep["ev"].u, refs, tseg, **PAR)


e = interleaved({"eval_osc_indices": new_route, "eval_batch_traj_to_host": old_eval, "numpy_pass": old_numpy}, timed_wall)
same = not R.mismatches({f: getattr(keep["new"], f).reshape(keep["old"][f].shape) for f in R.FIELDS}, keep["old"])
old_ms = e["eval_batch_traj_to_host"]["median_ms"] + e["numpy_pass"]["median_ms"]
res["end_to_end"] = {"times": e, "old_route_ms": old_ms, "old_over_new": old_ms / e["eval_osc_indices"]["median_ms"],
                     "routes_agree_bitwise": bool(same)}
print(json.dumps({"eval_osc_indices_ms": round(e["eval_osc_indices"]["median_ms"], 2), "old_route_ms": round(old_ms, 2),
                  "agree": bool(same)}), flush=True)

path = a.out or os.path.join(ROOT, "profiles", "r018_osc.json")
os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
with open(path, "w") as f:
    json.dump(res, f, indent=1)
    f.write("\n")
print("wrote", path)
