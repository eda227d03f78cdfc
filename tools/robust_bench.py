"""Robust scoring on the config-4 grid (10,000 candidates x 32 plant-mismatch draws),
two routes to the same per-candidate records, timed in one run on one GPU:

  (a) per-simulation costs (eval_batch_device: dtc_small_kernel, 320,000 records) and a device-side
      torch reduction of them by the semantics of include/mpct.h;
  (b) eval_robust_device: dtc_robust_kernel, one workgroup per candidate, records reduced in LDS.

Warm-up launches, then HIP-event timings of REPS repetitions per route, interleaved a, b, a, b, ..
so that clock drift hits both alike; median, min, max and the spread are reported, with the bytes
each route writes.  Also counts the candidates with no failed draw at the default bound.

python tools/robust_bench.py [--candidates C] [--draws D] [--reps N] [--out profiles/r07_robust_bench.json]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "model-predictive-control-tuning_amd"), ROOT]
import numpy as np
import torch
from mpct.dtc import config4_candidates, woodberry_mc
from mpct.engine import eval_batch_device, eval_robust_device, kernel_instance, robust_instance

ap = argparse.ArgumentParser()
ap.add_argument("--candidates", type=int, default=10000)
ap.add_argument("--draws", type=int, default=32)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--reps", type=int, default=11)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r07_robust_bench.json"))
a = ap.parse_args()
Cn, D, my = a.candidates, a.draws, 2
JB = 1e100  # the default bound (j_bound = 0)

sc, refs, v, _ = woodberry_mc(draws=D, n2_max=30, nu_max=10)
dev = torch.device("cuda", 0)
N2, Nu, dl, lm = (torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in config4_candidates(Cn))
refs_d, v_d = torch.from_numpy(refs).to(dev), torch.from_numpy(v).to(dev)
S = Cn * D
per = dict(J1=torch.empty((S, my), dtype=torch.float64, device=dev), status=torch.empty(S, dtype=torch.int32, device=dev))
rob = dict(mean=torch.empty((Cn, my), dtype=torch.float64, device=dev),
           worst=torch.empty((Cn, my), dtype=torch.float64, device=dev),
           n_failed=torch.empty(Cn, dtype=torch.int32, device=dev),
           worst_draw=torch.empty(Cn, dtype=torch.int32, device=dev),
           status=torch.empty(Cn, dtype=torch.int32, device=dev))


def route_a():
    eval_batch_device(sc, N2, Nu, dl, lm, refs_d, per, v=v_d)
    J1 = per["J1"].view(Cn, D, my)
    st = per["status"].view(Cn, D)
    fin = torch.isfinite(J1).all(dim=2)
    J = torch.where(fin, torch.nan_to_num(J1, nan=0.0, posinf=0.0).sum(dim=2), torch.inf)
    surv = (st == 0) & torch.isfinite(J) & (J <= JB)
    n = surv.sum(dim=1)
    m = surv.unsqueeze(2)
    mean = torch.where(m, J1, 0.0).sum(dim=1) / n.unsqueeze(1)
    worst = torch.where(m, J1, -torch.inf).amax(dim=1)
    worst = torch.where(n.unsqueeze(1) > 0, worst, torch.nan)
    wd = torch.where(n > 0, torch.where(surv, J, -torch.inf).argmax(dim=1), -1)
    return mean, worst, (D - n).to(torch.int32), wd.to(torch.int32), st.amax(dim=1)


def route_b():
    eval_robust_device(sc, N2, Nu, dl, lm, refs_d, rob, v=v_d)


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


for _ in range(a.warmup):
    route_a()
    route_b()
torch.cuda.synchronize()
ta, tb = [], []
for _ in range(a.reps):
    ta.append(timed(route_a))
    tb.append(timed(route_b))
ra = route_a()
route_b()
torch.cuda.synchronize()
nf_a, nf_b = ra[2].cpu().numpy(), rob["n_failed"].cpu().numpy()


def stats(t):
    t = np.sort(np.asarray(t))
    return {"median_ms": float(np.median(t)), "min_ms": float(t[0]), "max_ms": float(t[-1]),
            "spread_pct": float(100.0 * (t[-1] - t[0]) / np.median(t)), "all_ms": [float(x) for x in t]}


rec_bytes = Cn * (2 * my * 8 + 3 * 4)
res = {"tool": "tools/robust_bench.py", "workload": "config 4: DTC-GPC WoodBerry, plant-mismatch draws",
       "device": torch.cuda.get_device_name(0), "candidates": Cn, "draws": D, "nit": 200, "warmup": a.warmup,
       "reps": a.reps, "timing": "HIP events around each route, routes interleaved",
       "a_per_simulation_plus_torch": dict(stats(ta), instance=kernel_instance(sc) + " + torch reduction",
                                           bytes_written_by_kernels=S * (my * 8 + 4),
                                           bytes_written_records=rec_bytes),
       "b_eval_robust_device": dict(stats(tb), instance=robust_instance(sc), bytes_written=rec_bytes),
       "ratio_b_over_a_median": float(np.median(tb) / np.median(ta)),
       "n_failed_agree": bool(np.array_equal(nf_a, nf_b)),
       "candidates_without_failed_draw": int(np.count_nonzero(nf_b == 0)),
       "candidates_all_draws_failed": int(np.count_nonzero(nf_b == D)),
       "j_bound": JB}
os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
with open(a.out, "w") as f:
    json.dump(res, f, indent=1)
    f.write("\n")
print(json.dumps({k: res[k] for k in ("ratio_b_over_a_median", "n_failed_agree", "candidates_without_failed_draw")}
                 | {"a_median_ms": res["a_per_simulation_plus_torch"]["median_ms"],
                    "b_median_ms": res["b_eval_robust_device"]["median_ms"]}))
