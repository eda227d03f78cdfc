"""Greedy hypervolume subset selection (mpct_hv_select_device), timed on one GPU:

  (1) the call at n_pick = 20 and 64 against n_pick x the time of mpct_hypervolume_device on the same front,
      interleaved in the same run (tools/hv_bench.py's timing: HIP events, warm-ups, a, b, a, b, ..);
  (2) the time of every round from events round it (mpct_internal_hvsel_round_ms, a tool-only mode that
      waits for the stream) beside the share of points still uncovered when the round starts;
  (3) the contract as chunked torch expressions on the device (mpct.dist._hv_select_torch) and as numpy on
      the CPU (wall clock) at --numpy-samples points and --numpy-picks rounds, scaled to N and n_pick and
      labelled as scaled; every route must agree exactly;
  (4) what the selection buys: share after 20 greedy picks against n_covered / n_covered_all of the 20
      members with the largest excl (mpct_hypervolume_device on that subset).

Shapes: tools/hv_bench.py's two fronts from the same generators, its box [0, hi]^k, N = 2^20.

python tools/hv_select_bench.py [--reps N] [--out profiles/r015_hv_select.json]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "model-predictive-control-tuning_amd"), os.path.join(ROOT, "tests"), ROOT]
import numpy as np
import torch
from mpct import _lib
from mpct.dist import _hv_select_torch
from mpct.engine import HVSEL_FIELDS, hv_select_device, hypervolume_device, pareto_device

ap = argparse.ArgumentParser()
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--torch-reps", type=int, default=1)
ap.add_argument("--samples", type=int, default=1 << 20)
ap.add_argument("--numpy-samples", type=int, default=1 << 12)
ap.add_argument("--numpy-picks", type=int, default=4)
ap.add_argument("--picks", type=int, nargs="+", default=[20, 64])
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


def interleaved(routes, warmup):
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


def select_out(K):
    i32 = lambda: torch.empty(K, dtype=torch.int32, device=DEV)
    i64 = lambda n: torch.empty(n, dtype=torch.int64, device=DEV)
    return dict(n_picked=i64(1), pos=i32(), index=i32(), gain=i64(K), covered=i64(K),
                hv=torch.empty(K, dtype=torch.float64, device=DEV), ties=i32(), n_covered_all=i64(1))


def hv_out(M):
    return dict(n_covered=torch.empty(1, dtype=torch.int64, device=DEV), excl=torch.empty(M, dtype=torch.int64, device=DEV),
                depth_hist=torch.empty(8, dtype=torch.int64, device=DEV), hv=torch.empty(1, dtype=torch.float64, device=DEV))


def same(out, want):
    """a device result against a dict of the same fields (tensors, arrays or ints), exactly"""
    for f in HVSEL_FIELDS:
        g = out[f].cpu().numpy()
        w = want[f].cpu().numpy() if torch.is_tensor(want[f]) else np.asarray(want[f])
        if g.tobytes() != np.ascontiguousarray(np.broadcast_to(w, g.shape), dtype=g.dtype).tobytes():
            return False
    return True


N = a.samples
lib = _lib.load()
res = {"device": torch.cuda.get_device_name(0), "warmup": a.warmup, "reps": a.reps, "torch_reps": a.torch_reps, "samples": N,
       "numpy_samples": a.numpy_samples, "numpy_picks": a.numpy_picks, "seed": a.seed, "hi": a.hi, "box": "[0, hi]^k",
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
    hvo = hv_out(M)
    entry = {"C": Cn, "k": k, "members": M, "picks": {}}
    for K in a.picks:
        so = select_out(K)
        routes = {"hv_select": (lambda: hv_select_device(t, K, so, lo, ref, members=front, n_samples=N, seed=a.seed), a.reps),
                  "hypervolume": (lambda: hypervolume_device(t, hvo, lo, ref, members=front, n_samples=N, seed=a.seed), a.reps)}
        st = interleaved(routes, a.warmup)
        torch.cuda.synchronize()
        # (2) every round's time, in the tool-only mode
        ms = np.zeros(K, dtype=np.float32)
        so2 = select_out(K)
        lib.mpct_internal_hvsel_round_ms(ms.ctypes.data, K)      # the next call alone fills it
        try:
            hv_select_device(t, K, so2, lo, ref, members=front, n_samples=N, seed=a.seed)
        finally:
            lib.mpct_internal_hvsel_round_ms(None, 0)
        torch.cuda.synchronize()
        gain = so["gain"].cpu().numpy()
        covered = so["covered"].cpu().numpy()
        n_all = int(so["n_covered_all"].item())
        # uncovered when round r starts: all N in round 0 (it finds the coverable ones), then n_all - covered[r - 1]
        left = np.concatenate(([N], n_all - covered[:-1])) / float(N)
        per = {"round_ms": [float(x) for x in ms], "share_of_points_alive_at_start": [float(x) for x in left],
               "round_ms_over_round0": [float(x / ms[0]) for x in ms]}
        # (3) the torch route on the device
        keep = {}
        tt = [timed(lambda: keep.update(torch=_hv_select_torch(t, front, lo, ref, N, a.seed, K))) for _ in range(a.torch_reps)]
        torch.cuda.synchronize()
        agree = bool(same(so, keep["torch"]) and same(so2, keep["torch"]))
        d = st["hv_select"]["median_ms"]
        entry["picks"][str(K)] = {
            "n_picked": int(so["n_picked"].item()), "n_covered_all": n_all, "gain": [int(x) for x in gain],
            "share": [float(x) for x in covered / float(n_all)], "ties": [int(x) for x in so["ties"].cpu().numpy()],
            "times": st, "torch": stats(tt), "routes_agree": agree, "rounds": per,
            "ratios": {"hv_select_over_K_hypervolume": d / (K * st["hypervolume"]["median_ms"]),
                       "torch_over_device": float(np.median(tt)) / d}}
    # (3) numpy at fewer points and rounds, against the device at the same counts
    import hvsel_ref

    Nn, Kn = min(a.numpy_samples, N), a.numpy_picks
    sm = select_out(Kn)
    hv_select_device(t, Kn, sm, lo, ref, members=front, n_samples=Nn, seed=a.seed)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    want = hvsel_ref.select_np(A, front.cpu().numpy(), np.zeros(k), np.full(k, float(a.hi)), Nn, a.seed, Kn)
    tn = 1e3 * (time.perf_counter() - t0)
    entry["numpy_scaled"] = {"measured_ms": tn, "measured_samples": Nn, "measured_picks": Kn, "agrees": same(sm, want),
                             "scaled_ms": {str(K): tn * (N / Nn) * (K / Kn) for K in a.picks},
                             "note": "tests/hvsel_ref.select_np, one run at measured_samples points and measured_picks rounds, "
                                     "scaled linearly to N points and n_pick rounds"}
    # (4) greedy's 20 against the 20 largest excl
    K = 20
    so = select_out(K)
    hv_select_device(t, K, so, lo, ref, members=front, n_samples=N, seed=a.seed)
    hypervolume_device(t, hvo, lo, ref, members=front, n_samples=N, seed=a.seed)
    top = torch.argsort(hvo["excl"], descending=True, stable=True)[:K]
    sub = front[top].contiguous()
    ho = hv_out(K)
    hypervolume_device(t, ho, lo, ref, members=sub, n_samples=N, seed=a.seed)
    torch.cuda.synchronize()
    n_all = int(so["n_covered_all"].item())
    entry["greedy_against_top_excl"] = {
        "n_pick": K, "n_covered_all": n_all, "hypervolume_n_covered": int(hvo["n_covered"].item()),
        "greedy_share": float(so["covered"][-1].item() / n_all), "top_excl_share": float(ho["n_covered"].item() / n_all),
        "members_in_both": int(np.intersect1d(so["index"].cpu().numpy(), sub.cpu().numpy()).size)}
    res["shapes"]["%dx%d" % (Cn, k)] = entry
    print(json.dumps({"%dx%d" % (Cn, k): {K: {"ms": v["times"]["hv_select"]["median_ms"], "ratio": v["ratios"], "agree": v["routes_agree"]}
                                          for K, v in entry["picks"].items()},
                      "numpy_agrees": entry["numpy_scaled"]["agrees"], "buys": entry["greedy_against_top_excl"]}), flush=True)
if a.out:
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
