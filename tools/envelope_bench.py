"""Measurements of the trajectory envelopes (results in profiles/r020_envelope.json).

  kernel   mpct_envelope_device on one side (y [C, D, 3, 500], C = 4,096) with the levels forced to the lane kernel
           (draw_envelope_kernel) and to draw_stats_kernel through the dlane hook, against mpct_draw_stats_device on
           the same reshaped table -- the route of the parent commit -- and against a device-to-device
           hipMemcpyAsync of the bytes read; D = 8, 32, 128, with three levels and without.  HIP events around one
           call; envelope_spread_kernel is timed as the difference of a call with and without the spread.
  crossing the same with levels at a quarter of the candidates over the draw counts in between: where the lane
           kernel stops being the faster one, which sets kEnvDefaultDlane (csrc/envelope.h).
  entry    eval_robust_envelope end to end (host arrays in and out) on shell3x3_mc against the only route
           without it: eval_batch(want_traj=True) to the host plus a vectorised numpy reduction.

Warm-ups first, the variants interleaved repetition by repetition, median with range; the records are checked
against tests/envelope_ref.py inside the run (the first candidate of each shape, bit for bit).  The file's
bench_ab block is not measured here: it records bench.py of the parent commit from its own tree and of this one,
run alternately, and a rerun of this tool keeps it.

    python tools/envelope_bench.py [--reps 11] [--warmup 3] [--out profiles/r020_envelope.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "model-predictive-control-tuning_amd"), os.path.join(ROOT, "tests"), ROOT]

LEVELS = [0.05, 0.5, 0.95]


def med(v):
    v = sorted(v)
    return dict(median=v[len(v) // 2], min=v[0], max=v[-1], n=len(v))


def kernel_shape(Cn, D, rows, nit, levels, reps, warmup):
    import torch
    import draw_stats_ref as R
    import envelope_ref as E
    from mpct import _lib
    from mpct.engine import draw_stats_device, envelope_device

    lib = _lib.load()
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(Cn + D)
    m, nlev = rows * nit, len(levels)
    y = rng.random((Cn, D, rows, nit))
    y[rng.random(y.shape) < 0.02] = np.nan
    alive = (rng.random((Cn, D)) > 0.05).astype(np.int32)
    ty, ta = torch.tensor(y, device=dev), torch.tensor(alive, device=dev)
    tx = ty.view(Cn, D, m)
    fields = R.FIELDS if nlev else R.BASE

    def bufs(shape):
        return {f: torch.zeros(shape + ((nlev,) if f in R.LEVEL else ()), dtype=torch.int32 if f in R.INT_FIELDS else torch.float64,
                               device=dev) for f in fields}

    outs = {k: bufs((Cn, rows, nit)) for k in ("lane", "primitive_via_envelope")}
    flat = bufs((Cn, m))
    sp = {f: torch.zeros((Cn, rows), dtype=torch.int32 if f == "t_spread_max" else torch.float64, device=dev) for f in E.SPREAD}
    dst, dsta = torch.empty_like(ty), torch.empty_like(ta)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]

    def timed(fn):
        ev[0].record()
        fn()
        ev[1].record()
        ev[1].synchronize()
        return ev[0].elapsed_time(ev[1]) * 1e3    # microseconds

    def env(key, dlane, spread):
        def fn():
            assert lib.mpct_internal_envelope_dlane(dlane) == 0
            try:
                envelope_device(ty, None, {"y": outs[key], "spread_y": sp if spread else {}}, ta, levels if nlev else None, 0)
            finally:
                lib.mpct_internal_envelope_dlane(0)
        return fn

    run = {"draw_stats_device": lambda: draw_stats_device(tx, flat, ta, levels if nlev else None),
           "memcpy": lambda: (dst.copy_(ty), dsta.copy_(ta))}
    if not nlev or D <= _lib.ENVELOPE_LANE_MAX_DRAWS:
        run["lane"] = env("lane", _lib.ENVELOPE_LANE_MAX_DRAWS, False)
        run["lane_plus_spread"] = env("lane", _lib.ENVELOPE_LANE_MAX_DRAWS, True)
    if nlev:
        run["primitive_via_envelope"] = env("primitive_via_envelope", 1, False)
    for _ in range(warmup):
        for fn in run.values():
            timed(fn)
    t = {k: [] for k in run}
    for _ in range(reps):
        for k, fn in run.items():
            t[k].append(timed(fn))
    want, wsp = E.envelope_ref(y[:1], alive[:1], levels, t0=0)
    flat1 = {f: flat[f][:1].cpu().numpy().reshape(want[f].shape) for f in fields}
    R.assert_same_stats(flat1, want, fields=fields, msg="draw_stats %dx%d" % (Cn, D))
    for k in outs:
        if k in run:
            R.assert_same_stats({f: outs[k][f][:1].cpu().numpy() for f in fields}, want, fields=fields, msg="%s %dx%d" % (k, Cn, D))
    if "lane_plus_spread" in run:
        E.assert_same_spread({f: sp[f][:1].cpu().numpy() for f in E.SPREAD}, wsp, msg="spread")
    bytes_read = y.nbytes + alive.nbytes
    res = dict(C=Cn, D=D, rows=rows, nit=nit, columns=Cn * m, nlev=nlev, bytes_read=bytes_read, us={k: med(v) for k, v in t.items()},
               checked_candidates=1)
    for k in t:
        res.setdefault("GBps", {})[k] = bytes_read / res["us"][k]["median"] / 1e3
    if "lane" in t:
        res["lane_over_draw_stats"] = res["us"]["lane"]["median"] / res["us"]["draw_stats_device"]["median"]
        res["spread_us"] = res["us"]["lane_plus_spread"]["median"] - res["us"]["lane"]["median"]
    return res


def numpy_route(res, Cn, D, levels):
    """The host-side reduction a caller writes without the entry: classify by eval_robust's rule, then per sample
    mean / min / max and sorted quantiles (vectorised; not bit-compatible in the mean, which numpy sums pairwise)."""
    J = res.J1.reshape(Cn, D, -1).sum(axis=2)
    st = res.status.reshape(Cn, D)
    alive = (st == 0) & np.isfinite(J) & (J <= 1e100) & ~((st & 24) != 0).any(axis=1, keepdims=True)
    out = {}
    for side, a in (("y", res.y), ("u", res.u)):
        x = a.reshape(Cn, D, -1)
        x = np.where(alive[:, :, None] & np.isfinite(x), x, np.nan)
        with np.errstate(all="ignore"):
            n = np.isfinite(x).sum(axis=1)
            srt = np.sort(x, axis=1)
            o = dict(n=n, mean=np.nanmean(x, axis=1), lo=np.nanmin(x, axis=1), hi=np.nanmax(x, axis=1))
            for lv in levels:
                r = np.clip(np.ceil(lv * n), 1, np.maximum(n, 1)).astype(int) - 1
                o["q%g" % lv] = np.take_along_axis(srt, r[:, None, :], axis=1)[:, 0]
            o["spread"] = (o["hi"] - o["lo"]).reshape(Cn, a.shape[1], -1).sum(axis=2)
        out[side] = o
    return out


def entry(Cn, D, nit, reps, warmup):
    import draw_stats_ref as R
    import envelope_ref as E
    from mpct.engine import eval_batch, eval_robust_envelope
    from mpct.scenarios import candidate_grid, shell3x3_mc

    sc, refs, _ = shell3x3_mc(draws=D, nit=nit)
    cands = candidate_grid(Cn)
    run = {"eval_batch_traj_only": lambda: eval_batch(sc, *cands, refs, want_traj=True, device=0),
           "eval_batch_traj_plus_numpy": lambda: numpy_route(eval_batch(sc, *cands, refs, want_traj=True, device=0), Cn, D, LEVELS),
           "eval_robust_envelope": lambda: eval_robust_envelope(sc, *cands, refs, levels=LEVELS, device=0)}
    last = {}
    for _ in range(warmup):
        for k, fn in run.items():
            last[k] = fn()
    t = {k: [] for k in run}
    for _ in range(reps):
        for k, fn in run.items():
            t0 = time.perf_counter()
            last[k] = fn()
            t[k].append((time.perf_counter() - t0) * 1e3)
    ev, got, host = last["eval_batch_traj_only"], last["eval_robust_envelope"], last["eval_batch_traj_plus_numpy"]
    nchk = min(Cn, 2)
    alive = R.alive_ref(ev.J1.reshape(Cn, D, -1)[:nchk], ev.status.reshape(Cn, D)[:nchk], 0.0)
    for side, a, rec in (("y", ev.y, got.y), ("u", ev.u, got.u)):
        want, wsp = E.envelope_ref(a.reshape(Cn, D, -1, nit)[:nchk], alive, LEVELS, t0=0)
        R.assert_same_stats({f: rec[f][:nchk] for f in R.FIELDS}, want, msg="entry " + side)
        E.assert_same_spread({f: got.spread[side][f][:nchk] for f in E.SPREAD}, wsp, msg="entry spread " + side)
        live = rec["n"] > 0
        assert (host[side]["n"].reshape(rec["n"].shape) == rec["n"]).all()
        assert (host[side]["hi"].reshape(rec["hi"].shape)[live] == rec["hi"][live]).all()
    m = {k: med(v) for k, v in t.items()}
    return dict(scenario="shell3x3_mc nit=%d" % nit, C=Cn, D=D, levels=LEVELS, wall_ms=m,
                entry_over_numpy_route=m["eval_robust_envelope"]["median"] / m["eval_batch_traj_plus_numpy"]["median"],
                bytes_to_host_per_call=dict(eval_batch_traj=int(ev.y.nbytes + ev.u.nbytes + ev.J1.nbytes + ev.status.nbytes),
                                            eval_robust_envelope=int(sum(a.nbytes for s in (got.y, got.u) for a in s.values()) +
                                                                     sum(a.nbytes for s in got.spread.values() for a in s.values()))),
                checked_candidates=nchk)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--candidates", type=int, default=4096)
    ap.add_argument("--sweep", type=int, nargs="*", default=[28, 29, 40, 48, 56, 57, 64, 80, 96, 113])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r020_envelope.json"))
    a = ap.parse_args()
    import torch

    kern = [kernel_shape(a.candidates, D, 3, 500, lv, a.reps, a.warmup) for D in (8, 32, 128) for lv in (LEVELS, [])]
    # where the two kernels cross with levels: a quarter of the candidates, the draw counts between 32 and 128 and the
    # last ones of each tile width (28, 56, 113)
    sweep = [kernel_shape(a.candidates // 4, D, 3, 500, LEVELS, a.reps, a.warmup) for D in a.sweep]
    res = dict(tool="tools/envelope_bench.py", device=torch.cuda.get_device_name(0), reps=a.reps, warmup=a.warmup, kernel=kern,
               crossing=sweep, entry=entry(256, 8, 200, a.reps, a.warmup))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    if os.path.exists(a.out):
        with open(a.out) as f:
            old = json.load(f)
        if "bench_ab" in old:
            res["bench_ab"] = old["bench_ab"]
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    import __graft_entry__ as g

    g.build()
    main()
