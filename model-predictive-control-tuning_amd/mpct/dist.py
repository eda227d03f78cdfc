"""Candidate-level data parallelism: one process per GPU, strided candidate shards,
one all-gather of the per-candidate cost records, identical ranking on every rank.

Rank r of W scores candidates r, r+W, r+2W, ... (the split of mpct_eval_batch_multi /
mpct_shard_candidates).  The tuning grids are built cell by cell (config 3: all 1024 lambda draws
of one (N2, Nu) pair together, N2-major), so a contiguous split hands rank r one horizon and the
heaviest rank sets the time; the strided split gives every rank the same mix of cells.

Nothing is exchanged during a simulation (VNS2.m:148-169 and GAM_fun.m:79-91 evaluate every
candidate in isolation), so the only collective is the final all-gather.  The functions here are
backend-agnostic (torch.distributed with "nccl" = RCCL on the GPU box, "gloo" in the CPU tests).
"""
from __future__ import annotations

import json
import os

import numpy as np
import torch

SKIPPED_N2 = 0  # sentinel candidate: the kernel returns status MPCT_ST_SKIPPED (8) and NaN costs


def shard_indices(C: int, world: int, rank: int) -> np.ndarray:
    """Candidates of rank's strided shard of a C-candidate grid padded to a multiple of world:
    rank, rank + world, ... (ceil(C / world) of them); indices >= C are sentinel padding."""
    per = -(-C // world)
    return rank + world * np.arange(per, dtype=np.int64)


def band_work_estimate(N2, Nu, lam, nu=3):
    """A-priori latency estimate of one band-mode simulation (config 3, mdband_kernel.hip): the
    per-step output-row scan and QP grow with N2 and the QP size 3 Nu + 1, and smaller move weights
    bind the bands more often.  Fitted on the config-3 grid's measured GI iterations and DESIGN §7's
    flop model (log-linear, Spearman 0.98 over the grid, 0.49 within an (N2, Nu) cell):
    N2^0.77 (nu Nu + 1)^2.07 prod(lambda)^-0.099."""
    N2 = np.asarray(N2, dtype=float)
    M1 = nu * np.asarray(Nu, dtype=float) + 1.0
    lg = np.log10(np.maximum(np.abs(np.asarray(lam, dtype=float)), 1e-300)).reshape(N2.size, -1).sum(1)
    return N2 ** 0.769 * M1 ** 2.067 * 10.0 ** (-0.0988 * lg)


def shard_indices_keyed(work, world: int, rank: int, heavy_first: bool = False) -> np.ndarray:
    """Work-keyed split: candidates sorted by descending estimated work, dealt to the ranks in snake
    order (0..W-1, W-1..0, ...), so every rank gets one candidate of every work level and the heavy
    tail is spread evenly; each rank's candidates in ascending index order, or with heavy_first in
    descending estimated work (the band kernel dispatches in input order).  Pads like
    shard_indices (indices >= C are sentinels, dealt last)."""
    C = len(work)
    per = -(-C // world)
    order = np.concatenate([np.argsort(-np.asarray(work, dtype=float), kind="stable"),
                            np.arange(C, per * world)])
    pos = np.arange(per * world)
    rnd, j = pos // world, pos % world
    owner = np.where(rnd % 2 == 0, j, world - 1 - j)
    mine = order[owner == rank]
    return mine if heavy_first else np.sort(mine)


def pad_shard(N2, Nu, delta, lam, idx):
    """The candidate arrays at ``idx`` (shard_indices), padding indices >= C with skipped
    sentinels (N2 = 0: status 8, NaN costs)."""
    C = len(N2)
    idx = np.asarray(idx, dtype=np.int64)
    live = idx < C
    n = idx.size
    my, nu = delta.shape[1], lam.shape[1]
    oN2 = np.full(n, SKIPPED_N2, dtype=np.int32)
    oNu = np.ones(n, dtype=np.int32)
    od = np.ones((n, my))
    ol = np.ones((n, nu))
    oN2[live], oNu[live] = N2[idx[live]], Nu[idx[live]]
    od[live], ol[live] = delta[idx[live]], lam[idx[live]]
    return oN2, oNu, od, ol


def gather_costs(local: torch.Tensor, group=None, owners=None) -> torch.Tensor:
    """All-gather equal-size per-rank cost records [n, K] -> [world * n, K] in candidate order.
    Strided shards (owners None): the gathered block is rank-major, row j of rank r is candidate
    r + j*world, so one transpose of the (world, n) leading axes restores the grid's order.  Other
    splits: owners[r] = rank r's candidate indices (shard_indices_keyed, identical on every rank);
    the rows are scattered to them (sentinel indices >= C land past the end)."""
    import torch.distributed as dist

    world = dist.get_world_size(group)
    n = local.shape[0]
    out = torch.empty((world * n,) + tuple(local.shape[1:]), dtype=local.dtype, device=local.device)
    dist.all_gather_into_tensor(out, local.contiguous(), group=group)
    if owners is None:
        return out.view((world, n) + tuple(local.shape[1:])).transpose(0, 1).reshape((world * n,) + tuple(local.shape[1:]))
    idx = torch.as_tensor(np.concatenate(owners), dtype=torch.int64, device=local.device)
    res = torch.empty_like(out)
    res[idx] = out
    return res


def rank_candidates(costs: torch.Tensor, weights: torch.Tensor, C: int | None = None) -> torch.Tensor:
    """Candidate order by ascending weighted cost (Shell3x3.m:161 Pareto weights), ties by
    candidate index; NaN costs (failed / sentinel candidates) sort last.  Identical on every
    rank because every rank sorts the same gathered tensor.  GPU tensors go through the
    library's mpct_rank_device (one key kernel + a stable device radix sort on the current
    stream); CPU tensors (the gloo tests) through torch."""
    if C is not None:
        costs = costs[:C]
    if costs.is_cuda:
        from . import _lib

        c = costs.to(torch.float64).contiguous()
        w = weights.to(device=c.device, dtype=torch.float64).contiguous()
        perm = torch.empty(c.shape[0], dtype=torch.int32, device=c.device)
        stream = torch.cuda.current_stream(c.device).cuda_stream
        rc = _lib.load().mpct_rank_device(c.data_ptr(), c.shape[0], c.shape[1], w.data_ptr(), perm.data_ptr(),
                                          stream)
        if rc != 0:
            raise RuntimeError("mpct_rank_device failed (%d): %s" % (rc, _lib.load().mpct_last_error().decode()))
        return perm.to(torch.int64)
    s = costs @ weights
    s = torch.where(torch.isnan(s), torch.full_like(s, float("inf")), s)
    return torch.argsort(s, stable=True)


def _pareto_torch(costs: torch.Tensor, max_layers: int, chunk: int = 1024):
    """The contract of mpct_pareto_device (include/mpct.h) as chunked torch expressions, on the tensor's
    device: the CPU path of pareto_candidates, and what tools/pareto_bench.py times the kernel against."""
    Cn, k = costs.shape
    dev = costs.device
    valid = ~torch.isnan(costs).any(dim=1)

    def count(alive, todo):
        """dominators among `alive` of every candidate in `todo` (index tensor)"""
        out = torch.zeros(todo.numel(), dtype=torch.int64, device=dev)
        a_idx = torch.nonzero(alive).flatten()
        for b0 in range(0, todo.numel(), chunk):
            b = costs[todo[b0:b0 + chunk]]
            acc = torch.zeros(b.shape[0], dtype=torch.int64, device=dev)
            for a0 in range(0, a_idx.numel(), chunk):
                a = costs[a_idx[a0:a0 + chunk]]
                le = (a[:, None, :] <= b[None, :, :]).all(dim=2)
                lt = (a[:, None, :] < b[None, :, :]).any(dim=2)
                acc += (le & lt).sum(dim=0)
            out[b0:b0 + chunk] = acc
        return out

    dom = torch.full((Cn,), -1, dtype=torch.int32, device=dev)
    vi = torch.nonzero(valid).flatten()
    dom[vi] = count(valid, vi).to(torch.int32)
    members = torch.nonzero(valid & (dom == 0)).flatten()
    front = torch.full((Cn,), -1, dtype=torch.int32, device=dev)
    front[:members.numel()] = members.to(torch.int32)
    layer = None
    if max_layers > 0:
        layer = torch.where(valid, max_layers, -1).to(torch.int32)
        alive = valid.clone()
        for p in range(max_layers):
            todo = torch.nonzero(alive).flatten()
            if todo.numel() == 0:
                break
            top = todo[(dom[todo] == 0) if p == 0 else (count(alive, todo) == 0)]
            layer[top] = p
            alive[top] = False
    return dom, layer, front, int(members.numel())


def pareto_candidates(costs: torch.Tensor, C: int | None = None, max_layers: int = 0) -> dict:
    """Pareto front, domination counts and layers of the gathered cost records (the multi-objective
    counterpart of rank_candidates; contract: mpct_pareto_device in include/mpct.h).  Returns a dict of
    tensors on the costs' device: dom_count [C] int32 (-1: a NaN record), front [n_front] int64 ascending,
    and layer [C] int32 with max_layers in 1 .. 64.  Identical on every rank, because every rank analyses
    the same gathered tensor and all results are integers.  GPU tensors go through mpct_pareto_device on
    the current stream; CPU tensors (the gloo tests) through chunked torch expressions."""
    if C is not None:
        costs = costs[:C]
    if costs.dim() == 1:
        costs = costs[:, None]
    if not 0 <= int(max_layers) <= 64:
        raise ValueError("max_layers must be 0 .. 64")
    c = costs.to(torch.float64).contiguous()
    n = c.shape[0]
    if c.is_cuda:
        from . import engine

        out = dict(dom_count=torch.empty(n, dtype=torch.int32, device=c.device),
                   front=torch.empty(n, dtype=torch.int32, device=c.device),
                   n_front=torch.empty(1, dtype=torch.int32, device=c.device))
        if max_layers:
            out["layer"] = torch.empty(n, dtype=torch.int32, device=c.device)
        engine.pareto_device(c, out, max_layers=max_layers)
        res = dict(dom_count=out["dom_count"], front=out["front"][:int(out["n_front"].item())].to(torch.int64))
        if max_layers:
            res["layer"] = out["layer"]
        return res
    if not 1 <= c.shape[1] <= 16:
        raise ValueError("k must be 1 .. 16")
    dom, layer, front, nf = _pareto_torch(c, int(max_layers))
    res = dict(dom_count=dom, front=front[:nf].to(torch.int64))
    if max_layers:
        res["layer"] = layer
    return res


def _goal_torch(costs: torch.Tensor, goals: torch.Tensor, weights: torch.Tensor, n_best: int, chunk: int = 128) -> dict:
    """The contract of mpct_goal_attain_device (include/mpct.h) as chunked torch expressions, on the tensor's
    device: the CPU path of goal_attain_candidates.  Elementwise float64 operations round one by one, so the
    attainment factors are the kernel's bit for bit."""
    Cn, k = costs.shape
    G, dev = goals.shape[0], costs.device
    inf = float("inf")
    soft, hard = weights > 0, weights == 0
    iw = torch.where(soft, 1.0 / weights, torch.zeros_like(weights))
    ok = torch.where(soft, torch.isfinite(weights) & torch.isfinite(iw) & torch.isfinite(goals), hard & ~torch.isnan(goals))
    valid = ok.all(dim=1) & soft.any(dim=1)
    cvalid = ~torch.isnan(costs).any(dim=1)
    best = torch.full((G, n_best), -1, dtype=torch.int32, device=dev)
    gamma = torch.full((G, n_best), float("nan"), dtype=torch.float64, device=dev)
    active = torch.full((G, n_best), -1, dtype=torch.int32, device=dev)
    nf = torch.full((G,), -1, dtype=torch.int32, device=dev)
    na = torch.full((G,), -1, dtype=torch.int32, device=dev)
    wins = torch.zeros(Cn, dtype=torch.int32, device=dev)
    for g0 in range(0, G, chunk):
        v = torch.nonzero(valid[g0:g0 + chunk]).flatten() + g0
        if v.numel() == 0:
            continue
        gl, sf, hd = goals[v][:, None, :], soft[v][:, None, :], hard[v][:, None, :]
        term = (costs[None, :, :] - gl) * iw[v][:, None, :]
        feas = cvalid[None, :] & ((costs[None, :, :] <= gl) | ~hd).all(dim=2) & ~(torch.isnan(term) & sf).any(dim=2)
        tm = torch.where(sf & ~torch.isnan(term), term, torch.full_like(term, -inf))
        top = tm.max(dim=2, keepdim=True).values
        act = ((tm == top) & sf).to(torch.int8).argmax(dim=2)           # the smallest soft j that attains the maximum
        gam = tm.gather(2, act[:, :, None])[:, :, 0]                     # its term, sign of a zero included
        nf[v] = feas.sum(dim=1).to(torch.int32)
        na[v] = (feas & (gam <= 0)).sum(dim=1).to(torch.int32)
        if not Cn:
            continue
        # NaN sorts last and the sort is stable: ascending gamma, ties by ascending candidate index
        ranked = torch.sort(torch.where(feas, gam, torch.full_like(gam, float("nan"))), dim=1, stable=True).indices
        wins += torch.bincount(ranked[:, 0][feas.any(dim=1)], minlength=Cn).to(torch.int32)
        n = min(n_best, Cn)
        if n:
            order = ranked[:, :n]
            keep = feas.gather(1, order)
            best[v, :n] = torch.where(keep, order, torch.full_like(order, -1)).to(torch.int32)
            gamma[v, :n] = torch.where(keep, gam.gather(1, order), torch.full_like(gam[:, :n], float("nan")))
            active[v, :n] = torch.where(keep, act.gather(1, order), torch.full_like(order, -1)).to(torch.int32)
    return dict(best=best, gamma=gamma, active=active, n_feasible=nf, n_attained=na, wins=wins)


def goal_attain_candidates(costs: torch.Tensor, goals, weights, n_best: int = 1, C: int | None = None) -> dict:
    """Goal-attainment selection over the gathered cost records (contract: mpct_goal_attain_device in
    include/mpct.h): per goal / weight vector the ``n_best`` candidates with the smallest attainment factor
    gamma = max_j (F_j - goal_j) / w_j among those meeting every hard objective (w_j = 0).  ``goals`` and
    ``weights`` are (k,) or (G, k), a (k,) one is broadcast.  Returns a dict of tensors on the costs' device: best,
    active [G, n_best] int32, gamma [G, n_best] float64, n_feasible, n_attained [G] int32, wins [C] int32; an
    invalid goal vector has -1 / NaN rows and -1 counts.  Identical on every rank, because every rank analyses the
    same gathered tensor in a fixed order.  GPU tensors go through mpct_goal_attain_device on the current stream;
    CPU tensors (the gloo tests) through chunked torch expressions."""
    if C is not None:
        costs = costs[:C]
    if costs.dim() == 1:
        costs = costs[:, None]
    n_best = int(n_best)
    if not 0 <= n_best <= 16:
        raise ValueError("n_best must be 0 .. 16")
    c = costs.to(torch.float64).contiguous()
    n, k = c.shape
    if not 1 <= k <= 16:
        raise ValueError("k must be 1 .. 16")
    gl = torch.as_tensor(goals, dtype=torch.float64, device=c.device)
    w = torch.as_tensor(weights, dtype=torch.float64, device=c.device)
    G = next((int(x.shape[0]) for x in (gl, w) if x.dim() == 2), 1)
    gl = (gl if gl.dim() == 2 else gl[None, :].expand(G, -1)).contiguous()
    w = (w if w.dim() == 2 else w[None, :].expand(G, -1)).contiguous()
    if gl.shape != (G, k) or w.shape != (G, k):
        raise ValueError("goals and weights must be (k,) or (G, k)")
    if not c.is_cuda:
        return _goal_torch(c, gl, w, n_best)
    from . import engine

    out = dict(n_feasible=torch.empty(G, dtype=torch.int32, device=c.device),
               n_attained=torch.empty(G, dtype=torch.int32, device=c.device),
               wins=torch.empty(n, dtype=torch.int32, device=c.device))
    if n_best:
        out.update(best=torch.empty((G, n_best), dtype=torch.int32, device=c.device),
                   gamma=torch.empty((G, n_best), dtype=torch.float64, device=c.device),
                   active=torch.empty((G, n_best), dtype=torch.int32, device=c.device))
    engine.goal_attain_device(c, gl, w, out, n_best=n_best)
    if not n_best:
        out.update(best=torch.empty((G, 0), dtype=torch.int32, device=c.device),
                   gamma=torch.empty((G, 0), dtype=torch.float64, device=c.device),
                   active=torch.empty((G, 0), dtype=torch.int32, device=c.device))
    return out


def _hv_points(lo: torch.Tensor, ref: torch.Tensor, seed: int, i0: int, i1: int) -> torch.Tensor:
    """Sample points i0 .. i1 - 1 of the hypervolume contract (include/mpct.h), [i1 - i0, k] on lo's device.
    torch has no uint64 arithmetic: int64 products wrap to the same bits, and a logical right shift is an
    arithmetic one with the copied sign bits masked off."""
    def s64(c):
        c &= (1 << 64) - 1
        return c - (1 << 64) if c >= (1 << 63) else c

    def lsr(x, s):
        return (x >> s) & ((1 << (64 - s)) - 1)

    dev, k = lo.device, lo.numel()
    i = torch.arange(i0, i1, dtype=torch.int64, device=dev)[:, None]
    j = torch.arange(k, dtype=torch.int64, device=dev)[None, :]
    x = (16 * i + j + 1) * s64(0x9E3779B97F4A7C15) + s64(int(seed))
    x = (x ^ lsr(x, 30)) * s64(0xBF58476D1CE4E5B9)
    x = (x ^ lsr(x, 27)) * s64(0x94D049BB133111EB)
    x = x ^ lsr(x, 31)
    u = lsr(x, 11).to(torch.float64) * 2.0 ** -53
    return lo + u * (ref - lo)          # three kernels: the difference and the product are rounded


def _hypervolume_torch(costs: torch.Tensor, members, lo: torch.Tensor, ref: torch.Tensor, n_samples: int, seed: int,
                       chunk: int = 4096, mchunk: int = 2048):
    """The contract of mpct_hypervolume_device (include/mpct.h) as chunked torch expressions, on the tensor's
    device: the CPU path of hypervolume_candidates, and what tools/hv_bench.py times the kernel against.
    Returns (n_covered, excl [M] int64, depth_hist [8] int64, hv)."""
    Cn, k = costs.shape
    dev = costs.device
    mem = torch.arange(Cn, dtype=torch.int64, device=dev) if members is None else members.to(torch.int64)
    pos = torch.nonzero((mem >= 0) & (mem < Cn)).flatten()      # an entry outside [0, C) is skipped
    A = costs[mem[pos]]                                         # a NaN row covers nothing: NaN <= p is false
    excl = torch.zeros(mem.numel(), dtype=torch.int64, device=dev)
    hist = torch.zeros(8, dtype=torch.int64, device=dev)
    for i0 in range(0, n_samples, chunk):
        P = _hv_points(lo, ref, seed, i0, min(n_samples, i0 + chunk))
        depth = torch.zeros(P.shape[0], dtype=torch.int64, device=dev)
        which = torch.zeros(P.shape[0], dtype=torch.int64, device=dev)
        for m0 in range(0, A.shape[0], mchunk):
            le = (A[None, m0:m0 + mchunk, :] <= P[:, None, :]).all(dim=2)
            depth += le.sum(dim=1)
            which += (le * pos[None, m0:m0 + mchunk]).sum(dim=1)   # the covering entry itself where depth == 1
        hist += torch.bincount(depth.clamp(max=7), minlength=8)
        excl += torch.bincount(which[depth == 1], minlength=mem.numel())
    n_cov = int(n_samples - hist[0].item())
    vol = 1.0
    for l, r in zip(lo.tolist(), ref.tolist()):
        vol *= r - l
    return n_cov, excl, hist, (float(n_cov) / float(n_samples)) * vol


def hypervolume_candidates(costs: torch.Tensor, front=None, lo=None, ref=None, n_samples: int = 1 << 20, seed: int = 0,
                           C: int | None = None) -> dict:
    """Hypervolume of the members ``front`` (indices into the gathered cost records, e.g. pareto_candidates'
    front; -1 entries are skipped; None: every record) inside the box [lo, ref], and every member's exclusive
    contribution (contract: mpct_hypervolume_device in include/mpct.h).  Returns a dict: hv (float), n_covered
    (int), n_samples, excl [M] int64 and depth_hist [8] int64 on the costs' device, lo and ref [k] float64
    there too.  Identical on every rank: the sample points are a function of (seed, i) and all counts are
    integers.  ``lo`` / ``ref`` None: mpct.engine.default_box on the host.  GPU tensors go through
    mpct_hypervolume_device on the current stream; CPU tensors (the gloo tests) through chunked torch
    expressions."""
    from . import engine

    if C is not None:
        costs = costs[:C]
    if costs.dim() == 1:
        costs = costs[:, None]
    c = costs.to(torch.float64).contiguous()
    n, k = c.shape
    if not 1 <= k <= 16:
        raise ValueError("k must be 1 .. 16")
    if not 1 <= int(n_samples) <= 1 << 30:
        raise ValueError("n_samples must be 1 .. 2**30")
    mem = None if front is None else torch.as_tensor(front).to(device=c.device, dtype=torch.int32).contiguous().flatten()
    if lo is None or ref is None or not torch.is_tensor(lo) or not torch.is_tensor(ref):
        lo, ref = engine.default_box(c.cpu().numpy(), None if mem is None else mem.cpu().numpy(),
                                     lo.cpu().numpy() if torch.is_tensor(lo) else lo,
                                     ref.cpu().numpy() if torch.is_tensor(ref) else ref)
    lo = torch.as_tensor(lo, dtype=torch.float64).to(c.device).contiguous()
    ref = torch.as_tensor(ref, dtype=torch.float64).to(c.device).contiguous()
    if not (bool(torch.isfinite(lo).all()) and bool(torch.isfinite(ref).all()) and bool((lo < ref).all())):
        raise ValueError("the box needs finite lo and ref with lo < ref")
    M = n if mem is None else mem.numel()
    if c.is_cuda:
        out = dict(n_covered=torch.empty(1, dtype=torch.int64, device=c.device),
                   excl=torch.empty(M, dtype=torch.int64, device=c.device),
                   depth_hist=torch.empty(8, dtype=torch.int64, device=c.device),
                   hv=torch.empty(1, dtype=torch.float64, device=c.device))
        engine.hypervolume_device(c, out, lo, ref, members=mem, n_samples=n_samples, seed=seed)
        n_cov, excl, hist, hv = int(out["n_covered"].item()), out["excl"], out["depth_hist"], float(out["hv"].item())
    else:
        n_cov, excl, hist, hv = _hypervolume_torch(c, mem, lo, ref, int(n_samples), int(seed))
    return dict(hv=hv, n_covered=n_cov, n_samples=int(n_samples), excl=excl, depth_hist=hist, lo=lo, ref=ref)


def _hypervolume_exact_torch(costs: torch.Tensor, members, lo: torch.Tensor, ref: torch.Tensor):
    """The sweep of mpct_hypervolume_exact_device (include/mpct.h) as torch expressions on the
    tensor's device: the CPU path of hypervolume_exact_candidates.  The same terms as the kernel, products of
    non-negative differences of clipped coordinates, summed in another order: it agrees with the device within
    the contract's bound, not bitwise.  Returns (hv, excl [M] float64, n_active)."""
    dev, f64 = costs.device, torch.float64
    n, k = costs.shape
    idx = torch.arange(n, device=dev) if members is None else members.to(torch.int64)
    M = idx.numel()
    excl = torch.zeros(M, dtype=f64, device=dev)
    ok = (idx >= 0) & (idx < n)
    rows = costs[idx.clamp(0, max(n - 1, 0))] if n else torch.full((M, k), float("nan"), dtype=f64, device=dev)
    L = torch.cat([lo, torch.zeros(3 - k, dtype=f64, device=dev)])
    R = torch.cat([ref, torch.ones(3 - k, dtype=f64, device=dev)])
    b = torch.cat([rows, torch.zeros(M, 3 - k, dtype=f64, device=dev)], dim=1)
    nan = torch.isnan(b).any(dim=1)
    b = torch.where(b > L, b, L.expand_as(b)) + 0.0
    act = ok & ~nan & (b < R).all(dim=1)
    pos = torch.nonzero(act).flatten()
    na = int(pos.numel())
    if na == 0:
        return 0.0, excl, 0
    b = b[pos]

    def lexorder(keys):   # stable sorts from the last key to the first: the order (keys[0], keys[1], .., entry)
        o = torch.arange(na, device=dev)
        for key in reversed(keys):
            o = o[torch.sort(key[o], stable=True).indices]
        return o

    ox = lexorder([b[:, 0], b[:, 1], b[:, 2]])
    oz = lexorder([b[:, 2], b[:, 0], b[:, 1]])
    zrank = torch.empty(na, dtype=torch.int64, device=dev)
    zrank[oz] = torch.arange(na, device=dev)
    xs, yx, zrx = b[ox, 0], b[ox, 1], zrank[ox]
    zs = b[oz, 2]
    dx = torch.cat([xs[1:], R[0:1]]) - xs
    z1 = torch.cat([zs[1:], R[2:3]])
    inf = torch.full((na,), float("inf"), dtype=f64, device=dev)
    none = torch.full((na,), -1, dtype=torch.int64, device=dev)
    lane = torch.arange(na, device=dev)
    hv = torch.zeros((), dtype=f64, device=dev)
    part = torch.zeros(na, dtype=f64, device=dev)   # per entry in x order
    for s in torch.nonzero(z1 > zs).flatten().tolist():
        dz = z1[s] - zs[s]
        on = zrx <= s
        m1, h, m2 = torch.where(on, yx, inf), torch.where(on, lane, none), inf.clone()
        d = 1
        while d < na:   # inclusive scan of (m1, holder, m2), the left side winning a tie
            a1 = torch.cat([inf[:d], m1[:-d]])
            ha = torch.cat([none[:d], h[:-d]])
            a2 = torch.cat([inf[:d], m2[:-d]])
            left = a1 <= m1
            m2 = torch.where(left, torch.minimum(a2, m1), torch.minimum(m2, a1))
            m1, h = torch.where(left, a1, m1), torch.where(left, ha, h)
            d *= 2
        any_ = m1 < inf
        zero = torch.zeros_like(dx)
        hv = hv + dz * torch.where(any_, dx * (R[1] - m1), zero).sum()
        te = torch.where(any_, dx * (torch.minimum(m2, R[1:2]) - m1), zero)
        part.index_add_(0, h.clamp(min=0), dz * te)
    excl[pos[ox]] = part
    return float(hv), excl, na


def hypervolume_exact_candidates(costs: torch.Tensor, front=None, lo=None, ref=None, C: int | None = None) -> dict:
    """Exact hypervolume of the members ``front`` (indices into the gathered cost records, e.g.
    pareto_candidates' front; -1 entries are skipped; None: every record) inside the box [lo, ref], for at most
    three objectives, and every member's exclusive contribution (contract: mpct_hypervolume_exact_device in
    include/mpct.h).  Returns a dict: hv (float), n_active (int), excl [M] float64 on the costs' device, lo and
    ref [k] float64 there too.  ``lo`` / ``ref`` None: mpct.engine.default_box on the host.  GPU tensors go
    through mpct_hypervolume_exact_device on the current stream; CPU tensors (the gloo tests) through a torch
    restatement of the sweep, which sums the same non-negative terms in another order: the two paths agree
    within the contract's bound, (M^2 + 8) 2^-53 vol, not bitwise."""
    from . import engine

    if C is not None:
        costs = costs[:C]
    if costs.dim() == 1:
        costs = costs[:, None]
    c = costs.to(torch.float64).contiguous()
    n, k = c.shape
    if not 1 <= k <= 3:
        raise ValueError("k must be 1 .. 3: the exact hypervolume serves at most three objectives")
    mem = None if front is None else torch.as_tensor(front).to(device=c.device, dtype=torch.int32).contiguous().flatten()
    M = n if mem is None else mem.numel()
    if M > 65536:
        raise ValueError("at most 65536 members")
    if lo is None or ref is None or not torch.is_tensor(lo) or not torch.is_tensor(ref):
        lo, ref = engine.default_box(c.cpu().numpy(), None if mem is None else mem.cpu().numpy(),
                                     lo.cpu().numpy() if torch.is_tensor(lo) else lo,
                                     ref.cpu().numpy() if torch.is_tensor(ref) else ref)
    lo = torch.as_tensor(lo, dtype=torch.float64).to(c.device).contiguous()
    ref = torch.as_tensor(ref, dtype=torch.float64).to(c.device).contiguous()
    if not (bool(torch.isfinite(lo).all()) and bool(torch.isfinite(ref).all()) and bool((lo < ref).all())):
        raise ValueError("the box needs finite lo and ref with lo < ref")
    if c.is_cuda:
        out = dict(hv=torch.empty(1, dtype=torch.float64, device=c.device),
                   excl=torch.empty(M, dtype=torch.float64, device=c.device),
                   n_active=torch.empty(1, dtype=torch.int64, device=c.device))
        engine.hypervolume_exact_device(c, out, lo, ref, members=mem)
        hv, excl, na = float(out["hv"].item()), out["excl"], int(out["n_active"].item())
    else:
        hv, excl, na = _hypervolume_exact_torch(c, mem, lo, ref)
    return dict(hv=hv, n_active=na, excl=excl, lo=lo, ref=ref)


def _hv_select_torch(costs: torch.Tensor, members, lo: torch.Tensor, ref: torch.Tensor, n_samples: int, seed: int,
                     n_pick: int, chunk: int = 4096, mchunk: int = 2048) -> dict:
    """The contract of mpct_hv_select_device (include/mpct.h) as chunked torch expressions in int64 arithmetic,
    on the tensor's device: the CPU path of hv_select_candidates, and what tools/hv_select_bench.py times the
    kernels against.  Every round regenerates the points chunk by chunk; the "still uncovered" bits stay."""
    Cn, k = costs.shape
    dev = costs.device
    mem = torch.arange(Cn, dtype=torch.int64, device=dev) if members is None else members.to(torch.int64)
    M = mem.numel()
    pos = torch.nonzero((mem >= 0) & (mem < Cn)).flatten()      # an entry outside [0, C) is skipped
    A = costs[mem[pos]]                                         # a NaN row covers nothing
    alive = torch.ones(n_samples, dtype=torch.bool, device=dev)
    out = dict(pos=torch.full((n_pick,), -1, dtype=torch.int32, device=dev),
               index=torch.full((n_pick,), -1, dtype=torch.int32, device=dev),
               gain=torch.zeros(n_pick, dtype=torch.int64, device=dev),
               covered=torch.zeros(n_pick, dtype=torch.int64, device=dev),
               ties=torch.zeros(n_pick, dtype=torch.int32, device=dev))
    n_picked, covered, n_all, row = 0, 0, 0, None
    for r in range(n_pick if pos.numel() else 0):
        gains = torch.zeros(M, dtype=torch.int64, device=dev)
        for i0 in range(0, n_samples, chunk):
            i1 = min(n_samples, i0 + chunk)
            P = _hv_points(lo, ref, seed, i0, i1)
            if row is not None:
                alive[i0:i1] &= ~(row[None, :] <= P).all(dim=1)
            live = alive[i0:i1]
            if not bool(live.any()):
                continue
            anyc = torch.zeros(i1 - i0, dtype=torch.bool, device=dev)
            for m0 in range(0, A.shape[0], mchunk):
                le = (A[None, m0:m0 + mchunk, :] <= P[:, None, :]).all(dim=2)
                anyc |= le.any(dim=1)
                gains[pos[m0:m0 + mchunk]] += (le & live[:, None]).sum(dim=0)
            if r == 0:                                          # a point that nothing covers never counts again
                alive[i0:i1] &= anyc
        if r == 0:
            n_all = int(alive.sum().item())
        best = int(gains.max().item())
        if best == 0:
            break
        m = int(torch.nonzero(gains == best).flatten()[0].item())
        covered += best
        n_picked = r + 1
        row = costs[int(mem[m].item())]
        out["pos"][r], out["index"][r], out["gain"][r] = m, int(mem[m].item()), best
        out["covered"][r], out["ties"][r] = covered, int((gains == best).sum().item())
    out["covered"][n_picked:] = covered
    vol = 1.0
    for l, h in zip(lo.tolist(), ref.tolist()):
        vol *= h - l
    out["hv"] = (out["covered"].to(torch.float64) / float(n_samples)) * vol
    out.update(n_picked=n_picked, n_covered_all=n_all)
    return out


def hv_select_candidates(costs: torch.Tensor, n_pick: int, front=None, lo=None, ref=None, n_samples: int = 1 << 20,
                         seed: int = 0, C: int | None = None) -> dict:
    """The ``n_pick`` members of ``front`` (indices into the gathered cost records, e.g. pareto_candidates' front;
    -1 entries are skipped; None: every record) that carry it, by greedy forward selection on the coverage
    count (contract: mpct_hv_select_device in include/mpct.h).  Returns a dict: n_picked, n_covered_all, n_samples
    (int); pos, index, ties [n_pick] int32, gain, covered [n_pick] int64 and hv [n_pick] float64 on the costs'
    device, lo and ref [k] there too.  Identical on every rank, as hypervolume_candidates.  GPU tensors go
    through mpct_hv_select_device on the current stream; CPU tensors (the gloo tests) through chunked torch
    expressions."""
    from . import engine

    if C is not None:
        costs = costs[:C]
    if costs.dim() == 1:
        costs = costs[:, None]
    c = costs.to(torch.float64).contiguous()
    n, k = c.shape
    if not 1 <= k <= 16:
        raise ValueError("k must be 1 .. 16")
    if not 1 <= int(n_samples) <= 1 << 30:
        raise ValueError("n_samples must be 1 .. 2**30")
    if not 1 <= int(n_pick) <= 1024:
        raise ValueError("n_pick must be 1 .. 1024")
    n_pick = int(n_pick)
    mem = None if front is None else torch.as_tensor(front).to(device=c.device, dtype=torch.int32).contiguous().flatten()
    if lo is None or ref is None or not torch.is_tensor(lo) or not torch.is_tensor(ref):
        lo, ref = engine.default_box(c.cpu().numpy(), None if mem is None else mem.cpu().numpy(),
                                     lo.cpu().numpy() if torch.is_tensor(lo) else lo,
                                     ref.cpu().numpy() if torch.is_tensor(ref) else ref)
    lo = torch.as_tensor(lo, dtype=torch.float64).to(c.device).contiguous()
    ref = torch.as_tensor(ref, dtype=torch.float64).to(c.device).contiguous()
    if not (bool(torch.isfinite(lo).all()) and bool(torch.isfinite(ref).all()) and bool((lo < ref).all())):
        raise ValueError("the box needs finite lo and ref with lo < ref")
    if c.is_cuda:
        i32 = lambda: torch.empty(n_pick, dtype=torch.int32, device=c.device)
        i64 = lambda m: torch.empty(m, dtype=torch.int64, device=c.device)
        out = dict(n_picked=i64(1), pos=i32(), index=i32(), gain=i64(n_pick), covered=i64(n_pick),
                   hv=torch.empty(n_pick, dtype=torch.float64, device=c.device), ties=i32(), n_covered_all=i64(1))
        engine.hv_select_device(c, n_pick, out, lo, ref, members=mem, n_samples=n_samples, seed=seed)
        out["n_picked"], out["n_covered_all"] = int(out["n_picked"].item()), int(out["n_covered_all"].item())
    else:
        out = _hv_select_torch(c, mem, lo, ref, int(n_samples), int(seed), n_pick)
    out.update(n_samples=int(n_samples), lo=lo, ref=ref)
    return out


# measured one-GPU time of every config-3 cell alone (tools/shard_balance.py --cells): the (N2, Nu)
# cells of mpct.scenarios.config3_grid with 1024 lambda draws each, whole and in two halves
CELL_TABLE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "config3_cells.json")


def load_cell_table(path: str = CELL_TABLE) -> dict:
    """{(N2, Nu): {"ms": whole cell, "half_ms": [half 0, half 1], "n": draws}} from the committed
    table (tools/shard_balance.py --cells writes it)."""
    with open(path) as f:
        tj = json.load(f)
    return {(int(c["N2"]), int(c["Nu"])): dict(ms=float(c["ms"]), half_ms=[float(x) for x in c["half_ms"]],
                                               n=int(c["n"])) for c in tj["cells"]}


def cell_halves(idx, work):
    """The two halves of one cell's candidates `idx` (ascending): sorted by descending estimated
    work (ties by index) and dealt alternately, so both halves get the same share of the heavy draws."""
    order = np.asarray(idx)[np.argsort(-np.asarray(work, dtype=float), kind="stable")]
    return np.sort(order[0::2]), np.sort(order[1::2])


# overlap of a shard's cells on one GPU: the cells' class launches run side by side and their
# alone-times are mostly latency, not occupancy, so a shard takes about its heaviest cell plus a
# fraction of the others.  Least squares over the 48 shards of six measured plans
# (profiles/r06b_shard_plans.json): 0.873 x heaviest + 0.470 x the rest (rms 12 ms), i.e. the rest
# at 0.54 of the heaviest's weight
SHARD_OVERLAP = 0.54
# cells costlier than this are split into their two halves before packing (None: an even share,
# total / world).  Splitting measured no better: a half's alone-time is most of its cell's (the
# heaviest cell 129 ms whole, 119 + 93 ms as halves; mpct/config3_cells.json, profiles/r06a_shard_balance.json), so halves add load
SPLIT_MS = None


def plan_cells_lpt(N2, Nu, lam, world: int, table: dict | None = None, nu: int = 3, split_ms: float | None = SPLIT_MS,
                   beta: float = SHARD_OVERLAP):
    """Config 3's split from measured cell times.  The candidates are grouped
    into their (N2, Nu) cells, every cell costed by the committed table (a partial cell pro rata by
    its count; a cell the table lacks by band_work_estimate, scaled by the table's median ms per
    estimate unit).  A cell costlier than split_ms (None: an even share, total / world) is split
    into two halves (cell_halves; their own measured times for a whole table cell).  Then greedy
    longest-processing-time packing under the shard model of SHARD_OVERLAP: a shard's predicted
    time is its heaviest unit plus beta times the rest (beta = 1: plain LPT on sums); units by
    descending time (ties by cell), each to the rank whose prediction it raises least (ties by
    rank).  Every rank scores few cells, so its class launches stay full, and the predicted times
    balance.  Deterministic: every rank derives the same owners.

    Returns (owners, loads): owners[r] = rank r's candidate indices, ascending, padded to one size
    with distinct sentinel indices >= C (gather_costs scatters them past the grid); loads[r] = the
    predicted ms of rank r."""
    N2 = np.asarray(N2)
    Nu = np.asarray(Nu)
    C = N2.size
    table = load_cell_table() if table is None else table
    work = band_work_estimate(N2, Nu, lam, nu)
    keys = sorted(set(zip(N2.tolist(), Nu.tolist())))
    groups = {k: np.nonzero((N2 == k[0]) & (Nu == k[1]))[0] for k in keys}
    scale = float(np.median([t["ms"] / np.sum(band_work_estimate(np.full(t["n"], k[0]), np.full(t["n"], k[1]),
                                                                   np.ones((t["n"], nu)), nu))
                             for k, t in table.items()])) if table else 1.0
    cost = {}
    for k, idx in groups.items():
        t = table.get(k)
        cost[k] = t["ms"] * idx.size / t["n"] if t else scale * float(np.sum(work[idx]))
    lim = sum(cost.values()) / world if split_ms is None else split_ms
    units = []  # (ms, cell rank for ties, half, indices)
    for ci, k in enumerate(keys):
        idx = groups[k]
        t = table.get(k)
        if cost[k] > lim and idx.size >= 2:
            halves = cell_halves(idx, work[idx])
            for h, part in enumerate(halves):
                ms = t["half_ms"][h] * 2 * part.size / t["n"] if t else cost[k] * part.size / idx.size
                units.append((ms, ci, h, part))
        else:
            units.append((cost[k], ci, 0, idx))
    units.sort(key=lambda u: (-u[0], u[1], u[2]))
    top = [0.0] * world   # heaviest unit of each rank
    rest = [0.0] * world  # the sum of its others
    mine = [[] for _ in range(world)]
    for ms, _, _, idx in units:
        new = [max(top[r], ms) + beta * (rest[r] + min(top[r], ms)) for r in range(world)]
        r = int(np.argmin(new))
        rest[r] += min(top[r], ms)
        top[r] = max(top[r], ms)
        mine[r].append(idx)
    loads = [top[r] + beta * rest[r] for r in range(world)]
    owners = [np.sort(np.concatenate(m)) if m else np.zeros(0, np.int64) for m in mine]
    n = max(o.size for o in owners)
    nxt = C
    for r in range(world):
        pad = n - owners[r].size
        owners[r] = np.concatenate([owners[r], np.arange(nxt, nxt + pad)]).astype(np.int64)
        nxt += pad
    return owners, loads


def plan_shards(N2, Nu, lam, world: int, rank: int, keyed: bool | str = False, nu: int = 3):
    """The candidates rank scores and the owners table gather_costs needs: strided shards (owners
    None); keyed="cells" (config 3, bench.py): plan_cells_lpt over the committed cell-time table;
    keyed=True: round 3's snake deal of shard_indices_keyed by band_work_estimate (kept for the
    shard-balance comparison: measured slower).  The owners are identical on every
    rank, so the gathered rows land in the grid's order.  Returns (idx, owners)."""
    if keyed == "cells":
        owners, _ = plan_cells_lpt(N2, Nu, lam, world, nu=nu)
        return owners[rank], owners
    if keyed:
        work = band_work_estimate(N2, Nu, lam, nu)
        owners = [shard_indices_keyed(work, world, k) for k in range(world)]
        return owners[rank], owners
    return shard_indices(len(N2), world, rank), None


def worst_over_draws(J: torch.Tensor, n: int, nref: int) -> torch.Tensor:
    """Per-candidate cost of a Monte-Carlo batch (config 4): the plant-mismatch draws of one
    candidate ride the reference dimension (simulation s = c*nref + k, DTC_GPC_WW.m:18-19 with one
    mismatched plant per draw) and so sit on the candidate's rank; its record is the worst case over
    them, per output.  A failed or sentinel draw (NaN) makes the candidate's record NaN."""
    if nref == 1:
        return J
    return J.view(n, nref, J.shape[-1]).amax(dim=1)


def gather_and_rank(J: torch.Tensor, n: int, nref: int, weights: torch.Tensor, C: int, owners=None,
                    distributed: bool = True):
    """The data-parallel epilogue of one scoring step: the rank's simulation records J [n*nref, K]
    -> per-candidate records (worst_over_draws) -> one all-gather (gather_costs, owners as
    plan_shards returns them) -> the ranking every rank computes (rank_candidates) over the C real
    candidates.  Returns (gathered records [>= C, K], order [C]).

    The per-candidate records of engine.eval_robust_device plug in directly: pass the rank's
    ``worst`` (or ``mean``) tensor [n, my], with the candidates whose ``n_failed`` exceeds the
    tolerated count set to NaN (RobustResult.scores does the same on the host), as J with nref = 1:
    ``gather_and_rank(worst, n, 1, weights, C)``.  NaN records rank last."""
    local = worst_over_draws(J, n, nref)
    costs = gather_costs(local, owners=owners) if distributed else local
    return costs, rank_candidates(costs, weights, C)
