"""CPU, world_size 2 over gloo: mpct.dist.goal_attain_candidates after the cost all-gather.  Each rank holds
the strided shard of a generated cost table (sentinel rows NaN), gathers, and selects on the gathered tensor on
the CPU path; both ranks must return the reference's result, identically."""
import os

import numpy as np
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import goal_ref as R
from test_dist_gloo import _free_port

C_, K_, G_, NB_ = 301, 3, 40, 4


def _case():
    A = R.generated(C_, K_, 4)
    A[7, 1] = np.nan
    A[8] = -np.inf
    goals, weights = R.goal_vectors(G_, K_, 4)
    R.spoil(goals, weights, 5, "negative weight")
    return A, goals, weights


def _worker(rank, world, port, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from mpct.dist import gather_costs, goal_attain_candidates, shard_indices

        A, goals, weights = _case()
        idx = shard_indices(C_, world, rank)
        local = np.full((idx.size, K_), np.nan)
        local[idx < C_] = A[idx[idx < C_]]
        g = gather_costs(torch.from_numpy(local))
        res = goal_attain_candidates(g, goals, weights, n_best=NB_, C=C_)
        q.put((rank, {k: v.numpy() for k, v in res.items()}))
    finally:
        dist.destroy_process_group()


def test_two_rank_goal_attain(built):
    world = 2
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    got = [q.get(timeout=300) for _ in range(world)]
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    got.sort(key=lambda t: t[0])
    want = R.goal_np(*_case(), NB_)
    assert want["n_feasible"][5] == -1 and (want["n_feasible"][:5] >= 1).all() and want["wins"][7] == 0
    for rank, res in got:
        R.compare(res, want, "rank %d" % rank)
        assert res["best"].dtype == np.int32 and res["gamma"].dtype == np.float64
    for f in R.FIELDS:
        assert got[0][1][f].tobytes() == got[1][1][f].tobytes()
