"""CPU, world_size 2 over gloo: mpct.dist.pareto_candidates after the cost all-gather.  Each rank holds
the strided shard of a generated cost table (sentinel rows NaN), gathers, and analyses the gathered
tensor on the CPU path; both ranks must return the reference's result, identically."""
import os

import numpy as np
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import pareto_ref as R
from test_dist_gloo import _free_port

C_, K_, L_ = 301, 3, 6


def _table():
    A = R.generated(C_, K_, 6)
    A[7, 1] = np.nan
    return A


def _worker(rank, world, port, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from mpct.dist import gather_costs, pareto_candidates, shard_indices

        A = _table()
        idx = shard_indices(C_, world, rank)
        local = np.full((idx.size, K_), np.nan)
        local[idx < C_] = A[idx[idx < C_]]
        g = gather_costs(torch.from_numpy(local))
        res = pareto_candidates(g, C_, max_layers=L_)
        q.put((rank, {k: v.numpy() for k, v in res.items()}))
    finally:
        dist.destroy_process_group()


def test_two_rank_pareto(built):
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
    dom, layer, front, nf = R.pareto_np(_table(), L_)
    assert 1 <= nf < C_ - 1 and dom[7] == -1
    for rank, res in got:
        np.testing.assert_array_equal(res["dom_count"], dom)
        np.testing.assert_array_equal(res["layer"], layer)
        np.testing.assert_array_equal(res["front"], front[:nf])
        assert res["dom_count"].dtype == np.int32 and res["front"].dtype == np.int64
    for f in ("dom_count", "layer", "front"):
        assert got[0][1][f].tobytes() == got[1][1][f].tobytes()
