"""Calls of the three evaluation entries (mpct_eval_batch_device, mpct_eval_batch, mpct_eval_batch_multi)
with an explicit set of requested result fields, for tests/test_result_records_gpu.py (test helper; the
product API always passes all six cost fields).

Every requested buffer has GUARD elements before and after its S rows, and the whole buffer, guards
and rows, is filled with a canary before the call: a NaN with a fixed payload for doubles, 0x5A5A5A5A
for the int32 status and its 64-bit analogue for qp_iters.  A field that is not requested is passed as
NULL.  After the call the guards must be bit-identical to the canary, no element of a row may still
hold it (the kernels' own NaN has another payload), and no status may be MPCT_ST_NOT_RUN.

The candidate pools: 16 distinct valid candidates followed by three invalid ones (N2 = 0, Nu > N2,
N2 > n2_max: statuses 8, 16, 16).  A large batch is the pool tiled and permuted with a fixed seed
(tiled), so every record of it is known, bitwise, from one small call of the pool."""
import ctypes as C

import numpy as np

COST = ("J1", "j21", "j22", "Jnu", "status", "qp_iters")
TRAJ = ("y", "u", "ys", "uopt")
GUARD = 64
NIT = 60
ST_NOT_RUN = 128
CANARY = {np.dtype(np.float64): 0x7FF85A5A5A5A5A5A,   # a quiet NaN, payload 0x5A..; the kernels write 0x7ff8000000000000
          np.dtype(np.int32): 0x5A5A5A5A,
          np.dtype(np.int64): 0x5A5A5A5A5A5A5A5A}

# the field subsets of the large calls
BENCH = ("J1", "j22", "status", "qp_iters")            # bench.py's request
SINGLES = [(f,) for f in COST] + [COST]
FULL_SET = [(f,) for f in COST] + [tuple(g for g in COST if g != f) for f in COST] + [BENCH, COST]
assert len(FULL_SET) == 14 and len(SINGLES) == 7


def subset_id(fields):
    if tuple(fields) == COST:
        return "all"
    if tuple(fields) == BENCH:
        return "bench"
    return "+".join(fields) if len(fields) <= 2 else "no-" + "".join(f for f in COST if f not in fields)


def dtype_of(field):
    return np.dtype(np.int32 if field == "status" else np.int64 if field == "qp_iters" else np.float64)


def width(sc, field):
    """Elements per simulation of a result field."""
    return {"J1": sc.my, "j21": sc.my, "j22": sc.my, "Jnu": sc.nu, "status": 1, "qp_iters": 1,
            "y": sc.my * sc.nit, "ys": sc.my * sc.nit, "u": sc.nu * sc.nit, "uopt": sc.nu * sc.nit}[field]


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int64) if a.dtype == np.float64 else a


# ---------------------------------------------------------------------------------------------
# candidate pools
def pool(my, nu, n2_lo, n2_max, nu_lo, nu_max, dlog, llog, seed, nu_split=None):
    """(N2, Nu, delta, lambda) of 19 candidates: 16 valid ones drawn with numpy default_rng(seed) (N2 in
    n2_lo..n2_max, Nu in nu_lo..min(nu_max, N2), log10 delta ~ U(dlog), log10 lambda ~ U(llog); with
    nu_split the first eight take Nu <= nu_split and the last eight Nu > nu_split, their N2 raised to Nu
    where it was shorter), then N2 = 0, Nu > N2 (both inside the scenario's ranges) and N2 = n2_max + 1."""
    rng = np.random.default_rng(seed)
    N2 = rng.integers(n2_lo, n2_max + 1, 16)
    if nu_split is None:
        Nu = rng.integers(nu_lo, nu_max + 1, 16)
    else:
        Nu = np.concatenate([rng.integers(nu_lo, nu_split + 1, 8), rng.integers(nu_split + 1, nu_max + 1, 8)])
        N2[8:] = np.maximum(N2[8:], Nu[8:])   # the upper class keeps its Nu
    Nu = np.minimum(Nu, N2)
    d = 10.0 ** rng.uniform(dlog[0], dlog[1], (16, my))
    l = 10.0 ** rng.uniform(llog[0], llog[1], (16, nu))
    N2 = np.concatenate([N2, [0, nu_max - 1, n2_max + 1]]).astype(np.int32)
    Nu = np.concatenate([Nu, [nu_lo, nu_max, nu_lo]]).astype(np.int32)
    d = np.concatenate([d, np.full((3, my), 0.1)])
    l = np.concatenate([l, np.full((3, nu), 0.05)])
    key = np.concatenate([N2[:16, None], Nu[:16, None], d[:16], l[:16]], axis=1)
    assert len(np.unique(key, axis=0)) == 16   # distinct candidates
    return N2, Nu, d, l


INVALID_STATUS = (8, 16, 16)   # of pool candidates 16, 17, 18


def shell_pool(nu_max):
    """Shell 3x3 at n2_max = 30: tracking weights 1e-3..1e-1 and move weights 1e-3..1e-1 keep every
    loop clean (status 0 on the C port on all three reference sets of shell_refs).  nu_max = 8: eight
    candidates of the M <= 16 class (Nu <= 5) and eight of the <32> class (Nu = 6..8)."""
    return pool(3, 3, 8, 30, 1, nu_max, (-3, -1), (-3, -1), 20250701 + nu_max, nu_split=5 if nu_max > 5 else None)


def shell_refs(r):
    """Three distinct reference sets from the scenario's r [3, nit]: r, half of it, and its mirror
    image at three quarters."""
    return np.stack([r, 0.5 * r, -0.75 * r])


def scenario(name):
    """One scenario of tests/test_result_records_gpu.py, nit = NIT steps (no GPU needed to build it):
    dict(sc, pool, refs [nref_max, my, nit], v, open_loop, instance: what mpct_kernel_instance must say).
      shell5     Shell 3x3, n2_max 30, nu_max 5: the small-plant kernel alone
      shell8     nu_max 8 (M up to 24): the small-plant kernel and the general <32> class on fanned streams
      shell8-ol  the same with open_loop: the EXT instances of both classes, j21 and Jnu live
      dtc        WoodBerry config 4, three plant draws riding on three reference sets
      band       the synthetic 2 x (1 + 1) band plant with the output-bias estimator (band_mismatch_ref.py)
      nmpc       Van de Vusse NMPC, N <= 9, Nu <= 8 (M = 16: both QP-size classes)"""
    if name.startswith("shell"):
        from mpct.scenarios import shell3x3

        nu_max = 5 if name == "shell5" else 8
        sc, r, _ = shell3x3(n2_max=30, nu_max=nu_max, nit=NIT)
        ol = name.endswith("-ol")
        inst = {"shell5": "gpc_small_kernel", "shell8": "gpc_small_kernel + gpc_closed_loop_kernel<32,false,false>",
                "shell8-ol": "gpc_closed_loop_kernel<16,false,true> + <32,false,true>"}[name]
        return dict(sc=sc, pool=shell_pool(nu_max), refs=shell_refs(r), v=None, open_loop=ol, instance=inst)
    if name == "dtc":
        from mpct.dtc import woodberry_mc

        sc, refs, v, _ = woodberry_mc(draws=3, n2_max=30, nu_max=10, nit=NIT)
        # M = 2 Nu: Nu <= 8 runs dtc_small_kernel<16>, Nu = 9, 10 the <32> instance
        return dict(sc=sc, pool=pool(2, 2, 3, 30, 1, 10, (-1, 1), (-1, 1), 20250711, nu_split=8), refs=refs, v=v,
                    open_loop=False, instance="dtc_small_kernel<16> + dtc_small_kernel<32>")
    if name == "band":
        import band_mismatch_ref as bm

        sc = bm.synthetic_scenario(bm.synthetic_plants()[1], nit=NIT)
        r, v, _ = bm.synthetic_signals(NIT)
        return dict(sc=sc, pool=pool(2, 1, 3, 12, 1, 3, (-1, 0), (-1.5, 0.5), 20250712), refs=r[None], v=v[None],
                    open_loop=False,
                    instance="mdband_closed_loop_kernel (QP-size x LDS-tier class launches) + output-bias estimator")
    if name == "nmpc":
        from mpct import nmpc

        x0 = nmpc.steady_state()
        r, yref = nmpc.vandevusse_signals(x0, NIT)
        sc = nmpc.NmpcScenario(x0, nmpc.VDV_U0, nmpc.VDV_UMIN, nmpc.VDV_UMAX, nmpc.VDV_XMIN, nmpc.VDV_XMAX, yref, 9, 8)
        # M = 2 Nu: Nu <= 7 runs the M <= 15 class, Nu = 8 the <32> class
        return dict(sc=sc, pool=pool(2, 2, 3, 9, 2, 8, (-0.7, 0.0), (-1.5, -0.5), 20250713, nu_split=7), refs=r[None],
                    v=None, open_loop=False, instance="nmpc_closed_loop_kernel (QP-size x LDS-tier class launches)")
    raise ValueError(name)


def tiled(C, seed=20250702):
    """Pool indices of a C-candidate batch: the 19 pool candidates tiled, then permuted."""
    return np.random.default_rng(seed).permutation(np.arange(C) % 19)


# ---------------------------------------------------------------------------------------------
# the calls
class Call:
    """One call in flight (the device entry is not synchronised): finish() waits for it, checks the
    guards and canaries and returns {field: rows [S, width]}."""

    def __init__(self, rc, sc, S, bufs, keep, stream):
        self.rc, self.sc, self.S, self.bufs, self.keep, self.stream = rc, sc, S, bufs, keep, stream

    def finish(self):
        from mpct import _lib

        assert self.rc == 0, (self.rc, _lib.last_error())
        if self.stream is not None:
            self.stream.synchronize()
        out = {}
        for f, buf in self.bufs.items():
            a = buf if isinstance(buf, np.ndarray) else buf.cpu().numpy()
            dt = dtype_of(f)
            can = a.dtype.type(CANARY[dt])
            n = self.S * width(self.sc, f)
            assert a.size == n + 2 * GUARD
            assert np.all(a[:GUARD] == can) and np.all(a[GUARD + n:] == can), "guard of %s overwritten" % f
            rows = a[GUARD:GUARD + n]
            left = np.flatnonzero(rows == can)
            assert left.size == 0, "%s: %d of %d elements never written (first %s)" % (f, left.size, n, left[:8])
            out[f] = rows.view(dt).reshape(self.S, -1).copy()
        if "status" in out:
            assert not np.any(out["status"] & ST_NOT_RUN), np.flatnonzero(out["status"] & ST_NOT_RUN)[:8]
        self.keep = self.bufs = None
        return out


def launch(entry, sc, cands, refs, v=None, fields=COST, open_loop=False, want_traj=False, devices=(0, 0),
           stream=None):
    """Enqueue (device entry) or run (host entries) one call that requests exactly `fields`.
    entry: "device" (mpct_eval_batch_device on `stream`, a torch stream; None: the current one),
    "host" (mpct_eval_batch) or "multi" (mpct_eval_batch_multi over `devices`)."""
    from mpct import _lib
    from mpct.engine import _batch_args, _opts

    N2, Nu, d, l, refs, Cn, nref, vv = _batch_args(sc, *cands, refs, v)
    S = Cn * nref
    res = _lib.MpctResult()
    bufs, keep = {}, []
    o = _opts(open_loop, want_traj, 0 if entry != "multi" else -1)
    if entry == "device":
        import torch

        dev = torch.device("cuda", 0)
        if stream is None:
            stream = torch.cuda.current_stream(dev)
        ins = [torch.tensor(a, device=dev) if a is not None else None for a in (N2, Nu, d, l, refs, vv)]
        for f in fields:
            dt = dtype_of(f)
            tdt = torch.int32 if dt == np.int32 else torch.int64    # doubles as their bit patterns
            t = torch.full((S * width(sc, f) + 2 * GUARD,), CANARY[dt], dtype=tdt, device=dev)
            bufs[f] = t
            setattr(res, f, C.cast(C.c_void_p(t.data_ptr() + GUARD * dt.itemsize), dict(_lib.MpctResult._fields_)[f]))
        torch.cuda.synchronize(dev)   # inputs and canaries resident before the call is enqueued
        keep = ins
        rc = sc.lib.mpct_eval_batch_device(sc.handle, Cn, *[C.c_void_p(t.data_ptr()) if t is not None else None for t in ins[:4]],
                                           nref, C.c_void_p(ins[4].data_ptr()),
                                           C.c_void_p(ins[5].data_ptr()) if ins[5] is not None else None,
                                           C.byref(o), C.byref(res), C.c_void_p(stream.cuda_stream))
        return Call(rc, sc, S, bufs, keep, stream)
    for f in fields:
        dt = dtype_of(f)
        a = np.full(S * width(sc, f) + 2 * GUARD, CANARY[dt], dtype=np.int32 if dt == np.int32 else np.int64)
        bufs[f] = a
        setattr(res, f, C.cast(C.c_void_p(a.ctypes.data + GUARD * dt.itemsize), dict(_lib.MpctResult._fields_)[f]))
    args = (Cn, N2.ctypes.data, Nu.ctypes.data, d.ctypes.data, l.ctypes.data, nref, refs.ctypes.data,
            vv.ctypes.data if vv is not None else None, C.byref(o), C.byref(res))
    if entry == "host":
        rc = sc.lib.mpct_eval_batch(sc.handle, *args)
    elif entry == "multi":
        devs = np.ascontiguousarray(devices, dtype=np.int32)
        rc = sc.lib.mpct_eval_batch_multi(sc.handle, len(devs), devs.ctypes.data_as(_lib.c_int32_p), *args)
    else:
        raise ValueError(entry)
    return Call(rc, sc, S, bufs, None, None)


def call(entry, sc, cands, refs, v=None, fields=COST, **kw):
    return launch(entry, sc, cands, refs, v, fields, **kw).finish()


def take(cands, idx):
    """The candidates idx of a pool (N2, Nu, delta, lambda)."""
    return tuple(np.ascontiguousarray(a[idx]) for a in cands)


def expect(pool_rows, idx, nref):
    """The rows [len(idx) * nref, w] of the batch `idx` from the pool call's rows [19 * nref, w]."""
    w = pool_rows.shape[1]
    return pool_rows.reshape(19, nref, w)[idx].reshape(len(idx) * nref, w)
