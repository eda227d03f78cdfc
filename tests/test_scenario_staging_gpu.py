"""GPU: the staging of the scenario-taking host-pointer entries -- mpct_eval_robust, mpct_eval_robust_tail,
mpct_eval_indices and mpct_eval_robust_indices (mpct_eval_batch: tests/test_result_records_gpu.py).  Each
entry is called once per result field with only that field asked for (plus the field it cannot go
without), once with every field and, where it has two result structs, once with the first struct NULL;
what comes back must equal, byte for byte and NaNs included, what the entry's _device twin wrote for the
same inputs with every field asked for (the twin is held to its references by the entry's own suite).
Every buffer the caller hands over, input or output, lies between 64 canary bytes, which must survive the
call, and the inputs must come back unchanged; a field that is not asked for is NULL.

Scenarios and candidates are tests/record_calls.py's: the 19-candidate pool (16 valid, 3 invalid) of
shell5 (the generic robust path: launch_batch, then the reduction) and of dtc (the fused dtc_robust
path), both with mpct_robust_instance pinned, at C = 19 with 3 draws and C = 1 with 1 draw; band and nmpc
at C = 19 with 3 draws and every field.  The index entries run with a trajectory budget of two candidates
a chunk (ten chunks, the last one ragged) and with the default budget.  The tail and statistics entries
take nlev = 2 unequal levels, the robust indices nsel = 3 fields: an output-row field, an integer field
and an input-row field (W = 2 my + nu).

The regrow tests make, on one scenario handle and a stream of their own, a small, a larger and the small
device call again without waiting in between, so that the context's event-guarded scratch grows while
work is pending; then the same with a host call after every device call.  Every result must equal the
bytes of the same call on a fresh scenario.

No field of any of the four entries differs bitwise between the host and the device entry."""
import contextlib
import ctypes as C

import numpy as np
import pytest

import record_calls as rc
from test_host_staging_gpu import CANARY, Guarded

pytestmark = pytest.mark.gpu
OK = 0
F8, I4, I8 = np.float64, np.int32, np.int64
LEVELS = np.array([0.5, 0.9])
SELECTED = ("iae", "settle", "tv")   # an output-row field, an integer field (per output row) and an input-row field
ENTRIES = ("mpct_eval_robust", "mpct_eval_robust_tail", "mpct_eval_indices", "mpct_eval_robust_indices")
ROBUST_INSTANCE = {"shell5": "gpc_small_kernel + robust_reduce_kernel",
                   "dtc": "dtc_robust_kernel<16> + dtc_robust_kernel<32>"}
LARGE, SMALL = (19, 3), (1, 1)
ONE_CANDIDATE = 5   # of the pool, a valid one


@pytest.fixture(scope="module")
def gpu(built, has_gpu):
    if not has_gpu:
        pytest.skip("no GPU")
    return True


_scen = {}


def scen(name):
    """The scenario, the routing of its robust calls pinned (a routing change must not silently empty a test)."""
    from mpct.engine import robust_instance

    if name not in _scen:
        q = rc.scenario(name)
        if name in ROBUST_INSTANCE:
            assert robust_instance(q["sc"]) == ROBUST_INSTANCE[name]
        _scen[name] = q
    return _scen[name]


def draws(q, nref):
    """nref reference sets: the scenario's own, or (band, nmpc: one set) that set scaled by 1, 0.9 and 1.1"""
    refs = q["refs"]
    if refs.shape[0] < nref:
        refs = np.concatenate([f * refs[:1] for f in (1.0, 0.9, 1.1)[:nref]])
    return refs[:nref]


@contextlib.contextmanager
def index_budget(nbytes):
    from mpct import _lib

    lib = _lib.load()
    assert lib.mpct_internal_index_budget(int(nbytes)) == OK
    try:
        yield
    finally:
        lib.mpct_internal_index_budget(0)


class Twin:
    """One entry on one scenario at one shape.  A result field is named "<struct>.<member>"; structs lists
    the entry's result structs in argument order: (name, ctypes class, [(member, dtype, count)])."""

    def __init__(self, entry, q, Cn, nref):
        from mpct import _lib
        from mpct.engine import _batch_args, _opts

        sc = self.sc = q["sc"]
        self.entry = entry
        cands = q["pool"] if Cn == 19 else rc.take(q["pool"], np.arange(ONE_CANDIDATE, ONE_CANDIDATE + Cn))
        v = None if q["v"] is None else q["v"][:nref] if q["v"].shape[0] >= nref else q["v"][:1]
        N2, Nu, d, l, refs, Cn, nref, vv = _batch_args(sc, *cands, draws(q, nref), v)
        self.Cn, self.nref = Cn, nref
        self.inputs = {"N2": N2, "Nu": Nu, "delta": d, "lambda": l, "r": refs, "v": vv}
        my, nu, S = sc.my, sc.nu, Cn * nref
        self.per = nref * (my + nu) * sc.nit * 8   # one candidate's trajectories: the index entries' chunk unit
        o = _opts(False, False, 0)
        params = _lib.MpctIndexParams(2, 0.02, 1e-3)
        lv, nlev = LEVELS.ctypes.data_as(_lib.c_double_p), len(LEVELS)
        ids = np.ascontiguousarray([[n for n, _, _ in _lib.INDEX_FIELDS].index(f) for f in SELECTED], dtype=np.int32)
        W = sum(my if per_y else nu for n, per_y, _ in _lib.INDEX_FIELDS if n in SELECTED)
        assert W == 2 * my + nu
        robust = [("mean", F8, Cn * my), ("worst", F8, Cn * my), ("n_failed", I4, Cn), ("worst_draw", I4, Cn),
                  ("status", I4, Cn)]
        cost = [("J1", F8, S * my), ("j21", F8, S * my), ("j22", F8, S * my), ("Jnu", F8, S * nu), ("status", I4, S),
                ("qp_iters", I8, S)]
        index = [(n, I4 if is_int else F8, S * (my if per_y else nu)) for n, per_y, is_int in _lib.INDEX_FIELDS]
        stats = [(n, I4 if is_int else F8, Cn * W * (nlev if per_level else 1)) for n, is_int, per_level in _lib.STATS_FIELDS]
        tail = [("quantile", F8, Cn * nlev), ("cvar", F8, Cn * nlev), ("q_draw", I4, Cn * nlev)]
        self.requires, self.chunked = {}, False
        if entry == "mpct_eval_robust":
            self.mid = (0.0, C.byref(o))
            self.structs = [("out", _lib.MpctRobustResult, robust + [("J1", F8, S * my)])]
        elif entry == "mpct_eval_robust_tail":
            self.mid = (0.0, C.byref(o), nlev, lv)
            self.structs = [("out", _lib.MpctRobustResult, robust + [("J1", F8, S * my)]), ("tail", _lib.MpctRobustTail, tail)]
        elif entry == "mpct_eval_indices":
            self.mid = (C.byref(o), C.byref(params))
            self.structs = [("res", _lib.MpctResult, cost), ("out", _lib.MpctIndexResult, index)]
            self.requires = {"res." + m: ("out.iae",) for m, _, _ in cost}   # out needs a field of its own
            self.chunked = True
        elif entry == "mpct_eval_robust_indices":   # base->J1 must be NULL
            self.mid = (0.0, C.byref(o), C.byref(params), len(ids), ids.ctypes.data_as(_lib.c_int32_p), nlev, lv)
            self.structs = [("base", _lib.MpctRobustResult, robust), ("out", _lib.MpctDrawStats, stats)]
            self.chunked = True
        else:
            raise ValueError(entry)
        self.keep = (o, params, ids)
        self.fields = {s + "." + m: (k, m, np.dtype(dt).itemsize * n)
                       for k, (s, _, fl) in enumerate(self.structs) for m, dt, n in fl}
        self._want = {}

    def all_fields(self):
        return tuple(self.fields)

    def of_struct(self, k):
        return tuple(f for f, (j, _, _) in self.fields.items() if j == k)

    def subsets(self):
        """(fields asked for, first struct NULL?): every single field, all of them, the second struct alone"""
        one = [(tuple(dict.fromkeys((f,) + self.requires.get(f, ()))), False) for f in self.fields]
        return one + [(self.all_fields(), False)] + ([(self.of_struct(1), True)] if len(self.structs) == 2 else [])

    def _args(self, ptr, addr_of, null_first, tail=()):
        structs = []
        for k, (_, cls, _) in enumerate(self.structs):
            types = dict(cls._fields_)
            structs.append(None if k == 0 and null_first else
                           cls(**{m: C.cast(C.c_void_p(addr_of[f]), types[m]) for f, (j, m, _) in self.fields.items()
                                  if j == k and f in addr_of}))
        assert not null_first or not set(addr_of) & set(self.of_struct(0))
        args = (self.sc.handle, self.Cn, ptr("N2"), ptr("Nu"), ptr("delta"), ptr("lambda"), self.nref, ptr("r"), ptr("v"))
        return args + self.mid + tuple(None if s is None else C.byref(s) for s in structs) + tuple(tail), structs

    def device_buffers(self, subset):
        """the inputs on the device and a canary-filled buffer per field of `subset`, resident on return"""
        import torch

        dev = torch.device("cuda", 0)
        tin = {k: torch.tensor(v, device=dev) for k, v in self.inputs.items() if v is not None}
        tout = {f: torch.full((self.fields[f][2],), CANARY, dtype=torch.uint8, device=dev) for f in subset}
        torch.cuda.synchronize(dev)
        return tin, tout

    def device_launch(self, bufs, stream):
        """enqueue the _device entry on `stream`, asking for the fields `bufs` has buffers for; not synchronised"""
        from mpct import _lib

        tin, tout = bufs
        args, _ = self._args(lambda k: C.c_void_p(tin[k].data_ptr()) if k in tin else None,
                             {f: t.data_ptr() for f, t in tout.items()}, False, (C.c_void_p(stream.cuda_stream),))
        rcode = getattr(self.sc.lib, self.entry + "_device")(*args)
        assert rcode == OK, _lib.last_error()

    @staticmethod
    def device_bytes(bufs):
        return {f: t.cpu().numpy().tobytes() for f, t in bufs[1].items()}

    def device_call(self, subset, stream):
        """field -> the bytes the _device entry writes when asked for `subset`"""
        bufs = self.device_buffers(subset)
        self.device_launch(bufs, stream)
        stream.synchronize()
        return self.device_bytes(bufs)

    def want(self, budget=0):
        """field -> the bytes the _device entry writes with every field asked for; computed once per budget"""
        if budget not in self._want:
            import torch

            with index_budget(budget):
                self._want[budget] = self.device_call(self.all_fields(), torch.cuda.current_stream(torch.device("cuda", 0)))
        return self._want[budget]

    def host_call(self, subset, null_first=False):
        """the host entry asking for `subset` only; returns (rc, field -> Guarded, input -> Guarded)"""
        gin = {k: Guarded(v.nbytes, v) for k, v in self.inputs.items() if v is not None}
        gout = {f: Guarded(self.fields[f][2]) for f in subset}
        args, structs = self._args(lambda k: gin[k].addr if k in gin else None, {f: g.addr for f, g in gout.items()}, null_first)
        return getattr(self.sc.lib, self.entry)(*args), gout, gin

    def check_host(self, subset, null_first, want, note=""):
        from mpct import _lib

        what = "%s asking for %s%s%s" % (self.entry, ", ".join(subset), " (first struct NULL)" if null_first else "", note)
        rcode, gout, gin = self.host_call(subset, null_first)
        assert rcode == OK, what + ": " + _lib.last_error()
        for k, g in gin.items():
            assert g.untouched(), what + ": the input %s or its canaries changed" % k
        for f, g in gout.items():
            assert g.canaries_intact(), what + ": wrote outside %s" % f
            assert g.payload() == want[f], what + ": %s differs from the device entry's" % f

    def check(self, subsets):
        # the index entries: two candidates a chunk (C = 19: ten chunks, the last of one candidate), then the default
        for budget in ((2 * self.per, 0) if self.chunked else (0,)):
            want = self.want(budget)
            with index_budget(budget):
                for subset, null_first in subsets:
                    self.check_host(subset, null_first, want, ", budget %d" % budget)


_twins = {}


def twin(entry, name, shape):
    """the twin and, with it, its device references: made once and shared"""
    key = (entry, name, shape)
    if key not in _twins:
        _twins[key] = Twin(entry, scen(name), *shape)
    return _twins[key]


@pytest.mark.parametrize("shape", [LARGE, SMALL], ids=["C19x3", "C1x1"])
@pytest.mark.parametrize("name", ["shell5", "dtc"])
@pytest.mark.parametrize("entry", ENTRIES)
def test_field_subsets(gpu, entry, name, shape):
    t = twin(entry, name, shape)
    assert (t.Cn, t.nref) == shape
    t.check(t.subsets())


@pytest.mark.parametrize("name", ["band", "nmpc"])
@pytest.mark.parametrize("entry", ENTRIES)
def test_band_and_nmpc_all_fields(gpu, entry, name):
    t = twin(entry, name, LARGE)
    assert (t.Cn, t.nref) == LARGE
    t.check([(t.all_fields(), False)])


# ---- the event-guarded scratch of a context: the robust one (per-simulation J1 and status of the generic
# path; candidate lists and the tail's J1 sample of the fused one) and the index one (a chunk's trajectories)
@pytest.mark.parametrize("entry,name", [("mpct_eval_robust", "shell5"), ("mpct_eval_robust_tail", "dtc"),
                                        ("mpct_eval_indices", "shell5"), ("mpct_eval_robust_indices", "shell5")])
def test_scratch_regrow(gpu, entry, name):
    import torch

    scen(name)   # the routing is pinned
    stream = torch.cuda.Stream(torch.device("cuda", 0))

    def asked(t):   # without the caller's J1 the sample of a robust call lives in the scratch
        return tuple(f for f in t.all_fields() if f != "out.J1")

    ref = {}
    for shape in (SMALL, LARGE):   # each on a scenario of its own
        t = Twin(entry, rc.scenario(name), *shape)
        ref[shape] = t.device_call(asked(t), stream)
    for with_host in (False, True):
        q = rc.scenario(name)   # a fresh handle: its scratch starts empty, grows at the second call and stays
        twins = {shape: Twin(entry, q, *shape) for shape in (SMALL, LARGE)}
        calls = [(shape, twins[shape].device_buffers(asked(twins[shape]))) for shape in (SMALL, LARGE, SMALL)]
        for shape, bufs in calls:   # nothing waits for the stream between the device calls
            t = twins[shape]
            t.device_launch(bufs, stream)
            if with_host:
                t.check_host(asked(t), False, ref[shape], ", after the device call of C = %d" % shape[0])
        stream.synchronize()
        for k, (shape, bufs) in enumerate(calls):
            got = Twin.device_bytes(bufs)
            for f in got:
                assert got[f] == ref[shape][f], "%s: %s of device call %d (C = %d, host calls %s) differs from a fresh scenario's" % (
                    entry, f, k, shape[0], "between" if with_host else "none")
