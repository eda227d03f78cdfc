"""GPU: the staging of the six scenario-free host-pointer entries -- mpct_pareto, mpct_hypervolume,
mpct_hv_select, mpct_hypervolume_exact, mpct_indices and mpct_draw_stats.  Each entry is called once per
result field with only that field asked for (plus the field it cannot go without) and once with every
field; what comes back must equal, byte for byte, what the entry's _device twin wrote for the same
inputs (the twin is held to the numpy references by the entry's own suite).  Every buffer the caller
hands over, input or output, lies between 64 canary bytes, which must survive the call; a field that is
not asked for is NULL.  The shapes are small and keep every width apart: my != nu, int32 fields between
float64 ones, a member list shorter than the table."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
PAD, CANARY = 64, 0xA5
OK, EINVAL = 0, -1


@pytest.fixture(scope="module")
def gpu(built, has_gpu):
    if not has_gpu:
        pytest.skip("no GPU")
    return True


class Guarded:
    """nbytes of caller memory between two canaries; the payload starts as canary bytes too, or as `init`"""

    def __init__(self, nbytes, init=None):
        self.raw = np.full(PAD + nbytes + PAD, CANARY, dtype=np.uint8)
        self.n = nbytes
        if init is not None:
            self.raw[PAD:PAD + nbytes] = np.ascontiguousarray(init).view(np.uint8).ravel()
        self.before = self.raw.copy()

    @property
    def addr(self):
        return self.raw.ctypes.data + PAD

    def payload(self):
        return self.raw[PAD:PAD + self.n].tobytes()

    def canaries_intact(self):
        return bool((self.raw[:PAD] == CANARY).all() and (self.raw[PAD + self.n:] == CANARY).all())

    def untouched(self):
        return bool((self.raw == self.before).all())


class Case:
    """One entry at one shape.  inputs: name -> array or None (NULL) in any order; args(ptr): the entry's
    arguments up to the device ordinal / result struct, with ptr(name) the address of an input; fields:
    (name, dtype, count) of the result struct's members this shape can ask for; requires: the members a
    member cannot be asked for without; needs(subset): the inputs a call for `subset` has to pass."""

    def __init__(self, entry, struct, inputs, args, fields, requires=None, needs=None, extra_subsets=()):
        self.entry, self.struct, self.inputs, self.args, self.fields = entry, struct, inputs, args, fields
        self.requires = requires or {}
        self.needs = needs or (lambda subset: set(inputs))
        self.extra_subsets = list(extra_subsets)
        self._want = None

    def nbytes(self, f):
        return next(np.dtype(dt).itemsize * n for name, dt, n in self.fields if name == f)

    def result(self, addr_of):
        """the result struct with the member f at addr_of[f], NULL where addr_of has none"""
        types = dict(self.struct._fields_)
        return self.struct(**{f: C.cast(C.c_void_p(a), types[f]) for f, a in addr_of.items()})

    def subsets(self):
        names = [f for f, _, _ in self.fields]
        one = [tuple(dict.fromkeys((f,) + tuple(self.requires.get(f, ())))) for f in names]
        return one + self.extra_subsets + [tuple(names)]

    def want(self):
        """field -> the bytes the _device entry writes with every field asked for; computed once"""
        if self._want is None:
            import torch
            from mpct import _lib

            dev = torch.device("cuda", 0)
            tin = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in self.inputs.items() if v is not None}
            tout = {f: torch.full((max(self.nbytes(f), 1),), CANARY, dtype=torch.uint8, device=dev) for f, _, _ in self.fields}
            res = self.result({f: t.data_ptr() for f, t in tout.items()})
            args = self.args(lambda k: tin[k].data_ptr() if k in tin else None)
            st = torch.cuda.current_stream(dev).cuda_stream
            rc = getattr(_lib.load(), self.entry + "_device")(*args, C.byref(res), C.c_void_p(st))
            assert rc == OK, _lib.last_error()
            torch.cuda.synchronize(dev)
            self._want = {f: t.cpu().numpy()[:self.nbytes(f)].tobytes() for f, t in tout.items()}
        return self._want

    def host_call(self, subset, device=0):
        """the host entry asking for `subset` only; returns (rc, field -> Guarded, input -> Guarded)"""
        from mpct import _lib

        passed = self.needs(subset)
        gin = {k: Guarded(v.nbytes, v) for k, v in self.inputs.items() if v is not None and k in passed}
        gout = {f: Guarded(self.nbytes(f)) for f in subset}
        res = self.result({f: g.addr for f, g in gout.items()})
        args = self.args(lambda k: gin[k].addr if k in gin else None)
        rc = getattr(_lib.load(), self.entry)(*args, device, C.byref(res))
        return rc, gout, gin

    def check(self, device=0):
        from mpct import _lib

        want = self.want()
        for subset in self.subsets():
            what = "%s asking for %s" % (self.entry, ", ".join(subset))
            rc, gout, gin = self.host_call(subset, device)
            assert rc == OK, what + ": " + _lib.last_error()
            for k, g in gin.items():
                assert g.untouched(), what + ": the input %s or its canaries changed" % k
            for f, g in gout.items():
                assert g.canaries_intact(), what + ": wrote outside %s" % f
                assert g.payload() == want[f], what + ": %s differs from the device entry's" % f


# ---- the cases -----------------------------------------------------------------------------------
def _costs(Cn, k, seed):
    rng = np.random.default_rng(seed)
    return np.round(rng.random((Cn, k)) * 8.0) / 8.0  # a coarse grid: ties, duplicates and dominated rows


def pareto_case(max_layers, Cn=37, k=3):
    from mpct import _lib

    A = _costs(Cn, k, 11)
    fields = [("dom_count", np.int32, Cn), ("layer", np.int32, Cn), ("front", np.int32, Cn), ("n_front", np.int32, 1)]
    if max_layers == 0:
        fields = [f for f in fields if f[0] != "layer"]
    return Case("mpct_pareto", _lib.MpctParetoResult, {"costs": A},
                lambda p: (p("costs"), Cn, k, max_layers), fields, requires={"front": ("n_front",)})


def _hv_inputs(with_members, Cn=40, k=3, M=25):
    A = _costs(Cn, k, 12)
    members = None
    if with_members:
        members = np.random.default_rng(13).permutation(Cn)[:M].astype(np.int32)
        members[7] = -1
    else:
        M = Cn
    lo, ref = np.full(k, -0.125), np.array([1.0, 1.125, 1.25])
    return {"costs": A, "members": members, "lo": lo, "ref": ref}, Cn, k, M


N_SAMPLES, SEED, N_PICK = 256, 0x1234ABCD5678EF01, 5


def hv_case(with_members):
    from mpct import _lib

    inputs, Cn, k, M = _hv_inputs(with_members)
    fields = [("n_covered", np.int64, 1), ("excl", np.int64, M), ("depth_hist", np.int64, _lib.HV_BINS), ("hv", np.float64, 1)]
    return Case("mpct_hypervolume", _lib.MpctHvResult, inputs,
                lambda p: (p("costs"), Cn, k, p("members"), M, p("lo"), p("ref"), N_SAMPLES, SEED), fields)


def hvsel_case(with_members):
    from mpct import _lib

    inputs, Cn, k, M = _hv_inputs(with_members)
    K = N_PICK
    fields = [("n_picked", np.int64, 1), ("pos", np.int32, K), ("index", np.int32, K), ("gain", np.int64, K),
              ("covered", np.int64, K), ("hv", np.float64, K), ("ties", np.int32, K), ("n_covered_all", np.int64, 1)]
    return Case("mpct_hv_select", _lib.MpctHvSelectResult, inputs,
                lambda p: (p("costs"), Cn, k, p("members"), M, p("lo"), p("ref"), N_SAMPLES, SEED, K), fields)


def hvx_case(with_members):
    from mpct import _lib

    inputs, Cn, k, M = _hv_inputs(with_members)
    fields = [("hv", np.float64, 1), ("excl", np.float64, M), ("n_active", np.int64, 1)]
    return Case("mpct_hypervolume_exact", _lib.MpctHvxResult, inputs,
                lambda p: (p("costs"), Cn, k, p("members"), M, p("lo"), p("ref")), fields)


def index_case(S=6, nref=2, my=2, nu=3, nit=17):
    from mpct import _lib

    rng = np.random.default_rng(14)
    r = np.repeat(rng.random((nref, my, 1)) + 0.5, nit, axis=2)
    y = r[np.arange(S) % nref] * (1.0 - np.exp(-np.arange(nit) / 3.0)) + 0.01 * rng.standard_normal((S, my, nit))
    u = rng.standard_normal((S, nu, nit)).cumsum(axis=2)
    params = _lib.MpctIndexParams(2, 0.02, 1e-3)
    fields = [(n, np.int32 if is_int else np.float64, S * (my if per_y else nu)) for n, per_y, is_int in _lib.INDEX_FIELDS]
    of_y = tuple(n for n, per_y, _ in _lib.INDEX_FIELDS if per_y)
    of_u = tuple(n for n, per_y, _ in _lib.INDEX_FIELDS if not per_y)

    def needs(subset):  # y and r only behind an output-row field, u only behind an input-row field
        return ({"y", "r"} if set(subset) & set(of_y) else set()) | ({"u"} if set(subset) & set(of_u) else set())

    return Case("mpct_indices", _lib.MpctIndexResult, {"y": y, "u": u, "r": r},
                lambda p: (p("y"), p("u"), p("r"), S, nref, my, nu, nit, C.byref(params)), fields, needs=needs,
                extra_subsets=[of_u, of_y])


def stats_case(x_type, with_alive, Cn=5, D=7, m=3, nlev=2):
    from mpct import _lib

    rng = np.random.default_rng(15)
    if x_type == _lib.STAT_I32:
        x = rng.integers(-1, 20, size=(Cn, D, m)).astype(np.int32)  # -1: no value
    else:
        x = rng.standard_normal((Cn, D, m))
        x[1, 2, 0] = np.nan  # a draw that drops out of one column
    alive = None
    if with_alive:
        alive = (rng.random((Cn, D)) < 0.7).astype(np.int32)
        alive[3] = 0  # a candidate with no survivor
    levels = np.array([0.5, 0.9])
    fields = [(n, np.int32 if is_int else np.float64, Cn * m * (nlev if per_level else 1))
              for n, is_int, per_level in _lib.STATS_FIELDS]
    return Case("mpct_draw_stats", _lib.MpctDrawStats, {"x": x, "alive": alive},
                lambda p: (p("x"), x_type, p("alive"), Cn, D, m, nlev, levels.ctypes.data_as(_lib.c_double_p)), fields)


CASES = {
    "pareto": lambda: pareto_case(4),
    "pareto-no-layers": lambda: pareto_case(0),
    "hypervolume-members": lambda: hv_case(True),
    "hypervolume-all": lambda: hv_case(False),
    "hv_select-members": lambda: hvsel_case(True),
    "hv_select-all": lambda: hvsel_case(False),
    "hypervolume_exact-members": lambda: hvx_case(True),
    "hypervolume_exact-all": lambda: hvx_case(False),
    "indices": index_case,
    "draw_stats-f64-alive": lambda: stats_case(0, True),
    "draw_stats-f64": lambda: stats_case(0, False),
    "draw_stats-i32-alive": lambda: stats_case(1, True),
    "draw_stats-i32": lambda: stats_case(1, False),
}
ONE_PER_ENTRY = ["pareto", "hypervolume-members", "hv_select-members", "hypervolume_exact-members", "indices",
                 "draw_stats-i32-alive"]
_made = {}


def case(name):
    """the case and, with it, its device reference: made once and shared"""
    if name not in _made:
        _made[name] = CASES[name]()
    return _made[name]


@pytest.mark.parametrize("name", list(CASES))
def test_field_subsets(gpu, name):
    case(name).check()


# ---- the empty calls: MPCT_OK, the documented fills, nothing else written --------------------------
def _empty_call(entry, struct, args, fields):
    """call with every field asked for, each buffer `count` elements long; returns name -> (array, Guarded)"""
    from mpct import _lib

    c = Case(entry, struct, {}, lambda p: args, fields)
    rc, gout, _ = c.host_call(tuple(f for f, _, _ in fields))
    assert rc == OK, _lib.last_error()
    assert all(g.canaries_intact() for g in gout.values())
    return {f: (np.frombuffer(gout[f].payload(), dtype=dt), gout[f]) for f, dt, _ in fields}


def test_empty_calls(gpu):
    from mpct import _lib

    keep = Guarded(64, np.arange(8, dtype=np.float64))  # non-NULL inputs that nothing may read past or write
    p = keep.addr
    # C == 0: n_front[0] = 0, nothing else
    got = _empty_call("mpct_pareto", _lib.MpctParetoResult, (p, 0, 3, 4),
                      [("dom_count", np.int32, 4), ("layer", np.int32, 4), ("front", np.int32, 4), ("n_front", np.int32, 1)])
    assert got["n_front"][0][0] == 0
    assert all(got[f][1].untouched() for f in ("dom_count", "layer", "front"))
    # M == 0 with a table of 2 rows: every count 0, depth_hist[0] = N, hv from n_covered = 0
    hv_args = (p, 2, 3, p, 0, p, p + 24)  # costs, C, k, members, M, lo = (0, 1, 2), ref = (3, 4, 5)
    got = _empty_call("mpct_hypervolume", _lib.MpctHvResult, hv_args + (N_SAMPLES, SEED),
                      [("n_covered", np.int64, 1), ("excl", np.int64, 4), ("depth_hist", np.int64, _lib.HV_BINS), ("hv", np.float64, 1)])
    assert got["n_covered"][0][0] == 0 and got["hv"][0].tobytes() == np.float64(0.0).tobytes()
    assert got["depth_hist"][0].tolist() == [N_SAMPLES] + [0] * (_lib.HV_BINS - 1)
    assert got["excl"][1].untouched()
    K = N_PICK
    got = _empty_call("mpct_hv_select", _lib.MpctHvSelectResult, hv_args + (N_SAMPLES, SEED, K),
                      [("n_picked", np.int64, 1), ("pos", np.int32, K), ("index", np.int32, K), ("gain", np.int64, K),
                       ("covered", np.int64, K), ("hv", np.float64, K), ("ties", np.int32, K), ("n_covered_all", np.int64, 1)])
    assert got["n_picked"][0][0] == 0 and got["n_covered_all"][0][0] == 0
    assert got["pos"][0].tolist() == [-1] * K and got["index"][0].tolist() == [-1] * K
    assert got["gain"][0].tolist() == [0] * K and got["covered"][0].tolist() == [0] * K and got["ties"][0].tolist() == [0] * K
    assert got["hv"][0].tobytes() == np.zeros(K).tobytes()
    got = _empty_call("mpct_hypervolume_exact", _lib.MpctHvxResult, hv_args,
                      [("hv", np.float64, 1), ("excl", np.float64, 4), ("n_active", np.int64, 1)])
    assert got["hv"][0].tobytes() == np.float64(0.0).tobytes() and got["n_active"][0][0] == 0
    assert got["excl"][1].untouched()
    # S == 0 and C == 0 write nothing
    params = _lib.MpctIndexParams(2, 0.02, 1e-3)
    got = _empty_call("mpct_indices", _lib.MpctIndexResult, (p, p, p, 0, 2, 2, 3, 17, C.byref(params)),
                      [(n, np.int32 if is_int else np.float64, 4) for n, _, is_int in _lib.INDEX_FIELDS])
    assert all(g.untouched() for _, g in got.values())
    levels = np.array([0.5, 0.9])
    got = _empty_call("mpct_draw_stats", _lib.MpctDrawStats,
                      (p, _lib.STAT_F64, p, 0, 7, 3, 2, levels.ctypes.data_as(_lib.c_double_p)),
                      [(n, np.int32 if is_int else np.float64, 4) for n, is_int, _ in _lib.STATS_FIELDS])
    assert all(g.untouched() for _, g in got.values())
    assert keep.untouched()


# ---- the device ordinal ----------------------------------------------------------------------------
@pytest.mark.parametrize("name", ONE_PER_ENTRY)
def test_ordinal_out_of_range(gpu, name):
    import torch
    from mpct import _lib

    c = case(name)
    cur = torch.cuda.current_device()
    rc, gout, gin = c.host_call(tuple(f for f, _, _ in c.fields), device=torch.cuda.device_count())
    assert rc == EINVAL and "device ordinal out of range" in _lib.last_error()
    assert torch.cuda.current_device() == cur
    assert all(g.untouched() for g in list(gout.values()) + list(gin.values()))


@pytest.mark.parametrize("name", ONE_PER_ENTRY)
def test_other_device_leaves_the_current_one(gpu, name):
    """device = 1 while device 0 is current: the same bytes (the reference ran on device 0), device 0 still current"""
    import torch

    if torch.cuda.device_count() < 2:
        pytest.skip("one device visible")
    torch.cuda.set_device(0)
    case(name).check(device=1)
    assert torch.cuda.current_device() == 0
