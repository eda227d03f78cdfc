"""Python host mirror of the reference's closed-loop seam, over the libmpct C ABI.

  Scenario            mpct_scenario_create: plant/model/CARIMA tables + bounds + Yref
  eval_batch          mpct_eval_batch (host arrays): C candidates x nref reference sets
  eval_batch_device   mpct_eval_batch_device (torch CUDA tensors, enqueued on a stream)
  closedloop_toolbox  drop-in for closedloop_toolbox.m:1 (one candidate, full trajectories)
  pareto              mpct_pareto: front, domination counts and layers of a [C, k] cost table
  pareto_device       mpct_pareto_device (torch CUDA tensors, enqueued on the current stream)
  goal_attain         mpct_goal_attain: per goal / weight vector, the candidates that minimise the attainment factor
  goal_attain_device  mpct_goal_attain_device (torch CUDA tensors, enqueued on the current stream)
  hypervolume         mpct_hypervolume: Monte-Carlo hypervolume of a front in a box, per-member contributions
  hypervolume_device  mpct_hypervolume_device (torch CUDA tensors, enqueued on the current stream)
  hv_select           mpct_hv_select: the n members that carry a front, by greedy selection on the coverage count
  hv_select_device    mpct_hv_select_device (torch CUDA tensors, enqueued on the current stream)
  indices             mpct_indices: performance indices (IAE, overshoot, settling, valve travel ..) of trajectories
  indices_device      mpct_indices_device (torch CUDA tensors, enqueued on the current stream)
  eval_indices        mpct_eval_indices: score a batch and return only its index records
  eval_indices_device mpct_eval_indices_device (torch CUDA tensors, enqueued on a stream)
  draw_stats          mpct_draw_stats: per-column statistics of a [C, D, m] table over its draw axis
  draw_stats_device   mpct_draw_stats_device (torch CUDA tensors, enqueued on the current stream)
  eval_robust_indices mpct_eval_robust_indices: per-candidate statistics of the indices over the plant draws
  eval_robust_indices_device  mpct_eval_robust_indices_device (torch CUDA tensors, enqueued on a stream)
  limit_indices       mpct_limit_indices: band violation, saturation and rate-limit use of stored trajectories
  limit_indices_device  mpct_limit_indices_device (torch CUDA tensors, enqueued on the current stream)
  eval_limit_indices  mpct_eval_limit_indices: score a batch and return only its limit records
  eval_limit_indices_device  mpct_eval_limit_indices_device (torch CUDA tensors, enqueued on a stream)
  eval_robust_limit_indices  mpct_eval_robust_limit_indices: their statistics over the plant draws
  eval_robust_limit_indices_device  mpct_eval_robust_limit_indices_device (torch CUDA tensors, enqueued on a stream)
  reference_segments  mpct_reference_segments: the segment boundaries of a reference (host only)
  segment_indices     mpct_segment_indices: step-response indices per setpoint segment of stored trajectories
  segment_indices_device  mpct_segment_indices_device (torch CUDA tensors, enqueued on the current stream)
  eval_segment_indices  mpct_eval_segment_indices: score a batch and return only its segment records
  eval_segment_indices_device  mpct_eval_segment_indices_device (torch CUDA tensors, enqueued on a stream)
  eval_robust_segment_indices  mpct_eval_robust_segment_indices: their statistics over the plant draws
  eval_robust_segment_indices_device  mpct_eval_robust_segment_indices_device (torch CUDA tensors, enqueued on a stream)
  envelope            mpct_envelope: per-sample statistics of stored trajectories over the draws, and the band's spread
  envelope_device     mpct_envelope_device (torch CUDA tensors, enqueued on the current stream)
  eval_robust_envelope  mpct_eval_robust_envelope: score C x D closed loops and return their envelopes
  eval_robust_envelope_device  mpct_eval_robust_envelope_device (torch CUDA tensors, enqueued on a stream)

No CPU fallback: every numerical result comes from the HIP kernel.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass, field

import numpy as np

from . import _lib
from .lti import Tf, carima, descomp


def _dp(a):
    return a.ctypes.data_as(_lib.c_double_p)


def _ip(a):
    return a.ctypes.data_as(_lib.c_int32_p)


def _tptr(t, ty):
    """Device pointer of a torch tensor (None stays NULL)."""
    return C.cast(C.c_void_p(t.data_ptr()), ty) if t is not None else None


def _dtf_array(keep, entries):
    """mpct_dtf array of ``entries``: Tf's in any nesting of lists (a filter list, a my x nin grid, a
    list of such grids), flattened row-major.  The array and its coefficient buffers go into ``keep``."""
    flat = []

    def walk(e):
        if isinstance(e, Tf):
            flat.append(e)
        else:
            for x in e:
                walk(x)

    walk(entries)
    arr = (_lib.MpctDtf * len(flat))()
    for k, t in enumerate(flat):
        num = np.ascontiguousarray(t.num, dtype=float)
        den = np.ascontiguousarray(t.den, dtype=float)
        keep.extend([num, den])
        arr[k] = _lib.MpctDtf(len(num), _dp(num), _dp(den), int(t.delay))
    keep.append(arr)
    return arr


class MpctError(RuntimeError):
    pass


ESTIMATORS = {"output_bias": _lib.EST_OUTPUT_BIAS}   # Scenario(estimator=...) -> mpct_scenario_create_est's id


class Scenario:
    """Candidate-independent description of one tuning problem (MPCTuning's Par minus N/Nu/
    delta/lambda).  ``plant``/``model`` are my x (nu+nd) lists of :class:`Tf` (scaled, discrete:
    MPCTuning.m:162 Pze = L*Pz*R).  ``window``: 'toolbox' predicts t+1..t+N2 (PredictionHorizon
    semantics, closedloop_toolbox.m:38), 'gpc' predicts t+dmin+1..t+dmin+N2 (MatG.m / DTC_GPC_WW).
    ``exact_carima``: exact LCM (toolbox-equivalent) vs BA_MIMO's rounded roots.
    ``bands``: the toolbox MPC with measured disturbances and soft output bands (Shell7x5.m,
    WoodBerry.m; ABI mdband): dict(y_min, y_max, ecr_min, ecr_max, y_scale=None, u_scale=None,
    rho=1e4) of OV Min/Max, MinECR/MaxECR, ScaleFactors and Weights.ECR.  Scenarios with measured
    disturbances (nd > 0) always use that kernel (unbounded outputs when bands is None).
    ``host_carima``: False passes no CARIMA tables and lets the library derive them from the model
    (exact LCM, what the MATLAB MEX host does; toolbox window only).
    ``estimator``: None, or "output_bias" (band kernel only, mpct_scenario_create_est with
    MPCT_EST_OUTPUT_BIAS): ``plant`` and ``plant_variants`` may differ from ``model``; the controller
    corrects its prediction by the output bias b(t) = y(t) - y_model(t).  Closed loop
    only: ``open_loop=True`` on such a scenario raises."""

    def __init__(self, plant, model, nu, du_min, du_max, u_min, u_max, yref, n2_max, nu_max,
                 Ts=1.0, window="toolbox", weights_squared=True, exact_carima=True, vns_ink=10,
                 dtc=False, filters=None, dist=None, plant_variants=None, bands=None, host_carima=True, estimator=None):
        self.lib = _lib.load()
        self.plant, self.model = plant, model
        self.my, self.nin = len(model), len(model[0])
        self.nu = int(nu)
        self.nd = self.nin - self.nu
        self.yref = np.ascontiguousarray(np.asarray(yref, dtype=float).reshape(self.my, -1))
        self.nit = self.yref.shape[1]
        self.n2_max, self.nu_max, self.Ts = int(n2_max), int(nu_max), float(Ts)
        self.window, self.weights_squared, self.vns_ink = window, bool(weights_squared), int(vns_ink)
        Bn, An, dp = descomp(model)
        B, A, na, nb = carima(Bn, An, exact=exact_carima)
        self.dp, self.na, self.nb = dp, na, nb
        self.dmin = dp[:, : self.nu].min(axis=1)
        n1 = np.ones(self.my, dtype=np.int32) if window == "toolbox" else (self.dmin + 1).astype(np.int32)
        # DTC-GPC (DTC_GPC_WW.m): GPC window, deltaUFree on the delays net of dmin (dnz)
        self.dtc = bool(dtc)
        self.nq = len(dist[0]) if dist else 0
        self.dist, self.filters = dist, filters
        if self.dtc and window != "gpc":
            raise ValueError("DTC mode uses the GPC window (MatG/diophantine N1 = dmin+1)")
        dp_desc = (dp - self.dmin[:, None]) if self.dtc else dp
        keep = []  # keep every buffer alive for the descriptor's lifetime

        A_cat = np.ascontiguousarray(np.concatenate([np.asarray(a, dtype=float) / a[0] for a in A]))
        B_cat = np.ascontiguousarray(np.concatenate(
            [np.asarray(B[i][j], dtype=float) / A[i][0] for i in range(self.my) for j in range(self.nin)]))
        na32 = np.ascontiguousarray(na, dtype=np.int32)
        nb32 = np.ascontiguousarray(nb.ravel(), dtype=np.int32)
        dp32 = np.ascontiguousarray(dp_desc.ravel(), dtype=np.int32)
        bnds = [np.ascontiguousarray(np.broadcast_to(np.asarray(b, dtype=float), (self.nu,)))
                for b in (du_min, du_max, u_min, u_max)]
        self.bounds = bnds
        keep += [A_cat, B_cat, na32, nb32, dp32, n1, self.yref] + bnds
        d = _lib.MpctScenarioDesc()
        d.abi_version = _lib.ABI_VERSION
        d.my, d.nu, d.nd, d.nit = self.my, self.nu, self.nd, self.nit
        d.n2_max, d.nu_max = self.n2_max, self.nu_max
        d.weights_squared = int(self.weights_squared)
        d.vns_ink = self.vns_ink
        d.n1 = _ip(n1)
        d.plant = _dtf_array(keep, plant)
        d.model = _dtf_array(keep, model)
        if host_carima or self.dtc or not exact_carima:
            d.na, d.carima_A, d.nb, d.carima_B, d.dp = _ip(na32), _dp(A_cat), _ip(nb32), _dp(B_cat), _ip(dp32)
        d.du_min, d.du_max, d.u_min, d.u_max = (_dp(b) for b in bnds)
        d.yref = _dp(self.yref)
        d.dtc = int(self.dtc)
        d.nq = self.nq
        if filters is not None:
            d.filter = _dtf_array(keep, filters)
        if self.nq:
            d.dist = _dtf_array(keep, dist)
        self.nplant = len(plant_variants) if plant_variants else 1
        if self.nplant > 1:
            d.nplant = self.nplant
            d.plant_var = _dtf_array(keep, plant_variants)
        self.mdband = bands is not None or self.nd > 0
        if self.mdband:
            if window != "toolbox" or self.dtc:
                raise ValueError("the MD / output-band kernel predicts over the toolbox window (no DTC)")
            b = dict(bands or {})
            inf = np.full(self.my, np.inf)

            def vec(key, default, n):
                v = b.get(key)
                return np.ascontiguousarray(np.broadcast_to(np.asarray(default if v is None else v, dtype=float), (n,)))

            self.bands = {k: vec(k, dflt, n) for k, dflt, n in (
                ("y_min", -inf, self.my), ("y_max", inf, self.my), ("ecr_min", 1.0, self.my),
                ("ecr_max", 1.0, self.my), ("y_scale", 1.0, self.my), ("u_scale", 1.0, self.nu))}
            self.rho = float(b.get("rho", 1e4))
            keep.extend(self.bands.values())
            d.mdband = 1
            d.y_min, d.y_max = _dp(self.bands["y_min"]), _dp(self.bands["y_max"])
            d.ecr_min, d.ecr_max = _dp(self.bands["ecr_min"]), _dp(self.bands["ecr_max"])
            d.y_scale, d.u_scale = _dp(self.bands["y_scale"]), _dp(self.bands["u_scale"])
            d.rho_ecr = self.rho
        h = C.c_void_p()
        if estimator is not None and estimator not in ESTIMATORS:
            raise ValueError("estimator must be None or one of %s" % sorted(ESTIMATORS))
        self.estimator = estimator
        if estimator is None:
            rc, entry = self.lib.mpct_scenario_create(C.byref(d), C.byref(h)), "mpct_scenario_create"
        else:
            rc, entry = self.lib.mpct_scenario_create_est(C.byref(d), ESTIMATORS[estimator], C.byref(h)), \
                "mpct_scenario_create_est"
        if rc != 0:
            raise MpctError("%s failed (%d): %s" % (entry, rc, _lib.last_error()))
        self._h = h
        self._keep = keep
        self._desc = d   # the descriptor as passed (its buffers live in _keep)
        self.n1 = n1

    @property
    def handle(self):
        return self._h

    def table(self, which: int) -> np.ndarray:
        n = self.lib.mpct_scenario_table(self._h, which, None, 0)
        if n < 0:
            raise MpctError(_lib.last_error())
        buf = np.zeros(n)
        self.lib.mpct_scenario_table(self._h, which, _dp(buf), n)
        return buf

    def dims(self) -> dict:
        """mpct_scenario_table(2): the ABI-6 dims table, every entry named."""
        k = ["my", "nu", "nd", "n2_max", "nu_max", "tlen", "nx", "nyh", "nup", "nit", "nq"]
        t = self.table(2)
        if t.size != len(k):
            raise MpctError("dims table has %d entries, expected %d" % (t.size, len(k)))
        return dict(zip(k, t.astype(int).tolist()))

    def lds_bytes(self, N2=None, Nu=None, costs_only=False) -> int:
        """LDS per workgroup with the open-loop leg / trajectories (or, costs_only, of the
        cost-only instance GAM_fun.m:81 calls launch)."""
        if costs_only:
            return int(self.lib.mpct_lds_bytes_opts(self._h, None, N2 or self.n2_max, Nu or self.nu_max))
        return int(self.lib.mpct_lds_bytes(self._h, N2 or self.n2_max, Nu or self.nu_max))

    def close(self):
        if getattr(self, "_h", None):
            self.lib.mpct_scenario_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


@dataclass
class EvalResult:
    J1: np.ndarray          # (S, my)
    j21: np.ndarray         # (S, my)
    j22: np.ndarray         # (S, my)
    Jnu: np.ndarray         # (S, nu)
    status: np.ndarray      # (S,)
    qp_iters: np.ndarray    # (S,)
    y: np.ndarray | None = None      # (S, my, nit)
    u: np.ndarray | None = None      # (S, nu, nit)
    ys: np.ndarray | None = None
    uopt: np.ndarray | None = None
    nref: int = 1
    extra: dict = field(default_factory=dict)


def _opts(open_loop, want_traj, device=-1, max_qp_iter=0, feas_tol=0.0):
    return _lib.MpctOpts(int(open_loop), int(want_traj), int(max_qp_iter), int(device), float(feas_tol))


def _batch_args(sc, N2, Nu, delta, lam, refs, v):
    """The candidates and signals of one call as the contiguous arrays the library reads:
    (N2, Nu, delta, lam, refs, Cn, nref, vv); vv is None for a scenario without disturbance inputs,
    else v broadcast over the nref reference sets."""
    N2 = np.ascontiguousarray(np.atleast_1d(N2), dtype=np.int32)
    Cn = N2.size
    Nu = np.ascontiguousarray(np.broadcast_to(np.atleast_1d(Nu), (Cn,)), dtype=np.int32)
    delta = np.ascontiguousarray(np.asarray(delta, dtype=float).reshape(Cn, sc.my))
    lam = np.ascontiguousarray(np.asarray(lam, dtype=float).reshape(Cn, sc.nu))
    refs = np.ascontiguousarray(np.asarray(refs, dtype=float).reshape(-1, sc.my, sc.nit))
    nref = refs.shape[0]
    vv = None
    if sc.nd + sc.nq:
        vv = np.ascontiguousarray(np.broadcast_to(np.asarray(v, dtype=float).reshape(-1, sc.nd + sc.nq, sc.nit),
                                                  (nref, sc.nd + sc.nq, sc.nit)))
    return N2, Nu, delta, lam, refs, Cn, nref, vv


def _eval_result(sc, S, nref, open_loop, want_traj):
    """An EvalResult for S simulations and the MpctResult that points into it."""
    res = EvalResult(J1=np.zeros((S, sc.my)), j21=np.zeros((S, sc.my)), j22=np.zeros((S, sc.my)),
                     Jnu=np.zeros((S, sc.nu)), status=np.zeros(S, dtype=np.int32),
                     qp_iters=np.zeros(S, dtype=np.int64), nref=nref)
    r = _lib.MpctResult()
    r.J1, r.j21, r.j22, r.Jnu = _dp(res.J1), _dp(res.j21), _dp(res.j22), _dp(res.Jnu)
    r.status = _ip(res.status)
    r.qp_iters = res.qp_iters.ctypes.data_as(_lib.c_int64_p)
    if want_traj:
        res.y = np.zeros((S, sc.my, sc.nit))
        res.u = np.zeros((S, sc.nu, sc.nit))
        r.y, r.u = _dp(res.y), _dp(res.u)
        if open_loop:
            res.ys = np.zeros((S, sc.my, sc.nit))
            res.uopt = np.zeros((S, sc.nu, sc.nit))
            r.ys, r.uopt = _dp(res.ys), _dp(res.uopt)
    return res, r


def eval_batch(sc: Scenario, N2, Nu, delta, lam, refs, v=None, open_loop=False, want_traj=False,
               device=-1, max_qp_iter=0, feas_tol=0.0) -> EvalResult:
    """Score C candidates against nref reference sets (host arrays in, host arrays out)."""
    N2, Nu, delta, lam, refs, Cn, nref, vv = _batch_args(sc, N2, Nu, delta, lam, refs, v)
    res, r = _eval_result(sc, Cn * nref, nref, open_loop, want_traj)
    o = _opts(open_loop, want_traj, device, max_qp_iter, feas_tol)
    rc = sc.lib.mpct_eval_batch(sc.handle, Cn, N2.ctypes.data, Nu.ctypes.data, delta.ctypes.data,
                                lam.ctypes.data, nref, refs.ctypes.data,
                                vv.ctypes.data if vv is not None else None, C.byref(o), C.byref(r))
    if rc != 0:
        raise MpctError("mpct_eval_batch failed (%d): %s" % (rc, _lib.last_error()))
    return res


def eval_batch_device(sc: Scenario, N2, Nu, delta, lam, refs, out: dict, v=None, open_loop=False,
                      device=-1, stream=None):
    """Device-pointer entry: every argument is a CUDA (HIP) torch tensor already in HBM; results
    are written into the tensors of ``out`` (keys J1, j21, j22, Jnu, status, qp_iters).  The
    launch is enqueued on ``stream`` (torch stream; default: current) and not synchronised."""
    import torch

    if stream is None:
        stream = torch.cuda.current_stream()
    Cn = N2.numel()
    nref = refs.shape[0]
    r = _lib.MpctResult()
    r.J1 = _tptr(out.get("J1"), _lib.c_double_p)
    r.j21 = _tptr(out.get("j21"), _lib.c_double_p)
    r.j22 = _tptr(out.get("j22"), _lib.c_double_p)
    r.Jnu = _tptr(out.get("Jnu"), _lib.c_double_p)
    r.status = _tptr(out.get("status"), _lib.c_int32_p)
    r.qp_iters = _tptr(out.get("qp_iters"), _lib.c_int64_p)
    o = _opts(open_loop, False, device)
    rc = sc.lib.mpct_eval_batch_device(
        sc.handle, Cn, C.c_void_p(N2.data_ptr()), C.c_void_p(Nu.data_ptr()), C.c_void_p(delta.data_ptr()),
        C.c_void_p(lam.data_ptr()), nref, C.c_void_p(refs.data_ptr()),
        C.c_void_p(v.data_ptr()) if v is not None else None, C.byref(o), C.byref(r),
        C.c_void_p(stream.cuda_stream))
    if rc != 0:
        raise MpctError("mpct_eval_batch_device failed (%d): %s" % (rc, _lib.last_error()))


def closedloop_toolbox(sc: Scenario, r, v, N, Nu, delta, lam, nit=None):
    """[y,u,t,ys,uopt] = closedloop_toolbox(mpc_toolbox,r,v,N,Nu,delta,lambda,nit)
    (closedloop_toolbox.m:1).  N, Nu may be vectors (max taken, :38-40).  Row signals out."""
    nit = sc.nit if nit is None else int(nit)
    if nit != sc.nit:
        raise ValueError("scenario was built for nit=%d" % sc.nit)
    N2 = int(np.max(N))
    nuh = int(np.max(Nu))
    res = eval_batch(sc, [N2], [nuh], np.reshape(delta, (1, -1)), np.reshape(lam, (1, -1)),
                     np.asarray(r, dtype=float)[None], v=None if v is None or np.size(v) == 0 else np.asarray(v)[None],
                     open_loop=True, want_traj=True)
    t = np.arange(nit) * sc.Ts
    return res.y[0], res.u[0], t, res.ys[0], res.uopt[0]


def kernel_instance(sc: Scenario, open_loop=False, want_traj=False) -> str:
    """mpct_kernel_instance: the kernel instance eval_batch launches for these options."""
    buf = C.create_string_buffer(128)
    n = sc.lib.mpct_kernel_instance(sc.handle, C.byref(_opts(open_loop, want_traj)), buf, len(buf))
    if n < 0:
        raise MpctError(_lib.last_error())
    return buf.value.decode()


def shard_candidates(C_: int, ndev: int, k: int) -> np.ndarray:
    """mpct_shard_candidates: the candidates of device slot k (k, k+ndev, ... < C)."""
    lib = _lib.load()
    n = lib.mpct_shard_candidates(int(C_), int(ndev), int(k), None, 0)
    if n < 0:
        raise MpctError(_lib.last_error())
    idx = np.zeros(n, dtype=np.int64)
    lib.mpct_shard_candidates(int(C_), int(ndev), int(k), idx.ctypes.data_as(_lib.c_int64_p), n)
    return idx


def eval_batch_multi(sc: Scenario, devices, N2, Nu, delta, lam, refs, v=None, open_loop=False,
                     want_traj=False, max_qp_iter=0, feas_tol=0.0) -> EvalResult:
    """mpct_eval_batch_multi: one call scores the candidates on every GPU of ``devices`` at once
    (strided shards, one host thread, context and stream per list entry, results in the caller's
    order; a device may be listed more than once)."""
    devs = np.ascontiguousarray(np.atleast_1d(devices), dtype=np.int32)
    N2, Nu, delta, lam, refs, Cn, nref, vv = _batch_args(sc, N2, Nu, delta, lam, refs, v)
    res, r = _eval_result(sc, Cn * nref, nref, open_loop, want_traj)
    o = _opts(open_loop, want_traj, -1, max_qp_iter, feas_tol)
    rc = sc.lib.mpct_eval_batch_multi(sc.handle, len(devs), _ip(devs), Cn, N2.ctypes.data, Nu.ctypes.data,
                                      delta.ctypes.data, lam.ctypes.data, nref, refs.ctypes.data,
                                      vv.ctypes.data if vv is not None else None, C.byref(o), C.byref(r))
    if rc != 0:
        raise MpctError("mpct_eval_batch_multi failed (%d): %s" % (rc, _lib.last_error()))
    return res


# --------------------------------------------------------------------------------------------
# robust scoring over plant draws (mpct_eval_robust, include/mpct.h)
@dataclass
class RobustResult:
    """One record per candidate over its D draws.  A draw fails when its status is non-zero, its
    total cost J = sum_i J1_i is not finite, or J > j_bound; the statistics run over the others."""
    mean: np.ndarray          # (C, my) mean over the surviving draws of J1_i; NaN if none survives
    worst: np.ndarray         # (C, my) max over the surviving draws of J1_i; NaN if none survives
    n_failed: np.ndarray      # (C,) failed draws
    worst_draw: np.ndarray    # (C,) surviving draw with the largest J (lowest index on ties); -1 if none
    status: np.ndarray        # (C,) OR of the draws' status bits
    draws: int = 1
    J1: np.ndarray | None = None   # (C * draws, my) per-simulation costs of the same launch (want_J1)
    # tail statistics of the total cost J over the surviving draws (eval_robust(levels=...); include/mpct.h)
    levels: np.ndarray | None = None     # (nlev,) the levels asked for, each in (0, 1]
    quantile: np.ndarray | None = None   # (C, nlev) type-1 empirical quantile J_(ceil(a n)); NaN if none survives
    cvar: np.ndarray | None = None       # (C, nlev) mean of the survivors from that rank upwards
    q_draw: np.ndarray | None = None     # (C, nlev) the draw whose J is the quantile; -1 if none survives

    def scores(self, max_failed: int = 0, stat: str = "worst") -> np.ndarray:
        """(C, my) costs for ranking: the chosen statistic ('worst' or 'mean'), NaN for every
        candidate with more than ``max_failed`` failed draws (rank_candidates and mpct_rank_device
        sort NaN last)."""
        if stat not in ("worst", "mean"):
            raise ValueError("stat must be 'worst' or 'mean'")
        s = np.array(self.worst if stat == "worst" else self.mean, dtype=float, copy=True)
        s[np.asarray(self.n_failed) > int(max_failed)] = np.nan
        return s

    def pareto(self, stat: str = "worst", max_failed: int = 0, max_layers: int = 0, columns=(), device: int = -1):
        """Pareto analysis (``pareto``) of the (C, my) statistic ``scores`` returns, so a candidate with more
        than ``max_failed`` failed draws is invalid: dom_count and layer -1, never on the front.
        ``columns`` adds tail columns of an eval_robust(levels=...) result as further objectives: pairs
        (name, j) with name 'quantile' or 'cvar' and j the level's index."""
        return pareto(self._cost_table(stat, max_failed, columns), max_layers=max_layers, device=device)

    def goal_attain(self, goals, weights, n_best: int = 1, stat: str = "worst", max_failed: int = 0, columns=(),
                    device: int = -1):
        """Goal-attainment selection (``goal_attain``) over the cost table ``pareto`` analyses (same ``stat``,
        ``max_failed`` and ``columns``): a candidate over ``max_failed`` is feasible for no goal vector."""
        return goal_attain(self._cost_table(stat, max_failed, columns), goals, weights, n_best=n_best, device=device)

    def hypervolume(self, stat: str = "worst", max_failed: int = 0, columns=(), device: int = -1, **kw):
        """``hypervolume`` of the front of the cost table ``pareto`` analyses (same ``stat``, ``max_failed`` and
        ``columns``); ``kw`` are hypervolume's lo, ref, n_samples and seed."""
        costs = self._cost_table(stat, max_failed, columns)
        return pareto(costs, device=device).hypervolume(costs, device=device, **kw)

    def hypervolume_exact(self, stat: str = "worst", max_failed: int = 0, columns=(), device: int = -1, **kw):
        """``hypervolume_exact`` of the front of the cost table ``pareto`` analyses (at most three columns);
        ``kw`` are hypervolume_exact's lo and ref."""
        costs = self._cost_table(stat, max_failed, columns)
        return pareto(costs, device=device).hypervolume_exact(costs, device=device, **kw)

    def select(self, n_pick: int, stat: str = "worst", max_failed: int = 0, columns=(), device: int = -1, **kw):
        """``ParetoResult.select`` on the front of the cost table ``pareto`` analyses: the candidate indices of the
        ``n_pick`` members that carry it, in pick order; ``kw`` are hv_select's lo, ref, n_samples and seed."""
        costs = self._cost_table(stat, max_failed, columns)
        return pareto(costs, device=device).select(costs, n_pick, device=device, **kw)

    def _cost_table(self, stat, max_failed, columns):
        cols = [self.scores(max_failed, stat)]
        for name, j in columns:
            if name not in ("quantile", "cvar"):
                raise ValueError("columns take 'quantile' or 'cvar'")
            tab = getattr(self, name)
            if tab is None:
                raise ValueError("this result has no %s: call eval_robust with levels=" % name)
            cols.append(np.asarray(tab, dtype=float)[:, int(j)].reshape(-1, 1))
        costs = np.hstack(cols)
        costs[np.isnan(cols[0]).any(axis=1)] = np.nan   # the masking of scores covers the added columns too
        return costs


def _levels(levels):
    """The levels of a tail call as the contiguous float64 vector the library reads (a host pointer)."""
    lv = np.ascontiguousarray(np.atleast_1d(levels), dtype=np.float64)
    if lv.ndim != 1:
        raise ValueError("levels must be a vector")
    return lv


def eval_robust(sc: Scenario, N2, Nu, delta, lam, refs, v=None, j_bound=0.0, device=-1, want_J1=False,
                max_qp_iter=0, feas_tol=0.0, levels=None) -> RobustResult:
    """Score C candidates over the D = len(refs) draws (reference set k, plant variant k % nplant)
    and reduce on the device to per-candidate statistics (host arrays in and out).  ``j_bound``:
    a draw whose total cost exceeds it fails (0 = 1e100, inf allowed).  ``levels`` (up to 8 values in
    (0, 1]) adds the tail record of the total cost from the same launch (mpct_eval_robust_tail):
    quantile, cvar and q_draw, each of shape (C, nlev)."""
    N2, Nu, delta, lam, refs, Cn, D, vv = _batch_args(sc, N2, Nu, delta, lam, refs, v)
    res = RobustResult(mean=np.zeros((Cn, sc.my)), worst=np.zeros((Cn, sc.my)), n_failed=np.zeros(Cn, dtype=np.int32),
                       worst_draw=np.zeros(Cn, dtype=np.int32), status=np.zeros(Cn, dtype=np.int32), draws=D,
                       J1=np.zeros((Cn * D, sc.my)) if want_J1 else None)
    r = _lib.MpctRobustResult()
    r.mean, r.worst = _dp(res.mean), _dp(res.worst)
    r.n_failed, r.worst_draw, r.status = _ip(res.n_failed), _ip(res.worst_draw), _ip(res.status)
    if want_J1:
        r.J1 = _dp(res.J1)
    o = _opts(False, False, device, max_qp_iter, feas_tol)
    if levels is not None:
        lv = _levels(levels)
        res.levels = lv
        res.quantile, res.cvar = np.zeros((Cn, lv.size)), np.zeros((Cn, lv.size))
        res.q_draw = np.zeros((Cn, lv.size), dtype=np.int32)
        t = _lib.MpctRobustTail(_dp(res.quantile), _dp(res.cvar), _ip(res.q_draw))
        rc = sc.lib.mpct_eval_robust_tail(sc.handle, Cn, N2.ctypes.data, Nu.ctypes.data, delta.ctypes.data,
                                          lam.ctypes.data, D, refs.ctypes.data,
                                          vv.ctypes.data if vv is not None else None, float(j_bound), C.byref(o),
                                          lv.size, _dp(lv), C.byref(r), C.byref(t))
        if rc != 0:
            raise MpctError("mpct_eval_robust_tail failed (%d): %s" % (rc, _lib.last_error()))
        return res
    rc = sc.lib.mpct_eval_robust(sc.handle, Cn, N2.ctypes.data, Nu.ctypes.data, delta.ctypes.data, lam.ctypes.data,
                                 D, refs.ctypes.data, vv.ctypes.data if vv is not None else None, float(j_bound),
                                 C.byref(o), C.byref(r))
    if rc != 0:
        raise MpctError("mpct_eval_robust failed (%d): %s" % (rc, _lib.last_error()))
    return res


def _robust_struct(out: dict):
    r = _lib.MpctRobustResult()
    r.mean, r.worst = _tptr(out.get("mean"), _lib.c_double_p), _tptr(out.get("worst"), _lib.c_double_p)
    r.n_failed, r.worst_draw = _tptr(out.get("n_failed"), _lib.c_int32_p), _tptr(out.get("worst_draw"), _lib.c_int32_p)
    r.status, r.J1 = _tptr(out.get("status"), _lib.c_int32_p), _tptr(out.get("J1"), _lib.c_double_p)
    return r


def eval_robust_device(sc: Scenario, N2, Nu, delta, lam, refs, out: dict, v=None, j_bound=0.0, device=-1,
                       stream=None, levels=None):
    """Device-pointer entry of eval_robust: every argument is a CUDA (HIP) torch tensor; the records
    are written into the tensors of ``out`` (keys mean, worst: float64 [C, my]; n_failed, worst_draw,
    status: int32 [C]; J1: float64 [C * D, my]; any may be absent).  Enqueued on ``stream`` (torch
    stream; default: current) and not synchronised.  ``levels`` (a HOST sequence, up to 8 values in
    (0, 1]) adds the tail record through mpct_eval_robust_tail_device: ``out`` keys quantile, cvar
    (float64 [C, nlev]) and q_draw (int32 [C, nlev]), any may be absent."""
    import torch

    if stream is None:
        stream = torch.cuda.current_stream()
    r = _robust_struct(out)
    o = _opts(False, False, device)
    if levels is not None:
        lv = _levels(levels)
        t = _lib.MpctRobustTail(_tptr(out.get("quantile"), _lib.c_double_p), _tptr(out.get("cvar"), _lib.c_double_p),
                                _tptr(out.get("q_draw"), _lib.c_int32_p))
        rc = sc.lib.mpct_eval_robust_tail_device(
            sc.handle, N2.numel(), C.c_void_p(N2.data_ptr()), C.c_void_p(Nu.data_ptr()), C.c_void_p(delta.data_ptr()),
            C.c_void_p(lam.data_ptr()), refs.shape[0], C.c_void_p(refs.data_ptr()),
            C.c_void_p(v.data_ptr()) if v is not None else None, float(j_bound), C.byref(o), lv.size, _dp(lv),
            C.byref(r), C.byref(t), C.c_void_p(stream.cuda_stream))
        if rc != 0:
            raise MpctError("mpct_eval_robust_tail_device failed (%d): %s" % (rc, _lib.last_error()))
        return
    rc = sc.lib.mpct_eval_robust_device(
        sc.handle, N2.numel(), C.c_void_p(N2.data_ptr()), C.c_void_p(Nu.data_ptr()), C.c_void_p(delta.data_ptr()),
        C.c_void_p(lam.data_ptr()), refs.shape[0], C.c_void_p(refs.data_ptr()),
        C.c_void_p(v.data_ptr()) if v is not None else None, float(j_bound), C.byref(o), C.byref(r),
        C.c_void_p(stream.cuda_stream))
    if rc != 0:
        raise MpctError("mpct_eval_robust_device failed (%d): %s" % (rc, _lib.last_error()))


def robust_instance(sc: Scenario) -> str:
    """mpct_robust_instance: what eval_robust launches for this scenario."""
    buf = C.create_string_buffer(192)
    n = sc.lib.mpct_robust_instance(sc.handle, None, buf, len(buf))
    if n < 0:
        raise MpctError(_lib.last_error())
    return buf.value.decode()


# --------------------------------------------------------------------------------------------
# Pareto front, domination counts and layers of a scored grid (mpct_pareto, include/mpct.h)
@dataclass
class ParetoResult:
    """a dominates b when both are valid (no NaN cost), a <= b in every objective and a < b in one."""
    dom_count: np.ndarray           # (C,) valid candidates that dominate c; 0 = on the front; -1 = invalid
    layer: np.ndarray | None        # (C,) non-dominated-sorting layer, max_layers = deeper; -1 = invalid; None without max_layers
    front: np.ndarray               # (n_front,) the candidates with dom_count 0, ascending

    def hypervolume(self, costs, **kw):
        """``hypervolume`` of this front: ``costs`` is the table the front was computed from."""
        return hypervolume(costs, members=self.front, **kw)

    def hypervolume_exact(self, costs, **kw):
        """``hypervolume_exact`` of this front (at most three objectives): ``costs`` is the table the front was
        computed from."""
        return hypervolume_exact(costs, members=self.front, **kw)

    def select(self, costs, n_pick: int, **kw):
        """The candidate indices of the ``n_pick`` members that carry this front (fewer when the selection ends
        early), in pick order: ``hv_select`` over the front; ``costs`` is the table the front was computed from."""
        return hv_select(costs, n_pick, members=self.front, **kw).picked


def _pareto_costs(costs):
    a = np.ascontiguousarray(costs, dtype=np.float64)
    if a.ndim == 1:
        a = a.reshape(-1, 1)
    if a.ndim != 2:
        raise ValueError("costs must be (C, k)")
    return a


def pareto(costs, max_layers: int = 0, device: int = -1) -> ParetoResult:
    """mpct_pareto: Pareto front, domination counts and (with ``max_layers`` = 1 .. 64) the
    non-dominated-sorting layers of the (C, k) cost table, computed on the GPU (host arrays in and out)."""
    a = _pareto_costs(costs)
    Cn, k = a.shape
    dom = np.zeros(Cn, dtype=np.int32)
    lay = np.zeros(Cn, dtype=np.int32) if max_layers else None
    front = np.zeros(Cn, dtype=np.int32)
    nf = np.zeros(1, dtype=np.int32)
    r = _lib.MpctParetoResult(_ip(dom), _ip(lay) if lay is not None else None, _ip(front), _ip(nf))
    rc = _lib.load().mpct_pareto(a.ctypes.data, Cn, k, int(max_layers), int(device), C.byref(r))
    if rc != 0:
        raise MpctError("mpct_pareto failed (%d): %s" % (rc, _lib.last_error()))
    return ParetoResult(dom_count=dom, layer=lay, front=front[:int(nf[0])].copy())


def pareto_device(costs, out: dict, max_layers: int = 0):
    """mpct_pareto_device: ``costs`` is a float64 CUDA (HIP) tensor [C, k]; the results are written into the
    int32 tensors of ``out`` (keys dom_count, layer, front: [C]; n_front: [1]; any may be absent, front
    needs n_front).  Enqueued on the current torch stream of the tensor's device and not synchronised."""
    import torch

    if costs.dtype != torch.float64 or costs.dim() != 2 or not costs.is_contiguous():
        raise ValueError("costs must be a contiguous float64 tensor [C, k]")
    r = _lib.MpctParetoResult(*[_tptr(out.get(f), _lib.c_int32_p) for f in ("dom_count", "layer", "front", "n_front")])
    stream = torch.cuda.current_stream(costs.device).cuda_stream
    with torch.cuda.device(costs.device):
        rc = _lib.load().mpct_pareto_device(C.c_void_p(costs.data_ptr()), costs.shape[0], costs.shape[1],
                                            int(max_layers), C.byref(r), C.c_void_p(stream))
    if rc != 0:
        raise MpctError("mpct_pareto_device failed (%d): %s" % (rc, _lib.last_error()))


# --------------------------------------------------------------------------------------------
# Goal-attainment selection over a scored grid (mpct_goal_attain, include/mpct.h)
@dataclass
class GoalResult:
    """Per goal / weight vector g, the candidates that minimise gamma = max_j (F_j - goal_j) / w_j among those
    that meet every hard objective (w_j = 0: F_j <= goal_j); ties by ascending candidate index."""
    best: np.ndarray | None         # (G, n_best) candidates by ascending (gamma, index); -1 beyond n_feasible; None with n_best = 0
    gamma: np.ndarray | None        # (G, n_best) their attainment factors; NaN beyond n_feasible
    active: np.ndarray | None       # (G, n_best) the smallest j that attains the maximum; -1 beyond n_feasible
    n_feasible: np.ndarray          # (G,) feasible candidates
    n_attained: np.ndarray          # (G,) feasible candidates with gamma <= 0
    wins: np.ndarray                # (C,) goal vectors whose best[g, 0] is c

    def winners(self) -> np.ndarray:
        """The distinct ``best[:, 0]`` by descending ``wins``, ties by ascending index."""
        c = np.flatnonzero(self.wins > 0)
        return c[np.argsort(-self.wins[c].astype(np.int64), kind="stable")].astype(np.int32)


def _goal_rows(x, G, k, what):
    """goals or weights as a contiguous (G, k) float64 array; a (k,) one is broadcast (G None: one row)"""
    a = np.asarray(x, dtype=np.float64)
    if a.ndim == 1:
        a = np.broadcast_to(a, (1 if G is None else G, a.shape[0]))
    if a.ndim != 2 or a.shape[1] != k or (G is not None and a.shape[0] != G):
        raise ValueError("%s must be (k,) or (G, k) with k = %d" % (what, k))
    return np.ascontiguousarray(a)


def _goal_shapes(goals, weights, k):
    """goals and weights as (G, k) arrays, a (k,) one broadcast to the other's G"""
    G = next((np.shape(x)[0] for x in (goals, weights) if np.ndim(x) == 2), None)
    return _goal_rows(goals, G, k, "goals"), _goal_rows(weights, G, k, "weights")


def goal_attain(costs, goals, weights, n_best: int = 1, device: int = -1) -> GoalResult:
    """mpct_goal_attain: goal-attainment selection over the (C, k) cost table for the goal / weight vectors
    ``goals`` and ``weights`` ((k,) or (G, k); a (k,) one is broadcast), computed on the GPU (host arrays in
    and out).  A weight of 0 makes that objective a hard constraint ``F_j <= goal_j``."""
    a = _pareto_costs(costs)
    Cn, k = a.shape
    gl, w = _goal_shapes(goals, weights, k)
    G, nb = gl.shape[0], int(n_best)
    rows = max(nb, 0)
    best = np.zeros((G, rows), dtype=np.int32) if nb else None
    gam = np.zeros((G, rows), dtype=np.float64) if nb else None
    act = np.zeros((G, rows), dtype=np.int32) if nb else None
    nf, na = np.zeros(G, dtype=np.int32), np.zeros(G, dtype=np.int32)
    wins = np.zeros(Cn, dtype=np.int32)
    r = _lib.MpctGoalResult(_ip(best) if nb else None, _dp(gam) if nb else None, _ip(act) if nb else None, _ip(nf), _ip(na),
                            _ip(wins))
    rc = _lib.load().mpct_goal_attain(a.ctypes.data, Cn, k, gl.ctypes.data, w.ctypes.data, G, nb, int(device), C.byref(r))
    if rc != 0:
        raise MpctError("mpct_goal_attain failed (%d): %s" % (rc, _lib.last_error()))
    return GoalResult(best=best, gamma=gam, active=act, n_feasible=nf, n_attained=na, wins=wins)


def goal_attain_device(costs, goals, weights, out: dict, n_best: int = 1):
    """mpct_goal_attain_device: ``costs`` [C, k], ``goals`` and ``weights`` [G, k] are contiguous float64 CUDA (HIP)
    tensors; the results are written into the tensors of ``out`` (keys best, active: int32 [G, n_best]; gamma:
    float64 [G, n_best]; n_feasible, n_attained: int32 [G]; wins: int32 [C]; any may be absent).  Enqueued on the
    current torch stream of the tensor's device and not synchronised.  An invalid goal vector gets -1 / NaN rows."""
    import torch

    for t, what in ((costs, "costs"), (goals, "goals"), (weights, "weights")):
        if t.dtype != torch.float64 or t.dim() != 2 or not t.is_contiguous():
            raise ValueError("%s must be a contiguous float64 tensor [rows, k]" % what)
    if goals.shape != weights.shape or goals.shape[1] != costs.shape[1]:
        raise ValueError("goals and weights must both be [G, k]")
    types = dict(best=_lib.c_int32_p, gamma=_lib.c_double_p, active=_lib.c_int32_p, n_feasible=_lib.c_int32_p,
                 n_attained=_lib.c_int32_p, wins=_lib.c_int32_p)
    r = _lib.MpctGoalResult(*[_tptr(out.get(f), ty) for f, ty in types.items()])
    stream = torch.cuda.current_stream(costs.device).cuda_stream
    with torch.cuda.device(costs.device):
        rc = _lib.load().mpct_goal_attain_device(C.c_void_p(costs.data_ptr()), costs.shape[0], costs.shape[1],
                                                 C.c_void_p(goals.data_ptr()), C.c_void_p(weights.data_ptr()),
                                                 goals.shape[0], int(n_best), C.byref(r), C.c_void_p(stream))
    if rc != 0:
        raise MpctError("mpct_goal_attain_device failed (%d): %s" % (rc, _lib.last_error()))


# --------------------------------------------------------------------------------------------
# Hypervolume of a front in a box and per-member contributions (mpct_hypervolume, include/mpct.h)
@dataclass
class HypervolumeResult:
    """Monte-Carlo over ``n_samples`` counter-based points of the box [lo, ref]: member a covers point p when
    a <= p in every objective."""
    hv: float                       # n_covered / n_samples * volume
    n_covered: int                  # points covered by at least one member
    n_samples: int
    excl: np.ndarray                # (M,) int64 points that member m alone covers; 0: redundant
    depth_hist: np.ndarray          # (8,) int64 points covered by 0, 1, .., 6 and >= 7 members
    lo: np.ndarray                  # (k,) the box
    ref: np.ndarray
    volume: float                   # of the box
    members: np.ndarray | None = None   # (M,) the candidates excl refers to (-1: skipped); None: all, in order

    @property
    def contribution(self) -> np.ndarray:
        """(M,) the volume each member alone dominates"""
        return self.excl / self.n_samples * self.volume


def box_volume(lo, ref) -> float:
    """The product over ascending j of (ref_j - lo_j) from 1.0, every factor rounded (the contract's vol)."""
    vol = 1.0
    for l, r in zip(np.asarray(lo, dtype=np.float64).tolist(), np.asarray(ref, dtype=np.float64).tolist()):
        vol *= r - l
    return vol


def default_box(costs, members=None, lo=None, ref=None):
    """(lo, ref) with the ones not given computed over the members that have no NaN: lo = the column minima,
    ref = hi + 0.1 (hi - lo) with hi the column maxima, and hi + 0.1 max(|hi|, 1) where hi == lo."""
    a = _pareto_costs(costs)
    if lo is None or ref is None:
        m = None if members is None else np.asarray(members, dtype=np.int64).reshape(-1)
        rows = a if m is None else a[m[(m >= 0) & (m < a.shape[0])]]
        rows = rows[~np.isnan(rows).any(axis=1)]
        if rows.shape[0] == 0:
            raise ValueError("no member without NaN: give lo and ref explicitly")
        cmin, cmax = rows.min(axis=0), rows.max(axis=0)
        with np.errstate(invalid="ignore"):
            span = np.where(cmax == cmin, np.maximum(np.abs(cmax), 1.0), cmax - cmin)
        lo = cmin if lo is None else lo
        ref = cmax + 0.1 * span if ref is None else ref
    lo = np.array(np.broadcast_to(np.asarray(lo, dtype=np.float64), (a.shape[1],)))   # owned copies
    ref = np.array(np.broadcast_to(np.asarray(ref, dtype=np.float64), (a.shape[1],)))
    if not (np.isfinite(lo).all() and np.isfinite(ref).all()):
        raise ValueError("the box is not finite (lo = %s, ref = %s): give lo and ref explicitly" % (lo, ref))
    return lo, ref


def hypervolume(costs, members=None, lo=None, ref=None, n_samples: int = 1 << 20, seed: int = 0,
                device: int = -1) -> HypervolumeResult:
    """mpct_hypervolume: the hypervolume the rows ``members`` of the (C, k) cost table dominate inside the box
    [lo, ref] (None: all rows; -1 entries are skipped, so a -1-padded front may be passed), estimated over
    ``n_samples`` counter-based points on the GPU, with every member's exclusive contribution.  ``lo`` / ``ref``
    None: ``default_box``."""
    a = _pareto_costs(costs)
    Cn, k = a.shape
    mem = None if members is None else np.ascontiguousarray(members, dtype=np.int32).reshape(-1)
    M = Cn if mem is None else mem.size
    lo, ref = default_box(a, mem, lo, ref)
    excl = np.zeros(M, dtype=np.int64)
    hist = np.zeros(_lib.HV_BINS, dtype=np.int64)
    ncov = np.zeros(1, dtype=np.int64)
    hv = np.zeros(1, dtype=np.float64)
    i64 = lambda x: x.ctypes.data_as(_lib.c_int64_p)
    r = _lib.MpctHvResult(i64(ncov), i64(excl), i64(hist), _dp(hv))
    rc = _lib.load().mpct_hypervolume(a.ctypes.data, Cn, k, mem.ctypes.data if mem is not None else None, M,
                                      lo.ctypes.data, ref.ctypes.data, int(n_samples), int(seed) & (2 ** 64 - 1),
                                      int(device), C.byref(r))
    if rc != 0:
        raise MpctError("mpct_hypervolume failed (%d): %s" % (rc, _lib.last_error()))
    return HypervolumeResult(hv=float(hv[0]), n_covered=int(ncov[0]), n_samples=int(n_samples), excl=excl,
                             depth_hist=hist, lo=lo, ref=ref, volume=box_volume(lo, ref),
                             members=None if mem is None else mem.copy())


def hypervolume_device(costs, out: dict, lo, ref, members=None, n_samples: int = 1 << 20, seed: int = 0):
    """mpct_hypervolume_device: ``costs`` is a float64 CUDA (HIP) tensor [C, k], ``members`` an int32 tensor [M]
    or None (all rows), ``lo`` and ``ref`` float64 tensors [k] on the same device (there is no default box:
    computing one would wait for the device).  The results are written into the tensors of ``out`` (keys
    n_covered [1], excl [M], depth_hist [8]: int64; hv [1]: float64; any may be absent).  Enqueued on the
    current torch stream of the tensor's device and not synchronised."""
    import torch

    if costs.dtype != torch.float64 or costs.dim() != 2 or not costs.is_contiguous():
        raise ValueError("costs must be a contiguous float64 tensor [C, k]")
    k = costs.shape[1]
    for name, t in (("lo", lo), ("ref", ref)):
        if t.dtype != torch.float64 or t.shape != (k,) or not t.is_contiguous() or t.device != costs.device:
            raise ValueError("%s must be a contiguous float64 tensor [k] on the costs' device" % name)
    if members is not None and (members.dtype != torch.int32 or members.dim() != 1 or not members.is_contiguous()
                                or members.device != costs.device):
        raise ValueError("members must be a contiguous int32 tensor [M] on the costs' device")
    M = costs.shape[0] if members is None else members.shape[0]
    if out.get("excl") is not None and out["excl"].numel() < M:
        raise ValueError("out['excl'] holds fewer than M entries")
    r = _lib.MpctHvResult(*[_tptr(out.get(f), _lib.c_int64_p) for f in ("n_covered", "excl", "depth_hist")],
                          _tptr(out.get("hv"), _lib.c_double_p))
    stream = torch.cuda.current_stream(costs.device).cuda_stream
    with torch.cuda.device(costs.device):
        rc = _lib.load().mpct_hypervolume_device(C.c_void_p(costs.data_ptr()), costs.shape[0], k,
                                                 C.c_void_p(members.data_ptr()) if members is not None else None, M,
                                                 C.c_void_p(lo.data_ptr()), C.c_void_p(ref.data_ptr()), int(n_samples),
                                                 int(seed) & (2 ** 64 - 1), C.byref(r), C.c_void_p(stream))
    if rc != 0:
        raise MpctError("mpct_hypervolume_device failed (%d): %s" % (rc, _lib.last_error()))


# --------------------------------------------------------------------------------------------
# Exact hypervolume and contributions for at most three objectives (mpct_hypervolume_exact, include/mpct.h;
# DESIGN.md §19)
@dataclass
class HvExactResult:
    """The volume of the box [lo, ref] the members dominate and the volume each member alone dominates, by a
    sweep with rounding error only: at most (M^2 + 8) 2^-53 vol on each value."""
    hv: float                       # volume of the union of the members' boxes
    excl: np.ndarray                # (M,) float64 volume member m alone dominates; +0.0: redundant, inactive or duplicated
    n_active: int                   # members with a box of positive volume
    vol: float                      # of the box
    lo: np.ndarray                  # (k,) the box
    ref: np.ndarray
    members: np.ndarray | None = None   # (M,) the candidates excl refers to (-1: skipped); None: all, in order

    def contribution(self) -> np.ndarray:
        """(M,) each member's share of the hypervolume, excl / hv (zeros when hv is 0)"""
        return self.excl / self.hv if self.hv > 0.0 else np.zeros_like(self.excl)


def hypervolume_exact(costs, members=None, lo=None, ref=None, device: int = -1) -> HvExactResult:
    """mpct_hypervolume_exact: the exact hypervolume the rows ``members`` of the (C, k) cost table, k <= 3,
    dominate inside the box [lo, ref] (None: all rows; -1 entries are skipped, so a -1-padded front may be
    passed), with every member's exclusive contribution, computed by a sweep on the GPU.  ``lo`` / ``ref`` None:
    ``default_box``.  More than three columns raise MpctError (MPCT_ERANGE): there is no fall-back to the
    Monte-Carlo estimate of ``hypervolume``."""
    a = _pareto_costs(costs)
    Cn, k = a.shape
    mem = None if members is None else np.ascontiguousarray(members, dtype=np.int32).reshape(-1)
    M = Cn if mem is None else mem.size
    if k > _lib.HVX_MAX_OBJ:   # the library's error, before a default box is computed for nothing
        lo_, ref_ = np.zeros(k), np.ones(k)
    else:
        lo_, ref_ = default_box(a, mem, lo, ref)
    excl = np.zeros(M, dtype=np.float64)
    hv = np.zeros(1, dtype=np.float64)
    nact = np.zeros(1, dtype=np.int64)
    r = _lib.MpctHvxResult(_dp(hv), _dp(excl) if M else None, nact.ctypes.data_as(_lib.c_int64_p))
    rc = _lib.load().mpct_hypervolume_exact(a.ctypes.data, Cn, k, mem.ctypes.data if mem is not None else None, M,
                                            lo_.ctypes.data, ref_.ctypes.data, int(device), C.byref(r))
    if rc != 0:
        raise MpctError("mpct_hypervolume_exact failed (%d): %s" % (rc, _lib.last_error()))
    return HvExactResult(hv=float(hv[0]), excl=excl, n_active=int(nact[0]), vol=box_volume(lo_, ref_), lo=lo_, ref=ref_,
                         members=None if mem is None else mem.copy())


def hypervolume_exact_device(costs, out: dict, lo, ref, members=None):
    """mpct_hypervolume_exact_device: ``costs`` is a float64 CUDA (HIP) tensor [C, k], k <= 3, ``members`` an
    int32 tensor [M] or None (all rows), ``lo`` and ``ref`` float64 tensors [k] on the same device.  The results
    are written into the tensors of ``out`` (keys hv [1], excl [M]: float64; n_active [1]: int64; any may be
    absent).  Enqueued on the current torch stream of the tensor's device and not synchronised."""
    import torch

    if costs.dtype != torch.float64 or costs.dim() != 2 or not costs.is_contiguous():
        raise ValueError("costs must be a contiguous float64 tensor [C, k]")
    k = costs.shape[1]
    for name, t in (("lo", lo), ("ref", ref)):
        if t.dtype != torch.float64 or t.shape != (k,) or not t.is_contiguous() or t.device != costs.device:
            raise ValueError("%s must be a contiguous float64 tensor [k] on the costs' device" % name)
    if members is not None and (members.dtype != torch.int32 or members.dim() != 1 or not members.is_contiguous()
                                or members.device != costs.device):
        raise ValueError("members must be a contiguous int32 tensor [M] on the costs' device")
    M = costs.shape[0] if members is None else members.shape[0]
    if out.get("excl") is not None and out["excl"].numel() < M:
        raise ValueError("out['excl'] holds fewer than M entries")
    r = _lib.MpctHvxResult(_tptr(out.get("hv"), _lib.c_double_p), _tptr(out.get("excl"), _lib.c_double_p),
                           _tptr(out.get("n_active"), _lib.c_int64_p))
    stream = torch.cuda.current_stream(costs.device).cuda_stream
    with torch.cuda.device(costs.device):
        rc = _lib.load().mpct_hypervolume_exact_device(C.c_void_p(costs.data_ptr()), costs.shape[0], k,
                                                       C.c_void_p(members.data_ptr()) if members is not None else None, M,
                                                       C.c_void_p(lo.data_ptr()), C.c_void_p(ref.data_ptr()), C.byref(r),
                                                       C.c_void_p(stream))
    if rc != 0:
        raise MpctError("mpct_hypervolume_exact_device failed (%d): %s" % (rc, _lib.last_error()))


# --------------------------------------------------------------------------------------------
# Greedy hypervolume subset selection (mpct_hv_select, include/mpct.h)
HVSEL_FIELDS = ("n_picked", "pos", "index", "gain", "covered", "hv", "ties", "n_covered_all")


@dataclass
class HvSelectResult:
    """Greedy forward selection on the coverage count of ``hypervolume``'s sample points: round r picks the
    member that covers the most points no earlier pick covers.  The arrays hold ``n_pick`` slots; the slots
    from ``n_picked`` on hold the end-of-selection fill (pos, index -1; gain, ties 0)."""
    n_picked: int                   # rounds that picked a member
    pos: np.ndarray                 # (K,) int32 position in members of round r's pick
    index: np.ndarray               # (K,) int32 the candidate, members[pos]
    gain: np.ndarray                # (K,) int64 points newly covered by round r's pick
    covered: np.ndarray             # (K,) int64 running sum of gain
    hv: np.ndarray                  # (K,) covered / n_samples * volume
    ties: np.ndarray                # (K,) int32 entries that held round r's largest gain; 1: the pick was forced
    n_covered_all: int              # points covered by any member: hypervolume's n_covered
    n_samples: int
    lo: np.ndarray                  # (k,) the box
    ref: np.ndarray
    volume: float

    @property
    def picked(self) -> np.ndarray:
        """(n_picked,) the picked candidates in pick order"""
        return self.index[:self.n_picked]

    @property
    def share(self) -> np.ndarray:
        """(K,) covered / n_covered_all: the part of the front's coverage the first r + 1 picks hold"""
        with np.errstate(invalid="ignore", divide="ignore"):
            return self.covered / np.float64(self.n_covered_all)

    def cut(self, name: str) -> np.ndarray:
        """the array ``name`` cut to n_picked"""
        return getattr(self, name)[:self.n_picked]


def hv_select(costs, n_pick: int, members=None, lo=None, ref=None, n_samples: int = 1 << 20, seed: int = 0,
              device: int = -1) -> HvSelectResult:
    """mpct_hv_select: ``n_pick`` rounds of greedy forward selection among the rows ``members`` of the (C, k) cost
    table (None: all rows; -1 entries are skipped) on the coverage count of ``hypervolume``'s sample points in
    the box [lo, ref] (None: ``default_box``), on the GPU."""
    a = _pareto_costs(costs)
    Cn, k = a.shape
    mem = None if members is None else np.ascontiguousarray(members, dtype=np.int32).reshape(-1)
    M = Cn if mem is None else mem.size
    lo, ref = default_box(a, mem, lo, ref)
    K = max(int(n_pick), 0)
    i32 = {f: np.zeros(K, dtype=np.int32) for f in ("pos", "index", "ties")}
    i64 = {f: np.zeros(K, dtype=np.int64) for f in ("gain", "covered")}
    hv = np.zeros(K, dtype=np.float64)
    npk, nall = np.zeros(1, dtype=np.int64), np.zeros(1, dtype=np.int64)
    p64 = lambda x: x.ctypes.data_as(_lib.c_int64_p)
    r = _lib.MpctHvSelectResult(p64(npk), _ip(i32["pos"]), _ip(i32["index"]), p64(i64["gain"]), p64(i64["covered"]),
                                _dp(hv), _ip(i32["ties"]), p64(nall))
    rc = _lib.load().mpct_hv_select(a.ctypes.data, Cn, k, mem.ctypes.data if mem is not None else None, M,
                                    lo.ctypes.data, ref.ctypes.data, int(n_samples), int(seed) & (2 ** 64 - 1),
                                    int(n_pick), int(device), C.byref(r))
    if rc != 0:
        raise MpctError("mpct_hv_select failed (%d): %s" % (rc, _lib.last_error()))
    return HvSelectResult(n_picked=int(npk[0]), pos=i32["pos"], index=i32["index"], gain=i64["gain"],
                          covered=i64["covered"], hv=hv, ties=i32["ties"], n_covered_all=int(nall[0]),
                          n_samples=int(n_samples), lo=lo, ref=ref, volume=box_volume(lo, ref))


def hv_select_device(costs, n_pick: int, out: dict, lo, ref, members=None, n_samples: int = 1 << 20, seed: int = 0):
    """mpct_hv_select_device: tensors as for ``hypervolume_device``.  The results are written into the tensors of
    ``out`` (keys n_picked, n_covered_all [1], gain, covered [n_pick]: int64; pos, index, ties [n_pick]: int32;
    hv [n_pick]: float64; any may be absent).  Enqueued on the current torch stream of the tensor's device and
    not synchronised."""
    import torch

    if costs.dtype != torch.float64 or costs.dim() != 2 or not costs.is_contiguous():
        raise ValueError("costs must be a contiguous float64 tensor [C, k]")
    k = costs.shape[1]
    for name, t in (("lo", lo), ("ref", ref)):
        if t.dtype != torch.float64 or t.shape != (k,) or not t.is_contiguous() or t.device != costs.device:
            raise ValueError("%s must be a contiguous float64 tensor [k] on the costs' device" % name)
    if members is not None and (members.dtype != torch.int32 or members.dim() != 1 or not members.is_contiguous()
                                or members.device != costs.device):
        raise ValueError("members must be a contiguous int32 tensor [M] on the costs' device")
    M = costs.shape[0] if members is None else members.shape[0]
    for f in ("pos", "index", "gain", "covered", "hv", "ties"):
        if out.get(f) is not None and out[f].numel() < int(n_pick):
            raise ValueError("out[%r] holds fewer than n_pick entries" % f)
    ctype = dict(pos=_lib.c_int32_p, index=_lib.c_int32_p, ties=_lib.c_int32_p, hv=_lib.c_double_p)
    r = _lib.MpctHvSelectResult(*[_tptr(out.get(f), ctype.get(f, _lib.c_int64_p)) for f in HVSEL_FIELDS])
    stream = torch.cuda.current_stream(costs.device).cuda_stream
    with torch.cuda.device(costs.device):
        rc = _lib.load().mpct_hv_select_device(C.c_void_p(costs.data_ptr()), costs.shape[0], k,
                                               C.c_void_p(members.data_ptr()) if members is not None else None, M,
                                               C.c_void_p(lo.data_ptr()), C.c_void_p(ref.data_ptr()), int(n_samples),
                                               int(seed) & (2 ** 64 - 1), int(n_pick), C.byref(r), C.c_void_p(stream))
    if rc != 0:
        raise MpctError("mpct_hv_select_device failed (%d): %s" % (rc, _lib.last_error()))


# --------------------------------------------------------------------------------------------
# closed-loop performance indices per simulation (mpct_indices, mpct_eval_indices; include/mpct.h)
INDEX_FIELDS = tuple(n for n, _, _ in _lib.INDEX_FIELDS)


@dataclass
class IndexResult:
    """One array per field of mpct_index_result: the output-row fields (C, nref, my), the input-row fields
    (C, nref, nu); a field that was not asked for is None.  An invalid row (a non-finite sample in
    [t0, nit)) holds NaN / -1."""
    iae: np.ndarray | None = None
    ise: np.ndarray | None = None
    itae: np.ndarray | None = None
    emax: np.ndarray | None = None
    t_emax: np.ndarray | None = None
    over: np.ndarray | None = None
    e_final: np.ndarray | None = None
    settle: np.ndarray | None = None     # nit = not settled at the last sample
    tv: np.ndarray | None = None
    du2: np.ndarray | None = None
    dumax: np.ndarray | None = None
    u_lo: np.ndarray | None = None
    u_hi: np.ndarray | None = None
    nit: int = 0
    t0: int = 0
    batch: EvalResult | None = None      # eval_indices(want_costs=True): J1, j22, status, qp_iters of the same launch

    def costs(self, names, reduce: str = "max") -> np.ndarray:
        """(C, len(names)) float matrix for ``pareto``: each named field folded over the references and
        channels by ``reduce`` ('max' or 'sum').  ``e_final`` enters by its magnitude, ``settle`` and
        ``t_emax`` as samples after t0.  A candidate with an invalid row (NaN / -1) or, for ``settle``, an
        unsettled one (settle = nit) gets NaN in that column: invalid for ``pareto``, last for ``rank``."""
        if reduce not in ("max", "sum"):
            raise ValueError("reduce must be 'max' or 'sum'")
        cols = []
        for name in names:
            if name not in INDEX_FIELDS:
                raise ValueError("unknown index field %r" % (name,))
            a = getattr(self, name)
            if a is None:
                raise ValueError("this result has no %s" % name)
            a = np.asarray(a)
            x = a.reshape(a.shape[0], -1).astype(float)
            if name in ("settle", "t_emax"):
                bad = x < 0
                if name == "settle":
                    bad |= x >= self.nit
                x = np.where(bad, np.nan, x - self.t0)
            elif name == "e_final":
                x = np.abs(x)
            # a NaN in the row makes the fold NaN (np.max and np.sum propagate it)
            cols.append(x.max(axis=1) if reduce == "max" else x.sum(axis=1))
        return np.stack(cols, axis=1) if cols else np.zeros((0, 0))

    def goal_attain(self, names, goals, weights, n_best: int = 1, device: int = -1, **kw):
        """Goal-attainment selection (``goal_attain``) over the table ``costs(names, **kw)`` returns."""
        return goal_attain(self.costs(names, **kw), goals, weights, n_best=n_best, device=device)


def _index_fields(fields):
    fields = INDEX_FIELDS if fields is None else tuple(fields)
    for f in fields:
        if f not in INDEX_FIELDS:
            raise ValueError("unknown index field %r" % (f,))
    return fields


def _index_result(Cn, nref, my, nu, nit, t0, fields):
    """An IndexResult with the arrays of ``fields`` and the MpctIndexResult that points into them."""
    res = IndexResult(nit=int(nit), t0=int(t0))
    r = _lib.MpctIndexResult()
    for name, is_y, is_int in _lib.INDEX_FIELDS:
        if name in fields:
            a = np.zeros((Cn, nref, my if is_y else nu), dtype=np.int32 if is_int else np.float64)
            setattr(res, name, a)
            setattr(r, name, _ip(a) if is_int else _dp(a))
    return res, r


def indices(y, u, r, t0=0, band_rel=0.02, band_abs=0.0, fields=None, device=-1) -> IndexResult:
    """mpct_indices: the performance indices of stored trajectories, reduced on the GPU (host arrays in and
    out).  ``y`` (S, my, nit), ``u`` (S, nu, nit), ``r`` (nref, my, nit); simulation s reads reference set
    s % nref.  ``y`` and ``r`` may be None when ``fields`` names no output-row field, ``u`` when it names no
    input-row field.  The arrays of the result are (S / nref, nref, my) and (S / nref, nref, nu)."""
    fields = _index_fields(fields)
    y = None if y is None else np.ascontiguousarray(y, dtype=np.float64)
    u = None if u is None else np.ascontiguousarray(u, dtype=np.float64)
    r = None if r is None else np.ascontiguousarray(r, dtype=np.float64)
    if (y is not None and y.ndim != 3) or (u is not None and u.ndim != 3) or (r is not None and r.ndim != 3):
        raise ValueError("y, u and r must be 3-d: (S, my, nit), (S, nu, nit), (nref, my, nit)")
    if y is None and u is None:
        raise ValueError("y or u is needed")
    S, nit = (y if y is not None else u).shape[0], (y if y is not None else u).shape[2]
    my = y.shape[1] if y is not None else (r.shape[1] if r is not None else 0)
    nu = u.shape[1] if u is not None else 0
    nref = r.shape[0] if r is not None else 1
    if (u is not None and u.shape[::2] != (S, nit)) or (r is not None and (r.shape[1] != my or r.shape[2] != nit)):
        raise ValueError("y, u and r disagree on S, my or nit")
    if S % nref:
        raise ValueError("S must be a multiple of nref")
    res, out = _index_result(S // nref, nref, my, nu, nit, t0, fields)
    p = _lib.MpctIndexParams(int(t0), float(band_rel), float(band_abs))
    rc = _lib.load().mpct_indices(y.ctypes.data if y is not None else None, u.ctypes.data if u is not None else None,
                                  r.ctypes.data if r is not None else None, S, nref, my, nu, nit, C.byref(p), int(device),
                                  C.byref(out))
    if rc != 0:
        raise MpctError("mpct_indices failed (%d): %s" % (rc, _lib.last_error()))
    return res


def _index_struct(out: dict):
    r = _lib.MpctIndexResult()
    for name, _, is_int in _lib.INDEX_FIELDS:
        setattr(r, name, _tptr(out.get(name), _lib.c_int32_p if is_int else _lib.c_double_p))
    return r


def indices_device(y, u, r, out: dict, t0=0, band_rel=0.02, band_abs=0.0):
    """mpct_indices_device: ``y`` [S, my, nit], ``u`` [S, nu, nit], ``r`` [nref, my, nit] are contiguous float64
    CUDA (HIP) tensors (None where no field needs them); the records are written into the tensors of ``out``
    (keys as the fields of IndexResult: float64 / int32, [S, my] or [S, nu]; any may be absent).  Enqueued on
    the current torch stream of the tensors' device and not synchronised."""
    import torch

    some = y if y is not None else u
    for t in (y, u, r):
        if t is not None and (t.dtype != torch.float64 or t.dim() != 3 or not t.is_contiguous()):
            raise ValueError("y, u and r must be contiguous float64 tensors with three dimensions")
    S, nit = some.shape[0], some.shape[2]
    my = y.shape[1] if y is not None else (r.shape[1] if r is not None else 0)
    nu = u.shape[1] if u is not None else 0
    nref = r.shape[0] if r is not None else 1
    p = _lib.MpctIndexParams(int(t0), float(band_rel), float(band_abs))
    o = _index_struct(out)
    stream = torch.cuda.current_stream(some.device).cuda_stream
    ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None  # noqa: E731
    with torch.cuda.device(some.device):
        rc = _lib.load().mpct_indices_device(ptr(y), ptr(u), ptr(r), S, nref, my, nu, nit, C.byref(p), C.byref(o),
                                             C.c_void_p(stream))
    if rc != 0:
        raise MpctError("mpct_indices_device failed (%d): %s" % (rc, _lib.last_error()))


def eval_indices(sc, N2, Nu, delta, lam, refs, v=None, t0=0, band_rel=0.02, band_abs=0.0, fields=None,
                 want_costs=False, device=-1, max_qp_iter=0, feas_tol=0.0) -> IndexResult:
    """mpct_eval_indices: score C candidates against nref reference sets and return only the index records
    of the closed loops (host arrays in and out); the trajectories stay on the device.  ``want_costs`` adds
    ``batch``: J1, j22, status and qp_iters of the same launch, as eval_batch returns them."""
    fields = _index_fields(fields)
    N2, Nu, delta, lam, refs, Cn, nref, vv = _batch_args(sc, N2, Nu, delta, lam, refs, v)
    res, out = _index_result(Cn, nref, sc.my, sc.nu, sc.nit, t0, fields)
    br = None
    if want_costs:
        res.batch, br = _eval_result(sc, Cn * nref, nref, False, False)
    p = _lib.MpctIndexParams(int(t0), float(band_rel), float(band_abs))
    o = _opts(False, False, device, max_qp_iter, feas_tol)
    rc = sc.lib.mpct_eval_indices(sc.handle, Cn, N2.ctypes.data, Nu.ctypes.data, delta.ctypes.data, lam.ctypes.data,
                                  nref, refs.ctypes.data, vv.ctypes.data if vv is not None else None, C.byref(o),
                                  C.byref(p), C.byref(br) if br is not None else None, C.byref(out))
    if rc != 0:
        raise MpctError("mpct_eval_indices failed (%d): %s" % (rc, _lib.last_error()))
    return res


def eval_indices_device(sc, N2, Nu, delta, lam, refs, out: dict, v=None, t0=0, band_rel=0.02, band_abs=0.0,
                        device=-1, stream=None):
    """Device-pointer entry of eval_indices: every argument is a CUDA (HIP) torch tensor; the records are
    written into the tensors of ``out`` (the keys of indices_device, [C * nref, my] / [C * nref, nu], plus
    the optional J1, j21, j22, Jnu, status, qp_iters of eval_batch_device).  Enqueued on ``stream`` (torch
    stream; default: current) and not synchronised."""
    import torch

    if stream is None:
        stream = torch.cuda.current_stream()
    br = _lib.MpctResult()
    br.J1, br.j21 = _tptr(out.get("J1"), _lib.c_double_p), _tptr(out.get("j21"), _lib.c_double_p)
    br.j22, br.Jnu = _tptr(out.get("j22"), _lib.c_double_p), _tptr(out.get("Jnu"), _lib.c_double_p)
    br.status, br.qp_iters = _tptr(out.get("status"), _lib.c_int32_p), _tptr(out.get("qp_iters"), _lib.c_int64_p)
    p = _lib.MpctIndexParams(int(t0), float(band_rel), float(band_abs))
    o = _opts(False, False, device)
    io = _index_struct(out)
    rc = sc.lib.mpct_eval_indices_device(
        sc.handle, N2.numel(), C.c_void_p(N2.data_ptr()), C.c_void_p(Nu.data_ptr()), C.c_void_p(delta.data_ptr()),
        C.c_void_p(lam.data_ptr()), refs.shape[0], C.c_void_p(refs.data_ptr()),
        C.c_void_p(v.data_ptr()) if v is not None else None, C.byref(o), C.byref(p), C.byref(br), C.byref(io),
        C.c_void_p(stream.cuda_stream))
    if rc != 0:
        raise MpctError("mpct_eval_indices_device failed (%d): %s" % (rc, _lib.last_error()))


# --------------------------------------------------------------------------------------------
# statistics of a table over its draw axis, and of the indices over the plant draws (mpct_draw_stats,
# mpct_eval_robust_indices; include/mpct.h)
@dataclass
class DrawStats:
    """One record per column (c, i) of a (C, D, m) table over its surviving draws; NaN / -1 where none survives."""
    n: np.ndarray                        # (C, m) surviving draws
    mean: np.ndarray                     # (C, m)
    lo: np.ndarray                       # (C, m) smallest surviving value
    lo_draw: np.ndarray                  # (C, m) the lowest draw that holds it
    hi: np.ndarray                       # (C, m) largest surviving value
    hi_draw: np.ndarray                  # (C, m) the lowest draw that holds it
    levels: np.ndarray | None = None     # (nlev,)
    quantile: np.ndarray | None = None   # (C, m, nlev) type-1 quantile of the survivors
    cvar: np.ndarray | None = None       # (C, m, nlev) mean of the survivors from that rank upwards
    q_draw: np.ndarray | None = None     # (C, m, nlev) the draw whose value is the quantile


def _stats_arrays(Cn, m, nlev):
    """The nine arrays of a statistics record (the per-level ones None without levels) and the MpctDrawStats
    that points into them."""
    arr, r = {}, _lib.MpctDrawStats()
    for name, is_int, per_level in _lib.STATS_FIELDS:
        if per_level and not nlev:
            arr[name] = None
            continue
        a = np.zeros((Cn, m, nlev) if per_level else (Cn, m), dtype=np.int32 if is_int else np.float64)
        arr[name] = a
        setattr(r, name, _ip(a) if is_int else _dp(a))
    return arr, r


def _stats_struct(out: dict):
    r = _lib.MpctDrawStats()
    for name, is_int, _ in _lib.STATS_FIELDS:
        setattr(r, name, _tptr(out.get(name), _lib.c_int32_p if is_int else _lib.c_double_p))
    return r


def draw_stats(x, alive=None, levels=None, device=-1) -> DrawStats:
    """mpct_draw_stats: statistics of the (C, D, m) table ``x`` over its draw axis, reduced on the GPU (host
    arrays in and out).  An integer ``x`` enters as int32 (a negative value is "no value"), anything else as
    float64 (a non-finite value is no value).  ``alive`` (C, D): a zero drops the draw from every column of
    its candidate.  ``levels`` (up to 8 values in (0, 1]) adds quantile, cvar and q_draw."""
    x = np.asarray(x)
    is_int = np.issubdtype(x.dtype, np.integer)
    x = np.ascontiguousarray(x, dtype=np.int32 if is_int else np.float64)
    if x.ndim != 3:
        raise ValueError("x must be (C, D, m)")
    Cn, D, m = x.shape
    al = None
    if alive is not None:
        al = np.ascontiguousarray(alive, dtype=np.int32)
        if al.shape != (Cn, D):
            raise ValueError("alive must be (C, D)")
    lv = _levels(levels) if levels is not None else None
    nlev = 0 if lv is None else lv.size
    arr, r = _stats_arrays(Cn, m, nlev)
    rc = _lib.load().mpct_draw_stats(x.ctypes.data, _lib.STAT_I32 if is_int else _lib.STAT_F64,
                                     al.ctypes.data if al is not None else None, Cn, D, m, nlev,
                                     _dp(lv) if nlev else None, int(device), C.byref(r))
    if rc != 0:
        raise MpctError("mpct_draw_stats failed (%d): %s" % (rc, _lib.last_error()))
    return DrawStats(levels=lv, **arr)


def draw_stats_device(x, out: dict, alive=None, levels=None):
    """mpct_draw_stats_device: ``x`` is a contiguous float64 or int32 CUDA (HIP) tensor [C, D, m], ``alive`` an
    int32 tensor [C, D] or None; the records are written into the tensors of ``out`` (keys as the fields of
    DrawStats: n, lo_draw, hi_draw, q_draw int32, the others float64; [C, m] or [C, m, nlev]; any may be
    absent).  ``levels`` is a HOST sequence.  Enqueued on the current torch stream of the tensor's device and
    not synchronised."""
    import torch

    if x.dtype not in (torch.float64, torch.int32) or x.dim() != 3 or not x.is_contiguous():
        raise ValueError("x must be a contiguous float64 or int32 tensor [C, D, m]")
    if alive is not None and (alive.dtype != torch.int32 or tuple(alive.shape) != tuple(x.shape[:2]) or
                              not alive.is_contiguous()):
        raise ValueError("alive must be a contiguous int32 tensor [C, D]")
    lv = _levels(levels) if levels is not None else None
    nlev = 0 if lv is None else lv.size
    r = _stats_struct(out)
    stream = torch.cuda.current_stream(x.device).cuda_stream
    with torch.cuda.device(x.device):
        rc = _lib.load().mpct_draw_stats_device(
            C.c_void_p(x.data_ptr()), _lib.STAT_I32 if x.dtype == torch.int32 else _lib.STAT_F64,
            C.c_void_p(alive.data_ptr()) if alive is not None else None, x.shape[0], x.shape[1], x.shape[2], nlev,
            _dp(lv) if nlev else None, C.byref(r), C.c_void_p(stream))
    if rc != 0:
        raise MpctError("mpct_draw_stats_device failed (%d): %s" % (rc, _lib.last_error()))


@dataclass
class RobustIndexResult:
    """Per candidate and column, the statistics of the selected performance indices over the surviving plant
    draws.  ``columns`` names the W columns: (field name, channel) in selection order, an output-row field
    contributing my columns and an input-row field nu.  ``base`` is the RobustResult of the same launch
    (mean / worst of J1, n_failed, worst_draw, status)."""
    columns: list
    n: np.ndarray                        # (C, W)
    mean: np.ndarray
    lo: np.ndarray
    lo_draw: np.ndarray
    hi: np.ndarray
    hi_draw: np.ndarray
    base: RobustResult                   # costs() masks by its n_failed
    levels: np.ndarray | None = None
    quantile: np.ndarray | None = None   # (C, W, nlev)
    cvar: np.ndarray | None = None
    q_draw: np.ndarray | None = None

    def costs(self, stat="hi", names=None, max_failed: int = 0) -> np.ndarray:
        """(C, k) cost table for ``pareto``: the statistic ``stat`` ('mean', 'lo', 'hi', ('quantile', j) or
        ('cvar', j) with j the level's index) of the columns whose field is in ``names`` (None: every column,
        in selection order).  NaN for every candidate with more than ``max_failed`` failed draws, as
        RobustResult.scores masks."""
        if isinstance(stat, str):
            if stat not in ("mean", "lo", "hi"):
                raise ValueError("stat must be 'mean', 'lo', 'hi', ('quantile', j) or ('cvar', j)")
            tab = getattr(self, stat)
        else:
            name, j = stat
            if name not in ("quantile", "cvar"):
                raise ValueError("stat must be 'mean', 'lo', 'hi', ('quantile', j) or ('cvar', j)")
            if getattr(self, name) is None:
                raise ValueError("this result has no %s: call eval_robust_indices with levels=" % name)
            tab = getattr(self, name)[:, :, int(j)]
        if names is None:
            keep = list(range(len(self.columns)))
        else:
            for nm in names:
                if not any(f == nm for f, _ in self.columns):
                    raise ValueError("this result has no field %r" % (nm,))
            keep = [k for nm in names for k, (f, _) in enumerate(self.columns) if f == nm]
        out = np.array(np.asarray(tab, dtype=float)[:, keep], dtype=float, copy=True)
        out[np.asarray(self.base.n_failed) > int(max_failed)] = np.nan
        return out

    def pareto(self, stat="hi", names=None, max_failed: int = 0, max_layers: int = 0, device: int = -1):
        """Pareto analysis (``pareto``) of the table ``costs`` returns."""
        return pareto(self.costs(stat, names, max_failed), max_layers=max_layers, device=device)

    def goal_attain(self, stat, names, goals, weights, n_best: int = 1, max_failed: int = 0, device: int = -1):
        """Goal-attainment selection (``goal_attain``) over the table ``costs`` returns."""
        return goal_attain(self.costs(stat, names, max_failed=max_failed), goals, weights, n_best=n_best, device=device)

    def hypervolume(self, stat="hi", names=None, max_failed: int = 0, device: int = -1, **kw):
        """``hypervolume`` of the front of the table ``costs`` returns; ``kw`` are hypervolume's lo, ref,
        n_samples and seed."""
        costs = self.costs(stat, names, max_failed)
        return pareto(costs, device=device).hypervolume(costs, device=device, **kw)

    def hypervolume_exact(self, stat="hi", names=None, max_failed: int = 0, device: int = -1, **kw):
        """``hypervolume_exact`` of the front of the table ``costs`` returns (at most three columns); ``kw`` are
        hypervolume_exact's lo and ref."""
        costs = self.costs(stat, names, max_failed)
        return pareto(costs, device=device).hypervolume_exact(costs, device=device, **kw)

    def select(self, n_pick: int, stat="hi", names=None, max_failed: int = 0, device: int = -1, **kw):
        """``ParetoResult.select`` on the front of the table ``costs`` returns; ``kw`` are hv_select's lo, ref,
        n_samples and seed."""
        costs = self.costs(stat, names, max_failed)
        return pareto(costs, device=device).select(costs, n_pick, device=device, **kw)


def _field_ids(sc, fields):
    """The ids of the selected fields as the int32 vector the library reads, and the (field, channel) columns."""
    fields = _index_fields(fields)
    ids = np.ascontiguousarray([INDEX_FIELDS.index(f) for f in fields], dtype=np.int32)
    is_y = {n: y for n, y, _ in _lib.INDEX_FIELDS}
    cols = [(f, ch) for f in fields for ch in range(sc.my if is_y[f] else sc.nu)]
    return ids, cols


def eval_robust_indices(sc, N2, Nu, delta, lam, refs, v=None, fields=None, levels=None, j_bound=0.0, t0=0,
                        band_rel=0.02, band_abs=0.0, device=-1, max_qp_iter=0, feas_tol=0.0) -> RobustIndexResult:
    """mpct_eval_robust_indices: score C candidates over the D = len(refs) draws and reduce, on the device, the
    performance indices ``fields`` (default: all thirteen) of the C x D closed loops to per-candidate
    statistics over the surviving draws (host arrays in and out).  A draw survives by eval_robust's rule
    (status 0, total J1 finite and <= ``j_bound``); ``levels`` adds quantile, cvar and q_draw per column."""
    N2, Nu, delta, lam, refs, Cn, D, vv = _batch_args(sc, N2, Nu, delta, lam, refs, v)
    ids, cols = _field_ids(sc, fields)
    lv = _levels(levels) if levels is not None else None
    nlev = 0 if lv is None else lv.size
    arr, out = _stats_arrays(Cn, len(cols), nlev)
    base = RobustResult(mean=np.zeros((Cn, sc.my)), worst=np.zeros((Cn, sc.my)), n_failed=np.zeros(Cn, dtype=np.int32),
                        worst_draw=np.zeros(Cn, dtype=np.int32), status=np.zeros(Cn, dtype=np.int32), draws=D)
    br = _lib.MpctRobustResult()
    br.mean, br.worst = _dp(base.mean), _dp(base.worst)
    br.n_failed, br.worst_draw, br.status = _ip(base.n_failed), _ip(base.worst_draw), _ip(base.status)
    p = _lib.MpctIndexParams(int(t0), float(band_rel), float(band_abs))
    o = _opts(False, False, device, max_qp_iter, feas_tol)
    rc = sc.lib.mpct_eval_robust_indices(sc.handle, Cn, N2.ctypes.data, Nu.ctypes.data, delta.ctypes.data, lam.ctypes.data,
                                         D, refs.ctypes.data, vv.ctypes.data if vv is not None else None, float(j_bound),
                                         C.byref(o), C.byref(p), ids.size, _ip(ids), nlev, _dp(lv) if nlev else None,
                                         C.byref(br), C.byref(out))
    if rc != 0:
        raise MpctError("mpct_eval_robust_indices failed (%d): %s" % (rc, _lib.last_error()))
    return RobustIndexResult(columns=cols, levels=lv, base=base, **arr)


def eval_robust_indices_device(sc, N2, Nu, delta, lam, refs, out: dict, base: dict | None = None, v=None, fields=None,
                               levels=None, j_bound=0.0, t0=0, band_rel=0.02, band_abs=0.0, device=-1, stream=None):
    """Device-pointer entry of eval_robust_indices: every argument is a CUDA (HIP) torch tensor (``fields`` and
    ``levels`` are HOST sequences); the statistics are written into the tensors of ``out`` (the keys of
    draw_stats_device, [C, W] / [C, W, nlev]) and the robust record of J1 into those of ``base`` (the keys
    of eval_robust_device without J1).  Enqueued on ``stream`` (torch stream; default: current) and not
    synchronised."""
    import torch

    if stream is None:
        stream = torch.cuda.current_stream()
    ids, _ = _field_ids(sc, fields)
    lv = _levels(levels) if levels is not None else None
    nlev = 0 if lv is None else lv.size
    br = _robust_struct(base or {})
    p = _lib.MpctIndexParams(int(t0), float(band_rel), float(band_abs))
    o = _opts(False, False, device)
    so = _stats_struct(out)
    rc = sc.lib.mpct_eval_robust_indices_device(
        sc.handle, N2.numel(), C.c_void_p(N2.data_ptr()), C.c_void_p(Nu.data_ptr()), C.c_void_p(delta.data_ptr()),
        C.c_void_p(lam.data_ptr()), refs.shape[0], C.c_void_p(refs.data_ptr()),
        C.c_void_p(v.data_ptr()) if v is not None else None, float(j_bound), C.byref(o), C.byref(p), ids.size, _ip(ids),
        nlev, _dp(lv) if nlev else None, C.byref(br), C.byref(so), C.c_void_p(stream.cuda_stream))
    if rc != 0:
        raise MpctError("mpct_eval_robust_indices_device failed (%d): %s" % (rc, _lib.last_error()))


# --------------------------------------------------------------------------------------------
# trajectory envelopes over the plant draws (mpct_envelope, mpct_eval_robust_envelope; include/mpct.h)
SPREAD_FIELDS = (("spread", False), ("spread_max", False), ("t_spread_max", True))   # (name, integer?)


@dataclass
class EnvelopeResult:
    """Per candidate, row and sample, the statistics of the trajectories over the surviving plant draws.  ``y`` and
    ``u`` are dicts of the fields of DrawStats, each (C, rows, nit) or, per level, (C, rows, nit, nlev); None for
    a side that was not asked for.  ``spread`` maps 'y' / 'u' to a dict of spread, spread_max and t_spread_max, each
    (C, rows), over the samples t0 .. nit-1.  ``base`` is the RobustResult of the same launch
    (eval_robust_envelope), None for stored trajectories."""
    y: dict | None
    u: dict | None
    spread: dict
    t0: int = 0
    levels: np.ndarray | None = None
    base: RobustResult | None = None

    def costs(self, names=("spread",), sides=("y", "u"), max_failed: int | None = None) -> np.ndarray:
        """(C, k) cost table for ``pareto``: for each of ``names`` ('spread', 'spread_max', 't_spread_max') the rows
        of each side in ``sides`` that this result holds, side by side.  With a ``base`` and ``max_failed``, NaN
        for every candidate with more failed draws, as RobustResult.scores masks."""
        cols = []
        for nm in names:
            if nm not in [f for f, _ in SPREAD_FIELDS]:
                raise ValueError("names take 'spread', 'spread_max' or 't_spread_max'")
            for sd in sides:
                if sd in self.spread:
                    cols.append(np.asarray(self.spread[sd][nm], dtype=float))
        if not cols:
            raise ValueError("this result has no spread on the sides asked for")
        out = np.array(np.hstack(cols), dtype=float, copy=True)
        if max_failed is not None and self.base is not None:
            out[np.asarray(self.base.n_failed) > int(max_failed)] = np.nan
        return out

    def band(self, c: int, row: int, level_lo=None, level_hi=None, side: str = "y"):
        """The two lines to plot for candidate ``c`` and ``row`` of ``side``, each (nit,): the quantile lines at
        ``level_lo`` and ``level_hi`` (values of ``levels``), lo / hi where a level is None."""
        rec = self.y if side == "y" else self.u
        if rec is None:
            raise ValueError("this result has no side %r" % (side,))

        def line(level, edge):
            if level is None:
                return rec[edge][c, row]
            hit = np.flatnonzero(self.levels == float(level)) if self.levels is not None else ()
            if not len(hit):
                raise ValueError("level %r is not one of this result's levels" % (level,))
            return rec["quantile"][c, row, :, hit[0]]

        return line(level_lo, "lo"), line(level_hi, "hi")


def _envelope_side(Cn, rows, nit, nlev):
    """One side's record arrays, shaped (C, rows, nit[, nlev]), its spread arrays (C, rows) and the two structs that
    point into them."""
    arr, r = _stats_arrays(Cn, rows * nit, nlev)
    arr = {k: a.reshape((Cn, rows, nit, nlev) if a.ndim == 3 else (Cn, rows, nit)) for k, a in arr.items() if a is not None}
    sp = {n: np.zeros((Cn, rows), dtype=np.int32 if i else np.float64) for n, i in SPREAD_FIELDS}
    s = _lib.MpctEnvelopeSpread(_dp(sp["spread"]), _dp(sp["spread_max"]), _ip(sp["t_spread_max"]))
    return arr, r, sp, s


def _envelope_structs(out: dict):
    """The four structs of a device-pointer envelope call from ``out``: keys 'y' and 'u' (dicts of the tensors of
    draw_stats_device) and 'spread_y' and 'spread_u' (dicts of spread, spread_max, t_spread_max tensors)."""
    def sp(d):
        return _lib.MpctEnvelopeSpread(_tptr(d.get("spread"), _lib.c_double_p), _tptr(d.get("spread_max"), _lib.c_double_p),
                                       _tptr(d.get("t_spread_max"), _lib.c_int32_p))
    return (_stats_struct(out.get("y") or {}), _stats_struct(out.get("u") or {}), sp(out.get("spread_y") or {}),
            sp(out.get("spread_u") or {}))


def envelope(y, u, alive=None, levels=None, t0=0, device=-1) -> EnvelopeResult:
    """mpct_envelope: the envelopes over the draw axis of stored trajectories ``y`` (C, D, my, nit) and ``u``
    (C, D, nu, nit), either may be None, reduced on the GPU (host arrays in and out).  ``alive`` (C, D): a zero
    drops the draw from every sample of its candidate; a non-finite sample drops the draw from that sample.
    ``levels`` (up to 8 values in (0, 1]) adds quantile, cvar and q_draw; the spread covers t0 .. nit-1."""
    if y is None and u is None:
        raise ValueError("y and u are both None")
    ya = None if y is None else np.ascontiguousarray(y, dtype=np.float64)
    ua = None if u is None else np.ascontiguousarray(u, dtype=np.float64)
    ref = ya if ya is not None else ua
    if any(a is not None and (a.ndim != 4 or a.shape[:2] != ref.shape[:2] or a.shape[3] != ref.shape[3]) for a in (ya, ua)):
        raise ValueError("y must be (C, D, my, nit) and u (C, D, nu, nit)")
    Cn, D, _, nit = ref.shape
    al = None
    if alive is not None:
        al = np.ascontiguousarray(alive, dtype=np.int32)
        if al.shape != (Cn, D):
            raise ValueError("alive must be (C, D)")
    lv = _levels(levels) if levels is not None else None
    nlev = 0 if lv is None else lv.size
    my, nu = (0 if ya is None else ya.shape[2]), (0 if ua is None else ua.shape[2])
    sides, structs = {}, []
    for name, rows in (("y", my), ("u", nu)):
        if rows:
            sides[name] = _envelope_side(Cn, rows, nit, nlev)
            structs += [C.byref(sides[name][1]), C.byref(sides[name][3])]
        else:
            structs += [None, None]
    rc = _lib.load().mpct_envelope(ya.ctypes.data if my else None, ua.ctypes.data if nu else None,
                                   al.ctypes.data if al is not None else None, Cn, D, my, nu, nit, int(t0), nlev,
                                   _dp(lv) if nlev else None, int(device), structs[0], structs[2], structs[1], structs[3])
    if rc != 0:
        raise MpctError("mpct_envelope failed (%d): %s" % (rc, _lib.last_error()))
    return EnvelopeResult(y=sides["y"][0] if "y" in sides else None, u=sides["u"][0] if "u" in sides else None,
                          spread={k: v[2] for k, v in sides.items()}, t0=int(t0), levels=lv)


def envelope_device(y, u, out: dict, alive=None, levels=None, t0=0):
    """mpct_envelope_device: ``y`` [C, D, my, nit] and ``u`` [C, D, nu, nit] are contiguous float64 CUDA (HIP)
    tensors (either may be None), ``alive`` an int32 tensor [C, D] or None; the records are written into the
    tensors of ``out``: keys 'y' and 'u', dicts with the keys of draw_stats_device ([C, rows, nit] or
    [C, rows, nit, nlev]), and 'spread_y' and 'spread_u', dicts of spread, spread_max (float64) and t_spread_max
    (int32), each [C, rows]; any may be absent.  ``levels`` is a HOST sequence.  Enqueued on the current torch
    stream of the tensors' device and not synchronised."""
    import torch

    ref = y if y is not None else u
    for t in (y, u):
        if t is not None and (t.dtype != torch.float64 or t.dim() != 4 or not t.is_contiguous() or
                              tuple(t.shape[:2]) != tuple(ref.shape[:2]) or t.shape[3] != ref.shape[3]):
            raise ValueError("y and u must be contiguous float64 tensors [C, D, rows, nit]")
    if alive is not None and (alive.dtype != torch.int32 or tuple(alive.shape) != tuple(ref.shape[:2]) or
                              not alive.is_contiguous()):
        raise ValueError("alive must be a contiguous int32 tensor [C, D]")
    lv = _levels(levels) if levels is not None else None
    nlev = 0 if lv is None else lv.size
    oy, ou, sy, su = _envelope_structs(out)
    stream = torch.cuda.current_stream(ref.device).cuda_stream
    with torch.cuda.device(ref.device):
        rc = _lib.load().mpct_envelope_device(
            C.c_void_p(y.data_ptr()) if y is not None else None, C.c_void_p(u.data_ptr()) if u is not None else None,
            C.c_void_p(alive.data_ptr()) if alive is not None else None, ref.shape[0], ref.shape[1],
            y.shape[2] if y is not None else 0, u.shape[2] if u is not None else 0, ref.shape[3], int(t0), nlev,
            _dp(lv) if nlev else None, C.byref(oy), C.byref(ou), C.byref(sy), C.byref(su), C.c_void_p(stream))
    if rc != 0:
        raise MpctError("mpct_envelope_device failed (%d): %s" % (rc, _lib.last_error()))


def eval_robust_envelope(sc, N2, Nu, delta, lam, refs, v=None, levels=None, j_bound=0.0, t0=0, device=-1, max_qp_iter=0,
                         feas_tol=0.0) -> EnvelopeResult:
    """mpct_eval_robust_envelope: score C candidates over the D = len(refs) draws and reduce, on the device, the
    trajectories of the C x D closed loops to their envelopes over the surviving draws (host arrays in and out).
    A draw survives by eval_robust's rule (status 0, total J1 finite and <= ``j_bound``); ``levels`` adds
    quantile, cvar and q_draw per sample; the spread covers t0 .. nit-1."""
    N2, Nu, delta, lam, refs, Cn, D, vv = _batch_args(sc, N2, Nu, delta, lam, refs, v)
    lv = _levels(levels) if levels is not None else None
    nlev = 0 if lv is None else lv.size
    ay, ry, spy, sy = _envelope_side(Cn, sc.my, sc.nit, nlev)
    au, ru, spu, su = _envelope_side(Cn, sc.nu, sc.nit, nlev)
    base = RobustResult(mean=np.zeros((Cn, sc.my)), worst=np.zeros((Cn, sc.my)), n_failed=np.zeros(Cn, dtype=np.int32),
                        worst_draw=np.zeros(Cn, dtype=np.int32), status=np.zeros(Cn, dtype=np.int32), draws=D)
    br = _lib.MpctRobustResult()
    br.mean, br.worst = _dp(base.mean), _dp(base.worst)
    br.n_failed, br.worst_draw, br.status = _ip(base.n_failed), _ip(base.worst_draw), _ip(base.status)
    o = _opts(False, False, device, max_qp_iter, feas_tol)
    rc = sc.lib.mpct_eval_robust_envelope(sc.handle, Cn, N2.ctypes.data, Nu.ctypes.data, delta.ctypes.data, lam.ctypes.data,
                                          D, refs.ctypes.data, vv.ctypes.data if vv is not None else None, float(j_bound),
                                          C.byref(o), int(t0), nlev, _dp(lv) if nlev else None, C.byref(br), C.byref(ry),
                                          C.byref(ru), C.byref(sy), C.byref(su))
    if rc != 0:
        raise MpctError("mpct_eval_robust_envelope failed (%d): %s" % (rc, _lib.last_error()))
    return EnvelopeResult(y=ay, u=au, spread={"y": spy, "u": spu}, t0=int(t0), levels=lv, base=base)


def eval_robust_envelope_device(sc, N2, Nu, delta, lam, refs, out: dict, base: dict | None = None, v=None, levels=None,
                                j_bound=0.0, t0=0, device=-1, stream=None):
    """Device-pointer entry of eval_robust_envelope: every argument is a CUDA (HIP) torch tensor (``levels`` is a
    HOST sequence); the envelopes are written into the tensors of ``out`` (the keys of envelope_device) and the
    robust record of J1 into those of ``base`` (the keys of eval_robust_device without J1).  Enqueued on
    ``stream`` (torch stream; default: current) and not synchronised."""
    import torch

    if stream is None:
        stream = torch.cuda.current_stream()
    lv = _levels(levels) if levels is not None else None
    nlev = 0 if lv is None else lv.size
    br = _robust_struct(base or {})
    o = _opts(False, False, device)
    oy, ou, sy, su = _envelope_structs(out)
    rc = sc.lib.mpct_eval_robust_envelope_device(
        sc.handle, N2.numel(), C.c_void_p(N2.data_ptr()), C.c_void_p(Nu.data_ptr()), C.c_void_p(delta.data_ptr()),
        C.c_void_p(lam.data_ptr()), refs.shape[0], C.c_void_p(refs.data_ptr()),
        C.c_void_p(v.data_ptr()) if v is not None else None, float(j_bound), C.byref(o), int(t0), nlev,
        _dp(lv) if nlev else None, C.byref(br), C.byref(oy), C.byref(ou), C.byref(sy), C.byref(su),
        C.c_void_p(stream.cuda_stream))
    if rc != 0:
        raise MpctError("mpct_eval_robust_envelope_device failed (%d): %s" % (rc, _lib.last_error()))


# --------------------------------------------------------------------------------------------
# limit indices per simulation and their statistics over the draws (mpct_limit_indices, mpct_eval_limit_indices,
# mpct_eval_robust_limit_indices; include/mpct.h)
LIMIT_FIELDS = tuple(n for n, _, _ in _lib.LIMIT_FIELDS)
_LIMIT_BOUNDS = ("y_lo", "y_hi", "u_lo", "u_hi", "du_lo", "du_hi")


@dataclass
class LimitResult:
    """One array per field of mpct_limit_result: the output-row fields (C, nref, my), the input-row fields
    (C, nref, nu); a field that was not asked for is None.  An invalid row (a non-finite sample in
    [t0, nit)) holds NaN / -1."""
    viol: np.ndarray | None = None
    viol2: np.ndarray | None = None
    vmax: np.ndarray | None = None
    t_vmax: np.ndarray | None = None
    n_out: np.ndarray | None = None
    t_in: np.ndarray | None = None       # nit = still outside at the last sample
    y_margin: np.ndarray | None = None   # +inf without a bound
    n_lo: np.ndarray | None = None
    n_hi: np.ndarray | None = None
    n_rate: np.ndarray | None = None
    sat_run: np.ndarray | None = None
    u_margin: np.ndarray | None = None
    du_margin: np.ndarray | None = None
    nit: int = 0
    t0: int = 0
    batch: EvalResult | None = None      # eval_limit_indices(want_costs=True): J1, j22, status, qp_iters of the same launch

    def costs(self, names, reduce: str = "max") -> np.ndarray:
        """(C, len(names)) float matrix for ``pareto``: each named field folded over the references and
        channels by ``reduce`` ('max' or 'sum').  The integer fields enter as floats, ``t_vmax`` and ``t_in``
        as samples after t0.  The margins enter negated (less margin costs more), and a channel without a
        bound (an infinite margin) takes no part in the fold.  A candidate with an invalid row (NaN / -1), or
        with no bounded channel for a margin, gets NaN in that column: invalid for ``pareto``, last for
        ``rank``."""
        if reduce not in ("max", "sum"):
            raise ValueError("reduce must be 'max' or 'sum'")
        is_int = {n: i for n, _, i in _lib.LIMIT_FIELDS}
        cols = []
        for name in names:
            if name not in LIMIT_FIELDS:
                raise ValueError("unknown limit field %r" % (name,))
            a = getattr(self, name)
            if a is None:
                raise ValueError("this result has no %s" % name)
            a = np.asarray(a)
            x = a.reshape(a.shape[0], -1).astype(float)
            neutral = np.zeros(x.shape, dtype=bool)
            if is_int[name]:
                x = np.where(x < 0, np.nan, x - (self.t0 if name in ("t_vmax", "t_in") else 0))
            elif name.endswith("margin"):
                neutral = np.isposinf(x)
                x = -x
            # a NaN in the row makes the fold NaN (np.max and np.sum propagate it)
            x = np.where(neutral, -np.inf if reduce == "max" else 0.0, x)
            col = x.max(axis=1) if reduce == "max" else x.sum(axis=1)
            col = np.where(neutral.all(axis=1) & (x.shape[1] > 0), np.nan, col)
            cols.append(col)
        return np.stack(cols, axis=1) if cols else np.zeros((0, 0))

    def goal_attain(self, names, goals, weights, n_best: int = 1, device: int = -1, **kw):
        """Goal-attainment selection (``goal_attain``) over the table ``costs(names, **kw)`` returns."""
        return goal_attain(self.costs(names, **kw), goals, weights, n_best=n_best, device=device)


def _limit_fields(fields):
    fields = LIMIT_FIELDS if fields is None else tuple(fields)
    for f in fields:
        if f not in LIMIT_FIELDS:
            raise ValueError("unknown limit field %r" % (f,))
    return fields


def _limit_params(my, nu, t0, out_tol, sat_tol, bounds: dict):
    """The MpctLimitParams of a call and the host arrays it points to (keep them alive for the call).  ``bounds``
    maps y_lo, y_hi (my values) and u_lo, u_hi, du_lo, du_hi (nu values) to sequences; an absent or None entry
    stays NULL (no bound in the scenario-free entries, the scenario's own bound in the others)."""
    p = _lib.MpctLimitParams(int(t0), float(out_tol), float(sat_tol))
    keep = []
    for name in bounds:
        if name not in _LIMIT_BOUNDS:
            raise ValueError("unknown bound %r" % (name,))
    for name in _LIMIT_BOUNDS:
        a = bounds.get(name)
        if a is None:
            continue
        a = np.ascontiguousarray(np.broadcast_to(np.asarray(a, dtype=np.float64), (my if name[0] == "y" else nu,)))
        keep.append(a)
        setattr(p, name, _dp(a))
    return p, keep


def _limit_result(Cn, nref, my, nu, nit, t0, fields):
    """A LimitResult with the arrays of ``fields`` and the MpctLimitResult that points into them."""
    res = LimitResult(nit=int(nit), t0=int(t0))
    r = _lib.MpctLimitResult()
    for name, is_y, is_int in _lib.LIMIT_FIELDS:
        if name in fields:
            a = np.zeros((Cn, nref, my if is_y else nu), dtype=np.int32 if is_int else np.float64)
            setattr(res, name, a)
            setattr(r, name, _ip(a) if is_int else _dp(a))
    return res, r


def _limit_struct(out: dict):
    r = _lib.MpctLimitResult()
    for name, _, is_int in _lib.LIMIT_FIELDS:
        setattr(r, name, _tptr(out.get(name), _lib.c_int32_p if is_int else _lib.c_double_p))
    return r


def limit_indices(y, u, t0=0, out_tol=0.0, sat_tol=0.0, fields=None, nref=1, device=-1, **bounds) -> LimitResult:
    """mpct_limit_indices: the limit indices of stored trajectories, reduced on the GPU (host arrays in and
    out).  ``y`` (S, my, nit), ``u`` (S, nu, nit); ``y`` may be None when ``fields`` names no output-row field,
    ``u`` when it names no input-row field.  ``bounds``: y_lo, y_hi, u_lo, u_hi, du_lo, du_hi per channel (a
    scalar is broadcast; absent: no bound).  The arrays of the result are (S / nref, nref, my) and
    (S / nref, nref, nu)."""
    y = None if y is None else np.ascontiguousarray(y, dtype=np.float64)
    u = None if u is None else np.ascontiguousarray(u, dtype=np.float64)
    if (y is not None and y.ndim != 3) or (u is not None and u.ndim != 3):
        raise ValueError("y and u must be 3-d: (S, my, nit), (S, nu, nit)")
    if y is None and u is None:
        raise ValueError("y or u is needed")
    some = y if y is not None else u
    S, nit = some.shape[0], some.shape[2]
    my = y.shape[1] if y is not None else 0
    nu = u.shape[1] if u is not None else 0
    if u is not None and u.shape[::2] != (S, nit):
        raise ValueError("y and u disagree on S or nit")
    if fields is None:
        fields = tuple(n for n, is_y, _ in _lib.LIMIT_FIELDS if (y if is_y else u) is not None)
    fields = _limit_fields(fields)
    if nref < 1 or S % nref:
        raise ValueError("S must be a multiple of nref")
    res, out = _limit_result(S // nref, nref, my, nu, nit, t0, fields)
    p, keep = _limit_params(my, nu, t0, out_tol, sat_tol, bounds)
    rc = _lib.load().mpct_limit_indices(y.ctypes.data if y is not None else None, u.ctypes.data if u is not None else None,
                                        S, my, nu, nit, C.byref(p), int(device), C.byref(out))
    del keep
    if rc != 0:
        raise MpctError("mpct_limit_indices failed (%d): %s" % (rc, _lib.last_error()))
    return res


def limit_indices_device(y, u, out: dict, t0=0, out_tol=0.0, sat_tol=0.0, **bounds):
    """mpct_limit_indices_device: ``y`` [S, my, nit] and ``u`` [S, nu, nit] are contiguous float64 CUDA (HIP)
    tensors (None where no field needs them); the records are written into the tensors of ``out`` (keys as the
    fields of LimitResult: float64 / int32, [S, my] or [S, nu]; any may be absent).  ``bounds`` are HOST
    sequences, as in limit_indices.  Enqueued on the current torch stream of the tensors' device and not
    synchronised."""
    import torch

    some = y if y is not None else u
    for t in (y, u):
        if t is not None and (t.dtype != torch.float64 or t.dim() != 3 or not t.is_contiguous()):
            raise ValueError("y and u must be contiguous float64 tensors with three dimensions")
    S, nit = some.shape[0], some.shape[2]
    my = y.shape[1] if y is not None else 0
    nu = u.shape[1] if u is not None else 0
    p, keep = _limit_params(my, nu, t0, out_tol, sat_tol, bounds)
    o = _limit_struct(out)
    stream = torch.cuda.current_stream(some.device).cuda_stream
    ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None  # noqa: E731
    with torch.cuda.device(some.device):
        rc = _lib.load().mpct_limit_indices_device(ptr(y), ptr(u), S, my, nu, nit, C.byref(p), C.byref(o),
                                                   C.c_void_p(stream))
    del keep
    if rc != 0:
        raise MpctError("mpct_limit_indices_device failed (%d): %s" % (rc, _lib.last_error()))


def eval_limit_indices(sc, N2, Nu, delta, lam, refs, v=None, t0=0, out_tol=0.0, sat_tol=0.0, fields=None,
                       want_costs=False, device=-1, max_qp_iter=0, feas_tol=0.0, **bounds) -> LimitResult:
    """mpct_eval_limit_indices: score C candidates against nref reference sets and return only the limit
    records of the closed loops (host arrays in and out); the trajectories stay on the device.  A bound that
    is not given is the scenario's own (du_min / du_max / u_min / u_max, y_min / y_max of a band scenario), or
    none where the scenario holds none.  ``want_costs`` adds ``batch``: J1, j22, status and qp_iters of the
    same launch, as eval_batch returns them."""
    fields = _limit_fields(fields)
    N2, Nu, delta, lam, refs, Cn, nref, vv = _batch_args(sc, N2, Nu, delta, lam, refs, v)
    res, out = _limit_result(Cn, nref, sc.my, sc.nu, sc.nit, t0, fields)
    br = None
    if want_costs:
        res.batch, br = _eval_result(sc, Cn * nref, nref, False, False)
    p, keep = _limit_params(sc.my, sc.nu, t0, out_tol, sat_tol, bounds)
    o = _opts(False, False, device, max_qp_iter, feas_tol)
    rc = sc.lib.mpct_eval_limit_indices(sc.handle, Cn, N2.ctypes.data, Nu.ctypes.data, delta.ctypes.data,
                                        lam.ctypes.data, nref, refs.ctypes.data, vv.ctypes.data if vv is not None else None,
                                        C.byref(o), C.byref(p), C.byref(br) if br is not None else None, C.byref(out))
    del keep
    if rc != 0:
        raise MpctError("mpct_eval_limit_indices failed (%d): %s" % (rc, _lib.last_error()))
    return res


def eval_limit_indices_device(sc, N2, Nu, delta, lam, refs, out: dict, v=None, t0=0, out_tol=0.0, sat_tol=0.0,
                              device=-1, stream=None, **bounds):
    """Device-pointer entry of eval_limit_indices: every argument is a CUDA (HIP) torch tensor (``bounds`` are
    HOST sequences); the records are written into the tensors of ``out`` (the keys of limit_indices_device,
    [C * nref, my] / [C * nref, nu], plus the optional J1, j21, j22, Jnu, status, qp_iters of
    eval_batch_device).  Enqueued on ``stream`` (torch stream; default: current) and not synchronised."""
    import torch

    if stream is None:
        stream = torch.cuda.current_stream()
    br = _lib.MpctResult()
    br.J1, br.j21 = _tptr(out.get("J1"), _lib.c_double_p), _tptr(out.get("j21"), _lib.c_double_p)
    br.j22, br.Jnu = _tptr(out.get("j22"), _lib.c_double_p), _tptr(out.get("Jnu"), _lib.c_double_p)
    br.status, br.qp_iters = _tptr(out.get("status"), _lib.c_int32_p), _tptr(out.get("qp_iters"), _lib.c_int64_p)
    p, keep = _limit_params(sc.my, sc.nu, t0, out_tol, sat_tol, bounds)
    o = _opts(False, False, device)
    lo = _limit_struct(out)
    rc = sc.lib.mpct_eval_limit_indices_device(
        sc.handle, N2.numel(), C.c_void_p(N2.data_ptr()), C.c_void_p(Nu.data_ptr()), C.c_void_p(delta.data_ptr()),
        C.c_void_p(lam.data_ptr()), refs.shape[0], C.c_void_p(refs.data_ptr()),
        C.c_void_p(v.data_ptr()) if v is not None else None, C.byref(o), C.byref(p), C.byref(br), C.byref(lo),
        C.c_void_p(stream.cuda_stream))
    del keep
    if rc != 0:
        raise MpctError("mpct_eval_limit_indices_device failed (%d): %s" % (rc, _lib.last_error()))


def _limit_field_ids(sc, fields):
    """The MPCT_LX_* ids of the selected fields as the int32 vector the library reads, and the (field, channel)
    columns."""
    fields = _limit_fields(fields)
    ids = np.ascontiguousarray([LIMIT_FIELDS.index(f) for f in fields], dtype=np.int32)
    is_y = {n: y for n, y, _ in _lib.LIMIT_FIELDS}
    cols = [(f, ch) for f in fields for ch in range(sc.my if is_y[f] else sc.nu)]
    return ids, cols


def eval_robust_limit_indices(sc, N2, Nu, delta, lam, refs, v=None, fields=None, levels=None, j_bound=0.0, t0=0,
                              out_tol=0.0, sat_tol=0.0, device=-1, max_qp_iter=0, feas_tol=0.0,
                              **bounds) -> RobustIndexResult:
    """mpct_eval_robust_limit_indices: score C candidates over the D = len(refs) draws and reduce, on the
    device, the limit indices ``fields`` (default: all thirteen) of the C x D closed loops to per-candidate
    statistics over the surviving draws (host arrays in and out): eval_robust_indices for the limit indices,
    with the bounds of eval_limit_indices.  A draw without a value in a column (an invalid row, or an infinite
    margin: no bound) does not enter that column."""
    N2, Nu, delta, lam, refs, Cn, D, vv = _batch_args(sc, N2, Nu, delta, lam, refs, v)
    ids, cols = _limit_field_ids(sc, fields)
    lv = _levels(levels) if levels is not None else None
    nlev = 0 if lv is None else lv.size
    arr, out = _stats_arrays(Cn, len(cols), nlev)
    base = RobustResult(mean=np.zeros((Cn, sc.my)), worst=np.zeros((Cn, sc.my)), n_failed=np.zeros(Cn, dtype=np.int32),
                        worst_draw=np.zeros(Cn, dtype=np.int32), status=np.zeros(Cn, dtype=np.int32), draws=D)
    br = _lib.MpctRobustResult()
    br.mean, br.worst = _dp(base.mean), _dp(base.worst)
    br.n_failed, br.worst_draw, br.status = _ip(base.n_failed), _ip(base.worst_draw), _ip(base.status)
    p, keep = _limit_params(sc.my, sc.nu, t0, out_tol, sat_tol, bounds)
    o = _opts(False, False, device, max_qp_iter, feas_tol)
    rc = sc.lib.mpct_eval_robust_limit_indices(
        sc.handle, Cn, N2.ctypes.data, Nu.ctypes.data, delta.ctypes.data, lam.ctypes.data, D, refs.ctypes.data,
        vv.ctypes.data if vv is not None else None, float(j_bound), C.byref(o), C.byref(p), ids.size, _ip(ids), nlev,
        _dp(lv) if nlev else None, C.byref(br), C.byref(out))
    del keep
    if rc != 0:
        raise MpctError("mpct_eval_robust_limit_indices failed (%d): %s" % (rc, _lib.last_error()))
    return RobustIndexResult(columns=cols, levels=lv, base=base, **arr)


def eval_robust_limit_indices_device(sc, N2, Nu, delta, lam, refs, out: dict, base: dict | None = None, v=None,
                                     fields=None, levels=None, j_bound=0.0, t0=0, out_tol=0.0, sat_tol=0.0, device=-1,
                                     stream=None, **bounds):
    """Device-pointer entry of eval_robust_limit_indices: every argument is a CUDA (HIP) torch tensor
    (``fields``, ``levels`` and ``bounds`` are HOST sequences); ``out`` and ``base`` as in
    eval_robust_indices_device.  Enqueued on ``stream`` (torch stream; default: current) and not synchronised."""
    import torch

    if stream is None:
        stream = torch.cuda.current_stream()
    ids, _ = _limit_field_ids(sc, fields)
    lv = _levels(levels) if levels is not None else None
    nlev = 0 if lv is None else lv.size
    br = _robust_struct(base or {})
    p, keep = _limit_params(sc.my, sc.nu, t0, out_tol, sat_tol, bounds)
    o = _opts(False, False, device)
    so = _stats_struct(out)
    rc = sc.lib.mpct_eval_robust_limit_indices_device(
        sc.handle, N2.numel(), C.c_void_p(N2.data_ptr()), C.c_void_p(Nu.data_ptr()), C.c_void_p(delta.data_ptr()),
        C.c_void_p(lam.data_ptr()), refs.shape[0], C.c_void_p(refs.data_ptr()),
        C.c_void_p(v.data_ptr()) if v is not None else None, float(j_bound), C.byref(o), C.byref(p), ids.size, _ip(ids),
        nlev, _dp(lv) if nlev else None, C.byref(br), C.byref(so), C.c_void_p(stream.cuda_stream))
    del keep
    if rc != 0:
        raise MpctError("mpct_eval_robust_limit_indices_device failed (%d): %s" % (rc, _lib.last_error()))


# --------------------------------------------------------------------------------------------
# step-response indices per setpoint segment and their statistics over the draws (mpct_reference_segments,
# mpct_segment_indices, mpct_eval_segment_indices, mpct_eval_robust_segment_indices; include/mpct.h)
SEGMENT_FIELDS = tuple(n for n, _, _ in _lib.SEGMENT_FIELDS)


def reference_segments(r, extra=(), max_seg: int = _lib.SEG_MAX) -> np.ndarray:
    """mpct_reference_segments (host only): the segment boundaries of the reference ``r`` (my, nit) or
    (nref, my, nit) -- 0, every sample at which some row of some reference set changes, the ``extra`` event
    samples (a measured disturbance's instant) and nit -- as the int32 vector ``tseg`` the segment entries take."""
    r = np.ascontiguousarray(r, dtype=np.float64)
    if r.ndim == 2:
        r = r[None]
    if r.ndim != 3:
        raise ValueError("r must be (my, nit) or (nref, my, nit)")
    ex = np.ascontiguousarray(np.asarray(list(extra), dtype=np.int32))
    tseg = np.zeros(int(max_seg) + 1, dtype=np.int32)
    nseg = C.c_int32(0)
    rc = _lib.load().mpct_reference_segments(r.ctypes.data, r.shape[0], r.shape[1], r.shape[2],
                                             _ip(ex) if ex.size else None, ex.size, int(max_seg), _ip(tseg), C.byref(nseg))
    if rc != 0:
        raise MpctError("mpct_reference_segments failed (%d): %s" % (rc, _lib.last_error()))
    return tseg[:nseg.value + 1].copy()


def _segment_cost_table(get, names, tseg, segments, reduce):
    """the fold of SegmentResult.costs: get(name) -> float array (C, rows, nseg) with NaN for no value"""
    if reduce not in ("max", "sum"):
        raise ValueError("reduce must be 'max' or 'sum'")
    nseg = len(tseg) - 1
    seg = list(range(nseg)) if segments is None else [int(g) for g in segments]
    if any(g < 0 or g >= nseg for g in seg):
        raise ValueError("segment out of range")
    cols = []
    for name in names:
        x = get(name)[:, :, seg]
        x = x.reshape(x.shape[0], -1)
        # a NaN in the row makes the fold NaN (np.max and np.sum propagate it)
        cols.append(x.max(axis=1) if reduce == "max" else x.sum(axis=1))
    return np.stack(cols, axis=1) if cols else np.zeros((0, 0))


@dataclass
class SegmentResult:
    """One array per field of mpct_segment_result: the output-row fields (C, nref, my, nseg), the input-row
    fields (C, nref, nu, nseg); a field that was not asked for is None.  An invalid unit (a non-finite sample
    the segment reads) holds NaN / -1."""
    iae: np.ndarray | None = None
    ise: np.ndarray | None = None
    itae: np.ndarray | None = None
    emax: np.ndarray | None = None
    t_emax: np.ndarray | None = None     # an absolute sample
    over: np.ndarray | None = None
    under: np.ndarray | None = None
    e_final: np.ndarray | None = None
    settle: np.ndarray | None = None     # an absolute sample; tseg[g + 1] = not settled inside segment g
    rise: np.ndarray | None = None       # tseg[g + 1] - tseg[g] = rise_hi never reached; -1 = no step (sigma = 0)
    tv: np.ndarray | None = None
    du2: np.ndarray | None = None
    dumax: np.ndarray | None = None
    u_lo: np.ndarray | None = None
    u_hi: np.ndarray | None = None
    tseg: np.ndarray | None = None
    batch: EvalResult | None = None      # eval_segment_indices(want_costs=True): J1, j22, status, qp_iters of the same launch

    def costs(self, names, segments=None, reduce: str = "max") -> np.ndarray:
        """(C, len(names)) float matrix for ``pareto``: each named field folded over the references, the
        channels and the ``segments`` (None: all) by ``reduce`` ('max' or 'sum').  ``e_final`` enters by its
        magnitude, ``settle`` and ``t_emax`` as samples after the segment's start.  A candidate with an invalid
        unit (NaN / -1), an unsettled segment (settle = its end) or a step that never reaches ``rise_hi``
        (rise = the segment's length) gets NaN in that column: invalid for ``pareto``, last for ``rank``.  A
        ``rise`` of -1 where the unit is valid (no step on that channel in that segment) takes no part in the
        fold; a candidate without any step gets NaN."""
        tseg = np.asarray(self.tseg)
        a, b = tseg[:-1].astype(float), tseg[1:].astype(float)

        def get(name):
            if name not in SEGMENT_FIELDS:
                raise ValueError("unknown segment field %r" % (name,))
            arr = getattr(self, name)
            if arr is None:
                raise ValueError("this result has no %s" % name)
            arr = np.asarray(arr)
            x = arr.reshape(arr.shape[0], -1, arr.shape[-1]).astype(float)
            if name in ("settle", "t_emax"):
                bad = x < 0
                if name == "settle":
                    bad |= x >= b
                x = np.where(bad, np.nan, x - a)
            elif name == "rise":
                if self.settle is None and self.t_emax is None:
                    valid = np.ones(x.shape, dtype=bool)     # nothing tells an invalid unit from "no step"
                else:
                    other = np.asarray(self.settle if self.settle is not None else self.t_emax)
                    valid = other.reshape(x.shape) >= 0
                none = (x < 0) & valid
                x = np.where((x < 0) & ~valid, np.nan, np.where(x >= b - a, np.nan, x))
                # no step here: neutral in the fold, NaN where the candidate has no step at all
                x = np.where(none, -np.inf if reduce == "max" else 0.0, x)
                x = np.where(none.all(axis=(1, 2), keepdims=True), np.nan, x)
            elif name == "e_final":
                x = np.abs(x)
            return x

        return _segment_cost_table(get, names, tseg, segments, reduce)

    def goal_attain(self, names, goals, weights, n_best: int = 1, device: int = -1, **kw):
        """Goal-attainment selection (``goal_attain``) over the table ``costs(names, **kw)`` returns."""
        return goal_attain(self.costs(names, **kw), goals, weights, n_best=n_best, device=device)


def _segment_fields(fields):
    fields = SEGMENT_FIELDS if fields is None else tuple(fields)
    for f in fields:
        if f not in SEGMENT_FIELDS:
            raise ValueError("unknown segment field %r" % (f,))
    return fields


def _segment_params(tseg, base, band_rel, band_abs, rise_lo, rise_hi):
    """The MpctSegmentParams of a call and the host boundary vector it points to (keep it alive for the call)."""
    t = np.ascontiguousarray(np.asarray(tseg, dtype=np.int32).reshape(-1))
    if t.size < 2:
        raise ValueError("tseg needs at least two boundaries")
    p = _lib.MpctSegmentParams(t.size - 1, _ip(t), int(base), float(band_rel), float(band_abs), float(rise_lo),
                               float(rise_hi))
    return p, t


def _segment_result(Cn, nref, my, nu, tseg, fields):
    """A SegmentResult with the arrays of ``fields`` and the MpctSegmentResult that points into them."""
    nseg = len(tseg) - 1
    res = SegmentResult(tseg=np.array(tseg, dtype=np.int32))
    r = _lib.MpctSegmentResult()
    for name, is_y, is_int in _lib.SEGMENT_FIELDS:
        if name in fields:
            a = np.zeros((Cn, nref, my if is_y else nu, nseg), dtype=np.int32 if is_int else np.float64)
            setattr(res, name, a)
            setattr(r, name, _ip(a) if is_int else _dp(a))
    return res, r


def _segment_struct(out: dict):
    r = _lib.MpctSegmentResult()
    for name, _, is_int in _lib.SEGMENT_FIELDS:
        setattr(r, name, _tptr(out.get(name), _lib.c_int32_p if is_int else _lib.c_double_p))
    return r


def segment_indices(y, u, r, tseg, base=1, band_rel=0.02, band_abs=0.0, rise_lo=0.1, rise_hi=0.9, fields=None,
                    device=-1) -> SegmentResult:
    """mpct_segment_indices: the step-response indices per setpoint segment of stored trajectories, reduced on
    the GPU (host arrays in and out).  ``y`` (S, my, nit), ``u`` (S, nu, nit), ``r`` (nref, my, nit); simulation
    s reads reference set s % nref; ``tseg`` the nseg + 1 boundaries (``reference_segments``).  ``y`` and ``r``
    may be None when ``fields`` names no output-row field, ``u`` when it names no input-row field.  The arrays
    of the result are (S / nref, nref, my, nseg) and (S / nref, nref, nu, nseg)."""
    y = None if y is None else np.ascontiguousarray(y, dtype=np.float64)
    u = None if u is None else np.ascontiguousarray(u, dtype=np.float64)
    r = None if r is None else np.ascontiguousarray(r, dtype=np.float64)
    if (y is not None and y.ndim != 3) or (u is not None and u.ndim != 3) or (r is not None and r.ndim != 3):
        raise ValueError("y, u and r must be 3-d: (S, my, nit), (S, nu, nit), (nref, my, nit)")
    if y is None and u is None:
        raise ValueError("y or u is needed")
    some = y if y is not None else u
    S, nit = some.shape[0], some.shape[2]
    my = y.shape[1] if y is not None else 0
    nu = u.shape[1] if u is not None else 0
    nref = r.shape[0] if r is not None else 1
    if (u is not None and u.shape[::2] != (S, nit)) or (r is not None and y is not None and r.shape[1:] != (my, nit)):
        raise ValueError("y, u and r disagree on S, my or nit")
    if fields is None:
        fields = tuple(n for n, is_y, _ in _lib.SEGMENT_FIELDS if (y if is_y else u) is not None)
    fields = _segment_fields(fields)
    if S % nref:
        raise ValueError("S must be a multiple of nref")
    p, t = _segment_params(tseg, base, band_rel, band_abs, rise_lo, rise_hi)
    res, out = _segment_result(S // nref, nref, my, nu, t, fields)
    ptr = lambda a: a.ctypes.data if a is not None else None  # noqa: E731
    rc = _lib.load().mpct_segment_indices(ptr(y), ptr(u), ptr(r), S, nref, my, nu, nit, C.byref(p), int(device),
                                          C.byref(out))
    if rc != 0:
        raise MpctError("mpct_segment_indices failed (%d): %s" % (rc, _lib.last_error()))
    return res


def segment_indices_device(y, u, r, out: dict, tseg, base=1, band_rel=0.02, band_abs=0.0, rise_lo=0.1, rise_hi=0.9):
    """mpct_segment_indices_device: ``y`` [S, my, nit], ``u`` [S, nu, nit], ``r`` [nref, my, nit] are contiguous
    float64 CUDA (HIP) tensors (None where no field needs them), ``tseg`` a HOST sequence; the records are
    written into the tensors of ``out`` (keys as the fields of SegmentResult: float64 / int32, [S, my, nseg] or
    [S, nu, nseg]; any may be absent).  Enqueued on the current torch stream of the tensors' device and not
    synchronised."""
    import torch

    some = y if y is not None else u
    for t in (y, u, r):
        if t is not None and (t.dtype != torch.float64 or t.dim() != 3 or not t.is_contiguous()):
            raise ValueError("y, u and r must be contiguous float64 tensors with three dimensions")
    S, nit = some.shape[0], some.shape[2]
    my = y.shape[1] if y is not None else 0
    nu = u.shape[1] if u is not None else 0
    nref = r.shape[0] if r is not None else 1
    p, keep = _segment_params(tseg, base, band_rel, band_abs, rise_lo, rise_hi)
    o = _segment_struct(out)
    stream = torch.cuda.current_stream(some.device).cuda_stream
    ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None  # noqa: E731
    with torch.cuda.device(some.device):
        rc = _lib.load().mpct_segment_indices_device(ptr(y), ptr(u), ptr(r), S, nref, my, nu, nit, C.byref(p), C.byref(o),
                                                     C.c_void_p(stream))
    del keep
    if rc != 0:
        raise MpctError("mpct_segment_indices_device failed (%d): %s" % (rc, _lib.last_error()))


def eval_segment_indices(sc, N2, Nu, delta, lam, refs, v=None, tseg=None, extra=(), base=1, band_rel=0.02, band_abs=0.0,
                         rise_lo=0.1, rise_hi=0.9, fields=None, want_costs=False, device=-1, max_qp_iter=0,
                         feas_tol=0.0) -> SegmentResult:
    """mpct_eval_segment_indices: score C candidates against nref reference sets and return only the segment
    records of the closed loops (host arrays in and out); the trajectories stay on the device.  ``tseg``
    defaults to ``reference_segments(refs, extra)``.  ``want_costs`` adds ``batch``: J1, j22, status and
    qp_iters of the same launch, as eval_batch returns them."""
    fields = _segment_fields(fields)
    N2, Nu, delta, lam, refs, Cn, nref, vv = _batch_args(sc, N2, Nu, delta, lam, refs, v)
    if tseg is None:
        tseg = reference_segments(refs, extra)
    p, t = _segment_params(tseg, base, band_rel, band_abs, rise_lo, rise_hi)
    res, out = _segment_result(Cn, nref, sc.my, sc.nu, t, fields)
    br = None
    if want_costs:
        res.batch, br = _eval_result(sc, Cn * nref, nref, False, False)
    o = _opts(False, False, device, max_qp_iter, feas_tol)
    rc = sc.lib.mpct_eval_segment_indices(sc.handle, Cn, N2.ctypes.data, Nu.ctypes.data, delta.ctypes.data,
                                          lam.ctypes.data, nref, refs.ctypes.data, vv.ctypes.data if vv is not None else None,
                                          C.byref(o), C.byref(p), C.byref(br) if br is not None else None, C.byref(out))
    if rc != 0:
        raise MpctError("mpct_eval_segment_indices failed (%d): %s" % (rc, _lib.last_error()))
    return res


def eval_segment_indices_device(sc, N2, Nu, delta, lam, refs, out: dict, tseg, v=None, base=1, band_rel=0.02,
                                band_abs=0.0, rise_lo=0.1, rise_hi=0.9, device=-1, stream=None):
    """Device-pointer entry of eval_segment_indices: every argument is a CUDA (HIP) torch tensor (``tseg`` is a
    HOST sequence); the records are written into the tensors of ``out`` (the keys of segment_indices_device,
    [C * nref, my, nseg] / [C * nref, nu, nseg], plus the optional J1, j21, j22, Jnu, status, qp_iters of
    eval_batch_device).  Enqueued on ``stream`` (torch stream; default: current) and not synchronised."""
    import torch

    if stream is None:
        stream = torch.cuda.current_stream()
    br = _lib.MpctResult()
    br.J1, br.j21 = _tptr(out.get("J1"), _lib.c_double_p), _tptr(out.get("j21"), _lib.c_double_p)
    br.j22, br.Jnu = _tptr(out.get("j22"), _lib.c_double_p), _tptr(out.get("Jnu"), _lib.c_double_p)
    br.status, br.qp_iters = _tptr(out.get("status"), _lib.c_int32_p), _tptr(out.get("qp_iters"), _lib.c_int64_p)
    p, keep = _segment_params(tseg, base, band_rel, band_abs, rise_lo, rise_hi)
    o = _opts(False, False, device)
    so = _segment_struct(out)
    rc = sc.lib.mpct_eval_segment_indices_device(
        sc.handle, N2.numel(), C.c_void_p(N2.data_ptr()), C.c_void_p(Nu.data_ptr()), C.c_void_p(delta.data_ptr()),
        C.c_void_p(lam.data_ptr()), refs.shape[0], C.c_void_p(refs.data_ptr()),
        C.c_void_p(v.data_ptr()) if v is not None else None, C.byref(o), C.byref(p), C.byref(br), C.byref(so),
        C.c_void_p(stream.cuda_stream))
    del keep
    if rc != 0:
        raise MpctError("mpct_eval_segment_indices_device failed (%d): %s" % (rc, _lib.last_error()))


@dataclass
class RobustSegmentResult(RobustIndexResult):
    """RobustIndexResult for the segment indices: ``columns`` names the W columns as (field name, channel,
    segment) in selection order, an output-row field contributing my * nseg columns and an input-row field
    nu * nseg; ``tseg`` the boundaries."""
    tseg: np.ndarray | None = None

    def costs(self, stat="hi", names=None, segments=None, max_failed: int = 0) -> np.ndarray:
        """(C, k) cost table for ``pareto``: the statistic ``stat`` (as RobustIndexResult.costs) of the columns
        whose field is in ``names`` (None: every field) and whose segment is in ``segments`` (None: every
        segment), in selection order.  NaN for every candidate with more than ``max_failed`` failed draws."""
        cols, self.columns = self.columns, [(f, (ch, g)) for f, ch, g in self.columns]
        try:
            tab = RobustIndexResult.costs(self, stat, None, max_failed)
        finally:
            self.columns = cols
        if names is not None:
            for nm in names:
                if not any(f == nm for f, _, _ in cols):
                    raise ValueError("this result has no field %r" % (nm,))
        seg = None if segments is None else set(int(g) for g in segments)
        order = [k for nm in (names if names is not None else dict.fromkeys(f for f, _, _ in cols))
                 for k, (f, _, g) in enumerate(cols) if f == nm and (seg is None or g in seg)]
        return tab[:, order]


def _segment_field_ids(sc, fields, nseg):
    """The MPCT_SX_* ids of the selected fields as the int32 vector the library reads, and the (field, channel,
    segment) columns."""
    fields = _segment_fields(fields)
    ids = np.ascontiguousarray([SEGMENT_FIELDS.index(f) for f in fields], dtype=np.int32)
    is_y = {n: y for n, y, _ in _lib.SEGMENT_FIELDS}
    cols = [(f, ch, g) for f in fields for ch in range(sc.my if is_y[f] else sc.nu) for g in range(nseg)]
    return ids, cols


def eval_robust_segment_indices(sc, N2, Nu, delta, lam, refs, v=None, tseg=None, extra=(), fields=None, levels=None,
                                j_bound=0.0, base=1, band_rel=0.02, band_abs=0.0, rise_lo=0.1, rise_hi=0.9, device=-1,
                                max_qp_iter=0, feas_tol=0.0) -> RobustSegmentResult:
    """mpct_eval_robust_segment_indices: score C candidates over the D = len(refs) draws and reduce, on the
    device, the segment indices ``fields`` (default: all fifteen) of the C x D closed loops to per-candidate
    statistics over the surviving draws (host arrays in and out): eval_robust_indices per segment.  A draw
    without a value in a column (an invalid unit, or a rise of -1: no step) does not enter that column.
    ``base`` here is the base-level rule of the segments; the robust J1 record is the result's ``.base``."""
    N2, Nu, delta, lam, refs, Cn, D, vv = _batch_args(sc, N2, Nu, delta, lam, refs, v)
    if tseg is None:
        tseg = reference_segments(refs, extra)
    p, t = _segment_params(tseg, base, band_rel, band_abs, rise_lo, rise_hi)
    ids, cols = _segment_field_ids(sc, fields, t.size - 1)
    lv = _levels(levels) if levels is not None else None
    nlev = 0 if lv is None else lv.size
    arr, out = _stats_arrays(Cn, len(cols), nlev)
    rb = RobustResult(mean=np.zeros((Cn, sc.my)), worst=np.zeros((Cn, sc.my)), n_failed=np.zeros(Cn, dtype=np.int32),
                      worst_draw=np.zeros(Cn, dtype=np.int32), status=np.zeros(Cn, dtype=np.int32), draws=D)
    br = _lib.MpctRobustResult()
    br.mean, br.worst = _dp(rb.mean), _dp(rb.worst)
    br.n_failed, br.worst_draw, br.status = _ip(rb.n_failed), _ip(rb.worst_draw), _ip(rb.status)
    o = _opts(False, False, device, max_qp_iter, feas_tol)
    rc = sc.lib.mpct_eval_robust_segment_indices(
        sc.handle, Cn, N2.ctypes.data, Nu.ctypes.data, delta.ctypes.data, lam.ctypes.data, D, refs.ctypes.data,
        vv.ctypes.data if vv is not None else None, float(j_bound), C.byref(o), C.byref(p), ids.size, _ip(ids), nlev,
        _dp(lv) if nlev else None, C.byref(br), C.byref(out))
    if rc != 0:
        raise MpctError("mpct_eval_robust_segment_indices failed (%d): %s" % (rc, _lib.last_error()))
    return RobustSegmentResult(columns=cols, levels=lv, base=rb, tseg=t.copy(), **arr)


def eval_robust_segment_indices_device(sc, N2, Nu, delta, lam, refs, out: dict, tseg, base_out: dict | None = None, v=None,
                                       fields=None, levels=None, j_bound=0.0, base=1, band_rel=0.02, band_abs=0.0,
                                       rise_lo=0.1, rise_hi=0.9, device=-1, stream=None):
    """Device-pointer entry of eval_robust_segment_indices: every argument is a CUDA (HIP) torch tensor
    (``tseg``, ``fields`` and ``levels`` are HOST sequences); ``out`` as in eval_robust_indices_device, and
    ``base_out`` its ``base`` (the tensors of the robust J1 record).  Enqueued on ``stream`` (torch stream;
    default: current) and not synchronised."""
    import torch

    if stream is None:
        stream = torch.cuda.current_stream()
    p, keep = _segment_params(tseg, base, band_rel, band_abs, rise_lo, rise_hi)
    ids, _ = _segment_field_ids(sc, fields, keep.size - 1)
    lv = _levels(levels) if levels is not None else None
    nlev = 0 if lv is None else lv.size
    br = _robust_struct(base_out or {})
    o = _opts(False, False, device)
    so = _stats_struct(out)
    rc = sc.lib.mpct_eval_robust_segment_indices_device(
        sc.handle, N2.numel(), C.c_void_p(N2.data_ptr()), C.c_void_p(Nu.data_ptr()), C.c_void_p(delta.data_ptr()),
        C.c_void_p(lam.data_ptr()), refs.shape[0], C.c_void_p(refs.data_ptr()),
        C.c_void_p(v.data_ptr()) if v is not None else None, float(j_bound), C.byref(o), C.byref(p), ids.size, _ip(ids),
        nlev, _dp(lv) if nlev else None, C.byref(br), C.byref(so), C.c_void_p(stream.cuda_stream))
    del keep
    if rc != 0:
        raise MpctError("mpct_eval_robust_segment_indices_device failed (%d): %s" % (rc, _lib.last_error()))


# --------------------------------------------------------------------------------------------
# oscillation indices per setpoint segment and their statistics over the draws (mpct_osc_indices,
# mpct_eval_osc_indices, mpct_eval_robust_osc_indices; include/mpct.h)
OSC_FIELDS = tuple(n for n, _, _ in _lib.OSC_FIELDS)


@dataclass
class OscResult:
    """One array per field of mpct_osc_result: the output-row fields (C, nref, my, nseg), the input-row fields
    (C, nref, nu, nseg); a field that was not asked for is None.  An invalid unit (a non-finite sample the
    segment reads) holds NaN / -1."""
    ncross: np.ndarray | None = None     # band crossings of the output in the segment
    decay: np.ndarray | None = None      # A_{k0+2} / A_{k0}; +0.0 = no second peak on the same side
    period: np.ndarray | None = None     # T_{k0+2} - T_{k0} in samples; -1 = no second peak on the same side
    a_last: np.ndarray | None = None     # the peak of the last lobe
    nmove: np.ndarray | None = None      # moves outside the dead zone rev_tol
    nrev: np.ndarray | None = None       # direction reversals among them
    t_rev: np.ndarray | None = None      # an absolute sample; -1 = no reversal
    tseg: np.ndarray | None = None
    batch: EvalResult | None = None      # eval_osc_indices(want_costs=True): J1, j22, status, qp_iters of the same launch

    def costs(self, names, segments=None, reduce: str = "max") -> np.ndarray:
        """(C, len(names)) float matrix for ``pareto``: each named field folded over the references, the
        channels and the ``segments`` (None: all) by ``reduce`` ('max' or 'sum').  The integer fields enter as
        floats, ``t_rev`` as samples after the segment's start.  A candidate with an invalid unit (NaN / -1)
        gets NaN in that column, and so does one with a ``period`` or a ``t_rev`` of -1 (no second peak, no
        reversal: no value): invalid for ``pareto``, last for ``rank``."""
        tseg = np.asarray(self.tseg)
        a = tseg[:-1].astype(float)

        def get(name):
            if name not in OSC_FIELDS:
                raise ValueError("unknown oscillation field %r" % (name,))
            arr = getattr(self, name)
            if arr is None:
                raise ValueError("this result has no %s" % name)
            arr = np.asarray(arr)
            x = arr.reshape(arr.shape[0], -1, arr.shape[-1]).astype(float)
            if arr.dtype.kind == "i":
                x = np.where(x < 0, np.nan, x - a if name == "t_rev" else x)
            return x

        return _segment_cost_table(get, names, tseg, segments, reduce)

    def goal_attain(self, names, goals, weights, n_best: int = 1, device: int = -1, **kw):
        """Goal-attainment selection (``goal_attain``) over the table ``costs(names, **kw)`` returns."""
        return goal_attain(self.costs(names, **kw), goals, weights, n_best=n_best, device=device)


def _osc_fields(fields):
    fields = OSC_FIELDS if fields is None else tuple(fields)
    for f in fields:
        if f not in OSC_FIELDS:
            raise ValueError("unknown oscillation field %r" % (f,))
    return fields


def _osc_params(tseg, base, band_rel, band_abs, rev_tol):
    """The MpctOscParams of a call and the host boundary vector it points to (keep it alive for the call)."""
    t = np.ascontiguousarray(np.asarray(tseg, dtype=np.int32).reshape(-1))
    if t.size < 2:
        raise ValueError("tseg needs at least two boundaries")
    p = _lib.MpctOscParams(t.size - 1, _ip(t), int(base), float(band_rel), float(band_abs), float(rev_tol))
    return p, t


def _osc_result(Cn, nref, my, nu, tseg, fields):
    """An OscResult with the arrays of ``fields`` and the MpctOscResult that points into them."""
    nseg = len(tseg) - 1
    res = OscResult(tseg=np.array(tseg, dtype=np.int32))
    r = _lib.MpctOscResult()
    for name, is_y, is_int in _lib.OSC_FIELDS:
        if name in fields:
            a = np.zeros((Cn, nref, my if is_y else nu, nseg), dtype=np.int32 if is_int else np.float64)
            setattr(res, name, a)
            setattr(r, name, _ip(a) if is_int else _dp(a))
    return res, r


def _osc_struct(out: dict):
    r = _lib.MpctOscResult()
    for name, _, is_int in _lib.OSC_FIELDS:
        setattr(r, name, _tptr(out.get(name), _lib.c_int32_p if is_int else _lib.c_double_p))
    return r


def osc_indices(y, u, r, tseg, base=1, band_rel=0.02, band_abs=0.0, rev_tol=0.0, fields=None, device=-1) -> OscResult:
    """mpct_osc_indices: the oscillation indices per setpoint segment of stored trajectories, reduced on the
    GPU (host arrays in and out).  ``y`` (S, my, nit), ``u`` (S, nu, nit), ``r`` (nref, my, nit); simulation s
    reads reference set s % nref; ``tseg`` the nseg + 1 boundaries (``reference_segments``).  ``y`` and ``r``
    may be None when ``fields`` names no output-row field, ``u`` when it names no input-row field.  The arrays
    of the result are (S / nref, nref, my, nseg) and (S / nref, nref, nu, nseg)."""
    y = None if y is None else np.ascontiguousarray(y, dtype=np.float64)
    u = None if u is None else np.ascontiguousarray(u, dtype=np.float64)
    r = None if r is None else np.ascontiguousarray(r, dtype=np.float64)
    if (y is not None and y.ndim != 3) or (u is not None and u.ndim != 3) or (r is not None and r.ndim != 3):
        raise ValueError("y, u and r must be 3-d: (S, my, nit), (S, nu, nit), (nref, my, nit)")
    if y is None and u is None:
        raise ValueError("y or u is needed")
    some = y if y is not None else u
    S, nit = some.shape[0], some.shape[2]
    my = y.shape[1] if y is not None else 0
    nu = u.shape[1] if u is not None else 0
    nref = r.shape[0] if r is not None else 1
    if (u is not None and u.shape[::2] != (S, nit)) or (r is not None and y is not None and r.shape[1:] != (my, nit)):
        raise ValueError("y, u and r disagree on S, my or nit")
    if fields is None:
        fields = tuple(n for n, is_y, _ in _lib.OSC_FIELDS if (y if is_y else u) is not None)
    fields = _osc_fields(fields)
    if S % nref:
        raise ValueError("S must be a multiple of nref")
    p, t = _osc_params(tseg, base, band_rel, band_abs, rev_tol)
    res, out = _osc_result(S // nref, nref, my, nu, t, fields)
    ptr = lambda a: a.ctypes.data if a is not None else None  # noqa: E731
    rc = _lib.load().mpct_osc_indices(ptr(y), ptr(u), ptr(r), S, nref, my, nu, nit, C.byref(p), int(device), C.byref(out))
    if rc != 0:
        raise MpctError("mpct_osc_indices failed (%d): %s" % (rc, _lib.last_error()))
    return res


def osc_indices_device(y, u, r, out: dict, tseg, base=1, band_rel=0.02, band_abs=0.0, rev_tol=0.0):
    """mpct_osc_indices_device: ``y`` [S, my, nit], ``u`` [S, nu, nit], ``r`` [nref, my, nit] are contiguous
    float64 CUDA (HIP) tensors (None where no field needs them), ``tseg`` a HOST sequence; the records are
    written into the tensors of ``out`` (keys as the fields of OscResult: float64 / int32, [S, my, nseg] or
    [S, nu, nseg]; any may be absent).  Enqueued on the current torch stream of the tensors' device and not
    synchronised."""
    import torch

    some = y if y is not None else u
    for t in (y, u, r):
        if t is not None and (t.dtype != torch.float64 or t.dim() != 3 or not t.is_contiguous()):
            raise ValueError("y, u and r must be contiguous float64 tensors with three dimensions")
    S, nit = some.shape[0], some.shape[2]
    my = y.shape[1] if y is not None else 0
    nu = u.shape[1] if u is not None else 0
    nref = r.shape[0] if r is not None else 1
    p, keep = _osc_params(tseg, base, band_rel, band_abs, rev_tol)
    o = _osc_struct(out)
    stream = torch.cuda.current_stream(some.device).cuda_stream
    ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None  # noqa: E731
    with torch.cuda.device(some.device):
        rc = _lib.load().mpct_osc_indices_device(ptr(y), ptr(u), ptr(r), S, nref, my, nu, nit, C.byref(p), C.byref(o),
                                                 C.c_void_p(stream))
    del keep
    if rc != 0:
        raise MpctError("mpct_osc_indices_device failed (%d): %s" % (rc, _lib.last_error()))


def eval_osc_indices(sc, N2, Nu, delta, lam, refs, v=None, tseg=None, extra=(), base=1, band_rel=0.02, band_abs=0.0,
                     rev_tol=0.0, fields=None, want_costs=False, device=-1, max_qp_iter=0, feas_tol=0.0) -> OscResult:
    """mpct_eval_osc_indices: score C candidates against nref reference sets and return only the oscillation
    records of the closed loops (host arrays in and out); the trajectories stay on the device.  ``tseg``
    defaults to ``reference_segments(refs, extra)``.  ``want_costs`` adds ``batch``: J1, j22, status and
    qp_iters of the same launch, as eval_batch returns them."""
    fields = _osc_fields(fields)
    N2, Nu, delta, lam, refs, Cn, nref, vv = _batch_args(sc, N2, Nu, delta, lam, refs, v)
    if tseg is None:
        tseg = reference_segments(refs, extra)
    p, t = _osc_params(tseg, base, band_rel, band_abs, rev_tol)
    res, out = _osc_result(Cn, nref, sc.my, sc.nu, t, fields)
    br = None
    if want_costs:
        res.batch, br = _eval_result(sc, Cn * nref, nref, False, False)
    o = _opts(False, False, device, max_qp_iter, feas_tol)
    rc = sc.lib.mpct_eval_osc_indices(sc.handle, Cn, N2.ctypes.data, Nu.ctypes.data, delta.ctypes.data, lam.ctypes.data,
                                      nref, refs.ctypes.data, vv.ctypes.data if vv is not None else None, C.byref(o),
                                      C.byref(p), C.byref(br) if br is not None else None, C.byref(out))
    if rc != 0:
        raise MpctError("mpct_eval_osc_indices failed (%d): %s" % (rc, _lib.last_error()))
    return res


def eval_osc_indices_device(sc, N2, Nu, delta, lam, refs, out: dict, tseg, v=None, base=1, band_rel=0.02, band_abs=0.0,
                            rev_tol=0.0, device=-1, stream=None):
    """Device-pointer entry of eval_osc_indices: every argument is a CUDA (HIP) torch tensor (``tseg`` is a
    HOST sequence); the records are written into the tensors of ``out`` (the keys of osc_indices_device,
    [C * nref, my, nseg] / [C * nref, nu, nseg], plus the optional J1, j21, j22, Jnu, status, qp_iters of
    eval_batch_device).  Enqueued on ``stream`` (torch stream; default: current) and not synchronised."""
    import torch

    if stream is None:
        stream = torch.cuda.current_stream()
    br = _lib.MpctResult()
    br.J1, br.j21 = _tptr(out.get("J1"), _lib.c_double_p), _tptr(out.get("j21"), _lib.c_double_p)
    br.j22, br.Jnu = _tptr(out.get("j22"), _lib.c_double_p), _tptr(out.get("Jnu"), _lib.c_double_p)
    br.status, br.qp_iters = _tptr(out.get("status"), _lib.c_int32_p), _tptr(out.get("qp_iters"), _lib.c_int64_p)
    p, keep = _osc_params(tseg, base, band_rel, band_abs, rev_tol)
    o = _opts(False, False, device)
    so = _osc_struct(out)
    rc = sc.lib.mpct_eval_osc_indices_device(
        sc.handle, N2.numel(), C.c_void_p(N2.data_ptr()), C.c_void_p(Nu.data_ptr()), C.c_void_p(delta.data_ptr()),
        C.c_void_p(lam.data_ptr()), refs.shape[0], C.c_void_p(refs.data_ptr()),
        C.c_void_p(v.data_ptr()) if v is not None else None, C.byref(o), C.byref(p), C.byref(br), C.byref(so),
        C.c_void_p(stream.cuda_stream))
    del keep
    if rc != 0:
        raise MpctError("mpct_eval_osc_indices_device failed (%d): %s" % (rc, _lib.last_error()))


def _osc_field_ids(sc, fields, nseg):
    """The MPCT_OX_* ids of the selected fields as the int32 vector the library reads, and the (field, channel,
    segment) columns."""
    fields = _osc_fields(fields)
    ids = np.ascontiguousarray([OSC_FIELDS.index(f) for f in fields], dtype=np.int32)
    is_y = {n: y for n, y, _ in _lib.OSC_FIELDS}
    cols = [(f, ch, g) for f in fields for ch in range(sc.my if is_y[f] else sc.nu) for g in range(nseg)]
    return ids, cols


def eval_robust_osc_indices(sc, N2, Nu, delta, lam, refs, v=None, tseg=None, extra=(), fields=None, levels=None,
                            j_bound=0.0, base=1, band_rel=0.02, band_abs=0.0, rev_tol=0.0, device=-1, max_qp_iter=0,
                            feas_tol=0.0) -> RobustSegmentResult:
    """mpct_eval_robust_osc_indices: score C candidates over the D = len(refs) draws and reduce, on the device,
    the oscillation indices ``fields`` (default: all seven) of the C x D closed loops to per-candidate
    statistics over the surviving draws (host arrays in and out): eval_robust_segment_indices for the
    oscillation fields, returned as a RobustSegmentResult (``.costs(stat, names, segments)``).  A draw without
    a value in a column (an invalid unit, a period or a t_rev of -1) does not enter that column.  ``base``
    here is the base-level rule of the segments; the robust J1 record is the result's ``.base``."""
    N2, Nu, delta, lam, refs, Cn, D, vv = _batch_args(sc, N2, Nu, delta, lam, refs, v)
    if tseg is None:
        tseg = reference_segments(refs, extra)
    p, t = _osc_params(tseg, base, band_rel, band_abs, rev_tol)
    ids, cols = _osc_field_ids(sc, fields, t.size - 1)
    lv = _levels(levels) if levels is not None else None
    nlev = 0 if lv is None else lv.size
    arr, out = _stats_arrays(Cn, len(cols), nlev)
    rb = RobustResult(mean=np.zeros((Cn, sc.my)), worst=np.zeros((Cn, sc.my)), n_failed=np.zeros(Cn, dtype=np.int32),
                      worst_draw=np.zeros(Cn, dtype=np.int32), status=np.zeros(Cn, dtype=np.int32), draws=D)
    br = _lib.MpctRobustResult()
    br.mean, br.worst = _dp(rb.mean), _dp(rb.worst)
    br.n_failed, br.worst_draw, br.status = _ip(rb.n_failed), _ip(rb.worst_draw), _ip(rb.status)
    o = _opts(False, False, device, max_qp_iter, feas_tol)
    rc = sc.lib.mpct_eval_robust_osc_indices(
        sc.handle, Cn, N2.ctypes.data, Nu.ctypes.data, delta.ctypes.data, lam.ctypes.data, D, refs.ctypes.data,
        vv.ctypes.data if vv is not None else None, float(j_bound), C.byref(o), C.byref(p), ids.size, _ip(ids), nlev,
        _dp(lv) if nlev else None, C.byref(br), C.byref(out))
    if rc != 0:
        raise MpctError("mpct_eval_robust_osc_indices failed (%d): %s" % (rc, _lib.last_error()))
    return RobustSegmentResult(columns=cols, levels=lv, base=rb, tseg=t.copy(), **arr)


def eval_robust_osc_indices_device(sc, N2, Nu, delta, lam, refs, out: dict, tseg, base_out: dict | None = None, v=None,
                                   fields=None, levels=None, j_bound=0.0, base=1, band_rel=0.02, band_abs=0.0,
                                   rev_tol=0.0, device=-1, stream=None):
    """Device-pointer entry of eval_robust_osc_indices: every argument is a CUDA (HIP) torch tensor (``tseg``,
    ``fields`` and ``levels`` are HOST sequences); ``out`` as in eval_robust_indices_device, and ``base_out``
    its ``base`` (the tensors of the robust J1 record).  Enqueued on ``stream`` (torch stream; default:
    current) and not synchronised."""
    import torch

    if stream is None:
        stream = torch.cuda.current_stream()
    p, keep = _osc_params(tseg, base, band_rel, band_abs, rev_tol)
    ids, _ = _osc_field_ids(sc, fields, keep.size - 1)
    lv = _levels(levels) if levels is not None else None
    nlev = 0 if lv is None else lv.size
    br = _robust_struct(base_out or {})
    o = _opts(False, False, device)
    so = _stats_struct(out)
    rc = sc.lib.mpct_eval_robust_osc_indices_device(
        sc.handle, N2.numel(), C.c_void_p(N2.data_ptr()), C.c_void_p(Nu.data_ptr()), C.c_void_p(delta.data_ptr()),
        C.c_void_p(lam.data_ptr()), refs.shape[0], C.c_void_p(refs.data_ptr()),
        C.c_void_p(v.data_ptr()) if v is not None else None, float(j_bound), C.byref(o), C.byref(p), ids.size, _ip(ids),
        nlev, _dp(lv) if nlev else None, C.byref(br), C.byref(so), C.c_void_p(stream.cuda_stream))
    del keep
    if rc != 0:
        raise MpctError("mpct_eval_robust_osc_indices_device failed (%d): %s" % (rc, _lib.last_error()))
