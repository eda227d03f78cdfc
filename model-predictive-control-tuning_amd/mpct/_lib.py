"""ctypes binding of libmpct.so (include/mpct.h).  The product path has NO CPU fallback: if the
HIP library is missing, importing the engine raises."""
from __future__ import annotations

import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
_PKG = os.path.dirname(_HERE)
_CANDIDATES = ([os.environ["MPCT_LIB"]] if os.environ.get("MPCT_LIB") else []) + [
    os.path.join(_PKG, "csrc", "libmpct.so"),
    os.path.join(_HERE, "libmpct.so"),
]

c_int32_p = C.POINTER(C.c_int32)
c_double_p = C.POINTER(C.c_double)
c_int64_p = C.POINTER(C.c_int64)


class MpctDtf(C.Structure):
    _fields_ = [("len", C.c_int32), ("num", c_double_p), ("den", c_double_p), ("delay", C.c_int32)]


class MpctScenarioDesc(C.Structure):
    _fields_ = [
        ("abi_version", C.c_int32),
        ("my", C.c_int32), ("nu", C.c_int32), ("nd", C.c_int32),
        ("nit", C.c_int32),
        ("n2_max", C.c_int32), ("nu_max", C.c_int32),
        ("weights_squared", C.c_int32),
        ("vns_ink", C.c_int32),
        ("n1", c_int32_p),
        ("plant", C.POINTER(MpctDtf)),
        ("model", C.POINTER(MpctDtf)),
        ("na", c_int32_p),
        ("carima_A", c_double_p),
        ("nb", c_int32_p),
        ("carima_B", c_double_p),
        ("dp", c_int32_p),
        ("du_min", c_double_p), ("du_max", c_double_p),
        ("u_min", c_double_p), ("u_max", c_double_p),
        ("yref", c_double_p),
        ("dtc", C.c_int32),
        ("filter", C.POINTER(MpctDtf)),
        ("nq", C.c_int32),
        ("dist", C.POINTER(MpctDtf)),
        ("nplant", C.c_int32),
        ("plant_var", C.POINTER(MpctDtf)),
        ("mdband", C.c_int32),
        ("y_min", c_double_p), ("y_max", c_double_p),
        ("ecr_min", c_double_p), ("ecr_max", c_double_p),
        ("y_scale", c_double_p), ("u_scale", c_double_p),
        ("rho_ecr", C.c_double),
    ]


class MpctNmpcDesc(C.Structure):
    _fields_ = [
        ("abi_version", C.c_int32), ("model", C.c_int32),
        ("nx", C.c_int32), ("ny", C.c_int32), ("nu", C.c_int32),
        ("params", c_double_p), ("xc", c_int32_p),
        ("ts", C.c_double), ("nsub", C.c_int32),
        ("x0", c_double_p), ("u0", c_double_p),
        ("u_min", c_double_p), ("u_max", c_double_p),
        ("x_min", c_double_p), ("x_max", c_double_p),
        ("y_scale", c_double_p), ("u_scale", c_double_p),
        ("n_max", C.c_int32), ("nu_max", C.c_int32),
        ("nit", C.c_int32), ("yref", c_double_p), ("vns_ink", C.c_int32),
        ("sqp_max", C.c_int32), ("sqp_tol", C.c_double),
    ]


class MpctOpts(C.Structure):
    _fields_ = [("open_loop", C.c_int32), ("want_traj", C.c_int32), ("max_qp_iter", C.c_int32),
                ("device", C.c_int32), ("feas_tol", C.c_double)]


class MpctResult(C.Structure):
    _fields_ = [("J1", c_double_p), ("j21", c_double_p), ("j22", c_double_p), ("Jnu", c_double_p),
                ("status", c_int32_p), ("qp_iters", c_int64_p),
                ("y", c_double_p), ("u", c_double_p), ("ys", c_double_p), ("uopt", c_double_p)]


class MpctRobustResult(C.Structure):
    _fields_ = [("mean", c_double_p), ("worst", c_double_p), ("n_failed", c_int32_p), ("worst_draw", c_int32_p),
                ("status", c_int32_p), ("J1", c_double_p)]


class MpctParetoResult(C.Structure):
    _fields_ = [("dom_count", c_int32_p), ("layer", c_int32_p), ("front", c_int32_p), ("n_front", c_int32_p)]


class MpctGoalResult(C.Structure):
    _fields_ = [("best", c_int32_p), ("gamma", c_double_p), ("active", c_int32_p), ("n_feasible", c_int32_p),
                ("n_attained", c_int32_p), ("wins", c_int32_p)]


class MpctHvResult(C.Structure):
    _fields_ = [("n_covered", c_int64_p), ("excl", c_int64_p), ("depth_hist", c_int64_p), ("hv", c_double_p)]


class MpctHvSelectResult(C.Structure):
    _fields_ = [("n_picked", c_int64_p), ("pos", c_int32_p), ("index", c_int32_p), ("gain", c_int64_p),
                ("covered", c_int64_p), ("hv", c_double_p), ("ties", c_int32_p), ("n_covered_all", c_int64_p)]


class MpctHvxResult(C.Structure):
    _fields_ = [("hv", c_double_p), ("excl", c_double_p), ("n_active", c_int64_p)]


class MpctIndexParams(C.Structure):
    _fields_ = [("t0", C.c_int32), ("band_rel", C.c_double), ("band_abs", C.c_double)]


# the fields of mpct_index_result in the struct's order: (name, per output row?, integer?)
INDEX_FIELDS = [("iae", True, False), ("ise", True, False), ("itae", True, False), ("emax", True, False),
                ("t_emax", True, True), ("over", True, False), ("e_final", True, False), ("settle", True, True),
                ("tv", False, False), ("du2", False, False), ("dumax", False, False), ("u_lo", False, False),
                ("u_hi", False, False)]


class MpctIndexResult(C.Structure):
    _fields_ = [(n, c_int32_p if i else c_double_p) for n, _, i in INDEX_FIELDS]


class MpctLimitParams(C.Structure):
    _fields_ = [("t0", C.c_int32), ("out_tol", C.c_double), ("sat_tol", C.c_double),
                ("y_lo", c_double_p), ("y_hi", c_double_p), ("u_lo", c_double_p), ("u_hi", c_double_p),
                ("du_lo", c_double_p), ("du_hi", c_double_p)]


# the fields of mpct_limit_result in the struct's order (their positions are MPCT_LX_*): (name, per output row?, integer?)
LIMIT_FIELDS = [("viol", True, False), ("viol2", True, False), ("vmax", True, False), ("t_vmax", True, True),
                ("n_out", True, True), ("t_in", True, True), ("y_margin", True, False),
                ("n_lo", False, True), ("n_hi", False, True), ("n_rate", False, True), ("sat_run", False, True),
                ("u_margin", False, False), ("du_margin", False, False)]


class MpctLimitResult(C.Structure):
    _fields_ = [(n, c_int32_p if i else c_double_p) for n, _, i in LIMIT_FIELDS]


class MpctSegmentParams(C.Structure):
    _fields_ = [("nseg", C.c_int32), ("tseg", c_int32_p), ("base", C.c_int32), ("band_rel", C.c_double),
                ("band_abs", C.c_double), ("rise_lo", C.c_double), ("rise_hi", C.c_double)]


# the fields of mpct_segment_result in the struct's order (their positions are MPCT_SX_*): (name, per output row?, integer?)
SEGMENT_FIELDS = [("iae", True, False), ("ise", True, False), ("itae", True, False), ("emax", True, False),
                  ("t_emax", True, True), ("over", True, False), ("under", True, False), ("e_final", True, False),
                  ("settle", True, True), ("rise", True, True),
                  ("tv", False, False), ("du2", False, False), ("dumax", False, False), ("u_lo", False, False),
                  ("u_hi", False, False)]


class MpctSegmentResult(C.Structure):
    _fields_ = [(n, c_int32_p if i else c_double_p) for n, _, i in SEGMENT_FIELDS]


class MpctOscParams(C.Structure):
    _fields_ = [("nseg", C.c_int32), ("tseg", c_int32_p), ("base", C.c_int32), ("band_rel", C.c_double),
                ("band_abs", C.c_double), ("rev_tol", C.c_double)]


# the fields of mpct_osc_result in the struct's order (their positions are MPCT_OX_*): (name, per output row?, integer?)
OSC_FIELDS = [("ncross", True, True), ("decay", True, False), ("period", True, True), ("a_last", True, False),
              ("nmove", False, True), ("nrev", False, True), ("t_rev", False, True)]


class MpctOscResult(C.Structure):
    _fields_ = [(n, c_int32_p if i else c_double_p) for n, _, i in OSC_FIELDS]


class MpctRobustTail(C.Structure):
    _fields_ = [("quantile", c_double_p), ("cvar", c_double_p), ("q_draw", c_int32_p)]


# the fields of mpct_draw_stats_result in the struct's order: (name, integer?, per level?)
STATS_FIELDS = [("n", True, False), ("mean", False, False), ("lo", False, False), ("lo_draw", True, False),
                ("hi", False, False), ("hi_draw", True, False), ("quantile", False, True), ("cvar", False, True),
                ("q_draw", True, True)]


class MpctDrawStats(C.Structure):
    _fields_ = [(n, c_int32_p if i else c_double_p) for n, i, _ in STATS_FIELDS]


class MpctEnvelopeSpread(C.Structure):
    _fields_ = [("spread", c_double_p), ("spread_max", c_double_p), ("t_spread_max", c_int32_p)]


EXPORTS = [
    "mpct_abi_version", "mpct_last_error", "mpct_scenario_create", "mpct_scenario_destroy",
    "mpct_scenario_table", "mpct_eval_batch", "mpct_eval_batch_device", "mpct_lds_bytes", "mpct_lds_bytes_opts",
    "mpct_nmpc_scenario_create", "mpct_eval_batch_multi", "mpct_shard_candidates", "mpct_kernel_instance",
    "mpct_rank_device", "mpct_eval_robust", "mpct_eval_robust_device", "mpct_robust_instance",
    "mpct_scenario_create_est", "mpct_nmpc_scenario_create_var", "mpct_eval_robust_tail",
    "mpct_eval_robust_tail_device", "mpct_pareto_device", "mpct_pareto",
    "mpct_indices_device", "mpct_indices", "mpct_eval_indices", "mpct_eval_indices_device",
    "mpct_draw_stats_device", "mpct_draw_stats", "mpct_eval_robust_indices", "mpct_eval_robust_indices_device",
    "mpct_hypervolume_device", "mpct_hypervolume", "mpct_hv_select_device", "mpct_hv_select",
    "mpct_hypervolume_exact_device", "mpct_hypervolume_exact",
    "mpct_limit_indices_device", "mpct_limit_indices", "mpct_eval_limit_indices", "mpct_eval_limit_indices_device",
    "mpct_eval_robust_limit_indices", "mpct_eval_robust_limit_indices_device",
    "mpct_reference_segments", "mpct_segment_indices_device", "mpct_segment_indices", "mpct_eval_segment_indices",
    "mpct_eval_segment_indices_device", "mpct_eval_robust_segment_indices", "mpct_eval_robust_segment_indices_device",
    "mpct_osc_indices_device", "mpct_osc_indices", "mpct_eval_osc_indices", "mpct_eval_osc_indices_device",
    "mpct_eval_robust_osc_indices", "mpct_eval_robust_osc_indices_device",
    "mpct_goal_attain_device", "mpct_goal_attain",
    "mpct_envelope_device", "mpct_envelope", "mpct_eval_robust_envelope", "mpct_eval_robust_envelope_device",
]

ABI_VERSION = 7
TAIL_MAX_LEVELS, TAIL_MAX_DRAWS = 8, 4096
PARETO_MAX_OBJ, PARETO_MAX_C, PARETO_MAX_LAYERS = 16, 1048576, 64
GOAL_MAX_G, GOAL_MAX_BEST = 1048576, 16
HV_MAX_SAMPLES, HV_BINS = 1073741824, 8
HVSEL_MAX_PICKS = 1024
HVX_MAX_OBJ, HVX_MAX_M = 3, 65536
INDEX_MAX_ROWS, INDEX_SCRATCH_BYTES = 2147483647, 268435456
LIMIT_MAX_CH = 32
SEG_MAX = 16
STAT_F64, STAT_I32 = 0, 1
ENVELOPE_DLANE, ENVELOPE_LANE_MAX_DRAWS = 48, 227   # kEnvDefaultDlane, kEnvLaneMaxDraws (csrc/envelope.h)
ST_QP_MAXITER, ST_QP_INFEAS, ST_NONFINITE, ST_SKIPPED, ST_BADHORIZON = 1, 2, 4, 8, 16
ST_SQP_MAXITER, ST_BOUNDS, ST_NOT_RUN = 32, 64, 128
NMPC_VANDEVUSSE = 1
EST_OUTPUT_BIAS = 1

_lib = None


def lib_path() -> str:
    override = os.environ.get("MPCT_LIB")  # e.g. the -DMPCT_PROFILE diagnostic build
    if override:
        return override
    for p in _CANDIDATES:
        if os.path.exists(p):
            return p
    raise ImportError(
        "libmpct.so not found (looked in %s). Build it with `python -c 'import __graft_entry__ as g; "
        "g.build()'` — the engine has no CPU fallback." % ", ".join(_CANDIDATES))


def load():
    global _lib
    if _lib is not None:
        return _lib
    # One HIP runtime per process: PyTorch-ROCm ships its own libamdhip64.so.7 / libhsa-runtime64
    # (ROCm 7.0) and a second copy (/opt/rocm, 7.2) cannot open the device beside it.  Loading
    # torch first makes libmpct's NEEDED libamdhip64.so.7 bind to torch's copy by soname (libmpct
    # only uses hip_4.2-versioned symbols).  Without torch, the system runtime is used.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    lib = C.CDLL(lib_path())
    lib.mpct_abi_version.restype = C.c_int32
    lib.mpct_last_error.restype = C.c_char_p
    lib.mpct_scenario_create.argtypes = [C.POINTER(MpctScenarioDesc), C.POINTER(C.c_void_p)]
    lib.mpct_scenario_create.restype = C.c_int32
    lib.mpct_scenario_create_est.argtypes = [C.POINTER(MpctScenarioDesc), C.c_int32, C.POINTER(C.c_void_p)]
    lib.mpct_scenario_create_est.restype = C.c_int32
    lib.mpct_nmpc_scenario_create.argtypes = [C.POINTER(MpctNmpcDesc), C.POINTER(C.c_void_p)]
    lib.mpct_nmpc_scenario_create.restype = C.c_int32
    lib.mpct_nmpc_scenario_create_var.argtypes = [C.POINTER(MpctNmpcDesc), C.c_int32, c_double_p, c_double_p,
                                                  C.POINTER(C.c_void_p)]
    lib.mpct_nmpc_scenario_create_var.restype = C.c_int32
    lib.mpct_scenario_destroy.argtypes = [C.c_void_p]
    lib.mpct_scenario_destroy.restype = None
    lib.mpct_scenario_table.argtypes = [C.c_void_p, C.c_int32, c_double_p, C.c_int64]
    lib.mpct_scenario_table.restype = C.c_int64
    batch_args = [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32,
                  C.c_void_p, C.c_void_p, C.POINTER(MpctOpts), C.POINTER(MpctResult)]
    lib.mpct_eval_batch.argtypes = batch_args
    lib.mpct_eval_batch.restype = C.c_int32
    lib.mpct_eval_batch_device.argtypes = batch_args + [C.c_void_p]
    lib.mpct_eval_batch_device.restype = C.c_int32
    lib.mpct_lds_bytes.argtypes = [C.c_void_p, C.c_int32, C.c_int32]
    lib.mpct_lds_bytes.restype = C.c_int64
    lib.mpct_lds_bytes_opts.argtypes = [C.c_void_p, C.POINTER(MpctOpts), C.c_int32, C.c_int32]
    lib.mpct_lds_bytes_opts.restype = C.c_int64
    lib.mpct_eval_batch_multi.argtypes = [C.c_void_p, C.c_int32, c_int32_p] + batch_args[1:]
    lib.mpct_eval_batch_multi.restype = C.c_int32
    lib.mpct_shard_candidates.argtypes = [C.c_int64, C.c_int32, C.c_int32, c_int64_p, C.c_int64]
    lib.mpct_shard_candidates.restype = C.c_int64
    lib.mpct_kernel_instance.argtypes = [C.c_void_p, C.POINTER(MpctOpts), C.c_char_p, C.c_int32]
    lib.mpct_kernel_instance.restype = C.c_int32
    lib.mpct_rank_device.argtypes = [C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.mpct_rank_device.restype = C.c_int32
    robust_args = batch_args[:9] + [C.c_double, C.POINTER(MpctOpts), C.POINTER(MpctRobustResult)]
    lib.mpct_eval_robust.argtypes = robust_args
    lib.mpct_eval_robust.restype = C.c_int32
    lib.mpct_eval_robust_device.argtypes = robust_args + [C.c_void_p]
    lib.mpct_eval_robust_device.restype = C.c_int32
    lib.mpct_robust_instance.argtypes = [C.c_void_p, C.POINTER(MpctOpts), C.c_char_p, C.c_int32]
    lib.mpct_robust_instance.restype = C.c_int32
    tail_args = robust_args[:11] + [C.c_int32, c_double_p, C.POINTER(MpctRobustResult), C.POINTER(MpctRobustTail)]
    lib.mpct_eval_robust_tail.argtypes = tail_args
    lib.mpct_eval_robust_tail.restype = C.c_int32
    lib.mpct_eval_robust_tail_device.argtypes = tail_args + [C.c_void_p]
    lib.mpct_eval_robust_tail_device.restype = C.c_int32
    # the reduction of the generic robust path alone: a test hook, not part of include/mpct.h
    lib.mpct_internal_robust_reduce.argtypes = [C.c_int64, C.c_int32, C.c_int32, C.c_double, C.c_void_p, C.c_void_p,
                                                C.POINTER(MpctRobustResult), C.c_void_p]
    lib.mpct_internal_robust_reduce.restype = C.c_int32
    # robust_tail_kernel alone (levels on the host, status may be NULL): a test hook as well
    lib.mpct_internal_robust_tail.argtypes = [C.c_int64, C.c_int32, C.c_int32, C.c_double, C.c_void_p, C.c_void_p,
                                              C.c_int32, c_double_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.mpct_internal_robust_tail.restype = C.c_int32
    lib.mpct_pareto_device.argtypes = [C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.POINTER(MpctParetoResult),
                                       C.c_void_p]
    lib.mpct_pareto_device.restype = C.c_int32
    lib.mpct_pareto.argtypes = [C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.POINTER(MpctParetoResult)]
    lib.mpct_pareto.restype = C.c_int32
    # the device entry with the tile length and the a-split forced, and the default grid: test / bench hooks
    lib.mpct_internal_pareto_tuned.argtypes = lib.mpct_pareto_device.argtypes + [C.c_int32, C.c_int32]
    lib.mpct_internal_pareto_tuned.restype = C.c_int32
    lib.mpct_internal_pareto_grid.argtypes = [C.c_int64, c_int32_p]
    lib.mpct_internal_pareto_grid.restype = C.c_int32
    hv_args = [C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, C.c_uint64]
    lib.mpct_hypervolume_device.argtypes = hv_args + [C.POINTER(MpctHvResult), C.c_void_p]
    lib.mpct_hypervolume_device.restype = C.c_int32
    lib.mpct_hypervolume.argtypes = hv_args + [C.c_int32, C.POINTER(MpctHvResult)]
    lib.mpct_hypervolume.restype = C.c_int32
    # the tile length (0, 128, 256) and the largest grid (0: the default) of hv_count_kernel: a test / bench hook
    lib.mpct_internal_hv_tuned.argtypes = [C.c_int32, C.c_int32]
    lib.mpct_internal_hv_tuned.restype = C.c_int32
    lib.mpct_hv_select_device.argtypes = hv_args + [C.c_int32, C.POINTER(MpctHvSelectResult), C.c_void_p]
    lib.mpct_hv_select_device.restype = C.c_int32
    lib.mpct_hv_select.argtypes = hv_args + [C.c_int32, C.c_int32, C.POINTER(MpctHvSelectResult)]
    lib.mpct_hv_select.restype = C.c_int32
    hvx_args = hv_args[:7]
    lib.mpct_hypervolume_exact_device.argtypes = hvx_args + [C.POINTER(MpctHvxResult), C.c_void_p]
    lib.mpct_hypervolume_exact_device.restype = C.c_int32
    lib.mpct_hypervolume_exact.argtypes = hvx_args + [C.c_int32, C.POINTER(MpctHvxResult)]
    lib.mpct_hypervolume_exact.restype = C.c_int32
    # the tile length and the largest grid of hvsel_gain_kernel, and the per-round event times of the next
    # call alone (a host float array and its length, at least n_pick; None: off): test / tool hooks
    lib.mpct_internal_hvsel_tuned.argtypes = [C.c_int32, C.c_int32]
    lib.mpct_internal_hvsel_tuned.restype = C.c_int32
    lib.mpct_internal_hvsel_round_ms.argtypes = [C.c_void_p, C.c_int32]
    lib.mpct_internal_hvsel_round_ms.restype = C.c_int32
    index_args = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                  C.POINTER(MpctIndexParams)]
    lib.mpct_indices_device.argtypes = index_args + [C.POINTER(MpctIndexResult), C.c_void_p]
    lib.mpct_indices_device.restype = C.c_int32
    lib.mpct_indices.argtypes = index_args + [C.c_int32, C.POINTER(MpctIndexResult)]
    lib.mpct_indices.restype = C.c_int32
    eval_index_args = batch_args[:10] + [C.POINTER(MpctIndexParams), C.POINTER(MpctResult), C.POINTER(MpctIndexResult)]
    lib.mpct_eval_indices.argtypes = eval_index_args
    lib.mpct_eval_indices.restype = C.c_int32
    lib.mpct_eval_indices_device.argtypes = eval_index_args + [C.c_void_p]
    lib.mpct_eval_indices_device.restype = C.c_int32
    # the trajectory-scratch budget of the index entries in bytes (0: the default): a test / bench hook
    lib.mpct_internal_index_budget.argtypes = [C.c_int64]
    lib.mpct_internal_index_budget.restype = C.c_int32
    stats_args = [C.c_void_p, C.c_int32, C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_int32, c_double_p]
    lib.mpct_draw_stats_device.argtypes = stats_args + [C.POINTER(MpctDrawStats), C.c_void_p]
    lib.mpct_draw_stats_device.restype = C.c_int32
    lib.mpct_draw_stats.argtypes = stats_args + [C.c_int32, C.POINTER(MpctDrawStats)]
    lib.mpct_draw_stats.restype = C.c_int32
    robust_index_args = robust_args[:11] + [C.POINTER(MpctIndexParams), C.c_int32, c_int32_p, C.c_int32, c_double_p,
                                            C.POINTER(MpctRobustResult), C.POINTER(MpctDrawStats)]
    lib.mpct_eval_robust_indices.argtypes = robust_index_args
    lib.mpct_eval_robust_indices.restype = C.c_int32
    lib.mpct_eval_robust_indices_device.argtypes = robust_index_args + [C.c_void_p]
    lib.mpct_eval_robust_indices_device.restype = C.c_int32
    limit_args = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.POINTER(MpctLimitParams)]
    lib.mpct_limit_indices_device.argtypes = limit_args + [C.POINTER(MpctLimitResult), C.c_void_p]
    lib.mpct_limit_indices_device.restype = C.c_int32
    lib.mpct_limit_indices.argtypes = limit_args + [C.c_int32, C.POINTER(MpctLimitResult)]
    lib.mpct_limit_indices.restype = C.c_int32
    eval_limit_args = batch_args[:10] + [C.POINTER(MpctLimitParams), C.POINTER(MpctResult), C.POINTER(MpctLimitResult)]
    lib.mpct_eval_limit_indices.argtypes = eval_limit_args
    lib.mpct_eval_limit_indices.restype = C.c_int32
    lib.mpct_eval_limit_indices_device.argtypes = eval_limit_args + [C.c_void_p]
    lib.mpct_eval_limit_indices_device.restype = C.c_int32
    robust_limit_args = robust_args[:11] + [C.POINTER(MpctLimitParams), C.c_int32, c_int32_p, C.c_int32, c_double_p,
                                            C.POINTER(MpctRobustResult), C.POINTER(MpctDrawStats)]
    lib.mpct_eval_robust_limit_indices.argtypes = robust_limit_args
    lib.mpct_eval_robust_limit_indices.restype = C.c_int32
    lib.mpct_eval_robust_limit_indices_device.argtypes = robust_limit_args + [C.c_void_p]
    lib.mpct_eval_robust_limit_indices_device.restype = C.c_int32
    lib.mpct_reference_segments.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, c_int32_p, C.c_int32, C.c_int32,
                                            c_int32_p, c_int32_p]
    lib.mpct_reference_segments.restype = C.c_int32
    seg_args = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                C.POINTER(MpctSegmentParams)]
    lib.mpct_segment_indices_device.argtypes = seg_args + [C.POINTER(MpctSegmentResult), C.c_void_p]
    lib.mpct_segment_indices_device.restype = C.c_int32
    lib.mpct_segment_indices.argtypes = seg_args + [C.c_int32, C.POINTER(MpctSegmentResult)]
    lib.mpct_segment_indices.restype = C.c_int32
    eval_seg_args = batch_args[:10] + [C.POINTER(MpctSegmentParams), C.POINTER(MpctResult), C.POINTER(MpctSegmentResult)]
    lib.mpct_eval_segment_indices.argtypes = eval_seg_args
    lib.mpct_eval_segment_indices.restype = C.c_int32
    lib.mpct_eval_segment_indices_device.argtypes = eval_seg_args + [C.c_void_p]
    lib.mpct_eval_segment_indices_device.restype = C.c_int32
    robust_seg_args = robust_args[:11] + [C.POINTER(MpctSegmentParams), C.c_int32, c_int32_p, C.c_int32, c_double_p,
                                          C.POINTER(MpctRobustResult), C.POINTER(MpctDrawStats)]
    lib.mpct_eval_robust_segment_indices.argtypes = robust_seg_args
    lib.mpct_eval_robust_segment_indices.restype = C.c_int32
    lib.mpct_eval_robust_segment_indices_device.argtypes = robust_seg_args + [C.c_void_p]
    lib.mpct_eval_robust_segment_indices_device.restype = C.c_int32
    osc_args = seg_args[:8] + [C.POINTER(MpctOscParams)]
    lib.mpct_osc_indices_device.argtypes = osc_args + [C.POINTER(MpctOscResult), C.c_void_p]
    lib.mpct_osc_indices_device.restype = C.c_int32
    lib.mpct_osc_indices.argtypes = osc_args + [C.c_int32, C.POINTER(MpctOscResult)]
    lib.mpct_osc_indices.restype = C.c_int32
    eval_osc_args = batch_args[:10] + [C.POINTER(MpctOscParams), C.POINTER(MpctResult), C.POINTER(MpctOscResult)]
    lib.mpct_eval_osc_indices.argtypes = eval_osc_args
    lib.mpct_eval_osc_indices.restype = C.c_int32
    lib.mpct_eval_osc_indices_device.argtypes = eval_osc_args + [C.c_void_p]
    lib.mpct_eval_osc_indices_device.restype = C.c_int32
    robust_osc_args = robust_args[:11] + [C.POINTER(MpctOscParams), C.c_int32, c_int32_p, C.c_int32, c_double_p,
                                          C.POINTER(MpctRobustResult), C.POINTER(MpctDrawStats)]
    lib.mpct_eval_robust_osc_indices.argtypes = robust_osc_args
    lib.mpct_eval_robust_osc_indices.restype = C.c_int32
    lib.mpct_eval_robust_osc_indices_device.argtypes = robust_osc_args + [C.c_void_p]
    lib.mpct_eval_robust_osc_indices_device.restype = C.c_int32
    goal_args = [C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p, C.c_int64, C.c_int32]
    lib.mpct_goal_attain_device.argtypes = goal_args + [C.POINTER(MpctGoalResult), C.c_void_p]
    lib.mpct_goal_attain_device.restype = C.c_int32
    lib.mpct_goal_attain.argtypes = goal_args + [C.c_int32, C.POINTER(MpctGoalResult)]
    lib.mpct_goal_attain.restype = C.c_int32
    # the chunks of the candidate range (0: the default) and the tile length (0, 128, 256) of goal_pair_kernel, and
    # the grid {tile, chunks, candidates per chunk} that setting gives for G goal vectors and C candidates: test hooks
    lib.mpct_internal_goal_grid.argtypes = [C.c_int32, C.c_int32]
    lib.mpct_internal_goal_grid.restype = C.c_int32
    lib.mpct_internal_goal_geometry.argtypes = [C.c_int64, C.c_int64, c_int32_p]
    lib.mpct_internal_goal_geometry.restype = C.c_int32
    # the largest grid of draw_stats_kernel in workgroups (0: the default): a test hook
    lib.mpct_internal_draw_stats_grid.argtypes = [C.c_int32]
    lib.mpct_internal_draw_stats_grid.restype = C.c_int32
    env_out = [C.POINTER(MpctDrawStats), C.POINTER(MpctDrawStats), C.POINTER(MpctEnvelopeSpread), C.POINTER(MpctEnvelopeSpread)]
    env_args = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                C.c_int32, c_double_p]
    lib.mpct_envelope_device.argtypes = env_args + env_out + [C.c_void_p]
    lib.mpct_envelope_device.restype = C.c_int32
    lib.mpct_envelope.argtypes = env_args + [C.c_int32] + env_out
    lib.mpct_envelope.restype = C.c_int32
    robust_env_args = robust_args[:11] + [C.c_int32, C.c_int32, c_double_p, C.POINTER(MpctRobustResult)] + env_out
    lib.mpct_eval_robust_envelope.argtypes = robust_env_args
    lib.mpct_eval_robust_envelope.restype = C.c_int32
    lib.mpct_eval_robust_envelope_device.argtypes = robust_env_args + [C.c_void_p]
    lib.mpct_eval_robust_envelope_device.restype = C.c_int32
    # the largest grid of draw_envelope_kernel in workgroups (0: the default), and the draws up to which the levels
    # of an envelope run on that kernel (0: the default; above it draw_stats_kernel takes the table): test hooks
    lib.mpct_internal_envelope_grid.argtypes = [C.c_int32]
    lib.mpct_internal_envelope_grid.restype = C.c_int32
    lib.mpct_internal_envelope_dlane.argtypes = [C.c_int32]
    lib.mpct_internal_envelope_dlane.restype = C.c_int32
    if lib.mpct_abi_version() != ABI_VERSION:
        raise ImportError("libmpct ABI version mismatch")
    _lib = lib
    return lib


def last_error() -> str:
    return load().mpct_last_error().decode(errors="replace")
