"""ctypes binding of libt1d_hip.so (include/t1d.h).  There is no CPU fallback: if the HIP
library is missing or fails to load, every product path raises."""
import ctypes as C
import os
import subprocess

_PKG = os.path.dirname(os.path.abspath(__file__))
_ROOT = os.path.dirname(_PKG)
LIB_PATH = os.environ.get("T1D_LIB_PATH") or os.path.join(_PKG, "libt1d_hip.so")   # override: A/B builds only
SOURCES = [os.path.join(_PKG, "csrc", "t1d_abi.hip"), os.path.join(_PKG, "csrc", "t1d_kernels.hpp"),
           os.path.join(_PKG, "csrc", "t1d_device.hpp"), os.path.join(_PKG, "csrc", "t1d_dopri5.hpp"),
           os.path.join(_PKG, "csrc", "t1d_policy.hpp"), os.path.join(_PKG, "csrc", "t1d_policy_grad.hpp"),
           os.path.join(_PKG, "csrc", "t1d_gae.hpp"), os.path.join(_PKG, "csrc", "t1d_stepn_body.inc"),
           os.path.join(_PKG, "csrc", "t1d_dopri5_loop.inc"), os.path.join(_ROOT, "include", "t1d.h")]

T1D_F64, T1D_F32 = 0, 1
T1D_ST_NORMALS_EXHAUSTED, T1D_ST_NONFINITE, T1D_ST_BAD_INDEX, T1D_ST_STALL = 1, 2, 4, 8
T1D_ST_SOLVER_FAILED = 16
ABI_VERSION = 4
T1D_BATCH_NO_PUMP = 2
T1D_BATCH_NO_REFILL_DUE = 4
META_PLANNED = 0x200
P_NCOLS = 45
MEAL_UNUSED = 0x7FFFFFFF
META_EATING = 0x100
T1D_MLP_TANH, T1D_MLP_RELU = 0, 1
T1D_MLP_IDENTITY, T1D_MLP_LOGISTIC = 0, 1
T1D_COLLECT_CONTINUE, T1D_COLLECT_RESTART = 0, 1
T1D_LOSS_PPO_CLIP, T1D_LOSS_VALUE_MSE = 1, 2
MLP_MAX_HISTORY, MLP_MAX_LAYERS, MLP_MAX_WIDTH = 12, 4, 32

EXPORTS = ("t1d_abi_version", "t1d_last_error", "t1d_ctx_create", "t1d_ctx_set_option", "t1d_ctx_destroy", "t1d_reset",
           "t1d_step", "t1d_rollout_pid", "t1d_philox_normals", "t1d_sync", "t1d_split_tables",
           "t1d_rollout_bb", "t1d_random_meals", "t1d_outcome_stats", "t1d_model_rhs", "t1d_step_dopri5",
           "t1d_rollout_pid_dopri5", "t1d_rollout_bb_dopri5", "t1d_restart_done", "t1d_rollout_mlp",
           "t1d_collect_mlp", "t1d_rollout_mlp_dopri5", "t1d_mlp_action", "t1d_collect_mlp_dopri5",
           "t1d_mlp_grad_workspace", "t1d_mlp_grad", "t1d_mlp_features", "t1d_gae_workspace", "t1d_gae",
           "t1d_mlp_loss_workspace", "t1d_mlp_loss", "t1d_mlp_grad_tiles_workspace", "t1d_mlp_grad_tiles",
           "t1d_mlp_loss_tiles_workspace", "t1d_mlp_loss_tiles", "t1d_collect_pid", "t1d_collect_bb",
           "t1d_collect_pid_dopri5", "t1d_collect_bb_dopri5", "t1d_rollout_mlp_bolus", "t1d_collect_mlp_bolus",
           "t1d_rollout_mlp_dopri5_bolus", "t1d_mlp_bolus", "t1d_rollout_mlp_rel", "t1d_collect_mlp_rel",
           "t1d_rollout_mlp_dopri5_rel", "t1d_mlp_action_rel", "t1d_collect_mlp_limit", "t1d_gae_limit",
           "t1d_collect_pid_limit", "t1d_collect_bb_limit", "t1d_collect_mlp_dopri5_limit", "t1d_collect_pid_dopri5_limit",
           "t1d_collect_bb_dopri5_limit", "t1d_rollout_pid_gains", "t1d_rollout_pid_dopri5_gains")


class T1DError(RuntimeError):
    pass


class Batch(C.Structure):
    """struct t1d_batch (include/t1d.h)"""
    _fields_ = [
        ("n", C.c_int64), ("env_offset", C.c_int64), ("dtype", C.c_int32), ("n_meals", C.c_int32),
        ("n_normals", C.c_int32), ("flags", C.c_int32), ("seed", C.c_uint64),
        ("x", C.c_void_p), ("planned", C.c_void_p), ("last_qsto", C.c_void_p), ("last_food", C.c_void_p),
        ("t", C.c_void_p), ("meta", C.c_void_p), ("episode", C.c_void_p), ("next_meal", C.c_void_p),
        ("last_cgm", C.c_void_p), ("ar_e", C.c_void_p), ("pts", C.c_void_p), ("prev_risk", C.c_void_p), ("dbar", C.c_void_p),
        ("basal", C.c_void_p), ("bolus", C.c_void_p), ("cho", C.c_void_p), ("meal_time", C.c_void_p),
        ("meal_amt", C.c_void_p), ("normals", C.c_void_p), ("x0_override", C.c_void_p),
        ("cgm", C.c_void_p), ("bg", C.c_void_p), ("reward", C.c_void_p), ("done", C.c_void_p),
        ("lbgi", C.c_void_p), ("hbgi", C.c_void_p), ("risk", C.c_void_p), ("meal", C.c_void_p),
        ("insulin", C.c_void_p), ("cgm0", C.c_void_p),
    ]


# the accumulators and the four trace columns that t1d_pid, t1d_bb and t1d_mlp all carry, in the header's order
_STATS_FIELDS = [(k, C.c_void_p) for k in ("sum_risk", "min_bg", "max_bg", "n_low", "n_high")]
_TRACE_FIELDS = [(k, C.c_void_p) for k in ("bg_trace", "cgm_trace", "cho_trace", "insulin_trace")]


class Pid(C.Structure):
    """struct t1d_pid (include/t1d.h)"""
    _fields_ = [("P", C.c_double), ("I", C.c_double), ("D", C.c_double), ("target", C.c_double),
                ("integ", C.c_void_p), ("prev", C.c_void_p)] + _STATS_FIELDS + _TRACE_FIELDS + [("trace_row", C.c_int64)]


class PidGains(C.Structure):
    """struct t1d_pid_gains (include/t1d.h)"""
    _fields_ = [("P", C.c_void_p), ("I", C.c_void_p), ("D", C.c_void_p), ("target", C.c_void_p)]


class Bb(C.Structure):
    """struct t1d_bb (include/t1d.h)"""
    _fields_ = [("target", C.c_double), ("basal", C.c_void_p), ("cr", C.c_void_p), ("cf", C.c_void_p),
                ("prev_meal", C.c_void_p)] + _STATS_FIELDS + _TRACE_FIELDS + [("trace_row", C.c_int64)]


class Mlp(C.Structure):
    """struct t1d_mlp (include/t1d.h)"""
    _fields_ = [("history", C.c_int32), ("n_layers", C.c_int32), ("width", C.c_int32 * 4), ("hidden_act", C.c_int32),
                ("out_act", C.c_int32), ("n_policies", C.c_int64), ("envs_per_policy", C.c_int64), ("n_params", C.c_int64),
                ("cgm_mean", C.c_double), ("cgm_scale", C.c_double), ("ins_scale", C.c_double), ("cho_scale", C.c_double),
                ("out_scale", C.c_double), ("out_bias", C.c_double),
                ("params", C.c_void_p), ("cgm_hist", C.c_void_p), ("ins_hist", C.c_void_p), ("prev_meal", C.c_void_p),
                ("start_minute", C.c_void_p)] + _STATS_FIELDS + _TRACE_FIELDS + [("action_trace", C.c_void_p), ("trace_row", C.c_int64)]


class MealBolus(C.Structure):
    """struct t1d_meal_bolus (include/t1d.h)"""
    _fields_ = [("target", C.c_double), ("cr", C.c_void_p), ("cf", C.c_void_p), ("bolus_trace", C.c_void_p)]


class EnvOutput(C.Structure):
    """struct t1d_env_output (include/t1d.h)"""
    _fields_ = [("scale", C.c_void_p), ("bias", C.c_void_p)]


class TimeLimit(C.Structure):
    """struct t1d_time_limit (include/t1d.h)"""
    _fields_ = [("max_minutes", C.c_int32), ("reserved", C.c_int32), ("cut_trace", C.c_void_p), ("cut_feat", C.c_void_p)]


class GaeCut(C.Structure):
    """struct t1d_gae_cut (include/t1d.h)"""
    _fields_ = [("truncated", C.c_void_p), ("cut_value", C.c_void_p)]


class Outcome(C.Structure):
    """struct t1d_outcome (include/t1d.h)"""
    _fields_ = [("counts", C.c_void_p), ("pct", C.c_void_p), ("zone", C.c_void_p), ("risk_trace", C.c_void_p),
                ("q_lo", C.c_double), ("q_hi", C.c_double), ("chunk", C.c_int32)]


class Restart(C.Structure):
    """struct t1d_restart (include/t1d.h)"""
    _fields_ = [("days", C.c_int32), ("random_init_bg", C.c_int32), ("reset_outputs", C.c_int32), ("reserved", C.c_int32),
                ("meal_time", C.c_void_p), ("meal_amt", C.c_void_p), ("start_minute", C.c_void_p), ("h_carry", C.c_void_p),
                ("terminal_cgm", C.c_void_p), ("ep_return", C.c_void_p), ("ep_length", C.c_void_p),
                ("last_return", C.c_void_p), ("last_length", C.c_void_p)]


class Collect(C.Structure):
    """struct t1d_collect (include/t1d.h)"""
    _fields_ = [("explore_seed", C.c_uint64), ("sigma", C.c_void_p), ("on_done", C.c_int32), ("reserved", C.c_int32),
                ("restart", C.POINTER(Restart)), ("reward_trace", C.c_void_p), ("done_trace", C.c_void_p),
                ("eps_trace", C.c_void_p), ("feat_trace", C.c_void_p)]


class MlpBatch(C.Structure):
    """struct t1d_mlp_batch (include/t1d.h)"""
    _fields_ = [("n_rows", C.c_int64), ("feat", C.c_void_p), ("coef", C.c_void_p), ("y", C.c_void_p), ("grad", C.c_void_p),
                ("workspace", C.c_void_p), ("workspace_bytes", C.c_int64)]


class MlpLoss(C.Structure):
    """struct t1d_mlp_loss (include/t1d.h)"""
    _fields_ = [("n_rows", C.c_int64), ("kind", C.c_int32), ("reserved", C.c_int32), ("feat", C.c_void_p),
                ("eps", C.c_void_p), ("y_old", C.c_void_p), ("adv", C.c_void_p), ("sigma_old", C.c_void_p), ("sigma", C.c_void_p),
                ("target", C.c_void_p), ("clip", C.c_double), ("scale", C.c_double),
                ("y", C.c_void_p), ("coef_out", C.c_void_p), ("grad", C.c_void_p), ("stats", C.c_void_p),
                ("workspace", C.c_void_p), ("workspace_bytes", C.c_int64)]


class TileList(C.Structure):
    """struct t1d_tile_list (include/t1d.h)"""
    _fields_ = [("n_tiles", C.c_int64), ("tiles", C.c_void_p)]


class GaeBatch(C.Structure):
    """struct t1d_gae_batch (include/t1d.h)"""
    _fields_ = [("n_rows", C.c_int64), ("n_policies", C.c_int64), ("gamma", C.c_double), ("lam", C.c_double),
                ("reward", C.c_void_p), ("done", C.c_void_p), ("value", C.c_void_p), ("last_value", C.c_void_p),
                ("adv", C.c_void_p), ("ret", C.c_void_p), ("moments", C.c_void_p),
                ("workspace", C.c_void_p), ("workspace_bytes", C.c_int64)]


def _stale():
    return not os.path.exists(LIB_PATH) or any(os.path.exists(s) and os.path.getmtime(s) > os.path.getmtime(LIB_PATH)
                                               for s in SOURCES)


# The code-generation flags of the library: whatever compiles csrc/t1d_abi.hip to look at "the library's build" (the ISA
# tools, the register and scratch figures the tests assert) takes them from here.
# -fno-slp-vectorize: in the fp32 kernels the SLP vectoriser pairs a fifth of the arithmetic into v_pk_*_f32
# and pays more than it gains in the register moves that line the operands up (1 Mi envs fp32: 45.5 -> 42.4 us)
HIPCC_FLAGS = ["--offload-arch=gfx950", "-O3", "-fno-slp-vectorize", "-std=c++17"]


def build_command(out, verbose=False):
    """the command line that compiles the library into `out`"""
    cmd = [os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")] + HIPCC_FLAGS + ["-shared", "-fPIC", "-o", out, SOURCES[0]]
    if verbose:
        cmd.insert(1, "-Rpass-analysis=kernel-resource-usage")
    return cmd


def build(force=False, verbose=False):
    """Compile libt1d_hip.so for gfx950 in-tree with hipcc (cross-compiles without a GPU).  Safe when several
    processes (one per GPU) find the library stale at once: one builds under a file lock into a temporary
    file that is moved into place, the others wait and then find it fresh."""
    import fcntl
    if not (force or _stale()):
        return LIB_PATH
    with open(LIB_PATH + ".lock", "w") as lock:
        fcntl.flock(lock, fcntl.LOCK_EX)
        try:
            if force or _stale():
                tmp = "%s.tmp.%d" % (LIB_PATH, os.getpid())
                try:
                    subprocess.check_call(build_command(tmp, verbose))
                    os.replace(tmp, LIB_PATH)
                finally:
                    if os.path.exists(tmp):
                        os.remove(tmp)
        finally:
            fcntl.flock(lock, fcntl.LOCK_UN)
    return LIB_PATH


_lib = None


def lib():
    """Load the HIP library (building it first if the sources are newer).  Raises T1DError when
    it cannot be produced or loaded -- the product never falls back to a CPU path."""
    global _lib
    if _lib is not None:
        return _lib
    # torch first: the library launches on torch's streams, so its libamdhip64.so.7 must resolve to the HIP runtime torch
    # has loaded.  Loaded the other way round, torch (which asks for libamdhip64.so) maps a second HIP and HSA runtime
    # into the process, and whichever of the two starts second finds no device.
    import torch  # noqa: F401
    try:
        if _stale():
            build()
        L = C.CDLL(LIB_PATH)
    except (OSError, subprocess.CalledProcessError, FileNotFoundError) as e:
        raise T1DError("libt1d_hip.so (HIP/gfx950 extension) is not available: %s" % e) from e
    vp, i32, i64, u64, u32 = C.c_void_p, C.c_int32, C.c_int64, C.c_uint64, C.c_uint32
    dp = C.POINTER(C.c_double)
    L.t1d_abi_version.restype = C.c_int
    L.t1d_last_error.restype = C.c_char_p
    L.t1d_ctx_create.argtypes = [C.c_int, dp, C.c_int, C.c_int, dp, dp, C.POINTER(vp)]
    L.t1d_ctx_destroy.argtypes = [vp]
    L.t1d_ctx_set_option.argtypes = [vp, C.c_char_p, i64]
    L.t1d_reset.argtypes = [vp, C.POINTER(Batch), vp, C.c_int, vp]
    L.t1d_step.argtypes = [vp, C.POINTER(Batch), C.c_int, C.c_int, vp]
    L.t1d_step_dopri5.argtypes = [vp, C.POINTER(Batch), vp, vp, C.c_int, vp]
    L.t1d_rollout_pid.argtypes = [vp, C.POINTER(Batch), C.POINTER(Pid), C.c_int, C.c_int, C.c_int, vp]
    L.t1d_rollout_pid_gains.argtypes = [vp, C.POINTER(Batch), C.POINTER(Pid), C.POINTER(PidGains), C.c_int, C.c_int, C.c_int, vp]
    L.t1d_rollout_bb.argtypes = [vp, C.POINTER(Batch), C.POINTER(Bb), C.c_int, C.c_int, C.c_int, vp]
    L.t1d_rollout_mlp.argtypes = [vp, C.POINTER(Batch), C.POINTER(Mlp), C.c_int, C.c_int, C.c_int, vp]
    L.t1d_collect_mlp.argtypes = [vp, C.POINTER(Batch), C.POINTER(Mlp), C.POINTER(Collect), C.c_int, C.c_int, C.c_int, vp]
    L.t1d_collect_pid.argtypes = [vp, C.POINTER(Batch), C.POINTER(Pid), C.POINTER(Mlp), C.POINTER(Collect), C.c_int, C.c_int, C.c_int, vp]
    L.t1d_collect_bb.argtypes = [vp, C.POINTER(Batch), C.POINTER(Bb), C.POINTER(Mlp), C.POINTER(Collect), C.c_int, C.c_int, C.c_int, vp]
    L.t1d_rollout_pid_dopri5.argtypes = [vp, C.POINTER(Batch), C.POINTER(Pid), vp, vp, C.c_int, C.c_int, vp]
    L.t1d_rollout_pid_dopri5_gains.argtypes = [vp, C.POINTER(Batch), C.POINTER(Pid), C.POINTER(PidGains), vp, vp, C.c_int, C.c_int, vp]
    L.t1d_rollout_bb_dopri5.argtypes = [vp, C.POINTER(Batch), C.POINTER(Bb), vp, vp, C.c_int, C.c_int, vp]
    L.t1d_rollout_mlp_dopri5.argtypes = [vp, C.POINTER(Batch), C.POINTER(Mlp), vp, vp, C.c_int, C.c_int, vp]
    L.t1d_collect_mlp_dopri5.argtypes = [vp, C.POINTER(Batch), C.POINTER(Mlp), C.POINTER(Collect), vp, vp, C.c_int, C.c_int, vp]
    L.t1d_collect_pid_dopri5.argtypes = [vp, C.POINTER(Batch), C.POINTER(Pid), C.POINTER(Mlp), C.POINTER(Collect), vp, vp,
                                         C.c_int, C.c_int, vp]
    L.t1d_collect_bb_dopri5.argtypes = [vp, C.POINTER(Batch), C.POINTER(Bb), C.POINTER(Mlp), C.POINTER(Collect), vp, vp,
                                        C.c_int, C.c_int, vp]
    L.t1d_mlp_action.argtypes = [vp, C.POINTER(Batch), C.POINTER(Mlp), vp, vp]
    mb = C.POINTER(MealBolus)
    L.t1d_rollout_mlp_bolus.argtypes = [vp, C.POINTER(Batch), C.POINTER(Mlp), mb, C.c_int, C.c_int, C.c_int, vp]
    L.t1d_collect_mlp_bolus.argtypes = [vp, C.POINTER(Batch), C.POINTER(Mlp), C.POINTER(Collect), mb, C.c_int, C.c_int, C.c_int, vp]
    L.t1d_rollout_mlp_dopri5_bolus.argtypes = [vp, C.POINTER(Batch), C.POINTER(Mlp), mb, vp, vp, C.c_int, C.c_int, vp]
    L.t1d_mlp_bolus.argtypes = [vp, C.POINTER(Batch), C.POINTER(Mlp), mb, vp, vp]
    eo = C.POINTER(EnvOutput)
    L.t1d_rollout_mlp_rel.argtypes = [vp, C.POINTER(Batch), C.POINTER(Mlp), eo, mb, C.c_int, C.c_int, C.c_int, vp]
    L.t1d_collect_mlp_rel.argtypes = [vp, C.POINTER(Batch), C.POINTER(Mlp), C.POINTER(Collect), eo, mb, C.c_int, C.c_int, C.c_int, vp]
    L.t1d_rollout_mlp_dopri5_rel.argtypes = [vp, C.POINTER(Batch), C.POINTER(Mlp), eo, mb, vp, vp, C.c_int, C.c_int, vp]
    L.t1d_mlp_action_rel.argtypes = [vp, C.POINTER(Batch), C.POINTER(Mlp), eo, vp, vp]
    L.t1d_collect_mlp_limit.argtypes = [vp, C.POINTER(Batch), C.POINTER(Mlp), C.POINTER(Collect), eo, mb, C.POINTER(TimeLimit),
                                        C.c_int, C.c_int, C.c_int, vp]
    tl = C.POINTER(TimeLimit)
    L.t1d_collect_pid_limit.argtypes = [vp, C.POINTER(Batch), C.POINTER(Pid), C.POINTER(Mlp), C.POINTER(Collect), tl, C.c_int, C.c_int,
                                        C.c_int, vp]
    L.t1d_collect_bb_limit.argtypes = [vp, C.POINTER(Batch), C.POINTER(Bb), C.POINTER(Mlp), C.POINTER(Collect), tl, C.c_int, C.c_int,
                                       C.c_int, vp]
    L.t1d_collect_mlp_dopri5_limit.argtypes = [vp, C.POINTER(Batch), C.POINTER(Mlp), C.POINTER(Collect), tl, vp, vp, C.c_int, C.c_int, vp]
    L.t1d_collect_pid_dopri5_limit.argtypes = [vp, C.POINTER(Batch), C.POINTER(Pid), C.POINTER(Mlp), C.POINTER(Collect), tl, vp, vp,
                                               C.c_int, C.c_int, vp]
    L.t1d_collect_bb_dopri5_limit.argtypes = [vp, C.POINTER(Batch), C.POINTER(Bb), C.POINTER(Mlp), C.POINTER(Collect), tl, vp, vp,
                                              C.c_int, C.c_int, vp]
    L.t1d_mlp_grad_workspace.argtypes = [C.POINTER(Mlp), C.c_int, i64, i64]
    L.t1d_mlp_grad.argtypes = [C.c_int, C.c_int, i64, C.POINTER(Mlp), C.POINTER(MlpBatch), vp]
    L.t1d_mlp_loss_workspace.argtypes = [C.POINTER(Mlp), C.c_int, i64, i64]
    L.t1d_mlp_loss.argtypes = [C.c_int, C.c_int, i64, C.POINTER(Mlp), C.POINTER(MlpLoss), vp]
    L.t1d_mlp_grad_tiles_workspace.argtypes = [C.POINTER(Mlp), C.c_int, i64, i64]
    L.t1d_mlp_grad_tiles.argtypes = [C.c_int, C.c_int, i64, C.POINTER(Mlp), C.POINTER(MlpBatch), C.POINTER(TileList), vp]
    L.t1d_mlp_loss_tiles_workspace.argtypes = [C.POINTER(Mlp), C.c_int, i64, i64]
    L.t1d_mlp_loss_tiles.argtypes = [C.c_int, C.c_int, i64, C.POINTER(Mlp), C.POINTER(MlpLoss), C.POINTER(TileList), vp]
    L.t1d_mlp_features.argtypes = [vp, C.POINTER(Batch), C.POINTER(Mlp), vp, vp]
    L.t1d_gae_workspace.argtypes = [C.c_int, i64, C.POINTER(GaeBatch)]
    L.t1d_gae.argtypes = [C.c_int, C.c_int, i64, C.POINTER(GaeBatch), vp]
    L.t1d_gae_limit.argtypes = [C.c_int, C.c_int, i64, C.POINTER(GaeBatch), C.POINTER(GaeCut), vp]
    L.t1d_restart_done.argtypes = [vp, C.POINTER(Batch), vp, C.POINTER(Restart), vp]
    L.t1d_random_meals.argtypes = [C.c_int, u64, i64, i64, C.c_int, C.c_int, vp, C.c_int, vp, vp, vp]
    L.t1d_outcome_stats.argtypes = [C.c_int, C.c_int, i64, i64, vp, C.POINTER(Outcome), vp]
    L.t1d_philox_normals.argtypes = [vp, u64, i64, i64, u32, i32, i32, vp, vp]
    L.t1d_model_rhs.argtypes = [vp, C.c_int, i64, C.c_int, vp, vp, vp, vp, vp, vp, vp, vp]
    L.t1d_sync.argtypes = [vp, vp, C.POINTER(i32)]
    L.t1d_split_tables.argtypes = [dp, C.c_int, C.c_int, dp, C.c_int]
    for name in EXPORTS:
        if name not in ("t1d_last_error",):
            getattr(L, name).restype = C.c_int
    L.t1d_mlp_grad_workspace.restype = i64
    L.t1d_gae_workspace.restype = i64
    L.t1d_mlp_loss_workspace.restype = i64
    L.t1d_mlp_grad_tiles_workspace.restype = i64
    L.t1d_mlp_loss_tiles_workspace.restype = i64
    if L.t1d_abi_version() != ABI_VERSION:
        raise T1DError("libt1d_hip.so ABI version mismatch")
    _lib = L
    return L


def check(rc):
    if rc != 0:
        raise T1DError("t1d error %d: %s" % (rc, lib().t1d_last_error().decode()))
