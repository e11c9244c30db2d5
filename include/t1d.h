/*
 * t1d.h -- C ABI of libt1d_hip.so: the MI355X (gfx950) batched T1D glucose-insulin simulator.
 *
 * The reference (Sawyerbatch/simglucose, pure Python) has no FFI boundary; the boundary this
 * library replaces is the Python call chain below, for a whole batch of environments at once
 * (paths relative to the reference checkout):
 *
 *   t1d_reset        <- T1DSimEnv.reset / _reset        simglucose/simulation/env.py:119-155
 *                       T1DPatient.reset                simglucose/patient/t1dpatient.py:247-281
 *                       CGMSensor.reset / CGMNoise()    simglucose/sensor/cgm.py:47-50, noise_gen.py:15-28
 *   t1d_step         <- T1DSimEnv.step / mini_step      simglucose/simulation/env.py:48-117
 *                       InsulinPump.basal / .bolus      simglucose/actuator/pump.py:23-39
 *                       T1DPatient.step / model         simglucose/patient/t1dpatient.py:82-208,222-236
 *                       scipy ode('dopri5').integrate   simglucose/patient/t1dpatient.py:110-113,276
 *                         (replaced by fixed-step schemes built on n_sub sub-steps per minute: the split
 *                          integrator with per-minute step sizes by default, classical RK4 on request --
 *                          t1d_ctx_set_option "integrator" / "adaptive_gut")
 *   t1d_step_dopri5  <- the same step with scipy's dopri5 itself (the exact mode)
 *                       CGMSensor.measure / CGMNoise    simglucose/sensor/cgm.py:26-36, noise_gen.py:30-97
 *                       risk_index / risk_diff          simglucose/analysis/risk.py:5-17, env.py:27-33
 *   t1d_model_rhs    <- T1DPatient.model               simglucose/patient/t1dpatient.py:119-208
 *   t1d_rollout_pid  <- SimObj.simulate loop with       simglucose/simulation/sim_engine.py:29-39
 *                       PIDController.policy            simglucose/controller/pid_ctrller.py:17-36
 *   t1d_rollout_bb   <- the same loop with BBController  simglucose/controller/basal_bolus_ctrller.py:34-80
 *   t1d_rollout_mlp  <- the same loop with a learned policy: a small feed-forward network on the recent CGM, insulin
 *                       and meal history (no counterpart in the reference, whose controllers are hand-written; it is
 *                       what a user of simglucose/envs/simglucose_gym_env.py:14-106 trains)
 *   t1d_collect_mlp  <- that loop as a gym training loop runs it: the action sampled around the network's output, the
 *                       reward and done of every step kept, reset() when done comes back true
 *                       (simglucose/envs/simglucose_gym_env.py:39-73)
 *   t1d_rollout_pid_dopri5, t1d_rollout_bb_dopri5 <- the two loops with scipy's dopri5 itself (the exact mode)
 *   t1d_rollout_mlp_dopri5, t1d_collect_mlp_dopri5 <- t1d_rollout_mlp and t1d_collect_mlp in the exact mode
 *   t1d_collect_pid_dopri5, t1d_collect_bb_dopri5 <- t1d_collect_pid and t1d_collect_bb in the exact mode
 *   t1d_mlp_features <- the observation a gym trainer keeps for its critic's bootstrap: the network's inputs for the step that
 *                       would come next (no counterpart in the reference; its gym env hands back one CGM value, env.py:81)
 *   t1d_mlp_grad     <- the network again on a collected batch, and its weight gradient (what autograd does for a gym trainer)
 *   t1d_mlp_loss     <- the same with the PPO-clip or value loss inside the launch: one forward pass per epoch
 *   t1d_mlp_grad_tiles, t1d_mlp_loss_tiles  <- either on a minibatch: a list of 64-env tiles of the batch, read in place
 *   t1d_gae          <- the trainer's backward loop over a collected batch: advantages (generalised advantage estimation),
 *                       value targets and the advantage moments PPO normalises with (no counterpart in the reference)
 *   t1d_random_meals <- RandomScenario.create_scenario  simglucose/simulation/scenario_gen.py:33-60
 *   t1d_restart_done <- the reset() a gym training loop calls when done comes back true (T1DSimEnv.reset + a new
 *                       RandomScenario and start hour, simglucose/envs/simglucose_gym_env.py:58-73), for the finished envs only
 *   t1d_outcome_stats<- percent_stats, risk_index_trace, simglucose/analysis/report.py:74-133,198-217
 *                       CVGA_analysis
 *
 * Conventions
 *  - Every pointer inside t1d_batch is a DEVICE pointer (e.g. torch.Tensor.data_ptr()) owned by
 *    the caller, who keeps it alive until the stream has passed the call.  Arrays are struct-of-
 *    arrays with the env index fastest: a [K][n] array holds element k of env i at k*n + i.
 *    Floating arrays have the element type named by `dtype` (T1D_F64: double, T1D_F32: float).
 *  - Calls only enqueue work on `hip_stream` (a hipStream_t; NULL = default stream); they never
 *    synchronise.  Asynchronous faults surface at t1d_sync or the next call.
 *  - Return value 0 = success; negative = error (see T1D_E_*), message in t1d_last_error()
 *    (thread-local).  No C++ exception crosses this boundary.
 *  - A ctx is bound to one device and is not thread-safe: one host thread/process per GPU.  Every entry point
 *    that takes a ctx makes that device current (hipSetDevice) before it launches or allocates.
 */
#ifndef T1D_H
#define T1D_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define T1D_ABI_VERSION 4

enum { T1D_F64 = 0, T1D_F32 = 1 };

enum {
    T1D_OK = 0,
    T1D_E_INVALID = -1,      /* bad argument (null pointer, size, dtype, n_sub ...) */
    T1D_E_HIP = -2,          /* a HIP runtime call failed */
    T1D_E_NODEVICE = -3,     /* no usable gfx950 device */
    T1D_E_STATUS = -4        /* t1d_sync: a kernel raised a status bit (see T1D_ST_*) */
};

/* bits of the device status word returned through t1d_sync.  The word is cleared by the t1d_sync that reads it: a second
 * t1d_sync right after returns 0, and a bit tells of the launches since the last read.
 * T1D_ST_NONFINITE is raised by every launch that leaves a non-finite word (NaN, +-Inf) in some env's stored x[12], the
 * subcutaneous glucose that BG and the sensor read: by the launch in which a NaN action, or a non-finite word elsewhere in
 * the state, reaches x[12], and by every later launch for as long as it stays there.  Such an env is NOT visible in the
 * outputs: the sensor's clamp to its range turns a NaN sample into the range's lower end, so `cgm` reads sensor min, and
 * `done` = BG < 70 || BG > 350 is 0 for a NaN BG, so the env never ends and is never restarted (t1d_restart_done,
 * on_done = restart).  The bit is the only signal: a trainer that does not read t1d_sync sees an ordinary deep low.  In the
 * exact mode the solver gives up on such an env (T1D_ST_SOLVER_FAILED) and the env keeps its last accepted state, so a
 * non-finite word outside x[12] stays where it is and raises T1D_ST_SOLVER_FAILED alone.  The other envs are unaffected.
 * T1D_ST_NORMALS_EXHAUSTED is raised by the launch (t1d_reset included) that builds a 150-minute noise block for which
 * the rows are missing, not by the launches that go on using that block.  The block takes its ten rows in five pairs and
 * a pair counts as missing unless both of its rows exist: the draws of such a pair are zero as a whole. */
enum {
    T1D_ST_NORMALS_EXHAUSTED = 1,   /* host-normals mode ran past n_normals rows; zeros were used */
    T1D_ST_NONFINITE = 2,           /* some env's stored x[12] is NaN/Inf after the launch (above) */
    T1D_ST_BAD_INDEX = 4,           /* t1d_model_rhs: a patient index outside the context's table (row 0 was used) */
    T1D_ST_STALL = 8,               /* a wave of a persistent kernel gave up waiting for its workgroup (never, by design): results invalid */
    T1D_ST_SOLVER_FAILED = 16       /* t1d_step_dopri5: some env's solver gave up (step budget or step underflow; the reference raises
                                       "ODE solver failed"): that env kept its last accepted state for the rest of the call */
};

/* columns of one row of the patient table given to t1d_ctx_create (all double):
 * x0_1..x0_13 then the model parameters of params/vpatient_params.csv in this order. */
enum {
    T1D_P_X0 = 0,
    T1D_P_BW = 13, T1D_P_KABS, T1D_P_KMAX, T1D_P_KMIN, T1D_P_B, T1D_P_D, T1D_P_VG, T1D_P_VI,
    T1D_P_VMX, T1D_P_KM0, T1D_P_K2, T1D_P_K1, T1D_P_P2U, T1D_P_M1, T1D_P_M2, T1D_P_M4, T1D_P_M30,
    T1D_P_IB, T1D_P_KI, T1D_P_KP2, T1D_P_KP3, T1D_P_F, T1D_P_KE1, T1D_P_KE2, T1D_P_FSNC,
    T1D_P_VM0, T1D_P_KD, T1D_P_KSC, T1D_P_KA1, T1D_P_KA2, T1D_P_KP1, T1D_P_U2SS,
    T1D_P_NCOLS                                          /* = 45 */
};
/* sensor row (params/sensor_params.csv): PACF, gamma, lambda, delta, xi, sample_time, min, max */
#define T1D_SENSOR_NCOLS 8
/* pump row (params/pump_params.csv): min_bolus, max_bolus, inc_bolus, min_basal, max_basal, inc_basal */
#define T1D_PUMP_NCOLS 6

/* per-env packed integer word `meta`: bits 0-7 patient row, bit 8 "was eating last minute"
 * (t1dpatient.py:88,102 edge detector), bit 9 "planned_meal > 0" (with bit 8: the three meal words are live -- while
 * both are clear the next minute needs nothing of them but Dbar), bits 16-31 cursor into the meal table. */
#define T1D_META_PID(m)      ((m) & 0xffu)
#define T1D_META_EATING      0x100u
#define T1D_META_PLANNED     0x200u
#define T1D_META_CURSOR(m)   ((m) >> 16)

/* t1d_batch.flags; any other bit is rejected with T1D_E_INVALID */
enum {
    /* skip the InsulinPump quantiser: insulin = basal + bolus exactly as given (drives the patient model
     * the way T1DPatient.step(Action(CHO, insulin)) does, t1dpatient.py:82) */
    T1D_BATCH_NO_PUMP = 2,
    /* the caller vouches that no env starts a new 150-minute CGM-noise block during this t1d_step call
     * (e.g. all envs were reset together and the host tracks the clock): skips the refill pre-kernel */
    T1D_BATCH_NO_REFILL_DUE = 4
};

typedef struct t1d_ctx t1d_ctx;

typedef struct t1d_batch {
    int64_t n;                /* envs in this batch (this GPU's shard) */
    int64_t env_offset;       /* global index of env 0: Philox subsequence = env_offset + i */
    int32_t dtype;            /* T1D_F64 | T1D_F32 */
    int32_t n_meals;          /* rows of the meal table (0 = none) */
    int32_t n_normals;        /* rows of `normals` (0 = draw in-kernel with Philox) */
    int32_t flags;            /* T1D_BATCH_* */
    uint64_t seed;            /* Philox key */
    /* ---- state (read + written by t1d_step; written by t1d_reset).
     * PACKED layout (recommended; detected from the pointers): x, planned, last_qsto, last_food, last_cgm,
     * prev_risk, pts, dbar are consecutive rows of ONE [45][n] buffer in that order, and t, meta, next_meal are
     * consecutive rows of one [3][n] int32 buffer.  With it one-minute launches (minutes == 1) take the
     * persistent single-minute kernels and large fp64 batches the persistent multi-minute kernel; any other layout
     * runs the generic step kernel. */
    void* x;                  /* [13][n] ODE state */
    void* planned;            /* [n] planned_meal, g        (t1dpatient.py:229) */
    void* last_qsto;          /* [n] mg                     (t1dpatient.py:90)  */
    void* last_food;          /* [n] g                      (t1dpatient.py:99)  */
    int32_t* t;               /* [n] minutes since episode start */
    uint32_t* meta;           /* [n] packed: patient row | eating flag | meal cursor */
    uint32_t* episode;        /* [n] episode counter, pre-incremented by t1d_reset; separates the Philox
                                 streams of successive episodes of one env.  NULL = always 0 */
    int32_t* next_meal;       /* [n] minute of the next meal-table entry (INT32_MAX = none), maintained by
                                 t1d_reset/t1d_step so the common minute needs no table access.  NULL = the
                                 table row at the cursor is read every minute instead */
    void* last_cgm;           /* [n] sensor zero-order hold (cgm.py:32-36); never read with a 1-minute sensor, and then
                               * not maintained by one-minute launches (the observation is in cgm) */
    void* ar_e;               /* [n] AR(1) noise state      (noise_gen.py:86-88) */
    void* pts;                /* [26][n] CGM-noise spline of the current 150-min block: rows 0-10 the Johnson-SU
                                 points, 11-21 their knot second derivatives, 22-25 the current 15-min interval */
    void* prev_risk;          /* [n] risk index of CGM_hist[-1]: the default reward risk_diff (env.py:27-33) is
                               * risk(CGM_hist[-2]) - risk(CGM_hist[-1]); its first term is the second term of the step before */
    void* dbar;               /* [n] Dbar = last_qsto + last_food * 1000 (t1dpatient.py:130), kept beside the two words it is
                               * made of: in the minutes in which an env neither eats nor has a meal planned (bits 8, 9 of
                               * meta clear: ~95 %) the gastric-emptying term needs nothing else of the meal bookkeeping, and
                               * the one-minute kernels then read this word instead of three.  Written by t1d_reset and by
                               * every step that changes last_qsto / last_food.  NULL = not kept (never with the packed layout) */
    /* ---- inputs */
    const void* basal;        /* [n] U/min */
    const void* bolus;        /* [n] U/min, NULL = 0 */
    const void* cho;          /* [minutes][n] announced grams per minute, NULL = use meal table */
    const int32_t* meal_time; /* [n_meals][n] minute since episode start, ascending per env;
                                 unused slots = INT32_MAX; at most one entry per minute */
    const void* meal_amt;     /* [n_meals][n] grams */
    const void* normals;      /* [n_normals][n] standard normals in draw order (exact-parity mode) */
    const void* x0_override;  /* [13][n] initial state for t1d_reset, NULL = table x0 */
    /* ---- outputs (any of lbgi..cgm0 may be NULL) */
    void* cgm;                /* [n] observation: mean CGM over the step (env.py:81) */
    void* bg;                 /* [n] mean Gsub over the step (env.py:80) */
    void* reward;             /* [n] risk_diff */
    uint8_t* done;            /* [n] bg < 70 or bg > 350 */
    void* lbgi; void* hbgi; void* risk;   /* [n] risk_index([bg], 1) */
    void* meal;               /* [n] mean announced CHO (env.py:78) */
    void* insulin;            /* [n] mean pump output (env.py:79) */
    void* cgm0;               /* [n] written by t1d_reset only: CGM sample #0, the CGM_hist[0] of env.py:126 (may be NULL) */
} t1d_batch;

typedef struct t1d_pid {
    double P, I, D, target;   /* controller/pid_ctrller.py:7-15 */
    void* integ;              /* [n] integrated_state */
    void* prev;               /* [n] prev_state */
    /* optional per-env accumulators over the roll-out (NULL to skip) */
    void* sum_risk;           /* [n] += risk each step */
    void* min_bg; void* max_bg;   /* [n] */
    int32_t* n_low;           /* [n] += (bg < 70)  per step */
    int32_t* n_high;          /* [n] += (bg > 180) per step */
    /* optional history on the device (NULL to skip): row trace_row + s receives step s of this call */
    void* bg_trace;           /* [rows][n] mean BG of every step   (the BG column of show_history(), env.py:169-180) */
    void* cgm_trace;          /* [rows][n] observation of every step (the CGM column) */
    void* cho_trace;          /* [rows][n] mean announced CHO, g/min  (the CHO column) */
    void* insulin_trace;      /* [rows][n] mean pump output, U/min    (the insulin column) */
    int64_t trace_row;
} t1d_pid;

/* The PID controller's four numbers per env (t1d_rollout_pid_gains, t1d_rollout_pid_dopri5_gains): device arrays of n words in
 * the batch's dtype, read only.  All four must be set; a caller with one value for every env fills an array with it. */
typedef struct t1d_pid_gains {
    const void* P;            /* [n] */
    const void* I;            /* [n] */
    const void* D;            /* [n] */
    const void* target;       /* [n] */
} t1d_pid_gains;

/* BBController (controller/basal_bolus_ctrller.py:15-80) for closed-loop roll-outs: per-env constants the
 * host takes from vpatient_params.csv / Quest.csv (unknown patients: CR 1/15, CF 1/50, basal 1.43*57/6000,
 * :61-64) and one word of state. */
typedef struct t1d_bb {
    double target;            /* 140 mg/dL (:21) */
    const void* basal;        /* [n] u2ss * BW / 6000 U/min (:64) */
    const void* cr;           /* [n] Quest.csv CR, g/U */
    const void* cf;           /* [n] Quest.csv CF, mg/dL/U */
    void* prev_meal;          /* [n] state: info['meal'] of the previous step, g/min (0 after reset) */
    /* optional per-env accumulators over the roll-out (NULL to skip), as in t1d_pid */
    void* sum_risk; void* min_bg; void* max_bg; int32_t* n_low; int32_t* n_high;
    /* optional history on the device, as in t1d_pid */
    void* bg_trace; void* cgm_trace; void* cho_trace; void* insulin_trace; int64_t trace_row;
} t1d_bb;

/* A feed-forward policy for closed-loop roll-outs (t1d_rollout_mlp), evaluated once per env and step from what the roll-out
 * holds: the controller slot of SimObj.simulate (sim_engine.py:29-39) filled by a network instead of PIDController.policy
 * (pid_ctrller.py:17-36) or BBController.policy (basal_bolus_ctrller.py:34-80).  Floating arrays have the batch's dtype.
 * Features, H = history, F = 2 H + 3, in this order:
 *   k = 0 .. H-1   (CGM[-k] - cgm_mean) * cgm_scale: CGM[0] the observation the step starts from (batch.cgm on entry, as for
 *                  t1d_rollout_pid; env.py:81,142), CGM[-k] the observation k steps earlier
 *   k = 0 .. H-1   INS[-1-k] * ins_scale: the mean pump output of the k-th previous step, U/min -- info["insulin"], after
 *                  the quantiser (env.py:79; pump.py:23-39)
 *   prev_meal * cho_scale: the previous step's mean announced CHO, g/min (info["meal"], env.py:78; the word
 *                  basal_bolus_ctrller.py:38 reads; 0 after reset)
 *   sin(2 pi m / 1440), cos(2 pi m / 1440), m = (start_minute[i] + t[i]) mod 1440 at the start of the step
 * Layers: n_layers dense layers of width[l] outputs; width[n_layers - 1] == 1.  params holds, for each policy, the layers in
 * order, each as row-major W[out][in] followed by b[out]: n_params = sum over l of width[l] * (in_l + 1), in_0 = F, in_l =
 * width[l - 1].  Accumulation order, part of the contract so that a host can restate it: acc = b[o], then for j = 0, 1, ..
 * ascending acc = fma(W[o][j], in[j], acc).  Hidden activation (one for the whole net): tanh(v) = sign(v) (1 - E) / (1 + E),
 * E = exp(-2 |v|), or relu(v) = max(v, 0).  Output: basal = fma(out_scale, g(y), out_bias), g(y) = y or the logistic
 * 1 / (1 + exp(-y)); bolus = 0 (the *_bolus calls: the meal bolus of t1d_meal_bolus below); then the pump quantiser and the
 * step exactly as in t1d_step.
 * Env i uses policy i / envs_per_policy; batch.n == n_policies * envs_per_policy; envs_per_policy is a multiple of 64 (a
 * wave, and a 64-env chunk, has one weight set).
 * State: cgm_hist [H][n] and ins_hist [H][n], row k = CGM[-k] / INS[-1-k], read and written, shifted once per step (row 0 of
 * cgm_hist is taken from batch.cgm on entry); prev_meal [n].  A roll-out cut anywhere and resumed with them gives the same
 * words.  After t1d_reset: every row of cgm_hist = the reset observation, ins_hist = 0, prev_meal = 0. */
enum { T1D_MLP_TANH = 0, T1D_MLP_RELU = 1 };          /* t1d_mlp.hidden_act */
enum { T1D_MLP_IDENTITY = 0, T1D_MLP_LOGISTIC = 1 };  /* t1d_mlp.out_act */
typedef struct t1d_mlp {
    int32_t history;          /* H, 1 .. 12 */
    int32_t n_layers;         /* 1 .. 4 */
    int32_t width[4];         /* 1 .. 32 each, the last used one == 1; unused entries 0 */
    int32_t hidden_act;       /* T1D_MLP_TANH | T1D_MLP_RELU */
    int32_t out_act;          /* T1D_MLP_IDENTITY | T1D_MLP_LOGISTIC */
    int64_t n_policies;
    int64_t envs_per_policy;
    int64_t n_params;         /* words of one policy's weight set (checked against the widths) */
    double cgm_mean, cgm_scale, ins_scale, cho_scale, out_scale, out_bias;
    const void* params;       /* [n_policies][n_params] */
    void* cgm_hist;           /* [H][n] state */
    void* ins_hist;           /* [H][n] state */
    void* prev_meal;          /* [n] state */
    const int32_t* start_minute;   /* [n] minute of day at which the env's episode started, NULL = 0 */
    /* optional per-env accumulators over the roll-out (NULL to skip), as in t1d_pid */
    void* sum_risk; void* min_bg; void* max_bg; int32_t* n_low; int32_t* n_high;
    /* optional history on the device, as in t1d_pid; action_trace [rows][n]: the basal the network asked for, before the pump */
    void* bg_trace; void* cgm_trace; void* cho_trace; void* insulin_trace; void* action_trace; int64_t trace_row;
} t1d_mlp;

/* A hybrid closed loop: the network of t1d_mlp commands the basal rate, and a bolus calculator doses each announced meal by
 * BBController's rule (basal_bolus_ctrller.py:64-79) -- the rule of t1d_rollout_bb -- from words the step already holds.
 * Before every step of env i, after the network has produced its basal u (the exploration term of t1d_collect included):
 *   obs   = CGM[0]                        the observation the step starts from (what the features read)
 *   pm    = prev_meal                     mean announced CHO of the previous step, g/min (t1d_mlp.prev_meal)
 *   st    = the sensor's sample time, minutes
 *   corr  = obs > 150 ? (obs - target) / cf[i] : 0
 *   bolus = pm > 0 ? ((pm * st) / cr[i] + corr) / st : 0        U/min
 * in this operation order, every operation rounded once in the batch's dtype: the expressions of t1d_rollout_bb, so that under
 * a network whose output is the patient's basal rate the roll-out is t1d_rollout_bb's, bit for bit.  u and bolus then go through
 * the pump and the step exactly as t1d_step takes basal and bolus.  A restarted env (T1D_COLLECT_RESTART) has prev_meal = 0,
 * hence no bolus on its first step.  A NaN in pm or obs gives bolus 0 through the comparisons; a non-finite network output
 * raises what it raises without the bolus (T1D_ST_NONFINITE; in the exact mode the solver gives up on the NaN insulin and the
 * state stays: T1D_ST_SOLVER_FAILED), and the bolus of that step is still the rule's finite word.  The bolus is a deterministic function of the state: the policy's density, eps,
 * the features, t1d_mlp_grad, t1d_mlp_loss and t1d_gae are untouched.  cr, cf and bolus_trace have the batch's dtype. */
typedef struct t1d_meal_bolus {
    double target;        /* BBController.target, 140 mg/dL */
    const void* cr;       /* [n] carbohydrate ratio, g/U */
    const void* cf;       /* [n] correction factor, mg/dL/U */
    void* bolus_trace;    /* [rows][n] or NULL: row mlp.trace_row + s = the bolus of step s, before the pump */
} t1d_meal_bolus;

/* Per-env outcome statistics of a BG history kept on the device (analysis/report.py), one lane per env:
 *   counts     int32 [5][n]: samples with BG > 180, BG < 70, 70 <= BG <= 180, BG > 250, BG < 50  (percent_stats,
 *              report.py:74-92; divide by n_rows for the percentages)
 *   pct        [2][n]: np.percentile(BG, q_lo) and (BG, q_hi) per env: the order statistics a, b at rank
 *              floor(pos) and the next, pos = (n_rows - 1) q / 100, are found exactly (radix selection) and
 *              interpolated in fp64 as numpy's 'linear' method does.  Against the exact a + (b - a)(pos - floor(pos))
 *              the result is within (2 pos + 3) u |b - a| + (2 u + u_T) |pct|, u = 2^-53, u_T = 0 (fp64) or 2^-24
 *              (fp32), unless it underflows; numpy's own result meets the same bound and may differ in the last bits
 *              (it forms (n_rows - 1) (q / 100)).  A column that holds a NaN has NaN percentiles, as in numpy.  Between
 *              equal order statistics the result is that value (b == a -> a), also for infinities, where numpy's lerp
 *              gives NaN (inf - inf).
 *              zone uint8 [n]: CVGA zone 0..4 = A..E, 5 = none, from the clipped percentiles (CVGA_analysis,
 *              report.py:198-217; q = 2.5 / 97.5 there); NaN percentiles are in no zone (5)
 *   risk_trace [n_chunks][2][n]: LBGI and HBGI of every chunk of `chunk` samples, from the chunk mean of
 *              f(BG) = 1.509 (ln(BG)^1.084 - 5.381) over BG > 0 (risk_index_trace, report.py:95-110; chunk = 60);
 *              NaN samples and 0 < BG < 1 are skipped as BG <= 0 is, a chunk without a usable sample is NaN, and a
 *              chunk that holds +Inf reads LBGI = 0, HBGI = +Inf
 * A NaN sample is counted in no range.  Any output pointer may be NULL.  n_chunks = ceil(n_rows / chunk). */
typedef struct t1d_outcome {
    int32_t* counts; void* pct; uint8_t* zone; void* risk_trace;
    double q_lo, q_hi;
    int32_t chunk;
} t1d_outcome;

/* t1d_restart_done: what a restarted env needs besides the batch.  Floating arrays have the batch's dtype. */
typedef struct t1d_restart {
    int32_t days;             /* horizon of the meal tables: rows = 6 (days + 1) = batch.n_meals */
    int32_t random_init_bg;   /* as t1d_reset */
    int32_t reset_outputs;    /* 0 = of the outputs only cgm is written for a restarted env; bg, reward, done, lbgi, hbgi, risk,
                                 meal, insulin keep what the finished step left (the terminal transition a gym caller gets
                                 back with the new observation).  non-zero = they are written as t1d_reset writes them */
    int32_t reserved;         /* 0 */
    int32_t* meal_time;       /* the batch's own tables, writable: [rows][n] (== batch.meal_time) */
    void* meal_amt;           /* (== batch.meal_amt) */
    int32_t* start_minute;    /* [n] minute of day at which the env's current episode started; written for restarted envs */
    double* h_carry;          /* [n] or NULL: zeroed for restarted envs (t1d_step_dopri5) */
    void* terminal_cgm;       /* [n] or NULL: observation of the finished step, written for restarted envs only */
    void* ep_return;          /* [n] or NULL: running sum of reward over the env's current episode, += batch.reward in every call */
    int32_t* ep_length;       /* [n], with ep_return: steps of the current episode, += 1 in every call */
    void* last_return;        /* [n] or NULL (needs ep_return): ep_return of the env's last finished episode */
    int32_t* last_length;     /* [n] or NULL (needs ep_return): ep_length of it */
} t1d_restart;

/* t1d_collect_mlp: what a policy-gradient trainer needs of a roll-out under t1d_mlp besides the roll-out itself.  Floating
 * arrays have the batch's dtype. */
enum { T1D_COLLECT_CONTINUE = 0, T1D_COLLECT_RESTART = 1 };   /* t1d_collect.on_done */
typedef struct t1d_collect {
    uint64_t explore_seed;    /* Philox key of the exploration draws; its own key, not batch.seed */
    const void* sigma;        /* [n_policies]: std of the noise added to the network's output before the output function;
                                 NULL = no noise (no draw is made) */
    int32_t on_done;          /* T1D_COLLECT_CONTINUE: episodes never end (as t1d_rollout_mlp); T1D_COLLECT_RESTART: an env whose
                                 step comes back done starts its next episode before its next step, exactly as
                                 t1d_restart_done would */
    int32_t reserved;         /* 0 */
    const t1d_restart* restart;   /* on_done = T1D_COLLECT_RESTART: as for t1d_restart_done (h_carry must be NULL; in
                                     t1d_collect_mlp_dopri5 / t1d_collect_pid_dopri5 / t1d_collect_bb_dopri5 NULL or the
                                     call's h_carry); else ignored */
    /* optional histories, rows as the traces of t1d_mlp (row mlp.trace_row + s = step s of this call), NULL to skip */
    void* reward_trace;       /* [rows][n]    risk_diff of every step: what batch.reward would hold after that step */
    uint8_t* done_trace;      /* [rows][n]    batch.done of every step */
    void* eps_trace;          /* [rows][n]    the standard normal drawn for the step (0 where sigma is NULL) */
    void* feat_trace;         /* [rows][F][n] the F = 2 H + 3 features the network was given, in t1d_mlp's order */
} t1d_collect;

/* t1d_mlp_grad: the rows of a collected batch the network is evaluated on again, and what comes back.  Floating arrays
 * have the call's dtype. */
typedef struct t1d_mlp_batch {
    int64_t n_rows;           /* K >= 1 */
    const void* feat;         /* [n_rows][F][n]: rows of t1d_collect.feat_trace, F = 2 H + 3 */
    const void* coef;         /* [n_rows][n] or NULL: dL/dy of every sample */
    void* y;                  /* [n_rows][n] or NULL: the last layer's output, before noise and output function */
    void* grad;               /* [n_policies][n_params] or NULL (needs coef), OVERWRITTEN: grad[p][q] = sum over the rows s and
                                 the envs i of policy p of coef[s][i] * d y[s][i] / d params[p][q] */
    void* workspace;          /* device scratch for the partial sums; needed with grad */
    int64_t workspace_bytes;  /* at least t1d_mlp_grad_workspace() */
} t1d_mlp_batch;

/* t1d_mlp_loss: t1d_mlp_batch with the loss in place of coef.  Floating arrays have the call's dtype.  The struct shares its
 * name with the function, so it has no typedef: write `struct t1d_mlp_loss`. */
enum { T1D_LOSS_PPO_CLIP = 1, T1D_LOSS_VALUE_MSE = 2 };       /* t1d_mlp_loss.kind */
struct t1d_mlp_loss {
    int64_t n_rows;           /* K >= 1 */
    int32_t kind;             /* T1D_LOSS_PPO_CLIP | T1D_LOSS_VALUE_MSE */
    int32_t reserved;         /* 0 */
    const void* feat;         /* [n_rows][F][n], as t1d_mlp_batch.feat */
    /* T1D_LOSS_PPO_CLIP (else ignored) */
    const void* eps;          /* [n_rows][n] rows of t1d_collect.eps_trace */
    const void* y_old;        /* [n_rows][n] the collector's y: one y-only call under the collector's weights */
    const void* adv;          /* [n_rows][n] advantages */
    const void* sigma_old;    /* [n_policies] device, the call's dtype: t1d_collect.sigma of the collect call, > 0 */
    const void* sigma;        /* [n_policies] device, the call's dtype: the sigma being trained, > 0 (may be sigma_old) */
    /* T1D_LOSS_VALUE_MSE (else ignored) */
    const void* target;       /* [n_rows][n] the critic's regression target (t1d_gae_batch.ret) */
    double clip;              /* PPO: in (0, 1) */
    double scale;             /* finite: what every coef is multiplied by, 1 / (n_rows * n) for a mean */
    /* outputs, each optional, not all NULL */
    void* y;                  /* [n_rows][n] as t1d_mlp_batch.y */
    void* coef_out;           /* [n_rows][n] scale * d loss_i / d y of every sample */
    void* grad;               /* [n_policies][n_params] OVERWRITTEN: t1d_mlp_grad's grad for coef = coef_out */
    double* stats;            /* [n_policies][4] OVERWRITTEN, always double, unscaled (below) */
    void* workspace;          /* device scratch for the partial sums; needed with grad or stats */
    int64_t workspace_bytes;  /* at least t1d_mlp_loss_workspace() */
};

/* t1d_mlp_grad_tiles / t1d_mlp_loss_tiles: the minibatch of a call, as a list of tiles per policy.  A tile is the 64 envs of
 * one 64-env chunk of one policy in one row, numbered u = row * C + chunk, C = envs_per_policy / 64 (the unit t1d_mlp_grad's
 * summation order is stated in). */
typedef struct t1d_tile_list {
    int64_t n_tiles;          /* M >= 1: list positions per policy */
    const int32_t* tiles;     /* device, [n_policies][M]: tile ids u = row * C + chunk of that policy; an id < 0 or >= C *
                                 n_rows is skipped */
} t1d_tile_list;

/* t1d_gae: one collected batch of rewards, dones and the critic's values, and what comes back.  Floating arrays have the
 * call's dtype; done is what t1d_collect.done_trace holds. */
typedef struct t1d_gae_batch {
    int64_t n_rows;            /* K >= 1 */
    int64_t n_policies;        /* >= 1, n % n_policies == 0; only the moments use it */
    double gamma, lambda;      /* each in [0, 1] */
    const void* reward;        /* [K][n] */
    const uint8_t* done;       /* [K][n] or NULL = no episode ends */
    const void* value;         /* [K][n] or NULL = 0: V of the state each step started from */
    const void* last_value;    /* [n] or NULL = 0: V of the state after row K-1 (the bootstrap at the cut) */
    void* adv;                 /* [K][n] or NULL */
    void* ret;                 /* [K][n] or NULL: adv + value, the critic's regression target */
    double* moments;           /* [n_policies][2] or NULL: sum of adv and sum of adv^2 over the policy's K * n/n_policies samples, always double */
    void* workspace; int64_t workspace_bytes;   /* needed with moments */
} t1d_gae_batch;

/* A patient-relative policy output: in the *_rel calls basal = fma(scale[i], g(y), bias[i]) replaces
 * fma(out_scale, g(y), out_bias) of t1d_mlp -- one weight set then commands "a multiple of the patient's own basal rate" for a
 * cohort whose basal rates differ by a factor of four.  t1d_mlp.out_scale and out_bias are not read; g, the accumulation order
 * and the place of the collector's exploration term (in y, before g) are unchanged, and so are the pump, the bolus and the step.
 * Both arrays have the batch's dtype and are read per env, never per wave.  A non-finite scale or bias raises what a non-finite
 * network output raises (T1D_ST_NONFINITE; T1D_ST_SOLVER_FAILED in the exact mode).  The trainer's calls (t1d_mlp_grad,
 * t1d_mlp_loss, t1d_gae, t1d_mlp_features) are untouched: the policy's density lives in y. */
typedef struct t1d_env_output {
    const void* scale;   /* [n], batch dtype */
    const void* bias;    /* [n], batch dtype */
} t1d_env_output;

/* t1d_collect_mlp_limit: episodes with a time limit (max_episode_steps).  cut_feat has the batch's dtype. */
typedef struct t1d_time_limit {
    int32_t max_minutes;   /* >= 1: an episode whose clock t (minutes since its reset) is >= max_minutes when a step closes is cut */
    int32_t reserved;      /* 0 */
    uint8_t* cut_trace;    /* [rows][n] or NULL: 1 where step s was cut (never where done = 1), else 0; rows as t1d_collect's */
    void* cut_feat;        /* [F][n] or NULL, batch dtype: the features of the state a cut episode ended in; written for cut envs only */
} t1d_time_limit;

/* t1d_gae_limit: the second mask of a batch collected under a time limit.  cut_value has the call's dtype. */
typedef struct t1d_gae_cut {
    const uint8_t* truncated;  /* [K][n]: t1d_time_limit.cut_trace */
    const void* cut_value;     /* [n] or NULL = 0, call dtype: V of the state in cut_feat */
} t1d_gae_cut;

int t1d_abi_version(void);
const char* t1d_last_error(void);

/* Build the constant tables of one device.  patient_table: [n_patients][n_cols] (T1D_P_* order,
 * n_cols == T1D_P_NCOLS), sensor_row [T1D_SENSOR_NCOLS], pump_row [T1D_PUMP_NCOLS], all host
 * doubles, copied.  sample_time must be a whole number of minutes in [1, 150].  The cubic-spline
 * interpolation of the CGM noise (noise_gen.py:38-47) is built inside the library. */
int t1d_ctx_create(int hip_device, const double* patient_table, int n_patients, int n_cols,
                   const double* sensor_row, const double* pump_row, t1d_ctx** out);
int t1d_ctx_destroy(t1d_ctx* ctx);

/* Switches of a context.
 * "integrator": how `n_sub` sub-steps per minute replace scipy's dopri5 (t1dpatient.py:110-113,276):
 *   0 = classical RK4 on all 13 states;
 *   1 = the split scheme -- exact propagator for the linear insulin sub-system (:176-198), RK4 for the stomach with the
 *       gut compartment in exponential form (:133-148), RK4 at half as many steps for the glucose states with the
 *       absorbed mass shifted into the state (:151-173,201-202) -- which needs math = 1 and n_sub in {2, 4, 6, 8};
 *   -1 (default) = split whenever those hold, classical RK4 otherwise.
 * "adaptive_gut": step sizes of the split scheme.  1 (default) = per minute and env, by a deterministic rule on the state
 *   and the rates at the start of the minute: level 1 (gut n_sub steps, glucose n_sub/2) unless an argument of the
 *   gastric-emptying tanh pair (t1dpatient.py:138-140) moves fast through its transition, x3 is about to reach 0 (:167) or
 *   insulin action makes the tissue compartment fast (:169-172) -- then level 2 (gut 2 n_sub, glucose n_sub): ~0.7 % of the
 *   env-minutes of RandomScenario days.  Max error against a tight solve 9e-4 mg/dL on random-meal days (level 1
 *   everywhere: 7e-3); a glucose state that reaches 0 is held there as the reference holds it.  In one-minute launches the
 *   lanes of level 2 are set aside and integrated together at the end of the launch, in launches of several minutes they are
 *   parked with their state and finished at the end; in the generic kernels a wave runs at the level of its most refined lane.
 *   0 = level 1 in every minute; 2 = as 1 but in place in every kernel; 3 = as 1, set aside at any batch size (tests).
 * "math": 1 (default) = exp-based gastric-emptying term and Newton-refined reciprocals in the ODE right-hand side;
 *   0 = ocml tanh and IEEE divisions written exactly as t1dpatient.py:138-140,171,178 writes them, classical RK4
 *   (A/B and parity reference).
 * "split_refill": 1 (default) = when a launch takes at most one CGM sample (minutes <= sample_time) the rarely needed
 *   rebuild of the 150-minute noise block runs as its own small kernel ahead of a step kernel compiled without it (its
 *   registers would otherwise cost the step kernel ~20 %); 0 = always inline.
 * "single_minute_kernel": 1 (default) = one-minute launches on the packed layout take the persistent kernels.
 * "s1_blocks": grid of those kernels (0 = one workgroup per compute unit).
 * "defer_min_chunks": threshold (64-env chunks per workgroup) from which the set-aside form is used.
 * "multi_minute_kernel": a step of several minutes (1 < minutes <= sample_time: the reference's Dexcom / GuardianRT
 *   steps, env.py:75-81) on the packed layout in one launch of the persistent multi-minute kernel -- the state stays in
 *   registers across the minutes; a lane that the step-size rule puts at level 2 leaves a record in LDS (its state at the
 *   start of that minute) and the rest of its wave carries on at level 1; waves without a chunk to work on finish the
 *   records, every lane at its own level, beside the last chunks.  1 (default) = batches of "multi_minute_min_envs"
 *   (fp64: 262 144) / "multi_minute_min_envs_f32" (393 216) envs or more, where it beats the generic kernel (Dexcom steps,
 *   us per step, generic / persistent: fp64 96 / 84 at 256 Ki envs, 134 / 93 at 384 Ki, 172 / 117 at 512 Ki, 324 / 209
 *   at 1 Mi; fp32 65 / 59 at 384 Ki, 141 / 117 at 1 Mi; below the thresholds the generic kernel wins: tools/mm_thresholds.py);
 *   0 = never (the generic kernel: a wave runs at the level of its most refined lane); 2 = always.
 *   "park_cap": records per workgroup (0 = what fits in LDS beside the tables; a flagged lane that finds none free is
 *   taken again from its loads at the end of the launch, in place).  "record_group_min" (1..64, default 64): that many
 *   waiting records go ahead of a wave's next chunk (fewer: the records start earlier but in emptier waves -- measured
 *   slower from 512 Ki envs up, 3-5 % faster at 256 Ki).
 * "pingpong": 1 (default) = the persistent kernels walk every compute unit's chunks from the last to the first in every
 *   other launch, so that a launch starts on the lines the launch before it touched last -- what the 256 MB Infinity Cache
 *   in front of HBM still holds (walked in the same order every launch, a working set of about the cache's size is the
 *   pattern an LRU cache serves worst).  One-minute launches: no difference at 1 Mi fp64 envs, 5 % faster at 2 Mi, 8 % at
 *   4 Mi (80 us per Mi envs).  Results do not depend on it.  0 = always first to last.
 * "rollout_launches": t1d_rollout_pid / t1d_rollout_bb as one launch of that kernel per step, the controller fused into
 *   it: 1 (default) = batches of "rollout_launches_min_envs" (fp64: 524 288) / "rollout_launches_min_envs_f32" (786 432)
 *   envs or more; 0 = never (all steps inside one launch of the generic roll-out kernel); 2 = always. */
int t1d_ctx_set_option(t1d_ctx* ctx, const char* name, int64_t value);

/* Host-only helper (no device needed): the tables of the split integrator for one patient row
 * (T1D_P_* order, n_cols == T1D_P_NCOLS) and n_sub in {2, 4, 6, 8}: 28 n_sub + 21 entries of the insulin propagator
 * Phi(k / (2 n_sub)), k = 1 .. 2 n_sub (layout in simglucose_amd/csrc/t1d_device.hpp), followed by the four weights
 * E, wa, wm, wb of the exponential gut update for the gut step of level 1 (h = 1/n_sub) and of level 2 (h/2);
 * out_len >= 28 n_sub + 29.  What t1d_step uploads; exposed so that the tables can be checked against
 * an independent matrix exponential. */
int t1d_split_tables(const double* patient_row, int n_cols, int n_sub, double* out, int out_len);

/* Reset the envs whose mask byte is non-zero (mask == NULL: all).  Outputs as after
 * T1DSimEnv.reset(): cgm = CGM sample #1, cgm0 = CGM sample #0 (prev_risk = its risk index), bg/lbgi/hbgi/risk of the
 * initial state, reward 0, done 0.  random_init_bg != 0 draws x[3], x[4], x[12] ~ N(mu, 0.1 mu)
 * with Philox (statistical counterpart of t1dpatient.py:256-270; exact parity = x0_override). */
int t1d_reset(t1d_ctx* ctx, const t1d_batch* b, const uint8_t* mask, int random_init_bg, void* hip_stream);

/* Advance every env by `minutes` (normally int(sample_time)) with one kernel launch, the same
 * action held for the whole call; integrator and step sizes as set on the context, built on n_sub sub-steps per minute. */
int t1d_step(t1d_ctx* ctx, const t1d_batch* b, int minutes, int n_sub, void* hip_stream);

/* SciPy's DOPRI5 as the reference drives it (t1dpatient.py:110-113,276; rtol 1e-6, atol 1e-12, re-entered every minute,
 * predicted step carried between minutes).  fp64 batches only.  h_carry: device double [n], the predicted step of each env,
 * read and written; 0 = probe for an initial step (what the reference does after reset -- the caller zeroes it for every
 * env it resets).  nfev: device int32 [n] or NULL, RHS evaluations of each env in this call.  Any state layout.
 * Otherwise as t1d_step (n_sub does not apply).  One lane per env runs its own accept/reject loop, so a launch lasts as long
 * as the slowest env of each wave: on random-meal days 10.5 RHS evaluations per env-minute on average, 46.9 for the
 * slowest lane of a wave (1 Mi fp64 envs: 3.6 ms per one-minute launch).
 * An env whose solver gives up (500 steps in a minute, or a step below the resolution of t) keeps its last accepted
 * state for the rest of the call and raises T1D_ST_SOLVER_FAILED.  Closed-loop roll-outs in this mode: t1d_rollout_pid_dopri5 /
 * t1d_rollout_bb_dopri5 below. */
int t1d_step_dopri5(t1d_ctx* ctx, const t1d_batch* b, double* h_carry, int32_t* nfev, int minutes, void* hip_stream);

/* n_steps closed-loop steps in ONE launch: basal = PID(obs CGM), bolus = 0, then as t1d_step.
 * b->cgm must hold the current observation on entry (as left by t1d_reset / t1d_step). */
int t1d_rollout_pid(t1d_ctx* ctx, const t1d_batch* b, const t1d_pid* pid, int n_steps, int minutes,
                    int n_sub, void* hip_stream);

/* t1d_rollout_pid with a controller of its own for every env: env i computes PIDController.policy (pid_ctrller.py:17-36) with
 * gains.P[i], gains.I[i], gains.D[i] and gains.target[i] -- what batch_sim computes for a list of SimObj, each with its own
 * PIDController(P, I, D, target).  The four scalars pid.P, pid.I, pid.D and pid.target are NOT read; everything else of pid
 * (integ, prev, the accumulators, the trace columns, trace_row) means what it means in t1d_rollout_pid, as do the other
 * arguments, the plan and the state left behind.  The expression, its arithmetic and its contraction are those of the scalar
 * call: env i of a mixed batch is, bit for bit, env i of the same batch run by t1d_rollout_pid under
 * (P[i], I[i], D[i], target[i]), whichever kernel the plan picks.  The launch-per-step form reads the four words once per
 * env and step (and target once more when the step ends), the all-steps-in-one-launch form once per call.
 * T1D_E_INVALID, before the batch is looked at and before anything is launched: pid or its state NULL, as t1d_rollout_pid;
 * gains NULL, or any of its members NULL (the message names the member).  Then whatever t1d_rollout_pid rejects. */
int t1d_rollout_pid_gains(t1d_ctx* ctx, const t1d_batch* b, const t1d_pid* pid, const t1d_pid_gains* gains, int n_steps,
                          int minutes, int n_sub, void* hip_stream);

/* SimObj.simulate (sim_engine.py:29-39) with BBController for n_steps env.steps in ONE launch: per step
 * basal = bb.basal; bolus = (prev_meal*sample_time/CR + (CGM > 150)*(CGM - target)/CF) / sample_time if
 * prev_meal > 0 else 0 (basal_bolus_ctrller.py:66-79), where CGM is the previous step's observation (batch.cgm on
 * entry) and prev_meal the previous step's mean announced CHO; then the same step as t1d_step with meals from the
 * meal tables.  Outputs/state as t1d_rollout_pid; bb.prev_meal is updated. */
int t1d_rollout_bb(t1d_ctx* ctx, const t1d_batch* batch, const t1d_bb* bb, int n_steps, int minutes,
                   int n_sub, void* stream);

/* SimObj.simulate (sim_engine.py:29-39) with the policy of t1d_mlp for n_steps env.steps in ONE launch, the env state in
 * registers, the two windows and the layer activations in LDS, the weights through the scalar data cache.  fp64 and fp32, any
 * state layout, the fixed-step integrators as configured on the context (the exact mode: t1d_rollout_mlp_dopri5), meals from the
 * meal tables.  Outputs, state and the last step's reward as t1d_rollout_pid; mlp.cgm_hist / ins_hist / prev_meal are
 * updated.  Anything out of range -- history, n_layers, a width, an activation code, a NULL array, n_params, or
 * n != n_policies * envs_per_policy -- is T1D_E_INVALID before anything is launched. */
int t1d_rollout_mlp(t1d_ctx* ctx, const t1d_batch* batch, const t1d_mlp* mlp, int n_steps, int minutes,
                    int n_sub, void* stream);

/* t1d_rollout_mlp as a policy-gradient trainer collects a batch of trajectories: n_steps steps in ONE launch, the env state in
 * registers, windows and activations in LDS, the weights through the scalar data cache, with exploration noise, the reward and
 * done of every step, the features the network saw, and episodes that end and start again without leaving the device.
 * Action: y = the last layer's output as in t1d_rollout_mlp; z = fma(sigma[p], eps, y) for the env's policy p (z = y with sigma
 *   NULL); basal = fma(out_scale, g(z), out_bias), bolus = 0.  action_trace holds that basal, before the pump.  The Gaussian
 *   lives in the pre-output space; the log-probability is the host's business, from eps and sigma.
 * Draw: eps = (T) philox_pair(explore_seed, g, k, m).x -- the first normal of Philox block m of episode k of subsequence g (the
 *   layout of t1d_philox_normals) -- with g = env_offset + i, k the env's batch.episode counter at that step (0 with a NULL
 *   array) and m the env's t at the start of the step, minutes since its episode began (m < 2^24: an episode of 31 years).  It
 *   depends on nothing else, so a roll-out cut anywhere, sharded anywhere or with other neighbours draws the same numbers.
 *   A caller who passes batch.seed as explore_seed makes eps the normal the sensor noise takes from the same block: exploration
 *   then correlates with the CGM noise.
 * on_done = T1D_COLLECT_RESTART: after a step with done != 0 the env goes through what t1d_restart_done(mask = done,
 *   reset_outputs as given) does to it -- the episode accumulators of t1d_restart advance every step for every env,
 *   terminal_cgm is written, the env gets a new start hour, a new column of the meal tables, a reset and episode + 1 -- and
 *   its policy state becomes what follows a reset: every cgm_hist row the new first observation, ins_hist = 0, prev_meal = 0,
 *   the time-of-day features from the new start_minute (mlp.start_minute is restart.start_minute, or NULL).  Trace rows of
 *   step s always describe step s: cgm_trace[s] is the terminal observation of an env that finished there, the new episode's
 *   first observation shows in feat_trace[s + 1] and in batch.cgm.
 * After the call batch.*, the env state, mlp.cgm_hist / ins_hist / prev_meal and the sum_risk .. n_high accumulators (which run
 *   on across episodes) are what n_steps x (t1d_rollout_mlp(1), t1d_restart_done, the reset of the policy state of the envs
 *   that were done) leave, bit for bit; with sigma NULL and T1D_COLLECT_CONTINUE, what t1d_rollout_mlp leaves.
 * T1D_E_INVALID before anything is launched, nothing changed: whatever t1d_rollout_mlp rejects; with T1D_COLLECT_RESTART
 *   whatever t1d_restart_done rejects (a NULL batch.episode, tables that are not the batch's own, n_meals != 6 (days + 1), host
 *   normals, x0_override), a NULL restart and a non-NULL restart->h_carry (the exact mode's collector is
 *   t1d_collect_mlp_dopri5); on_done outside {0, 1}; reserved != 0. */
int t1d_collect_mlp(t1d_ctx* ctx, const t1d_batch* batch, const t1d_mlp* mlp, const t1d_collect* collect, int n_steps,
                    int minutes, int n_sub, void* stream);

/* t1d_rollout_pid / t1d_rollout_bb with what t1d_collect_mlp adds: trajectories collected while a classical controller drives
 * the envs -- the data a network is fitted to before it explores (behaviour cloning), and the return and length of the
 * controller under the collectors' episode rules.  n_steps steps in ONE launch, the env state in registers, the two feature
 * windows and the features in LDS (4 H + 3 words per lane).  fp64 and fp32, any state layout, the fixed-step integrators as
 * configured on the context, meals from the meal tables.
 * Controller: the struct's gains or constants, its state (integ / prev, prev_meal), its accumulators, its four traces and its
 *   trace_row mean what they mean in t1d_rollout_pid / t1d_rollout_bb, and the action of a step is the word that entry point
 *   computes from the same observation and state.
 * Features: of feat (a t1d_mlp) only history, cgm_mean, cgm_scale, ins_scale, cho_scale, cgm_hist, ins_hist, prev_meal,
 *   start_minute (NULL = 0) and action_trace are read.  The widths, n_layers, params, the output function, n_policies /
 *   envs_per_policy, its accumulators, its other traces and its trace_row are ignored and may be 0 / NULL; batch.n need not be
 *   a multiple of 64.  Before each step the F = 2 H + 3 features of t1d_mlp are formed by the collectors' own device code --
 *   the words t1d_mlp_features would return at that moment, bit for bit -- and written to collect->feat_trace; the windows and
 *   prev_meal are maintained as in t1d_collect_mlp.
 * Action trace: feat->action_trace[trace_row + s] = basal + bolus of step s, one addition in the batch's dtype, before the
 *   pump; trace_row is the controller's, as for every row of this call.  With the features of the same row it is the
 *   regression sample for a network with identity output.
 * Per step: reward_trace and done_trace as in t1d_collect_mlp.  collect->sigma and collect->eps_trace must be NULL (there is
 *   no exploration noise); explore_seed is ignored.
 * on_done = T1D_COLLECT_RESTART: as in t1d_collect_mlp -- a finished env goes through what t1d_restart_done does to it, its
 *   feature windows become those of a fresh reset, and its controller state becomes what PIDController.reset /
 *   BBController.reset leave: integ = prev = 0, bb.prev_meal = 0.  The ep_return .. last_length accumulators advance as
 *   documented there.
 * Equivalence: after the call the batch, the env state, the controller state, the feature windows, the accumulators, the
 *   restart outputs and every trace row are what n_steps x (t1d_mlp_features; t1d_rollout_pid(1) or t1d_rollout_bb(1) through
 *   the generic roll-out kernel, "rollout_launches" = 0; the shift of the windows with prev_meal = batch.meal;
 *   t1d_restart_done; the reset of the windows and of the controller state of the envs that were done) leave, bit for bit,
 *   wherever the call is cut.  With T1D_COLLECT_CONTINUE the env and the controller end where t1d_rollout_pid(n_steps) /
 *   t1d_rollout_bb(n_steps) leave them.
 * T1D_E_INVALID before anything is launched, nothing changed: whatever t1d_rollout_pid / t1d_rollout_bb rejects; whatever
 *   t1d_collect_mlp rejects of collect and of the fields of feat that are read (history outside [1, 12], a NULL cgm_hist /
 *   ins_hist / prev_meal, with T1D_COLLECT_RESTART a start_minute that is neither NULL nor restart->start_minute); a non-NULL
 *   sigma or eps_trace; a non-NULL restart->h_carry (these two calls run the fixed-step integrators only; the exact mode's
 *   are t1d_collect_pid_dopri5 / t1d_collect_bb_dopri5). */
int t1d_collect_pid(t1d_ctx* ctx, const t1d_batch* batch, const t1d_pid* pid, const t1d_mlp* feat, const t1d_collect* collect,
                    int n_steps, int minutes, int n_sub, void* hip_stream);
int t1d_collect_bb(t1d_ctx* ctx, const t1d_batch* batch, const t1d_bb* bb, const t1d_mlp* feat, const t1d_collect* collect,
                   int n_steps, int minutes, int n_sub, void* hip_stream);

/* SimObj.simulate (sim_engine.py:29-39) with PIDController.policy (pid_ctrller.py:17-36) and the integrator of
 * t1d_step_dopri5, scipy's dopri5 as the reference drives it (t1dpatient.py:110-113,276): t1d_rollout_pid (controller,
 * b->cgm on entry, accumulators, traces, the last step's reward) in the exact mode.  All n_steps steps of `minutes` minutes
 * are ONE launch in which every env walks through its own minutes at its own pace: the body of the kernel's one loop is one
 * step attempt of the driver, and an env that completes a minute finishes it and opens its next one without waiting for the
 * other 63 envs of its wave.  A wave then lasts as long as the env with the largest total of step attempts over the launch,
 * not as the per-minute maxima summed up (random-meal days, RHS evaluations per env-minute: mean 9.7, per-minute maximum of a
 * wave 39.8, largest 240-minute total of a wave 13.8).  Envs never exchange data and the controller is evaluated without FMA
 * contraction, like the solver: the results are those of a loop of t1d_step_dopri5 with the controller computed operation
 * by operation between the calls, bit for bit, whatever the other envs of the batch do.
 * h_carry: device double [n], read and written, 0 = probe (as t1d_step_dopri5); nfev: device int32 [n] or NULL, the RHS
 * evaluations of each env over the whole call.  fp64 batches only; meals from the meal tables.  An env whose solver gives
 * up keeps its last accepted state for the rest of the call (its clock, meals and noise go on) and raises
 * T1D_ST_SOLVER_FAILED; the other envs are unaffected. */
int t1d_rollout_pid_dopri5(t1d_ctx* ctx, const t1d_batch* b, const t1d_pid* pid, double* h_carry, int32_t* nfev,
                           int n_steps, int minutes, void* hip_stream);

/* t1d_rollout_pid_dopri5 with gains.P[i], gains.I[i], gains.D[i] and gains.target[i] for env i, as t1d_rollout_pid_gains
 * has them: the four scalars of pid are NOT read, everything else is t1d_rollout_pid_dopri5's.  The controller is evaluated
 * without FMA contraction, operation by operation, as there: env i is bit for bit env i of the scalar call under its gains.
 * T1D_E_INVALID as t1d_rollout_pid_gains (NULL gains or member, ahead of the batch's checks), then whatever
 * t1d_rollout_pid_dopri5 rejects. */
int t1d_rollout_pid_dopri5_gains(t1d_ctx* ctx, const t1d_batch* b, const t1d_pid* pid, const t1d_pid_gains* gains,
                                 double* h_carry, int32_t* nfev, int n_steps, int minutes, void* hip_stream);

/* The same with BBController (basal_bolus_ctrller.py:34-80; sim_engine.py:29-39; t1dpatient.py:110-113,276): t1d_rollout_bb
 * in the exact mode -- the reference's own regression run (sim_results.csv).  bb.prev_meal is updated. */
int t1d_rollout_bb_dopri5(t1d_ctx* ctx, const t1d_batch* b, const t1d_bb* bb, double* h_carry, int32_t* nfev,
                          int n_steps, int minutes, void* hip_stream);

/* SimObj.simulate (sim_engine.py:29-39) with the policy of t1d_mlp and the integrator of t1d_step_dopri5: t1d_rollout_mlp
 * (features, layers, output function, bolus = 0, windows, prev_meal, accumulators, the five trace columns with action_trace,
 * the last step's reward) in the exact mode, with the solver and the free-running lanes of t1d_rollout_pid_dopri5.  All
 * n_steps steps are ONE launch in which every env walks through its minutes at its own pace; an env that opens a step
 * evaluates the network then, whatever the other 63 envs of its wave are doing.  The two windows (a ring whose head each
 * env keeps for itself) and the layer activations are in LDS, the weights go through the scalar data cache, one set per wave.
 * The action of a step is the word t1d_rollout_mlp and t1d_mlp_action compute from the same windows, prev_meal, clock,
 * start_minute and weights; everything else is what t1d_rollout_pid_dopri5 does.  The results are those of a loop of
 * t1d_mlp_action, t1d_step_dopri5 (bolus = 0), the shift of the windows and prev_meal = batch.meal, bit for bit, whatever
 * the other envs of the batch do and wherever the roll-out is cut.
 * fp64 batches only; meals from the meal tables; every policy t1d_rollout_mlp accepts is accepted (the workgroup shrinks from
 * four waves to two or one where the columns need the room).  h_carry, nfev and T1D_ST_SOLVER_FAILED as in
 * t1d_rollout_pid_dopri5; mlp.cgm_hist / ins_hist / prev_meal are updated (row 0 of cgm_hist is taken from batch.cgm on entry).
 * T1D_E_INVALID before anything is launched, nothing changed: whatever t1d_rollout_mlp rejects and whatever
 * t1d_rollout_pid_dopri5 rejects (an fp32 batch, a NULL h_carry, dense cho, n_steps < 1, minutes out of range). */
int t1d_rollout_mlp_dopri5(t1d_ctx* ctx, const t1d_batch* b, const t1d_mlp* mlp, double* h_carry, int32_t* nfev,
                           int n_steps, int minutes, void* hip_stream);

/* t1d_collect_mlp in the exact mode: the gym training loop of simglucose/envs/simglucose_gym_env.py:39-73 (the action sampled
 * around the network's output, reward and done of every step, reset() when done comes back true) with the integrator of
 * t1d_step_dopri5, scipy's dopri5 as the reference drives it (t1dpatient.py:110-113,276).  All of t1d_collect_mlp's
 * contract -- action, draw, traces, on_done, the accumulators -- on the solver and the free-running lanes of
 * t1d_rollout_mlp_dopri5: ONE launch in which every env walks through its minutes, its steps and its episodes at its own pace.
 * Action: y, z = fma(sigma[p], eps, y) (z = y with sigma NULL), basal = fma(out_scale, g(z), out_bias), bolus = 0, as in
 *   t1d_collect_mlp; y is the word t1d_rollout_mlp_dopri5 and t1d_mlp_action compute.  action_trace holds that basal.
 * Draw: eps = philox_pair(explore_seed, env_offset + i, k, m).x with k the env's batch.episode counter at that step (0 with a
 *   NULL array) and m its t at the start of the step, exactly as in t1d_collect_mlp; no draw and eps_trace = 0 with sigma NULL.
 * Traces: row trace_row + s of reward_trace, done_trace, eps_trace, feat_trace and of the five t1d_mlp columns describes step
 *   s of this call for every env, although the envs reach step s at different moments of the launch.
 * on_done = T1D_COLLECT_RESTART: after a step with done != 0 the env goes through what t1d_restart_done(mask = done,
 *   reset_outputs as given) does to it with restart->h_carry = h_carry: its predicted solver step becomes 0, so the first
 *   minute of the new episode probes, as the reference's solver does after T1DPatient.reset.  Its policy state becomes that of a
 *   fresh reset (every cgm_hist row the new first observation, ins_hist = 0, prev_meal = 0), the time-of-day features come
 *   from the new start_minute and the draw key from the new episode counter.  The episode accumulators of t1d_restart advance
 *   every step for every env.  restart->h_carry must be NULL or h_carry: either way the env's entry of h_carry is zeroed.
 * After the call batch.*, the env state, h_carry, mlp.cgm_hist / ins_hist / prev_meal, the accumulators, the restart outputs
 *   and every trace row are what n_steps x (t1d_rollout_mlp_dopri5(1), t1d_restart_done with h_carry, the reset of the policy
 *   state of the envs that were done) leave, bit for bit, whatever the other envs of the batch do and wherever the call is
 *   cut; with sigma NULL and T1D_COLLECT_CONTINUE, what t1d_rollout_mlp_dopri5 leaves.  nfev: the RHS evaluations of each env
 *   over the whole call, across its episodes.
 * An env whose solver gives up raises T1D_ST_SOLVER_FAILED and keeps its last accepted state while its clock, meals and noise
 *   go on, as in t1d_rollout_mlp_dopri5 -- until the end of the call or of its episode: a restarted env starts its new episode
 *   with a working solver.  The bit-for-bit equivalence above is for envs whose solver does not fail (the loop of one-step
 *   calls tries the solver again in every step).
 * T1D_E_INVALID before anything is launched, nothing changed: whatever t1d_rollout_mlp_dopri5 rejects (an fp32 batch, a NULL
 *   h_carry, dense cho, n_steps < 1, minutes out of range, a bad policy); whatever t1d_collect_mlp rejects of collect (on_done
 *   outside {0, 1}, reserved != 0, with T1D_COLLECT_RESTART a NULL restart, a NULL batch.episode, tables that are not the
 *   batch's own, n_meals != 6 (days + 1), host normals, x0_override); a restart->h_carry that is neither NULL nor h_carry;
 *   with T1D_COLLECT_RESTART an mlp.start_minute that is neither NULL nor restart->start_minute, as in t1d_collect_mlp. */
int t1d_collect_mlp_dopri5(t1d_ctx* ctx, const t1d_batch* b, const t1d_mlp* mlp, const t1d_collect* collect,
                           double* h_carry, int32_t* nfev, int n_steps, int minutes, void* hip_stream);

/* t1d_collect_pid / t1d_collect_bb in the exact mode: trajectories collected while a classical controller drives the envs on
 * scipy's dopri5 as the reference drives it (t1dpatient.py:110-113,276) -- behaviour-cloning samples and the controller's
 * return and length under the collectors' episode rules, on the integrator of t1d_collect_mlp_dopri5; with BBController the
 * reference's own regression run (sim_results.csv).  All of t1d_collect_pid's contract -- the fields of feat that are read,
 * the features, the action trace, reward and done, on_done, the accumulators; no sigma, no eps_trace -- on the solver and the
 * free-running lanes of t1d_rollout_pid_dopri5: ONE launch in which every env walks through its minutes, its steps and its
 * episodes at its own pace.  The two feature windows (a ring whose head each env keeps for itself) and the features are in
 * LDS, 4 H + 3 words per lane.  fp64 batches only; meals from the meal tables; batch.n need not be a multiple of 64.
 * Controller: the struct means what it means in t1d_rollout_pid_dopri5 / t1d_rollout_bb_dopri5, and the basal and bolus of a
 *   step are the words that entry point computes from the same observation and state, without FMA contraction.
 * Features: as in t1d_collect_pid -- of feat only history, the four feature scales, cgm_hist, ins_hist, prev_meal, start_minute
 *   and action_trace are read, the network's fields may hold anything -- and the rows of feat_trace are the words
 *   t1d_mlp_features would return at that moment, bit for bit.
 * Action trace: feat->action_trace[trace_row + s] = basal + bolus of step s, one fp64 addition, before the pump.  trace_row is
 *   the controller's, as for every row of this call: row trace_row + s describes step s for every env, although the envs reach
 *   step s at different moments of the launch.
 * on_done = T1D_COLLECT_RESTART: as in t1d_collect_mlp_dopri5 -- t1d_restart_done with restart->h_carry = h_carry for this env,
 *   so the first minute of its new episode probes; its feature windows become those of a fresh reset and its controller state
 *   what PIDController.reset / BBController.reset leave (integ = prev = 0, bb.prev_meal = 0).  restart->h_carry must be NULL or
 *   h_carry: either way the env's entry of h_carry is zeroed.
 * Equivalence: after the call batch.*, the env state, h_carry, the controller state, the feature windows, the accumulators, the
 *   restart outputs and every trace row are what n_steps x (t1d_mlp_features; t1d_rollout_pid_dopri5(1) or
 *   t1d_rollout_bb_dopri5(1); the shift of the windows with prev_meal = batch.meal; t1d_restart_done with h_carry; the reset of
 *   the windows and of the controller state of the envs that were done) leave, bit for bit, whatever the other envs of the
 *   batch do and wherever the call is cut.  With T1D_COLLECT_CONTINUE the env, the controller state, the accumulators, the
 *   four trace columns, h_carry and nfev are what t1d_rollout_pid_dopri5(n_steps) / t1d_rollout_bb_dopri5(n_steps) leave.
 *   nfev: the RHS evaluations of each env over the whole call, across its episodes.
 * An env whose solver gives up raises T1D_ST_SOLVER_FAILED and keeps its last accepted state while its clock, meals and noise
 *   go on, until the end of the call or of its episode, as in t1d_collect_mlp_dopri5; the equivalence above is for envs whose
 *   solver does not fail.
 * T1D_E_INVALID before anything is launched, nothing changed: whatever t1d_rollout_pid_dopri5 / t1d_rollout_bb_dopri5 rejects
 *   (an fp32 batch, a NULL h_carry, dense cho, n_steps < 1, minutes out of range, NULL controller state); whatever
 *   t1d_collect_pid rejects of feat and collect (history outside [1, 12], a NULL cgm_hist / ins_hist / prev_meal, with
 *   T1D_COLLECT_RESTART a start_minute that is neither NULL nor restart->start_minute, a non-NULL sigma or eps_trace, on_done
 *   outside {0, 1}, reserved != 0, and with T1D_COLLECT_RESTART everything t1d_restart_done rejects); a restart->h_carry that
 *   is neither NULL nor h_carry. */
int t1d_collect_pid_dopri5(t1d_ctx* ctx, const t1d_batch* b, const t1d_pid* pid, const t1d_mlp* feat, const t1d_collect* collect,
                           double* h_carry, int32_t* nfev, int n_steps, int minutes, void* hip_stream);
int t1d_collect_bb_dopri5(t1d_ctx* ctx, const t1d_batch* b, const t1d_bb* bb, const t1d_mlp* feat, const t1d_collect* collect,
                          double* h_carry, int32_t* nfev, int n_steps, int minutes, void* hip_stream);

/* The policy of t1d_mlp alone, one lane per env: action[i] (device [n], the batch's dtype) = the basal, before the pump,
 * that the next step of t1d_rollout_mlp / t1d_rollout_mlp_dopri5 would ask for env i -- from batch.cgm (CGM[0]), rows 1 ..
 * of mlp.cgm_hist, mlp.ins_hist, mlp.prev_meal, batch.t and mlp.start_minute, with the arithmetic of the roll-outs, word for
 * word.  It changes nothing: no state is written and no step is taken (the accumulators and trace pointers of mlp are not
 * used).  fp64 and fp32, any integrator, any state layout.  What a step() loop needs to drive the env with the roll-outs'
 * policy: action, t1d_step / t1d_step_dopri5, then cgm_hist and ins_hist shifted by one row with batch.cgm / batch.insulin
 * in row 0 and prev_meal = batch.meal.  T1D_E_INVALID: a NULL action, and whatever t1d_rollout_mlp rejects of the policy. */
int t1d_mlp_action(t1d_ctx* ctx, const t1d_batch* b, const t1d_mlp* mlp, void* action, void* hip_stream);

/* The features of the step that would come next, one lane per env: feat (device [F][n], F = 2 H + 3, the batch's dtype) = what
 * the next step of t1d_collect_mlp / t1d_collect_mlp_dopri5 would write to its feat_trace row, bit for bit -- the device's
 * mlp_features on batch.cgm (CGM[0]), rows 1 .. of mlp.cgm_hist, mlp.ins_hist, mlp.prev_meal, batch.t and mlp.start_minute,
 * the inputs of t1d_mlp_action, with the device's sinpi / cospi for the time-of-day pair.  After a collect call these are
 * the features of the state after its last step (for an env that finished there and was restarted: of its new episode's first
 * state), which the call recorded nowhere: what a critic evaluated by t1d_mlp_grad needs for the bootstrap value at the cut
 * (t1d_gae_batch.last_value).  It changes nothing: no state is written and no step is taken; the weights are not read.
 * fp64 and fp32, any integrator, any state layout.  T1D_E_INVALID: a NULL feat, and whatever t1d_mlp_action rejects. */
int t1d_mlp_features(t1d_ctx* ctx, const t1d_batch* b, const t1d_mlp* mlp, void* feat, void* hip_stream);

/* t1d_rollout_mlp, t1d_collect_mlp and t1d_rollout_mlp_dopri5 with the meal bolus of t1d_meal_bolus in every step, in one
 * launch as their siblings: everything else -- arguments, state, traces, draws, restarts, the cut that changes no result -- is
 * the sibling's, and the result is that of a loop of t1d_mlp_action, t1d_mlp_bolus, t1d_step (t1d_step_dopri5) with that basal
 * and bolus, the shift of the windows and prev_meal = batch.meal, bit for bit.  T1D_E_INVALID before anything is launched,
 * nothing changed: a NULL meal_bolus, cr or cf, and whatever the sibling rejects, with its texts under the call's own name.
 * The exact mode's collector has no such form: t1d_collect_mlp_dopri5 always runs with bolus = 0. */
int t1d_rollout_mlp_bolus(t1d_ctx* ctx, const t1d_batch* batch, const t1d_mlp* mlp, const t1d_meal_bolus* meal_bolus, int n_steps,
                          int minutes, int n_sub, void* hip_stream);
int t1d_collect_mlp_bolus(t1d_ctx* ctx, const t1d_batch* batch, const t1d_mlp* mlp, const t1d_collect* collect,
                          const t1d_meal_bolus* meal_bolus, int n_steps, int minutes, int n_sub, void* hip_stream);
int t1d_rollout_mlp_dopri5_bolus(t1d_ctx* ctx, const t1d_batch* b, const t1d_mlp* mlp, const t1d_meal_bolus* meal_bolus,
                                 double* h_carry, int32_t* nfev, int n_steps, int minutes, void* hip_stream);

/* The rule of t1d_meal_bolus alone, one lane per env, beside t1d_mlp_action: bolus[i] (device [n], the batch's dtype) = the
 * bolus, before the pump, that the next step of a *_bolus call would ask for env i -- from batch.cgm (CGM[0]) and
 * mlp.prev_meal, with the kernels' own function, so the word is theirs.  It changes nothing (bolus_trace is not used).
 * T1D_E_INVALID: a NULL meal_bolus, cr, cf or bolus, and whatever t1d_mlp_action rejects. */
int t1d_mlp_bolus(t1d_ctx* ctx, const t1d_batch* b, const t1d_mlp* mlp, const t1d_meal_bolus* meal_bolus, void* bolus, void* hip_stream);

/* The *_bolus calls above under the patient-relative output of t1d_env_output, in one launch each: arguments, state, traces,
 * draws, restarts and cuts are the sibling's, and the result is that of a loop of t1d_mlp_action_rel, t1d_mlp_bolus (with a
 * meal_bolus), t1d_step (t1d_step_dopri5), the shift of the windows and prev_meal = batch.meal, bit for bit.  meal_bolus may be
 * NULL: no bolus, the result of t1d_rollout_mlp / t1d_collect_mlp / t1d_rollout_mlp_dopri5 with the per-env pair.
 * T1D_E_INVALID before anything is launched, nothing changed: a NULL env_output, scale or bias; a meal_bolus without cr or cf;
 * and whatever the sibling rejects.  The exact mode's collector has no such form. */
int t1d_rollout_mlp_rel(t1d_ctx* ctx, const t1d_batch* batch, const t1d_mlp* mlp, const t1d_env_output* env_output,
                        const t1d_meal_bolus* meal_bolus, int n_steps, int minutes, int n_sub, void* hip_stream);
int t1d_collect_mlp_rel(t1d_ctx* ctx, const t1d_batch* batch, const t1d_mlp* mlp, const t1d_collect* collect,
                        const t1d_env_output* env_output, const t1d_meal_bolus* meal_bolus, int n_steps, int minutes, int n_sub,
                        void* hip_stream);
int t1d_rollout_mlp_dopri5_rel(t1d_ctx* ctx, const t1d_batch* b, const t1d_mlp* mlp, const t1d_env_output* env_output,
                               const t1d_meal_bolus* meal_bolus, double* h_carry, int32_t* nfev, int n_steps, int minutes,
                               void* hip_stream);

/* t1d_collect_mlp, t1d_collect_mlp_bolus and t1d_collect_mlp_rel with a time limit, in one launch as they are: the matching
 * existing call is t1d_collect_mlp_rel with an env_output, else t1d_collect_mlp_bolus with a meal_bolus, else t1d_collect_mlp,
 * and everything the limit does not touch -- arguments, state, traces, draws -- is that call's.
 * When a step is cut: after a step closes, done is formed as ever; cut = !done && t >= max_minutes, t the env's clock after the
 *   step (minutes since its reset).  Termination wins over truncation.
 * What is recorded for a cut step: done_trace holds 0, cut_trace holds 1 and batch.done stays 0.  cut_feat[j][i] holds the F =
 *   2 H + 3 features of the state after that step, formed by the collectors' own device function from the shifted windows,
 *   prev_meal = the step's meal and the clock start_minute + t: what t1d_mlp_features would return at that moment, bit for
 *   bit -- the state a critic bootstraps from (t1d_gae_cut.cut_value).  cut_feat is written for cut envs only.
 * What happens to a cut env: what happens to a finished one, which is t1d_restart_done with its mask byte set -- the episode
 *   accumulators move to last_*, terminal_cgm is written, the env gets a new start hour, a new meal column, a reset and
 *   episode + 1 -- and its policy state becomes that of a fresh reset.
 * Equivalence: after the call everything is what n_steps x (the matching one-step call; cut = !done && t >= max_minutes;
 *   t1d_mlp_features for the cut envs; t1d_restart_done(mask = done | cut); the reset of the policy state of the masked envs)
 *   leave, bit for bit, wherever the call is cut into launches.  With a max_minutes no env reaches the result is the matching
 *   existing call's, bit for bit.
 * T1D_E_INVALID before anything is launched, nothing changed: whatever the matching existing call rejects; a NULL limit,
 *   max_minutes < 1 or reserved != 0; on_done != T1D_COLLECT_RESTART (a cut restarts); n_steps * minutes > max_minutes -- so an
 *   env is cut at most once per call and one cut_feat column per env is enough.
 * The other collectors have the same limit: the five calls below.  What has none is the exact MLP collector under a meal bolus
 *   or a relative output: there is no t1d_collect_mlp_dopri5_bolus or _rel to put a limit on, and t1d_collect_mlp_dopri5_limit
 *   takes neither struct. */
int t1d_collect_mlp_limit(t1d_ctx* ctx, const t1d_batch* batch, const t1d_mlp* mlp, const t1d_collect* collect,
                          const t1d_env_output* env_output /* NULL = t1d_mlp's out_scale / out_bias */,
                          const t1d_meal_bolus* meal_bolus /* NULL = no bolus */,
                          const t1d_time_limit* limit, int n_steps, int minutes, int n_sub, void* hip_stream);

/* t1d_collect_pid, t1d_collect_bb, t1d_collect_mlp_dopri5, t1d_collect_pid_dopri5 and t1d_collect_bb_dopri5 with the time limit
 * of t1d_collect_mlp_limit, in one launch as they are: the matching existing call is the one without _limit in its name, and
 * everything the limit does not touch -- arguments, state, traces, draws, h_carry and nfev -- is that call's.
 * When a step is cut: after a step closes, done is formed as ever; cut = !done && t >= max_minutes, t the env's clock after the
 *   step (minutes since its reset).  Termination wins over truncation.
 * What is recorded for a cut step: done_trace holds 0, cut_trace holds 1 and batch.done stays 0.  cut_feat[j][i] holds the F =
 *   2 H + 3 features of the state after that step (H = feat.history for the controllers), formed by the collectors' own device
 *   function from the shifted windows, prev_meal = the step's meal and the clock start_minute + t: what t1d_mlp_features would
 *   return at that moment, bit for bit.  cut_feat is written for cut envs only.  Every trace row, cut_trace's too, is the row of
 *   the call's other traces: the controller's trace_row in the four controller calls, mlp.trace_row in the MLP call.
 * What happens to a cut env: what happens to a finished one, which is t1d_restart_done with its mask byte set -- the episode
 *   accumulators move to last_*, terminal_cgm is written, the env gets a new start hour, a new meal column, a reset and
 *   episode + 1 -- then the reset of the feature windows (every cgm_hist row the new first observation, ins_hist and prev_meal 0)
 *   and of the controller state (pid.integ = pid.prev = 0; bb.prev_meal = 0), and in the exact mode h_carry = 0: the first
 *   minute of the new episode probes the step size.
 * Equivalence: after the call everything is what n_steps x (t1d_mlp_features for the trace row; the matching one-step call; for
 *   the controllers the shift of the windows; cut = !done && t >= max_minutes; t1d_mlp_features for the cut envs;
 *   t1d_restart_done(mask = done | cut); the reset of windows, prev_meal and controller state of the masked envs) leave, bit
 *   for bit (in the exact mode: for envs whose solver does not give up), wherever the call is cut into launches -- each launch
 *   takes the same t1d_time_limit.  With a max_minutes no env reaches the result is the matching existing call's, bit for bit.
 * T1D_E_INVALID before anything is launched, nothing changed: whatever the matching existing call rejects, under this call's
 *   name; a NULL limit, max_minutes < 1 or reserved != 0; on_done != T1D_COLLECT_RESTART (a cut restarts); n_steps * minutes >
 *   max_minutes -- so an env is cut at most once per call and one cut_feat column per env is enough. */
int t1d_collect_pid_limit(t1d_ctx* ctx, const t1d_batch* batch, const t1d_pid* pid, const t1d_mlp* feat, const t1d_collect* collect,
                          const t1d_time_limit* limit, int n_steps, int minutes, int n_sub, void* hip_stream);
int t1d_collect_bb_limit(t1d_ctx* ctx, const t1d_batch* batch, const t1d_bb* bb, const t1d_mlp* feat, const t1d_collect* collect,
                         const t1d_time_limit* limit, int n_steps, int minutes, int n_sub, void* hip_stream);
int t1d_collect_mlp_dopri5_limit(t1d_ctx* ctx, const t1d_batch* b, const t1d_mlp* mlp, const t1d_collect* collect,
                                 const t1d_time_limit* limit, double* h_carry, int32_t* nfev, int n_steps, int minutes,
                                 void* hip_stream);
int t1d_collect_pid_dopri5_limit(t1d_ctx* ctx, const t1d_batch* b, const t1d_pid* pid, const t1d_mlp* feat,
                                 const t1d_collect* collect, const t1d_time_limit* limit, double* h_carry, int32_t* nfev,
                                 int n_steps, int minutes, void* hip_stream);
int t1d_collect_bb_dopri5_limit(t1d_ctx* ctx, const t1d_batch* b, const t1d_bb* bb, const t1d_mlp* feat,
                                const t1d_collect* collect, const t1d_time_limit* limit, double* h_carry, int32_t* nfev,
                                int n_steps, int minutes, void* hip_stream);

/* t1d_mlp_action under t1d_env_output: action[i] = the basal, before the pump, that the next step of a *_rel call would ask for
 * env i, by the kernels' own function.  It takes no meal_bolus: t1d_mlp_bolus is the bolus half of a step loop, with or without
 * a relative output.  T1D_E_INVALID: a NULL env_output, scale or bias, and whatever t1d_mlp_action rejects. */
int t1d_mlp_action_rel(t1d_ctx* ctx, const t1d_batch* b, const t1d_mlp* mlp, const t1d_env_output* env_output, void* action,
                       void* hip_stream);

/* The network of t1d_mlp on recorded features, and the gradient of a scalar loss with respect to its weights: the other half of
 * a policy-gradient iteration after t1d_collect_mlp / t1d_collect_mlp_dopri5.  No ctx; nothing is allocated, the call only
 * enqueues work on the stream.  fp64 and fp32.  Of t1d_mlp only history, n_layers, width, hidden_act, n_policies,
 * envs_per_policy, n_params and params are used; the state arrays, the feature scales, the traces and the output function are
 * ignored and may be NULL or 0 (noise and output function come after y and stay the host's business, like log_prob).
 *   y      y[s][i] = the last layer's output for the features feat[s][.][i] under the weights of policy i / envs_per_policy,
 *          computed by the device code of the roll-outs and collectors (bias first, then one fma per input, ascending, the
 *          same tanh): with sigma = NULL, out_act = T1D_MLP_IDENTITY, out_scale = 1 and out_bias = 0, y[s] equals
 *          action_trace[s] of the collect call that produced feat[s], bit for bit.  In general it is the word that call
 *          added sigma * eps to.
 *   grad   the vector-Jacobian product above, by back-propagation through the recomputed activations a: the derivative of
 *          tanh is 1 - a^2, that of relu is (a > 0 ? 1 : 0).  A NaN row (row 0 of a trace buffer) is the caller's to skip.
 *          Deterministic and portable: no floating-point atomics, and the summation order depends only on (n,
 *          envs_per_policy, n_rows, dtype, widths) -- not on the CU count, the grid, a context option or timing; two calls
 *          give identical bits.  The order: a tile is the 64 envs of one 64-env chunk of a policy in one row; the tiles of a
 *          policy are numbered u = s * C + chunk, C = envs_per_policy / 64.  With T = max(1, ceil(n_policies * C * n_rows /
 *          2048)), partial k of a policy covers tiles k T .. min((k + 1) T, C * n_rows) - 1 in ascending order; within a tile
 *          parameter q adds coef-weighted terms of the samples (q + m) mod 64, m = 0 .. 63, each with one fma onto the
 *          running partial, which starts at 0.  grad[p][q] = ((0 + partial 0) + partial 1) + ... in ascending k.
 *   workspace  t1d_mlp_grad_workspace(mlp, dtype, n, n_rows) bytes (host only, mlp.params may be NULL; < 0 = invalid
 *          arguments): n_policies * ceil(C * n_rows / T) * n_params words.  Nothing beyond them is written.
 * T1D_E_INVALID before anything is launched and before the device is touched: whatever t1d_rollout_mlp rejects of the fields
 * named above; n != n_policies * envs_per_policy or envs_per_policy % 64 != 0; n_rows < 1; a NULL feat; y and grad both NULL;
 * grad without coef; grad with a NULL or too small workspace. */
int64_t t1d_mlp_grad_workspace(const t1d_mlp* mlp, int dtype, int64_t n, int64_t n_rows);
int t1d_mlp_grad(int hip_device, int dtype, int64_t n, const t1d_mlp* mlp, const t1d_mlp_batch* io, void* hip_stream);

/* t1d_mlp_grad with the loss inside the launch: the network on recorded features once, the loss of every sample from y in a
 * register, its derivative as coef, the weight gradient and the per-policy sums a trainer logs -- one forward pass where a
 * y-only call, a dozen elementwise kernels and a gradient call that evaluates the network again stood.  No ctx; nothing is
 * allocated, the call only enqueues work on the stream.  fp64 and fp32; t1d_mlp is read as by t1d_mlp_grad.
 * Arithmetic, part of the contract so that a host can restate it.  T is the call's type, p = i / envs_per_policy the env's
 * policy, c = (T) clip and k = (T) scale; every operation below is one operation in T unless it says double, products and
 * quotients are taken left to right; the compiler may contract a product and a sum into one fma where none is written.
 *   T1D_LOSS_PPO_CLIP, so = sigma_old[p], sg = sigma[p]:
 *     z      = fma(so, eps, y_old)                          the action the collector took, by its own expression
 *     e_old  = (z - y_old) / so
 *     e_new  = (z - y) / sg
 *     logr   = 0.5 * ((e_old - e_new) * (e_old + e_new)) + (log(so) - log(sg))
 *     r      = exp(logr)
 *     active = adv >= 0 ? r <= 1 + c : r >= 1 - c
 *     loss_i = -min(r * adv, min(max(r, 1 - c), 1 + c) * adv)
 *     g      = active ? -(r * adv) : 0
 *     coef   = k * g * e_new / sg
 *     dsig_i = g * (e_new * e_new - 1) / sg                 d loss_i / d sigma[p]
 *     stats[p] = (sum loss_i, number of samples not active, sum of expm1(logr) - logr formed in double from (double) logr,
 *                 sum dsig_i)
 *   logr is a product of difference and sum so that it is exactly 0 where y == y_old and sg == so bit for bit: under
 *   unchanged weights r == 1 for every sample, stats[p] = (-sum adv, 0, 0.0, .) and coef = -k * adv * e_new / sg.
 *   T1D_LOSS_VALUE_MSE:
 *     d      = y - target
 *     loss_i = 0.5 * d * d
 *     coef   = k * d
 *     stats[p] = (sum loss_i, 0, 0, 0)
 *   A NaN row (row 0 of a trace buffer) is the caller's to skip.  sigma > 0 is the caller's responsibility: it is device data
 *   and is not read on the host.
 * y is t1d_mlp_grad's y and grad is t1d_mlp_grad's grad for coef = coef_out, both bit for bit (the same partition into tiles
 *   and partials, the same order).  Without grad the back-propagation is skipped; y, coef_out and stats are still written.
 * stats: every sample's four terms are converted to double and added in double, unscaled.  Deterministic and portable like
 *   grad, over the same partition: lane l of partial k adds the terms of env 64 chunk + l of its tiles in ascending tile
 *   order onto 0; the 64 lane sums are folded: for d = 32, 16, 8, 4, 2, 1: lane l += lane l + d (l < d), the result is lane
 *   0; stats[p][j] = ((0 + partial 0) + partial 1) + ... in ascending k.  A policy's row depends on its own envs alone.
 * workspace: t1d_mlp_loss_workspace(mlp, dtype, n, n_rows) bytes (host only, mlp.params may be NULL; < 0 = invalid arguments)
 *   = W rounded up to a multiple of 8, plus 32 bytes for every partial, n_policies * ceil(C * n_rows / T) of them, with W =
 *   t1d_mlp_grad_workspace() of the same arguments.  Nothing beyond them is written.  It needs the alignment of a double.
 * T1D_E_INVALID before anything is launched and before the device is touched: whatever t1d_mlp_grad rejects of mlp, dtype, n,
 * n_rows and feat; a NULL io; a kind that is neither of the two; a NULL eps, y_old, adv, sigma_old or sigma with
 * T1D_LOSS_PPO_CLIP, a NULL target with T1D_LOSS_VALUE_MSE; with T1D_LOSS_PPO_CLIP a clip outside (0, 1) or NaN; a scale that
 * is not finite; y, coef_out, grad and stats all NULL; grad or stats with a NULL or too small workspace. */
int64_t t1d_mlp_loss_workspace(const t1d_mlp* mlp, int dtype, int64_t n, int64_t n_rows);
int t1d_mlp_loss(int hip_device, int dtype, int64_t n, const t1d_mlp* mlp, const struct t1d_mlp_loss* io, void* hip_stream);

/* t1d_mlp_grad and t1d_mlp_loss on a minibatch: the same call on the tiles a list names, read and written in place -- the
 * gradient step of a PPO epoch on a random part of the batch without a gathered copy of it.  No ctx; nothing is allocated, the
 * call only enqueues work on the stream.  fp64 and fp32; mlp and io are read as by the plain call, and nothing is added to
 * either struct.
 * Same arrays: feat, eps, y_old, adv, target, coef, y and coef_out keep their full [n_rows][...][n] layout and addressing; only
 *   the listed tiles are visited.  Position j of policy p's row names tile u = tiles[p][j]: row u / C, envs p * envs_per_policy
 *   + 64 * (u % C) .. + 63.  y and coef_out are written at the listed tiles' own positions; every other word of them is left
 *   untouched.
 * Duplicates: the list may name a tile twice (sampling with replacement); the tile then counts twice in grad and stats, and its
 *   words of y and coef_out are written twice with the same values.
 * Skipped ids: an id < 0 or >= C * n_rows is skipped: nothing is read or written for it and it adds nothing to any sum.  The
 *   ids are device data that the host cannot check, so the bound check is made on the device and is part of the contract, not
 *   a debug aid; -1 serves as padding.  A list of skipped ids alone gives grad = 0 and stats = 0.
 * Order: t1d_mlp_grad's rule with list positions in place of tile numbers.  With T = max(1, ceil(n_policies * M / 2048)),
 *   partial k of a policy covers positions k T .. min((k + 1) T, M) - 1 in ascending order; inside a tile the order is that of
 *   the plain call; grad[p][q] and stats[p][j] = ((0 + partial 0) + partial 1) + ... in ascending k.  Deterministic and portable
 *   as the plain calls are: the order depends only on (n_policies, M, dtype, widths) and the list.
 * Two identities follow, both bit for bit:
 *   - with the identity list 0 .. C * n_rows - 1 for every policy, every output equals the plain call's;
 *   - for any list without skipped ids, grad, stats and the visited words of y / coef_out equal those of a plain call on the
 *     gathered batch: n' = 64 * n_policies, envs_per_policy' = 64, n_rows' = M, row j of policy p holding tile tiles[p][j] of
 *     every array (the same scale, sigma and weights).
 * scale stays the caller's, e.g. 1 / (64 * M * n_policies) for a mean over the listed samples.
 * workspace: t1d_mlp_grad_tiles_workspace(mlp, dtype, n, n_tiles) bytes = n_policies * ceil(M / T) * n_params words;
 *   t1d_mlp_loss_tiles_workspace(mlp, dtype, n, n_tiles) = that rounded up to a multiple of 8, plus 32 bytes for every partial,
 *   n_policies * ceil(M / T) of them (host only, mlp.params may be NULL; < 0 = invalid arguments, n_tiles < 1 among them).
 *   Neither depends on n_rows.  Nothing beyond them is written.
 * T1D_E_INVALID before anything is launched and before the device is touched: everything the plain call rejects; a NULL list,
 * a NULL tiles, n_tiles < 1; n_policies * n_tiles > 2^31 - 1; grad (or stats) with a workspace smaller than the
 * _tiles_workspace() of the call. */
int64_t t1d_mlp_grad_tiles_workspace(const t1d_mlp* mlp, int dtype, int64_t n, int64_t n_tiles);
int t1d_mlp_grad_tiles(int hip_device, int dtype, int64_t n, const t1d_mlp* mlp, const t1d_mlp_batch* io, const t1d_tile_list* list,
                       void* hip_stream);
int64_t t1d_mlp_loss_tiles_workspace(const t1d_mlp* mlp, int dtype, int64_t n, int64_t n_tiles);
int t1d_mlp_loss_tiles(int hip_device, int dtype, int64_t n, const t1d_mlp* mlp, const struct t1d_mlp_loss* io,
                       const t1d_tile_list* list, void* hip_stream);

/* Generalised advantage estimation over a collected batch: the scan from (reward, done, value) to advantages and value targets,
 * and the per-policy sums advantage normalisation needs -- what stands between t1d_collect_mlp / t1d_collect_mlp_dopri5 and the
 * loss t1d_mlp_grad differentiates.  No ctx; nothing is allocated, the call only enqueues work on the stream.  fp64 and fp32;
 * n is any positive number of envs (no multiple of 64 is asked for); policy p owns envs [p E, (p + 1) E), E = n / n_policies.
 * One lane per env, rows walked from the last to the first.
 * Arithmetic, part of the contract so that a host can restate it.  With T the call's type, g = (T) gamma and gl = (T) (gamma *
 * lambda), the product formed in double, for every env and s = K-1 down to 0:
 *     live   = done == NULL || done[s] == 0
 *     vn     = live ? (s == K-1 ? last_value : value[s+1]) : 0
 *     an     = live ? (s == K-1 ? 0 : adv[s+1]) : 0            (the running word, kept in a register: adv may be NULL)
 *     delta  = fma(g, vn, reward[s]) - value[s]
 *     adv[s] = fma(gl, an, delta)
 *     ret[s] = adv[s] + value[s]
 *   vn and an are SELECTED, never multiplied by zero: a NaN or a stale word in value[s+1] or last_value behind a done does
 *   not reach row s.  That matters with T1D_COLLECT_RESTART: row s + 1 of a collector's traces belongs to the NEXT episode of
 *   an env that finished in row s, and so does the critic's value of it.  A NULL value or last_value reads as 0.
 *   done is a true termination (BG left [70, 350], batch.done); the cut at the end of the batch is what last_value is for.
 *   Episodes cut by a time limit (t1d_collect_mlp_limit) have a second mask and take t1d_gae_limit:
 *     ended = done && done[s] != 0
 *     trunc = !ended && truncated[s] != 0
 *     vn    = ended ? 0 : trunc ? cut_value[i] : (s == K-1 ? last_value : value[s+1])
 *     an    = (ended || trunc) ? 0 : (s == K-1 ? 0 : adv[s+1])
 *   and the rest unchanged.  Both are selected, never multiplied: a NaN in value[s+1] or adv[s+1] behind a cut does not reach
 *   row s, and neither does a NaN in the cut_value of an env that was not cut.  A NULL cut_value reads as 0.
 * moments[p] = (sum of adv, sum of adv^2) over the K E samples of policy p, in double whatever the dtype.  Deterministic and
 *   portable: no floating-point atomics, and the summation order depends only on (n, n_policies, n_rows, dtype) -- not on the
 *   CU count, the grid or timing; two calls give identical bits, and a policy's pair depends on its own envs' words alone.
 *   The order is stated relative to the policy, so a policy's pair does not depend on where its envs sit in the batch (the
 *   policies' env blocks permuted as whole blocks give the permuted moments).  Every env forms a = ((0 + x[K-1]) + x[K-2]) +
 *   .. + x[0] and b = fma(x[0], x[0], .. fma(x[K-1], x[K-1], 0)) with x[s] = (double) adv[s].  A tile is the envs 64 c .. min(64
 *   c + 63, E - 1) of a policy, counted from the policy's first env; partial c adds the a (the b) of the tile's envs in
 *   ascending order onto 0.  moments[p]: lane l = 0 .. 63 adds the policy's partials l, l + 64, .. in ascending order onto 0;
 *   then the lane sums are folded: for d = 32, 16, 8, 4, 2, 1: lane l += lane l + d (l < d); the result is lane 0.
 * workspace: t1d_gae_workspace(dtype, n, io) bytes (host only; < 0 = invalid arguments; of io only n_rows, n_policies, gamma and
 *   lambda are looked at): 16 bytes for every partial, n_policies * ceil(E / 64) of them.  It does not grow with n_rows.
 *   Nothing beyond them is written.
 * T1D_E_INVALID before anything is launched and before the device is touched: a NULL io or reward; adv, ret and moments all
 * NULL; n_rows < 1 or n < 1; n_policies < 1 or n % n_policies != 0; gamma or lambda outside [0, 1] or NaN; a bad dtype; moments
 * with a NULL or too small workspace; and beyond the sizes the kernels index: n > 2^31, n_rows * n > 2^40, n_policies > 2^31 - 1.
 * The workspace needs the alignment of a double, no more. */
int64_t t1d_gae_workspace(int dtype, int64_t n, const t1d_gae_batch* io);
int t1d_gae(int hip_device, int dtype, int64_t n, const t1d_gae_batch* io, void* hip_stream);
/* t1d_gae with the truncation mask (the recurrence above): workspace, moments order and determinism are t1d_gae's, and with an
 * all-zero truncated the outputs are t1d_gae's bits.  T1D_E_INVALID, before the device is touched: a NULL cut or truncated, and
 * whatever t1d_gae rejects. */
int t1d_gae_limit(int hip_device, int dtype, int64_t n, const t1d_gae_batch* io, const t1d_gae_cut* cut, void* hip_stream);

/* RandomScenario.create_scenario (simulation/scenario_gen.py:33-60) for n envs on the device: fills per-env
 * meal tables meal_time int32 [6 (days + 1)][n] (minutes since the episode start, ascending, unused =
 * INT32_MAX) and meal_amt [6 (days + 1)][n] (grams, dtype T1D_F64/F32) covering `days` days of an episode
 * that starts at start_minute_of_day[i] (device int32 [n]) or, if that is NULL, at start_scalar for every
 * env.  Statistical counterpart of the reference's numpy stream (Philox, subsequence = env_offset + i);
 * exact replays of a reference scenario go through explicit tables instead.  No ctx needed.
 * The stream, draw for draw (restated on the host in oracle/t1d_streams.py): Philox4x32-10 as rocRAND runs it -- counter =
 * (block lo, block hi, subsequence lo, subsequence hi), key = (key lo, key hi), the block of word offset o is o / 4 -- with
 *   key = seed ^ 0x5ce9a7105ce9a710: a key domain of the scenario's own, so that a batch and its meal tables may share a seed;
 *   subsequence g = env_offset + i, all 64 bits of it;
 *   candidate k = 0 .. 5 (breakfast, snack, lunch, snack, dinner, snack) of calendar day d = 0 .. days (day 0 is the day the
 *   episode starts in) owns the two blocks at word offset 8 (6 d + k): the first as rocrand_uniform_double2 -> (u.x, u.y) in
 *   (0, 1], the second as rocrand_normal_double2 -> (g.x, g.y); g.y is not used.
 * With the windows (p, lb, ub, mu [hours], sd [minutes], grams mean, grams sd) = (.95, 5, 9, 7, 60, 45, 10), (.3, 9, 10, 9.5, 30,
 * 10, 5), (.95, 10, 14, 12, 60, 70, 10), (.3, 14, 16, 15, 30, 10, 5), (.95, 16, 20, 18, 60, 80, 10), (.3, 20, 23, 21.5, 30, 10, 5)
 * and Phi the standard normal CDF:
 *   present = u.x <= p                                                          (rand() < p, :48)
 *   tod     = rint(60 mu + sd Phi^-1(Phi_a + u.y (Phi_b - Phi_a))) minutes, Phi_a = Phi((60 lb - 60 mu) / sd), Phi_b likewise of
 *             ub; rint rounds to nearest, ties to even (np.round, :49-54); then clamped to [60 lb, 60 ub] (a guard)
 *   grams   = max(rint(mean + sd_grams g.x), 0), the zero a +0                   (:56-57)
 *   minute  = 1440 d + tod - start
 * A candidate becomes the next row of the env's column if it is present, 0 <= minute < 1440 days, and minute differs from the
 * minute of the row written before it: windows meet at their bounds, and the reference's scenario keeps one meal per minute,
 * the earlier one here.  Rows are in candidate order, which is ascending time. */
int t1d_random_meals(int hip_device, uint64_t seed, int64_t env_offset, int64_t n, int dtype, int days,
                     const int32_t* start_minute_of_day, int start_scalar, int32_t* meal_time, void* meal_amt,
                     void* stream);

/* The numbers of analysis/report.py per env from a BG history [n_rows][n] kept on the device (see t1d_outcome). */
int t1d_outcome_stats(int hip_device, int dtype, int64_t n, int64_t n_rows, const void* bg_trace,
                      const t1d_outcome* out, void* stream);

/* The standard normals the kernels draw in Philox mode for episode `episode`: out[r][i] = draw
 * (draw0 + r) of env (env_offset + i), doubles [n_draws][n] on the device.  Draw 0 is the AR(1)
 * initial value, draws 1.. are the block normals in consumption order (so the array can be fed
 * back as `normals`); draws -3..-1 are the three random_init_bg normals (x[3], x[4], x[12]).
 * Lets a test replay a Philox run through the oracle.
 * philox_pair(seed, g, episode, m) = rocrand_normal_double2 of the Philox4x32-10 block (episode << 24) + m (word offset four
 * times that; counter and key as under t1d_random_meals) of subsequence g = env_offset + i under key = seed: two Box-Muller
 * normals (.x, .y).  An episode has 2^24 pairs of its own; episode is the value of batch.episode during it (1 after the
 * first t1d_reset).  Draw 0 is pair 0 .x; draws -3, -2, -1 are pair 1 .x, pair 1 .y, pair 2 .x; draw 1 + 10 b + j (j = 0 .. 9,
 * noise block b) is pair 3 + 5 b + j / 2, .x for even j and .y for odd j. */
int t1d_philox_normals(t1d_ctx* ctx, uint64_t seed, int64_t env_offset, int64_t n, uint32_t episode,
                       int32_t draw0, int32_t n_draws, double* out_device, void* hip_stream);

/* T1DPatient.model (t1dpatient.py:119-208) for n independent points, one lane each: dxdt[k][i] = d x_k / dt at state
 * x[13][n] for patient row pid[i] of the context's table, with cho[i] grams eaten in the minute (:121), insulin[i]
 * U/min (:122; the pump is not applied) and the bookkeeping values last_qsto[i] (mg) / last_food[i] (g) behind Dbar
 * (:130).  math = 0: ocml tanh and IEEE divisions as the reference writes them; 1: the arithmetic the step kernels use.
 * All device arrays of `dtype`; pid int32 [n]. */
int t1d_model_rhs(t1d_ctx* ctx, int dtype, int64_t n, int math, const void* x, const int32_t* pid, const void* cho,
                  const void* insulin, const void* last_qsto, const void* last_food, void* dxdt, void* hip_stream);

/* Start the next episode of the envs whose mask byte is non-zero (mask == NULL: batch.done), where they are: one launch, one
 * lane per env, meant to follow every t1d_step of a gym-style loop -- no host round trip, nothing allocated, the other envs
 * untouched (one byte read each; with the accumulators below 33 bytes more).  Everything the new episode draws is keyed by
 * the env's OWN episode index k = its batch.episode counter before the call (0 for an env never reset) and its global id
 * g = env_offset + i, so an env's k-th episode is one thing however it was reached and whatever the rest of the batch did
 * (shards of a multi-GPU job = slices of one batch, through every restart).  A restarted env
 *   1. gets cgm[i] stored to terminal_cgm[i]; ep_return / ep_length move to last_return / last_length and restart at 0
 *      (every env, restarted or not, first adds this step's reward and 1 to them);
 *   2. draws its start hour: h = (z >> 11) mod 24 with z = splitmix64 finaliser of g * 0x9E3779B97F4A7C15 +
 *      (seed * 1000003 + k), all mod 2^64; start_minute[i] = 60 h;
 *   3. writes its column of the meal tables with what t1d_random_meals(seed * 7919 + k mod 2^64, env_offset = g, n = 1, days,
 *      start 60 h) writes;
 *   4. is reset as by t1d_reset (patient state, random_init_bg draws, noise state, CGM samples #0 and #1, prev_risk, cgm0,
 *      cursor 0, next_meal = its new row 0, episode = k + 1 -- the `ep` of the Philox draws), and h_carry[i] = 0.
 * With k = 0 and seed s this is the first episode BatchedGymT1DSimEnv(seed = s).reset() builds.  Batches with host normals or
 * x0_override have no per-episode source on the device: T1D_E_INVALID, as are tables that are not the batch's own, n_meals
 * != 6 (days + 1) and a NULL batch.episode.  fp64 and fp32, any state layout.  Option "restart_compact": 1 (default) = a workgroup
 * collects the finished envs of 4 096 in LDS and restarts them with full waves; 0 = every lane restarts its own env, in waves
 * with one or two live lanes (same results; gym step at 1 Mi fp64 envs with 1.5 % of the envs finishing per step: 0.35 ms
 * against 1.05 ms, 0.21 ms without any restart: profiles/autoreset). */
int t1d_restart_done(t1d_ctx* ctx, const t1d_batch* b, const uint8_t* mask, const t1d_restart* r, void* hip_stream);

/* Wait for the stream and return the accumulated status bits through *status (then clear them). */
int t1d_sync(t1d_ctx* ctx, void* hip_stream, int32_t* status);

#ifdef __cplusplus
}
#endif
#endif /* T1D_H */
