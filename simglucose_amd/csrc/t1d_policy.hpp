// t1d_policy.hpp -- closed-loop roll-outs under a small feed-forward policy evaluated inside the kernel (gfx950 only):
// t1d_rollout_mlp of include/t1d.h.  Included by t1d_abi.hip after t1d_kernels.hpp, whose step_body / load_env /
// store_env / write_outputs it calls as they are.
//
//   mlp_rollout_kernel   n_steps x (features -> dense layers -> basal, then step_body) in ONE launch, the env state in
//                        registers as in rollout_pid_kernel.  What does not fit beside the integrator's registers lives
//                        in LDS, one column of 64 lanes per word (word k of lane l at k * 64 + l: every access of a wave
//                        covers 64 consecutive words, so no two lanes of a group meet on a bank):
//                          rows 0 .. H-1     the CGM window as a ring: CGM[-k] sits in row (head + k) mod H
//                          rows H .. 2H-1    the insulin window, same ring: INS[-1-k] in row H + (head + k) mod H
//                          rows 2H ..        the layer input: the F = 2H + 3 features, then each hidden layer's output
//                        `head` is wave-uniform (every lane takes a step per iteration), so a step overwrites the oldest row
//                        instead of moving 2H words; the arrays in memory are in window order on entry and on exit.
//                        A layer's outputs are accumulated four at a time in registers and written back over its inputs
//                        once the layer is complete.
//   weights              one set per wave (envs_per_policy is a multiple of 64): read through the scalar data cache from
//                        the constant address space (s_load_dword*), straight into the FMA's scalar operand -- no LDS,
//                        no vector register; nothing is ever stored through the scalar unit.
//   block size           64 .. 256 threads, chosen per launch (t1d_rollout_mlp): the most waves whose columns fit in a
//                        workgroup's LDS beside the integrator's tables.  The launch bound is one wave per SIMD: a roll-out
//                        step with the noise-block refill inline needs more than the 256 registers two waves would leave
//                        each (rollout_pid_kernel, bound to two, keeps ~300 bytes per lane in scratch); with the whole
//                        file seven of the eight instances report no scratch (profiles/policy).
#pragma once
#include "t1d_kernels.hpp"

namespace t1d {

constexpr int kMlpMaxHistory = 12, kMlpMaxLayers = 4, kMlpMaxWidth = 32;
#ifndef T1D_POLICY_THREADS
#define T1D_POLICY_THREADS 256            // launch bound: 4 waves per workgroup = 1 per SIMD, the whole register file each
#endif

template <typename T> struct MlpArgs {
    const T* params;                      // [n_policies][n_params]
    T* cgm_hist; T* ins_hist; T* prev_meal; const int32_t* start_minute;
    T cgm_mean, cgm_scale, ins_scale, cho_scale, out_scale, out_bias;
    T* sum_risk; T* min_bg; T* max_bg; int32_t* n_low; int32_t* n_high;
    T* bg_trace; T* cgm_trace; T* cho_trace; T* ins_trace; T* act_trace; int64_t trace_row;
    unsigned envs_per_policy, widths;     // widths: width[l] in bits 8 l .. 8 l + 7
    int n_params, history, n_layers, hidden_act, out_act, n_steps;
    int lds_off;                          // bytes of dynamic LDS ahead of the columns (the propagator table)
    int cols;                             // rows of a wave's column block: 2 H + the widest layer input
};

// ---- activations on the fast exp of t1d_device.hpp ----------------------------------------------------------------
// tanh(v) = sign(v) (1 - E) / (1 + E) with E = exp(-2 |v|) <= 1: no overflow, absolute error ~2 ulp of 1 (the relative
// error grows towards v = 0, where 1 - E cancels: |error| stays below 3e-16 in fp64).
template <typename T>
__device__ __forceinline__ T mlp_tanh(T v)
{
    const T lim = sizeof(T) == 8 ? T(20) : T(10);            // tanh(20) = 1 - 3e-18, tanh(10) = 1 - 8e-9: both round to 1
    const T a = t_min(v < T(0) ? -v : v, lim);
    const T E = exp_core(T(-2) * a);
    const T r = fdiv(T(1) - E, T(1) + E);
    return v != v ? v : (v < T(0) ? -r : r);                 // fmin would turn a NaN into the limit: it is handed on instead
}
// logistic(v) = 1 / (1 + exp(-v)), the argument clamped to where the result has already reached 0 or 1
template <typename T>
__device__ __forceinline__ T mlp_logistic(T v)
{
    const T lim = sizeof(T) == 8 ? T(700) : T(80);
    const T E = exp_core(t_max(t_min(-v, lim), -lim));
    return v != v ? v : fdiv(T(1), T(1) + E);                // a NaN stays a NaN (pump_quantise hands it on: the step raises T1D_ST_NONFINITE)
}

// sin and cos of 2 pi m / 1440 for the minute of day m in [0, 1440): sinpi / cospi of m / 720 -- their argument
// reduction is exact and has no large-argument path to pay registers for
__device__ __forceinline__ void mlp_time_of_day(int m, double& s, double& c) { const double x = (double)m / 720.0; s = sinpi(x); c = cospi(x); }
__device__ __forceinline__ void mlp_time_of_day(int m, float& s, float& c) { const float x = (float)m / 720.0f; s = sinpif(x); c = cospif(x); }

// The dense layers on the lane's column.  buf: rows of the layer input (row j at buf[j * 64]); w: this wave's weight set,
// layer after layer, each as row-major W[out][in] followed by b[out].  Accumulation order (include/t1d.h): acc = b[o],
// then acc = fma(W[o][j], in[j], acc) for j ascending.  -> the last layer's single output, before the output function.
// KEEP (t1d_policy_grad.hpp): a hidden layer's outputs go behind its inputs instead of over them, so that on return the
// column holds the features and then every hidden layer's activations, in order; the arithmetic is the same.
template <typename T, bool KEEP = false>
__device__ __forceinline__ T mlp_layers(const MlpArgs<T>& c, const __attribute__((address_space(4))) T* w, T* buf, int in_w)
{
    T y = T(0);
#pragma unroll 1
    for (int l = 0; l < c.n_layers; ++l) {
        const int out_w = (int)((c.widths >> (8 * l)) & 0xffu);
        const __attribute__((address_space(4))) T* bias = w + out_w * in_w;
        T out[kMlpMaxWidth];
#pragma unroll
        for (int ob = 0; ob < kMlpMaxWidth; ob += 4) {
            if (ob < out_w) {                                            // wave-uniform
                // four outputs share every input word read from LDS; beyond the layer's width the last row is computed
                // again and dropped
                const int last = out_w - 1;
                const int o0 = ob, o1 = ob + 1 < last ? ob + 1 : last, o2 = ob + 2 < last ? ob + 2 : last, o3 = ob + 3 < last ? ob + 3 : last;
                const __attribute__((address_space(4))) T* r0 = w + o0 * in_w;
                const __attribute__((address_space(4))) T* r1 = w + o1 * in_w;
                const __attribute__((address_space(4))) T* r2 = w + o2 * in_w;
                const __attribute__((address_space(4))) T* r3 = w + o3 * in_w;
                T a0 = bias[o0], a1 = bias[o1], a2 = bias[o2], a3 = bias[o3];
#pragma unroll 1
                for (int j = 0; j < in_w; ++j) {
                    const T x = buf[j * 64];
                    a0 = fma((T)r0[j], x, a0); a1 = fma((T)r1[j], x, a1); a2 = fma((T)r2[j], x, a2); a3 = fma((T)r3[j], x, a3);
                }
                out[ob] = a0; out[ob + 1] = a1; out[ob + 2] = a2; out[ob + 3] = a3;
            }
        }
        if (l + 1 == c.n_layers) { y = out[0]; break; }
        // the layer is complete: its outputs replace its inputs, then the activation runs over them in place
        if constexpr (KEEP) buf += in_w * 64;
#pragma unroll
        for (int o = 0; o < kMlpMaxWidth; ++o)
            if (o < out_w) buf[o * 64] = out[o];
#pragma unroll 1
        for (int o = 0; o < out_w; ++o) {
            const T v = buf[o * 64];
            buf[o * 64] = c.hidden_act == 0 ? mlp_tanh(v) : (v < T(0) ? T(0) : v);      // relu; a NaN stays a NaN
        }
        w = bias + out_w;
        in_w = out_w;
    }
    return y;
}

// The F = 2 H + 3 features of a step, in the order of include/t1d.h, into buf (the rows behind the lane's two windows).
// col: the lane's column; head: the ring row of CGM[0] / INS[-1] (wave-uniform in mlp_rollout_kernel, per lane where the
// lanes of a wave are in different steps); clock: start_minute + t at the start of the step.
template <typename T>
__device__ __forceinline__ void mlp_features(const MlpArgs<T>& c, const T* col, T* buf, int head, T prev_meal, int clock)
{
    const int H = c.history;
    for (int k = 0, r = head; k < H; ++k) {
        buf[k * 64] = (col[r * 64] - c.cgm_mean) * c.cgm_scale;
        buf[(H + k) * 64] = col[(H + r) * 64] * c.ins_scale;
        r = r + 1 == H ? 0 : r + 1;
    }
    buf[2 * H * 64] = prev_meal * c.cho_scale;
    int m = clock % 1440;
    m = m < 0 ? m + 1440 : m;
    T sn, cs;
    mlp_time_of_day(m, sn, cs);
    buf[(2 * H + 1) * 64] = sn; buf[(2 * H + 2) * 64] = cs;
}

// the basal the policy asks for, from the last layer's output (plus the exploration term, where there is one)
template <typename T>
__device__ __forceinline__ T mlp_output(const MlpArgs<T>& c, T y)
{
    return fma(c.out_scale, c.out_act == 0 ? y : mlp_logistic(y), c.out_bias);
}

// features -> layers -> output function: the action of one step.  Every kernel that evaluates the policy calls this (or its
// three parts, where something goes in between), so that they all give the same word for the same windows, clock and weights.
template <typename T>
__device__ __forceinline__ T mlp_action(const MlpArgs<T>& c, const __attribute__((address_space(4))) T* w, const T* col, T* buf,
                                        int head, T prev_meal, int clock)
{
    mlp_features(c, col, buf, head, prev_meal, clock);
    return mlp_output(c, mlp_layers(c, w, buf, 2 * c.history + 3));
}

// the weight set of the wave of env i: a scalar base, whatever the compiler can prove about the lane index
template <typename T>
__device__ __forceinline__ const __attribute__((address_space(4))) T* mlp_wave_weights(const MlpArgs<T>& c, unsigned i)
{
    const unsigned wave0 = __builtin_amdgcn_readfirstlane(i & ~63u);
    return (const __attribute__((address_space(4))) T*)(c.params + (size_t)(wave0 / c.envs_per_policy) * (size_t)c.n_params);
}

// rollout_body (t1d_kernels.hpp) with the policy in place of the two hand-written controllers.  col: the lane's column.
template <int VARIANT, typename T, typename P, typename PR = NoProp>
__device__ __forceinline__ void mlp_rollout_body(const KArgs<T>& a, const MlpArgs<T>& c, P& p, unsigned i, uint32_t pid, Env<T>& e,
                                                 T* col, PR pr = PR())
{
    constexpr int MATH = VariantMath<VARIANT>::value;
    typedef const __attribute__((address_space(4))) T* WPtr;
    const int H = c.history;
    T* const buf = col + 2 * H * 64;
    const WPtr w = mlp_wave_weights(c, i);
    T obs = at(a.cgm, i);
    col[0] = obs;                                               // CGM[0] is the observation the step starts from
    for (int k = 1; k < H; ++k) col[k * 64] = at(rowv(c.cgm_hist, a.n, k), i);
    for (int k = 0; k < H; ++k) col[(H + k) * 64] = at(rowv(c.ins_hist, a.n, k), i);
    int head = 0;
    T prev_meal = at(c.prev_meal, i);
    const int start = c.start_minute ? (int)at(c.start_minute, i) : 0;
    T sum_risk = c.sum_risk ? at(c.sum_risk, i) : T(0);
    T min_bg = c.min_bg ? at(c.min_bg, i) : T(0), max_bg = c.max_bg ? at(c.max_bg, i) : T(0);
    int n_low = c.n_low ? at(c.n_low, i) : 0, n_high = c.n_high ? at(c.n_high, i) : 0;
    StepOut<T> o{obs, T(0), T(0), T(0)};
    T cgm_before = T(0);                        // CGM of the step before the last one, once two steps have run
#pragma unroll 1
    for (int s = 0; s < c.n_steps; ++s) {
        const T u = mlp_action(c, w, col, buf, head, prev_meal, start + e.t);
        o = step_body<MATH, T, P, true, PR, VariantInfo<VARIANT>::tiered>(a, p, i, e, u, T(0), true, pr);
        obs = o.cgm;
        prev_meal = o.meal;
        head = head == 0 ? H - 1 : head - 1;                    // the oldest row becomes the newest
        col[head * 64] = o.cgm; col[(H + head) * 64] = o.ins;
        if (c.bg_trace) c.bg_trace[(c.trace_row + s) * a.n + i] = o.bg;
        if (c.cgm_trace) c.cgm_trace[(c.trace_row + s) * a.n + i] = o.cgm;
        if (c.cho_trace) c.cho_trace[(c.trace_row + s) * a.n + i] = o.meal;
        if (c.ins_trace) c.ins_trace[(c.trace_row + s) * a.n + i] = o.ins;
        if (c.act_trace) c.act_trace[(c.trace_row + s) * a.n + i] = u;
        if (s + 1 < c.n_steps) cgm_before = o.cgm;  // CGM history advances every step
        if (c.sum_risk) { T l, h, r; risk_index1<MATH>(o.bg, l, h, r); sum_risk += r; }
        min_bg = o.bg < min_bg ? o.bg : min_bg;
        max_bg = o.bg > max_bg ? o.bg : max_bg;
        n_low += o.bg < T(70); n_high += o.bg > T(180);
    }
    // the last step's reward: against the step before it, or against what the state carried in (one step)
    T rp = e.prev_risk;
    if (c.n_steps > 1) { T l, h; risk_index1<MATH>(cgm_before, l, h, rp); }
    write_outputs<MATH>(a, i, e, o, rp);
    store_env(a, i, pid, e);
    for (int k = 0, r = head; k < H; ++k) {                     // the windows back in window order
        at(rowv(c.cgm_hist, a.n, k), i) = col[r * 64];
        at(rowv(c.ins_hist, a.n, k), i) = col[(H + r) * 64];
        r = r + 1 == H ? 0 : r + 1;
    }
    at(c.prev_meal, i) = prev_meal;
    if (c.sum_risk) at(c.sum_risk, i) = sum_risk;
    if (c.min_bg) at(c.min_bg, i) = min_bg;
    if (c.max_bg) at(c.max_bg, i) = max_bg;
    if (c.n_low) at(c.n_low, i) = n_low;
    if (c.n_high) at(c.n_high, i) = n_high;
}

// VARIANT as for rollout_pid_kernel.  blockDim.x is any multiple of 64 up to T1D_POLICY_THREADS; dynamic LDS: the
// propagator table (split variants), then cols * 64 words for each wave.
template <int VARIANT, typename T>
__global__ __launch_bounds__(T1D_POLICY_THREADS) void mlp_rollout_kernel(const KArgs<T> a, const MlpArgs<T> c)
{
    using VI = VariantInfo<VARIANT>;
    constexpr int kParRows = VI::split ? DP_COUNT : DP_RK4_COUNT;
    __shared__ T lds[VI::lds_pars ? kParRows * kMaxPatients : 1];
    if (VI::lds_pars) stage_pars(a, lds, kParRows);
    if (VI::split) stage_prop(a, (T*)t1d_dyn_lds);
    const unsigned i = blockIdx.x * blockDim.x + threadIdx.x;
    __builtin_assume(i < (1u << 28));          // host guarantees n <= 2^28: i * sizeof(T) fits a 32-bit voffset
    if ((int64_t)i >= a.n) return;
    T* const col = (T*)(t1d_dyn_lds + c.lds_off) + (threadIdx.x >> 6) * (c.cols * 64) + (threadIdx.x & 63u);
    const uint32_t meta = at(a.meta, i);
    const uint32_t pid = T1D_META_PID(meta);
    Env<T> e;
    load_env(a, i, meta, e);
    if constexpr (VARIANT == 4 || VARIANT == 6) {
        ParsReg<T> p;
        p.load(a.dpar, (int)pid);
        mlp_rollout_body<VARIANT>(a, c, p, i, pid, e, col, PropLds<T>{(const T*)t1d_dyn_lds, a.np_pad, (int)pid});
    } else if constexpr (VARIANT == 7) {
        ParsLds<T> p{lds, (int)pid};
        mlp_rollout_body<VARIANT>(a, c, p, i, pid, e, col, PropLds<T>{(const T*)t1d_dyn_lds, a.np_pad, (int)pid});
    } else if constexpr (VARIANT == 3) {
        ParsReg<T> p;
        p.load(a.dpar, (int)pid);
        mlp_rollout_body<VARIANT>(a, c, p, i, pid, e, col);
    } else {
        ParsLds<T> p{lds, (int)pid};
        mlp_rollout_body<VARIANT>(a, c, p, i, pid, e, col);
    }
}

// ---- t1d_collect_mlp: trajectories for a policy-gradient trainer --------------------------------------------------------
//   mlp_collect_kernel   mlp_rollout_kernel with what a trainer needs of every step: exploration noise on the network's
//                        output, the reward and done of every step, the features the network was given, and episodes that
//                        end (include/t1d.h).  The env state stays in registers, windows and activations in the LDS
//                        columns, the weights (and the policy's sigma) go through the scalar data cache, as above.
//   draw                 eps = philox_pair(explore_seed, global env id, the env's episode counter, the env's t).x: one
//                        Philox set-up per lane and step, none without sigma.  Keyed by what the env is and where it
//                        stands, so cuts, shards and neighbours do not show in it.
//   a finished env       on_done = 1: the lane writes its outputs and its state as the end of the launch would, then
//                        collect_restart -- restart_front / restart_env on the words in memory, what restart_kernel runs
//                        for it -- then loads the new episode and fills its window rows with the new first observation.
//                        A lane that did not finish writes nothing of its state between the steps.  collect_restart is
//                        written to be kept out of line, as noise_refill is (T1D_COLLECT_RESTART_INLINE=0: eighteen Philox
//                        set-ups, erfinv and the reset then cost code and registers on that path only), and like
//                        noise_refill it is inlined by default, on measurement: around a call the register allocator
//                        keeps part of the step's state in scratch in every step (0.8 - 1.3 KB per lane against 0.6 - 0.9,
//                        and 12 - 22 % on a launch in which no env finishes; profiles/collect).  Inside the branch the env
//                        state is dead between store_env and load_env, so the restart's registers overlap it.
template <typename T> struct CollectArgs {
    uint64_t explore_seed;
    const T* sigma;                       // [n_policies], null = no noise
    T* reward_trace; uint8_t* done_trace; T* eps_trace; T* feat_trace;
    const MealSlots* slots;               // the meal windows in device memory (on_done = 1)
    int on_done;
};

#ifndef T1D_COLLECT_RESTART_INLINE
#define T1D_COLLECT_RESTART_INLINE 1
#endif
#if T1D_COLLECT_RESTART_INLINE
#define T1D_COLLECT_RESTART_ATTR __forceinline__
#else
#define T1D_COLLECT_RESTART_ATTR __noinline__
#endif

// The next episode of env i, whose finished step is in memory (outputs and state): t1d_restart_done for one env.  All
// arguments by value: out of line, a reference would pin the caller's copy of the kernel arguments in scratch.
template <typename T>
__device__ T1D_COLLECT_RESTART_ATTR void collect_restart(KArgs<T> a, RestartArgs<T> r, const MealSlots* ms, unsigned i)
{
    if (restart_front(a, r, a.done, i)) restart_env(a, r, *ms, i);
}

// collect_restart with the decision taken by the caller instead of read from batch.done: t1d_restart_done for one env whose mask
// byte is set.  An env cut by a time limit restarts with done = 0 in memory (mlp_collect_limit_kernel).
template <typename T>
__device__ T1D_COLLECT_RESTART_ATTR void collect_restart_masked(KArgs<T> a, RestartArgs<T> r, const MealSlots* ms, unsigned i)
{
    restart_front_set(a, r, i);
    restart_env(a, r, *ms, i);
}

// ---- t1d_meal_bolus: a bolus calculator beside the network (the *_bolus entry points of include/t1d.h) ---------------------
// The network commands the basal rate; each announced meal is dosed by BBController's rule, rollout_body's expressions
// (t1d_kernels.hpp) in its operation order, from words the stepping kernels hold anyway: the observation the step starts from
// (CGM[0]) and prev_meal.  A NaN in pm or obs gives 0 through the comparisons.  Every kernel that forms the bolus calls
// meal_bolus, so the word is theirs.
//   cr[i], cf[i]   per-lane vector loads.  T1D_BOLUS_LOAD_ONCE = 0: at their use, inside the pm > 0 branch -- a step without
//                  an announced meal reads neither, and nothing of the rule is alive across the step.  1: once per launch,
//                  two more words alive through every step.  The instances' scratch is within 8 bytes per lane between the
//                  two forms and above the bolus-free siblings' in both (profiles/policy/kernel_resources_bolus.txt), and the
//                  clock does not separate them either (profiles/policy/README.md), so the default is the form that keeps
//                  nothing alive.
#ifndef T1D_BOLUS_LOAD_ONCE
#define T1D_BOLUS_LOAD_ONCE 0
#endif
template <typename T> struct BolusArgs {
    T target;                             // BBController.target
    const T* cr; const T* cf;             // [n]
    T* bolus_trace;                       // [rows][n] or null: row mlp.trace_row + s = the bolus of step s, before the pump
};
template <typename T> struct BolusLane { T cr, cf; };           // the lane's two constants where they are loaded once

template <typename T>
__device__ __forceinline__ BolusLane<T> bolus_lane(const BolusArgs<T>& m, unsigned i)
{
    if (T1D_BOLUS_LOAD_ONCE) return BolusLane<T>{at(m.cr, i), at(m.cf, i)};
    return BolusLane<T>{T(1), T(1)};
}

template <typename T>
__device__ __forceinline__ T meal_bolus(const BolusArgs<T>& m, const BolusLane<T>& l, unsigned i, T st, T obs, T pm)
{
    T bolus = T(0);
    if (pm > T(0)) {
        // BBController._bb_policy (basal_bolus_ctrller.py:64-79)
        const T cr = T1D_BOLUS_LOAD_ONCE ? l.cr : (T)at(m.cr, i);
        const T corr = obs > T(150) ? (obs - m.target) / (T1D_BOLUS_LOAD_ONCE ? l.cf : (T)at(m.cf, i)) : T(0);
        bolus = ((pm * st) / cr + corr) / st;
    }
    return bolus;
}

// the bolus of a step of a kernel built with one BolusArgs behind its arguments, and its trace word
template <typename T>
__device__ __forceinline__ T step_bolus(const BolusArgs<T>& m, const BolusLane<T>& l, unsigned i, T st, T obs, T pm, int64_t trow)
{
    const T bolus = meal_bolus(m, l, i, st, obs, pm);
    if (m.bolus_trace) m.bolus_trace[trow] = bolus;
    return bolus;
}
// the first (the only) member of a kernel's trailing pack
template <typename A, typename... R> __device__ __forceinline__ const A& pack_first(const A& a, const R&...) { return a; }

// ---- t1d_env_output: a patient-relative output (the *_rel entry points of include/t1d.h) ------------------------------------
// basal = fma(scale[i], g(y), bias[i]) in the place of fma(out_scale, g(y), out_bias): one weight set commands "a multiple of
// the patient's own basal rate" for a mixed cohort.  The lanes of a wave belong to different patients, so the pair is two
// per-lane vector loads and nothing of it is wave-uniform.  Every *_rel kernel forms the action through the mlp_output below,
// so the word is theirs.  A non-finite scale or bias gives a non-finite basal: what a non-finite network output raises.
//   scale[i], bias[i]   T1D_REL_LOAD_ONCE = 1: once per launch, two more words alive through every step (the fixed-step kernels
//                       only: in the exact mode the pair is always loaded where a step opens).  0: at their use, once per
//                       step -- nothing of the pair is alive across the step.  Loaded once, three of the four fp32 instances
//                       keep 8 bytes per lane less in scratch and one fp64 instance 4 bytes less; the other four are equal
//                       (profiles/policy/kernel_resources_rel.txt).  So once per launch is the default.
#ifndef T1D_REL_LOAD_ONCE
#define T1D_REL_LOAD_ONCE 1
#endif
template <typename T> struct EnvOutArgs { const T* scale; const T* bias; };          // [n] each
template <typename T> struct EnvOutLane { T scale, bias; };

template <typename T>
__device__ __forceinline__ EnvOutLane<T> env_out_lane(const EnvOutArgs<T>& eo, unsigned i)
{
    return EnvOutLane<T>{at(eo.scale, i), at(eo.bias, i)};
}

// the basal a relative policy asks for: mlp_output with the lane's pair in the place of out_scale / out_bias, g unchanged
template <typename T>
__device__ __forceinline__ T mlp_output(const MlpArgs<T>& c, T y, const EnvOutLane<T>& l)
{
    return fma(l.scale, c.out_act == 0 ? y : mlp_logistic(y), l.bias);
}

// mlp_action under the lane's pair: the action of one step of a relative policy
template <typename T>
__device__ __forceinline__ T mlp_action(const MlpArgs<T>& c, const __attribute__((address_space(4))) T* w, const T* col, T* buf,
                                        int head, T prev_meal, int clock, const EnvOutLane<T>& l)
{
    mlp_features(c, col, buf, head, prev_meal, clock);
    return mlp_output(c, mlp_layers(c, w, buf, 2 * c.history + 3), l);
}

// ---- t1d_time_limit: episodes cut at max_minutes (t1d_collect_mlp_limit of include/t1d.h) -----------------------------------
// After a step closes, an env that did not finish and whose clock e.t has reached max_minutes is cut: its step is recorded with
// done = 0 and cut = 1, the features of the state it ended in go to cut_feat (mlp_features on the shifted windows, the step's
// meal and the clock start + e.t: the words t1d_mlp_features would return), and the env restarts as a finished one does.  Of all
// this only max_minutes (wave-uniform) is looked at outside the cut branch, and nothing of it is alive across step_body.
template <typename T> struct LimitArgs {
    int max_minutes;
    uint8_t* cut_trace;                   // [rows][n] or null
    T* cut_feat;                          // [F][n] or null
};

// what mlp_collect_body's trailing pack means: one BolusArgs -- the *_bolus kernels, a bolus in every step; a BolusArgs and an
// EnvOutArgs -- the *_rel kernels, the bolus a wave-uniform run-time switch (cr is NULL for a policy without meal_bolus); with a
// LimitArgs behind the two -- the *_limit kernels, the *_rel form with the time limit, in which the pair is a wave-uniform
// switch as well (scale is NULL for a policy that is not relative: the lane's pair is then out_scale, out_bias, and fma forms
// the word mlp_output forms from them)
template <typename T> __device__ __forceinline__ bool bolus_on(const BolusArgs<T>&) { return true; }
template <typename T, typename... L> __device__ __forceinline__ bool bolus_on(const BolusArgs<T>& m, const EnvOutArgs<T>&, const L&...) { return m.cr != nullptr; }
template <typename A, typename B, typename... L> __device__ __forceinline__ const B& pack_second(const A&, const B& b, const L&...) { return b; }
template <typename A, typename B, typename C> __device__ __forceinline__ const C& pack_third(const A&, const B&, const C& c) { return c; }

// the lane's pair under a *_limit kernel
template <typename T>
__device__ __forceinline__ EnvOutLane<T> env_out_lane_or(const MlpArgs<T>& c, const EnvOutArgs<T>& eo, unsigned i)
{
    if (eo.scale) return env_out_lane(eo, i);                  // wave-uniform
    return EnvOutLane<T>{c.out_scale, c.out_bias};
}

// t1d_mlp_bolus: the rule alone, one lane per env -- the bolus the next step of a *_bolus roll-out would ask for, from
// batch.cgm (CGM[0]) and the policy's prev_meal.  Reads only; writes bolus [n].
template <typename T>
__global__ __launch_bounds__(T1D_POLICY_THREADS) void mlp_bolus_kernel(const KArgs<T> a, const MlpArgs<T> c, const BolusArgs<T> m, T* bolus)
{
    const unsigned i = blockIdx.x * blockDim.x + threadIdx.x;
    __builtin_assume(i < (1u << 28));          // host guarantees n <= 2^28: i * sizeof(T) fits a 32-bit voffset
    if ((int64_t)i >= a.n) return;
    const T obs = at(a.cgm, i), pm = at(c.prev_meal, i);
    at(bolus, i) = meal_bolus(m, bolus_lane(m, i), i, T(a.sen.st), obs, pm);
}

// write_outputs (t1d_kernels.hpp) with the risk of o.cgm handed in -- the word the collector's body formed the step's reward
// with -- instead of evaluated once more.  mlp_collect_body evaluates that risk in its loop, and write_outputs again where a
// finished env's step goes to memory and where the launch ends; the compiler is free to contract each inlined copy differently,
// and in an fp64 instance of mlp_collect_rel_kernel the copy in the finished-env branch came out 2 ulp from the loop's for one
// ending in about five hundred: the env's last_return then was not the loop of one-step launches' word.  The *_rel kernels
// therefore have one evaluation per step, and everything written about the step comes from it.
template <int MATH, typename T>
__device__ __forceinline__ void write_outputs_rc(const KArgs<T>& a, unsigned i, Env<T>& e, const StepOut<T>& o, T rp, T rc)
{
    if (ab_flag(a, 0x100)) rc = T(0);
    at(a.reward, i) = rp - rc;
    e.prev_risk = rc;
    at(a.cgm, i) = o.cgm; at(a.bg, i) = o.bg;
    at(a.done, i) = (o.bg < T(70) || o.bg > T(350)) ? 1 : 0;  // env.py:103
    if (a.lbgi || a.hbgi || a.risk) {
        T l, h, r;
        risk_index1<MATH>(o.bg, l, h, r);                 // env.py:85
        if (a.lbgi) at(a.lbgi, i) = l;
        if (a.hbgi) at(a.hbgi, i) = h;
        if (a.risk) at(a.risk, i) = r;
    }
    if (a.meal) at(a.meal, i) = o.meal;
    if (a.insulin) at(a.insulin, i) = o.ins;
    if (!(fabs((double)e.x[12]) <= 1.0e300)) atomicOr(a.status, T1D_ST_NONFINITE);
}

// mlp_rollout_body with the exploration draw, the per-step reward / done / feature histories and the restart of finished
// envs.  Without sigma and with on_done = 0 it computes what mlp_rollout_body computes, word for word.
// MB: nothing (bolus 0: t1d_collect_mlp) or one BolusArgs (t1d_collect_mlp_bolus, and t1d_rollout_mlp_bolus in the form just
// named): the meal bolus of the step goes into the pump's bolus slot beside the network's basal.  A restarted env has
// prev_meal = 0, hence no bolus on its first step.
// MB = one BolusArgs and one EnvOutArgs (the *_rel entry points): the action is formed with the lane's scale and bias, and the
// bolus is there when the BolusArgs has a cr.
// MB = those two and one LimitArgs (t1d_collect_mlp_limit): the same, the pair there when the EnvOutArgs has a scale, and an env
// whose clock has reached max_minutes when a step closes is cut and restarts (LimitArgs above).
template <int VARIANT, typename T, typename P, typename PR = NoProp, typename... MB>
__device__ __forceinline__ void mlp_collect_body(const KArgs<T>& a, const MlpArgs<T>& c, const CollectArgs<T>& g, const RestartArgs<T>& r,
                                                 P& p, unsigned i, uint32_t pid, Env<T>& e, T* col, PR pr = PR(), const MB&... mb)
{
    constexpr int MATH = VariantMath<VARIANT>::value;
    constexpr bool REL = sizeof...(MB) >= 2, LIMIT = sizeof...(MB) == 3;
    typedef const __attribute__((address_space(4))) T* WPtr;
    const int H = c.history, F = 2 * H + 3;
    T* const buf = col + 2 * H * 64;
    const unsigned wave0 = __builtin_amdgcn_readfirstlane(i & ~63u);
    const unsigned pol = wave0 / c.envs_per_policy;
    const WPtr w = (WPtr)(c.params + (size_t)pol * (size_t)c.n_params);
    const T sg = g.sigma ? (T)((WPtr)g.sigma)[pol] : T(0);      // one sigma per wave, as the weights
    col[0] = at(a.cgm, i);                                      // CGM[0] is the observation the step starts from
    for (int k = 1; k < H; ++k) col[k * 64] = at(rowv(c.cgm_hist, a.n, k), i);
    for (int k = 0; k < H; ++k) col[(H + k) * 64] = at(rowv(c.ins_hist, a.n, k), i);
    int head = 0;
    T prev_meal = at(c.prev_meal, i);
    int start = c.start_minute ? (int)at(c.start_minute, i) : 0;
    uint32_t ep = (g.sigma && a.episode) ? at(a.episode, i) : 0u;
    T sum_risk = c.sum_risk ? at(c.sum_risk, i) : T(0);
    T min_bg = c.min_bg ? at(c.min_bg, i) : T(0), max_bg = c.max_bg ? at(c.max_bg, i) : T(0);
    int n_low = c.n_low ? at(c.n_low, i) : 0, n_high = c.n_high ? at(c.n_high, i) : 0;
    StepOut<T> o{T(0), T(0), T(0), T(0)};
    T rp = e.prev_risk;                         // risk of the observation the last step started from
    bool fresh = false;                         // the last step ended the episode: outputs and state are in memory already
    BolusLane<T> bl{T(1), T(1)};
    if constexpr (sizeof...(MB) > 0) { if (bolus_on(mb...)) bl = bolus_lane(pack_first(mb...), i); }
    EnvOutLane<T> el{T(1), T(0)};
    if constexpr (LIMIT && T1D_REL_LOAD_ONCE) el = env_out_lane_or(c, pack_second(mb...), i);
    else if constexpr (REL && T1D_REL_LOAD_ONCE) el = env_out_lane(pack_second(mb...), i);
#pragma unroll 1
    for (int s = 0; s < c.n_steps; ++s) {
        const int64_t trow = (c.trace_row + s) * a.n + i;
        mlp_features(c, col, buf, head, prev_meal, start + e.t);
        if (g.feat_trace)
            for (int j = 0; j < F; ++j) g.feat_trace[((c.trace_row + s) * F + j) * a.n + i] = buf[j * 64];
        T y = mlp_layers(c, w, buf, F);
        T eps = T(0);
        if (g.sigma) {                          // wave-uniform
            eps = (T)philox_pair(g.explore_seed, (uint64_t)(a.env_offset + i), ep, (uint32_t)e.t).x;
            y = fma(sg, eps, y);
        }
        T u;
        if constexpr (LIMIT) u = mlp_output(c, y, T1D_REL_LOAD_ONCE ? el : env_out_lane_or(c, pack_second(mb...), i));
        else if constexpr (REL) u = mlp_output(c, y, T1D_REL_LOAD_ONCE ? el : env_out_lane(pack_second(mb...), i));
        else u = mlp_output(c, y);
        T bolus = T(0);
        if constexpr (sizeof...(MB) > 0) { if (bolus_on(mb...)) bolus = step_bolus(pack_first(mb...), bl, i, T(a.sen.st), col[head * 64], prev_meal, trow); }
        rp = e.prev_risk;
        o = step_body<MATH, T, P, true, PR, VariantInfo<VARIANT>::tiered>(a, p, i, e, u, bolus, true, pr);
        // the step's reward and done, as write_outputs forms them
        T rl, rh, rc;
        risk_index1<MATH>(o.cgm, rl, rh, rc);
        e.prev_risk = rc;
        const T reward = rp - rc;
        const bool fin = o.bg < T(70) || o.bg > T(350);
        prev_meal = o.meal;
        head = head == 0 ? H - 1 : head - 1;                    // the oldest row becomes the newest
        col[head * 64] = o.cgm; col[(H + head) * 64] = o.ins;
        if (c.bg_trace) c.bg_trace[trow] = o.bg;
        if (c.cgm_trace) c.cgm_trace[trow] = o.cgm;
        if (c.cho_trace) c.cho_trace[trow] = o.meal;
        if (c.ins_trace) c.ins_trace[trow] = o.ins;
        if (c.act_trace) c.act_trace[trow] = u;
        if (g.reward_trace) g.reward_trace[trow] = reward;
        if (g.done_trace) g.done_trace[trow] = fin ? 1 : 0;
        if (g.eps_trace) g.eps_trace[trow] = eps;
        if (c.sum_risk) { T l, h, q; risk_index1<MATH>(o.bg, l, h, q); sum_risk += q; }
        min_bg = o.bg < min_bg ? o.bg : min_bg;
        max_bg = o.bg > max_bg ? o.bg : max_bg;
        n_low += o.bg < T(70); n_high += o.bg > T(180);
        fresh = false;
        bool cut = false;                       // the time limit ends the episode here (never a finished one)
        if constexpr (LIMIT) {
            const LimitArgs<T>& lim = pack_third(mb...);
            cut = !fin && e.t >= lim.max_minutes;
            if (lim.cut_trace) lim.cut_trace[trow] = cut ? 1 : 0;
        }
        if (g.on_done) {
            if (fin || cut) {
                if constexpr (LIMIT) {
                    // the features of the state the cut episode ended in: the windows are shifted, prev_meal is the step's meal
                    // and e.t the clock after the step -- what t1d_mlp_features would read; buf is free between two steps
                    const LimitArgs<T>& lim = pack_third(mb...);
                    if (cut && lim.cut_feat) {
                        mlp_features(c, col, buf, head, prev_meal, start + e.t);
                        for (int j = 0; j < F; ++j) at(rowv(lim.cut_feat, a.n, j), i) = buf[j * 64];
                    }
                }
                // the finished step goes to memory as the end of a launch leaves it; the restart works on those words
                if constexpr (REL) write_outputs_rc<MATH>(a, i, e, o, rp, rc);
                else write_outputs<MATH>(a, i, e, o, rp);
                store_env(a, i, pid, e);
                if constexpr (LIMIT) collect_restart_masked<T>(a, r, g.slots, i);      // a cut env's done is 0
                else collect_restart<T>(a, r, g.slots, i);
                load_env(a, i, at(a.meta, i), e);
                const T first = at(a.cgm, i);                   // the new episode's first observation
                for (int k = 0; k < H; ++k) { col[k * 64] = first; col[(H + k) * 64] = T(0); }
                prev_meal = T(0);
                if (c.start_minute) start = (int)at(c.start_minute, i);
                if (g.sigma) ep = at(a.episode, i);
                fresh = true;
            } else if (r.ep_return) {                           // restart_front's accumulators for an env that goes on
                const T sum = at(r.ep_return, i) + reward;
                const int len = at(r.ep_length, i) + 1;
                at(r.ep_return, i) = sum; at(r.ep_length, i) = len;
            }
        }
    }
    if (!fresh) {
        if constexpr (REL) write_outputs_rc<MATH>(a, i, e, o, rp, e.prev_risk);     // the last step's risk
        else write_outputs<MATH>(a, i, e, o, rp);
        store_env(a, i, pid, e);
    }
    for (int k = 0, q = head; k < H; ++k) {                     // the windows back in window order
        at(rowv(c.cgm_hist, a.n, k), i) = col[q * 64];
        at(rowv(c.ins_hist, a.n, k), i) = col[(H + q) * 64];
        q = q + 1 == H ? 0 : q + 1;
    }
    at(c.prev_meal, i) = prev_meal;
    if (c.sum_risk) at(c.sum_risk, i) = sum_risk;
    if (c.min_bg) at(c.min_bg, i) = min_bg;
    if (c.max_bg) at(c.max_bg, i) = max_bg;
    if (c.n_low) at(c.n_low, i) = n_low;
    if (c.n_high) at(c.n_high, i) = n_high;
}

// Launch shape, LDS and VARIANT as for mlp_rollout_kernel.
template <int VARIANT, typename T>
__global__ __launch_bounds__(T1D_POLICY_THREADS) void mlp_collect_kernel(const KArgs<T> a, const MlpArgs<T> c, const CollectArgs<T> g,
                                                                         const RestartArgs<T> r)
{
    using VI = VariantInfo<VARIANT>;
    constexpr int kParRows = VI::split ? DP_COUNT : DP_RK4_COUNT;
    __shared__ T lds[VI::lds_pars ? kParRows * kMaxPatients : 1];
    if (VI::lds_pars) stage_pars(a, lds, kParRows);
    if (VI::split) stage_prop(a, (T*)t1d_dyn_lds);
    const unsigned i = blockIdx.x * blockDim.x + threadIdx.x;
    __builtin_assume(i < (1u << 28));          // host guarantees n <= 2^28: i * sizeof(T) fits a 32-bit voffset
    if ((int64_t)i >= a.n) return;
    T* const col = (T*)(t1d_dyn_lds + c.lds_off) + (threadIdx.x >> 6) * (c.cols * 64) + (threadIdx.x & 63u);
    const uint32_t meta = at(a.meta, i);
    const uint32_t pid = T1D_META_PID(meta);
    Env<T> e;
    load_env(a, i, meta, e);
    if constexpr (VARIANT == 4 || VARIANT == 6) {
        ParsReg<T> p;
        p.load(a.dpar, (int)pid);
        mlp_collect_body<VARIANT>(a, c, g, r, p, i, pid, e, col, PropLds<T>{(const T*)t1d_dyn_lds, a.np_pad, (int)pid});
    } else if constexpr (VARIANT == 7) {
        ParsLds<T> p{lds, (int)pid};
        mlp_collect_body<VARIANT>(a, c, g, r, p, i, pid, e, col, PropLds<T>{(const T*)t1d_dyn_lds, a.np_pad, (int)pid});
    } else if constexpr (VARIANT == 3) {
        ParsReg<T> p;
        p.load(a.dpar, (int)pid);
        mlp_collect_body<VARIANT>(a, c, g, r, p, i, pid, e, col);
    } else {
        ParsLds<T> p{lds, (int)pid};
        mlp_collect_body<VARIANT>(a, c, g, r, p, i, pid, e, col);
    }
}

// mlp_collect_kernel with the meal bolus of m in every step (t1d_collect_mlp_bolus, t1d_rollout_mlp_bolus): the same body with
// one BolusArgs in its trailing pack.  A kernel of its own name and not an instance of one template with the pack, so that the
// bolus-free instances keep their symbols from build to build (tools/isa_diff.py compares by symbol).
template <int VARIANT, typename T>
__global__ __launch_bounds__(T1D_POLICY_THREADS) void mlp_collect_bolus_kernel(const KArgs<T> a, const MlpArgs<T> c, const CollectArgs<T> g,
                                                                               const RestartArgs<T> r, const BolusArgs<T> m)
{
    using VI = VariantInfo<VARIANT>;
    constexpr int kParRows = VI::split ? DP_COUNT : DP_RK4_COUNT;
    __shared__ T lds[VI::lds_pars ? kParRows * kMaxPatients : 1];
    if (VI::lds_pars) stage_pars(a, lds, kParRows);
    if (VI::split) stage_prop(a, (T*)t1d_dyn_lds);
    const unsigned i = blockIdx.x * blockDim.x + threadIdx.x;
    __builtin_assume(i < (1u << 28));          // host guarantees n <= 2^28: i * sizeof(T) fits a 32-bit voffset
    if ((int64_t)i >= a.n) return;
    T* const col = (T*)(t1d_dyn_lds + c.lds_off) + (threadIdx.x >> 6) * (c.cols * 64) + (threadIdx.x & 63u);
    const uint32_t meta = at(a.meta, i);
    const uint32_t pid = T1D_META_PID(meta);
    Env<T> e;
    load_env(a, i, meta, e);
    if constexpr (VARIANT == 4 || VARIANT == 6) {
        ParsReg<T> p;
        p.load(a.dpar, (int)pid);
        mlp_collect_body<VARIANT>(a, c, g, r, p, i, pid, e, col, PropLds<T>{(const T*)t1d_dyn_lds, a.np_pad, (int)pid}, m);
    } else if constexpr (VARIANT == 7) {
        ParsLds<T> p{lds, (int)pid};
        mlp_collect_body<VARIANT>(a, c, g, r, p, i, pid, e, col, PropLds<T>{(const T*)t1d_dyn_lds, a.np_pad, (int)pid}, m);
    } else if constexpr (VARIANT == 3) {
        ParsReg<T> p;
        p.load(a.dpar, (int)pid);
        mlp_collect_body<VARIANT>(a, c, g, r, p, i, pid, e, col, NoProp(), m);
    } else {
        ParsLds<T> p{lds, (int)pid};
        mlp_collect_body<VARIANT>(a, c, g, r, p, i, pid, e, col, NoProp(), m);
    }
}

// mlp_collect_kernel under a relative policy (t1d_collect_mlp_rel, t1d_rollout_mlp_rel): the same body with a BolusArgs and an
// EnvOutArgs in its trailing pack.  m.cr == NULL: no meal bolus, a wave-uniform branch in every step -- one family for the
// relative policy with and without the bolus.
template <int VARIANT, typename T>
__global__ __launch_bounds__(T1D_POLICY_THREADS) void mlp_collect_rel_kernel(const KArgs<T> a, const MlpArgs<T> c, const CollectArgs<T> g,
                                                                               const RestartArgs<T> r, const EnvOutArgs<T> eo, const BolusArgs<T> m)
{
    using VI = VariantInfo<VARIANT>;
    constexpr int kParRows = VI::split ? DP_COUNT : DP_RK4_COUNT;
    __shared__ T lds[VI::lds_pars ? kParRows * kMaxPatients : 1];
    if (VI::lds_pars) stage_pars(a, lds, kParRows);
    if (VI::split) stage_prop(a, (T*)t1d_dyn_lds);
    const unsigned i = blockIdx.x * blockDim.x + threadIdx.x;
    __builtin_assume(i < (1u << 28));          // host guarantees n <= 2^28: i * sizeof(T) fits a 32-bit voffset
    if ((int64_t)i >= a.n) return;
    T* const col = (T*)(t1d_dyn_lds + c.lds_off) + (threadIdx.x >> 6) * (c.cols * 64) + (threadIdx.x & 63u);
    const uint32_t meta = at(a.meta, i);
    const uint32_t pid = T1D_META_PID(meta);
    Env<T> e;
    load_env(a, i, meta, e);
    if constexpr (VARIANT == 4 || VARIANT == 6) {
        ParsReg<T> p;
        p.load(a.dpar, (int)pid);
        mlp_collect_body<VARIANT>(a, c, g, r, p, i, pid, e, col, PropLds<T>{(const T*)t1d_dyn_lds, a.np_pad, (int)pid}, m, eo);
    } else if constexpr (VARIANT == 7) {
        ParsLds<T> p{lds, (int)pid};
        mlp_collect_body<VARIANT>(a, c, g, r, p, i, pid, e, col, PropLds<T>{(const T*)t1d_dyn_lds, a.np_pad, (int)pid}, m, eo);
    } else if constexpr (VARIANT == 3) {
        ParsReg<T> p;
        p.load(a.dpar, (int)pid);
        mlp_collect_body<VARIANT>(a, c, g, r, p, i, pid, e, col, NoProp(), m, eo);
    } else {
        ParsLds<T> p{lds, (int)pid};
        mlp_collect_body<VARIANT>(a, c, g, r, p, i, pid, e, col, NoProp(), m, eo);
    }
}

// mlp_collect_rel_kernel with episodes cut at a time limit (t1d_collect_mlp_limit): the same body with a LimitArgs behind the
// BolusArgs and the EnvOutArgs.  eo.scale == NULL: the policy's own out_scale / out_bias, m.cr == NULL: no meal bolus -- one
// family for the plain, the hybrid and the relative policy under a limit.
template <int VARIANT, typename T>
__global__ __launch_bounds__(T1D_POLICY_THREADS) void mlp_collect_limit_kernel(const KArgs<T> a, const MlpArgs<T> c, const CollectArgs<T> g,
                                                                               const RestartArgs<T> r, const EnvOutArgs<T> eo, const BolusArgs<T> m,
                                                                               const LimitArgs<T> lim)
{
    using VI = VariantInfo<VARIANT>;
    constexpr int kParRows = VI::split ? DP_COUNT : DP_RK4_COUNT;
    __shared__ T lds[VI::lds_pars ? kParRows * kMaxPatients : 1];
    if (VI::lds_pars) stage_pars(a, lds, kParRows);
    if (VI::split) stage_prop(a, (T*)t1d_dyn_lds);
    const unsigned i = blockIdx.x * blockDim.x + threadIdx.x;
    __builtin_assume(i < (1u << 28));          // host guarantees n <= 2^28: i * sizeof(T) fits a 32-bit voffset
    if ((int64_t)i >= a.n) return;
    T* const col = (T*)(t1d_dyn_lds + c.lds_off) + (threadIdx.x >> 6) * (c.cols * 64) + (threadIdx.x & 63u);
    const uint32_t meta = at(a.meta, i);
    const uint32_t pid = T1D_META_PID(meta);
    Env<T> e;
    load_env(a, i, meta, e);
    if constexpr (VARIANT == 4 || VARIANT == 6) {
        ParsReg<T> p;
        p.load(a.dpar, (int)pid);
        mlp_collect_body<VARIANT>(a, c, g, r, p, i, pid, e, col, PropLds<T>{(const T*)t1d_dyn_lds, a.np_pad, (int)pid}, m, eo, lim);
    } else if constexpr (VARIANT == 7) {
        ParsLds<T> p{lds, (int)pid};
        mlp_collect_body<VARIANT>(a, c, g, r, p, i, pid, e, col, PropLds<T>{(const T*)t1d_dyn_lds, a.np_pad, (int)pid}, m, eo, lim);
    } else if constexpr (VARIANT == 3) {
        ParsReg<T> p;
        p.load(a.dpar, (int)pid);
        mlp_collect_body<VARIANT>(a, c, g, r, p, i, pid, e, col, NoProp(), m, eo, lim);
    } else {
        ParsLds<T> p{lds, (int)pid};
        mlp_collect_body<VARIANT>(a, c, g, r, p, i, pid, e, col, NoProp(), m, eo, lim);
    }
}

// ---- t1d_collect_pid / t1d_collect_bb: trajectories under the two hand-written controllers ---------------------------------
//   ctrl_collect_kernel  mlp_collect_kernel with the controller of rollout_pid_kernel in the place of the network: the env state
//                        in registers, the two windows and the feature buffer in the lane's LDS column (4 H + 3 words per lane:
//                        there are no activation columns), no weights and no draw.  Every step forms the features a network
//                        would have been given (mlp_features, written to feat_trace) and records what the controller asked for
//                        (basal + bolus, to the policy's action_trace): the two halves of a behaviour-cloning sample.  Reward,
//                        done, the restart of a finished env and the episode accumulators are mlp_collect_body's; a restarted
//                        env's controller state becomes what PIDController.reset / BBController.reset leave.
//   the controller       ctrl_policy below: rollout_body's expressions (t1d_kernels.hpp) under the same run-time `kind`, so that
//                        the action of a step is the word rollout_pid_kernel computes from the same observation and state.
//                        rollout_body leaves the PID's contraction into fused multiply-adds to the compiler, which forms
//                        u = fma(I, integ, P (obs - target)) + D (obs - prev) / st and integ = fma(obs - target, st, integ) in
//                        all eight instances of rollout_pid_kernel; left to itself here it formed fma(P, obs - target, I integ)
//                        in an fp32 instance, another word.  So ctrl_policy writes the two fused multiply-adds out.  Calling
//                        it from rollout_body as well moved instructions in three of that kernel's fp32 instances, so
//                        rollout_body keeps its text: change one, check the other (tests/test_gpu_collect_ctrl.py does).
//   traces               every row index is the controller's trace_row (PidArgs); the policy's own trace_row is not read.
template <typename T>
__device__ __forceinline__ void ctrl_policy(const PidArgs<T>& c, bool bb, T st, T obs, T bb_basal, T bb_cr, T bb_cf, T prev_meal,
                                            T& integ, T& prev, T& u, T& bolus)
{
    bolus = T(0);
    if (bb) {
        // BBController._bb_policy (basal_bolus_ctrller.py:64-79)
        u = bb_basal;
        if (prev_meal > T(0)) {
            const T corr = obs > T(150) ? (obs - c.target) / bb_cf : T(0);
            bolus = ((prev_meal * st) / bb_cr + corr) / st;
        }
    } else {
        // PIDController.policy (pid_ctrller.py:17-36): P (obs - target) + I integ + D (obs - prev) / st, integ += (obs - target) st
        u = fma(c.I, integ, c.P * (obs - c.target)) + c.D * (obs - prev) / st;
        prev = obs;
        integ = fma(obs - c.target, st, integ);
    }
}

// LM: nothing (t1d_collect_pid / t1d_collect_bb) or one LimitArgs (t1d_collect_pid_limit / t1d_collect_bb_limit): an env whose
// clock has reached max_minutes when a step closes is cut and restarts, as in mlp_collect_body.
template <int VARIANT, typename T, typename P, typename PR = NoProp, typename... LM>
__device__ __forceinline__ void ctrl_collect_body(const KArgs<T>& a, const PidArgs<T>& c, const MlpArgs<T>& f, const CollectArgs<T>& g,
                                                  const RestartArgs<T>& r, P& p, unsigned i, uint32_t pid, Env<T>& e, T* col, PR pr = PR(),
                                                  const LM&... lm)
{
    constexpr int MATH = VariantMath<VARIANT>::value;
    constexpr bool LIMIT = sizeof...(LM) == 1;
    const int H = f.history, F = 2 * H + 3;
    T* const buf = col + 2 * H * 64;
    T obs = at(a.cgm, i);
    col[0] = obs;                                               // CGM[0] is the observation the step starts from
    for (int k = 1; k < H; ++k) col[k * 64] = at(rowv(f.cgm_hist, a.n, k), i);
    for (int k = 0; k < H; ++k) col[(H + k) * 64] = at(rowv(f.ins_hist, a.n, k), i);
    int head = 0;
    T feat_meal = at(f.prev_meal, i);                           // the policy's prev_meal: its own array, the same word after a step
    int start = f.start_minute ? (int)at(f.start_minute, i) : 0;
    const bool bb = c.kind == 1;
    T integ = T(0), prev = T(0), bb_basal = T(0), bb_cr = T(1), bb_cf = T(1), prev_meal = T(0);
    if (bb) { bb_basal = at(c.bb_basal, i); bb_cr = at(c.bb_cr, i); bb_cf = at(c.bb_cf, i); prev_meal = at(c.bb_prev_meal, i); }
    else { integ = at(c.integ, i); prev = at(c.prev, i); }
    T sum_risk = c.sum_risk ? at(c.sum_risk, i) : T(0);
    T min_bg = c.min_bg ? at(c.min_bg, i) : T(0), max_bg = c.max_bg ? at(c.max_bg, i) : T(0);
    int n_low = c.n_low ? at(c.n_low, i) : 0, n_high = c.n_high ? at(c.n_high, i) : 0;
    const T st = T(a.sen.st);
    StepOut<T> o{T(0), T(0), T(0), T(0)};
    T rp = e.prev_risk;                         // risk of the observation the last step started from
    bool fresh = false;                         // the last step ended the episode: outputs and state are in memory already
#pragma unroll 1
    for (int s = 0; s < c.n_steps; ++s) {
        const int64_t trow = (c.trace_row + s) * a.n + i;
        mlp_features(f, col, buf, head, feat_meal, start + e.t);
        if (g.feat_trace)
            for (int j = 0; j < F; ++j) g.feat_trace[((c.trace_row + s) * F + j) * a.n + i] = buf[j * 64];
        T u, bolus;
        ctrl_policy(c, bb, st, obs, bb_basal, bb_cr, bb_cf, prev_meal, integ, prev, u, bolus);
        if (f.act_trace) f.act_trace[trow] = u + bolus;         // what the controller asked for, before the pump
        rp = e.prev_risk;
        o = step_body<MATH, T, P, true, PR, VariantInfo<VARIANT>::tiered>(a, p, i, e, u, bolus, true, pr);
        // the step's reward and done, as write_outputs forms them
        T rl, rh, rc;
        risk_index1<MATH>(o.cgm, rl, rh, rc);
        e.prev_risk = rc;
        const T reward = rp - rc;
        const bool fin = o.bg < T(70) || o.bg > T(350);
        obs = o.cgm;
        prev_meal = o.meal;
        feat_meal = o.meal;
        head = head == 0 ? H - 1 : head - 1;                    // the oldest row becomes the newest
        col[head * 64] = o.cgm; col[(H + head) * 64] = o.ins;
        if (c.bg_trace) c.bg_trace[trow] = o.bg;
        if (c.cgm_trace) c.cgm_trace[trow] = o.cgm;
        if (c.cho_trace) c.cho_trace[trow] = o.meal;
        if (c.ins_trace) c.ins_trace[trow] = o.ins;
        if (g.reward_trace) g.reward_trace[trow] = reward;
        if (g.done_trace) g.done_trace[trow] = fin ? 1 : 0;
        if (c.sum_risk) { T l, h, q; risk_index1<MATH>(o.bg, l, h, q); sum_risk += q; }
        min_bg = o.bg < min_bg ? o.bg : min_bg;
        max_bg = o.bg > max_bg ? o.bg : max_bg;
        n_low += o.bg < T(70); n_high += o.bg > T(180);
        fresh = false;
        bool cut = false;                       // the time limit ends the episode here (never a finished one)
        if constexpr (LIMIT) {
            const LimitArgs<T>& lim = pack_first(lm...);
            cut = !fin && e.t >= lim.max_minutes;
            if (lim.cut_trace) lim.cut_trace[trow] = cut ? 1 : 0;
        }
        if (g.on_done) {
            if (fin || cut) {
                if constexpr (LIMIT) {
                    // the features of the state the cut episode ended in: the windows are shifted, feat_meal is the step's meal
                    // and e.t the clock after the step -- what t1d_mlp_features would read; buf is free between two steps
                    const LimitArgs<T>& lim = pack_first(lm...);
                    if (cut && lim.cut_feat) {
                        mlp_features(f, col, buf, head, feat_meal, start + e.t);
                        for (int j = 0; j < F; ++j) at(rowv(lim.cut_feat, a.n, j), i) = buf[j * 64];
                    }
                }
                // the finished step goes to memory as the end of a launch leaves it; the restart works on those words
                write_outputs<MATH>(a, i, e, o, rp);
                store_env(a, i, pid, e);
                if constexpr (LIMIT) collect_restart_masked<T>(a, r, g.slots, i);      // a cut env's done is 0
                else collect_restart<T>(a, r, g.slots, i);
                load_env(a, i, at(a.meta, i), e);
                obs = at(a.cgm, i);                             // the new episode's first observation
                for (int k = 0; k < H; ++k) { col[k * 64] = obs; col[(H + k) * 64] = T(0); }
                feat_meal = T(0);
                integ = T(0); prev = T(0); prev_meal = T(0);    // PIDController.reset, BBController.reset
                if (f.start_minute) start = (int)at(f.start_minute, i);
                fresh = true;
            } else if (r.ep_return) {                           // restart_front's accumulators for an env that goes on
                const T sum = at(r.ep_return, i) + reward;
                const int len = at(r.ep_length, i) + 1;
                at(r.ep_return, i) = sum; at(r.ep_length, i) = len;
            }
        }
    }
    if (!fresh) {
        write_outputs<MATH>(a, i, e, o, rp);
        store_env(a, i, pid, e);
    }
    for (int k = 0, q = head; k < H; ++k) {                     // the windows back in window order
        at(rowv(f.cgm_hist, a.n, k), i) = col[q * 64];
        at(rowv(f.ins_hist, a.n, k), i) = col[(H + q) * 64];
        q = q + 1 == H ? 0 : q + 1;
    }
    at(f.prev_meal, i) = feat_meal;
    if (bb) at(c.bb_prev_meal, i) = prev_meal;
    else { at(c.integ, i) = integ; at(c.prev, i) = prev; }
    if (c.sum_risk) at(c.sum_risk, i) = sum_risk;
    if (c.min_bg) at(c.min_bg, i) = min_bg;
    if (c.max_bg) at(c.max_bg, i) = max_bg;
    if (c.n_low) at(c.n_low, i) = n_low;
    if (c.n_high) at(c.n_high, i) = n_high;
}

// Launch shape, LDS and VARIANT as for mlp_rollout_kernel, with cols = 4 H + 3.  Any n: no lane looks at another.
template <int VARIANT, typename T>
__global__ __launch_bounds__(T1D_POLICY_THREADS) void ctrl_collect_kernel(const KArgs<T> a, const PidArgs<T> c, const MlpArgs<T> f,
                                                                          const CollectArgs<T> g, const RestartArgs<T> r)
{
    using VI = VariantInfo<VARIANT>;
    constexpr int kParRows = VI::split ? DP_COUNT : DP_RK4_COUNT;
    __shared__ T lds[VI::lds_pars ? kParRows * kMaxPatients : 1];
    if (VI::lds_pars) stage_pars(a, lds, kParRows);
    if (VI::split) stage_prop(a, (T*)t1d_dyn_lds);
    const unsigned i = blockIdx.x * blockDim.x + threadIdx.x;
    __builtin_assume(i < (1u << 28));          // host guarantees n <= 2^28: i * sizeof(T) fits a 32-bit voffset
    if ((int64_t)i >= a.n) return;
    T* const col = (T*)(t1d_dyn_lds + f.lds_off) + (threadIdx.x >> 6) * (f.cols * 64) + (threadIdx.x & 63u);
    const uint32_t meta = at(a.meta, i);
    const uint32_t pid = T1D_META_PID(meta);
    Env<T> e;
    load_env(a, i, meta, e);
    if constexpr (VARIANT == 4 || VARIANT == 6) {
        ParsReg<T> p;
        p.load(a.dpar, (int)pid);
        ctrl_collect_body<VARIANT>(a, c, f, g, r, p, i, pid, e, col, PropLds<T>{(const T*)t1d_dyn_lds, a.np_pad, (int)pid});
    } else if constexpr (VARIANT == 7) {
        ParsLds<T> p{lds, (int)pid};
        ctrl_collect_body<VARIANT>(a, c, f, g, r, p, i, pid, e, col, PropLds<T>{(const T*)t1d_dyn_lds, a.np_pad, (int)pid});
    } else if constexpr (VARIANT == 3) {
        ParsReg<T> p;
        p.load(a.dpar, (int)pid);
        ctrl_collect_body<VARIANT>(a, c, f, g, r, p, i, pid, e, col);
    } else {
        ParsLds<T> p{lds, (int)pid};
        ctrl_collect_body<VARIANT>(a, c, f, g, r, p, i, pid, e, col);
    }
}

// ctrl_collect_kernel with episodes cut at a time limit (t1d_collect_pid_limit, t1d_collect_bb_limit): the same body with a
// LimitArgs in its trailing pack.  A kernel of its own name, as mlp_collect_limit_kernel is, so that ctrl_collect_kernel's
// instances keep their symbols and their instruction streams.
template <int VARIANT, typename T>
__global__ __launch_bounds__(T1D_POLICY_THREADS) void ctrl_collect_limit_kernel(const KArgs<T> a, const PidArgs<T> c, const MlpArgs<T> f,
                                                                                const CollectArgs<T> g, const RestartArgs<T> r,
                                                                                const LimitArgs<T> lim)
{
    using VI = VariantInfo<VARIANT>;
    constexpr int kParRows = VI::split ? DP_COUNT : DP_RK4_COUNT;
    __shared__ T lds[VI::lds_pars ? kParRows * kMaxPatients : 1];
    if (VI::lds_pars) stage_pars(a, lds, kParRows);
    if (VI::split) stage_prop(a, (T*)t1d_dyn_lds);
    const unsigned i = blockIdx.x * blockDim.x + threadIdx.x;
    __builtin_assume(i < (1u << 28));          // host guarantees n <= 2^28: i * sizeof(T) fits a 32-bit voffset
    if ((int64_t)i >= a.n) return;
    T* const col = (T*)(t1d_dyn_lds + f.lds_off) + (threadIdx.x >> 6) * (f.cols * 64) + (threadIdx.x & 63u);
    const uint32_t meta = at(a.meta, i);
    const uint32_t pid = T1D_META_PID(meta);
    Env<T> e;
    load_env(a, i, meta, e);
    if constexpr (VARIANT == 4 || VARIANT == 6) {
        ParsReg<T> p;
        p.load(a.dpar, (int)pid);
        ctrl_collect_body<VARIANT>(a, c, f, g, r, p, i, pid, e, col, PropLds<T>{(const T*)t1d_dyn_lds, a.np_pad, (int)pid}, lim);
    } else if constexpr (VARIANT == 7) {
        ParsLds<T> p{lds, (int)pid};
        ctrl_collect_body<VARIANT>(a, c, f, g, r, p, i, pid, e, col, PropLds<T>{(const T*)t1d_dyn_lds, a.np_pad, (int)pid}, lim);
    } else if constexpr (VARIANT == 3) {
        ParsReg<T> p;
        p.load(a.dpar, (int)pid);
        ctrl_collect_body<VARIANT>(a, c, f, g, r, p, i, pid, e, col, NoProp(), lim);
    } else {
        ParsLds<T> p{lds, (int)pid};
        ctrl_collect_body<VARIANT>(a, c, f, g, r, p, i, pid, e, col, NoProp(), lim);
    }
}

// t1d_mlp_features: the features alone, one lane per env -- what the next step of a collector would write to its feat_trace
// row, from the words mlp_action_kernel (t1d_dopri5.hpp) reads: batch.cgm (CGM[0]), rows 1 .. of cgm_hist, ins_hist, prev_meal,
// batch.t and start_minute.  Reads only; writes feat [F][n].  Dynamic LDS: cols * 64 words for each wave, the lane's column in
// window order (head 0), as for mlp_action_kernel.
template <typename T>
__global__ __launch_bounds__(T1D_POLICY_THREADS) void mlp_features_kernel(const KArgs<T> a, const MlpArgs<T> c, T* feat)
{
    const unsigned i = blockIdx.x * blockDim.x + threadIdx.x;
    __builtin_assume(i < (1u << 28));          // host guarantees n <= 2^28: i * sizeof(T) fits a 32-bit voffset
    if ((int64_t)i >= a.n) return;
    T* const col = (T*)t1d_dyn_lds + (threadIdx.x >> 6) * (c.cols * 64) + (threadIdx.x & 63u);
    const int H = c.history, F = 2 * H + 3;
    T* const buf = col + 2 * H * 64;
    col[0] = at(a.cgm, i);
    for (int k = 1; k < H; ++k) col[k * 64] = at(rowv(c.cgm_hist, a.n, k), i);
    for (int k = 0; k < H; ++k) col[(H + k) * 64] = at(rowv(c.ins_hist, a.n, k), i);
    const int start = c.start_minute ? (int)at(c.start_minute, i) : 0;
    const T prev_meal = at(c.prev_meal, i);
    const int t = at(a.t, i);
    mlp_features(c, col, buf, 0, prev_meal, start + t);
    for (int j = 0; j < F; ++j) at(rowv(feat, a.n, j), i) = buf[j * 64];
}

} // namespace t1d
