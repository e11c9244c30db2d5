// t1d_policy_grad.hpp -- the policy network of t1d_policy.hpp on recorded features, and its weight gradient (gfx950 only):
// t1d_mlp_grad of include/t1d.h.  Included by t1d_abi.hip after t1d_policy.hpp, whose mlp_layers / mlp_tanh it calls as
// they are, so that y is the word the roll-outs and the collectors computed from the same features and weights.
//
//   tile                 64 envs of one policy (one 64-env chunk, so one weight set) in one row of the feature trace.  The
//                        tiles of a policy are numbered u = row * chunks + chunk (chunks = envs_per_policy / 64).
//   wave                 one workgroup = one wave = tiles [k * tiles_per_wave, (k + 1) * tiles_per_wave) of one policy; the
//                        host fixes tiles_per_wave from (n, envs_per_policy, n_rows) alone (grad_partition in t1d_abi.hip).
//   LDS                  one column of 64 lanes per word, as in mlp_rollout_kernel (word r of sample s at r * 64 + s):
//                          rows 0 .. A-1       the F features, then every hidden layer's activations (mlp_layers<T, true>)
//                          row  A              1.0, the "input" of every bias
//                          rows A+1 ..         delta = dL/d(pre-activation) of every layer's outputs, layer after layer;
//                                              the last layer's single delta is coef
//                        F = 27 with widths 32/32/32/1 takes 221 rows: 110.5 KiB in fp64, so one wave per workgroup and as
//                        many workgroups on a CU as its 160 KiB hold (one for that net, four for H = 4 with 16/16/1).
//   phase A              lanes = samples: features from memory into the column, mlp_layers (weights through the scalar
//                        data cache), y stored; then the deltas from coef down to layer 0, four inputs at a time:
//                        delta_in[j] = act'(x[j]) * sum over o ascending of W[o][j] delta_out[o], act' = 1 - x^2 (tanh) or
//                        x > 0 (relu) from the stored activation x.
//   phase B              lanes = weights: lane t owns parameters q = t, t + 64, ... (at most kGradSlots of them, in
//                        registers) and adds delta[o][s] * in[j][s] of the tile's 64 samples to each with one fma per
//                        sample, in the order s = (t + m) mod 64, m = 0 .. 63.  Starting at the lane's own sample keeps
//                        the 64 lanes of a read on 64 different banks whatever rows they read; no cross-lane reduction.
//                        The accumulators carry on across the wave's tiles, then go to the workspace as one partial
//                        [n_params] (vector stores).
//   mlp_grad_sum_kernel  grad[p][q] = the partials of policy p added in wave order.
//   with LossArgs        t1d_mlp_loss: mlp_grad_kernel<T, LossArgs<T, KIND>>, the same kernel with a third argument and the loss
//                        between the forward pass and the deltas (the template's trailing pack is empty for t1d_mlp_grad,
//                        whose two instances are compiled from the text they always were).
//                        coef is not read: every lane forms it from y and the loss's inputs of its sample (loss_ppo_clip /
//                        loss_value_mse, the arithmetic of include/t1d.h) and writes it to the last layer's delta row, so
//                        the network is evaluated once and y and coef make no round trip through memory.  Everything from
//                        there on is the code above in its order: grad is what mlp_grad_kernel gives for the stored coef.
//                        The four statistics of a sample are added, in double, to four per-lane sums over the wave's
//                        tiles; behind the tile loop the 64 lane sums are folded 32, 16, .. 1 lanes down and lane 0 stores
//                        one partial [4] per wave behind the gradient partials.  With partial == NULL the deltas and phase
//                        B are skipped; y, coef_out and the statistics are still formed.
//   mlp_loss_stats_kernel  stats[p][k] = the partials of policy p added in wave order.
//   with TileArgs        t1d_mlp_grad_tiles / t1d_mlp_loss_tiles: a TileArgs as the pack's last member, and the waves walk the
//                        positions of the policy's row of a tile list instead of the tile numbers: position pos names tile
//                        u = ids[pol][pos], read through the scalar data cache like the weights, so it is wave-uniform; an id
//                        outside [0, tiles of a policy) is stepped over by one uniform branch around the whole tile body.
//                        Everything inside a tile is the code above on the arrays' own addresses, and the partition is the
//                        one above with positions for tiles, so the identity list gives the plain call's bits and any list
//                        those of a plain call on the gathered tiles.  The instances without TileArgs are compiled from the
//                        text they always were.
// Nothing here is atomic and nothing depends on the grid the hardware happens to run: two calls give the same bits.
#pragma once
#include "t1d_policy.hpp"

namespace t1d {

constexpr int kGradSlots = 48;            // parameters per lane: ceil(3041 / 64) for F = 27, widths 32/32/32/1
constexpr int kGradMaxWaves = 2048;       // partial sums per call, about (grad_partition)

template <typename T> struct GradArgs {
    const T* feat; const T* coef; T* y; T* partial;
    int64_t n;
    unsigned chunks;                      // 64-env chunks of one policy
    unsigned tiles;                       // chunks * n_rows: tiles of one policy (with TileArgs: the positions of its list row)
    unsigned tiles_per_wave, waves_per_policy, n_waves;
    int act_rows;                         // A: F + the hidden widths
};

// t1d_mlp_loss: what the loss of a sample is formed from.  The scalars are the call's doubles converted once on the host.
template <typename T, int KIND> struct LossArgs {   // KIND: T1D_LOSS_PPO_CLIP | T1D_LOSS_VALUE_MSE
    const T* eps; const T* y_old; const T* adv; const T* target;
    const T* sigma_old; const T* sigma;   // [n_policies]
    T* coef_out;                          // [K][n] or null
    double* stat_partial;                 // [n_waves][4] or null
    T clip, scale;
};

// t1d_mlp_grad_tiles / t1d_mlp_loss_tiles: the list the waves walk.  GradArgs.tiles is then the positions of one policy.
struct TileArgs {
    const int32_t* ids;                   // [n_policies][GradArgs.tiles]
    unsigned limit;                       // chunks * n_rows: an id is a tile of the policy when (unsigned)id < limit
};

// the kind of mlp_grad_kernel's trailing pack: 0 without a LossArgs (coef is read from memory), else that of its first member
template <typename... LS> struct LossKind { static constexpr int value = 0; };
template <typename T, int KIND, typename... R> struct LossKind<LossArgs<T, KIND>, R...> { static constexpr int value = KIND; };
template <typename A, typename... R> __device__ __forceinline__ const A& loss_first(const A& a, const R&...) { return a; }
// the pack's TileArgs, which is its last member, or none
template <typename... LS> struct HasTiles { static constexpr bool value = false; };
template <typename A, typename... R> struct HasTiles<A, R...> { static constexpr bool value = HasTiles<R...>::value; };
template <> struct HasTiles<TileArgs> { static constexpr bool value = true; };
__device__ __forceinline__ const TileArgs& tiles_last(const TileArgs& a) { return a; }
template <typename A, typename... R> __device__ __forceinline__ const TileArgs& tiles_last(const A&, const R&... r) { return tiles_last(r...); }

// a wave-uniform word a lane computed, moved to scalar registers so that it costs no vector register in the tile loop
__device__ __forceinline__ float loss_uniform(float v) { return __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, v))); }
__device__ __forceinline__ double loss_uniform(double v)
{
    const long long b = __double_as_longlong(v);
    const unsigned lo = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)b), hi = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)(b >> 32));
    return __longlong_as_double((long long)((unsigned long long)hi << 32 | lo));
}
__device__ __forceinline__ float loss_exp(float x) { return expf(x); }
__device__ __forceinline__ double loss_exp(double x) { return exp(x); }
__device__ __forceinline__ float loss_log(float x) { return logf(x); }
__device__ __forceinline__ double loss_log(double x) { return log(x); }

// T1D_LOSS_PPO_CLIP of include/t1d.h for one sample: -> coef; st[0..3] += (loss, not active, expm1(logr) - logr, dsig).
// dlog = log(sigma_old) - log(sigma).  e_old - e_new is exactly 0 where y == y_old and sg == so bit for bit (the two
// quotients are then the same operation on the same words), so logr is 0 and r is 1 there however the rest is contracted.
template <typename T>
__device__ __forceinline__ T loss_ppo_clip(T y, T eps, T y_old, T adv, T so, T sg, T dlog, T clip, T scale, double (&st)[4])
{
    const T z = fma(so, eps, y_old);
    const T e_old = (z - y_old) / so, e_new = (z - y) / sg;
    const T logr = T(0.5) * ((e_old - e_new) * (e_old + e_new)) + dlog;
    const T r = loss_exp(logr);
    const T lo = T(1) - clip, hi = T(1) + clip;
    const bool active = adv >= T(0) ? r <= hi : r >= lo;
    const T ra = r * adv;
    const T loss = -fmin(ra, fmin(fmax(r, lo), hi) * adv);
    const T gg = active ? -ra : T(0);
    const T dsig = gg * (e_new * e_new - T(1)) / sg;
    const double lr = (double)logr;
    st[0] += (double)loss; st[1] += active ? 0.0 : 1.0; st[2] += expm1(lr) - lr; st[3] += (double)dsig;
    return scale * gg * e_new / sg;
}

// T1D_LOSS_VALUE_MSE
template <typename T>
__device__ __forceinline__ T loss_value_mse(T y, T target, T scale, double (&st)[4])
{
    const T d = y - target;
    st[0] += (double)(T(0.5) * d * d);
    return scale * d;
}

// all lanes of the wave have made their LDS writes visible to each other, and the compiler moves no access across
__device__ __forceinline__ void grad_wave_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// the LDS rows parameter q multiplies: (input row) | (delta row) << 16, both already times 64
template <typename T>
__device__ __forceinline__ unsigned grad_rows_of(const MlpArgs<T>& c, int act_rows, unsigned q)
{
    unsigned base = 0, xoff = 0, doff = (unsigned)act_rows + 1u, res = 0;
    int in_w = 2 * c.history + 3;
    for (int l = 0; l < c.n_layers; ++l) {
        const unsigned out_w = (c.widths >> (8 * l)) & 0xffu;
        const unsigned nw = out_w * (unsigned)in_w;
        if (q >= base && q < base + nw + out_w) {
            const unsigned r = q - base;
            const unsigned o = r < nw ? r / (unsigned)in_w : r - nw;
            const unsigned x = r < nw ? xoff + (r - o * (unsigned)in_w) : (unsigned)act_rows;
            res = (x * 64u) | ((doff + o) * 64u) << 16;
        }
        base += nw + out_w; xoff += (unsigned)in_w; doff += out_w; in_w = (int)out_w;
    }
    return res;                           // q beyond n_params: rows 0 and 0, read and never stored
}

// Dynamic LDS: (act_rows + 1 + the sum of all widths) * 64 words.  Grid: n_waves workgroups of 64 threads.  LS: nothing
// (t1d_mlp_grad: coef is read from g.coef) or one LossArgs<T, KIND> (t1d_mlp_loss: coef comes from the loss, g.coef is not
// looked at), and behind either a TileArgs for the listed calls.
template <typename T, typename... LS>
__global__ __launch_bounds__(64) void mlp_grad_kernel(const MlpArgs<T> c, const GradArgs<T> g, const LS... lp)
{
    constexpr int KIND = LossKind<LS...>::value;
    constexpr bool LISTED = HasTiles<LS...>::value;
    typedef const __attribute__((address_space(4))) T* WPtr;
    const unsigned lane = threadIdx.x;
    const unsigned wave = blockIdx.x;
    const unsigned pol = wave / g.waves_per_policy, part = wave - pol * g.waves_per_policy;
    const unsigned t0 = part * g.tiles_per_wave;
    const unsigned t1 = t0 + g.tiles_per_wave < g.tiles ? t0 + g.tiles_per_wave : g.tiles;
    T* const blk = (T*)t1d_dyn_lds;
    T* const col = blk + lane;
    const WPtr w = (WPtr)(c.params + (size_t)pol * (size_t)c.n_params);
    const int F = 2 * c.history + 3, A = g.act_rows, L = c.n_layers;
    const bool with_grad = g.partial != nullptr;                // kernel argument: wave-uniform
    const int n_slots = (c.n_params + 63) >> 6;

    T acc[kGradSlots];
    unsigned rows[kGradSlots];
#pragma unroll
    for (int k = 0; k < kGradSlots; ++k) { acc[k] = T(0); rows[k] = 0; }
    if (with_grad) {
#pragma unroll
        for (int k = 0; k < kGradSlots; ++k)
            if (k < n_slots) rows[k] = grad_rows_of(c, A, (unsigned)k * 64u + lane);
        col[A * 64] = T(1);
    }
    // offsets of the last layer: its weights in the set, its inputs and its delta among the rows
    int w_last = 0, x_last = 0, d_last = A + 1;
    for (int l = 0, in_w = F; l + 1 < L; ++l) {
        const int out_w = (int)((c.widths >> (8 * l)) & 0xffu);
        w_last += out_w * (in_w + 1); x_last += in_w; d_last += out_w; in_w = out_w;
    }
    // the loss: the policy's two sigmas and the difference of their logarithms, one per wave; the lane's four sums
    double st[4] = {0.0, 0.0, 0.0, 0.0};
    T so = T(1), sg = T(1), dlog = T(0);
    if constexpr (KIND == T1D_LOSS_PPO_CLIP) {
        const auto& ls = loss_first(lp...);
        so = (T)((WPtr)ls.sigma_old)[pol]; sg = (T)((WPtr)ls.sigma)[pol];
        dlog = loss_uniform(loss_log(so) - loss_log(sg));
    }

#pragma unroll 1
    for (unsigned pos = t0; pos < t1; ++pos) {
        unsigned u = pos;
        if constexpr (LISTED) {
            const TileArgs& tl = tiles_last(lp...);
            typedef const __attribute__((address_space(4))) int32_t* IPtr;
            u = (unsigned)((IPtr)tl.ids)[(size_t)pol * g.tiles + pos];           // wave-uniform: a scalar load
            if (u >= tl.limit) continue;                                         // id < 0 or beyond the policy's tiles: skipped
        }
        const unsigned row = u / g.chunks, chunk = u - row * g.chunks;
        const int64_t i = (int64_t)pol * c.envs_per_policy + (int64_t)chunk * 64 + lane;
        const T* const f = g.feat + (int64_t)row * F * g.n + i;
        for (int j = 0; j < F; ++j) col[j * 64] = f[(int64_t)j * g.n];
        T in0 = T(0), in1 = T(0), in2 = T(0);                   // the sample's loss inputs, asked for ahead of the layers
        if constexpr (KIND == T1D_LOSS_PPO_CLIP) {
            const auto& ls = loss_first(lp...);
            in0 = ls.eps[(int64_t)row * g.n + i]; in1 = ls.y_old[(int64_t)row * g.n + i]; in2 = ls.adv[(int64_t)row * g.n + i];
        }
        if constexpr (KIND == T1D_LOSS_VALUE_MSE) in0 = loss_first(lp...).target[(int64_t)row * g.n + i];
        const T y = mlp_layers<T, true>(c, w, col, F);
        if (g.y) g.y[(int64_t)row * g.n + i] = y;
        T coef = T(0);
        if constexpr (KIND != 0) {
            const auto& ls = loss_first(lp...);
            if constexpr (KIND == T1D_LOSS_PPO_CLIP) coef = loss_ppo_clip(y, in0, in1, in2, so, sg, dlog, ls.clip, ls.scale, st);
            else coef = loss_value_mse(y, in0, ls.scale, st);
            if (ls.coef_out) ls.coef_out[(int64_t)row * g.n + i] = coef;
        }
        if (!with_grad) continue;

        // ---- phase A, backwards: delta of layer l's outputs -> delta of layer l - 1's outputs (= layer l's inputs)
        if constexpr (KIND == 0) coef = g.coef[(int64_t)row * g.n + i];
        col[d_last * 64] = coef;
        int woff = w_last, xoff = x_last, doff = d_last;
#pragma unroll 1
        for (int l = L - 1; l >= 1; --l) {
            const int out_w = (int)((c.widths >> (8 * l)) & 0xffu), in_w = (int)((c.widths >> (8 * (l - 1))) & 0xffu);
            const WPtr W = w + woff;                            // row-major [out_w][in_w]
            const T* const dout = col + doff * 64;
            T* const din = col + (doff - in_w) * 64;
            const T* const x = col + xoff * 64;                 // this layer's inputs: the activations of layer l - 1
#pragma unroll 1
            for (int jb = 0; jb < in_w; jb += 4) {
                // beyond the layer's inputs the last one is computed again
                const int last = in_w - 1;
                const int j0 = jb, j1 = jb + 1 < last ? jb + 1 : last, j2 = jb + 2 < last ? jb + 2 : last, j3 = jb + 3 < last ? jb + 3 : last;
                T a0 = T(0), a1 = T(0), a2 = T(0), a3 = T(0);
#pragma unroll 1
                for (int o = 0; o < out_w; ++o) {
                    const T d = dout[o * 64];
                    const WPtr r = W + o * in_w;
                    a0 = fma((T)r[j0], d, a0); a1 = fma((T)r[j1], d, a1); a2 = fma((T)r[j2], d, a2); a3 = fma((T)r[j3], d, a3);
                }
                const T x0 = x[j0 * 64], x1 = x[j1 * 64], x2 = x[j2 * 64], x3 = x[j3 * 64];
                if (c.hidden_act == 0) {
                    a0 *= T(1) - x0 * x0; a1 *= T(1) - x1 * x1; a2 *= T(1) - x2 * x2; a3 *= T(1) - x3 * x3;
                } else {
                    a0 = x0 > T(0) ? a0 : T(0); a1 = x1 > T(0) ? a1 : T(0); a2 = x2 > T(0) ? a2 : T(0); a3 = x3 > T(0) ? a3 : T(0);
                }
                din[j3 * 64] = a3; din[j2 * 64] = a2; din[j1 * 64] = a1; din[j0 * 64] = a0;
            }
            // layer l - 1: its inputs are F features (l == 1) or the layer before's outputs
            const int in_prev = l >= 2 ? (int)((c.widths >> (8 * (l - 2))) & 0xffu) : F;
            woff -= in_w * (in_prev + 1); xoff -= in_prev; doff -= in_w;
        }
        grad_wave_sync();

        // ---- phase B: every lane its parameters, the tile's samples starting at the lane's own
#pragma unroll 1
        for (unsigned m = 0; m < 64u; ++m) {
            const unsigned s = (lane + m) & 63u;
#pragma unroll
            for (int kb = 0; kb < kGradSlots; kb += 4) {
                if (kb < n_slots) {                             // wave-uniform
#pragma unroll
                    for (int k = kb; k < kb + 4; ++k)
                        acc[k] = fma(blk[(rows[k] >> 16) + s], blk[(rows[k] & 0xffffu) + s], acc[k]);
                }
            }
        }
        grad_wave_sync();                                       // the next tile overwrites what was just read
    }
    if (with_grad) {
        T* const out = g.partial + (size_t)wave * (size_t)c.n_params;
#pragma unroll
        for (int k = 0; k < kGradSlots; ++k) {
            const unsigned q = (unsigned)k * 64u + lane;
            if (k < n_slots && q < (unsigned)c.n_params) out[q] = acc[k];
        }
    }
    if constexpr (KIND != 0) {
        const auto& ls = loss_first(lp...);
        if (ls.stat_partial) {                                   // kernel argument: wave-uniform
            // lane l += lane l + d for l < d, as gae_moments_kernel folds: a shuffle goes through the LDS crossbar without
            // taking LDS space, which a y-only call of a small net does not have.  Lanes >= d add words that are no
            // longer part of the sum (or their own); they never feed lane 0, and only lane 0 is stored.
#pragma unroll
            for (int k = 0; k < 4; ++k) {
#pragma unroll
                for (int d = 32; d >= 1; d >>= 1) st[k] += __shfl_down(st[k], d, 64);
            }
            if (lane == 0) {
                double* const out = ls.stat_partial + 4 * (size_t)wave;
                out[0] = st[0]; out[1] = st[1]; out[2] = st[2]; out[3] = st[3];
            }
        }
    }
}

// grad[p][q] = partial[p][0][q] + partial[p][1][q] + ... in that order; one lane per parameter
template <typename T>
__global__ __launch_bounds__(256) void mlp_grad_sum_kernel(const T* partial, T* grad, unsigned waves_per_policy, unsigned n_params, unsigned total)
{
    const unsigned e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= total) return;
    const unsigned p = e / n_params, q = e - p * n_params;
    const T* src = partial + (size_t)p * waves_per_policy * n_params + q;
    T sum = T(0);
    for (unsigned k = 0; k < waves_per_policy; ++k) sum += src[(size_t)k * n_params];
    grad[e] = sum;
}

// stats[p][k] = partial[p][0][k] + partial[p][1][k] + ... in that order; one lane per word
__global__ __launch_bounds__(64) void mlp_loss_stats_kernel(const double* partial, double* stats, unsigned waves_per_policy, unsigned total)
{
    const unsigned e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= total) return;
    const unsigned p = e >> 2, k = e & 3u;
    const double* src = partial + 4 * (size_t)p * waves_per_policy + k;
    double sum = 0.0;
    for (unsigned j = 0; j < waves_per_policy; ++j) sum += src[4 * (size_t)j];
    stats[e] = sum;
}

} // namespace t1d
