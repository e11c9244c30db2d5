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
    unsigned tiles;                       // chunks * n_rows: tiles of one policy
    unsigned tiles_per_wave, waves_per_policy, n_waves;
    int act_rows;                         // A: F + the hidden widths
};

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

// Dynamic LDS: (act_rows + 1 + the sum of all widths) * 64 words.  Grid: n_waves workgroups of 64 threads.
template <typename T>
__global__ __launch_bounds__(64) void mlp_grad_kernel(const MlpArgs<T> c, const GradArgs<T> g)
{
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

#pragma unroll 1
    for (unsigned u = t0; u < t1; ++u) {
        const unsigned row = u / g.chunks, chunk = u - row * g.chunks;
        const int64_t i = (int64_t)pol * c.envs_per_policy + (int64_t)chunk * 64 + lane;
        const T* const f = g.feat + (int64_t)row * F * g.n + i;
        for (int j = 0; j < F; ++j) col[j * 64] = f[(int64_t)j * g.n];
        const T y = mlp_layers<T, true>(c, w, col, F);
        if (g.y) g.y[(int64_t)row * g.n + i] = y;
        if (!with_grad) continue;

        // ---- phase A, backwards: delta of layer l's outputs -> delta of layer l - 1's outputs (= layer l's inputs)
        col[d_last * 64] = g.coef[(int64_t)row * g.n + i];
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

} // namespace t1d
