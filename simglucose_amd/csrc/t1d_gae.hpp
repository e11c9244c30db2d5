// t1d_gae.hpp -- advantages, value targets and per-policy advantage moments from (reward, done, value) (gfx950 only):
// t1d_gae of include/t1d.h.  Included by t1d_abi.hip; needs nothing of the simulator.
//
//   gae_kernel           one lane per env, the K rows walked from the last to the first.  Every load and store of a wave is 64
//                        consecutive words of one row.  The scan is a pure stream (fp64: 17 bytes read and 16 written per
//                        sample) with three dependent operations per row, so what matters is how many loads a wave has in
//                        flight: the rows are taken in groups of kGaeRows.  FULL (reward, done, value, adv and ret all
//                        given: what a trainer calls) is the streaming form: the K mod kGaeRows top rows go first, then the
//                        whole groups with every load and store unconditional, so that the compiler can count them -- the
//                        loads of group g + 1 are issued before group g is computed, into the other of two register
//                        buffers (the loop is unrolled by two, so no group is copied), and group g waits with the 24 loads
//                        of group g + 1 still outstanding (s_waitcnt vmcnt(24) or more in the loop, never vmcnt(0): checked
//                        in the ISA); the last one or two groups are computed behind the loop.  With a NULL array the same rows are taken one group
//                        at a time under wave-uniform branches, which the wait counter cannot see through.
//                        No LDS, no barrier.  value[s + 1] and adv[s + 1] of the recurrence stay in registers.
//   gae_limit_kernel     t1d_gae_limit: gae_kernel with the truncation mask of a batch collected under a time limit -- one more
//                        byte per sample, selected in gae_rows beside done -- and the lane's cut_value.
//   moments              every lane adds adv and adv^2 of its rows in double, in scan order.  The order of everything after
//                        that is stated relative to the policy, so that a policy's sums do not depend on where its envs
//                        sit in the batch: with moments a wave takes one tile -- the envs 64 c .. 64 c + 63 of one policy,
//                        counted from the policy's first env (E need not be a multiple of 64: a policy's last tile is
//                        short, and its lanes past the end idle; with E a multiple of 64 this is the plain mapping).  The
//                        wave adds its lanes' pairs in ascending order (v_readlane: the word of lane j in a scalar
//                        register, every lane forms the same sum) and stores one partial [2] per tile.  No atomics.
//   gae_moments_kernel   one wave per policy: lane l adds the policy's partials l, l + 64, .. in ascending order, then the 64
//                        lane sums are folded 32, 16, .. 1 lanes down.
// Nothing depends on the grid the hardware happens to run: two calls give the same bits.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace t1d {

constexpr int kGaeBlock = 256;            // 4 waves: no LDS and no barrier tie them together, the size only spares the dispatcher
#ifndef T1D_GAE_ROWS
#define T1D_GAE_ROWS 8                    // A/B builds only (profiles/policy/README.md)
#endif
constexpr int kGaeRows = T1D_GAE_ROWS;    // rows per group; two groups of loads in flight

template <typename T> struct GaeArgs {
    const T* reward; const uint8_t* done; const T* value; const T* last_value;
    T* adv; T* ret;
    double* partial;                      // [n_policies][tiles][2], null = no moments
    int64_t n, n_rows, envs_per_policy;
    unsigned tiles;                       // ceil(envs_per_policy / 64): tiles, and partials, of one policy
    unsigned n_waves;                     // waves with work: ceil(n / 64), with moments n_policies * tiles
    T g, gl;                              // (T) gamma, (T) (gamma * lambda)
};

// t1d_gae_limit: the second mask and the value of the state each cut episode ended in.  GaeNoCut: t1d_gae, which has neither
template <typename T> struct GaeCutArgs { const uint8_t* truncated; const T* cut_value; };      // [K][n]; [n] or null = 0
struct GaeNoCut {};
template <typename C> constexpr bool kGaeCut = !__is_same(C, GaeNoCut);

template <typename T, bool CUT = false> struct GaeGroup { T r[kGaeRows]; T v[kGaeRows]; uint8_t d[kGaeRows]; };
template <typename T> struct GaeGroup<T, true> { T r[kGaeRows]; T v[kGaeRows]; uint8_t d[kGaeRows]; uint8_t c[kGaeRows]; };    // c: truncated
template <typename T> struct GaeState { T vn, an; double sum, sq; };

// rows top, top - 1, .. of env i, every load issued before anything is used.  FULL: all kGaeRows rows, nothing asked;
// else the first `rows` of them, and a NULL value or done reads as 0
template <typename T, bool FULL, typename C>
__device__ __forceinline__ void gae_load(const GaeArgs<T>& a, const C& cut, int64_t i, int64_t top, int rows, GaeGroup<T, kGaeCut<C>>& q)
{
#pragma unroll
    for (int k = 0; k < kGaeRows; ++k) {
        const int64_t at = (top - k) * a.n + i;
        if constexpr (FULL) {
            q.r[k] = a.reward[at]; q.v[k] = a.value[at]; q.d[k] = a.done[at];
            if constexpr (kGaeCut<C>) q.c[k] = cut.truncated[at];
        } else {
            q.r[k] = T(0); q.v[k] = T(0); q.d[k] = 0;
            if constexpr (kGaeCut<C>) q.c[k] = 0;
            if (k < rows) {                                     // wave-uniform
                q.r[k] = a.reward[at];
                if (a.value) q.v[k] = a.value[at];
                if (a.done) q.d[k] = a.done[at];
                if constexpr (kGaeCut<C>) q.c[k] = cut.truncated[at];
            }
        }
    }
}

// the recurrence over the rows of a loaded group (include/t1d.h), and the lane's two running sums.  CUT: cv is the lane's
// cut_value, selected (never multiplied) where the row was truncated and not done
template <typename T, bool MOMENTS, bool FULL, bool CUT>
__device__ __forceinline__ void gae_rows(const GaeArgs<T>& a, int64_t i, int64_t top, int rows, bool live_lane, const GaeGroup<T, CUT>& q,
                                         GaeState<T>& st, T cv)
{
#pragma unroll
    for (int k = 0; k < kGaeRows; ++k) {
        if (FULL || k < rows) {                                 // wave-uniform
            const int64_t at = (top - k) * a.n + i;
            const bool live = q.d[k] == 0;
            T v1 = live ? st.vn : T(0);                         // selected: a NaN behind a done goes nowhere
            T a1 = live ? st.an : T(0);
            if constexpr (CUT) {
                const bool trunc = live && q.c[k] != 0;         // done wins
                v1 = trunc ? cv : v1;
                a1 = trunc ? T(0) : a1;
            }
            const T delta = __builtin_fma(a.g, v1, q.r[k]) - q.v[k];
            st.an = __builtin_fma(a.gl, a1, delta);
            st.vn = q.v[k];
            if (live_lane) {
                if (FULL || a.adv) a.adv[at] = st.an;
                if (FULL || a.ret) a.ret[at] = st.an + st.vn;
            }
            if constexpr (MOMENTS) { const double x = (double)st.an; st.sum += x; st.sq = __builtin_fma(x, x, st.sq); }
        }
    }
}

// Grid: ceil(n_waves / 4) workgroups of kGaeBlock threads.  FULL: reward, done, value, adv and ret are all given.
template <typename T, bool MOMENTS, bool FULL>
__global__ __launch_bounds__(kGaeBlock) void gae_kernel(const GaeArgs<T> a)
{
    constexpr bool CUT = false;
    const GaeNoCut cut;
    const unsigned lane = threadIdx.x & 63u;
    const unsigned wave = __builtin_amdgcn_readfirstlane(blockIdx.x * (kGaeBlock / 64) + (threadIdx.x >> 6));
    if (wave >= a.n_waves) return;                              // wave-uniform
    // the wave's first env and how many envs it has
    int64_t first = (int64_t)wave * 64, count = a.n - first;
    if constexpr (MOMENTS) {
        const unsigned pol = wave / a.tiles, tile = wave - pol * a.tiles;
        first = (int64_t)pol * a.envs_per_policy + (int64_t)tile * 64;
        count = a.envs_per_policy - (int64_t)tile * 64;
    }
    const int live_lanes = count < 64 ? (int)count : 64;        // >= 1
    const bool live_lane = (int)lane < live_lanes;
    const int64_t i = first + (live_lane ? lane : 0);           // lanes past the end repeat the first env and store nothing
    // vn: V of the state after the row at hand; an: adv of the row after the row at hand
    GaeState<T> st{a.last_value ? a.last_value[i] : T(0), T(0), 0.0, 0.0};
    const T cv = T(0);                                          // no cut: never read
    GaeGroup<T, CUT> cur;
    int64_t top = a.n_rows - 1;
    if constexpr (FULL) {
        const int rem = (int)(a.n_rows % kGaeRows);
        if (rem) {
            gae_load<T, false>(a, cut, i, top, rem, cur);
            gae_rows<T, MOMENTS, false, CUT>(a, i, top, rem, live_lane, cur, st, cv);
            top -= rem;
        }
        if (top >= 0) {                                         // whole groups: top + 1 is a multiple of kGaeRows
            // two buffers taken in turn, the loop unrolled by two so that no group is ever copied: a copy would wait for
            // the loads it moves
            GaeGroup<T, CUT> alt;
            gae_load<T, true>(a, cut, i, top, kGaeRows, cur);
#pragma unroll 1
            for (; top >= 2 * kGaeRows; top -= 2 * kGaeRows) {
                gae_load<T, true>(a, cut, i, top - kGaeRows, kGaeRows, alt);
                gae_rows<T, MOMENTS, true, CUT>(a, i, top, kGaeRows, live_lane, cur, st, cv);
                gae_load<T, true>(a, cut, i, top - 2 * kGaeRows, kGaeRows, cur);
                gae_rows<T, MOMENTS, true, CUT>(a, i, top - kGaeRows, kGaeRows, live_lane, alt, st, cv);
            }
            if (top >= kGaeRows) {                              // two groups left, the upper one loaded
                gae_load<T, true>(a, cut, i, top - kGaeRows, kGaeRows, alt);
                gae_rows<T, MOMENTS, true, CUT>(a, i, top, kGaeRows, live_lane, cur, st, cv);
                gae_rows<T, MOMENTS, true, CUT>(a, i, top - kGaeRows, kGaeRows, live_lane, alt, st, cv);
            } else {
                gae_rows<T, MOMENTS, true, CUT>(a, i, top, kGaeRows, live_lane, cur, st, cv);
            }
        }
    } else {
#pragma unroll 1
        for (; top >= 0; top -= kGaeRows) {
            const int rows = top + 1 < kGaeRows ? (int)(top + 1) : kGaeRows;
            gae_load<T, false>(a, cut, i, top, rows, cur);
            gae_rows<T, MOMENTS, false, CUT>(a, i, top, rows, live_lane, cur, st, cv);
        }
    }
    if constexpr (MOMENTS) {
        const unsigned s_lo = (unsigned)__double_as_longlong(st.sum), s_hi = (unsigned)(__double_as_longlong(st.sum) >> 32);
        const unsigned q_lo = (unsigned)__double_as_longlong(st.sq), q_hi = (unsigned)(__double_as_longlong(st.sq) >> 32);
        double s_acc = 0.0, q_acc = 0.0;
#pragma unroll
        for (int j = 0; j < 64; ++j) {
            if (j < live_lanes) {                               // wave-uniform
                const unsigned long long sb = (unsigned long long)(unsigned)__builtin_amdgcn_readlane((int)s_lo, j)
                                              | (unsigned long long)(unsigned)__builtin_amdgcn_readlane((int)s_hi, j) << 32;
                const unsigned long long qb = (unsigned long long)(unsigned)__builtin_amdgcn_readlane((int)q_lo, j)
                                              | (unsigned long long)(unsigned)__builtin_amdgcn_readlane((int)q_hi, j) << 32;
                s_acc += __longlong_as_double((long long)sb);
                q_acc += __longlong_as_double((long long)qb);
            }
        }
        if (lane == 0) { a.partial[2 * (size_t)wave] = s_acc; a.partial[2 * (size_t)wave + 1] = q_acc; }
    }
}


// gae_kernel with the truncation mask (t1d_gae_limit): the same scan with one more byte per sample in every group of loads -- 32
// outstanding in the FULL form's loop instead of 24 -- and the lane's cut_value in one more register.  A kernel of its own name
// and not a further template argument of gae_kernel, so that the uncut instances keep their symbols (tools/isa_diff.py compares
// by symbol); and its own copy of the kernel's lines, not a function both call: behind a call, even an inlined one, the uncut
// instances came out with other instructions.  Change one, change the other: with an all-zero mask the two give the same
// bits (tests/test_gpu_time_limit.py).
template <typename T, bool MOMENTS, bool FULL>
__global__ __launch_bounds__(kGaeBlock) void gae_limit_kernel(const GaeArgs<T> a, const GaeCutArgs<T> cut)
{
    constexpr bool CUT = true;
    const unsigned lane = threadIdx.x & 63u;
    const unsigned wave = __builtin_amdgcn_readfirstlane(blockIdx.x * (kGaeBlock / 64) + (threadIdx.x >> 6));
    if (wave >= a.n_waves) return;                              // wave-uniform
    // the wave's first env and how many envs it has
    int64_t first = (int64_t)wave * 64, count = a.n - first;
    if constexpr (MOMENTS) {
        const unsigned pol = wave / a.tiles, tile = wave - pol * a.tiles;
        first = (int64_t)pol * a.envs_per_policy + (int64_t)tile * 64;
        count = a.envs_per_policy - (int64_t)tile * 64;
    }
    const int live_lanes = count < 64 ? (int)count : 64;        // >= 1
    const bool live_lane = (int)lane < live_lanes;
    const int64_t i = first + (live_lane ? lane : 0);           // lanes past the end repeat the first env and store nothing
    // vn: V of the state after the row at hand; an: adv of the row after the row at hand
    GaeState<T> st{a.last_value ? a.last_value[i] : T(0), T(0), 0.0, 0.0};
    const T cv = cut.cut_value ? cut.cut_value[i] : T(0);
    GaeGroup<T, CUT> cur;
    int64_t top = a.n_rows - 1;
    if constexpr (FULL) {
        const int rem = (int)(a.n_rows % kGaeRows);
        if (rem) {
            gae_load<T, false>(a, cut, i, top, rem, cur);
            gae_rows<T, MOMENTS, false, CUT>(a, i, top, rem, live_lane, cur, st, cv);
            top -= rem;
        }
        if (top >= 0) {                                         // whole groups: top + 1 is a multiple of kGaeRows
            // two buffers taken in turn, the loop unrolled by two so that no group is ever copied: a copy would wait for
            // the loads it moves
            GaeGroup<T, CUT> alt;
            gae_load<T, true>(a, cut, i, top, kGaeRows, cur);
#pragma unroll 1
            for (; top >= 2 * kGaeRows; top -= 2 * kGaeRows) {
                gae_load<T, true>(a, cut, i, top - kGaeRows, kGaeRows, alt);
                gae_rows<T, MOMENTS, true, CUT>(a, i, top, kGaeRows, live_lane, cur, st, cv);
                gae_load<T, true>(a, cut, i, top - 2 * kGaeRows, kGaeRows, cur);
                gae_rows<T, MOMENTS, true, CUT>(a, i, top - kGaeRows, kGaeRows, live_lane, alt, st, cv);
            }
            if (top >= kGaeRows) {                              // two groups left, the upper one loaded
                gae_load<T, true>(a, cut, i, top - kGaeRows, kGaeRows, alt);
                gae_rows<T, MOMENTS, true, CUT>(a, i, top, kGaeRows, live_lane, cur, st, cv);
                gae_rows<T, MOMENTS, true, CUT>(a, i, top - kGaeRows, kGaeRows, live_lane, alt, st, cv);
            } else {
                gae_rows<T, MOMENTS, true, CUT>(a, i, top, kGaeRows, live_lane, cur, st, cv);
            }
        }
    } else {
#pragma unroll 1
        for (; top >= 0; top -= kGaeRows) {
            const int rows = top + 1 < kGaeRows ? (int)(top + 1) : kGaeRows;
            gae_load<T, false>(a, cut, i, top, rows, cur);
            gae_rows<T, MOMENTS, false, CUT>(a, i, top, rows, live_lane, cur, st, cv);
        }
    }
    if constexpr (MOMENTS) {
        const unsigned s_lo = (unsigned)__double_as_longlong(st.sum), s_hi = (unsigned)(__double_as_longlong(st.sum) >> 32);
        const unsigned q_lo = (unsigned)__double_as_longlong(st.sq), q_hi = (unsigned)(__double_as_longlong(st.sq) >> 32);
        double s_acc = 0.0, q_acc = 0.0;
#pragma unroll
        for (int j = 0; j < 64; ++j) {
            if (j < live_lanes) {                               // wave-uniform
                const unsigned long long sb = (unsigned long long)(unsigned)__builtin_amdgcn_readlane((int)s_lo, j)
                                              | (unsigned long long)(unsigned)__builtin_amdgcn_readlane((int)s_hi, j) << 32;
                const unsigned long long qb = (unsigned long long)(unsigned)__builtin_amdgcn_readlane((int)q_lo, j)
                                              | (unsigned long long)(unsigned)__builtin_amdgcn_readlane((int)q_hi, j) << 32;
                s_acc += __longlong_as_double((long long)sb);
                q_acc += __longlong_as_double((long long)qb);
            }
        }
        if (lane == 0) { a.partial[2 * (size_t)wave] = s_acc; a.partial[2 * (size_t)wave + 1] = q_acc; }
    }
}


// moments[p] = (sum of adv, sum of adv^2) of policy p from its partials.  Grid: n_policies workgroups of 64 threads.  A lane's
// partials are loaded kGaeFold at a time before they are added, in their order: one wave has a whole policy, and only loads in
// flight hide the latency.
constexpr int kGaeFold = 16;
__global__ __launch_bounds__(64) void gae_moments_kernel(const double* partial, double* moments, unsigned tiles)
{
    const double* const src = partial + 2 * (size_t)blockIdx.x * tiles;
    double s = 0.0, q = 0.0;
    for (unsigned base = threadIdx.x; base < tiles; base += 64u * kGaeFold) {
        double vs[kGaeFold], vq[kGaeFold];                      // two 8-byte loads: the workspace need not be 16-byte aligned
#pragma unroll
        for (int u = 0; u < kGaeFold; ++u) {
            const size_t k = base + 64u * u < tiles ? base + 64u * u : base;
            vs[u] = src[2 * k]; vq[u] = src[2 * k + 1];
        }
#pragma unroll
        for (int u = 0; u < kGaeFold; ++u) {
            const bool in = base + 64u * u < tiles;
            s = in ? s + vs[u] : s;
            q = in ? q + vq[u] : q;
        }
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) { s += __shfl_down(s, d, 64); q += __shfl_down(q, d, 64); }
    if (threadIdx.x == 0) { moments[2 * (size_t)blockIdx.x] = s; moments[2 * (size_t)blockIdx.x + 1] = q; }
}

} // namespace t1d
