// t1d_abi.hip -- host side of the C ABI of libt1d_hip.so (gfx950 only; see include/t1d.h): context and tables, argument
// checks, kernel selection and launches.  A step or a roll-out is planned by plan_call (which kernel instance, grid,
// block, dynamic LDS) and launched by launch_plan.  The kernels that run the policy network (t1d_policy.hpp,
// t1d_dopri5.hpp) get their workgroup and dynamic LDS from launch_shape, through one line of constants per family
// (shape_mlp, shape_mlp_dopri5, shape_mlp_alone); the gradient kernel's LDS is counted by grad_wave_lds.  All of these
// are pure functions, checked on the CPU by tests/dispatch_plan_driver.cpp.  Each argument struct of a kernel has one
// builder (make_*), each group of entry-point checks one function (check_*); by_dtype and by_variant pick the template
// instance.  The kernels are in t1d_kernels.hpp, the per-lane arithmetic in t1d_device.hpp.  This is the one
// translation unit of the library.
#include "../../include/t1d.h"
#include "t1d_kernels.hpp"
#include "t1d_dopri5.hpp"
#include "t1d_policy.hpp"
#include "t1d_policy_grad.hpp"
#include "t1d_gae.hpp"

#include <climits>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <new>
#include <string>
#include <type_traits>
#include <vector>

// =============================================================================================
// host side
// =============================================================================================
using namespace t1d;

struct t1d_ctx {
    int device = -1;
    int np = 0, S = 0;
    double sensor[T1D_SENSOR_NCOLS];
    double pump[T1D_PUMP_NCOLS];
    double* d_par64 = nullptr; float* d_par32 = nullptr;
    double* d_raw64 = nullptr;   // [kRawPars][kMaxPatients] the caller's model columns as they are (t1d_step_dopri5)
    double* d_x0 = nullptr;
    double* d_minv64 = nullptr; float* d_minv32 = nullptr;
    int* d_status = nullptr;
    MealSlots* d_slots = nullptr;    // meal_slots() on the device, for kernels that restart an env themselves (t1d_collect_mlp)
    int math = 1;            // RHS arithmetic variant (t1d_ctx_set_option "math")
    int n_cu = 256;
    int lds_per_block = 65536;   // hipDeviceAttributeMaxSharedMemoryPerBlock (160 KiB on gfx950)
    std::vector<std::pair<const void*, size_t>> lds_allowed;   // kernels whose dynamic-LDS ceiling has been raised above 64 KiB, and to what
    int s1_blocks = 0;       // > 0: grid of the single-minute kernels (tests exercise many chunks per block)
    int split_refill = 1;    // 1 = noise-block refills run in their own kernel ahead of a refill-free step kernel
    int adaptive_gut = 1;    // 1 (default) = the split integrator picks its step sizes per minute and env; 0 = level 1 everywhere
    int single_minute_kernel = 1;   // 1 = minutes == 1 launches of the split integrator use the persistent early-store kernels
    int integrator = -1;     // 0 = classical RK4 on all 13 states, 1 = split scheme, -1 = split whenever n_sub allows it
    int split_nsub = 0;      // n_sub the split tables on the device were built for (0 = none yet)
    int np_pad = 0;
    double* d_prop64 = nullptr; float* d_prop32 = nullptr;   // [kPropRows(split_nsub)][np_pad]
    // both tables as the persistent kernels keep them in LDS at row stride 32, the pump and sensor limits behind them
    // (s1_stage_image); rebuilt with the tables, by ensure_split alone; null for more than 32 patients
    double* d_img64 = nullptr; float* d_img32 = nullptr;
    long long* d_trace = nullptr;    // T1D_S1_TRACE builds
    int defer_min_chunks = 1;        // adaptive_gut = 1: one-minute launches set lanes of level 2 aside from this many chunks per CU up
    int multi_minute_kernel = 1;     // steps of several minutes (minutes <= sample_time) on the packed layout through the persistent kernel with the state in registers across the minutes: 0 never (generic kernel), 1 = fp64 batches of multi_minute_min_envs envs or more, 2 always
    int multi_minute_min_envs = 262144, multi_minute_min_envs_f32 = 393216;      // measured crossovers: tools/mm_thresholds.py
    int park_cap = 0;                // records for set-aside lanes per workgroup of that kernel (0 = what fits in LDS; tests force the overflow path with a small one)
    int pingpong = 1;                // the persistent one-minute kernels walk a CU's chunks backwards in every other launch (below)
    mutable unsigned launches = 0;   // one-minute launches so far
    int record_group_min = 64;       // the multi-minute kernel: that many waiting records go ahead of a wave's next chunk
    int rollout_launches = 1;        // closed-loop roll-outs as one launch of that kernel per step: 0 never (all steps inside one launch of the generic kernel), 1 from rollout_launches_min_envs envs up, 2 always
    int rollout_launches_min_envs = 524288, rollout_launches_min_envs_f32 = 786432;
    int restart_compact = 1;         // t1d_restart_done: 1 = a workgroup collects the finished envs of 4 096 in LDS and restarts them with full waves; 0 = every lane its own env
    std::vector<double> ptab;    // the caller's table, kept for rebuilding the split tables
    std::vector<double> dpar;    // host copy of the derived-parameter table
};

static MealSlots meal_slots();
static thread_local std::string g_err;
static int fail(int code, const std::string& msg) { g_err = msg; return code; }
#define T1D_HIP(call)                                                                         \
    do {                                                                                      \
        hipError_t _e = (call);                                                               \
        if (_e != hipSuccess)                                                                 \
            return fail(T1D_E_HIP, std::string(#call) + ": " + hipGetErrorString(_e));        \
    } while (0)

// Minv [11][11] with M = Minv . y: second derivatives at the knots of the not-a-knot cubic spline
// through 11 points at 15-minute spacing -- what scipy's interp1d(kind='cubic') builds in
// noise_gen.py:45.  Interior rows: M[k-1] + 4 M[k] + M[k+1] = 6 (y[k-1] - 2 y[k] + y[k+1]) / h^2; the two
// not-a-knot rows make the third derivative continuous at the first and last interior knots.
static std::vector<double> spline_second_derivative_operator()
{
    const int K = 11;
    const double h = 15.0;
    std::vector<double> A(K * K, 0.0), B(K * K, 0.0);
    for (int k = 1; k < K - 1; ++k) {
        A[k * K + k - 1] = 1.0; A[k * K + k] = 4.0; A[k * K + k + 1] = 1.0;
        B[k * K + k - 1] = 6.0 / (h * h); B[k * K + k] = -12.0 / (h * h); B[k * K + k + 1] = 6.0 / (h * h);
    }
    A[0] = 1.0; A[1] = -2.0; A[2] = 1.0;
    A[(K - 1) * K + K - 3] = 1.0; A[(K - 1) * K + K - 2] = -2.0; A[(K - 1) * K + K - 1] = 1.0;
    // Gauss-Jordan with partial pivoting on [A | B]
    for (int c = 0; c < K; ++c) {
        int piv = c;
        for (int r = c + 1; r < K; ++r) if (std::fabs(A[r * K + c]) > std::fabs(A[piv * K + c])) piv = r;
        if (piv != c) for (int j = 0; j < K; ++j) { std::swap(A[c * K + j], A[piv * K + j]); std::swap(B[c * K + j], B[piv * K + j]); }
        const double d = A[c * K + c];
        for (int j = 0; j < K; ++j) { A[c * K + j] /= d; B[c * K + j] /= d; }
        for (int r = 0; r < K; ++r) {
            if (r == c) continue;
            const double f = A[r * K + c];
            if (f == 0.0) continue;
            for (int j = 0; j < K; ++j) { A[r * K + j] -= f * A[c * K + j]; B[r * K + j] -= f * B[c * K + j]; }
        }
    }
    return B;
}


// ---- host tables of the split integrator ------------------------------------------------------------
// exp(A) for a small dense matrix: scaling and squaring with a degree-16 Taylor polynomial
static void mat_expm(int n, const double* A, double* E)
{
    double nrm = 0.0;
    for (int i = 0; i < n; ++i) { double r = 0.0; for (int j = 0; j < n; ++j) r += std::fabs(A[i * n + j]); nrm = std::max(nrm, r); }
    int sq = 0;
    while (nrm > 0.03125 && sq < 60) { nrm *= 0.5; ++sq; }
    const double sc = std::ldexp(1.0, -sq);
    std::vector<double> B(n * n), term(n * n, 0.0), tmp(n * n);
    for (int k = 0; k < n * n; ++k) B[k] = A[k] * sc;
    for (int i = 0; i < n; ++i) { for (int j = 0; j < n; ++j) E[i * n + j] = (i == j); term[i * n + i] = 1.0; }
    for (int d = 1; d <= 16; ++d) {
        for (int i = 0; i < n; ++i)
            for (int j = 0; j < n; ++j) {
                double v = 0.0;
                for (int k = 0; k < n; ++k) v += term[i * n + k] * B[k * n + j];
                tmp[i * n + j] = v / (double)d;
            }
        term = tmp;
        for (int k = 0; k < n * n; ++k) E[k] += term[k];
    }
    for (int q = 0; q < sq; ++q) {
        for (int i = 0; i < n; ++i)
            for (int j = 0; j < n; ++j) {
                double v = 0.0;
                for (int k = 0; k < n; ++k) v += E[i * n + k] * E[k * n + j];
                tmp[i * n + j] = v;
            }
        for (int k = 0; k < n * n; ++k) E[k] = tmp[k];
    }
}

// One patient row -> kPropRows(n_sub) propagator entries (layout: t1d_device.hpp) followed by the four x2 weights
// E, wa, wm, wb for the gut step of level 1 (h = 1/n_sub) and of level 2 (h/2).  The insulin
// sub-system in the order s = (x5, x9, x10, x11, x6, x7, x8, u, 1) (t1dpatient.py:176-198); weights of
// x2' = -kabs x2 + F (:148) from the moments I_k = int_0^1 exp(-z (1 - s)) s^k ds = sum_j (-z)^j k! / (k + j + 1)!,
// z = kabs h, of the quadratic through F(0), F(h/2), F(h).
static void split_tables_row(const double* r, int n_sub, double* out)
{
    double A[81] = {0.0};
    auto at = [&](int i, int j) -> double& { return A[i * 9 + j]; };
    at(0, 0) = -(r[T1D_P_M2] + r[T1D_P_M4]); at(0, 1) = r[T1D_P_M1]; at(0, 2) = r[T1D_P_KA1]; at(0, 3) = r[T1D_P_KA2];
    at(1, 1) = -(r[T1D_P_M1] + r[T1D_P_M30]); at(1, 0) = r[T1D_P_M2];
    at(2, 2) = -(r[T1D_P_KA1] + r[T1D_P_KD]); at(2, 7) = 1.0;
    at(3, 2) = r[T1D_P_KD]; at(3, 3) = -r[T1D_P_KA2];
    at(4, 4) = -r[T1D_P_P2U]; at(4, 0) = r[T1D_P_P2U] / r[T1D_P_VI]; at(4, 8) = -r[T1D_P_P2U] * r[T1D_P_IB];
    at(5, 5) = -r[T1D_P_KI]; at(5, 0) = r[T1D_P_KI] / r[T1D_P_VI];
    at(6, 6) = -r[T1D_P_KI]; at(6, 5) = r[T1D_P_KI];
    double Ah[81], Ph[81], Pk[81], tmp[81];
    const int nb = 2 * n_sub;                            // blocks: tau = k / nb
    const double hb = 1.0 / (double)nb;
    for (int k = 0; k < 81; ++k) Ah[k] = A[k] * hb;
    mat_expm(9, Ah, Ph);
    std::memcpy(Pk, Ph, sizeof(Pk));
    static const int c6[7] = {4, 0, 1, 2, 3, 7, 8};      // x6 <- x6, x5, x9, x10, x11, u, 1
    static const int c8[7] = {6, 5, 0, 1, 2, 3, 7};      // x8 <- x8, x7, x5, x9, x10, x11, u
    for (int k = 1; k <= nb; ++k) {
        double* o = out + (k - 1) * 14;
        for (int j = 0; j < 7; ++j) { o[j] = Pk[4 * 9 + c6[j]]; o[7 + j] = Pk[6 * 9 + c8[j]]; }
        if (k == nb) break;
        for (int i = 0; i < 9; ++i)
            for (int j = 0; j < 9; ++j) {
                double v = 0.0;
                for (int q = 0; q < 9; ++q) v += Ph[i * 9 + q] * Pk[q * 9 + j];
                tmp[i * 9 + j] = v;
            }
        std::memcpy(Pk, tmp, sizeof(Pk));
    }
    double* t = out + 14 * nb;                           // tail: Phi(1)
    static const int c5[5] = {0, 1, 2, 3, 7};
    for (int j = 0; j < 5; ++j) { t[j] = Pk[0 * 9 + c5[j]]; t[5 + j] = Pk[1 * 9 + c5[j]]; }
    t[10] = Pk[2 * 9 + 2]; t[11] = Pk[2 * 9 + 7];
    t[12] = Pk[3 * 9 + 2]; t[13] = Pk[3 * 9 + 3]; t[14] = Pk[3 * 9 + 7];
    static const int c7[6] = {5, 0, 1, 2, 3, 7};
    for (int j = 0; j < 6; ++j) t[15 + j] = Pk[5 * 9 + c7[j]];
    const double h1 = 1.0 / (double)n_sub;
    const double hs[2] = {h1, 0.5 * h1};                 // gut step of level 1, 2 (the order of DP_X2E, DP_X2E2)
    for (int part = 0; part < 2; ++part) {
        const double hh = hs[part], z = r[T1D_P_KABS] * hh;
        double I[3];
        for (int k = 0; k < 3; ++k) {
            double term = 1.0, sum = 0.0;                // term = (-z)^j k! / (k + j + 1)!
            for (int q = 1; q <= k + 1; ++q) term /= (double)q;
            for (int q = 1; q <= k; ++q) term *= (double)q;
            for (int j = 0; j < 60; ++j) {
                sum += term;
                term *= -z / (double)(k + j + 2);
                if (std::fabs(term) < 1e-30) break;
            }
            I[k] = sum;
        }
        double* w = out + kPropRows(n_sub) + 4 * part;
        w[0] = std::exp(-z);
        w[1] = hh * (2.0 * I[2] - 3.0 * I[1] + I[0]);
        w[2] = hh * (-4.0 * I[2] + 4.0 * I[1]);
        w[3] = hh * (2.0 * I[2] - I[1]);
    }
}

extern "C" int t1d_split_tables(const double* patient_row, int n_cols, int n_sub, double* out, int out_len)
{
    if (!patient_row || !out) return fail(T1D_E_INVALID, "t1d_split_tables: NULL argument");
    if (n_cols != T1D_P_NCOLS) return fail(T1D_E_INVALID, "t1d_split_tables: n_cols must be T1D_P_NCOLS (45)");
    if (n_sub < 2 || n_sub > 8 || (n_sub & 1)) return fail(T1D_E_INVALID, "t1d_split_tables: n_sub must be 2, 4, 6 or 8");
    if (out_len < kPropRows(n_sub) + 8) return fail(T1D_E_INVALID, "t1d_split_tables: out_len < 28 n_sub + 29");
    split_tables_row(patient_row, n_sub, out);
    return T1D_OK;
}

// (re)build the device tables of the split integrator for n_sub sub-steps per minute
static int ensure_split(t1d_ctx* c, int ng)
{
    static_assert(DP_X2WB2 == DP_X2E + 7 && DP_X2E2 == DP_X2E + 4, "x2 weight rows are consecutive");
    if (c->split_nsub == ng) return T1D_OK;
    T1D_HIP(hipDeviceSynchronize());                     // kernels in flight may still be reading the old tables
    const int rows = kPropRows(ng), npp = c->np_pad;
    std::vector<double> prop((size_t)rows * npp, 0.0), one((size_t)rows + 8);
    for (int j = 0; j < c->np; ++j) {
        split_tables_row(c->ptab.data() + (size_t)j * T1D_P_NCOLS, ng, one.data());
        for (int k = 0; k < rows; ++k) prop[(size_t)k * npp + j] = one[k];
        for (int k = 0; k < 8; ++k) c->dpar[(size_t)(DP_X2E + k) * kMaxPatients + j] = one[rows + k];   // DP_X2E .. DP_X2WB2
    }
    std::vector<float> propf(prop.begin(), prop.end()), dpf(c->dpar.begin(), c->dpar.end());
    (void)hipFree(c->d_prop64); (void)hipFree(c->d_prop32); c->d_prop64 = nullptr; c->d_prop32 = nullptr;
    T1D_HIP(hipMalloc((void**)&c->d_prop64, prop.size() * 8));
    T1D_HIP(hipMalloc((void**)&c->d_prop32, propf.size() * 4));
    T1D_HIP(hipMemcpy(c->d_prop64, prop.data(), prop.size() * 8, hipMemcpyHostToDevice));
    T1D_HIP(hipMemcpy(c->d_prop32, propf.data(), propf.size() * 4, hipMemcpyHostToDevice));
    T1D_HIP(hipMemcpy(c->d_par64, c->dpar.data(), c->dpar.size() * 8, hipMemcpyHostToDevice));
    T1D_HIP(hipMemcpy(c->d_par32, dpf.data(), dpf.size() * 4, hipMemcpyHostToDevice));
    (void)hipFree(c->d_img64); (void)hipFree(c->d_img32); c->d_img64 = nullptr; c->d_img32 = nullptr;
    if (c->np <= 32) {
        // [DP_COUNT + rows][32]: the words the kernels would gather from dpar and prop, zero beyond np; then lconst's eight
        std::vector<double> img((size_t)(DP_COUNT + rows) * 32 + kImgConst, 0.0);
        for (int j = 0; j < c->np; ++j) {
            for (int k = 0; k < DP_COUNT; ++k) img[(size_t)k * 32 + j] = c->dpar[(size_t)k * kMaxPatients + j];
            for (int k = 0; k < rows; ++k) img[(size_t)(DP_COUNT + k) * 32 + j] = prop[(size_t)k * npp + j];
        }
        double* const lc = img.data() + (size_t)(DP_COUNT + rows) * 32;
        lc[0] = c->pump[5]; lc[1] = c->pump[3]; lc[2] = c->pump[4];      // inc_basal, min_basal, max_basal
        lc[3] = c->pump[2]; lc[4] = c->pump[0]; lc[5] = c->pump[1];      // inc_bolus, min_bolus, max_bolus
        lc[6] = c->sensor[6]; lc[7] = c->sensor[7];                      // vmin, vmax
        std::vector<float> imgf(img.begin(), img.end());
        T1D_HIP(hipMalloc((void**)&c->d_img64, img.size() * 8));
        T1D_HIP(hipMalloc((void**)&c->d_img32, imgf.size() * 4));
        T1D_HIP(hipMemcpy(c->d_img64, img.data(), img.size() * 8, hipMemcpyHostToDevice));
        T1D_HIP(hipMemcpy(c->d_img32, imgf.data(), imgf.size() * 4, hipMemcpyHostToDevice));
    }
    c->split_nsub = ng;
    return T1D_OK;
}

#if T1D_S1_TRACE
extern "C" int t1d_debug_trace(t1d_ctx* c, long long* out) { return hipMemcpy(out, c->d_trace, 128 * 4 * 64 * sizeof(long long), hipMemcpyDeviceToHost) == hipSuccess ? 0 : -1; }
#endif
extern "C" int t1d_abi_version(void) { return T1D_ABI_VERSION; }
extern "C" const char* t1d_last_error(void) { return g_err.c_str(); }

extern "C" int t1d_ctx_create(int hip_device, const double* ptab, int n_patients, int n_cols,
                              const double* sensor_row, const double* pump_row, t1d_ctx** out)
{
    try {
        if (!out) return fail(T1D_E_INVALID, "t1d_ctx_create: out is NULL");
        *out = nullptr;
        if (!ptab || !sensor_row || !pump_row) return fail(T1D_E_INVALID, "t1d_ctx_create: NULL table");
        if (n_cols != T1D_P_NCOLS) return fail(T1D_E_INVALID, "t1d_ctx_create: n_cols must be T1D_P_NCOLS (45)");
        if (n_patients < 1 || n_patients > kMaxPatients)
            return fail(T1D_E_INVALID, "t1d_ctx_create: n_patients must be in [1, 64]");
        const double st = sensor_row[5];
        if (!(st >= 1.0) || st != std::floor(st) || st > 1440.0)
            return fail(T1D_E_INVALID, "t1d_ctx_create: sensor sample_time must be a whole number of minutes >= 1");
        if (st > 150.0) return fail(T1D_E_INVALID, "t1d_ctx_create: sensor sample_time must be <= 150 minutes");
        for (int k = 2; k < 6; k += 3)
            if (!(pump_row[k] > 0.0)) return fail(T1D_E_INVALID, "t1d_ctx_create: pump increments must be > 0");
        int ndev = 0;
        if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1)
            return fail(T1D_E_NODEVICE, "t1d_ctx_create: no HIP device visible");
        if (hip_device < 0 || hip_device >= ndev) return fail(T1D_E_INVALID, "t1d_ctx_create: bad device index");
        T1D_HIP(hipSetDevice(hip_device));
        int n_cu = 0;
        T1D_HIP(hipDeviceGetAttribute(&n_cu, hipDeviceAttributeMultiprocessorCount, hip_device));

        t1d_ctx* c = new (std::nothrow) t1d_ctx();
        if (!c) return fail(T1D_E_INVALID, "t1d_ctx_create: out of host memory");
        int lds_max = 0;
        if (hipDeviceGetAttribute(&lds_max, hipDeviceAttributeMaxSharedMemoryPerBlock, hip_device) == hipSuccess && lds_max > 0) c->lds_per_block = lds_max;
        c->device = hip_device; c->n_cu = n_cu > 0 ? n_cu : 256; c->np = n_patients; c->S = (int)std::floor(150.0 / st);   // noise_gen.py:41-42
        std::memcpy(c->sensor, sensor_row, sizeof(c->sensor));
        std::memcpy(c->pump, pump_row, sizeof(c->pump));

        const int np = n_patients;
        std::vector<double> dp((size_t)DP_COUNT * kMaxPatients, 0.0), x0((size_t)13 * np);
        for (int j = 0; j < np; ++j) {
            const double* r = ptab + (size_t)j * n_cols;
            auto set = [&](int idx, double v) { dp[(size_t)idx * kMaxPatients + j] = v; };
            set(DP_KMAX, r[T1D_P_KMAX]); set(DP_KMIN, r[T1D_P_KMIN]); set(DP_KABS, r[T1D_P_KABS]);
            set(DP_HK, (r[T1D_P_KMAX] - r[T1D_P_KMIN]) / 2.0);
            set(DP_B, r[T1D_P_B]); set(DP_D, r[T1D_P_D]);
            set(DP_CAA, 5.0 / 2.0 / (1.0 - r[T1D_P_B])); set(DP_CCC, 5.0 / 2.0 / r[T1D_P_D]);
            set(DP_RATC, r[T1D_P_F] * r[T1D_P_KABS] / r[T1D_P_BW]);
            set(DP_KP1, r[T1D_P_KP1]); set(DP_KP2, r[T1D_P_KP2]); set(DP_KP3, r[T1D_P_KP3]);
            set(DP_FSNC, r[T1D_P_FSNC]); set(DP_KE1, r[T1D_P_KE1]); set(DP_KE2, r[T1D_P_KE2]);
            set(DP_K1, r[T1D_P_K1]); set(DP_K2, r[T1D_P_K2]); set(DP_VM0, r[T1D_P_VM0]);
            set(DP_VMX, r[T1D_P_VMX]); set(DP_KM0, r[T1D_P_KM0]);
            set(DP_M24, r[T1D_P_M2] + r[T1D_P_M4]); set(DP_M1, r[T1D_P_M1]);
            set(DP_KA1, r[T1D_P_KA1]); set(DP_KA2, r[T1D_P_KA2]); set(DP_VI, r[T1D_P_VI]);
            set(DP_P2U, r[T1D_P_P2U]); set(DP_IB, r[T1D_P_IB]); set(DP_KI, r[T1D_P_KI]);
            set(DP_M130, r[T1D_P_M1] + r[T1D_P_M30]); set(DP_M2, r[T1D_P_M2]);
            set(DP_KA1KD, r[T1D_P_KA1] + r[T1D_P_KD]); set(DP_KD, r[T1D_P_KD]); set(DP_KSC, r[T1D_P_KSC]);
            set(DP_INSC, 6000.0 / r[T1D_P_BW]); set(DP_VG, r[T1D_P_VG]); set(DP_IVI, 1.0 / r[T1D_P_VI]); set(DP_IVG, 1.0 / r[T1D_P_VG]);
            set(DP_DK, r[T1D_P_KMAX] - r[T1D_P_KMIN]);
            set(DP_CF, r[T1D_P_F] / r[T1D_P_BW]);
            for (int k = 0; k < 13; ++k) x0[(size_t)k * np + j] = r[T1D_P_X0 + k];
        }
        std::vector<double> raw((size_t)kRawPars * kMaxPatients, 0.0);
        for (int j = 0; j < np; ++j)
            for (int k = 0; k < kRawPars; ++k) raw[(size_t)k * kMaxPatients + j] = ptab[(size_t)j * n_cols + T1D_P_BW + k];
        c->ptab.assign(ptab, ptab + (size_t)np * n_cols);
        c->dpar = dp;
        c->np_pad = (np + 1) & ~1;
        std::vector<float> dpf(dp.begin(), dp.end());
        const std::vector<double> minv = spline_second_derivative_operator();
        std::vector<float> minvf(minv.begin(), minv.end());
        auto up = [&](void** dst, const void* src, size_t bytes) -> hipError_t {
            hipError_t e = hipMalloc(dst, bytes);
            if (e != hipSuccess) return e;
            return hipMemcpy(*dst, src, bytes, hipMemcpyHostToDevice);
        };
        hipError_t e = hipSuccess;
        if (e == hipSuccess) e = up((void**)&c->d_par64, dp.data(), dp.size() * 8);
        if (e == hipSuccess) e = up((void**)&c->d_par32, dpf.data(), dpf.size() * 4);
        if (e == hipSuccess) e = up((void**)&c->d_x0, x0.data(), x0.size() * 8);
        if (e == hipSuccess) e = up((void**)&c->d_raw64, raw.data(), raw.size() * 8);
        if (e == hipSuccess) e = up((void**)&c->d_minv64, minv.data(), minv.size() * 8);
        if (e == hipSuccess) e = up((void**)&c->d_minv32, minvf.data(), minvf.size() * 4);
#if T1D_S1_TRACE
        if (e == hipSuccess) e = hipMalloc((void**)&c->d_trace, 128 * 4 * 64 * sizeof(long long));
        if (e == hipSuccess) e = hipMemset(c->d_trace, 0, 128 * 4 * 64 * sizeof(long long));
#endif
        const MealSlots slots = meal_slots();
        if (e == hipSuccess) e = up((void**)&c->d_slots, &slots, sizeof(slots));
        if (e == hipSuccess) e = hipMalloc((void**)&c->d_status, sizeof(int));
        if (e == hipSuccess) e = hipMemset(c->d_status, 0, sizeof(int));
        if (e != hipSuccess) {
            std::string m = std::string("t1d_ctx_create: ") + hipGetErrorString(e);
            t1d_ctx_destroy(c);
            return fail(T1D_E_HIP, m);
        }
        *out = c;
        return T1D_OK;
    } catch (const std::exception& ex) {
        return fail(T1D_E_INVALID, std::string("t1d_ctx_create: ") + ex.what());
    } catch (...) {
        return fail(T1D_E_INVALID, "t1d_ctx_create: unknown exception");
    }
}

extern "C" int t1d_ctx_set_option(t1d_ctx* c, const char* name, int64_t value)
{
    if (!c || !name) return fail(T1D_E_INVALID, "t1d_ctx_set_option: NULL argument");
    struct Opt { const char* name; int t1d_ctx::*field; int64_t lo, hi; };
    static const Opt opts[] = {
        {"math", &t1d_ctx::math, 0, 1},
        {"split_refill", &t1d_ctx::split_refill, 0, 1},
        {"defer_min_chunks", &t1d_ctx::defer_min_chunks, 0, 65535},
        {"multi_minute_kernel", &t1d_ctx::multi_minute_kernel, 0, 2},
        {"multi_minute_min_envs", &t1d_ctx::multi_minute_min_envs, 0, 1 << 28},
        {"multi_minute_min_envs_f32", &t1d_ctx::multi_minute_min_envs_f32, 0, 1 << 28},
        {"park_cap", &t1d_ctx::park_cap, 0, 65535},
        {"pingpong", &t1d_ctx::pingpong, 0, 1},
        {"record_group_min", &t1d_ctx::record_group_min, 1, 64},
        {"rollout_launches", &t1d_ctx::rollout_launches, 0, 2},
        {"rollout_launches_min_envs", &t1d_ctx::rollout_launches_min_envs, 0, 1 << 28},
        {"rollout_launches_min_envs_f32", &t1d_ctx::rollout_launches_min_envs_f32, 0, 1 << 28},
        {"restart_compact", &t1d_ctx::restart_compact, 0, 1},
        {"s1_blocks", &t1d_ctx::s1_blocks, 0, 65535},
        {"adaptive_gut", &t1d_ctx::adaptive_gut, 0, 3},
        {"single_minute_kernel", &t1d_ctx::single_minute_kernel, 0, 1},
        {"integrator", &t1d_ctx::integrator, -1, 1},
    };
    for (const Opt& o : opts)
        if (std::strcmp(name, o.name) == 0) {
            if (value < o.lo || value > o.hi)
                return fail(T1D_E_INVALID, std::string("t1d_ctx_set_option: ") + name + " must be in [" + std::to_string(o.lo) + ", " + std::to_string(o.hi) + "]");
            c->*(o.field) = (int)value;
            return T1D_OK;
        }
    return fail(T1D_E_INVALID, std::string("t1d_ctx_set_option: unknown option ") + name);
}

extern "C" int t1d_ctx_destroy(t1d_ctx* c)
{
    if (!c) return T1D_OK;
    (void)hipSetDevice(c->device);
    (void)hipFree(c->d_par64); (void)hipFree(c->d_par32); (void)hipFree(c->d_x0);
    (void)hipFree(c->d_minv64); (void)hipFree(c->d_minv32); (void)hipFree(c->d_status);
    (void)hipFree(c->d_prop64); (void)hipFree(c->d_prop32); (void)hipFree(c->d_trace); (void)hipFree(c->d_raw64);
    (void)hipFree(c->d_img64); (void)hipFree(c->d_img32); (void)hipFree(c->d_slots);
    delete c;
    return T1D_OK;
}

static int check_batch(const char* who, const t1d_ctx* c, const t1d_batch* b, bool need_action)
{
    if (!c) return fail(T1D_E_INVALID, std::string(who) + ": ctx is NULL");
    if (!b) return fail(T1D_E_INVALID, std::string(who) + ": batch is NULL");
    if (b->n < 1 || b->n > (int64_t)1 << 28)
        return fail(T1D_E_INVALID, std::string(who) + ": batch.n out of range");
    if (b->dtype != T1D_F64 && b->dtype != T1D_F32) return fail(T1D_E_INVALID, std::string(who) + ": bad dtype");
    if (!b->x || !b->planned || !b->last_qsto || !b->last_food || !b->t || !b->meta || !b->last_cgm ||
        !b->ar_e || !b->pts || !b->prev_risk)
        return fail(T1D_E_INVALID, std::string(who) + ": a state pointer is NULL");
    if (!b->cgm || !b->bg || !b->reward || !b->done)
        return fail(T1D_E_INVALID, std::string(who) + ": cgm/bg/reward/done outputs are required");
    if (need_action && !b->basal) return fail(T1D_E_INVALID, std::string(who) + ": basal is NULL");
    if (b->n_meals < 0 || b->n_meals > 65535) return fail(T1D_E_INVALID, std::string(who) + ": n_meals out of range");
    if (b->n_meals > 0 && (!b->meal_time || !b->meal_amt))
        return fail(T1D_E_INVALID, std::string(who) + ": n_meals > 0 but meal table pointer is NULL");
    if (b->n_normals < 0) return fail(T1D_E_INVALID, std::string(who) + ": n_normals < 0");
    if (b->n_normals > 0 && !b->normals) return fail(T1D_E_INVALID, std::string(who) + ": n_normals > 0 but normals is NULL");
    const int known = T1D_BATCH_NO_PUMP | T1D_BATCH_NO_REFILL_DUE | (T1D_AB_FLAGS ? 0x1f00 : 0);
    if (b->flags & ~known) return fail(T1D_E_INVALID, std::string(who) + ": unknown bit in batch.flags");
    // a ctx is bound to one device: every entry point that takes one launches (and allocates) there
    if (hipSetDevice(c->device) != hipSuccess) return fail(T1D_E_HIP, std::string(who) + ": hipSetDevice failed");
    return T1D_OK;
}

template <typename T>
static KArgs<T> make_args(const t1d_ctx* c, const t1d_batch* b, int minutes, int n_sub)
{
    KArgs<T> a;
    a.n = b->n; a.env_offset = b->env_offset; a.seed = b->seed;
    a.x = (T*)b->x; a.planned = (T*)b->planned; a.last_qsto = (T*)b->last_qsto; a.last_food = (T*)b->last_food;
    a.t = b->t; a.meta = b->meta; a.episode = b->episode; a.next_meal = b->next_meal;
    a.last_cgm = (T*)b->last_cgm; a.ar_e = (T*)b->ar_e; a.pts = (T*)b->pts; a.prev_risk = (T*)b->prev_risk; a.dbar = (T*)b->dbar;
    a.basal = (const T*)b->basal; a.bolus = (const T*)b->bolus; a.cho = (const T*)b->cho;
    a.meal_time = b->meal_time; a.meal_amt = (const T*)b->meal_amt;
    a.normals = b->n_normals > 0 ? (const T*)b->normals : nullptr;
    a.x0_override = (const T*)b->x0_override;
    a.cgm = (T*)b->cgm; a.bg = (T*)b->bg; a.reward = (T*)b->reward; a.done = b->done;
    a.lbgi = (T*)b->lbgi; a.hbgi = (T*)b->hbgi; a.risk = (T*)b->risk; a.meal = (T*)b->meal; a.insulin = (T*)b->insulin; a.cgm0 = (T*)b->cgm0;
    a.dpar = sizeof(T) == 8 ? (const T*)c->d_par64 : (const T*)c->d_par32;
    a.x0tab = c->d_x0;
    a.minv = sizeof(T) == 8 ? (const T*)c->d_minv64 : (const T*)c->d_minv32;
    a.status = c->d_status; a.trace = c->d_trace;
    a.sen.pacf = (T)c->sensor[0]; a.sen.gamma = (T)c->sensor[1]; a.sen.lambda = (T)c->sensor[2];
    a.sen.delta = (T)c->sensor[3]; a.sen.xi = (T)c->sensor[4]; a.sen.st = (int)c->sensor[5];
    a.sen.vmin = (T)c->sensor[6]; a.sen.vmax = (T)c->sensor[7];
    a.pump.min_bolus = (T)c->pump[0]; a.pump.max_bolus = (T)c->pump[1]; a.pump.inc_bolus = (T)c->pump[2];
    a.pump.min_basal = (T)c->pump[3]; a.pump.max_basal = (T)c->pump[4]; a.pump.inc_basal = (T)c->pump[5];
    a.np = c->np; a.S = c->S; a.n_meals = b->n_meals; a.n_normals = b->n_normals;
    a.minutes = minutes; a.n_sub = n_sub; a.flags = b->flags | (c->pingpong && (c->launches & 1) ? kFlagReverse : 0);
    a.prop = sizeof(T) == 8 ? (const T*)c->d_prop64 : (const T*)c->d_prop32;
    a.img = sizeof(T) == 8 ? (const T*)c->d_img64 : (const T*)c->d_img32;
    a.prop_rows = c->split_nsub ? kPropRows(c->split_nsub) : 0; a.np_pad = c->np_pad;
    return a;
}

static inline dim3 grid_for(int64_t n) { return dim3((unsigned)((n + kBlock - 1) / kBlock)); }

// f(T()) with T the word of dtype: for the entry points whose two arms would differ in double / float alone
template <typename F>
static auto by_dtype(int dtype, F&& f) { return dtype == T1D_F64 ? f(double()) : f(float()); }

extern "C" int t1d_reset(t1d_ctx* c, const t1d_batch* b, const uint8_t* mask, int random_init_bg, void* stream)
{
    int rc = check_batch("t1d_reset", c, b, false);
    if (rc) return rc;
    by_dtype(b->dtype, [&](auto t) {
        using T = decltype(t);
        hipLaunchKernelGGL(reset_kernel<T>, grid_for(b->n), dim3(kBlock), 0, (hipStream_t)stream, make_args<T>(c, b, 1, 1), mask, random_init_bg);
    });
    T1D_HIP(hipGetLastError());
    return T1D_OK;
}

// more than 64 KiB of dynamic LDS has to be allowed per kernel (a context belongs to one device)
static hipError_t allow_lds(t1d_ctx* c, const void* fn, size_t bytes)
{
    if (bytes <= 65536) return hipSuccess;
    for (auto& f : c->lds_allowed)
        if (f.first == fn) {
            if (f.second >= bytes) return hipSuccess;
            hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
            if (e == hipSuccess) f.second = bytes;
            return e;
        }
    hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
    if (e == hipSuccess) c->lds_allowed.push_back({fn, bytes});
    return e;
}

// ---- kernel selection ------------------------------------------------------------------------------------------------
// Which kernel a step or a roll-out launches, with which template arguments, on what grid and with how much dynamic LDS:
// plan_call, a pure function of the context, the batch and the call (no HIP call, no change to the context; tested on
// the CPU by tests/dispatch_plan_driver.cpp).  launch_plan maps the plan to the template instance and launches it.
enum class Kern { step, rollout, step1, step1d, stepn };   // step_kernel, rollout_pid_kernel, step1_kernel, step1d_kernel, stepn_kernel

struct Plan {
    Kern kernel = Kern::step;
    bool f64 = true;
    int variant = 0;             // step_kernel, rollout_pid_kernel: VARIANT -- reference arithmetic (0), fast classical RK4 (3),
                                 // split at level 1 (4), split with per-minute step sizes in place (7 in fp64, 6 in fp32)
    bool refill = false;         // step_kernel: REFILL, the noise-block refill inside the step kernel
    int stride = 32;             // step1_kernel: STRIDE, the row stride of the tables in LDS
    bool extra = false;          // step1_kernel, step1d_kernel, stepn_kernel: EXTRA, the optional outputs
    bool tiered = false;         // step1_kernel: TIERED, per-minute step sizes
    bool ctrl = false;           // stepn_kernel: CTRL, one closed-loop roll-out step per launch, the controller in its prologue
    bool refill_ahead = false;   // refill_kernel runs ahead of the kernel (ahead of each launch of a roll-out)
    bool tables = false;         // the split integrator is asked for: its tables are (re)built for n_sub first (ensure_split)
    unsigned grid = 0, block = 0;
    size_t lds = 0;              // dynamic LDS bytes
    int nchunks = 0, cap = 0, mode = 0;   // persistent kernels: chunks of 64 envs; stepn_kernel: record capacity, mode
};

static bool is_packed(const t1d_batch* b, size_t esz)
{
    const char* xb = (const char*)b->x;
    const size_t rowb = (size_t)b->n * esz;
    return (const char*)b->planned == xb + 13 * rowb && (const char*)b->last_qsto == xb + 14 * rowb &&
           (const char*)b->last_food == xb + 15 * rowb && (const char*)b->last_cgm == xb + 16 * rowb &&
           (const char*)b->prev_risk == xb + 17 * rowb && (const char*)b->pts == xb + 18 * rowb &&
           (const char*)b->dbar == xb + (size_t)kRowDbar * rowb &&
           b->next_meal && (const char*)b->meta == (const char*)b->t + (size_t)b->n * 4 &&
           (const char*)b->next_meal == (const char*)b->t + (size_t)b->n * 8 &&
           (size_t)kPackedRows * rowb < ((size_t)1 << 32);
}

// The plan of a step (rollout = false) or of a closed-loop roll-out.  On an error *out still says whether the split tables
// are asked for (the caller builds them either way).  one_launch: a roll-out that has no launch-per-step form
// (t1d_rollout_mlp) -- all its steps in one launch of the generic grid, whatever "rollout_launches" says.
static int plan_call(const char* who, const t1d_ctx* c, const t1d_batch* b, int minutes, int n_sub, bool rollout, Plan* out,
                     bool one_launch = false)
{
    Plan& p = *out;
    p = Plan();
    if (minutes < 1 || minutes > 100000) return fail(T1D_E_INVALID, std::string(who) + ": minutes out of range");
    if (n_sub < 1 || n_sub > 4096) return fail(T1D_E_INVALID, std::string(who) + ": n_sub out of range");
    bool split = c->math != 0 && n_sub >= 2 && n_sub <= 8 && !(n_sub & 1);     // what the split integrator needs
    if (c->integrator == 1 && !split)
        return fail(T1D_E_INVALID, std::string(who) + ": the split integrator needs math = 1 and n_sub in {2, 4, 6, 8}");
    split = split && c->integrator != 0;
    p.tables = split;
    p.f64 = b->dtype == T1D_F64;
    const size_t esz = p.f64 ? 8 : 4;
    p.extra = b->lbgi || b->hbgi || b->risk || b->meal || b->insulin;
    // At most one CGM sample per launch (minutes <= sample_time): the noise-block refill can run as its own kernel ahead of
    // a step kernel compiled without it
    const bool split_refill = c->math != 0 && c->split_refill && minutes <= (int)c->sensor[5];

    // The persistent kernels: the split integrator on the packed layout, the noise refill kept out of the step kernel,
    // tables that fit in LDS; one workgroup of 4 x T1D_S1_WAVES waves per CU
    const int stride = c->np <= 32 ? 32 : 64;
    const size_t tables = (size_t)(DP_COUNT + kPropRows(n_sub)) * stride * esz;
    const bool persist = split_refill && split && c->single_minute_kernel && is_packed(b, esz) &&
                         !(T1D_AB_FLAGS && (b->flags & 0x600)) && tables + 512 <= (size_t)c->lds_per_block;
    const int nchunks = (int)((b->n + 63) / 64);
    const int blocks = std::min(c->s1_blocks > 0 ? c->s1_blocks : c->n_cu, nchunks);
    const int per_block = (nchunks + blocks - 1) / blocks;

    // The multi-minute kernel.  Steps of several minutes: the state in registers across the minutes, lanes of level 2
    // parked and finished at the end (measured, Dexcom steps: fp64 147 against 184 us at 512 Ki envs, 257 against 339 at
    // 1 Mi, 883 against 1254 at 4 Mi, level at 256 Ki, the generic kernel ahead below; fp32 within 6 % of the generic
    // kernel at every size).  Roll-outs of large batches: one launch per step, the controller in its prologue -- the
    // step-size rule's lanes of level 2 are set aside, where the all-steps-in-one-launch kernel runs each wave at the level
    // of its most refined lane (a step of one minute too: the kernel takes any minutes >= 1).
    const bool want_n = rollout
        ? !one_launch && c->multi_minute_kernel != 0 && (c->rollout_launches == 2 || (c->rollout_launches == 1 &&
              b->n >= (p.f64 ? c->rollout_launches_min_envs : c->rollout_launches_min_envs_f32)))
        : minutes > 1 && (c->multi_minute_kernel == 2 || (c->multi_minute_kernel == 1 &&
              b->n >= (p.f64 ? c->multi_minute_min_envs : c->multi_minute_min_envs_f32)));
    // its LDS beside the tables: the redo map (one bit per env of the workgroup's share) and the records -- as many as fit,
    // never more than the workgroup's env-minutes
    const size_t map = (size_t)per_block * 8 + 8, rec = (size_t)kSnParkT * esz + (size_t)kSnParkI * sizeof(int);
    if (persist && want_n && stride == 32 && tables + map + 1024 <= (size_t)c->lds_per_block) {
        long long cap = (long long)(((size_t)c->lds_per_block - 1024 - tables - map) / rec) / 64 * 64;
        const long long share = ((long long)per_block * 64 * minutes + 63) / 64 * 64;
        if (cap > share) cap = share;
        if (c->park_cap > 0 && cap > (c->park_cap + 63) / 64 * 64) cap = (c->park_cap + 63) / 64 * 64;
        p.kernel = Kern::stepn;
        p.ctrl = rollout;
        p.extra = p.extra || rollout;            // a roll-out has the one instance stepn_kernel<T, true, true>
        // a roll-out refills ahead of every step, whatever T1D_BATCH_NO_REFILL_DUE says (the clocks are the envs')
        p.refill_ahead = rollout || !(b->flags & T1D_BATCH_NO_REFILL_DUE);
        p.grid = blocks; p.block = p.f64 ? sn_threads<double>() : sn_threads<float>();
        p.lds = tables + (size_t)cap * rec + map;
        p.nchunks = nchunks; p.cap = (int)cap;
        p.mode = (c->adaptive_gut != 0 ? 1 : 0) | (c->adaptive_gut == 2 ? 2 : 0) | (c->record_group_min << 8);
        return T1D_OK;
    }
    if (persist && !rollout && minutes == 1) {
        // One simulated minute per launch: the persistent early-store kernels.  With per-minute step sizes, lanes of level 2
        // are set aside and integrated together at the end of the launch (step1d_kernel) where the list of the CU's envs
        // fits next to the tables; adaptive_gut = 2 asks for the in-place form, 3 for the set-aside form at any batch size.
        const size_t lds1d = tables + (size_t)kS1DPark * (18 * esz + 3 * sizeof(int)) + (size_t)per_block * 64 * sizeof(uint16_t);
        p.tiered = c->adaptive_gut != 0;
        const bool defer = p.tiered && (c->adaptive_gut == 3 || (c->adaptive_gut == 1 && per_block >= c->defer_min_chunks)) &&
                           stride == 32 && per_block * 64 <= 65536 && lds1d + 512 <= (size_t)c->lds_per_block;
        p.kernel = defer ? Kern::step1d : Kern::step1;
        p.stride = stride;
        p.refill_ahead = !(b->flags & T1D_BATCH_NO_REFILL_DUE);
        p.grid = blocks;
        p.block = defer ? (p.f64 ? s1d_threads<double>() : s1d_threads<float>()) : (p.f64 ? s1_threads<double>() : s1_threads<float>());
        p.lds = defer ? lds1d : tables;
        p.nchunks = nchunks;
        return T1D_OK;
    }

    // The generic kernels keep the propagator table [rows][np_pad] in dynamic LDS, next to a static parameter table in the
    // LDS-parameter variants.  Where it does not fit (many patients x many sub-steps): classical RK4 when the caller left the
    // choice of integrator to the library.
    if (split) {
        p.lds = (size_t)kPropRows(n_sub) * c->np_pad * esz;
        if (p.lds + (size_t)DP_COUNT * kMaxPatients * esz + 1024 > (size_t)c->lds_per_block) {
            if (c->integrator == 1)
                return fail(T1D_E_INVALID, std::string(who) + ": split tables exceed the LDS of a workgroup" +
                                           (rollout ? "" : " (n_patients x n_sub too large)") + "; use integrator 0 or -1");
            split = false; p.lds = 0;          // the RK4 fallback
        }
    }
    p.kernel = rollout ? Kern::rollout : Kern::step;
    // with per-lane step sizes the parameters fit in VGPRs in fp32 only
    p.variant = c->math == 0 ? 0 : !split ? 3 : !c->adaptive_gut ? 4 : p.f64 ? 7 : 6;
    p.refill = !split_refill;
    p.refill_ahead = !rollout && split_refill && !(b->flags & T1D_BATCH_NO_REFILL_DUE);
    p.grid = (unsigned)((b->n + kBlock - 1) / kBlock); p.block = kBlock;
    return T1D_OK;
}

// plan_call, then the split tables wherever the split integrator is asked for: also where the plan then fails for want
// of LDS or falls back to RK4
static int plan_and_tables(const char* who, t1d_ctx* c, const t1d_batch* b, int minutes, int n_sub, bool rollout, Plan* p,
                           bool one_launch = false)
{
    const int rc = plan_call(who, c, b, minutes, n_sub, rollout, p, one_launch);
    const int e = p->tables ? ensure_split(c, n_sub) : T1D_OK;
    return e ? e : rc;
}

template <typename T, typename... X> using KernelFn = void (*)(KArgs<T>, X...);

// one launch of a planned kernel, its dynamic-LDS ceiling raised first.  A persistent kernel counts the launch before its
// arguments are built: KArgs.flags carries the new pingpong parity.
template <typename T, typename... X, typename... A>
static int launch(t1d_ctx* c, const t1d_batch* b, const Plan& p, int minutes, int n_sub, hipStream_t s, KernelFn<T, X...> kernel, A... rest)
{
    T1D_HIP(allow_lds(c, (const void*)kernel, p.lds));
    if (p.kernel != Kern::step && p.kernel != Kern::rollout) ++c->launches;
    hipLaunchKernelGGL(kernel, dim3(p.grid), dim3(p.block), p.lds, s, make_args<T>(c, b, minutes, n_sub), rest...);
    return T1D_OK;
}

// the generic kernels by variant: f(std::integral_constant<int, VARIANT>()) for the VARIANT of a plan; the split
// variant with per-minute step sizes is 7 in fp64, 6 in fp32
template <typename T, typename F>
static auto by_variant(int variant, F&& f)
{
    switch (variant) {
    case 0: return f(std::integral_constant<int, 0>());
    case 3: return f(std::integral_constant<int, 3>());
    case 4: return f(std::integral_constant<int, 4>());
    default: return f(std::integral_constant<int, sizeof(T) == 8 ? 7 : 6>());
    }
}

template <typename T, bool REFILL>
static KernelFn<T> step_fn(int variant)
{
    return by_variant<T>(variant, [](auto v) -> KernelFn<T> { return step_kernel<decltype(v)::value, T, REFILL>; });
}

template <typename T>
static KernelFn<T, PidArgs<T>> rollout_fn(int variant)
{
    return by_variant<T>(variant, [](auto v) -> KernelFn<T, PidArgs<T>> { return rollout_pid_kernel<decltype(v)::value, T>; });
}

template <typename T, int STRIDE>
static KernelFn<T, int> step1_fn(bool extra, bool tiered)
{
    if (extra) return tiered ? step1_kernel<T, STRIDE, true, true> : step1_kernel<T, STRIDE, true, false>;
    return tiered ? step1_kernel<T, STRIDE, false, true> : step1_kernel<T, STRIDE, false, false>;
}

// the refill (if planned), then the planned kernel; pa: the controller of a roll-out (stepn_kernel: of one step)
template <typename T>
static int launch_plan(t1d_ctx* c, const t1d_batch* b, const Plan& p, int minutes, int n_sub, const PidArgs<T>& pa, hipStream_t s)
{
    if (p.refill_ahead)
        hipLaunchKernelGGL(refill_kernel<T>, grid_for(b->n), dim3(kBlock), 0, s, make_args<T>(c, b, minutes, n_sub));
    switch (p.kernel) {
    case Kern::step:
        return launch(c, b, p, minutes, n_sub, s, p.refill ? step_fn<T, true>(p.variant) : step_fn<T, false>(p.variant));
    case Kern::rollout:
        return launch(c, b, p, minutes, n_sub, s, rollout_fn<T>(p.variant), pa);
    case Kern::step1:
        return launch(c, b, p, minutes, n_sub, s, p.stride == 32 ? step1_fn<T, 32>(p.extra, p.tiered) : step1_fn<T, 64>(p.extra, p.tiered),
                      p.nchunks);
    case Kern::step1d:
        return launch(c, b, p, minutes, n_sub, s, p.extra ? step1d_kernel<T, true> : step1d_kernel<T, false>, p.nchunks);
    case Kern::stepn:
        return launch(c, b, p, minutes, n_sub, s,
                      p.ctrl ? stepn_kernel<T, true, true> : p.extra ? stepn_kernel<T, true, false> : stepn_kernel<T, false, false>,
                      pa, p.nchunks, p.cap, p.mode);
    }
    return T1D_OK;
}

extern "C" int t1d_step(t1d_ctx* c, const t1d_batch* b, int minutes, int n_sub, void* stream)
{
    int rc = check_batch("t1d_step", c, b, true);
    if (rc) return rc;
    Plan p;
    rc = plan_and_tables("t1d_step", c, b, minutes, n_sub, false, &p);
    if (rc) return rc;
    hipStream_t s = (hipStream_t)stream;
    rc = p.f64 ? launch_plan<double>(c, b, p, minutes, n_sub, PidArgs<double>{}, s) : launch_plan<float>(c, b, p, minutes, n_sub, PidArgs<float>{}, s);
    if (rc) return rc;
    T1D_HIP(hipGetLastError());
    return T1D_OK;
}

// What every exact-mode call asks of its arguments, checked before any device work.  rollout: n_steps closed-loop
// steps, whose actions are the controller's and whose meals the meal table's; else one step with the batch's actions
// (t1d_step_dopri5).
static int check_dopri5(const char* who, const t1d_ctx* c, const t1d_batch* b, const double* h_carry, int n_steps, int minutes,
                        bool rollout = true)
{
    const std::string w(who);
    if (!c) return fail(T1D_E_INVALID, w + ": ctx is NULL");
    if (!b) return fail(T1D_E_INVALID, w + ": batch is NULL");
    if (!h_carry) return fail(T1D_E_INVALID, w + ": h_carry is NULL");
    if (b->dtype != T1D_F64) return fail(T1D_E_INVALID, w + ": fp64 batches only");
    if (rollout && n_steps < 1) return fail(T1D_E_INVALID, w + ": n_steps < 1");
    if (minutes < 1 || minutes > 100000) return fail(T1D_E_INVALID, w + ": minutes out of range");
    if (rollout && b->cho) return fail(T1D_E_INVALID, w + ": dense cho is not supported, use the meal table");
    return check_batch(who, c, b, !rollout);
}

// The exact mode (t1d_dopri5.hpp): one lane per env on the grid of the generic kernel, whatever the layout; no plan, no
// refill ahead (the noise-block refill runs inline).
extern "C" int t1d_step_dopri5(t1d_ctx* c, const t1d_batch* b, double* h_carry, int32_t* nfev, int minutes, void* stream)
{
    const int rc = check_dopri5("t1d_step_dopri5", c, b, h_carry, /* n_steps */ 1, minutes, /* rollout */ false);
    if (rc) return rc;
    hipLaunchKernelGGL(dopri5_step_kernel, grid_for(b->n), dim3(kBlock), 0, (hipStream_t)stream, make_args<double>(c, b, minutes, 1),
                       (const double*)c->d_raw64, h_carry, nfev);
    T1D_HIP(hipGetLastError());
    return T1D_OK;
}

template <typename T>
static PidArgs<T> make_pid(const t1d_pid* p, int n_steps)
{
    PidArgs<T> c;
    c.P = (T)p->P; c.I = (T)p->I; c.D = (T)p->D; c.target = (T)p->target;
    c.integ = (T*)p->integ; c.prev = (T*)p->prev; c.sum_risk = (T*)p->sum_risk;
    c.min_bg = (T*)p->min_bg; c.max_bg = (T*)p->max_bg; c.n_low = p->n_low; c.n_high = p->n_high;
    c.n_steps = n_steps;
    c.kind = 0; c.bb_basal = nullptr; c.bb_cr = nullptr; c.bb_cf = nullptr; c.bb_prev_meal = nullptr;
    c.bg_trace = (T*)p->bg_trace; c.cgm_trace = (T*)p->cgm_trace; c.cho_trace = (T*)p->cho_trace; c.ins_trace = (T*)p->insulin_trace;
    c.trace_row = p->trace_row;
    return c;
}

template <typename T>
static PidArgs<T> make_bb(const t1d_bb* p, int n_steps)
{
    PidArgs<T> c;
    c.P = c.I = c.D = T(0); c.target = (T)p->target;
    c.integ = nullptr; c.prev = nullptr; c.sum_risk = (T*)p->sum_risk;
    c.min_bg = (T*)p->min_bg; c.max_bg = (T*)p->max_bg; c.n_low = p->n_low; c.n_high = p->n_high;
    c.n_steps = n_steps;
    c.kind = 1; c.bb_basal = (const T*)p->basal; c.bb_cr = (const T*)p->cr; c.bb_cf = (const T*)p->cf; c.bb_prev_meal = (T*)p->prev_meal;
    c.bg_trace = (T*)p->bg_trace; c.cgm_trace = (T*)p->cgm_trace; c.cho_trace = (T*)p->cho_trace; c.ins_trace = (T*)p->insulin_trace;
    c.trace_row = p->trace_row;
    return c;
}

// all n_steps in one launch of rollout_pid_kernel, or one launch of stepn_kernel per step
template <typename T>
static int run_rollout(t1d_ctx* c, const t1d_batch* b, const Plan& p, const PidArgs<T>& pa, int n_steps, int minutes, int n_sub, hipStream_t s)
{
    if (!p.ctrl) return launch_plan<T>(c, b, p, minutes, n_sub, pa, s);
    for (int k = 0; k < n_steps; ++k) {
        PidArgs<T> one = pa;
        one.n_steps = 1; one.trace_row += k;
        const int rc = launch_plan<T>(c, b, p, minutes, n_sub, one, s);
        if (rc) return rc;
    }
    return T1D_OK;
}

// the batch and the step count of a fixed-step closed-loop call: the controller acts, the meals are the meal table's
static int check_closed_loop(const char* who, const t1d_ctx* c, const t1d_batch* b, int n_steps)
{
    const int rc = check_batch(who, c, b, false);
    if (rc) return rc;
    if (b->cho) return fail(T1D_E_INVALID, std::string(who) + ": dense cho is not supported, use the meal table");
    if (n_steps < 1) return fail(T1D_E_INVALID, std::string(who) + ": n_steps < 1");
    return T1D_OK;
}

// a closed-loop roll-out under the PID controller pid or the basal-bolus controller bb (the other one NULL)
static int launch_rollout(const char* who, t1d_ctx* c, const t1d_batch* b, const t1d_pid* pid, const t1d_bb* bb, int n_steps,
                          int minutes, int n_sub, void* stream)
{
    int rc = check_closed_loop(who, c, b, n_steps);
    if (rc) return rc;
    Plan p;
    rc = plan_and_tables(who, c, b, minutes, n_sub, true, &p);
    if (rc) return rc;
    hipStream_t s = (hipStream_t)stream;
    if (p.f64) rc = run_rollout<double>(c, b, p, pid ? make_pid<double>(pid, n_steps) : make_bb<double>(bb, n_steps), n_steps, minutes, n_sub, s);
    else rc = run_rollout<float>(c, b, p, pid ? make_pid<float>(pid, n_steps) : make_bb<float>(bb, n_steps), n_steps, minutes, n_sub, s);
    if (rc) return rc;
    T1D_HIP(hipGetLastError());
    return T1D_OK;
}

extern "C" int t1d_rollout_pid(t1d_ctx* c, const t1d_batch* b, const t1d_pid* pid, int n_steps, int minutes,
                               int n_sub, void* stream)
{
    if (!pid || !pid->integ || !pid->prev) return fail(T1D_E_INVALID, "t1d_rollout_pid: pid state is NULL");
    return launch_rollout("t1d_rollout_pid", c, b, pid, nullptr, n_steps, minutes, n_sub, stream);
}

// ---- t1d_pid_gains: the PID controller's four numbers per env (t1d_rollout_pid_gains, t1d_rollout_pid_dopri5_gains) -------
// needs no device: both calls check it ahead of the batch, so that a bad call is refused on any machine
static int check_pid_gains(const char* who, const t1d_pid_gains* g)
{
    const std::string w = std::string(who) + ": ";
    if (!g) return fail(T1D_E_INVALID, w + "gains is NULL");
    if (!g->P) return fail(T1D_E_INVALID, w + "gains.P is NULL");
    if (!g->I) return fail(T1D_E_INVALID, w + "gains.I is NULL");
    if (!g->D) return fail(T1D_E_INVALID, w + "gains.D is NULL");
    if (!g->target) return fail(T1D_E_INVALID, w + "gains.target is NULL");
    return T1D_OK;
}

// make_pid with the arrays of g; the four scalars of p are not read
template <typename T>
static PidGainArgs<T> make_pid_gains(const t1d_pid* p, const t1d_pid_gains* g, int n_steps)
{
    t1d_pid q = *p;
    q.P = q.I = q.D = q.target = 0.0;
    PidGainArgs<T> c;
    static_cast<PidArgs<T>&>(c) = make_pid<T>(&q, n_steps);
    c.gP = (const T*)g->P; c.gI = (const T*)g->I; c.gD = (const T*)g->D; c.gtarget = (const T*)g->target;
    return c;
}

template <typename T>
static KernelFn<T, PidGainArgs<T>> rollout_gains_fn(int variant)
{
    return by_variant<T>(variant, [](auto v) -> KernelFn<T, PidGainArgs<T>> { return rollout_pid_gains_kernel<decltype(v)::value, T>; });
}

// run_rollout with the per-env form of the plan's kernel: rollout_pid_gains_kernel where the plan says rollout_pid_kernel,
// one stepn_gains_kernel per step behind its refill where it says stepn_kernel<T, true, true>.  The plan is the scalar call's.
template <typename T>
static int run_rollout_gains(t1d_ctx* c, const t1d_batch* b, const Plan& p, const PidGainArgs<T>& pa, int n_steps, int minutes, int n_sub, hipStream_t s)
{
    if (p.kernel == Kern::rollout) return launch(c, b, p, minutes, n_sub, s, rollout_gains_fn<T>(p.variant), pa);
    if (p.kernel != Kern::stepn || !p.ctrl) return fail(T1D_E_INVALID, "t1d_rollout_pid_gains: the plan names no roll-out kernel");
    for (int k = 0; k < n_steps; ++k) {
        PidGainArgs<T> one = pa;
        one.n_steps = 1; one.trace_row += k;
        if (p.refill_ahead)
            hipLaunchKernelGGL(refill_kernel<T>, grid_for(b->n), dim3(kBlock), 0, s, make_args<T>(c, b, minutes, n_sub));
        const int rc = launch(c, b, p, minutes, n_sub, s, stepn_gains_kernel<T>, one, p.nchunks, p.cap, p.mode);
        if (rc) return rc;
    }
    return T1D_OK;
}

extern "C" int t1d_rollout_pid_gains(t1d_ctx* c, const t1d_batch* b, const t1d_pid* pid, const t1d_pid_gains* gains, int n_steps,
                                     int minutes, int n_sub, void* stream)
{
    const char* who = "t1d_rollout_pid_gains";
    if (!pid || !pid->integ || !pid->prev) return fail(T1D_E_INVALID, "t1d_rollout_pid_gains: pid state is NULL");
    int rc = check_pid_gains(who, gains);
    if (rc) return rc;
    rc = check_closed_loop(who, c, b, n_steps);
    if (rc) return rc;
    Plan p;
    rc = plan_and_tables(who, c, b, minutes, n_sub, true, &p);
    if (rc) return rc;
    hipStream_t s = (hipStream_t)stream;
    if (p.f64) rc = run_rollout_gains<double>(c, b, p, make_pid_gains<double>(pid, gains, n_steps), n_steps, minutes, n_sub, s);
    else rc = run_rollout_gains<float>(c, b, p, make_pid_gains<float>(pid, gains, n_steps), n_steps, minutes, n_sub, s);
    if (rc) return rc;
    T1D_HIP(hipGetLastError());
    return T1D_OK;
}

extern "C" int t1d_rollout_bb(t1d_ctx* c, const t1d_batch* b, const t1d_bb* bb, int n_steps, int minutes,
                              int n_sub, void* stream)
{
    if (!bb || !bb->basal || !bb->cr || !bb->cf || !bb->prev_meal)
        return fail(T1D_E_INVALID, "t1d_rollout_bb: basal / cr / cf / prev_meal must be set");
    return launch_rollout("t1d_rollout_bb", c, b, nullptr, bb, n_steps, minutes, n_sub, stream);
}

// ---- t1d_rollout_mlp (t1d_policy.hpp) ---------------------------------------------------------------------------------
template <typename T>
static KernelFn<T, MlpArgs<T>> mlp_rollout_fn(int variant)
{
    return by_variant<T>(variant, [](auto v) -> KernelFn<T, MlpArgs<T>> { return mlp_rollout_kernel<decltype(v)::value, T>; });
}

template <typename T>
static MlpArgs<T> make_mlp(const t1d_mlp* m, int n_steps)
{
    MlpArgs<T> c;
    c.params = (const T*)m->params;
    c.cgm_hist = (T*)m->cgm_hist; c.ins_hist = (T*)m->ins_hist; c.prev_meal = (T*)m->prev_meal; c.start_minute = m->start_minute;
    c.cgm_mean = (T)m->cgm_mean; c.cgm_scale = (T)m->cgm_scale; c.ins_scale = (T)m->ins_scale; c.cho_scale = (T)m->cho_scale;
    c.out_scale = (T)m->out_scale; c.out_bias = (T)m->out_bias;
    c.sum_risk = (T*)m->sum_risk; c.min_bg = (T*)m->min_bg; c.max_bg = (T*)m->max_bg; c.n_low = m->n_low; c.n_high = m->n_high;
    c.bg_trace = (T*)m->bg_trace; c.cgm_trace = (T*)m->cgm_trace; c.cho_trace = (T*)m->cho_trace; c.ins_trace = (T*)m->insulin_trace;
    c.act_trace = (T*)m->action_trace; c.trace_row = m->trace_row;
    c.envs_per_policy = (unsigned)m->envs_per_policy;
    c.widths = 0;
    for (int l = 0; l < m->n_layers; ++l) c.widths |= (unsigned)m->width[l] << (8 * l);
    c.n_params = (int)m->n_params; c.history = m->history; c.n_layers = m->n_layers;
    c.hidden_act = m->hidden_act; c.out_act = m->out_act; c.n_steps = n_steps;
    c.lds_off = 0; c.cols = 0;
    return c;
}

// every field of the policy that has a range; -> the rows of a wave's column block in *cols
// state = false (t1d_mlp_grad): the network alone, of n envs -- out_act and the state arrays are not looked at
static int check_mlp_net(const char* who, int64_t n, const t1d_mlp* m, int* cols, bool state)
{
    const std::string w = std::string(who) + ": ";
    if (!m) return fail(T1D_E_INVALID, w + "mlp is NULL");
    if (m->history < 1 || m->history > kMlpMaxHistory) return fail(T1D_E_INVALID, w + "history must be in [1, 12]");
    if (m->n_layers < 1 || m->n_layers > kMlpMaxLayers) return fail(T1D_E_INVALID, w + "n_layers must be in [1, 4]");
    const int F = 2 * m->history + 3;
    int64_t count = 0;
    int in_w = F, widest = F;
    for (int l = 0; l < m->n_layers; ++l) {
        if (m->width[l] < 1 || m->width[l] > kMlpMaxWidth) return fail(T1D_E_INVALID, w + "every width must be in [1, 32]");
        count += (int64_t)m->width[l] * (in_w + 1);
        in_w = m->width[l];
        if (l + 1 < m->n_layers) widest = std::max(widest, in_w);
    }
    if (m->width[m->n_layers - 1] != 1) return fail(T1D_E_INVALID, w + "the last layer's width must be 1");
    if (m->n_params != count) return fail(T1D_E_INVALID, w + "n_params must be " + std::to_string(count) + " for these widths");
    if (m->hidden_act != T1D_MLP_TANH && m->hidden_act != T1D_MLP_RELU) return fail(T1D_E_INVALID, w + "unknown hidden_act");
    if (state && m->out_act != T1D_MLP_IDENTITY && m->out_act != T1D_MLP_LOGISTIC) return fail(T1D_E_INVALID, w + "unknown out_act");
    if (!m->params || (state && (!m->cgm_hist || !m->ins_hist || !m->prev_meal)))
        return fail(T1D_E_INVALID, w + (state ? "params / cgm_hist / ins_hist / prev_meal must be set" : "params must be set"));
    if (m->n_policies < 1) return fail(T1D_E_INVALID, w + "n_policies < 1");
    if (m->envs_per_policy < 64 || m->envs_per_policy % 64) return fail(T1D_E_INVALID, w + "envs_per_policy must be a multiple of 64");
    if (m->envs_per_policy > ((int64_t)1 << 28) || m->n_policies > ((int64_t)1 << 28) || n != m->n_policies * m->envs_per_policy)
        return fail(T1D_E_INVALID, w + (state ? "batch.n must be n_policies * envs_per_policy" : "n must be n_policies * envs_per_policy"));
    *cols = 2 * m->history + widest;
    return T1D_OK;
}

static int check_mlp(const char* who, const t1d_batch* b, const t1d_mlp* m, int* cols) { return check_mlp_net(who, b->n, m, cols, true); }

// The launch shape of the kernels that run the policy: every wave of a workgroup has per_wave bytes of dynamic LDS of
// its own, behind front bytes they share (rounded up to 16) and beside fixed bytes of static LDS.  The workgroup is the
// largest, from `largest` threads down by halves to one wave, whose LDS stays within the ceiling.  A pure function,
// like plan_call; each family below brings its constants and its refusal.  Checked on the CPU by
// tests/dispatch_plan_driver.cpp.
struct Shape { unsigned threads = 0, grid = 0; size_t front = 0, lds = 0; };   // lds: dynamic bytes; front: where the waves' begin

static bool launch_shape(int64_t n, size_t fixed, size_t front, size_t per_wave, unsigned largest, size_t ceiling, Shape* sh)
{
    sh->front = (front + 15) & ~(size_t)15;
    sh->threads = largest;
    while (sh->threads > 64 && fixed + sh->front + per_wave * (sh->threads / 64) > ceiling) sh->threads /= 2;
    sh->grid = (unsigned)((n + sh->threads - 1) / sh->threads);
    sh->lds = sh->front + per_wave * (sh->threads / 64);
    return fixed + sh->lds <= ceiling;      // false: not even one wave fits
}

// the fixed-step kernels' (t1d_rollout_mlp, t1d_collect_mlp), into the plan and the policy's arguments.  Dynamic LDS:
// the propagator table as the plan sized it, then the columns of every wave (the LDS-parameter variants hold theirs in
// static LDS)
template <typename T>
static int shape_mlp(const char* who, const t1d_ctx* c, const t1d_batch* b, int cols, Plan& p, MlpArgs<T>& ma)
{
    const size_t fixed = (p.variant == 0 || p.variant == 7 ? (size_t)DP_COUNT * kMaxPatients * sizeof(T) : 0) + 256;   // static LDS
    Shape sh;
    if (!launch_shape(b->n, fixed, p.lds, (size_t)cols * 64 * sizeof(T), T1D_POLICY_THREADS, (size_t)c->lds_per_block, &sh))
        return fail(T1D_E_INVALID, std::string(who) + ": the integrator's tables leave no room in LDS for one wave of this policy");
    ma.lds_off = (int)sh.front; ma.cols = cols;
    p.lds = sh.lds; p.block = sh.threads; p.grid = sh.grid;
    return T1D_OK;
}

// the exact mode's (dopri5_mlp_rollout_kernel, dopri5_mlp_collect_kernel): for every wave RollCold's words and the
// policy's columns; the workgroup is the most waves (4, 2 or 1) whose pieces fit beside the raw patient rows
static int shape_mlp_dopri5(const char* who, const t1d_ctx* c, int64_t n, int cols, Shape* sh)
{
    const size_t fixed = (size_t)kRawPars * kMaxPatients * sizeof(double) + 256;           // static LDS
    if (!launch_shape(n, fixed, 0, (size_t)kRollColdWaveBytes + (size_t)cols * 64 * sizeof(double), kBlock, (size_t)c->lds_per_block, sh))
        return fail(T1D_E_INVALID, std::string(who) + ": the patient rows leave no room in LDS for one wave of this policy");
    return T1D_OK;
}

// the policy's alone (mlp_action_kernel, mlp_features_kernel): the columns of every wave, within the 64 KiB any kernel
// may have without asking; one wave of the widest policy is 28 KiB, so there is nothing to refuse
template <typename T>
static Shape shape_mlp_alone(const t1d_ctx* c, int64_t n, int cols)
{
    Shape sh;
    (void)launch_shape(n, 0, 0, (size_t)cols * 64 * sizeof(T), T1D_POLICY_THREADS, std::min<size_t>((size_t)c->lds_per_block, 65536) - 256, &sh);
    return sh;
}

// ---- t1d_meal_bolus: the bolus calculator of the *_bolus entry points (BolusArgs, t1d_policy.hpp) ------------------------
// needs no device: every *_bolus call checks it first, so that a bad call is refused on any machine
static int check_meal_bolus(const char* who, const t1d_meal_bolus* mb)
{
    const std::string w = std::string(who) + ": ";
    if (!mb) return fail(T1D_E_INVALID, w + "meal_bolus is NULL");
    if (!mb->cr || !mb->cf) return fail(T1D_E_INVALID, w + "meal_bolus.cr / cf must be set");
    return T1D_OK;
}

template <typename T>
static BolusArgs<T> make_bolus(const t1d_meal_bolus* mb)
{
    return BolusArgs<T>{(T)mb->target, (const T*)mb->cr, (const T*)mb->cf, (T*)mb->bolus_trace};
}

// ---- t1d_env_output: the per-env scale and bias of the *_rel entry points (EnvOutArgs, t1d_policy.hpp) -------------------
// needs no device, like check_meal_bolus; a *_rel call's meal_bolus may be NULL (no bolus), and is checked when it is not
static int check_env_output(const char* who, const t1d_env_output* eo, const t1d_meal_bolus* mb)
{
    const std::string w = std::string(who) + ": ";
    if (!eo) return fail(T1D_E_INVALID, w + "env_output is NULL");
    if (!eo->scale || !eo->bias) return fail(T1D_E_INVALID, w + "env_output.scale / bias must be set");
    return mb ? check_meal_bolus(who, mb) : T1D_OK;
}

template <typename T>
static EnvOutArgs<T> make_env_out(const t1d_env_output* eo)
{
    return EnvOutArgs<T>{(const T*)eo->scale, (const T*)eo->bias};
}

// the BolusArgs of a *_rel kernel: all NULL switches the bolus off
template <typename T>
static BolusArgs<T> make_bolus_or_none(const t1d_meal_bolus* mb)
{
    return mb ? make_bolus<T>(mb) : BolusArgs<T>{};
}

template <typename T> using CollectFn = KernelFn<T, MlpArgs<T>, CollectArgs<T>, RestartArgs<T>>;
template <typename T> using CollectBolusFn = KernelFn<T, MlpArgs<T>, CollectArgs<T>, RestartArgs<T>, BolusArgs<T>>;
template <typename T>
static CollectBolusFn<T> mlp_collect_bolus_fn(int variant)
{
    return by_variant<T>(variant, [](auto v) -> CollectBolusFn<T> { return mlp_collect_bolus_kernel<decltype(v)::value, T>; });
}

template <typename T> using CollectRelFn = KernelFn<T, MlpArgs<T>, CollectArgs<T>, RestartArgs<T>, EnvOutArgs<T>, BolusArgs<T>>;
template <typename T>
static CollectRelFn<T> mlp_collect_rel_fn(int variant)
{
    return by_variant<T>(variant, [](auto v) -> CollectRelFn<T> { return mlp_collect_rel_kernel<decltype(v)::value, T>; });
}

// mb == NULL: t1d_rollout_mlp, mlp_rollout_kernel.  With mb (t1d_rollout_mlp_bolus): the collector's kernel with no sigma, no
// collector traces and T1D_COLLECT_CONTINUE -- the form in which it computes what mlp_rollout_kernel computes, word for word
// (mlp_collect_body), at the same cost (README.md) -- so that the bolus needs one new kernel family and not two.
// With eo (t1d_rollout_mlp_rel): the relative policy's family in that same form, with or without mb.
template <typename T>
static int run_rollout_mlp(const char* who, t1d_ctx* c, const t1d_batch* b, const t1d_mlp* m, const t1d_env_output* eo,
                           const t1d_meal_bolus* mb, Plan p, int cols, int n_steps, int minutes, int n_sub, hipStream_t s)
{
    MlpArgs<T> ma = make_mlp<T>(m, n_steps);
    const int rc = shape_mlp<T>(who, c, b, cols, p, ma);
    if (rc) return rc;
    if (!eo && !mb) return launch(c, b, p, minutes, n_sub, s, mlp_rollout_fn<T>(p.variant), ma);
    CollectArgs<T> ga = {};
    ga.on_done = T1D_COLLECT_CONTINUE;
    if (eo)
        return launch(c, b, p, minutes, n_sub, s, mlp_collect_rel_fn<T>(p.variant), ma, ga, RestartArgs<T>{}, make_env_out<T>(eo),
                      make_bolus_or_none<T>(mb));
    return launch(c, b, p, minutes, n_sub, s, mlp_collect_bolus_fn<T>(p.variant), ma, ga, RestartArgs<T>{}, make_bolus<T>(mb));
}

static int rollout_mlp_entry(const char* who, t1d_ctx* c, const t1d_batch* b, const t1d_mlp* mlp, const t1d_env_output* eo,
                             const t1d_meal_bolus* mb, int n_steps, int minutes, int n_sub, void* stream)
{
    int rc = check_closed_loop(who, c, b, n_steps);
    if (rc) return rc;
    int cols = 0;
    rc = check_mlp(who, b, mlp, &cols);
    if (rc) return rc;
    // the plan of a roll-out that keeps all its steps in one launch: variant, refill and the propagator table's LDS
    Plan p;
    rc = plan_and_tables(who, c, b, minutes, n_sub, true, &p, true);
    if (rc) return rc;
    hipStream_t s = (hipStream_t)stream;
    rc = p.f64 ? run_rollout_mlp<double>(who, c, b, mlp, eo, mb, p, cols, n_steps, minutes, n_sub, s)
               : run_rollout_mlp<float>(who, c, b, mlp, eo, mb, p, cols, n_steps, minutes, n_sub, s);
    if (rc) return rc;
    T1D_HIP(hipGetLastError());
    return T1D_OK;
}

extern "C" int t1d_rollout_mlp(t1d_ctx* c, const t1d_batch* b, const t1d_mlp* mlp, int n_steps, int minutes,
                               int n_sub, void* stream)
{
    return rollout_mlp_entry("t1d_rollout_mlp", c, b, mlp, nullptr, nullptr, n_steps, minutes, n_sub, stream);
}

extern "C" int t1d_rollout_mlp_bolus(t1d_ctx* c, const t1d_batch* b, const t1d_mlp* mlp, const t1d_meal_bolus* mb, int n_steps,
                                     int minutes, int n_sub, void* stream)
{
    const int rc = check_meal_bolus("t1d_rollout_mlp_bolus", mb);
    if (rc) return rc;
    return rollout_mlp_entry("t1d_rollout_mlp_bolus", c, b, mlp, nullptr, mb, n_steps, minutes, n_sub, stream);
}

extern "C" int t1d_rollout_mlp_rel(t1d_ctx* c, const t1d_batch* b, const t1d_mlp* mlp, const t1d_env_output* eo, const t1d_meal_bolus* mb,
                                   int n_steps, int minutes, int n_sub, void* stream)
{
    const int rc = check_env_output("t1d_rollout_mlp_rel", eo, mb);
    if (rc) return rc;
    return rollout_mlp_entry("t1d_rollout_mlp_rel", c, b, mlp, eo, mb, n_steps, minutes, n_sub, stream);
}

// The exact mode's roll-outs (t1d_dopri5.hpp): all n_steps in one launch of dopri5_rollout_kernel on the grid of
// dopri5_step_kernel, every lane at its own pace; no plan, no refill ahead.
static int launch_rollout_dopri5(const char* who, t1d_ctx* c, const t1d_batch* b, const t1d_pid* pid, const t1d_bb* bb,
                                 double* h_carry, int32_t* nfev, int n_steps, int minutes, void* stream)
{
    const int rc = check_dopri5(who, c, b, h_carry, n_steps, minutes);
    if (rc) return rc;
    hipLaunchKernelGGL(dopri5_rollout_kernel, grid_for(b->n), dim3(kBlock), 0, (hipStream_t)stream, make_args<double>(c, b, minutes, 1),
                       pid ? make_pid<double>(pid, n_steps) : make_bb<double>(bb, n_steps), (const double*)c->d_raw64, h_carry, nfev);
    T1D_HIP(hipGetLastError());
    return T1D_OK;
}

extern "C" int t1d_rollout_pid_dopri5(t1d_ctx* c, const t1d_batch* b, const t1d_pid* pid, double* h_carry, int32_t* nfev,
                                      int n_steps, int minutes, void* stream)
{
    if (!pid || !pid->integ || !pid->prev) return fail(T1D_E_INVALID, "t1d_rollout_pid_dopri5: pid state is NULL");
    return launch_rollout_dopri5("t1d_rollout_pid_dopri5", c, b, pid, nullptr, h_carry, nfev, n_steps, minutes, stream);
}

extern "C" int t1d_rollout_pid_dopri5_gains(t1d_ctx* c, const t1d_batch* b, const t1d_pid* pid, const t1d_pid_gains* gains,
                                            double* h_carry, int32_t* nfev, int n_steps, int minutes, void* stream)
{
    const char* who = "t1d_rollout_pid_dopri5_gains";
    if (!pid || !pid->integ || !pid->prev) return fail(T1D_E_INVALID, "t1d_rollout_pid_dopri5_gains: pid state is NULL");
    int rc = check_pid_gains(who, gains);
    if (rc) return rc;
    rc = check_dopri5(who, c, b, h_carry, n_steps, minutes);
    if (rc) return rc;
    hipLaunchKernelGGL(dopri5_rollout_gains_kernel, grid_for(b->n), dim3(kBlock), 0, (hipStream_t)stream, make_args<double>(c, b, minutes, 1),
                       make_pid_gains<double>(pid, gains, n_steps), (const double*)c->d_raw64, h_carry, nfev);
    T1D_HIP(hipGetLastError());
    return T1D_OK;
}

extern "C" int t1d_rollout_bb_dopri5(t1d_ctx* c, const t1d_batch* b, const t1d_bb* bb, double* h_carry, int32_t* nfev,
                                     int n_steps, int minutes, void* stream)
{
    if (!bb || !bb->basal || !bb->cr || !bb->cf || !bb->prev_meal)
        return fail(T1D_E_INVALID, "t1d_rollout_bb_dopri5: bb is NULL, or basal / cr / cf / prev_meal is not set");
    return launch_rollout_dopri5("t1d_rollout_bb_dopri5", c, b, nullptr, bb, h_carry, nfev, n_steps, minutes, stream);
}

// one launch of an exact-mode policy kernel in the shape of shape_mlp_dopri5; rest: what the kernel takes behind KArgs
template <typename... X, typename... A>
static int launch_mlp_dopri5(const char* who, t1d_ctx* c, const t1d_batch* b, int cols, int minutes, void* stream,
                             KernelFn<double, X...> kernel, A... rest)
{
    Shape sh;
    const int rc = shape_mlp_dopri5(who, c, b->n, cols, &sh);
    if (rc) return rc;
    T1D_HIP(allow_lds(c, (const void*)kernel, sh.lds));
    hipLaunchKernelGGL(kernel, dim3(sh.grid), dim3(sh.threads), sh.lds, (hipStream_t)stream, make_args<double>(c, b, minutes, 1), rest...);
    T1D_HIP(hipGetLastError());
    return T1D_OK;
}

// The exact mode's roll-out under the policy of t1d_mlp (dopri5_mlp_rollout_kernel, t1d_dopri5.hpp).
// mb == NULL: t1d_rollout_mlp_dopri5; with mb dopri5_mlp_rollout_bolus_kernel (t1d_rollout_mlp_dopri5_bolus); with eo
// dopri5_mlp_rollout_rel_kernel, with or without mb (t1d_rollout_mlp_dopri5_rel)
static int rollout_mlp_dopri5_entry(const char* who, t1d_ctx* c, const t1d_batch* b, const t1d_mlp* mlp, const t1d_env_output* eo,
                                    const t1d_meal_bolus* mb, double* h_carry, int32_t* nfev, int n_steps, int minutes, void* stream)
{
    int rc = check_dopri5(who, c, b, h_carry, n_steps, minutes);
    if (rc) return rc;
    int cols = 0;
    rc = check_mlp(who, b, mlp, &cols);
    if (rc) return rc;
    MlpArgs<double> ma = make_mlp<double>(mlp, n_steps);
    ma.cols = cols;
    if (eo)
        return launch_mlp_dopri5(who, c, b, cols, minutes, stream, dopri5_mlp_rollout_rel_kernel, ma, make_env_out<double>(eo),
                                 make_bolus_or_none<double>(mb), (const double*)c->d_raw64, h_carry, nfev);
    if (!mb) return launch_mlp_dopri5(who, c, b, cols, minutes, stream, dopri5_mlp_rollout_kernel, ma, (const double*)c->d_raw64, h_carry, nfev);
    return launch_mlp_dopri5(who, c, b, cols, minutes, stream, dopri5_mlp_rollout_bolus_kernel, ma, make_bolus<double>(mb),
                             (const double*)c->d_raw64, h_carry, nfev);
}

extern "C" int t1d_rollout_mlp_dopri5(t1d_ctx* c, const t1d_batch* b, const t1d_mlp* mlp, double* h_carry, int32_t* nfev,
                                      int n_steps, int minutes, void* stream)
{
    return rollout_mlp_dopri5_entry("t1d_rollout_mlp_dopri5", c, b, mlp, nullptr, nullptr, h_carry, nfev, n_steps, minutes, stream);
}

extern "C" int t1d_rollout_mlp_dopri5_bolus(t1d_ctx* c, const t1d_batch* b, const t1d_mlp* mlp, const t1d_meal_bolus* mb, double* h_carry,
                                            int32_t* nfev, int n_steps, int minutes, void* stream)
{
    const int rc = check_meal_bolus("t1d_rollout_mlp_dopri5_bolus", mb);
    if (rc) return rc;
    return rollout_mlp_dopri5_entry("t1d_rollout_mlp_dopri5_bolus", c, b, mlp, nullptr, mb, h_carry, nfev, n_steps, minutes, stream);
}

extern "C" int t1d_rollout_mlp_dopri5_rel(t1d_ctx* c, const t1d_batch* b, const t1d_mlp* mlp, const t1d_env_output* eo,
                                          const t1d_meal_bolus* mb, double* h_carry, int32_t* nfev, int n_steps, int minutes, void* stream)
{
    const int rc = check_env_output("t1d_rollout_mlp_dopri5_rel", eo, mb);
    if (rc) return rc;
    return rollout_mlp_dopri5_entry("t1d_rollout_mlp_dopri5_rel", c, b, mlp, eo, mb, h_carry, nfev, n_steps, minutes, stream);
}

// The policy alone (mlp_action_kernel, t1d_dopri5.hpp) or its features alone (mlp_features_kernel, t1d_policy.hpp), of
// the state as it is: nothing is stepped.  what: the name of the output in the messages.
// front: what the kernel takes between MlpArgs and the output, as a function of the dtype tag (t1d_mlp_action_rel: the pair).
template <typename K, typename... F>
static int launch_mlp_alone(const char* who, const char* what, t1d_ctx* c, const t1d_batch* b, const t1d_mlp* mlp, void* out, void* stream, K kernel,
                            F... front)
{
    int rc = check_batch(who, c, b, false);
    if (rc) return rc;
    if (!out) return fail(T1D_E_INVALID, std::string(who) + ": " + what + " is NULL");
    int cols = 0;
    rc = check_mlp(who, b, mlp, &cols);
    if (rc) return rc;
    by_dtype(b->dtype, [&](auto t) {
        using T = decltype(t);
        MlpArgs<T> ma = make_mlp<T>(mlp, 0);
        ma.cols = cols;
        const Shape sh = shape_mlp_alone<T>(c, b->n, cols);
        hipLaunchKernelGGL(kernel(t), dim3(sh.grid), dim3(sh.threads), sh.lds, (hipStream_t)stream, make_args<T>(c, b, 1, 1), ma, front(t)..., (T*)out);
    });
    T1D_HIP(hipGetLastError());
    return T1D_OK;
}

extern "C" int t1d_mlp_action(t1d_ctx* c, const t1d_batch* b, const t1d_mlp* mlp, void* action, void* stream)
{
    return launch_mlp_alone("t1d_mlp_action", "action", c, b, mlp, action, stream, [](auto t) { return mlp_action_kernel<decltype(t)>; });
}

extern "C" int t1d_mlp_action_rel(t1d_ctx* c, const t1d_batch* b, const t1d_mlp* mlp, const t1d_env_output* eo, void* action, void* stream)
{
    const int rc = check_env_output("t1d_mlp_action_rel", eo, nullptr);
    if (rc) return rc;
    return launch_mlp_alone("t1d_mlp_action_rel", "action", c, b, mlp, action, stream, [](auto t) { return mlp_action_rel_kernel<decltype(t)>; },
                            [eo](auto t) { return make_env_out<decltype(t)>(eo); });
}

extern "C" int t1d_mlp_features(t1d_ctx* c, const t1d_batch* b, const t1d_mlp* mlp, void* feat, void* stream)
{
    return launch_mlp_alone("t1d_mlp_features", "feat", c, b, mlp, feat, stream, [](auto t) { return mlp_features_kernel<decltype(t)>; });
}

// The meal bolus alone (mlp_bolus_kernel, t1d_policy.hpp), beside t1d_mlp_action: t1d_mlp_action's checks, one lane per env,
// no LDS.
extern "C" int t1d_mlp_bolus(t1d_ctx* c, const t1d_batch* b, const t1d_mlp* mlp, const t1d_meal_bolus* mb, void* bolus, void* stream)
{
    const char* who = "t1d_mlp_bolus";
    int rc = check_meal_bolus(who, mb);
    if (rc) return rc;
    rc = check_batch(who, c, b, false);
    if (rc) return rc;
    if (!bolus) return fail(T1D_E_INVALID, std::string(who) + ": bolus is NULL");
    int cols = 0;
    rc = check_mlp(who, b, mlp, &cols);
    if (rc) return rc;
    by_dtype(b->dtype, [&](auto t) {
        using T = decltype(t);
        hipLaunchKernelGGL(mlp_bolus_kernel<T>, dim3((unsigned)((b->n + T1D_POLICY_THREADS - 1) / T1D_POLICY_THREADS)), dim3(T1D_POLICY_THREADS),
                           0, (hipStream_t)stream, make_args<T>(c, b, 1, 1), make_mlp<T>(mlp, 0), make_bolus<T>(mb), (T*)bolus);
    });
    T1D_HIP(hipGetLastError());
    return T1D_OK;
}

// the six meal windows of RandomScenario.create_scenario (scenario_gen.py:38-45) as the kernels take them
static MealSlots meal_slots()
{
    MealSlots ms;
    const double prob[6] = {0.95, 0.3, 0.95, 0.3, 0.95, 0.3};          // scenario_gen.py:38-45
    const double lb[6] = {5, 9, 10, 14, 16, 20}, ub[6] = {9, 10, 14, 16, 20, 23}, mu[6] = {7, 9.5, 12, 15, 18, 21.5};
    const double sd[6] = {60, 30, 60, 30, 60, 30}, amu[6] = {45, 10, 70, 10, 80, 10}, asd[6] = {10, 5, 10, 5, 10, 5};
    for (int k = 0; k < 6; ++k) {
        ms.prob[k] = prob[k]; ms.lb[k] = lb[k] * 60.0; ms.ub[k] = ub[k] * 60.0; ms.mu[k] = mu[k] * 60.0;
        ms.sd[k] = sd[k]; ms.amu[k] = amu[k]; ms.asd[k] = asd[k];
        const double ca = 0.5 * std::erfc(-((ms.lb[k] - ms.mu[k]) / sd[k]) / std::sqrt(2.0));
        const double cb = 0.5 * std::erfc(-((ms.ub[k] - ms.mu[k]) / sd[k]) / std::sqrt(2.0));
        ms.cdf_a[k] = ca; ms.cdf_w[k] = cb - ca;
    }
    return ms;
}

template <typename T>
static RestartArgs<T> make_restart(const t1d_restart* r)
{
    RestartArgs<T> ra;
    ra.days = r->days; ra.random_init_bg = r->random_init_bg; ra.reset_outputs = r->reset_outputs;
    ra.meal_time = r->meal_time; ra.meal_amt = (T*)r->meal_amt; ra.start_minute = r->start_minute; ra.h_carry = r->h_carry;
    ra.terminal_cgm = (T*)r->terminal_cgm; ra.ep_return = (T*)r->ep_return; ra.ep_length = r->ep_length;
    ra.last_return = (T*)r->last_return; ra.last_length = r->last_length;
    return ra;
}

template <typename T>
static void launch_restart(const t1d_ctx* c, const t1d_batch* b, const uint8_t* mask, const t1d_restart* r, hipStream_t s)
{
    const RestartArgs<T> ra = make_restart<T>(r);
    const uint8_t* m = mask ? mask : b->done;
    if (c->restart_compact) {
        const int64_t per = (int64_t)kBlock * kRestartTile;
        hipLaunchKernelGGL((restart_kernel<true, T>), dim3((unsigned)((b->n + per - 1) / per)), dim3(kBlock), 0, s,
                           make_args<T>(c, b, 1, 1), ra, m, meal_slots());
    } else {
        hipLaunchKernelGGL((restart_kernel<false, T>), grid_for(b->n), dim3(kBlock), 0, s, make_args<T>(c, b, 1, 1), ra, m, meal_slots());
    }
}

// what a batch and a t1d_restart must be for an env to be restarted on the device; needs no device
static int check_restart(const char* who, const t1d_batch* b, const t1d_restart* r)
{
    const std::string w = std::string(who) + ": ";
    if (!b) return fail(T1D_E_INVALID, w + "batch is NULL");
    if (!r) return fail(T1D_E_INVALID, w + "restart is NULL");
    if (r->days < 1 || r->days > 10000) return fail(T1D_E_INVALID, w + "days out of range");
    if (r->reserved != 0) return fail(T1D_E_INVALID, w + "reserved must be 0");
    if (b->normals || b->n_normals != 0)
        return fail(T1D_E_INVALID, w + "host-normals batches have no per-episode source on the device");
    if (b->x0_override) return fail(T1D_E_INVALID, w + "x0_override has no per-episode source on the device");
    if (!r->meal_time || !r->meal_amt || !r->start_minute)
        return fail(T1D_E_INVALID, w + "meal_time / meal_amt / start_minute is NULL");
    if (r->meal_time != b->meal_time || r->meal_amt != b->meal_amt)
        return fail(T1D_E_INVALID, w + "meal_time / meal_amt must be the tables the batch names");
    if (b->n_meals != 6 * (r->days + 1)) return fail(T1D_E_INVALID, w + "batch.n_meals must be 6 (days + 1)");
    if (!b->episode) return fail(T1D_E_INVALID, w + "batch.episode is NULL (the episode index keys the new episode)");
    if (!r->ep_return != !r->ep_length) return fail(T1D_E_INVALID, w + "ep_return and ep_length go together");
    if ((r->last_return || r->last_length) && !r->ep_return)
        return fail(T1D_E_INVALID, w + "last_return / last_length need ep_return and ep_length");
    return T1D_OK;
}

extern "C" int t1d_restart_done(t1d_ctx* c, const t1d_batch* b, const uint8_t* mask, const t1d_restart* r, void* stream)
{
    // what needs no device is checked first, so that a bad call is refused on any machine
    int rc = check_restart("t1d_restart_done", b, r);
    if (rc) return rc;
    if (r->h_carry && b->dtype != T1D_F64) return fail(T1D_E_INVALID, "t1d_restart_done: h_carry belongs to fp64 batches");
    rc = check_batch("t1d_restart_done", c, b, false);
    if (rc) return rc;
    by_dtype(b->dtype, [&](auto t) { launch_restart<decltype(t)>(c, b, mask, r, (hipStream_t)stream); });
    T1D_HIP(hipGetLastError());
    return T1D_OK;
}

// ---- t1d_collect_mlp (t1d_policy.hpp) ---------------------------------------------------------------------------------
template <typename T>
static CollectFn<T> mlp_collect_fn(int variant)
{
    return by_variant<T>(variant, [](auto v) -> CollectFn<T> { return mlp_collect_kernel<decltype(v)::value, T>; });
}

template <typename T>
static CollectArgs<T> make_collect(const t1d_ctx* c, const t1d_collect* g)
{
    CollectArgs<T> ga;
    ga.explore_seed = g->explore_seed; ga.sigma = (const T*)g->sigma; ga.on_done = g->on_done;
    ga.reward_trace = (T*)g->reward_trace; ga.done_trace = g->done_trace; ga.eps_trace = (T*)g->eps_trace; ga.feat_trace = (T*)g->feat_trace;
    ga.slots = c->d_slots;
    return ga;
}

// ---- t1d_time_limit: the limit of t1d_collect_mlp_limit (LimitArgs, t1d_policy.hpp) ---------------------------------------
// needs no device.  n_steps * minutes <= max_minutes: an env is cut at most once per call, so cut_feat has one column per env
static int check_time_limit(const char* who, const t1d_collect* g, const t1d_time_limit* lim, int n_steps, int minutes)
{
    const std::string w = std::string(who) + ": ";
    if (!lim) return fail(T1D_E_INVALID, w + "limit is NULL");
    if (lim->max_minutes < 1) return fail(T1D_E_INVALID, w + "limit.max_minutes < 1");
    if (lim->reserved != 0) return fail(T1D_E_INVALID, w + "limit.reserved must be 0");
    if (g && g->on_done != T1D_COLLECT_RESTART) return fail(T1D_E_INVALID, w + "a time limit needs on_done = T1D_COLLECT_RESTART (a cut env restarts)");
    if (n_steps > 0 && minutes > 0 && (int64_t)n_steps * minutes > lim->max_minutes)
        return fail(T1D_E_INVALID, w + "n_steps * minutes must not exceed limit.max_minutes (an env is cut at most once per call)");
    return T1D_OK;
}

template <typename T>
static LimitArgs<T> make_limit(const t1d_time_limit* lim)
{
    return LimitArgs<T>{lim->max_minutes, lim->cut_trace, (T*)lim->cut_feat};
}

template <typename T> using CollectLimitFn = KernelFn<T, MlpArgs<T>, CollectArgs<T>, RestartArgs<T>, EnvOutArgs<T>, BolusArgs<T>, LimitArgs<T>>;
template <typename T>
static CollectLimitFn<T> mlp_collect_limit_fn(int variant)
{
    return by_variant<T>(variant, [](auto v) -> CollectLimitFn<T> { return mlp_collect_limit_kernel<decltype(v)::value, T>; });
}

// mb == NULL: t1d_collect_mlp; with mb the same kernel family with the bolus switched on (t1d_collect_mlp_bolus); with eo the
// relative policy's family, with or without mb (t1d_collect_mlp_rel); with lim the time limit's family, with or without either
// (t1d_collect_mlp_limit)
template <typename T>
static int run_collect_mlp(const char* who, t1d_ctx* c, const t1d_batch* b, const t1d_mlp* m, const t1d_collect* g, const t1d_env_output* eo,
                           const t1d_meal_bolus* mb, const t1d_time_limit* lim, Plan p, int cols, int n_steps, int minutes, int n_sub,
                           hipStream_t s)
{
    MlpArgs<T> ma = make_mlp<T>(m, n_steps);
    const int rc = shape_mlp<T>(who, c, b, cols, p, ma);
    if (rc) return rc;
    const RestartArgs<T> ra = g->on_done == T1D_COLLECT_RESTART ? make_restart<T>(g->restart) : RestartArgs<T>{};
    if (lim)
        return launch(c, b, p, minutes, n_sub, s, mlp_collect_limit_fn<T>(p.variant), ma, make_collect<T>(c, g), ra,
                      eo ? make_env_out<T>(eo) : EnvOutArgs<T>{}, make_bolus_or_none<T>(mb), make_limit<T>(lim));
    if (eo)
        return launch(c, b, p, minutes, n_sub, s, mlp_collect_rel_fn<T>(p.variant), ma, make_collect<T>(c, g), ra, make_env_out<T>(eo),
                      make_bolus_or_none<T>(mb));
    if (!mb) return launch(c, b, p, minutes, n_sub, s, mlp_collect_fn<T>(p.variant), ma, make_collect<T>(c, g), ra);
    return launch(c, b, p, minutes, n_sub, s, mlp_collect_bolus_fn<T>(p.variant), ma, make_collect<T>(c, g), ra, make_bolus<T>(mb));
}

// what a t1d_collect must be, for both collectors, and the policy beside it (checked by check_mlp; NULL is left to
// that); needs no device.  h_carry: the exact mode's array (NULL: fixed-step)
static int check_collect(const char* who, const t1d_batch* b, const t1d_mlp* m, const t1d_collect* g, const double* h_carry)
{
    const std::string w = std::string(who) + ": ";
    if (!g) return fail(T1D_E_INVALID, w + "collect is NULL");
    if (g->on_done != T1D_COLLECT_CONTINUE && g->on_done != T1D_COLLECT_RESTART)
        return fail(T1D_E_INVALID, w + "on_done must be T1D_COLLECT_CONTINUE or T1D_COLLECT_RESTART");
    if (g->reserved != 0) return fail(T1D_E_INVALID, w + "reserved must be 0");
    if (g->on_done == T1D_COLLECT_RESTART) {
        if (!g->restart) return fail(T1D_E_INVALID, w + "on_done = T1D_COLLECT_RESTART needs restart");
        int rr = check_restart(who, b, g->restart);
        if (rr) return rr;
        if (!h_carry && g->restart->h_carry)
            return fail(T1D_E_INVALID, w + "restart.h_carry must be NULL (the exact mode's collector is t1d_collect_mlp_dopri5)");
        if (h_carry && g->restart->h_carry && g->restart->h_carry != h_carry)
            return fail(T1D_E_INVALID, w + "restart.h_carry must be NULL or the call's h_carry");
        // a restarted env's time-of-day features follow its new start: the array the restart writes is the one the
        // policy reads
        if (m && m->start_minute && m->start_minute != g->restart->start_minute)
            return fail(T1D_E_INVALID, w + "mlp.start_minute must be restart.start_minute (or NULL)");
    }
    return T1D_OK;
}

static int collect_mlp_entry(const char* who, t1d_ctx* c, const t1d_batch* b, const t1d_mlp* mlp, const t1d_collect* g,
                             const t1d_env_output* eo, const t1d_meal_bolus* mb, int n_steps, int minutes, int n_sub, void* stream,
                             const t1d_time_limit* lim = nullptr)
{
    int rc = check_collect(who, b, mlp, g, nullptr);
    if (rc) return rc;
    rc = check_closed_loop(who, c, b, n_steps);
    if (rc) return rc;
    int cols = 0;
    rc = check_mlp(who, b, mlp, &cols);
    if (rc) return rc;
    Plan p;
    rc = plan_and_tables(who, c, b, minutes, n_sub, true, &p, true);
    if (rc) return rc;
    hipStream_t s = (hipStream_t)stream;
    rc = p.f64 ? run_collect_mlp<double>(who, c, b, mlp, g, eo, mb, lim, p, cols, n_steps, minutes, n_sub, s)
               : run_collect_mlp<float>(who, c, b, mlp, g, eo, mb, lim, p, cols, n_steps, minutes, n_sub, s);
    if (rc) return rc;
    T1D_HIP(hipGetLastError());
    return T1D_OK;
}

extern "C" int t1d_collect_mlp(t1d_ctx* c, const t1d_batch* b, const t1d_mlp* mlp, const t1d_collect* g, int n_steps, int minutes,
                               int n_sub, void* stream)
{
    return collect_mlp_entry("t1d_collect_mlp", c, b, mlp, g, nullptr, nullptr, n_steps, minutes, n_sub, stream);
}

extern "C" int t1d_collect_mlp_bolus(t1d_ctx* c, const t1d_batch* b, const t1d_mlp* mlp, const t1d_collect* g, const t1d_meal_bolus* mb,
                                     int n_steps, int minutes, int n_sub, void* stream)
{
    const int rc = check_meal_bolus("t1d_collect_mlp_bolus", mb);
    if (rc) return rc;
    return collect_mlp_entry("t1d_collect_mlp_bolus", c, b, mlp, g, nullptr, mb, n_steps, minutes, n_sub, stream);
}

extern "C" int t1d_collect_mlp_rel(t1d_ctx* c, const t1d_batch* b, const t1d_mlp* mlp, const t1d_collect* g, const t1d_env_output* eo,
                                   const t1d_meal_bolus* mb, int n_steps, int minutes, int n_sub, void* stream)
{
    const int rc = check_env_output("t1d_collect_mlp_rel", eo, mb);
    if (rc) return rc;
    return collect_mlp_entry("t1d_collect_mlp_rel", c, b, mlp, g, eo, mb, n_steps, minutes, n_sub, stream);
}

// the three calls above under a time limit (mlp_collect_limit_kernel): their checks under this call's name, then the limit's
extern "C" int t1d_collect_mlp_limit(t1d_ctx* c, const t1d_batch* b, const t1d_mlp* mlp, const t1d_collect* g, const t1d_env_output* eo,
                                     const t1d_meal_bolus* mb, const t1d_time_limit* lim, int n_steps, int minutes, int n_sub, void* stream)
{
    const char* who = "t1d_collect_mlp_limit";
    int rc = eo ? check_env_output(who, eo, mb) : mb ? check_meal_bolus(who, mb) : T1D_OK;
    if (rc) return rc;
    rc = check_time_limit(who, g, lim, n_steps, minutes);
    if (rc) return rc;
    return collect_mlp_entry(who, c, b, mlp, g, eo, mb, n_steps, minutes, n_sub, stream, lim);
}

// ---- t1d_collect_pid / t1d_collect_bb (ctrl_collect_kernel, t1d_policy.hpp) ----------------------------------------------
template <typename T> using CtrlCollectFn = KernelFn<T, PidArgs<T>, MlpArgs<T>, CollectArgs<T>, RestartArgs<T>>;
template <typename T>
static CtrlCollectFn<T> ctrl_collect_fn(int variant)
{
    return by_variant<T>(variant, [](auto v) -> CtrlCollectFn<T> { return ctrl_collect_kernel<decltype(v)::value, T>; });
}

// the t1d_mlp of a controller's collector with nothing but the fields that are read: history, the four feature scales, the
// two windows, prev_meal, start_minute and action_trace.  No network (n_layers = 0), no accumulators, no other trace.
static t1d_mlp features_only(const t1d_mlp* m)
{
    t1d_mlp f = {};
    f.history = m->history;
    f.cgm_mean = m->cgm_mean; f.cgm_scale = m->cgm_scale; f.ins_scale = m->ins_scale; f.cho_scale = m->cho_scale;
    f.cgm_hist = m->cgm_hist; f.ins_hist = m->ins_hist; f.prev_meal = m->prev_meal; f.start_minute = m->start_minute;
    f.action_trace = m->action_trace;
    return f;
}

template <typename T> using CtrlCollectLimitFn = KernelFn<T, PidArgs<T>, MlpArgs<T>, CollectArgs<T>, RestartArgs<T>, LimitArgs<T>>;
template <typename T>
static CtrlCollectLimitFn<T> ctrl_collect_limit_fn(int variant)
{
    return by_variant<T>(variant, [](auto v) -> CtrlCollectLimitFn<T> { return ctrl_collect_limit_kernel<decltype(v)::value, T>; });
}

// lim == NULL: t1d_collect_pid / t1d_collect_bb; with lim the time limit's family (t1d_collect_pid_limit / t1d_collect_bb_limit)
template <typename T>
static int run_collect_ctrl(const char* who, t1d_ctx* c, const t1d_batch* b, const PidArgs<T>& pa, const t1d_mlp* feat, const t1d_collect* g,
                            const t1d_time_limit* lim, Plan p, int minutes, int n_sub, hipStream_t s)
{
    const t1d_mlp fm = features_only(feat);
    MlpArgs<T> fa = make_mlp<T>(&fm, pa.n_steps);
    // a wave's columns: the two windows and the F = 2 H + 3 features, no activations
    const int rc = shape_mlp<T>(who, c, b, 4 * fm.history + 3, p, fa);
    if (rc) return rc;
    const RestartArgs<T> ra = g->on_done == T1D_COLLECT_RESTART ? make_restart<T>(g->restart) : RestartArgs<T>{};
    if (lim) return launch(c, b, p, minutes, n_sub, s, ctrl_collect_limit_fn<T>(p.variant), pa, fa, make_collect<T>(c, g), ra, make_limit<T>(lim));
    return launch(c, b, p, minutes, n_sub, s, ctrl_collect_fn<T>(p.variant), pa, fa, make_collect<T>(c, g), ra);
}

// a collector under the PID controller pid or the basal-bolus controller bb (the other one NULL).  What needs no device is
// checked first, so that a bad call is refused on any machine.
static int launch_collect_ctrl(const char* who, t1d_ctx* c, const t1d_batch* b, const t1d_pid* pid, const t1d_bb* bb, const t1d_mlp* feat,
                               const t1d_collect* g, int n_steps, int minutes, int n_sub, void* stream, const t1d_time_limit* lim = nullptr,
                               bool limited = false)
{
    const std::string w = std::string(who) + ": ";
    if (!feat) return fail(T1D_E_INVALID, w + "feat is NULL");
    if (feat->history < 1 || feat->history > kMlpMaxHistory) return fail(T1D_E_INVALID, w + "history must be in [1, 12]");
    if (!feat->cgm_hist || !feat->ins_hist || !feat->prev_meal) return fail(T1D_E_INVALID, w + "cgm_hist / ins_hist / prev_meal must be set");
    int rc = check_collect(who, b, feat, g, nullptr);
    if (rc) return rc;
    if (g->sigma || g->eps_trace) return fail(T1D_E_INVALID, w + "sigma and eps_trace must be NULL (a controller has no exploration noise)");
    if (n_steps < 1) return fail(T1D_E_INVALID, w + "n_steps < 1");
    if (b && b->cho) return fail(T1D_E_INVALID, w + "dense cho is not supported, use the meal table");
    if (minutes < 1 || minutes > 100000) return fail(T1D_E_INVALID, w + "minutes out of range");
    if (n_sub < 1 || n_sub > 4096) return fail(T1D_E_INVALID, w + "n_sub out of range");
    if (limited) {                              // the *_limit calls: the sibling's checks that need no device, then the limit's
        rc = check_time_limit(who, g, lim, n_steps, minutes);
        if (rc) return rc;
    }
    rc = check_closed_loop(who, c, b, n_steps);
    if (rc) return rc;
    Plan p;
    rc = plan_and_tables(who, c, b, minutes, n_sub, true, &p, true);
    if (rc) return rc;
    hipStream_t s = (hipStream_t)stream;
    if (p.f64) rc = run_collect_ctrl<double>(who, c, b, pid ? make_pid<double>(pid, n_steps) : make_bb<double>(bb, n_steps), feat, g, lim, p, minutes, n_sub, s);
    else rc = run_collect_ctrl<float>(who, c, b, pid ? make_pid<float>(pid, n_steps) : make_bb<float>(bb, n_steps), feat, g, lim, p, minutes, n_sub, s);
    if (rc) return rc;
    T1D_HIP(hipGetLastError());
    return T1D_OK;
}

extern "C" int t1d_collect_pid(t1d_ctx* c, const t1d_batch* b, const t1d_pid* pid, const t1d_mlp* feat, const t1d_collect* g,
                               int n_steps, int minutes, int n_sub, void* stream)
{
    if (!pid || !pid->integ || !pid->prev) return fail(T1D_E_INVALID, "t1d_collect_pid: pid state is NULL");
    return launch_collect_ctrl("t1d_collect_pid", c, b, pid, nullptr, feat, g, n_steps, minutes, n_sub, stream);
}

extern "C" int t1d_collect_bb(t1d_ctx* c, const t1d_batch* b, const t1d_bb* bb, const t1d_mlp* feat, const t1d_collect* g,
                              int n_steps, int minutes, int n_sub, void* stream)
{
    if (!bb || !bb->basal || !bb->cr || !bb->cf || !bb->prev_meal)
        return fail(T1D_E_INVALID, "t1d_collect_bb: basal / cr / cf / prev_meal must be set");
    return launch_collect_ctrl("t1d_collect_bb", c, b, nullptr, bb, feat, g, n_steps, minutes, n_sub, stream);
}

// the two calls above under a time limit (ctrl_collect_limit_kernel): their checks under this call's name, then the limit's
extern "C" int t1d_collect_pid_limit(t1d_ctx* c, const t1d_batch* b, const t1d_pid* pid, const t1d_mlp* feat, const t1d_collect* g,
                                     const t1d_time_limit* lim, int n_steps, int minutes, int n_sub, void* stream)
{
    if (!pid || !pid->integ || !pid->prev) return fail(T1D_E_INVALID, "t1d_collect_pid_limit: pid state is NULL");
    return launch_collect_ctrl("t1d_collect_pid_limit", c, b, pid, nullptr, feat, g, n_steps, minutes, n_sub, stream, lim, true);
}

extern "C" int t1d_collect_bb_limit(t1d_ctx* c, const t1d_batch* b, const t1d_bb* bb, const t1d_mlp* feat, const t1d_collect* g,
                                    const t1d_time_limit* lim, int n_steps, int minutes, int n_sub, void* stream)
{
    if (!bb || !bb->basal || !bb->cr || !bb->cf || !bb->prev_meal)
        return fail(T1D_E_INVALID, "t1d_collect_bb_limit: basal / cr / cf / prev_meal must be set");
    return launch_collect_ctrl("t1d_collect_bb_limit", c, b, nullptr, bb, feat, g, n_steps, minutes, n_sub, stream, lim, true);
}

// The exact mode's collector (dopri5_mlp_collect_kernel, t1d_dopri5.hpp): the checks of t1d_rollout_mlp_dopri5 and of
// t1d_collect_mlp, then one launch in the shape of t1d_rollout_mlp_dopri5.
// limited: t1d_collect_mlp_dopri5_limit (dopri5_mlp_collect_limit_kernel), the same checks under that name, then the limit's.
static int collect_mlp_dopri5_entry(const char* who, t1d_ctx* c, const t1d_batch* b, const t1d_mlp* mlp, const t1d_collect* g,
                                    const t1d_time_limit* lim, bool limited, double* h_carry, int32_t* nfev, int n_steps, int minutes,
                                    void* stream)
{
    int rc = check_dopri5(who, c, b, h_carry, n_steps, minutes);
    if (rc) return rc;
    rc = check_collect(who, b, mlp, g, h_carry);
    if (rc) return rc;
    int cols = 0;
    rc = check_mlp(who, b, mlp, &cols);
    if (rc) return rc;
    if (limited) {
        rc = check_time_limit(who, g, lim, n_steps, minutes);
        if (rc) return rc;
    }
    MlpArgs<double> ma = make_mlp<double>(mlp, n_steps);
    ma.cols = cols;
    RestartArgs<double> ra = g->on_done == T1D_COLLECT_RESTART ? make_restart<double>(g->restart) : RestartArgs<double>{};
    if (g->on_done == T1D_COLLECT_RESTART) ra.h_carry = h_carry;      // the env's predicted step is part of what restarts
    if (limited)
        return launch_mlp_dopri5(who, c, b, cols, minutes, stream, dopri5_mlp_collect_limit_kernel, ma, make_collect<double>(c, g), ra,
                                 make_limit<double>(lim), (const double*)c->d_raw64, h_carry, nfev);
    return launch_mlp_dopri5(who, c, b, cols, minutes, stream, dopri5_mlp_collect_kernel, ma, make_collect<double>(c, g), ra,
                             (const double*)c->d_raw64, h_carry, nfev);
}

extern "C" int t1d_collect_mlp_dopri5(t1d_ctx* c, const t1d_batch* b, const t1d_mlp* mlp, const t1d_collect* g, double* h_carry,
                                      int32_t* nfev, int n_steps, int minutes, void* stream)
{
    return collect_mlp_dopri5_entry("t1d_collect_mlp_dopri5", c, b, mlp, g, nullptr, false, h_carry, nfev, n_steps, minutes, stream);
}

extern "C" int t1d_collect_mlp_dopri5_limit(t1d_ctx* c, const t1d_batch* b, const t1d_mlp* mlp, const t1d_collect* g,
                                            const t1d_time_limit* lim, double* h_carry, int32_t* nfev, int n_steps, int minutes,
                                            void* stream)
{
    return collect_mlp_dopri5_entry("t1d_collect_mlp_dopri5_limit", c, b, mlp, g, lim, true, h_carry, nfev, n_steps, minutes, stream);
}

// The exact mode's collectors under the PID controller pid or the basal-bolus controller bb, the other one NULL
// (dopri5_ctrl_collect_kernel, t1d_dopri5.hpp): what t1d_collect_pid asks of feat and collect, then what
// t1d_rollout_pid_dopri5 asks of the rest -- the batch's own checks last, so that a bad call is refused on any machine --
// then one launch in the shape of t1d_rollout_mlp_dopri5 with a wave's columns of ctrl_collect_kernel.
static int launch_collect_ctrl_dopri5(const char* who, t1d_ctx* c, const t1d_batch* b, const t1d_pid* pid, const t1d_bb* bb,
                                      const t1d_mlp* feat, const t1d_collect* g, double* h_carry, int32_t* nfev, int n_steps,
                                      int minutes, void* stream, const t1d_time_limit* lim = nullptr, bool limited = false)
{
    const std::string w = std::string(who) + ": ";
    if (!feat) return fail(T1D_E_INVALID, w + "feat is NULL");
    if (feat->history < 1 || feat->history > kMlpMaxHistory) return fail(T1D_E_INVALID, w + "history must be in [1, 12]");
    if (!feat->cgm_hist || !feat->ins_hist || !feat->prev_meal) return fail(T1D_E_INVALID, w + "cgm_hist / ins_hist / prev_meal must be set");
    if (!h_carry) return fail(T1D_E_INVALID, w + "h_carry is NULL");
    int rc = check_collect(who, b, feat, g, h_carry);
    if (rc) return rc;
    if (g->sigma || g->eps_trace) return fail(T1D_E_INVALID, w + "sigma and eps_trace must be NULL (a controller has no exploration noise)");
    rc = check_dopri5(who, c, b, h_carry, n_steps, minutes);
    if (rc) return rc;
    if (limited) {                              // the *_limit calls: the sibling's checks, then the limit's
        rc = check_time_limit(who, g, lim, n_steps, minutes);
        if (rc) return rc;
    }
    const PidArgs<double> pa = pid ? make_pid<double>(pid, n_steps) : make_bb<double>(bb, n_steps);
    const t1d_mlp fm = features_only(feat);
    MlpArgs<double> fa = make_mlp<double>(&fm, n_steps);
    const int cols = 4 * fm.history + 3;        // a wave's columns: the two windows and the F = 2 H + 3 features, no activations
    fa.cols = cols;
    RestartArgs<double> ra = g->on_done == T1D_COLLECT_RESTART ? make_restart<double>(g->restart) : RestartArgs<double>{};
    if (g->on_done == T1D_COLLECT_RESTART) ra.h_carry = h_carry;      // the env's predicted step is part of what restarts
    if (limited)
        return launch_mlp_dopri5(who, c, b, cols, minutes, stream, dopri5_ctrl_collect_limit_kernel, pa, fa, make_collect<double>(c, g), ra,
                                 make_limit<double>(lim), (const double*)c->d_raw64, h_carry, nfev);
    return launch_mlp_dopri5(who, c, b, cols, minutes, stream, dopri5_ctrl_collect_kernel, pa, fa, make_collect<double>(c, g), ra,
                             (const double*)c->d_raw64, h_carry, nfev);
}

extern "C" int t1d_collect_pid_dopri5(t1d_ctx* c, const t1d_batch* b, const t1d_pid* pid, const t1d_mlp* feat, const t1d_collect* g,
                                      double* h_carry, int32_t* nfev, int n_steps, int minutes, void* stream)
{
    if (!pid || !pid->integ || !pid->prev) return fail(T1D_E_INVALID, "t1d_collect_pid_dopri5: pid state is NULL");
    return launch_collect_ctrl_dopri5("t1d_collect_pid_dopri5", c, b, pid, nullptr, feat, g, h_carry, nfev, n_steps, minutes, stream);
}

extern "C" int t1d_collect_bb_dopri5(t1d_ctx* c, const t1d_batch* b, const t1d_bb* bb, const t1d_mlp* feat, const t1d_collect* g,
                                     double* h_carry, int32_t* nfev, int n_steps, int minutes, void* stream)
{
    if (!bb || !bb->basal || !bb->cr || !bb->cf || !bb->prev_meal)
        return fail(T1D_E_INVALID, "t1d_collect_bb_dopri5: bb is NULL, or basal / cr / cf / prev_meal is not set");
    return launch_collect_ctrl_dopri5("t1d_collect_bb_dopri5", c, b, nullptr, bb, feat, g, h_carry, nfev, n_steps, minutes, stream);
}

// the two calls above under a time limit (dopri5_ctrl_collect_limit_kernel)
extern "C" int t1d_collect_pid_dopri5_limit(t1d_ctx* c, const t1d_batch* b, const t1d_pid* pid, const t1d_mlp* feat, const t1d_collect* g,
                                            const t1d_time_limit* lim, double* h_carry, int32_t* nfev, int n_steps, int minutes,
                                            void* stream)
{
    if (!pid || !pid->integ || !pid->prev) return fail(T1D_E_INVALID, "t1d_collect_pid_dopri5_limit: pid state is NULL");
    return launch_collect_ctrl_dopri5("t1d_collect_pid_dopri5_limit", c, b, pid, nullptr, feat, g, h_carry, nfev, n_steps, minutes, stream,
                                      lim, true);
}

extern "C" int t1d_collect_bb_dopri5_limit(t1d_ctx* c, const t1d_batch* b, const t1d_bb* bb, const t1d_mlp* feat, const t1d_collect* g,
                                           const t1d_time_limit* lim, double* h_carry, int32_t* nfev, int n_steps, int minutes,
                                           void* stream)
{
    if (!bb || !bb->basal || !bb->cr || !bb->cf || !bb->prev_meal)
        return fail(T1D_E_INVALID, "t1d_collect_bb_dopri5_limit: bb is NULL, or basal / cr / cf / prev_meal is not set");
    return launch_collect_ctrl_dopri5("t1d_collect_bb_dopri5_limit", c, b, nullptr, bb, feat, g, h_carry, nfev, n_steps, minutes, stream,
                                      lim, true);
}

extern "C" int t1d_random_meals(int hip_device, uint64_t seed, int64_t env_offset, int64_t n, int dtype, int days,
                                const int32_t* start_minute_of_day, int start_scalar, int32_t* meal_time, void* meal_amt,
                                void* stream)
{
    if (!meal_time || !meal_amt) return fail(T1D_E_INVALID, "t1d_random_meals: output pointer is NULL");
    if (n < 1 || n > (int64_t)1 << 28) return fail(T1D_E_INVALID, "t1d_random_meals: n out of range");
    if (days < 1 || days > 10000) return fail(T1D_E_INVALID, "t1d_random_meals: days out of range");
    if (dtype != T1D_F64 && dtype != T1D_F32) return fail(T1D_E_INVALID, "t1d_random_meals: bad dtype");
    if (!start_minute_of_day && (start_scalar < 0 || start_scalar >= 1440))
        return fail(T1D_E_INVALID, "t1d_random_meals: start minute of day must be in [0, 1440)");
    T1D_HIP(hipSetDevice(hip_device));
    const MealSlots ms = meal_slots();
    by_dtype(dtype, [&](auto t) {
        using T = decltype(t);
        hipLaunchKernelGGL(random_meals_kernel<T>, grid_for(n), dim3(kBlock), 0, (hipStream_t)stream, seed, env_offset, n, days,
                           start_minute_of_day, start_scalar, meal_time, (T*)meal_amt, ms);
    });
    T1D_HIP(hipGetLastError());
    return T1D_OK;
}

extern "C" int t1d_outcome_stats(int hip_device, int dtype, int64_t n, int64_t n_rows, const void* bg_trace,
                                 const t1d_outcome* out, void* stream)
{
    if (!bg_trace || !out) return fail(T1D_E_INVALID, "t1d_outcome_stats: NULL argument");
    if (n < 1 || n > (int64_t)1 << 28 || n_rows < 1) return fail(T1D_E_INVALID, "t1d_outcome_stats: n / n_rows out of range");
    if (dtype != T1D_F64 && dtype != T1D_F32) return fail(T1D_E_INVALID, "t1d_outcome_stats: bad dtype");
    if (out->risk_trace && out->chunk < 1) return fail(T1D_E_INVALID, "t1d_outcome_stats: chunk < 1");
    if ((out->pct || out->zone) && !(out->q_lo >= 0.0 && out->q_lo <= 100.0 && out->q_hi >= 0.0 && out->q_hi <= 100.0))
        return fail(T1D_E_INVALID, "t1d_outcome_stats: percentiles must be in [0, 100]");
    T1D_HIP(hipSetDevice(hip_device));
    const int chunk = out->chunk > 0 ? out->chunk : 60;
    by_dtype(dtype, [&](auto t) {
        using T = decltype(t);
        hipLaunchKernelGGL(outcome_kernel<T>, grid_for(n), dim3(kBlock), 0, (hipStream_t)stream, n, n_rows, (const T*)bg_trace, out->counts,
                           (T*)out->pct, out->zone, (T*)out->risk_trace, out->q_lo, out->q_hi, chunk);
    });
    T1D_HIP(hipGetLastError());
    return T1D_OK;
}

// How t1d_mlp_grad cuts the work: a tile is one 64-env chunk of a policy in one row, a policy's tiles are numbered row by
// row, and one wave takes tiles_per_wave consecutive ones and writes one partial sum.  From the shapes alone (include/t1d.h).
// The listed calls (t1d_mlp_grad_tiles, t1d_mlp_loss_tiles) cut the n_tiles positions of a policy's list row by the same rule:
// positions is what the waves walk, tiles for a plain call (n_tiles = 0).
struct GradPartition { int64_t chunks, tiles, tiles_per_wave, waves_per_policy, positions; };
static bool grad_partition(const t1d_mlp* m, int64_t n_rows, GradPartition* gp, int64_t n_tiles = 0)
{
    gp->chunks = m->envs_per_policy / 64;
    if (n_rows > INT_MAX / gp->chunks) return false;
    gp->tiles = gp->chunks * n_rows;
    if (n_tiles > INT_MAX / m->n_policies) return false;
    gp->positions = n_tiles ? n_tiles : gp->tiles;
    gp->tiles_per_wave = std::max<int64_t>(1, (m->n_policies * gp->positions + kGradMaxWaves - 1) / kGradMaxWaves);
    gp->waves_per_policy = (gp->positions + gp->tiles_per_wave - 1) / gp->tiles_per_wave;
    return m->n_policies * gp->waves_per_policy <= INT_MAX;
}

// n_tiles: NULL for a plain call, else the n_tiles of a listed one
static int check_mlp_grad(const char* who, int dtype, int64_t n, const t1d_mlp* mlp, int64_t n_rows, GradPartition* gp,
                          const int64_t* n_tiles = nullptr)
{
    const std::string w = std::string(who) + ": ";
    if (dtype != T1D_F64 && dtype != T1D_F32) return fail(T1D_E_INVALID, w + "bad dtype");
    if (n < 1 || n > (int64_t)1 << 28) return fail(T1D_E_INVALID, w + "n out of range");
    if (n_rows < 1) return fail(T1D_E_INVALID, w + "n_rows < 1");
    if (n_tiles && *n_tiles < 1) return fail(T1D_E_INVALID, w + "n_tiles < 1");
    int cols = 0;
    const int rc = check_mlp_net(who, n, mlp, &cols, false);
    if (rc) return rc;
    if (!grad_partition(mlp, n_rows, gp)) return fail(T1D_E_INVALID, w + "n_rows is too large");
    if (n_tiles && !grad_partition(mlp, n_rows, gp, *n_tiles)) return fail(T1D_E_INVALID, w + "n_policies * n_tiles is too large");
    return T1D_OK;
}

// the list of a listed call
static int check_tile_list(const char* who, const t1d_tile_list* list)
{
    const std::string w = std::string(who) + ": ";
    if (!list) return fail(T1D_E_INVALID, w + "the tile list is NULL");
    if (!list->tiles) return fail(T1D_E_INVALID, w + "tiles is NULL");
    if (list->n_tiles < 1) return fail(T1D_E_INVALID, w + "n_tiles < 1");
    return T1D_OK;
}

static int64_t grad_workspace_bytes(const t1d_mlp* m, int dtype, const GradPartition& gp)
{
    return m->n_policies * gp.waves_per_policy * m->n_params * (int64_t)(dtype == T1D_F64 ? sizeof(double) : sizeof(float));
}

// t1d_mlp_loss: t1d_mlp_grad's partition and gradient partials, and one partial [4] of doubles per wave behind them
static int64_t loss_stats_offset(const t1d_mlp* m, int dtype, const GradPartition& gp)
{
    return (grad_workspace_bytes(m, dtype, gp) + 7) / 8 * 8;
}

static int64_t loss_workspace_bytes(const t1d_mlp* m, int dtype, const GradPartition& gp)
{
    return loss_stats_offset(m, dtype, gp) + m->n_policies * gp.waves_per_policy * 4 * (int64_t)sizeof(double);
}

// the workspace of a call of these shapes; the weights themselves are not needed to size it
static int64_t mlp_workspace(const char* who, const t1d_mlp* mlp, int dtype, int64_t n, int64_t n_rows,
                             int64_t (*bytes)(const t1d_mlp*, int, const GradPartition&), const int64_t* n_tiles = nullptr)
{
    if (!mlp) return fail(T1D_E_INVALID, std::string(who) + ": mlp is NULL");
    t1d_mlp m = *mlp;
    if (!m.params) m.params = &m;
    GradPartition gp;
    const int rc = check_mlp_grad(who, dtype, n, &m, n_rows, &gp, n_tiles);
    if (rc) return rc;
    return bytes(&m, dtype, gp);
}

extern "C" int64_t t1d_mlp_grad_workspace(const t1d_mlp* mlp, int dtype, int64_t n, int64_t n_rows)
{
    return mlp_workspace("t1d_mlp_grad_workspace", mlp, dtype, n, n_rows, grad_workspace_bytes);
}

extern "C" int64_t t1d_mlp_loss_workspace(const t1d_mlp* mlp, int dtype, int64_t n, int64_t n_rows)
{
    return mlp_workspace("t1d_mlp_loss_workspace", mlp, dtype, n, n_rows, loss_workspace_bytes);
}

// the listed calls: the partition depends on n_tiles alone, so the size does not ask for n_rows
extern "C" int64_t t1d_mlp_grad_tiles_workspace(const t1d_mlp* mlp, int dtype, int64_t n, int64_t n_tiles)
{
    return mlp_workspace("t1d_mlp_grad_tiles_workspace", mlp, dtype, n, 1, grad_workspace_bytes, &n_tiles);
}

extern "C" int64_t t1d_mlp_loss_tiles_workspace(const t1d_mlp* mlp, int dtype, int64_t n, int64_t n_tiles)
{
    return mlp_workspace("t1d_mlp_loss_tiles_workspace", mlp, dtype, n, 1, loss_workspace_bytes, &n_tiles);
}

// The LDS of one wave of mlp_grad_kernel (t1d_policy_grad.hpp): act_rows = F + the hidden widths of activations; with
// grad one row of ones and one delta row per unit of every layer behind them.  Every row a variant of the kernel adds
// must be counted here.  From the policy alone: checked on the CPU by tests/dispatch_plan_driver.cpp.
static size_t grad_wave_lds(const t1d_mlp* m, bool with_grad, size_t word, int* act_rows)
{
    int rows = 2 * m->history + 3, deltas = 0;
    for (int l = 0; l < m->n_layers; ++l) { if (l + 1 < m->n_layers) rows += m->width[l]; deltas += m->width[l]; }
    *act_rows = rows;
    return (size_t)(with_grad ? rows + 1 + deltas : rows) * 64 * word;      // without grad only the activations are kept
}

// Above 64 KiB the kernel's ceiling is raised, and a net that does not fit the device is refused.
static int grad_lds(const char* who, const void* kernel, size_t lds)
{
    if (lds > 65536) {
        int limit = 0, dev = 0;
        T1D_HIP(hipGetDevice(&dev));
        T1D_HIP(hipDeviceGetAttribute(&limit, hipDeviceAttributeMaxSharedMemoryPerBlock, dev));
        if (lds > (size_t)limit) return fail(T1D_E_INVALID, std::string(who) + ": one wave of this policy does not fit in the device's LDS");
        T1D_HIP(hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    }
    return T1D_OK;
}

// mlp_grad_kernel<T, LS...> with one wave per partial sum of the partition, then the sum of the partials.  io: a
// t1d_mlp_batch or a t1d_mlp_loss (feat, y, grad, workspace); ls: the LossArgs of t1d_mlp_loss, nothing for
// t1d_mlp_grad; behind either the TileArgs of a listed call, whose waves walk gp.positions list positions.
template <typename T, typename IO, typename... LS>
static int launch_grad(const char* who, const t1d_mlp* m, int64_t n, const IO* io, const void* coef, const GradPartition& gp, hipStream_t s,
                       LS... ls)
{
    MlpArgs<T> c = make_mlp<T>(m, 0);
    GradArgs<T> g;
    g.feat = (const T*)io->feat; g.coef = (const T*)coef; g.y = (T*)io->y; g.partial = io->grad ? (T*)io->workspace : nullptr;
    g.n = n;
    g.chunks = (unsigned)gp.chunks; g.tiles = (unsigned)gp.positions; g.tiles_per_wave = (unsigned)gp.tiles_per_wave;
    g.waves_per_policy = (unsigned)gp.waves_per_policy; g.n_waves = (unsigned)(m->n_policies * gp.waves_per_policy);
    void (*const fn)(MlpArgs<T>, GradArgs<T>, LS...) = mlp_grad_kernel<T, LS...>;
    const size_t lds = grad_wave_lds(m, io->grad != nullptr, sizeof(T), &g.act_rows);
    const int rc = grad_lds(who, (const void*)fn, lds);
    if (rc) return rc;
    hipLaunchKernelGGL(fn, dim3(g.n_waves), dim3(64), lds, s, c, g, ls...);
    if (io->grad) {
        const unsigned total = (unsigned)(m->n_policies * m->n_params);
        hipLaunchKernelGGL(mlp_grad_sum_kernel<T>, dim3((total + 255) / 256), dim3(256), 0, s, (const T*)io->workspace, (T*)io->grad,
                           g.waves_per_policy, (unsigned)m->n_params, total);
    }
    return T1D_OK;
}

// t1d_mlp_grad (list == NULL) and t1d_mlp_grad_tiles
static int mlp_grad_entry(const char* who, int hip_device, int dtype, int64_t n, const t1d_mlp* mlp, const t1d_mlp_batch* io,
                          const t1d_tile_list* list, bool listed, void* stream)
{
    const std::string w = std::string(who) + ": ";
    if (!io) return fail(T1D_E_INVALID, w + "io is NULL");
    int rc = listed ? check_tile_list(who, list) : T1D_OK;
    if (rc) return rc;
    GradPartition gp;
    rc = check_mlp_grad(who, dtype, n, mlp, io->n_rows, &gp, listed ? &list->n_tiles : nullptr);
    if (rc) return rc;
    if (!io->feat) return fail(T1D_E_INVALID, w + "feat is NULL");
    if (!io->y && !io->grad) return fail(T1D_E_INVALID, w + "y and grad are both NULL");
    if (io->grad && !io->coef) return fail(T1D_E_INVALID, w + "grad needs coef");
    if (io->grad && (!io->workspace || io->workspace_bytes < grad_workspace_bytes(mlp, dtype, gp)))
        return fail(T1D_E_INVALID, w + "grad needs a workspace of " + who + "_workspace() bytes");
    if (mlp->n_policies * mlp->n_params > INT_MAX) return fail(T1D_E_INVALID, w + "too many policies");
    T1D_HIP(hipSetDevice(hip_device));
    rc = by_dtype(dtype, [&](auto t) {
        using T = decltype(t);
        if (!listed) return launch_grad<T>(who, mlp, n, io, io->coef, gp, (hipStream_t)stream);
        return launch_grad<T>(who, mlp, n, io, io->coef, gp, (hipStream_t)stream, TileArgs{list->tiles, (unsigned)gp.tiles});
    });
    if (rc) return rc;
    T1D_HIP(hipGetLastError());
    return T1D_OK;
}

extern "C" int t1d_mlp_grad(int hip_device, int dtype, int64_t n, const t1d_mlp* mlp, const t1d_mlp_batch* io, void* stream)
{
    return mlp_grad_entry("t1d_mlp_grad", hip_device, dtype, n, mlp, io, nullptr, false, stream);
}

extern "C" int t1d_mlp_grad_tiles(int hip_device, int dtype, int64_t n, const t1d_mlp* mlp, const t1d_mlp_batch* io,
                                  const t1d_tile_list* list, void* stream)
{
    return mlp_grad_entry("t1d_mlp_grad_tiles", hip_device, dtype, n, mlp, io, list, true, stream);
}

// t1d_mlp_loss: the statistics live in registers, so the launch is t1d_mlp_grad's with the LossArgs behind it (and the
// TileArgs of t1d_mlp_loss_tiles behind those)
template <typename T, int KIND>
static int launch_mlp_loss(const char* who, int dtype, const t1d_mlp* m, int64_t n, const struct t1d_mlp_loss* io, const GradPartition& gp,
                           const t1d_tile_list* list, hipStream_t s)
{
    LossArgs<T, KIND> ls;
    ls.eps = (const T*)io->eps; ls.y_old = (const T*)io->y_old; ls.adv = (const T*)io->adv; ls.target = (const T*)io->target;
    ls.sigma_old = (const T*)io->sigma_old; ls.sigma = (const T*)io->sigma;
    ls.coef_out = (T*)io->coef_out;
    ls.stat_partial = io->stats ? (double*)((char*)io->workspace + loss_stats_offset(m, dtype, gp)) : nullptr;
    ls.clip = (T)io->clip; ls.scale = (T)io->scale;
    const int rc = list ? launch_grad<T>(who, m, n, io, nullptr, gp, s, ls, TileArgs{list->tiles, (unsigned)gp.tiles})
                        : launch_grad<T>(who, m, n, io, nullptr, gp, s, ls);
    if (rc) return rc;
    if (io->stats) {
        const unsigned total = (unsigned)(4 * m->n_policies);
        hipLaunchKernelGGL(mlp_loss_stats_kernel, dim3((total + 63) / 64), dim3(64), 0, s, (const double*)ls.stat_partial, io->stats,
                           (unsigned)gp.waves_per_policy, total);
    }
    return T1D_OK;
}

// t1d_mlp_loss (list == NULL) and t1d_mlp_loss_tiles
static int mlp_loss_entry(const char* who, int hip_device, int dtype, int64_t n, const t1d_mlp* mlp, const struct t1d_mlp_loss* io,
                          const t1d_tile_list* list, bool listed, void* stream)
{
    const std::string w = std::string(who) + ": ";
    if (!io) return fail(T1D_E_INVALID, w + "io is NULL");
    int rc = listed ? check_tile_list(who, list) : T1D_OK;
    if (rc) return rc;
    GradPartition gp;
    rc = check_mlp_grad(who, dtype, n, mlp, io->n_rows, &gp, listed ? &list->n_tiles : nullptr);
    if (rc) return rc;
    if (!io->feat) return fail(T1D_E_INVALID, w + "feat is NULL");
    if (io->kind == T1D_LOSS_PPO_CLIP) {
        if (!io->eps || !io->y_old || !io->adv || !io->sigma_old || !io->sigma)
            return fail(T1D_E_INVALID, w + "T1D_LOSS_PPO_CLIP needs eps, y_old, adv, sigma_old and sigma");
        if (!(io->clip > 0.0 && io->clip < 1.0)) return fail(T1D_E_INVALID, w + "clip must be in (0, 1)");
    } else if (io->kind == T1D_LOSS_VALUE_MSE) {
        if (!io->target) return fail(T1D_E_INVALID, w + "T1D_LOSS_VALUE_MSE needs target");
    } else {
        return fail(T1D_E_INVALID, w + "unknown kind");
    }
    if (!std::isfinite(io->scale)) return fail(T1D_E_INVALID, w + "scale must be finite");
    if (!io->y && !io->coef_out && !io->grad && !io->stats) return fail(T1D_E_INVALID, w + "y, coef_out, grad and stats are all NULL");
    if ((io->grad || io->stats) && (!io->workspace || io->workspace_bytes < loss_workspace_bytes(mlp, dtype, gp)))
        return fail(T1D_E_INVALID, w + "grad and stats need a workspace of " + who + "_workspace() bytes");
    if (mlp->n_policies * mlp->n_params > INT_MAX) return fail(T1D_E_INVALID, w + "too many policies");
    T1D_HIP(hipSetDevice(hip_device));
    const bool ppo = io->kind == T1D_LOSS_PPO_CLIP;
    const t1d_tile_list* const tl = listed ? list : nullptr;
    if (dtype == T1D_F64)
        rc = ppo ? launch_mlp_loss<double, T1D_LOSS_PPO_CLIP>(who, dtype, mlp, n, io, gp, tl, (hipStream_t)stream)
                 : launch_mlp_loss<double, T1D_LOSS_VALUE_MSE>(who, dtype, mlp, n, io, gp, tl, (hipStream_t)stream);
    else
        rc = ppo ? launch_mlp_loss<float, T1D_LOSS_PPO_CLIP>(who, dtype, mlp, n, io, gp, tl, (hipStream_t)stream)
                 : launch_mlp_loss<float, T1D_LOSS_VALUE_MSE>(who, dtype, mlp, n, io, gp, tl, (hipStream_t)stream);
    if (rc) return rc;
    T1D_HIP(hipGetLastError());
    return T1D_OK;
}

extern "C" int t1d_mlp_loss(int hip_device, int dtype, int64_t n, const t1d_mlp* mlp, const struct t1d_mlp_loss* io, void* stream)
{
    return mlp_loss_entry("t1d_mlp_loss", hip_device, dtype, n, mlp, io, nullptr, false, stream);
}

extern "C" int t1d_mlp_loss_tiles(int hip_device, int dtype, int64_t n, const t1d_mlp* mlp, const struct t1d_mlp_loss* io,
                                  const t1d_tile_list* list, void* stream)
{
    return mlp_loss_entry("t1d_mlp_loss_tiles", hip_device, dtype, n, mlp, io, list, true, stream);
}

// t1d_gae (t1d_gae.hpp): every argument is checked here, before the device is touched.  -> the tiles of one policy (its 64-env
// pieces counted from its first env: one partial sum each) in *tiles
static int check_gae(const char* who, int dtype, int64_t n, const t1d_gae_batch* io, int64_t* tiles)
{
    const std::string w = std::string(who) + ": ";
    if (!io) return fail(T1D_E_INVALID, w + "io is NULL");
    if (dtype != T1D_F64 && dtype != T1D_F32) return fail(T1D_E_INVALID, w + "bad dtype");
    if (n < 1 || n > (int64_t)1 << 31) return fail(T1D_E_INVALID, w + "n out of range");
    if (io->n_rows < 1 || io->n_rows > ((int64_t)1 << 40) / n) return fail(T1D_E_INVALID, w + "n_rows out of range");
    if (io->n_policies < 1 || io->n_policies > INT_MAX || n % io->n_policies)
        return fail(T1D_E_INVALID, w + "n_policies must be in [1, 2^31 - 1] and divide n");
    if (!(io->gamma >= 0.0 && io->gamma <= 1.0) || !(io->lambda >= 0.0 && io->lambda <= 1.0))
        return fail(T1D_E_INVALID, w + "gamma and lambda must be in [0, 1]");
    *tiles = (n / io->n_policies + 63) / 64;
    return T1D_OK;
}

extern "C" int64_t t1d_gae_workspace(int dtype, int64_t n, const t1d_gae_batch* io)
{
    int64_t tiles = 0;
    const int rc = check_gae("t1d_gae_workspace", dtype, n, io, &tiles);
    if (rc) return rc;
    return io->n_policies * tiles * 2 * (int64_t)sizeof(double);
}

// cut == NULL: t1d_gae, gae_kernel; else t1d_gae_limit, gae_limit_kernel with the second mask
template <typename T>
static void launch_gae(int64_t n, const t1d_gae_batch* io, const t1d_gae_cut* cut, int64_t tiles, hipStream_t s)
{
    GaeArgs<T> a;
    a.reward = (const T*)io->reward; a.done = io->done; a.value = (const T*)io->value; a.last_value = (const T*)io->last_value;
    a.adv = (T*)io->adv; a.ret = (T*)io->ret; a.partial = io->moments ? (double*)io->workspace : nullptr;
    a.n = n; a.n_rows = io->n_rows; a.envs_per_policy = n / io->n_policies; a.tiles = (unsigned)tiles;
    a.n_waves = (unsigned)(io->moments ? io->n_policies * tiles : (n + 63) / 64);
    a.g = (T)io->gamma; a.gl = (T)(io->gamma * io->lambda);
    const dim3 grid((a.n_waves + kGaeBlock / 64 - 1) / (kGaeBlock / 64));
    // every array given: the streaming form, whose loads and stores the compiler can count
    const bool full = io->done && io->value && io->adv && io->ret;
    if (cut) {
        const GaeCutArgs<T> ca{cut->truncated, (const T*)cut->cut_value};
        if (io->moments) hipLaunchKernelGGL((full ? gae_limit_kernel<T, true, true> : gae_limit_kernel<T, true, false>), grid, dim3(kGaeBlock), 0, s, a, ca);
        else hipLaunchKernelGGL((full ? gae_limit_kernel<T, false, true> : gae_limit_kernel<T, false, false>), grid, dim3(kGaeBlock), 0, s, a, ca);
    } else if (io->moments) {
        hipLaunchKernelGGL((full ? gae_kernel<T, true, true> : gae_kernel<T, true, false>), grid, dim3(kGaeBlock), 0, s, a);
    } else {
        hipLaunchKernelGGL((full ? gae_kernel<T, false, true> : gae_kernel<T, false, false>), grid, dim3(kGaeBlock), 0, s, a);
    }
    if (io->moments)
        hipLaunchKernelGGL(gae_moments_kernel, dim3((unsigned)io->n_policies), dim3(64), 0, s, (const double*)io->workspace, io->moments,
                           a.tiles);
}

// t1d_gae (cut == NULL, limit = false) and t1d_gae_limit
static int gae_entry(const char* who, int hip_device, int dtype, int64_t n, const t1d_gae_batch* io, const t1d_gae_cut* cut, bool limit,
                     void* stream)
{
    const std::string w = std::string(who) + ": ";
    int64_t tiles = 0;
    const int rc = check_gae(who, dtype, n, io, &tiles);
    if (rc) return rc;
    if (!io->reward) return fail(T1D_E_INVALID, w + "reward is NULL");
    if (!io->adv && !io->ret && !io->moments) return fail(T1D_E_INVALID, w + "adv, ret and moments are all NULL");
    if (io->moments && (!io->workspace || io->workspace_bytes < io->n_policies * tiles * 2 * (int64_t)sizeof(double)))
        return fail(T1D_E_INVALID, w + "moments need a workspace of t1d_gae_workspace() bytes");
    if (limit && (!cut || !cut->truncated)) return fail(T1D_E_INVALID, w + "cut and cut.truncated must be set");
    T1D_HIP(hipSetDevice(hip_device));
    by_dtype(dtype, [&](auto t) { launch_gae<decltype(t)>(n, io, cut, tiles, (hipStream_t)stream); });
    T1D_HIP(hipGetLastError());
    return T1D_OK;
}

extern "C" int t1d_gae(int hip_device, int dtype, int64_t n, const t1d_gae_batch* io, void* stream)
{
    return gae_entry("t1d_gae", hip_device, dtype, n, io, nullptr, false, stream);
}

extern "C" int t1d_gae_limit(int hip_device, int dtype, int64_t n, const t1d_gae_batch* io, const t1d_gae_cut* cut, void* stream)
{
    return gae_entry("t1d_gae_limit", hip_device, dtype, n, io, cut, true, stream);
}

extern "C" int t1d_philox_normals(t1d_ctx* c, uint64_t seed, int64_t env_offset, int64_t n, uint32_t episode,
                                  int32_t draw0, int32_t n_draws, double* out, void* stream)
{
    if (!c || !out || n < 1 || n_draws < 1 || draw0 < -3) return fail(T1D_E_INVALID, "t1d_philox_normals: bad argument");
    T1D_HIP(hipSetDevice(c->device));
    hipLaunchKernelGGL(philox_normals_kernel, grid_for(n), dim3(kBlock), 0, (hipStream_t)stream, seed, env_offset, n,
                       episode, draw0, n_draws, out);
    T1D_HIP(hipGetLastError());
    return T1D_OK;
}

template <typename T>
static void launch_rhs(const t1d_ctx* c, int64_t n, int math, const void* x, const int32_t* pid, const void* cho, const void* insulin,
                       const void* last_qsto, const void* last_food, void* dxdt, const T* par, hipStream_t s)
{
    hipLaunchKernelGGL((math ? rhs_kernel<1, T> : rhs_kernel<0, T>), grid_for(n), dim3(kBlock), 0, s, n, (const T*)x, pid, (const T*)cho,
                       (const T*)insulin, (const T*)last_qsto, (const T*)last_food, (T*)dxdt, par, c->np, c->d_status);
}

extern "C" int t1d_model_rhs(t1d_ctx* c, int dtype, int64_t n, int math, const void* x, const int32_t* pid, const void* cho,
                             const void* insulin, const void* last_qsto, const void* last_food, void* dxdt, void* stream)
{
    if (!c || !x || !pid || !cho || !insulin || !last_qsto || !last_food || !dxdt) return fail(T1D_E_INVALID, "t1d_model_rhs: NULL argument");
    if (n < 1 || n > (int64_t)1 << 28) return fail(T1D_E_INVALID, "t1d_model_rhs: n out of range");
    if (dtype != T1D_F64 && dtype != T1D_F32) return fail(T1D_E_INVALID, "t1d_model_rhs: bad dtype");
    if (math != 0 && math != 1) return fail(T1D_E_INVALID, "t1d_model_rhs: math must be 0 or 1");
    T1D_HIP(hipSetDevice(c->device));
    hipStream_t s = (hipStream_t)stream;
    if (dtype == T1D_F64) launch_rhs<double>(c, n, math, x, pid, cho, insulin, last_qsto, last_food, dxdt, c->d_par64, s);
    else launch_rhs<float>(c, n, math, x, pid, cho, insulin, last_qsto, last_food, dxdt, c->d_par32, s);
    T1D_HIP(hipGetLastError());
    return T1D_OK;
}

extern "C" int t1d_sync(t1d_ctx* c, void* stream, int32_t* status)
{
    if (!c) return fail(T1D_E_INVALID, "t1d_sync: ctx is NULL");
    T1D_HIP(hipSetDevice(c->device));
    T1D_HIP(hipStreamSynchronize((hipStream_t)stream));
    int st = 0;
    T1D_HIP(hipMemcpy(&st, c->d_status, sizeof(int), hipMemcpyDeviceToHost));
    if (st) T1D_HIP(hipMemset(c->d_status, 0, sizeof(int)));
    if (status) *status = st;
    if (st) return fail(T1D_E_STATUS, "t1d_sync: device status bits set: " + std::to_string(st));
    return T1D_OK;
}
