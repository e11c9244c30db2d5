// t1d_dopri5.hpp -- the exact mode: scipy.integrate.ode('dopri5') as the reference drives it (t1dpatient.py:110-113,276),
// one lane per env, fp64 only.  Included by t1d_abi.hip after t1d_kernels.hpp; launched by t1d_step_dopri5 and, for closed-loop
// roll-outs with every lane at its own pace, by t1d_rollout_pid_dopri5 / t1d_rollout_bb_dopri5 (include/t1d.h).
//
// The fixed-step schemes of t1d_device.hpp are close to SciPy's solution but cannot reproduce it: part of the difference is
// SciPy's own error (tolerance 1e-6 relative), which only SciPy's algorithm repeats.  What is restated here, line for line,
// is the oracle's restatement of Hairer's driver (oracle/t1d_oracle.c: t1d_o_rhs, o_hinit, t1d_o_dopri5_minute), which
// tests/test_oracle_golden.py pins to the reference:
//   rhs_scipy      T1DPatient.model (t1dpatient.py:119-208) from the RAW parameter columns in the reference's order of
//                  evaluation -- ocml tanh, IEEE divisions, no precomputed combinations.  rhs<0> groups some terms
//                  differently; a difference of one ulp can decide an accept/reject at the tolerance boundary, and every
//                  such flip moves the trace by up to the solver's tolerance, so the exact mode has an RHS of its own.
//   dopri5_minute  one integrate() call on [t, t+1], x = t: rtol 1e-6, atol 1e-12, safety 0.9, fac1 0.2, fac2 10,
//                  beta 0.04, uround 2.3e-16, nmax 500, hmax 1; the initial-step probe only when the carried step is 0;
//                  FSAL; the predicted step written back on the last accepted step.
// Both bodies are compiled with FMA contraction off, as the oracle is (oracle/Makefile: -ffp-contract=off).
// Each lane runs its own accept/reject loop; in dopri5_step_kernel a wave runs each minute until its slowest lane is done, in
// dopri5_rollout_kernel until the lane with the most step attempts over the launch is.  The loop ends on every input: a
// lane gives up after nmax steps or when the step underflows (NaN states included), which the kernel reports as
// T1D_ST_SOLVER_FAILED -- where the reference raises "ODE solver failed".
#pragma once
#include "t1d_kernels.hpp"
#include "t1d_policy.hpp"

namespace t1d {

constexpr int kRawPars = T1D_P_NCOLS - T1D_P_BW;     // the 32 model columns of a patient row (T1D_P_BW .. T1D_P_U2SS)

// the raw parameter table, [kRawPars][kMaxPatients] (patient fastest), staged in LDS; indexed by T1D_P_* column
struct ParsRaw {
    const double* base;
    int pid;
    __device__ __forceinline__ double operator()(int col) const { return base[(col - T1D_P_BW) * kMaxPatients + pid]; }
};

// t1d_o_rhs (oracle/t1d_oracle.c) = T1DPatient.model (t1dpatient.py:119-208), operation for operation.
// d = CHO eaten this minute in mg/min (:121, cho * 1000), ins = insulin in U/min, lq / lf = last_Qsto / last_foodtaken.
__device__ __forceinline__ void rhs_scipy(const ParsRaw& p, const double (&x)[13], double d, double ins, double lq, double lf,
                                          double (&dx)[13])
{
#pragma clang fp contract(off)
    const double insulin = ins * 6000.0 / p(T1D_P_BW);                                      // :122
    const double qsto = x[0] + x[1];                                                        // :126
    const double Dbar = lq + lf * 1000.0;                                                   // :130
    const double kmax = p(T1D_P_KMAX), kmin = p(T1D_P_KMIN), b = p(T1D_P_B), dd = p(T1D_P_D);
    double kgut;
    dx[0] = -kmax * x[0] + d;                                                               // :133
    if (Dbar > 0.0) {                                                                       // :135-140
        const double aa = 5.0 / 2.0 / (1.0 - b) / Dbar;
        const double cc = 5.0 / 2.0 / dd / Dbar;
        kgut = kmin + (kmax - kmin) / 2.0 * (tanh(aa * (qsto - b * Dbar)) - tanh(cc * (qsto - dd * Dbar)) + 2.0);
    } else {
        kgut = kmax;                                                                        // :142
    }
    dx[1] = kmax * x[0] - x[1] * kgut;                                                      // :145
    const double kabs = p(T1D_P_KABS);
    dx[2] = kgut * x[1] - kabs * x[2];                                                      // :148

    const double Rat = p(T1D_P_F) * kabs * x[2] / p(T1D_P_BW);                             // :151
    const double EGPt = p(T1D_P_KP1) - p(T1D_P_KP2) * x[3] - p(T1D_P_KP3) * x[8];           // :153
    const double Uiit = p(T1D_P_FSNC);                                                      // :155
    const double ke2 = p(T1D_P_KE2);
    const double Et = (x[3] > ke2) ? p(T1D_P_KE1) * (x[3] - ke2) : 0.0;                    // :158-161
    const double k1 = p(T1D_P_K1), k2 = p(T1D_P_K2);
    dx[3] = (EGPt > 0.0 ? EGPt : 0.0) + Rat - Uiit - Et - k1 * x[3] + k2 * x[4];           // :165
    dx[3] = (x[3] >= 0.0) ? dx[3] : 0.0 * dx[3];                                           // :167

    const double Vmt = p(T1D_P_VM0) + p(T1D_P_VMX) * x[6];                                 // :169
    const double Uidt = Vmt * x[4] / (p(T1D_P_KM0) + x[4]);                                 // :171
    dx[4] = -Uidt + k1 * x[3] - k2 * x[4];                                                  // :172
    dx[4] = (x[4] >= 0.0) ? dx[4] : 0.0 * dx[4];                                           // :173

    const double m1 = p(T1D_P_M1), m2 = p(T1D_P_M2), ka1 = p(T1D_P_KA1), ka2 = p(T1D_P_KA2);
    dx[5] = -(m2 + p(T1D_P_M4)) * x[5] + m1 * x[9] + ka1 * x[10] + ka2 * x[11];            // :176
    const double It = x[5] / p(T1D_P_VI);                                                   // :178
    dx[5] = (x[5] >= 0.0) ? dx[5] : 0.0 * dx[5];                                           // :179

    const double p2u = p(T1D_P_P2U), ki = p(T1D_P_KI);
    dx[6] = -p2u * x[6] + p2u * (It - p(T1D_P_IB));                                        // :182
    dx[7] = -ki * (x[7] - It);                                                              // :185
    dx[8] = -ki * (x[8] - x[7]);                                                            // :187

    dx[9] = -(m1 + p(T1D_P_M30)) * x[9] + m2 * x[5];                                        // :190
    dx[9] = (x[9] >= 0.0) ? dx[9] : 0.0 * dx[9];                                           // :191

    const double kd = p(T1D_P_KD);
    dx[10] = insulin - (ka1 + kd) * x[10];                                                  // :194
    dx[10] = (x[10] >= 0.0) ? dx[10] : 0.0 * dx[10];                                       // :195
    dx[11] = kd * x[10] - ka2 * x[11];                                                      // :197
    dx[11] = (x[11] >= 0.0) ? dx[11] : 0.0 * dx[11];                                       // :198
    const double ksc = p(T1D_P_KSC);
    dx[12] = (-ksc * x[12] + ksc * x[3]);                                                   // :201
    dx[12] = (x[12] >= 0.0) ? dx[12] : 0.0 * dx[12];                                       // :202
}

// o_hinit: the driver's initial-step probe (one extra RHS evaluation)
__device__ __forceinline__ double dopri5_hinit(const ParsRaw& p, const double (&y)[13], const double (&f0)[13], double d,
                                               double ins, double lq, double lf, double hmax, double atol, double rtol)
{
#pragma clang fp contract(off)
    double dnf = 0.0, dny = 0.0, y1[13], f1[13];
#pragma unroll
    for (int i = 0; i < 13; ++i) {
        const double sk = atol + rtol * fabs(y[i]);
        dnf += (f0[i] / sk) * (f0[i] / sk);
        dny += (y[i] / sk) * (y[i] / sk);
    }
    double h = (dnf <= 1e-10 || dny <= 1e-10) ? 1e-6 : sqrt(dny / dnf) * 0.01;
    if (h > hmax) h = hmax;
#pragma unroll
    for (int i = 0; i < 13; ++i) y1[i] = y[i] + h * f0[i];
    rhs_scipy(p, y1, d, ins, lq, lf, f1);
    double der2 = 0.0;
#pragma unroll
    for (int i = 0; i < 13; ++i) {
        const double sk = atol + rtol * fabs(y[i]);
        der2 += ((f1[i] - f0[i]) / sk) * ((f1[i] - f0[i]) / sk);
    }
    der2 = sqrt(der2) / h;
    const double der12 = fmax(fabs(der2), sqrt(dnf));
    const double h1 = (der12 <= 1e-15) ? fmax(1e-6, fabs(h) * 1e-3) : pow(0.01 / der12, 1.0 / 5.0);
    h = fmin(fmin(100.0 * fabs(h), h1), hmax);
    return h;
}

// t1d_o_dopri5_minute: one integrate() from x = t_start to t_start + 1, in resumable form so that a kernel can walk a lane
// through its minutes one step attempt at a time (dopri5_rollout_kernel) or run a minute to its end (dopri5_minute).
// Dopri5Run: the words the driver carries from one step attempt to the next.
struct Dopri5Run {
    double x, h, facold, k1[13];
    int nstep;
    bool last, reject;
};
constexpr double kDopriRtol = 1e-6, kDopriAtol = 1e-12, kDopriHmax = 1.0;

// enter a minute at x = t_start: SciPy re-enters the driver every minute -- a fresh first stage and, when the carried
// step is 0, the initial-step probe
__device__ __forceinline__ void dopri5_enter(const ParsRaw& p, const double (&y)[13], double d, double ins, double lq, double lf,
                                             double h_carry, double t_start, Dopri5Run& r, int& nfcn)
{
#pragma clang fp contract(off)
    r.x = t_start; r.h = h_carry; r.facold = 1e-4;
    r.nstep = 0; r.last = false; r.reject = false;
    rhs_scipy(p, y, d, ins, lq, lf, r.k1); nfcn++;
    if (r.h == 0.0) { r.h = dopri5_hinit(p, y, r.k1, d, ins, lq, lf, kDopriHmax, kDopriAtol, kDopriRtol); nfcn++; }
}

// one step attempt towards xend: six RHS evaluations, the error estimate, accept or reject, the next step size.
// y: the state, advanced in place by an accepted step.  Returns 0 = go on, 1 = the minute is done (the predicted step
// written to h_carry), -1 = the driver gives up (nmax steps, or a step below the resolution of x): y is at the last
// accepted point.
__device__ __forceinline__ int dopri5_attempt(const ParsRaw& p, double (&y)[13], double d, double ins, double lq, double lf,
                                              double& h_carry, double xend, Dopri5Run& r, int& nfcn)
{
#pragma clang fp contract(off)
    const double a21 = 0.2, a31 = 3.0 / 40.0, a32 = 9.0 / 40.0, a41 = 44.0 / 45.0,
        a42 = -56.0 / 15.0, a43 = 32.0 / 9.0, a51 = 19372.0 / 6561.0, a52 = -25360.0 / 2187.0,
        a53 = 64448.0 / 6561.0, a54 = -212.0 / 729.0, a61 = 9017.0 / 3168.0, a62 = -355.0 / 33.0,
        a63 = 46732.0 / 5247.0, a64 = 49.0 / 176.0, a65 = -5103.0 / 18656.0, a71 = 35.0 / 384.0,
        a73 = 500.0 / 1113.0, a74 = 125.0 / 192.0, a75 = -2187.0 / 6784.0, a76 = 11.0 / 84.0,
        e1 = 71.0 / 57600.0, e3 = -71.0 / 16695.0, e4 = 71.0 / 1920.0, e5 = -17253.0 / 339200.0,
        e6 = 22.0 / 525.0, e7 = -1.0 / 40.0;
    const double rtol = kDopriRtol, atol = kDopriAtol, safe = 0.9, fac1 = 0.2, fac2 = 10.0, uround = 2.3e-16, beta = 0.04;
    const int nmax = 500;
    const double expo1 = 0.2 - beta * 0.75, facc1 = 1.0 / fac1, facc2 = 1.0 / fac2;
    const double hmax = kDopriHmax;
    double k2[13], k3[13], k4[13], k5[13], k6[13], y1[13], ysti[13];
    double (&k1)[13] = r.k1;
    double h = r.h;

    if (r.nstep > nmax) return -1;
    if (0.1 * fabs(h) <= fabs(r.x) * uround) return -1;
    if ((r.x + 1.01 * h - xend) > 0.0) { h = xend - r.x; r.last = true; }
    r.nstep++;
#pragma unroll
    for (int i = 0; i < 13; ++i) y1[i] = y[i] + h * a21 * k1[i];
    rhs_scipy(p, y1, d, ins, lq, lf, k2);
#pragma unroll
    for (int i = 0; i < 13; ++i) y1[i] = y[i] + h * (a31 * k1[i] + a32 * k2[i]);
    rhs_scipy(p, y1, d, ins, lq, lf, k3);
#pragma unroll
    for (int i = 0; i < 13; ++i) y1[i] = y[i] + h * (a41 * k1[i] + a42 * k2[i] + a43 * k3[i]);
    rhs_scipy(p, y1, d, ins, lq, lf, k4);
#pragma unroll
    for (int i = 0; i < 13; ++i) y1[i] = y[i] + h * (a51 * k1[i] + a52 * k2[i] + a53 * k3[i] + a54 * k4[i]);
    rhs_scipy(p, y1, d, ins, lq, lf, k5);
#pragma unroll
    for (int i = 0; i < 13; ++i) ysti[i] = y[i] + h * (a61 * k1[i] + a62 * k2[i] + a63 * k3[i] + a64 * k4[i] + a65 * k5[i]);
    rhs_scipy(p, ysti, d, ins, lq, lf, k6);
#pragma unroll
    for (int i = 0; i < 13; ++i) y1[i] = y[i] + h * (a71 * k1[i] + a73 * k3[i] + a74 * k4[i] + a75 * k5[i] + a76 * k6[i]);
    rhs_scipy(p, y1, d, ins, lq, lf, k2);              // k2 <- k7 (the first stage of the next step: FSAL)
    nfcn += 6;
    double err = 0.0;
#pragma unroll
    for (int i = 0; i < 13; ++i) {
        const double ke = (e1 * k1[i] + e3 * k3[i] + e4 * k4[i] + e5 * k5[i] + e6 * k6[i] + e7 * k2[i]) * h;
        const double sk = atol + rtol * fmax(fabs(y[i]), fabs(y1[i]));
        err += (ke / sk) * (ke / sk);
    }
    err = sqrt(err / 13.0);
    const double fac11 = pow(err, expo1);
    double fac = fac11 / pow(r.facold, beta);
    fac = fmax(facc2, fmin(facc1, fac / safe));
    double hnew = h / fac;
    if (err <= 1.0) {
        r.facold = fmax(err, 1e-4);
#pragma unroll
        for (int i = 0; i < 13; ++i) { k1[i] = k2[i]; y[i] = y1[i]; }
        r.x += h;
        if (r.last) { h_carry = hnew; return 1; }
        if (fabs(hnew) > hmax) hnew = hmax;
        if (r.reject) hnew = fmin(fabs(hnew), fabs(h));
        r.reject = false;
    } else {
        hnew = h / fmin(facc1, fac11 / safe);
        r.reject = true;
        r.last = false;
    }
    r.h = hnew;
    return 0;
}

// one minute to its end.  y: the state, advanced in place (left at the last accepted point if the solver gives up);
// h_carry: the predicted step, read (0 = probe) and written on success; nfcn: RHS evaluations of this call, added.
// Returns false where the driver gives up.
__device__ __forceinline__ bool dopri5_minute(const ParsRaw& p, double (&y)[13], double d, double ins, double lq, double lf,
                                              double& h_carry, double t_start, int& nfcn)
{
#pragma clang fp contract(off)
    Dopri5Run r;
    dopri5_enter(p, y, d, ins, lq, lf, h_carry, t_start, r, nfcn);
    const double xend = t_start + 1.0;
    for (;;) {
        const int rc = dopri5_attempt(p, y, d, ins, lq, lf, h_carry, xend, r, nfcn);
        if (rc) return rc > 0;
    }
}

// eat_minute's bookkeeping needs no parameter; the MinuteIn it also returns is for the fixed-step RHS, and of it the exact
// mode uses d_mg = to_eat * 1000 only (the rest is dead code)
struct NoDerivedPars {
    __device__ __forceinline__ double operator()(int) const { return 1.0; }
};

// One t1d_step_dopri5 call: the generic step (step_kernel / step_body: pump, meal lookup and bookkeeping, CGM noise with the
// block refill inline, outputs, state) with dopri5_minute in place of the fixed-step integrator.  Any state layout; every
// state word the generic kernel writes is written (dbar included), so an env can go on under t1d_step afterwards.
// raw: [kRawPars][kMaxPatients]; h_carry [n] read and written; nfev [n] or NULL.
__global__ __launch_bounds__(kBlock, 1) void dopri5_step_kernel(const KArgs<double> a, const double* __restrict__ raw,
                                                                double* h_carry, int32_t* nfev)
{
    __shared__ double lds[kRawPars * kMaxPatients];
    for (int j = threadIdx.x; j < kRawPars * kMaxPatients; j += blockDim.x) lds[j] = raw[j];
    __syncthreads();
    const unsigned i = blockIdx.x * kBlock + threadIdx.x;
    __builtin_assume(i < (1u << 28));          // host guarantees n <= 2^28: i * sizeof(T) fits a 32-bit voffset
    if ((int64_t)i >= a.n) return;
    const uint32_t meta = at(a.meta, i);
    const uint32_t pid = T1D_META_PID(meta);
    Env<double> e;
    load_env(a, i, meta, e);
    const double basal = at(a.basal, i);
    const double bolus = a.bolus ? at(a.bolus, i) : 0.0;
    const double rp = e.prev_risk;
    const ParsRaw p{lds, (int)pid};
    NoDerivedPars nop;
    double q_basal, q_bolus;                   // as step_body: env.py:51-52, or T1DPatient.step driven directly
    if (a.flags & T1D_BATCH_NO_PUMP) {
        q_basal = basal; q_bolus = a.bolus ? bolus : 0.0;
    } else {
        q_basal = pump_quantise(basal, a.pump.inc_basal, a.pump.min_basal, a.pump.max_basal);
        q_bolus = a.pump.min_bolus > 0.0 ? a.pump.min_bolus : 0.0;
        if (a.bolus) q_bolus = pump_quantise(bolus, a.pump.inc_bolus, a.pump.min_bolus, a.pump.max_bolus);
    }
    const double insulin = q_basal + q_bolus;
    const double div = double(a.minutes);
    double hc = at(h_carry, i);
    int nf = 0;
    bool failed = false;
    StepOut<double> o{0.0, 0.0, 0.0, 0.0};
    for (int m = 0; m < a.minutes; ++m) {
        const double meal = a.cho ? at(row(a.cho, a.n, m), i) : meal_lookup(a, i, e);      // env.py:50
        bool due;
        const double noise = measure_noise<true>(a, i, e, due);
        const MinuteIn<double> u = eat_minute<0, double>(nop, e.x, meal, insulin, e.planned, e.lq, e.lf, e.eating);
        // a lane whose solver gave up keeps its state at the last accepted point for the rest of the call
        if (!failed) failed = !dopri5_minute(p, e.x, u.d_mg, insulin, e.lq, e.lf, hc, (double)e.t, nf);
        e.t += 1;
        const double gsub = e.x[12] / p(T1D_P_VG);                                        // t1dpatient.py:217-218
        const double cgm = measure_apply(a, e, gsub, noise, due);                         // env.py:62
        o.meal += meal / div; o.ins += insulin / div; o.bg += gsub / div; o.cgm += cgm / div;   // env.py:78-81
    }
    write_outputs<0>(a, i, e, o, rp);
    store_env(a, i, pid, e);
    at(h_carry, i) = hc;
    if (nfev) at(nfev, i) = nf;
    if (failed) atomicOr(a.status, T1D_ST_SOLVER_FAILED);
}

// ---- closed-loop roll-outs in the exact mode (t1d_rollout_pid_dopri5 / t1d_rollout_bb_dopri5) ---------------------------
// PIDController.policy (pid_ctrller.py:17-36) / BBController._bb_policy (basal_bolus_ctrller.py:64-79): the arithmetic of
// rollout_body (t1d_kernels.hpp), restated with FMA contraction off like everything else the exact mode computes, so that
// a roll-out gives what a step() loop with the controller evaluated operation by operation gives.  The controller's state
// lives in memory: it is touched once per step.  obs: the previous step's observation; st: the sensor's sample time.
__device__ __forceinline__ void dopri5_controller(const PidArgs<double>& c, unsigned i, double obs, double st, double& u, double& bolus)
{
#pragma clang fp contract(off)
    bolus = 0.0;
    if (c.kind == 1) {
        u = at(c.bb_basal, i);
        const double prev_meal = at(c.bb_prev_meal, i);
        if (prev_meal > 0.0) {
            const double corr = obs > 150.0 ? (obs - c.target) / at(c.bb_cf, i) : 0.0;
            bolus = ((prev_meal * st) / at(c.bb_cr, i) + corr) / st;
        }
    } else {
        const double integ = at(c.integ, i), prev = at(c.prev, i);
        u = c.P * (obs - c.target) + c.I * integ + c.D * (obs - prev) / st;
        at(c.prev, i) = obs;
        at(c.integ, i) = integ + (obs - c.target) * st;
    }
}

// The words of a lane that only its minute boundaries touch, kept in LDS between them ([word][lane]: no bank conflict):
// dopri5_attempt needs every register of the unified file for its stage vectors (dopri5_step_kernel: 256 VGPRs + 220
// AGPRs), and what is reloaded at the top of the boundary block is not alive across the step attempts.  STRIDE: the lanes
// that share a block of words -- the workgroup (RollCold) or, where the workgroup's size is chosen per launch, the wave.
template <int STRIDE> struct RollColdT {
    enum { PLANNED, LAST_CGM, PREV_RISK, CUR0, CUR1, CUR2, CUR3, NOISE, O_CGM, O_BG, O_MEAL, O_INS, HC, NF };
    enum { CURSOR, NEXT_MEAL, NEXT_MEAL_LOADED, NI };
    double* f; int* w;
    __device__ __forceinline__ void save(const Env<double>& e, const StepOut<double>& o, double noise, double hc) const
    {
        f[PLANNED * STRIDE] = e.planned; f[LAST_CGM * STRIDE] = e.last_cgm; f[PREV_RISK * STRIDE] = e.prev_risk;
#pragma unroll
        for (int k = 0; k < 4; ++k) f[(CUR0 + k) * STRIDE] = e.cur[k];
        f[NOISE * STRIDE] = noise; f[HC * STRIDE] = hc;
        f[O_CGM * STRIDE] = o.cgm; f[O_BG * STRIDE] = o.bg; f[O_MEAL * STRIDE] = o.meal; f[O_INS * STRIDE] = o.ins;
        w[CURSOR * STRIDE] = e.cursor; w[NEXT_MEAL * STRIDE] = e.next_meal; w[NEXT_MEAL_LOADED * STRIDE] = e.next_meal_loaded;
    }
    __device__ __forceinline__ void load(Env<double>& e, StepOut<double>& o, double& noise, double& hc) const
    {
        e.planned = f[PLANNED * STRIDE]; e.last_cgm = f[LAST_CGM * STRIDE]; e.prev_risk = f[PREV_RISK * STRIDE];
#pragma unroll
        for (int k = 0; k < 4; ++k) e.cur[k] = f[(CUR0 + k) * STRIDE];
        noise = f[NOISE * STRIDE]; hc = f[HC * STRIDE];
        o.cgm = f[O_CGM * STRIDE]; o.bg = f[O_BG * STRIDE]; o.meal = f[O_MEAL * STRIDE]; o.ins = f[O_INS * STRIDE];
        e.cursor = w[CURSOR * STRIDE]; e.next_meal = w[NEXT_MEAL * STRIDE]; e.next_meal_loaded = w[NEXT_MEAL_LOADED * STRIDE];
    }
};
typedef RollColdT<kBlock> RollCold;

// c.n_steps closed-loop steps of a.minutes minutes in one launch, every lane at its own pace.  The body of the one loop is
// ONE step attempt of the driver for every lane that still has work; ahead of it, only the lanes that have just completed a
// minute (or enter their first) run the boundary block: finish the minute as dopri5_step_kernel does, at the end of a step
// the outputs, the trace rows, the statistics and the controller, then open the next minute.  Inside a launch nothing
// forces the 64 envs of a wave to be in the same minute, so a wave pays for the lane with the largest TOTAL of step
// attempts, not for the per-minute maximum summed over the minutes.  Lanes never exchange data, and a lane executes the
// operations dopri5_step_kernel and the controller would execute for its env, in the same order: its results do not depend
// on its neighbours, and are those of a step() loop, bit for bit.  What a step leaves behind once per step (observation,
// reward, risk, controller state, statistics) goes through memory as in that loop; what a minute needs is in RollCold.
// The loop ends: a lane either completes a minute or spends one of the driver's nmax step attempts of that minute.
// A lane whose solver gives up keeps its last accepted state for the rest of the launch; its clock, meals and noise go on.
// Grid, block, tables and arguments as dopri5_step_kernel; nfev: RHS evaluations of each env in this launch.
// The loop is one text, t1d_dopri5_loop.inc, which this kernel and the eight below include between their braces; a kernel
// defines ahead of the include what it is and the action it takes where a step opens (the list is at the top of that file).
__global__ __launch_bounds__(kBlock, 1) void dopri5_rollout_kernel(const KArgs<double> a, const PidArgs<double> c,
                                                                   const double* __restrict__ raw, double* h_carry, int32_t* nfev)
{
    // its own: RollCold in static LDS; PidArgs' bb_prev_meal; where a step opens, the controller on the last observation
#define DOPRI5_STATE
#define DOPRI5_BB
#define DOPRI5_ACTION                                                                                                          \
    double u, bolus;                                                                                                           \
    dopri5_controller(c, i, at(a.cgm, i), st, u, bolus);
#include "t1d_dopri5_loop.inc"
}

// dopri5_rollout_kernel under PIDController with env i's own P[i], I[i], D[i] and target[i] (t1d_rollout_pid_dopri5_gains):
// the controller below where dopri5_controller stands.  The four words are loaded inside the boundary block where a step
// opens, next to the controller's state, and are dead before dopri5_attempt like everything else of that block.  The
// expression is dopri5_controller's, contraction off: an env under gains g computes, operation by operation, what the
// scalar call computes under g.
__device__ __forceinline__ void dopri5_controller_gains(const PidGainArgs<double>& c, unsigned i, double obs, double st, double& u)
{
#pragma clang fp contract(off)
    const double integ = at(c.integ, i), prev = at(c.prev, i);
    const double kP = at(c.gP, i), kI = at(c.gI, i), kD = at(c.gD, i), target = at(c.gtarget, i);
    u = kP * (obs - target) + kI * integ + kD * (obs - prev) / st;
    at(c.prev, i) = obs;
    at(c.integ, i) = integ + (obs - target) * st;
}

__global__ __launch_bounds__(kBlock, 1) void dopri5_rollout_gains_kernel(const KArgs<double> a, const PidGainArgs<double> c,
                                                                         const double* __restrict__ raw, double* h_carry, int32_t* nfev)
{
    // its own: RollCold in static LDS; where a step opens, the controller under the env's gains, no bolus
#define DOPRI5_STATE
#define DOPRI5_ACTION                                                                                                          \
    double u, bolus;                                                                                                           \
    dopri5_controller_gains(c, i, at(a.cgm, i), st, u);                                                                        \
    bolus = 0.0;
#include "t1d_dopri5_loop.inc"
}

// ---- closed-loop roll-outs in the exact mode under the policy of t1d_mlp (t1d_rollout_mlp_dopri5) -----------------------
// dopri5_rollout_kernel with the network of t1d_policy.hpp where dopri5_controller stands: solver, eat_minute, measure_*,
// the pump and the outputs are the shared loop's (t1d_dopri5_loop.inc); the action is mlp_action, the function
// mlp_rollout_kernel calls, so a step asks for the word t1d_rollout_mlp would ask for from the same windows, prev_meal,
// clock and weights (the functions of t1d_policy.hpp carry no contract(off): the pragma of this file is set per function
// and stays in the solver's).  Where the policy's words live:
//   windows      2 H rows of the lane's LDS column ([row][lane], no bank conflict), a ring as in mlp_rollout_body.  The
//                lanes of a wave are in different steps, so the head is per lane: after s steps of this launch CGM[0] sits
//                in row (H - s mod H) mod H, worked out from the lane's own step counter when a step ends.  In window
//                order in mlp.cgm_hist / ins_hist on entry and on exit.
//   layer buffer the rows behind the windows; live, like mlp_layers' out[] registers, only inside the boundary block of a
//                lane that opens a step.  Nothing of the policy is in a register across dopri5_attempt.
//   weights      one set per wave through the scalar data cache, as in mlp_rollout_kernel; only the lanes that open a step
//                at that moment are active while the network runs.
//   prev_meal, accumulators   through memory once per step, as dopri5_rollout_kernel passes the controller's state.
// LDS: the raw patient rows (static), then for each wave RollCold's words (stride 64) and the column block -- the workgroup
// is 4, 2 or 1 waves, the most that fit (t1d_rollout_mlp_dopri5), so every wave owns a contiguous piece of dynamic LDS
// whose layout does not depend on the workgroup's size.
constexpr int kRollColdWaveBytes = (int)(RollColdT<64>::NF * sizeof(double) + RollColdT<64>::NI * sizeof(int)) * 64;

// Three pieces of the loop (t1d_dopri5_loop.inc) as functions, called by every kernel with windows except
// dopri5_mlp_rollout_kernel, for which the loop has the same lines in place (DOPRI5_WRITTEN_OUT): calling these from that
// kernel changed its register allocation and cost it 0.5 - 0.7 % at 1 Mi envs when tried
// (profiles/policy/kernel_resources_collect_exact.txt), and writing the lines out for the others moves all six of them and
// makes two spill more (the figures are in t1d_dopri5_loop.inc).  A change to one of them is a change to those lines.
// the windows into the lane's column, in window order (head 0)
__device__ __forceinline__ void dopri5_mlp_load_windows(const KArgs<double>& a, const MlpArgs<double>& c, unsigned i, double* col)
{
    const int H = c.history;
    col[0] = at(a.cgm, i);                                      // CGM[0] is the observation the first step starts from
    for (int k = 1; k < H; ++k) col[k * 64] = at(rowv(c.cgm_hist, a.n, k), i);
    for (int k = 0; k < H; ++k) col[(H + k) * 64] = at(rowv(c.ins_hist, a.n, k), i);
}

// the windows back in window order after s steps of this launch
__device__ __forceinline__ void dopri5_mlp_store_windows(const KArgs<double>& a, const MlpArgs<double>& c, unsigned i, const double* col, int s)
{
    const int H = c.history, q = s % H;
    for (int k = 0, row = q ? H - q : 0; k < H; ++k) {
        at(rowv(c.cgm_hist, a.n, k), i) = col[row * 64];
        at(rowv(c.ins_hist, a.n, k), i) = col[(H + row) * 64];
        row = row + 1 == H ? 0 : row + 1;
    }
}

// a step closes under the policy: its four trace columns (row tr), prev_meal and the statistics
__device__ __forceinline__ void dopri5_mlp_step_words(const MlpArgs<double>& c, unsigned i, int64_t tr, const StepOut<double>& o)
{
    if (c.bg_trace) c.bg_trace[tr] = o.bg;
    if (c.cgm_trace) c.cgm_trace[tr] = o.cgm;
    if (c.cho_trace) c.cho_trace[tr] = o.meal;
    if (c.ins_trace) c.ins_trace[tr] = o.ins;
    at(c.prev_meal, i) = o.meal;
    if (c.sum_risk) { double l, h, rk; risk_index1<0>(o.bg, l, h, rk); at(c.sum_risk, i) = at(c.sum_risk, i) + rk; }
    if (c.min_bg) { const double v = at(c.min_bg, i); at(c.min_bg, i) = o.bg < v ? o.bg : v; }
    if (c.max_bg) { const double v = at(c.max_bg, i); at(c.max_bg, i) = o.bg > v ? o.bg : v; }
    if (c.n_low) at(c.n_low, i) = at(c.n_low, i) + (o.bg < 70.0);
    if (c.n_high) at(c.n_high, i) = at(c.n_high, i) + (o.bg > 180.0);
}

__global__ __launch_bounds__(kBlock, 1) void dopri5_mlp_rollout_kernel(const KArgs<double> a, const MlpArgs<double> c,
                                                                       const double* __restrict__ raw, double* h_carry, int32_t* nfev)
{
    // its own: c's windows, with their load, store and step words as lines of the loop (above: the three functions); where
    // a step opens, the network on them, no bolus
#define DOPRI5_WINDOWS c
#define DOPRI5_WRITTEN_OUT
#define DOPRI5_ACTION                                                                                                         \
    const double u = mlp_action(c, mlp_wave_weights(c, i), col, buf, head, prev_meal, start + e.t);                            \
    if (c.act_trace) c.act_trace[(c.trace_row + s) * a.n + i] = u;                                                             \
    const double bolus = 0.0;
#include "t1d_dopri5_loop.inc"
}

// ---- t1d_rollout_mlp_dopri5_bolus: the roll-out above with the meal bolus of t1d_meal_bolus (t1d_policy.hpp) -----------------
// The bolus is formed where a step opens, next to mlp_action: meal_bolus -- the function of the fixed-step kernels -- on the
// column's CGM[0] (the observation the step starts from) and the prev_meal read there, to bolus_trace, then into the q_bolus
// quantiser call that receives 0.0 above.  Like the network's words, nothing of it is in a register across dopri5_attempt.
// A kernel of its own and not a run-time switch inside dopri5_mlp_rollout_kernel: that kernel's text moved into a function
// shared by two wrappers no longer compiled to the same instructions (13 987 and 14 070 against 13 879, by reference and by
// value), and it is the one whose machine code has to stay (tools/isa_diff.py).
__global__ __launch_bounds__(kBlock, 1) void dopri5_mlp_rollout_bolus_kernel(const KArgs<double> a, const MlpArgs<double> c,
                                                                             const BolusArgs<double> mb, const double* __restrict__ raw,
                                                                             double* h_carry, int32_t* nfev)
{
    // its own: c's windows; where a step opens, the network on them and the meal bolus
#define DOPRI5_WINDOWS c
#define DOPRI5_ACTION                                                                                                          \
    const double u = mlp_action(c, mlp_wave_weights(c, i), col, buf, head, prev_meal, start + e.t);                            \
    if (c.act_trace) c.act_trace[(c.trace_row + s) * a.n + i] = u;                                                             \
    const double bolus = step_bolus(mb, bolus_lane(mb, i), i, double(a.sen.st), col[head * 64], prev_meal,                     \
                                    (c.trace_row + s) * a.n + i);
#include "t1d_dopri5_loop.inc"
}

// ---- t1d_rollout_mlp_dopri5_rel: the roll-out under a relative policy (t1d_env_output, t1d_policy.hpp) ----------------------
// dopri5_mlp_rollout_bolus_kernel with the action formed under the lane's scale and bias and the meal bolus a wave-uniform
// switch (mb.cr == NULL: none).  The pair is loaded in the boundary block where a step opens, next to the network: like the
// network's words and the bolus, nothing of it is in a register across dopri5_attempt.  A kernel of its own for the reason
// given above: the kernels that exist keep their machine code.
__global__ __launch_bounds__(kBlock, 1) void dopri5_mlp_rollout_rel_kernel(const KArgs<double> a, const MlpArgs<double> c,
                                                                           const EnvOutArgs<double> eo, const BolusArgs<double> mb,
                                                                           const double* __restrict__ raw, double* h_carry, int32_t* nfev)
{
    // its own: c's windows; where a step opens, the network under the lane's pair and, where there is one, the meal bolus
#define DOPRI5_WINDOWS c
#define DOPRI5_ACTION                                                                                                          \
    const double u = mlp_action(c, mlp_wave_weights(c, i), col, buf, head, prev_meal, start + e.t, env_out_lane(eo, i));       \
    if (c.act_trace) c.act_trace[(c.trace_row + s) * a.n + i] = u;                                                             \
    double bolus = 0.0;                                                                                                        \
    if (mb.cr) /* wave-uniform */                                                                                              \
        bolus = step_bolus(mb, bolus_lane(mb, i), i, double(a.sen.st), col[head * 64], prev_meal, (c.trace_row + s) * a.n + i);
#include "t1d_dopri5_loop.inc"
}

// ---- trajectories for a policy-gradient trainer in the exact mode (t1d_collect_mlp_dopri5) ------------------------------
// dopri5_mlp_rollout_kernel with the collector's work (mlp_collect_body, t1d_policy.hpp) in the boundary block.  A kernel of
// its own: the roll-out keeps its registers and its arguments.
//   a step opens    mlp_action in its three parts: the features (to feat_trace), the layers, then the draw -- keyed by the
//                   env's global id, its episode counter and its clock, as in mlp_collect_body -- and sigma on the last
//                   layer's output, the output function, the pump.  eps_trace is written here: the step that uses the
//                   draw is the row it describes, and nothing of it has to wait for the step's end.
//   a step closes   reward and done as write_outputs forms them, to their trace rows; ep_return / ep_length advance.
//   done, restart   the loop's DOPRI5_COLLECT part (t1d_dopri5_loop.inc).
// Nothing of the policy, the draw or the restart is in a register across dopri5_attempt.
// DOPRI5_MLP_COLLECT_ACTION: the action of this kernel and of dopri5_mlp_collect_limit_kernel.
#define DOPRI5_MLP_COLLECT_ACTION                                                                                              \
    typedef const __attribute__((address_space(4))) double* WPtr;                                                              \
    const unsigned wave0 = __builtin_amdgcn_readfirstlane(i & ~63u);                                                           \
    const unsigned pol = wave0 / c.envs_per_policy;                                                                            \
    const WPtr w = (WPtr)(c.params + (size_t)pol * (size_t)c.n_params);                                                        \
    mlp_features(c, col, buf, head, prev_meal, start + e.t);                                                                   \
    if (g.feat_trace)                                                                                                          \
        for (int j = 0; j < F; ++j) g.feat_trace[((c.trace_row + s) * F + j) * a.n + i] = buf[j * 64];                         \
    double y = mlp_layers(c, w, buf, F);                                                                                       \
    double eps = 0.0;                                                                                                          \
    if (g.sigma) { /* wave-uniform */                                                                                          \
        const uint32_t ep = a.episode ? at(a.episode, i) : 0u;                                                                 \
        eps = (double)philox_pair(g.explore_seed, (uint64_t)(a.env_offset + i), ep, (uint32_t)e.t).x;                          \
        y = fma((double)((WPtr)g.sigma)[pol], eps, y);                                                                         \
    }                                                                                                                          \
    if (g.eps_trace) g.eps_trace[(c.trace_row + s) * a.n + i] = eps;                                                           \
    const double u = mlp_output(c, y);                                                                                         \
    if (c.act_trace) c.act_trace[(c.trace_row + s) * a.n + i] = u;                                                             \
    const double bolus = 0.0;
__global__ __launch_bounds__(kBlock, 1) void dopri5_mlp_collect_kernel(const KArgs<double> a, const MlpArgs<double> c,
                                                                       const CollectArgs<double> g, const RestartArgs<double> ra,
                                                                       const double* __restrict__ raw, double* h_carry, int32_t* nfev)
{
    // its own: c's windows, the collector's frame; where a step opens, features, layers, the draw, the output function
#define DOPRI5_WINDOWS c
#define DOPRI5_COLLECT
#define DOPRI5_ACTION DOPRI5_MLP_COLLECT_ACTION
#include "t1d_dopri5_loop.inc"
}

// ---- trajectories under the two hand-written controllers in the exact mode (t1d_collect_pid_dopri5 / t1d_collect_bb_dopri5) ----
// dopri5_mlp_collect_kernel with dopri5_controller where the network stands, and the feature bookkeeping of ctrl_collect_body
// (t1d_policy.hpp).  The wave's piece of dynamic LDS is Cold's words and cols = 4 H + 3 columns -- the two windows as a ring
// with a per-lane head, then the F = 2 H + 3 features; there are no activation columns.
//   a step opens    the features a network would have been given (mlp_features, to feat_trace), then dopri5_controller on the
//                   last observation with its state in memory -- the word t1d_rollout_pid_dopri5 / t1d_rollout_bb_dopri5
//                   computes -- then basal + bolus to the policy's action trace, then the pump on each.
//   a step closes   outputs, reward and done, the controller's four trace columns, both prev_meal words, the accumulators,
//                   the ring head.
//   done, restart   as in dopri5_mlp_collect_kernel; the controller's state in memory becomes what PIDController.reset /
//                   BBController.reset leave.
// Every trace row index is the controller's trace_row (PidArgs), as in ctrl_collect_kernel; n_steps is the controller's too.
// No network runs: there is no wave-uniform weight pointer, no lane looks at another, and n may be any number.
// Nothing of the features, the controller or the restart is in a register across dopri5_attempt.
//
// The restart is inlined (collect_restart), as in the other collectors.  Tried as a real call of this kernel's own
// (__noinline__, arguments by value): 158 spilled VGPRs instead of 347 and a fifth less time at 1 Mi envs, but WRONG -- envs
// that did not restart came back with other state words and garbage in h_carry once another lane of their wave had made the
// call (profiles/collect/README.md).  Do not move the restart out of line without the restart test of
// tests/test_gpu_collect_ctrl_dopri5.py.
// DOPRI5_CTRL_COLLECT_ACTION: the action of this kernel and of dopri5_ctrl_collect_limit_kernel.  What the controller asked
// for goes to the action trace before the pump: one addition, contraction off.
#define DOPRI5_CTRL_COLLECT_ACTION                                                                                             \
    mlp_features(f, col, buf, head, prev_meal, start + e.t);                                                                   \
    if (g.feat_trace)                                                                                                          \
        for (int j = 0; j < F; ++j) g.feat_trace[((c.trace_row + s) * F + j) * a.n + i] = buf[j * 64];                         \
    double u, bolus;                                                                                                           \
    dopri5_controller(c, i, at(a.cgm, i), st, u, bolus);                                                                       \
    if (f.act_trace) {                                                                                                         \
        _Pragma("clang fp contract(off)")                                                                                      \
        f.act_trace[(c.trace_row + s) * a.n + i] = u + bolus;                                                                  \
    }
__global__ __launch_bounds__(kBlock, 1) void dopri5_ctrl_collect_kernel(const KArgs<double> a, const PidArgs<double> c,
                                                                        const MlpArgs<double> f, const CollectArgs<double> g,
                                                                        const RestartArgs<double> ra, const double* __restrict__ raw,
                                                                        double* h_carry, int32_t* nfev)
{
    // its own: f's windows, PidArgs' words, the collector's frame; where a step opens, the features, then the controller
#define DOPRI5_STATE
#define DOPRI5_BB
#define DOPRI5_WINDOWS f
#define DOPRI5_COLLECT
#define DOPRI5_ACTION DOPRI5_CTRL_COLLECT_ACTION
#include "t1d_dopri5_loop.inc"
}

// ---- the two collectors above with episodes cut at a time limit (t1d_collect_mlp_dopri5_limit, t1d_collect_pid_dopri5_limit,
// t1d_collect_bb_dopri5_limit; LimitArgs, t1d_policy.hpp) ------------------------------------------------------------------
// dopri5_mlp_collect_kernel and dopri5_ctrl_collect_kernel with a LimitArgs behind their arguments.  Kernels of their own and
// not a run-time switch in those two: the two kernels above keep their registers and their instruction streams.  What differs
// is the loop's DOPRI5_LIMIT part, in the boundary block, where a step closes:
//   cut             !fin and the env's clock e.t has reached max_minutes; to cut_trace's row of the step.  Termination wins.
//   a cut env       in the restart branch, before anything of it goes to memory: its cut features to cut_feat.  Then the restart
//                   of a finished env, with collect_restart_masked (its done byte is 0) where collect_restart stands.
// The restart stays inlined (the comment above dopri5_ctrl_collect_kernel).  Of the limit only max_minutes, a kernel argument, is
// looked at outside the cut branch, and nothing of it is in a register across dopri5_attempt.
__global__ __launch_bounds__(kBlock, 1) void dopri5_mlp_collect_limit_kernel(const KArgs<double> a, const MlpArgs<double> c,
                                                                             const CollectArgs<double> g, const RestartArgs<double> ra,
                                                                             const LimitArgs<double> lim, const double* __restrict__ raw,
                                                                             double* h_carry, int32_t* nfev)
{
#define DOPRI5_WINDOWS c
#define DOPRI5_COLLECT
#define DOPRI5_LIMIT
#define DOPRI5_ACTION DOPRI5_MLP_COLLECT_ACTION
#include "t1d_dopri5_loop.inc"
}

__global__ __launch_bounds__(kBlock, 1) void dopri5_ctrl_collect_limit_kernel(const KArgs<double> a, const PidArgs<double> c,
                                                                              const MlpArgs<double> f, const CollectArgs<double> g,
                                                                              const RestartArgs<double> ra, const LimitArgs<double> lim,
                                                                              const double* __restrict__ raw, double* h_carry, int32_t* nfev)
{
#define DOPRI5_STATE
#define DOPRI5_BB
#define DOPRI5_WINDOWS f
#define DOPRI5_COLLECT
#define DOPRI5_LIMIT
#define DOPRI5_ACTION DOPRI5_CTRL_COLLECT_ACTION
#include "t1d_dopri5_loop.inc"
}
#undef DOPRI5_MLP_COLLECT_ACTION
#undef DOPRI5_CTRL_COLLECT_ACTION

// t1d_mlp_action: the policy alone, one lane per env -- the action the next step of a roll-out would ask for, from
// batch.cgm (CGM[0]), rows 1 .. of cgm_hist, ins_hist, prev_meal, batch.t and start_minute.  Reads only; writes action [n].
// Dynamic LDS: cols * 64 words for each wave, the lane's column in window order (head 0).
template <typename T>
__global__ __launch_bounds__(T1D_POLICY_THREADS) void mlp_action_kernel(const KArgs<T> a, const MlpArgs<T> c, T* action)
{
    const unsigned i = blockIdx.x * blockDim.x + threadIdx.x;
    __builtin_assume(i < (1u << 28));          // host guarantees n <= 2^28: i * sizeof(T) fits a 32-bit voffset
    if ((int64_t)i >= a.n) return;
    T* const col = (T*)t1d_dyn_lds + (threadIdx.x >> 6) * (c.cols * 64) + (threadIdx.x & 63u);
    const int H = c.history;
    col[0] = at(a.cgm, i);
    for (int k = 1; k < H; ++k) col[k * 64] = at(rowv(c.cgm_hist, a.n, k), i);
    for (int k = 0; k < H; ++k) col[(H + k) * 64] = at(rowv(c.ins_hist, a.n, k), i);
    const int start = c.start_minute ? (int)at(c.start_minute, i) : 0;
    const T prev_meal = at(c.prev_meal, i);
    const int t = at(a.t, i);
    action[i] = mlp_action(c, mlp_wave_weights(c, i), col, col + 2 * H * 64, 0, prev_meal, start + t);
}

// t1d_mlp_action_rel: mlp_action_kernel under a relative policy -- the action with the lane's scale and bias (t1d_env_output)
template <typename T>
__global__ __launch_bounds__(T1D_POLICY_THREADS) void mlp_action_rel_kernel(const KArgs<T> a, const MlpArgs<T> c, const EnvOutArgs<T> eo, T* action)
{
    const unsigned i = blockIdx.x * blockDim.x + threadIdx.x;
    __builtin_assume(i < (1u << 28));          // host guarantees n <= 2^28: i * sizeof(T) fits a 32-bit voffset
    if ((int64_t)i >= a.n) return;
    T* const col = (T*)t1d_dyn_lds + (threadIdx.x >> 6) * (c.cols * 64) + (threadIdx.x & 63u);
    const int H = c.history;
    col[0] = at(a.cgm, i);
    for (int k = 1; k < H; ++k) col[k * 64] = at(rowv(c.cgm_hist, a.n, k), i);
    for (int k = 0; k < H; ++k) col[(H + k) * 64] = at(rowv(c.ins_hist, a.n, k), i);
    const int start = c.start_minute ? (int)at(c.start_minute, i) : 0;
    const T prev_meal = at(c.prev_meal, i);
    const int t = at(a.t, i);
    action[i] = mlp_action(c, mlp_wave_weights(c, i), col, col + 2 * H * 64, 0, prev_meal, start + t, env_out_lane(eo, i));
}

} // namespace t1d
