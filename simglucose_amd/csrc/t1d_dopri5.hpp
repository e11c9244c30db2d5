// t1d_dopri5.hpp -- the exact mode: scipy.integrate.ode('dopri5') as the reference drives it (t1dpatient.py:110-113,276),
// one lane per env, fp64 only.  Included by t1d_abi.hip after t1d_kernels.hpp; launched by t1d_step_dopri5 (include/t1d.h).
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
// Each lane runs its own accept/reject loop; a wave runs until its slowest lane is done.  The loop ends on every input: a
// lane gives up after nmax steps or when the step underflows (NaN states included), which the kernel reports as
// T1D_ST_SOLVER_FAILED -- where the reference raises "ODE solver failed".
#pragma once
#include "t1d_kernels.hpp"

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

// t1d_o_dopri5_minute: one integrate() from x = t_start to t_start + 1.  y: the state, advanced in place (left at the last
// accepted point if the solver gives up); h_carry: the predicted step, read (0 = probe) and written on success; nfcn: RHS
// evaluations of this call, added.  Returns false where the driver gives up (nmax steps, or a step below the resolution of x).
__device__ __forceinline__ bool dopri5_minute(const ParsRaw& p, double (&y)[13], double d, double ins, double lq, double lf,
                                              double& h_carry, double t_start, int& nfcn)
{
#pragma clang fp contract(off)
    const double a21 = 0.2, a31 = 3.0 / 40.0, a32 = 9.0 / 40.0, a41 = 44.0 / 45.0,
        a42 = -56.0 / 15.0, a43 = 32.0 / 9.0, a51 = 19372.0 / 6561.0, a52 = -25360.0 / 2187.0,
        a53 = 64448.0 / 6561.0, a54 = -212.0 / 729.0, a61 = 9017.0 / 3168.0, a62 = -355.0 / 33.0,
        a63 = 46732.0 / 5247.0, a64 = 49.0 / 176.0, a65 = -5103.0 / 18656.0, a71 = 35.0 / 384.0,
        a73 = 500.0 / 1113.0, a74 = 125.0 / 192.0, a75 = -2187.0 / 6784.0, a76 = 11.0 / 84.0,
        e1 = 71.0 / 57600.0, e3 = -71.0 / 16695.0, e4 = 71.0 / 1920.0, e5 = -17253.0 / 339200.0,
        e6 = 22.0 / 525.0, e7 = -1.0 / 40.0;
    const double rtol = 1e-6, atol = 1e-12, safe = 0.9, fac1 = 0.2, fac2 = 10.0, uround = 2.3e-16, beta = 0.04;
    const int nmax = 500;
    const double expo1 = 0.2 - beta * 0.75, facc1 = 1.0 / fac1, facc2 = 1.0 / fac2;
    const double xend = t_start + 1.0, hmax = 1.0;
    double x = t_start, h = h_carry, facold = 1e-4;
    double k1[13], k2[13], k3[13], k4[13], k5[13], k6[13], y1[13], ysti[13];
    int nstep = 0;
    bool last = false, reject = false;

    rhs_scipy(p, y, d, ins, lq, lf, k1); nfcn++;          // SciPy re-enters the driver every minute: a fresh first stage
    if (h == 0.0) { h = dopri5_hinit(p, y, k1, d, ins, lq, lf, hmax, atol, rtol); nfcn++; }
    for (;;) {
        if (nstep > nmax) return false;
        if (0.1 * fabs(h) <= fabs(x) * uround) return false;
        if ((x + 1.01 * h - xend) > 0.0) { h = xend - x; last = true; }
        nstep++;
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
        double fac = fac11 / pow(facold, beta);
        fac = fmax(facc2, fmin(facc1, fac / safe));
        double hnew = h / fac;
        if (err <= 1.0) {
            facold = fmax(err, 1e-4);
#pragma unroll
            for (int i = 0; i < 13; ++i) { k1[i] = k2[i]; y[i] = y1[i]; }
            x += h;
            if (last) { h_carry = hnew; return true; }
            if (fabs(hnew) > hmax) hnew = hmax;
            if (reject) hnew = fmin(fabs(hnew), fabs(h));
            reject = false;
        } else {
            hnew = h / fmin(facc1, fac11 / safe);
            reject = true;
            last = false;
        }
        h = hnew;
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

} // namespace t1d
