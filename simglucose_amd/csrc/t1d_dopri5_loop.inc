// t1d_dopri5_loop.inc -- the body of the nine closed-loop kernels of the exact mode (t1d_dopri5.hpp), included between the
// braces of each: the free-running DOPRI5 loop, once.  a, c, raw, h_carry and nfev are the kernel's arguments: c carries
// n_steps, trace_row, the four trace columns and the statistics (a PidArgs, a PidGainArgs or an MlpArgs).
//
// The loop.  Its body is ONE step attempt of the driver (dopri5_attempt) for every lane that still has work.  Ahead of it,
// only the lanes that have just completed a minute (or enter their first) run the boundary block:
//   finish the minute    cold.load, the clock, Gsub, the CGM sample, the step's means -- as dopri5_step_kernel does;
//   a step closes        write_outputs, then the roll-out's own: the trace row, prev_meal, the statistics; m = 0, ++s; with
//                        windows the ring head; in a collector reward / done / cut and the restart of an env that is done;
//   s == n_steps         the lane leaves the loop;
//   a step opens         the kernel's DOPRI5_ACTION (controller or network), the pump, the step's sums cleared;
//   a minute opens       meal_lookup, measure_noise, eat_minute, dopri5_enter, cold.save.
// Behind the loop the epilogue: state, h_carry, nfev, the status word, the windows back in window order.
// A lane whose solver gives up (failed) takes no more step attempts: it walks through its boundary blocks alone.
//
// What a kernel defines ahead of the include (all of it is undefined again at the end of this file):
//   DOPRI5_ACTION        statements, where a step opens: they declare u (the basal asked for) and bolus, write the action's
//                        trace and whatever else is the kernel's own there.  With DOPRI5_WINDOWS they see head (the ring's
//                        head row), start (start_minute) and prev_meal; with DOPRI5_STATE st, the sensor's sample time.
//   DOPRI5_STATE         a hand-written controller acts on the last observation: st is needed.  Without DOPRI5_WINDOWS the
//                        kernel has no dynamic LDS: RollCold, static, stride kBlock (the workgroup is kBlock lanes).
//   DOPRI5_BB            c is a PidArgs: bb_prev_meal follows the step's meal under BBController, and a restart resets the
//                        controller's words.
//   DOPRI5_WINDOWS w     w is the MlpArgs whose two windows the kernel keeps: the wave's piece of dynamic LDS is
//                        RollColdT<64>'s words, then the columns (t1d_dopri5.hpp: where the policy's words live); the
//                        workgroup's size is the launch's.  w.prev_meal follows the step's meal.
//   DOPRI5_WRITTEN_OUT   (dopri5_mlp_rollout_kernel alone) the windows' load and store and the step's words are lines of this
//                        text where the other window kernels call dopri5_mlp_load_windows / _store_windows / _step_words.
//   DOPRI5_COLLECT       a collector: g (CollectArgs) and ra (RestartArgs) are arguments.  Needs DOPRI5_WINDOWS.
//   DOPRI5_LIMIT         ... with episodes cut at a time limit: lim (LimitArgs) is an argument.  Needs DOPRI5_COLLECT.
//
// Why text and not functions: these kernels fill the unified register file, and their machine code follows the shape of the
// source.  Found when the nine bodies were folded into this file (cross-compiled, every kernel's instruction stream compared
// with tools/isa_diff.py; profiles/dopri5/isa_diff_loop.txt):
//   - pieces substituted as text -- preprocessor definitions, #if -- left every stream as it was: all nine kernels compile
//     to the instructions they had as nine written-out bodies.
//   - the same lines behind a __forceinline__ function and in place are two different things to the compiler, in both
//     directions.  dopri5_rollout_kernel's loop in a function: 11 892 instructions before and after, in another order.  The
//     two controller collectors with the cut test, cut trace, cut features and the restart call behind functions overloaded on
//     LimitArgs / an empty tag: 20 261 against 19 988 and 20 811 against 20 511.
//   - which is why DOPRI5_WRITTEN_OUT exists.  With the three calls, dopri5_mlp_rollout_kernel has 13 887 instructions
//     against 13 879 (any one of them moves it: 13 882 - 13 884) and was 0.5 - 0.7 % slower at 1 Mi envs
//     (profiles/policy/kernel_resources_collect_exact.txt).  With the lines in place, the six kernels that have always made
//     the calls move instead -- bolus 14 062 against 14 069, rel 14 349 against 14 119, the collectors 21 527 / 21 530,
//     19 983 / 19 988, 22 050 / 22 018, 20 486 / 20 511 -- and two of them spill more: dopri5_mlp_rollout_rel_kernel 70 VGPRs
//     against 0, dopri5_mlp_collect_limit_kernel 356 against 338.  The four collectors follow dopri5_mlp_load_windows alone,
//     the bolus and rel roll-outs need dopri5_mlp_step_words as well.  Reading the structs through references instead of the
//     kernel's arguments made no difference to any of them.
//   - the wave's piece of LDS and the pump, once functions of their own (dopri5_mlp_lane_lds, dopri5_mlp_pump), moved nothing
//     either way and are lines of this text now.
#if defined(DOPRI5_LIMIT) && !defined(DOPRI5_COLLECT) || defined(DOPRI5_COLLECT) && !defined(DOPRI5_WINDOWS)
#error "DOPRI5_LIMIT needs DOPRI5_COLLECT, DOPRI5_COLLECT needs DOPRI5_WINDOWS"
#endif
    __shared__ double lds[kRawPars * kMaxPatients];
#ifdef DOPRI5_WINDOWS
    typedef RollColdT<64> Cold;
    constexpr int kColdStride = 64;
#else
    typedef RollCold Cold;
    constexpr int kColdStride = kBlock;
    __shared__ double cold_f[Cold::NF * kBlock];
    __shared__ int cold_w[Cold::NI * kBlock];
#endif
    for (int j = threadIdx.x; j < kRawPars * kMaxPatients; j += blockDim.x) lds[j] = raw[j];
    __syncthreads();
#ifdef DOPRI5_WINDOWS
    const unsigned i = blockIdx.x * blockDim.x + threadIdx.x;
#else
    const unsigned i = blockIdx.x * kBlock + threadIdx.x;
#endif
    __builtin_assume(i < (1u << 28));          // host guarantees n <= 2^28: i * sizeof(T) fits a 32-bit voffset
    if ((int64_t)i >= a.n) return;             // the lanes past the end leave, the others never look at them
#ifdef DOPRI5_WINDOWS
    // the wave's piece of dynamic LDS: Cold's doubles, Cold's ints, the columns
    unsigned char* const piece = t1d_dyn_lds + (threadIdx.x >> 6) * (kRollColdWaveBytes + DOPRI5_WINDOWS.cols * 64 * (int)sizeof(double));
    const unsigned lane = threadIdx.x & 63u;
    const Cold cold{(double*)piece + lane, (int*)(piece + Cold::NF * 64 * sizeof(double)) + lane};
    double* const col = (double*)(piece + kRollColdWaveBytes) + lane;
    const int H = DOPRI5_WINDOWS.history;
#ifdef DOPRI5_COLLECT
    const int F = 2 * H + 3;
#endif
    double* const buf = col + 2 * H * 64;
#endif
    const uint32_t meta = at(a.meta, i);
    const uint32_t pid = T1D_META_PID(meta);
    Env<double> e;
    load_env(a, i, meta, e);
    const ParsRaw p{lds, (int)pid};
    NoDerivedPars nop;
#ifndef DOPRI5_WINDOWS
    const Cold cold{cold_f + threadIdx.x, cold_w + threadIdx.x};
#endif
    const double div = double(a.minutes);
#ifdef DOPRI5_STATE
    const double st = double(a.sen.st);
#endif
#if defined(DOPRI5_WINDOWS) && !defined(DOPRI5_WRITTEN_OUT)
    dopri5_mlp_load_windows(a, DOPRI5_WINDOWS, i, col);
#elif defined(DOPRI5_WINDOWS)
    col[0] = at(a.cgm, i);                                      // CGM[0] is the observation the first step starts from
    for (int k = 1; k < H; ++k) col[k * 64] = at(rowv(DOPRI5_WINDOWS.cgm_hist, a.n, k), i);
    for (int k = 0; k < H; ++k) col[(H + k) * 64] = at(rowv(DOPRI5_WINDOWS.ins_hist, a.n, k), i);
#endif
    double hc = at(h_carry, i), noise = 0.0, insulin = 0.0, d_mg = 0.0;
    StepOut<double> o{0.0, 0.0, 0.0, 0.0};
    Dopri5Run r{};
    int nf = 0, m = 0, s = 0;
    bool due = false, failed = false, boundary = true, fresh = true;
#ifdef DOPRI5_COLLECT
    bool stored = false;                        // the last step ended the episode: the state in memory is the new episode's
#endif
    cold.save(e, o, noise, hc);
    for (;;) {
        if (boundary) {
            cold.load(e, o, noise, hc);
            if (!fresh) {
                e.t += 1;
                const double gsub = e.x[12] / p(T1D_P_VG);                                    // t1dpatient.py:217-218
                const double cgm = measure_apply(a, e, gsub, noise, due);                     // env.py:62
                o.bg += gsub / div; o.cgm += cgm / div;                                       // env.py:80-81
                if (++m == a.minutes) {                  // the step is complete: what t1d_step_dopri5 leaves, then the kernel's own
                    const double rp = e.prev_risk;
                    write_outputs<0>(a, i, e, o, rp);
#ifdef DOPRI5_COLLECT
                    const double reward = rp - e.prev_risk;     // the word write_outputs stored in batch.reward
                    const bool fin = o.bg < 70.0 || o.bg > 350.0;
#ifdef DOPRI5_LIMIT
                    const bool cut = !fin && e.t >= lim.max_minutes;    // the time limit ends the episode here (never a finished one)
#endif
#endif
                    const int64_t tr = (c.trace_row + s) * a.n + i;
#ifdef DOPRI5_COLLECT
                    if (g.reward_trace) g.reward_trace[tr] = reward;
                    if (g.done_trace) g.done_trace[tr] = fin ? 1 : 0;
#ifdef DOPRI5_LIMIT
                    if (lim.cut_trace) lim.cut_trace[tr] = cut ? 1 : 0;
#endif
#endif
#if defined(DOPRI5_WINDOWS) && !defined(DOPRI5_STATE) && !defined(DOPRI5_WRITTEN_OUT)
                    dopri5_mlp_step_words(c, i, tr, o);
#else
                    if (c.bg_trace) c.bg_trace[tr] = o.bg;
                    if (c.cgm_trace) c.cgm_trace[tr] = o.cgm;
                    if (c.cho_trace) c.cho_trace[tr] = o.meal;
                    if (c.ins_trace) c.ins_trace[tr] = o.ins;
#ifdef DOPRI5_BB
                    if (c.kind == 1) at(c.bb_prev_meal, i) = o.meal;
#endif
#ifdef DOPRI5_WINDOWS
                    at(DOPRI5_WINDOWS.prev_meal, i) = o.meal;
#endif
                    if (c.sum_risk) { double l, h, rk; risk_index1<0>(o.bg, l, h, rk); at(c.sum_risk, i) = at(c.sum_risk, i) + rk; }
                    if (c.min_bg) { const double v = at(c.min_bg, i); at(c.min_bg, i) = o.bg < v ? o.bg : v; }
                    if (c.max_bg) { const double v = at(c.max_bg, i); at(c.max_bg, i) = o.bg > v ? o.bg : v; }
                    if (c.n_low) at(c.n_low, i) = at(c.n_low, i) + (o.bg < 70.0);
                    if (c.n_high) at(c.n_high, i) = at(c.n_high, i) + (o.bg > 180.0);
#endif
                    m = 0; ++s;
#ifdef DOPRI5_WINDOWS
                    // The lanes of a wave are in different steps, so the ring's head is per lane: after s steps of this launch
                    // CGM[0] sits in row (H - s mod H) mod H.  The oldest row becomes the newest.
                    const int q = s % H, head = q ? H - q : 0;
                    col[head * 64] = o.cgm; col[(H + head) * 64] = o.ins;
#endif
#ifdef DOPRI5_COLLECT
                    // done, restart: the lane writes its state as the end of the launch would, runs the restart --
                    // t1d_restart_done for this env alone, on the words in memory --, loads the new episode, fills its window
                    // rows with the new first observation and starts again with prev_meal = 0, a carried step of 0 and a
                    // working solver.  The ring head stays where the lane's step counter puts it: every row holds the same
                    // word.  start_minute, the episode counter and prev_meal are read from memory where a step opens, so the
                    // new ones are picked up there; the Cold words are saved again at the end of the boundary block.  The
                    // other lanes of the wave are inactive meanwhile and go on with their step attempts afterwards.
                    if (g.on_done) {
#ifdef DOPRI5_LIMIT
                        if (fin || cut) {
                            // a cut env, before anything of it goes to memory: its cut features -- mlp_features on the shifted
                            // windows (the head just computed), the step's meal (the word prev_meal has just been given) and
                            // the clock start_minute + e.t, what t1d_mlp_features would return; buf is free between two steps
                            if (cut && lim.cut_feat) {
                                const int start = DOPRI5_WINDOWS.start_minute ? (int)at(DOPRI5_WINDOWS.start_minute, i) : 0;
                                mlp_features(DOPRI5_WINDOWS, col, buf, head, o.meal, start + e.t);
                                for (int j = 0; j < F; ++j) at(rowv(lim.cut_feat, a.n, j), i) = buf[j * 64];
                            }
#else
                        if (fin) {
#endif
                            // the finished step is in memory (write_outputs); the state follows, and the restart works on those words
                            store_env(a, i, pid, e);
                            if (failed) atomicOr(a.status, T1D_ST_SOLVER_FAILED);
#ifdef DOPRI5_LIMIT
                            collect_restart_masked<double>(a, ra, g.slots, i);          // a cut env's done is 0
#else
                            collect_restart<double>(a, ra, g.slots, i);
#endif
                            load_env(a, i, at(a.meta, i), e);
                            const double first = at(a.cgm, i);  // the new episode's first observation
                            for (int k = 0; k < H; ++k) { col[k * 64] = first; col[(H + k) * 64] = 0.0; }
                            at(DOPRI5_WINDOWS.prev_meal, i) = 0.0;
#ifdef DOPRI5_BB
                            if (c.kind == 1) at(c.bb_prev_meal, i) = 0.0;                     // BBController.reset
                            else { at(c.integ, i) = 0.0; at(c.prev, i) = 0.0; }               // PIDController.reset
#endif
                            hc = 0.0;                           // T1DPatient.reset builds the solver afresh: the first minute probes
                            failed = false;
                            stored = s == c.n_steps;
                        } else if (ra.ep_return) {              // restart_front's accumulators for an env that goes on
                            const double sum = at(ra.ep_return, i) + reward;
                            const int len = at(ra.ep_length, i) + 1;
                            at(ra.ep_return, i) = sum; at(ra.ep_length, i) = len;
                        }
                    }
#endif
                }
            }
            if (s == c.n_steps) break;
            if (m == 0) {                                // a step opens: the kernel's action, then the pump
#ifdef DOPRI5_WINDOWS
                const int q = s % H, head = q ? H - q : 0;
                const int start = DOPRI5_WINDOWS.start_minute ? (int)at(DOPRI5_WINDOWS.start_minute, i) : 0;
                const double prev_meal = at(DOPRI5_WINDOWS.prev_meal, i);
#endif
                DOPRI5_ACTION
                double q_basal = u, q_bolus = bolus;     // as step_body with a bolus given: env.py:51-52
                if (!(a.flags & T1D_BATCH_NO_PUMP)) {
                    q_basal = pump_quantise(u, a.pump.inc_basal, a.pump.min_basal, a.pump.max_basal);
                    q_bolus = pump_quantise(bolus, a.pump.inc_bolus, a.pump.min_bolus, a.pump.max_bolus);
                }
                insulin = q_basal + q_bolus;
                o = StepOut<double>{0.0, 0.0, 0.0, 0.0};
            }
            const double meal = meal_lookup(a, i, e);                                         // env.py:50
            noise = measure_noise<true>(a, i, e, due);
            const MinuteIn<double> u = eat_minute<0, double>(nop, e.x, meal, insulin, e.planned, e.lq, e.lf, e.eating);
            d_mg = u.d_mg;
            o.meal += meal / div; o.ins += insulin / div;                                     // env.py:78-79
            if (!failed) dopri5_enter(p, e.x, d_mg, insulin, e.lq, e.lf, hc, (double)e.t, r, nf);
            cold.save(e, o, noise, hc);
            fresh = false; boundary = false;
        }
        if (failed) { boundary = true; continue; }
        const int rc = dopri5_attempt(p, e.x, d_mg, insulin, e.lq, e.lf, cold.f[Cold::HC * kColdStride], (double)e.t + 1.0, r, nf);
        failed = rc < 0;
        boundary = rc != 0;
    }
#ifdef DOPRI5_COLLECT
    if (!stored)
#endif
    store_env(a, i, pid, e);
    at(h_carry, i) = hc;
    if (nfev) at(nfev, i) = nf;
    if (failed) atomicOr(a.status, T1D_ST_SOLVER_FAILED);
#if defined(DOPRI5_WINDOWS) && !defined(DOPRI5_WRITTEN_OUT)
    dopri5_mlp_store_windows(a, DOPRI5_WINDOWS, i, col, s);
#elif defined(DOPRI5_WINDOWS)
    const int q = s % H;
    for (int k = 0, row = q ? H - q : 0; k < H; ++k) {         // the windows back in window order
        at(rowv(DOPRI5_WINDOWS.cgm_hist, a.n, k), i) = col[row * 64];
        at(rowv(DOPRI5_WINDOWS.ins_hist, a.n, k), i) = col[(H + row) * 64];
        row = row + 1 == H ? 0 : row + 1;
    }
#endif
#undef DOPRI5_ACTION
#undef DOPRI5_STATE
#undef DOPRI5_BB
#undef DOPRI5_WINDOWS
#undef DOPRI5_WRITTEN_OUT
#undef DOPRI5_COLLECT
#undef DOPRI5_LIMIT
