// t1d_stepn_body.inc -- the body of stepn_kernel and stepn_gains_kernel (t1d_kernels.hpp), included between the braces of
// each: T, EXTRA, CTRL, a, c, nchunks, park_cap and mode are the kernel's.  One text, so that the two cannot drift apart;
// what differs goes through pid_words / pid_action / pid_integ, which are overloaded on the type of c.
    constexpr int STRIDE = 32;
    constexpr int NT = sn_threads<T>();
    T* const ldp = (T*)t1d_dyn_lds;                        // [DP_COUNT][STRIDE]
    T* const lpr = ldp + DP_COUNT * STRIDE;                // [prop_rows][STRIDE]
    T* const park_t = lpr + a.prop_rows * STRIDE;          // [kSnParkT][park_cap]
    int* const park_i = (int*)(park_t + kSnParkT * park_cap);      // [kSnParkI][park_cap]
    const int per_block = (nchunks + (int)gridDim.x - 1) / (int)gridDim.x;
    unsigned long long* const redo = (unsigned long long*)(park_i + kSnParkI * park_cap + ((kSnParkI * park_cap) & 1));   // [per_block]: envs to take again
    __shared__ int queue, taken, parked, passed, redo_any, redo_next;
    __shared__ T lconst[kLcSize + 2];                    // (two words more than the layout's, as since round 3: the other __shared__
                                                         // words of the kernel keep their addresses, and the kernel its machine code)
    s1_stage_tables<T, STRIDE>(a, ldp, lpr, lconst);
    const int first = (int)blockIdx.x * per_block;
    const int count = nchunks - first < per_block ? nchunks - first : per_block;
    const bool tiered = (mode & 1) != 0, all_redo = (mode & 2) != 0;
    const int group_min = mode >> 8;                        // records that go ahead of the next chunk (1..64)
    if (threadIdx.x == 0) {
        queue = 0; taken = 0; parked = 0; passed = all_redo ? count : 0; redo_any = 0; redo_next = 0;
        T hc[5];
        split_step_sizes<T>(a.n_sub, hc);
        for (int k = 0; k < 5; ++k) lconst[kLcHc1 + k] = hc[k];
        split_step_sizes<T>(2 * a.n_sub, hc);
        for (int k = 0; k < 5; ++k) lconst[kLcHc2 + k] = hc[k];
    }
    for (int j = threadIdx.x; j < park_cap; j += NT) park_i[4 * park_cap + j] = -1;
    for (int j = threadIdx.x; j < per_block; j += NT) {
        unsigned long long bits = 0ull;
        if (all_redo && j < count) {                        // every env of the chunk that exists
            const int64_t left = a.n - (int64_t)(first + j) * 64;
            bits = left >= 64 ? ~0ull : (left > 0 ? (1ull << left) - 1ull : 0ull);
        }
        redo[j] = bits;
    }
    if (threadIdx.x == 0 && all_redo) redo_any = 1;
    __syncthreads();
    const unsigned lane = threadIdx.x & 63u;
    const BRows<T> X(a.x, a.n, kPackedRows);                // rows 0-12 x, 13 planned, 14 last_qsto, 15 last_food, 16 last_cgm, 17 prev_risk, 18.. pts
    const BRows<int32_t> I(a.t, a.n, 3);                    // rows t, meta, next_meal
    const T inv_div = T(1) / T(a.minutes);
    const int st = a.sen.st;
    // ---- the pieces of an item
    // a chunk's loads, the controller (CTRL), the pump (env.py:51-52)
    auto load_lane = [&](SnLane<T>& L, unsigned i) {
        // what the pump and the first minute's bookkeeping need is requested first (loads return in order)
        const uint32_t meta = (uint32_t)(int32_t)at(I(1), i);
        L.t = at(I(0), i);
        L.next_meal = at(I(2), i);
        T basal = T(0), bolus = T(0);
        bool has_bolus = a.bolus != nullptr;
        PidWords<T> k_w{T(0), T(0), T(0), T(0)};
        T obs = T(0), k_integ = T(0), k_prev = T(0), bb_basal = T(0), bb_cr = T(1), bb_cf = T(1), prev_meal = T(0);
        if (CTRL) {
            obs = at(a.cgm, i);
            if (c.kind == 1) { bb_basal = at(c.bb_basal, i); bb_cr = at(c.bb_cr, i); bb_cf = at(c.bb_cf, i); prev_meal = at(c.bb_prev_meal, i); }
            else { k_integ = at(c.integ, i); k_prev = at(c.prev, i); k_w = pid_words(c, i); }
        } else {
            basal = at(a.basal, i);
            if (has_bolus) bolus = at(a.bolus, i);
        }
        L.planned = at(X(13), i); L.lq = at(X(14), i); L.lf = at(X(15), i);
#pragma unroll
        for (int k = 0; k < 13; ++k) L.x[k] = at(X(k), i);
        L.last_cgm = st == 1 ? T(0) : (T)at(X(16), i);       // with a 1-minute sensor the held value is never read
        L.i = i; L.m = 0; L.dirty = 0;
        L.pid = T1D_META_PID(meta);
        L.eating = (meta & T1D_META_EATING) != 0;
        L.cursor = (int)T1D_META_CURSOR(meta);
        if (CTRL) {
            const T stT = T(st);
            has_bolus = true;
            if (c.kind == 1) {                              // BBController._bb_policy (basal_bolus_ctrller.py:64-79)
                basal = bb_basal;
                if (prev_meal > T(0)) {
                    const T corr = obs > T(150) ? (obs - c.target) / bb_cf : T(0);
                    bolus = ((prev_meal * stT) / bb_cr + corr) / stT;
                }
            } else {                                        // PIDController.policy (pid_ctrller.py:17-36); its state moves on in the epilogue
                basal = pid_action(c, k_w, obs, k_integ, k_prev, stT);
            }
        }
        T q_basal, q_bolus;
        if (a.flags & T1D_BATCH_NO_PUMP) {
            q_basal = basal; q_bolus = has_bolus ? bolus : T(0);
        } else {
            pump_lconst(lconst, basal, bolus, has_bolus, q_basal, q_bolus);
        }
        L.insulin = q_basal + q_bolus;
        L.bg_sum = T(0); L.cgm_sum = T(0); L.meal_sum = T(0);
    };
    // scenario meal (env.py:50) -> meal bookkeeping (t1dpatient.py:82-107) -> the first gastric-emptying flux and the rule
    auto minute_head = [&](SnLane<T>& L, T& meal, TierPre<T>& tp) -> MinuteIn<T> {
        if (a.cho) {
            meal = at(rowv(a.cho, a.n, L.m), L.i);
            asm volatile("" : "+v"(meal));
        } else {
            meal = meal_lookup<T, true>(a, L.i, L);
        }
        ParsLdsS<T, STRIDE> pl{ldp, (int)L.pid};
        MinuteIn<T> u = eat_minute<1, T>(pl, L.x, meal, L.insulin, L.planned, L.lq, L.lf, L.eating);
        if (tiered) tp = tier_pre(pl, u, L.x);
        else { tp.f1 = kgut_flux(pl, u, L.x[0], L.x[1]); tp.level2 = false; }
        return u;
    };
    // the parameters of a chunk's minute loop, gathered into registers once per chunk: 16 model constants + the 4 gut weights
    // of level 1
    auto gather_pars = [&](ParsReg<T>& p, uint32_t pid) {
        ParsLdsS<T, STRIDE> pl{ldp, (int)pid};
#pragma unroll
        for (int k = 0; k < (int)(sizeof(kSplitPars) / sizeof(int)); ++k) p.v[kSplitPars[k]] = pl(kSplitPars[k]);
#pragma unroll
        for (int k = 0; k < 4; ++k) p.v[kSplitW(1) + k] = pl(kSplitW(1) + k);
    };
    // ... and for the records: the weights of both levels (a lone wave cannot hide the LDS latency of ~200 parameter reads
    // per minute behind anything: from LDS the pass over the records took three times as long)
    auto gather_pars2 = [&](ParsReg<T>& p, uint32_t pid) {
        gather_pars(p, pid);
        ParsLdsS<T, STRIDE> pl{ldp, (int)pid};
#pragma unroll
        for (int k = 0; k < 4; ++k) p.v[kSplitW(2) + k] = pl(kSplitW(2) + k);
    };
    // one minute of a chunk at level 1: step sizes from LDS
    auto integrate = [&](ParsReg<T>& p, SnLane<T>& L, const MinuteIn<T>& u, T f1) {
        PropLdsS<T, STRIDE> pr{lpr, (int)L.pid};
        p.pin_split();
        split_level<1, T, ParsReg<T>, decltype(pr), true, true>(p, pr, u, L.x, a.n_sub, f1, false, lconst + kLcHc1);
    };
    // clock, Gsub (t1dpatient.py:217-218), the CGM sample if one is due (cgm.py:26-36), the step's means (env.py:78-81)
    auto minute_tail = [&](SnLane<T>& L, T meal) {
        L.t += 1;
        ParsLdsS<T, STRIDE> pl{ldp, (int)L.pid};
        const T gsub = L.x[12] * pl(DP_IVG);
        int q, r;
        divmod_uniform(L.t, st, q, r);
        if (r == 0) {
            T cur[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) cur[k] = at(X(40 + k), L.i);
            bool entered = false;
            const T noise = noise_sample<false>(a, L.i, 1 + q, cur, &entered);
            if (entered) {
#pragma unroll
                for (int k = 0; k < 4; ++k) at(X(40 + k), L.i) = cur[k];
            }
            int z = 0;
            asm volatile("" : "+v"(z));
            const T vmin = lconst[kLcVmin + z], vmax = lconst[kLcVmax + z];
            T cv = gsub + noise;
            cv = cv > vmin ? cv : vmin;
            cv = cv < vmax ? cv : vmax;
            L.last_cgm = cv;
        }
        L.meal_sum += meal * inv_div; L.bg_sum += gsub * inv_div; L.cgm_sum += L.last_cgm * inv_div;
    };
    // the step's epilogue (env.py:85-117) and the state's way back
    auto epilogue = [&](SnLane<T>& L) {
        const unsigned i = L.i;
#pragma unroll
        for (int k = 0; k < 13; ++k) at(X(k), i) = L.x[k];
        if (L.dirty & 1) { at(X(13), i) = L.planned; at(X(14), i) = L.lq; at(X(15), i) = L.lf; at(X(kRowDbar), i) = dbar_of(L.lq, L.lf); }
        at(I(0), i) = L.t;
        if (L.dirty & 2) at(I(2), i) = L.next_meal;
        if (L.dirty & 5) at(I(1), i) = (int32_t)(L.pid | (L.eating ? T1D_META_EATING : 0u) | (L.planned > T(0) ? T1D_META_PLANNED : 0u) | ((uint32_t)L.cursor << 16));
        if (st != 1) at(X(16), i) = L.last_cgm;
        const T rp = at(X(17), i);                          // risk index of the previous step's CGM
        const T cgm_out = L.cgm_sum, bg_out = L.bg_sum;
        if (CTRL && c.kind == 0) {                          // pid_ctrller.py:30-33: the observation the policy acted on is still in place
            const T obs = at(a.cgm, i);
            at(c.integ, i) = pid_integ(c, i, (T)at(c.integ, i), obs, T(st));
            at(c.prev, i) = obs;
        }
        at(a.cgm, i) = cgm_out; at(a.bg, i) = bg_out;
        if (!(fabs((double)L.x[12]) <= 1.0e300)) atomicOr(a.status, T1D_ST_NONFINITE);
        T l, h, r = T(0), rc = T(0);
        risk_index1<1>(cgm_out, l, h, rc);
        at(a.reward, i) = rp - rc;                                                             // env.py:27-33
        at(X(17), i) = rc;
        at(a.done, i) = (bg_out < T(70) || bg_out > T(350)) ? 1 : 0;                           // env.py:103
        T ins_out = L.insulin;
        if (a.minutes != 1) {                               // the mean as env.py:79 accumulates it
            ins_out = T(0);
            for (int m = 0; m < a.minutes; ++m) ins_out += L.insulin * inv_div;
        }
        if (EXTRA) {
            const bool want_risk = a.lbgi || a.hbgi || a.risk || (CTRL && c.sum_risk);
            if (want_risk) risk_index1<1>(bg_out, l, h, r);                                    // env.py:85
            if (a.lbgi) at(a.lbgi, i) = l;
            if (a.hbgi) at(a.hbgi, i) = h;
            if (a.risk) at(a.risk, i) = r;
            if (a.meal) at(a.meal, i) = L.meal_sum;
            if (a.insulin) at(a.insulin, i) = ins_out;
        }
        if (CTRL) {
            if (c.kind == 1) at(c.bb_prev_meal, i) = L.meal_sum;
            if (c.bg_trace) c.bg_trace[c.trace_row * a.n + i] = bg_out;
            if (c.cgm_trace) c.cgm_trace[c.trace_row * a.n + i] = cgm_out;
            if (c.cho_trace) c.cho_trace[c.trace_row * a.n + i] = L.meal_sum;
            if (c.ins_trace) c.ins_trace[c.trace_row * a.n + i] = ins_out;
            if (c.sum_risk) at(c.sum_risk, i) = (T)at(c.sum_risk, i) + r;
            if (c.min_bg) { const T v = at(c.min_bg, i); at(c.min_bg, i) = bg_out < v ? bg_out : v; }
            if (c.max_bg) { const T v = at(c.max_bg, i); at(c.max_bg, i) = bg_out > v ? bg_out : v; }
            if (c.n_low) at(c.n_low, i) = (int)at(c.n_low, i) + (bg_out < T(70) ? 1 : 0);
            if (c.n_high) at(c.n_high, i) = (int)at(c.n_high, i) + (bg_out > T(180) ? 1 : 0);
        }
    };
    for (;;) {
        // ---- the next work item: a chunk while the queue lasts, else up to 64 records -- whatever is there: a wave with
        // nothing else to do takes a single record too (the record's minutes then run beside the last chunks, not behind
        // them) --, at the very end the words of the redo map
        int w_chunk = -1, w_lo = 0, w_n = 0, w_redo = -1;
        if (lane == 0) {
            // a full wave's worth of records goes ahead of the next chunk: worked off in full waves while the chunks last,
            // they leave only the stragglers for the end of the launch
            bool full = false;
            if (!all_redo) {
                int pk = __hip_atomic_load(&parked, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                pk = pk < park_cap ? pk : park_cap;
                int tk = __hip_atomic_load(&taken, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                const int av = pk - tk < 64 ? pk - tk : 64;
                if (av >= group_min && __hip_atomic_compare_exchange_strong(&taken, &tk, tk + av, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP)) {
                    w_lo = tk; w_n = av; full = true;
                }
            }
            const int cc = (all_redo || full) ? count : atomicAdd(&queue, 1);
            if (cc < count) w_chunk = cc;
            else if (!full) {
                for (int spins = 0;; ++spins) {
                    // `passed` first: once every chunk is past its last decision the record count is final
                    const int ps = __hip_atomic_load(&passed, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
                    int pk = __hip_atomic_load(&parked, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                    pk = pk < park_cap ? pk : park_cap;
                    int tk = __hip_atomic_load(&taken, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                    const int avail = pk - tk;
                    if (avail > 0) {
                        const int n = avail < 64 ? avail : 64;
                        if (__hip_atomic_compare_exchange_strong(&taken, &tk, tk + n, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP)) {
                            w_lo = tk; w_n = n;
                            break;
                        }
                        continue;
                    }
                    if (ps >= count) {
                        // no record left and no chunk that could still leave one: what remains is the redo map, final now
                        if (__hip_atomic_load(&redo_any, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP)) {
                            const int rw = atomicAdd(&redo_next, 1);
                            if (rw < count) w_redo = rw;
                        }
                        break;
                    }
                    if (spins > kSnSpinLimit) { atomicOr(a.status, T1D_ST_STALL); break; }
                    __builtin_amdgcn_s_sleep(16);
                }
            }
        }
        w_chunk = __builtin_amdgcn_readfirstlane(w_chunk);
        w_lo = __builtin_amdgcn_readfirstlane(w_lo);
        w_n = __builtin_amdgcn_readfirstlane(w_n);
        w_redo = __builtin_amdgcn_readfirstlane(w_redo);
        if (w_chunk < 0 && w_n == 0 && w_redo < 0) break;   // wave-uniform
#if T1D_S1_PHASE_PRIO
        __builtin_amdgcn_s_setprio(T1D_S1_PHASE_PRIO);
#endif
        if (w_chunk < 0) {
            // ---- records: each lane from the minute it was parked in (which the rule, on the same state, puts at level 2
            // again); a word of the redo map: the envs of a chunk that found no record free, from their loads.  Every lane
            // at its own level, in place.
            // (Every lane reads -- the idle ones a record or env of a neighbour, and do nothing with it: a load under a
            // divergent branch writes only the active lanes of its registers, which makes the compiler keep the previous
            // item's values alive in the others across the whole item loop: 27 register pairs spilled and reloaded per item.)
            SnLane<T> L;
            bool active;
            if (w_n > 0) {
                sn_wait_records(park_i, park_cap, w_lo, w_n, lane, a.status);
                active = (int)lane < w_n;
                sn_unpark(L, park_t, park_i, park_cap, w_lo + (active ? (int)lane : 0));
            } else {
                const unsigned i = (unsigned)(first + w_redo) * 64u + lane;
                __builtin_assume(i < (1u << 28));
                active = ((redo[w_redo] >> lane) & 1ull) != 0ull;
                load_lane(L, (int64_t)i < a.n ? i : (unsigned)(a.n - 1));
            }
            // (fp64; the fp32 instantiation has no registers to spare at four waves per SIMD and keeps reading LDS)
            constexpr bool kRecReg = sizeof(T) == 8;
            ParsReg<T> p;
            if constexpr (kRecReg) gather_pars2(p, L.pid);
            for (;;) {
                const bool on = active && L.m < a.minutes;
                if (__builtin_amdgcn_ballot_w64(on) == 0ull) break;             // wave-uniform
                if (on) {
                    T meal = T(0);
                    TierPre<T> tp{T(0), false};
                    const T planned0 = L.planned, lq0 = L.lq, lf0 = L.lf;
                    const int nm0 = L.next_meal, cur0 = L.cursor;
                    const bool eat0 = L.eating;
                    const MinuteIn<T> u = minute_head(L, meal, tp);
                    L.dirty |= ((L.planned != planned0 || L.lq != lq0 || L.lf != lf0) ? 1 : 0) | (L.next_meal != nm0 ? 2 : 0) |
                               ((L.cursor != cur0 || L.eating != eat0) ? 4 : 0);
                    PropLdsS<T, STRIDE> pr{lpr, (int)L.pid};
                    if constexpr (kRecReg) {
                        p.pin_split();
                        split_level<0, T, ParsReg<T>, decltype(pr), true, true>(p, pr, u, L.x, a.n_sub, tp.f1, tp.level2, lconst + kLcHc1);
                    } else {
                        ParsLdsS<T, STRIDE> pl{ldp, (int)L.pid};
                        split_level<0, T, ParsLdsS<T, STRIDE>, decltype(pr), true>(pl, pr, u, L.x, a.n_sub, tp.f1, tp.level2);
                    }
                    minute_tail(L, meal);
                    L.m += 1;
                }
            }
            if (active) { epilogue(L); }
            continue;
        }
        // ---- a chunk
        const unsigned i0 = (unsigned)(first + ((a.flags & kFlagReverse) ? count - 1 - w_chunk : w_chunk)) * 64u + lane;   // (kFlagReverse: above)
        __builtin_assume(i0 < (1u << 28));
        bool left = (int64_t)i0 >= a.n;                     // lanes beyond the batch have nothing to finish
        SnLane<T> L;
        {
            load_lane(L, left ? (unsigned)(a.n - 1) : i0);  // (every lane loads: see above)
            ParsReg<T> p;
            gather_pars(p, L.pid);
            while (!left && L.m < a.minutes) {
                T meal = T(0);
                TierPre<T> tp{T(0), false};
                // the lane as it stands at the start of the minute: what a record holds
                const T planned0 = L.planned, lq0 = L.lq, lf0 = L.lf;
                const int nm0 = L.next_meal, cur0 = L.cursor;
                const bool eat0 = L.eating;
                const MinuteIn<T> u = minute_head(L, meal, tp);
                if (tp.level2) {
                    // level 2: leave a record (or, no record free, a bit in the redo map) and be done with this item
                    L.planned = planned0; L.lq = lq0; L.lf = lf0; L.next_meal = nm0; L.cursor = cur0; L.eating = eat0;
                    const int slot = atomicAdd(&parked, 1);
                   
                    if (slot < park_cap) sn_park(L, park_t, park_i, park_cap, slot);
                    else {
                       
                        const unsigned rel = L.i - (unsigned)first * 64u;
                        atomicOr(&redo[rel >> 6], 1ull << (rel & 63u));
                        redo_any = 1;
                    }
                    left = true;
                    break;
                }
                L.dirty |= ((L.planned != planned0 || L.lq != lq0 || L.lf != lf0) ? 1 : 0) | (L.next_meal != nm0 ? 2 : 0) |
                           ((L.cursor != cur0 || L.eating != eat0) ? 4 : 0);
#if T1D_S1_PHASE_PRIO
                __builtin_amdgcn_s_setprio(0);              // the integration fills the issue slots the other phases leave
#endif
                integrate(p, L, u, tp.f1);
#if T1D_S1_PHASE_PRIO
                __builtin_amdgcn_s_setprio(T1D_S1_PHASE_PRIO);
#endif
                minute_tail(L, meal);
                L.m += 1;
            }
        }
        // past this chunk's last decision: it can leave no more records.  (Lane 0 of a chunk is always a live env.  The
        // count goes up BEFORE the epilogue, not as the loop body's last statement: a one-lane atomic right in front of
        // the back edge came out of hipcc 7.2 with the other 63 lanes dropped from the next trip.)
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        if (lane == 0) atomicAdd(&passed, 1);
        if (!left) { epilogue(L); }
    }
    __builtin_amdgcn_s_waitcnt(0x0070);
