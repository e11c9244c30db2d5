// The kernel plan of t1d_step and of the roll-outs (plan_call in t1d_abi.hip) for hand-made contexts and batches, checked
// against a table of expected rows: template instance, refill ahead, grid, block, dynamic LDS and the record capacity of
// stepn_kernel.  Behind them the launch shapes of the kernels that run the policy (shape_mlp after plan_call, shape_mlp_dopri5,
// shape_mlp_alone) and the LDS of one wave of mlp_grad_kernel (grad_wave_lds), against this file's own arithmetic.  No HIP
// call: the batch pointers are computed addresses that are never dereferenced.  Built and run by test_dispatch_plan.py;
// prints one line per row and exits non-zero on any mismatch.
#include "../simglucose_amd/csrc/t1d_abi.hip"

#include <cstdint>

static const int kLds160 = 160 * 1024;    // hipDeviceAttributeMaxSharedMemoryPerBlock on gfx950

// a batch of n envs; packed: the state rows of one [45][n] buffer and t, meta, next_meal of one [3][n] buffer
static t1d_batch make_batch(int dtype, int64_t n, bool packed)
{
    t1d_batch b;
    std::memset(&b, 0, sizeof(b));
    b.n = n; b.dtype = dtype;
    const size_t rowb = (size_t)n * (dtype == T1D_F64 ? 8 : 4);
    char* x = (char*)(uintptr_t)0x100000000ull;
    char* t = x + (kPackedRows + 1) * rowb;
    char* io = t + 4 * (size_t)n * 4;
    b.x = x; b.planned = x + 13 * rowb; b.last_qsto = x + 14 * rowb; b.last_food = x + 15 * rowb; b.last_cgm = x + 16 * rowb;
    b.prev_risk = x + 17 * rowb; b.pts = x + 18 * rowb; b.dbar = x + kRowDbar * rowb;
    b.t = (int32_t*)t; b.meta = (uint32_t*)(t + n * 4); b.next_meal = (int32_t*)(t + n * 8);
    if (!packed) b.dbar = x + (kRowDbar + 1) * rowb;
    b.ar_e = io; b.basal = io + rowb; b.cgm = io + 2 * rowb; b.bg = io + 3 * rowb; b.reward = io + 4 * rowb; b.done = (uint8_t*)(io + 5 * rowb);
    return b;
}

struct Call {
    int dtype = T1D_F64, np = 30, sample_time = 1, minutes = 1, n_sub = 4;
    int64_t n = 65536;
    bool packed = true, extra = false, rollout = false;
    int flags = 0, lds_per_block = kLds160;
    std::vector<std::pair<const char*, int64_t>> opts;
};

// today's formulas: the persistent kernels' tables in LDS; per_block = chunks of 64 envs per workgroup
static size_t esz_of(const Call& k) { return k.dtype == T1D_F64 ? 8 : 4; }
static size_t tables(const Call& k, int stride) { return (size_t)(DP_COUNT + kPropRows(k.n_sub)) * stride * esz_of(k); }
static int per_block(const Call& k, int blocks) { const int ch = (int)((k.n + 63) / 64); return (ch + blocks - 1) / blocks; }
static size_t lds_step1d(const Call& k) { return tables(k, 32) + (size_t)kS1DPark * (18 * esz_of(k) + 12) + (size_t)per_block(k, 256) * 64 * 2; }
static size_t lds_generic(const Call& k) { return (size_t)kPropRows(k.n_sub) * ((k.np + 1) & ~1) * esz_of(k); }
static unsigned grid_generic(const Call& k) { return (unsigned)((k.n + 255) / 256); }
// stepn_kernel: the redo map and as many records (21 T + 5 int each, a multiple of 64) as fit, at most the env-minutes
static int stepn_cap(const Call& k)
{
    const size_t rec = 21 * esz_of(k) + 20, map = (size_t)per_block(k, 256) * 8 + 8;
    long long cap = (long long)((kLds160 - 1024 - tables(k, 32) - map) / rec) / 64 * 64;
    cap = std::min(cap, ((long long)per_block(k, 256) * 64 * k.minutes + 63) / 64 * 64);
    return (int)cap;
}
static size_t lds_stepn(const Call& k, int cap) { return tables(k, 32) + (size_t)cap * (21 * esz_of(k) + 20) + (size_t)per_block(k, 256) * 8 + 8; }

static std::string describe(const Plan& p)
{
    const char* T = p.f64 ? "double" : "float";
    const char* tf[2] = {"false", "true"};
    char s[256];
    switch (p.kernel) {
    case Kern::step: snprintf(s, sizeof(s), "step_kernel<%d, %s, %s>", p.variant, T, tf[p.refill]); break;
    case Kern::rollout: snprintf(s, sizeof(s), "rollout_pid_kernel<%d, %s>", p.variant, T); break;
    case Kern::step1: snprintf(s, sizeof(s), "step1_kernel<%s, %d, %s, %s>", T, p.stride, tf[p.extra], tf[p.tiered]); break;
    case Kern::step1d: snprintf(s, sizeof(s), "step1d_kernel<%s, %s>", T, tf[p.extra]); break;
    case Kern::stepn: snprintf(s, sizeof(s), "stepn_kernel<%s, %s, %s> cap %d", T, tf[p.extra], tf[p.ctrl], p.cap); break;
    }
    char r[400];
    snprintf(r, sizeof(r), "%s%s grid %u block %u lds %zu", s, p.refill_ahead ? " after refill" : "", p.grid, p.block, p.lds);
    return r;
}

// the expected row in describe's words; block: the kernel family's workgroup
static std::string expect(const Call& k, const std::string& kernel, bool refill, unsigned grid, size_t lds)
{
    const bool f64 = k.dtype == T1D_F64;
    unsigned block = kBlock;
    if (kernel.rfind("step1_", 0) == 0) block = f64 ? s1_threads<double>() : s1_threads<float>();
    if (kernel.rfind("step1d_", 0) == 0) block = f64 ? s1d_threads<double>() : s1d_threads<float>();
    if (kernel.rfind("stepn_", 0) == 0) block = f64 ? sn_threads<double>() : sn_threads<float>();
    char r[400];
    snprintf(r, sizeof(r), "%s%s grid %u block %u lds %zu", kernel.c_str(), refill ? " after refill" : "", grid, block, lds);
    return r;
}

static int g_failed = 0, g_rows = 0;

static void report(const char* name, const std::string& got, const std::string& want)
{
    const bool ok = got == want;
    printf("%s %-56s %s\n", ok ? "ok  " : "FAIL", name, got.c_str());
    if (!ok) { printf("     %-56s %s\n", "expected", want.c_str()); ++g_failed; }
    ++g_rows;
}

static void make_ctx(const Call& k, t1d_ctx& c)
{
    c.np = k.np; c.np_pad = (k.np + 1) & ~1; c.n_cu = 256; c.lds_per_block = k.lds_per_block;
    std::memset(c.sensor, 0, sizeof(c.sensor));
    c.sensor[5] = k.sample_time;
    for (auto& o : k.opts)
        if (t1d_ctx_set_option(&c, o.first, o.second)) { printf("bad option %s\n", o.first); ++g_failed; }
}

static void row(const char* name, const Call& k, const std::string& want, bool show_tables = false)
{
    t1d_ctx c;
    make_ctx(k, c);
    t1d_batch b = make_batch(k.dtype, k.n, k.packed);
    b.flags = k.flags;
    if (k.extra) b.lbgi = (char*)b.x + 100;
    Plan p;
    const int rc = plan_call(k.rollout ? "t1d_rollout_pid" : "t1d_step", &c, &b, k.minutes, k.n_sub, k.rollout, &p);
    std::string got = rc ? "error " + std::to_string(rc) + " " + t1d_last_error() : describe(p);
    if (show_tables) got += p.tables ? " tables" : " no tables";
    report(name, got, want);
}

// ---- the kernels that run the policy ----------------------------------------------------------------------------------
// the two policies of the rows: H = 4 with widths (16, 16, 1) and H = 12 with widths (32, 32, 32, 1)
struct Net { const char* name; int history, n_layers, width[4]; };
static const Net kNets[2] = {{"H 4 (16, 16, 1)", 4, 3, {16, 16, 1, 0}}, {"H 12 (32, 32, 32, 1)", 12, 4, {32, 32, 32, 1}}};

// the rows of a wave's column block: 2 H for the windows, then the wider of the features and the widest hidden layer
static int cols_of(const Net& p)
{
    int widest = 2 * p.history + 3;
    for (int l = 0; l + 1 < p.n_layers; ++l) widest = std::max(widest, p.width[l]);
    return 2 * p.history + widest;
}

// the t1d_mlp of p for one policy of n envs, as check_mlp takes it; the pointers are never dereferenced
static t1d_mlp make_net(const Net& p, int64_t n)
{
    t1d_mlp m;
    std::memset(&m, 0, sizeof(m));
    m.history = p.history; m.n_layers = p.n_layers;
    int in_w = 2 * p.history + 3;
    for (int l = 0; l < p.n_layers; ++l) { m.width[l] = p.width[l]; m.n_params += p.width[l] * (in_w + 1); in_w = p.width[l]; }
    m.hidden_act = T1D_MLP_TANH; m.out_act = T1D_MLP_LOGISTIC;
    m.n_policies = 1; m.envs_per_policy = n;
    m.params = m.cgm_hist = m.ins_hist = m.prev_meal = (void*)(uintptr_t)0x100000000ull;
    return m;
}

// The expected shape: the most waves of 4, 2 and 1 whose pieces fit under the ceiling beside the fixed bytes and the front
// bytes (rounded up to 16), or the refusal.  seen[]: which outcomes a family has shown -- 4, 2, 1 waves, refused.
static std::string want_shape(int64_t n, size_t fixed, size_t front, size_t per_wave, size_t ceiling, const std::string& refusal, bool seen[4])
{
    const size_t off = (front + 15) / 16 * 16;
    for (int k = 0; k < 3; ++k) {
        const int waves = 4 >> k;
        if (fixed + off + per_wave * waves > ceiling) continue;
        seen[k] = true;
        char r[200];
        snprintf(r, sizeof(r), "threads %d grid %lld lds %zu off %zu", 64 * waves, (long long)((n + 64 * waves - 1) / (64 * waves)), off + per_wave * waves, off);
        return r;
    }
    seen[3] = true;
    return "error " + std::to_string(T1D_E_INVALID) + " " + refusal;
}

static std::string shape_text(unsigned threads, unsigned grid, size_t lds, size_t off)
{
    char r[200];
    snprintf(r, sizeof(r), "threads %u grid %u lds %zu off %zu", threads, grid, lds, off);
    return r;
}

static void all_seen(const char* family, const bool seen[4], int n_outcomes)
{
    static const char* what[4] = {"four waves", "two waves", "one wave", "the refusal"};
    for (int k = 0; k < n_outcomes; ++k) report((std::string(family) + " shows " + what[k]).c_str(), seen[k] ? "yes" : "no", "yes");
}

// t1d_rollout_mlp, t1d_collect_mlp: plan_call for a roll-out in one launch, then shape_mlp.  variant: what the plan must
// choose; the static parameter table goes with variants 0 and 7, the propagator table in front with the split variants
template <typename T>
static void mlp_row(const char* name, const Call& k, const Net& net, int variant, bool seen[4])
{
    t1d_ctx c;
    make_ctx(k, c);
    t1d_batch b = make_batch(k.dtype, k.n, false);
    const t1d_mlp m = make_net(net, k.n);
    int cols = 0;
    Plan p;
    MlpArgs<T> ma = make_mlp<T>(&m, 1);
    int rc = check_mlp("t1d_rollout_mlp", &b, &m, &cols);
    if (!rc && cols != cols_of(net)) { report(name, "cols " + std::to_string(cols), "cols " + std::to_string(cols_of(net))); return; }
    if (!rc) rc = plan_call("t1d_rollout_mlp", &c, &b, k.minutes, k.n_sub, true, &p, true);
    if (!rc) rc = shape_mlp<T>("t1d_rollout_mlp", &c, &b, cols, p, ma);
    const std::string got = "variant " + std::to_string(p.variant) + " " +
        (rc ? "error " + std::to_string(rc) + " " + t1d_last_error() : shape_text(p.block, p.grid, p.lds, (size_t)ma.lds_off));
    const size_t fixed = (variant == 0 || variant == 7 ? (size_t)DP_COUNT * 64 * sizeof(T) : 0) + 256;
    const size_t front = variant == 0 || variant == 3 ? 0 : lds_generic(k);
    report(name, got, "variant " + std::to_string(variant) + " " +
           want_shape(k.n, fixed, front, (size_t)cols_of(net) * 64 * sizeof(T), (size_t)k.lds_per_block,
                      "t1d_rollout_mlp: the integrator's tables leave no room in LDS for one wave of this policy", seen));
}

static void policy_rows()
{
    bool seen_mlp[4] = {}, seen_exact[4] = {}, seen_alone[4] = {};
    for (int dt : {T1D_F64, T1D_F32})
        for (const Net& net : kNets)
            for (int big = 0; big < 2; ++big)
                for (int lds : {kLds160, 65536})
                    for (int opt = 0; opt < 3; ++opt)
                        for (int64_t n : {(int64_t)192, (int64_t)65536}) {
                            if (opt && n != 192) continue;
                            const bool f64 = dt == T1D_F64;
                            Call k; k.dtype = dt; k.n = n; k.sample_time = 3; k.minutes = 3; k.lds_per_block = lds;
                            k.np = big ? 64 : 30; k.n_sub = big ? 8 : 4;
                            if (opt == 1) k.opts = {{"math", 0}};
                            if (opt == 2) k.opts = {{"integrator", 0}};
                            // 64 patients x n_sub 8 beside the parameter table in 64 KiB: the plan falls back to RK4
                            const bool rk4 = opt == 2 || (big && lds == 65536);
                            const int variant = opt == 1 ? 0 : rk4 ? 3 : f64 ? 7 : 6;
                            const std::string name = std::string(f64 ? "fp64 " : "fp32 ") + "mlp " + net.name + ", " + std::to_string(k.np) + " x " +
                                std::to_string(k.n_sub) + ", " + std::to_string(lds / 1024) + " KiB" + (opt == 1 ? ", math 0" : opt == 2 ? ", integrator 0" : "") +
                                ", n " + std::to_string(n);
                            if (f64) mlp_row<double>(name.c_str(), k, net, variant, seen_mlp); else mlp_row<float>(name.c_str(), k, net, variant, seen_mlp);
                        }
    all_seen("t1d_rollout_mlp", seen_mlp, 4);

    // the exact mode: the raw patient rows (32 columns of 64 doubles) and 256 bytes fixed; per wave RollCold's 13 doubles and
    // 3 ints per lane and the columns.  32 KiB is no gfx950's: the row of the refusal
    for (const Net& net : kNets)
        for (int lds : {kLds160, 65536, 32768}) {
            t1d_ctx c;
            c.lds_per_block = lds;
            Shape sh;
            const int64_t n = 65536 + 64;
            const int rc = shape_mlp_dopri5("t1d_rollout_mlp_dopri5", &c, n, cols_of(net), &sh);
            const std::string name = std::string("exact mode mlp ") + net.name + ", " + std::to_string(lds / 1024) + " KiB";
            report(name.c_str(), rc ? "error " + std::to_string(rc) + " " + t1d_last_error() : shape_text(sh.threads, sh.grid, sh.lds, sh.front),
                   want_shape(n, (size_t)32 * 64 * 8 + 256, 0, (size_t)(13 * 8 + 3 * 4) * 64 + (size_t)cols_of(net) * 64 * 8, (size_t)lds,
                              "t1d_rollout_mlp_dopri5: the patient rows leave no room in LDS for one wave of this policy", seen_exact));
        }
    all_seen("t1d_rollout_mlp_dopri5", seen_exact, 4);

    // the policy alone: nothing fixed, the ceiling 64 KiB less 256 bytes whatever the device has; never refused
    for (int dt : {T1D_F64, T1D_F32})
        for (const Net& net : kNets) {
            const bool f64 = dt == T1D_F64;
            t1d_ctx c;
            c.lds_per_block = kLds160;
            const int64_t n = 192;
            const Shape sh = f64 ? shape_mlp_alone<double>(&c, n, cols_of(net)) : shape_mlp_alone<float>(&c, n, cols_of(net));
            const std::string name = std::string(f64 ? "fp64 " : "fp32 ") + "t1d_mlp_action " + net.name;
            report(name.c_str(), shape_text(sh.threads, sh.grid, sh.lds, sh.front),
                   want_shape(n, 0, 0, (size_t)cols_of(net) * 64 * (f64 ? 8 : 4), 65280, "never", seen_alone));
        }
    all_seen("t1d_mlp_action", seen_alone, 2);

    // one wave of mlp_grad_kernel: the features and every hidden unit's activation; with grad a row of ones and a delta
    // per unit of every layer
    for (int dt : {T1D_F64, T1D_F32})
        for (const Net& net : kNets)
            for (bool grad : {false, true}) {
                const size_t word = dt == T1D_F64 ? 8 : 4;
                int act = 2 * net.history + 3, units = 0;
                for (int l = 0; l < net.n_layers; ++l) { units += net.width[l]; if (l + 1 < net.n_layers) act += net.width[l]; }
                const size_t want = (size_t)(grad ? act + 1 + units : act) * 64 * word;
                const t1d_mlp m = make_net(net, 64);
                int act_rows = 0;
                const size_t lds = grad_wave_lds(&m, grad, word, &act_rows);
                const std::string name = std::string(word == 8 ? "fp64 " : "fp32 ") + "mlp_grad_kernel " + net.name + (grad ? ", grad" : ", forward");
                report(name.c_str(), "act_rows " + std::to_string(act_rows) + " lds " + std::to_string(lds) + (lds > 65536 ? " above 64 KiB" : ""),
                       "act_rows " + std::to_string(act) + " lds " + std::to_string(want) + (want > 65536 ? " above 64 KiB" : ""));
            }
}

int main()
{
    const int F64 = T1D_F64, F32 = T1D_F32;
    for (int dt : {F64, F32}) {
        const bool f64 = dt == F64;
        const std::string T = f64 ? "double" : "float", V = f64 ? "7" : "6";
        auto tag = [&](const char* s) { static std::string n; n = (f64 ? "fp64 " : "fp32 ") + std::string(s); return n.c_str(); };
        Call k; k.dtype = dt;

        // one minute, packed, 30 patients: the set-aside form, then the in-place forms and stride 64
        row(tag("1 min"), k, expect(k, "step1d_kernel<" + T + ", false>", true, 256, lds_step1d(k)));
        { Call e = k; e.extra = true; row(tag("1 min, extra outputs"), e, expect(e, "step1d_kernel<" + T + ", true>", true, 256, lds_step1d(e))); }
        { Call e = k; e.flags = T1D_BATCH_NO_REFILL_DUE; row(tag("1 min, no refill due"), e, expect(e, "step1d_kernel<" + T + ", false>", false, 256, lds_step1d(e))); }
        { Call e = k; e.opts = {{"adaptive_gut", 0}}; row(tag("1 min, adaptive_gut 0"), e, expect(e, "step1_kernel<" + T + ", 32, false, false>", true, 256, tables(e, 32))); }
        { Call e = k; e.opts = {{"adaptive_gut", 2}}; e.extra = true; row(tag("1 min, adaptive_gut 2, extra"), e, expect(e, "step1_kernel<" + T + ", 32, true, true>", true, 256, tables(e, 32))); }
        { Call e = k; e.np = 40; row(tag("1 min, 40 patients"), e, expect(e, "step1_kernel<" + T + ", 64, false, true>", true, 256, tables(e, 64))); }
        { Call e = k; e.n = 1 << 20; e.opts = {{"s1_blocks", 8}}; row(tag("1 min, 1 Mi envs on 8 blocks"), e, expect(e, "step1_kernel<" + T + ", 32, false, true>", true, 8, tables(e, 32))); }
        { Call e = k; e.opts = {{"adaptive_gut", 3}, {"defer_min_chunks", 5}}; row(tag("1 min, adaptive_gut 3"), e, expect(e, "step1d_kernel<" + T + ", false>", true, 256, lds_step1d(e))); }
        { Call e = k; e.opts = {{"defer_min_chunks", 5}}; row(tag("1 min, defer_min_chunks above the share"), e, expect(e, "step1_kernel<" + T + ", 32, false, true>", true, 256, tables(e, 32))); }
        { Call e = k; e.opts = {{"single_minute_kernel", 0}}; row(tag("1 min, single_minute_kernel 0"), e, expect(e, "step_kernel<" + V + ", " + T + ", false>", true, grid_generic(e), lds_generic(e))); }

        // the generic kernel
        { Call e = k; e.packed = false; row(tag("unpacked"), e, expect(e, "step_kernel<" + V + ", " + T + ", false>", true, grid_generic(e), lds_generic(e))); }
        { Call e = k; e.opts = {{"integrator", 0}}; row(tag("integrator 0"), e, expect(e, "step_kernel<3, " + T + ", false>", true, grid_generic(e), 0)); }
        { Call e = k; e.n_sub = 3; row(tag("n_sub 3"), e, expect(e, "step_kernel<3, " + T + ", false>", true, grid_generic(e), 0)); }
        { Call e = k; e.opts = {{"math", 0}}; row(tag("math 0"), e, expect(e, "step_kernel<0, " + T + ", true>", false, grid_generic(e), 0)); }
        { Call e = k; e.opts = {{"split_refill", 0}}; row(tag("split_refill 0"), e, expect(e, "step_kernel<" + V + ", " + T + ", true>", false, grid_generic(e), lds_generic(e))); }
        { Call e = k; e.opts = {{"adaptive_gut", 0}}; e.packed = false; row(tag("unpacked, adaptive_gut 0"), e, expect(e, "step_kernel<4, " + T + ", false>", true, grid_generic(e), lds_generic(e))); }
        { Call e = k; e.minutes = 3; row(tag("3 min, 1-min sensor"), e, expect(e, "step_kernel<" + V + ", " + T + ", true>", false, grid_generic(e), lds_generic(e))); }

        // Dexcom steps (3 minutes): the multi-minute kernel from its threshold up
        Call d = k; d.sample_time = 3; d.minutes = 3;
        const int64_t thr = f64 ? 262144 : 393216;
        { Call e = d; e.n = thr - 1; row(tag("Dexcom below the threshold"), e, expect(e, "step_kernel<" + V + ", " + T + ", false>", true, grid_generic(e), lds_generic(e))); }
        { Call e = d; e.n = thr; const int cap = stepn_cap(e);
          row(tag("Dexcom at the threshold"), e, expect(e, "stepn_kernel<" + T + ", false, false> cap " + std::to_string(cap), true, 256, lds_stepn(e, cap))); }
        { Call e = d; e.n = 1 << 20; e.extra = true; e.flags = T1D_BATCH_NO_REFILL_DUE; const int cap = stepn_cap(e);
          row(tag("Dexcom 1 Mi, extra, no refill due"), e, expect(e, "stepn_kernel<" + T + ", true, false> cap " + std::to_string(cap), false, 256, lds_stepn(e, cap))); }
        { Call e = d; e.n = 1 << 20; e.opts = {{"park_cap", 100}};
          row(tag("Dexcom 1 Mi, park_cap 100"), e, expect(e, "stepn_kernel<" + T + ", false, false> cap 128", true, 256, lds_stepn(e, 128))); }
        { Call e = d; e.n = 1 << 20; e.opts = {{"multi_minute_kernel", 0}}; row(tag("Dexcom 1 Mi, multi_minute_kernel 0"), e, expect(e, "step_kernel<" + V + ", " + T + ", false>", true, grid_generic(e), lds_generic(e))); }
        { Call e = d; e.n = 4096; e.opts = {{"multi_minute_kernel", 2}}; const int cap = stepn_cap(e);
          row(tag("Dexcom 4 Ki, multi_minute_kernel 2"), e, expect(e, "stepn_kernel<" + T + ", false, false> cap " + std::to_string(cap), true, 64, lds_stepn(e, cap))); }
        { Call e = d; e.n = 1 << 20; e.np = 40; row(tag("Dexcom 1 Mi, 40 patients"), e, expect(e, "step_kernel<" + V + ", " + T + ", false>", true, grid_generic(e), lds_generic(e))); }

        // roll-outs: one stepn_kernel launch per step from the threshold up, else all steps in one rollout_pid_kernel
        Call r = d; r.rollout = true;
        const int64_t rthr = f64 ? 524288 : 786432;
        { Call e = r; e.n = rthr - 1; row(tag("roll-out below the threshold"), e, expect(e, "rollout_pid_kernel<" + V + ", " + T + ">", false, grid_generic(e), lds_generic(e))); }
        { Call e = r; e.n = rthr; const int cap = stepn_cap(e);
          row(tag("roll-out at the threshold"), e, expect(e, "stepn_kernel<" + T + ", true, true> cap " + std::to_string(cap), true, 256, lds_stepn(e, cap))); }
        { Call e = r; e.n = 1 << 20; e.sample_time = 1; e.minutes = 1; e.flags = T1D_BATCH_NO_REFILL_DUE; const int cap = stepn_cap(e);
          row(tag("roll-out 1 Mi, 1 min, no refill due"), e, expect(e, "stepn_kernel<" + T + ", true, true> cap " + std::to_string(cap), true, 256, lds_stepn(e, cap))); }
        { Call e = r; e.n = 1 << 20; e.opts = {{"rollout_launches", 0}}; row(tag("roll-out 1 Mi, rollout_launches 0"), e, expect(e, "rollout_pid_kernel<" + V + ", " + T + ">", false, grid_generic(e), lds_generic(e))); }
        { Call e = r; e.n = 4096; e.opts = {{"rollout_launches", 2}}; const int cap = stepn_cap(e);
          row(tag("roll-out 4 Ki, rollout_launches 2"), e, expect(e, "stepn_kernel<" + T + ", true, true> cap " + std::to_string(cap), true, 64, lds_stepn(e, cap))); }
        { Call e = r; e.n = 1 << 20; e.opts = {{"multi_minute_kernel", 0}}; row(tag("roll-out 1 Mi, multi_minute_kernel 0"), e, expect(e, "rollout_pid_kernel<" + V + ", " + T + ">", false, grid_generic(e), lds_generic(e))); }
        { Call e = r; e.n = 1 << 20; e.opts = {{"math", 0}}; row(tag("roll-out 1 Mi, math 0"), e, expect(e, "rollout_pid_kernel<0, " + T + ">", false, grid_generic(e), 0)); }

        // 64 patients x n_sub 8 in 64 KiB of LDS: the generic kernel cannot hold the split tables.  RK4 with integrator = -1,
        // an error with integrator = 1; the tables are built either way
        for (bool ro : {false, true}) {
            Call e = k; e.np = 64; e.n_sub = 8; e.packed = false; e.rollout = ro; e.lds_per_block = 65536;
            row(tag(ro ? "roll-out, 64 KiB LDS, integrator -1" : "64 KiB LDS, integrator -1"), e,
                expect(e, ro ? "rollout_pid_kernel<3, " + T + ">" : "step_kernel<3, " + T + ", false>", !ro, grid_generic(e), 0) + " tables", true);
            e.opts = {{"integrator", 1}};
            row(tag(ro ? "roll-out, 64 KiB LDS, integrator 1" : "64 KiB LDS, integrator 1"), e,
                "error " + std::to_string(T1D_E_INVALID) + (ro ? " t1d_rollout_pid: split tables exceed the LDS of a workgroup; use integrator 0 or -1"
                                                                : " t1d_step: split tables exceed the LDS of a workgroup (n_patients x n_sub too large); use integrator 0 or -1") + " tables", true);
        }
    }
    policy_rows();
    printf("%d rows, %d failed\n", g_rows, g_failed);
    return g_failed ? 1 : 0;
}
