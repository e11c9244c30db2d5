// The kernel plan of t1d_step and of the roll-outs (plan_call in t1d_abi.hip) for hand-made contexts and batches, checked
// against a table of expected rows: template instance, refill ahead, grid, block, dynamic LDS and the record capacity of
// stepn_kernel.  No HIP call: the batch pointers are computed addresses that are never dereferenced.  Built and run by
// test_dispatch_plan.py; prints one line per row and exits non-zero on any mismatch.
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

static void row(const char* name, const Call& k, const std::string& want, bool show_tables = false)
{
    t1d_ctx c;
    c.np = k.np; c.np_pad = (k.np + 1) & ~1; c.n_cu = 256; c.lds_per_block = k.lds_per_block;
    std::memset(c.sensor, 0, sizeof(c.sensor));
    c.sensor[5] = k.sample_time;
    for (auto& o : k.opts)
        if (t1d_ctx_set_option(&c, o.first, o.second)) { printf("bad option %s\n", o.first); ++g_failed; }
    t1d_batch b = make_batch(k.dtype, k.n, k.packed);
    b.flags = k.flags;
    if (k.extra) b.lbgi = (char*)b.x + 100;
    Plan p;
    const int rc = plan_call(k.rollout ? "t1d_rollout_pid" : "t1d_step", &c, &b, k.minutes, k.n_sub, k.rollout, &p);
    std::string got = rc ? "error " + std::to_string(rc) + " " + t1d_last_error() : describe(p);
    if (show_tables) got += p.tables ? " tables" : " no tables";
    const bool ok = got == want;
    printf("%s %-56s %s\n", ok ? "ok  " : "FAIL", name, got.c_str());
    if (!ok) { printf("     %-56s %s\n", "expected", want.c_str()); ++g_failed; }
    ++g_rows;
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
    printf("%d rows, %d failed\n", g_rows, g_failed);
    return g_failed ? 1 : 0;
}
