// mcx_host_launch.hpp -- which kernels run: the three selection tables (step / group / scam) and their launchers -- each pooled entry
// naming the shared layouts it reads -- and plan_kernels, the one place that reads the test switches and holds the "where it wins" rules,
// run once at mcmcx_init; its KernelPlan (mcx_host_engine.hpp) is all the launchers, mcmcx_init and pooled_alloc consult.
// Part of the ONE translation unit mcx_api.hip (included there, in this order: mcx_host_engine, mcx_host_linalg, mcx_host_launch,
// mcx_host_adapt, mcx_host_pooled, mcx_host_callbacks); not a stand-alone header.

// (the bytes of dynamic LDS a launch passes come from the kernel's own layout, stated next to the kernel: DESIGN.md)
// one-wave workgroups of `bytes` of LDS cost no occupancy: eight still fit a CU, or all T tiles are resident at once anyway (few chains)
static bool lds_resident(size_t bytes, int T, int cus)
{
    const int per_cu = (int)(LDS_PER_CU / bytes);
    return per_cu >= 8 || (per_cu >= 1 && (long long)T <= (long long)per_cu * cus);
}
static bool pooled_use_mfma(const mcmcx_engine *h, const mcx_switches &sw)
{
    // (SCAM has its own)
    if (!h->pooled || (h->cfg.method != MCMCX_METHOD_DRAM && h->cfg.method != MCMCX_METHOD_RAM
        && h->cfg.method != MCMCX_METHOD_ER)) return false;
    // DR: with its dense tables, and above
    if (h->dodr) {
        // npar 20 (8.3e8 against 8.9e8 iterations/s
        // for the lane kernel with its LDS vectors at 20;
        int dmin = 21;
        // 32: 5.6e8 / 2.5e8, 50: 3.2e8 / 0.8e8)
        if (sw.pooled_mfma_dr_min >= 0) dmin = sw.pooled_mfma_dr_min;
        if (h->d < dmin) return false;
    }
    if (sw.pooled_scalar > 0) return false;                                            // A/B switch for tests: the lane-per-chain kernel
    return PooledMfmaLds(h->d).bytes <= LDS_PER_CU;
}
// iteration cut at the evaluations
static bool phased(const mcmcx_engine *h) { return h->tkind == TGT_HOST || h->tkind == TGT_EXPCOLS || h->tkind == TGT_MODULE; }
// ... except where the DEVICE evaluates between the phases (the response-column target): KernelPlan::fused_cols
static bool phase_cut(const mcmcx_engine *h) { return phased(h) && !h->plan.fused_cols; }
// the step kernels' method class (EngineDev::method): pooled RAM adapts on the host side, the kernels see a plain Metropolis step
static int kernel_method(const mcmcx_engine *h)
{
    const int m = h->cfg.method;
    return (m == MCMCX_METHOD_RAM && !h->pooled) ? M_RAM : (m == MCMCX_METHOD_ER ? M_ER : M_DRAM);
}
static bool dr_fits_lds(const mcmcx_engine *h) { return DrLds::bytes(h->d) <= LDS_PER_CU; }    // npar <= 160
// the phase kernels, step_kernel_cols and run1_kernel: delayed rejection's two work vectors where they are in LDS (EngineDev::dr_lds)
static size_t lds_step(const mcmcx_engine *h) { return DrLds::bytes(h->d, h->plan.dr_lds); }
// step_kernel_dr keeps the second stage's two vectors in LDS, step_kernel_dr_big in global scratch.  LDS pays while eight waves
// still fit a CU (npar <= 20: 6.9e8 against 6.0e8 iterations/s at 20); beyond, the waves it costs are worth more than the bytes
// it saves (npar 24: 3.1e8 against 4.1e8, 64: 3.2e7 / 4.6e7, 100: 0.8e7 / 1.7e7 -- tools/dr_sweep.py)
// (the pooled form, whose factors come through the scalar cache, is bound by that latency rather than by waves: LDS down to four
//  waves per CU -- npar 32: 2.5e8 against 2.2e8, 50: 7.4e7 / 8.1e7, 100: 0.8e7 / 1.3e7 -- tools/pooled_dr_probe.py)
static bool dr_vectors_in_lds(const mcmcx_engine *h, const mcx_switches &sw, int min_waves)
{
    if (!dr_fits_lds(h)) return false;
    if (sw.dr_big >= 0) return sw.dr_big == 0;                                        // A/B switch for tests: 1 = global scratch, 0 = LDS
    return DrLds::bytes(h->d) * (size_t)min_waves <= LDS_PER_CU;
}
static void launch_init(mcmcx_engine *h)
{ hipLaunchKernelGGL(init_kernel, dim3(h->ntiles), dim3(64), 0, h->stream, h->E); }
// ---- which sampling kernel runs: ONE table per launcher, walked in order by plan_kernels -- the first entry whose predicate holds is
// the one the launcher runs, its name noted at each launch for mcmcx_last_kernel (bench.py labels its roofline with it).  The
// predicates read the configuration and the plan only.  The tables are exported through mcmcx_debug_kernel_table, so that
// tests/test_kernel_table.py can list every selectable instance and require a parity test that asserted each of them.  A configuration
// no entry accepts is an error of the run (launch_err), never a silent no-launch.
struct KernelEntry {
    const char *family;                                   // "step" (launch_step), "group" (launch_group), "scam" (launch_scam)
    const char *name;
    bool (*when)(const mcmcx_engine *);
    void (*launch)(mcmcx_engine *, int it0, int it1);  // (nullptr: PHASE_TABLE -- host_iteration launches the phases)
    unsigned shared = 0;                                  // pooled mode: the SharedLayout bits its kernel reads (SH_R: E.sharedR's factor)
};
static const KernelEntry *pick_entry(const mcmcx_engine *h, const KernelEntry *tab, size_t n)
{
    for (size_t i = 0; i < n; ++i)
        if (tab[i].when(h)) return &tab[i];
    return nullptr;
}
static void launch_entry(mcmcx_engine *h, const KernelEntry *e, const char *family, int it0, int it1)
{
    if (!e) { h->launch_err = std::string("no ") + family + " kernel covers this configuration"; return; }
    h->last_kernel = e->name;
    h->last_instance = nullptr;                           // (a launcher that stands for several template instances names the one it takes)
    e->launch(h, it0, it1);
}
// ---- the lane-group step kernel (mcx_group.hpp): four chains per wave, factors in registers
static const int GROUP_MAXSEG = 256;                  // iterations per launch (one accept byte per chain and iteration in d_accb)
static const int GROUP_MAX_NPAR = 64, GROUP_MAX_NPAR_DR = 32;      // (with delayed rejection three tables must fit a lane's registers)
// what the kernel covers: MCMC_run with per-chain Cholesky factors (method 'dram', with or without delayed rejection), one of
// the single-launch device targets, one response column
static bool group_covers(const mcmcx_engine *h)
{
    const mcmcx_config &c = h->cfg;
    return !h->pooled && (c.method == MCMCX_METHOD_DRAM || (c.method == MCMCX_METHOD_ER && !h->dodr)) && !h->usesvd && !phased(h)
        && h->ny == 1 &&
           (h->tkind == TGT_GAUSS || h->tkind == TGT_BANANA || h->tkind == TGT_EXPDATA) && h->d <= (h->dodr ? GROUP_MAX_NPAR_DR
               : GROUP_MAX_NPAR) &&
           !(h->tkind == TGT_BANANA && h->d < 2) && !(h->tkind == TGT_EXPDATA && h->d < 2);
}
// ... and where it is the faster one (tools/group_sweep.py, profiles/r04_a/group_sweep.txt: proposals/s of both kernel families over npar,
// target, delayed rejection and chain count).  Up to 16384 chains always: the chip is not full, a chain's iteration is latency, and
// sixteen lanes per chain with the factors on chip take 2-5 us where a lane takes 7-160 (4x-33x).  With the chip full, from npar 11
// on: 1.04-1.3x without delayed rejection up to npar 20 and 1.7-3x above, 1.1-3.7x with it; at npar <= 10 the lane kernels, which keep
// the factor in LDS there, stay ahead (group: 0.35-0.9x).
// ... and with which group width: four lanes per chain (sixteen chains per wave) for small npar with the chip full, where sixteen lanes
// would mostly idle (tools/quad_sweep.py, profiles/r04_b/quad_sweep.txt: without delayed rejection 1.3-3.6x the sixteen-lane form at npar
// <= 16 and 1.1-3.2x the lane kernels up to 131072 chains -- 1.5-1.7x at any count from npar 11 on; with it at npar <= 8)
static int group_width(const mcmcx_engine *h)
{
    if ((long long)h->cfg.nchains <= 16384 || h->d > 16 || h->cfg.updatesigma) return 16;
    if (!h->dodr) return 4;
    return h->d <= 8 ? 4 : 16;
}
static bool group_wins(const mcmcx_engine *h, int drm, int gw)
{
    const long long n = h->cfg.nchains;
    const int d = h->d;
    if (h->cfg.updatesigma) {
        // MCMC_updatesigma2's gamma sampler is a serial, data-dependent sequence of draws per chain: a group wave runs it for four chains,
        // a lane wave for 64 (tools/group_probe2.py: 2.3-12x up to 1024 chains, 0.9-5x at 16384, 0.45-0.8x beyond without delayed
        // rejection, 1.3-1.6x with it at npar 20)
        if (n <= 8192) return true;
        if (n <= 16384) return d >= 4;
        return h->dodr && d >= 11;
    }
    if (n <= 16384) return true;
    if (gw == 4) return h->dodr ? (drm == 2 || n <= 131072) : (d >= 11 || n <= 131072);
    return d >= 11 || (h->dodr && d >= 9 && n <= 131072);
}
// an instance's name for mcmcx_debug_last_instance, from the template parameters themselves: "group_step_kernel<16,20,2,gauss>"
static std::string group_inst_name(int gw, int d4, int drm, int tk)
{
    const char *t = tk == TGT_GAUSS ? "gauss" : tk == TGT_BANANA ? "banana" : tk == TGT_EXPDATA ? "expdata" : "any";
    return "group_step_kernel<" + std::to_string(gw) + "," + std::to_string(d4) + "," + std::to_string(drm) + "," + t + ">";
}
// one instantiation per (group width, npar rounded up, delayed-rejection form, target kind); DRM 0 = none, 1 = the general form (R, R2, iC
// in registers), 2 = drscale a power of two (no R2; iC in LDS): the instantiation without R2 runs unless the device flag says that some
// factor leaves the range in which R'z / drscale is R2'z bit for bit; the general one is queued behind the same flag and returns at once
// otherwise
template <int GW, int D4, int DRM, int TK>
static void launch_group_inst(mcmcx_engine *h, int it0, int it1)
{
    const dim3 g(h->ntiles * (GW == 16 ? 16 : 4)), b(64);           // 64 / GW chains per wave
    const double *lam = h->E.tgt.lamT;
    // what the branches below launch, in their order (a refusal fails the run whatever the name says)
    static const std::string inst = DRM == 0 ? group_inst_name(GW, D4, 0, TK) : DRM == 1 ? group_inst_name(GW, D4, 1, -1)
        : group_inst_name(GW, D4, 2, TK) + "+" + group_inst_name(GW, D4, 1, -1);
    h->last_instance = inst.c_str();
    if constexpr (DRM != 0 && D4 > GROUP_MAX_NPAR_DR) h->launch_err = "group kernel: no delayed-rejection instantiation above npar " +
        std::to_string(GROUP_MAX_NPAR_DR);
    else if constexpr (TK == TGT_EXPDATA && D4 != 4) h->launch_err = "group kernel: the expdata target has two parameters";
    else if constexpr (DRM == 0) hipLaunchKernelGGL((group_step_kernel<GW, D4, 0, TK>), g, b, 0, h->stream, h->E, it0, it1, lam, h->d_accb,
        (const int *)nullptr, 0);
    else if constexpr (DRM == 1) hipLaunchKernelGGL((group_step_kernel<GW, D4, 1, -1>), g, b, 0, h->stream, h->E, it0, it1, lam, h->d_accb,
        (const int *)nullptr, 0);
    else {
        hipLaunchKernelGGL((group_step_kernel<GW, D4, 2, TK>), g, b, 0, h->stream, h->E, it0, it1, lam, h->d_accb, (const int *)h->d_gflag,
            0);
        hipLaunchKernelGGL((group_step_kernel<GW, D4, 1, -1>), g, b, 0, h->stream, h->E, it0, it1, lam, h->d_accb, (const int *)h->d_gflag,
            1);
    }
}
template <int GW, int D4, int DRM>
static void launch_group_tk(mcmcx_engine *h, int it0, int it1)
{
    if (h->tkind == TGT_BANANA) launch_group_inst<GW, D4, DRM, TGT_BANANA>(h, it0, it1);
    else if (h->tkind == TGT_EXPDATA) launch_group_inst<GW, D4, DRM, TGT_EXPDATA>(h, it0, it1);
    else launch_group_inst<GW, D4, DRM, TGT_GAUSS>(h, it0, it1);
}
template <int GW, int DRM>
static void launch_group_d4(mcmcx_engine *h, int it0, int it1)
{
    if constexpr (GW == 4) {                              // quads: npar <= 16
        switch (h->plan.group_d4) {
        case 4: launch_group_tk<4, 4, DRM>(h, it0, it1); break;
        case 8: launch_group_tk<4, 8, DRM>(h, it0, it1); break;
        case 12: launch_group_tk<4, 12, DRM>(h, it0, it1); break;
        case 16: launch_group_tk<4, 16, DRM>(h, it0, it1); break;
        default: h->launch_err = "group kernel (quads): npar > 16";
        }
    } else {
        switch (h->plan.group_d4) {
        case 4: launch_group_tk<16, 4, DRM>(h, it0, it1); break;
        case 8: launch_group_tk<16, 8, DRM>(h, it0, it1); break;
        case 12: launch_group_tk<16, 12, DRM>(h, it0, it1); break;
        case 16: launch_group_tk<16, 16, DRM>(h, it0, it1); break;
        case 20: launch_group_tk<16, 20, DRM>(h, it0, it1); break;
        case 24: launch_group_tk<16, 24, DRM>(h, it0, it1); break;
        default:
            // DRM = 2 (iC as a square in LDS) is the plan's choice up to npar 24 only (plan_kernels): larger sizes are not instantiated --
            // at 28 / 32 they could not hold the two waves per SIMD they would declare (Weak 12)
            if constexpr (DRM != 2) {
                switch (h->plan.group_d4) {
                case 28: launch_group_tk<16, 28, DRM>(h, it0, it1); return;
                case 32: launch_group_tk<16, 32, DRM>(h, it0, it1); return;
                default: break;
                }
            }
            if constexpr (DRM == 0) {                                    // (above 32: sizes of eight, no delayed rejection)
                switch (h->plan.group_d4) {
                case 40: launch_group_tk<16, 40, DRM>(h, it0, it1); return;
                case 48: launch_group_tk<16, 48, DRM>(h, it0, it1); return;
                case 56: launch_group_tk<16, 56, DRM>(h, it0, it1); return;
                case 64: launch_group_tk<16, 64, DRM>(h, it0, it1); return;
                default: break;
                }
            }
            h->launch_err = "group kernel: no instantiation for npar " + std::to_string(h->d) + " with delayed-rejection mode " +
                std::to_string(DRM);
        }
    }
}
static const KernelEntry GROUP_TABLE[] = {
    {"group", "group_step_kernel",            [](const mcmcx_engine *h) { return h->plan.group_gw == 16 && h->plan.group_drm == 0; },
        launch_group_d4<16, 0>},
    {"group", "group_step_kernel<DR>",        [](const mcmcx_engine *h) { return h->plan.group_gw == 16 && h->plan.group_drm == 1; },
        launch_group_d4<16, 1>},
    {"group", "group_step_kernel<DR2>",       [](const mcmcx_engine *h) { return h->plan.group_gw == 16 && h->plan.group_drm == 2; },
        launch_group_d4<16, 2>},
    {"group", "group_step_kernel<quad>",      [](const mcmcx_engine *h) { return h->plan.group_gw == 4 && h->plan.group_drm == 0; },
        launch_group_d4<4, 0>},
    {"group", "group_step_kernel<quad, DR>",  [](const mcmcx_engine *h) { return h->plan.group_gw == 4 && h->plan.group_drm == 1; },
        launch_group_d4<4, 1>},
    {"group", "group_step_kernel<quad, DR2>", [](const mcmcx_engine *h) { return h->plan.group_gw == 4 && h->plan.group_drm == 2; },
        launch_group_d4<4, 2>},
};
static void launch_group(mcmcx_engine *h, int it0, int it1)
{
    if (h->plan.group_drm == 2 && h->group_check_due) {  // the factors have been rewritten since the last look
        (void)hipMemsetAsync(h->d_gflag, 0, sizeof(int), h->stream);
        hipLaunchKernelGGL(group_check_kernel, dim3(h->ntiles), dim3(64), 0, h->stream, h->E, h->d_gflag);
        h->group_check_due = false;
    }
    launch_entry(h, h->plan.step, "group", it0, it1);
    if (h->d_accb && h->launch_err.empty()) {
        const long long n = (long long)(it1 - it0 + 1) * h->ntiles;
        hipLaunchKernelGGL(group_pack_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, h->stream, h->E, h->d_accb, it0, it1);
    }
}
// pooled_mfma_kernel<false, true>: two waves per SIMD (256 registers, some state spilled) pay with more tiles than SIMDs: from two per SIMD
// where the LDS vector lets eight waves on a CU (npar <= 39: +25 .. +55 %), from eight where it lets six (npar 50: 0.80 at 2048 tiles, 0.99
// at 4096, 1.14 at 16384); with one tile per SIMD the spills are all they buy (0.83 .. 0.90) -- tools/pooled_waves_probe.py
static bool pooled_two_waves(const mcmcx_engine *h, const mcx_switches &sw)
{
    // (test switch: either instance on a small problem)
    if (sw.pooled_waves == 1 || sw.pooled_waves == 2) return sw.pooled_waves == 2;
    return h->ntiles >= (PooledMfmaLds(h->d).bytes * 8 <= LDS_PER_CU ? 2048 : 8192);
}
// pooled_mfma_ks_kernel: the forty-row LDS vector (eight tiles on a CU whatever npar is) where the whole vector leaves fewer, for the
// problems that fill those CUs: npar 41..64, no delayed rejection, and two tiles per SIMD or more.  Against pooled_mfma_kernel<false, true>
// at 16384 tiles (tools/pooled_ks_sweep.py, profiles/r06_j): 1.00 at npar 41 / 44 (seven tiles there), 1.06 .. 1.10 at 45..52 (six),
// 1.12 .. 1.25 at 53..64 (five); with a non-Gaussian target 1.05 .. 1.42.  Against what the engine took before at fewer tiles
// (tools/pooled_ks_tiles.py; pooled_mfma_kernel<false> below 8192): 1.15 .. 1.22 at 2048 / 4096 tiles for npar 45 / 50, 0.98 / 1.02 at 64;
// 0.63 .. 0.69 at 1024 tiles (one per SIMD: the spills are all two waves buy there).
static bool pooled_forty_rows(const mcmcx_engine *h, const mcx_switches &sw)
{
    const int d4 = (h->d + 3) & ~3;
    if (!pooled_use_mfma(h, sw) || h->dodr || d4 <= PKS || d4 > 64) return false;
    // (test switch: either form on a small problem)
    if (sw.pooled_ks == 0 || sw.pooled_ks == 1) return sw.pooled_ks == 1;
    return sw.pooled_waves != 1 && h->ntiles >= 2048;
}
#define STEP_ARGS h->stream, h->E, it0, it1
#define STEP_RS (h->d_ramscale + it0)
#define STEP_TGT h->E.tgt.mu, h->E.tgt.lamT
#define G1 dim3(h->ntiles), dim3(64)
// a step form's launch (mcx_step.hpp): the form names its kernel and its LDS
#define STEP_LAUNCH(Form, ...) hipLaunchKernelGGL((step_entry(Form())), G1, StepLds<Form>::bytes(h->d, h->P), STEP_ARGS, __VA_ARGS__)
// method = 'ram' with few chains: sixteen lanes per chain, the factor in registers, dchud / dchdd on it there (mcx_group_ram.hpp) where it
// is the faster one (tools/ram_group_sweep.py, profiles/r05_b/ram_group_sweep.txt: chain-iterations/s of both families over npar, chain
// count and regime): one wave per SIMD and four chains per wave, so the chip holds 4096 chains at once and the kernel saturates there
// (1.68e8 / 4.6e8 / 1.1e9 chain-iterations/s at npar 50 / 20 / 10) -- 9x / 6x / 6x the lane kernels up to 4096 chains, still 2.9x / 1.7x /
// 2.0x at 16384 and 1.6x / 1.1x / 1.2x at 32768; from 65536 chains on the streaming kernels are ahead (0.93 / 0.74 / 0.63)
static bool ram_group_wins(const mcmcx_engine *h)
{
    const long long n = h->cfg.nchains;
    return n <= 16384 || (n <= 32768 && h->d >= 17);
}
static bool ram_group_covers(const mcmcx_engine *h)
{
    return !h->pooled && h->cfg.method == MCMCX_METHOD_RAM && !h->usesvd && !phased(h) && h->ny == 1 && h->d <= 64 &&
           (h->tkind == TGT_GAUSS || h->tkind == TGT_BANANA || h->tkind == TGT_EXPDATA) && !(h->tkind == TGT_BANANA && h->d < 2);
}
template <int D4>
static void launch_group_ram_d4(mcmcx_engine *h, int it0, int it1)
{
    static const std::string inst = "group_ram_kernel<" + std::to_string(D4) + ">";
    h->last_instance = inst.c_str();
    hipLaunchKernelGGL((group_ram_kernel<D4, -1>), dim3(h->ntiles * 16), dim3(64), 0, h->stream, h->E, it0, it1,
        (const double *)h->d_ramscale, h->E.tgt.lamT, h->d_accb);
}
static void launch_group_ram(mcmcx_engine *h, int it0, int it1)
{
    switch (h->plan.ram_group_d4) {
    case 16: launch_group_ram_d4<16>(h, it0, it1); break;
    case 32: launch_group_ram_d4<32>(h, it0, it1); break;
    case 56: launch_group_ram_d4<56>(h, it0, it1); break;
    case 64: launch_group_ram_d4<64>(h, it0, it1); break;
    default: h->launch_err = "group_ram_kernel: no instantiation for npar " + std::to_string(h->d); return;
    }
    if (h->d_accb) {
        const long long n = (long long)(it1 - it0 + 1) * h->ntiles;
        hipLaunchKernelGGL(group_pack_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, h->stream, h->E, h->d_accb, it0, it1);
    }
}
#ifdef MCX_VARIANTS                // measured negatives, built only by tools/build_variant.sh -DMCX_VARIANTS -- never part of libmcmcx.so
#include "../../tools/variants/variants.inc"
#else
#define MCX_VARIANT_STEP_ENTRIES
#define MCX_VARIANT_SVD_SWEEP(stream, Gc, rot, state, anyrot, nlanes, d, lss) false
#define MCX_VARIANT_COV(h, g8, n10, noff, it, mode) false
#endif
static const KernelEntry STEP_TABLE[] = {
    // ---- a device target with response columns (nycol >= 1 sums of squares per point): the phases of an iteration in one launch
    // (one instantiation per method class: MCMC_run_ram's carries the rank-one update's panels, the others do not)
    // (a data set per chain, mcmcx_set_target_expdata_all: the same kernels with the evaluations' data loads per lane; never pooled)
    {"step", "step_kernel_cols<ram, pcd>", [](const mcmcx_engine *h) {
        return h->plan.fused_cols && kernel_method(h) == M_RAM && h->cdata_mode != 0; },
     [](mcmcx_engine *h, int it0, int it1) { hipLaunchKernelGGL((step_kernel_cols<1, true>), G1, lds_step(h), STEP_ARGS,
         (const double *)h->d_ramscale, (const double *)nullptr, (const double *)nullptr, (const double *)nullptr); }},
    {"step", "step_kernel_cols<pcd>", [](const mcmcx_engine *h) { return h->plan.fused_cols && h->cdata_mode != 0; },
     [](mcmcx_engine *h, int it0, int it1) { hipLaunchKernelGGL((step_kernel_cols<0, true>), G1, lds_step(h), STEP_ARGS,
         (const double *)h->d_ramscale, (const double *)nullptr, (const double *)nullptr, (const double *)nullptr); }},
    {"step", "step_kernel_cols<ram>", [](const mcmcx_engine *h) { return h->plan.fused_cols && kernel_method(h) == M_RAM; },
     [](mcmcx_engine *h, int it0, int it1) { hipLaunchKernelGGL(step_kernel_cols<1>, G1, lds_step(h), STEP_ARGS,
         (const double *)h->d_ramscale, (const double *)nullptr, (const double *)nullptr, (const double *)nullptr); }},
    {"step", "step_kernel_cols", [](const mcmcx_engine *h) { return h->plan.fused_cols; },
     [](mcmcx_engine *h, int it0, int it1) { hipLaunchKernelGGL(step_kernel_cols<0>, G1, lds_step(h), STEP_ARGS,
         (const double *)h->d_ramscale, (const double *)(h->pooled ? h->E.sharedR : nullptr), (const double *)h->pool.d_R2,
         (const double *)h->pool.d_iC); }, SH_R | SH_DR},
    // ---- pooled mode (one shared factor)
    {"step", "pooled_mfma_kernel<true>", [](const mcmcx_engine *h) { return h->plan.pooled_dr_mfma; },
     [](mcmcx_engine *h, int it0, int it1) { hipLaunchKernelGGL(pooled_mfma_kernel<true>, G1, PooledMfmaLds(h->d).bytes, STEP_ARGS,
         STEP_TGT, h->pool.d_RT, h->pool.d_R2T, h->pool.d_iCd); }, SH_RT | SH_DRT},
    MCX_VARIANT_STEP_ENTRIES
    {"step", "pooled_mfma_ks_kernel", [](const mcmcx_engine *h) { return h->plan.pooled_forty_rows; },
     [](mcmcx_engine *h, int it0, int it1) {
         // (npar 49..52: the fourth output block has four rows and goes through the 4 x 4 x 4 instruction)
         const size_t lds = pooled_ks_lds();
         if (((h->d + 3) & ~3) == 52) hipLaunchKernelGGL(pooled_mfma_ks_kernel<true>, G1, lds, STEP_ARGS, STEP_TGT, h->pool.d_RT);
         else hipLaunchKernelGGL(pooled_mfma_ks_kernel<false>, G1, lds, STEP_ARGS, STEP_TGT, h->pool.d_RT); }, SH_RT},
    {"step", "pooled_mfma_kernel<false, true>", [](const mcmcx_engine *h) {
        return h->plan.pooled_mfma && h->plan.pooled_two_waves; },
     [](mcmcx_engine *h, int it0, int it1) { hipLaunchKernelGGL((pooled_mfma_kernel<false, true>), G1, PooledMfmaLds(h->d).bytes, STEP_ARGS,
         STEP_TGT, h->pool.d_RT, (const double *)nullptr, (const double *)nullptr); }, SH_RT},
    {"step", "pooled_mfma_kernel<false>", [](const mcmcx_engine *h) { return h->plan.pooled_mfma; },
     [](mcmcx_engine *h, int it0, int it1) { hipLaunchKernelGGL(pooled_mfma_kernel<false>, G1, PooledMfmaLds(h->d).bytes, STEP_ARGS,
         STEP_TGT, h->pool.d_RT, (const double *)nullptr, (const double *)nullptr); }, SH_RT},
    {"step", "step_kernel_pooled_dr_big", [](const mcmcx_engine *h) { return h->pooled && h->dodr && !h->plan.dr_vectors_in_lds; },
     [](mcmcx_engine *h, int it0, int it1) { STEP_LAUNCH(StepPooledDrBig, STEP_RS, STEP_TGT, h->E.sharedR, h->pool.d_R2, h->pool.d_iC); },
     SH_R | SH_DR},
    {"step", "step_kernel_pooled_dr", [](const mcmcx_engine *h) { return h->pooled && h->dodr; },
     [](mcmcx_engine *h, int it0, int it1) { STEP_LAUNCH(StepPooledDr, STEP_RS, STEP_TGT, h->E.sharedR, h->pool.d_R2, h->pool.d_iC); },
     SH_R | SH_DR},
    {"step", "step_kernel<false, false, true>", [](const mcmcx_engine *h) { return h->pooled != 0; },
     [](mcmcx_engine *h, int it0, int it1) { STEP_LAUNCH(StepPooled, STEP_RS, STEP_TGT, h->E.sharedR); }, SH_R},
    // ---- method = 'ram', per-chain factors
    {"step", "group_ram_kernel", [](const mcmcx_engine *h) { return h->plan.ram_group_d4 != 0; }, launch_group_ram},
    {"step", "step_kernel_ram_fullr", [](const mcmcx_engine *h) { return kernel_method(h) == M_RAM && h->usesvd; },
     [](mcmcx_engine *h, int it0, int it1) { STEP_LAUNCH(StepRamFullr, STEP_RS, STEP_TGT, h->E.sharedR); }},
    {"step", "step_kernel_ram_ldsr", [](const mcmcx_engine *h) {
        return kernel_method(h) == M_RAM && h->plan.lds_form == LDS_RAM_R; },
     [](mcmcx_engine *h, int it0, int it1) { STEP_LAUNCH(StepRamLdsr, STEP_RS, STEP_TGT, h->E.sharedR); }},
    {"step", "step_kernel_ram_wide", [](const mcmcx_engine *h) {
        return kernel_method(h) == M_RAM && h->d > RAM_SMALL_MAX && h->plan.ram_wide; },
     [](mcmcx_engine *h, int it0, int it1) { STEP_LAUNCH(StepRamWide, STEP_RS, STEP_TGT, h->d_pair); }},
    {"step", "step_kernel<true, false, false>", [](const mcmcx_engine *h) { return kernel_method(h) == M_RAM; },
     [](mcmcx_engine *h, int it0, int it1) { STEP_LAUNCH(StepRam, STEP_RS, STEP_TGT, h->E.sharedR); }},
    // ---- delayed rejection, per-chain factors: the second stage's two vectors in global scratch / in LDS
    {"step", "step_kernel_dr_big", [](const mcmcx_engine *h) { return h->dodr && !h->plan.dr_vectors_in_lds; },
     [](mcmcx_engine *h, int it0, int it1) { hipLaunchKernelGGL(step_kernel_dr_big, G1, 0, STEP_ARGS, STEP_TGT); }},
    {"step", "step_kernel_dr", [](const mcmcx_engine *h) { return h->dodr != 0; },
     [](mcmcx_engine *h, int it0, int it1) { hipLaunchKernelGGL(step_kernel_dr, G1, DrLds::bytes(h->d), STEP_ARGS, STEP_TGT); }},
    // ---- AM / Metropolis / early rejection: state + factor in LDS, state in LDS, nothing in LDS
    {"step", "step_kernel_ldsr", [](const mcmcx_engine *h) { return h->plan.lds_form == LDS_STATE_R; },
     [](mcmcx_engine *h, int it0, int it1) { STEP_LAUNCH(StepLdsr, STEP_RS, STEP_TGT, h->E.sharedR); }},
    {"step", "step_kernel_ldsv", [](const mcmcx_engine *h) { return h->plan.lds_form != LDS_NONE; },
     [](mcmcx_engine *h, int it0, int it1) { STEP_LAUNCH(StepLdsv, STEP_RS, STEP_TGT, h->E.sharedR); }},
    {"step", "step_kernel<false, false, false>", [](const mcmcx_engine *) { return true; },
     [](mcmcx_engine *h, int it0, int it1) { STEP_LAUNCH(StepPlain, STEP_RS, STEP_TGT, h->E.sharedR); }},
};
static void launch_step(mcmcx_engine *h, int it0, int it1)
{
    if (h->plan.group_d4) launch_group(h, it0, it1);
    else launch_entry(h, h->plan.step, "step", it0, it1);
}
// every chain's copy of a K-vector, filled on the device
static int dev_bcast(mcmcx_engine *h, double *dst, const std::vector<double> &v)
{
    double *tmp = nullptr;
    HIPCHK(hipMalloc(&tmp, v.size() * sizeof(double)));
    hipError_t e = hipMemcpy(tmp, v.data(), v.size() * sizeof(double), hipMemcpyHostToDevice);
    if (e == hipSuccess) {
        const unsigned gy = (unsigned)std::min<size_t>(v.size(), 64);
        hipLaunchKernelGGL(bcast_kernel, dim3(h->ntiles, gy), dim3(64), 0, h->stream, dst, tmp, v.size());
        e = hipGetLastError();
        if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
    }
    (void)hipFree(tmp);
    if (e != hipSuccess) return fail(-100, hipGetErrorString(e));
    return 0;
}
// the dense layout's length (PooledState): d4 rows (pad rows zero) + slack; the stride of pooled SCAM's U block
static size_t dense_len(const mcmcx_engine *h) { return (size_t)((h->d + 3) & ~3) * h->d + PWS; }
// 13..15 output blocks (npar 193..240): twelve waves of 170 registers (scam_pooled12_kernel) instead of sixteen of 128
static bool scam_use_12(const mcmcx_engine *h, const mcx_switches &sw)
{
    const int nt = (h->d + 15) / 16;
    if (sw.scam_pooled_16 > 0) return false;                                          // A/B switch for tests: the sixteen-wave layout
    return nt >= 13 && nt <= 15;
}
// opt-in fast proposals with the Gaussian target: the workgroup-per-tile kernel of the pooled mode with each chain's own
// rotation column (g_U = nullptr) -- the target's d x d product on the matrix cores instead of lane by lane
static bool scam_fast_tile_kernel(const mcmcx_engine *h, const mcx_switches &sw)
{
    return h->cfg.scam_fast && h->tkind == TGT_GAUSS && !h->has_lo && !h->has_hi && !h->has_pri &&
           ScamPooledLds(h->d).bytes <= LDS_PER_CU && !(sw.scam_fast_lanes > 0);
}
// few tiles: several waves per tile (scam_mw_kernel), so that a sub-step is not bound by the latency of one wave's loads
// while most of the chip idles -- as many waves as keep the chip's ~2048 resident-wave slots busy, at most 8 (sixteen
// waves of 128 registers spill the products' panels)
static int scam_tile_waves(const mcmcx_engine *h, const mcx_switches &sw)
{
    int nw = 1;
    // (1024 tiles x npar 200: 8.4e6 at two waves per tile, 8.9e6 at four, 9.0e6 at eight -- profiles/r05_d/c5rep_waves.txt)
    while (nw < 8 && (long long)h->ntiles * nw * 2 <= 8192) nw *= 2;
    { const int v = sw.scam_waves; if (v == 1 || v == 2 || v == 4 || v == 8) nw = v; }   // A/B switch for tests
    // (npar > 1200: the one-wave kernel needs no LDS)
    if (ScamMwLds(h->d).bytes > LDS_PER_CU) nw = 1;
    return nw;
}
#define SCAM_POOLED_ARGS ScamPooledLds(h->d).bytes, h->stream, h->E, it0, it1, h->E.tgt.mu, h->E.tgt.lamT
// (SH_UREP: the per-chain kernels read every chain's own rotation, E.Rf / E.qstd -- in pooled mode above npar 240, copies of the one)
static const KernelEntry SCAM_TABLE[] = {
    {"scam", "step_kernel_cols<scam, pcd>", [](const mcmcx_engine *h) { return h->plan.fused_cols && !h->pooled && h->cdata_mode != 0; },
     [](mcmcx_engine *h, int it0, int it1) { hipLaunchKernelGGL((step_kernel_cols<2, true>), G1, 0, STEP_ARGS,
         (const double *)h->d_ramscale, (const double *)nullptr, (const double *)nullptr, (const double *)nullptr); }},
    {"scam", "step_kernel_cols<scam>", [](const mcmcx_engine *h) { return h->plan.fused_cols && !h->pooled; },
     [](mcmcx_engine *h, int it0, int it1) { hipLaunchKernelGGL(step_kernel_cols<2>, G1, 0, STEP_ARGS, (const double *)h->d_ramscale,
         (const double *)nullptr, (const double *)nullptr, (const double *)nullptr); }},
    // pooled: 16-row output blocks, min(12, 4*(nt/4)) block waves + 4 chain-group waves; twelve waves of 170 registers for 13..15 blocks
    {"scam", "scam_pooled12_kernel", [](const mcmcx_engine *h) { return h->pooled && !h->plan.scam_replicated && h->plan.scam_pooled12; },
     [](mcmcx_engine *h, int it0, int it1) { const size_t st = dense_len(h);
        hipLaunchKernelGGL(scam_pooled12_kernel, dim3(h->ntiles), dim3(768), SCAM_POOLED_ARGS, h->pool.d_U, h->pool.d_U + st,
            h->pool.d_U + 2 * st); }, SH_U},
    {"scam", "scam_pooled_kernel", [](const mcmcx_engine *h) { return h->pooled && !h->plan.scam_replicated; },
     [](mcmcx_engine *h, int it0, int it1) { const size_t st = dense_len(h); const int nw = 4 + std::min(12, ((h->d + 15) / 16) & ~3);
        hipLaunchKernelGGL(scam_pooled_kernel, dim3(h->ntiles), dim3(64 * nw), SCAM_POOLED_ARGS, h->pool.d_U, h->pool.d_U + st,
            h->pool.d_U + 2 * st); }, SH_U},
    // (the sixteen-wave layout whatever npar: every lane fetches the column of its own chain's factor per sub-step, and four
    //  waves per SIMD cover that better than three -- 4.62e8 against 4.45e8 proposals/s at npar 200)
    {"scam", "scam_pooled_kernel<per-chain>", [](const mcmcx_engine *h) { return h->plan.scam_fast_tile; },
     [](mcmcx_engine *h, int it0, int it1) { const int nw = 4 + std::min(12, ((h->d + 15) / 16) & ~3);
        hipLaunchKernelGGL(scam_pooled_kernel, dim3(h->ntiles), dim3(64 * nw), SCAM_POOLED_ARGS, (const double *)nullptr,
            (const double *)nullptr, (const double *)nullptr); }, SH_UREP},
    {"scam", "scam_mw_kernel<8>", [](const mcmcx_engine *h) { return h->plan.scam_waves == 8; },
     [](mcmcx_engine *h, int it0, int it1) { hipLaunchKernelGGL(scam_mw_kernel<8>, dim3(h->ntiles), dim3(512), ScamMwLds(h->d).bytes,
         STEP_ARGS, STEP_TGT); }, SH_UREP},
    {"scam", "scam_mw_kernel<4>", [](const mcmcx_engine *h) { return h->plan.scam_waves == 4; },
     [](mcmcx_engine *h, int it0, int it1) { hipLaunchKernelGGL(scam_mw_kernel<4>, dim3(h->ntiles), dim3(256), ScamMwLds(h->d).bytes,
         STEP_ARGS, STEP_TGT); }, SH_UREP},
    {"scam", "scam_mw_kernel<2>", [](const mcmcx_engine *h) { return h->plan.scam_waves == 2; },
     [](mcmcx_engine *h, int it0, int it1) { hipLaunchKernelGGL(scam_mw_kernel<2>, dim3(h->ntiles), dim3(128), ScamMwLds(h->d).bytes,
         STEP_ARGS, STEP_TGT); }, SH_UREP},
    {"scam", "scam_kernel", [](const mcmcx_engine *) { return true; },
     [](mcmcx_engine *h, int it0, int it1) { hipLaunchKernelGGL(scam_kernel, G1, 0, STEP_ARGS, STEP_TGT); }, SH_UREP},
};
static void launch_scam(mcmcx_engine *h, int it0, int it1) { launch_entry(h, h->plan.scam, "scam", it0, it1); }
// ---- pooled mode with the iteration cut at the USER's evaluations (a target module's kernel or host callbacks between the engine's
// launches): no launcher runs a segment, host_iteration (mcx_host_callbacks.hpp) launches the phases one by one in the form the plan names
// here, and notes the entry's name for mcmcx_last_kernel.  The entries exist for that name and for the shared layouts they declare.
// The matrix-core form covers what one pass of four output blocks does (npar <= 64, the largest a target module is compiled for by
// default); its second stage reads the dense R2 (SH_DRT) and, for the two quadratic forms, the packed inverse covariance (SH_DR).
static const int POOLED_PHASE_MFMA_MAX_NPAR = 64;
// ... and where it wins: tools/pooled_phase_sweep.py (profiles/r08_a/phase_form_sweep.txt), the test module's iteration in both forms over
// npar 10 / 20 / 50 / 64 and 1024 / 65536 / 1048576 chains, user kernel and ticks included: everywhere measured -- lane / mfma 1.18 .. 1.29
// at npar 10, 1.21 .. 1.38 at 20, 1.37 .. 1.63 at 50, 1.25 .. 1.72 at 64 without delayed rejection, 1.07 .. 1.27 with it (its two quadratic
// forms stay on the scalar cache in both).  No crossover inside that range: the lane form keeps what was not measured, npar < 10, and
// what the one-pass product does not cover.  MCMCX_POOLED_PHASE_MFMA = 1 / 0 forces either form where both cover (A/B, tests).
static bool pooled_phase_mfma(const mcmcx_engine *h, const mcx_switches &sw)
{
    if (h->d > POOLED_PHASE_MFMA_MAX_NPAR) return false;
    if (sw.pooled_phase_mfma == 0 || sw.pooled_phase_mfma == 1) return sw.pooled_phase_mfma == 1;
    return h->d >= 10;
}
static const KernelEntry PHASE_TABLE[] = {
    {"scam", "host_phase_kernel<pooled scam>", [](const mcmcx_engine *h) { return h->cfg.method == MCMCX_METHOD_SCAM; }, nullptr, SH_UREP},
    {"step", "pooled_phase_mfma_kernel", [](const mcmcx_engine *h) { return h->plan.pooled_phase == 2; }, nullptr,
        SH_RT | SH_DRT | SH_DR},
    {"step", "pooled_phase_kernel", [](const mcmcx_engine *h) { return h->plan.pooled_phase == 1; }, nullptr, SH_R | SH_DR},
};
// the adaptation's SVD one workgroup per chain (mcx_svd.hpp) where its rings and row groups are instantiated
static const int SVD_BLOCKED_MIN = 48, SVD_BLOCKED_MAX = 256;
static bool svd_blocked(const mcmcx_engine *h, const mcx_switches &sw)
{
    if (!h->usesvd || h->pooled || h->cfg.method == MCMCX_METHOD_RAM) return false;
    // test switch: the lane SVD (the engine's form below npar 48 and above 256)
    if (sw.svd_lane > 0) return false;
    // (its rings and row groups are instantiated up to npar 256)
    return h->d >= SVD_BLOCKED_MIN && h->d <= SVD_BLOCKED_MAX;
}
// the blocked SVD's forms (SvdPlan): from npar (SVD_BLOCKED_MIN .. SVD_BLOCKED_MAX) and the number of chains alone
#define MCX_SVD_FORM(field, kernel) (a.field = kernel, #kernel)
static SvdPlan plan_svd(int d, int nlanes)
{
    SvdPlan a;
    if (d <= 200) {
        const int RL = d <= 64 ? 8 : d <= 128 ? 16 : 25;
        a.sweep_name = RL == 8 ? MCX_SVD_FORM(sweep32, svd_sweep_stream32_kernel<8>)
            : RL == 16 ? MCX_SVD_FORM(sweep32, svd_sweep_stream32_kernel<16>) : MCX_SVD_FORM(sweep32, svd_sweep_stream32_kernel<25>);
        a.sweep_lds = svd_ring_lds(svd_ring_cols(32, false), svd_ring_ls(RL));
    } else {
        const int RL = d <= 208 ? 26 : 32;
        a.svd_sb = 24;                               // pair-lanes: whole waves of octets, one wave of loaders at least
        a.sweep_name = RL == 26 ? MCX_SVD_FORM(sweep, svd_sweep_stream_kernel<26>) : MCX_SVD_FORM(sweep, svd_sweep_stream_kernel<32>);
        a.sweep_lds = svd_ring_lds(svd_ring_cols(a.svd_sb, true), svd_ring_ls(RL));
    }
    const int RP = d <= 64 ? 4 : d <= 128 ? 8 : d <= 208 ? 13 : 16;
    a.applyv_name = RP == 4 ? MCX_SVD_FORM(applyv, svd_applyv_stream32_kernel<4>)
        : RP == 8 ? MCX_SVD_FORM(applyv, svd_applyv_stream32_kernel<8>)
        : RP == 13 ? MCX_SVD_FORM(applyv, svd_applyv_stream32_kernel<13>) : MCX_SVD_FORM(applyv, svd_applyv_stream32_kernel<16>);
    a.applyv_lds = svd_ring_lds(svd_ring_cols(32, false), svd_ring_slot(RP));
    a.applyv_grid = (unsigned)(32 * ((nlanes + 7) / 8));                  // four one-wave workgroups per chain, a chain's on one XCD
    return a;
}
#undef MCX_SVD_FORM
// the adaptation tick's forms (AdaptPlan): from npar, the tile count and the plan's tile_factor / svd_blocked
static void plan_adapt(const mcmcx_engine *h, KernelPlan &p)
{
    AdaptPlan &a = p.adapt;
    const int d = h->d;
    a.n10 = (d + TD - 1) / TD; a.noff = a.n10 * (a.n10 - 1) / 2;          // blocks of ten (triangular on the diagonal)
    a.g8 = (unsigned)(8 * ((h->ntiles + 7) / 8));
    a.post_lds = adapt_post_lds(d);
    const bool xg = a.post_lds > LDS_PER_CU;
    if (xg) a.post_lds = 0;
    a.post = h->usesvd ? (xg ? adapt_post_kernel<true, true> : adapt_post_kernel<true, false>)
                       : (xg ? adapt_post_kernel<false, true> : adapt_post_kernel<false, false>);
    a.post_name = h->usesvd ? (xg ? "adapt_post_kernel<true,true>" : "adapt_post_kernel<true,false>")
                            : (xg ? "adapt_post_kernel<false,true>" : "adapt_post_kernel<false,false>");
    if (p.tile_factor) {
        const int nc = (d + 15) / 16, nw = nc <= 2 ? 4 : nc == 3 ? 2 : 1, ch = 4 * nw;
        a.factor = nc == 1 ? tile_factor_kernel<1, 4> : nc == 2 ? tile_factor_kernel<2, 4> : nc == 3 ? tile_factor_kernel<3, 2>
            : tile_factor_kernel<4, 1>;
        a.factor_name = nc == 1 ? "tile_factor_kernel<1,4>" : nc == 2 ? "tile_factor_kernel<2,4>" : nc == 3 ? "tile_factor_kernel<3,2>"
            : "tile_factor_kernel<4,1>";
        a.factor_block = (unsigned)(64 * nw);
        a.factor_lds = TileFactorLds(h->P, nw).bytes;
        a.factor_grid = a.g8 * (unsigned)(64 / ch);
    }
    if (p.svd_blocked) a.svd = plan_svd(d, h->nlanes);
}
// ---- the plan: every kernel form the engine takes, decided once at mcmcx_init before anything is allocated.  Its inputs are the
// configuration, the problem's shape, the target kind, the switches (read here, nowhere else) and the CU count; never a device pointer.
static void plan_kernels(mcmcx_engine *h)
{
    mcx_switches sw;
    sw.read();                                       // the A/B switches as the environment has them now: fixed for the engine's life
    KernelPlan &p = h->plan;
    p = KernelPlan();
    const mcmcx_config &c = h->cfg;
    const int d = h->d, P = h->P, T = h->ntiles;
    const bool am = p.am = (c.method != MCMCX_METHOD_RAM) && (c.doadapt != 0 || c.doburnin != 0) && !h->pooled;
    // the response-column target: the phases fused into one launch per segment (step_kernel_cols); MCMCX_COLS_PHASED=1 keeps the
    // separate launches (A/B, tests)
    p.fused_cols = h->tkind == TGT_EXPCOLS && !(sw.cols_phased > 0);
    // pooled mode with a user module or host callbacks: the phase launches read the shared tables (SCAM: every chain's copy of the
    // rotation)
    const bool pphase = h->pooled && phase_cut(h);
    if (pphase && c.method != MCMCX_METHOD_SCAM) p.pooled_phase = pooled_phase_mfma(h, sw) ? 2 : 1;
    // step_kernel_pooled_dr_big's and pooled_mfma_kernel<true>'s quadratic-form vectors; npar > 320: adapt_post_kernel's work vector
    p.xscr = (h->pooled && h->dodr && !pphase) || d > 320;
    p.dr_lds = h->dodr && dr_fits_lds(h);
    p.dr_vectors_in_lds = dr_vectors_in_lds(h, sw, h->pooled ? 4 : 8);
    {   // plain AM / Metropolis / ER step kernel: state and scratch vectors in LDS (4 d x 512 bytes per wave) when that costs no
        // occupancy -- eight waves per CU still fit (npar <= 10), or all tiles are resident at once anyway (few chains)
        hipDeviceProp_t prop;
        int cus = 256;
        if (hipGetDeviceProperties(&prop, c.device) == hipSuccess && prop.multiProcessorCount > 0) cus = prop.multiProcessorCount;
        const bool fits = lds_resident(StepLds<StepLdsv>::bytes(d, P), T, cus);
        // (MCMCX_LDS_SCRATCH = 0: off, A/B)
        p.lds_form = (!h->pooled && !h->dodr && c.method != MCMCX_METHOD_RAM && c.method != MCMCX_METHOD_SCAM && fits
            && sw.lds_scratch != 0) ? LDS_STATE : LDS_NONE;
        // ... and the packed factor with it (step_kernel_ldsr) where one column panel covers npar and state + factor of all tiles
        // are resident at once: (2 npar + npar (npar + 1) / 2) x 512 bytes per wave, 38 KiB at npar = 10 = four waves per CU
        const bool fits_r = lds_resident(StepLds<StepLdsr>::bytes(d, P), T, cus);
        // MCMCX_LDS_SCRATCH=1: the state only (A/B)
        if (p.lds_form != LDS_NONE && !h->usesvd && d <= TW && fits_r && sw.lds_scratch != 1) p.lds_form = LDS_STATE_R;
        // method='ram' (per-chain factor, Cholesky form): the factor DCHUD / DCHDD rewrite every iteration, and their rotations, in LDS for
        // the launch where one column panel covers npar and all tiles are resident at once (step_kernel_ram_ldsr)
        if (!h->pooled && c.method == MCMCX_METHOD_RAM && !h->usesvd && d <= RW && lds_resident(StepLds<StepRamLdsr>::bytes(d, P), T, cus)
            && sw.lds_scratch != 0) p.lds_form = LDS_RAM_R;
    }
    // the user's functions on the host and at most sixteen tiles: candidate, results and flags in mapped host memory -- a phase kernel's
    // stores ARE the hand-over, the host's results are read by the next one in place (MCMCX_HOST_MAPPED=0: device buffers and copies)
    p.host_mapped = h->tkind == TGT_HOST && T <= 16 && sw.host_mapped != 0;
    // (RAM / SCAM use cs as sweep scratch)
    p.cs_mapped = p.host_mapped && (c.method == MCMCX_METHOD_DRAM || c.method == MCMCX_METHOD_ER);
    // (MCMCX_HOST_FUSE=0: one launch per phase, the A/B form the tests compare with)
    p.host_fuse = sw.host_fuse != 0;
    // pooled SCAM: npar > 240: slower, not refused -- scam_kernel / scam_mw_kernel on per-chain copies; a user target: the per-chain phases
    p.scam_replicated = h->usesvd && h->pooled && c.method == MCMCX_METHOD_SCAM && (ScamPooledLds(d).bytes > LDS_PER_CU || pphase);
    p.pooled_mfma = pooled_use_mfma(h, sw) && !pphase;
    p.pooled_dr_mfma = p.pooled_mfma && h->dodr;                 // the second stage on the matrix cores too
    p.pooled_two_waves = pooled_two_waves(h, sw);
    p.pooled_forty_rows = pooled_forty_rows(h, sw);
    p.ram_wide = sw.ram_wide != 0;
    // (MCMCX_RAM_PAIR=0: every update sweep stores the factor -- the A/B form, and the one the tests compare with)
    p.ram_pair = p.ram_wide && sw.ram_pair != 0;
    p.scam_pooled12 = scam_use_12(h, sw);
    p.scam_fast_tile = scam_fast_tile_kernel(h, sw);
    p.scam_waves = scam_tile_waves(h, sw);
    // the lane-group step kernel where it covers the configuration: MCMCX_GROUP = 1 / 0 forces it on / off (A/B, tests)
    if (group_covers(h)) {
        int ex = 0;
        const bool pow2 = h->dodr && c.drscale > 0.0 && std::frexp(c.drscale, &ex) == 0.5 && ex > -64 && ex < 64;
        // (the power-of-two form keeps iC in LDS: above npar 24 that leaves fewer waves per CU than the register form's four)
        const int drm = !h->dodr ? 0 : (pow2 && d <= 24 && sw.group_dr2 != 0) ? 2 : 1;
        // (MCMCX_GROUP_GW 4 / 16: A/B, tests)
        const int gw = (d <= 16 && sw.group_gw != -1) ? (sw.group_gw == 4 ? 4 : 16) : group_width(h);
        if (sw.group != -1 ? sw.group != 0 : group_wins(h, drm, gw)) {
            p.group_d4 = d <= 32 ? ((d + 3) & ~3) : ((d + 7) & ~7);
            p.group_gw = gw;
            p.group_drm = drm;
        }
    }
    // method = 'ram' with few chains on the lane-group kernel (MCMCX_RAM_GROUP = 1 / 0: always where it covers / never; A/B, tests)
    if (ram_group_covers(h)) {
        const int rg = sw.ram_group != -1 ? sw.ram_group : sw.group;  // (the kernel-family switch of the tests covers it too)
        if (rg != -1 ? rg != 0 : ram_group_wins(h)) p.ram_group_d4 = d <= 16 ? 16 : d <= 32 ? 32 : d <= 56 ? 56 : 64;
    }
    // the adaptation's factorisation (Cholesky branch) with the matrices in LDS (tile_factor_kernel): any chain count, npar <= 32 -- config
    // 3's size (npar 20, delayed rejection, 262144 chains): 2.11 -> 1.44 ms per tick, bound by VALU issue (~25 instructions per inner step
    // of four chains). Above npar 32 adapt_post_kernel's 8 x 8 register blocks stay: at npar 50 x 1 048 576 chains they stream the matrices
    // ~5.6 times (16.0 ms) and still beat the LDS form, whose three waves per CU issue ~15 x the instructions per chain (35.2 ms;
    // profiles/r05_a/tick_ab.txt). MCMCX_TILE_FACTOR = 0 / 1: never / up to npar 64 (test switch: both forms on one problem).
    p.tile_factor = am && !h->usesvd && d <= (sw.tile_factor == 1 ? 64 : 32) && sw.tile_factor != 0;
    // (an adaptation that never runs needs no form)
    p.svd_blocked = svd_blocked(h, sw) && (c.doadapt != 0 || c.doburnin != 0);
    // (test switch: covmat_rows, the lane form)
    p.cov_batch = !(sw.cov_batch_rows > 0);
    plan_adapt(h, p);
    // every predicate's inputs are fixed from here on: the launchers run the entry found now
    if (pphase) (c.method == MCMCX_METHOD_SCAM ? p.scam : p.step) = pick_entry(h, PHASE_TABLE,
        sizeof(PHASE_TABLE) / sizeof(PHASE_TABLE[0]));
    else if (c.method == MCMCX_METHOD_SCAM) p.scam = pick_entry(h, SCAM_TABLE, sizeof(SCAM_TABLE) / sizeof(SCAM_TABLE[0]));
    else if (p.group_d4) p.step = pick_entry(h, GROUP_TABLE, sizeof(GROUP_TABLE) / sizeof(GROUP_TABLE[0]));
    else p.step = pick_entry(h, STEP_TABLE, sizeof(STEP_TABLE) / sizeof(STEP_TABLE[0]));
    p.ram_pair = p.ram_pair && p.step && std::strcmp(p.step->name, "step_kernel_ram_wide") == 0;      // (only that kernel pairs)
    // pooled mode: the shared layouts that entry reads (no R2 / iC without DR; the lane kernels read the SVD factor in the dense layout)
    const KernelEntry *e = c.method == MCMCX_METHOD_SCAM ? p.scam : p.step;
    p.shared = (h->pooled && e) ? e->shared & (h->dodr ? ~0u : ~(unsigned)(SH_DR | SH_DRT)) : 0;
    if (h->usesvd && (p.shared & SH_R)) p.shared ^= SH_R | SH_RT;
}
