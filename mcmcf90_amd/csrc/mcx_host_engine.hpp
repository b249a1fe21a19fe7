// mcx_host_engine.hpp -- the engine object behind a mcmcx_handle: error reporting, the test switches, the kernel plan, the host and device
// state of N chains and pooled mode's shared tables (PooledState), allocation helpers.
// Part of the ONE translation unit mcx_api.hip (included there, in this order: mcx_host_engine, mcx_host_linalg, mcx_host_launch,
// mcx_host_adapt, mcx_host_pooled, mcx_host_callbacks); not a stand-alone header.

using namespace mcx;
static_assert(MCMCX_HE_INB == HE_INB && MCMCX_HE_PRI == HE_PRI && MCMCX_HE_SS == HE_SS && MCMCX_HX_STAGE2 == HX_STAGE2
    && MCMCX_HX_CRIT == HX_CRIT,
              "include/mcmcx_target.h and mcx_kernels.hpp disagree about the phase-state slots");

static thread_local std::string g_err;
static int fail(int code, const std::string &msg) { g_err = msg; return code; }

#define HIPCHK(call)                                                                              \
    do {                                                                                          \
        hipError_t e_ = (call);                                                                   \
        if (e_ != hipSuccess)                                                                     \
            return fail(-100, std::string(#call) + ": " + hipGetErrorString(e_));                 \
    } while (0)

// The test switches (tests, tools): each FORCES one of two kernel forms that the engine also chooses by itself for some configuration -- so
// that the parity tests can run both forms on the same small problem.  None selects a form the engine would never take (those live in
// tools/variants, outside this library).  Read from the environment once per engine, by plan_kernels at mcmcx_init (mcx_host_launch.hpp),
// the only code that reads them -- never at launch time.  -1 = not set.
struct mcx_switches {
    int pooled_mfma_dr_min = -1, pooled_scalar = -1, dr_big = -1, scam_pooled_16 = -1, scam_fast_lanes = -1, scam_waves = -1,
        svd_lane = -1, cov_batch_rows = -1, ram_wide = -1, pooled_waves = -1, pooled_ks = -1, cols_phased = -1, host_mapped = -1,
            host_fuse = -1, lds_scratch = -1, group = -1, group_dr2 = -1, group_gw = -1, ram_group = -1, tile_factor = -1,
            pooled_phase_mfma = -1, ram_pair = -1;
    static int get(const char *name) { const char *e = getenv(name); return e ? atoi(e) : -1; }
    void read()
    {
        pooled_mfma_dr_min = get("MCMCX_POOLED_MFMA_DR_MIN"); pooled_scalar = get("MCMCX_POOLED_SCALAR"); dr_big = get("MCMCX_DR_BIG");
        scam_pooled_16 = get("MCMCX_SCAM_POOLED_16"); scam_fast_lanes = get("MCMCX_SCAM_FAST_LANES");
        scam_waves = get("MCMCX_SCAM_WAVES"); svd_lane = get("MCMCX_SVD_LANE"); cov_batch_rows = get("MCMCX_COV_BATCH_ROWS");
        ram_wide = get("MCMCX_RAM_WIDE"); pooled_waves = get("MCMCX_POOLED_WAVES"); pooled_ks = get("MCMCX_POOLED_KS");
        cols_phased = get("MCMCX_COLS_PHASED"); host_mapped = get("MCMCX_HOST_MAPPED"); host_fuse = get("MCMCX_HOST_FUSE");
        lds_scratch = get("MCMCX_LDS_SCRATCH"); group = get("MCMCX_GROUP"); group_dr2 = get("MCMCX_GROUP_DR2");
        group_gw = get("MCMCX_GROUP_GW"); ram_group = get("MCMCX_RAM_GROUP"); tile_factor = get("MCMCX_TILE_FACTOR");
        pooled_phase_mfma = get("MCMCX_POOLED_PHASE_MFMA"); ram_pair = get("MCMCX_RAM_PAIR");
    }
};
// the plain lane step's LDS form (EngineDev::lds_scratch): nothing, the state and scratch vectors (step_kernel_ldsv), those and the packed
// factor (step_kernel_ldsr); method = 'ram': the factor and its rotations (step_kernel_ram_ldsr)
enum LdsForm { LDS_NONE = 0, LDS_STATE = 1, LDS_STATE_R = 2, LDS_RAM_R = 3 };
// pooled mode's device layouts of the shared tables (PooledState), as KernelPlan::shared records which the planned kernel reads
enum SharedLayout { SH_R = 1, SH_RT = 2, SH_DR = 4, SH_DRT = 8, SH_U = 16, SH_UREP = 32 };
struct KernelEntry;
// The adaptation tick's forms (launch_adapt, mcx_host_adapt.hpp): everything about its launches that npar, the tile count and the plan's
// switches decide -- the kernels as pointers to the chosen instantiations, so that the tick compares nothing.
// The blocked SVD's forms (plan_svd, a function of npar and the chain count; launch_svd runs them): the sweep with all 32 lanes of a row
// group on pairs up to npar 200 (svd_sweep_stream32_kernel<RL>), 24 pair-lanes (svd_sb) and a wave of loaders above
// (svd_sweep_stream_kernel<RL>); the log replayed on V (svd_applyv_stream32_kernel<RP>).  The names are the instances', for
// mcmcx_debug_symsvd.
struct SvdPlan {
    void (*sweep32)(double *, mcx_d2 *, uint8_t *, int *, int, int) = nullptr;
    void (*sweep)(double *, mcx_d2 *, uint8_t *, int *, int, int, int) = nullptr; int svd_sb = 0;
    size_t sweep_lds = 0;
    void (*applyv)(double *, const mcx_d2 *, const uint8_t *, int, int) = nullptr; unsigned applyv_grid = 0; size_t applyv_lds = 0;
    const char *sweep_name = "", *applyv_name = "";
};
struct AdaptPlan {
    int n10 = 0, noff = 0; unsigned g8 = 0;            // the covariance's cover in blocks of TD: diagonal, off-diagonal, the grid's base
    // adapt_post_kernel<SVD, XG>: XG (npar > 320) keeps the work vector in global scratch and takes no LDS (slower; no limit)
    void (*post)(EngineDev, int, int, int, uint8_t *, int) = nullptr; size_t post_lds = 0;
    // KernelPlan::tile_factor: tile_factor_kernel<NC, NW> -- 4 NW neighbouring chains' packed matrices in LDS
    void (*factor)(EngineDev) = nullptr; unsigned factor_grid = 0, factor_block = 0; size_t factor_lds = 0;
    SvdPlan svd;                                       // KernelPlan::svd_blocked
    const char *post_name = "", *factor_name = "";     // the instances' names, for mcmcx_debug_calculate_R
};
// Which kernel forms the engine runs.  Decided ONCE, by plan_kernels at mcmcx_init (mcx_host_launch.hpp), from the configuration, the
// problem's shape, the target kind, the switches and the CU count -- never from what was allocated; mcmcx_init allocates as it says and
// every launcher reads it.
struct KernelPlan {
    int lds_form = LDS_NONE;
    bool dr_lds = false;                // delayed rejection's work vectors fit LDS (EngineDev::dr_lds)
    bool dr_vectors_in_lds = false;     // ... and its second stage keeps two vectors there (step_kernel_dr against step_kernel_dr_big)
    // lane-group step kernel (mcx_group.hpp): npar rounded up (0 = not this kernel), delayed-rejection mode, lanes per chain
    int group_d4 = 0, group_drm = 0, group_gw = 16;
    // method = 'ram' on group_ram_kernel (mcx_group_ram.hpp): npar rounded up to its instantiation, 0 = not
    int ram_group_d4 = 0;
    bool tile_factor = false;           // the adaptation's Cholesky branch through tile_factor_kernel (npar <= 64)
    bool svd_blocked = false;           // the adaptation's SVD one workgroup per chain (svd_blocked_kernel and its sweeps)
    bool cov_batch = true;              // the covariance's batch branch in blocks (adapt_covb_*) where it applies
    // pooled SCAM above npar 240 or with a user target: the shared rotation copied to every chain, the per-chain kernels / phases run
    bool scam_replicated = false;
    // host callbacks with few chains: the exchange vectors in page-locked host memory the device reads and writes directly (no copies
    // between the phases)
    bool host_mapped = false, cs_mapped = false;
    bool host_fuse = true;              // host callbacks: the next iteration's proposal rides in this iteration's last launch
    bool fused_cols = false;            // the response-column target's phases in one launch per segment (step_kernel_cols)
    bool pooled_mfma = false;           // pooled mode on the matrix cores (pooled_mfma_kernel and kin)
    bool pooled_dr_mfma = false;        // ... with delayed rejection: the dense R2 / iC tables (pooled_mfma_kernel<true>)
    bool pooled_two_waves = false, pooled_forty_rows = false;
    // pooled mode with the iteration cut at the user's evaluations (a target module, host callbacks): 0 = not, 1 = pooled_phase_kernel
    // (lane form), 2 = pooled_phase_mfma_kernel (the proposals on the matrix cores); SCAM runs the per-chain phases on the replicated
    // rotation
    int pooled_phase = 0;
    bool ram_wide = false;              // method = 'ram' above RAM_SMALL_MAX through step_kernel_ram_wide
    // ... whose update-only waves store the factor once per two iterations (ram_update_pair; [3 npar] more scratch doubles per chain)
    bool ram_pair = false;
    bool scam_pooled12 = false, scam_fast_tile = false; int scam_waves = 1;
    bool am = false;                    // the per-chain adaptation (not RAM, not pooled): covariance, mean and factor scratch per chain
    bool xscr = false;                  // the chains' global scratch vectors (EngineDev::xscr): pooled DR, or npar > 320
    unsigned shared = 0;                // pooled mode: the SharedLayout bits the chosen entry reads, all pooled_alloc allocates
    const KernelEntry *step = nullptr;  // what launch_step runs: a GROUP_TABLE entry when group_d4, a STEP_TABLE one otherwise
    const KernelEntry *scam = nullptr;  // what launch_scam runs
    AdaptPlan adapt;                    // what launch_adapt runs
};
// Pooled mode (one proposal factor for all chains): the host masters the ticks compute (mcx_host_pooled.hpp) and the device layouts
// pooled_upload writes from them.  Packed = the upper triangle (h_pidx); dense = M[s*d + o] = A(o, s) for the matrix A applied to z (R' of a
// Cholesky factor, a full factor itself), npar rounded up to four rows, pad rows and PWS slack zero (dense_layout).
struct PooledState {
    int status = 0; double alpha = 0.0;                  // pooled RAM: skipped ticks, mean acceptance of the last tick
    double W = 0.0; std::vector<double> mean, C, R;      // chainwsum, chainmean, chaincmat (packed), the Cholesky factor (packed)
    std::vector<double> Rf;                              // condmax > 0: covtor_svd's full factor U sqrt(s) 2.4/sqrt(d), column-major
    std::vector<double> U, std;                          // SCAM: the shared rotation (column-major) and qcovstd
    std::vector<double> R2, iC;                          // delayed rejection: factor / drscale (stored like the factor), dpotri(R) packed
    double *d_R = nullptr;                               // SH_R: R packed -- the lane kernels' E.sharedR, step_kernel_cols
    double *d_RT = nullptr;                              // SH_RT: R or Rf dense -- pooled_mfma*_kernel; Rf: the lane kernels' E.sharedR
    double *d_R2 = nullptr, *d_iC = nullptr;             // SH_DR: R2 (packed; Rf / drscale dense), iC packed -- *_pooled_dr*, _cols
    double *d_R2T = nullptr, *d_iCd = nullptr;           // SH_DRT: R2 dense, iC dense and symmetric -- pooled_mfma_kernel<true>
    double *d_U = nullptr;                               // SH_U: [U col-major | pad | U row-major | pad | std] -- scam_pooled[12]_kernel
};                                                       // (SH_UREP: U and std copied to every chain's E.Rf / E.qstd -- npar > 240)
// The thinned sample store (mcmcx_set_samples): iteration i is kept when i >= first and (i - first) % thin == 0 (thin = 0: off), in slot
// (number kept before it) % capacity of the ring `store`, [capacity][ntiles][nfields][64] doubles (mcx_samples.hpp)
struct SamplePlan { int first = 1, thin = 0, capacity = 0; long long kept = 0; double *store = nullptr; };
struct mcmcx_engine {
    mcmcx_config cfg;
    KernelPlan plan;
    SamplePlan samp;
    int d = 0, P = 0, ntiles = 0, nlanes = 0;
    int dodr = 0, usesvd = 0;
    bool inited = false;
    int simuind = 0;
    // name of the sampling kernel launch_step / launch_scam ran last, or of pooled mode's phase form (mcmcx_last_kernel)
    const char *last_kernel = "";
    // ... and, where an entry stands for several template instances (the group kernels), the instance(s) it launched, joined by '+'
    // (mcmcx_debug_last_instance); nullptr: the entry's own name
    const char *last_instance = nullptr;
    std::string launch_err;             // set by a launcher that found no kernel for the configuration: the run fails with it
    // host copies of the problem
    std::vector<double> par0, cmat0;                 // cmat0 col-major d*d
    // per-chain start points: 0 all chains at par0, 1 given (start_all, [nchains][npar] row-major), 2 drawn on the device at
    // mcmcx_init (start_scale); after init, the chains that made more than one attempt and those that fell back to par0
    int start_mode = 0; std::vector<double> start_all; double start_scale = 0.0; long long start_redrew = 0, start_fell = 0;
    double sigma2 = 1.0; int nobs = 1; bool sigma2ok = false;
    int ny = 1; std::vector<double> sigma2v; std::vector<int> nobsv;      // nycol columns (host callbacks only when > 1)
    int tkind = -1, tncols = 1; std::vector<double> tmu, tlam, tx, ty, tlo, thi, tpmu, tpsig; double tb = 0.1;
    // a data set per chain (mcmcx_set_target_expdata_all): 0 one data set for all chains, 1 y per chain, 2 x and y per chain; the call's
    // copies y_all [nchains][tncols][ndata] and (mode 2) x_all [nchains][ndata] until init_chain_data has filled the device tables
    int cdata_mode = 0, cdata_n = 0; std::vector<double> ty_all, tx_all; long long cdata_bytes = 0;
    bool has_lo = false, has_hi = false, has_pri = false;
    mcmcx_ssfun_t h_ss = nullptr; mcmcx_ssfun_er_t h_ss_er = nullptr; mcmcx_priorfun_t h_pri = nullptr; mcmcx_checkbounds_t h_cb = nullptr;
        void *h_user = nullptr;
    mcmcx_ssfun_batch_t h_ss_batch = nullptr; int h_threads = 1;      // batched form of the user's ssfunction (opt-in)
    int mod_max_ny = 8;
    hipModule_t mod = nullptr; hipFunction_t mod_fn = nullptr; void *d_moddata = nullptr;   // user target module (include/mcmcx_target.h)
    std::vector<double> h_bth, h_bss; std::vector<int> h_bidx;
    // host side of the callback path: page-locked, so that the candidates come back and the results go out as asynchronous copies
    // on the engine's stream with ONE synchronisation per stage (pageable buffers cost a staged, blocking copy each way)
    struct Pinned {
        double *p = nullptr; size_t cap = 0, n = 0;
        int resize(size_t m) {
            n = m;
            if (m <= cap) return 0;
            if (p) (void)hipHostFree(p);
            p = nullptr; cap = 0;
            if (hipHostMalloc((void **)&p, m * sizeof(double), hipHostMallocDefault) != hipSuccess) return -1;
            cap = m; return 0;
        }
        double &operator[](size_t i) { return p[i]; }
        double *data() { return p; }
        size_t size() const { return n; }
        void release() { if (p) (void)hipHostFree(p); p = nullptr; cap = n = 0; }
    } h_cand, h_ev, h_hx;
    int pooled = 0; PooledState pool;                 // pooled mode
    // host callbacks: the next iteration's proposal already ran in the previous iteration's last launch
    bool p0_done = false;
    // a host-callback iteration failed half way: the chains' stream positions are undefined, later runs are refused
    bool failed = false;
    std::vector<void *> hallocs;
    mcmcx_exchange_t xfn = nullptr; void *xuser = nullptr; double *xbuf = nullptr;
    struct mcmcx_comm *comm = nullptr;                // the node's communicator (mcx_comm.hpp); nullptr = this GPU alone
    // [nranks][len + 1] per-rank moment vectors (+ the rank's stop flag), [len + 1] their tree sum
    double *d_gather = nullptr, *d_pooled = nullptr;
    double h_flag = 0.0;                              // this rank's stop flag of the exchange being enqueued (1 = a caught signal)
    bool run_entered = false;                         // mcmcx_run is past its argument checks (a failure from here on may strand peers)
    // the summed stop flag of the tick just applied was non-zero: every rank leaves after this tick
    bool stop_seen = false;
    double S02eff = 0.0;
    // device
    hipStream_t stream = nullptr; bool own_stream = false;
    EngineDev E{};
    std::vector<void *> allocs;
    double *d_ramscale = nullptr, *d_moments = nullptr;
    double *d_pair = nullptr;           // KernelPlan::ram_pair: [3 npar] scratch doubles per chain (step_kernel_ram_wide's pair_scr)
    void *d_scratch = nullptr; size_t scratch_cap = 0;  // the sample store's readers' scratch, in bytes (samples_scratch): grows only
    // blocked SVD of the adaptation (large npar)
    double *d_Gc = nullptr, *d_Vc = nullptr, *d_svc = nullptr; uint8_t *d_need = nullptr, *d_state = nullptr; int *d_anyrot = nullptr;
    int wcap = 0;
    // lane-group kernels: the factors were rewritten since the last range check (DR2), its flag, the accept bytes of a launch
    bool group_check_due = true; int *d_gflag = nullptr; uint8_t *d_accb = nullptr;
    // MCMC_run1: the caller evaluates; exchange vectors of run1_kernel
    bool external = false; double *d_r1 = nullptr; std::vector<double> h_r1;
    // timing of the step kernel
    std::vector<std::pair<hipEvent_t, hipEvent_t>> pending;
    double ms_total = 0.0; long long launches = 0, steps = 0;
};

struct DevBufs {                                       // hipFree on every exit path
    std::vector<void *> p;
    template <typename T> hipError_t alloc(T **q, size_t bytes) { void *v = nullptr; hipError_t e = hipMalloc(&v, bytes);
        if (e == hipSuccess) p.push_back(v); *q = (T *)v; return e; }
    ~DevBufs() { for (void *v : p) (void)hipFree(v); }
};

template <typename T>
static int dev_alloc(mcmcx_engine *h, T **p, size_t n, bool zero = true)
{
    void *q = nullptr;
    size_t bytes = std::max<size_t>(n, 1) * sizeof(T);
    hipError_t e = hipMalloc(&q, bytes);
    if (e != hipSuccess) return fail(-101, "hipMalloc of " + std::to_string(bytes) + " bytes: " + hipGetErrorString(e));
    if (zero) { e = hipMemsetAsync(q, 0, bytes, h->stream); if (e != hipSuccess) return fail(-101, hipGetErrorString(e)); }
    h->allocs.push_back(q);
    *p = (T *)q;
    return 0;
}

// page-locked host memory mapped into the device's address space (the same pointer on both sides)
template <typename T>
static int host_alloc(mcmcx_engine *h, T **p, size_t n)
{
    void *q = nullptr;
    size_t bytes = std::max<size_t>(n, 1) * sizeof(T);
    hipError_t e = hipHostMalloc(&q, bytes, hipHostMallocMapped | hipHostMallocCoherent);
    if (e != hipSuccess) return fail(-101, "hipHostMalloc of " + std::to_string(bytes) + " bytes: " + hipGetErrorString(e));
    memset(q, 0, bytes);
    h->hallocs.push_back(q);
    *p = (T *)q;
    return 0;
}

template <typename T>
static int dev_upload(mcmcx_engine *h, const T **p, const std::vector<T> &v)
{
    T *q = nullptr;
    int rc = dev_alloc(h, &q, v.size(), false);
    if (rc) return rc;
    if (!v.empty()) {
        hipError_t e = hipMemcpy(q, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice);
        if (e != hipSuccess) return fail(-102, hipGetErrorString(e));
    }
    *p = q;
    return 0;
}

// No limit on npar like the reference (MCMC_init.F90:81-102 allocates whatever the namelist says) -- beyond int-sized packed indices.  Up
// to 256 every kernel family applies; above, the forms that keep an npar-vector per lane in LDS give way to global scratch where the 160
// KiB end (delayed rejection > 160, the adaptation's work vector > 320, the pooled-moment kernel from 316 on), the blocked SVD to the
// lane-per-chain SVD (> 256), the matrix-core pooled kernels to the lane kernels (their own LDS tests): slower, never refused. response
// columns (mcmc.F90:30-33: whatever mcmcnycol.dat says): every per-column array is sized at mcmcx_init
static const int MCX_MAX_NYCOL = 4096;
// P = npar (npar + 1) / 2 = 8 390 656 at the cap, 64 P = 537 M and (2 npar + P) 64 = 538 M: every int-typed index expression of the device
// code (pidx, rowstart, e * 64 + lane) stays below 2**31 with a factor of four to spare -- at 8192, the cap up to round 5, 64 P is 2.147e9
// > INT_MAX and only the size_t casts of every current use site kept it correct.  Larger problems are refused loudly at
// mcmcx_create.
static const int MCX_MAX_NPAR = 4096;
