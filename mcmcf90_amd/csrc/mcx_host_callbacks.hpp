// mcx_host_callbacks.hpp -- the iteration cut at the user's evaluations: host_eval (the user's host ssfunction / priorfun / checkbounds, a
// target module's kernel or the response-column target between the phase kernels), launch_phase (which kernel carries a phase, per chain or
// in pooled mode's two forms) and host_iteration, the one statement of the protocol; MCMC_run1's exchange vectors.
// Part of the ONE translation unit mcx_api.hip (included there, in this order: mcx_host_engine, mcx_host_linalg, mcx_host_launch,
// mcx_host_adapt, mcx_host_pooled, mcx_host_callbacks); not a stand-alone header.

// Host-callback evaluation of one candidate vector per chain, in chain order, from the calling thread
// (the reference's callbacks keep SAVEd state and are not thread-safe: testcases/mcmcrun.F90:69-70).
// src: tile-interleaved device vector [T][stride][64]; only chains with want != 0 (hx slot) are evaluated.
// what: 0 = checkbounds, priorfun, ssfunction (MCMC_run.F90:47-56); 1 = checkbounds and priorfun only, 2 = ssfunction_er
// with each chain's threshold (the two halves of an early-rejection iteration, MCMC_run_er.F90:54-76)
static int host_eval(mcmcx_engine *h, const double *dev_src, int stride_k, bool use_stage2_flag, int what = 0)
{
    const int d = h->d, T = h->ntiles;
    if (h->tkind == TGT_EXPCOLS) {                      // device-resident response-column target: no host round trip
        const int s2 = use_stage2_flag ? 1 : 0;
        if (h->cdata_mode) hipLaunchKernelGGL(dev_eval_kernel<true>, dim3(T), dim3(64), 0, h->stream, h->E, dev_src, stride_k, s2, what);
        else hipLaunchKernelGGL(dev_eval_kernel, dim3(T), dim3(64), 0, h->stream, h->E, dev_src, stride_k, s2, what);
        HIPCHK(hipGetLastError());
        return 0;
    }
    if (h->tkind == TGT_MODULE) {                       // the user's own device code, loaded from a code object
        mcmcx_target_args a;
        a.src = dev_src; a.hev = h->E.hev; a.hx = h->E.hx; a.userdata = h->d_moddata;
        a.stride_k = stride_k; a.npar = d; a.ny = h->ny; a.nhe = NHE - 1 + h->ny; a.nhx = NHX; a.nchains = h->cfg.nchains;
        a.use_stage2 = use_stage2_flag ? 1 : 0; a.what = what;
        size_t asz = sizeof(a);
        void *cfgv[] = {HIP_LAUNCH_PARAM_BUFFER_POINTER, &a, HIP_LAUNCH_PARAM_BUFFER_SIZE, &asz, HIP_LAUNCH_PARAM_END};
        HIPCHK(hipModuleLaunchKernel(h->mod_fn, (unsigned)T, 1, 1, 64, 1, 1, 0, h->stream, nullptr, cfgv));
        return 0;
    }
    const size_t L = (size_t)T * 64;
    const int ny = h->ny, nhe = NHE - 1 + ny;
    const bool src_mapped = h->plan.host_mapped && (dev_src == h->E.cand || h->plan.cs_mapped);
    const bool mapped = h->plan.host_mapped;                 // flags and results in place
    if ((!src_mapped && h->h_cand.resize(L * stride_k)) || (!mapped && (h->h_ev.resize(L * nhe) || (use_stage2_flag
        && h->h_hx.resize(L * NHX)))))
        return fail(-100, "host callbacks: no page-locked memory for the candidates");
    std::vector<double> ssc(ny, 0.0);
    if (!src_mapped) HIPCHK(hipMemcpyAsync(h->h_cand.data(), dev_src, L * stride_k * 8, hipMemcpyDeviceToHost, h->stream));
    if (use_stage2_flag && !mapped) HIPCHK(hipMemcpyAsync(h->h_hx.data(), h->E.hx, h->h_hx.size() * 8, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));             // (also: the previous stage's results have left h_ev)
    const double *h_cand = src_mapped ? dev_src : h->h_cand.data();
    const double *hx = mapped ? h->E.hx : h->h_hx.data();
    double *h_ev = mapped ? h->E.hev : h->h_ev.data();
    memset(h_ev, 0, L * nhe * sizeof(double));
    std::vector<double> th(d);
    // The chains in order, on this thread: bounds, then the prior where in bounds (MCMC_run.F90:54-56: prior first), then the sum of
    // squares where it is needed -- at once, or queued for the user's ssfunction_batch (opt-in; ssfunction_er keeps the per-chain call)
    const bool batch = h->h_ss_batch && !(what == 2 && h->h_ss_er);
    if (batch) { h->h_bidx.clear(); h->h_bth.clear(); }
    for (int c = 0; c < h->cfg.nchains; ++c) {
        const int t = c / 64, l = c % 64;
        if (use_stage2_flag && hx[((size_t)t * NHX + HX_STAGE2) * 64 + l] == 0.0) continue;
        for (int k = 0; k < d; ++k) th[k] = h_cand[((size_t)t * stride_k + k) * 64 + l];
        int inb = 1;
        double pri = 0.0;
        if (what != 2) {
            inb = h->h_cb ? h->h_cb(th.data(), d, h->h_user) : 1;                    // checkbounds0.f90: .true.
            if (inb) pri = h->h_pri ? h->h_pri(th.data(), d, h->h_user) : 0.0;
        }
        h_ev[((size_t)t * nhe + HE_INB) * 64 + l] = inb ? 1.0 : 0.0;
        h_ev[((size_t)t * nhe + HE_PRI) * 64 + l] = pri;
        if (what == 1 || !inb) continue;                                             // (no sum of squares: its slots stay zero)
        if (batch) { h->h_bidx.push_back(c); h->h_bth.insert(h->h_bth.end(), th.begin(), th.end()); continue; }
        std::fill(ssc.begin(), ssc.end(), 0.0);
        if (what == 2 && h->h_ss_er)                                                 // MCMC_ssfunction_er(newpar, sscrit)
            h->h_ss_er(th.data(), d, ny, hx[((size_t)t * NHX + HX_CRIT) * 64 + l], ssc.data(), h->h_user);
        else h->h_ss(th.data(), d, ny, ssc.data(), h->h_user);                       // (ssfunction_er0.f90: no er for ss)
        for (int j = 0; j < ny; ++j) h_ev[((size_t)t * nhe + HE_SS + j) * 64 + l] = ssc[j];
    }
    if (batch) {                                         // ONE call of ssfunction_batch per worker thread over the queued chains
        const int n = (int)h->h_bidx.size();
        h->h_bss.assign((size_t)n * ny, 0.0);
        // the first evaluation (MCMC_init's starting point) stays on the calling thread: user code commonly loads its
        // data on first call (testcases/mcmcrun.F90:69-70) -- after that concurrent calls only read it
        const int nt = h->inited ? std::max(1, std::min(h->h_threads, n)) : 1;
        if (nt <= 1) { if (n > 0) h->h_ss_batch(h->h_bth.data(), d, n, ny, h->h_bss.data(), h->h_user); }
        else {
            std::vector<std::thread> pool;
            for (int w = 0; w < nt; ++w) {
                const int lo = (int)((long long)n * w / nt), hi = (int)((long long)n * (w + 1) / nt);
                if (hi > lo) pool.emplace_back([=]() { h->h_ss_batch(h->h_bth.data() + (size_t)lo * d, d, hi - lo, ny,
                    h->h_bss.data() + (size_t)lo * ny, h->h_user); });
            }
            for (auto &t : pool) t.join();
        }
        for (int i = 0; i < n; ++i) {
            const int c = h->h_bidx[i], t = c / 64, l = c % 64;
            for (int j = 0; j < ny; ++j) h_ev[((size_t)t * nhe + HE_SS + j) * 64 + l] = h->h_bss[(size_t)i * ny + j];
        }
    }
    if (!mapped) HIPCHK(hipMemcpyAsync(h->E.hev, h->h_ev.data(), h->h_ev.size() * 8, hipMemcpyHostToDevice, h->stream));
    return 0;
}

// ---- the phase launches.  An iteration cut at the evaluations runs as phases: 0 the proposal, 1 the first stage's decision (with delayed
// rejection: and the second stage's proposal), 2 the second stage's decision, 3 early rejection's threshold, 4 its decision; SCAM: 5 a
// component's proposal, 6 its decision, 7 the iteration's end.  Which kernel carries a phase is the plan's business: the per-chain
// host_phase_kernel / host_phase_seq_kernel, or in pooled mode (KernelPlan::pooled_phase, the shared tables in PooledState's layouts)
// pooled_phase_kernel / pooled_phase_mfma_kernel.  launch_phase and launch_scam_phase are the only code that knows their argument lists;
// both leave h->p0_done saying whether iteration it + 1's proposal rode along, and report the launch's error.
template <int PA, int PB>
static void launch_pooled_lane(mcmcx_engine *h, int itA)
{
    hipLaunchKernelGGL((pooled_phase_kernel<PA, PB>), dim3(h->ntiles), dim3(64), PA == 2 ? lds_step(h) : 0, h->stream, h->E, itA, itA + 1,
        (const double *)h->d_ramscale, (const double *)h->E.sharedR, (const double *)h->pool.d_R2, (const double *)h->pool.d_iC);
}
// PA < 0: iteration itB's proposal alone
template <int PA, bool STAGE2>
static void launch_pooled_mfma(mcmcx_engine *h, int itA, int itB)
{
    const size_t lds = pooled_phase_mfma_lds(h->d, PA == 2 && h->plan.dr_lds);
    hipLaunchKernelGGL((pooled_phase_mfma_kernel<PA, STAGE2>), dim3(h->ntiles), dim3(64), lds, h->stream, h->E, itA, itB,
        (const double *)h->d_ramscale, (const double *)(STAGE2 ? h->pool.d_R2T : h->pool.d_RT), (const double *)h->pool.d_iC,
        h->cfg.method == MCMCX_METHOD_RAM ? 1 : 0);
}
// Phase P (0 .. 4) of iteration it; next: iteration it + 1's proposal behind it in the same launch (P an iteration's last phase: 1, 2, 4).
// The matrix-core form carries the launches with a proposal in them -- with delayed rejection phase 1's second-stage proposal too --
// and leaves the others to the lane form; the per-chain kernels take the step size at ramscale + it, the others the table's base.
template <int P>
static int launch_phase(mcmcx_engine *h, int it, bool next = false)
{
    constexpr bool LAST = P == 1 || P == 2 || P == 4;
    const dim3 g(h->ntiles), b(64);
    const size_t lds = P == 2 ? lds_step(h) : 0;
    const double *rs0 = h->d_ramscale;
    const int form = h->plan.pooled_phase;
    h->p0_done = LAST && next;
    if (h->p0_done) {
        if constexpr (LAST) {
            if (form == 0) hipLaunchKernelGGL((host_phase_seq_kernel<P, 0, -1>), g, b, lds, h->stream, h->E, it, 0, it + 1, 0, 0, 0, rs0);
            else if (form == 2) launch_pooled_mfma<P, false>(h, it, it + 1);
            else launch_pooled_lane<P, 0>(h, it);
        }
    }
    else if (form == 0) hipLaunchKernelGGL((host_phase_kernel<P>), g, b, lds, h->stream, h->E, it, rs0 + it, 0);
    else if (form == 2 && P == 0) launch_pooled_mfma<-1, false>(h, it, it);
    else if (form == 2 && P == 1 && h->dodr) launch_pooled_mfma<1, true>(h, it, it);
    else launch_pooled_lane<P, -1>(h, it);
    HIPCHK(hipGetLastError());
    return 0;
}
// SCAM's phases of component j, on the per-chain kernels (pooled mode: on every chain's copy of the shared rotation).  A decision (6)
// carries what no evaluation separates from it: PB = 5 the next component's proposal, PB = 7 the iteration's end and, PC = 5, iteration
// it + 1's first proposal -- in one launch, or with MCMCX_HOST_FUSE=0 one launch per phase
template <int PA, int PB = -1, int PC = -1>
static int launch_scam_phase(mcmcx_engine *h, int it, int j)
{
    const dim3 g(h->ntiles), b(64);
    const double *rs0 = h->d_ramscale;
    const int auxB = PB == 5 ? j + 1 : 0;
    h->p0_done = false;
    if constexpr (PB >= 0) if (h->plan.host_fuse) {
        hipLaunchKernelGGL((host_phase_seq_kernel<PA, PB, PC>), g, b, 0, h->stream, h->E, it, j, it, auxB, PC >= 0 ? it + 1 : 0, 0, rs0);
        h->p0_done = PC >= 0;
        HIPCHK(hipGetLastError());
        return 0;
    }
    hipLaunchKernelGGL((host_phase_kernel<PA>), g, b, 0, h->stream, h->E, it, rs0 + it, j);
    HIPCHK(hipGetLastError());
    if constexpr (PB >= 0) { hipLaunchKernelGGL((host_phase_kernel<PB>), g, b, 0, h->stream, h->E, it, rs0 + it, auxB);
        HIPCHK(hipGetLastError()); }
    return 0;
}

// One iteration of MCMC_run / MCMC_run_er / MCMC_run_scam with the user's evaluations between the phases, in every form of the plan.
// fuse_next: iteration it + 1 follows without a tick in between -- its proposal rides in this iteration's last launch, and h->p0_done
// tells the next call so (MCMCX_HOST_FUSE=0: one launch per phase, the A/B form the tests compare with)
static int host_iteration(mcmcx_engine *h, int it, bool fuse_next)
{
    const int d = h->d;
    const bool p0_done = h->p0_done;
    int rc;
    fuse_next = fuse_next && h->plan.host_fuse;
    if (h->pooled) h->last_kernel = (h->plan.pooled_phase ? h->plan.step : h->plan.scam)->name;
    if (h->cfg.method == MCMCX_METHOD_SCAM) {           // MCMC_run_scam: npar componentwise proposals, each evaluated by the user
        for (int j = 0; j < d; ++j) {
            if (j == 0 && !p0_done && (rc = launch_scam_phase<5>(h, it, 0))) return rc;
            if ((rc = host_eval(h, h->E.cand, d, false))) return rc;
            rc = j + 1 < d ? launch_scam_phase<6, 5>(h, it, j) : fuse_next ? launch_scam_phase<6, 7, 5>(h, it, j)
                : launch_scam_phase<6, 7>(h, it, j);
            if (rc) return rc;
        }
        return 0;
    }
    if (!p0_done && (rc = launch_phase<0>(h, it))) return rc;
    if (h->cfg.method == MCMCX_METHOD_ER) {             // MCMC_run_er: the threshold is drawn between priorfun and ssfunction_er
        if ((rc = host_eval(h, h->E.cand, d, false, 1)) || (rc = launch_phase<3>(h, it)) || (rc = host_eval(h, h->E.cand, d, true, 2)))
            return rc;
        return launch_phase<4>(h, it, fuse_next);
    }
    if ((rc = host_eval(h, h->E.cand, d, false))) return rc;
    if (!h->dodr) return launch_phase<1>(h, it, fuse_next);
    if ((rc = launch_phase<1>(h, it)) || (rc = host_eval(h, h->E.cs, 2 * d, true))) return rc;
    return launch_phase<2>(h, it, fuse_next);
}

// ---- MCMC_run1 / MCMC_run1_er: the arithmetic of one invocation (run1_kernel), all chains at once, vectors row-major per chain
static int run1_check(mcmcx_engine *h)
{
    if (!h) return fail(-1, "null handle");
    if (!h->inited) return fail(-40, "we have not inited");                           // MCMC_run1.F90:55
    if (!h->external) return
        fail(-42, "mcmcx_run1_*: needs mcmcx_set_target_external (the caller evaluates ssfunction / priorfun / checkbounds)");
    return 0;
}
static void run1_put(mcmcx_engine *h, int slot0, int K, const double *src /* [nchains][K] or nullptr */)
{
    const int n1 = 3 * h->d + 3 * h->ny + NR1;
    for (int c = 0; c < h->cfg.nchains; ++c) {
        const int t = c / 64, l = c % 64;
        for (int k = 0; k < K; ++k) h->h_r1[((size_t)t * n1 + slot0 + k) * 64 + l] = src ? src[(size_t)c * K + k] : 0.0;
    }
}
static void run1_get(mcmcx_engine *h, int slot0, int K, double *dst)
{
    const int n1 = 3 * h->d + 3 * h->ny + NR1;
    for (int c = 0; c < h->cfg.nchains; ++c) {
        const int t = c / 64, l = c % 64;
        for (int k = 0; k < K; ++k) dst[(size_t)c * K + k] = h->h_r1[((size_t)t * n1 + slot0 + k) * 64 + l];
    }
}
template <int MODE>
static int run1_launch(mcmcx_engine *h, int drstage)
{
    HIPCHK(hipSetDevice(h->cfg.device));
    HIPCHK(hipMemcpyAsync(h->d_r1, h->h_r1.data(), h->h_r1.size() * 8, hipMemcpyHostToDevice, h->stream));
    hipLaunchKernelGGL((run1_kernel<MODE>), dim3(h->ntiles), dim3(64), MODE == 0 ? lds_step(h) : 0, h->stream, h->E, h->d_r1, drstage);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(h->h_r1.data(), h->d_r1, h->h_r1.size() * 8, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    return 0;
}
