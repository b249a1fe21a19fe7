// mcx_host_adapt.hpp -- the adaptation tick's launch sequence (MCMC_adapt.F90:12-230) and its schedule.
// Part of the ONE translation unit mcx_api.hip (included there, in this order: mcx_host_engine, mcx_host_linalg, mcx_host_launch,
// mcx_host_adapt, mcx_host_pooled, mcx_host_callbacks); not a stand-alone header.

// The blocked SVD's launch sequence (mcx_svd.hpp) on chain-major arrays, in plain arguments: launch_adapt runs it on the engine's buffers,
// mcmcx_debug_symsvd on a caller's matrices -- one statement of the sweep loop, its stop and the forms the plan names.  Gc: in the
// matrices, out the sorted singular vectors; Vc, rot (the rotation log, d (d - 1) / 2 entries per chain), state, anyrot: scratch; svc: out
// the singular values.  sweeps (host, [nlanes], may be null; tests): += 1 for every sweep a chain rotated in -- what the routine returns
// (oracle/mcx_svd.h) -- read from `state` after each sweep, where 1 means "rotated in the sweep just run".
static void launch_svd(const SvdPlan &a, hipStream_t stream, double *Gc, double *Vc, double *svc, mcx_d2 *rot, uint8_t *state,
                       const uint8_t *need, int *anyrot, int nlanes, int d, int32_t *sweeps = nullptr)
{
    const dim3 L(nlanes), b64(64), b256(256);
    std::vector<uint8_t> st(sweeps ? (size_t)nlanes : 0);
    hipLaunchKernelGGL(svd_init_kernel, L, b256, 0, stream, Vc, state, need, nlanes, d);
    for (int sweep = 0; sweep < 60; ++sweep) {
        (void)hipMemsetAsync(anyrot, 0, sizeof(int), stream);
        // the sweep: every later column streamed past a block's pair-lanes through an LDS ring (mcx_svd.hpp); then the log replayed on V
        if (!a.sweep32) hipLaunchKernelGGL(a.sweep, L, b256, a.sweep_lds, stream, Gc, rot, state, anyrot, nlanes, d, a.svd_sb);
        else if (!MCX_VARIANT_SVD_SWEEP(stream, Gc, rot, state, anyrot, nlanes, d, a.sweep_lds)) hipLaunchKernelGGL(a.sweep32, L, b256,
            a.sweep_lds, stream, Gc, rot, state, anyrot, nlanes, d);
        hipLaunchKernelGGL(a.applyv, dim3(a.applyv_grid), b64, a.applyv_lds, stream, Vc, (const mcx_d2 *)rot, state, nlanes, d);
        int any = 0;
        // (reported by the caller's hipGetLastError)
        if (hipMemcpyAsync(&any, anyrot, sizeof(int), hipMemcpyDeviceToHost, stream) != hipSuccess
            || (sweeps && hipMemcpyAsync(st.data(), state, (size_t)nlanes, hipMemcpyDeviceToHost, stream) != hipSuccess)
            || hipStreamSynchronize(stream) != hipSuccess) break;
        if (sweeps) for (int c = 0; c < nlanes; ++c) sweeps[c] += st[c] == 1;
        if (!any) break;
    }
    hipLaunchKernelGGL(svd_finish_kernel, L, b256, 0, stream, Gc, Vc, svc, state, nlanes, d);
}

// The factorisation's launches (MCMC_calculate_R for the chains with ADF_DOCALC, and with mode != 0 the covariance's bookkeeping in the
// same kernel): the tail of the tick, and all of mcmcx_debug_calculate_R (mode 0: the bookkeeping rewrites what it read) -- one statement
// of the instance choice, the grids and the LDS sizes the plan names.
static void launch_factor(mcmcx_engine *h, int it, int mode, int batch_done)
{
    const AdaptPlan &a = h->plan.adapt;
    const dim3 T(h->ntiles), b64(64), b256(256);
    if (!h->plan.svd_blocked) {
        // the whole rest of the tick in adapt_post_kernel (phase 0) -- or, with tile_factor, its covariance bookkeeping (phase 3) and
        // dpotf2 (+ dtrti2 / dlauu2 with delayed rejection) on the packed matrices in LDS, read and written once (mcx_group.hpp)
        hipLaunchKernelGGL(a.post, T, b64, a.post_lds, h->stream, h->E, it, mode, a.factor ? 3 : 0, (uint8_t *)nullptr, batch_done);
        if (a.factor) hipLaunchKernelGGL(a.factor, dim3(a.factor_grid), dim3(a.factor_block), a.factor_lds, h->stream, h->E);
        return;
    }
    // large npar with an SVD factor: the factorisation runs one workgroup per chain on chain-major copies, one launch
    // pair per Jacobi sweep (the rotation log lives in Gw, which is free between tile2chain and the next tick)
    const size_t DD = (size_t)h->d * h->d;
    const dim3 tg((unsigned)((DD + 63) / 64), (unsigned)h->ntiles), tg1((unsigned)((h->d + 63) / 64), (unsigned)h->ntiles);
    hipLaunchKernelGGL(a.post, T, b64, a.post_lds, h->stream, h->E, it, mode, 1, h->d_need, batch_done);
    hipLaunchKernelGGL(tile2chain_kernel, tg, b256, 0, h->stream, h->E.Gw, h->d_Gc, DD, DD, h->d_need);
    launch_svd(a.svd, h->stream, h->d_Gc, h->d_Vc, h->d_svc, (mcx_d2 *)h->E.Gw, h->d_state, h->d_need, h->d_anyrot, h->nlanes, h->d);
    hipLaunchKernelGGL(chain2tile_kernel, tg, b256, 0, h->stream, h->d_Gc, h->E.Vw, DD, DD, h->d_need);
    hipLaunchKernelGGL(chain2tile_kernel, tg1, b256, 0, h->stream, h->d_svc, h->E.cs, (size_t)h->d, (size_t)2 * h->d, h->d_need);
    hipLaunchKernelGGL(a.post, T, b64, a.post_lds, h->stream, h->E, it, mode, 2, h->d_need, batch_done);
}

// Reads the plan (KernelPlan::adapt: the geometry and the kernel instantiations, chosen at mcmcx_init), it and mode -- nothing is
// decided here but what the tick's mode decides.
static void launch_adapt(mcmcx_engine *h, int it, int mode)
{
    const AdaptPlan &a = h->plan.adapt;
    const dim3 T(h->ntiles), b64(64);
    // the AP window (a batch recompute at every adaptation: no blocked update)
    const bool ap = (mode & AD_AM) && h->cfg.adapthist > 1;
    // covmat's batch branch in blocks (adapt_covb_*): the AP window; with initcmatn = 0 the first AM adaptation and the greedy restarts.
    // Which lanes take it is the lanes' own business (ADF_BATCH); a tick that cannot hold any skips the launches.
    const int batch_done = (h->plan.cov_batch &&
                            (ap || (h->cfg.initcmatn == 0 && ((mode & AD_FIRST) || ((mode & AD_BURN) && h->cfg.greedy != 0))))) ? 1 : 0;
    hipLaunchKernelGGL(adapt_pre_kernel, T, b64, 0, h->stream, h->E, it, mode);
    if (batch_done) {
        hipLaunchKernelGGL(adapt_covb_diag_kernel, dim3(a.g8 * a.n10), b64, 0, h->stream, h->E, it, a.n10);
        if (a.noff > 0) hipLaunchKernelGGL(adapt_covb_off_kernel, dim3(a.g8 * a.noff), b64, 0, h->stream, h->E, it, a.noff);
    }
    if (!ap && !MCX_VARIANT_COV(h, a.g8, a.n10, a.noff, it, mode)) {
        hipLaunchKernelGGL(adapt_cov_diag_kernel, dim3(a.g8 * a.n10), b64, 0, h->stream, h->E, it, mode, a.n10);
        if (a.noff > 0) hipLaunchKernelGGL(adapt_cov_off_kernel, dim3(a.g8 * a.noff), b64, 0, h->stream, h->E, it, mode, a.noff);
    }
    launch_factor(h, it, mode, batch_done);
}

// Which branch of MCMC_adapt fires at iteration `it` (0 = none).  MCMC_adapt.F90:42-46, 60-61, 105.
static int adapt_mode(const mcmcx_config &c, int it)
{
    if (c.method == MCMCX_METHOD_RAM) return 0;
    if (c.doadapt == 0 && c.doburnin == 0) return 0;
    if (c.adaptend > 0 && it > c.adaptend) return 0;
    bool m1 = (c.adaptint != 0) && (it % c.adaptint == 0);
    bool m2 = (c.badaptint != 0) && (it % c.badaptint == 0);
    if (!m1 && !m2) return 0;
    if (it < c.burnintime && c.doburnin != 0 && m2) return AD_BURN;
    if (it >= c.burnintime + c.adaptint + c.adapthist && c.doadapt != 0)
        return AD_AM | ((it == c.burnintime + c.adaptint + c.adapthist) ? AD_FIRST : 0);
    return 0;
}

// pooled RAM: every adaptint iterations once the burn-in is over (MCMC_run_ram.F90:123-131), up to adaptend
static bool pooled_ram_due(const mcmcx_engine *h, int it)
{
    const mcmcx_config &c = h->cfg;
    if (!h->pooled || c.method != MCMCX_METHOD_RAM || c.doadapt == 0 || c.adaptint <= 0) return false;
    if (it < c.burnintime && c.doburnin != 0) return false;
    if (c.adaptend > 0 && it > c.adaptend) return false;
    return it % c.adaptint == 0;
}
