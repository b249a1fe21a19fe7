// mcx_host_diag.hpp -- the sample store's convergence summary, host side (mcmcx_samples_stats / _dev / _diag): the window checks, the tile
// scratch, the launches of mcx_diag.hpp's kernels and of moments_tree_kernel, and the finish -- pure host arithmetic on a stats vector.
// Part of the ONE translation unit mcx_api.hip (included there after mcx_host_samples.hpp); not a stand-alone header.

static int diag_stats_len(int nfields, int maxlag) { return 3 + nfields * (maxlag + 4); }

// every refusal is -49, on the host, before anything is launched or allocated
static int diag_check(mcmcx_engine *h, int s0, int ns, int maxlag, const void *out, const char *who)
{
    if (!h) return fail(-49, std::string(who) + ": null handle");
    if (!out) return fail(-49, std::string(who) + ": null output");
    if (maxlag < 0 || maxlag > MCMCX_DIAG_MAXLAG) return fail(-49, std::string(who) + ": maxlag " + std::to_string(maxlag) +
        " outside 0 .. " + std::to_string(MCMCX_DIAG_MAXLAG));
    if (!h->inited) return fail(-49, std::string(who) + ": we have not inited");
    if (h->samp.thin <= 0) return fail(-49, std::string(who) + ": no samples are kept (mcmcx_set_samples before mcmcx_init)");
    if (ns < 4) return fail(-49, std::string(who) + ": a window of " + std::to_string(ns) + " samples (two halves of two need 4)");
    const long long have = samples_retained(h);
    if (s0 < 0 || (long long)s0 + ns > have) return fail(-49, std::string(who) + ": samples " + std::to_string(s0) + " .. " +
        std::to_string((long long)s0 + ns - 1) + " asked for, " + std::to_string(have) + " retained");
    return 0;
}

// the scratch: [ntiles][nfields][maxlag + 3] tile rows, shift[nfields], one stats vector (the host form's staging); allocated at the first
// call, grows only, freed by mcmcx_destroy
static int diag_scratch(mcmcx_engine *h, size_t need)
{
    if (need <= h->diag_cap) return 0;
    HIPCHK(hipStreamSynchronize(h->stream));                    // an earlier summary may still read the old one
    if (h->d_diag) (void)hipFree(h->d_diag);
    h->d_diag = nullptr; h->diag_cap = 0;
    void *q = nullptr;
    const hipError_t e = hipMalloc(&q, need * sizeof(double));
    if (e != hipSuccess) return fail(-101, "hipMalloc of " + std::to_string(need * sizeof(double)) + " bytes: " + hipGetErrorString(e));
    h->d_diag = (double *)q; h->diag_cap = need;
    return 0;
}

// the stats vector of the window into dev_out (nullptr: the scratch's staging vector, returned in *staged); asynchronous on the stream
static int diag_launch(mcmcx_engine *h, int s0, int ns, int maxlag, const double *shift, double *dev_out, double **staged)
{
    const SamplePlan &s = h->samp;
    HIPCHK(hipSetDevice(h->cfg.device));
    const int nf = samples_nfields(h), T = h->ntiles, nh = ns / 2, K = std::min(maxlag, nh - 1);
    const int len = nf * (maxlag + 3), slen = diag_stats_len(nf, maxlag);
    int rc = diag_scratch(h, (size_t)T * (size_t)len + (size_t)nf + (size_t)slen); if (rc) return rc;
    double *rows = h->d_diag, *dshift = rows + (size_t)T * (size_t)len, *stage = dshift + nf;
    if (!dev_out) dev_out = stage;
    if (staged) *staged = dev_out;
    const long long have = samples_retained(h);
    const size_t slot0 = (size_t)((s.kept - have + s0) % s.capacity);
    if (shift) HIPCHK(hipMemcpyAsync(dshift, shift, (size_t)nf * sizeof(double), hipMemcpyHostToDevice, h->stream));
    else hipLaunchKernelGGL(diag_shift_kernel, dim3((unsigned)((nf + 255) / 256)), dim3(256), 0, h->stream, (const double *)s.store, dshift,
        slot0, T, nf);
    DiagArgs A;
    A.store = s.store; A.shift = dshift; A.out = rows; A.slot0 = slot0; A.cap = (size_t)s.capacity;
    A.ntiles = T; A.nfields = nf; A.nchains = h->cfg.nchains; A.ns = ns; A.nh = nh; A.K = K; A.maxlag = maxlag;
    const dim3 grid((unsigned)T, (unsigned)((nf + 3) / 4)), block(256);
    // the window length W of the instantiation holds lags 0 .. W - 1 >= K
    if (K == 0) hipLaunchKernelGGL(diag_tile_kernel<1>, grid, block, 0, h->stream, A);
    else if (K <= 8) hipLaunchKernelGGL(diag_tile_kernel<9>, grid, block, 0, h->stream, A);
    else if (K <= 16) hipLaunchKernelGGL(diag_tile_kernel<17>, grid, block, 0, h->stream, A);
    else hipLaunchKernelGGL(diag_tile_kernel<33>, grid, block, 0, h->stream, A);
    for (long long stride = 1;; stride *= 64) {                            // as pooled_moments_launch does
        const long long groups = (T + 64 * stride - 1) / (64 * stride);
        hipLaunchKernelGGL(moments_tree_kernel, dim3((unsigned)((len + 255) / 256), (unsigned)groups), dim3(256), 0, h->stream, rows, T,
                           len, (int)stride, (double *)nullptr);
        if (groups == 1) break;
    }
    hipLaunchKernelGGL(diag_pack_kernel, dim3((unsigned)((slen + 255) / 256)), dim3(256), 0, h->stream, (const double *)rows,
        (const double *)dshift, dev_out, nf, maxlag, 2.0 * (double)h->cfg.nchains, (double)nh, (double)K);
    HIPCHK(hipGetLastError());
    return 0;
}

// The finish (include/mcmcx.h states it): table[f] = mean, sd, rhat, ess, mcse, W, Bn, truncated
static int diag_finish(const double *stats, int nfields, int maxlag, double *table)
{
    const double M = stats[0], nh = stats[1], Kd = stats[2];
    // the header is a caller's (perhaps a sum over ranks): checked as doubles before anything is converted or indexed with it
    if (!(Kd >= 0.0 && Kd <= (double)maxlag) || Kd != std::floor(Kd)) return fail(-49, "mcmcx_samples_diag: the vector's K is no integer "
        "in 0 .. maxlag");
    if (!(M >= 2.0) || !(nh >= 2.0)) return fail(-49, "mcmcx_samples_diag: the vector's M and n_h must be at least 2");
    if (!(Kd <= nh - 1.0)) return fail(-49, "mcmcx_samples_diag: the vector's K exceeds n_h - 1 (summing vectors adds M, S1, S2 and G; n_h, "
        "K and the shifts are the window's and stay)");
    const int K = (int)Kd;
    const int npairs = (K + 1) / 2;
    const double cap = 1.0 / std::log10(M * nh);
    for (int f = 0; f < nfields; ++f) {
        const double *p = stats + 3 + (size_t)f * (size_t)(maxlag + 4), *G = p + 3;
        const double shift = p[0], S1 = p[1], S2 = p[2];
        const double Wv = G[0] / (M * (nh - 1.0));
        const double Bn = (S2 - S1 * S1 / M) / (M - 1.0);
        const double varp = Wv * (nh - 1.0) / nh + Bn;
        const double rhat = std::sqrt(varp / Wv);
        auto rho = [&](int t) { return t == 0 ? 1.0 : 1.0 - (Wv - G[t] / (M * nh)) / varp; };
        double sum = 0.0, prev = 0.0;
        bool stopped = false;
        for (int k = 0; k < npairs; ++k) {
            double P = rho(2 * k) + rho(2 * k + 1);
            if (P <= 0.0) { stopped = true; break; }
            if (k > 0 && P > prev) P = prev;
            sum = sum + P; prev = P;
        }
        double tau = -1.0 + 2.0 * sum;
        if (tau < cap) tau = cap;
        const double ess = npairs > 0 ? M * nh / tau : std::nan("");
        const double sd = std::sqrt(varp);
        double *o = table + (size_t)f * 8;
        o[0] = shift + S1 / M; o[1] = sd; o[2] = rhat; o[3] = ess; o[4] = sd / std::sqrt(ess); o[5] = Wv; o[6] = Bn;
        o[7] = stopped ? 0.0 : 1.0;
    }
    return 0;
}
