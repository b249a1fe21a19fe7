// mcx_host_diag.hpp -- the sample store's convergence summary, host side (mcmcx_samples_stats / _dev / _diag): its own refusals, its layout
// of the readers' scratch, the launches of mcx_diag.hpp's kernels, and the finish -- pure host arithmetic on a stats vector.  The window,
// the scratch, the shift and the tree launch are mcx_host_samples.hpp's.
// Part of the ONE translation unit mcx_api.hip (included there after mcx_host_samples.hpp); not a stand-alone header.

static int diag_stats_len(int nfields, int maxlag) { return 3 + nfields * (maxlag + 4); }
// doubles of the scratch: [ntiles][nfields][maxlag + 3] tile rows, shift[nfields], for a transformed summary (kind != 0) its parameter
// a[nfields], one stats vector (the host form's staging)
static size_t diag_scratch_len(int ntiles, int nfields, int maxlag, int kind = XF_IDENTITY)
{
    return (size_t)ntiles * (size_t)nfields * (size_t)(maxlag + 3) + (size_t)nfields * (kind != XF_IDENTITY ? 2 : 1) +
        (size_t)diag_stats_len(nfields, maxlag);
}

// every refusal is `code` (-49; -53 from the transformed summary's entries), on the host, before anything is launched or allocated
static int diag_check(mcmcx_engine *h, int s0, int ns, int maxlag, const void *out, const char *who, int code = -49)
{
    if (!h) return fail(code, std::string(who) + ": null handle");
    if (!out) return fail(code, std::string(who) + ": null output");
    if (maxlag < 0 || maxlag > MCMCX_DIAG_MAXLAG) return fail(code, std::string(who) + ": maxlag " + std::to_string(maxlag) +
        " outside 0 .. " + std::to_string(MCMCX_DIAG_MAXLAG));
    return samples_window_check(h, s0, ns, code, 4, who);      // two halves of two samples
}

// what a transformed summary refuses on top of that, -53: decided by the arguments alone, so looked at first
static int diag_xf_check(int kind, const double *a, const char *who)
{
    if (kind < XF_IDENTITY || kind > XF_SQUARE) return fail(-53, std::string(who) + ": kind " + std::to_string(kind) + " outside 0 .. 3");
    if (kind != XF_IDENTITY && !a) return fail(-53, std::string(who) + ": null a (only kind 0 does not look at it)");
    return 0;
}

// diag_tile_kernel<W> of u(x): W = 1, 9, 17, 33 holds lags 0 .. W - 1 >= K
template <int KIND>
static void diag_xf_tile_launch(const DiagArgs &A, const double *da, dim3 grid, hipStream_t stream)
{
    const dim3 block(256);
    if (A.K == 0) hipLaunchKernelGGL((diag_xf_tile_kernel<1, KIND>), grid, block, 0, stream, A, da);
    else if (A.K <= 8) hipLaunchKernelGGL((diag_xf_tile_kernel<9, KIND>), grid, block, 0, stream, A, da);
    else if (A.K <= 16) hipLaunchKernelGGL((diag_xf_tile_kernel<17, KIND>), grid, block, 0, stream, A, da);
    else hipLaunchKernelGGL((diag_xf_tile_kernel<33, KIND>), grid, block, 0, stream, A, da);
}

// The stats vector of u(window W) (scratch w of diag_scratch_len doubles) into dev_out; asynchronous on `stream`.  shift: host memory or
// nullptr (u of chain 0 of window sample 0); a: host memory, u's parameter per field (not looked at by kind 0).
static int diag_launch(const SampleWin &W, double *w, int maxlag, int kind, const double *a, const double *shift, double *dev_out,
                       hipStream_t stream)
{
    const int nf = W.nfields, T = W.ntiles, nh = W.ns / 2, K = std::min(maxlag, nh - 1);
    const int len = nf * (maxlag + 3), slen = diag_stats_len(nf, maxlag);
    double *rows = w, *dshift = rows + (size_t)T * (size_t)len, *da = dshift + nf;
    if (kind != XF_IDENTITY) HIPCHK(hipMemcpyAsync(da, a, (size_t)nf * sizeof(double), hipMemcpyHostToDevice, stream));
    if (kind == XF_IDENTITY || shift) { int rc = samples_shift(W, shift, dshift, stream); if (rc) return rc; }
    else {
        const dim3 g((unsigned)((nf + 255) / 256)), b(256);
        if (kind == XF_LE) hipLaunchKernelGGL(diag_xf_shift_kernel<XF_LE>, g, b, 0, stream, W.store, da, dshift, W.slot0, T, nf);
        else if (kind == XF_FOLD) hipLaunchKernelGGL(diag_xf_shift_kernel<XF_FOLD>, g, b, 0, stream, W.store, da, dshift, W.slot0, T, nf);
        else hipLaunchKernelGGL(diag_xf_shift_kernel<XF_SQUARE>, g, b, 0, stream, W.store, da, dshift, W.slot0, T, nf);
    }
    DiagArgs A;
    A.store = W.store; A.shift = dshift; A.out = rows; A.slot0 = W.slot0; A.cap = W.cap;
    A.ntiles = T; A.nfields = nf; A.nchains = W.nchains; A.ns = W.ns; A.nh = nh; A.K = K; A.maxlag = maxlag;
    const dim3 grid((unsigned)T, (unsigned)((nf + 3) / 4)), block(256);
    if (kind == XF_LE) diag_xf_tile_launch<XF_LE>(A, da, grid, stream);
    else if (kind == XF_FOLD) diag_xf_tile_launch<XF_FOLD>(A, da, grid, stream);
    else if (kind == XF_SQUARE) diag_xf_tile_launch<XF_SQUARE>(A, da, grid, stream);
    // the window length W of the instantiation holds lags 0 .. W - 1 >= K
    else if (K == 0) hipLaunchKernelGGL(diag_tile_kernel<1>, grid, block, 0, stream, A);
    else if (K <= 8) hipLaunchKernelGGL(diag_tile_kernel<9>, grid, block, 0, stream, A);
    else if (K <= 16) hipLaunchKernelGGL(diag_tile_kernel<17>, grid, block, 0, stream, A);
    else hipLaunchKernelGGL(diag_tile_kernel<33>, grid, block, 0, stream, A);
    moments_tree_launch(stream, rows, T, len, nullptr);
    hipLaunchKernelGGL(diag_pack_kernel, dim3((unsigned)((slen + 255) / 256)), dim3(256), 0, stream, (const double *)rows,
        (const double *)dshift, dev_out, nf, maxlag, 2.0 * (double)W.nchains, (double)nh, (double)K);
    HIPCHK(hipGetLastError());
    return 0;
}

// the stats vector of u(the engine's window) into dev_out (nullptr: the scratch's staging vector, returned in *staged)
static int diag_engine(mcmcx_engine *h, int s0, int ns, int maxlag, int kind, const double *a, const double *shift, double *dev_out,
                       double **staged)
{
    HIPCHK(hipSetDevice(h->cfg.device));
    const SampleWin W = samples_window(h, s0, ns);
    const size_t need = diag_scratch_len(W.ntiles, W.nfields, maxlag, kind);
    int rc = samples_scratch(h, need * sizeof(double)); if (rc) return rc;
    double *w = (double *)h->d_scratch;
    if (!dev_out) dev_out = w + need - (size_t)diag_stats_len(W.nfields, maxlag);
    if (staged) *staged = dev_out;
    return diag_launch(W, w, maxlag, kind, a, shift, dev_out, h->stream);
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
