// mcx_host_diag.hpp -- the sample store's convergence summary, host side (mcmcx_samples_stats / _dev / _diag): its own refusals, its layout
// of the readers' scratch, the launches of mcx_diag.hpp's and mcx_diag_xf.hpp's kernels, and the finish -- pure host arithmetic on a stats
// vector; for the step summary (mcx_host_diag_step.hpp) too the argument block, the choice of an instantiation by K and what follows a
// tile kernel.  The window, the scratch, a reader's prologue, the shift and the tree launch are mcx_host_samples.hpp's.
// Part of the ONE translation unit mcx_api.hip (included there after mcx_host_samples.hpp); not a stand-alone header.

static int diag_stats_len(int nfields, int maxlag) { return 3 + nfields * (maxlag + 4); }
// doubles of the scratch before the one stats vector at its end (the host form's staging): [ntiles][nfields][maxlag + 3] tile rows,
// shift[nfields] and, for a transformed summary (kind != 0), its parameter a[nfields]
static size_t diag_work_len(int ntiles, int nfields, int maxlag, int kind = XF_IDENTITY)
{
    return (size_t)ntiles * (size_t)nfields * (size_t)(maxlag + 3) + (size_t)nfields * (kind != XF_IDENTITY ? 2 : 1);
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

// The summaries' argument block of window W: shift[nfields] in dshift, the tile rows in rows
static DiagArgs diag_args(const SampleWin &W, const double *dshift, double *rows, int maxlag)
{
    DiagArgs A;
    A.store = W.store; A.shift = dshift; A.out = rows; A.slot0 = W.slot0; A.cap = W.cap;
    A.ntiles = W.ntiles; A.nfields = W.nfields; A.nchains = W.nchains; A.ns = W.ns; A.nh = W.ns / 2;
    A.K = std::min(maxlag, A.nh - 1); A.maxlag = maxlag;
    return A;
}

// The instantiation of a tile kernel by K: its window length W = 1, 9, 17, 33 holds lags 0 .. W - 1 >= K.  f is handed W as a
// std::integral_constant, a compile-time value; the identity's, the transformed and the step kernels are all chosen here
template <class F>
static void diag_with_W(int K, F &&f)
{
    if (K == 0) f(std::integral_constant<int, 1>());
    else if (K <= 8) f(std::integral_constant<int, 9>());
    else if (K <= 16) f(std::integral_constant<int, 17>());
    else f(std::integral_constant<int, 33>());
}

static dim3 diag_grid(const DiagArgs &A) { return dim3((unsigned)A.ntiles, (unsigned)((A.nfields + 3) / 4)); }

// what follows a tile kernel, whichever it was: the tree over the tiles' rows and the stats vector packed into dev_out
static int diag_finish_launch(const DiagArgs &A, double *dev_out, hipStream_t stream)
{
    const int slen = diag_stats_len(A.nfields, A.maxlag);
    moments_tree_launch(stream, A.out, A.ntiles, A.nfields * (A.maxlag + 3), nullptr);
    hipLaunchKernelGGL(diag_pack_kernel, dim3((unsigned)((slen + 255) / 256)), dim3(256), 0, stream, (const double *)A.out, A.shift,
        dev_out, A.nfields, A.maxlag, 2.0 * (double)A.nchains, (double)A.nh, (double)A.K);
    HIPCHK(hipGetLastError());
    return 0;
}

// diag_xf_shift_kernel<KIND> and diag_xf_tile_kernel<W, KIND> of one kind
template <int KIND>
static void diag_xf_launch(const DiagArgs &A, const double *da, double *dshift, bool own_shift, hipStream_t stream)
{
    if (own_shift) hipLaunchKernelGGL(diag_xf_shift_kernel<KIND>, dim3((unsigned)((A.nfields + 255) / 256)), dim3(256), 0, stream, A.store,
        da, dshift, A.slot0, A.ntiles, A.nfields);
    diag_with_W(A.K, [&](auto w) {
        hipLaunchKernelGGL((diag_xf_tile_kernel<decltype(w)::value, KIND>), diag_grid(A), dim3(256), 0, stream, A, da);
    });
}

// The stats vector of u(window W) (scratch w: diag_work_len doubles and, where dev_out lies there, the vector) into dev_out; asynchronous
// on `stream`.  shift: host memory or nullptr (u of chain 0 of window sample 0); a: host memory, u's parameter per field (not looked at
// by kind 0).
static int diag_launch(const SampleWin &W, double *w, int maxlag, int kind, const double *a, const double *shift, double *dev_out,
                       hipStream_t stream)
{
    const int nf = W.nfields;
    double *rows = w, *dshift = rows + (size_t)W.ntiles * (size_t)nf * (size_t)(maxlag + 3), *da = dshift + nf;
    const DiagArgs A = diag_args(W, dshift, rows, maxlag);
    if (kind != XF_IDENTITY) HIPCHK(hipMemcpyAsync(da, a, (size_t)nf * sizeof(double), hipMemcpyHostToDevice, stream));
    if (kind == XF_IDENTITY || shift) { int rc = samples_shift(W, shift, dshift, stream); if (rc) return rc; }
    if (kind == XF_LE) diag_xf_launch<XF_LE>(A, da, dshift, !shift, stream);
    else if (kind == XF_FOLD) diag_xf_launch<XF_FOLD>(A, da, dshift, !shift, stream);
    else if (kind == XF_SQUARE) diag_xf_launch<XF_SQUARE>(A, da, dshift, !shift, stream);
    else diag_with_W(A.K, [&](auto w) {
        hipLaunchKernelGGL(diag_tile_kernel<decltype(w)::value>, diag_grid(A), dim3(256), 0, stream, A);
    });
    return diag_finish_launch(A, dev_out, stream);
}

// mcmcx_samples_stats, mcmcx_samples_stats_of (`code` -53: kind 0 and a null `a` pass diag_xf_check) and their _dev forms: the refusals,
// then the stats vector of u(the engine's window) into dev_out or, host_out given, into the scratch's staging vector and from there
static int diag_run(mcmcx_engine *h, int s0, int ns, int maxlag, int kind, const double *a, const double *shift, void *dev_out,
                    double *host_out, const char *who, int code = -49)
{
    int rc = diag_xf_check(kind, a, who); if (rc) return rc;
    if ((rc = diag_check(h, s0, ns, maxlag, dev_out ? dev_out : host_out, who, code))) return rc;
    const int nf = samples_nfields(h);
    const size_t work = diag_work_len(h->ntiles, nf, maxlag, kind), slen = (size_t)diag_stats_len(nf, maxlag);
    return samples_run<double>(h, s0, ns, work + slen, work, slen, dev_out, host_out, [&](const SampleWin &W, double *w, double *out) {
        return diag_launch(W, w, maxlag, kind, a, shift, out, h->stream);
    });
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
