// mcx_host_diag_step.hpp -- the summary of a step function of the sample store, host side (mcmcx_samples_stats_step / _dev,
// mcmcx_debug_samples_stats_step, mcmcx_samples_rank_scores): its own refusals, its layout of the readers' scratch, the launches of
// mcx_diag_step.hpp's kernels, and the table of normal scores -- pure host arithmetic on histogram counts.  The window, the scratch, a
// reader's prologue, the staging of keys and the tree launch are mcx_host_samples.hpp's; the stats vector's length, the argument block,
// the choice of an instantiation by K and what follows the tile kernel mcx_host_diag.hpp's; the edges' rules mcx_host_hist.hpp's.
// Part of the ONE translation unit mcx_api.hip (included there after mcx_host_hist.hpp); not a stand-alone header.

// doubles of the scratch before the one stats vector at its end (the host form's staging): the summary's tile rows and shift[nfields],
// the edges' keys [nfields][nbins + 1], the table [nfields][nbins + 2]
static size_t diag_step_work_len(int ntiles, int nfields, int maxlag, int nbins)
{
    return diag_work_len(ntiles, nfields, maxlag) + (size_t)nfields * (size_t)(2 * nbins + 3);
}

// every refusal is -54, on the host, before anything is launched or allocated.  What the arguments alone decide comes first: the
// pointers and the bin count here (of the edge table the first field's row: every store has one field at least) ...
static int diag_step_check_args(int nbins, const double *edges, const double *table, const void *out, const char *who)
{
    if (!out) return fail(-54, std::string(who) + ": null output");
    if (!edges) return fail(-54, std::string(who) + ": null edge table");
    if (!table) return fail(-54, std::string(who) + ": null table");
    if (nbins < 1 || nbins > MCMCX_STEP_MAXBINS) return fail(-54, std::string(who) + ": " + std::to_string(nbins) + " bins, outside 1 .. " +
        std::to_string(MCMCX_STEP_MAXBINS));
    return hist_check_edges(edges, 1, nbins, who, -54);
}

// ... then the handle, the rest of the edges now that nfields is known, and everything mcmcx_samples_stats refuses
static int diag_step_check(mcmcx_engine *h, int s0, int ns, int maxlag, int nbins, const double *edges, const double *table,
                           const void *out, const char *who)
{
    int rc = diag_step_check_args(nbins, edges, table, out, who); if (rc) return rc;
    if (!h) return fail(-54, std::string(who) + ": null handle");
    if ((rc = hist_check_edges(edges, samples_nfields(h), nbins, who, -54))) return rc;
    return diag_check(h, s0, ns, maxlag, out, who, -54);
}

// The stats vector of u(window W) (scratch w: diag_step_work_len doubles and, where dev_out lies there, the vector) into dev_out;
// asynchronous on `stream`.  edges, table and shift are host memory; shift == nullptr: u of chain 0 of window sample 0.
static int diag_step_launch(const SampleWin &W, double *w, int maxlag, int nbins, const double *edges, const double *table,
                            const double *shift, double *dev_out, hipStream_t stream)
{
    const int nf = W.nfields, ne = nbins + 1, nc = nbins + 2;
    double *rows = w, *dshift = rows + (size_t)W.ntiles * (size_t)nf * (size_t)(maxlag + 3);
    unsigned long long *dkeys = (unsigned long long *)(dshift + nf);
    double *dtable = (double *)(dkeys + (size_t)nf * (size_t)ne);
    int rc = samples_stage_keys(dkeys, edges, (size_t)nf * (size_t)ne, stream); if (rc) return rc;
    HIPCHK(hipMemcpyAsync(dtable, table, (size_t)nf * (size_t)nc * sizeof(double), hipMemcpyHostToDevice, stream));
    const DiagArgs A = diag_args(W, dshift, rows, maxlag);
    const unsigned long long *ek = dkeys;
    const double *tb = dtable;
    if (shift) HIPCHK(hipMemcpyAsync(dshift, shift, (size_t)nf * sizeof(double), hipMemcpyHostToDevice, stream));
    else hipLaunchKernelGGL(diag_step_shift_kernel, dim3((unsigned)((nf + 255) / 256)), dim3(256), 0, stream, W.store, ek, tb, dshift,
        W.slot0, W.ntiles, nf, nbins);
    const size_t lds = DiagStepLds(nbins).bytes;
    diag_with_W(A.K, [&](auto w_) {
        hipLaunchKernelGGL(diag_step_tile_kernel<decltype(w_)::value>, diag_grid(A), dim3(256), lds, stream, A, ek, tb, nbins);
    });
    return diag_finish_launch(A, dev_out, stream);
}

// mcmcx_samples_stats_step and its _dev form: the refusals, then the stats vector of u(the engine's window) into dev_out or, host_out
// given, into the scratch's staging vector and from there
static int diag_step_run(mcmcx_engine *h, int s0, int ns, int maxlag, int nbins, const double *edges, const double *table,
                         const double *shift, void *dev_out, double *host_out, const char *who)
{
    int rc = diag_step_check(h, s0, ns, maxlag, nbins, edges, table, dev_out ? dev_out : host_out, who); if (rc) return rc;
    const int nf = samples_nfields(h);
    const size_t work = diag_step_work_len(h->ntiles, nf, maxlag, nbins), slen = (size_t)diag_stats_len(nf, maxlag);
    return samples_run<double>(h, s0, ns, work + slen, work, slen, dev_out, host_out, [&](const SampleWin &W, double *w, double *out) {
        return diag_step_launch(W, w, maxlag, nbins, edges, table, shift, out, h->stream);
    });
}

// Phi^-1(p) for 0 < p < 1: Wichura's algorithm AS241 (Applied Statistics 37, 1988), routine PPND16, operation by operation -- three
// pairs of polynomials of degree seven in Horner's form, highest coefficient first, about 1e-16 relative accuracy.  No contraction: every
// product and sum is one IEEE operation (the translation unit is built with contraction off; the pragma says so here too).
static double step_horner7(const double (&c)[8], double r)
{
#pragma clang fp contract(off)
    double s = c[0];
    for (int i = 1; i < 8; ++i) s = s * r + c[i];
    return s;
}

static double step_ppnd16(double p)
{
#pragma clang fp contract(off)
    static const double A[8] = {2.5090809287301226727e+3, 3.3430575583588128105e+4, 6.7265770927008700853e+4, 4.5921953931549871457e+4,
                                1.3731693765509461125e+4, 1.9715909503065514427e+3, 1.3314166789178437745e+2, 3.3871328727963666080e+0};
    static const double B[8] = {5.2264952788528545610e+3, 2.8729085735721942674e+4, 3.9307895800092710610e+4, 2.1213794301586595867e+4,
                                5.3941960214247511077e+3, 6.8718700749205790830e+2, 4.2313330701600911252e+1, 1.0};
    static const double C[8] = {7.74545014278341407640e-4, 2.27238449892691845833e-2, 2.41780725177450611770e-1, 1.27045825245236838258e+0,
                                3.64784832476320460504e+0, 5.76949722146069140550e+0, 4.63033784615654529590e+0, 1.42343711074968357734e+0};
    static const double D[8] = {1.05075007164441684324e-9, 5.47593808499534494600e-4, 1.51986665636164571966e-2, 1.48103976427480074590e-1,
                                6.89767334985100004550e-1, 1.67638483018380384940e+0, 2.05319162663775882187e+0, 1.0};
    static const double E[8] = {2.01033439929228813265e-7, 2.71155556874348757815e-5, 1.24266094738807843860e-3, 2.65321895265761230930e-2,
                                2.96560571828504891230e-1, 1.78482653991729133580e+0, 5.46378491116411436990e+0, 6.65790464350110377720e+0};
    static const double F[8] = {2.04426310338993978564e-15, 1.42151175831644588870e-7, 1.84631831751005468180e-5, 7.86869131145613259100e-4,
                                1.48753612908506148525e-2, 1.36929880922735805310e-1, 5.99832206555887937690e-1, 1.0};
    const double q = p - 0.5;
    if (std::fabs(q) <= 0.425) {
        const double r = 0.180625 - q * q;
        return step_horner7(A, r) * q / step_horner7(B, r);
    }
    double r = q < 0.0 ? p : 1.0 - p;
    r = std::sqrt(-std::log(r));
    double x;
    if (r <= 5.0) { r = r - 1.6; x = step_horner7(C, r) / step_horner7(D, r); }
    else { r = r - 5.0; x = step_horner7(E, r) / step_horner7(F, r); }
    return q < 0.0 ? -x : x;
}

// scores[f][b] = Phi^-1 of the average 1-based rank of cell b's values in Blom's form, +0.0 for an empty cell (include/mcmcx.h has the
// definition).  Integers in int64_t; a total above 2**61 is refused, so that 2 before + count + 1 cannot wrap.
static int step_rank_scores(const int64_t *counts, int nfields, int nbins, double *scores)
{
    const char *who = "mcmcx_samples_rank_scores";
    const int nc = nbins + 2;
    for (int f = 0; f < nfields; ++f) {
        const int64_t *c = counts + (size_t)f * (size_t)nc;
        int64_t n = 0;
        for (int b = 0; b < nc; ++b) {
            if (c[b] < 0) return fail(-54, std::string(who) + ": cell " + std::to_string(b) + " of field " + std::to_string(f) +
                " has a negative count");
            if (c[b] > ((int64_t)1 << 61) - n) return fail(-54, std::string(who) + ": the counts of field " + std::to_string(f) +
                " add up to more than 2**61");
            n += c[b];
        }
        if (n < 1) return fail(-54, std::string(who) + ": field " + std::to_string(f) + " has no counts");
    }
    for (int f = 0; f < nfields; ++f) {
        const int64_t *c = counts + (size_t)f * (size_t)nc;
        double *o = scores + (size_t)f * (size_t)nc;
        int64_t n = 0, before = 0;
        for (int b = 0; b < nc; ++b) n += c[b];
        for (int b = 0; b < nc; ++b) {
            if (c[b] > 0) {
                const double p = ((double)(2 * before + c[b] + 1) * 0.5 - 0.375) / ((double)n + 0.25);
                o[b] = step_ppnd16(p);
            } else o[b] = 0.0;
            before += c[b];
        }
    }
    return 0;
}
