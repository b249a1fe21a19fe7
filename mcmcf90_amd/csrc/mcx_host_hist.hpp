// mcx_host_hist.hpp -- marginal and pairwise joint histograms of the sample store, host side (mcmcx_samples_hist / _hist2 / _hist_edges /
// _hist_density, mcmcx_debug_samples_hist): its own refusals, its layout of the readers' scratch, the launches of mcx_hist.hpp's kernels,
// the uniform edges and the density finish -- pure host arithmetic.  The window, the scratch, a reader's prologue and the staging of keys
// are mcx_host_samples.hpp's.
// Part of the ONE translation unit mcx_api.hip (included there after mcx_host_quant.hpp); not a stand-alone header.

// every refusal is -52, on the host, before anything is launched or allocated.  What the arguments alone decide comes first, so that it
// is refused, and can be tested, without an engine: the pointers and the counts here, ...
static int hist_check_args(int nbins, int maxbins, const void *edges, const void *out, const char *who)
{
    if (!out) return fail(-52, std::string(who) + ": null output");
    if (!edges) return fail(-52, std::string(who) + ": null edge table");
    if (nbins < 1 || nbins > maxbins) return fail(-52, std::string(who) + ": " + std::to_string(nbins) + " bins, outside 1 .. " +
        std::to_string(maxbins));
    return 0;
}

static int hist_check_npairs(int npairs, const void *pairs, const char *who)
{
    if (!pairs) return fail(-52, std::string(who) + ": null pair list");
    if (npairs < 1 || npairs > MCMCX_HIST2_MAXPAIRS) return fail(-52, std::string(who) + ": " + std::to_string(npairs) +
        " pairs, outside 1 .. " + std::to_string(MCMCX_HIST2_MAXPAIRS));
    return 0;
}

// ... the edges, edges[nrows][nbins + 1]: no NaN, non-decreasing by key within a row (equal neighbours and +-inf are allowed), ...
// (`code`: -52; -54 from the step summary's entries, which hold their edges to the same rules)
static int hist_check_edges(const double *edges, int nrows, int nbins, const char *who, int code = -52)
{
    for (int f = 0; f < nrows; ++f) {
        const double *e = edges + (size_t)f * (size_t)(nbins + 1);
        unsigned long long prev = 0ull;
        for (int i = 0; i <= nbins; ++i) {
            if (e[i] != e[i]) return fail(code, std::string(who) + ": edge " + std::to_string(i) + " of field " + std::to_string(f) +
                " is a NaN");
            unsigned long long b; memcpy(&b, e + i, 8);
            const unsigned long long k = quant_key(b);
            if (i > 0 && k < prev) return fail(code, std::string(who) + ": edges " + std::to_string(i - 1) + " and " + std::to_string(i) +
                " of field " + std::to_string(f) + " decrease (the key order: -0.0 lies below +0.0)");
            prev = k;
        }
    }
    return 0;
}

// ... and the pairs, once nfields is known
static int hist_check_pairs(const int32_t *pairs, int npairs, int nfields, const char *who)
{
    for (int p = 0; p < 2 * npairs; ++p)
        if (pairs[p] < 0 || pairs[p] >= nfields) return fail(-52, std::string(who) + ": pair " + std::to_string(p / 2) + " names field " +
            std::to_string(pairs[p]) + ", outside 0 .. " + std::to_string(nfields - 1));
    return 0;
}

// The checks of an engine's call in their order: the arguments alone (of the edge table the first field's row: every store has one field
// at least), the null handle, the rest of the table and the pairs now that nfields is known, the shared window checks.  two: the 2-D form
static int hist_check(mcmcx_engine *h, int s0, int ns, bool two, int npairs, const int32_t *pairs, int nbins, const double *edges,
                      const void *out, const char *who)
{
    int rc = hist_check_args(nbins, two ? MCMCX_HIST2_MAXBINS : MCMCX_HIST_MAXBINS, edges, out, who); if (rc) return rc;
    if (two && (rc = hist_check_npairs(npairs, pairs, who))) return rc;
    if ((rc = hist_check_edges(edges, 1, nbins, who))) return rc;
    if (!h) return fail(-52, std::string(who) + ": null handle");
    const int nf = samples_nfields(h);
    if ((rc = hist_check_edges(edges, nf, nbins, who))) return rc;
    if (two && (rc = hist_check_pairs(pairs, npairs, nf, who))) return rc;
    return samples_window_check(h, s0, ns, -52, 1, who);
}

// 64-bit words of a call's table and of its edge keys
static size_t hist_table_words(int nf, int npairs, int nbins)
{
    return npairs ? (size_t)npairs * (size_t)(nbins + 2) * (size_t)(nbins + 2) : (size_t)nf * (size_t)(nbins + 2);
}
static size_t hist_key_words(int nf, int nbins) { return (size_t)nf * (size_t)(nbins + 1); }

// chunk = 0: the default, 32 768 window samples per blockIdx.z
static QuantWin hist_window(const SampleWin &W, int chunk)
{
    QuantWin A;
    A.win = W; A.chunk = std::min(W.ns, chunk > 0 ? chunk : 32768);
    return A;
}

// The 1-D table (npairs = 0) or the 2-D table of window A into dev_out, the edges' keys staged in `wkeys` (hist_key_words); asynchronous
// on `stream`.  The grid: about ten blocks per compute unit over the fields or pairs, a wave never more than 128 tiles and a block never
// more than 32 768 window samples of them -- 2**30 values, so that a 32-bit counter in LDS cannot wrap whatever n is.
static int hist_launch(const QuantWin &A, unsigned long long *wkeys, int nbins, const double *edges, int npairs, const int32_t *pairs,
                       unsigned long long *dev_out, hipStream_t stream)
{
    const int nf = A.win.nfields, T = A.win.ntiles, ne = nbins + 1, ny = npairs ? npairs : nf;
    const size_t words = hist_table_words(nf, npairs, nbins);
    int rc = samples_stage_keys(wkeys, edges, hist_key_words(nf, nbins), stream); if (rc) return rc;
    int top = 1;
    while (2 * top <= ne) top *= 2;
    const long long t4 = ((long long)T + 3) / 4;
    const long long gx = std::min(t4, std::max<long long>(std::max(1, 2560 / ny), (t4 + 127) / 128));
    const dim3 grid((unsigned)gx, (unsigned)ny, (unsigned)((A.win.ns + A.chunk - 1) / A.chunk)), block(256);
    const unsigned long long *ek = wkeys;
    hipLaunchKernelGGL(quant_counts_zero_kernel, dim3((unsigned)((words + 255) / 256)), block, 0, stream, dev_out, (int)words);
    if (!npairs) {
        hipLaunchKernelGGL(hist_kernel, grid, block, HistLds(nbins, false).bytes, stream, A, ek, dev_out, nbins, top);
    } else {
        HistPairs P;
        for (int p = 0; p < HIST2_MAXPAIRS; ++p) { P.j[p] = p < npairs ? pairs[2 * p] : 0; P.k[p] = p < npairs ? pairs[2 * p + 1] : 0; }
        hipLaunchKernelGGL(hist2_kernel, grid, block, HistLds(nbins, true).bytes, stream, A, ek, P, dev_out, nbins, top);
    }
    HIPCHK(hipGetLastError());
    return 0;
}

// mcmcx_samples_hist, _hist2 (two: npairs pairs) and their _dev forms: the refusals, then the table of the engine's window into dev_out
// or, host_out given, into the scratch's staging table and from there; the scratch holds the edges' keys, then that table
static int hist_run(mcmcx_engine *h, int s0, int ns, bool two, int npairs, const int32_t *pairs, int nbins, const double *edges,
                    void *dev_out, int64_t *host_out, const char *who)
{
    int rc = hist_check(h, s0, ns, two, npairs, pairs, nbins, edges, dev_out ? dev_out : host_out, who); if (rc) return rc;
    const size_t m = hist_key_words(samples_nfields(h), nbins), words = hist_table_words(samples_nfields(h), npairs, nbins);
    typedef unsigned long long u64;
    return samples_run<u64>(h, s0, ns, m + words, m, words, dev_out, host_out, [&](const SampleWin &W, u64 *w, u64 *out) {
        return hist_launch(hist_window(W, 0), w, nbins, edges, npairs, pairs, out, h->stream);
    });
}

// e_i = lo + (hi - lo) * ((double)i / nbins) for i < nbins, e_nbins = hi
static int hist_edges(double lo, double hi, int nbins, double *out)
{
    if (!std::isfinite(lo) || !std::isfinite(hi)) return fail(-52, "mcmcx_samples_hist_edges: lo and hi must be finite");
    if (!(lo < hi)) return fail(-52, "mcmcx_samples_hist_edges: lo must lie below hi");
    const double w = hi - lo;
    for (int i = 0; i < nbins; ++i) out[i] = lo + w * ((double)i / (double)nbins);
    out[nbins] = hi;
    if (hist_check_edges(out, 1, nbins, "mcmcx_samples_hist_edges")) return fail(-52, "mcmcx_samples_hist_edges: the edges of " +
        std::to_string(lo) + " .. " + std::to_string(hi) + " are not non-decreasing (hi - lo overflows)");
    return 0;
}

// density_b = count_b / (n * (e_b - e_{b-1})) for the nbins inner cells, n the sum of the field's nbins + 2 cells
static void hist_density(const int64_t *counts, const double *edges, int nfields, int nbins, double *out)
{
    for (int f = 0; f < nfields; ++f) {
        const int64_t *c = counts + (size_t)f * (size_t)(nbins + 2);
        const double *e = edges + (size_t)f * (size_t)(nbins + 1);
        int64_t n = 0;
        for (int b = 0; b < nbins + 2; ++b) n += c[b];
        for (int b = 1; b <= nbins; ++b) out[(size_t)f * (size_t)nbins + (size_t)(b - 1)] = (double)c[b] / ((double)n * (e[b] - e[b - 1]));
    }
}
