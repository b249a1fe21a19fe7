// mcx_host_quant.hpp -- exact order statistics, tail counts and quantiles of the sample store, host side (mcmcx_samples_order_stats /
// _counts / _quantile_ranks / _quantiles): its own refusals, its layouts of the readers' scratch, the launches of mcx_quant.hpp's kernels,
// the quantile's finish.  The window, the scratch, a reader's prologue and the staging of keys are mcx_host_samples.hpp's.
// Part of the ONE translation unit mcx_api.hip (included there after mcx_host_diag.hpp); not a stand-alone header.

// every refusal is -50, on the host, before anything is launched or allocated (nr: the number of ranks or thresholds).  What the
// arguments alone decide comes first, so that it is refused, and can be tested, without an engine
static int quant_check(mcmcx_engine *h, int s0, int ns, int nr, const void *arg, const void *out, const char *who)
{
    if (!out) return fail(-50, std::string(who) + ": null output");
    if (!arg) return fail(-50, std::string(who) + ": null argument array");
    if (nr < 1 || nr > MCMCX_QUANT_MAXR) return fail(-50, std::string(who) + ": " + std::to_string(nr) +
        " ranks or thresholds, outside 1 .. " + std::to_string(MCMCX_QUANT_MAXR));
    if (!h) return fail(-50, std::string(who) + ": null handle");
    return samples_window_check(h, s0, ns, -50, 1, who);
}

static int quant_check_ranks(long long n, int nr, const int64_t *ranks, const char *who)
{
    for (int k = 0; k < nr; ++k)
        if (ranks[k] < 0 || ranks[k] >= n) return fail(-50, std::string(who) + ": rank " + std::to_string((long long)ranks[k]) +
            " outside 0 .. " + std::to_string(n - 1));
    return 0;
}

// 64-bit words of a select's scratch (table, prefix, rest, leader, the host form's staging vector)
static size_t quant_select_words(int nf, int nr) { return (size_t)nf * (size_t)nr * (size_t)(QUANT_NB + 4); }

static QuantWin quant_window(const SampleWin &W)
{
    QuantWin A;
    A.win = W; A.chunk = std::min(W.ns, 65536);
    return A;
}

// The select of nr ranks per field over window A with scratch `w` (quant_select_words), the result into dev_out[nfields][nr];
// asynchronous on `stream`.  The grid: about ten blocks per compute unit over the fields, a wave never more than 128 tiles and a block
// never more than 65 536 window samples of them -- 2**31 values, so that a 32-bit counter in LDS cannot wrap whatever n is.
static int quant_select_launch(const QuantWin &A, unsigned long long *w, int nr, const int64_t *ranks, double *dev_out, hipStream_t stream)
{
    const int nf = A.win.nfields, T = A.win.ntiles;
    const size_t m = (size_t)nf * (size_t)nr;
    QuantState S;
    S.table = w; S.prefix = w + m * QUANT_NB; S.rest = S.prefix + m; S.leader = S.rest + m; S.nr = nr;
    QuantRanks R;
    for (int k = 0; k < QUANT_MAXR; ++k) R.r[k] = k < nr ? (long long)ranks[k] : 0;
    const long long t4 = ((long long)T + 3) / 4;
    const long long gx = std::min(t4, std::max<long long>(std::max(1, 2560 / nf), (t4 + 127) / 128));
    const dim3 grid((unsigned)gx, (unsigned)nf, (unsigned)((A.win.ns + A.chunk - 1) / A.chunk)), block(256);
    const size_t lds = quant_hist_lds(nr);
    hipLaunchKernelGGL(quant_init_kernel, dim3((unsigned)((m * QUANT_NB + 255) / 256)), block, 0, stream, S, R, nf);
    for (int sh = 64 - QUANT_B; sh >= 0; sh -= QUANT_B) {
        hipLaunchKernelGGL(quant_hist_kernel, grid, block, lds, stream, A, S, sh);
        hipLaunchKernelGGL(quant_pick_kernel, dim3((unsigned)nf), block, 0, stream, S);
    }
    hipLaunchKernelGGL(quant_out_kernel, dim3((unsigned)((m + 255) / 256)), block, 0, stream, S, dev_out, nf);
    HIPCHK(hipGetLastError());
    return 0;
}

// mcmcx_samples_order_stats and its _dev form: the refusals, then the select into dev_out or, host_out given, into the scratch's
// staging vector (the last nfields * nr words of quant_select_words) and from there
static int quant_order_stats_run(mcmcx_engine *h, int s0, int ns, int nr, const int64_t *ranks, void *dev_out, double *host_out,
                                 const char *who)
{
    int rc = quant_check(h, s0, ns, nr, ranks, dev_out ? dev_out : host_out, who); if (rc) return rc;
    if ((rc = quant_check_ranks((long long)ns * h->cfg.nchains, nr, ranks, who))) return rc;
    const size_t m = (size_t)samples_nfields(h) * (size_t)nr, need = quant_select_words(samples_nfields(h), nr);
    typedef unsigned long long u64;
    return samples_run<u64>(h, s0, ns, need, need - m, m, dev_out, host_out, [&](const SampleWin &W, u64 *w, u64 *out) {
        return quant_select_launch(quant_window(W), w, nr, ranks, (double *)out, h->stream);
    });
}

// lt / le of nq thresholds per field (x[nfields][nq], host) over window A into dev_out[nfields][nq][2], the thresholds' keys staged in
// xkey; asynchronous on `stream`
static int quant_counts_launch(const QuantWin &A, unsigned long long *xkey, int nq, const double *x, unsigned long long *dev_out,
                               hipStream_t stream)
{
    const int nf = A.win.nfields, T = A.win.ntiles;
    const size_t m = (size_t)nf * (size_t)nq;
    int rc = samples_stage_keys(xkey, x, m, stream); if (rc) return rc;
    const int fb = (nf + 3) / 4;
    const long long gx = std::min<long long>(T, std::max<long long>(std::max(1, 2560 / fb), ((long long)T + 32767) / 32768));
    const dim3 grid((unsigned)gx, (unsigned)fb, (unsigned)((A.win.ns + A.chunk - 1) / A.chunk)), block(256);
    hipLaunchKernelGGL(quant_counts_zero_kernel, dim3((unsigned)((2 * m + 255) / 256)), block, 0, stream, dev_out, (int)(2 * m));
    const unsigned long long *xk = xkey;
    if (nq <= 2) hipLaunchKernelGGL(quant_counts_kernel<2>, grid, block, 0, stream, A, xk, dev_out, nq);
    else if (nq <= 8) hipLaunchKernelGGL(quant_counts_kernel<8>, grid, block, 0, stream, A, xk, dev_out, nq);
    else hipLaunchKernelGGL(quant_counts_kernel<32>, grid, block, 0, stream, A, xk, dev_out, nq);
    HIPCHK(hipGetLastError());
    return 0;
}

// mcmcx_samples_counts and its _dev form: the refusals, then the counts into dev_out or, host_out given, into the scratch's own (its
// first 2 nfields nq words; the keys lie behind them) and from there
static int quant_counts_run(mcmcx_engine *h, int s0, int ns, int nq, const double *x, void *dev_out, int64_t *host_out, const char *who)
{
    int rc = quant_check(h, s0, ns, nq, x, dev_out ? dev_out : host_out, who); if (rc) return rc;
    const size_t m2 = (size_t)samples_nfields(h) * (size_t)nq * 2;
    typedef unsigned long long u64;
    return samples_run<u64>(h, s0, ns, m2 + m2 / 2, 0, m2, dev_out, host_out, [&](const SampleWin &W, u64 *w, u64 *out) {
        return quant_counts_launch(quant_window(W), w + m2, nq, x, out, h->stream);
    });
}

// Hyndman-Fan type 7: pos = p (n - 1), lo = floor(pos), hi = min(lo + 1, n - 1), g = pos - lo
static int quant_ranks(long long n, int nq, const double *probs, int64_t *ranks, double *frac)
{
    for (int k = 0; k < nq; ++k) {
        const double p = probs[k];
        if (!(p >= 0.0 && p <= 1.0)) return fail(-50, "mcmcx_samples_quantile_ranks: a probability outside 0 .. 1");
        const double pos = p * (double)(n - 1), fl = std::floor(pos);
        const long long lo = (long long)fl;
        ranks[2 * k] = lo; ranks[2 * k + 1] = std::min(lo + 1, n - 1);
        frac[k] = pos - fl;
    }
    return 0;
}

// q = a when a and b have equal bits, else a + (b - a) g  (os[nfields][2 nq] -> out[nfields][nq])
static void quant_finish(const double *os, const double *frac, int nfields, int nq, double *out)
{
    for (int f = 0; f < nfields; ++f)
        for (int k = 0; k < nq; ++k) {
            const double a = os[((size_t)f * nq + k) * 2], b = os[((size_t)f * nq + k) * 2 + 1];
            out[(size_t)f * nq + k] = memcmp(&a, &b, 8) == 0 ? a : a + (b - a) * frac[k];
        }
}
