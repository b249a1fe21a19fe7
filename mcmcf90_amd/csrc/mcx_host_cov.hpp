// mcx_host_cov.hpp -- the sample store's posterior covariance, host side (mcmcx_samples_cov / _dev / _finish, mcmcx_debug_samples_cov):
// its own refusals, its layout of the readers' scratch, the launches of mcx_cov.hpp's kernels -- the choice of their form, the grids, the
// tree and the pack for the batch-means covariance (mcx_host_bm.hpp) too -- and the finish, pure host arithmetic on a cov vector.  The
// window, the scratch, a reader's prologue, the shift and the tree launch are mcx_host_samples.hpp's.
// Part of the ONE translation unit mcx_api.hip (included there after mcx_host_quant.hpp); not a stand-alone header.

static size_t cov_row_len(int nfields) { return (size_t)nfields + (size_t)nfields * (size_t)(nfields + 1) / 2; }
static size_t cov_vec_len(int nfields) { return 1 + (size_t)nfields + cov_row_len(nfields); }
// doubles of the scratch before the one cov vector at its end (the host form's staging): [ntiles][row] tile rows, shift[nfields]
static size_t cov_work_len(int ntiles, int nfields) { return (size_t)ntiles * cov_row_len(nfields) + (size_t)nfields; }

// every refusal is -51, on the host, before anything is launched or allocated
static int cov_check(mcmcx_engine *h, int s0, int ns, const void *out, const char *who)
{
    if (!h) return fail(-51, std::string(who) + ": null handle");
    if (!out) return fail(-51, std::string(who) + ": null output");
    return samples_window_check(h, s0, ns, -51, 1, who);
}

// The launches of a covariance over the tiles of a store of nf fields, the batch-means covariance's too: `tile` launches the caller's
// kernel<NS, OFF> on a grid it is handed (NS and OFF as std::integral_constant, compile-time values), then the tree over the tile rows
// and the vector [n, shift, S, G] packed into dev_out.  Asynchronous on `stream`.
template <class L>
static int cov_tiles_launch(int nf, int T, double *rows, const double *dshift, double n, double *dev_out, hipStream_t stream, L &&tile)
{
    using std::integral_constant;
    typedef integral_constant<bool, false> diag;
    const int nblk = (nf + 1 + 15) / 16;                        // 16-row blocks of the fields and the row of ones
    const dim3 grid((unsigned)T);
    if (nblk == 1) tile(integral_constant<int, 1>(), diag(), grid);     // form A: the whole upper block triangle in one wave
    else if (nblk == 2) tile(integral_constant<int, 2>(), diag(), grid);
    else if (nblk == 3) tile(integral_constant<int, 3>(), diag(), grid);
    else if (nblk <= 4) tile(integral_constant<int, 4>(), diag(), grid);
    else {                                                      // form B: super-blocks of two, their diagonal and their pairs
        const int nsup = (nblk + 1) / 2;
        tile(integral_constant<int, 2>(), diag(), dim3((unsigned)T, (unsigned)nsup));
        tile(integral_constant<int, 4>(), integral_constant<bool, true>(), dim3((unsigned)T, (unsigned)(nsup * (nsup - 1) / 2)));
    }
    // the length is a size_t at real sizes only in bytes: nfields <= 2047 keeps it an int (the store's nfields is far below)
    const int ilen = (int)cov_row_len(nf), vlen = (int)cov_vec_len(nf);
    moments_tree_launch(stream, rows, T, ilen, nullptr);
    hipLaunchKernelGGL(cov_pack_kernel, dim3((unsigned)((vlen + 255) / 256)), dim3(256), 0, stream, (const double *)rows, dshift, dev_out,
        nf, ilen, n);
    HIPCHK(hipGetLastError());
    return 0;
}

// The cov vector of window W (scratch w: cov_work_len doubles and, where dev_out lies there, the vector) into dev_out; asynchronous on
// `stream`.  shift: host memory or nullptr (chain 0 of window sample 0).
static int cov_launch(const SampleWin &W, double *w, const double *shift, double *dev_out, hipStream_t stream)
{
    double *rows = w, *dshift = rows + (size_t)W.ntiles * cov_row_len(W.nfields);
    int rc = samples_shift(W, shift, dshift, stream); if (rc) return rc;
    CovArgs A;
    A.store = W.store; A.shift = dshift; A.out = rows; A.slot0 = W.slot0; A.cap = W.cap;
    A.ntiles = W.ntiles; A.nfields = W.nfields; A.nchains = W.nchains; A.ns = W.ns;
    return cov_tiles_launch(W.nfields, W.ntiles, rows, dshift, (double)((int64_t)W.ns * (int64_t)W.nchains), dev_out, stream,
        [&](auto ns, auto off, dim3 grid) {
            hipLaunchKernelGGL((cov_tile_kernel<decltype(ns)::value, decltype(off)::value>), grid, dim3(64), 0, stream, A);
        });
}

// mcmcx_samples_cov and its _dev form: the refusals, then the cov vector of the engine's window into dev_out or, host_out given, into the
// scratch's staging vector and from there
static int cov_run(mcmcx_engine *h, int s0, int ns, const double *shift, void *dev_out, double *host_out, const char *who)
{
    int rc = cov_check(h, s0, ns, dev_out ? dev_out : host_out, who); if (rc) return rc;
    const size_t work = cov_work_len(h->ntiles, samples_nfields(h)), vlen = cov_vec_len(samples_nfields(h));
    return samples_run<double>(h, s0, ns, work + vlen, work, vlen, dev_out, host_out, [&](const SampleWin &W, double *w, double *out) {
        return cov_launch(W, w, shift, out, h->stream);
    });
}

// The finish (include/mcmcx.h states it): mean[nf], cov and corr column-major nf x nf (corr may be null)
static int cov_finish(const double *vec, int nf, double *mean, double *cov, double *corr)
{
    const double n = vec[0];
    // the header is a caller's (perhaps a sum over ranks): checked as a double before anything is computed with it
    if (!(n >= 2.0) || n != std::floor(n)) return fail(-51, "mcmcx_samples_cov_finish: the vector's n must be an integer of at least 2");
    const double *shift = vec + 1, *S = shift + nf, *G = S + nf;
    for (int j = 0; j < nf; ++j) mean[j] = shift[j] + S[j] / n;
    for (int j = 0; j < nf; ++j)
        for (int k = j; k < nf; ++k) {
            const double c = (G[cov_pair((size_t)j, (size_t)k, (size_t)nf)] - S[j] * S[k] / n) / (n - 1.0);
            cov[(size_t)k * nf + j] = c; cov[(size_t)j * nf + k] = c;
        }
    if (corr)
        for (int j = 0; j < nf; ++j)
            for (int k = 0; k < nf; ++k) {
                const double cjj = cov[(size_t)j * nf + j], ckk = cov[(size_t)k * nf + k];
                if (j == k) corr[(size_t)k * nf + j] = cjj > 0.0 ? 1.0 : cjj / (std::sqrt(cjj) * std::sqrt(cjj));
                else corr[(size_t)k * nf + j] = cov[(size_t)k * nf + j] / (std::sqrt(cjj) * std::sqrt(ckk));
            }
    return 0;
}
