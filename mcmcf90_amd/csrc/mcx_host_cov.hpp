// mcx_host_cov.hpp -- the sample store's posterior covariance, host side (mcmcx_samples_cov / _dev / _finish, mcmcx_debug_samples_cov):
// its own refusals, its layout of the readers' scratch, the launches of mcx_cov.hpp's kernels, and the finish -- pure host arithmetic on
// a cov vector.  The window, the scratch, the shift and the tree launch are mcx_host_samples.hpp's.
// Part of the ONE translation unit mcx_api.hip (included there after mcx_host_quant.hpp); not a stand-alone header.

static size_t cov_row_len(int nfields) { return (size_t)nfields + (size_t)nfields * (size_t)(nfields + 1) / 2; }
static size_t cov_vec_len(int nfields) { return 1 + (size_t)nfields + cov_row_len(nfields); }
// doubles of the scratch: [ntiles][row] tile rows, shift[nfields], one cov vector (the host form's staging)
static size_t cov_scratch_len(int ntiles, int nfields)
{
    return (size_t)ntiles * cov_row_len(nfields) + (size_t)nfields + cov_vec_len(nfields);
}

// every refusal is -51, on the host, before anything is launched or allocated
static int cov_check(mcmcx_engine *h, int s0, int ns, const void *out, const char *who)
{
    if (!h) return fail(-51, std::string(who) + ": null handle");
    if (!out) return fail(-51, std::string(who) + ": null output");
    return samples_window_check(h, s0, ns, -51, 1, who);
}

// The cov vector of window W (scratch w of cov_scratch_len doubles) into dev_out; asynchronous on `stream`.  shift: host memory or
// nullptr (chain 0 of window sample 0).
static int cov_launch(const SampleWin &W, double *w, const double *shift, double *dev_out, hipStream_t stream)
{
    const int nf = W.nfields, T = W.ntiles;
    const size_t len = cov_row_len(nf);
    double *rows = w, *dshift = rows + (size_t)T * len;
    int rc = samples_shift(W, shift, dshift, stream); if (rc) return rc;
    CovArgs A;
    A.store = W.store; A.shift = dshift; A.out = rows; A.slot0 = W.slot0; A.cap = W.cap;
    A.ntiles = T; A.nfields = nf; A.nchains = W.nchains; A.ns = W.ns;
    const int nblk = (nf + 1 + 15) / 16;                        // 16-row blocks of the fields and the row of ones
    const dim3 block(64);
    if (nblk <= 4) {                                            // form A: the whole upper block triangle in one wave
        const dim3 grid((unsigned)T);
        if (nblk == 1) hipLaunchKernelGGL((cov_tile_kernel<1, false>), grid, block, 0, stream, A);
        else if (nblk == 2) hipLaunchKernelGGL((cov_tile_kernel<2, false>), grid, block, 0, stream, A);
        else if (nblk == 3) hipLaunchKernelGGL((cov_tile_kernel<3, false>), grid, block, 0, stream, A);
        else hipLaunchKernelGGL((cov_tile_kernel<4, false>), grid, block, 0, stream, A);
    } else {                                                    // form B: super-blocks of two, their diagonal and their pairs
        const int nsup = (nblk + 1) / 2;
        hipLaunchKernelGGL((cov_tile_kernel<2, false>), dim3((unsigned)T, (unsigned)nsup), block, 0, stream, A);
        hipLaunchKernelGGL((cov_tile_kernel<4, true>), dim3((unsigned)T, (unsigned)(nsup * (nsup - 1) / 2)), block, 0, stream, A);
    }
    // the length is a size_t at real sizes only in bytes: nfields <= 2047 keeps it an int (the store's nfields is far below)
    const int ilen = (int)len, vlen = (int)cov_vec_len(nf);
    moments_tree_launch(stream, rows, T, ilen, nullptr);
    hipLaunchKernelGGL(cov_pack_kernel, dim3((unsigned)((vlen + 255) / 256)), dim3(256), 0, stream, (const double *)rows,
        (const double *)dshift, dev_out, nf, ilen, (double)((int64_t)W.ns * (int64_t)W.nchains));
    HIPCHK(hipGetLastError());
    return 0;
}

// the cov vector of the engine's window into dev_out (nullptr: the scratch's staging vector, returned in *staged)
static int cov_engine(mcmcx_engine *h, int s0, int ns, const double *shift, double *dev_out, double **staged)
{
    HIPCHK(hipSetDevice(h->cfg.device));
    const SampleWin W = samples_window(h, s0, ns);
    const size_t need = cov_scratch_len(W.ntiles, W.nfields);
    int rc = samples_scratch(h, need * sizeof(double)); if (rc) return rc;
    double *w = (double *)h->d_scratch;
    if (!dev_out) dev_out = w + need - cov_vec_len(W.nfields);
    if (staged) *staged = dev_out;
    return cov_launch(W, w, shift, dev_out, h->stream);
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
