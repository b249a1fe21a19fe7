// mcx_host_bm.hpp -- the sample store's batch-means covariance, host side (mcmcx_samples_cov_bm / _dev, mcmcx_debug_samples_cov_bm) and
// its two finishes, the multivariate ESS and the multivariate split-R-hat (mcmcx_samples_mess, mcmcx_samples_mpsrf): the refusals, the
// launches of mcx_bm.hpp's kernels, and pure host arithmetic on a cov vector and a batch-means vector.  The window, the scratch, a reader's
// prologue and the shift are mcx_host_samples.hpp's; the vector's layout, its scratch, the launches around the tile kernel (form, grids,
// tree, pack) and its finish formulas are mcx_host_cov.hpp's.
// Part of the ONE translation unit mcx_api.hip (included there after mcx_host_cov.hpp); not a stand-alone header.

// every refusal is -55, on the host, before anything is launched or allocated
static int bm_check(mcmcx_engine *h, int s0, int ns, int batch, const void *out, const char *who)
{
    if (!h) return fail(-55, std::string(who) + ": null handle");
    if (!out) return fail(-55, std::string(who) + ": null output");
    int rc = samples_window_check(h, s0, ns, -55, 1, who); if (rc) return rc;
    if (batch < 1 || batch > ns) return fail(-55, std::string(who) + ": a batch of " + std::to_string(batch) + " samples, 1 .. ns = " +
        std::to_string(ns) + " it must be");
    return 0;
}

// The batch-means vector of window W (scratch w as cov_launch's) into dev_out; asynchronous on `stream`.  shift: host memory or nullptr
// (chain 0 of window sample 0).  1 <= batch <= W.ns; the last W.ns - nb batch samples are not read.
static int bm_launch(const SampleWin &W, int batch, double *w, const double *shift, double *dev_out, hipStream_t stream)
{
    const int nb = W.ns / batch;
    double *rows = w, *dshift = rows + (size_t)W.ntiles * cov_row_len(W.nfields);
    int rc = samples_shift(W, shift, dshift, stream); if (rc) return rc;
    BmArgs A;
    A.store = W.store; A.shift = dshift; A.out = rows; A.slot0 = W.slot0; A.cap = W.cap;
    A.ntiles = W.ntiles; A.nfields = W.nfields; A.nchains = W.nchains; A.ns = nb * batch; A.batch = batch;
    return cov_tiles_launch(W.nfields, W.ntiles, rows, dshift, (double)((int64_t)nb * (int64_t)W.nchains), dev_out, stream,
        [&](auto ns, auto off, dim3 grid) {
            hipLaunchKernelGGL((bm_tile_kernel<decltype(ns)::value, decltype(off)::value>), grid, dim3(64), 0, stream, A);
        });
}

// mcmcx_samples_cov_bm and its _dev form: the refusals, then the batch-means vector of the engine's window into dev_out or, host_out
// given, into the scratch's staging vector and from there
static int bm_run(mcmcx_engine *h, int s0, int ns, int batch, const double *shift, void *dev_out, double *host_out, const char *who)
{
    int rc = bm_check(h, s0, ns, batch, dev_out ? dev_out : host_out, who); if (rc) return rc;
    const size_t work = cov_work_len(h->ntiles, samples_nfields(h)), vlen = cov_vec_len(samples_nfields(h));
    return samples_run<double>(h, s0, ns, work + vlen, work, vlen, dev_out, host_out, [&](const SampleWin &W, double *w, double *out) {
        return bm_launch(W, batch, w, shift, out, h->stream);
    });
}

// ---- the finishes (include/mcmcx.h states them): pure host, no handle, no device
// what both refuse of their arguments
static int bm_finish_check(const double *cov_vec, const double *bm_vec, int nf, int nsel, const int32_t *sel, const double *out4,
                           const char *who)
{
    if (!cov_vec || !bm_vec || !sel || !out4) return fail(-55, std::string(who) + ": null argument");
    if (nf < 1) return fail(-55, std::string(who) + ": nfields < 1");
    if (nsel < 1 || nsel > nf) return fail(-55, std::string(who) + ": nsel outside 1 .. nfields");
    for (int j = 0; j < nsel; ++j)
        if (sel[j] < 0 || sel[j] >= nf) return fail(-55, std::string(who) + ": sel[" + std::to_string(j) + "] outside 0 .. nfields - 1");
    for (const double n : {cov_vec[0], bm_vec[0]})
        if (!(n >= 2.0) || n != std::floor(n)) return fail(-55, std::string(who) + ": a vector's n must be an integer of at least 2");
    return 0;
}

// A[sel, sel] column-major m x m, A_jk = (G_jk - S_j * S_k / n) / den of a vector [n, shift, S, G packed]
static void bm_moment(const double *vec, int nf, int m, const int32_t *sel, double den, std::vector<double> &A)
{
    const double n = vec[0], *S = vec + 1 + nf, *G = S + nf;
    A.assign((size_t)m * m, 0.0);
    for (int a = 0; a < m; ++a)
        for (int b = 0; b < m; ++b) {
            const int j = std::min(sel[a], sel[b]), k = std::max(sel[a], sel[b]);
            A[(size_t)b * m + a] = (G[cov_pair((size_t)j, (size_t)k, (size_t)nf)] - S[j] * S[k] / n) / den;
        }
}

// The upper Cholesky factor R (A = R' R) column by column, sums ascending, no fma; A and R column-major m x m, R's lower part zero.
// 0, or j + 1 at the first pivot that is not > 0 (R is then unfinished).  T = double is the header's loop; long double is lambda1's
template <class T>
static int bm_chol(int m, const std::vector<T> &A, std::vector<T> &R)
{
    R.assign((size_t)m * m, (T)0);
    for (int j = 0; j < m; ++j) {
        for (int i = 0; i < j; ++i) {
            T t = 0;
            for (int k = 0; k < i; ++k) t = t + R[(size_t)i * m + k] * R[(size_t)j * m + k];
            R[(size_t)j * m + i] = (A[(size_t)j * m + i] - t) / R[(size_t)i * m + i];
        }
        T t = 0;
        for (int k = 0; k < j; ++k) t = t + R[(size_t)j * m + k] * R[(size_t)j * m + k];
        const T p = A[(size_t)j * m + j] - t;
        if (!(p > (T)0)) return j + 1;
        R[(size_t)j * m + j] = std::sqrt(p);
    }
    return 0;
}

// 2 sum log r_jj, summed ascending
static double bm_logdet(int m, const std::vector<double> &R)
{
    double s = 0.0;
    for (int j = 0; j < m; ++j) s = s + std::log(R[(size_t)j * m + j]);
    return 2.0 * s;
}

static int bm_mess(const double *cov_vec, const double *bm_vec, int nf, int batch, int m, const int32_t *sel, double *out4, double *ess)
{
    const double n = cov_vec[0], qn = std::nan("");
    std::vector<double> L, Sg, R;
    bm_moment(cov_vec, nf, m, sel, n - 1.0, L);
    bm_moment(bm_vec, nf, m, sel, bm_vec[0] - 1.0, Sg);
    for (double &x : Sg) x = (double)batch * x;
    if (ess) for (int j = 0; j < m; ++j) ess[j] = n * L[(size_t)j * m + j] / Sg[(size_t)j * m + j];
    const double ldl = bm_chol(m, L, R) ? qn : bm_logdet(m, R);
    const double lds = bm_chol(m, Sg, R) ? qn : bm_logdet(m, R);
    out4[0] = n * std::exp((ldl - lds) / (double)m); out4[1] = n; out4[2] = ldl; out4[3] = lds;
    return (ldl != ldl || lds != lds) ? 1 : 0;
}

static int bm_mpsrf(const double *cov_vec, const double *bm_vec, int nf, int n_h, int m, const int32_t *sel, double *out4, double *W_out,
                    double *Bn_out)
{
    const double M = bm_vec[0], nh = (double)n_h, qn = std::nan("");
    std::vector<double> Tm, SSm, W((size_t)m * m), Bn((size_t)m * m), R;
    bm_moment(cov_vec, nf, m, sel, 1.0, Tm);
    bm_moment(bm_vec, nf, m, sel, 1.0, SSm);
    for (size_t e = 0; e < W.size(); ++e) { W[e] = (Tm[e] - nh * SSm[e]) / (M * (nh - 1.0)); Bn[e] = SSm[e] / (M - 1.0); }
    if (W_out) std::copy(W.begin(), W.end(), W_out);
    if (Bn_out) std::copy(Bn.begin(), Bn.end(), Bn_out);
    out4[0] = out4[1] = qn; out4[2] = M; out4[3] = nh;
    if (bm_chol(m, W, R)) return 1;
    // lambda1 of C = R^-T Bn R^-1.  The reduction loses cond(W) u of lambda1 in any working precision, and the marginal R-hats it is read
    // beside carry n u: it is carried in long double (the factor again, X = R^-T Bn by forward substitution down every column of Bn,
    // C = X R^-1 by forward substitution along every row of X, the upper triangle computed and mirrored), the cyclic Jacobi of the rounded
    // C gives the eigenvector u, and lambda1 = u' C u / u' u: the Rayleigh quotient is second order in u's error
    typedef long double ld;
    std::vector<ld> Wl(W.begin(), W.end()), Rl, X((size_t)m * m), Cl((size_t)m * m);
    double l1 = qn;
    bool finite = bm_chol(m, Wl, Rl) == 0;
    for (int c = 0; finite && c < m; ++c)
        for (int i = 0; i < m; ++i) {
            ld t = 0;
            for (int k = 0; k < i; ++k) t = t + Rl[(size_t)i * m + k] * X[(size_t)c * m + k];
            X[(size_t)c * m + i] = ((ld)Bn[(size_t)c * m + i] - t) / Rl[(size_t)i * m + i];
        }
    for (int i = 0; finite && i < m; ++i)
        for (int j = i; j < m; ++j) {
            ld t = 0;                                           // row i of C left of the diagonal: the mirrored entries
            for (int k = 0; k < j; ++k) t = t + Cl[(size_t)k * m + i] * Rl[(size_t)j * m + k];
            const ld c = (X[(size_t)j * m + i] - t) / Rl[(size_t)j * m + j];
            Cl[(size_t)j * m + i] = c; Cl[(size_t)i * m + j] = c;
        }
    std::vector<double> Cm(Cl.begin(), Cl.end()), V, sv;
    for (const double c : Cm) finite = finite && std::isfinite(c);
    if (finite) {
        std::vector<double> u(m, 1.0);
        if (m > 1) { host_symsvd(m, Cm, V, sv); std::copy(V.begin(), V.begin() + m, u.begin()); }    // the largest singular value's vector
        ld num = 0, den = 0;
        for (int a = 0; a < m; ++a) {
            ld t = 0;
            for (int b = 0; b < m; ++b) t = t + Cl[(size_t)b * m + a] * (ld)u[b];
            num = num + (ld)u[a] * t; den = den + (ld)u[a] * (ld)u[a];
        }
        l1 = (double)(num / den);
    }
    out4[0] = std::sqrt((nh - 1.0) / nh + l1); out4[1] = l1;
    return l1 != l1 ? 1 : 0;
}
