// mcx_host_samples.hpp -- the thinned sample store's host side (mcmcx_set_samples): the rule, the store's allocation, the keep between two
// launches, the window checks and launches of the two read kernels (mcx_samples.hpp) -- and what every reader of the ring shares
// (mcx_host_diag.hpp, mcx_host_quant.hpp, mcx_host_hist.hpp, mcx_host_diag_step.hpp, mcx_host_cov.hpp, mcx_host_bm.hpp): the window as a
// launch argument, its refusals, the one scratch, a reader's prologue, the default shift, the staging of keys, the launch of the pooled
// moment tree, the host form of a staged result and the debug probes' own store.
// Part of the ONE translation unit mcx_api.hip (included there after mcx_host_launch.hpp); not a stand-alone header.

// Iteration it is kept: a function of the configuration alone -- the same on every rank, no collective behind it.  thin = 0: never.
static bool sample_due(const mcmcx_engine *h, int it)
{
    const SamplePlan &s = h->samp;
    return s.thin > 0 && it >= s.first && (it - s.first) % s.thin == 0;
}

static int samples_nfields(const mcmcx_engine *h) { return h->d + 2 * h->ny + 1; }

// the ring, with the engine's other device state (mcmcx_init); not cleared: a slot is read only after it was kept
static int samples_alloc(mcmcx_engine *h)
{
    SamplePlan &s = h->samp;
    s.kept = 0; s.store = nullptr;
    if (s.thin <= 0) return 0;
    return dev_alloc(h, &s.store, (size_t)s.capacity * (size_t)h->ntiles * (size_t)samples_nfields(h) * 64, false);
}

// Keep the state as iteration `it` left it, on the engine's stream behind the launch (and the tick's adaptation, which does not move
// theta) that ended there.  The slot is a launch argument -- no counter lives on the device -- and follows from `it` alone.
static int samples_keep(mcmcx_engine *h, int it)
{
    SamplePlan &s = h->samp;
    const long long n = (long long)(it - s.first) / s.thin;                 // kept before this one
    const int nf = samples_nfields(h);
    hipLaunchKernelGGL(samples_keep_kernel, dim3((unsigned)h->ntiles, (unsigned)((nf + 4 * SAMP_KR - 1) / (4 * SAMP_KR))), dim3(256), 0,
        h->stream, h->E, s.store, (size_t)(n % s.capacity), nf);
    HIPCHK(hipGetLastError());
    s.kept = n + 1;
    return 0;
}

static long long samples_retained(const mcmcx_engine *h) { return std::min<long long>(h->samp.kept, h->samp.capacity); }

// The window of retained samples s0 .. s0 + ns - 1 as the readers' launch argument: the ONE place that knows where it lies in the ring
static SampleWin samples_window(const mcmcx_engine *h, int s0, int ns)
{
    const SamplePlan &s = h->samp;
    SampleWin W;
    W.store = s.store; W.slot0 = (size_t)((s.kept - samples_retained(h) + s0) % s.capacity); W.cap = (size_t)s.capacity;
    W.ntiles = h->ntiles; W.nfields = samples_nfields(h); W.nchains = h->cfg.nchains; W.ns = ns;
    return W;
}

// The refusals of a window that every reader shares, after its own (`code`: the reader's refusal code, min_ns: its shortest window), on the
// host, before anything is launched or allocated.  h is not null.
static int samples_window_check(const mcmcx_engine *h, int s0, int ns, int code, int min_ns, const char *who)
{
    if (!h->inited) return fail(code, std::string(who) + ": we have not inited");
    if (h->samp.thin <= 0) return fail(code, std::string(who) + ": no samples are kept (mcmcx_set_samples before mcmcx_init)");
    if (ns < min_ns) return fail(code, std::string(who) + ": a window of " + std::to_string(ns) + " samples, " + std::to_string(min_ns) +
        " at least");
    const long long have = samples_retained(h);
    if (s0 < 0 || (long long)s0 + ns > have) return fail(code, std::string(who) + ": samples " + std::to_string(s0) + " .. " +
        std::to_string((long long)s0 + ns - 1) + " asked for, " + std::to_string(have) + " retained");
    return 0;
}

// a getter's window: retained samples s0 .. s0 + ns - 1 of chains c0 .. c0 + nc - 1 (checked on the host, before any launch)
static int samples_check(mcmcx_engine *h, int s0, int ns, int c0, int nc, int layout, const void *out, const char *who)
{
    if (!h) return fail(-1, "null handle");
    if (!h->inited) return fail(-40, "we have not inited");
    if (!out) return fail(-1, std::string(who) + ": null argument");
    // (a store that keeps nothing is refused before the layout is looked at)
    if (h->samp.thin > 0 && layout != 0 && layout != 1) return fail(-48, std::string(who) + ": layout must be 0 ([ns][nc][nfields]) or 1 "
        "([ns][nfields][nc])");
    int rc = samples_window_check(h, s0, ns, -48, 1, who); if (rc) return rc;
    if (c0 < 0 || nc < 1 || (long long)c0 + nc > h->cfg.nchains) return fail(-48, std::string(who) + ": chains " + std::to_string(c0) +
        " .. " + std::to_string((long long)c0 + nc - 1) + " asked for, nchains = " + std::to_string(h->cfg.nchains));
    return 0;
}

// ... into dev_out ([ns][nc][nfields] or [ns][nfields][nc] doubles), asynchronous on the engine's stream
static int samples_read(mcmcx_engine *h, int s0, int ns, int c0, int nc, int layout, double *dev_out)
{
    HIPCHK(hipSetDevice(h->cfg.device));
    const SampleWin W = samples_window(h, s0, ns);
    const int nf = W.nfields;
    const unsigned tw = (unsigned)((c0 + nc - 1) / 64 - c0 / 64 + 1), sg = (unsigned)std::min(ns, 65535);
    const unsigned fg = (unsigned)((nf + 4 * SAMP_KR - 1) / (4 * SAMP_KR));
    if (layout == 1) hipLaunchKernelGGL(samples_read_rows_kernel, dim3(tw, fg, sg), dim3(256), 0, h->stream, W.store, dev_out, W.slot0,
        W.cap, W.ntiles, nf, ns, c0, nc);
    else hipLaunchKernelGGL(samples_read_chains_kernel, dim3(tw, sg), dim3(256), 0, h->stream, W.store, dev_out, W.slot0, W.cap, W.ntiles,
        nf, ns, c0, nc);
    HIPCHK(hipGetLastError());
    return 0;
}

// ---- what the readers of the ring share
// The readers' scratch, h->d_scratch: allocated at the first call, grows only, freed by mcmcx_destroy; every reader carves its own layout
// out of it (tile rows, shift, tables, the host form's staging vector).  ONE for all of them is sound because every reader works on
// h->stream alone, which is fixed at mcmcx_init: a later call's kernels run behind an earlier call's, whichever reader it was, and a host
// form synchronises the stream before it returns, so nothing reads a staging vector after the next call may write there.
static int samples_scratch(mcmcx_engine *h, size_t bytes)
{
    if (bytes <= h->scratch_cap) return 0;
    HIPCHK(hipStreamSynchronize(h->stream));                    // an earlier call may still use the old one
    if (h->d_scratch) (void)hipFree(h->d_scratch);
    h->d_scratch = nullptr; h->scratch_cap = 0;
    const hipError_t e = hipMalloc(&h->d_scratch, bytes);
    if (e != hipSuccess) {
        h->d_scratch = nullptr;
        return fail(-101, "hipMalloc of " + std::to_string(bytes) + " bytes: " + hipGetErrorString(e));
    }
    h->scratch_cap = bytes;
    return 0;
}

// the host form of a result a launch left in device memory at `staged`
static int samples_fetch(mcmcx_engine *h, void *host_out, const void *staged, size_t bytes)
{
    HIPCHK(hipStreamSynchronize(h->stream));
    HIPCHK(hipMemcpy(host_out, staged, bytes, hipMemcpyDeviceToHost));
    return 0;
}

// What every reader's entry does once its refusals are past: the device, the window, the scratch grown to `need` words of T, the reader's
// launch(window, scratch, out) with out the caller's dev_out or, host_out given (a host form: dev_out is null), the staging area the
// reader names -- `len` words at word stage_at of its layout -- and then the staged result to the host.
template <class T, class L>
static int samples_run(mcmcx_engine *h, int s0, int ns, size_t need, size_t stage_at, size_t len, void *dev_out, void *host_out, L &&launch)
{
    HIPCHK(hipSetDevice(h->cfg.device));
    const SampleWin W = samples_window(h, s0, ns);
    int rc = samples_scratch(h, need * sizeof(T)); if (rc) return rc;
    T *w = (T *)h->d_scratch, *out = dev_out ? (T *)dev_out : w + stage_at;
    if ((rc = launch(W, w, out)) || !host_out) return rc;
    return samples_fetch(h, host_out, out, len * sizeof(T));
}

// shift[nfields] of a reduction into dshift: the caller's (host memory) or, shift == nullptr, chain 0 of window sample 0
static int samples_shift(const SampleWin &W, const double *shift, double *dshift, hipStream_t stream)
{
    const int nf = W.nfields;
    if (shift) HIPCHK(hipMemcpyAsync(dshift, shift, (size_t)nf * sizeof(double), hipMemcpyHostToDevice, stream));
    else hipLaunchKernelGGL(diag_shift_kernel, dim3((unsigned)((nf + 255) / 256)), dim3(256), 0, stream, W.store, dshift, W.slot0, W.ntiles,
        nf);
    return 0;
}

// dst[i] = quant_key(the bits of src[i]) (src: host memory, edges or thresholds), asynchronous on `stream`.  From pageable memory a copy is
// staged before it returns: the keys here, and whatever else a reader copies up from a caller's array, need only live until then.
static int samples_stage_keys(unsigned long long *dst, const double *src, size_t count, hipStream_t stream)
{
    std::vector<unsigned long long> keys(count);
    for (size_t i = 0; i < count; ++i) { unsigned long long b; memcpy(&b, src + i, 8); keys[i] = quant_key(b); }
    HIPCHK(hipMemcpyAsync(dst, keys.data(), count * sizeof(unsigned long long), hipMemcpyHostToDevice, stream));
    return 0;
}

// The T tile rows of `len` doubles in `rows` summed into row 0 (and into dst, if given) by the fixed pairwise tree of
// moments_tree_kernel (mcx_moments.hpp has its definition), six levels per launch: the pooled moments, the summary and the covariance
static void moments_tree_launch(hipStream_t stream, double *rows, int T, int len, double *dst)
{
    for (long long stride = 1;; stride *= 64) {
        const long long groups = (T + 64 * stride - 1) / (64 * stride);
        hipLaunchKernelGGL(moments_tree_kernel, dim3((unsigned)((len + 255) / 256), (unsigned)groups), dim3(256), 0, stream, rows, T, len,
                           (int)stride, dst);
        if (groups == 1) break;
    }
}

// A debug probe's own store (mcmcx_debug_samples_*; tests only): ns slots of ceil(nchains / 64) tiles and nfields fields filled from
// values[ns][nfields][nchains] through samples_row, the padding lanes of the last tile NaN -- which a kernel that did not mask them would
// sum, count or spread --, and a scratch of the reader's own layout beside it.  The probes work on stream 0; both buffers are freed
// with the struct.
struct DebugStore {
    DevBufs g;
    SampleWin win;
    void *scratch = nullptr;

    int open(int device, int nchains, int nfields, int ns, const double *values, size_t scratch_bytes)
    {
        int ndev = 0;
        if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) return fail(-10, "no HIP device: the mcmcx engine has no CPU fallback");
        HIPCHK(hipSetDevice(device));
        const int T = (nchains + 63) / 64;
        const size_t words = (size_t)ns * (size_t)T * (size_t)nfields * 64;
        std::vector<double> host(words, std::nan(""));
        for (int s = 0; s < ns; ++s)
            for (int f = 0; f < nfields; ++f)
                for (int c = 0; c < nchains; ++c)
                    host[samples_row((size_t)s, (size_t)T, (size_t)nfields, (size_t)(c / 64), (size_t)f) + (size_t)(c % 64)] =
                        values[((size_t)s * (size_t)nfields + (size_t)f) * (size_t)nchains + (size_t)c];
        double *store = nullptr;
        HIPCHK(g.alloc(&store, words * 8)); HIPCHK(g.alloc(&scratch, scratch_bytes));
        HIPCHK(hipMemcpy(store, host.data(), words * 8, hipMemcpyHostToDevice));
        win = {store, 0, (size_t)ns, T, nfields, nchains, ns};
        return 0;
    }

    // what a launch on stream 0 left at `src`, to the host
    int fetch(void *out, const void *src, size_t bytes)
    {
        HIPCHK(hipStreamSynchronize(0));
        HIPCHK(hipMemcpy(out, src, bytes, hipMemcpyDeviceToHost));
        return 0;
    }
};
