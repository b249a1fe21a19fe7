// mcx_host_samples.hpp -- the thinned sample store's host side (mcmcx_set_samples): the rule, the store's allocation, the keep between two
// launches, the window checks and launches of the two read kernels (mcx_samples.hpp).
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

// a getter's window: retained samples s0 .. s0 + ns - 1 of chains c0 .. c0 + nc - 1 (checked on the host, before any launch)
static int samples_check(mcmcx_engine *h, int s0, int ns, int c0, int nc, int layout, const void *out, const char *who)
{
    if (!h) return fail(-1, "null handle");
    if (!h->inited) return fail(-40, "we have not inited");
    if (!out) return fail(-1, std::string(who) + ": null argument");
    const SamplePlan &s = h->samp;
    const long long have = samples_retained(h);
    if (s.thin <= 0) return fail(-48, std::string(who) + ": no samples are kept (mcmcx_set_samples before mcmcx_init)");
    if (layout != 0 && layout != 1) return fail(-48, std::string(who) + ": layout must be 0 ([ns][nc][nfields]) or 1 ([ns][nfields][nc])");
    if (s0 < 0 || ns < 1 || (long long)s0 + ns > have) return fail(-48, std::string(who) + ": samples " + std::to_string(s0) + " .. " +
        std::to_string((long long)s0 + ns - 1) + " asked for, " + std::to_string(have) + " retained");
    if (c0 < 0 || nc < 1 || (long long)c0 + nc > h->cfg.nchains) return fail(-48, std::string(who) + ": chains " + std::to_string(c0) +
        " .. " + std::to_string((long long)c0 + nc - 1) + " asked for, nchains = " + std::to_string(h->cfg.nchains));
    return 0;
}

// ... into dev_out ([ns][nc][nfields] or [ns][nfields][nc] doubles), asynchronous on the engine's stream
static int samples_read(mcmcx_engine *h, int s0, int ns, int c0, int nc, int layout, double *dev_out)
{
    const SamplePlan &s = h->samp;
    const long long have = samples_retained(h);
    HIPCHK(hipSetDevice(h->cfg.device));
    const int nf = samples_nfields(h);
    const unsigned tw = (unsigned)((c0 + nc - 1) / 64 - c0 / 64 + 1), sg = (unsigned)std::min(ns, 65535);
    const unsigned fg = (unsigned)((nf + 4 * SAMP_KR - 1) / (4 * SAMP_KR));
    const size_t slot0 = (size_t)((s.kept - have + s0) % s.capacity);
    if (layout == 1) hipLaunchKernelGGL(samples_read_rows_kernel, dim3(tw, fg, sg), dim3(256), 0, h->stream, (const double *)s.store,
        dev_out, slot0, (size_t)s.capacity, h->ntiles, nf, ns, c0, nc);
    else hipLaunchKernelGGL(samples_read_chains_kernel, dim3(tw, sg), dim3(256), 0, h->stream, (const double *)s.store, dev_out, slot0,
        (size_t)s.capacity, h->ntiles, nf, ns, c0, nc);
    HIPCHK(hipGetLastError());
    return 0;
}
