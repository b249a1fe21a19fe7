// mcx_api.hip -- host side of libmcmcx.so: the C ABI of include/mcmcx.h.
//
// Owns the device state of N chains, cuts the iteration range into launches of the
// step kernel separated by the adaptation ticks of MCMC_adapt (MCMC_adapt.F90:40-46),
// and decodes the device history back into the reference's chain/sschain/s2chain
// form.  No CPU fallback: every numerical step of the sampler runs in the HIP kernels
// of mcx_kernels.hpp; without a GPU every entry point that needs one fails.
// ONE translation unit: the host parts below are included in order (engine object, initial factor, kernel selection and
// launchers, the sample store, adaptation tick, pooled mode and communicator, host callbacks); this file holds the extern "C" entry
// points and mcmcx_init's steps.
#include <hip/hip_runtime.h>
#include <csignal>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include <algorithm>
#include "../../include/mcmcx.h"
#include "../../include/mcmcx_target.h"
#include "mcx_kernels.hpp"
#include "mcx_group.hpp"
#include "mcx_group_ram.hpp"

#include "mcx_host_engine.hpp"
#include "mcx_host_linalg.hpp"
#include "mcx_host_launch.hpp"
#include "mcx_host_samples.hpp"
#include "mcx_host_diag.hpp"
#include "mcx_host_quant.hpp"
#include "mcx_host_hist.hpp"
#include "mcx_host_diag_step.hpp"
#include "mcx_host_cov.hpp"
#include "mcx_host_bm.hpp"
#include "mcx_host_adapt.hpp"
#include "mcx_host_pooled.hpp"
#include "mcx_host_callbacks.hpp"

// ------------------------------------------------------------------ C ABI
extern "C" {

const char *mcmcx_last_error(void) { return g_err.c_str(); }
const char *mcmcx_version(void) { return "mcmcx 0.3 (gfx950)"; }
int32_t mcmcx_device_count(void) { int n = 0; return (hipGetDeviceCount(&n) == hipSuccess) ? n : 0; }
int mcmcx_device_info(int32_t device, char *buf, int32_t len)
{
    if (!buf || len < 2) return fail(-1, "mcmcx_device_info: bad argument");
    hipDeviceProp_t prop;
    char bus[64] = "?";
    hipError_t e = hipGetDeviceProperties(&prop, device);
    if (e != hipSuccess) { snprintf(buf, (size_t)len, "device %d: %s", device, hipGetErrorString(e)); return fail(-10, buf); }
    (void)hipDeviceGetPCIBusId(bus, (int)sizeof bus, device);
    snprintf(buf, (size_t)len, "%s %s, pci %s, %d CUs, %.0f GiB", prop.name, prop.gcnArchName, bus, prop.multiProcessorCount,
        (double)prop.totalGlobalMem / (1024.0 * 1024.0 * 1024.0));
    return 0;
}

// what identifies the physical device and its clock limits (bench.py puts it in its JSON line: the pool's boxes differ by ~8 %)
int mcmcx_device_ident(int32_t device, char *uuid_hex, int32_t len, int32_t *out5)
{
    if (!uuid_hex || len < 33 || !out5) return fail(-1, "mcmcx_device_ident: bad argument (uuid buffer of >= 33 bytes, five integers)");
    hipUUID u;
    HIPCHK(hipDeviceGetUuid(&u, device));
    for (int i = 0; i < 16; ++i) snprintf(uuid_hex + 2 * i, 3, "%02x", (unsigned)(unsigned char)u.bytes[i]);
    int v = 0;
    HIPCHK(hipDeviceGetAttribute(&v, hipDeviceAttributeClockRate, device)); out5[0] = v;                 // kHz, the engine clock's limit
    HIPCHK(hipDeviceGetAttribute(&v, hipDeviceAttributeMemoryClockRate, device)); out5[1] = v;           // kHz
    HIPCHK(hipDeviceGetAttribute(&v, hipDeviceAttributeMemoryBusWidth, device)); out5[2] = v;            // bits
    HIPCHK(hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, device)); out5[3] = v;
    HIPCHK(hipDeviceGetAttribute(&v, hipDeviceAttributeL2CacheSize, device)); out5[4] = v;
    return 0;
}

const char *mcmcx_last_kernel(mcmcx_handle h)
{
    static thread_local std::string name;
    name = h ? h->last_kernel : "";
    // template instances are launched as (k<...>)
    if (name.size() >= 2 && name.front() == '(' && name.back() == ')') name = name.substr(1, name.size() - 2);
    return name.c_str();
}

void mcmcx_config_defaults(mcmcx_config *c)                      // mcmcinit.F90:184-230
{
    memset(c, 0, sizeof *c);
    c->npar = 0; c->nchains = 1; c->method = MCMCX_METHOD_DRAM;
    c->nsimu = 0; c->doadapt = 1; c->doburnin = 0; c->burnintime = 0; c->badaptint = -1;
    c->greedy = 0; c->scalelimit = 0.05; c->scalefactor = 2.5; c->drscale = 0.0;
    c->adaptint = 100; c->adapthist = 0; c->adaptend = 0; c->initcmatn = 0;
    c->N0 = 1.0; c->S02 = 0.0; c->updatesigma = 1; c->condmax = 0.0;
    c->alphatarget = 0.234; c->nuparam = 0.7;
    c->seed = MCMCX_DEFAULT_SEED; c->chain_id0 = 0; c->record_accept = 0; c->record_chain = 0; c->device = 0; c->scam_fast = 0;
}

int mcmcx_create(const mcmcx_config *cfg_in, mcmcx_handle *out)
{
    if (!cfg_in || !out) return fail(-1, "mcmcx_create: null argument");
    mcmcx_config c = *cfg_in;
    // check_mcmcinit_parameters, mcmcinit.F90:235-368
    if (c.adapthist < 0) c.adapthist = 0;
    if (c.adaptint < 0) { c.adaptint = 0; c.doadapt = 0; }
    if (c.burnintime < 0) c.burnintime = 0;
    if (c.badaptint <= 0) c.badaptint = c.adaptint;
    if (c.badaptint == 0) c.doburnin = 0;
    if (c.initcmatn < 0) c.initcmatn = 0;
    if (c.scalelimit < 0.0 || c.scalelimit > 0.5)
        return fail(-2, "ERROR: Scalelimit control variable should be between [0,0.5]");
    if (c.scalefactor < 0.0) c.scalefactor = 1.0;
    if (c.method != MCMCX_METHOD_DRAM && c.method != MCMCX_METHOD_RAM && c.method != MCMCX_METHOD_SCAM &&
        c.method != MCMCX_METHOD_ER) return fail(-3, "unknown method");
    if (c.method == MCMCX_METHOD_ER) c.drscale = 0.0;                                // 'no dr with er', MCMC_run_er.F90:26-29
    if (c.method == MCMCX_METHOD_SCAM) {                                             // mcmcinit.F90:321-330
        if (c.condmax <= 0.0) c.condmax = 1.0e15;
        c.doburnin = 0; c.drscale = 0.0;
    }
    if (c.method == MCMCX_METHOD_RAM) c.drscale = 0.0;
    if (c.method != MCMCX_METHOD_SCAM) c.scam_fast = 0;
    if (c.nsimu < 1) return fail(-4, "nsimu <= 0 stopping");                         // mcmc_main.F90:22-25
    if (c.npar < 1 || c.npar > MCX_MAX_NPAR) return fail(-5, "npar must be in 1.." + std::to_string(MCX_MAX_NPAR));
    if (c.nchains < 1) return fail(-5, "nchains must be >= 1");
    if (c.doadapt && c.method != MCMCX_METHOD_RAM) {
        if (c.adaptint == 0) return fail(-7, "doadapt with adaptint = 0");
    }
    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev < 1) return fail(-10, "no HIP device: the mcmcx engine has no CPU fallback");
    if (c.device < 0 || c.device >= ndev) return fail(-10, "bad device ordinal");
    HIPCHK(hipSetDevice(c.device));
    mcmcx_engine *h = new mcmcx_engine();
    h->cfg = c; h->d = c.npar; h->P = c.npar * (c.npar + 1) / 2;
    h->ntiles = (c.nchains + 63) / 64; h->nlanes = h->ntiles * 64;
    h->dodr = (c.drscale > 0.0) ? 1 : 0; h->usesvd = (c.condmax > 0.0) ? 1 : 0; h->pooled = c.pooled ? 1 : 0;
    e = hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking);
    if (e != hipSuccess) { delete h; return fail(-100, hipGetErrorString(e)); }
    h->own_stream = true;
    *out = h;
    return 0;
}

int mcmcx_destroy(mcmcx_handle h)
{
    if (!h) return 0;
    (void)hipSetDevice(h->cfg.device);
    if (h->stream) (void)hipStreamSynchronize(h->stream);
    for (auto &p : h->pending) { (void)hipEventDestroy(p.first); (void)hipEventDestroy(p.second); }
    for (void *p : h->allocs) (void)hipFree(p);
    if (h->d_scratch) (void)hipFree(h->d_scratch);              // the scratch of the sample store's readers (samples_scratch)
    for (void *p : h->hallocs) (void)hipHostFree(p);
    h->h_cand.release(); h->h_ev.release(); h->h_hx.release();
    if (h->own_stream && h->stream) (void)hipStreamDestroy(h->stream);
    if (h->mod) (void)hipModuleUnload(h->mod);
    delete h;
    return 0;
}

int mcmcx_set_stream(mcmcx_handle h, void *s)
{
    if (!h) return fail(-1, "null handle");
    if (h->inited) return fail(-1, "mcmcx_set_stream after mcmcx_init");
    if (h->own_stream && h->stream) (void)hipStreamDestroy(h->stream);
    h->stream = (hipStream_t)s; h->own_stream = false;
    return 0;
}

int mcmcx_set_par0(mcmcx_handle h, const double *p, int32_t n)
{
    if (!h || !p) return fail(-1, "null argument");
    if (n != h->d) return fail(-20, "par0 and npar dont match");                     // MCMC_init.F90:173
    h->par0.assign(p, p + n);
    return 0;
}
// ---- per-chain start points (include/mcmcx.h, "Per-chain start points"): given by the caller, or drawn on the device at mcmcx_init
// (start_spread_kernel).  The later call wins; every refusal is -56 and changes nothing.
static_assert(MCMCX_START_TRIES == START_TRIES, "include/mcmcx.h and mcx_start.hpp disagree about the attempts of a drawn start");
static int start_refused(mcmcx_handle h, const char *who)
{
    if (!h) return fail(-56, std::string(who) + ": null handle");
    if (h->inited) return fail(-56, std::string(who) + " after mcmcx_init (the start points are set there)");
    if (h->external) return fail(-56, std::string(who) + ": not with mcmcx_set_target_external (the caller holds the chains' states)");
    return 0;
}
int mcmcx_set_par0_all(mcmcx_handle h, const double *par0_all, int32_t nchains, int32_t npar)
{
    int rc = start_refused(h, "mcmcx_set_par0_all"); if (rc) return rc;
    if (!par0_all) return fail(-56, "mcmcx_set_par0_all: null array");
    if (nchains != h->cfg.nchains || npar != h->d) return fail(-56, "mcmcx_set_par0_all: the array is [" + std::to_string(nchains) + "]["
        + std::to_string(npar) + "] but the handle has nchains = " + std::to_string(h->cfg.nchains) + ", npar = " + std::to_string(h->d));
    const size_t n = (size_t)nchains * npar;
    for (size_t e = 0; e < n; ++e) if (!std::isfinite(par0_all[e])) return fail(-56, "mcmcx_set_par0_all: a value that is not finite "
        "(chain " + std::to_string(e / npar) + ", parameter " + std::to_string(e % npar) + ")");
    h->start_all.assign(par0_all, par0_all + n);
    h->start_mode = 1;
    return 0;
}
int mcmcx_set_par0_spread(mcmcx_handle h, double scale)
{
    int rc = start_refused(h, "mcmcx_set_par0_spread"); if (rc) return rc;
    if (!std::isfinite(scale) || !(scale > 0.0)) return fail(-56, "mcmcx_set_par0_spread: scale must be finite and > 0");
    h->start_scale = scale;
    h->start_mode = 2;
    std::vector<double>().swap(h->start_all);
    return 0;
}
int mcmcx_start_info(mcmcx_handle h, int64_t *out3)
{
    if (!h || !h->inited) return fail(-40, "we have not inited");
    if (!out3) return fail(-1, "mcmcx_start_info: null argument");
    out3[0] = h->start_mode; out3[1] = h->start_redrew; out3[2] = h->start_fell;
    return 0;
}
// ---- a data set per chain (include/mcmcx.h, "Many fits in one run"): the response-column target with every chain's own observations.
// Every target setter drops what an earlier mcmcx_set_target_expdata_all left: the last setter called wins.
static void drop_chain_data(mcmcx_engine *h)
{
    h->cdata_mode = 0; h->cdata_n = 0;
    std::vector<double>().swap(h->ty_all); std::vector<double>().swap(h->tx_all);
}
int mcmcx_set_target_expdata_all(mcmcx_handle h, int32_t nchains, int32_t ndata, int32_t nycol, const double *x, int32_t x_per_chain,
                                 const double *y_all)
{
    const char *who = "mcmcx_set_target_expdata_all";
    if (!h) return fail(-58, std::string(who) + ": null handle");
    if (h->inited) return fail(-58, std::string(who) + " after mcmcx_init (the data tables are filled there)");
    if (!x || !y_all) return fail(-58, std::string(who) + ": null array");
    if (nchains != h->cfg.nchains) return fail(-58, std::string(who) + ": y_all has " + std::to_string(nchains) +
        " data sets but the handle has nchains = " + std::to_string(h->cfg.nchains));
    if (ndata < 1) return fail(-58, std::string(who) + ": ndata must be >= 1");
    if (x_per_chain != 0 && x_per_chain != 1) return fail(-58, std::string(who) + ": x_per_chain must be 0 or 1");
    if (h->pooled) return fail(-58, std::string(who) + ": not in pooled mode (one proposal factor pooled over different posteriors is not "
        "a method)");
    if (nycol < 1 || nycol > MCX_MAX_NYCOL) return fail(-21, "nycol must be in 1.." + std::to_string(MCX_MAX_NYCOL));
    if (h->d != 1 + nycol) return fail(-22, "response-column target needs npar = 1 + nycol");
    drop_chain_data(h);
    const size_t N = (size_t)nchains, n = (size_t)ndata;
    h->tkind = TGT_EXPCOLS; h->tncols = nycol;
    h->cdata_mode = x_per_chain ? 2 : 1; h->cdata_n = ndata;
    h->ty_all.assign(y_all, y_all + N * (size_t)nycol * n);
    std::vector<double>().swap(h->ty);
    if (x_per_chain) { h->tx_all.assign(x, x + N * n); std::vector<double>().swap(h->tx); }
    else h->tx.assign(x, x + n);
    return 0;
}
int mcmcx_chain_data_info(mcmcx_handle h, int64_t *out4)
{
    if (!h || !h->inited) return fail(-40, "we have not inited");
    if (!out4) return fail(-1, "mcmcx_chain_data_info: null argument");
    const bool data = h->tkind == TGT_EXPDATA || h->tkind == TGT_EXPCOLS;
    out4[0] = h->cdata_mode; out4[1] = data ? h->E.tgt.ndata : 0; out4[2] = !data ? 0 : h->tkind == TGT_EXPCOLS ? h->tncols : 1;
    out4[3] = h->cdata_bytes;
    return 0;
}
int mcmcx_set_cmat0(mcmcx_handle h, const double *c, int32_t n)
{
    if (!h || !c) return fail(-1, "null argument");
    if (n != h->d) return fail(-20, "cmat0 and npar dont match");                    // MCMC_init.F90:207
    h->cmat0.assign(c, c + (size_t)n * n);
    return 0;
}
int mcmcx_set_sigma2nobs(mcmcx_handle h, const double *s2, const int32_t *nobs, int32_t nycol)
{
    if (!h || !s2 || !nobs) return fail(-1, "null argument");
    if (nycol < 1 || nycol > MCX_MAX_NYCOL) return fail(-21, "nycol must be in 1.." + std::to_string(MCX_MAX_NYCOL));
    if (h->inited) return fail(-20, "set sigma2 / nobs before mcmcx_init");
    h->ny = nycol; h->sigma2v.assign(s2, s2 + nycol); h->nobsv.assign(nobs, nobs + nycol);
    h->sigma2 = s2[0]; h->nobs = nobs[0]; h->sigma2ok = true;
    return 0;
}
int mcmcx_set_target_gauss(mcmcx_handle h, const double *mu, const double *lam)
{
    if (!h || !mu || !lam) return fail(-1, "null argument");
    drop_chain_data(h); h->tkind = TGT_GAUSS; h->tmu.assign(mu, mu + h->d); h->tlam.assign(lam, lam + (size_t)h->d * h->d);
    return 0;
}
int mcmcx_set_target_banana(mcmcx_handle h, double b)
{
    if (!h) return fail(-1, "null handle");
    if (h->d < 2) return fail(-22, "banana target needs npar >= 2");
    drop_chain_data(h); h->tkind = TGT_BANANA; h->tb = b;
    return 0;
}
int mcmcx_set_target_expdata(mcmcx_handle h, int32_t n, const double *x, const double *y)
{
    if (!h || !x || !y || n < 1) return fail(-1, "bad argument");
    if (h->d != 2) return fail(-22, "expdata target needs npar = 2");
    drop_chain_data(h); h->tkind = TGT_EXPDATA; h->tx.assign(x, x + n); h->ty.assign(y, y + n);
    return 0;
}
int mcmcx_set_target_expdata_cols(mcmcx_handle h, int32_t n, int32_t nycol, const double *x, const double *y)
{
    if (!h || !x || !y || n < 1) return fail(-1, "bad argument");
    if (nycol < 1 || nycol > MCX_MAX_NYCOL) return fail(-21, "nycol must be in 1.." + std::to_string(MCX_MAX_NYCOL));
    if (h->d != 1 + nycol) return fail(-22, "response-column target needs npar = 1 + nycol");
    drop_chain_data(h); h->tkind = TGT_EXPCOLS; h->tncols = nycol; h->tx.assign(x, x + n); h->ty.assign(y, y + (size_t)n * nycol);
    return 0;
}
int mcmcx_set_target_host(mcmcx_handle h, mcmcx_ssfun_t ss, mcmcx_priorfun_t pri, mcmcx_checkbounds_t cb, void *user)
{
    if (!h || !ss) return fail(-1, "mcmcx_set_target_host: ssfunction is required");     // ssfunction0.f90:10-14
    drop_chain_data(h); h->tkind = TGT_HOST; h->h_ss = ss; h->h_ss_batch = nullptr; h->h_pri = pri; h->h_cb = cb; h->h_user = user;
    return 0;
}

int mcmcx_set_target_host_batch(mcmcx_handle h, mcmcx_ssfun_batch_t ss_batch, mcmcx_priorfun_t pri, mcmcx_checkbounds_t cb, void *user,
    int32_t nthreads)
{
    if (!h || !ss_batch) return fail(-1, "mcmcx_set_target_host_batch: ssfunction_batch is required");
    if (h->inited) return fail(-20, "set the target before mcmcx_init");
    drop_chain_data(h); h->tkind = TGT_HOST; h->h_ss_batch = ss_batch; h->h_ss = nullptr; h->h_pri = pri; h->h_cb = cb; h->h_user = user;
    h->h_threads = nthreads < 1 ? 1 : nthreads;
    return 0;
}

int mcmcx_set_target_external(mcmcx_handle h)
{
    if (!h) return fail(-1, "null handle");
    if (h->inited) return fail(-2, "mcmcx_set_target_external after mcmcx_init");
    drop_chain_data(h);
    h->tkind = TGT_HOST; h->h_ss = nullptr; h->h_ss_batch = nullptr; h->h_pri = nullptr; h->h_cb = nullptr; h->h_user = nullptr;
    h->external = true;
    return 0;
}

int mcmcx_set_samples(mcmcx_handle h, int32_t first, int32_t thin, int32_t capacity)
{
    if (!h) return fail(-1, "null handle");
    if (h->inited) return fail(-47, "mcmcx_set_samples after mcmcx_init (the store is allocated there)");
    if (thin > 0 && h->external) return fail(-47, "mcmcx_set_samples: not with mcmcx_set_target_external (the caller drives the "
        "iterations)");
    if (first < 1 || thin < 0 || (thin > 0 && capacity < 1)) return fail(-47, "mcmcx_set_samples: first >= 1, thin >= 0 and, with "
        "thin > 0, capacity >= 1 (first = " + std::to_string(first) + ", thin = " + std::to_string(thin) + ", capacity = " +
        std::to_string(capacity) + ")");
    h->samp.first = first; h->samp.thin = thin; h->samp.capacity = thin > 0 ? capacity : 0;
    return 0;
}

int mcmcx_set_target_module(mcmcx_handle h, const char *code_object_path, const char *kernel_name, const void *userdata, int64_t nbytes)
{
    if (!h || !code_object_path || !kernel_name) return fail(-1, "mcmcx_set_target_module: null argument");
    if (h->inited) return fail(-20, "set the target before mcmcx_init");
    HIPCHK(hipSetDevice(h->cfg.device));
    hipError_t e = hipModuleLoad(&h->mod, code_object_path);
    if (e != hipSuccess) return fail(-37, std::string("cannot load the target module ") + code_object_path + ": " + hipGetErrorString(e));
    e = hipModuleGetFunction(&h->mod_fn, h->mod, kernel_name);
    if (e != hipSuccess) return fail(-37,
        std::string("target module: no kernel named ") + kernel_name + " (define it with MCMCX_DEFINE_TARGET, include/mcmcx_target.h)");
    for (const char *suffix : {"_abi", "_max_npar"}) {
        hipDeviceptr_t p = nullptr; size_t sz = 0; int v = 0;
        e = hipModuleGetGlobal(&p, &sz, h->mod, (std::string(kernel_name) + suffix).c_str());
        if (e != hipSuccess || sz != sizeof(int)) return fail(-37,
            std::string("target module: ") + kernel_name + suffix + " is missing (not built with MCMCX_DEFINE_TARGET?)");
        HIPCHK(hipMemcpy(&v, p, sizeof(int), hipMemcpyDeviceToHost));
        if (suffix[1] == 'a' && v != MCMCX_TARGET_ABI) return fail(-37, "target module: built against another mcmcx_target.h (abi " +
            std::to_string(v) + ")");
        if (suffix[1] == 'm' && h->d > v) return fail(-37, "target module: npar = " + std::to_string(h->d)
            + " but the module was compiled with MCMCX_TARGET_MAX_NPAR = " + std::to_string(v));
    }
    {   // response columns the module's kernel has room for (modules built before round 5 have no such symbol: eight)
        hipDeviceptr_t p = nullptr; size_t sz = 0; int v = 8;
        if (hipModuleGetGlobal(&p, &sz, h->mod, (std::string(kernel_name) + "_max_ny").c_str()) == hipSuccess && sz == sizeof(int))
            HIPCHK(hipMemcpy(&v, p, sizeof(int), hipMemcpyDeviceToHost));
        else (void)hipGetLastError();
        h->mod_max_ny = v;
    }
    if (userdata && nbytes > 0) {
        HIPCHK(hipMalloc(&h->d_moddata, (size_t)nbytes));
        h->allocs.push_back(h->d_moddata);
        HIPCHK(hipMemcpy(h->d_moddata, userdata, (size_t)nbytes, hipMemcpyHostToDevice));
    }
    drop_chain_data(h); h->tkind = TGT_MODULE;
    return 0;
}

int mcmcx_set_target_host_er(mcmcx_handle h, mcmcx_ssfun_er_t ss_er)
{
    if (!h) return fail(-1, "null handle");
    if (h->inited) return fail(-20, "set the target before mcmcx_init");
    h->h_ss_er = ss_er;
    return 0;
}

int mcmcx_set_bounds(mcmcx_handle h, const double *lo, const double *hi)
{
    if (!h) return fail(-1, "null handle");
    h->has_lo = lo != nullptr; h->has_hi = hi != nullptr;
    if (lo) h->tlo.assign(lo, lo + h->d);
    if (hi) h->thi.assign(hi, hi + h->d);
    return 0;
}
int mcmcx_set_priors(mcmcx_handle h, const double *mu, const double *sig)
{
    if (!h || !mu || !sig) return fail(-1, "null argument");
    h->has_pri = true; h->tpmu.assign(mu, mu + h->d); h->tpsig.assign(sig, sig + h->d);
    return 0;
}

// ---- mcmcx_init in steps.  What needs no device memory comes first, so that an invalid configuration allocates nothing; where one
// trips several checks the code that wins is, in this order: -30, -36, -31 (init_check), then -- the plan made -- the pooled -36, -32,
// the two pooled -8, -34 and the external-target -8 (initial_factor).  The external target is checked first of these: it is a host target
// without callbacks, and nothing of what follows is meant for it.
struct InitialFactor { std::vector<double> Rp, Cp, Rfull, qstd, iCp, R2p; };  // R(cmat0), cmat0 packed; the SVD factor; DR: dpotri(R), R2
static int init_check(mcmcx_engine *h)
{
    const int d = h->d;
    if ((int)h->par0.size() != d) return fail(-30, "user initialization error: par0 not set");
    if (h->cmat0.empty()) {                                                           // MCMC_initcmat0: identity
        h->cmat0.assign((size_t)d * d, 0.0);
        for (int i = 0; i < d; ++i) h->cmat0[(size_t)i * d + i] = 1.0;
    }
    if (!h->sigma2ok) { h->sigma2 = 1.0; h->nobs = 1; h->ny = 1; }                    // MCMC_init.F90:52-59
    if (h->ny == 1) { h->sigma2v.assign(1, h->sigma2); h->nobsv.assign(1, h->nobs); }
    const int ny = h->ny;
    if (ny > 1 && !phased(h)) return
        fail(-36, "nycol > 1 needs the host-callback or the response-column target (the other built-in targets have one column)");
    if (h->tkind == TGT_MODULE && ny > h->mod_max_ny)
        return fail(-36, "target module: nycol = " + std::to_string(ny) + " but the module was compiled with MCMCX_TARGET_MAX_NY = " +
            std::to_string(h->mod_max_ny));
    if (h->tkind == TGT_EXPCOLS
        && h->tncols != ny) return fail(-36, "response-column target: mcmcx_set_sigma2nobs must give one sigma2 / nobs per column");
    if (h->tkind < 0) return fail(-31, "no target: the device engine needs mcmcx_set_target_*");
    if (h->external && h->samp.thin > 0) return fail(-47, "mcmcx_set_samples: not with mcmcx_set_target_external (the caller drives the "
        "iterations)");
    if (h->external && h->start_mode) return fail(-56, "per-chain start points: not with mcmcx_set_target_external (the caller holds the "
        "chains' states)");
    return 0;
}
static int initial_factor(mcmcx_engine *h, InitialFactor &f)
{
    const mcmcx_config &c = h->cfg;
    const int d = h->d, P = h->P;
    if (h->external && h->pooled) return fail(-8, "mcmcx_set_target_external: not in pooled mode (the caller drives one evaluation at a "
        "time; pooled mode takes a target module, mcmcx_set_target_module, or host callbacks, mcmcx_set_target_host)");
    // (a target module or host callbacks: every method, SCAM through the replicated rotation)
    if (h->ny > 1 && h->pooled && h->plan.fused_cols && c.method == MCMCX_METHOD_SCAM)
        return fail(-36, "nycol > 1 in pooled mode: not with method = 'scam' on the device-resident response-column target");
    int info = host_initial_R(d, h->cmat0, f.Rp, f.Cp);
    // the drawn starts are par0 + scale U0'z with U0 this Cholesky factor, whatever factor the proposals use (condmax > 0, SCAM)
    if (h->start_mode == 2 && info != 0) return fail(-56, "mcmcx_set_par0_spread: could not factor the initial covariance (dpotf2 stopped "
        "at column " + std::to_string(info) + "): the starts are drawn with its Cholesky factor");
    if (h->usesvd) {                                                                  // Cp (packed cmat0) is still needed
        if (info != 0) { f.Rp.assign(P, 0.0); info = 0; }
        info = host_initial_svd(d, h->cmat0, c.condmax, c.method == MCMCX_METHOD_SCAM, f.Rfull, f.qstd);
    }
    if (info != 0) return fail(-32, "could not factor the initial covariance");      // MCMC_init.F90:110
    if (h->pooled && (long long)c.nchains * (h->comm ? h->comm->nranks : 1) < 2)
        return fail(-8, "pooled mode needs at least 2 chains over all ranks");
    if (h->pooled && h->plan.fused_cols && c.method == MCMCX_METHOD_SCAM)
        return fail(-8, "pooled mode with method = 'scam': not on the device-resident response-column target (expcols)");
    if (h->dodr) {                                      // iC = dpotri(R), R2 = R/drscale, MCMC_adapt.F90:216-225
        f.iCp = f.Rp; f.R2p.resize(P);
        if (h->usesvd) for (int j = 0; j < d; ++j) for (int i = 0; i <= j; ++i) f.iCp[h_pidx(i, j, d)] = f.Rfull[(size_t)j * d + i];
        if (host_potri(d, f.iCp) != 0) return fail(-34, "ERROR: cannot invert cmat");
        for (int e = 0; e < P; ++e) f.R2p[e] = f.Rp[e] / c.drscale;
    }
    return 0;
}
static int init_engine_dev(mcmcx_engine *h, const InitialFactor &f)    // EngineDev's scalars, the target's and the problem's tables
{
    const mcmcx_config &c = h->cfg;
    EngineDev &E = h->E;
    E = EngineDev{};                                    // every table nullptr until a step below allocates it
    h->S02eff = (c.S02 <= 0.0) ? h->sigma2 : c.S02;                                   // MCMC_init.F90:114-116
    E.d = h->d; E.P = h->P; E.ntiles = h->ntiles;
    E.method = kernel_method(h);
    E.usesvd = h->usesvd; E.doscam = (c.method == MCMCX_METHOD_SCAM) ? 1 : 0; E.condmax = c.condmax;
    E.scam_fast = c.scam_fast ? 1 : 0;
    E.greedy = c.greedy; E.adapthist = c.adapthist; E.initcmatn = (double)c.initcmatn;
    E.dodr = h->dodr; E.updatesigma = c.updatesigma; E.doadapt = c.doadapt; E.doburnin = c.doburnin; E.burnintime = c.burnintime;
    E.gam_shape = c.N0 / 2.0 + (double)h->nobs / 2.0; E.N0S02 = c.N0 * h->S02eff;
    E.ny = h->ny; E.hs = h->d + h->ny;
    E.alphatarget = c.alphatarget; E.drscale = c.drscale; E.scalelimit = c.scalelimit; E.scalefactor = c.scalefactor;
    E.k0 = c.seed; E.chain_id0 = c.chain_id0;
    E.dr_lds = h->plan.dr_lds ? 1 : 0;
    E.lds_scratch = h->plan.lds_form;
    E.tgt.kind = phased(h) ? (int)TGT_HOST : h->tkind;   // the kernels know one phase-cut mode; who evaluates is the host's business
    E.tgt.b = h->tb; E.tgt.ndata = h->cdata_mode ? h->cdata_n : (int)h->tx.size(); E.tgt.ncols = h->tncols;
    const int d = h->d;
    int rc;
    if (h->tkind == TGT_GAUSS) {
        if ((rc = dev_upload(h, &E.tgt.mu, h->tmu))) return rc;
        std::vector<double> lt((size_t)(d + 4) * d + 64, 0.0);     // transpose; zero pad rows + slack for the panel / MFMA tile reads
        for (int i = 0; i < d; ++i) for (int j = 0; j < d; ++j) lt[(size_t)j * d + i] = h->tlam[(size_t)i * d + j];
        if ((rc = dev_upload(h, &E.tgt.lamT, lt))) return rc;
    }
    if (h->cdata_mode) {                                 // a data set per chain: init_chain_data's tables, and the shared x where kept
        const size_t L = (size_t)h->ntiles * 64, n = (size_t)h->cdata_n;
        double *yc = nullptr, *xc = nullptr;
        if ((rc = dev_alloc(h, &yc, L * (size_t)h->tncols * n, false))) return rc;
        if (h->cdata_mode == 2 ? (rc = dev_alloc(h, &xc, L * n, false)) : (rc = dev_upload(h, &E.tgt.x, h->tx))) return rc;
        E.tgt.yc = yc; E.tgt.xpc = xc ? 1 : 0;
        if (xc) E.tgt.xc = xc;
        h->cdata_bytes = (long long)((L * (size_t)h->tncols * n + (xc ? L * n : 0)) * sizeof(double));
    } else if (h->tkind == TGT_EXPDATA || h->tkind == TGT_EXPCOLS) {
        if ((rc = dev_upload(h, &E.tgt.x, h->tx)) || (rc = dev_upload(h, &E.tgt.y, h->ty))) return rc;
    }
    if (h->has_lo && (rc = dev_upload(h, &E.tgt.lo, h->tlo))) return rc;
    if (h->has_hi && (rc = dev_upload(h, &E.tgt.hi, h->thi))) return rc;
    if (h->has_pri) { if ((rc = dev_upload(h, &E.tgt.pmu, h->tpmu))) return rc; if ((rc = dev_upload(h, &E.tgt.psig, h->tpsig))) return rc;
        }
    if ((rc = dev_upload(h, &E.par0, h->par0))) return rc;
    return dev_upload(h, &E.cmat0p, f.Cp);
}
// the chains' state and scratch vectors, their SVD factors and the adaptation's work space, the delayed-rejection tables, the history
// ring, AM's state
static int init_chains(mcmcx_engine *h, const InitialFactor &f)
{
    const mcmcx_config &c = h->cfg;
    EngineDev &E = h->E;
    const int d = h->d, P = h->P, T = h->ntiles, ny = h->ny;
    const size_t L = (size_t)T * 64, DD = (size_t)d * d;
    int rc;
    if ((rc = dev_alloc(h, &E.theta, L * d))) return rc;
    if ((rc = h->plan.host_mapped ? host_alloc(h, &E.cand, L * d) : dev_alloc(h, &E.cand, L * d))) return rc;
    if ((rc = dev_alloc(h, &E.zs, L * 2 * d))) return rc;
    if ((rc = h->plan.cs_mapped ? host_alloc(h, &E.cs, L * 2 * d) : dev_alloc(h, &E.cs, L * 2 * d))) return rc;
    if (h->plan.xscr && (rc = dev_alloc(h, &E.xscr, L * 2 * d))) return rc;
    if (h->plan.ram_pair && (rc = dev_alloc(h, &h->d_pair, L * 3 * d))) return rc;
    if ((rc = dev_alloc(h, &E.scal, L * NSCAL))) return rc;
    if ((rc = dev_alloc(h, &E.ictr, L * NICTR))) return rc;
    if ((rc = dev_alloc(h, &E.rngn, L))) return rc;
    if (!h->pooled && (rc = dev_alloc(h, &E.R, L * P, false))) return rc;          // pooled: one shared factor instead
    if ((rc = dev_alloc(h, &E.basetheta, L * d))) return rc;
    if (h->start_mode && (rc = dev_alloc(h, &E.start, L * d, false))) return rc;       // the chains' own start points (init_starts)
    if (h->usesvd && !h->pooled) {                      // (pooled: pooled_alloc)
        if ((rc = dev_alloc(h, &E.Rf, L * DD, false))) return rc;
        if (c.method != MCMCX_METHOD_RAM) {                 // work space of the adaptation's SVD; RAM never refactors
            if ((rc = dev_alloc(h, &E.Gw, L * DD)) || (rc = dev_alloc(h, &E.Vw, L * DD))) return rc;
            if (h->plan.svd_blocked && ((rc = dev_alloc(h, &h->d_Gc, L * DD, false)) || (rc = dev_alloc(h, &h->d_Vc, L * DD, false))
                || (rc = dev_alloc(h, &h->d_svc, L * d, false)) || (rc = dev_alloc(h, &h->d_need, L)) || (rc = dev_alloc(h, &h->d_state, L))
                || (rc = dev_alloc(h, &h->d_anyrot, 1)))) return rc;    // chain-major copies for svd_blocked_kernel
        }
        if ((rc = dev_alloc(h, &E.qstd, L * d))) return rc;
        if (h->dodr && (rc = dev_alloc(h, &E.R2f, L * DD, false))) return rc;
        if ((rc = dev_bcast(h, E.Rf, f.Rfull)) || (rc = dev_bcast(h, E.qstd, f.qstd))) return rc;
        if (h->dodr) {
            std::vector<double> r2 = f.Rfull;
            for (auto &v : r2) v = v / c.drscale;
            if ((rc = dev_bcast(h, E.R2f, r2))) return rc;
        }
    }
    // (pooled: one R2 and one iC for every chain, pooled_alloc)
    if (h->dodr && !h->pooled && ((rc = dev_alloc(h, &E.R2, L * P, false)) || (rc = dev_alloc(h, &E.iC, L * P, false)))) return rc;
    const bool am = h->plan.am;
    h->wcap = 0;
    if (am || c.record_chain) {                         // the history ring
        // AP windows (adapthist > 1) may reach back to an arbitrarily old row: keep everything.  Otherwise the longest
        // window is the first AM one, rows 2 .. T1 with T1 the first multiple of adaptint / badaptint that is
        // >= burnintime + adaptint + adapthist (MCMC_adapt.F90:42-46,105): up to adaptint - 1 iterations past that
        // threshold when it is not a multiple itself (burn-in ticks only rescale and never restart the window)
        long long wc = (c.record_chain || (am && c.adapthist > 1)) ? (long long)c.nsimu + 1
                                      : (long long)c.burnintime + 2LL * c.adaptint + c.adapthist + 2;
        if (wc > (long long)c.nsimu + 1) wc = (long long)c.nsimu + 1;
        h->wcap = (int)wc;
        if ((rc = dev_alloc(h, &E.hist, L * (size_t)h->wcap * (d + ny), false))) return rc;
        if ((rc = dev_alloc(h, &E.wacc, (size_t)T * h->wcap))) return rc;
        if (c.record_chain && c.updatesigma) { E.record_s2 = 1; if ((rc = dev_alloc(h, &E.s2hist, L * (size_t)h->wcap * ny))) return rc; }
    }
    E.wcap = h->wcap > 0 ? h->wcap : 1;
    if (am && ((rc = dev_alloc(h, &E.cmat, L * P)) || (rc = dev_alloc(h, &E.mean, L * d)) || (rc = dev_alloc(h, &E.Rtmp, L * P))
        || (rc = dev_alloc(h, &E.rowlist, L * (size_t)(h->wcap + 1))))) return rc;
    return 0;
}
// the host-callback / response-column phase buffers, the accept records, the RAM step sizes, the pooled moments' workspace
static int init_run_buffers(mcmcx_engine *h)
{
    const mcmcx_config &c = h->cfg;
    EngineDev &E = h->E;
    const int d = h->d, P = h->P, T = h->ntiles, ny = h->ny;
    const size_t L = (size_t)T * 64;
    int rc;
    if (phased(h)) {
        const size_t nhev = L * (NHE - 1 + ny);
        if ((rc = h->plan.host_mapped ? host_alloc(h, &E.hev, nhev) : dev_alloc(h, &E.hev, nhev))) return rc;
        if (ny > 1) {
            if ((rc = dev_alloc(h, &E.ssv, L * ny)) || (rc = dev_alloc(h, &E.s2v, L * ny)) || (rc = dev_alloc(h, &E.ss2v, L * ny))
                || (rc = dev_bcast(h, E.s2v, h->sigma2v))) return rc;
            std::vector<double> gs(ny);
            for (int j = 0; j < ny; ++j) gs[j] = c.N0 / 2.0 + (double)h->nobsv[j] / 2.0;
            if ((rc = dev_upload(h, &E.gshapev, gs))) return rc;
        }
        if ((rc = h->plan.host_mapped ? host_alloc(h, &E.hx, L * NHX) : dev_alloc(h, &E.hx, L * NHX))) return rc;
    }
    if (h->external && (rc = dev_alloc(h, &h->d_r1, L * (size_t)(3 * d + 3 * ny + NR1)))) return rc;   // MCMC_run1: run1_kernel's vectors
    if (c.record_accept && (rc = dev_alloc(h, &E.accmask, (size_t)c.nsimu * T))) return rc;
    // the lane-group kernels: accept bytes of a launch; the range flag of the power-of-two delayed-rejection form
    if ((h->plan.group_d4 || h->plan.ram_group_d4) && (E.hist || E.accmask)
        && (rc = dev_alloc(h, &h->d_accb, L * (size_t)GROUP_MAXSEG))) return rc;
    if (h->plan.group_d4 && h->plan.group_drm == 2 && (rc = dev_alloc(h, &h->d_gflag, 1))) return rc;
    // 1/simuind**nuparam, computed like the reference: real(simuind) is default REAL (MCMC_run_ram.F90:166)
    {
        std::vector<double> rs((size_t)c.nsimu + 2, 0.0);
        for (int it = 1; it <= c.nsimu; ++it) rs[it] = 1.0 / std::pow((double)(float)it, c.nuparam);
        const double *p = nullptr;
        if ((rc = dev_upload(h, &p, rs))) return rc;
        h->d_ramscale = const_cast<double *>(p);
    }
    if ((rc = dev_alloc(h, &h->d_moments, (size_t)(T + 1) * (2 + d + P)))) return rc;                 // longest pooled vector: 2 + d + P
    if ((rc = dev_alloc(h, &h->d_gather, (size_t)(h->comm ? h->comm->nranks : 1) * (3 + d + P)))) return rc;   // ... + the stop flag
    return dev_alloc(h, &h->d_pooled, (size_t)(3 + d + P));
}
// E.start, when the chains have start points of their own: the caller's rows (padding lanes of the last tile: par0), or drawn by
// start_spread_kernel with the shared packed factor U0 = f.Rp; dst (theta, chainmean) is then a copy of it instead of par0's broadcast
static int init_starts(mcmcx_engine *h, const InitialFactor &f)
{
    EngineDev &E = h->E;
    const int d = h->d, T = h->ntiles, N = h->cfg.nchains;
    h->start_redrew = h->start_fell = 0;
    if (h->start_mode == 1) {
        std::vector<double> st((size_t)T * 64 * d);
        for (int c = 0; c < T * 64; ++c)
            for (int k = 0; k < d; ++k)
                st[((size_t)(c / 64) * d + k) * 64 + (c % 64)] = c < N ? h->start_all[(size_t)c * d + k] : h->par0[k];
        HIPCHK(hipMemcpyAsync(E.start, st.data(), st.size() * sizeof(double), hipMemcpyHostToDevice, h->stream));
        HIPCHK(hipStreamSynchronize(h->stream));
        std::vector<double>().swap(h->start_all);       // the device table holds them now: the host copy of the call is released
        return 0;
    }
    DevBufs tmp;
    double *U0 = nullptr; uint32_t *tries = nullptr;
    HIPCHK(tmp.alloc(&U0, f.Rp.size() * sizeof(double)));
    HIPCHK(tmp.alloc(&tries, (size_t)T * 64 * sizeof(uint32_t)));
    HIPCHK(hipMemcpyAsync(U0, f.Rp.data(), f.Rp.size() * sizeof(double), hipMemcpyHostToDevice, h->stream));
    hipLaunchKernelGGL(start_spread_kernel, dim3(T), dim3(64), 0, h->stream, E, (const double *)U0, h->start_scale, N, tries);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemsetAsync(E.zs, 0, (size_t)T * 64 * 2 * d * sizeof(double), h->stream));     // the attempts' normals: scratch as allocated
    std::vector<uint32_t> tr((size_t)T * 64);
    HIPCHK(hipMemcpyAsync(tr.data(), tries, tr.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    for (int c = 0; c < N; ++c) {
        if ((tr[c] & ~START_FELL_BACK) > 1u) h->start_redrew += 1;
        if (tr[c] & START_FELL_BACK) h->start_fell += 1;
    }
    return 0;
}
// E.tgt.yc / xc, when every chain has a data set of its own: the call's rows staged into tiles, yc [tile][j * ndata + i][64] and (mode 2)
// xc [tile][i][64] with 64-bit indices; lanes of the last tile without a chain hold +0.0.  The host copies of the call are released here.
static int init_chain_data(mcmcx_engine *h)
{
    EngineDev &E = h->E;
    const size_t T = (size_t)h->ntiles, N = (size_t)h->cfg.nchains, n = (size_t)h->cdata_n, rows = (size_t)h->tncols * n;
    {
        std::vector<double> st(T * rows * 64, 0.0);
        for (size_t c = 0; c < N; ++c)
            for (size_t r = 0; r < rows; ++r) st[((c / 64) * rows + r) * 64 + (c % 64)] = h->ty_all[c * rows + r];
        HIPCHK(hipMemcpyAsync(const_cast<double *>(E.tgt.yc), st.data(), st.size() * sizeof(double), hipMemcpyHostToDevice, h->stream));
        HIPCHK(hipStreamSynchronize(h->stream));
    }
    if (h->cdata_mode == 2) {
        std::vector<double> st(T * n * 64, 0.0);
        for (size_t c = 0; c < N; ++c)
            for (size_t i = 0; i < n; ++i) st[((c / 64) * n + i) * 64 + (c % 64)] = h->tx_all[c * n + i];
        HIPCHK(hipMemcpyAsync(const_cast<double *>(E.tgt.xc), st.data(), st.size() * sizeof(double), hipMemcpyHostToDevice, h->stream));
        HIPCHK(hipStreamSynchronize(h->stream));
    }
    std::vector<double>().swap(h->ty_all); std::vector<double>().swap(h->tx_all);
    return 0;
}
static int fill_start(mcmcx_engine *h, double *dst)         // dst = every chain's start: par0, or its row of E.start
{
    if (!h->E.start) return dev_bcast(h, dst, h->par0);
    HIPCHK(hipMemcpyAsync(dst, h->E.start, (size_t)h->ntiles * 64 * h->d * sizeof(double), hipMemcpyDeviceToDevice, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    return 0;
}
// fill theta = the start (par0), R = R(cmat0), chaincmat = cmat0, chainmean = the start, scalars; the first evaluation
static int init_fill(mcmcx_engine *h, const InitialFactor &f)
{
    const mcmcx_config &c = h->cfg;
    EngineDev &E = h->E;
    const int T = h->ntiles;
    std::vector<double> sc((size_t)T * 64 * NSCAL, 0.0);
    std::vector<uint32_t> ic((size_t)T * 64 * NICTR, 0u);
    for (int t = 0; t < T; ++t)
        for (int l = 0; l < 64; ++l) {
            sc[((size_t)t * NSCAL + S_SIGMA2) * 64 + l] = h->sigma2;
            sc[((size_t)t * NSCAL + S_WSUM) * 64 + l] = (double)c.initcmatn;
            ic[((size_t)t * NICTR + I_CHAININD) * 64 + l] = 1;
            ic[((size_t)t * NICTR + I_CURCOUNT) * 64 + l] = 1;
            ic[((size_t)t * NICTR + I_BASECNT) * 64 + l] = 1;
            ic[((size_t)t * NICTR + I_WINSTART) * 64 + l] = 2;
        }
    HIPCHK(hipMemcpyAsync(E.scal, sc.data(), sc.size() * 8, hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipMemcpyAsync(E.ictr, ic.data(), ic.size() * 4, hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    int rc;
    if (h->start_mode && (rc = init_starts(h, f))) return rc;
    if (h->cdata_mode && (rc = init_chain_data(h))) return rc;
    if ((rc = fill_start(h, E.theta))) return rc;
    if (!h->pooled && (rc = dev_bcast(h, E.R, f.Rp))) return rc;
    if (h->dodr && !h->pooled && ((rc = dev_bcast(h, E.R2, f.R2p)) || (rc = dev_bcast(h, E.iC, f.iCp)))) return rc;
    if (h->plan.am && ((rc = dev_bcast(h, E.cmat, f.Cp)) || (rc = fill_start(h, E.mean)))) return rc;
    // first point: sspri1, ss1 from the callbacks (MCMC_run.F90:35-36) -- with MCMC_run1 every evaluation is the caller's, this one too
    if (!h->external && phased(h) && (rc = host_eval(h, E.theta, h->d, false))) return rc;
    launch_init(h);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(h->stream));
    return 0;
}

int mcmcx_init(mcmcx_handle h)
{
    if (!h) return fail(-1, "null handle");
    if (h->inited) return fail(1, "Warning(mcmcinit): allready inited");            // MCMC_init.F90:24-27
    HIPCHK(hipSetDevice(h->cfg.device));
    int rc = init_check(h);
    if (rc) return rc;
    plan_kernels(h);                                 // which kernels run: decided here, once; what follows allocates as the plan says
    InitialFactor f;
    if ((rc = initial_factor(h, f))) return rc;
    if ((rc = init_engine_dev(h, f)) || (rc = init_chains(h, f))) return rc;
    if (h->pooled) {                                 // the shared tables' masters as MCMC_init leaves a chain's, in the planned layouts
        PooledState &s = h->pool;
        s.R = f.Rp; s.C = f.Cp; s.mean = h->par0; s.W = (double)h->cfg.initcmatn;
        if (h->cfg.method == MCMCX_METHOD_SCAM) { s.U = f.Rfull; s.std = f.qstd; } else s.Rf = f.Rfull;
        if (h->dodr) pooled_dr_fresh(h);
        if ((rc = pooled_alloc(h)) || (rc = pooled_upload(h))) return rc;
    }
    if ((rc = init_run_buffers(h)) || (rc = samples_alloc(h)) || (rc = init_fill(h, f))) return rc;
    if (sample_due(h, 1) && (rc = samples_keep(h, 1))) return rc;         // iteration 1 is the start point (the reference's chain row 1)
    h->simuind = 1;
    h->inited = true;
    return 0;
}

int mcmcx_install_signal_handlers(void)
{
    struct sigaction act;
    memset(&act, 0, sizeof(act));
    act.sa_handler = on_signal;
    sigemptyset(&act.sa_mask);
    const int sigs[] = {SIGHUP, SIGINT, SIGTERM, SIGTSTP, SIGUSR1, SIGUSR2};
    for (int sg : sigs) if (sigaction(sg, &act, nullptr) != 0) return fail(-1, "sigaction failed");
    g_sig_installed = true;
    return 0;
}
int mcmcx_interrupted(void) { return g_interrupt ? 1 : 0; }
void mcmcx_clear_interrupt(void) { g_interrupt = 0; }

static int run_impl(mcmcx_handle h, int32_t upto);
int mcmcx_run(mcmcx_handle h, int32_t upto)
{
    const int rc = run_impl(h, upto);
    // Several ranks meet in this engine's ticks: one that fails must not leave the others waiting in the next gather --
    // the communicator is marked failed, which the peers' waits poll (comm_wait_stream, shm_barrier)
    // -- once the run has entered its loop, that is: an argument or state error returned before that (-40 not inited, -41 external
    // target) strands nobody, and marking the communicator for it would abort peers that have nothing to do with it
    if (rc < 0 && h && h->inited && h->run_entered && collective_run(h)) comm_mark_failed(h->comm);
    if (h) h->run_entered = false;
    return rc;
}
static int run_impl(mcmcx_handle h, int32_t upto)
{
    if (!h) return fail(-1, "null handle");
    if (!h->inited) return fail(-40, "we have not inited");                           // MCMC_run.F90:22
    if (h->external) return fail(-41, "mcmcx_run: the target is external (mcmcx_set_target_external): drive the chain with mcmcx_run1_*");
    // (with the phases fused, iteration it + 1's proposal -- Philox draws included -- has already run when an error surfaces in iteration
    // it's evaluation; a second run on the handle would draw that proposal again and leave the reference's stream order silently: ADVICE
    // round 5)
    if (h->failed) return fail(-42, "mcmcx_run: an earlier run on this handle failed inside a host-callback iteration; its chains are in an undefined state -- destroy the handle");
    HIPCHK(hipSetDevice(h->cfg.device));
    const mcmcx_config &c = h->cfg;
    if (upto > c.nsimu) upto = c.nsimu;
    const int maxseg = (h->plan.group_d4 || h->plan.ram_group_d4) ? GROUP_MAXSEG
                       : (c.method == MCMCX_METHOD_RAM && !h->pooled) ? 4096 : 1 << 30;
    int it = h->simuind + 1;
    // Several ranks that meet in this engine's ticks (pooled mode with a communicator): a rank that left the loop alone --
    // on a signal it happened to see first, or on an error of its own -- would leave its peers waiting in the next gather.
    // So a signal only raises this rank's stop flag in the exchanged vector and the run is left at the tick where every
    // rank reads the summed flag (pooled_reduce); an error marks the communicator failed (mcmcx_run).
    const bool coll = collective_run(h);
    h->run_entered = true;
    // ... which needs a tick ahead.  Whether one lies in (it, upto] follows from the configuration alone, the same on every
    // rank: past the last one (doadapt = 0, iterations beyond adaptend, the tail of a run) no collective is left to strand a
    // peer in, and a signal is acted on at the next launch boundary like in a run of one rank.
    int last_tick = 0;
    if (coll) for (int i2 = upto; i2 >= it; --i2) if (adapt_mode(c, i2) != 0 || pooled_ram_due(h, i2)) { last_tick = i2; break; }
    h->stop_seen = false;
    while (it <= upto) {
        if (g_interrupt && (!coll || it > last_tick)) {     // a caught signal: stop at this launch boundary
            int rc = mcmcx_sync(h); if (rc) return rc;
            h->simuind = it - 1;
            return MCMCX_INTERRUPTED;
        }
        int end = it, mode = 0;
        bool ramtick = false;
        for (;; ++end) {                                    // extend the launch up to the next tick or kept iteration
            mode = adapt_mode(c, end);
            ramtick = pooled_ram_due(h, end);
            if (mode != 0 || ramtick || sample_due(h, end) || end == upto || end - it + 1 >= maxseg) break;
        }
        if (phase_cut(h)) {
            for (int i2 = it; i2 <= end; ++i2) { int rc = host_iteration(h, i2, i2 < end); if (rc) { h->failed = true; return rc; } }
        } else {
            hipEvent_t e0 = nullptr, e1 = nullptr;
            hipError_t er = hipEventCreate(&e0);
            if (er == hipSuccess) er = hipEventCreate(&e1);
            if (er == hipSuccess) er = hipEventRecord(e0, h->stream);
            if (er == hipSuccess) {
                h->launch_err.clear();
                if (h->cfg.method == MCMCX_METHOD_SCAM) launch_scam(h, it, end); else launch_step(h, it, end);
                er = hipGetLastError();
            }
            // a cover predicate and the dispatch disagree: fail, never skip iterations silently
            if (er == hipSuccess && !h->launch_err.empty()) {
                if (e0) (void)hipEventDestroy(e0);
                if (e1) (void)hipEventDestroy(e1);
                return fail(-103, "step launch: " + h->launch_err);
            }
            if (er == hipSuccess) er = hipEventRecord(e1, h->stream);
            if (er != hipSuccess) {                       // nothing is left behind on the error path
                if (e0) (void)hipEventDestroy(e0);
                if (e1) (void)hipEventDestroy(e1);
                return fail(-100, std::string("step launch: ") + hipGetErrorString(er));
            }
            h->pending.emplace_back(e0, e1);
            h->launches += 1; h->steps += (end - it + 1);
        }
        int trc = 0;
        if (mode != 0) {
            if (h->pooled) trc = pooled_tick(h, end, mode);
            else { launch_adapt(h, end, mode); h->group_check_due = true; HIPCHK(hipGetLastError()); }
        }
        if (ramtick && trc == 0) trc = pooled_ram_tick(h, end);
        if (trc) return trc;
        // a kept iteration (mcmcx_set_samples): the state the launch wrote back, behind the tick (which does not move theta) and outside
        // the step kernels' event pair
        if (sample_due(h, end)) { int rc = samples_keep(h, end); if (rc) return rc; }
        if (h->stop_seen) {                                 // every rank read the same summed stop flag at this tick: leave together,
            h->stop_seen = false;                           // after iteration `end` WITH its adaptation applied (a resumed run
            int rc = mcmcx_sync(h); if (rc) return rc;      // continues at end + 1 like an uninterrupted one)
            h->simuind = end;
            return MCMCX_INTERRUPTED;
        }
        it = end + 1;
        if (g_sig_installed) { HIPCHK(hipStreamSynchronize(h->stream)); h->simuind = std::max(h->simuind, end); }
        if (h->pending.size() > 4096) { int rc = mcmcx_sync(h); if (rc) return rc; }
    }
    h->simuind = std::max(h->simuind, (int)upto);
    return 0;
}

int mcmcx_run1_decide(mcmcx_handle h, int32_t drstage, const double *oldpar2, const double *ssprev2, const double *sspri2,
                      const double *oldpar1, const double *ssprev1, const double *sspri1, const double *alpha12,
                      const double *newpar, const double *ss, const double *sspri, double *alpha_out, int32_t *reject_out)
{
    int rc = run1_check(h); if (rc) return rc;
    if (!oldpar1 || !ssprev1 || !sspri1 || !newpar || !ss || !sspri || !alpha_out
        || !reject_out) return fail(-1, "mcmcx_run1_decide: null argument");
    const bool dr2 = drstage > 1 && h->dodr;
    if (dr2 && (!oldpar2 || !ssprev2 || !sspri2
        || !alpha12)) return fail(-1, "mcmcx_run1_decide: the second stage needs oldpar2, ssprev2, sspri2, alpha12");
    const int d = h->d, ny = h->ny, n = h->cfg.nchains, s0 = 3 * d + 3 * ny;
    h->h_r1.assign((size_t)h->ntiles * 64 * (s0 + NR1), 0.0);
    run1_put(h, 0, d, dr2 ? oldpar2 : nullptr); run1_put(h, d, d, oldpar1); run1_put(h, 2 * d, d, newpar);
    run1_put(h, 3 * d, ny, dr2 ? ssprev2 : nullptr); run1_put(h, 3 * d + ny, ny, ssprev1); run1_put(h, 3 * d + 2 * ny, ny, ss);
    run1_put(h, s0 + R1_PRI2, 1, dr2 ? sspri2 : nullptr); run1_put(h, s0 + R1_PRI1, 1, sspri1); run1_put(h, s0 + R1_PRI, 1, sspri);
    run1_put(h, s0 + R1_A12, 1, dr2 ? alpha12 : nullptr);
    if ((rc = run1_launch<0>(h, drstage))) return rc;
    run1_get(h, s0 + R1_ALPHA, 1, alpha_out);
    std::vector<double> rj(n);
    run1_get(h, s0 + R1_REJECT, 1, rj.data());
    for (int c = 0; c < n; ++c) reject_out[c] = rj[c] != 0.0 ? 1 : 0;
    return 0;
}

int mcmcx_run1_propose(mcmcx_handle h, int32_t stage, const double *from, double *newpar_out)
{
    int rc = run1_check(h); if (rc) return rc;
    if (!from || !newpar_out) return fail(-1, "mcmcx_run1_propose: null argument");
    const int d = h->d, ny = h->ny;
    h->h_r1.assign((size_t)h->ntiles * 64 * (3 * d + 3 * ny + NR1), 0.0);
    run1_put(h, 0, d, from);
    if (stage > 1 && h->dodr) rc = run1_launch<2>(h, 2); else rc = run1_launch<1>(h, 1);
    if (rc) return rc;
    run1_get(h, 2 * d, d, newpar_out);
    return 0;
}

int mcmcx_run1_sscrit(mcmcx_handle h, const double *ssprev1, const double *sspri1, double *sscrit_out)
{
    int rc = run1_check(h); if (rc) return rc;
    if (!ssprev1 || !sspri1 || !sscrit_out) return fail(-1, "mcmcx_run1_sscrit: null argument");
    const int d = h->d, ny = h->ny, s0 = 3 * d + 3 * ny;
    h->h_r1.assign((size_t)h->ntiles * 64 * (s0 + NR1), 0.0);
    run1_put(h, 3 * d + ny, ny, ssprev1); run1_put(h, s0 + R1_PRI1, 1, sspri1);
    if ((rc = run1_launch<3>(h, 1))) return rc;
    run1_get(h, s0 + R1_CRIT, 1, sscrit_out);
    return 0;
}

int mcmcx_sync(mcmcx_handle h)
{
    if (!h) return fail(-1, "null handle");
    HIPCHK(hipSetDevice(h->cfg.device));
    HIPCHK(hipStreamSynchronize(h->stream));
    for (auto &p : h->pending) {
        float ms = 0.f;
        HIPCHK(hipEventElapsedTime(&ms, p.first, p.second));
        h->ms_total += ms;
        (void)hipEventDestroy(p.first); (void)hipEventDestroy(p.second);
    }
    h->pending.clear();
    return 0;
}

int mcmcx_kernel_time(mcmcx_handle h, double *ms, int64_t *launches, int64_t *steps, int reset)
{
    int rc = mcmcx_sync(h);
    if (rc) return rc;
    if (ms) *ms = h->ms_total;
    if (launches) *launches = h->launches;
    if (steps) *steps = h->steps;
    if (reset) { h->ms_total = 0.0; h->launches = 0; h->steps = 0; }
    return 0;
}

int32_t mcmcx_simuind(mcmcx_handle h) { return h ? h->simuind : -1; }



int mcmcx_get_counters(mcmcx_handle h, int32_t chain, int32_t *out)
{
    int rc = check_chain(h, chain); if (rc) return rc;
    std::vector<uint32_t> v;
    if ((rc = fetch_chain_vec(h, h->E.ictr, NICTR, chain, v))) return rc;
    out[0] = (int32_t)v[I_STAYED]; out[1] = (int32_t)v[I_BNDSTAYED]; out[2] = (int32_t)v[I_DRACC]; out[3] = (int32_t)v[I_DRTRIES];
    out[4] = (int32_t)v[I_CHAININD]; out[5] = (int32_t)v[I_STATUS]; out[6] = (int32_t)v[I_ERSTAYED]; out[7] = (int32_t)v[I_CURCOUNT];
    return 0;
}

int mcmcx_get_totals_n(mcmcx_handle h, int64_t *out, int32_t n)
{
    if (!out || n < 1) return fail(-1, "mcmcx_get_totals_n: bad argument");
    int64_t t7[7];
    int rc = mcmcx_get_totals(h, t7); if (rc) return rc;
    for (int i = 0; i < n; ++i) out[i] = i < 7 ? t7[i] : 0;
    return 0;
}

int mcmcx_get_totals(mcmcx_handle h, int64_t *t7)
{
    if (!h || !h->inited) return fail(-40, "we have not inited");
    std::vector<uint32_t> v;
    int rc = fetch(h, h->E.ictr, (size_t)h->nlanes * NICTR, v); if (rc) return rc;
    for (int i = 0; i < 7; ++i) t7[i] = 0;
    for (int c = 0; c < h->cfg.nchains; ++c) {
        int t = c / 64, l = c % 64;
        auto at = [&](int k) { return (int64_t)v[((size_t)t * NICTR + k) * 64 + l]; };
        t7[0] += at(I_STAYED); t7[1] += at(I_BNDSTAYED); t7[2] += at(I_DRACC); t7[3] += at(I_DRTRIES);
        t7[5] += at(I_DOWNS); t7[6] |= at(I_STATUS);
    }
    t7[6] |= h->pool.status;                            // pooled RAM: a tick whose Gram matrix was not positive definite was skipped
    // proposals evaluated: one per iteration (d componentwise ones with method='scam') + the delayed-rejection tries
    t7[4] = (int64_t)h->cfg.nchains * (int64_t)(h->simuind - 1) * (h->cfg.method == MCMCX_METHOD_SCAM ? h->d : 1) + t7[3];
    return 0;
}

int mcmcx_get_theta(mcmcx_handle h, double *out)
{
    if (!h || !h->inited) return fail(-40, "we have not inited");
    std::vector<double> v;
    int rc = fetch(h, h->E.theta, (size_t)h->nlanes * h->d, v); if (rc) return rc;
    for (int c = 0; c < h->cfg.nchains; ++c)
        for (int k = 0; k < h->d; ++k) out[(size_t)c * h->d + k] = v[((size_t)(c / 64) * h->d + k) * 64 + (c % 64)];
    return 0;
}

int mcmcx_get_scalars(mcmcx_handle h, double *out)
{
    if (!h || !h->inited) return fail(-40, "we have not inited");
    std::vector<double> v;
    int rc = fetch(h, h->E.scal, (size_t)h->nlanes * NSCAL, v); if (rc) return rc;
    const int idx[4] = {S_SS1, S_PRI1, S_SIGMA2, S_ALPHA12};
    for (int c = 0; c < h->cfg.nchains; ++c)
        for (int k = 0; k < 4; ++k) out[(size_t)c * 4 + k] = v[((size_t)(c / 64) * NSCAL + idx[k]) * 64 + (c % 64)];
    return 0;
}

int mcmcx_get_rng(mcmcx_handle h, int32_t chain, uint64_t *n, int32_t *saved, double *saved_y)
{
    int rc = check_chain(h, chain); if (rc) return rc;
    std::vector<uint64_t> vn; std::vector<uint32_t> vi; std::vector<double> vs;
    if ((rc = fetch_chain_vec(h, h->E.rngn, 1, chain, vn))) return rc;
    if ((rc = fetch_chain_vec(h, h->E.ictr, NICTR, chain, vi))) return rc;
    if ((rc = fetch_chain_vec(h, h->E.scal, NSCAL, chain, vs))) return rc;
    if (n) *n = vn[0];
    if (saved) *saved = (int32_t)vi[I_SAVED];
    if (saved_y) *saved_y = vs[S_SAVEDY];
    return 0;
}

int mcmcx_get_R(mcmcx_handle h, int32_t chain, double *R)
{
    int rc = check_chain(h, chain); if (rc) return rc;
    std::vector<double> p;
    if (h->pooled) { pooled_out(h, pooled_R(h), !h->usesvd, R); return 0; }
    if (h->usesvd) {                                     // full column-major factor
        if ((rc = fetch_chain_vec(h, h->E.Rf, h->d * h->d, chain, p))) return rc;
        memcpy(R, p.data(), sizeof(double) * p.size());
        return 0;
    }
    if ((rc = fetch_chain_vec(h, h->E.R, h->P, chain, p))) return rc;
    unpack_upper(h->d, p, R, false);
    return 0;
}

int mcmcx_get_qcovstd(mcmcx_handle h, int32_t chain, double *std)
{
    int rc = check_chain(h, chain); if (rc) return rc;
    if (h->pooled && h->cfg.method == MCMCX_METHOD_SCAM) { pooled_out(h, h->pool.std, false, std); return 0; }
    if (!h->E.qstd) return fail(-45, "no SVD state (condmax = 0)");
    std::vector<double> p;
    if ((rc = fetch_chain_vec(h, h->E.qstd, h->d, chain, p))) return rc;
    memcpy(std, p.data(), sizeof(double) * p.size());
    return 0;
}

int mcmcx_get_dr(mcmcx_handle h, int32_t chain, double *R2, double *iC)
{
    int rc = check_chain(h, chain); if (rc) return rc;
    if (!h->dodr) return fail(-43, "drscale = 0: no delayed-rejection state");
    std::vector<double> p;
    if (h->pooled) {                                    // one pair of tables for every chain
        pooled_out(h, h->pool.R2, !h->usesvd, R2);
        pooled_out(h, h->pool.iC, true, iC);
        return 0;
    }
    if (R2 && h->usesvd) { if ((rc = fetch_chain_vec(h, h->E.R2f, h->d * h->d, chain, p))) return rc; memcpy(R2, p.data(),
        sizeof(double) * p.size()); }
    else if (R2) { if ((rc = fetch_chain_vec(h, h->E.R2, h->P, chain, p))) return rc; unpack_upper(h->d, p, R2, false); }
    if (iC) { if ((rc = fetch_chain_vec(h, h->E.iC, h->P, chain, p))) return rc; unpack_upper(h->d, p, iC, false); }
    return 0;
}

int mcmcx_get_chaincov(mcmcx_handle h, int32_t chain, double *cmat, double *mean, double *wsum)
{
    int rc = check_chain(h, chain); if (rc) return rc;
    std::vector<double> s;
    if ((rc = fetch_chain_vec(h, h->E.scal, NSCAL, chain, s))) return rc;
    if (wsum) *wsum = s[S_WSUM];
    if (!h->E.cmat) {                                   // no AM state on the device: chaincmat = cmat0, chainmean = the chain's start
        if (cmat) memcpy(cmat, h->cmat0.data(), sizeof(double) * (size_t)h->d * h->d);
        if (mean && h->E.start) {
            std::vector<double> m;
            if ((rc = fetch_chain_vec(h, h->E.start, h->d, chain, m))) return rc;
            memcpy(mean, m.data(), sizeof(double) * (size_t)h->d);
        } else if (mean) memcpy(mean, h->par0.data(), sizeof(double) * (size_t)h->d);
        return 0;
    }
    std::vector<double> p, m;
    if ((rc = fetch_chain_vec(h, h->E.cmat, h->P, chain, p))) return rc;
    if ((rc = fetch_chain_vec(h, h->E.mean, h->d, chain, m))) return rc;
    if (cmat) unpack_upper(h->d, p, cmat, true);
    if (mean) memcpy(mean, m.data(), sizeof(double) * (size_t)h->d);
    return 0;
}

int mcmcx_get_accept_masks(mcmcx_handle h, uint64_t *masks, int32_t *ntiles)
{
    if (!h || !h->inited) return fail(-40, "we have not inited");
    if (ntiles) *ntiles = h->ntiles;
    if (!h->E.accmask) return fail(-42, "record_accept was not requested");
    if (!masks) return 0;
    std::vector<uint64_t> v;
    int rc = fetch(h, h->E.accmask, (size_t)h->simuind * h->ntiles, v); if (rc) return rc;
    memcpy(masks, v.data(), v.size() * 8);
    return 0;
}

int mcmcx_get_accepted(mcmcx_handle h, int32_t chain, uint8_t *acc)
{
    int rc = check_chain(h, chain); if (rc) return rc;
    const int tile = chain / 64, lane = chain % 64;
    if (h->E.accmask) {
        std::vector<uint64_t> v;
        if ((rc = fetch(h, h->E.accmask, (size_t)h->simuind * h->ntiles, v))) return rc;
        for (int it = 1; it <= h->simuind; ++it) acc[it - 1] = (uint8_t)((v[(size_t)(it - 1) * h->ntiles + tile] >> lane) & 1ull);
        return 0;
    }
    if (h->cfg.record_chain && h->E.wacc) {
        std::vector<uint64_t> v;
        if ((rc = fetch(h, h->E.wacc + (size_t)tile * h->wcap, (size_t)h->wcap, v))) return rc;
        for (int it = 1; it <= h->simuind; ++it) acc[it - 1] = (uint8_t)((v[it % h->wcap] >> lane) & 1ull);
        return 0;
    }
    return fail(-42, "record_accept / record_chain was not requested");
}

int mcmcx_get_chain(mcmcx_handle h, int32_t chain, double *chain_out, double *ss_out, double *s2_out, int32_t *nrows)
{
    int rc = check_chain(h, chain); if (rc) return rc;
    if (!h->cfg.record_chain || !h->E.hist) return fail(-42, "record_chain was not requested");
    const int tile = chain / 64, lane = chain % 64, d = h->d, W = h->wcap;
    std::vector<uint64_t> m;
    if ((rc = fetch(h, h->E.wacc + (size_t)tile * W, (size_t)W, m))) return rc;
    // this chain's lane of the history ring, gathered on the device: hv[slot*(d+1) + k]
    auto gather = [&](const double *src, size_t n, std::vector<double> &dst) -> int {
        double *tmp = nullptr;
        HIPCHK(hipMalloc(&tmp, n * sizeof(double)));       // (freed on every path below)
        hipLaunchKernelGGL(gather_lane_kernel, dim3((unsigned)std::min<size_t>((n + 255) / 256, 4096)), dim3(256), 0, h->stream, src, tmp,
            n, lane);
        hipError_t e = hipGetLastError();
        if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
        dst.resize(n);
        if (e == hipSuccess) e = hipMemcpy(dst.data(), tmp, n * sizeof(double), hipMemcpyDeviceToHost);
        (void)hipFree(tmp);
        if (e != hipSuccess) return fail(-100, hipGetErrorString(e));
        return 0;
    };
    std::vector<double> hv;
    const int ny = h->ny, hs = d + ny;                  // history row: theta, ss per column
    if ((rc = gather(h->E.hist + (size_t)tile * W * hs * 64, (size_t)W * hs, hv))) return rc;
    int row = -1;
    for (int it = 1; it <= h->simuind; ++it) {
        const size_t so = (size_t)(it % W) * hs;
        if ((m[it % W] >> lane) & 1ull) {
            ++row;
            if (chain_out) {
                for (int k = 0; k < d; ++k) chain_out[(size_t)row * (d + 1) + k] = hv[so + k];
                chain_out[(size_t)row * (d + 1) + d] = 1.0;
            }
            if (ss_out) { for (int j = 0; j < ny; ++j) ss_out[(size_t)row * (ny + 1) + j] = hv[so + d + j];
                ss_out[(size_t)row * (ny + 1) + ny] = 1.0; }
        } else {
            if (chain_out) chain_out[(size_t)row * (d + 1) + d] += 1.0;
            if (ss_out) ss_out[(size_t)row * (ny + 1) + ny] += 1.0;
        }
    }
    if (nrows) *nrows = row + 1;
    if (s2_out && h->E.s2hist) {
        std::vector<double> sv;
        if ((rc = gather(h->E.s2hist + (size_t)tile * W * ny * 64, (size_t)W * ny, sv))) return rc;
        for (int it = 1; it <= h->simuind; ++it) for (int j = 0; j < ny;
            ++j) s2_out[(size_t)(it - 1) * ny + j] = sv[(size_t)(it % W) * ny + j];
    }
    return 0;
}

int32_t mcmcx_samples_kept(mcmcx_handle h, int32_t *oldest_iteration, int32_t *thin, int32_t *nfields)
{
    if (!h) return -1;
    const long long have = samples_retained(h);
    if (oldest_iteration) *oldest_iteration = (int32_t)(h->samp.first + (h->samp.kept - have) * h->samp.thin);
    if (thin) *thin = h->samp.thin;
    if (nfields) *nfields = samples_nfields(h);
    return (int32_t)have;
}

int mcmcx_get_samples_dev(mcmcx_handle h, int32_t s0, int32_t ns, int32_t c0, int32_t nc, int32_t layout, void *dev_out)
{
    int rc = samples_check(h, s0, ns, c0, nc, layout, dev_out, "mcmcx_get_samples_dev"); if (rc) return rc;
    return samples_read(h, s0, ns, c0, nc, layout, (double *)dev_out);
}

int mcmcx_get_samples(mcmcx_handle h, int32_t s0, int32_t ns, int32_t c0, int32_t nc, int32_t layout, double *host_out)
{
    int rc = samples_check(h, s0, ns, c0, nc, layout, host_out, "mcmcx_get_samples"); if (rc) return rc;
    HIPCHK(hipSetDevice(h->cfg.device));
    const size_t bytes = (size_t)ns * (size_t)nc * (size_t)samples_nfields(h) * sizeof(double);
    DevBufs g;
    double *tmp = nullptr;
    if (g.alloc(&tmp, bytes) != hipSuccess) return fail(-101, "mcmcx_get_samples: hipMalloc of " + std::to_string(bytes) + " bytes failed");
    if ((rc = samples_read(h, s0, ns, c0, nc, layout, tmp))) return rc;
    return samples_fetch(h, host_out, tmp, bytes);
}

// ------------------------------------------------------------------ the sample store's convergence summary (mcx_host_diag.hpp)
int32_t mcmcx_samples_stats_len(mcmcx_handle h, int32_t maxlag)
{
    if (!h) return fail(-49, "mcmcx_samples_stats_len: null handle");
    if (maxlag < 0 || maxlag > MCMCX_DIAG_MAXLAG) return fail(-49, "mcmcx_samples_stats_len: maxlag " + std::to_string(maxlag) +
        " outside 0 .. " + std::to_string(MCMCX_DIAG_MAXLAG));
    return diag_stats_len(samples_nfields(h), maxlag);
}

int mcmcx_samples_stats_dev(mcmcx_handle h, int32_t s0, int32_t ns, int32_t maxlag, const double *shift, void *dev_out)
{
    return diag_run(h, s0, ns, maxlag, XF_IDENTITY, nullptr, shift, dev_out, nullptr, "mcmcx_samples_stats_dev");
}

int mcmcx_samples_stats(mcmcx_handle h, int32_t s0, int32_t ns, int32_t maxlag, const double *shift, double *host_out)
{
    return diag_run(h, s0, ns, maxlag, XF_IDENTITY, nullptr, shift, nullptr, host_out, "mcmcx_samples_stats");
}

// ... of an elementwise function of the stored values (mcx_diag_xf.hpp): kind 0 runs the summary's own kernels
int mcmcx_samples_stats_of_dev(mcmcx_handle h, int32_t s0, int32_t ns, int32_t maxlag, int32_t kind, const double *a, const double *shift,
                               void *dev_out)
{
    return diag_run(h, s0, ns, maxlag, kind, a, shift, dev_out, nullptr, "mcmcx_samples_stats_of_dev", -53);
}

int mcmcx_samples_stats_of(mcmcx_handle h, int32_t s0, int32_t ns, int32_t maxlag, int32_t kind, const double *a, const double *shift,
                           double *host_out)
{
    return diag_run(h, s0, ns, maxlag, kind, a, shift, nullptr, host_out, "mcmcx_samples_stats_of", -53);
}

// ... of a step function of the stored values, u_f(x) = table_f[cell_f(x)] (mcx_diag_step.hpp)
int mcmcx_samples_stats_step_dev(mcmcx_handle h, int32_t s0, int32_t ns, int32_t maxlag, int32_t nbins, const double *edges,
                                 const double *table, const double *shift, void *dev_out)
{
    return diag_step_run(h, s0, ns, maxlag, nbins, edges, table, shift, dev_out, nullptr, "mcmcx_samples_stats_step_dev");
}

int mcmcx_samples_stats_step(mcmcx_handle h, int32_t s0, int32_t ns, int32_t maxlag, int32_t nbins, const double *edges,
                             const double *table, const double *shift, double *host_out)
{
    return diag_step_run(h, s0, ns, maxlag, nbins, edges, table, shift, nullptr, host_out, "mcmcx_samples_stats_step");
}

// the table of normal scores from 1-D histogram counts: pure host, no handle, no device
int mcmcx_samples_rank_scores(const int64_t *counts, int32_t nfields, int32_t nbins, double *scores_out)
{
    if (!counts || !scores_out) return fail(-54, "mcmcx_samples_rank_scores: null argument");
    if (nfields < 1) return fail(-54, "mcmcx_samples_rank_scores: nfields < 1");
    if (nbins < 1 || nbins > MCMCX_STEP_MAXBINS) return fail(-54, "mcmcx_samples_rank_scores: " + std::to_string(nbins) +
        " bins, outside 1 .. " + std::to_string(MCMCX_STEP_MAXBINS));
    return step_rank_scores(counts, nfields, nbins, scores_out);
}

int mcmcx_samples_diag(const double *stats, int32_t nfields, int32_t maxlag, double *table)
{
    if (!stats || !table) return fail(-49, "mcmcx_samples_diag: null argument");
    if (nfields < 1) return fail(-49, "mcmcx_samples_diag: nfields < 1");
    if (maxlag < 0 || maxlag > MCMCX_DIAG_MAXLAG) return fail(-49, "mcmcx_samples_diag: maxlag " + std::to_string(maxlag) +
        " outside 0 .. " + std::to_string(MCMCX_DIAG_MAXLAG));
    return diag_finish(stats, nfields, maxlag, table);
}

// ------------------------------------------------------------------ order statistics, counts, quantiles of the store (mcx_host_quant.hpp)
int mcmcx_samples_order_stats_dev(mcmcx_handle h, int32_t s0, int32_t ns, int32_t nr, const int64_t *ranks, void *dev_out)
{
    return quant_order_stats_run(h, s0, ns, nr, ranks, dev_out, nullptr, "mcmcx_samples_order_stats_dev");
}

int mcmcx_samples_order_stats(mcmcx_handle h, int32_t s0, int32_t ns, int32_t nr, const int64_t *ranks, double *host_out)
{
    return quant_order_stats_run(h, s0, ns, nr, ranks, nullptr, host_out, "mcmcx_samples_order_stats");
}

int mcmcx_samples_counts_dev(mcmcx_handle h, int32_t s0, int32_t ns, int32_t nq, const double *x, void *dev_out)
{
    return quant_counts_run(h, s0, ns, nq, x, dev_out, nullptr, "mcmcx_samples_counts_dev");
}

int mcmcx_samples_counts(mcmcx_handle h, int32_t s0, int32_t ns, int32_t nq, const double *x, int64_t *host_out)
{
    return quant_counts_run(h, s0, ns, nq, x, nullptr, host_out, "mcmcx_samples_counts");
}

int mcmcx_samples_quantile_ranks(int64_t n, int32_t nq, const double *probs, int64_t *ranks, double *frac)
{
    if (!probs || !ranks || !frac) return fail(-50, "mcmcx_samples_quantile_ranks: null argument");
    if (nq < 1) return fail(-50, "mcmcx_samples_quantile_ranks: nq < 1");
    if (n < 1) return fail(-50, "mcmcx_samples_quantile_ranks: n < 1");
    return quant_ranks((long long)n, nq, probs, ranks, frac);
}

int mcmcx_samples_quantiles(mcmcx_handle h, int32_t s0, int32_t ns, int32_t nq, const double *probs, double *host_out)
{
    int rc = quant_check(h, s0, ns, nq, probs, host_out, "mcmcx_samples_quantiles"); if (rc) return rc;
    if (nq > MCMCX_QUANT_MAXR / 2) return fail(-50, "mcmcx_samples_quantiles: " + std::to_string(nq) + " probabilities, at most " +
        std::to_string(MCMCX_QUANT_MAXR / 2) + " (two ranks each)");
    int64_t ranks[MCMCX_QUANT_MAXR];
    double frac[MCMCX_QUANT_MAXR / 2];
    if ((rc = quant_ranks((long long)ns * h->cfg.nchains, nq, probs, ranks, frac))) return rc;
    const int nf = samples_nfields(h);
    std::vector<double> os((size_t)nf * (size_t)nq * 2);
    if ((rc = mcmcx_samples_order_stats(h, s0, ns, 2 * nq, ranks, os.data()))) return rc;
    quant_finish(os.data(), frac, nf, nq, host_out);
    return 0;
}

// ------------------------------------------------------------------ the sample store's posterior covariance (mcx_host_cov.hpp)
int32_t mcmcx_samples_cov_len(mcmcx_handle h)
{
    if (!h) return fail(-51, "mcmcx_samples_cov_len: null handle");
    return (int32_t)cov_vec_len(samples_nfields(h));
}

int mcmcx_samples_cov_dev(mcmcx_handle h, int32_t s0, int32_t ns, const double *shift, void *dev_out)
{
    return cov_run(h, s0, ns, shift, dev_out, nullptr, "mcmcx_samples_cov_dev");
}

int mcmcx_samples_cov(mcmcx_handle h, int32_t s0, int32_t ns, const double *shift, double *host_out)
{
    return cov_run(h, s0, ns, shift, nullptr, host_out, "mcmcx_samples_cov");
}

int mcmcx_samples_cov_finish(const double *vec, int32_t nfields, double *mean, double *cov, double *corr)
{
    if (!vec || !mean || !cov) return fail(-51, "mcmcx_samples_cov_finish: null argument");
    if (nfields < 1) return fail(-51, "mcmcx_samples_cov_finish: nfields < 1");
    return cov_finish(vec, nfields, mean, cov, corr);
}


// ------------------------------------------------------------------ the sample store's batch-means covariance and its finishes (mcx_host_bm.hpp)
int mcmcx_samples_cov_bm_dev(mcmcx_handle h, int32_t s0, int32_t ns, int32_t batch, const double *shift, void *dev_out)
{
    return bm_run(h, s0, ns, batch, shift, dev_out, nullptr, "mcmcx_samples_cov_bm_dev");
}

int mcmcx_samples_cov_bm(mcmcx_handle h, int32_t s0, int32_t ns, int32_t batch, const double *shift, double *host_out)
{
    return bm_run(h, s0, ns, batch, shift, nullptr, host_out, "mcmcx_samples_cov_bm");
}

int mcmcx_samples_mess(const double *cov_vec, const double *bm_vec, int32_t nfields, int32_t batch, int32_t nsel, const int32_t *sel,
                       double *out4, double *ess_out)
{
    const char *who = "mcmcx_samples_mess";
    int rc = bm_finish_check(cov_vec, bm_vec, nfields, nsel, sel, out4, who); if (rc) return rc;
    if (batch < 1) return fail(-55, std::string(who) + ": batch < 1");
    if (bm_vec[0] * (double)batch != cov_vec[0]) return fail(-55, std::string(who) + ": the two vectors do not cover the same samples "
        "(bm_vec[0] * batch must be cov_vec[0])");
    return bm_mess(cov_vec, bm_vec, nfields, batch, nsel, sel, out4, ess_out);
}

int mcmcx_samples_mpsrf(const double *cov_vec, const double *bm_vec, int32_t nfields, int32_t n_h, int32_t nsel, const int32_t *sel,
                        double *out4, double *W_out, double *Bn_out)
{
    const char *who = "mcmcx_samples_mpsrf";
    int rc = bm_finish_check(cov_vec, bm_vec, nfields, nsel, sel, out4, who); if (rc) return rc;
    if (n_h < 2) return fail(-55, std::string(who) + ": n_h < 2");
    const double M = bm_vec[0];
    if (M != 2.0 * std::floor(M / 2.0) || M * (double)n_h != cov_vec[0]) return fail(-55, std::string(who) + ": bm_vec must hold the two "
        "half-window means of every chain (bm_vec[0] even, bm_vec[0] * n_h = cov_vec[0])");
    return bm_mpsrf(cov_vec, bm_vec, nfields, n_h, nsel, sel, out4, W_out, Bn_out);
}

// ------------------------------------------------------------------ marginal and joint histograms of the store (mcx_host_hist.hpp)
int mcmcx_samples_hist_dev(mcmcx_handle h, int32_t s0, int32_t ns, int32_t nbins, const double *edges, void *dev_out)
{
    return hist_run(h, s0, ns, false, 0, nullptr, nbins, edges, dev_out, nullptr, "mcmcx_samples_hist_dev");
}

int mcmcx_samples_hist(mcmcx_handle h, int32_t s0, int32_t ns, int32_t nbins, const double *edges, int64_t *host_out)
{
    return hist_run(h, s0, ns, false, 0, nullptr, nbins, edges, nullptr, host_out, "mcmcx_samples_hist");
}

int mcmcx_samples_hist2_dev(mcmcx_handle h, int32_t s0, int32_t ns, int32_t npairs, const int32_t *pairs, int32_t nbins,
                            const double *edges, void *dev_out)
{
    return hist_run(h, s0, ns, true, npairs, pairs, nbins, edges, dev_out, nullptr, "mcmcx_samples_hist2_dev");
}

int mcmcx_samples_hist2(mcmcx_handle h, int32_t s0, int32_t ns, int32_t npairs, const int32_t *pairs, int32_t nbins, const double *edges,
                        int64_t *host_out)
{
    return hist_run(h, s0, ns, true, npairs, pairs, nbins, edges, nullptr, host_out, "mcmcx_samples_hist2");
}

int mcmcx_samples_hist_edges(double lo, double hi, int32_t nbins, double *edges_out)
{
    if (!edges_out) return fail(-52, "mcmcx_samples_hist_edges: null output");
    if (nbins < 1 || nbins > MCMCX_HIST_MAXBINS) return fail(-52, "mcmcx_samples_hist_edges: " + std::to_string(nbins) +
        " bins, outside 1 .. " + std::to_string(MCMCX_HIST_MAXBINS));
    return hist_edges(lo, hi, nbins, edges_out);
}

int mcmcx_samples_hist_density(const int64_t *counts, const double *edges, int32_t nfields, int32_t nbins, double *density_out)
{
    if (!counts || !edges || !density_out) return fail(-52, "mcmcx_samples_hist_density: null argument");
    if (nfields < 1) return fail(-52, "mcmcx_samples_hist_density: nfields < 1");
    if (nbins < 1 || nbins > MCMCX_HIST_MAXBINS) return fail(-52, "mcmcx_samples_hist_density: " + std::to_string(nbins) +
        " bins, outside 1 .. " + std::to_string(MCMCX_HIST_MAXBINS));
    hist_density(counts, edges, nfields, nbins, density_out);
    return 0;
}


int32_t mcmcx_pooled_moments_len(mcmcx_handle h) { return h ? 1 + h->d + h->P : -1; }

static int pooled_vec_len(const mcmcx_engine *h, int kind) { return kind == 2 ? 2 + h->P : 1 + h->d + h->P + (kind == 1 ? 1 : 0); }

static int pooled_moments_launch(mcmcx_engine *h, double *dev_dst, int kind, int it)
{   // (declared above)
    if (!h || !h->inited) return fail(-40, "we have not inited");
    HIPCHK(hipSetDevice(h->cfg.device));
    const int len = pooled_vec_len(h, kind), T = h->ntiles;
    const double rs = (kind == 2) ? 1.0 / std::pow((double)(float)it, h->cfg.nuparam) : 0.0;      // like d_ramscale (MCMC_run_ram.F90:166)
    const size_t mlds = MomentsLds(h->d, false).bytes;
    if (mlds <= LDS_PER_CU) hipLaunchKernelGGL(moments_kernel<false>, dim3(T), dim3(256), mlds, h->stream, h->E, h->d_moments,
        h->cfg.nchains, kind, it, rs);
    // npar >= 316: (64 (d | 1) + 320) 8 bytes exceed 160 KiB (317: 164 864)
    else hipLaunchKernelGGL(moments_kernel<true>, dim3(T), dim3(256), MomentsLds(h->d, true).bytes, h->stream, h->E, h->d_moments,
        h->cfg.nchains, kind, it, rs);
    moments_tree_launch(h->stream, h->d_moments, T, len, dev_dst);
    HIPCHK(hipGetLastError());
    return 0;
}

int mcmcx_pooled_moments(mcmcx_handle h, double *out)
{
    int rc = pooled_moments_launch(h, nullptr, 0, 0); if (rc) return rc;
    std::vector<double> v;
    if ((rc = fetch(h, h->d_moments, (size_t)(1 + h->d + h->P), v))) return rc;
    memcpy(out, v.data(), sizeof(double) * v.size());
    return 0;
}

int mcmcx_set_exchange(mcmcx_handle h, mcmcx_exchange_t fn, void *user, void *dev_buf)
{
    if (!h) return fail(-1, "null handle");
    if (fn && !dev_buf) return fail(-1, "mcmcx_set_exchange: dev_buf is required");
    h->xfn = fn; h->xuser = user; h->xbuf = (double *)dev_buf;
    return 0;
}

int mcmcx_get_pooled(mcmcx_handle h, double *cmat, double *mean, double *wsum, double *R)
{
    if (!h || !h->inited) return fail(-40, "we have not inited");
    if (!h->pooled) return fail(-44, "not in pooled mode");
    if (cmat) unpack_upper(h->d, h->pool.C, cmat, true);
    if (mean) memcpy(mean, h->pool.mean.data(), sizeof(double) * (size_t)h->d);
    if (wsum) *wsum = h->pool.W;
    pooled_out(h, pooled_R(h), !h->usesvd, R);                  // scam: the rotation U; condmax > 0: the full SVD factor; column-major
    return 0;
}

/* same, result left in device memory at dev_out (e.g. the buffer an RCCL all-reduce works on);
 * asynchronous on the engine's stream: call mcmcx_sync before another stream reads it */
int mcmcx_pooled_moments_dev(mcmcx_handle h, void *dev_out)
{
    if (!dev_out) return fail(-1, "null argument");
    return pooled_moments_launch(h, (double *)dev_out, 0, 0);
}

// ------------------------------------------------------------------ the node: several GPUs, one communicator
int mcmcx_set_comm(mcmcx_handle h, mcmcx_comm_t c)
{
    if (!h) return fail(-1, "null handle");
    if (h->inited) return fail(-1, "mcmcx_set_comm after mcmcx_init");
    if (c && c->device != h->cfg.device) return fail(-1, "mcmcx_set_comm: the communicator lives on device " + std::to_string(c->device)
        + ", the engine on " + std::to_string(h->cfg.device));
    h->comm = c;
    return 0;
}

int mcmcx_allreduce_moments(mcmcx_handle h, double *host_out)
{
    if (!h || !h->inited) return fail(-40, "we have not inited");
    if (h->comm && h->comm->single_process && h->comm->nranks > 1)
        return fail(-1, "mcmcx_allreduce_moments: this communicator drives several GPUs from one process; use mcmcx_allreduce_moments_all");
    int rc = allreduce_moments_enqueue(h, 0); if (rc) return rc;
    if (host_out) {
        HIPCHK(hipStreamSynchronize(h->stream));
        HIPCHK(hipMemcpy(host_out, h->d_pooled, (size_t)(1 + h->d + h->P) * 8, hipMemcpyDeviceToHost));
    }
    return 0;
}

int mcmcx_allreduce_moments_all(mcmcx_handle *hs, int32_t n, double *host_out)
{
    if (!hs || n < 1) return fail(-1, "bad argument");
    for (int i = 0; i < n; ++i) if (!hs[i] || !hs[i]->inited) return fail(-40, "we have not inited");
    int rc;
    for (int i = 0; i < n; ++i) if ((rc = allreduce_moments_enqueue(hs[i], 1))) return rc;
    NCCLCHK(ncclGroupStart());                                  // one thread, several devices: the gathers go out as a group
    for (int i = 0; i < n; ++i) if ((rc = allreduce_moments_enqueue(hs[i], 2))) { (void)ncclGroupEnd(); return rc; }
    NCCLCHK(ncclGroupEnd());
    for (int i = 0; i < n; ++i) if ((rc = allreduce_moments_enqueue(hs[i], 3))) return rc;
    if (host_out) {
        HIPCHK(hipSetDevice(hs[0]->cfg.device));
        HIPCHK(hipStreamSynchronize(hs[0]->stream));
        HIPCHK(hipMemcpy(host_out, hs[0]->d_pooled, (size_t)(1 + hs[0]->d + hs[0]->P) * 8, hipMemcpyDeviceToHost));
    }
    return 0;
}

// mcmcx_run on n engines at once, one host thread per engine (each GPU has its own stream; in pooled mode the threads
// meet in the all-gather of every adaptation tick).  User host callbacks are not thread-safe: engines with
// a host target run one after the other on the calling thread instead.
int mcmcx_run_all(mcmcx_handle *hs, int32_t n, int32_t upto)
{
    if (!hs || n < 1) return fail(-1, "bad argument");
    bool serial = (n == 1);
    for (int i = 0; i < n; ++i) { if (!hs[i]) return fail(-1, "null handle"); if (phased(hs[i]) && hs[i]->tkind == TGT_HOST) serial = true;
        }
    if (serial) {
        // (engines that meet in a communicator's ticks cannot run one after the other: the first would wait for the rest in its first tick)
        for (int i = 0; n > 1 && i < n; ++i) if (collective_run(hs[i])) return fail(-8, "mcmcx_run_all: pooled mode over a communicator "
            "with host callbacks needs one process per GPU (the callbacks run on the calling thread, one engine after the other); with a target "
            "module every engine has a thread of its own");
        int worst = 0;
        for (int i = 0; i < n; ++i) { int rc = mcmcx_run(hs[i], upto); if (rc < 0) return rc; worst = std::max(worst, rc); }
        return worst;
    }
    std::vector<int> rcs(n, 0); std::vector<std::string> errs(n);
    std::vector<std::thread> th;
    for (int i = 1; i < n; ++i) th.emplace_back([&, i]() { rcs[i] = mcmcx_run(hs[i], upto); if (rcs[i] < 0) errs[i] = g_err; });
    rcs[0] = mcmcx_run(hs[0], upto); if (rcs[0] < 0) errs[0] = g_err;
    for (auto &t : th) t.join();
    int worst = 0;
    for (int i = 0; i < n; ++i) { if (rcs[i] < 0) return fail(rcs[i], "engine " + std::to_string(i) + ": " + errs[i]);
        worst = std::max(worst, rcs[i]); }
    return worst;
}

} // extern "C"

extern "C" {
// ------------------------------------------------------------------ debug probes (tests only)
// The kernel-selection tables (launch_step / launch_group / launch_scam, pooled mode's phase forms): entry `index` as "family:name" into
// buf; returns the number of
// entries (so index = -1 with buf = NULL just counts).  Needs no device.
int mcmcx_debug_kernel_table(int32_t index, char *buf, int32_t len)
{
    const KernelEntry *tabs[] = {STEP_TABLE, GROUP_TABLE, SCAM_TABLE, PHASE_TABLE};
    const size_t ns[] = {sizeof(STEP_TABLE) / sizeof(STEP_TABLE[0]), sizeof(GROUP_TABLE) / sizeof(GROUP_TABLE[0]),
        sizeof(SCAM_TABLE) / sizeof(SCAM_TABLE[0]), sizeof(PHASE_TABLE) / sizeof(PHASE_TABLE[0])};
    int total = 0, k = index;
    for (int t = 0; t < 4; ++t) {
        if (k >= 0 && k < (int)ns[t] && buf && len > 0) { snprintf(buf, (size_t)len, "%s:%s", tabs[t][k].family, tabs[t][k].name);
            k = -1 - total - (int)ns[t]; }
        else if (k >= 0) k -= (int)ns[t];
        total += (int)ns[t];
    }
    return total;
}

// The template instance(s) behind the table name of the last run: the group launchers note theirs (launch_group_inst,
// launch_group_ram_d4), every other entry is its own name.  Reads two fields of the handle; nothing is launched.
int mcmcx_debug_last_instance(mcmcx_handle h, char *buf, int32_t len)
{
    const char *who = "mcmcx_debug_last_instance";
    if (!h || !buf) return fail(-57, std::string(who) + ": null argument");
    const std::string name = h->last_instance ? h->last_instance : mcmcx_last_kernel(h);
    if (len < 1 || (size_t)len <= name.size()) return fail(-57, std::string(who) + ": len too small for \"" + name + "\"");
    snprintf(buf, (size_t)len, "%s", name.c_str());
    return 0;
}

int64_t mcmcx_debug_samples_offset(int64_t slot, int64_t ntiles, int64_t nfields, int64_t tile, int64_t field)
{
    return (int64_t)samples_row((size_t)slot, (size_t)ntiles, (size_t)nfields, (size_t)tile, (size_t)field);
}

int64_t mcmcx_debug_quant_key(double x, int32_t inverse)
{
    unsigned long long b;
    memcpy(&b, &x, 8);
    return (int64_t)(inverse ? quant_unkey(b) : quant_key(b));
}

// the select's own kernels on a caller's array: a store of one slot, one field, ceil(n / 64) tiles and n chains; the padding lanes of
// the last tile are filled with all-ones words (the smallest key there is), which a select that counted them would return
int mcmcx_debug_order_stats(int32_t device, int64_t n, const double *values, int32_t nr, const int64_t *ranks, double *out)
{
    if (!values || !ranks || !out) return fail(-50, "mcmcx_debug_order_stats: null argument");
    if (nr < 1 || nr > MCMCX_QUANT_MAXR) return fail(-50, "mcmcx_debug_order_stats: nr outside 1 .. " + std::to_string(MCMCX_QUANT_MAXR));
    if (n < 1 || n > 2147483584ll) return fail(-50, "mcmcx_debug_order_stats: n outside 1 .. 2**31 - 64");
    int rc = quant_check_ranks((long long)n, nr, ranks, "mcmcx_debug_order_stats"); if (rc) return rc;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) return fail(-10, "no HIP device: the mcmcx engine has no CPU fallback");
    HIPCHK(hipSetDevice(device));
    const int T = (int)((n + 63) / 64);
    DevBufs g;
    double *store = nullptr, *dout = nullptr; unsigned long long *w = nullptr;
    HIPCHK(g.alloc(&store, (size_t)T * 512)); HIPCHK(g.alloc(&dout, (size_t)nr * 8));
    HIPCHK(g.alloc(&w, quant_select_words(1, nr) * sizeof(unsigned long long)));
    HIPCHK(hipMemset(store, 0xFF, (size_t)T * 512));
    HIPCHK(hipMemcpy(store, values, (size_t)n * 8, hipMemcpyHostToDevice));
    const SampleWin W = {store, 0, 1, T, 1, (int)n, 1};         // one slot, one field
    if ((rc = quant_select_launch(quant_window(W), w, nr, ranks, dout, 0))) return rc;
    HIPCHK(hipMemcpy(out, dout, (size_t)nr * 8, hipMemcpyDeviceToHost));
    return 0;
}

// the covariance's own kernels on a caller's array: a store of ns slots, ceil(nchains / 64) tiles and nfields fields filled from
// values[ns][nfields][nchains]; the padding lanes of the last tile hold NaN, which a kernel that multiplied them by zero would spread
int mcmcx_debug_samples_cov(int32_t device, int32_t nchains, int32_t nfields, int32_t ns, const double *values, const double *shift,
                            double *out)
{
    if (!values || !out) return fail(-51, "mcmcx_debug_samples_cov: null argument");
    if (nchains < 1 || nfields < 1 || nfields > 2047 || ns < 1) return fail(-51, "mcmcx_debug_samples_cov: nchains, ns < 1 or nfields "
        "outside 1 .. 2047");
    const size_t work = cov_work_len((nchains + 63) / 64, nfields), vlen = cov_vec_len(nfields);
    DebugStore D;
    int rc = D.open(device, nchains, nfields, ns, values, (work + vlen) * 8); if (rc) return rc;
    double *w = (double *)D.scratch;
    if ((rc = cov_launch(D.win, w, shift, w + work, 0))) return rc;
    return D.fetch(out, w + work, vlen * 8);
}

// the batch-means covariance's own kernels on a caller's array, as mcmcx_debug_samples_cov lays it out: values[ns][nfields][nchains], the
// padding lanes of the last tile hold NaN, which a kernel that summed or multiplied them would spread
int mcmcx_debug_samples_cov_bm(int32_t device, int32_t nchains, int32_t nfields, int32_t ns, int32_t batch, const double *values,
                               const double *shift, double *out)
{
    if (!values || !out) return fail(-55, "mcmcx_debug_samples_cov_bm: null argument");
    if (nchains < 1 || nfields < 1 || nfields > 2047 || ns < 1) return fail(-55, "mcmcx_debug_samples_cov_bm: nchains, ns < 1 or nfields "
        "outside 1 .. 2047");
    if (batch < 1 || batch > ns) return fail(-55, "mcmcx_debug_samples_cov_bm: batch outside 1 .. ns");
    const size_t work = cov_work_len((nchains + 63) / 64, nfields), vlen = cov_vec_len(nfields);
    DebugStore D;
    int rc = D.open(device, nchains, nfields, ns, values, (work + vlen) * 8); if (rc) return rc;
    double *w = (double *)D.scratch;
    if ((rc = bm_launch(D.win, batch, w, shift, w + work, 0))) return rc;
    return D.fetch(out, w + work, vlen * 8);
}

// the summary's own kernels, of u(x), on a caller's array: a store of ns slots, ceil(nchains / 64) tiles and nfields fields filled from
// values[ns][nfields][nchains]; the padding lanes of the last tile hold NaN, which a kernel that did not mask them would sum -- and under
// kind 1 with a positive-NaN a count
int mcmcx_debug_samples_stats(int32_t device, int32_t nchains, int32_t nfields, int32_t ns, const double *values, int32_t maxlag,
                              int32_t kind, const double *a, const double *shift, double *out)
{
    const char *who = "mcmcx_debug_samples_stats";
    int rc = diag_xf_check(kind, a, who); if (rc) return rc;
    if (!values || !out) return fail(-53, std::string(who) + ": null argument");
    if (nchains < 1 || nfields < 1 || ns < 4) return fail(-53, std::string(who) + ": nchains, nfields < 1 or ns < 4");
    if (maxlag < 0 || maxlag > MCMCX_DIAG_MAXLAG) return fail(-53, std::string(who) + ": maxlag " + std::to_string(maxlag) +
        " outside 0 .. " + std::to_string(MCMCX_DIAG_MAXLAG));
    const size_t work = diag_work_len((nchains + 63) / 64, nfields, maxlag, kind), slen = (size_t)diag_stats_len(nfields, maxlag);
    DebugStore D;
    if ((rc = D.open(device, nchains, nfields, ns, values, (work + slen) * 8))) return rc;
    double *w = (double *)D.scratch;
    if ((rc = diag_launch(D.win, w, maxlag, kind, a, shift, w + work, 0))) return rc;
    return D.fetch(out, w + work, slen * 8);
}

// the step summary's own kernels on a caller's array, laid out as mcmcx_debug_samples_stats lays it out: the padding lanes of the last
// tile hold NaN, which a kernel that did not mask them would look up (the last cell) and sum
int mcmcx_debug_samples_stats_step(int32_t device, int32_t nchains, int32_t nfields, int32_t ns, const double *values, int32_t maxlag,
                                   int32_t nbins, const double *edges, const double *table, const double *shift, double *out)
{
    const char *who = "mcmcx_debug_samples_stats_step";
    int rc = diag_step_check_args(nbins, edges, table, out, who); if (rc) return rc;
    if (!values) return fail(-54, std::string(who) + ": null values");
    if (nchains < 1 || nfields < 1 || ns < 4) return fail(-54, std::string(who) + ": nchains, nfields < 1 or ns < 4");
    if (maxlag < 0 || maxlag > MCMCX_DIAG_MAXLAG) return fail(-54, std::string(who) + ": maxlag " + std::to_string(maxlag) +
        " outside 0 .. " + std::to_string(MCMCX_DIAG_MAXLAG));
    if ((rc = hist_check_edges(edges, nfields, nbins, who, -54))) return rc;
    const size_t work = diag_step_work_len((nchains + 63) / 64, nfields, maxlag, nbins), slen = (size_t)diag_stats_len(nfields, maxlag);
    DebugStore D;
    if ((rc = D.open(device, nchains, nfields, ns, values, (work + slen) * 8))) return rc;
    double *w = (double *)D.scratch;
    if ((rc = diag_step_launch(D.win, w, maxlag, nbins, edges, table, shift, w + work, 0))) return rc;
    return D.fetch(out, w + work, slen * 8);
}

// the histograms' own kernels on a caller's array: a store of ns slots, ceil(nchains / 64) tiles and nfields fields filled from
// values[ns][nfields][nchains]; the padding lanes of the last tile hold NaN, which a kernel that counted them would put into the last cell
int mcmcx_debug_samples_hist(int32_t device, int32_t nchains, int32_t nfields, int32_t ns, const double *values, int32_t nbins,
                             const double *edges, int32_t npairs, const int32_t *pairs, int32_t chunk, int64_t *out1, int64_t *out2)
{
    const char *who = "mcmcx_debug_samples_hist";
    if (!values) return fail(-52, std::string(who) + ": null values");
    int rc = hist_check_args(nbins, out2 ? MCMCX_HIST2_MAXBINS : MCMCX_HIST_MAXBINS, edges, out1 ? (void *)out1 : (void *)out2, who);
    if (rc) return rc;
    if (out2 && (rc = hist_check_npairs(npairs, pairs, who))) return rc;
    if (nchains < 1 || nfields < 1 || ns < 1 || chunk < 0) return fail(-52, std::string(who) + ": nchains, nfields, ns < 1 or chunk < 0");
    if ((rc = hist_check_edges(edges, nfields, nbins, who))) return rc;
    if (out2 && (rc = hist_check_pairs(pairs, npairs, nfields, who))) return rc;
    const size_t m = hist_key_words(nfields, nbins), n1 = hist_table_words(nfields, 0, nbins);
    const size_t n2 = out2 ? hist_table_words(nfields, npairs, nbins) : 0;
    DebugStore D;
    if ((rc = D.open(device, nchains, nfields, ns, values, (m + std::max(n1, n2)) * 8))) return rc;
    unsigned long long *w = (unsigned long long *)D.scratch;
    const QuantWin A = hist_window(D.win, chunk);
    if (out1 && ((rc = hist_launch(A, w, nbins, edges, 0, nullptr, w + m, 0)) || (rc = D.fetch(out1, w + m, n1 * 8)))) return rc;
    if (out2 && ((rc = hist_launch(A, w, nbins, edges, npairs, pairs, w + m, 0)) || (rc = D.fetch(out2, w + m, n2 * 8)))) return rc;
    return 0;
}

// The three statements of the pinned SVD (oracle/mcx_svd.h) on a caller's matrices: form 0 host_symsvd (no device), form 1 symsvd_dev one
// lane per matrix on tiles of 64, form 2 the blocked kernels through plan_svd and launch_svd -- what launch_adapt runs, nothing restated.
int mcmcx_debug_symsvd(int32_t device, int32_t form, int32_t d, int32_t nmat, const double *A, const uint8_t *need, double *V_out,
                       double *s_out, int32_t *sweeps_out, char *forms, int32_t len)
{
    const char *who = "mcmcx_debug_symsvd";
    if (!A || !V_out || !s_out) return fail(-1, std::string(who) + ": null argument");
    if (d < 1 || d > 4096) return fail(-1, std::string(who) + ": d outside 1 .. 4096");
    if (nmat < 1) return fail(-1, std::string(who) + ": nmat < 1");
    if (form < 0 || form > 2) return fail(-1, std::string(who) + ": form " + std::to_string(form) + " outside 0 .. 2");
    if (form == 2 && (d < SVD_BLOCKED_MIN || d > SVD_BLOCKED_MAX)) return fail(-1, std::string(who) + ": the blocked form covers npar " +
        std::to_string(SVD_BLOCKED_MIN) + " .. " + std::to_string(SVD_BLOCKED_MAX));
    const SvdPlan sp = form == 2 ? plan_svd(d, nmat) : SvdPlan();
    const std::string names = form == 0 ? "host_symsvd" : form == 1 ? "symsvd_dev" : std::string(sp.sweep_name) + "+" + sp.applyv_name;
    if (forms && (len < 1 || (size_t)len <= names.size())) return fail(-1, std::string(who) + ": len too small for \"" + names + "\"");
    const size_t DD = (size_t)d * d;
    std::vector<uint8_t> nd(nmat, 1);
    if (need) for (int m = 0; m < nmat; ++m) nd[m] = need[m] ? 1 : 0;
    if (form == 0) {
        std::vector<double> G, V, sv;
        for (int m = 0; m < nmat; ++m) {
            if (!nd[m]) continue;
            G.assign(A + (size_t)m * DD, A + (size_t)(m + 1) * DD);
            const int sw = host_symsvd(d, G, V, sv);
            std::copy(V.begin(), V.end(), V_out + (size_t)m * DD); std::copy(sv.begin(), sv.end(), s_out + (size_t)m * d);
            if (sweeps_out) sweeps_out[m] = sw;
        }
        if (forms) snprintf(forms, (size_t)len, "%s", names.c_str());
        return 0;
    }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) return fail(-10, "no HIP device: the mcmcx engine has no CPU fallback");
    HIPCHK(hipSetDevice(device));
    DevBufs g;
    uint8_t *dneed = nullptr;
    std::vector<int32_t> sw(nmat, 0);
    if (form == 1) {
        const int T = (nmat + 63) / 64;
        std::vector<double> Gt((size_t)T * DD * 64, 0.0), st((size_t)T * d * 64);
        for (int m = 0; m < nmat; ++m)
            for (size_t e = 0; e < DD; ++e) Gt[((size_t)(m / 64) * DD + e) * 64 + m % 64] = A[(size_t)m * DD + e];
        double *dG = nullptr, *dV = nullptr, *ds = nullptr; int *dsw = nullptr;
        HIPCHK(g.alloc(&dG, Gt.size() * 8)); HIPCHK(g.alloc(&dV, Gt.size() * 8)); HIPCHK(g.alloc(&ds, st.size() * 8));
        HIPCHK(g.alloc(&dsw, (size_t)nmat * sizeof(int))); HIPCHK(g.alloc(&dneed, (size_t)nmat));
        HIPCHK(hipMemcpy(dG, Gt.data(), Gt.size() * 8, hipMemcpyHostToDevice));
        HIPCHK(hipMemset(dV, 0, Gt.size() * 8)); HIPCHK(hipMemset(ds, 0, st.size() * 8));
        HIPCHK(hipMemset(dsw, 0, (size_t)nmat * sizeof(int)));
        HIPCHK(hipMemcpy(dneed, nd.data(), (size_t)nmat, hipMemcpyHostToDevice));
        hipLaunchKernelGGL(debug_symsvd_kernel, dim3(T), dim3(64), 0, 0, dG, dV, ds, dsw, (const uint8_t *)dneed, nmat, d);
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpy(Gt.data(), dV, Gt.size() * 8, hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(st.data(), ds, st.size() * 8, hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(sw.data(), dsw, (size_t)nmat * sizeof(int), hipMemcpyDeviceToHost));
        for (int m = 0; m < nmat; ++m) {
            if (!nd[m]) continue;
            for (size_t e = 0; e < DD; ++e) V_out[(size_t)m * DD + e] = Gt[((size_t)(m / 64) * DD + e) * 64 + m % 64];
            for (int j = 0; j < d; ++j) s_out[(size_t)m * d + j] = st[((size_t)(m / 64) * d + j) * 64 + m % 64];
        }
    } else {
        double *dG = nullptr, *dV = nullptr, *ds = nullptr; mcx_d2 *rot = nullptr; uint8_t *state = nullptr; int *anyrot = nullptr;
        const size_t npairs = std::max<size_t>((size_t)d * (d - 1) / 2, 1);
        HIPCHK(g.alloc(&dG, (size_t)nmat * DD * 8)); HIPCHK(g.alloc(&dV, (size_t)nmat * DD * 8));
        HIPCHK(g.alloc(&ds, (size_t)nmat * d * 8));
        HIPCHK(g.alloc(&rot, (size_t)nmat * npairs * sizeof(mcx_d2))); HIPCHK(g.alloc(&state, (size_t)nmat));
        HIPCHK(g.alloc(&dneed, (size_t)nmat)); HIPCHK(g.alloc(&anyrot, sizeof(int)));
        HIPCHK(hipMemcpy(dG, A, (size_t)nmat * DD * 8, hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(dneed, nd.data(), (size_t)nmat, hipMemcpyHostToDevice));
        HIPCHK(hipMemset(state, 0, (size_t)nmat)); HIPCHK(hipMemset(ds, 0, (size_t)nmat * d * 8));
        launch_svd(sp, 0, dG, dV, ds, rot, state, dneed, anyrot, nmat, d, sw.data());
        HIPCHK(hipGetLastError());
        HIPCHK(hipDeviceSynchronize());
        std::vector<double> Vh((size_t)nmat * DD), sh((size_t)nmat * d);
        HIPCHK(hipMemcpy(Vh.data(), dG, Vh.size() * 8, hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(sh.data(), ds, sh.size() * 8, hipMemcpyDeviceToHost));
        for (int m = 0; m < nmat; ++m) {
            if (!nd[m]) continue;
            std::copy(Vh.begin() + (size_t)m * DD, Vh.begin() + (size_t)(m + 1) * DD, V_out + (size_t)m * DD);
            std::copy(sh.begin() + (size_t)m * d, sh.begin() + (size_t)(m + 1) * d, s_out + (size_t)m * d);
        }
    }
    if (sweeps_out) for (int m = 0; m < nmat; ++m) if (nd[m]) sweeps_out[m] = sw[m];
    if (forms) snprintf(forms, (size_t)len, "%s", names.c_str());
    return 0;
}

// The tick's factorisation on a caller's covariances: launch_factor, the function launch_adapt ends in, with mode 0 -- nothing about the
// instances, grids or LDS sizes is restated here.  Everything is decided before the first write.
int mcmcx_debug_calculate_R(mcmcx_handle h, const double *cmat, const uint8_t *need, int32_t *info_out, char *forms, int32_t len)
{
    const char *who = "mcmcx_debug_calculate_R";
    if (!h || !cmat || !info_out) return fail(-57, std::string(who) + ": null argument");
    if (!h->inited) return fail(-57, std::string(who) + ": the engine is not initialised");
    if (h->pooled) return fail(-57, std::string(who) + ": not in pooled mode (the host factors the shared covariance)");
    if (h->cfg.method == MCMCX_METHOD_RAM) return fail(-57, std::string(who) + ": not with method = 'ram' (no adaptation tick)");
    if (!h->plan.am || !h->E.cmat) return fail(-57, std::string(who) + ": the engine has no adaptation state (doadapt = doburnin = 0)");
    const AdaptPlan &a = h->plan.adapt;
    const std::string post = a.post_name;
    const std::string names = h->plan.svd_blocked ? post + ":1+" + a.svd.sweep_name + "+" + a.svd.applyv_name + "+" + post + ":2"
        : a.factor ? post + ":3+" + a.factor_name : post;
    if (forms && (len < 1 || (size_t)len <= names.size())) return fail(-57, std::string(who) + ": len too small for \"" + names + "\"");
    const int d = h->d, P = h->P, n = h->cfg.nchains;
    const size_t DD = (size_t)d * d;
    std::vector<uint32_t> ic, flags0((size_t)h->nlanes);
    std::vector<double> cm;
    int rc;
    if ((rc = fetch(h, h->E.ictr, (size_t)h->nlanes * NICTR, ic)) || (rc = fetch(h, h->E.cmat, (size_t)h->nlanes * P, cm))) return rc;
    auto at = [&](int c, int k) -> uint32_t & { return ic[((size_t)(c / 64) * NICTR + k) * 64 + c % 64]; };
    for (int c = 0; c < h->nlanes; ++c) {
        const bool on = c < n && (!need || need[c]);
        flags0[c] = at(c, I_ADFLAGS);
        at(c, I_ADFLAGS) = on ? (uint32_t)ADF_DOCALC : 0u;
        at(c, I_INFO) = (uint32_t)MCMCX_DEBUG_INFO_SENTINEL;
        if (!on) continue;
        const double *A = cmat + (size_t)c * DD;
        for (int j = 0; j < d; ++j)
            for (int i = 0; i <= j; ++i) cm[((size_t)(c / 64) * P + h_pidx(i, j, d)) * 64 + c % 64] = A[(size_t)i + (size_t)j * d];
    }
    HIPCHK(hipMemcpyAsync(h->E.cmat, cm.data(), cm.size() * 8, hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipMemcpyAsync(h->E.ictr, ic.data(), ic.size() * 4, hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    launch_factor(h, 0, 0, 0);
    HIPCHK(hipGetLastError());
    if ((rc = fetch(h, h->E.ictr, (size_t)h->nlanes * NICTR, ic))) return rc;
    for (int c = 0; c < n; ++c) info_out[c] = (int32_t)at(c, I_INFO);
    for (int c = 0; c < h->nlanes; ++c) at(c, I_ADFLAGS) = flags0[c];
    HIPCHK(hipMemcpyAsync(h->E.ictr, ic.data(), ic.size() * 4, hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    if (forms) snprintf(forms, (size_t)len, "%s", names.c_str());
    return 0;
}

// ... and the host's statement of it: host_initial_R, then host_potri on the scaled factor (initial_factor's sequence).  No device.
int mcmcx_debug_host_calculate_R(int32_t d, const double *A, double *R_out, double *iC_out, int32_t *info_out)
{
    if (!A || !R_out || !info_out) return fail(-57, "mcmcx_debug_host_calculate_R: null argument");
    if (d < 1 || d > 4096) return fail(-57, "mcmcx_debug_host_calculate_R: d outside 1 .. 4096");
    const std::vector<double> cm(A, A + (size_t)d * d);
    std::vector<double> Rp, Cp;
    info_out[0] = host_initial_R(d, cm, Rp, Cp); info_out[1] = 0;
    if (info_out[0] != 0) return 0;
    std::vector<double> p = Rp;
    unpack_upper(d, Rp, R_out, false);
    if (!iC_out) return 0;
    info_out[1] = host_potri(d, p);
    if (info_out[1] == 0) unpack_upper(d, p, iC_out, false);
    return 0;
}

int mcmcx_debug_math(int32_t op, int32_t n, const double *a, const double *b, double *out)
{
    if (n < 1 || !a || !out) return fail(-1, "bad argument");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) return fail(-10, "no HIP device: the mcmcx engine has no CPU fallback");
    DevBufs g;
    double *da = nullptr, *db = nullptr, *dout = nullptr;
    HIPCHK(g.alloc(&da, (size_t)n * 8)); HIPCHK(g.alloc(&dout, (size_t)n * 8));
    HIPCHK(hipMemcpy(da, a, (size_t)n * 8, hipMemcpyHostToDevice));
    if (b) { HIPCHK(g.alloc(&db, (size_t)n * 8)); HIPCHK(hipMemcpy(db, b, (size_t)n * 8, hipMemcpyHostToDevice)); }
    hipLaunchKernelGGL(debug_math_kernel, dim3((n + 255) / 256), dim3(256), 0, 0, op, n, da, db, dout);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpy(out, dout, (size_t)n * 8, hipMemcpyDeviceToHost));
    return 0;
}

// Replace the SVD proposal factor of EVERY chain (per-chain mode, condmax > 0): R column-major d x d (scam: the rotation U),
// qcovstd (scam; may be NULL).  Lets a test feed the factors an external LAPACK returned at an adaptation
// (tests/test_gpu_parity.py: the MKL-linked reference's logged dgesvd results at d = 200).
int mcmcx_debug_set_factor(mcmcx_handle h, const double *R_colmajor, const double *qcovstd)
{
    if (!h || !h->inited || !R_colmajor) return fail(-1, "mcmcx_debug_set_factor: bad argument");
    if (!h->usesvd || h->pooled
        || !h->E.Rf) return fail(-45, "mcmcx_debug_set_factor: per-chain SVD factor only (condmax > 0, not pooled)");
    HIPCHK(hipSetDevice(h->cfg.device));
    HIPCHK(hipStreamSynchronize(h->stream));
    std::vector<double> r(R_colmajor, R_colmajor + (size_t)h->d * h->d);
    int rc = dev_bcast(h, h->E.Rf, r); if (rc) return rc;
    if (qcovstd && h->E.qstd) { std::vector<double> q(qcovstd, qcovstd + h->d); if ((rc = dev_bcast(h, h->E.qstd, q))) return rc; }
    return 0;
}

int mcmcx_debug_rng(uint32_t seed, uint32_t chain_id, int32_t kind, int32_t n, double a, double b, double *out, uint64_t *nused)
{
    if (n < 1 || !out) return fail(-1, "bad argument");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) return fail(-10, "no HIP device: the mcmcx engine has no CPU fallback");
    DevBufs g;
    double *dout = nullptr; uint64_t *dn = nullptr;
    HIPCHK(g.alloc(&dout, (size_t)n * 8)); HIPCHK(g.alloc(&dn, 8));
    hipLaunchKernelGGL(debug_rng_kernel, dim3(1), dim3(64), 0, 0, seed, chain_id, kind, n, a, b, dout, dn);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpy(out, dout, (size_t)n * 8, hipMemcpyDeviceToHost));
    if (nused) HIPCHK(hipMemcpy(nused, dn, 8, hipMemcpyDeviceToHost));
    return 0;
}

} // extern "C"
