/*
 * include/mcmcx.h -- C ABI of the MI355X-native adaptive-Metropolis engine (libmcmcx.so).
 *
 * This is the drop-in boundary for mcmcf90's sampling hot path.  A Fortran host
 * (mcmcf90_amd/fortran/mcmcx_mod.F90: module mcmcmod + subroutine mcmc_main, same
 * names as mcmc.F90:12 / mcmc_main.F90:12) binds these entry points through
 * ISO_C_BINDING; tests and bench.py bind them through ctypes.  Plain pointers and
 * sizes only, all host memory unless a name says "dev".  Every function returns
 * 0 on success, <0 on a fatal error (the reference would `stop`: doerror,
 * matutils.F90:764-789), >0 for a warning; mcmcx_last_error() returns the text.
 *
 * What each entry point replaces in the reference:
 *
 *   mcmcx_create            MCMC_init_namelist + check_mcmcinit_parameters   mcmcinit.F90:184-230, 235-368
 *   mcmcx_set_par0          MCMC_setpar0_vec                                 MCMC_init.F90:168-183
 *   mcmcx_set_cmat0         MCMC_setcmat0_mat                                MCMC_init.F90:201-218
 *   mcmcx_set_sigma2nobs    MCMC_setsigma2nobs_vec                           MCMC_init.F90:295-323
 *   mcmcx_set_target_*      the user's ssfunction (device-resident form)     external_inc.h:12-19
 *   mcmcx_set_bounds        the user's checkbounds (box form)                external_inc.h:29-32
 *   mcmcx_set_priors        default priorfun + priorsfile                    priorfun.f90:31-103
 *   mcmcx_init              MCMC_init tail: first MCMC_calculate_R, counters MCMC_init.F90:81-160
 *   mcmcx_run               MCMC_run / MCMC_run_ram loop, MCMC_adapt,        MCMC_run.F90:41-107,
 *                           MCMC_adapt_ram, MCMC_savechain                   MCMC_run_ram.F90:45-81, MCMC_adapt.F90:12-174
 *   mcmcx_get_chain         chain / sschain / s2chain module arrays          mcmc.F90:31-33, MCMC_aux.F90:167-185
 *   mcmcx_get_chaincov      chaincmat / chainmean / chainwsum                mcmc.F90:38-40
 *   mcmcx_get_counters      stayed, bndstayed, draccepted, drtries           mcmc.F90:46-55
 *   mcmcx_run1_*            the arithmetic of one MCMC_run1 / MCMC_run1_er call  MCMC_run1.F90:131-199, MCMC_run1_er.F90:122-182
 *
 * N independent chains run at once; chain c draws from the Philox4x32-10 stream
 * keyed (seed, chain_id0 + c) and, in the default "replicas" mode, is the
 * reference's single chain to the last bit of its accept/reject sequence.
 */
#ifndef MCMCX_H
#define MCMCX_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MCMCX_METHOD_DRAM 0   /* method = 'dram' (AM / DRAM), mcmc_main.F90:35-36 */
#define MCMCX_METHOD_RAM  1   /* method = 'ram',              mcmc_main.F90:33-34 */
#define MCMCX_METHOD_SCAM 2   /* method = 'scam',             mcmc_main.F90:29-30 */
#define MCMCX_METHOD_ER   3   /* method = 'er',               mcmc_main.F90:31-32 */

#define MCMCX_DEFAULT_SEED 0x6D636D63u

/* Numeric members of namelist /mcmc/ (mcmcinit.F90:74-82) plus the multi-chain extensions. */
typedef struct mcmcx_config {
    int32_t npar;          /* d */
    int32_t nchains;       /* N independent chains on this device */
    int32_t method;
    int32_t nsimu;
    int32_t doadapt, doburnin, adaptint, adapthist, badaptint, adaptend, initcmatn;
    int32_t burnintime, greedy, updatesigma;
    double  scalelimit, scalefactor, drscale, N0, S02, condmax, alphatarget, nuparam;
    uint32_t seed;         /* Philox key word 0 */
    uint32_t chain_id0;    /* Philox key word 1 of chain 0 (rank offset when sharded) */
    int32_t record_accept; /* keep the wavefront accept ballots of every iteration */
    int32_t record_chain;  /* keep every accepted row (the reference's chain/sschain/s2chain) */
    int32_t device;        /* HIP device ordinal */
    int32_t pooled;        /* 1: one proposal factor shared by all chains, adapted from the pooled empirical
                            * covariance of the current states (multi-chain extension; 0 = the reference's per-chain AM).
                            * Every target takes it -- the built-in ones, a target module (mcmcx_set_target_module) and host
                            * callbacks (mcmcx_set_target_host / _host_batch / _host_er), nycol > 1 included -- except
                            * mcmcx_set_target_external (-8) and method = 'scam' on the response-column target (-8 / -36);
                            * no chain holds a factor of its own then */
    int32_t scam_fast;     /* method = 'scam' only, opt-in (default 0 = the reference's operations): the componentwise proposal
                            * newpar = U (U'oldpar + delta e_j) (MCMC_run_scam.F90:106-115: two dgemv) is formed as
                            * newpar = oldpar + delta U(:,j) -- the same point up to the rounding of U U' = I, one column
                            * of the rotation instead of two passes over it.  Every kernel form computes
                            * newpar_k = fma(delta, U(k,j), oldpar_k) with delta the sub-step's first draw, which the test oracle
                            * restates (oracle/mcx_oracle.h, scam_fast): the engine is pinned to that restatement bit for bit on every
                            * chain (tests/test_gpu_every_chain.py, test_gpu_pooled.py, test_gpu_scam_fast.py), and to the
                            * reference and its reference-order form only to rounding level (same accept sequences on the
                            * reference's fixtures, states within 1e-6; tests/test_oracle_scam_fast.py). */
} mcmcx_config;

typedef struct mcmcx_engine *mcmcx_handle;

void mcmcx_config_defaults(mcmcx_config *cfg);                 /* mcmcinit.F90:184-230 */
int  mcmcx_create(const mcmcx_config *cfg, mcmcx_handle *out);
int  mcmcx_destroy(mcmcx_handle h);
const char *mcmcx_last_error(void);
const char *mcmcx_version(void);
int32_t mcmcx_device_count(void);                              /* HIP devices visible to this process (0: none -- nothing will run) */
int mcmcx_device_info(int32_t device, char *buf, int32_t len); /* "name arch, pci bus id, CUs, memory" of one of them (diagnostics) */
/* the device's UUID as 32 hex digits (len >= 33) and out5 = {engine clock limit kHz, memory clock limit kHz, memory bus width
 * in bits, compute units, L2 bytes}: what tells two boxes of a pool apart in a benchmark line (diagnostics) */
int mcmcx_device_ident(int32_t device, char *uuid_hex, int32_t len, int32_t *out5);
const char *mcmcx_last_kernel(mcmcx_handle h);                /* the sampling kernel the last mcmcx_run launched, as spelled in the
                                                                  source ("step_kernel<true, false, false>", "scam_pooled_kernel", ...);
                                                                  "" before the first run or with per-chain factors and the
                                                                  iteration cut at a user module's / host callbacks' evaluations;
                                                                  pooled mode names its phase form there ("pooled_phase_kernel",
                                                                  "pooled_phase_mfma_kernel", "host_phase_kernel<pooled scam>")
                                                                  (diagnostics) */

int mcmcx_set_par0(mcmcx_handle h, const double *par0, int32_t npar);
/* ---- Per-chain start points (no counterpart in the single-chain reference, which starts its one chain at par0).  By default every
 * chain starts at par0; two calls, both before mcmcx_init and both off by default, give every chain a start of its own.  A run that uses
 * neither is bit for bit the run without them.  Chain c is then the reference's single chain started at its start point: oldpar is the
 * start, the first ss / sspri is evaluated there, chain row 1 is the start, chainmean is the start at init and at both restarts of the
 * adaptation (the greedy restart of the burn-in, MCMC_adapt.F90:83-101, and the first AM tick); everything else is unchanged, the chain's
 * stream (seed, chain_id0 + c) included.  mcmcx_set_par0 is still required: par0 stays the shift of the pooled moments and the pooled
 * state's initial mean, and in pooled mode nothing but theta changes.  mcmcx_get_theta right after init returns the starts;
 * mcmcx_set_samples with first = 1 keeps them as sample 0.  The later of the two calls wins.
 *
 * mcmcx_set_par0_all: par0_all is host memory, [nchains][npar] row-major like mcmcx_get_theta's rows, copied at the call.  A start
 * outside the box of mcmcx_set_bounds is taken as it is, as par0 is.
 *
 * mcmcx_set_par0_spread: the starts are drawn on the device at mcmcx_init (start_spread_kernel).  The definition is the contract
 * (tests/start_ref.py restates it with the oracle's generator):
 *   Stream: chain c draws from its own Philox stream, key (seed, chain_id0 + c), starting at uniform number 2**63 with an empty polar
 *     cache -- no run reaches that number, there is no new key and no new generator, the chain's sampling stream is not advanced, and the
 *     starts do not depend on how the chains are sharded over engines.
 *   Factor: U0 = dpotf2('U', cmat0) * 2.4 / sqrt(npar), the initial Cholesky proposal factor (what mcmcx_get_R shows after init on the
 *     Cholesky path) -- with condmax > 0 and method = 'scam' too.  If that factorisation fails, mcmcx_init refuses.
 *   One attempt: z_k = normal_bm(), k = 0 .. npar-1 in that order; x_j = the fma chain t = fma(U0(i,j), z_i, t) from +0.0, i ascending to j;
 *     theta_k = par0_k + (scale * x_k): one multiplication, then one addition, no contraction.
 *   Bounds: with mcmcx_set_bounds, an attempt the proposals' box test rejects is followed by another one from the next normals of the same
 *     stream (the polar cache carries over), MCMCX_START_TRIES attempts at the most; after that the chain starts at par0, bit for bit.  A
 *     user's checkbounds callback or module function is not consulted.
 *   scale = 1 is one draw of the initial proposal distribution around par0; scale = sqrt(npar) / 2.4 is N(par0, cmat0).
 *
 * Cost: a device table of the starts, ceil(nchains / 64) x npar x 64 doubles, allocated only when one of the two calls was made (400 MB
 * at 1 048 576 chains x npar 50).  mcmcx_set_par0_all also holds its copy of par0_all in host memory from the call until mcmcx_init has
 * filled the device table (init stages a second, tile-interleaved host vector of that size for the upload); both are released there.
 *
 * mcmcx_start_info, after init: out3 = {mode: 0 shared par0, 1 given, 2 spread; chains that made more than one attempt; chains that fell
 * back to par0}.  It is a getter and answers like the other getters, not with -56: -40 for a null handle or one that is not inited, -1
 * for a null out3.
 *
 * The two setters refuse with -56 (the reason in mcmcx_last_error), nothing allocated or launched: a null handle or array; nchains or npar that differ
 * from the handle's; a value of par0_all that is not finite; a scale that is not finite or not > 0 (0 is refused, not "off"); either call
 * after mcmcx_init; mcmcx_set_target_external (mcmcx_init returns the -56 when the external target was chosen after the call); and at
 * mcmcx_init, for spread, a cmat0 whose Cholesky factorisation failed. */
#define MCMCX_START_TRIES 64
int mcmcx_set_par0_all(mcmcx_handle h, const double *par0_all /* [nchains][npar] */, int32_t nchains, int32_t npar);
int mcmcx_set_par0_spread(mcmcx_handle h, double scale);
int mcmcx_start_info(mcmcx_handle h, int64_t *out3);
int mcmcx_set_cmat0(mcmcx_handle h, const double *cmat0_colmajor, int32_t npar);
int mcmcx_set_sigma2nobs(mcmcx_handle h, const double *sigma2, const int32_t *nobs, int32_t nycol);
int mcmcx_set_target_gauss(mcmcx_handle h, const double *mu, const double *lam_rowmajor);
int mcmcx_set_target_banana(mcmcx_handle h, double b);
int mcmcx_set_target_expdata(mcmcx_handle h, int32_t ndata, const double *x, const double *y);
/* The same model with nycol response columns (a vector-valued ssfunction, external_inc.h:4-9; one sigma2 per column,
 * MCMC_DRAM.F90:100-118, 192-206): ss_j = sum_i (y_j(i) - theta_1 exp(-theta_{1+j} x_i))**2, npar = 1 + nycol,
 * y = [nycol][ndata].  Device-resident; the iteration is cut at the evaluations like the host-callback path (several
 * short launches per iteration, no host round trip).  Give the nycol sigma2 / nobs with mcmcx_set_sigma2nobs. */
int mcmcx_set_target_expdata_cols(mcmcx_handle h, int32_t ndata, int32_t nycol, const double *x, const double *y);
/* ---- Many fits in one run: a data set per chain for the response-column target (no counterpart in the reference, whose one chain
 * has one data set).  mcmcx_set_target_expdata_all is mcmcx_set_target_expdata_cols with every chain's own observations: the model is
 * that call's, operation for operation -- ss_j = the fma chain from +0.0 over i ascending of r * r, r = y_j(i) - theta_1 exp(-(theta_{1+j}
 * x_i)), npar = 1 + nycol -- and chain c is the reference's single chain on chain c's data: its stream (seed, chain_id0 + c), its
 * factor and its counters are what the same chain has in a run with that one data set.  A run that does not make the call is bit for
 * bit the run without it; every chain given the same data is the mcmcx_set_target_expdata_cols run.
 *
 * y_all is host memory, [nchains][nycol][ndata]; x is [ndata], shared by all chains, when x_per_chain = 0 and [nchains][ndata] when it
 * is 1.  Both are copied at the call and not inspected: NaN and inf propagate as the arithmetic says.  The call composes with
 * mcmcx_set_par0_all / _spread, mcmcx_set_bounds, mcmcx_set_priors, mcmcx_set_sigma2nobs (one sigma2 / nobs per column, shared by the
 * chains) and mcmcx_set_samples, whose ss and sigma2 fields are then per fit; every method runs (dram with and without delayed
 * rejection, ram, er, scam).  The last target setter called wins.
 *
 * Cost: device tables, tile-interleaved like every per-chain array and allocated only when the call was made,
 *   y: ceil(nchains / 64) x nycol x ndata x 64 doubles, row j * ndata + i of a tile;
 *   x: ceil(nchains / 64) x ndata x 64 doubles when x_per_chain = 1 (otherwise the shared x[ndata]);
 * lanes of the last tile without a chain hold +0.0 (46 MB and 23 MB at 262 144 chains, nycol 2, ndata 11).  A wave's load of one
 * element is one contiguous 512-byte segment.  The call's host copies live until mcmcx_init has filled the tables (init stages a
 * tile-interleaved host vector of the same size for the upload); both are released there.
 *
 * mcmcx_chain_data_info, after init: out4 = {mode: 0 one data set for all chains, 1 y per chain, 2 x and y per chain; ndata; nycol;
 * bytes of the per-chain device tables} (ndata and nycol: 0 for a target without data).  It is a getter and answers like the other
 * getters: -40 for a null handle or one that is not inited, -1 for a null out4.
 *
 * mcmcx_set_target_expdata_all refuses with -58 (the reason in mcmcx_last_error), nothing allocated or launched and the handle's target
 * unchanged: a null handle, x or y_all; nchains that differs from the handle's; ndata < 1; x_per_chain outside 0 .. 1; a call after
 * mcmcx_init; pooled mode (one proposal factor pooled over different posteriors is not a method).  As in mcmcx_set_target_expdata_cols,
 * nycol out of range is -21 and npar != 1 + nycol is -22. */
int mcmcx_set_target_expdata_all(mcmcx_handle h, int32_t nchains, int32_t ndata, int32_t nycol, const double *x, int32_t x_per_chain,
                                 const double *y_all /* [nchains][nycol][ndata] */);
int mcmcx_chain_data_info(mcmcx_handle h, int64_t *out4);
/* Host-callback target: the user's own ssfunction / priorfun / checkbounds (external_inc.h:4-33) behind plain C
 * signatures (the Fortran shim adapts the array-result / assumed-shape ABIs).  The engine calls them from the
 * thread that calls mcmcx_run, one chain after the other, at the points the reference does (MCMC_run.F90:47,55-56,
 * 69,74-75); the candidates make a D2H/H2D round trip per stage, so this is the plumbing path, not the fast one.
 * priorfun / checkbounds may be NULL (flat prior, no bounds = the library defaults).  With cfg.pooled = 1 the proposals
 * come from the one shared factor; the callbacks are called exactly as without it. */
typedef void    (*mcmcx_ssfun_t)(const double *theta, int32_t npar, int32_t ny, double *ss_out, void *user);
typedef double  (*mcmcx_priorfun_t)(const double *theta, int32_t npar, void *user);
typedef int32_t (*mcmcx_checkbounds_t)(const double *theta, int32_t npar, void *user);
int mcmcx_set_target_host(mcmcx_handle h, mcmcx_ssfun_t ss, mcmcx_priorfun_t pri, mcmcx_checkbounds_t cb, void *user);
/* Batched form of the same (opt-in; external_inc.h:12-19 has no counterpart): ss_batch evaluates n candidates in one
 * call -- theta[n][npar] row-major (= Fortran theta(npar,n)), ss[n][ny] -- and, with nthreads > 1, is called from that
 * many threads at once on disjoint slices, so it must be re-entrant (the very first evaluation, at mcmcx_init, is made
 * from the calling thread alone, so load-on-first-call code is safe).  Bounds and prior stay per chain on the calling
 * thread, before the batch.  (method = 'er' with mcmcx_set_target_host_er keeps the per-chain path.)  cfg.pooled = 1: as
 * for mcmcx_set_target_host. */
typedef void (*mcmcx_ssfun_batch_t)(const double *theta, int32_t npar, int32_t n, int32_t ny, double *ss_out, void *user);
int mcmcx_set_target_host_batch(mcmcx_handle h, mcmcx_ssfun_batch_t ss_batch, mcmcx_priorfun_t pri, mcmcx_checkbounds_t cb,
                                void *user, int32_t nthreads);
/* The user's ssfunction / priorfun / checkbounds as DEVICE code: a code object (hipcc --genco) whose kernel
 * `kernel_name` was defined with MCMCX_DEFINE_TARGET (include/mcmcx_target.h).  The engine launches it where the
 * reference calls the functions; candidates and results never leave HBM.  userdata (nbytes, may be NULL) is copied
 * to the device and handed to the functions.  With cfg.pooled = 1 the engine's share of an iteration reads the one
 * shared factor (npar <= 64: the proposal's product on the matrix cores where that is the faster form) and no chain
 * holds a factor of its own; several GPUs: mcmcx_set_comm + mcmcx_run_all, or the mcmcx_set_exchange hook. */
int mcmcx_set_target_module(mcmcx_handle h, const char *code_object_path, const char *kernel_name, const void *userdata, int64_t nbytes);
/* method='er' with host callbacks: the user's ssfunction_er(theta,npar,ny,sscrit) (external_inc.h:16-20), which may
 * stop summing once it passes sscrit; NULL (default) = ssfunction, like ssfunction_er0.f90.  Same `user` pointer. */
typedef void (*mcmcx_ssfun_er_t)(const double *theta, int32_t npar, int32_t ny, double sscrit, double *ss_out, void *user);
int mcmcx_set_target_host_er(mcmcx_handle h, mcmcx_ssfun_er_t ss_er);
int mcmcx_set_bounds(mcmcx_handle h, const double *lo, const double *hi);       /* NULL = unbounded side */
int mcmcx_set_priors(mcmcx_handle h, const double *mu, const double *sig);      /* sig <= 0: flat */
int mcmcx_set_stream(mcmcx_handle h, void *hip_stream);

int mcmcx_init(mcmcx_handle h);
/* iterations simuind+1 .. upto.  Returns MCMCX_INTERRUPTED (> 0) when a signal caught by
 * mcmcx_install_signal_handlers arrived: the run stopped at a launch boundary, mcmcx_simuind() says where, and
 * every getter is valid for the iterations done (the reference saves the chain "upto simuind" and stops,
 * MCMC_signal_handler.F90:95-107).  In pooled mode with a communicator of several ranks the run is left only at an
 * adaptation tick, by agreement of all ranks (every rank's stop flag travels with the pooled vector), so that no rank
 * is left waiting in a collective: that tick's adaptation IS applied before the ranks return, so mcmcx_clear_interrupt +
 * mcmcx_run resumes into the trajectory of an uninterrupted run.  Where no tick lies ahead of the call's `upto`
 * (doadapt = 0, past adaptend, the tail of a run) nothing collective remains and the rank that caught the signal returns
 * at its next launch boundary by itself.  A rank that fails marks the communicator and its peers' waits give up (< 0).
 * A run that failed inside a host-callback iteration (a HIP error around the user's ssfunction / priorfun / checkbounds) leaves
 * the handle unusable: with the phases fused, the next iteration's proposal -- its random draws included -- has already run, and a
 * second mcmcx_run would draw it again and leave the reference's stream order.  Later calls return -42; destroy the handle.
 * (mcmcx_create refuses npar > 4096 with -5: the packed triangle's int-typed indices, 64 npar (npar + 1) / 2 < 2**31.) */
int mcmcx_run(mcmcx_handle h, int32_t upto);
int mcmcx_sync(mcmcx_handle h);

/* ---- MCMC_run1 / MCMC_run1_er (mcmc_main_one, mcmc_main.F90:49-70): one evaluation of ssfunction per program
 * invocation, the chain's state carried in files between invocations (MCMC_run1.F90:14-29).  The file protocol is the
 * host's (the Fortran shim's mcmc_main_one); what is arithmetic in one invocation runs here, on the factors of
 * mcmcx_init (R, R2 = R/drscale, iC) and the chain's stream.  mcmcx_set_target_external declares that EVERY
 * evaluation of ssfunction / priorfun / checkbounds is the caller's -- mcmcx_init evaluates nothing, mcmcx_run refuses.
 * All chains at once; vectors are row-major per chain ([nchains][npar], [nchains][nycol], [nchains]).
 *   mcmcx_run1_decide   alpha = MCMC_alpha(oldpar1 -> newpar) in stage 1 (MCMC_run1.F90:141), or
 *                       MCMC_DR_alpha13(oldpar2, oldpar1, newpar) in stage 2 with drscale > 0 (:137-139; oldpar2 =
 *                       the current point, oldpar1 = the rejected first try); then reject = MCMC_reject(alpha) (:143).
 *                       The stage-2 arguments may be NULL in stage 1.
 *   mcmcx_run1_propose  newpar = MCMC_propose(from, R) (stage 1) or (from, R2) (stage 2 with drscale > 0) (:185-189)
 *   mcmcx_run1_sscrit   sscrit = MCMC_sscrit(ssprev1, sspri1) = -2 log u + sum(ss/sigma2) + pri  (MCMC_run1_er.F90:168) */
int mcmcx_set_target_external(mcmcx_handle h);
int mcmcx_run1_decide(mcmcx_handle h, int32_t drstage, const double *oldpar2, const double *ssprev2, const double *sspri2,
                      const double *oldpar1, const double *ssprev1, const double *sspri1, const double *alpha12,
                      const double *newpar, const double *ss, const double *sspri, double *alpha_out, int32_t *reject_out);
int mcmcx_run1_propose(mcmcx_handle h, int32_t stage, const double *from, double *newpar_out);
int mcmcx_run1_sscrit(mcmcx_handle h, const double *ssprev1, const double *sspri1, double *sscrit_out);
#define MCMCX_INTERRUPTED 2
/* SIGHUP, SIGINT, SIGTERM, SIGTSTP, SIGUSR1, SIGUSR2 (the set of signalqq.c:57-62) raise a flag that mcmcx_run
 * polls between kernel launches; mcmcx_interrupted() reads it, mcmcx_clear_interrupt() resets it */
int mcmcx_install_signal_handlers(void);
int mcmcx_interrupted(void);
void mcmcx_clear_interrupt(void);

int32_t mcmcx_simuind(mcmcx_handle h);
/* counters[0..7] = stayed, bndstayed, draccepted, drtries, chainind, status bits, erstayed, run length of the
 * current row, of one chain */
int mcmcx_get_counters(mcmcx_handle h, int32_t chain, int32_t *counters8);
/* over all chains: sums of stayed, bndstayed, draccepted, drtries, proposals (stage 1 + stage 2), RAM iterations that
 * were Cholesky downdates (a < 0, MCMC_run_ram.F90:168-172); [6] = the OR of every chain's status bits
 * (MCMCX_ST_*: where the reference would have stopped -- matutils.F90:719-722, MCMC_adapt.F90:221 -- or kept its old
 * factor, MCMC_adapt.F90:168-171) */
#define MCMCX_ST_RAM_DOWNDATE_FAIL 1
#define MCMCX_ST_CHOL_FAIL 2
#define MCMCX_ST_POTRI_FAIL 4
int mcmcx_get_totals(mcmcx_handle h, int64_t *totals7);      /* writes SEVEN values (five before library version 0.2) */
int mcmcx_get_totals_n(mcmcx_handle h, int64_t *totals, int32_t n);   /* the first n of them: the caller states its buffer */
int mcmcx_get_theta(mcmcx_handle h, double *theta_rowmajor /* [nchains][npar] */);
/* per chain: ss1, sspri1, sigma2, alpha12 */
int mcmcx_get_scalars(mcmcx_handle h, double *out /* [nchains][4] */);
/* per chain: uniforms drawn, polar cache flag, cached deviate */
int mcmcx_get_rng(mcmcx_handle h, int32_t chain, uint64_t *n, int32_t *saved, double *saved_y);
int mcmcx_get_R(mcmcx_handle h, int32_t chain, double *R_colmajor);    /* upper triangular, or the full SVD factor when condmax > 0 */
int mcmcx_get_qcovstd(mcmcx_handle h, int32_t chain, double *std);      /* SCAM: qcovstd (mcmc.F90:37) */
int mcmcx_get_chaincov(mcmcx_handle h, int32_t chain, double *cmat_colmajor, double *mean, double *wsum);
/* delayed-rejection state of one chain: R2 = R/drscale and the upper triangle of iC (mcmc.F90:36) */
int mcmcx_get_dr(mcmcx_handle h, int32_t chain, double *R2_colmajor, double *iC_colmajor);
/* accept flags of iterations 1..simuind for one chain (needs record_accept or record_chain) */
int mcmcx_get_accepted(mcmcx_handle h, int32_t chain, uint8_t *accepted);
/* raw wavefront ballots: masks[(it-1)*ntiles + tile], bit l = chain tile*64+l moved at iteration it */
int mcmcx_get_accept_masks(mcmcx_handle h, uint64_t *masks, int32_t *ntiles);
/* run-length compressed chain of one chain, like chain(1:chainind,:) / sschain / s2chain
 * (needs record_chain).  chain: [nrows][npar+1] row-major; ss: [nrows][nycol+1] (ss per column, repeat count);
 * s2: [simuind][nycol] */
int mcmcx_get_chain(mcmcx_handle h, int32_t chain, double *chain_out, double *ss_out, double *s2_out,
                    int32_t *nrows);
/* pooled moments of the current states of all chains of this device (shifted by par0):
 * out = [count, sum_j (th-par0)_j (npar), sum (th-par0)_j (th-par0)_k j<=k (npar(npar+1)/2)] */
int mcmcx_pooled_moments(mcmcx_handle h, double *out);
int32_t mcmcx_pooled_moments_len(mcmcx_handle h);
/* same, written to a device buffer of the caller (the operand of an RCCL all-reduce); asynchronous on
 * the engine's stream */
int mcmcx_pooled_moments_dev(mcmcx_handle h, void *dev_out);

/* ---- thinned samples of ALL chains, kept on the device (no counterpart in the single-chain reference, whose chain / sschain /
 * s2chain arrays -- record_chain, mcmcx_get_chain -- hold every row of one chain).
 * mcmcx_set_samples, before mcmcx_init: iteration i, 1 <= i <= nsimu, is kept when i >= first and (i - first) % thin == 0, in a ring
 * of `capacity` slots (once it is full the oldest sample is overwritten); thin = 0 switches sampling off again (the default).
 * Iteration 1 is the state mcmcx_init leaves (the reference's chain row 1; mcmcx_simuind is 1 after init), so first = 1 keeps the
 * start point, stored at init.  Refused with -47: first < 1, thin < 0, capacity < 1 with thin > 0, a call after mcmcx_init, and
 * mcmcx_set_target_external (the engine does not run the iterations there; mcmcx_init returns the -47 when the external target was
 * chosen after this call).  The store -- capacity x ceil(nchains / 64) x 64 x nfields doubles -- is allocated by mcmcx_init with
 * the engine's other device state; if that fails, init fails with the size in its message.
 * How: a kept iteration ends the launch of the sampling kernel, like an adaptation tick does, and a copy kernel of its own stores
 * the state the launch wrote back; no sampling kernel knows about the store.  Launch boundaries do not matter to the chains, so a
 * run with sampling on is bit-identical -- states, stream positions, factors, counters -- to the same run without it, and
 * mcmcx_kernel_time / mcmcx_last_kernel keep describing the sampling kernels alone.  The cost is the copy plus one more launch per
 * kept iteration: the lane-group kernels reload their factors into registers at every launch, so a small thin costs them
 * throughput ("Thinned samples", has the measured table). */
int mcmcx_set_samples(mcmcx_handle h, int32_t first, int32_t thin, int32_t capacity);
/* Returns the number of samples retained now (0 before any was kept or with sampling off): retained sample s (0 = oldest) is
 * iteration oldest_iteration + s * thin.  nfields = npar + 2 nycol + 1: the fields of one chain are theta[npar], ss[nycol], sspri,
 * sigma2[nycol].  Valid after a run that returned MCMCX_INTERRUPTED, for the iterations up to mcmcx_simuind.  The out arguments
 * may be NULL.  (No counterpart in the reference.) */
int32_t mcmcx_samples_kept(mcmcx_handle h, int32_t *oldest_iteration, int32_t *thin, int32_t *nfields);
/* Retained samples s0 .. s0 + ns - 1 of chains c0 .. c0 + nc - 1 (no counterpart in the reference).  layout 0: [ns][nc][nfields],
 * one chain's fields contiguous like mcmcx_get_theta's rows; layout 1: [ns][nfields][nc], the chain index running fastest.
 * mcmcx_get_samples copies to host memory and synchronises; mcmcx_get_samples_dev writes into the caller's DEVICE buffer and is
 * asynchronous on the engine's stream like mcmcx_pooled_moments_dev (mcmcx_sync before another stream reads it).  A window outside
 * the retained samples or the chains, ns < 1, nc < 1 or another layout is refused with -48 before anything is launched.
 * mcmcx_get_samples stages the WHOLE window in a temporary device buffer of ns x nc x nfields doubles, on top of the ring (the
 * size is in the message if that allocation fails): at large chain counts read a few samples per call, or use the _dev form. */
int mcmcx_get_samples(mcmcx_handle h, int32_t s0, int32_t ns, int32_t c0, int32_t nc, int32_t layout, double *host_out);
int mcmcx_get_samples_dev(mcmcx_handle h, int32_t s0, int32_t ns, int32_t c0, int32_t nc, int32_t layout, void *dev_out);

/* ---- convergence summary of the retained samples, reduced on the device where the ring lies (no counterpart in the reference):
 * posterior mean and standard deviation, split-R-hat, bulk ESS (Stan's multi-chain estimator over split chains with Geyer's initial
 * monotone sequence, applied to the values as they are: the rank-normalised R-hat and bulk ESS, which mean something for a heavy-tailed
 * field too, are mcmcx_samples_stats_step's below) and MCSE of every field of the store.  Device scratch is ntiles x nfields x (maxlag + 3) doubles (plus nfields
 * for the shift and one stats vector), not a copy of the window; no sampling kernel and no state of the run is touched, so a run
 * with a summary call in the middle is the same run.  The definition is the contract -- sums in a fixed order, restated bit for bit
 * in numpy by tests/diag_ref.py:
 *   Window: retained samples s0 .. s0 + ns - 1 (ns >= 4) of ALL chains, oldest first.  n_h = ns / 2 (integer); half 0 is window
 *   samples 0 .. n_h - 1, half 1 is ns - n_h .. ns - 1 (an odd ns drops the middle sample); K = min(maxlag, n_h - 1) with
 *   0 <= maxlag <= MCMCX_DIAG_MAXLAG; M = 2 nchains split chains.
 *   shift_f: the caller's shift[f], or with shift == NULL field f of chain 0 in window sample 0.
 *   Per chain, half h and field f, in IEEE doubles without contraction:
 *     y_i = x_i - shift_f;  s = (..((y_0 + y_1) + y_2) ..);  m = s / n_h;  z_i = y_i - m;
 *     g_t = sum over i = 0 .. n_h - 1 - t, ascending, of z_i * z_{i+t} (a = a + z_i * z_{i+t} from +0.0), t = 0 .. K.
 *   The chain's terms per field: m_0 + m_1, m_0 m_0 + m_1 m_1, g0_t + g1_t (t = 0 .. K).
 *   Across chains, exactly the pooled moments' reduction: the 64 lanes of a tile in the adjacent-pairs tree, a lane without a chain
 *   contributing +0.0, then the tiles in the fixed pairwise tree (for s = 1, 2, 4, ..: v[t] += v[t + s]; no partner, no addition).
 *   Result per field: S1, S2, G_0 .. G_K.
 *   The stats vector, 3 + nfields (maxlag + 4) doubles: [M, n_h, K, then per field: shift, S1, S2, G_0 .. G_maxlag], slots beyond K
 *   +0.0.  It is additive over disjoint chain sets that used the same shift (add M and the sums): several ranks add their vectors
 *   and finish; nothing collective happens here.
 *   Finish (mcmcx_samples_diag: pure host, no handle, no device), per field, in this order:
 *     W = G_0 / (M (n_h - 1));  Bn = (S2 - S1 S1 / M) / (M - 1);  varp = W (n_h - 1) / n_h + Bn;  rhat = sqrt(varp / W);
 *     rho_0 = 1, rho_t = 1 - (W - G_t / (M n_h)) / varp;
 *     pairs P_k = rho_2k + rho_2k+1 for k = 0 .. (K + 1) / 2 - 1: stop at the first P_k <= 0, each kept P_k := min(P_k, P_k-1);
 *     tau = -1 + 2 sum of kept P_k;  tau = max(tau, 1 / log10(M n_h));  ess = M n_h / tau;
 *     truncated = 1 if no pair stopped the sum, else 0;  mean = shift + S1 / M;  sd = sqrt(varp);  mcse = sd / sqrt(ess).
 *   table[nfields][8]: mean, sd, rhat, ess, mcse, W, Bn, truncated.  truncated = 1: the lag window ended while the pairs were still
 *   positive, so ess is an UPPER bound (raise maxlag, or thin more).  maxlag = 0 gives K = 0 and no pairs: ess and mcse are NaN
 *   and truncated = 1 -- the R-hat-only mode.  Non-finite samples propagate.
 * Reading the numbers: with n_h short against the autocorrelation time split-R-hat sits above 1 even at stationarity (an AR(1)
 * with coefficient 0.5 and n_h = 32 gives 1.03, with 0.9 it gives 1.30): choose thin, not capacity, to fix it.  Unless the chains
 * were given start points of their own (mcmcx_set_par0_all, mcmcx_set_par0_spread) they all start at par0, and R-hat then measures
 * stationarity within the window, not recovery from dispersed starts.
 * mcmcx_samples_stats copies the vector to host memory and synchronises; mcmcx_samples_stats_dev writes it into the caller's DEVICE
 * buffer, asynchronous on the engine's stream.  shift, if given, is host memory in both forms; it is staged during the call, so it need
 * only stay valid until the call returns.  Refused with -49 (the reason in
 * mcmcx_last_error) before anything is launched: a null handle or output, an engine that is not inited, sampling off, ns < 4, a
 * window outside the retained samples, maxlag outside 0 .. MCMCX_DIAG_MAXLAG.  The scratch is allocated at the first call, grows
 * only and is freed by mcmcx_destroy; if the allocation fails the size is in the message (-101). */
#define MCMCX_DIAG_MAXLAG 32
/* 3 + nfields (maxlag + 4) (no counterpart in the reference) */
int32_t mcmcx_samples_stats_len(mcmcx_handle h, int32_t maxlag);
/* the stats vector of the window to host memory (no counterpart in the reference) */
int mcmcx_samples_stats(mcmcx_handle h, int32_t s0, int32_t ns, int32_t maxlag, const double *shift /* [nfields] host, or NULL */,
                        double *host_out);
/* ... into a device buffer, asynchronous on the engine's stream (no counterpart in the reference) */
int mcmcx_samples_stats_dev(mcmcx_handle h, int32_t s0, int32_t ns, int32_t maxlag, const double *shift, void *dev_out);
/* the finish: stats vector (one engine's, or the sum of several) -> table[nfields][8] (no counterpart in the reference) */
int mcmcx_samples_diag(const double *stats, int32_t nfields, int32_t maxlag, double *table);

/* ---- the summary of an elementwise function of the retained samples (no counterpart in the reference): the other half of the standard
 * table -- tail ESS, folded split-R-hat, the MCSE of the sd, the ESS at a quantile -- is the summary above of u(x) instead of x, reduced
 * where the ring lies, with the same scratch (plus nfields doubles for a) and without a copy of the window.  The definition, restated
 * bit for bit in numpy by tests/diag_xf_ref.py:
 *   For a call with `kind` and a per-field parameter a[nfields] the stats vector is BY DEFINITION the vector mcmcx_samples_stats would
 *   return if every stored value x of field f were replaced by u_f(x):
 *     kind 0, MCMCX_XF_IDENTITY:  u_f(x) = x.  a is not looked at and may be NULL; the result has the same bits as mcmcx_samples_stats.
 *     kind 1, MCMCX_XF_LE:        u_f(x) = 1.0 if key(x) <= key(a_f), else +0.0 -- the KEY order of mcmcx_samples_order_stats below, not
 *                                 the IEEE comparison: le of mcmcx_samples_counts and the values of mcmcx_samples_quantiles mean the
 *                                 same thing here, NaNs take part and -0.0 lies below +0.0.
 *     kind 2, MCMCX_XF_FOLD:      u_f(x) = fabs(x - a_f): one IEEE subtraction, then the sign cleared.
 *     kind 3, MCMCX_XF_SQUARE:    d = x - a_f;  u_f(x) = d * d: two IEEE operations, no contraction.
 *   Everything after u is the summary's definition above, word for word: y_i = u(x_i) - shift_f, the half means, the lag sums in their
 *   order, the tile tree with padding lanes masked to +0.0, the tiles' pairwise tree, the vector's length and layout.  shift == NULL
 *   means u_f of field f of chain 0 in window sample 0.  mcmcx_samples_diag finishes the vector unchanged, and it stays additive over
 *   engines that used the same kind, a and shift.
 *   Non-finite values propagate as the arithmetic says (kind 1 maps every value, NaNs included, to 1.0 or +0.0).  An indicator that is
 *   constant over the window -- a_f below or above every value -- has G_0 = 0, so W = 0 and its R-hat and ESS are NaN (0 / 0), not 1.
 * Reading the numbers: tail ESS is the smaller ess of kind 1 at the 5 % and the 95 % quantile; the MCSE of P(x <= q) is
 * sqrt(p (1 - p) / ess).  Folded split-R-hat is rhat of kind 2 at the median: when all chains start at par0 (no mcmcx_set_par0_all /
 * mcmcx_set_par0_spread) the plain R-hat measures
 * drift, and chains that agree in location but differ in scale show only here.  The MCSE of the sd is mcse / (2 sd) of kind 3 at the
 * mean (the delta method on the variance).  For an indicator a shift of zeros is exact (every y is 0 or 1).
 * a and shift are host memory in both forms and are staged during the call.  mcmcx_samples_stats_of copies the vector to host memory
 * and synchronises; mcmcx_samples_stats_of_dev writes it into the caller's DEVICE buffer, asynchronous on the engine's stream.  Refused
 * with -53 (the reason in mcmcx_last_error) on the host, before anything is launched or allocated: a kind outside 0 .. 3, a NULL a with
 * kind != 0, and everything mcmcx_samples_stats refuses. */
#define MCMCX_XF_IDENTITY 0
#define MCMCX_XF_LE 1
#define MCMCX_XF_FOLD 2
#define MCMCX_XF_SQUARE 3
/* the stats vector of u(window) to host memory (no counterpart in the reference) */
int mcmcx_samples_stats_of(mcmcx_handle h, int32_t s0, int32_t ns, int32_t maxlag, int32_t kind, const double *a /* [nfields] host */,
                           const double *shift /* [nfields] host, or NULL */, double *host_out);
/* ... into a device buffer, asynchronous on the engine's stream (no counterpart in the reference) */
int mcmcx_samples_stats_of_dev(mcmcx_handle h, int32_t s0, int32_t ns, int32_t maxlag, int32_t kind, const double *a,
                               const double *shift, void *dev_out);

/* ---- exact order statistics, tail counts and quantiles of the retained samples, reduced on the device where the ring lies (no
 * counterpart in the reference): credible intervals, medians and tail probabilities of every field without moving the window.  The
 * r-th smallest of a multiset and an integer count depend on no order of summation, so the results are exact; the definition is
 * restated in numpy by tests/quant_ref.py:
 *   Window: retained samples s0 .. s0 + ns - 1 (ns >= 1) of ALL nchains chains; n = ns * nchains values per field, as int64_t (it
 *   passes 2**31 at real sizes).  The padding lanes of the last tile are never counted.
 *   Key: with b the double's bits, key(x) = b ^ (b >> 63 ? 0xFFFFFFFFFFFFFFFF : 0x8000000000000000).  The unsigned order of the keys
 *   is the total order: negative NaNs < -inf < ... < -0.0 < +0.0 < ... < +inf < positive NaNs.  It is the key order, not the IEEE
 *   comparison: -0.0 lies below +0.0 and NaNs take part.  On doubles that are no NaN it sorts as IEEE does.
 *   Order statistic: os_f(r), 0 <= r < n, is the value of field f whose key is the r-th smallest of the window's n keys, returned
 *   with its own bits (the inverse key map).
 *   Counts: for a threshold x, lt_f(x) is the number of window values of field f with key < key(x), le_f(x) with key <= key(x).
 *   Counts are additive over disjoint chain sets: several ranks bisect on summed counts for a rank of the union, and
 *   le_f(x) / n is P(field f <= x); nothing collective happens here.
 *   Quantile (Hyndman-Fan type 7, numpy's default position), in IEEE doubles without contraction:
 *     pos = p * (double)(n - 1);  lo = floor(pos);  hi = min(lo + 1, n - 1);  g = pos - lo;  a = os(lo);  b = os(hi);
 *     q = a when a and b have equal bits, otherwise q = a + (b - a) * g.
 * How: a most-significant-digit radix select on the keys, eight passes of one byte, each streaming the window once and counting
 * the digits of the values that match a rank's prefix with 64-bit integer atomics; no float atomic, no host round trip between the
 * passes.  The counts are one pass.  No sampling kernel and no state of the run is touched: a run with these calls in the middle
 * is the same run.  1 <= nr, nq <= MCMCX_QUANT_MAXR; ranks need be neither sorted nor distinct.  ranks, x and probs are host memory
 * in every form and are staged during the call, so they need only stay valid until it returns.  The host forms copy the result and
 * synchronise; the _dev forms write into the caller's DEVICE buffer, asynchronous on the engine's stream.  Device scratch is
 * nfields x nr x 260 64-bit words, allocated at the first call, growing only, freed by mcmcx_destroy; if the allocation fails the
 * size is in the message (-101).  Refused with -50 (the reason in mcmcx_last_error) on the host, before anything is launched or
 * allocated: a null handle, output or argument array, an engine that is not inited, sampling off, ns < 1, a window outside the
 * retained samples, nr or nq out of range, a rank outside 0 .. n - 1, a probability outside [0, 1] or NaN. */
#define MCMCX_QUANT_MAXR 32
/* os_f(ranks[k]) of every field to host memory, host_out[nfields][nr] (no counterpart in the reference) */
int mcmcx_samples_order_stats(mcmcx_handle h, int32_t s0, int32_t ns, int32_t nr, const int64_t *ranks /* [nr] host */,
                              double *host_out);
/* ... into a device buffer of nfields x nr doubles, asynchronous on the engine's stream (no counterpart in the reference) */
int mcmcx_samples_order_stats_dev(mcmcx_handle h, int32_t s0, int32_t ns, int32_t nr, const int64_t *ranks, void *dev_out);
/* lt and le of nq thresholds per field, x[nfields][nq] host -> host_out[nfields][nq][2] (no counterpart in the reference) */
int mcmcx_samples_counts(mcmcx_handle h, int32_t s0, int32_t ns, int32_t nq, const double *x, int64_t *host_out);
/* ... into a device buffer of nfields x nq x 2 64-bit integers, asynchronous on the engine's stream (no counterpart in the reference) */
int mcmcx_samples_counts_dev(mcmcx_handle h, int32_t s0, int32_t ns, int32_t nq, const double *x, void *dev_out);
/* the quantile's positions: ranks[2 nq] = lo, hi per probability, frac[nq] = g.  Pure host, no handle, no device; refuses (-50) a p
 * outside [0, 1], a NaN p and n < 1 (no counterpart in the reference) */
int mcmcx_samples_quantile_ranks(int64_t n, int32_t nq, const double *probs, int64_t *ranks, double *frac);
/* quantiles of every field, host_out[nfields][nq], nq <= MCMCX_QUANT_MAXR / 2: the ranks, their order statistics, the finish
 * (no counterpart in the reference) */
int mcmcx_samples_quantiles(mcmcx_handle h, int32_t s0, int32_t ns, int32_t nq, const double *probs, double *host_out);

/* ---- posterior covariance and correlation of the retained samples, reduced on the device where the ring lies, on the f64 matrix cores
 * (no counterpart in the reference, whose chaincmat is one chain's adaptation state): the joint second moment of ALL chains times a
 * window of retained samples.  Device scratch is ntiles x (nfields + nfields (nfields + 1) / 2) doubles for the tile rows (plus
 * nfields for the shift and one vector), not a copy of the window: 195 MB at 16384 tiles and 53 fields, 170 MB at 1024 tiles and 203
 * fields.  No sampling kernel and no state of the run is touched, so a run with these calls in the middle is the same run.  The
 * definition is the contract -- every sum has a fixed order -- restated bit for bit in numpy by tests/cov_ref.py:
 *   Window: retained samples s0 .. s0 + ns - 1 (ns >= 1) of ALL chains, oldest first; n = ns * nchains, held as int64_t and
 *   returned as a double.  All nfields fields of the store are used, in the store's order.
 *   shift_f: the caller's shift[f], or with shift == NULL field f of chain 0 in window sample 0 (mcmcx_samples_stats' rule).
 *   z_f = x_f - shift_f, one IEEE subtraction.
 *   Per tile T of 64 chains (lane c belongs to it when 64 T + c < nchains), for every field j and every pair j <= k, fma being the
 *   fused multiply-add with one rounding:
 *     s_j  = +0.0;  for each window sample w ascending, for each lane c ascending that belongs:  s_j  = s_j + z_j[w][c]
 *     g_jk = +0.0;  for each window sample w ascending, for each lane c ascending that belongs:  g_jk = fma(z_j[w][c], z_k[w][c], g_jk)
 *   A padding lane of the last tile contributes nothing (the kernel selects +0.0 for it, it does not multiply by zero:
 *   fma(+0, +0, a) = a and a + 0 = a for every a these chains can hold).  This is the order in which v_mfma_f64_16x16x4_f64 adds
 *   with the chains on its k axis, four per instruction in ascending k; s_j is the same chain against a row of ones
 *   (fma(z, 1.0, a) = a + z).
 *   Across tiles: the pooled moments' fixed pairwise tree (for s = 1, 2, 4, ..: v[t] += v[t + s]; no partner, no addition).
 *   The vector, mcmcx_samples_cov_len = 1 + 2 nfields + nfields (nfields + 1) / 2 doubles:
 *     [n, shift[nfields], S[nfields], G packed by rows of the upper triangle]
 *   pair j <= k at j nfields - j (j - 1) / 2 + (k - j), the order of mcmcx_pooled_moments' third part.  It is additive over disjoint
 *   chain sets that used the same shift: add n, S and G and keep the shifts; nothing collective happens here.
 *   Finish (mcmcx_samples_cov_finish: pure host, no handle, no device; corr may be NULL), without contraction:
 *     mean_j = shift_j + S_j / n
 *     C_jk   = (G_jk - S_j * S_k / n) / (n - 1)     for j <= k, mirrored into the full column-major nfields x nfields matrix
 *     corr_jk = C_jk / (sqrt(C_jj) * sqrt(C_kk))    off the diagonal;  corr_jj = 1.0 when C_jj > 0, else C_jj / (sqrt(C_jj) sqrt(C_jj))
 *   A field that is constant over the window (sspri under a flat prior) has C_jj = 0 and gives 0 / 0 = NaN in its row and column of
 *   corr, the diagonal included: the IEEE answer.  Non-finite samples propagate into the entries they take part in.
 * Reading the numbers: G - S S / n cancels, and a shift far from the mean costs as many digits as (mean - shift)^2 / variance has;
 * `mean` from mcmcx_samples_diag is a good shift (the default, one chain's value in the window, is good once the chains have met).
 * The theta block of C is a valid mcmcx_set_cmat0 of the next run -- the reference's mcmccovf.dat cycle over all chains.
 * mcmcx_samples_cov copies the vector to host memory and synchronises; mcmcx_samples_cov_dev writes it into the caller's DEVICE
 * buffer, asynchronous on the engine's stream.  shift, if given, is host memory in both forms and is staged during the call.  Refused
 * with -51 (the reason in mcmcx_last_error) on the host, before anything is launched or allocated: a null handle or output, an engine
 * that is not inited, sampling off, ns < 1, a window outside the retained samples; the finish also refuses a null argument,
 * nfields < 1, and an n in the vector that is below 2 or no integer.  The scratch is a buffer of its own, allocated at the first call,
 * growing only, freed by mcmcx_destroy; if the allocation fails the size is in the message (-101). */
/* 1 + 2 nfields + nfields (nfields + 1) / 2 (no counterpart in the reference) */
int32_t mcmcx_samples_cov_len(mcmcx_handle h);
/* the cov vector of the window to host memory (no counterpart in the reference) */
int mcmcx_samples_cov(mcmcx_handle h, int32_t s0, int32_t ns, const double *shift /* [nfields] host, or NULL */, double *host_out);
/* ... into a device buffer, asynchronous on the engine's stream (no counterpart in the reference) */
int mcmcx_samples_cov_dev(mcmcx_handle h, int32_t s0, int32_t ns, const double *shift, void *dev_out);
/* the finish: cov vector (one engine's, or the sum of several) -> mean[nfields], cov and corr column-major nfields x nfields; corr may
 * be NULL (no counterpart in the reference) */
int mcmcx_samples_cov_finish(const double *vec, int32_t nfields, double *mean, double *cov, double *corr);

/* ---- batch-means covariance of the retained samples, reduced on the device where the ring lies, on the f64 matrix cores (no
 * counterpart in the reference): the covariance, over ALL chains, of the MEANS of batches of `batch` consecutive window samples --
 * the one primitive behind the two joint diagnostics the per-field summary cannot give: the multivariate effective sample size
 * (mcmcx_samples_mess, batch ~ sqrt(ns)) and the multivariate split-R-hat (mcmcx_samples_mpsrf, batch = half the window).  The
 * covariance's kernel body with the batch accumulation in front of its staging: the same rows are streamed once, 1 / batch of the
 * matrix instructions are issued.  Scratch, vector layout, tree and shift rule are mcmcx_samples_cov's.  No sampling kernel and no
 * state of the run is touched.  The definition is the contract, restated bit for bit in numpy by tests/bm_ref.py:
 *   Window: retained samples s0 .. s0 + ns - 1 of ALL chains, oldest first, under mcmcx_samples_cov's rules.  1 <= batch <= ns,
 *   nb = ns / batch in integer division; batch k is window samples k batch .. (k + 1) batch - 1; the last ns - nb batch samples of
 *   the window are not read.
 *   shift_f: the caller's shift[f], or with shift == NULL field f of chain 0 in window sample 0 (mcmcx_samples_cov's rule).
 *   Batch mean, per chain, field and batch, in IEEE doubles without contraction:
 *     z_i = x_i - shift_f;   s = (..((z_0 + z_1) + z_2)..), the sum starting at z_0, not at +0.0;   y = s / (double)batch
 *   Per tile of 64 chains, the covariance's order with the batch means in the place of z:
 *     s_j  = +0.0;  for each batch k ascending, for each lane c ascending that belongs:  s_j  = s_j + y_j[k][c]
 *     g_jk = +0.0;  for each batch k ascending, for each lane c ascending that belongs:  g_jk = fma(y_j[k][c], y_k[k][c], g_jk)
 *   A padding lane of the last tile is selected to +0.0, not multiplied.
 *   Across tiles: the pooled moments' fixed pairwise tree.
 *   The vector, mcmcx_samples_cov_len doubles in the cov vector's layout:  [n_b, shift[nfields], S[nfields], G packed]
 *   with n_b = nb * nchains, held as int64_t and returned as a double.
 * Consequences: mcmcx_samples_cov_finish applied to it gives the mean and the covariance of the batch means.  It is additive over
 * disjoint chain sets that used the same shift and the same batch.  With batch = 1 it has the bits of mcmcx_samples_cov's vector
 * (y = z / 1.0 = z).
 * mcmcx_samples_cov_bm copies the vector to host memory and synchronises; mcmcx_samples_cov_bm_dev writes it into the caller's DEVICE
 * buffer, asynchronous on the engine's stream.  Refused with -55 (the reason in mcmcx_last_error) on the host, before anything is
 * launched or allocated: everything mcmcx_samples_cov refuses, and a batch outside 1 .. ns. */
/* the batch-means vector of the window to host memory (no counterpart in the reference) */
int mcmcx_samples_cov_bm(mcmcx_handle h, int32_t s0, int32_t ns, int32_t batch, const double *shift /* [nfields] host, or NULL */,
                         double *host_out);
/* ... into a device buffer, asynchronous on the engine's stream (no counterpart in the reference) */
int mcmcx_samples_cov_bm_dev(mcmcx_handle h, int32_t s0, int32_t ns, int32_t batch, const double *shift, void *dev_out);
/* The two finishes: pure host, no handle, no device, without contraction.  Both take a selection sel[nsel] of field indices (a field
 * that is constant over the window, sspri under a flat prior, makes every matrix singular: leave it out), the cov vector
 * (mcmcx_samples_cov) and the batch-means vector of the SAME samples; the two shifts may differ.  With [n, shift, S, G] one vector,
 * C(vec)_jk = (G_jk - S_j * S_k / n) / (n - 1) is mcmcx_samples_cov_finish's.  Refused with -55: a null cov_vec, bm_vec, sel or out4,
 * nfields < 1, nsel outside 1 .. nfields, a sel[j] outside 0 .. nfields - 1, an n in either vector that is below 2 or no integer,
 * and what each states below.
 * The Cholesky factor both use, A = R' R with R upper triangular, column by column, sums ascending, no fma:
 *     for j = 0 .. nsel - 1:
 *         for i = 0 .. j - 1:   t = 0;  for k = 0 .. i - 1: t = t + R_ki * R_kj;   R_ij = (A_ij - t) / R_ii
 *         t = 0;  for k = 0 .. j - 1: t = t + R_kj * R_kj;   p = A_jj - t;   R_jj = sqrt(p)
 * A pivot p that is not > 0 (NaN included) is no refusal: the return value is +1, a warning, and the results that need the factor
 * are NaN.  logdet A = 2 * (..((log R_00 + log R_11) + ..), summed ascending.
 *
 * mcmcx_samples_mess: the multivariate effective sample size of Vats, Flegal and Jones (2019) in its replicated-batch-means form.
 * Also refuses batch < 1 and bm_vec[0] * batch != cov_vec[0]: both vectors must cover the same nb * batch samples of every chain
 * (hand mcmcx_samples_cov the window trimmed to nb * batch samples).  n = cov_vec[0];
 *     Lambda = C(cov_vec)[sel, sel];   Sigma = batch * C(bm_vec)[sel, sel]
 *     mess = n * exp((logdet Lambda - logdet Sigma) / nsel);     out4 = {mess, n, logdet Lambda, logdet Sigma}
 *     ess_out[j] = n * Lambda_jj / Sigma_jj      (ess_out may be NULL)
 * Sigma / n is the Monte-Carlo covariance of the mean vector: its error ellipsoid.  ess_out is the univariate batch-means ESS, a
 * second opinion beside mcmcx_samples_diag's; mess may exceed n (antithetic chains).  A failed factor leaves its logdet and mess NaN.
 *
 * mcmcx_samples_mpsrf: the multivariate potential scale reduction factor of Brooks and Gelman (1998) over split chains.  cov_vec
 * covers a window of exactly 2 n_h samples, bm_vec the same window with batch = n_h, so bm_vec[0] = M = 2 nchains split chains;
 * also refuses n_h < 2, an odd bm_vec[0] and bm_vec[0] * n_h != cov_vec[0].  n = cov_vec[0]; per selected pair
 *     T   = G - S * S' / n        from cov_vec           SSm = G_b - S_b * S_b' / M      from bm_vec
 *     W   = (T - n_h * SSm) / (M * (n_h - 1))            Bn  = SSm / (M - 1)
 *     lambda1 = the largest eigenvalue of C = R^-T Bn R^-1 with W = R' R.  The factor above decides whether W is positive definite;
 *               for lambda1 the factor and the two triangular solves are repeated in long double (the reduction costs cond(W)
 *               roundings of its working precision), a cyclic Jacobi on the rounded C gives the eigenvector u, and
 *               lambda1 = u' C u / u' u
 *     mpsrf = sqrt((n_h - 1) / n_h + lambda1);           out4 = {mpsrf, lambda1, M, n_h}
 * W_out and Bn_out (column-major nsel x nsel, either may be NULL) take W and Bn.  With nsel = 1 this is mcmcx_samples_diag's
 * split-R-hat; coda's factor (M + 1) / M on lambda1 is left out on purpose, so that the two agree.  mpsrf >= the split-R-hat of every
 * selected field (the Rayleigh quotient at a unit vector).  A W that is not positive definite returns +1 with NaN in out4[0 .. 1]. */
int mcmcx_samples_mess(const double *cov_vec, const double *bm_vec, int32_t nfields, int32_t batch, int32_t nsel, const int32_t *sel,
                       double *out4, double *ess_out /* [nsel] or NULL */);
int mcmcx_samples_mpsrf(const double *cov_vec, const double *bm_vec, int32_t nfields, int32_t n_h, int32_t nsel, const int32_t *sel,
                        double *out4, double *W_out, double *Bn_out /* col-major nsel^2, or NULL */);

/* ---- marginal and pairwise joint histograms of the retained samples, counted on the device where the ring lies (no counterpart in
 * the reference, whose toolchain draws its hist / dens / pairs panels from a chain file): the density of every field and of pairs of
 * fields without moving the window.  A histogram is a vector of integers and depends on no order of summation, so the results are
 * exact; the definition is restated in numpy by tests/hist_ref.py:
 *   Window: retained samples s0 .. s0 + ns - 1 (ns >= 1) of ALL nchains chains; n = ns * nchains values per field, as int64_t.  The
 *   padding lanes of the last tile are never counted.
 *   Key order: everything is in the order of the keys of mcmcx_samples_order_stats above -- the IEEE order on doubles that are no
 *   NaN, with -0.0 < +0.0, negative NaNs below everything and positive NaNs above.
 *   Edges: edges[nfields][nbins + 1], host memory, 1 <= nbins <= MCMCX_HIST_MAXBINS.  Within a field the edges are non-decreasing by
 *   key; equal neighbours are allowed and give an empty bin, +-inf is allowed; a NaN edge or a decreasing pair is refused.
 *   Cell: cell_f(x) is the number of edges e_i of field f with key(e_i) <= key(x), 0 .. nbins + 1.  Cell 0 is below e_0; cell b,
 *   1 <= b <= nbins, is e_{b-1} <= x < e_b -- left-closed and right-open, the last bin too, unlike np.histogram; cell nbins + 1 is at
 *   or above e_nbins.  Positive NaNs land in cell nbins + 1, negative NaNs in cell 0.
 *   1-D: out[nfields][nbins + 2] int64, the number of window values of field f in each cell.  The cells of a field sum to n, and the
 *   running sum through cell b equals lt_f(e_b) of mcmcx_samples_counts.
 *   2-D: pairs[npairs][2] holds field indices in 0 .. nfields - 1, 1 <= npairs <= MCMCX_HIST2_MAXPAIRS; j == k and repeated pairs
 *   are allowed.  1 <= nbins <= MCMCX_HIST2_MAXBINS, the edge table has the same layout (all nfields rows).
 *   out[npairs][nbins + 2][nbins + 2] counts the (sample, chain) points with cell_j(x_j) = a and cell_k(x_k) = b at [a][b]: summing
 *   over b gives field j's 1-D result, summing over a field k's.  96 bins keep (nbins + 2)^2 32-bit counters and both edge rows
 *   (40 KB) well inside a workgroup's default 64 KiB of LDS.
 *   Both results are additive over disjoint chain sets; nothing collective happens here.
 *   Uniform edges of one field (mcmcx_samples_hist_edges: pure host), without contraction:
 *     e_i = lo + (hi - lo) * ((double)i / nbins) for i < nbins, e_nbins = hi
 *   Density (mcmcx_samples_hist_density: pure host), n being the sum of the field's nbins + 2 cells:
 *     density_b = (double)count_b / ((double)n * (e_b - e_{b-1})),  1 <= b <= nbins;  an empty-width bin gives the IEEE answer.
 * How: one pass over the window in whole rows; the field's edge keys are staged in LDS, the cell comes from a binary search over
 * them, the counters are 32-bit in LDS (a block never counts 2**31 values) and are flushed with 64-bit integer atomics to the zeroed
 * table; the 2-D kernel gives each workgroup one pair and reads both fields' rows together.  No float atomic.  No sampling kernel and
 * no state of the run is touched: a run with these calls in the middle is the same run.  edges and pairs are host memory in every
 * form and are staged during the call, so they need only stay valid until it returns.  The host forms copy the result and
 * synchronise; the _dev forms write into the caller's DEVICE buffer, asynchronous on the engine's stream.  Device scratch is the
 * readers' one buffer: the edge keys and, for the host forms, the table.  Refused with -52 (the reason in mcmcx_last_error) on the
 * host, before anything is launched or allocated -- first what the arguments alone decide: a null output, edge table or pair list,
 * nbins or npairs out of range, a NaN or decreasing edge (of the first field's row; of the others once nfields is known), a pair
 * index outside 0 .. nfields - 1; then a null handle, an engine that is not inited, sampling off, ns < 1, a window outside the
 * retained samples. */
#define MCMCX_HIST_MAXBINS 1024
#define MCMCX_HIST2_MAXBINS 96
#define MCMCX_HIST2_MAXPAIRS 64
/* the 1-D table of every field to host memory, host_out[nfields][nbins + 2] (no counterpart in the reference) */
int mcmcx_samples_hist(mcmcx_handle h, int32_t s0, int32_t ns, int32_t nbins, const double *edges /* [nfields][nbins + 1] host */,
                       int64_t *host_out);
/* ... into a device buffer of nfields x (nbins + 2) 64-bit integers, asynchronous on the engine's stream (no counterpart in the
 * reference) */
int mcmcx_samples_hist_dev(mcmcx_handle h, int32_t s0, int32_t ns, int32_t nbins, const double *edges, void *dev_out);
/* the 2-D tables of npairs pairs of fields to host memory, host_out[npairs][nbins + 2][nbins + 2] (no counterpart in the reference) */
int mcmcx_samples_hist2(mcmcx_handle h, int32_t s0, int32_t ns, int32_t npairs, const int32_t *pairs /* [npairs][2] host */,
                        int32_t nbins, const double *edges /* [nfields][nbins + 1] host */, int64_t *host_out);
/* ... into a device buffer of npairs x (nbins + 2)^2 64-bit integers, asynchronous on the engine's stream (no counterpart in the
 * reference) */
int mcmcx_samples_hist2_dev(mcmcx_handle h, int32_t s0, int32_t ns, int32_t npairs, const int32_t *pairs, int32_t nbins,
                            const double *edges, void *dev_out);
/* nbins + 1 uniform edges of one field from lo to hi.  Pure host, no handle, no device; refuses (-52) a null output, nbins outside
 * 1 .. MCMCX_HIST_MAXBINS, a lo or hi that is not finite, lo >= hi and a result that is not non-decreasing (hi - lo overflows)
 * (no counterpart in the reference) */
int mcmcx_samples_hist_edges(double lo, double hi, int32_t nbins, double *edges_out);
/* the finish: 1-D counts[nfields][nbins + 2] (one engine's, or the sum of several) and their edges -> density_out[nfields][nbins].
 * Pure host, no handle, no device; refuses (-52) a null argument, nfields < 1, nbins outside 1 .. MCMCX_HIST_MAXBINS (no
 * counterpart in the reference) */
int mcmcx_samples_hist_density(const int64_t *counts, const double *edges, int32_t nfields, int32_t nbins,
                               double *density_out /* [nfields][nbins] */);

/* ---- the summary of a step function of the retained samples (no counterpart in the reference): the rank-normalised split-R-hat and
 * bulk ESS of Vehtari, Gelman, Simpson, Carpenter and Buerkner (2021) -- the Rhat and ess_bulk columns of Stan and ArviZ --, the ESS of an
 * interval probability P(a <= x < b) and of any binned functional are the summary above of
 *     u_f(x) = table_f[cell_f(x)]
 * reduced where the ring lies, with the same scratch (plus the staged edge keys and table) and without a copy of the window.  The
 * definition, restated bit for bit in numpy by tests/diag_step_ref.py:
 *   Edges: edges[nfields][nbins + 1], host memory, 1 <= nbins <= MCMCX_STEP_MAXBINS (512 cells), held to the rules of mcmcx_samples_hist:
 *   within a field non-decreasing by key; equal neighbours and +-inf are allowed; a NaN or a decreasing edge is refused.
 *   Table: table[nfields][nbins + 2] doubles, host memory.  Any bits are allowed; NaN and inf propagate as the arithmetic says.
 *   The stats vector is BY DEFINITION the vector mcmcx_samples_stats would return if every stored value x of field f were replaced by
 *   table[f][cell_f(x)], cell_f(x) being the histograms' cell: the number of edges e_i of field f with key(e_i) <= key(x), 0 .. nbins + 1.
 *   NaNs take part and -0.0 lies below +0.0.
 *   Everything after u is the summary's definition above, word for word: y_i = u(x_i) - shift_f, the half means, the lag sums in their
 *   order, the tile tree with padding lanes masked to +0.0, the tiles' pairwise tree, the vector's length and layout.  shift == NULL
 *   means u_f of field f of chain 0 in window sample 0.  mcmcx_samples_diag finishes the vector unchanged, and it stays additive over
 *   engines that used the same edges, table and shift.
 * Rank normalisation over cells: with the edges at order statistics of the window (mcmcx_samples_order_stats), the counts of
 * mcmcx_samples_hist and the table of mcmcx_samples_rank_scores, every value is replaced by the normal score of the AVERAGE RANK OF ITS
 * CELL -- ties are treated as the average-rank convention treats them, and 128 cells give the exact rank-normalised R-hat within 5e-4
 * and its ESS within 2.5 %.  A field that is constant over the window falls into one cell: G_0 = 0, NaN.
 * mcmcx_samples_rank_scores, per field, with n the sum of the field's nbins + 2 cells and before_b the sum of the cells below b, both in
 * int64_t: a cell with count_b > 0 gets
 *     p = ((double)(2 before_b + count_b + 1) * 0.5 - 0.375) / ((double)n + 0.25)
 * -- its average 1-based rank r in Blom's form (r - 3/8) / (n + 1/4) -- and the score Phi^-1(p); an empty cell gets +0.0.  Phi^-1 is
 * Wichura's algorithm AS241, routine PPND16 (Applied Statistics 37, 1988), operation by operation, without contraction.
 * edges, table and shift are host memory in both forms and are staged during the call.  mcmcx_samples_stats_step copies the vector to
 * host memory and synchronises; mcmcx_samples_stats_step_dev writes it into the caller's DEVICE buffer, asynchronous on the engine's
 * stream.  Refused with -54 (the reason in mcmcx_last_error) on the host, before anything is launched or allocated -- first what the
 * arguments alone decide: a null output, edges or table, nbins outside 1 .. MCMCX_STEP_MAXBINS, a NaN or decreasing edge; then
 * everything mcmcx_samples_stats refuses. */
#define MCMCX_STEP_MAXBINS 510
/* the stats vector of table[cell(window)] to host memory (no counterpart in the reference) */
int mcmcx_samples_stats_step(mcmcx_handle h, int32_t s0, int32_t ns, int32_t maxlag, int32_t nbins,
                             const double *edges /* [nfields][nbins + 1] host */, const double *table /* [nfields][nbins + 2] host */,
                             const double *shift /* [nfields] host, or NULL */, double *host_out);
/* ... into a device buffer, asynchronous on the engine's stream (no counterpart in the reference) */
int mcmcx_samples_stats_step_dev(mcmcx_handle h, int32_t s0, int32_t ns, int32_t maxlag, int32_t nbins, const double *edges,
                                 const double *table, const double *shift, void *dev_out);
/* 1-D counts[nfields][nbins + 2] (one engine's, or the sum of several) -> scores_out[nfields][nbins + 2], the table of normal scores.
 * Pure host, no handle, no device; refuses (-54) a null argument, nfields < 1, nbins outside 1 .. MCMCX_STEP_MAXBINS, a negative count,
 * a field whose counts add up to less than 1 (or to more than 2**61) (no counterpart in the reference) */
int mcmcx_samples_rank_scores(const int64_t *counts, int32_t nfields, int32_t nbins, double *scores_out);

/* Pooled mode across several GPUs: at every adaptation tick the engine writes its local moment vector
 * (mcmcx_pooled_moments_len doubles) to dev_buf, synchronises its stream and calls fn(user); fn must sum dev_buf
 * over all ranks in place (an RCCL all-reduce) and return after the result is visible.  Without a hook the local
 * moments are used (single GPU). */
typedef void (*mcmcx_exchange_t)(void *user);
int mcmcx_set_exchange(mcmcx_handle h, mcmcx_exchange_t fn, void *user, void *dev_buf);
/* pooled proposal state: chaincmat, chainmean, chainwsum and the shared factor R (column-major d x d) */
int mcmcx_get_pooled(mcmcx_handle h, double *cmat_colmajor, double *mean, double *wsum, double *R_colmajor);

/* ---- several GPUs of one node (no counterpart in the single-chain reference).  Chains are
 * sharded by rank (cfg.chain_id0 = rank * nchains keys the streams, so results do not depend on the GPU count); the
 * one exchange is the pooled moment vector, combined over RCCL (all-gather + a fixed pairwise tree over the ranks:
 * bit-identical on 1, 2, 4, 8 GPUs).  Attach a communicator before mcmcx_init; in pooled mode every adaptation tick
 * then uses the moments of ALL ranks.
 *   one process per GPU:   mcmcx_comm_create(key, rank, nranks, device, MCMCX_COMM_RCCL, &c) on every rank with the
 *                          same `key` (names a POSIX shm segment that carries the ncclUniqueId: one node, no MPI);
 *   one process, N GPUs:   mcmcx_comm_create_all(N, NULL, comms) (ncclCommInitAll), one engine per comms[i],
 *                          mcmcx_run_all / mcmcx_allreduce_moments_all drive them together.
 * MCMCX_COMM_HOST stages the gather through the shm segment instead of RCCL: for ranks that share one GPU. */
typedef struct mcmcx_comm *mcmcx_comm_t;
#define MCMCX_COMM_RCCL 0
#define MCMCX_COMM_HOST 1
int mcmcx_comm_create(const char *key, int32_t rank, int32_t nranks, int32_t device, int32_t backend, mcmcx_comm_t *out);
int mcmcx_comm_create_all(int32_t ndev, const int32_t *devices /* NULL: 0..ndev-1 */, mcmcx_comm_t *out /* [ndev] */);
int mcmcx_comm_destroy(mcmcx_comm_t c);
int32_t mcmcx_comm_rank(mcmcx_comm_t c);
int32_t mcmcx_comm_size(mcmcx_comm_t c);
int mcmcx_comm_barrier(mcmcx_comm_t c);
/* sum (op 0) / maximum (op 1) of n <= 512 host doubles over the ranks, in place (ncclAllReduce) */
int mcmcx_comm_allreduce_host(mcmcx_comm_t c, double *inout, int32_t n, int32_t op);
int mcmcx_set_comm(mcmcx_handle h, mcmcx_comm_t c);
/* pooled moments (layout of mcmcx_pooled_moments) of the chains of ALL ranks; collective: every rank calls it.
 * host_out may be NULL: the result stays on the device and the call is asynchronous on the engine's stream. */
int mcmcx_allreduce_moments(mcmcx_handle h, double *host_out);
int mcmcx_allreduce_moments_all(mcmcx_handle *hs, int32_t n, double *host_out);
/* mcmcx_run for the n engines of a one-process node, one host thread each */
int mcmcx_run_all(mcmcx_handle *hs, int32_t n, int32_t upto);

/* device time of the step kernel over all launches since the last reset, measured with HIP
 * events on the engine's stream; launches = number of step-kernel launches, steps = iterations */
int mcmcx_kernel_time(mcmcx_handle h, double *ms, int64_t *launches, int64_t *steps, int reset);

/* Test probes of the device primitives (no reference counterpart; used by tests/ only).
 * op: 0 log, 1 exp, 2 sqrt, 3 a/b, 4 fma(a,b,a), 5 drotg digest.  kind: 0 uniform, 1 normal, 2 gamma(a,b). */
int mcmcx_debug_math(int32_t op, int32_t n, const double *a, const double *b, double *out);
int mcmcx_debug_rng(uint32_t seed, uint32_t chain_id, int32_t kind, int32_t n, double a, double b, double *out,
                    uint64_t *nused);
/* element offset of row `field` of tile `tile` in slot `slot` of the sample store, [slot][ntiles][nfields][64] doubles: the host
 * build of the one function the store's kernels index with (no reference counterpart; a test checks it beyond 2**32).  Needs no device. */
int64_t mcmcx_debug_samples_offset(int64_t slot, int64_t ntiles, int64_t nfields, int64_t tile, int64_t field);
/* The order statistics' own kernels on a caller's array (no counterpart in the reference; tests only): values[n] is treated as a
 * store of one slot, one field and ceil(n / 64) tiles with n chains, out[nr] takes os(ranks[k]).  A run cannot put +-0, +-inf,
 * NaNs, denormals or values that differ in their last byte only into the ring; this can.  Refusals are -50. */
int mcmcx_debug_order_stats(int32_t device, int64_t n, const double *values, int32_t nr, const int64_t *ranks, double *out);
/* The covariance's own kernels on a caller's array (no counterpart in the reference; tests only): values[ns][nfields][nchains] host
 * is laid out as a store of ns slots and ceil(nchains / 64) tiles, the padding lanes of the last tile filled with NaN by this entry
 * so that the mask is exercised; out takes the cov vector.  A run cannot put NaN, inf, a forty-decade dynamic range or chosen field
 * counts into the ring; this can.  shift: [nfields] host or NULL.  Refusals are -51. */
int mcmcx_debug_samples_cov(int32_t device, int32_t nchains, int32_t nfields, int32_t ns, const double *values, const double *shift,
                            double *out);
/* The batch-means covariance's own kernels on a caller's array (no counterpart in the reference; tests only):
 * values[ns][nfields][nchains] host laid out as mcmcx_debug_samples_cov lays it out, the padding lanes of the last tile filled with
 * NaN by this entry; out takes the batch-means vector.  shift: [nfields] host or NULL.  Refusals are -55, what the arguments decide
 * before a device is looked for: a null values or out, nchains or ns < 1, nfields outside 1 .. 2047, batch outside 1 .. ns. */
int mcmcx_debug_samples_cov_bm(int32_t device, int32_t nchains, int32_t nfields, int32_t ns, int32_t batch, const double *values,
                               const double *shift, double *out);
/* The histograms' own kernels on a caller's array (no counterpart in the reference; tests only): values[ns][nfields][nchains] host is
 * laid out as a store of ns slots and ceil(nchains / 64) tiles, the padding lanes of the last tile filled with NaN by this entry (a
 * kernel that counted them would show them in the last cell); out1[nfields][nbins + 2] takes the 1-D table, out2[npairs][nbins + 2]
 * [nbins + 2] the 2-D tables of `pairs`; either may be NULL (then npairs and pairs are not looked at, or nbins may reach
 * MCMCX_HIST_MAXBINS).  chunk = 0 is the default number of window samples per block, a small chunk forces several window chunks per
 * tile.  A run cannot put +-0, +-inf, NaNs, denormals or values equal to an edge into the ring; this can.  Refusals are -52, what
 * the arguments decide before a device is looked for. */
int mcmcx_debug_samples_hist(int32_t device, int32_t nchains, int32_t nfields, int32_t ns, const double *values, int32_t nbins,
                             const double *edges, int32_t npairs, const int32_t *pairs, int32_t chunk, int64_t *out1, int64_t *out2);
/* The summary's own kernels, of u(x), on a caller's array (no counterpart in the reference; tests only): values[ns][nfields][nchains]
 * host is laid out as a store of ns slots and ceil(nchains / 64) tiles, the padding lanes of the last tile filled with NaN by this
 * entry (a kernel that did not mask them would sum them, and count them under kind 1 with a NaN a); out takes the stats vector of
 * mcmcx_samples_stats_of.  A run cannot put +-0, +-inf, NaNs, denormals or values equal to a into the ring; this can.  a: [nfields]
 * host (NULL with kind 0), shift: [nfields] host or NULL.  Refusals are -53, what the arguments decide before a device is looked for:
 * a kind outside 0 .. 3, a NULL a with kind != 0, a null values or out, nchains or nfields < 1, ns < 4, maxlag out of range. */
int mcmcx_debug_samples_stats(int32_t device, int32_t nchains, int32_t nfields, int32_t ns, const double *values, int32_t maxlag,
                              int32_t kind, const double *a, const double *shift, double *out);
/* The step summary's own kernels on a caller's array (no counterpart in the reference; tests only): values[ns][nfields][nchains] host
 * laid out as mcmcx_debug_samples_stats lays it out, the padding lanes of the last tile filled with NaN by this entry (a kernel that did
 * not mask them would look them up in the last cell and sum them); out takes the stats vector of mcmcx_samples_stats_step.  edges:
 * [nfields][nbins + 1] host, table: [nfields][nbins + 2] host, shift: [nfields] host or NULL.  Refusals are -54, what the arguments
 * decide before a device is looked for: a null out, edges, table or values, nbins out of range, a NaN or decreasing edge, nchains or
 * nfields < 1, ns < 4, maxlag out of range. */
int mcmcx_debug_samples_stats_step(int32_t device, int32_t nchains, int32_t nfields, int32_t ns, const double *values, int32_t maxlag,
                                   int32_t nbins, const double *edges, const double *table, const double *shift, double *out);
/* The adaptation's singular value decomposition on a caller's matrices (no counterpart in the reference; tests only), in each of the
 * engine's three statements of the pinned one-sided Jacobi routine: form 0 the host's (the shared initial factor; no device is
 * touched), form 1 the lane form (one lane per matrix, the matrices interleaved into tiles of 64 as the engine stores them; lanes
 * past nmat and lanes with need == 0 are inactive), form 2 the blocked kernels (npar 48 .. 256), chosen and launched by the very
 * functions the adaptation tick calls, with nmat as its number of chains.  A run feeds these routines covariances of smooth chains
 * only; this can feed zeros, ties, rank-deficient, ill-scaled and non-finite matrices, and neighbours that converge in different
 * sweeps.  A: [nmat][d * d] column-major symmetric, host; need: [nmat] host, 0 = leave this matrix out, or NULL = all.
 * V_out[nmat][d * d] takes the singular vectors (columns), s_out[nmat][d] the singular values, descending; rows of matrices with
 * need == 0 are left as the caller filled them, in sweeps_out too.  sweeps_out: [nmat] or NULL, the number of sweeps in which the
 * matrix rotated (60 at the cap: the routine's return value).  forms: NULL, or a buffer of len bytes for the names of what ran:
 * "host_symsvd", "symsvd_dev", or the blocked form's two kernel instances joined by "+".  Refusals are -1, decided before a device
 * is looked for: a null A, V_out or s_out, d < 1, nmat < 1, an unknown form, form 2 outside npar 48 .. 256, a len too small. */
int mcmcx_debug_symsvd(int32_t device, int32_t form, int32_t d, int32_t nmat, const double *A, const uint8_t *need, double *V_out,
                       double *s_out, int32_t *sweeps_out, char *forms, int32_t len);
/* The adaptation tick's own factorisation -- MCMC_calculate_R: dpotf2, the 2.4 / sqrt(npar) scaling, with delayed rejection dpotri and
 * R2 = R / drscale; with condmax > 0 the SVD branch -- on a caller's covariances, in the kernel instances the engine's plan chose (no
 * counterpart in the reference; tests only).  h: an initialised per-chain adaptive engine (not pooled, not method = 'ram', doadapt or
 * doburnin set).  cmat: [nchains][npar * npar] column-major symmetric, host, its upper triangle packed into the chains' covariance
 * (chains with need == 0 keep theirs); need: [nchains] host, 0 = this chain does not recompute, or NULL = all.  The entry sets the
 * chains' tick flags to "recompute the factor" where need and to nothing elsewhere (and restores them), presets the chains' LAPACK
 * info to MCMCX_DEBUG_INFO_SENTINEL, launches what the tick launches for the factorisation -- the same function, with mode 0, in which
 * the covariance bookkeeping rewrites what it read -- and synchronises.  info_out[nchains] takes the chains' info as the kernels left
 * it: 0, dpotf2's failing pivot (1-based; the SVD branch: npar when the largest singular value is 0), the sentinel where need == 0.
 * forms: NULL, or a buffer of len bytes for the names of what ran: "adapt_post_kernel<false,false>", or
 * "adapt_post_kernel<false,false>:3+tile_factor_kernel<2,4>" (the number is the phase), or for the blocked SVD
 * "adapt_post_kernel<true,false>:1+<sweep>+<replay>+adapt_post_kernel<true,false>:2".  R, R2, iC, the status bits and the (floored)
 * covariance are read with mcmcx_get_R, mcmcx_get_dr, mcmcx_get_counters and mcmcx_get_chaincov.  Refusals are -57, decided before
 * anything is written or launched: a null h, cmat or info_out, an engine that is not initialised, pooled, method = 'ram' or without
 * adaptation, a len too small. */
#define MCMCX_DEBUG_INFO_SENTINEL (-77)
int mcmcx_debug_calculate_R(mcmcx_handle h, const double *cmat, const uint8_t *need, int32_t *info_out, char *forms, int32_t len);
/* The host's statement of the same (the shared initial factor's host_initial_R and host_potri; no device, no handle): A [d * d]
 * column-major symmetric; R_out [d * d] takes the scaled factor's upper triangle (zeros below) and info_out[0] dpotf2's info; when that
 * is 0, iC_out [d * d] (may be NULL) takes dpotri's result on R and info_out[1] its info (a zero on the diagonal: iC_out untouched).
 * Refused with -57, nothing written: a null A, R_out or info_out, d outside 1 .. 4096. */
int mcmcx_debug_host_calculate_R(int32_t d, const double *A, double *R_out, double *iC_out, int32_t *info_out);
/* the host build of the key map the order statistics sort by (no counterpart in the reference): the key of x's bits, or with
 * inverse != 0 the bits whose key x's bits are.  Needs no device. */
int64_t mcmcx_debug_quant_key(double x, int32_t inverse);
/* The engine's kernel-selection tables (which sampling kernel a configuration runs: launch_step / launch_group / launch_scam of
 * mcx_api.hip), entry `index` as "family:name" into buf -- the name mcmcx_last_kernel reports after a run.  Returns the number
 * of entries (index = -1, buf = NULL: count only).  Needs no device.  tests/test_kernel_table.py requires a parity test per entry. */
int mcmcx_debug_kernel_table(int32_t index, char *buf, int32_t len);
/* The template instance(s) the last mcmcx_run launched for the step, joined by '+', into buf: a group entry stands for one instance
 * per (group width, npar rounded up, delayed-rejection form, target kind) -- "group_step_kernel<16,20,0,gauss>",
 * "group_step_kernel<4,8,1,any>" (the general delayed-rejection form takes its target at run time),
 * "group_step_kernel<16,20,2,banana>+group_step_kernel<16,20,1,any>" (the power-of-two form queues both), "group_ram_kernel<32>";
 * every other entry is the name mcmcx_last_kernel reports, and "" before the first run.  Read-only, nothing is launched.  Refused with
 * -57, nothing written: a null h or buf, a len too small. */
int mcmcx_debug_last_instance(mcmcx_handle h, char *buf, int32_t len);
/* every chain's SVD proposal factor (per-chain mode, condmax > 0) replaced by R (column-major d x d; scam: the rotation)
 * and qcovstd (scam; NULL = keep): a test feeds the factors an external dgesvd returned at an adaptation */
int mcmcx_debug_set_factor(mcmcx_handle h, const double *R_colmajor, const double *qcovstd);

#ifdef __cplusplus
}
#endif
#endif
