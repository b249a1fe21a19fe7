// tools/variants/variants.inc -- kernel forms that were MEASURED AND LOST, kept buildable outside the product (VERDICT round 5, item 3).
// Included by mcx_api.hip only under -DMCX_VARIANTS (tools/build_variant.sh NAME -DMCX_VARIANTS -> variants_build/libmcmcx_NAME.so);
// libmcmcx.so is never built with it, so none of this can be the engine's choice.  Selection at run time, in the variant build only:
//   MCMCX_POOLED_WAVES=3   pooled_mfma2_kernel   a tile as a workgroup of two waves            80.3 against 73.7 ms (profiles/r05_a/c4_pooled_phases.txt)
//   MCMCX_POOLED_WAVES=4   pooled_mfma3_kernel   half a tile per wave, no workgroup            91.2 against 73.5 ms (profiles/r05_e/pooled_carry_ab.txt)
//   MCMCX_DR_GENERAL=1     step_kernel<false, true, false>   delayed rejection through the general step_body<DR>   (superseded by step_kernel_dr, round 2)
//   MCMCX_SVD_SHARED_ROT=1 svd_sweep_stream32s_kernel        a pair's rotation worked out once per pair            0.688 against 0.525 s per adaptation
//   MCMCX_COV_FIFO=1       adapt_cov_{diag,off}_fifo_kernel  the covariance update's folds behind a per-lane FIFO   104.9 against 33.7 ms (profiles/r06_d)
// All five are bit-equal to the library's forms (they were table entries with parity tests up to round 5: git show ccf9723:tests/test_gpu_pooled.py,
// test_gpu_parity.py); tools/variants/check_variants.py reruns those comparisons against a variant build.
#include "mcx_pooled2.hpp"
#include "mcx_svd_shared_rot.hpp"
#include "mcx_cov_fifo.hpp"
static int variant_env(const char *name) { const char *e = getenv(name); return e ? atoi(e) : -1; }
static bool variant_pooled_ok(const mcmcx_engine *h) { return h->plan.pooled_mfma && !h->dodr && h->d >= 17 && h->d <= 64; }
#define MCX_VARIANT_STEP_ENTRIES \
    {"step", "pooled_mfma3_kernel", [](const mcmcx_engine *h) { return variant_pooled_ok(h) && variant_env("MCMCX_POOLED_WAVES") == 4; }, \
     [](mcmcx_engine *h, int it0, int it1) { hipLaunchKernelGGL(pooled_mfma3_kernel, dim3(2 * h->ntiles), dim3(64), PooledMfmaLds(h->d).bytes / 2, STEP_ARGS, STEP_TGT, h->pool.d_RT); }, SH_RT}, \
    {"step", "pooled_mfma2_kernel", [](const mcmcx_engine *h) { return variant_pooled_ok(h) && variant_env("MCMCX_POOLED_WAVES") == 3; }, \
     [](mcmcx_engine *h, int it0, int it1) { hipLaunchKernelGGL(pooled_mfma2_kernel, dim3(h->ntiles), dim3(128), PooledMfmaLds(h->d).bytes, STEP_ARGS, STEP_TGT, h->pool.d_RT); }, SH_RT}, \
    {"step", "step_kernel<false, true, false>", [](const mcmcx_engine *h) { return !h->pooled && kernel_method(h) != M_RAM && h->dodr && !phased(h) && variant_env("MCMCX_DR_GENERAL") == 1; }, \
     [](mcmcx_engine *h, int it0, int it1) { hipLaunchKernelGGL((step_kernel<false, true, false>), G1, lds_step(h), STEP_ARGS, STEP_RS, STEP_TGT, h->E.sharedR); }},
static bool variant_svd_sweep(hipStream_t stream, double *Gc, mcx_d2 *rot, uint8_t *state, int *anyrot, int nlanes, int d, size_t lss)
{
    if (variant_env("MCMCX_SVD_SHARED_ROT") != 1) return false;
    if (d <= 64) hipLaunchKernelGGL(svd_sweep_stream32s_kernel<8>, dim3(nlanes), dim3(256), lss, stream, Gc, rot, state, anyrot, nlanes, d);
    else if (d <= 128) hipLaunchKernelGGL(svd_sweep_stream32s_kernel<16>, dim3(nlanes), dim3(256), lss, stream, Gc, rot, state, anyrot, nlanes, d);
    else hipLaunchKernelGGL(svd_sweep_stream32s_kernel<25>, dim3(nlanes), dim3(256), lss, stream, Gc, rot, state, anyrot, nlanes, d);
    return true;
}
#define MCX_VARIANT_SVD_SWEEP(stream, Gc, rot, state, anyrot, nlanes, d, lss) variant_svd_sweep((stream), (Gc), (rot), (state), (anyrot), (nlanes), (d), (lss))
static bool variant_cov(mcmcx_engine *h, unsigned g8, int n10, int noff, int it, int mode)
{
    if (variant_env("MCMCX_COV_FIFO") != 1) return false;
    hipLaunchKernelGGL(adapt_cov_diag_fifo_kernel, dim3(g8 * n10), dim3(64), (size_t)CQ * (1 + TD) * 64 * sizeof(double), h->stream, h->E, it, mode, n10);
    if (noff > 0) hipLaunchKernelGGL(adapt_cov_off_fifo_kernel, dim3(g8 * noff), dim3(64), (size_t)CQ * (1 + 2 * TD) * 64 * sizeof(double), h->stream, h->E, it, mode, noff);
    return true;
}
#define MCX_VARIANT_COV(h, g8, n10, noff, it, mode) variant_cov((h), (g8), (n10), (noff), (it), (mode))
