// mcx_diag_xf.hpp -- the convergence summary of an elementwise function of the stored values (mcmcx_samples_stats_of; no counterpart in the
// single-chain reference): tail ESS, folded split-R-hat, the MCSE of the sd and the ESS at a quantile are mcmcx_samples_stats of
//     kind 1, LE      u_f(x) = 1.0 if key(x) <= key(a_f), else +0.0      (quant_key's order: NaNs take part, -0.0 lies below +0.0)
//     kind 2, FOLD    u_f(x) = fabs(x - a_f)                             (one subtraction, then the sign cleared)
//     kind 3, SQUARE  u_f(x) = d * d with d = x - a_f                    (two operations, no contraction)
// with everything after u the summary's own definition (include/mcmcx.h).  u is a compile-time functor at the two
// places a value leaves its load -- the mean pass here and diag_block (mcx_diag.hpp) -- and a_f is read once per wave, beside the shift.
// Kind 0 is diag_tile_kernel<W> itself and has no kernel here.  Included after mcx_quant.hpp, which owns the key map.
//
// diag_xf_tile_kernel restates diag_tile_kernel's body instead of sharing it, and that was measured (profiles/r20_a/summary_body_ab.txt):
// with one body, the argument block by const reference and u a functor, all twenty tile kernels keep their registers and waves (two of
// W = 33 lose two VGPRs) and their instruction counts within 32, but the schedules differ, and over a whole ring at W = 33 the identity
// is slower in all six cells measured, by 0.4 - 1.2 % (70.3 -> 71.1 ms on the headline's shape), and kind 1 by 0.5 % (79.9 -> 80.3 ms);
// the restated kernels' own two runs differ by 0.1 - 1.0 % there.  Both are held to the same restatement, bit for bit, by the tests; a
// change to one body belongs in the other.
#pragma once
#include "mcx_quant.hpp"

namespace mcx {

constexpr int XF_IDENTITY = 0, XF_LE = 1, XF_FOLD = 2, XF_SQUARE = 3;       // = MCMCX_XF_*

template <int KIND> struct Xf;
// key(x) <= key(a) without forming x's key (six vector operations a value; this is three).  With b the bits and m = 0x7FF..F if a's sign
// bit is set, else 0:  (b_x ^ m) <= (b_a ^ m) as SIGNED integers.  a's sign clear: an x with its sign set is negative here and lies
// below a in the key order too, the others compare by their bits as their keys do.  Set: an x with its sign clear stays non-negative,
// above a; among those with it set the lower 63 bits are inverted, as in their keys.  Held to quant_key's order by the tests.
template <> struct Xf<XF_LE> {
    long long m, ta;
    MCX_DEV Xf(double a) : m(__double_as_longlong(a) < 0 ? 0x7FFFFFFFFFFFFFFFll : 0ll), ta(__double_as_longlong(a) ^ m) {}
    MCX_DEV double operator()(double x) const { return (__double_as_longlong(x) ^ m) <= ta ? 1.0 : 0.0; }
};
template <> struct Xf<XF_FOLD> {
    double a;
    MCX_DEV Xf(double a_) : a(a_) {}
    MCX_DEV double operator()(double x) const { return fabs(x - a); }
};
template <> struct Xf<XF_SQUARE> {
    double a;
    MCX_DEV Xf(double a_) : a(a_) {}
    MCX_DEV double operator()(double x) const { const double d = x - a; return d * d; }
};

// Waves per SIMD diag_tile_kernel<W> reaches (8, 4, 3, 2 at W = 1, 9, 17, 33), asked of the transformed forms too: left alone the
// scheduler takes W = 9 with the square to 144 registers, three waves, and that pass reads 1.10 x the identity where it is bound by its
// loads.
constexpr int diag_xf_waves(int W) { return W == 1 ? 8 : W == 9 ? 4 : W == 17 ? 3 : 2; }

// diag_tile_kernel<W> of u_f(x): the same grid, the same argument block, a[nfields] behind it
template <int W, int KIND>
__global__ __launch_bounds__(256, diag_xf_waves(W)) void diag_xf_tile_kernel(DiagArgs A, const double *xa)
{
    constexpr int B = W < DIAG_LB ? DIAG_LB : W;
    static_assert(B % W == 0, "the block is whole turns of the window");
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const size_t tile = blockIdx.x;
    const int f = (int)blockIdx.y * 4 + wave;
    if (f >= A.nfields) return;                                 // the whole wave
    const double sh = A.shift[f];
    const Xf<KIND> xf(xa[f]);
    double ms = -0.0, m2 = -0.0, g[W];                          // -0.0 + x is x: the sums start with their first term
#pragma unroll
    for (int t = 0; t < W; ++t) g[t] = -0.0;
#pragma clang loop unroll(disable)
    for (int h = 0; h < 2; ++h) {
        int n = A.nh;                                           // opaque per half (mcx_diag.hpp says why)
        asm volatile("" : "+s"(n));
        const int w0 = h ? A.ns - n : 0;
        auto row = [&](int i) {
            return A.store + samples_row(samples_slot(A.slot0, w0 + i, A.cap), (size_t)A.ntiles, (size_t)A.nfields, tile, (size_t)f) + lane;
        };
        double s = -0.0;
        for (int j0 = 0; j0 < n; j0 += DIAG_LB) {
            double v[DIAG_LB];
#pragma unroll
            for (int q = 0; q < DIAG_LB; ++q) v[q] = *row(min(j0 + q, n - 1));
#pragma unroll
            for (int q = 0; q < DIAG_LB; ++q) if (j0 + q < n) s = s + (xf(v[q]) - sh);
        }
        const double m = s / (double)n;
        double z[W], a[W];
#pragma unroll
        for (int t = 0; t < W; ++t) { z[t] = 0.0; a[t] = 0.0; }
        diag_block<W, B, true>(row, 0, n, sh, m, z, a, xf);
        for (int j0 = B; j0 < n; j0 += B) diag_block<W, B, false>(row, j0, n, sh, m, z, a, xf);
        ms = ms + m; m2 = m2 + m * m;
#pragma unroll
        for (int t = 0; t < W; ++t) g[t] = g[t] + a[t];
    }
    const bool act = tile * 64 + (size_t)lane < (size_t)A.nchains;             // the tile's 64 chains: masked, then the xor-butterfly
    auto tile_sum = [&](double x) {
        x = act ? x : 0.0;
#pragma unroll
        for (int k = 1; k < 64; k <<= 1) x = x + __shfl_xor(x, k);
        return x;
    };
    double o = 0.0;                                             // lane j writes term j; lags beyond K stay +0.0
    { const double r = tile_sum(ms); if (lane == 0) o = r; }
    { const double r = tile_sum(m2); if (lane == 1) o = r; }
#pragma unroll
    for (int t = 0; t < W; ++t) {
        const double r = tile_sum(g[t]);
        if (lane == 2 + t && t <= A.K) o = r;
    }
    const int len = A.maxlag + 3;
    if (lane < len) A.out[(tile * (size_t)A.nfields + (size_t)f) * (size_t)len + (size_t)lane] = o;
}

// shift == NULL: u_f of field f of chain 0 (tile 0, lane 0) in window sample 0
template <int KIND>
__global__ void diag_xf_shift_kernel(const double *store, const double *a, double *shift, size_t slot, int ntiles, int nfields)
{
    const int f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f < nfields) shift[f] = Xf<KIND>(a[f])(store[samples_row(slot, (size_t)ntiles, (size_t)nfields, 0, (size_t)f)]);
}

} // namespace mcx
