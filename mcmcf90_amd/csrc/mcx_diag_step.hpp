// mcx_diag_step.hpp -- the convergence summary of a step function of the stored values (mcmcx_samples_stats_step; no counterpart in the
// single-chain reference): rank-normalised split-R-hat and bulk ESS, the ESS of an interval probability and of any binned functional are
// mcmcx_samples_stats of
//     u_f(x) = table_f[cell_f(x)],   cell_f(x) = the number of edges e_i of field f with key(e_i) <= key(x)     (0 .. nbins + 1)
// -- the histograms' cell (mcx_hist.hpp: hist_cell over the field's edge keys, quant_key's order, NaNs take part, -0.0 lies below +0.0)
// and a table of nbins + 2 doubles per field -- with everything after u the summary's own definition (include/mcmcx.h; DESIGN.md
// section 5g).  u is a functor at the two places a value leaves its load, as in mcx_diag_xf.hpp: the mean pass here and diag_block
// (mcx_diag.hpp).  Included after mcx_hist.hpp, which owns the search.
//
// LDS: a block's four waves serve four fields, as in diag_tile_kernel, and each wave stages its own field's nbins + 1 edge keys and
// nbins + 2 table entries, (2 nbins + 3) 64-bit words a field, sized by the launch: 2.0 KB a block at 30 bins, 8.2 KB at 126, 32.7 KB at
// the cap of 510.  The registers allow 8 / 5 / 3 / 2 waves a SIMD at W = 1 / 9 / 17 / 33 (44 / 94 / 140 / 236 VGPRs, no scratch:
// profiles/kernel_resources.txt), that many blocks a compute unit, and its 160 KiB of LDS hold eight blocks up to 318 bins and five,
// three or two up to the cap: the registers bound the occupancy, as in the identity, except at W = 1 above 318 bins (four blocks at the
// cap).  One field a block would quarter the LDS and change nothing below that; the grid stays the identity's.
//
// The kernel restates diag_tile_kernel's body, as diag_xf_tile_kernel does and for the measured reason given there (mcx_diag_xf.hpp;
// profiles/r20_a/summary_body_ab.txt); a change to one body belongs in the others.
#pragma once
#include "mcx_diag.hpp"
#include "mcx_hist.hpp"

namespace mcx {

constexpr int STEP_MAXBINS = 510;   // = MCMCX_STEP_MAXBINS: 512 cells
constexpr int STEP_TOP = 256;       // the largest power of two <= STEP_MAXBINS + 1 edges: the search's first step at every bin count

// u_f of one field: ek[ne] the edge keys, tb[ne + 1] the table, both in LDS (or, for the shift kernel, in device memory).  The search
// starts at STEP_TOP whatever ne is -- a step beyond ne changes nothing (hist_cell) --, so that its nine steps are unrolled into
// straight-line code: with the step count a launch argument every value's search is a loop of its own, and in the unrolled block of
// W = 33 the stores into the window of centred values are then merged across those loops' exits, the window is indexed dynamically and
// lives in scratch.
struct XfStep {
    const unsigned long long *ek;
    const double *tb;
    int ne;
    MCX_DEV double operator()(double x) const
    {
        return tb[hist_cell(ek, ne, STEP_TOP, quant_key((unsigned long long)__double_as_longlong(x)))];
    }
};

// Waves per SIMD diag_tile_kernel<W> reaches (8, 4, 3, 2 at W = 1, 9, 17, 33), asked of the step forms too, as of the transformed ones
constexpr int diag_step_waves(int W) { return W == 1 ? 8 : W == 9 ? 4 : W == 17 ? 3 : 2; }

// diag_tile_kernel<W> of u_f(x): the same grid, the same argument block; ekey[nfields][nbins + 1] and table[nfields][nbins + 2] behind
// it.  Dynamic LDS: 4 (2 nbins + 3) words of 64 bits.  Every wave passes the barrier before one without a field leaves.
// Its LDS, per wave (four of them): ek [nbins + 1] keys | tb [nbins + 2] table values, words of 64 bits all
struct DiagStepLds {
    int tb;                                                         // behind the wave's ek; in words
    size_t wave, bytes;                                             // a wave's stride
    MCX_HD explicit DiagStepLds(int nbins) : tb(nbins + 1), wave((size_t)(tb + (nbins + 2))),
        bytes(4 * wave * sizeof(unsigned long long)) {}
};
template <int W>
__global__ __launch_bounds__(256, diag_step_waves(W)) void diag_step_tile_kernel(DiagArgs A, const unsigned long long *__restrict__ ekey,
    const double *__restrict__ table, int nbins)
{
    extern __shared__ unsigned long long step_lds[];
    constexpr int B = W < DIAG_LB ? DIAG_LB : W;
    static_assert(B % W == 0, "the block is whole turns of the window");
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, ne = nbins + 1, nc = nbins + 2;
    const size_t tile = blockIdx.x;
    const int f = (int)blockIdx.y * 4 + wave;
    // DiagStepLds, spelled out (taking the offsets from it moves an instruction of every instance)
    unsigned long long *ek = step_lds + (size_t)wave * (size_t)(ne + nc);
    double *tb = (double *)(ek + ne);
    if (f < A.nfields) {
        for (int i = lane; i < ne; i += 64) ek[i] = ekey[(size_t)f * (size_t)ne + (size_t)i];
        for (int i = lane; i < nc; i += 64) tb[i] = table[(size_t)f * (size_t)nc + (size_t)i];
    }
    __syncthreads();
    if (f >= A.nfields) return;                                 // the whole wave
    const double sh = A.shift[f];
    const XfStep xf = {ek, tb, ne};
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

// shift == NULL: u_f of field f of chain 0 (tile 0, lane 0) in window sample 0, the keys and the table read where they were staged
__global__ void diag_step_shift_kernel(const double *store, const unsigned long long *ekey, const double *table, double *shift, size_t slot,
    int ntiles, int nfields, int nbins)
{
    const int f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= nfields) return;
    const XfStep xf = {ekey + (size_t)f * (size_t)(nbins + 1), table + (size_t)f * (size_t)(nbins + 2), nbins + 1};
    shift[f] = xf(store[samples_row(slot, (size_t)ntiles, (size_t)nfields, 0, (size_t)f)]);
}

} // namespace mcx
