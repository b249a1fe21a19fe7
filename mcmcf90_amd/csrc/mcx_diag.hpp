// mcx_diag.hpp -- the convergence summary of the thinned sample store (mcmcx_samples_stats; no counterpart in the single-chain reference):
// diag_tile_kernel reduces a window of the ring where it lies to one row of sums per tile, moments_tree_kernel (mcx_moments.hpp, as it is)
// finishes them over the tiles, diag_pack_kernel lays the stats vector out.  None of them is a sampling kernel: they draw nothing, write
// nothing but their scratch and the caller's vector, and are no entry of the kernel-selection tables.
//
// The definition (include/mcmcx.h has it in full).  Window samples 0 .. ns - 1, n_h = ns / 2, half 0 = samples
// 0 .. n_h - 1, half 1 = samples ns - n_h .. ns - 1, K = min(maxlag, n_h - 1).  Per chain, half and field, in plain IEEE doubles:
//     y_i = x_i - shift_f,  s = (..((y_0 + y_1) + y_2) ..),  m = s / n_h,  z_i = y_i - m,
//     g_t = sum over i = 0 .. n_h - 1 - t, ascending, of z_i z_{i+t}     (a = a + z_i * z_{i+t} from +0.0),  t = 0 .. K
// and the chain's terms per field are  m_0 + m_1,  m_0 m_0 + m_1 m_1,  g0_t + g1_t (t = 0 .. K).  Over the chains they are summed like the
// pooled moments: the 64 lanes of a tile in the adjacent-pairs tree (tree64's order, here an xor-butterfly), a lane without a chain
// contributing +0.0 (masked: the store's padding rows hold no defined values), the tiles in moments_tree_kernel's fixed pairwise tree.
//
// Shape: a lane per chain, a wave per field row, a loop over the window's slots; every load is one 512-byte row of the store, every
// offset goes through samples_row in size_t.  Two passes over a half: the mean first, then the centred products.  The last W centred values
// and the W lag sums live in registers with compile-time indices -- a rotating window, the loop over the samples unrolled by its length
// W; a dynamically indexed window would live in scratch.  Each lag's sum is a sequence of its own, so every instantiation (W = 1, 9, 17,
// 33, chosen by K on the host) gives the same bits for the lags it shares with another.
#pragma once
#include "mcx_samples.hpp"

namespace mcx {

constexpr int DIAG_MAXLAG = 32;     // = MCMCX_DIAG_MAXLAG
constexpr int DIAG_LB = 8;          // rows a wave has in flight

// The window's members (a SampleWin's, mcx_samples.hpp) stand here one by one, filled from one by diag_launch on the host: with the window
// as ONE member the argument block is laid out and loaded differently, and diag_tile_kernel<W> compiles to other scalar code (six
// instructions fewer, two scalar registers more at W = 33) -- the kernel is the definition's bits and stays the instructions it was
struct DiagArgs {
    const double *store; const double *shift; double *out;      // the ring; shift[nfields]; out[ntiles][nfields][maxlag + 3]
    size_t slot0, cap;                                          // ring slot of window sample 0, the ring's capacity
    int ntiles, nfields, nchains, ns, nh, K, maxlag;
};

// Samples j0 .. j0 + B - 1 of a half (those below n): z_j = (x_j - shift) - m enters the window at j % W and every lag sum takes its
// product, a_t = a_t + z_{j-t} z_j -- g_t's terms in g_t's order (i = j - t ascending; the product commutes).  HEAD: the half's first
// block, where lag t has no partner yet for j < t (decided at compile time: j = u there).  Rows are loaded DIAG_LB at a time, past the
// half's end the last one again (a valid row, not used).  xf: the elementwise function a value passes where it leaves its load -- the
// summary's own is the identity, the transformed summaries' (mcx_diag_xf.hpp) are compile-time functors too.
struct XfIdentity { MCX_DEV double operator()(double x) const { return x; } };
template <int W, int B, bool HEAD, class Row, class U = XfIdentity>
MCX_DEV void diag_block(Row &&row, int j0, int n, double sh, double m, double (&z)[W], double (&a)[W], const U &xf = U())
{
#pragma unroll
    for (int u0 = 0; u0 < B; u0 += DIAG_LB) {
        double v[DIAG_LB];
#pragma unroll
        for (int q = 0; q < DIAG_LB; ++q)
            if (u0 + q < B) v[q] = *row(min(j0 + u0 + q, n - 1));
#pragma unroll
        for (int q = 0; q < DIAG_LB; ++q) {
            const int u = u0 + q;
            if (u < B && j0 + u < n) {
                const double zn = (xf(v[q]) - sh) - m;
                z[u % W] = zn;
#pragma unroll
                for (int t = 0; t < W; ++t)
                    if (!HEAD || t <= u) a[t] = a[t] + z[((u - t) % W + W) % W] * zn;
            }
        }
    }
}

// grid (ntiles, ceil(nfields / 4)), 256 threads: wave w of block (t, b) reduces field 4 b + w of tile t.  No barrier, no LDS.
template <int W>
__global__ __launch_bounds__(256) void diag_tile_kernel(DiagArgs A)
{
    constexpr int B = W < DIAG_LB ? DIAG_LB : W;                // samples per unrolled block: a multiple of W
    static_assert(B % W == 0, "the block is whole turns of the window");
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const size_t tile = blockIdx.x;
    const int f = (int)blockIdx.y * 4 + wave;
    if (f >= A.nfields) return;                                 // the whole wave
    const double sh = A.shift[f];
    // -0.0 + x is x for every x (the sign of a zero included): the sums below start with their first term, as the definition's do
    double ms = -0.0, m2 = -0.0, g[W];
#pragma unroll
    for (int t = 0; t < W; ++t) g[t] = -0.0;
#pragma clang loop unroll(disable)
    for (int h = 0; h < 2; ++h) {
        // n_h, made opaque per half: as a loop invariant the head block's W comparisons with it and W clamped indices are all formed
        // before the loop and kept in scalar registers across it, more than there are (43 spilled at W = 33)
        int n = A.nh;
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
            for (int q = 0; q < DIAG_LB; ++q) if (j0 + q < n) s = s + (v[q] - sh);
        }
        const double m = s / (double)n;
        double z[W], a[W];
#pragma unroll
        for (int t = 0; t < W; ++t) { z[t] = 0.0; a[t] = 0.0; }
        diag_block<W, B, true>(row, 0, n, sh, m, z, a);
        for (int j0 = B; j0 < n; j0 += B) diag_block<W, B, false>(row, j0, n, sh, m, z, a);
        ms = ms + m; m2 = m2 + m * m;
#pragma unroll
        for (int t = 0; t < W; ++t) g[t] = g[t] + a[t];
    }
    // the tile's 64 chains: masked, then the xor-butterfly (lane l takes v_l + v_{l^1}, then (..) + (..)_{l^2}, ...: tree64's additions;
    // every lane ends with the sum lane 0 has)
    const bool act = tile * 64 + (size_t)lane < (size_t)A.nchains;
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

// shift == NULL: field f of chain 0 (tile 0, lane 0) in window sample 0
__global__ void diag_shift_kernel(const double *store, double *shift, size_t slot, int ntiles, int nfields)
{
    const int f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f < nfields) shift[f] = store[samples_row(slot, (size_t)ntiles, (size_t)nfields, 0, (size_t)f)];
}

// [M, n_h, K, then per field: shift, S1, S2, G_0 .. G_maxlag] from the tree's result v[nfields][maxlag + 3] (copies, no arithmetic)
__global__ void diag_pack_kernel(const double *v, const double *shift, double *out, int nfields, int maxlag, double M, double nh, double K)
{
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= 3 + nfields * (maxlag + 4)) return;
    if (k < 3) { out[k] = k == 0 ? M : k == 1 ? nh : K; return; }
    const int f = (k - 3) / (maxlag + 4), j = (k - 3) % (maxlag + 4);
    out[k] = j == 0 ? shift[f] : v[(size_t)f * (maxlag + 3) + (j - 1)];
}

} // namespace mcx
