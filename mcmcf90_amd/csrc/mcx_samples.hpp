// mcx_samples.hpp -- the thinned sample store (mcmcx_set_samples; no counterpart in the single-chain reference): samples_keep_kernel copies
// the state of ALL chains into one slot of a ring between two launches of the sampling kernels, samples_read_rows_kernel /
// samples_read_chains_kernel map a window of the ring to the caller's layout.  None of them is a sampling kernel: they draw nothing, move
// no state and are no entry of the kernel-selection tables.
//
// One slot holds every chain in the state's own tile-interleaved layout, [tile][field][64], the fields of a chain being
//     theta[npar], ss[nycol], sspri, sigma2[nycol]            (nfields = npar + 2 nycol + 1)
// so that keeping a sample is whole 512-byte rows copied from E.theta and from the scalar state: with one response column the rows S_SS1,
// S_PRI1, S_SIGMA2 of E.scal (every kernel form writes its lane state back there at a launch's end), with nycol > 1 the per-column vectors
// E.ssv / E.s2v the phase kernels keep current (E.scal holds column 1 only) and S_PRI1.  Lanes beyond nchains in the last tile copy the
// padding.  Every offset into the store goes through samples_row, in size_t: capacity x ntiles x nfields x 64 passes 2**31 at real sizes.
#pragma once
#include "mcx_common.hpp"

namespace mcx {

// element offset of row `field` of tile `tile` in slot `slot` of a store of [slot][ntiles][nfields][64] doubles (compiled for the host too:
// mcmcx_debug_samples_offset lets a test check the arithmetic beyond 2**32 without a store of that size)
__host__ MCX_DEV size_t samples_row(size_t slot, size_t ntiles, size_t nfields, size_t tile, size_t field)
{
    return ((slot * ntiles + tile) * nfields + field) * 64;
}

// A window of the ring as a launch argument of the store's readers (mcx_diag.hpp, mcx_quant.hpp, mcx_cov.hpp): window samples 0 .. ns - 1
// of all chains, window sample w in ring slot samples_slot(slot0, w, cap).  The host makes it in ONE place (samples_window).  QuantWin
// holds one; DiagArgs and CovArgs hold its members one by one (mcx_diag.hpp says why).
struct SampleWin {
    const double *store;                                        // [slot][ntiles][nfields][64]
    size_t slot0, cap;                                          // ring slot of window sample 0, the ring's capacity
    int ntiles, nfields, nchains, ns;
};

// ring slot of window sample w: (slot0 + w) % cap as in samples_read, for slot0 < cap and w < cap (a window is never longer than the ring)
// -- without the 64-bit division the % would cost every row
MCX_DEV size_t samples_slot(size_t slot0, int w, size_t cap)
{
    const size_t q = slot0 + (size_t)w;
    return q >= cap ? q - cap : q;
}

// where field f of a tile's chains lives in the engine's state (a 64-double row)
MCX_DEV const double *samples_src(const EngineDev &E, size_t tile, int f)
{
    const int d = E.d, ny = E.ny;
    if (f < d) return E.theta + (tile * (size_t)d + (size_t)f) * 64;
    f -= d;
    if (ny == 1) return E.scal + (tile * NSCAL + (size_t)(f == 0 ? S_SS1 : f == 1 ? S_PRI1 : S_SIGMA2)) * 64;
    if (f < ny) return E.ssv + (tile * (size_t)ny + (size_t)f) * 64;
    if (f == ny) return E.scal + (tile * NSCAL + S_PRI1) * 64;
    return E.s2v + (tile * (size_t)ny + (size_t)(f - ny - 1)) * 64;
}

constexpr int SAMP_KR = 4;      // rows a wave has in flight
constexpr int SAMP_FB = 64;     // fields per LDS tile of the transposing read (a chain's run of the output: 512 bytes)

// grid (ntiles, ceil(nfields / (4 SAMP_KR))), 256 threads: wave w of block (t, b) copies rows (4 b + w) SAMP_KR .. + SAMP_KR - 1 of tile t
__global__ __launch_bounds__(256) void samples_keep_kernel(EngineDev E, double *store, size_t slot, int nfields)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const size_t tile = blockIdx.x;
    const int f0 = ((int)blockIdx.y * 4 + wave) * SAMP_KR;
    double v[SAMP_KR];
#pragma unroll
    for (int u = 0; u < SAMP_KR; ++u) if (f0 + u < nfields) v[u] = samples_src(E, tile, f0 + u)[lane];
#pragma unroll
    for (int u = 0; u < SAMP_KR; ++u)
        if (f0 + u < nfields) store[samples_row(slot, (size_t)E.ntiles, (size_t)nfields, tile, (size_t)(f0 + u)) + lane] = v[u];
}

// layout 1, out[ns][nfields][nc]: retained sample s of the window is ring slot (slot0 + s) % cap; rows of the store go out as rows of
// the output, the first and the last tile of the chain window partially (c0 need not be a multiple of 64).
// grid (tiles of the window, ceil(nfields / (4 SAMP_KR)), min(ns, 65535)), 256 threads
__global__ __launch_bounds__(256) void samples_read_rows_kernel(const double *store, double *out, size_t slot0, size_t cap, int ntiles,
    int nfields, int ns, int c0, int nc)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const size_t tile = (size_t)(c0 / 64) + blockIdx.x;
    const int f0 = ((int)blockIdx.y * 4 + wave) * SAMP_KR;
    const long long c = (long long)tile * 64 + lane - c0;
    const bool mine = c >= 0 && c < nc;
    for (int s = blockIdx.z; s < ns; s += gridDim.z) {
        const size_t slot = (slot0 + (size_t)s) % cap;
        double v[SAMP_KR];
#pragma unroll
        for (int u = 0; u < SAMP_KR; ++u)
            if (f0 + u < nfields) v[u] = store[samples_row(slot, (size_t)ntiles, (size_t)nfields, tile, (size_t)(f0 + u)) + lane];
#pragma unroll
        for (int u = 0; u < SAMP_KR; ++u)
            if (mine && f0 + u < nfields) out[((size_t)s * (size_t)nfields + (size_t)(f0 + u)) * (size_t)nc + (size_t)c] = v[u];
    }
}

// layout 0, out[ns][nc][nfields]: a 64-chain x SAMP_FB-field transpose through LDS, so that the store is read in whole rows and the
// output written in runs of up to SAMP_FB consecutive fields of one chain.  The LDS tile's rows are padded by one double: the column
// read T[lane][chain] (ds_read_b64, stride 65 doubles = 130 banks) puts the 32 lanes of a half wave on 32 different bank pairs.
// A loop over field blocks keeps the tile at 33 KiB whatever nfields is.  grid (tiles of the window, min(ns, 65535)), 256 threads
__global__ __launch_bounds__(256) void samples_read_chains_kernel(const double *store, double *out, size_t slot0, size_t cap, int ntiles,
    int nfields, int ns, int c0, int nc)
{
    __shared__ double T[SAMP_FB][65];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const size_t tile = (size_t)(c0 / 64) + blockIdx.x;
    for (int s = blockIdx.y; s < ns; s += gridDim.y) {
        const size_t slot = (slot0 + (size_t)s) % cap;
        for (int fb = 0; fb < nfields; fb += SAMP_FB) {
            __syncthreads();                                    // the previous block's column reads are done
            for (int r0 = wave * (SAMP_FB / 4); r0 < (wave + 1) * (SAMP_FB / 4); r0 += SAMP_KR) {
                double v[SAMP_KR];
#pragma unroll
                for (int u = 0; u < SAMP_KR; ++u)
                    if (fb + r0 + u < nfields)
                        v[u] = store[samples_row(slot, (size_t)ntiles, (size_t)nfields, tile, (size_t)(fb + r0 + u)) + lane];
#pragma unroll
                for (int u = 0; u < SAMP_KR; ++u) if (fb + r0 + u < nfields) T[r0 + u][lane] = v[u];
            }
            __syncthreads();
            const int f = fb + lane;
            for (int cl = wave; cl < 64; cl += 4) {
                const long long c = (long long)tile * 64 + cl - c0;
                if (c >= 0 && c < nc && f < nfields) out[((size_t)s * (size_t)nc + (size_t)c) * (size_t)nfields + (size_t)f] = T[lane][cl];
            }
        }
    }
}

} // namespace mcx
