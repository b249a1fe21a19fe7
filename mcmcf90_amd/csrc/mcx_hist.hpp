// mcx_hist.hpp -- marginal and pairwise joint histograms of the thinned sample store (mcmcx_samples_hist / _hist2; no counterpart in the
// single-chain reference): what a user plots first, the density of every field and of pairs of fields, counted where the ring lies.
// None of these is a sampling kernel: they draw nothing, write nothing but the caller's table, and are no entry of the kernel-selection
// tables.
//
// The definition (include/mcmcx.h has it in full).  Everything is in the key order of mcx_quant.hpp (quant_key):
// the IEEE order on doubles that are no NaN, -0.0 below +0.0, negative NaNs below everything and positive NaNs above.  A field has
// nbins + 1 edges, non-decreasing by key;
//     cell_f(x) = the number of edges e_i of field f with key(e_i) <= key(x)            (0 .. nbins + 1)
// so cell 0 lies below e_0, cell b is e_{b-1} <= x < e_b, and cell nbins + 1 is at or above the last edge.  The 1-D table counts the
// window's values of a field per cell, the 2-D table the window's (sample, chain) points per pair of cells of two fields.  Every count
// is an integer: no order of summation, no tolerance.
//
// Both kernels stream the window in whole 512-byte rows (a lane per chain, a loop over the window's slots, every offset through
// samples_row in size_t), search the field's edge keys staged in LDS, count in 32-bit LDS counters and flush the non-zero ones to the
// zeroed table of 64-bit counts with integer atomics.  The host bounds what one block counts below 2**31 (a wave never more than 128
// tiles, a block never more than QuantWin::chunk <= 32 768 window samples of them), so an LDS counter cannot wrap whatever n is.
#pragma once
#include "mcx_quant.hpp"

namespace mcx {

constexpr int HIST_MAXBINS = 1024;  // = MCMCX_HIST_MAXBINS
constexpr int HIST2_MAXBINS = 96;   // = MCMCX_HIST2_MAXBINS: 98 x 98 counters and two edge rows are 40 KB of LDS
constexpr int HIST2_MAXPAIRS = 64;  // = MCMCX_HIST2_MAXPAIRS
constexpr int HIST_LB = 8;          // rows a wave has in flight (the 2-D kernel: HIST_LB / 2 of either field)

struct HistPairs { int j[HIST2_MAXPAIRS], k[HIST2_MAXPAIRS]; }; // a launch argument: staged by the launch itself

// The cell of a key: how many of the ne edge keys ek[0 .. ne - 1] (ascending, in LDS) are <= key.  "t edges are <= key" is true up to
// the cell and false above it, so the descent over the powers of two from `top` (the largest one <= ne) adds every step that keeps it
// true: floor(log2(ne)) + 1 LDS reads for every lane, no branch that depends on the value.
MCX_DEV int hist_cell(const unsigned long long *ek, int ne, int top, unsigned long long key)
{
    int pos = 0;
    for (int step = top; step > 0; step >>= 1) {
        const int t = pos + step;
        const unsigned long long e = ek[min(t, ne) - 1];
        if (t <= ne && e <= key) pos = t;
    }
    return pos;
}

// out[nfields][nbins + 2], zeroed before the launch; ekey[nfields][nbins + 1] the edges' keys.
// grid (gx, nfields, gz), 256 threads, dynamic LDS: nbins + 1 keys of 64 bits, then nbins + 2 counters of 32 bits.  The block's four
// waves take tiles 4 bx + w, + 4 gx, ..; blockIdx.z takes window samples z chunk .. (z + 1) chunk - 1.  One LDS atomic per value: the
// values of a field that has converged spread over the bins, so the lanes of a wave mostly hit different counters.
// hist_kernel's LDS: ek [nbins + 1] keys of 64 bits | cnt [nbins + 2] counters of 32 bits; hist2_kernel's (pair = true): ekj [nbins + 1] |
// ekk [nbins + 1] | cnt [(nbins + 2)**2].  Offsets in words of 64 bits
struct HistLds {
    int ekk, cnt;                                                   // (ek / ekj at 0)
    size_t bytes;
    MCX_HD HistLds(int nbins, bool pair) : ekk(pair ? nbins + 1 : 0), cnt(pair ? 2 * (nbins + 1) : nbins + 1),
        bytes((size_t)cnt * sizeof(unsigned long long) + (size_t)(nbins + 2) * (size_t)(pair ? nbins + 2 : 1) * sizeof(unsigned int)) {}
};
__global__ __launch_bounds__(256) void hist_kernel(QuantWin A, const unsigned long long *__restrict__ ekey, unsigned long long *out,
    int nbins, int top)
{
    extern __shared__ unsigned long long hist_lds[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, ne = nbins + 1, nc = nbins + 2;
    const int f = blockIdx.y;
    // HistLds(nbins, false), spelled out (taking the offset from it moves this kernel's instructions)
    unsigned long long *ek = hist_lds;
    unsigned int *cnt = (unsigned int *)(hist_lds + ne);
    for (int i = threadIdx.x; i < ne; i += 256) ek[i] = ekey[(size_t)f * (size_t)ne + (size_t)i];
    for (int i = threadIdx.x; i < nc; i += 256) cnt[i] = 0u;
    __syncthreads();
    const int w0 = (int)blockIdx.z * A.chunk, w1 = min(A.win.ns, w0 + A.chunk);
    for (size_t tile = (size_t)blockIdx.x * 4 + wave; tile < (size_t)A.win.ntiles; tile += (size_t)gridDim.x * 4) {
        const bool act = tile * 64 + (size_t)lane < (size_t)A.win.nchains;      // the store's padding rows hold no defined values
        for (int j0 = w0; j0 < w1; j0 += HIST_LB) {
            double v[HIST_LB];
#pragma unroll
            for (int q = 0; q < HIST_LB; ++q)
                v[q] = A.win.store[samples_row(samples_slot(A.win.slot0, min(j0 + q, w1 - 1), A.win.cap), (size_t)A.win.ntiles,
                                               (size_t)A.win.nfields, tile, (size_t)f) + lane];
#pragma unroll
            for (int q = 0; q < HIST_LB; ++q) {
                if (j0 + q >= w1) break;                        // the whole wave
                const int cell = hist_cell(ek, ne, top, quant_key((unsigned long long)__double_as_longlong(v[q])));
                if (act) atomicAdd(&cnt[cell], 1u);
            }
        }
    }
    __syncthreads();
    unsigned long long *table = out + (size_t)f * (size_t)nc;
    for (int i = threadIdx.x; i < nc; i += 256) {
        const unsigned int c = cnt[i];
        if (c) atomicAdd(&table[i], (unsigned long long)c);     // integer adds commute: no arrival order in the result
    }
}

// out[npairs][nbins + 2][nbins + 2], zeroed before the launch: pair blockIdx.y = (fields P.j, P.k) counts the window's points with
// cell_j(x_j) = a and cell_k(x_k) = b at [a][b].  grid (gx, npairs, gz), 256 threads, dynamic LDS: two rows of nbins + 1 keys, then
// (nbins + 2)**2 counters of 32 bits.  Tiles and window samples as in hist_kernel; both fields' rows of a tile and slot are read
// together, the same row twice where j == k.
__global__ __launch_bounds__(256) void hist2_kernel(QuantWin A, const unsigned long long *__restrict__ ekey, HistPairs P,
    unsigned long long *out, int nbins, int top)
{
    extern __shared__ unsigned long long hist_lds[];
    constexpr int LB = HIST_LB / 2;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, ne = nbins + 1, nc = nbins + 2;
    const int fj = P.j[blockIdx.y], fk = P.k[blockIdx.y];
    const HistLds lds(nbins, true);
    unsigned long long *ekj = hist_lds, *ekk = hist_lds + lds.ekk;
    unsigned int *cnt = (unsigned int *)(hist_lds + lds.cnt);
    for (int i = threadIdx.x; i < ne; i += 256) {
        ekj[i] = ekey[(size_t)fj * (size_t)ne + (size_t)i];
        ekk[i] = ekey[(size_t)fk * (size_t)ne + (size_t)i];
    }
    for (int i = threadIdx.x; i < nc * nc; i += 256) cnt[i] = 0u;
    __syncthreads();
    const int w0 = (int)blockIdx.z * A.chunk, w1 = min(A.win.ns, w0 + A.chunk);
    for (size_t tile = (size_t)blockIdx.x * 4 + wave; tile < (size_t)A.win.ntiles; tile += (size_t)gridDim.x * 4) {
        const bool act = tile * 64 + (size_t)lane < (size_t)A.win.nchains;
        for (int j0 = w0; j0 < w1; j0 += LB) {
            double vj[LB], vk[LB];
#pragma unroll
            for (int q = 0; q < LB; ++q) {
                const size_t slot = samples_slot(A.win.slot0, min(j0 + q, w1 - 1), A.win.cap);
                vj[q] = A.win.store[samples_row(slot, (size_t)A.win.ntiles, (size_t)A.win.nfields, tile, (size_t)fj) + lane];
                vk[q] = A.win.store[samples_row(slot, (size_t)A.win.ntiles, (size_t)A.win.nfields, tile, (size_t)fk) + lane];
            }
#pragma unroll
            for (int q = 0; q < LB; ++q) {
                if (j0 + q >= w1) break;                        // the whole wave
                const int a = hist_cell(ekj, ne, top, quant_key((unsigned long long)__double_as_longlong(vj[q])));
                const int b = hist_cell(ekk, ne, top, quant_key((unsigned long long)__double_as_longlong(vk[q])));
                if (act) atomicAdd(&cnt[a * nc + b], 1u);
            }
        }
    }
    __syncthreads();
    unsigned long long *table = out + (size_t)blockIdx.y * (size_t)(nc * nc);
    for (int i = threadIdx.x; i < nc * nc; i += 256) {
        const unsigned int c = cnt[i];
        if (c) atomicAdd(&table[i], (unsigned long long)c);
    }
}

} // namespace mcx
