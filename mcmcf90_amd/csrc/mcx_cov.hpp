// mcx_cov.hpp -- the posterior covariance of the thinned sample store on the f64 matrix cores (mcmcx_samples_cov; no counterpart in the
// single-chain reference): cov_tile_kernel reduces a window of the ring where it lies to one row of sums per tile -- S_j and the upper
// triangle of G_jk --, moments_tree_kernel (mcx_moments.hpp, as it is) finishes them over the tiles, diag_shift_kernel (mcx_diag.hpp, as it
// is) takes the default shift, cov_pack_kernel lays the vector out.  None of them is a sampling kernel: they draw nothing, write nothing
// but their scratch and the caller's vector, and are no entry of the kernel-selection tables.
//
// The definition (include/mcmcx.h has it in full).  z_f = x_f - shift_f; per tile, over the window's samples w
// ascending and within a sample the tile's lanes c = 0 .. 63 ascending, a lane without a chain selected to +0.0:
//     s_j  = s_j + z_j[w][c]                     from +0.0
//     g_jk = fma(z_j[w][c], z_k[w][c], g_jk)     from +0.0,  j <= k
// That is the rank-(64 ns) update Z Z' with the chains on the k axis of v_mfma_f64_16x16x4_f64: the instruction makes four fma into C in
// ascending k = lane >> 4 (mfma_wave_product relies on the same), so sixteen of them per slot, chain group m = 0 .. 15 holding chains
// 4 m + k, are the chain above.  s_j is the same chain against a row of ones (fma(z, 1.0, a) = a + z): row `nfields` of the staged
// matrix, so the sums come out of the matrix cores with the products.
//
// Shape: one wave per workgroup and tile.  Per slot the wave loads its rows (whole 512-byte rows of the store through samples_row, all of
// them in flight at once), subtracts the shift and masks the padding lanes ONCE while staging them into LDS as Z[row][COV_LD]; then lane l
// reads, per 16-row block b and chain group m, the one operand Z[16 b + (l & 15)][4 m + (l >> 4)] -- it is the A operand of block row b
// and the B operand of block column b -- and issues one MFMA per block pair.  The accumulators (one mcx_d4 per block pair and lane) stay
// in registers across the whole window; the next slot's rows are loaded before the current slot's MFMAs issue and wait in registers.
// COV_LD = 65: the compiler pairs the operand reads of chain groups m and m + 1 into ds_read2_b64, which serves sixteen lanes -- one k,
// rows 0 .. 15 -- per LDS cycle and banks them by (dword address) mod 32: the rows fall on dwords 130 row + const = 2 row mod 32, all
// different, so the read has no bank conflict (checked in the disassembly: every operand read of every instantiation is a ds_read2_b64; an
// even stride would put rows r and r + 8 on one bank).  The staging write is 64 consecutive doubles.
//
// Form A (cov_tile_kernel<NS, false>, NS = 1 .. 4, nfields + 1 <= 16 NS): blocks 0 .. NS - 1, the upper block triangle, NS (NS + 1) / 2
// accumulators -- ten at the headline's 53 fields.  Form B (any nfields): the blocks in super-blocks of two; grid.y of
// cov_tile_kernel<2, false> takes the diagonal super-blocks (three accumulators), grid.y of cov_tile_kernel<4, true> the pairs I < J of
// super-blocks (blocks 2 I, 2 I + 1 against 2 J, 2 J + 1: four accumulators), each workgroup reading the rows of its two field ranges
// again.  The chain of a pair (j, k) is the same instructions in the same order whichever form and workgroup holds it.
#pragma once
#include "mcx_diag.hpp"

namespace mcx {

constexpr int COV_LD = 65;          // doubles per staged row: 64 chains + 1 of padding

// the window's members one by one, like DiagArgs and for its reason: with a SampleWin as one member every cov_tile_kernel instantiation
// loads its arguments in other groups and allocates other scalar registers
struct CovArgs {
    const double *store; const double *shift; double *out;      // the ring; shift[nfields]; out[ntiles][nf + nf (nf + 1) / 2]
    size_t slot0, cap;                                          // ring slot of window sample 0, the ring's capacity
    int ntiles, nfields, nchains, ns;
};

// where pair j <= k lies in the packed upper triangle (rows of the triangle one after the other: mcmcx_pooled_moments' order)
__host__ MCX_DEV size_t cov_pair(size_t j, size_t k, size_t nfields) { return j * nfields - j * (j - 1) / 2 + (k - j); }

// staged block s of the workgroup is block cov_block(s) of the rows 0 .. nfields (fields, then the row of ones)
template <int NS, bool OFF>
MCX_DEV int cov_block(int s, int y)
{
    if (!OFF) return NS * y + s;
    // y counts the pairs I < J of super-blocks by columns: (0,1), (0,2), (1,2), (0,3), ..
    int J = (int)((sqrt(8.0 * (double)y + 1.0) + 1.0) * 0.5);
    while (J * (J - 1) / 2 > y) --J;
    while ((J + 1) * J / 2 <= y) ++J;
    const int I = y - J * (J - 1) / 2;
    return s < 2 ? 2 * I + s : 2 * J + (s - 2);
}

// is the block pair (a, b) of the staged blocks one this workgroup accumulates
template <int NS, bool OFF>
constexpr bool cov_takes(int a, int b) { return OFF ? (a < 2 && b >= 2) : a <= b; }

// grid (ntiles, y), 64 threads.  !OFF: y = 1 and blocks 0 .. NS - 1 (form A), or NS = 2 and y over the super-blocks (form B's diagonal);
// OFF: NS = 4, y over the pairs of super-blocks
template <int NS, bool OFF>
__global__ __launch_bounds__(64) void cov_tile_kernel(CovArgs A)
{
    static_assert(!OFF || NS == 4, "a pair of super-blocks is four staged blocks");
    constexpr int NR = 16 * NS;
    __shared__ double Z[NR * COV_LD];
    __shared__ double SH[NR];
    const int lane = threadIdx.x, li = lane & 15, lk = lane >> 4;
    const size_t tile = blockIdx.x;
    const int nf = A.nfields;
    const bool act = tile * 64 + (size_t)lane < (size_t)A.nchains;
    int blk[NS];
#pragma unroll
    for (int s = 0; s < NS; ++s) blk[s] = cov_block<NS, OFF>(s, (int)blockIdx.y);
    if (lane < NR) { const int f = 16 * blk[lane >> 4] + (lane & 15); SH[lane] = A.shift[f < nf ? f : nf - 1]; }
    mcx_d4 acc[NS][NS];
#pragma unroll
    for (int a = 0; a < NS; ++a)
#pragma unroll
        for (int b = 0; b < NS; ++b) acc[a][b] = mcx_d4{0.0, 0.0, 0.0, 0.0};
    double v[NR];
    // Staged row r is row 16 bo[r >> 4] + (r & 15) of the matrix: a field below nfo, the ones at nfo, nothing above.  nfo and bo are nf and
    // blk made opaque where they are used: as loop invariants the NR row tests and NR clamped row offsets are all formed before the loop
    // and kept in scalar registers across it, more than there are (237 spilled at NS = 4)
    // the rows of window sample w; a row that is no field loads the last field again (a valid row, not used)
    auto load = [&](int w) {
        int nfo = nf, bo[NS];
        asm volatile("" : "+s"(nfo));
#pragma unroll
        for (int s = 0; s < NS; ++s) { bo[s] = blk[s]; asm volatile("" : "+s"(bo[s])); }
        const double *p = A.store + samples_row(samples_slot(A.slot0, w, A.cap), (size_t)A.ntiles, (size_t)nf, tile, 0) + lane;
#pragma unroll
        for (int r = 0; r < NR; ++r) { const int f = 16 * bo[r >> 4] + (r & 15); v[r] = p[(size_t)(f < nfo ? f : nfo - 1) * 64]; }
    };
    load(0);
    __syncthreads();                                            // SH
    for (int w = 0; w < A.ns; ++w) {
        {
            int nfo = nf, bo[NS];
            asm volatile("" : "+s"(nfo));
#pragma unroll
            for (int s = 0; s < NS; ++s) { bo[s] = blk[s]; asm volatile("" : "+s"(bo[s])); }
#pragma unroll
            for (int r = 0; r < NR; ++r) {
                const int f = 16 * bo[r >> 4] + (r & 15);
                // selected, not multiplied: the padding lanes and the rows loaded again hold no defined values
                Z[r * COV_LD + lane] = f < nfo ? (act ? v[r] - SH[r] : 0.0) : (f == nfo ? 1.0 : 0.0);
            }
        }
        __syncthreads();
        load(w + 1 < A.ns ? w + 1 : w);                         // in flight under the MFMAs (the last slot again: valid, not used)
        const double *zp = Z + li * COV_LD + lk;
#pragma unroll 4
        for (int m = 0; m < 16; ++m) {
            double op[NS];
#pragma unroll
            for (int s = 0; s < NS; ++s) op[s] = zp[16 * s * COV_LD + 4 * m];
#pragma unroll
            for (int a = 0; a < NS; ++a)
#pragma unroll
                for (int b = 0; b < NS; ++b)
                    if (cov_takes<NS, OFF>(a, b)) acc[a][b] = __builtin_amdgcn_mfma_f64_16x16x4f64(op[a], op[b], acc[a][b], 0, 0, 0);
        }
        __syncthreads();                                        // the operand reads are done before the next slot is staged
    }
    // lane l, register q of block pair (a, b) holds row j = 16 blk[a] + (l >> 4) + 4 q, column k = 16 blk[b] + (l & 15): column nf is S_j,
    // a column below it with j <= k is G_jk; nothing else is written
    const size_t len = (size_t)nf + (size_t)nf * (size_t)(nf + 1) / 2;
    double *o = A.out + tile * len;
#pragma unroll
    for (int a = 0; a < NS; ++a)
#pragma unroll
        for (int b = 0; b < NS; ++b)
            if (cov_takes<NS, OFF>(a, b)) {
                const int k = 16 * blk[b] + li;
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int j = 16 * blk[a] + lk + 4 * q;
                    if (j < nf && k == nf) o[j] = acc[a][b][q];
                    else if (j <= k && k < nf) o[(size_t)nf + cov_pair((size_t)j, (size_t)k, (size_t)nf)] = acc[a][b][q];
                }
            }
}

// [n, shift[nfields], S[nfields], G packed] from the tree's result v[nfields + nfields (nfields + 1) / 2] (copies, no arithmetic)
__global__ void cov_pack_kernel(const double *v, const double *shift, double *out, int nfields, int len, double n)
{
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= 1 + nfields + len) return;
    out[k] = k == 0 ? n : k <= nfields ? shift[k - 1] : v[k - 1 - nfields];
}

} // namespace mcx
