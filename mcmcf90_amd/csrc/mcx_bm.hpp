// mcx_bm.hpp -- the batch-means covariance of the thinned sample store on the f64 matrix cores (mcmcx_samples_cov_bm; no counterpart in the
// single-chain reference): the covariance, over all chains, of the MEANS of batches of `batch` consecutive window samples -- what the
// multivariate ESS (batch ~ sqrt(ns)) and the multivariate split-R-hat (batch = the half window) are finished from on the host
// (mcx_host_bm.hpp).  bm_tile_kernel restates cov_tile_kernel's body (mcx_cov.hpp, as it is) with the batch accumulation in front of the
// staging; cov_block, cov_takes, cov_pair, COV_LD, cov_pack_kernel, diag_shift_kernel and moments_tree_kernel are used as they are.  No
// sampling kernel: it draws nothing, writes nothing but its scratch and the caller's vector, and is no entry of the kernel-selection tables.
//
// The definition (include/mcmcx.h has it in full).  z = x_f - shift_f; per chain, field and batch k the mean
//     y = (..((z_0 + z_1) + z_2)..) / (double)batch         over window samples k batch .. (k + 1) batch - 1, the sum starting at z_0
// and per tile, over the batches k ascending and within a batch the tile's lanes c = 0 .. 63 ascending, a lane without a chain selected
// to +0.0, the covariance's chains with y in the place of z:
//     s_j  = s_j + y_j[k][c]                     from +0.0
//     g_jk = fma(y_j[k][c], y_k[k][c], g_jk)     from +0.0,  j <= k
// With batch = 1, y = z / 1.0 = z and the rows are cov_tile_kernel's bit for bit (the kernel leaves that division out: it is exact).
//
// Shape: cov_tile_kernel's -- one wave per workgroup and tile, the rows of the next sample in flight in registers, Z[row][COV_LD] in LDS,
// one MFMA chain per block pair.  The running sum of a batch needs no register: lane l stages column l of Z and nobody else touches that
// column before the operand reads, so the sum lives in Z[row][l] across the batch -- read, add, written back by the same lane, no barrier.
// Only the last sample of a batch divides, selects the padding lanes and the rows that are no field, synchronises and issues the MFMAs:
// the same bytes as the covariance are read once, 1 / batch of its MFMAs are issued.  The staging comes in four compile-time forms (first
// sample of a batch or not, dividing or not) chosen by wave-uniform branches, so the unrolled row loop has no branch inside.
#pragma once
#include "mcx_cov.hpp"

namespace mcx {

// CovArgs' members and the batch length; ns counts the samples that are read: nb * batch
struct BmArgs {
    const double *store; const double *shift; double *out;      // the ring; shift[nfields]; out[ntiles][nf + nf (nf + 1) / 2]
    size_t slot0, cap;                                          // ring slot of window sample 0, the ring's capacity
    int ntiles, nfields, nchains, ns, batch;
};

// grid and forms as cov_tile_kernel's: grid (ntiles, y), 64 threads
template <int NS, bool OFF>
__global__ __launch_bounds__(64) void bm_tile_kernel(BmArgs A)
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
    // nfo and bo are nf and blk made opaque where they are used, for cov_tile_kernel's reason: as loop invariants the NR row tests and
    // clamped row offsets would all be kept in scalar registers across the loop, more than there are
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
    const double db = (double)A.batch;
    // the rows in registers into this lane's column of Z.  FIRST: the batch's sum starts at z_0, else the column's sum + z.  END: the
    // batch ends here, so what is staged is the operand -- selected, not multiplied: the padding lanes and the rows loaded again hold no
    // defined values -- and with DIV it is divided first (batch > 1).  Before the end the column holds sums only this lane reads.
    auto stage = [&](auto first, auto end, auto div) {
        int nfo = nf, bo[NS];
        asm volatile("" : "+s"(nfo));
#pragma unroll
        for (int s = 0; s < NS; ++s) { bo[s] = blk[s]; asm volatile("" : "+s"(bo[s])); }
#pragma unroll
        for (int r = 0; r < NR; ++r) {
            double *zc = Z + r * COV_LD + lane;
            double s = v[r] - SH[r];
            if (!decltype(first)::value) s = *zc + s;
            if (decltype(div)::value) s = s / db;
            if (decltype(end)::value) {
                const int f = 16 * bo[r >> 4] + (r & 15);
                *zc = f < nfo ? (act ? s : 0.0) : (f == nfo ? 1.0 : 0.0);
            } else *zc = s;
        }
    };
    using T = std::true_type; using F = std::false_type;
    load(0);
    __syncthreads();                                            // SH
    int i = 0;                                                  // where window sample w lies in its batch
    for (int w = 0; w < A.ns; ++w) {
        const bool first = i == 0, end = i + 1 == A.batch;
        const int next = w + 1 < A.ns ? w + 1 : w;              // (the last slot again: valid, not used)
        if (!end) {
            if (first) stage(T{}, F{}, F{}); else stage(F{}, F{}, F{});
            load(next);
            ++i;
            continue;
        }
        if (first) stage(T{}, T{}, F{});                        // batch = 1: y = z / 1.0 = z, the covariance's staging
        else stage(F{}, T{}, T{});
        i = 0;
        __syncthreads();
        load(next);                                             // in flight under the MFMAs
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
        __syncthreads();                                        // the operand reads are done before the next batch is staged
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

} // namespace mcx
