// mcx_pooled_phase.hpp -- pooled mode with the iteration cut at the USER's evaluations (a target module's kernel or host callbacks between
// the engine's launches): pooled_phase_kernel (lane = chain, the shared tables through the scalar cache) and pooled_phase_mfma_kernel (the
// proposals' products on the f64 matrix cores).  (one of the family headers mcx_kernels.hpp includes, after mcx_phase)
#pragma once
#include "mcx_phase.hpp"

namespace mcx {

// pooled method = 'ram': the tick's statistic (moments_kernel kind 2) reads the last iteration's normals from the (it & 1) half of the
// chain's two normal vectors, where the single-launch kernels leave them; the phases keep stage-1 normals in the first half (the tail of
// step_kernel_cols)
MCX_DEV void pooled_phase_keep_normals(const EngineDev &E, int tile, int lane, int it)
{
    if (E.dodr || !(it & 1)) return;
    double *zs_t = E.zs + (size_t)tile * 2 * E.d * 64;
    for (int k = 0; k < E.d; ++k) GV(zs_t, E.d + k) = GV(zs_t, k);
}

// ---------------------------------------------------------------- the lane form
// The phase bodies of the host-callback path with the shared factor, second-stage factor and inverse covariance passed (trmv_shared /
// gemvN_shared / quadform_sym_shared): PA the phase of iteration itA, PB = 0 the proposal of iteration itB = itA + 1 riding behind an
// iteration's last phase (host_iteration's fuse_next), PB < 0 none.  The kernels see pooled RAM as a plain Metropolis step (kernel_method),
// so the method class is 0: no instantiation carries the rank-one update.
template <int PA, int PB>
__global__ __launch_bounds__(64) void pooled_phase_kernel(EngineDev E, int itA, int itB, const double *__restrict__ ramscale,
    const double *__restrict__ sR, const double *__restrict__ sR2, const double *__restrict__ siC)
{
    extern __shared__ double X[];
    const int lane = threadIdx.x, tile = blockIdx.x;
    host_phase_body<PA, 0>(E, tile, lane, itA, ramscale + itA, 0, X, sR, sR2, siC);
    if constexpr (PB >= 0) host_phase_body<PB, 0>(E, tile, lane, itB, ramscale + itB, 0, X, sR, sR2, siC);
    else if constexpr (PA == 1 || PA == 2 || PA == 4) pooled_phase_keep_normals(E, tile, lane, itA);   // (PA == 1 with DR: returns at once)
}

// ---------------------------------------------------------------- the proposals on the matrix cores
// newpar = oldpar + R'z (STAGE2: newpar2 = oldpar + R2'z for the chains whose first stage was rejected) as pooled_mfma_kernel makes it: one
// wave per tile, z straight into the LDS vector X [d4][64], P = M'z as v_mfma_f64_16x16x4_f64 tiles against the dense table g_M (SH_RT /
// SH_DRT: M[s*d + o] = R(s,o); condmax > 0: the full factor), the products over the vector they came from (npar <= 64: one pass of four
// output blocks), the candidate back in lane = chain order.  Rows beyond an output block's last column are zero in a triangular factor and
// are skipped (they would add 0*z): per chain the accumulation order of trmv_shared / gemvN_shared, so the lane form bit for bit.
// The chain's stream moves exactly as in host_phase_body<0> / <1>; its state is stored before the product, which then holds no more than
// the sixteen accumulators.  keepz: the normals go to the chain's global vector too (pooled RAM's statistic reads them).
template <bool STAGE2>
MCX_DEV void pooled_phase_propose(const EngineDev &E, int tile, int lane, double *X, const double *__restrict__ g_M, int keepz)
{
    const int d = E.d, d4 = (d + 3) & ~3, nt = (d + 15) >> 4, li = lane & 15, lk = lane >> 4;
    const double *theta_t = E.theta + (size_t)tile * d * 64;
    double *dst_t = STAGE2 ? E.cs + (size_t)tile * 2 * d * 64 : E.cand + (size_t)tile * d * 64;
    double *zs_t = E.zs + ((size_t)tile * 2 + (STAGE2 ? 1 : 0)) * d * 64;
    double *hx = E.hx + (size_t)tile * NHX * 64;
    const bool m = STAGE2 ? GV(hx, HX_STAGE2) != 0.0 : true;
    if (STAGE2 && !__any(m)) return;                                   // nobody's first stage was rejected
    {
        LaneState L;
        lane_load(E, tile, lane, L);
        if (STAGE2 && !m) for (int k = 0; k < d; ++k) XL(k) = 0.0;     // a chain that does not draw: newpar2 = oldpar, never looked at
        const double su = MCX_POOLED_GEN(L.g, X, lane, d, m);
        if (!STAGE2) GV(hx, HX_SU) = su;
        lane_store(E, tile, lane, L);
    }
    if (keepz) for (int k = 0; k < d; ++k) GV(zs_t, k) = XL(k);
    for (int k = d; k < d4; ++k) XL(k) = 0.0;
    mcx_d4 c[4][4];
    if (E.usesvd) mfma_wave_product<false>(g_M, X, lane, d, d4, 0, nt, c);
    else mfma_wave_product<true>(g_M, X, lane, d, d4, 0, nt, c);
#pragma unroll
    for (int b = 0; b < 4; ++b)
        if (b < nt) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = 16 * b + lk + 4 * r;
                if (row < d4) {                                         // rows >= d are never read
                    double *o = X + (size_t)row * 64 + li;
                    o[0] = c[b][0][r]; o[16] = c[b][1][r]; o[32] = c[b][2][r]; o[48] = c[b][3][r];
                }
            }
        }
    constexpr int CB = MCX_POOLED_CB;                    // state elements' loads before their stores (pooled_mfma_kernel: candidate_from_T)
    for (int k0 = 0; k0 < d; k0 += CB) {
        double th[CB], tv[CB];
#pragma unroll
        for (int u = 0; u < CB; ++u) { const int k = (k0 + u < d) ? k0 + u : d - 1; th[u] = GV(theta_t, k); tv[u] = XL(k); }
#pragma unroll
        for (int u = 0; u < CB; ++u) if (k0 + u < d) GV(dst_t, k0 + u) = th[u] + tv[u];
    }
}
// PA: the phase of iteration itA that precedes the proposal in the launch -- -1 none (the run's or a segment's first proposal), 1 / 2 / 4
// an iteration's last phase, followed by iteration itB's proposal; <1, true>: the first stage's decision followed by the second stage's
// proposal (delayed rejection).  The phases hand over through the chain's own state as in host_phase_seq_kernel; the decision of phase 2
// reads the packed inverse covariance siC (quadform_sym_shared) and takes its two work vectors from the LDS the proposal uses after it.
// Two waves per SIMD: what the LDS vector leaves a CU at npar 50 (six waves) needs no more.
// Its LDS: the proposal's vector X [d4][64] doubles; phase 2's decision, which runs before it, takes its two work vectors (DrLds, where
// they are in LDS) from the same rows
MCX_HD size_t pooled_phase_mfma_lds(int d, bool dr_vectors)
{
    const size_t x = (size_t)((d + 3) & ~3) * 64 * sizeof(double), q = DrLds::bytes(d, dr_vectors);
    return x > q ? x : q;
}
template <int PA, bool STAGE2>
__global__ __launch_bounds__(64, 2) void pooled_phase_mfma_kernel(EngineDev E, int itA, int itB, const double *__restrict__ ramscale,
    const double *__restrict__ g_M, const double *__restrict__ siC, int keepz)
{
    extern __shared__ double X[];
    const int lane = threadIdx.x, tile = blockIdx.x;
    if constexpr (PA >= 0) host_phase_body<PA, 0, false>(E, tile, lane, itA, ramscale + itA, 0, X, nullptr, nullptr, siC);
    (void)itB;
    pooled_phase_propose<STAGE2>(E, tile, lane, X, g_M, keepz);
}

} // namespace mcx
