// mcx_start.hpp -- per-chain start points drawn on the device (mcmcx_set_par0_spread; the definition is include/mcmcx.h's, restated in
// tests/start_ref.py): start_spread_kernel (one of the family headers mcx_kernels.hpp includes, after mcx_adapt)
#pragma once
#include "mcx_adapt.hpp"

namespace mcx {

constexpr int START_TRIES = 64;                      // MCMCX_START_TRIES (include/mcmcx.h; mcx_api.hip asserts that they agree)
constexpr uint64_t START_STREAM_N0 = 1ull << 63;     // the first uniform of a chain's start draws: no run reaches that number
constexpr uint32_t START_FELL_BACK = 0x80000000u;    // tries[]: the chain used up its attempts and starts at par0

// One lane = one chain, one wave = one tile.  An attempt: z_k = rng_normal, k ascending, from the chain's own Philox stream (seed,
// chain_id0 + chain) at uniform number 2**63 (so the sampling stream, which starts at 0, is not advanced and the starts do not depend
// on how chains are spread over engines); x = U0' z as mcxo_trmv_ut's fma chains (from +0.0, i ascending to j) with U0 the SHARED
// packed initial factor; start_k = par0_k + (scale * x_k), two roundings (the file is compiled with -ffp-contract=off).  With a box
// (mcmcx_set_bounds) a rejected attempt is followed by another one from the next normals of the same stream, the polar cache carried
// over; after START_TRIES rejected attempts the chain starts at par0 bit for bit.  The lanes of a wave leave the loop at different
// trip counts: it runs under a diverging exec mask, bounded by the constant.  The attempt's normals live in the chain's scratch
// vector zs (npar doubles per lane in memory, not in registers: no npar-sized register array, nothing to spill); U0 and par0 are
// uniform addresses, read through the scalar cache.  Padding lanes of the last tile get par0.
// tries[tile * 64 + lane] = attempts made (1 .. START_TRIES), | START_FELL_BACK when none was inside the box.
__global__ __launch_bounds__(64) void start_spread_kernel(EngineDev E, const double *__restrict__ U0, double scale, int nchains,
                                                          uint32_t *__restrict__ tries)
{
    const int lane = threadIdx.x, tile = blockIdx.x, d = E.d;
    const int chain = tile * 64 + lane;
    double *st = E.start + (size_t)tile * d * 64;
    double *z = E.zs + (size_t)tile * 2 * d * 64;
    Rng g;
    g.k0 = E.k0; g.k1 = E.chain_id0 + (uint32_t)chain; g.n = START_STREAM_N0; g.c2 = g.c3 = 0u; g.cblk = 0; g.saved = 0; g.saved_y = 0.0;
    uint32_t ntry = 0;
    bool done = !(chain < nchains);
    if (done) for (int k = 0; k < d; ++k) GV(st, k) = E.par0[k];
    while (!done) {
        ++ntry;
        for (int k = 0; k < d; ++k) GV(z, k) = rng_normal(g);
        for (int j = 0; j < d; ++j) {
            double t = 0.0;
            for (int i = 0; i <= j; ++i) t = dfma(U0[pidx(i, j, d)], GV(z, i), t);
            GV(st, j) = E.par0[j] + (scale * t);
        }
        done = target_inbounds(E.tgt, d, lane, st);
        if (!done && ntry == (uint32_t)START_TRIES) {
            for (int k = 0; k < d; ++k) GV(st, k) = E.par0[k];
            ntry |= START_FELL_BACK;
            done = true;
        }
    }
    tries[chain] = ntry;
}

} // namespace mcx
