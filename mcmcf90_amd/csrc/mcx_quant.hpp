// mcx_quant.hpp -- exact order statistics and tail counts of the thinned sample store (mcmcx_samples_order_stats / _counts; no counterpart
// in the single-chain reference): a most-significant-digit radix select on 64-bit keys, reduced where the ring lies.  None of these is a
// sampling kernel: they draw nothing, write nothing but their scratch and the caller's vector, and are no entry of the kernel-selection
// tables.
//
// The definition (include/mcmcx.h has it in full).  With b the double's bits,
//     key(x) = b ^ (b >> 63 ? 0xFFFFFFFFFFFFFFFF : 0x8000000000000000)
// and the unsigned order of the keys is the total order: negative NaNs < -inf < .. < -0.0 < +0.0 < .. < +inf < positive NaNs.  os_f(r) is
// the value of field f whose key is the r-th smallest (0-based) of the window's n = ns x nchains keys, returned with its own bits;
// lt_f(x) / le_f(x) count the window's keys below / not above key(x).  Neither depends on an order of summation: every count is an integer.
//
// Select: 64 / QUANT_B passes from the top digit down.  A pass streams the window once in whole 512-byte rows (a lane per chain, a loop
// over the window's slots, every offset through samples_row in size_t); a value whose bits above the pass's digit equal the prefix of a
// (field, rank) counts its digit in that rank's histogram in LDS, and the block flushes its non-zero bins to the table
// [nfields][nr][2**B] of 64-bit counts with integer atomics.  quant_pick_kernel then finds each rank's bin, extends its prefix, takes the
// counts below the bin off the rank and clears the table; quant_out_kernel maps the finished prefixes back.  Ranks of a field whose
// prefixes are equal share one histogram, the first of them (their leader) -- in pass 1 all of them.
#pragma once
#include "mcx_diag.hpp"

namespace mcx {

constexpr int QUANT_MAXR = 32;      // = MCMCX_QUANT_MAXR
constexpr int QUANT_B = 8;          // bits per digit
constexpr int QUANT_NB = 1 << QUANT_B;
constexpr int QUANT_LB = 8;         // rows a wave has in flight

// the key map and its inverse (compiled for the host too: mcmcx_debug_quant_key, and the host's staging of the thresholds)
__host__ MCX_DEV unsigned long long quant_key(unsigned long long b) { return b ^ ((b >> 63) ? ~0ull : 0x8000000000000000ull); }
__host__ MCX_DEV unsigned long long quant_unkey(unsigned long long k) { return k ^ ((k >> 63) ? 0x8000000000000000ull : ~0ull); }

struct QuantRanks { long long r[QUANT_MAXR]; };                 // a launch argument: staged by the launch itself

struct QuantWin {
    SampleWin win;                                              // the window (mcx_samples.hpp)
    int chunk;                                                  // window samples per blockIdx.z (32-bit counters stay below 2**32)
};

// scratch of a select, in 64-bit words: table[nfields][nr][2**B], then prefix, rest (the rank inside the prefix's bucket) and leader,
// [nfields][nr] each
struct QuantState {
    unsigned long long *table, *prefix, *rest, *leader;
    int nr;
};

// table := 0; prefix := 0, rest := rank, leader := 0 (the empty prefix is every rank's)
__global__ __launch_bounds__(256) void quant_init_kernel(QuantState S, QuantRanks R, int nfields)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x, m = (size_t)nfields * (size_t)S.nr;
    if (i < m * QUANT_NB) S.table[i] = 0ull;
    if (i < m) { S.prefix[i] = 0ull; S.rest[i] = (unsigned long long)R.r[i % (size_t)S.nr]; S.leader[i] = 0ull; }
}

// One pass: the digit at bit `sh` of every window value of field blockIdx.y whose higher bits equal a leader's prefix.
// grid (gx, nfields, gz), 256 threads, nr x 2**B 32-bit counters of dynamic LDS.  The block's four waves take tiles 4 bx + w,
// + 4 gx, ..; blockIdx.z takes window samples z chunk .. (z + 1) chunk - 1.  The leading digits are nearly the same for every value
// of a field, so a digit that is the same in all matching lanes of a wave is ONE add of their number (a ballot against the first
// matching lane's digit); only a wave whose digits differ falls back to an atomic per lane.
MCX_HD size_t quant_hist_lds(int nr) { return (size_t)nr * QUANT_NB * sizeof(unsigned int); }    // [nr][2**B] counters
__global__ __launch_bounds__(256) void quant_hist_kernel(QuantWin A, QuantState S, int sh)
{
    extern __shared__ unsigned int quant_lds[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nr = S.nr;
    const int f = blockIdx.y;
    __shared__ unsigned long long lpre[QUANT_MAXR];             // the field's leaders: their prefixes and rank indices, compacted
    __shared__ int lidx[QUANT_MAXR], nlead;
    for (int i = threadIdx.x; i < nr * QUANT_NB; i += 256) quant_lds[i] = 0u;
    if (threadIdx.x == 0) {
        int n = 0;
        for (int k = 0; k < nr; ++k)
            if (S.leader[(size_t)f * nr + k] == (unsigned long long)k) { lpre[n] = S.prefix[(size_t)f * nr + k]; lidx[n++] = k; }
        nlead = n;
    }
    __syncthreads();
    const int nl = nlead;
    const int w0 = (int)blockIdx.z * A.chunk, w1 = min(A.win.ns, w0 + A.chunk);
    const int hs = sh + QUANT_B;                                // the prefix is the bits from hs up (none in the first pass)
    for (size_t tile = (size_t)blockIdx.x * 4 + wave; tile < (size_t)A.win.ntiles; tile += (size_t)gridDim.x * 4) {
        const bool act = tile * 64 + (size_t)lane < (size_t)A.win.nchains;      // the store's padding rows hold no defined values
        for (int j0 = w0; j0 < w1; j0 += QUANT_LB) {
            double v[QUANT_LB];
#pragma unroll
            for (int q = 0; q < QUANT_LB; ++q)
                v[q] = A.win.store[samples_row(samples_slot(A.win.slot0, min(j0 + q, w1 - 1), A.win.cap), (size_t)A.win.ntiles,
                                               (size_t)A.win.nfields, tile, (size_t)f) + lane];
#pragma unroll
            for (int q = 0; q < QUANT_LB; ++q) {
                if (j0 + q >= w1) break;                        // the whole wave
                const unsigned long long key = quant_key((unsigned long long)__double_as_longlong(v[q]));
                const unsigned int digit = (unsigned int)(key >> sh) & (QUANT_NB - 1);
                const unsigned long long top = hs < 64 ? key >> hs : 0ull;
                for (int a = 0; a < nl; ++a) {
                    const bool match = act && top == lpre[a];
                    const unsigned long long m = __ballot(match);
                    if (!m) continue;
                    const int k = lidx[a];
                    const int first = __ffsll((long long)m) - 1;
                    const unsigned int d0 = (unsigned int)__builtin_amdgcn_readlane((int)digit, first);
                    const unsigned long long u = __ballot(match && digit == d0);
                    if (u == m) { if (lane == first) atomicAdd(&quant_lds[k * QUANT_NB + (int)d0], (unsigned int)__popcll(m)); }
                    else if (match) atomicAdd(&quant_lds[k * QUANT_NB + (int)digit], 1u);
                }
            }
        }
    }
    __syncthreads();
    unsigned long long *table = S.table + (size_t)f * (size_t)nr * QUANT_NB;
    for (int i = threadIdx.x; i < nr * QUANT_NB; i += 256) {
        const unsigned int c = quant_lds[i];
        if (c) atomicAdd(&table[i], (unsigned long long)c);     // integer adds commute: no arrival order in the result
    }
}

// Between two passes, one block of 256 threads per field (thread t = bin t): for every rank the bin of its leader's histogram that holds
// it -- the first whose inclusive running count exceeds `rest` --, prefix := prefix << B | bin, rest -= the counts below the bin; then
// the new leaders (the first rank of the field with the same prefix) and the field's table cleared.  The prefix is stored right-aligned.
__global__ __launch_bounds__(256) void quant_pick_kernel(QuantState S)
{
    __shared__ unsigned long long wsum[4], npre[QUANT_MAXR];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, nr = S.nr;
    const size_t f0 = (size_t)blockIdx.x * (size_t)nr;
    unsigned long long *table = S.table + f0 * QUANT_NB;
    for (int k = 0; k < nr; ++k) {
        const unsigned long long c = table[(size_t)S.leader[f0 + k] * QUANT_NB + t], rest = S.rest[f0 + k];
        unsigned long long incl = c;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const unsigned long long o = __shfl_up(incl, d);
            if (lane >= d) incl += o;
        }
        __syncthreads();                                        // the previous rank's wsum is read
        if (lane == 63) wsum[wave] = incl;
        __syncthreads();
        for (int w = 0; w < wave; ++w) incl += wsum[w];
        const unsigned long long excl = incl - c;
        if (excl <= rest && rest < incl) {                      // one thread: rest is below the histogram's total
            npre[k] = (S.prefix[f0 + k] << QUANT_B) | (unsigned long long)t;
            S.rest[f0 + k] = rest - excl;
        }
    }
    __syncthreads();
    if (t < nr) {
        int l = t;
        for (int k = t - 1; k >= 0; --k) if (npre[k] == npre[t]) l = k;
        S.prefix[f0 + t] = npre[t];
        S.leader[f0 + t] = (unsigned long long)l;
    }
    for (int i = t; i < nr * QUANT_NB; i += 256) table[i] = 0ull;
}

// after the last pass the prefix is the key: out[nfields][nr] takes the values' own bits
__global__ __launch_bounds__(256) void quant_out_kernel(QuantState S, double *out, int nfields)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < (size_t)nfields * (size_t)S.nr) out[i] = __longlong_as_double((long long)quant_unkey(S.prefix[i]));
}

// ---- counts: one pass.  out[nfields][nq][2] = lt, le, 64-bit, zeroed by quant_counts_zero_kernel; xkey[nfields][nq] the thresholds' keys.
__global__ __launch_bounds__(256) void quant_counts_zero_kernel(unsigned long long *out, int n)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) out[i] = 0ull;
}

// grid (gx, ceil(nfields / 4), gz), 256 threads: wave w of block (b, y, z) takes field 4 y + w, tiles b, b + gx, .. and window samples
// z chunk .. (z + 1) chunk - 1.  Two key compares per value and threshold into per-lane 32-bit counts in registers (NQ, the
// instantiation's bound on nq, makes their indices compile-time), the wave's 64 lanes summed in 64 bits, one integer atomic per wave
// and count.  No LDS.
template <int NQ>
__global__ __launch_bounds__(256) void quant_counts_kernel(QuantWin A, const unsigned long long *__restrict__ xkey, unsigned long long *out,
    int nq)
{
    constexpr int LB = NQ > 8 ? 4 : QUANT_LB;                   // rows in flight: fewer where the counts take the registers
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int f = (int)blockIdx.y * 4 + wave;
    if (f >= A.win.nfields) return;                             // the whole wave
    unsigned long long xk[NQ];
#pragma unroll
    for (int q = 0; q < NQ; ++q) { xk[q] = xkey[(size_t)f * (size_t)nq + (size_t)min(q, nq - 1)]; asm volatile("" : "+v"(xk[q])); }
    unsigned int lt[NQ], le[NQ];
#pragma unroll
    for (int q = 0; q < NQ; ++q) { lt[q] = 0u; le[q] = 0u; }
    const int w0 = (int)blockIdx.z * A.chunk, w1 = min(A.win.ns, w0 + A.chunk);
    for (size_t tile = blockIdx.x; tile < (size_t)A.win.ntiles; tile += gridDim.x) {
        const bool act = tile * 64 + (size_t)lane < (size_t)A.win.nchains;
        for (int j0 = w0; j0 < w1; j0 += LB) {
            double v[LB];
#pragma unroll
            for (int u = 0; u < LB; ++u)
                v[u] = A.win.store[samples_row(samples_slot(A.win.slot0, min(j0 + u, w1 - 1), A.win.cap), (size_t)A.win.ntiles,
                                               (size_t)A.win.nfields, tile, (size_t)f) + lane];
#pragma unroll
            for (int u = 0; u < LB; ++u) {
                const unsigned long long key = quant_key((unsigned long long)__double_as_longlong(v[u]));
                const unsigned int one = (act && j0 + u < w1) ? 1u : 0u;
#pragma unroll
                for (int q = 0; q < NQ; ++q) { lt[q] += key < xk[q] ? one : 0u; le[q] += key <= xk[q] ? one : 0u; }
            }
        }
    }
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
        unsigned long long a = lt[q], b = le[q];
#pragma unroll
        for (int k = 1; k < 64; k <<= 1) { a += __shfl_xor(a, k); b += __shfl_xor(b, k); }
        if (lane == 0 && q < nq) {
            unsigned long long *o = out + ((size_t)f * (size_t)nq + (size_t)q) * 2;
            if (a) atomicAdd(o, a);
            if (b) atomicAdd(o + 1, b);
        }
    }
}

} // namespace mcx
