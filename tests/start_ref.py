"""The drawn start points of mcmcx_set_par0_spread, restated with the oracle's generator (include/mcmcx.h, "Per-chain start points", is the
definition; start_spread_kernel, mcmcf90_amd/csrc/mcx_start.hpp, is the device's statement).  TEST INFRASTRUCTURE.

Chain c draws from its own Philox stream, key (seed, chain_id0 + c), from uniform number 2**63 on with an empty polar cache (the oracle's
`Rng` has a settable `n`).  One attempt: z_k = mcxo_normal, k ascending; x = U0'z through mcxo_trmv_ut (fma chains from +0.0, i ascending
to j); theta = par0 + (scale * x), two roundings.  U0 = dpotf2('U', cmat0) * 2.4 / sqrt(npar).  With a box, an attempt outside it
(mcxt_inbounds' test: lo < theta < hi, a NaN is outside) is followed by the next one from the same stream, TRIES at the most; then par0."""
import ctypes as C
import math

import numpy as np

TRIES = 64                      # MCMCX_START_TRIES
N0 = 1 << 63                    # the first uniform of the start draws
SEED = 0x6D636D63               # MCMCX_DEFAULT_SEED, the oracle's default


def initial_factor(oracle, cmat0):
    """U0[i, j], upper triangular: what host_initial_R returns and mcmcx_get_R shows after init.  None when dpotf2 fails."""
    L = oracle.lib()
    cm = np.asarray(cmat0, dtype=np.float64)
    d = cm.shape[0]
    A = np.asfortranarray(np.triu(cm).copy())
    if L.mcxo_potrf_u(d, A.ctypes.data_as(oracle._DP)) != 0:
        return None
    return np.triu(np.array(A)) * 2.4 / math.sqrt(float(d))


def start_rng(oracle, chain_id, seed=SEED):
    g = oracle.Rng()
    g.key[0], g.key[1] = seed, chain_id
    g.n, g.saved, g.saved_y = N0, 0, 0.0
    return g


def inbounds(theta, lo, hi):
    ok = True
    if lo is not None:
        ok = ok and bool(np.all(theta > lo))
    if hi is not None:
        ok = ok and bool(np.all(theta < hi))
    return ok


def attempt(oracle, g, U0f, par0, scale):
    """One attempt from the stream g: the next npar normals, U0'z, par0 + scale x."""
    L = oracle.lib()
    d = len(par0)
    x = np.array([L.mcxo_normal(C.byref(g)) for _ in range(d)])
    L.mcxo_trmv_ut(d, U0f.ctypes.data_as(oracle._DP), x.ctypes.data_as(oracle._DP))
    return par0 + (scale * x)


def starts(oracle, nchains, par0, cmat0, scale, lo=None, hi=None, seed=SEED, chain_id0=0):
    """(theta[nchains, npar], tries[nchains], fell[nchains]): every chain's start, the attempts it made (1 .. TRIES) and whether none
    of them was inside the box (the start is then par0 bit for bit)."""
    par0 = np.asarray(par0, dtype=np.float64)
    U0 = initial_factor(oracle, cmat0)
    assert U0 is not None, "cmat0 has no Cholesky factor: mcmcx_init refuses"
    U0f = np.asfortranarray(U0)
    lo = None if lo is None else np.asarray(lo, dtype=np.float64)
    hi = None if hi is None else np.asarray(hi, dtype=np.float64)
    out = np.zeros((nchains, len(par0))); tries = np.zeros(nchains, dtype=np.int64); fell = np.zeros(nchains, dtype=bool)
    for c in range(nchains):
        g = start_rng(oracle, chain_id0 + c, seed)
        for t in range(1, TRIES + 1):
            th = attempt(oracle, g, U0f, par0, scale)
            tries[c] = t
            if inbounds(th, lo, hi):
                break
        else:
            th, fell[c] = par0.copy(), True
        out[c] = th
    return out, tries, fell


def info(tries, fell):
    """mcmcx_start_info's out3[1:] of these chains: those that made more than one attempt, those that fell back to par0."""
    return int((tries > 1).sum()), int(fell.sum())
