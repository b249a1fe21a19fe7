"""The convergence summary of a window of retained samples (mcmcx_samples_stats / mcmcx_samples_diag), restated in numpy from its definition
in include/mcmcx.h -- NOT from the kernels' scheme (a wave per field row, a rotating window of centred values, instantiations by lag count):

    window           samples 0 .. ns - 1, n_h = ns // 2, half 0 = samples 0 .. n_h - 1, half 1 = samples ns - n_h .. ns - 1, K = min(maxlag, n_h - 1)
    per chain, half  y_i = x_i - shift;  s = (..((y_0 + y_1) + y_2) ..);  m = s / n_h;  z_i = y_i - m;
                     g_t = sum over i = 0 .. n_h - 1 - t ascending of z_i * z_{i+t}, from +0.0
    a chain's terms  m_0 + m_1,  m_0 m_0 + m_1 m_1,  g0_t + g1_t  (t = 0 .. K)
    over the chains  the pooled moments' trees (tests/moment_tree_ref.py: tile_sums, tile_tree)
    stats vector     [M = 2 nchains, n_h, K, then per field: shift, S1, S2, G_0 .. G_maxlag], slots beyond K +0.0

Every addition and product is one IEEE operation of numpy (vectorised over chains and fields only), so a device that does the same operations on
the same operands gives the same bits."""
import math

import numpy as np

from moment_tree_ref import tile_sums, tile_tree

MAXLAG_MAX = 32
COLUMNS = ("mean", "sd", "rhat", "ess", "mcse", "W", "Bn", "truncated")


def stats_len(nfields, maxlag):
    return 3 + nfields * (maxlag + 4)


def half_terms(x, shift, K):
    """x[n_h][nfields][nc], shift[nfields] -> (m[nfields][nc], g[K + 1][nfields][nc]) of one half."""
    n = x.shape[0]
    y = x - shift[None, :, None]
    s = y[0].copy()
    for i in range(1, n):
        s = s + y[i]
    m = s / float(n)
    z = y - m[None]
    g = np.zeros((K + 1,) + m.shape)
    for t in range(K + 1):
        a = np.zeros_like(m)
        for i in range(n - t):
            a = a + z[i] * z[i + t]
        g[t] = a
    return m, g


def stats_ref(x, maxlag, shift=None):
    """x[ns][nfields][nc] (Engine.samples(layout=1) of the window) -> the stats vector."""
    x = np.asarray(x, dtype=np.float64)
    ns, nf, nc = x.shape
    assert ns >= 4 and 0 <= maxlag <= MAXLAG_MAX
    nh = ns // 2
    K = min(maxlag, nh - 1)
    shift = x[0, :, 0].copy() if shift is None else np.asarray(shift, dtype=np.float64)
    m0, g0 = half_terms(x[:nh], shift, K)
    m1, g1 = half_terms(x[ns - nh:], shift, K)
    terms = np.zeros((nc, nf, maxlag + 3))
    terms[:, :, 0] = (m0 + m1).T
    terms[:, :, 1] = (m0 * m0 + m1 * m1).T
    for t in range(K + 1):
        terms[:, :, 2 + t] = (g0[t] + g1[t]).T
    summed = tile_tree(tile_sums(terms.reshape(nc, nf * (maxlag + 3)))).reshape(nf, maxlag + 3)
    out = np.zeros(stats_len(nf, maxlag))
    out[0], out[1], out[2] = 2.0 * nc, float(nh), float(K)
    per = out[3:].reshape(nf, maxlag + 4)
    per[:, 0] = shift
    per[:, 1:] = summed
    return out


def finish_ref(stats, nfields, maxlag):
    """The finish, per field, in the order include/mcmcx.h states it -> table[nfields][8]."""
    stats = np.asarray(stats, dtype=np.float64)
    M, nh, K = float(stats[0]), float(stats[1]), int(stats[2])
    per = stats[3:].reshape(nfields, maxlag + 4)
    table = np.zeros((nfields, 8))
    cap = 1.0 / math.log10(M * nh)
    with np.errstate(all="ignore"):
        for f in range(nfields):
            shift, S1, S2 = (np.float64(v) for v in per[f, :3])
            G = per[f, 3:].astype(np.float64)
            W = G[0] / np.float64(M * (nh - 1.0))
            Bn = (S2 - S1 * S1 / M) / (M - 1.0)
            varp = W * (nh - 1.0) / nh + Bn
            rhat = np.sqrt(varp / W)
            rho = [np.float64(1.0)] + [1.0 - (W - G[t] / (M * nh)) / varp for t in range(1, K + 1)]
            total, prev, stopped = np.float64(0.0), None, False
            for k in range((K + 1) // 2):
                P = rho[2 * k] + rho[2 * k + 1]
                if P <= 0.0:
                    stopped = True
                    break
                if prev is not None and P > prev:
                    P = prev
                total = total + P
                prev = P
            tau = -1.0 + 2.0 * total
            if tau < cap:
                tau = np.float64(cap)
            ess = M * nh / tau if (K + 1) // 2 > 0 else np.float64(np.nan)
            sd = np.sqrt(varp)
            table[f] = (shift + S1 / M, sd, rhat, ess, sd / np.sqrt(ess), W, Bn, 0.0 if stopped else 1.0)
    return table


def summary_ref(x, maxlag, shift=None):
    x = np.asarray(x, dtype=np.float64)
    return finish_ref(stats_ref(x, maxlag, shift), x.shape[1], maxlag)
