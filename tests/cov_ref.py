"""The sample store's cov vector (mcmcx_samples_cov, include/mcmcx.h) restated from its documented definition, independent of the library:

    z_f = x_f - shift_f                                         (shift None: field f of chain 0 in window sample 0)
    per tile of 64 chains, window samples ascending, lanes 0 .. 63 ascending, a lane without a chain skipped:
        s_j  = s_j + z_j                 from +0.0
        g_jk = fma(z_j, z_k, g_jk)       from +0.0,  j <= k
    over the tiles: tests/moment_tree_ref.py's fixed pairwise tree
    vector: [n, shift[nf], S[nf], G packed by rows of the upper triangle]
    finish: mean = shift + S / n;  C = (G - S_j S_k / n) / (n - 1);  corr = C_jk / (sqrt(C_jj) sqrt(C_kk)), 1.0 on a positive diagonal

The fma is libm's through ctypes (as tests/test_gpu_pooled.py takes it), vectorised with np.frompyfunc over [tiles, pairs] for each step
(sample, lane) of the chain: about 1e6 fma per second, so callers keep padded lanes x ns x pairs near 1e6.  Everything else is one IEEE
operation per numpy operation."""
import ctypes as C

import numpy as np

from moment_tree_ref import tile_tree

_libm = C.CDLL("libm.so.6")
_libm.fma.restype = C.c_double
_libm.fma.argtypes = [C.c_double, C.c_double, C.c_double]
_fma = np.frompyfunc(lambda a, b, c: _libm.fma(a, b, c), 3, 1)
U = 2.0 ** -53


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def vec_len(nf):
    return 1 + 2 * nf + nf * (nf + 1) // 2


def pair_index(j, k, nf):
    """Where pair j <= k sits in the packed upper triangle."""
    return j * nf - j * (j - 1) // 2 + (k - j)


def all_pairs(nf):
    """(J, K): the pairs j <= k in packed order."""
    J, K = np.triu_indices(nf)
    return J, K


def shifted(X, shift=None):
    """(z[ns][nf][nchains], shift[nf])"""
    X = np.asarray(X, dtype=np.float64)
    sh = X[0, :, 0].copy() if shift is None else np.asarray(shift, dtype=np.float64).copy()
    return X - sh[None, :, None], sh


def _tiles(z):
    """[ns][nf][T][64] and the mask [T][64] of the lanes that hold a chain"""
    ns, nf, nch = z.shape
    T = (nch + 63) // 64
    zp = np.zeros((ns, nf, T * 64))
    zp[:, :, :nch] = z
    return zp.reshape(ns, nf, T, 64), (np.arange(T * 64) < nch).reshape(T, 64), T


def tile_S(z):
    """[T][nf]: the running sum of every tile"""
    zt, m, T = _tiles(z)
    ns, nf = z.shape[:2]
    s = np.zeros((T, nf))
    for w in range(ns):
        for c in range(64):
            on = m[:, c]
            if on.any():
                s[on] = s[on] + zt[w][:, :, c][:, on].T                             # [tiles on][nf]
    return s


def tile_G(z, J, K):
    """[T][len(J)]: the fma chain of every tile for the pairs (J[p], K[p])"""
    zt, m, T = _tiles(z)
    ns = z.shape[0]
    g = np.zeros((T, len(J)))
    for w in range(ns):
        for c in range(64):
            on = m[:, c]
            if on.any():
                zw = zt[w][:, :, c][:, on]                                          # [nf][tiles on]
                a, b = zw[J].T, zw[K].T                                             # [tiles on][pairs]
                g[on] = _fma(a, b, g[on]).astype(np.float64)
    return g


def cov_vector_ref(X, shift=None, pairs=None):
    """The vector of X[ns][nf][nchains]; with pairs = (J, K) only those entries of G are computed, the others are NaN-free zeros the
    caller must not compare."""
    with np.errstate(all="ignore"):                             # inf - inf and the like are the caller's data
        z, sh = shifted(X, shift)
        ns, nf, nch = z.shape
        out = np.zeros(vec_len(nf))
        out[0] = float(ns * nch)
        out[1:1 + nf] = sh
        out[1 + nf:1 + 2 * nf] = tile_tree(tile_S(z))
        J, K = all_pairs(nf) if pairs is None else pairs
        g = tile_tree(tile_G(z, np.asarray(J), np.asarray(K)))
        out[1 + 2 * nf + pair_index(np.asarray(J), np.asarray(K), nf)] = g
    return out


def finish_ref(vec, nf):
    """(mean[nf], cov[nf][nf], corr[nf][nf]) of a vector; raises ValueError where mcmcx_samples_cov_finish refuses"""
    vec = np.asarray(vec, dtype=np.float64)
    n = vec[0]
    if not (n >= 2.0) or n != np.floor(n):
        raise ValueError("n")
    sh, S, G = vec[1:1 + nf], vec[1 + nf:1 + 2 * nf], vec[1 + 2 * nf:]
    with np.errstate(all="ignore"):
        mean = sh + S / n
        cov = np.zeros((nf, nf))
        J, K = all_pairs(nf)
        c = (G - S[J] * S[K] / n) / (n - 1.0)
        cov[J, K] = c
        cov[K, J] = c
        d = np.sqrt(np.diag(cov))
        corr = cov / (d[:, None] * d[None, :])
        dd = np.diag(cov)
        corr[np.arange(nf), np.arange(nf)] = np.where(dd > 0.0, 1.0, np.diag(corr))
    return mean, cov, corr


def longdouble_ref(X, shift=None):
    """(S, G packed, bound_S, bound_G): np.longdouble accumulation of z_j and z_j z_k over the whole window, and the forward bound of any
    summation order, 2 n u sum|terms|."""
    z, _ = shifted(X, shift)
    ns, nf, nch = z.shape
    n = ns * nch
    zl = z.transpose(1, 0, 2).reshape(nf, n).astype(np.longdouble)
    J, K = all_pairs(nf)
    with np.errstate(all="ignore"):
        S = zl.sum(axis=1)
        G = (zl @ zl.T)[J, K]
        aS = np.abs(zl).sum(axis=1)
        aG = (np.abs(zl) @ np.abs(zl).T)[J, K]
    return S, G, 2.0 * n * U * aS, 2.0 * n * U * aG
