"""A numpy restatement of the Cholesky branch of MCMC_calculate_R -- LAPACK's dpotf2('U'), dtrti2('U','N') and dlauu2('U') as the oracle
(oracle/mcx_oracle.c: mcxo_potrf_u, mcxo_potri_u), the host (host_initial_R, host_potri) and the device forms (calculate_R / potri_packed,
tile_factor_kernel) all state them: every dot product and column sweep one ascending fma chain per element, the pivot test `!(ajj > 0)`,
dpotri's test for an exact zero on the diagonal, and the two zero skips -- dtrmv's `if x(jj) != 0` and dgemv's `if temp != 0`.

The skips are flags here (skip_zeros), so that a test can show a family of matrices on which dropping them changes bits: a zero times a
finite column changes nothing, a zero times an infinity is a NaN.  numpy has no fma; the one rounding primitive comes from libm (scalars)
and from the oracle's mcxo_fma_v (vectors).  Order of operations, skips and tests are this file's own.

Matrices are [i, j] arrays; only the upper triangle is read or written."""
import ctypes as C
import ctypes.util

import numpy as np

_libm = C.CDLL(ctypes.util.find_library("m") or "libm.so.6")
_libm.fma.restype = C.c_double
_libm.fma.argtypes = [C.c_double, C.c_double, C.c_double]
_DP = C.POINTER(C.c_double)
_L = None


def _fma_v(a, b, c):
    """c <- fma(a, b, c) element-wise, in place; a, c contiguous float64 vectors, b a vector or a scalar"""
    global _L
    if _L is None:
        from oracle import pyoracle
        _L = pyoracle.lib()
    n = c.shape[0]
    if n == 0:
        return
    if np.ndim(b) == 0:
        b = np.full(n, b)
    assert a.flags.c_contiguous and b.flags.c_contiguous and c.flags.c_contiguous and a.shape[0] == n and b.shape[0] == n
    _L.mcxo_fma_v(n, a.ctypes.data_as(_DP), b.ctypes.data_as(_DP), c.ctypes.data_as(_DP), c.ctypes.data_as(_DP))


def potrf_u(A):
    """dpotf2('U') in place on a copy: returns (T, info).  On failure at pivot j (info = j + 1) T holds the rows above j, the failed
    pivot's value on the diagonal (as LAPACK leaves it) and A below."""
    T = np.array(A, dtype=np.float64, order="C")
    n = T.shape[0]
    with np.errstate(all="ignore"):
        for j in range(n):
            # t[k - j] = sum_{i < j} T(i, k) T(i, j), ascending i, for k = j .. n - 1 (k = j: the pivot's own ddot)
            t = np.zeros(n - j)
            for i in range(j):
                _fma_v(T[i, j:], T[i, j], t)
            ajj = T[j, j] - t[0]
            if not (ajj > 0.0):
                T[j, j] = ajj
                return T, j + 1
            ajj = np.sqrt(ajj)
            T[j, j] = ajj
            if j < n - 1:
                rinv = 1.0 / ajj
                T[j, j + 1:] = (T[j, j + 1:] - t[1:]) * rinv
    return T, 0


def potri_u(R, skip_zeros=True, skip_trti=None, skip_lauu=None):
    """dpotri('U') = dtrti2 + dlauu2 on a copy: returns (upper triangle of inv(R'R), info); info = j + 1 for an exact zero at (j, j),
    nothing computed.  skip_zeros = False drops both zero skips (skip_trti / skip_lauu: one of them)."""
    st = skip_zeros if skip_trti is None else skip_trti
    sl = skip_zeros if skip_lauu is None else skip_lauu
    n = R.shape[0]
    for j in range(n):
        if R[j, j] == 0.0:
            return np.array(R, dtype=np.float64), j + 1
    # column-major work copy: W[j, i] = element (i, j), so that a column's head W[j, :i] is contiguous
    W = np.array(np.asarray(R, dtype=np.float64).T, order="C")
    with np.errstate(all="ignore"):
        for j in range(n):                                  # dtrti2
            W[j, j] = 1.0 / W[j, j]
            ajj = -W[j, j]
            for jj in range(j):                             # dtrmv('U','N','N') with the inverted leading block
                temp = W[j, jj]
                if temp != 0.0 or not st:
                    _fma_v(W[jj, :jj], temp, W[j, :jj])
                    W[j, jj] = temp * W[jj, jj]
            W[j, :j] = ajj * W[j, :j]
        for i in range(n):                                  # dlauu2
            aii = W[i, i]
            if i < n - 1:
                dot = 0.0
                for k in range(i, n):
                    dot = _libm.fma(W[k, i], W[k, i], dot)
                W[i, :i] = aii * W[i, :i]
                for k in range(i + 1, n):
                    temp = W[k, i]
                    if temp != 0.0 or not sl:
                        _fma_v(W[k, :i], temp, W[i, :i])
                W[i, i] = dot
            else:
                W[i, :i + 1] = aii * W[i, :i + 1]
    return np.triu(W.T), 0


def calculate_R(A, drscale=0.0, skip_zeros=True):
    """The Cholesky branch of MCMC_calculate_R: (R, R2, iC, info, info2) with R = T 2.4 / sqrt(n); R2 = R / drscale and iC = dpotri(R)
    with delayed rejection (None otherwise, or when dpotf2 failed)."""
    n = A.shape[0]
    T, info = potrf_u(A)
    if info != 0:
        return None, None, None, info, 0
    with np.errstate(all="ignore"):
        R = np.triu(T) * 2.4 / np.sqrt(float(n))
        if not drscale > 0.0:
            return R, None, None, 0, 0
        iC, info2 = potri_u(R, skip_zeros)
        return R, R / drscale, (iC if info2 == 0 else None), 0, info2
