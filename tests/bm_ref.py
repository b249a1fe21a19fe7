"""The sample store's batch-means vector (mcmcx_samples_cov_bm) and its two finishes (mcmcx_samples_mess, mcmcx_samples_mpsrf) restated from
include/mcmcx.h's definition, independent of the library:

    z = x_f - shift_f                                           (shift None: field f of chain 0 in window sample 0)
    per chain, field and batch k of `batch` consecutive samples:   y = (..((z_0 + z_1) + z_2)..) / batch, the sum starting at z_0
    then tests/cov_ref.py's tile sums, fma chains and tree on y[nb][nf][nchains]; the last ns - nb batch samples are not read
    vector: [nb * nchains, shift[nf], S[nf], G packed by rows of the upper triangle]

The finishes are written with the header's loops: the upper Cholesky factor column by column, sums ascending, no fma."""
import numpy as np

import cov_ref
from moment_tree_ref import tile_tree


def batch_means(X, batch, shift=None):
    """(y[nb][nf][nchains], shift[nf]): a sequential sum per lane starting at z_0, then one division"""
    z, sh = cov_ref.shifted(X, shift)
    ns = z.shape[0]
    nb = ns // batch
    y = np.empty((nb,) + z.shape[1:])
    for k in range(nb):
        s = z[k * batch].copy()
        for i in range(1, batch):
            s = s + z[k * batch + i]
        y[k] = s / float(batch)
    return y, sh


def bm_vector_ref(X, batch, shift=None, pairs=None):
    """The batch-means vector of X[ns][nf][nchains]; with pairs = (J, K) only those entries of G are computed (cov_ref.cov_vector_ref's rule)."""
    with np.errstate(all="ignore"):
        y, sh = batch_means(X, batch, shift)
        nb, nf, nch = y.shape
        out = np.zeros(cov_ref.vec_len(nf))
        out[0] = float(nb * nch)
        out[1:1 + nf] = sh
        out[1 + nf:1 + 2 * nf] = tile_tree(cov_ref.tile_S(y))
        J, K = cov_ref.all_pairs(nf) if pairs is None else pairs
        g = tile_tree(cov_ref.tile_G(y, np.asarray(J), np.asarray(K)))
        out[1 + 2 * nf + cov_ref.pair_index(np.asarray(J), np.asarray(K), nf)] = g
    return out


def longdouble_ref(X, batch, shift=None):
    """(S, G packed, bound_S, bound_G) of the batch means in np.longdouble, the means themselves formed in longdouble too.  The bound: a
    mean carries (batch) roundings, relative error at most batch u of sum|z| / batch =: a; the sums over n_b terms add 2 n_b u sum|terms| as in
    cov_ref.longdouble_ref -- together, to first order and doubled for the products, (2 n_b + 2 batch + 2) u sum a_j a_k, a_j = mean|z_j|."""
    z, _ = cov_ref.shifted(X, shift)
    ns, nf, nch = z.shape
    nb = ns // batch
    zl = z[:nb * batch].astype(np.longdouble).reshape(nb, batch, nf, nch)
    y = zl.sum(axis=1) / np.longdouble(batch)
    a = np.abs(zl).sum(axis=1) / np.longdouble(batch)
    n = nb * nch
    yl = y.transpose(1, 0, 2).reshape(nf, n)
    al = a.transpose(1, 0, 2).reshape(nf, n)
    J, K = cov_ref.all_pairs(nf)
    c = (2.0 * n + 2.0 * batch + 2.0) * cov_ref.U
    return yl.sum(axis=1), (yl @ yl.T)[J, K], c * al.sum(axis=1), c * (al @ al.T)[J, K]


# ---------------------------------------------------------------- the finishes
def _moment(vec, nf, sel, den):
    """A[sel, sel], A_jk = (G_jk - S_j S_k / n) / den"""
    vec = np.asarray(vec, dtype=np.float64)
    n, S, G = vec[0], vec[1 + nf:1 + 2 * nf], vec[1 + 2 * nf:]
    m = len(sel)
    A = np.zeros((m, m))
    with np.errstate(all="ignore"):
        for a in range(m):
            for b in range(m):
                j, k = min(sel[a], sel[b]), max(sel[a], sel[b])
                A[a, b] = (G[cov_ref.pair_index(j, k, nf)] - S[j] * S[k] / n) / den
    return A


def chol_ref(A):
    """(R, ok): the header's loop; ok False at the first pivot that is not > 0"""
    m = A.shape[0]
    R = np.zeros((m, m))
    with np.errstate(all="ignore"):
        for j in range(m):
            for i in range(j):
                t = 0.0
                for k in range(i):
                    t = t + R[k, i] * R[k, j]
                R[i, j] = (A[i, j] - t) / R[i, i]
            t = 0.0
            for k in range(j):
                t = t + R[k, j] * R[k, j]
            p = A[j, j] - t
            if not (p > 0.0):
                return R, False
            R[j, j] = np.sqrt(p)
    return R, True


def logdet_ref(A):
    R, ok = chol_ref(A)
    if not ok:
        return np.nan
    s = 0.0
    for j in range(A.shape[0]):
        s = s + np.log(R[j, j])
    return 2.0 * s


def mess_ref(cov_vec, bm_vec, nf, batch, sel):
    """(warn, out4 = [mess, n, logdet Lambda, logdet Sigma], ess[nsel])"""
    n = cov_vec[0]
    with np.errstate(all="ignore"):
        L = _moment(cov_vec, nf, sel, n - 1.0)
        Sg = float(batch) * _moment(bm_vec, nf, sel, bm_vec[0] - 1.0)
        ess = n * np.diag(L) / np.diag(Sg)
        ldl, lds = logdet_ref(L), logdet_ref(Sg)
        mess = n * np.exp((ldl - lds) / float(len(sel)))
    return int(np.isnan(ldl) or np.isnan(lds)), np.array([mess, n, ldl, lds]), ess


def mpsrf_ref(cov_vec, bm_vec, nf, n_h, sel):
    """(warn, out4 = [mpsrf, lambda1, M, n_h], W, Bn); lambda1 from numpy's symmetric eigensolver on R^-T Bn R^-1"""
    M, nh = bm_vec[0], float(n_h)
    with np.errstate(all="ignore"):
        T, SSm = _moment(cov_vec, nf, sel, 1.0), _moment(bm_vec, nf, sel, 1.0)
        W = (T - nh * SSm) / (M * (nh - 1.0))
        Bn = SSm / (M - 1.0)
        R, ok = chol_ref(W)
        if not ok or not (np.isfinite(Bn).all() and np.isfinite(R).all()):
            return 1, np.array([np.nan, np.nan, M, nh]), W, Bn
        Ri = np.linalg.inv(R)
        Cm = Ri.T @ Bn @ Ri
        l1 = np.linalg.eigvalsh((Cm + Cm.T) / 2.0)[-1]
        return 0, np.array([np.sqrt((nh - 1.0) / nh + l1), l1, M, nh]), W, Bn
