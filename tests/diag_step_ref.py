"""The summary of a step function of a window of retained samples (mcmcx_samples_stats_step) and the table of normal scores
(mcmcx_samples_rank_scores), restated from their definitions in include/mcmcx.h:

    u_f(x) = table[f][cell_f(x)],  cell_f(x) = the number of edges of field f whose key is not above x's      (tests/hist_ref.py: cells)

then the summary's own stats vector (tests/diag_ref.py) of u in place of every stored x; shift = None is u_f of field f of chain 0 in
window sample 0.  The scores, per field, with n the sum of the cells and before_b the sum of the cells below b, in Python integers:

    count_b > 0:  p = ((2 before_b + count_b + 1) * 0.5 - 0.375) / (n + 0.25),  score = Phi^-1(p)            empty cell: +0.0

with statistics.NormalDist().inv_cdf for Phi^-1 (the standard library's AS241).  rank_summary_ref composes the rank-normalised table of
Engine.samples_summary(rank=True) from these and the other restatements."""
from statistics import NormalDist

import numpy as np

import diag_ref
import hist_ref
import quant_ref

_INV = NormalDist().inv_cdf


def u_ref(X, edges, table):
    """X[ns][nfields][nc], edges[nfields][nbins + 1], table[nfields][nbins + 2] -> u(X), the same shape."""
    X = np.asarray(X, dtype=np.float64)
    edges, table = np.asarray(edges, dtype=np.float64), np.asarray(table, dtype=np.float64)
    assert edges.shape[0] == X.shape[1] and table.shape == (X.shape[1], edges.shape[1] + 1)
    u = np.empty_like(X)
    for f in range(X.shape[1]):
        u[:, f, :] = table[f][hist_ref.cells(X[:, f, :], edges[f])]
    return u


def u_loop(X, edges, table):
    """The same value by value, by the definition's own words."""
    X = np.asarray(X, dtype=np.float64)
    u = np.empty_like(X)
    for f in range(X.shape[1]):
        c = hist_ref.cells_loop(X[:, f, :], edges[f]).reshape(X[:, f, :].shape)
        for i in range(X.shape[0]):
            for k in range(X.shape[2]):
                u[i, f, k] = table[f][c[i, k]]
    return u


def stats_ref(X, edges, table, maxlag, shift=None):
    with np.errstate(all="ignore"):
        return diag_ref.stats_ref(u_ref(X, edges, table), maxlag, shift)


def summary_ref(X, edges, table, maxlag, shift=None):
    X = np.asarray(X, dtype=np.float64)
    return diag_ref.finish_ref(stats_ref(X, edges, table, maxlag, shift), X.shape[1], maxlag)


def rank_p(counts):
    """[nfields][nbins + 2] float64: p of every cell that is not empty, NaN for an empty one."""
    c = np.asarray(counts, dtype=np.int64)
    p = np.full(c.shape, np.nan)
    for f in range(c.shape[0]):
        n, before = int(c[f].sum()), 0
        for b in range(c.shape[1]):
            k = int(c[f, b])
            if k > 0:
                p[f, b] = (float(2 * before + k + 1) * 0.5 - 0.375) / (float(n) + 0.25)
            before += k
    return p


def rank_scores_ref(counts):
    p = rank_p(counts)
    return np.array([[0.0 if np.isnan(v) else _INV(float(v)) for v in row] for row in p]).reshape(p.shape)


def rank_edges_ref(X, cells):
    """edges[nfields][cells - 1]: the values at the 0-based ranks (k n) // cells of every field's n = ns x nc values in key order."""
    X = np.asarray(X, dtype=np.float64)
    n = X.shape[0] * X.shape[2]
    ranks = [(k * n) // cells for k in range(1, cells)]
    out = np.empty((X.shape[1], cells - 1))
    for f in range(X.shape[1]):
        v = X[:, f, :].ravel()
        out[f] = v[np.argsort(quant_ref.key(v), kind="stable")][ranks]
    return out


def fold_scores_ref(counts, edges, centre, scores=rank_scores_ref):
    """Engine.samples_summary's table of the folded values |x - centre| over the cells of x (mcmcf90_amd.engine.samples_fold_scores)."""
    c, e = np.asarray(counts, dtype=np.int64), np.asarray(edges, dtype=np.float64)
    out = np.zeros(c.shape)
    with np.errstate(all="ignore"):
        for f in range(c.shape[0]):
            pos = np.concatenate([e[f, :1], (e[f, :-1] + e[f, 1:]) * 0.5, e[f, -1:]])
            uniq, inv = np.unique(np.fabs(pos - centre[f]), return_inverse=True)
            group = np.zeros(max(uniq.size, 3), dtype=np.int64)
            np.add.at(group, inv, c[f])
            out[f] = scores(group[None, :])[0][inv]
    return out


def rank_summary_ref(X, maxlag, cells=128, scores=rank_scores_ref):
    """dict(rhat_rank, ess_bulk_rank, truncated_rank, rhat_max) of X[ns][nfields][nc], composed as Engine.samples_summary(rank=True)
    composes it.  `scores`: the table of normal scores (the library's, where its last bits are to be the composition's)."""
    X = np.asarray(X, dtype=np.float64)
    nf = X.shape[1]
    edges = rank_edges_ref(X, cells)
    counts = hist_ref.hist_ref(X, edges)
    zero = np.zeros(nf)
    r = summary_ref(X, edges, scores(counts), maxlag, zero)
    med = quant_ref.quantiles_ref(X, [0.5])[:, 0]
    rf = summary_ref(X, edges, fold_scores_ref(counts, edges, med, scores), maxlag, zero)
    with np.errstate(all="ignore"):
        return dict(rhat_rank=r[:, 2].copy(), ess_bulk_rank=r[:, 3].copy(), truncated_rank=r[:, 7].copy(),
                    rhat_max=np.maximum(r[:, 2], rf[:, 2]))


def exact_rank_summary_ref(X, maxlag):
    """The exact rank-normalised table: scipy's average ranks of all ns x nc values of a field, Blom's form, scipy's Phi^-1."""
    from scipy.special import ndtri
    from scipy.stats import rankdata
    X = np.asarray(X, dtype=np.float64)
    Z = np.empty_like(X)
    for f in range(X.shape[1]):
        v = X[:, f, :]
        Z[:, f, :] = ndtri((rankdata(v.ravel(), method="average").reshape(v.shape) - 0.375) / (v.size + 0.25))
    return diag_ref.summary_ref(Z, maxlag, np.zeros(X.shape[1]))
