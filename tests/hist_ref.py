"""The definition of the sample store's histograms (include/mcmcx.h), restated in numpy.

Everything is in the key order of tests/quant_ref.py (`key`): the IEEE order on doubles that are no NaN, -0.0 below +0.0, negative NaNs
below everything, positive NaNs above.  A field has nbins + 1 edges, non-decreasing by key; cell(x) is the number of edges e_i with
key(e_i) <= key(x): np.searchsorted(edge_keys, keys, side="right"), 0 .. nbins + 1.  The 1-D table counts a field's window values per cell,
the 2-D table the window's (sample, chain) points per pair of cells of two fields.  Uniform edges and the density are plain IEEE doubles."""
import numpy as np

from quant_ref import key


def cells(values, edges):
    """int64 cells of `values` (any shape) among one field's edges[nbins + 1]."""
    ek = key(np.asarray(edges, dtype=np.float64))
    v = np.asarray(values, dtype=np.float64)
    return np.searchsorted(ek, key(v).ravel(), side="right").reshape(v.shape).astype(np.int64)


def cells_loop(values, edges):
    """The same by the definition's own words: for every value, count the edges whose key is not above its key."""
    ek = [int(k) for k in key(np.asarray(edges, dtype=np.float64))]
    return np.array([sum(1 for e in ek if e <= int(k)) for k in key(np.asarray(values, dtype=np.float64).ravel())], dtype=np.int64)


def edges_ok(edges):
    """No NaN, non-decreasing by key within every row of edges[nfields][nbins + 1]."""
    e = np.atleast_2d(np.asarray(edges, dtype=np.float64))
    k = key(e)
    return bool(not np.isnan(e).any() and np.all(k[:, 1:] >= k[:, :-1]))


def hist_ref(X, edges):
    """X[ns][nfields][nc], edges[nfields][nbins + 1] -> int64 [nfields][nbins + 2]."""
    X = np.asarray(X, dtype=np.float64)
    edges = np.asarray(edges, dtype=np.float64)
    nb = edges.shape[1] - 1
    out = np.zeros((X.shape[1], nb + 2), dtype=np.int64)
    for f in range(X.shape[1]):
        out[f] = np.bincount(cells(X[:, f, :], edges[f]).ravel(), minlength=nb + 2)
    return out


def hist2_ref(X, pairs, edges):
    """-> int64 [npairs][nbins + 2][nbins + 2], [a][b] = points with field j in cell a and field k in cell b."""
    X = np.asarray(X, dtype=np.float64)
    edges = np.asarray(edges, dtype=np.float64)
    nc = edges.shape[1] + 1
    out = np.zeros((len(pairs), nc, nc), dtype=np.int64)
    for p, (j, k) in enumerate(pairs):
        a, b = cells(X[:, j, :], edges[j]).ravel(), cells(X[:, k, :], edges[k]).ravel()
        out[p] = np.bincount(a * nc + b, minlength=nc * nc).reshape(nc, nc)
    return out


def uniform_edges_ref(lo, hi, nbins):
    """e_i = lo + (hi - lo) * (i / nbins) for i < nbins, e_nbins = hi: one IEEE operation each."""
    lo, hi = np.float64(lo), np.float64(hi)
    t = np.arange(nbins, dtype=np.float64) / np.float64(nbins)
    return np.concatenate([lo + (hi - lo) * t, [hi]])


def density_ref(counts, edges):
    """counts[nfields][nbins + 2], edges[nfields][nbins + 1] -> [nfields][nbins]: count_b / (n (e_b - e_{b-1})), n the sum of all cells."""
    c = np.asarray(counts, dtype=np.int64)
    e = np.asarray(edges, dtype=np.float64)
    n = c.sum(axis=1).astype(np.float64)[:, None]
    with np.errstate(divide="ignore", invalid="ignore"):
        return c[:, 1:-1].astype(np.float64) / (n * (e[:, 1:] - e[:, :-1]))
