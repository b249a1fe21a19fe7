"""The definition of the sample store's order statistics, counts and quantiles (include/mcmcx.h), restated in numpy.

Key: with b the double's bits, key(x) = b ^ (b >> 63 ? 0xFFFFFFFFFFFFFFFF : 0x8000000000000000); the unsigned order of the keys is the total
order (negative NaNs < -inf < ... < -0.0 < +0.0 < ... < +inf < positive NaNs).  os(r) is the value whose key is the r-th smallest of the
window's keys, with its own bits; lt(x) / le(x) count the keys below / not above key(x).  The quantile is Hyndman-Fan type 7:
pos = p (n - 1), lo = floor(pos), hi = min(lo + 1, n - 1), g = pos - lo, q = a if a and b have equal bits else a + (b - a) g."""
import numpy as np

SIGN = np.uint64(0x8000000000000000)
ONES = np.uint64(0xFFFFFFFFFFFFFFFF)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def key(x):
    """uint64 keys of an array of doubles."""
    b = bits(x)
    return b ^ np.where((b >> np.uint64(63)) != 0, ONES, SIGN)


def unkey(k):
    """The doubles (as float64) whose keys are k."""
    k = np.ascontiguousarray(k, dtype=np.uint64)
    return (k ^ np.where((k >> np.uint64(63)) != 0, SIGN, ONES)).view(np.float64)


def sorted_keys(X):
    """X[ns][nfields][nc] -> per field the window's n = ns * nc keys, ascending: [nfields][n] uint64."""
    X = np.asarray(X, dtype=np.float64)
    k = key(np.ascontiguousarray(np.moveaxis(X, 1, 0)).reshape(X.shape[1], -1))
    return np.sort(k, axis=1)


def order_stats_ref(X, ranks):
    """[nfields][nr] float64 with the values' own bits."""
    sk = sorted_keys(X)
    return unkey(np.ascontiguousarray(sk[:, np.asarray(ranks, dtype=np.int64)]))


def order_stats_1d(values, ranks):
    sk = np.sort(key(np.asarray(values, dtype=np.float64)))
    return unkey(np.ascontiguousarray(sk[np.asarray(ranks, dtype=np.int64)]))


def counts_ref(X, x):
    """x[nfields][nq] -> int64 [nfields][nq][2] = lt, le."""
    sk = sorted_keys(X)
    kx = key(np.asarray(x, dtype=np.float64))
    out = np.zeros(kx.shape + (2,), dtype=np.int64)
    for f in range(sk.shape[0]):
        out[f, :, 0] = np.searchsorted(sk[f], kx[f], side="left")
        out[f, :, 1] = np.searchsorted(sk[f], kx[f], side="right")
    return out


def quantile_ranks_ref(n, probs):
    """(ranks[nq][2] int64, frac[nq]) in IEEE doubles: pos = p * float(n - 1)."""
    p = np.asarray(probs, dtype=np.float64).ravel()
    pos = p * np.float64(n - 1)
    fl = np.floor(pos)
    lo = fl.astype(np.int64)
    return np.stack([lo, np.minimum(lo + 1, n - 1)], axis=1), pos - fl


def finish_ref(a, b, g):
    """q = a where a and b have equal bits, else a + (b - a) * g (elementwise, plain IEEE)."""
    a, b, g = (np.asarray(v, dtype=np.float64) for v in (a, b, g))
    with np.errstate(invalid="ignore", over="ignore"):
        lerp = a + (b - a) * g
    return np.where(bits(a) == bits(b), a, lerp)


def quantiles_ref(X, probs):
    """[nfields][nq] from the window X[ns][nfields][nc]."""
    X = np.asarray(X, dtype=np.float64)
    n = X.shape[0] * X.shape[2]
    ranks, frac = quantile_ranks_ref(n, probs)
    os_ = order_stats_ref(X, ranks.ravel()).reshape(X.shape[1], -1, 2)
    return finish_ref(os_[:, :, 0], os_[:, :, 1], frac[None, :])
