"""The summary of an elementwise function of a window of retained samples (mcmcx_samples_stats_of), restated in numpy from its definition
in include/mcmcx.h: the stats vector is the summary's own (tests/diag_ref.py) of u_f(x) in place of every stored x,

    kind 0  IDENTITY  u_f(x) = x
    kind 1  LE        u_f(x) = 1.0 if key(x) <= key(a_f) else +0.0       the key order of tests/quant_ref.py, not the IEEE comparison
    kind 2  FOLD      u_f(x) = fabs(x - a_f)                             one subtraction, then the sign cleared
    kind 3  SQUARE    d = x - a_f;  u_f(x) = d * d                       two operations

and shift = None is u_f of field f of chain 0 in window sample 0.  One IEEE operation per numpy operation."""
import numpy as np

import diag_ref
import quant_ref

IDENTITY, LE, FOLD, SQUARE = 0, 1, 2, 3


def u_ref(X, kind, a):
    """X[ns][nfields][nc], a[nfields] -> u(X), the same shape."""
    X = np.asarray(X, dtype=np.float64)
    if kind == IDENTITY:
        return X.copy()
    a = np.asarray(a, dtype=np.float64).reshape(1, -1, 1)
    assert a.shape[1] == X.shape[1]
    with np.errstate(all="ignore"):
        if kind == LE:
            return np.where(quant_ref.key(X) <= quant_ref.key(a), 1.0, 0.0)
        if kind == FOLD:
            return np.fabs(X - a)
        if kind == SQUARE:
            d = X - a
            return d * d
    raise ValueError(kind)


def stats_ref(X, kind, a, maxlag, shift=None):
    """The stats vector; shift = None is diag_ref's own default applied to u(X), which is u of X[0, :, 0]."""
    with np.errstate(all="ignore"):
        return diag_ref.stats_ref(u_ref(X, kind, a), maxlag, shift)


def summary_ref(X, kind, a, maxlag, shift=None):
    X = np.asarray(X, dtype=np.float64)
    return diag_ref.finish_ref(stats_ref(X, kind, a, maxlag, shift), X.shape[1], maxlag)
