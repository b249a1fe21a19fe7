"""Gaussian problems whose sums of squares leave the comfortable range: +inf and NaN (overflow), an infinite sigma2, subnormal values.

No new target: the built-in ss = v' Lam v (oracle/mcx_targets.h, mcxt_ss_gauss) reaches all three by scaling.  With Lam = s Lam0 and sigma2 = s
the acceptance ratio keeps its O(1) size while ss itself is s times larger (or smaller).  Everything here is a function of its arguments and of
fixed seeds, so the CPU tests (the oracle against the reference) and the GPU tests (the engine against the oracle) run the very same inputs.

overflow(d, T, c)   s = M / T with M = 1.797e308: ss = +inf wherever v' Lam0 v > T.  Lam0 is tests/test_gpu_every_chain.py's A A' + I with rows and
                    columns 0 and 1 replaced by the block [[a, -b], [-b, a]], a = 0.9 T, b = 0.95 a (every entry of s Lam0 stays finite).  Rows 0
                    and 1 fall into different partial chains of mcxt_ss_gauss: a proposal with v0 - v1 > 1.2 or so has y_0 = +inf and y_1 = -inf
                    and ss = inf + (-inf) = NaN, although the exact value is finite.  cmat0 = c inv(Lam0), symmetrised, its leading block blk I
                    (T moves the share of +inf, blk the share of NaN: the pair's threshold does not depend on T).
overflow_ar1(d, T, c)   the same scaling without the pair block: Lam0 = inv(0.9**|i-j|), cmat0 = c (0.7 S + 0.3 I).  Rows of either sign
                    overflow in one proposal, so NaN appears here too.
subnormal(d, t)     the plain problem of tests/test_gpu_every_chain.py with Lam = t Lam0, sigma2 = t, t = 2**-1030 or 2**-1060: every ss is a
                    non-zero subnormal, the acceptance rate is what it is at t = 1; a kernel that flushes denormals sees ss = 0 and accepts all.
An infinite sigma2 is overflow_ar1 with updatesigma = 1, N0 = 1, S02 = 1e307 (INF_SIGMA2): the gamma draw overflows in part of the chains and
(ss2 - ss1) / inf is 0 or NaN.
"""
import numpy as np

M = 1.797e308
INF_SIGMA2 = dict(updatesigma=1, N0=1.0, S02=1e307)


def lam0_dense(d):
    """tests/test_gpu_every_chain.py's precision matrix"""
    r = np.random.default_rng(3000 + d)
    A = r.standard_normal((d, d)) / np.sqrt(d)
    return A @ A.T + np.eye(d)


def overflow(d, T, c, blk=0.5):
    s = M / T
    lam0 = lam0_dense(d)
    a = 0.9 * T
    b = 0.95 * a
    lam0[:2, :] = 0.0
    lam0[:, :2] = 0.0
    lam0[:2, :2] = [[a, -b], [-b, a]]
    cmat0 = c * np.linalg.inv(lam0)
    cmat0 = 0.5 * (cmat0 + cmat0.T)
    cmat0[:2, :2] = blk * np.eye(2)
    mu = np.linspace(-0.5, 0.5, d)
    lam = s * lam0
    assert np.isfinite(lam).all()
    return dict(kind="gauss", npar=d, par0=mu + 0.05, cmat0=cmat0, mu=mu, lam=lam, sigma2=s)


def overflow_ar1(d, T, c):
    s = M / T
    S = 0.9 ** np.abs(np.subtract.outer(np.arange(d), np.arange(d)))
    lam = s * np.linalg.inv(S)
    assert np.isfinite(lam).all()
    mu = np.linspace(-0.5, 0.5, d)
    return dict(kind="gauss", npar=d, par0=mu + 0.05, cmat0=c * (0.7 * S + 0.3 * np.eye(d)), mu=mu, lam=lam, sigma2=s)


def subnormal(d, t):
    lam0 = lam0_dense(d)
    return dict(kind="gauss", npar=d, par0=np.full(d, 0.1), cmat0=np.linalg.inv(lam0), mu=np.linspace(-0.5, 0.5, d), lam=t * lam0, sigma2=t)


def is_subnormal(x):
    x = np.abs(np.asarray(x, dtype=np.float64))
    return (x > 0.0) & (x < np.finfo(np.float64).tiny)


def same_bits_or_nan(a, b):
    """Bit for bit, except that a NaN equals a NaN whatever its sign and payload (x86 and gfx950 generate different default NaNs)."""
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return (a.view(np.uint64) == b.view(np.uint64)) | (np.isnan(a) & np.isnan(b))
