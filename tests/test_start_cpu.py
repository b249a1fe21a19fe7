"""tests/start_ref.py, the restatement of the drawn start points (mcmcx_set_par0_spread), checked on the CPU: against scalar loops written
here from the definition in include/mcmcx.h (a Philox4x32-10 in Python integers, the polar method with the oracle's pinned logarithm, an
exactly rounded fma through rational arithmetic), the stream's separation from the sampling stream, sharding invariance, the retry rule,
the fallback and the distribution."""
import ctypes as C
import math
from fractions import Fraction

import numpy as np

import start_ref as sr


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


# ---------------------------------------------------------------- scalar loops
def _philox(ctr0, ctr1, k0, k1):
    M = 0xFFFFFFFF
    c0, c1, c2, c3 = ctr0, ctr1, 0, 0
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c0, 0xCD9E8D57 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & M, (p0 >> 32) ^ c3 ^ k1, p0 & M
        k0, k1 = (k0 + 0x9E3779B9) & M, (k1 + 0xBB67AE85) & M
    return c0, c1, c2, c3


class _Stream:
    """normal_bm over uniform number n of the stream (seed, chain): mcmcrand.F90:166-190."""

    def __init__(self, oracle, seed, chain, n):
        self.L, self.seed, self.chain, self.n, self.saved = oracle.lib(), seed, chain, n, None

    def uniform(self):
        blk = self.n >> 1
        x = _philox(blk & 0xFFFFFFFF, blk >> 32, self.seed, self.chain)
        b = ((x[3] << 32) | x[2]) if (self.n & 1) else ((x[1] << 32) | x[0])
        self.n += 1
        return float(b >> 11) * 2.0 ** -53

    def normal(self):
        if self.saved is not None:
            y, self.saved = self.saved, None
            return y
        while True:
            x1 = self.uniform(); x2 = self.uniform()
            x1 = 2.0 * x1 - 1.0; x2 = 2.0 * x2 - 1.0
            xx = x1 * x1 + x2 * x2
            if xx < 1.0 and xx != 0.0:
                break
        z = math.sqrt(-2.0 * self.L.mcxo_log(xx) / xx)
        self.saved = z * x1
        return z * x2


def _fma(a, b, c):
    return float(Fraction(a) * Fraction(b) + Fraction(c))          # one rounding (int / int is correctly rounded)


def _scalar_start(oracle, chain, par0, U0, scale, lo, hi, seed=sr.SEED):
    d = len(par0)
    g = _Stream(oracle, seed, chain, 1 << 63)
    for t in range(1, 65):
        z = [g.normal() for _ in range(d)]
        th = []
        for j in range(d):
            acc = 0.0
            for i in range(j + 1):
                acc = _fma(float(U0[i, j]), z[i], acc)
            th.append(float(par0[j]) + (float(scale) * acc))
        if all((lo is None or th[k] > lo[k]) and (hi is None or th[k] < hi[k]) for k in range(d)):
            return np.array(th), t, False
    return np.array(par0, dtype=np.float64), 64, True


def _problem(d, seed=11):
    r = np.random.default_rng(seed)
    A = r.standard_normal((d, d)) / np.sqrt(d)
    return np.linspace(-0.3, 0.4, d), A @ A.T + 0.5 * np.eye(d)


# ---------------------------------------------------------------- tests
def test_the_factor_is_dpotf2_times_the_am_scale(oracle):
    par0, cm = _problem(6)
    U0 = sr.initial_factor(oracle, cm)
    assert np.array_equal(U0, np.triu(U0)) and np.allclose(U0.T @ U0, cm * 2.4 ** 2 / 6, rtol=1e-13)
    ref = np.linalg.cholesky(cm).T * 2.4 / math.sqrt(6.0)
    assert np.allclose(U0, ref, rtol=1e-13)
    bad = cm.copy(); bad[3, 3] = -1.0
    assert sr.initial_factor(oracle, bad) is None


def test_restatement_equals_scalar_loops(oracle):
    for d, scale, box in ((1, 1.0, None), (5, 0.7, None), (7, math.sqrt(7.0) / 2.4, 1.0), (12, 2.0, 1.2)):
        par0, cm = _problem(d)
        sd = np.sqrt(np.diag(cm))
        lo, hi = (None, None) if box is None else (par0 - box * sd, par0 + box * sd)
        th, tries, fell = sr.starts(oracle, 9, par0, cm, scale, lo, hi, chain_id0=6)
        U0 = sr.initial_factor(oracle, cm)
        for c in range(9):
            w, t, f = _scalar_start(oracle, 6 + c, par0, U0, scale, lo, hi)
            assert (_bits(th[c]) == _bits(w)).all() and tries[c] == t and fell[c] == f, (d, c)
        if box is not None:                                    # npar 7: redraws, no fallback; npar 12 at twice the proposal's scale: both
            assert (tries > 1).any() and (fell.any() == (d == 12)) and (d != 12 or not fell.all())


def test_start_stream_is_not_the_sampling_stream(oracle):
    L = oracle.lib()
    d = 6
    for chain in (0, 6, 588):
        g, s = sr.start_rng(oracle, chain), oracle.Rng()
        s.key[0], s.key[1], s.n, s.saved, s.saved_y = sr.SEED, chain, 0, 0, 0.0
        a = [L.mcxo_normal(C.byref(g)) for _ in range(2 * d)]
        b = [L.mcxo_normal(C.byref(s)) for _ in range(2 * d)]
        assert g.n >= (1 << 63) + 2 * d and s.n < (1 << 32) and not set(a) & set(b)
        assert (g.key[0], g.key[1]) == (s.key[0], s.key[1])          # the same key: no new stream, a far position of the chain's own


def test_starts_do_not_depend_on_the_sharding(oracle):
    par0, cm = _problem(5)
    sd = np.sqrt(np.diag(cm))
    kw = dict(par0=par0, cmat0=cm, scale=1.3, lo=par0 - 1.5 * sd, hi=par0 + 1.5 * sd)
    N = 20
    th, tr, fl = sr.starts(oracle, N, chain_id0=0, **kw)
    a, b = sr.starts(oracle, N // 2, chain_id0=0, **kw), sr.starts(oracle, N // 2, chain_id0=N // 2, **kw)
    assert (_bits(th) == _bits(np.vstack([a[0], b[0]]))).all()
    assert (tr == np.concatenate([a[1], b[1]])).all() and (fl == np.concatenate([a[2], b[2]])).all()
    assert len(np.unique(th[:, 0])) == N and (tr > 1).any()


def test_retry_rule_counts_match_a_plain_loop(oracle):
    """A half space through par0 rejects about half the attempts: tries is geometric, and the counts are those of a loop that takes the
    stream's normals npar at a time."""
    L = oracle.lib()
    d, N = 3, 200
    par0, cm = _problem(d)
    hi = np.array([par0[0], np.inf, np.inf])
    th, tries, fell = sr.starts(oracle, N, par0, cm, 1.0, None, hi, chain_id0=3)
    U0f = np.asfortranarray(sr.initial_factor(oracle, cm))
    for c in range(N):
        g, n = sr.start_rng(oracle, 3 + c), 0
        while True:
            n += 1
            x = np.array([L.mcxo_normal(C.byref(g)) for _ in range(d)])
            L.mcxo_trmv_ut(d, U0f.ctypes.data_as(oracle._DP), x.ctypes.data_as(oracle._DP))
            cand = par0 + 1.0 * x
            if cand[0] < hi[0]:
                break
        assert n == tries[c] and (_bits(cand) == _bits(th[c])).all()
    assert not fell.any() and 0.35 < (tries == 1).mean() < 0.65 and tries.max() >= 4
    assert sr.info(tries, fell) == (int((tries > 1).sum()), 0)


def test_fallback_is_par0_bit_for_bit(oracle):
    d = 4
    par0, cm = _problem(d)
    par0[2] = -0.0                                             # the sign of a zero is par0's too
    lo, hi = np.full(d, -10.0), np.full(d, 10.0)
    lo[1], hi[1] = 1.0, -1.0                                   # lo > hi in one component: no attempt can meet it
    th, tries, fell = sr.starts(oracle, 5, par0, cm, 1.0, lo, hi)
    assert fell.all() and (tries == sr.TRIES).all() and sr.TRIES == 64
    assert (_bits(th) == _bits(np.tile(par0, (5, 1)))).all()
    assert sr.info(tries, fell) == (5, 5)


def test_moments_of_20000_starts(oracle):
    """N(par0, scale**2 U0'U0): the sample mean within 5 standard errors per component, every covariance entry within 5 standard errors
    (var of a sample covariance entry of a Gaussian: (S_ii S_jj + S_ij**2) / (n - 1)); scale = sqrt(npar) / 2.4 makes that cmat0."""
    d, N = 3, 20000
    par0, cm = _problem(d)
    scale = math.sqrt(float(d)) / 2.4
    th, tries, fell = sr.starts(oracle, N, par0, cm, scale)
    assert (tries == 1).all() and not fell.any()
    U0 = sr.initial_factor(oracle, cm)
    S = scale ** 2 * (U0.T @ U0)
    assert np.allclose(S, cm, rtol=1e-12)
    se_mean = np.sqrt(np.diag(S) / N)
    assert (np.abs(th.mean(axis=0) - par0) < 5.0 * se_mean).all(), (th.mean(axis=0) - par0) / se_mean
    Sh = np.cov(th.T)
    se_cov = np.sqrt((np.outer(np.diag(S), np.diag(S)) + S ** 2) / (N - 1))
    assert (np.abs(Sh - S) < 5.0 * se_cov).all(), (Sh - S) / se_cov
