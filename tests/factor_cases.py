"""Edge covariances for the Cholesky branch of MCMC_calculate_R (dpotf2, the scaling, dpotri) in its four statements: the host's
(host_initial_R / host_potri), the lane form (calculate_R / potri_packed in adapt_post_kernel), tile_factor_kernel, and potri_packed on
an SVD factor -- reached through mcmcx_debug_host_calculate_R and mcmcx_debug_calculate_R.

cases(d) is an ordered dict name -> (matrix, info): svd_cases' families (info None: whatever the oracle says) and constructed ones whose
outcome follows from the construction -- info is dpotf2's: 0, or k + 1 for a failure placed at the 0-based pivot k:

    neg_at(k)        dense with A[k, k] = -1: the pivot is negative whatever was subtracted
    zero_at(k)       dense with row and column k zeroed: the pivot is exactly +0 (0 - sum of 0 * 0)
    negzero_at(k)    diag(1, .., -0.0 at k, .., 1): the pivot is -0.0 - 0
    nan_diag(k)      dense with A[k, k] = NaN
    nan_off(i, k)    dense with A[i, k] = A[k, i] = NaN, i < k (i = k // 2): row i of the factor carries it to pivot k, the first it reaches
    inf_diag(k)      dense with A[k, k] = +inf: succeeds -- the pivot is +inf, 1 / sqrt is 0, row k of the factor is zeros
    diagonal         diag(10**linspace(-150, 150, d)): every off-diagonal an exact zero, every zero skip taken
    subn             dense * 1e-310: subnormal entries, the inverse overflows
    zero_meets_inf   (d >= 4) blocks S1, S2, one column c, an identity: S1 and S2 are dense * 1e-316, so the inverted factor holds
                     1e158s there; c is coupled to S1 only (1e-6, diagonal 1e306), so in dtrti2 its column of the inverted factor
                     overflows to infinities over S1's rows and stays exactly zero over S2's.  The identity's columns then bring a zero
                     temp (their element of row c) to that column in dtrmv, and S2's rows bring a zero temp (their element of column c)
                     to it in dlauu2's dgemv: with the skip nothing happens, without it 0 * inf = NaN.  A condition, not a recipe:
                     tests/test_factor_cpu.py requires that the restatement without either skip differs from the oracle here.

k runs over 0, d - 1 and every seam below d among 7, 8, 9, 15, 16, 17, 31, 32, 33, 47, 48: the 8 x 8 blocks of calculate_R and the
16-column lane ownership of tile_factor_kernel."""
import collections

import numpy as np

import svd_cases

SEAMS = (7, 8, 9, 15, 16, 17, 31, 32, 33, 47, 48)
SVD_FAMILIES = ("identity", "zero", "dense", "lowrank", "rank1", "few", "block", "ill", "ones", "small", "tiny", "huge")
_CASES = {}


def pivots(d):
    """the 0-based pivots a failure is placed at"""
    return sorted({0, d - 1} | {k for k in SEAMS if k < d})


def _dense(d):
    return np.array(svd_cases.cases(d)["dense"])


def zero_meets_inf(d):
    assert d >= 4
    h1 = max(1, d // 4); h2 = max(1, d // 4); c = h1 + h2
    A = np.eye(d)
    A[:h1, :h1] = _dense(h1) * 1e-316
    A[h1:c, h1:c] = _dense(h2) * 1e-316
    A[:h1, c] = A[c, :h1] = 1e-6
    A[c, c] = 1e306
    return (A + A.T) / 2


def cases(d):
    if d in _CASES:
        return _CASES[d]
    out = collections.OrderedDict()
    sc = svd_cases.cases(d)
    for n in SVD_FAMILIES:
        out[n] = (sc[n], None)
    dense = _dense(d)
    for k in pivots(d):
        A = dense.copy(); A[k, k] = -1.0
        out["neg_at(%d)" % k] = (A, k + 1)
        A = dense.copy(); A[k, :] = 0.0; A[:, k] = 0.0
        out["zero_at(%d)" % k] = (A, k + 1)
        A = np.eye(d); A[k, k] = -0.0
        out["negzero_at(%d)" % k] = (A, k + 1)
        A = dense.copy(); A[k, k] = np.nan
        out["nan_diag(%d)" % k] = (A, k + 1)
        if k > 0:
            A = dense.copy(); A[k // 2, k] = A[k, k // 2] = np.nan
            out["nan_off(%d,%d)" % (k // 2, k)] = (A, k + 1)
        A = dense.copy(); A[k, k] = np.inf
        out["inf_diag(%d)" % k] = (A, 0)
    out["diagonal"] = (np.diag(10.0 ** np.linspace(-150, 150, d)), 0)
    out["subn"] = (dense * 1e-310, 0)
    if d >= 4:
        out["zero_meets_inf"] = (zero_meets_inf(d), 0)
    for k, (v, info) in out.items():
        assert v.shape == (d, d) and np.array_equal(v, v.T, equal_nan=True), k
        v = np.array(v); v.setflags(write=False)
        out[k] = (v, info)
    _CASES[d] = out
    return out


def same_bits(a, b):
    """bit for bit (NaN payloads and signs included)"""
    return bool(np.array_equal(svd_cases.bits(a), svd_cases.bits(b)))


def same_bits_nan_sign_open(a, b):
    """bit for bit, the sign of a NaN left open (svd_cases.same_bits_up_to_nan_sign: for host code, where two compilers may order the
    operands of one operation on two NaNs differently; here it is 0 * inf and inf - inf, whose default NaN x86 returns negative and
    whose sign a compiler may fold either way) -- and for the device against the host-built oracle, where the default NaN is positive"""
    return svd_cases.same_bits_up_to_nan_sign(a, b)
