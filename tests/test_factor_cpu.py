"""The Cholesky branch of MCMC_calculate_R without a device: the numpy restatement (tests/factor_ref.py) against the oracle's dpotf2 and
dpotri bit for bit on every family of tests/factor_cases.py, the oracle against a long-double residual within Higham's componentwise
bound, the host's statement (mcmcx_debug_host_calculate_R: host_initial_R + host_potri) against the oracle bit for bit, and the oracle's
own mcxo_calculate_R against its two routines.  tests/test_gpu_factor.py holds the device forms to the same references."""
import ctypes as C

import numpy as np
import pytest

import factor_cases as fc
import factor_ref as fr
import svd_cases

SIZES = (1, 2, 7, 8, 9, 16, 17, 33, 64, 65)
DP = C.POINTER(C.c_double)
_ORC = {}


def oracle_factor(oracle, d, name):
    """(T, info, R, iC, info2) of mcxo_potrf_u and, where it succeeds, of mcxo_potri_u on R = triu(T) 2.4 / sqrt(d); once per matrix"""
    if (d, name) not in _ORC:
        L = oracle.lib()
        A = fc.cases(d)[name][0]
        W = np.asfortranarray(np.array(A))
        info = int(L.mcxo_potrf_u(d, W.ctypes.data_as(DP)))
        T = np.triu(np.array(W)); R = iC = None; info2 = 0
        if info == 0:
            with np.errstate(all="ignore"):
                R = T * 2.4 / np.sqrt(float(d))
            W2 = np.asfortranarray(R.copy())
            info2 = int(L.mcxo_potri_u(d, W2.ctypes.data_as(DP)))
            iC = np.triu(np.array(W2))
        _ORC[(d, name)] = (T, info, R, iC, info2)
    return _ORC[(d, name)]


@pytest.mark.parametrize("d", SIZES)
def test_restatement_is_the_oracle_bit_for_bit(oracle, d):
    """dpotf2 (factor, failed pivot's value and info) and dpotri (inverse and info) of factor_ref against the oracle's, every family, bit
    for bit, the sign of a NaN aside (numpy's operand order and the C compiler's).  Every constructed failure returns exactly the
    constructed info, every constructed success 0."""
    for name, (A, want) in fc.cases(d).items():
        T, info, R, iC, info2 = oracle_factor(oracle, d, name)
        if want is not None:
            assert info == want, (name, info, want)
        Tr, ir = fr.potrf_u(A)
        assert ir == info and fc.same_bits_nan_sign_open(np.triu(Tr), T), (name, ir, info)
        if info == 0:
            Ir, i2 = fr.potri_u(R)
            assert i2 == info2 and fc.same_bits_nan_sign_open(Ir, iC), (name, i2, info2)
            assert info2 == 0, name                                # a positive pivot's root, scaled, is not zero


# every npar at which tests/test_gpu_factor.py runs a device form with delayed rejection, from 4 on
SKIP_SIZES = (7, 8, 9, 15, 16, 17, 25, 31, 32, 33, 47, 48, 49, 63, 64, 65)


@pytest.mark.parametrize("d", SKIP_SIZES)
def test_zero_skips_decide_bits_on_zero_meets_inf(oracle, d):
    """The family's condition, at every npar the device forms get it: without dtrmv's skip, and without dgemv's, the restatement
    differs from the oracle (a NaN where the oracle has none) -- so a statement that lost either skip cannot pass on it."""
    T, info, R, iC, info2 = oracle_factor(oracle, d, "zero_meets_inf")
    assert info == 0 and info2 == 0
    assert fc.same_bits(fr.potri_u(R)[0], iC)
    for kw in (dict(skip_trti=False), dict(skip_lauu=False), dict(skip_zeros=False)):
        X = fr.potri_u(R, **kw)[0]
        assert not fc.same_bits_nan_sign_open(X, iC), kw
        assert np.isnan(X).sum() > np.isnan(iC).sum(), kw


def test_oracle_factor_within_the_componentwise_backward_bound(oracle):
    """|A - R'R| <= gamma_{d+1} |R'||R| componentwise, gamma_k = k u / (1 - k u), u = 2**-53 (Higham, Accuracy and Stability, Thm 10.3;
    fma chains only tighten it), for the oracle's dpotf2 on every succeeding finite family; the residual and |R'||R| in long double
    (64-bit significand: its own error is 2**-11 of u).  The theorem's model excludes underflow, so a family whose A has a non-zero
    entry below 2**-969 = 2**-1022 / u (subn, zero_meets_inf: an absolute error of half a subnormal ulp is no longer below u |x|) is
    left out -- the constructed block matrix also overflows on purpose.  Worst ratio residual / bound measured: 0.83 (tiny at d = 1,
    where the bound is 2 u a and a correctly rounded root squared may be off by nearly that), over 86 matrices: the bound is derived,
    not tuned."""
    worst, seen = (0.0, (0, "")), 0
    u = np.longdouble(2.0) ** -53
    for d in SIZES:
        g = (d + 1) * u / (1 - (d + 1) * u)
        for name, (A, _) in fc.cases(d).items():
            T, info, R, iC, info2 = oracle_factor(oracle, d, name)
            nz = np.abs(A[A != 0])
            if info != 0 or not np.all(np.isfinite(A)) or not np.all(np.isfinite(T)) or (nz.size and nz.min() < 2.0 ** -969):
                continue
            Tl = T.astype(np.longdouble); Al = np.triu(A).astype(np.longdouble)
            res = np.abs(np.triu(Tl.T @ Tl) - Al)
            bnd = g * np.triu(np.abs(Tl).T @ np.abs(Tl))
            assert np.all(res <= bnd), (d, name, float((res / np.where(bnd > 0, bnd, 1)).max()))
            r = float((res[bnd > 0] / bnd[bnd > 0]).max()) if np.any(bnd > 0) else 0.0
            worst = max(worst, (r, (d, name)))
            seen += 1
    print("worst backward-error ratio %.3g at %s over %d matrices" % (worst[0], worst[1], seen))
    assert seen >= 60 and worst[0] < 1.0, (seen, worst)


@pytest.mark.parametrize("d", SIZES)
def test_host_statement_is_the_oracle(oracle, d):
    """mcmcx_debug_host_calculate_R: R, iC and both infos on every family, bit for bit (the sign of a NaN left open, as for the host's SVD:
    two host compilers); a failed dpotf2 writes neither matrix."""
    from mcmcf90_amd.engine import debug_host_calculate_R
    for name, (A, _) in fc.cases(d).items():
        T, info, R, iC, info2 = oracle_factor(oracle, d, name)
        Rh, iCh, ih, ih2 = debug_host_calculate_R(A, fill=7.0)
        assert (ih, ih2) == (info, info2), (name, ih, ih2, info, info2)
        if info != 0:
            assert np.all(Rh == 7.0) and np.all(iCh == 7.0), name
            continue
        assert fc.same_bits_nan_sign_open(Rh, R), name
        assert fc.same_bits_nan_sign_open(iCh, iC), name
        Rh2, iCh2, _, _ = debug_host_calculate_R(A, with_inverse=False, fill=7.0)
        assert fc.same_bits_nan_sign_open(Rh2, R) and np.all(iCh2 == 7.0), name


def test_dpotf2_cannot_hand_dpotri_a_zero_diagonal():
    """dpotri's refusal (an exact zero on the factor's diagonal) is not reachable through dpotf2: the smallest pivot there is, 5e-324,
    has the root 2.2e-162, and scaled by 2.4 / sqrt(npar) that is not zero -- so the entry inverts (to infinities here) and info2 is 0.
    host_potri's early return itself is not run by this entry; its callers work on a copy (pooled_dr_fresh) or fail mcmcx_init."""
    from mcmcf90_amd.engine import debug_host_calculate_R
    A = np.diag([5e-324, 1.0, 5e-324])
    R, iC, info, info2 = debug_host_calculate_R(A, fill=7.0)
    assert (info, info2) == (0, 0) and R[0, 0] > 0.0 and R[2, 2] > 0.0 and np.all(iC != 7.0)


def test_host_statement_refusals_write_nothing():
    from mcmcf90_amd import _lib
    L = _lib.load()
    IP = C.POINTER(C.c_int32)
    for null, d, frag in (("A", 3, b"null"), ("R", 3, b"null"), ("info", 3, b"null"), (None, 0, b"d outside"), (None, -2, b"d outside"),
                          (None, 4097, b"d outside")):
        A = np.eye(3).ravel(); R = np.full(9, 7.0); iC = np.full(9, 7.0); info = np.full(2, 7, dtype=np.int32)
        rc = L.mcmcx_debug_host_calculate_R(d, None if null == "A" else A.ctypes.data_as(DP), None if null == "R" else R.ctypes.data_as(DP),
                                            iC.ctypes.data_as(DP), None if null == "info" else info.ctypes.data_as(IP))
        assert rc == -57 and frag in L.mcmcx_last_error(), (null, d, rc, L.mcmcx_last_error())
        assert np.all(R == 7.0) and np.all(iC == 7.0) and np.all(info == 7), (null, d)


@pytest.mark.parametrize("drscale", [0.0, 2.0])
def test_oracle_calculate_R_binding(oracle, drscale):
    """pyoracle.calculate_R (mcxo_calculate_R for a configuration) is its two routines: R = dpotf2 2.4 / sqrt(n), R2 = R / drscale,
    iC = dpotri(R); a failure leaves R, R2 and iC as they were and returns the pivot."""
    cfg = oracle.make_cfg(nsimu=10, drscale=drscale)
    for d in (1, 9, 17):
        for name, (A, _) in fc.cases(d).items():
            T, info, R, iC, info2 = oracle_factor(oracle, d, name)
            o = oracle.calculate_R(cfg, A)
            assert o.info == info, (d, name)
            if info != 0:
                assert fc.same_bits(o.R, o.R_before)
                assert not drscale or (fc.same_bits(o.R2, o.R2_before) and fc.same_bits(o.iC, o.iC_before))
                continue
            assert fc.same_bits(np.triu(o.R), R), (d, name)
            if drscale:
                with np.errstate(all="ignore"):
                    assert fc.same_bits(np.triu(o.R2), R / drscale) and fc.same_bits(np.triu(o.iC), iC), (d, name)
            assert fc.same_bits(o.cmat, A) and o.floored == 0


def test_oracle_calculate_R_svd_branch_reports_a_zero_diagonal(oracle):
    """condmax > 0 with delayed rejection: dpotri runs on the upper triangle of U sqrt(s) 2.4 / sqrt(n).  For an ascending diagonal
    matrix U is a permutation with a zero on its diagonal and the oracle returns -2000 - info2 (the reference stops); for the zero
    matrix the largest singular value is 0 and info = n."""
    cfg = oracle.make_cfg(nsimu=10, drscale=2.0, condmax=1e10)
    for d in (2, 8, 9, 17):
        o = oracle.calculate_R(cfg, np.diag(np.arange(1.0, d + 1)))
        assert o.info == -2001, (d, o.info)
        assert oracle.calculate_R(cfg, np.zeros((d, d))).info == d
        o = oracle.calculate_R(cfg, fc.cases(d)["dense"][0])
        assert o.info == 0 and o.floored == 0
        o = oracle.calculate_R(cfg, fc.cases(d)["lowrank"][0])
        assert o.info == 0 and o.floored == 1
