"""The pinned SVD without a GPU: host_symsvd (mcmcx_debug_symsvd, form 0: the statement that factorises every run's initial covariance)
bit for bit against the oracle's routine on the edge matrices of tests/svd_cases.py; the probe's need mask and refusals; and the oracle's
routine itself against high-precision references -- reconstruction and orthogonality in long double, singular values against mpmath's
symmetric eigensolver at 50 digits -- and against what its header defines it to do on ill-scaled input (the 60-sweep cap)."""
import ctypes as C
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from svd_cases import FAMILIES, ILL_SCALED, bits, cases, check_refusals, oracle_svd, same_bits_up_to_nan_sign

EPS = 2.0 ** -52
WELL_SCALED = tuple(n for n in FAMILIES if n not in ILL_SCALED)


def _names(d):
    # tiny above npar 65: subnormal arithmetic on the CPU, 8 s a call at 129
    return [n for n in FAMILIES if not (n == "tiny" and d > 65)]


def _host(A):
    from mcmcf90_amd.engine import debug_symsvd
    V, s, sw, forms = debug_symsvd(0, A[None])
    assert forms == "host_symsvd"
    return V[0], s[0], int(sw[0])


@pytest.mark.parametrize("d", [1, 2, 3, 7, 8, 9, 16, 17, 48, 65, 129])
def test_host_symsvd_equals_the_oracle(oracle, d):
    """V, s and the sweep count, bit for bit, every family.  Where the routine returns NaNs (huge) they must stand at the same elements with
    the same payload; their SIGN is left open, and only here, between two host compilers: huge at npar 7 gives s = 0x7ff8000000000000
    in the oracle's build and 0xfff8000000000000 in the library's host build, from the operand order of one addition of two NaNs
    (svd_cases.same_bits_up_to_nan_sign).  The device forms are held to the oracle's NaN bits too (tests/test_gpu_svd.py).  One probe call
    per matrix, side by side in threads: form 0 touches no device and the sweep-cap cases take 0.65 s each at npar 129."""
    names = _names(d)
    ref = oracle_svd(oracle, d, names)
    cs = cases(d)
    with ThreadPoolExecutor(max_workers=8) as ex:
        got = list(ex.map(lambda n: _host(cs[n]), names))
    for n, (V, s, sw), (Vo, so, swo) in zip(names, got, ref):
        assert sw == swo, (d, n, sw, swo)
        if n == "huge":
            assert same_bits_up_to_nan_sign(s, so) and same_bits_up_to_nan_sign(V, Vo), (d, n)
            continue
        assert np.array_equal(bits(s), bits(so)), (d, n)
        assert np.array_equal(bits(V), bits(Vo)), (d, n)


def test_need_mask_leaves_rows_alone(oracle):
    """One call, nine matrices, every other one masked out: the masked rows keep the caller's sentinel in V, s and the sweep counts, the
    others equal the oracle; need = all zeros succeeds and writes nothing."""
    from mcmcf90_amd.engine import debug_symsvd
    d = 9
    names = list(WELL_SCALED[:9])
    A = np.stack([cases(d)[n] for n in names])
    need = np.arange(len(names)) % 2
    V, s, sw, forms = debug_symsvd(0, A, need=need, fill=-7.25, sweeps_fill=-3)
    for m, (Vo, so, swo) in enumerate(oracle_svd(oracle, d, names)):
        if need[m]:
            assert sw[m] == swo and np.array_equal(bits(V[m]), bits(Vo)) and np.array_equal(bits(s[m]), bits(so)), names[m]
        else:
            assert sw[m] == -3 and np.all(V[m] == -7.25) and np.all(s[m] == -7.25), names[m]
    V, s, sw, forms = debug_symsvd(0, A, need=np.zeros(len(names)), fill=-7.25, sweeps_fill=-3)
    assert np.all(V == -7.25) and np.all(s == -7.25) and np.all(sw == -3) and forms == "host_symsvd"


def test_refusals_need_no_device():
    check_refusals()
    from mcmcf90_amd import _lib
    L = _lib.load()
    dp = C.POINTER(C.c_double)
    A = np.eye(2).ravel(); V = np.zeros(4); s = np.zeros(2)
    buf = C.create_string_buffer(len("host_symsvd") + 1)                 # ... and a buffer that just fits is taken
    assert L.mcmcx_debug_symsvd(0, 0, 2, 1, A.ctypes.data_as(dp), None, V.ctypes.data_as(dp), s.ctypes.data_as(dp), None, buf, len(buf)) == 0
    assert buf.value == b"host_symsvd" and np.array_equal(V, A) and np.array_equal(s, [1.0, 1.0])
    assert L.mcmcx_debug_symsvd(0, 0, 2, 1, A.ctypes.data_as(dp), None, V.ctypes.data_as(dp), s.ctypes.data_as(dp), None, None, 0) == 0


def _residuals(A, V, s):
    """max |V diag(s) V' - A| / max |A| and max |V'V - I| in long double"""
    Al, Vl, sl = A.astype(np.longdouble), V.astype(np.longdouble), s.astype(np.longdouble)
    amax = np.max(np.abs(Al))
    rec = np.max(np.abs((Vl * sl) @ Vl.T - Al)) / (amax if amax > 0 else np.longdouble(1))
    orth = np.max(np.abs(Vl.T @ Vl - np.eye(A.shape[0], dtype=np.longdouble)))
    return float(rec), float(orth)


@pytest.mark.parametrize("d", [1, 2, 3, 7, 8, 9, 16, 17, 48, 65, 129, 256])
def test_oracle_reconstructs_and_is_orthogonal(oracle, d):
    """The oracle's routine on the well-scaled families: max |V diag(s) V' - A| / max |A| and max |V'V - I|, evaluated in long double,
    within 8 d eps.  The bound is the issue's: about 3.5 times the worst it measured (2.3 d eps at npar 256: orthogonality 1.3e-13 for
    rank1 and ill, reconstruction 9.3e-14 for ill).  Measured here, over these twelve sizes: 2.77 d eps, both
    at npar 256 for ill -- orthogonality 1.58e-13 (rank1 1.40e-13), reconstruction 1.13e-13 (lowrank 9.88e-14)."""
    assert np.finfo(np.longdouble).eps < 2.0 ** -60, "long double is no wider than double here: no high-precision reference"
    names = list(WELL_SCALED)
    for n, (V, s, sw) in zip(names, oracle_svd(oracle, d, names)):
        rec, orth = _residuals(cases(d)[n], V, s)
        print("svd residuals d %d %s: sweeps %d reconstruction %.3g (%.2f d eps) orthogonality %.3g (%.2f d eps)"
              % (d, n, sw, rec, rec / (d * EPS), orth, orth / (d * EPS)))
        assert np.all(np.diff(s) <= 0) and np.all(s >= 0), (d, n)
        assert rec <= 8 * d * EPS, (d, n, rec)
        assert orth <= 8 * d * EPS, (d, n, orth)


SV_MEASURED = 1.53e-15              # the worst over the cases below: dense at npar 16, 6.89 eps (few at 17: 1.46e-15, lowrank at 16: 1.44e-15)
SV_BOUND = 4 * SV_MEASURED          # 6.12e-15 = 27.6 eps


@pytest.mark.parametrize("d", [1, 2, 3, 7, 8, 9, 16, 17])
def test_oracle_singular_values_against_mpmath(oracle, d):
    """s against the eigenvalues of mpmath.eigsy at 50 digits (a PSD matrix's singular values; for the indefinite rounding of a
    rank-deficient family their absolute values), as max_j |s_j - lambda_j| / lambda_max.  Measured first, then bound at four times the measured worst:
    measured 1.53e-15 (dense at npar 16), asserted 6.12e-15.  A matrix of zeros (zero; diag_rep below npar 4) has no scale: s must be 0."""
    import mpmath
    names = list(WELL_SCALED)
    with mpmath.workdps(50):
        for n, (V, s, sw) in zip(names, oracle_svd(oracle, d, names)):
            A = cases(d)[n]
            ev = mpmath.eigsy(mpmath.matrix(A.tolist()), eigvals_only=True)
            lam = sorted((abs(ev[i]) for i in range(d)), reverse=True)
            if lam[0] == 0:
                assert not A.any() and not s.any(), (d, n)
                continue
            err = float(max(abs(mpmath.mpf(float(s[j])) - lam[j]) for j in range(d)) / lam[0])
            print("svd mpmath d %d %s: %.3g (%.2f eps)" % (d, n, err, err / EPS))
            assert err <= SV_BOUND, (d, n, err)


@pytest.mark.parametrize("d", [48, 65])
def test_oracle_ill_scaled_families_hit_the_sweep_cap(oracle, d):
    """What the routine is defined to do where its tolerance test degenerates: alpha * beta underflows to 0 (small, tiny) or overflows
    (huge), |gamma| <= 1e-15 sqrt(alpha beta) never holds, every sweep rotates, and the loop ends at exactly 60 sweeps; huge returns
    non-finite values.  (The device forms must reproduce these bit for bit: tests/test_gpu_svd.py.)"""
    for n, (V, s, sw) in zip(ILL_SCALED, oracle_svd(oracle, d, ILL_SCALED)):
        assert sw == 60, (d, n, sw)
        if n == "huge":
            assert not (np.all(np.isfinite(V)) and np.all(np.isfinite(s))), d
        else:
            assert np.all(np.isfinite(V)) and np.all(np.isfinite(s)), (d, n)
