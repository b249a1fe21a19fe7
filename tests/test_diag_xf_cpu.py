"""The summary of an elementwise function of the sample store without a GPU (mcmcx_samples_stats_of, include/mcmcx.h): the numpy restatement
(tests/diag_xf_ref.py) against scalar loops and the host build of the key map, what the new diagnostics read on data whose answer is known
(folded split-R-hat on chains that differ in scale only, tail ESS on iid draws, the indicator's exact count), the refusals that need no
device, and the build's report of the new kernels."""
import ctypes as C
import math
import os
import struct

import numpy as np
import pytest

import diag_ref
import diag_xf_ref
import quant_ref
from mcmcf90_amd import _lib

DP = C.POINTER(C.c_double)
NAN_NEG = struct.unpack("<d", struct.pack("<Q", 0xFFF8000000000000))[0]
NAN_POS = struct.unpack("<d", struct.pack("<Q", 0x7FF8000000000000))[0]
SPECIALS = [0.0, -0.0, np.inf, -np.inf, NAN_POS, NAN_NEG, 5e-324, -5e-324, 2.2250738585072009e-308, -2.2250738585072009e-308,
            1.0, -1.0, np.nextafter(1.0, 2.0), np.nextafter(1.0, 0.0), 1e300, -1e300, 0.3]


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _grid():
    """X[ns = 1][nfields = len(SPECIALS)][nc = len(SPECIALS)]: every special value against every special a_f (equal ones included)."""
    v = np.array(SPECIALS)
    return np.broadcast_to(v[None, None, :], (1, v.size, v.size)).copy(), v.copy()


def test_key_compare_is_the_order_statistics_own():
    """u_ref of kind 1 against a scalar loop over mcmcx_debug_quant_key: +-0, +-inf, both NaN signs, denormals, values equal to a."""
    L = _lib.load()
    X, a = _grid()
    got = diag_xf_ref.u_ref(X, diag_xf_ref.LE, a)

    def ukey(x):
        return L.mcmcx_debug_quant_key(float(x), 0) & 0xFFFFFFFFFFFFFFFF
    for f, af in enumerate(a):
        for c, x in enumerate(X[0, f]):
            want = 1.0 if ukey(x) <= ukey(af) else 0.0
            assert _bits(got[0, f, c]) == _bits(want), (x, af, got[0, f, c])
    k, j, p, n = 0, 1, 4, 5                                     # +0.0, -0.0, the positive and the negative NaN in SPECIALS
    assert got[0, j, k] == 0.0 and got[0, k, j] == 1.0 and got[0, j, j] == 1.0, "-0.0 lies below +0.0"
    assert np.all(got[0, p] == 1.0) and np.all(got[0, n, [c for c in range(a.size) if c != n]] == 0.0), "NaNs sit at the two ends"


def test_fold_and_square_are_one_and_two_operations():
    X, a = _grid()
    with np.errstate(all="ignore"):
        fold, sq = diag_xf_ref.u_ref(X, diag_xf_ref.FOLD, a), diag_xf_ref.u_ref(X, diag_xf_ref.SQUARE, a)
    assert np.array_equal(_bits(diag_xf_ref.u_ref(X, diag_xf_ref.IDENTITY, None)), _bits(X))
    for f, af in enumerate(a):
        for c, x in enumerate(X[0, f]):
            with np.errstate(all="ignore"):
                d = np.float64(x) - np.float64(af)
                wf, ws = math.fabs(d), d * d
            assert _bits(fold[0, f, c]) == _bits(wf) and _bits(sq[0, f, c]) == _bits(ws), (x, af)
    assert not np.signbit(fold).any(), "the sign is cleared, a NaN's too"


def _split_scale(seed, scale=3.0, nc=584, ns=64):
    x = np.random.default_rng(seed).normal(size=(ns, 1, nc))
    x[:, :, 1::2] *= scale
    return x


@pytest.mark.parametrize("seed", range(10))
def test_folded_rhat_sees_chains_that_differ_in_scale(seed):
    """584 chains of 64 iid draws, every other chain with sd 3 instead of 1.  |x| of N(0, s^2) has mean s sqrt(2 / pi) and variance
    s^2 (1 - 2 / pi): between the chains' means 2 / pi, within (1 + 9) / 2 (1 - 2 / pi), so R-hat tends to sqrt(1 + B / W) =
    sqrt(1 + 0.6366 / 1.8169) = 1.162.  The plain R-hat sees nothing: the locations agree."""
    x = _split_scale(seed)
    med = np.median(x, axis=(0, 2))
    folded = diag_xf_ref.summary_ref(x, diag_xf_ref.FOLD, med, 0)[0][2]
    plain = diag_ref.summary_ref(x, 0)[0][2]
    print("seed %d: folded %.4f plain %.4f" % (seed, folded, plain))
    assert abs(folded - 1.16) <= 0.02, folded
    assert abs(plain - 1.0) <= 0.005, plain


@pytest.mark.parametrize("seed", range(10))
def test_tail_ess_of_iid_draws_is_the_number_of_draws(seed):
    """iid normal draws of the same shape: the ESS of the indicator x <= q05 over M n_h (Geyer's estimator on white noise reads a little
    above 1)."""
    x = np.random.default_rng(100 + seed).normal(size=(64, 1, 584))
    q05 = np.quantile(x, 0.05, axis=(0, 2))
    t = diag_xf_ref.summary_ref(x, diag_xf_ref.LE, q05, 16, shift=np.zeros(1))[0]
    ratio = t[3] / (2.0 * 584 * 32)
    print("seed %d: ess / (M n_h) %.4f" % (seed, ratio))
    assert 0.95 <= ratio <= 1.2, ratio


def test_the_indicator_counts_exactly():
    """ns = 8: n_h = 4 is a power of two and the halves cover the window, so with a shift of zeros every half mean is k / 4 exactly and
    S1 n_h is the number of window values with key <= key(a) -- samples_counts' le."""
    rng = np.random.default_rng(5)
    for nc in (1, 65, 583):
        X = rng.normal(size=(8, 3, nc))
        X[rng.integers(8), 1, rng.integers(nc)] = NAN_POS
        X[rng.integers(8), 2, rng.integers(nc)] = -0.0
        a = np.array([0.3, NAN_POS, 0.0])
        st = diag_xf_ref.stats_ref(X, diag_xf_ref.LE, a, 3, shift=np.zeros(3))
        per = st[3:].reshape(3, 7)
        le = quant_ref.counts_ref(X, a[:, None])[:, 0, 1]
        assert np.array_equal(per[:, 1] * 4.0, le.astype(np.float64)), (nc, per[:, 1] * 4.0, le)
        assert le[1] == 8 * nc, "everything lies at or below a positive NaN"


def test_refusals_that_need_no_device():
    L = _lib.load()
    buf = np.zeros(64)
    p = buf.ctypes.data_as(DP)
    for fn, out in ((L.mcmcx_samples_stats_of, p), (L.mcmcx_samples_stats_of_dev, C.c_void_p(8))):
        for kind in (-1, 4, 2 ** 31 - 1):
            assert fn(None, 0, 8, 4, kind, p, None, out) == -53 and b"kind" in L.mcmcx_last_error(), kind
        for kind in (1, 2, 3):
            assert fn(None, 0, 8, 4, kind, None, None, out) == -53 and b"null a" in L.mcmcx_last_error(), kind
        assert fn(None, 0, 8, 4, 0, None, None, out) == -53 and b"null handle" in L.mcmcx_last_error()
        assert fn(None, 0, 8, 4, 1, p, None, out) == -53 and b"null handle" in L.mcmcx_last_error()
    x = np.zeros(4 * 2 * 3)
    xp = x.ctypes.data_as(DP)

    def dbg(nch=3, nf=2, ns=4, values=xp, maxlag=1, kind=1, a=p, out=p):
        return L.mcmcx_debug_samples_stats(0, nch, nf, ns, values, maxlag, kind, a, None, out)
    for kw, word in ((dict(kind=-1), b"kind"), (dict(kind=4), b"kind"), (dict(a=None), b"null a"), (dict(values=None), b"null argument"),
                     (dict(out=None), b"null argument"), (dict(nch=0), b"nchains"), (dict(nf=0), b"nfields"), (dict(ns=3), b"ns < 4"),
                     (dict(maxlag=-1), b"maxlag"), (dict(maxlag=33), b"maxlag")):
        assert dbg(**kw) == -53 and word in L.mcmcx_last_error(), (kw, L.mcmcx_last_error())
    assert np.all(buf == 0.0)


def test_transformed_kernels_hold_their_lag_window_in_registers():
    """The twelve transformed instantiations in the build's report of the shipped code object (its sha is checked by
    tests/test_evidence_is_current.py): the parameter and the key compare fit beside the rotating window -- no scratch, no vector or
    scalar spill, no LDS, at least two waves per SIMD."""
    rows = {}
    for line in open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "kernel_resources.txt")):
        if line.startswith("diag_xf_tile_kernel<"):
            f = line.split()
            rows["".join(f[:-9])] = dict(zip(("vgpr", "agpr", "sgpr", "scratch", "vspill", "sspill", "lds", "wg", "waves"), map(int, f[-9:])))
    assert sorted(rows) == sorted("diag_xf_tile_kernel<%d,%d>" % (w, k) for w in (1, 9, 17, 33) for k in (1, 2, 3)), sorted(rows)
    for name, r in rows.items():
        assert r["scratch"] == r["vspill"] == r["sspill"] == r["lds"] == r["agpr"] == 0, (name, r)
        assert r["waves"] >= 2, (name, r)
