"""The sample store's batch-means covariance and its finishes without a GPU: the exports, the restatement (tests/bm_ref.py) against the
covariance's at batch = 1 and against an np.longdouble reference within the derived forward bound, mcmcx_samples_mess / _mpsrf against the
restated finishes, lambda1 against the exact eigenvalue (mpmath, 50 digits) beside scipy's, the identities with the per-field split-R-hat, the
motivating case (marginals at 1.003, the vector at 1.4), the multivariate ESS of AR(1) fields of known autocorrelation, additivity, a constant
field, the refusals, and the build's resource report of the new kernels."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import bm_ref
import cov_ref
import diag_ref
from mcmcf90_amd import _lib
from mcmcf90_amd.engine import McmcError, samples_cov_finish, samples_diag, samples_mess, samples_mpsrf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DP = C.POINTER(C.c_double)
IP = C.POINTER(C.c_int32)
NAMES = ("mcmcx_samples_cov_bm", "mcmcx_samples_cov_bm_dev", "mcmcx_samples_mess", "mcmcx_samples_mpsrf", "mcmcx_debug_samples_cov_bm")


def _data(seed, ns=20, nf=10, nch=583):
    """Correlated, well-conditioned fields with means of order one: [ns][nf][nch] (tests/test_cov_cpu.py's)"""
    rng = np.random.default_rng(seed)
    A = rng.normal(size=(nf, nf)) + 2.0 * np.eye(nf)
    return np.einsum("fg,sgc->sfc", A, rng.normal(size=(ns, nf, nch))) + rng.normal(size=nf)[None, :, None]


def _vec(X, batch, shift=None):
    """A batch-means vector of X[ns][nf][nch] in numpy's own summation order (batch = 1: a cov vector): what the finishes take is any
    vector of the layout, and the statistical cases below are too large for the bit-exact restatement (1e6 fma per second)."""
    z, sh = cov_ref.shifted(X, shift)
    ns, nf, nch = z.shape
    nb = ns // batch
    y = z[:nb * batch].reshape(nb, batch, nf, nch).sum(axis=1) / float(batch)
    yl = y.transpose(1, 0, 2).reshape(nf, nb * nch)
    J, K = cov_ref.all_pairs(nf)
    return np.concatenate([[float(nb * nch)], sh, yl.sum(axis=1), (yl @ yl.T)[J, K]])


@pytest.fixture(scope="module")
def vectors():
    """seed -> (X, restated cov vector of the 20 samples, restated batch-means vector at batch 4): 583 chains are 640 padded lanes x
    (20 + 5) x 55 pairs = 8.8e5 fma each"""
    out = {}
    for seed in range(3):
        X = _data(seed)
        out[seed] = (X, cov_ref.cov_vector_ref(X), bm_ref.bm_vector_ref(X, 4))
    return out


def test_exports_exist_and_the_header_compiles_as_c(tmp_path):
    L = _lib.load()
    for n in NAMES:
        assert n in _lib.SYMBOLS and getattr(L, n) is not None, n
    hdr = open(os.path.join(ROOT, "include", "mcmcx.h")).read()
    for n in NAMES:
        assert re.search(r"\b%s\s*\(" % n, re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)), n
    src = tmp_path / "use.c"
    src.write_text('#include "mcmcx.h"\nint main(void) { double c[4] = {8, 0, 0, 9}, b[4] = {4, 0, 0, 2}, o[4], e[1]; int32_t s[1] = {0}; '
                   'return mcmcx_samples_mess(c, b, 1, 2, 1, s, o, e) + mcmcx_samples_mpsrf(c, b, 1, 2, 1, s, o, 0, 0); }\n')
    p = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I" + os.path.join(ROOT, "include"), "-c", str(src),
                        "-o", str(tmp_path / "use.o")], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert p.returncode == 0, p.stdout.decode()


def test_restatement_at_batch_one_is_the_covariance_bit_for_bit(vectors):
    X = vectors[0][0][:6]                                       # 640 lanes x 6 x 55 = 2.1e5 fma, twice
    for shift in (None, np.linspace(-1.0, 1.0, 10)):
        a, b = bm_ref.bm_vector_ref(X, 1, shift), cov_ref.cov_vector_ref(X, shift)
        assert np.array_equal(cov_ref.bits(a), cov_ref.bits(b))
    # a remainder is not read; batch = ns is one mean per chain
    assert np.array_equal(cov_ref.bits(bm_ref.bm_vector_ref(X[:, :3, :70], 4)), cov_ref.bits(bm_ref.bm_vector_ref(X[:4, :3, :70], 4)))
    v = bm_ref.bm_vector_ref(X[:, :3, :70], 6)
    assert v[0] == 70.0
    y, _ = bm_ref.batch_means(X[:, :3, :70], 6)
    assert y.shape == (1, 3, 70) and np.allclose(y[0], (X[:, :3, :70] - X[0, :3, 0][None, :, None]).mean(axis=0), rtol=1e-14, atol=1e-15)


def test_restatement_against_the_longdouble_reference(vectors):
    """|G - G_ref| and |S - S_ref| within bm_ref.longdouble_ref's forward bound (derived there, not measured)."""
    assert np.finfo(np.longdouble).nmant >= 63
    for seed, (X, _, bm) in vectors.items():
        S, G, bS, bG = bm_ref.longdouble_ref(X, 4)
        assert bm[0] == 5 * 583 and np.array_equal(bm[1:11], X[0, :, 0])
        eS = np.abs(bm[11:21].astype(np.longdouble) - S)
        eG = np.abs(bm[21:].astype(np.longdouble) - G)
        assert np.all(eS <= bS) and np.all(eG <= bG), (seed, float((eS / bS).max()), float((eG / bG).max()))
        # and the finish of it is the covariance of the batch means
        y, _ = bm_ref.batch_means(X, 4)
        flat = (y + X[0, :, 0][None, :, None]).transpose(1, 0, 2).reshape(10, -1)
        mean, cov, _ = samples_cov_finish(bm, 10)
        assert np.allclose(mean, flat.mean(axis=1), rtol=1e-10, atol=0.0) and np.allclose(cov, np.cov(flat), rtol=1e-10, atol=0.0)


def _close(g, w, what):
    g, w = np.asarray(g, dtype=np.float64), np.asarray(w, dtype=np.float64)
    assert g.shape == w.shape and np.array_equal(np.isnan(g), np.isnan(w)), what
    assert np.allclose(g, w, rtol=1e-13, atol=0.0, equal_nan=True), (what, g, w)


def test_finishes_against_the_restated_finishes(vectors):
    """The same operations on both sides: W, Bn, the log-dets and ess_out to 1e-13 relative, NaN pattern equal (lambda1 has a test of its
    own).  The mpsrf window is the first sixteen samples: its halves are batches of eight."""
    for seed, (X, cv, bm) in vectors.items():
        for sel in ([0, 1, 2, 3, 4, 5, 6, 7, 8, 9], [7, 2, 5], [4]):
            r = samples_mess(cv, bm, 10, 4, sel)
            warn, out4, ess = bm_ref.mess_ref(cv, bm, 10, 4, sel)
            assert r["warn"] == warn == 0
            _close([r["mess"], r["n"], r["logdet_lambda"], r["logdet_sigma"]], out4, (seed, sel))
            _close(r["ess_bm"], ess, (seed, sel))
            c16, b8 = _vec(X[:16], 1), _vec(X[:16], 8)
            m = samples_mpsrf(c16, b8, 10, 8, sel)
            warn, out4, W, Bn = bm_ref.mpsrf_ref(c16, b8, 10, 8, sel)
            assert m["warn"] == warn == 0 and m["M"] == 2 * 583 and m["n_h"] == 8
            _close(m["W"], W, (seed, sel)); _close(m["Bn"], Bn, (seed, sel))
            assert np.array_equal(m["W"], m["W"].T) and np.array_equal(m["Bn"], m["Bn"].T)
            assert abs(m["lambda1"] - out4[1]) <= 1e-12 * out4[1] and abs(m["mpsrf"] - out4[0]) <= 1e-12 * out4[0]
    # a vector with a NaN and an inf entry: the pattern is the restatement's
    X, cv, bm = vectors[0]
    cv, bm = cv.copy(), bm.copy()
    cv[1 + 10 + 3] = np.nan
    bm[1 + 20 + cov_ref.pair_index(5, 7, 10)] = np.inf
    for sel in ([0, 1, 2], [2, 3], [5, 6, 7, 8]):
        r = samples_mess(cv, bm, 10, 4, sel)
        warn, out4, ess = bm_ref.mess_ref(cv, bm, 10, 4, sel)
        assert r["warn"] == warn
        _close([r["mess"], r["n"], r["logdet_lambda"], r["logdet_sigma"]], out4, sel)
        _close(r["ess_bm"], ess, sel)


def _pencil_data(seed, cond, nf=8, nch=583, ns=16):
    """Chains whose within-chain covariance has condition number `cond` (eigenvalues log-spaced, a random rotation) and whose means are
    spread by a tenth of a standard normal: [ns][nf][nch]"""
    rng = np.random.default_rng(seed)
    Q, _ = np.linalg.qr(rng.normal(size=(nf, nf)))
    A = Q * np.sqrt(np.logspace(0.0, -np.log10(cond), nf))[None, :]
    return np.einsum("fg,sgc->sfc", A, rng.normal(size=(ns, nf, nch))) + 0.1 * rng.normal(size=(nf, nch))[None]


@pytest.mark.parametrize("cond", [1.0, 1e2, 1e4])
def test_lambda1_against_the_exact_eigenvalue(cond):
    """lambda1 is the largest eigenvalue of the pencil (Bn, W) of the RETURNED matrices.  The exact one: mpmath at 50 digits (the
    Cholesky-reduced symmetric problem, eigsy).  The tolerance is not fixed in advance: scipy.linalg.eigh(Bn, W)'s float64 error against the
    exact value is measured, and the C finish is allowed 8 x that, with a floor of nsel 2^-52 lambda1 -- both routes are a Cholesky
    reduction and a symmetric eigensolver, backward stable with constants of this size.  The measured errors are in DESIGN.md 5i-2."""
    import mpmath
    import scipy.linalg
    nsel = 8
    X = _pencil_data(int(cond), cond)
    m = samples_mpsrf(_vec(X, 1), _vec(X, 8), 8, 8, list(range(nsel)))
    assert m["warn"] == 0
    W, Bn = m["W"], m["Bn"]
    assert 0.3 * cond < np.linalg.cond(W) < 3.0 * cond
    with mpmath.workdps(50):
        Wm, Bm = mpmath.matrix(W.tolist()), mpmath.matrix(Bn.tolist())
        Lc = mpmath.cholesky(Wm)                                # W = L L'
        Li = mpmath.inverse(Lc)
        Cm = Li * Bm * Li.T
        Cm = (Cm + Cm.T) / 2
        exact = max(mpmath.eigsy(Cm, eigvals_only=True))
        e_scipy = abs(mpmath.mpf(float(scipy.linalg.eigh(Bn, W, eigvals_only=True)[-1])) - exact)
        e_c = abs(mpmath.mpf(float(m["lambda1"])) - exact)
        tol = max(8 * e_scipy, nsel * mpmath.mpf(2) ** -52 * exact)
        print("cond %g: lambda1 %.17g, relative error of scipy %.3g, of the C finish %.3g, allowed %.3g"
              % (cond, m["lambda1"], float(e_scipy / exact), float(e_c / exact), float(tol / exact)))
        assert e_c <= tol
    assert m["mpsrf"] == np.sqrt(7.0 / 8.0 + m["lambda1"])


def test_one_field_is_the_split_rhat_and_the_vector_is_never_below_a_field():
    """nsel = 1: mpsrf is mcmcx_samples_diag's rhat within 1e-9 (shift = the mean, unit-scale data: both are sums of n = 4e4 terms, n u
    apart).  nsel > 1: mpsrf >= every selected field's split-R-hat times (1 - 1e-12), the Rayleigh quotient at e_j."""
    X = _data(5, ns=64, nf=4, nch=583)
    X = X / X.std(axis=(0, 2))[None, :, None]
    mean = X.mean(axis=(0, 2))
    rhat = samples_diag(diag_ref.stats_ref(X, 0, mean), 4, 0)[:, 2]
    cv, bv = _vec(X, 1, mean), _vec(X, 32, mean)
    for j in range(4):
        m = samples_mpsrf(cv, bv, 4, 32, [j])
        assert m["warn"] == 0 and abs(m["mpsrf"] - rhat[j]) <= 1e-9, (j, m["mpsrf"], rhat[j])
    for sel in ([0, 1], [3, 1, 2], [0, 1, 2, 3]):
        m = samples_mpsrf(cv, bv, 4, 32, sel)
        assert m["mpsrf"] >= rhat[sel].max() * (1.0 - 1e-12), (sel, m["mpsrf"], rhat[sel])
    # the two shifts may differ
    m2 = samples_mpsrf(_vec(X, 1), bv, 4, 32, [0, 1, 2, 3])
    assert abs(m2["mpsrf"] - m["mpsrf"]) <= 1e-9


def _motivating(offset):
    rng = np.random.default_rng(2024)
    nch, ns, rho = 583, 64, 0.99
    Lc = np.linalg.cholesky(np.array([[1.0, rho], [rho, 1.0]]))
    X = np.einsum("fg,sgc->sfc", Lc, rng.normal(size=(ns, 2, nch)))
    minor = np.array([1.0, -1.0]) / np.sqrt(2.0)
    return X + (offset * rng.normal(size=nch))[None, None, :] * minor[None, :, None]


def test_the_motivating_case():
    """Two fields of correlation 0.99, 583 chains of 64 samples, every chain offset by N(0, 0.1^2) along the minor axis (1, -1) / sqrt(2),
    along which the within-chain sd is 0.1: both marginal split-R-hats below 1.01, the multivariate one within 5 % of
    sqrt(31 / 32 + (0.01 + 0.01 / 32) / 0.01) = 1.414; without the offsets it is below 1.01 too."""
    want = np.sqrt(31.0 / 32.0 + (0.01 + 0.01 / 32.0) / 0.01)
    for offset in (0.1, 0.0):
        X = _motivating(offset)
        mean = X.mean(axis=(0, 2))
        rhat = samples_diag(diag_ref.stats_ref(X, 0, mean), 2, 0)[:, 2]
        m = samples_mpsrf(_vec(X, 1, mean), _vec(X, 32, mean), 2, 32, [0, 1])
        print("offset %g: marginal split-R-hat %.4f %.4f, mpsrf %.4f (expected %.4f with the offsets)" % (offset, rhat[0], rhat[1], m["mpsrf"], want))
        assert m["warn"] == 0 and np.all(rhat < 1.01)
        if offset:
            assert abs(m["mpsrf"] - want) <= 0.05 * want
        else:
            assert m["mpsrf"] < 1.01
        assert m["mpsrf"] >= rhat.max() * (1.0 - 1e-12)


@pytest.mark.parametrize("phi,ns,b", [(0.5, 256, 16), (0.9, 512, 32), (0.0, 64, 8)])
def test_mess_of_ar1_fields_of_known_autocorrelation(phi, ns, b):
    """Four independent stationary AR(1) fields, 583 chains: mess / n against the finite-b value 1 / (1 + 2 sum_{k<b} (1 - k / b) phi^k)
    (k from 1; not the asymptote (1 - phi) / (1 + phi)), within 5 sqrt(2 / n_b) / sqrt(4): the relative sd of a variance estimate from
    n_b batch means is sqrt(2 / n_b), the fourth root of a product of four independent ones has half of it, five of those."""
    rng = np.random.default_rng(int(100 * phi) + ns)
    nch, nf = 583, 4
    e = rng.normal(size=(ns, nf, nch))
    X = np.empty_like(e)
    X[0] = e[0]
    for t in range(1, ns):
        X[t] = phi * X[t - 1] + np.sqrt(1.0 - phi * phi) * e[t]
    mean = X.mean(axis=(0, 2))
    r = samples_mess(_vec(X, 1, mean), _vec(X, b, mean), nf, b, [0, 1, 2, 3])
    want = 1.0 / (1.0 + 2.0 * sum((1.0 - k / b) * phi ** k for k in range(1, b)))
    n_b = (ns // b) * nch
    bound = 5.0 * np.sqrt(2.0 / n_b) / np.sqrt(4.0)
    dev = r["mess"] / r["n"] / want - 1.0
    print("phi %g: mess / n %.5f, expected %.5f, deviation %+.2f %%, bound %.2f %%" % (phi, r["mess"] / r["n"], want, 100 * dev, 100 * bound))
    assert r["warn"] == 0 and r["n"] == ns * nch and abs(dev) <= bound
    # the univariate batch-means ESS of every field is the same quantity for one field: twice the bound (one field, not four)
    assert np.all(np.abs(r["ess_bm"] / r["n"] / want - 1.0) <= 2.0 * bound)


def test_vectors_of_disjoint_chain_sets_finish_like_the_whole():
    X = _data(8, ns=16, nf=5, nch=583)
    shift = X[0, :, 0].copy()
    for batch in (4, 8):
        whole_c, whole_b = _vec(X, 1, shift), _vec(X, batch, shift)
        c = _vec(X[:, :, :300], 1, shift) + _vec(X[:, :, 300:], 1, shift)
        b = _vec(X[:, :, :300], batch, shift) + _vec(X[:, :, 300:], batch, shift)
        c[1:6] = shift; b[1:6] = shift
        assert c[0] == 16 * 583 and b[0] == (16 // batch) * 583
        r, w = samples_mess(c, b, 5, batch, [0, 1, 2, 3, 4]), samples_mess(whole_c, whole_b, 5, batch, [0, 1, 2, 3, 4])
        assert abs(r["mess"] - w["mess"]) <= 1e-10 * w["mess"] and np.allclose(r["ess_bm"], w["ess_bm"], rtol=1e-10, atol=0.0)
    r, w = samples_mpsrf(c, b, 5, 8, [0, 1, 2, 3, 4]), samples_mpsrf(whole_c, whole_b, 5, 8, [0, 1, 2, 3, 4])
    assert abs(r["mpsrf"] - w["mpsrf"]) <= 1e-10 * w["mpsrf"]
    # the bit-exact restatement is additive in the same sense: the parts' sum within the forward bound of the whole
    Xs = X[:8, :, :130]
    a = bm_ref.bm_vector_ref(Xs[:, :, :64], 4, shift) + bm_ref.bm_vector_ref(Xs[:, :, 64:], 4, shift)
    S, G, bS, bG = bm_ref.longdouble_ref(Xs, 4, shift)
    assert a[0] == 2 * 130
    assert np.all(np.abs(a[6:11].astype(np.longdouble) - S) <= bS) and np.all(np.abs(a[11:].astype(np.longdouble) - G) <= bG)


def test_a_constant_selected_field_warns_and_gives_nan():
    X = _data(11, ns=16, nf=5, nch=65)
    X[:, 3, :] = -2.5
    c, b4, b8 = _vec(X, 1), _vec(X, 4), _vec(X, 8)
    L = _lib.load()
    r = samples_mess(c, b4, 5, 4, [0, 3, 4])
    assert r["warn"] == 1 and np.isnan(r["mess"]) and np.isnan(r["logdet_lambda"]) and np.isnan(r["logdet_sigma"]) and r["n"] == 16 * 65
    assert np.array_equal(np.isnan(r["ess_bm"]), [False, True, False])
    warn, out4, ess = bm_ref.mess_ref(c, b4, 5, 4, [0, 3, 4])
    assert warn == 1 and np.array_equal(np.isnan(out4), [True, False, True, True])
    m = samples_mpsrf(c, b8, 5, 8, [0, 3, 4])
    assert m["warn"] == 1 and np.isnan(m["mpsrf"]) and np.isnan(m["lambda1"]) and m["M"] == 130 and m["n_h"] == 8
    assert np.all(m["W"][1] == 0.0) and np.all(m["Bn"][:, 1] == 0.0)
    # without it everything is finite, and a warning is not an error: last_error is not what reports it
    r = samples_mess(c, b4, 5, 4, [0, 1, 2, 4])
    m = samples_mpsrf(c, b8, 5, 8, [0, 1, 2, 4])
    assert r["warn"] == 0 and m["warn"] == 0 and np.isfinite(r["mess"]) and np.isfinite(m["mpsrf"]) and np.isfinite(r["ess_bm"]).all()
    assert L is not None


def test_every_refusal_is_minus_55():
    L = _lib.load()
    p = lambda a: a.ctypes.data_as(DP)
    q = lambda a: a.ctypes.data_as(IP)
    # one field: [n, shift, S, G].  cov: 8 samples; bm at batch 2: 4 means; at n_h = 2 over a window of 4: M = 2
    cv, bv = np.array([8.0, 0.0, 1.0, 9.0]), np.array([4.0, 0.0, 0.5, 2.0])
    c4, b2 = np.array([4.0, 0.0, 1.0, 9.0]), np.array([2.0, 0.0, 0.5, 2.0])
    sel, o4, e1, w1 = np.zeros(1, dtype=np.int32), np.full(4, 7.0), np.full(1, 7.0), np.full(1, 7.0)
    assert L.mcmcx_samples_mess(p(cv), p(bv), 1, 2, 1, q(sel), p(o4), p(e1)) == 0
    assert L.mcmcx_samples_mess(p(cv), p(bv), 1, 2, 1, q(sel), p(o4), None) == 0
    assert L.mcmcx_samples_mpsrf(p(c4), p(b2), 1, 2, 1, q(sel), p(o4), p(w1), None) == 0
    o4[:] = 7.0; e1[:] = 7.0; w1[:] = 7.0
    bad = np.array([1], dtype=np.int32)
    neg = np.array([-1], dtype=np.int32)
    for args in ((None, p(bv), 1, 2, 1, q(sel), p(o4), p(e1)), (p(cv), None, 1, 2, 1, q(sel), p(o4), p(e1)),
                 (p(cv), p(bv), 1, 2, 1, None, p(o4), p(e1)), (p(cv), p(bv), 1, 2, 1, q(sel), None, p(e1)),
                 (p(cv), p(bv), 0, 2, 1, q(sel), p(o4), p(e1)), (p(cv), p(bv), 1, 2, 0, q(sel), p(o4), p(e1)),
                 (p(cv), p(bv), 1, 2, 2, q(sel), p(o4), p(e1)), (p(cv), p(bv), 1, 2, 1, q(bad), p(o4), p(e1)),
                 (p(cv), p(bv), 1, 2, 1, q(neg), p(o4), p(e1)), (p(cv), p(bv), 1, 0, 1, q(sel), p(o4), p(e1)),
                 (p(cv), p(bv), 1, 4, 1, q(sel), p(o4), p(e1)), (p(cv), p(bv), 1, 1, 1, q(sel), p(o4), p(e1))):
        assert L.mcmcx_samples_mess(*args) == -55 and len(L.mcmcx_last_error()) > 0, args[2:5]
    for n in (1.0, 0.0, -2.0, 2.5, np.nan, np.inf):
        for which in (0, 1):
            v = [cv.copy(), bv.copy()]
            v[which][0] = n
            assert L.mcmcx_samples_mess(p(v[0]), p(v[1]), 1, 2, 1, q(sel), p(o4), p(e1)) == -55, (n, which)
            assert L.mcmcx_samples_mpsrf(p(v[0]), p(v[1]), 1, 2, 1, q(sel), p(o4), p(w1), p(w1)) == -55, (n, which)
    for args in ((None, p(b2), 1, 2, 1, q(sel), p(o4), p(w1), p(w1)), (p(c4), None, 1, 2, 1, q(sel), p(o4), p(w1), p(w1)),
                 (p(c4), p(b2), 1, 2, 1, None, p(o4), p(w1), p(w1)), (p(c4), p(b2), 1, 2, 1, q(sel), None, p(w1), p(w1)),
                 (p(c4), p(b2), 0, 2, 1, q(sel), p(o4), p(w1), p(w1)), (p(c4), p(b2), 1, 2, 2, q(sel), p(o4), p(w1), p(w1)),
                 (p(c4), p(b2), 1, 2, 1, q(bad), p(o4), p(w1), p(w1)), (p(c4), p(b2), 1, 1, 1, q(sel), p(o4), p(w1), p(w1)),
                 (p(c4), p(b2), 1, 3, 1, q(sel), p(o4), p(w1), p(w1)), (p(cv), p(b2), 1, 2, 1, q(sel), p(o4), p(w1), p(w1))):
        assert L.mcmcx_samples_mpsrf(*args) == -55 and len(L.mcmcx_last_error()) > 0, args[2:5]
    b3 = np.array([3.0, 0.0, 0.5, 2.0])                         # an odd number of split chains
    assert L.mcmcx_samples_mpsrf(p(np.array([6.0, 0.0, 1.0, 9.0])), p(b3), 1, 2, 1, q(sel), p(o4), p(w1), p(w1)) == -55
    assert np.all(o4 == 7.0) and np.all(e1 == 7.0) and np.all(w1 == 7.0)
    out = np.full(8, 7.0)
    for fn in (L.mcmcx_samples_cov_bm, L.mcmcx_samples_cov_bm_dev):
        assert fn(None, 0, 4, 2, None, p(out)) == -55 and b"null handle" in L.mcmcx_last_error()
    # the debug entry checks its arguments before it looks for a device
    assert L.mcmcx_debug_samples_cov_bm(0, 4, 1, 2, 1, None, None, p(out)) == -55
    assert L.mcmcx_debug_samples_cov_bm(0, 4, 1, 2, 1, p(cv), None, None) == -55
    for nch, nf, ns, batch in ((0, 1, 2, 1), (4, 0, 2, 1), (4, 1, 0, 1), (4, 2048, 2, 1), (4, 1, 2, 0), (4, 1, 2, 3), (4, 1, 2, -1)):
        assert L.mcmcx_debug_samples_cov_bm(0, nch, nf, ns, batch, p(cv), None, p(out)) == -55, (nch, nf, ns, batch)
    assert np.all(out == 7.0)
    with pytest.raises(McmcError):
        samples_mess(np.zeros(5), bv, 1, 2, [0])
    with pytest.raises(McmcError):
        samples_mpsrf(c4, b2, 1, 2, [0, 0])


def test_bm_kernels_keep_their_accumulators_in_registers():
    """The build's report of the shipped code object: the bm_ rows are exactly bm_tile_kernel's instantiations -- NS = 1 .. 4 of form A,
    of which <2, false> is form B's diagonal too, and <4, true>, form B's pairs: five kernels (cov_pack_kernel, the covariance's sixth row,
    is used as it is) -- every one without scratch and without a vector or scalar spill, at the covariance's LDS."""
    rows = {}
    for line in open(os.path.join(ROOT, "profiles", "kernel_resources.txt")):
        if line.startswith("bm_"):
            f = line.split()
            rows[" ".join(f[:-9])] = dict(zip(("vgpr", "agpr", "sgpr", "scratch", "vspill", "sspill", "lds", "wg", "waves"), map(int, f[-9:])))
    assert sorted(rows) == ["bm_tile_kernel<1, false>", "bm_tile_kernel<2, false>", "bm_tile_kernel<3, false>", "bm_tile_kernel<4, false>",
                            "bm_tile_kernel<4, true>"], sorted(rows)
    for name, r in rows.items():
        assert r["scratch"] == r["vspill"] == r["sspill"] == 0, (name, r)
        assert r["waves"] >= 1 and r["wg"] == 64
    assert rows["bm_tile_kernel<4, false>"]["lds"] == 64 * 65 * 8 + 64 * 8
