"""The sample store's posterior covariance without a GPU: the exports, mcmcx_samples_cov_finish against the restatement of include/mcmcx.h's
definition (tests/cov_ref.py), the restatement itself against an independent np.longdouble reference within the derived forward bound, the
finish against numpy's cov / corrcoef, the NaN pattern of a constant field, additivity, the finish's refusals, the packed index, and the
build's resource report of the new kernels."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import cov_ref
from mcmcf90_amd import _lib
from mcmcf90_amd.engine import McmcError, samples_cov_finish, samples_cov_len

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DP = C.POINTER(C.c_double)
NAMES = ("mcmcx_samples_cov_len", "mcmcx_samples_cov", "mcmcx_samples_cov_dev", "mcmcx_samples_cov_finish", "mcmcx_debug_samples_cov")


def _data(seed, ns=20, nf=10, nch=583):
    """Correlated, well-conditioned fields with means of order one: [ns][nf][nch]"""
    rng = np.random.default_rng(seed)
    A = rng.normal(size=(nf, nf)) + 2.0 * np.eye(nf)
    return np.einsum("fg,sgc->sfc", A, rng.normal(size=(ns, nf, nch))) + rng.normal(size=nf)[None, :, None]


@pytest.fixture(scope="module")
def vectors():
    """seed -> (X, restated vector): 583 chains are 640 padded lanes x 20 samples x 55 pairs = 7.0e5 fma each"""
    out = {}
    for seed in range(5):
        X = _data(seed)
        out[seed] = (X, cov_ref.cov_vector_ref(X))
    return out


def test_exports_exist_and_the_header_compiles_as_c(tmp_path):
    L = _lib.load()
    for n in NAMES:
        assert n in _lib.SYMBOLS and getattr(L, n) is not None, n
    hdr = open(os.path.join(ROOT, "include", "mcmcx.h")).read()
    for n in NAMES:
        assert re.search(r"\b%s\s*\(" % n, re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)), n
    assert hdr.count("no counterpart in the reference") >= 5
    src = tmp_path / "use.c"
    src.write_text('#include "mcmcx.h"\nint main(void) { double v[6] = {4, 0, 0, 1, 2, 3}, m[1], c[1]; '
                   'return mcmcx_samples_cov_finish(v, 1, m, c, 0) != -51 ? 0 : 1; }\n')
    p = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I" + os.path.join(ROOT, "include"), "-c", str(src),
                        "-o", str(tmp_path / "use.o")], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert p.returncode == 0, p.stdout.decode()
    assert samples_cov_len(53) == 1 + 106 + 53 * 54 // 2


def test_finish_against_the_restated_finish(vectors):
    """The same operations on both sides; only sqrt and the division order could differ: 1e-13 relative, NaN pattern equal."""
    for seed, (X, vec) in vectors.items():
        got, want = samples_cov_finish(vec, 10), cov_ref.finish_ref(vec, 10)
        for g, w in zip(got, want):
            assert g.shape == w.shape and np.array_equal(np.isnan(g), np.isnan(w)), seed
            assert np.allclose(g, w, rtol=1e-13, atol=0.0, equal_nan=True), seed
        assert np.array_equal(got[1], got[1].T) and np.array_equal(np.diag(got[2]), np.ones(10))
    # a vector with NaN and inf entries: the pattern is the restatement's
    vec = vectors[0][1].copy()
    vec[1 + 10 + 3] = np.nan
    vec[1 + 20 + cov_ref.pair_index(5, 7, 10)] = np.inf
    got, want = samples_cov_finish(vec, 10), cov_ref.finish_ref(vec, 10)
    for g, w in zip(got, want):
        assert np.array_equal(np.isnan(g), np.isnan(w)) and np.array_equal(np.isinf(g), np.isinf(w))
        assert np.allclose(g, w, rtol=1e-13, atol=0.0, equal_nan=True)


def test_restatement_against_the_longdouble_reference(vectors):
    """|G - G_ref| <= 2 n u sum|z_j z_k| and |S - S_ref| <= 2 n u sum|z_j|, u = 2**-53: the forward bound gamma_n sum|a_i b_i| of any
    summation order (derived, not measured)."""
    assert np.finfo(np.longdouble).nmant >= 63
    for seed, (X, vec) in vectors.items():
        S, G, bS, bG = cov_ref.longdouble_ref(X)
        assert vec[0] == 20 * 583 and np.array_equal(vec[1:11], X[0, :, 0])
        eS = np.abs(vec[11:21].astype(np.longdouble) - S)
        eG = np.abs(vec[21:].astype(np.longdouble) - G)
        assert np.all(eS <= bS) and np.all(eG <= bG), (seed, float((eS / bS).max()), float((eG / bG).max()))


def test_finish_against_numpy_cov_and_corrcoef(vectors):
    for seed, (X, vec) in vectors.items():
        flat = X.transpose(1, 0, 2).reshape(10, -1)
        mean, cov, corr = samples_cov_finish(vec, 10)
        assert np.allclose(mean, flat.mean(axis=1), rtol=1e-10, atol=0.0)
        assert np.allclose(cov, np.cov(flat), rtol=1e-10, atol=0.0)
        assert np.allclose(corr, np.corrcoef(flat), rtol=1e-10, atol=1e-12)


def test_constant_field_gives_its_nan_row_and_column_and_nowhere_else():
    X = _data(11, ns=4, nf=5, nch=65)                           # 128 lanes x 4 x 15 pairs = 7.7e3 fma
    X[:, 3, :] = -2.5
    vec = cov_ref.cov_vector_ref(X)
    mean, cov, corr = samples_cov_finish(vec, 5)
    assert mean[3] == -2.5 and np.all(cov[3] == 0.0) and np.all(cov[:, 3] == 0.0)
    want = np.zeros((5, 5), dtype=bool)
    want[3, :] = want[:, 3] = True
    assert np.array_equal(np.isnan(corr), want)
    assert not np.isnan(mean).any() and not np.isnan(cov).any()
    rmean, rcov, rcorr = cov_ref.finish_ref(vec, 5)
    assert np.array_equal(np.isnan(rcorr), want)


def test_vectors_of_disjoint_chain_sets_add_up(vectors):
    X = vectors[1][0]
    shift = X[0, :, 0].copy()
    a = cov_ref.cov_vector_ref(X[:, :, :300], shift)            # 320 + 320 lanes x 20 x 55 = 7.0e5 fma
    b = cov_ref.cov_vector_ref(X[:, :, 300:], shift)
    tot = a + b
    tot[1:11] = shift
    S, G, bS, bG = cov_ref.longdouble_ref(X, shift)
    assert tot[0] == 20 * 583
    assert np.all(np.abs(tot[11:21].astype(np.longdouble) - S) <= bS) and np.all(np.abs(tot[21:].astype(np.longdouble) - G) <= bG)
    whole = samples_cov_finish(vectors[1][1], 10)
    parts = samples_cov_finish(tot, 10)
    # the finish divides by n - 1 what the bound covers; the covariances are of order one to a hundred here
    J, K = cov_ref.all_pairs(10)
    n = tot[0]
    # both sides lie within the bound of the exact sums; the finish's own four roundings are 4 u (|G| + |S_j S_k| / n) at the most on each
    tol = (2.0 * bG + 2.0 * (bS[J] * np.abs(S[K]) + bS[K] * np.abs(S[J]) + bS[J] * bS[K]) / n
           + 8.0 * cov_ref.U * (np.abs(G) + np.abs(S[J] * S[K]) / n)) / (n - 1.0)
    assert np.all(np.abs(parts[1][J, K] - whole[1][J, K]) <= np.asarray(tol, dtype=np.float64))
    assert np.allclose(parts[0], whole[0], rtol=1e-12, atol=0.0)


def test_every_finish_refusal_is_minus_51():
    L = _lib.load()
    v = np.array([4.0, 0.0, 0.0, 1.0, 0.5, 2.0])                # nfields 1 has 4 doubles; 2 has 8: built per case below
    m, c, r = np.full(4, 7.0), np.full(16, 7.0), np.full(16, 7.0)
    p = lambda a: a.ctypes.data_as(DP)
    good = np.array([4.0, 0.0, 1.0, 2.0])
    assert L.mcmcx_samples_cov_finish(p(good), 1, p(m), p(c), None) == 0 and m[0] == 0.25
    m[:] = 7.0; c[:] = 7.0
    assert L.mcmcx_samples_cov_finish(None, 1, p(m), p(c), p(r)) == -51 and b"null" in L.mcmcx_last_error()
    assert L.mcmcx_samples_cov_finish(p(good), 1, None, p(c), p(r)) == -51
    assert L.mcmcx_samples_cov_finish(p(good), 1, p(m), None, p(r)) == -51
    for nf in (0, -3):
        assert L.mcmcx_samples_cov_finish(p(good), nf, p(m), p(c), p(r)) == -51 and b"nfields" in L.mcmcx_last_error()
    for n in (1.0, 0.0, -2.0, 2.5, 1e6 + 0.5, np.nan, -np.inf):
        bad = good.copy()
        bad[0] = n
        assert L.mcmcx_samples_cov_finish(p(bad), 1, p(m), p(c), p(r)) == -51 and b"integer" in L.mcmcx_last_error(), n
    assert np.all(m == 7.0) and np.all(c == 7.0) and np.all(r == 7.0)
    assert L.mcmcx_samples_cov_len(None) == -51
    out = np.full(8, 7.0)
    for fn in (L.mcmcx_samples_cov, L.mcmcx_samples_cov_dev):
        assert fn(None, 0, 1, None, p(out)) == -51 and b"null handle" in L.mcmcx_last_error()
    # the debug entry checks its arguments before it looks for a device
    assert L.mcmcx_debug_samples_cov(0, 4, 1, 1, None, None, p(out)) == -51
    assert L.mcmcx_debug_samples_cov(0, 4, 1, 1, p(good), None, None) == -51
    for nch, nf, ns in ((0, 1, 1), (4, 0, 1), (4, 1, 0), (4, 2048, 1)):
        assert L.mcmcx_debug_samples_cov(0, nch, nf, ns, p(good), None, p(out)) == -51
    assert np.all(out == 7.0)
    with pytest.raises(McmcError):
        samples_cov_finish(np.zeros(5), 1)
    with pytest.raises(McmcError):
        samples_cov_finish(np.array([1.0, 0.0, 0.0, 0.0]), 1)


@pytest.mark.parametrize("nf", [1, 2, 17])
def test_packed_index_formula(nf):
    """Pair j <= k at j nf - j (j - 1) / 2 + (k - j): the upper triangle by rows, every slot once -- and the finish reads it there."""
    seen = [cov_ref.pair_index(j, k, nf) for j in range(nf) for k in range(j, nf)]
    assert seen == list(range(nf * (nf + 1) // 2))
    vec = np.zeros(samples_cov_len(nf))
    vec[0] = 5.0
    for j in range(nf):
        for k in range(j, nf):
            vec[1 + 2 * nf + j * nf - j * (j - 1) // 2 + (k - j)] = 4.0 * (100 * j + k + 1)
    _, cov, _ = samples_cov_finish(vec, nf)
    for j in range(nf):
        for k in range(j, nf):
            assert cov[j, k] == cov[k, j] == 100 * j + k + 1


def test_cov_kernels_keep_their_accumulators_in_registers():
    """The build's report of the shipped code object (its sha is checked by tests/test_evidence_is_current.py): every kernel of mcx_cov.hpp
    without scratch and without a vector or scalar spill -- the accumulators and the rows in flight are registers only while their indices
    are compile-time ones."""
    rows = {}
    for line in open(os.path.join(ROOT, "profiles", "kernel_resources.txt")):
        if line.startswith("cov_"):
            f = line.split()
            rows[" ".join(f[:-9])] = dict(zip(("vgpr", "agpr", "sgpr", "scratch", "vspill", "sspill", "lds", "wg", "waves"), map(int, f[-9:])))
    assert sorted(rows) == ["cov_pack_kernel", "cov_tile_kernel<1, false>", "cov_tile_kernel<2, false>", "cov_tile_kernel<3, false>",
                            "cov_tile_kernel<4, false>", "cov_tile_kernel<4, true>"], sorted(rows)
    for name, r in rows.items():
        assert r["scratch"] == r["vspill"] == r["sspill"] == 0, (name, r)
    # four blocks of sixteen rows at 65 doubles (the odd stride the operand read needs) and their shifts
    assert rows["cov_tile_kernel<4, false>"]["lds"] == 64 * 65 * 8 + 64 * 8
