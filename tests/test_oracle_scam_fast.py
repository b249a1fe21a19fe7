"""The oracle's restatement of mcmcx_config::scam_fast (oracle/mcx_oracle.h, the chain's scam_fast switch), on its own -- no GPU.

The engine's opt-in SCAM proposal is newpar_k = fma(zj, U(k,j), oldpar_k) with zj = normal * qcovstd_j the sub-step's first draw, in place of the
reference's U (U'oldpar + zj e_j) (MCMC_run_scam.F90:106-115).  The GPU tests hold every kernel form of it to this restatement bit for bit
(tests/test_gpu_every_chain.py, tests/test_gpu_pooled.py, tests/test_gpu_scam_fast.py); what ties the restatement itself down is here:

 - to the REFERENCE: its three SCAM fixtures (real reference, several adaptations each) -- the same run-length column and stream position,
   rows and moments to rounding level;
 - to the DEFAULT oracle, bit for bit, wherever the two forms are the same arithmetic: a rotation that is a signed permutation (products
   by 0 and +-1 are exact, so U'x and U y are), and in bits NOT equal once an adaptation has produced a general rotation;
 - to EXACT arithmetic: on a flat target every sub-step is accepted and draws no uniform, so the state after an iteration is a function of
   the normals alone, restated here in rationals and rounded once per element -- which an unfused zj * U(k,j) + oldpar_k, U(j,k) for
   U(k,j), or a deviate from another place in the stream each miss;
 - and, with the switch off, run_chain is what it was: one fixture per method."""
import ctypes as C
from fractions import Fraction

import numpy as np
import pytest
from golden_util import load, accepted_from_runlen

SCAM_FIXTURES = ["s1_gauss6_scam", "s4_expdata_scam_s2", "s5_banana20_scam"]


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _same(a, b):
    """every reference-visible output of two runs, bit for bit"""
    for k in ("chain", "sschain", "s2chain", "alpha", "R", "chaincmat", "chainmean", "qcovstd", "theta"):
        np.testing.assert_array_equal(_bits(getattr(a, k)), _bits(getattr(b, k)), err_msg=k)
    np.testing.assert_array_equal(a.accepted, b.accepted)
    assert (a.rng_n, a.rng_saved, a.stayed, a.nprop, a.chainind, a.simuind) == (b.rng_n, b.rng_saved, b.stayed, b.nprop, b.chainind, b.simuind)
    assert _bits(a.rng_saved_y) == _bits(b.rng_saved_y) and _bits(a.ss1) == _bits(b.ss1) and _bits(a.chainwsum) == _bits(b.chainwsum)


@pytest.mark.parametrize("name", SCAM_FIXTURES)
def test_fast_oracle_reproduces_the_reference_scam_fixtures(oracle, name):
    """Run-length column and stream position identical; head rows, tail rows, final covariance and mean within 1e-6 relative, scaled as
    tests/test_gpu_scam_fast.py scales them.  Measured (the print below; DESIGN.md section 8 records them): 5.5e-12 for s1_gauss6_scam,
    1.5e-13 for s4_expdata_scam_s2, 5.5e-11 for s5_banana20_scam (the tail rows, after 14, 19 and 3 adaptations)."""
    z, cfg, prob = load(name, oracle)
    o = oracle.run_chain(cfg, prob, chain_id=int(z["chain_id"]), scam_fast=True)
    assert o.rc == 0 and o.simuind == cfg.nsimu
    np.testing.assert_array_equal(o.chain[:, -1].astype(np.int32), z["runlen"])
    np.testing.assert_array_equal(o.accepted, accepted_from_runlen(z["runlen"]))
    assert o.rng_n == int(z["rng_n"]) and o.chainind == int(z["chainind"])
    k = z["rows_head"].shape[0]
    scale = np.maximum(np.abs(z["rows_tail"]).max(axis=0), 1e-3)
    dev = [np.max(np.abs(o.chain[:k, :-1] - z["rows_head"]) / scale), np.max(np.abs(o.chain[-k:, :-1] - z["rows_tail"]) / scale),
           np.max(np.abs(np.triu(o.chaincmat) - np.triu(z["chaincmat"]))) / np.max(np.abs(z["chaincmat"])),
           np.max(np.abs(o.chainmean - z["chainmean"])) / max(np.max(np.abs(z["chainmean"])), 1e-300)]
    print("%s: fast oracle against the reference, head rows / tail rows / covariance / mean: %s" % (name, ["%.2e" % v for v in dev]))
    assert max(dev) < 1e-6, dev


def _diag_problem(d=7, nsimu=60):
    """A correlated Gaussian target started from a DIAGONAL covariance whose entries are not sorted: the pinned SVD returns a permutation,
    and with adaptint = nsimu no tick replaces it before the run ends."""
    r = np.random.default_rng(77)
    A = r.standard_normal((d, d)) / np.sqrt(d)
    ckw = dict(nsimu=nsimu, method="scam", adaptint=nsimu, updatesigma=0)
    pkw = dict(kind="gauss", npar=d, par0=np.full(d, 0.1), cmat0=np.diag([0.3, 0.9, 0.1, 0.7, 0.2, 1.1, 0.5][:d]), mu=np.linspace(-0.5, 0.5, d), lam=A @ A.T + np.eye(d))
    return ckw, pkw


def test_fast_equals_default_bit_for_bit_where_the_rotation_is_a_permutation(oracle):
    ckw, pkw = _diag_problem()
    cfg, prob = oracle.make_cfg(**ckw), oracle.Problem(**pkw)
    for cid in (0, 5, 69):
        a = oracle.run_chain(cfg, prob, chain_id=cid)
        b = oracle.run_chain(cfg, prob, chain_id=cid, scam_fast=True)
        R = oracle.run_chain(cfg, prob, chain_id=cid, upto=cfg.nsimu - 1, scam_fast=True).R     # the only tick is at nsimu: every proposal used this one
        assert np.isin(R, (0.0, 1.0, -1.0)).all() and (np.abs(R).sum(axis=0) == 1).all() and (np.abs(R).sum(axis=1) == 1).all()
        assert not np.array_equal(np.abs(R), np.eye(prob.npar))         # ... and not the identity: a column index taken for a row index shows
        assert 0.5 < np.minimum(a.alpha[1:], 1.0).mean() < 0.95        # sub-steps are accepted AND rejected (the last component's alpha)
        _same(a, b)


def test_fast_equals_default_bit_for_bit_at_a_signed_permutation(oracle):
    """The same with signs: a rotation set from outside (LiveChain.set_R), three of its columns negative and no column in its own place."""
    ckw, pkw = _diag_problem()
    d = pkw["npar"]
    cfg, prob = oracle.make_cfg(**ckw), oracle.Problem(**pkw)
    perm, sign = np.array([3, 0, 6, 1, 5, 2, 4]), np.array([1.0, -1.0, 1.0, -1.0, 1.0, 1.0, -1.0])
    U = np.zeros((d, d)); U[perm, np.arange(d)] = sign
    std = np.sqrt(np.array([1.1, 0.9, 0.7, 0.5, 0.3, 0.2, 0.1]))
    for cid in (0, 64):
        lcs = [oracle.LiveChain(cfg, prob, chain_id=cid, scam_fast=f) for f in (False, True)]
        for lc in lcs:
            lc.set_R(U); lc.set_qcovstd(std)
            lc.run(cfg.nsimu - 1)                               # (the tick at nsimu would replace the factor)
            R = np.ctypeslib.as_array(lc.ch.contents.R, shape=(d, d)).T
            assert np.isin(R, (0.0, 1.0, -1.0)).all() and np.array_equal(R, U) and (R < 0).sum() == 3
        a, b = lcs
        np.testing.assert_array_equal(_bits(a.theta), _bits(b.theta))
        np.testing.assert_array_equal(a.accepted, b.accepted)
        assert a.ch.contents.rng.n == b.ch.contents.rng.n and a.ch.contents.rng.saved == b.ch.contents.rng.saved
        n = a.ch.contents.chainind
        assert n == b.ch.contents.chainind and n > 40
        rows = [np.ctypeslib.as_array(lc.ch.contents.chain, shape=(cfg.nsimu, d + 1))[:n] for lc in lcs]
        np.testing.assert_array_equal(_bits(rows[0]), _bits(rows[1]))
        assert 0 < a.accepted.sum() and a.alpha12 == b.alpha12
        for lc in lcs:
            lc.close()


def test_fast_departs_from_default_in_bits_once_the_rotation_is_general(oracle):
    """After the first adaptation of a correlated target the rotation is a general orthogonal matrix: the two forms are another arithmetic
    (the switch does something), and draw in the same order (the accept sequence over the run stays equal)."""
    ckw, pkw = _diag_problem(nsimu=60)
    ckw["adaptint"] = 20
    cfg, prob = oracle.make_cfg(**ckw), oracle.Problem(**pkw)
    for cid in (0, 5):
        _same(oracle.run_chain(cfg, prob, chain_id=cid, upto=20), oracle.run_chain(cfg, prob, chain_id=cid, upto=20, scam_fast=True))
        a, b = oracle.run_chain(cfg, prob, chain_id=cid), oracle.run_chain(cfg, prob, chain_id=cid, scam_fast=True)
        assert not np.isin(a.R, (0.0, 1.0, -1.0)).all()
        assert not np.array_equal(_bits(a.theta), _bits(b.theta)) and not np.array_equal(_bits(a.chain[21:]), _bits(b.chain[21:]))
        np.testing.assert_array_equal(a.accepted, b.accepted)
        assert a.rng_n == b.rng_n and a.chainind == b.chainind
        assert np.max(np.abs(a.theta - b.theta)) < 1e-9


def test_fast_candidate_is_one_fused_multiply_add_of_the_first_draw(oracle):
    """sigma2 = 1e300 makes the target flat: (ss2 - ss1) / sigma2 underflows against 1, alpha is 1.0, every sub-step is accepted and none
    draws a uniform -- the stream holds the normals only, and the state after iteration i is the start point with
    theta_k <- fma(zj, U(k,j), theta_k) applied for j = 0..npar-1, i - 1 times over.  Restated in rationals, rounded once per element
    (float(Fraction) rounds to nearest even), with the normals drawn from a copy of the chain's own generator."""
    d, nsimu = 5, 7
    r = np.random.default_rng(5)
    A = r.standard_normal((d, d))
    cmat0 = A @ A.T + 0.5 * np.eye(d)
    cmat0 = 0.5 * (cmat0 + cmat0.T)
    ckw = dict(nsimu=nsimu, method="scam", adaptint=nsimu, updatesigma=0)
    pkw = dict(kind="gauss", npar=d, par0=np.linspace(0.3, 1.7, d) / 3.0, cmat0=cmat0, mu=np.zeros(d), lam=np.eye(d), sigma2=1e300)
    cfg, prob = oracle.make_cfg(**ckw), oracle.Problem(**pkw)
    L = oracle.lib()
    for cid in (0, 9):
        lc = oracle.LiveChain(cfg, prob, chain_id=cid, scam_fast=True)
        g = oracle.Rng.from_buffer_copy(lc.ch.contents.rng)
        U = np.ctypeslib.as_array(lc.ch.contents.R, shape=(d, d)).T.copy()
        std = np.ctypeslib.as_array(lc.ch.contents.qcovstd, shape=(d,)).copy()
        assert not np.isin(U, (0.0, 1.0, -1.0)).any() and not np.allclose(U, U.T)      # a general rotation: U(k,j) is not U(j,k)
        lc.run(nsimu - 1)
        th = [Fraction(float(v)) for v in prob.par0]
        unfused_differs = 0
        for it in range(2, nsimu):
            for j in range(d):
                zj = L.mcxo_normal(C.byref(g)) * std[j]
                for k in range(d):
                    unfused_differs += float(zj * U[k, j]) + float(th[k]) != float(Fraction(zj) * Fraction(U[k, j]) + th[k])
                    th[k] = Fraction(float(Fraction(zj) * Fraction(U[k, j]) + th[k]))
        assert unfused_differs > 10                             # the case tells the fused form from the unfused one
        np.testing.assert_array_equal(_bits(lc.theta), _bits([float(v) for v in th]))
        assert lc.accepted.all() and lc.ch.contents.chainind == nsimu - 1
        assert (lc.ch.contents.rng.n, lc.ch.contents.rng.saved) == (g.n, g.saved)      # nothing but the normals was drawn
        lc.close()


@pytest.mark.parametrize("name", ["c3_banana20_dram", "c4_gauss50_ram", "s1_gauss6_scam", "e7_gauss10_er"])
def test_switch_off_leaves_run_chain_as_it_was(oracle, name):
    """The switch sits at the end of the chain struct (mirrored in pyoracle.Chain): with it off -- by default and spelled out -- every method
    gives the fixture's run-length column, stream position and rows as before, and the fields in front of it read as before."""
    z, cfg, prob = load(name, oracle)
    a = oracle.run_chain(cfg, prob, chain_id=int(z["chain_id"]))
    b = oracle.run_chain(cfg, prob, chain_id=int(z["chain_id"]), scam_fast=False)
    _same(a, b)
    assert a.rc == 0 and a.rng_n == int(z["rng_n"]) and a.chainind == int(z["chainind"])
    np.testing.assert_array_equal(a.chain[:, -1].astype(np.int32), z["runlen"])
    k = z["rows_head"].shape[0]
    scale = np.maximum(np.abs(z["rows_tail"]).max(axis=0), 1e-3)
    assert np.max(np.abs(a.chain[:k, :-1] - z["rows_head"]) / scale) < 1e-7 and np.max(np.abs(a.chain[-k:, :-1] - z["rows_tail"]) / scale) < 1e-7
    assert (a.n_ss_inf, a.n_ss_nan) == (0, 0)                  # (the two counters right in front of the switch)
    fields = [f[0] for f in oracle.Chain._fields_]
    assert fields[-1] == "scam_fast" and fields[-3:-1] == ["n_ss_inf", "n_ss_nan"] and fields.index("continue_on_downdate_fail") < fields.index("qcovstd")
    if cfg.method == 2:                                         # ... and on this SCAM fixture the switch is not a no-op
        f = oracle.run_chain(cfg, prob, chain_id=int(z["chain_id"]), scam_fast=True)
        assert not np.array_equal(_bits(f.theta), _bits(a.theta))
