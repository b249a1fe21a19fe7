"""The oracle against the REAL reference where sums of squares are +inf, NaN or subnormal and where sigma2 is infinite
(tests/edge_problems.py; fixtures tests/golden/edge/, oracle/gen_golden.py's edge_cases(): one chain of 170 iterations each, whole chains).

Every GPU test of these inputs compares the engine with the oracle, so the oracle has to be the reference's there first.  What the reference
does (flang -O2, the fixtures are its word):
 - a NaN alpha draws no uniform and rejects: every comparison of MCMC_alpha and MCMC_reject is false (MCMC_DRAM.F90:100-118, 140-155),
   min(1, NaN) is NaN in MCMC_DR_alpha13 (:178, 185) -- the stream position of x1, x2, x7 pins it;
 - early rejection ACCEPTS a proposal whose ss is NaN (`ss2 >= sscrit` is false, MCMC_run_er.F90:72-78), then sits on ss1 = NaN, where sscrit is
   NaN and every proposal is accepted, +inf included, until a finite one comes (x5, x6: NaN and +inf rows in sschain);
 - method = 'ram' STOPS at the first NaN alpha: a = NaN fails `a >= 0` (MCMC_run_ram.F90:166-171), dchdd's `norm < 1` fails on NaN
   (dchdd.f:150-153) and choldowndate stops (matutils.F90:719-722).  x3 holds the iteration (stop_at) and the run up to the one before; the
   oracle reports the same iteration as ram_downdate_fail, and with continue_on_downdate_fail -- what the engine does for a million chains --
   leaves the factor untouched and goes on;
 - sigma2 = +inf out of MCMC_updatesigma2 (1 / gamma with the gamma draw underflowing to 0) makes alpha 1 or NaN (x7);
 - a subnormal mcmcsigma2.dat is read exactly and nothing is flushed: x8 .. x10 have the run lengths and stream position of the unit-scale run.
The same problems run live against oracle/_ref where it is built, on further chains."""
import os

import numpy as np
import pytest

import edge_problems as ep
from golden_util import GOLDEN, load, accepted_from_runlen

RTOL = 1e-7      # rows relative to the column scale, ss and sigma2 relative: tests/test_oracle_golden.py's
DENORM_MIN = 5e-324


def _names():
    return sorted(f[:-4] for f in os.listdir(os.path.join(GOLDEN, "edge")) if f.endswith(".npz"))


def _ss_atol(prob):
    """Oracle and reference hand mcxt_ss_gauss states that differ in their last bits (another BLAS in the proposal).  Above the subnormal range
    that is RTOL's business.  Inside it every operation rounds to a multiple of 2**-1074 whatever the operand's size: the npar fma of a row's
    y_i may each move by one such step, y_i v_i carries them times |v_i| < 3 and rounds again, as does each of the npar additions:
    npar (3 npar + 2) steps at the most."""
    d = prob.npar
    return d * (3 * d + 2) * DENORM_MIN if ep.is_subnormal(prob.sigma2) else 0.0


def _compare(o, chain, sschain, s2chain, chaincmat, chainmean, rng_n, prob, what=""):
    assert o.rng_n == int(rng_n), what                                              # the stream position: the random_number log
    assert o.chainind == chain.shape[0], what
    np.testing.assert_array_equal(o.chain[:, -1].astype(np.int64), chain[:, -1].astype(np.int64), err_msg=what)       # run-length column
    np.testing.assert_array_equal(o.accepted, accepted_from_runlen(chain[:, -1]), err_msg=what)
    assert np.isfinite(chain).all() and np.isfinite(chaincmat).all() and np.isfinite(chainmean).all(), what        # the reference's states stay finite
    scale = np.maximum(np.abs(chain[:, :-1]).max(axis=0), 1e-3)
    assert np.max(np.abs(o.chain[:, :-1] - chain[:, :-1]) / scale) < RTOL, what     # every stored state
    ss_o, ss_r = o.sschain[:, 0], sschain[:, 0]
    np.testing.assert_array_equal(np.isnan(ss_o), np.isnan(ss_r), err_msg=what)     # NaN where the reference has NaN, +-inf where it has +-inf
    inf = np.isinf(ss_r)
    np.testing.assert_array_equal(ss_o[inf], ss_r[inf], err_msg=what)
    fin = np.isfinite(ss_r)
    np.testing.assert_allclose(ss_o[fin], ss_r[fin], rtol=RTOL, atol=_ss_atol(prob), err_msg=what)
    if s2chain is not None:
        inf = np.isinf(s2chain)
        assert not np.isnan(s2chain).any() and np.array_equal(o.s2chain[inf], s2chain[inf]), what
        np.testing.assert_allclose(o.s2chain[~inf], s2chain[~inf], rtol=RTOL, err_msg=what)
    cs = np.max(np.abs(chaincmat))
    assert np.max(np.abs(o.chaincmat - chaincmat)) <= 1e-9 * cs, what
    np.testing.assert_allclose(o.chainmean, chainmean, rtol=1e-9, atol=1e-9 * np.abs(chainmean).max() + 1e-12, err_msg=what)


# what each fixture must hold for the comparison to say anything: (ss = NaN rows or NaN alphas, ss = +inf proposals) at least
REGIME = {"x1_ovf7_am": (3, 20), "x2_ovf13_dr": (3, 8), "x3_ovf20_ram": (0, 4), "x4_ovf12_scam": (3, 50), "x5_ovf9_er": (3, 20), "x6_ovf9_er_priors": (3, 20),
          "x7_ovf10_s2inf": (3, 20)}


@pytest.mark.parametrize("name", _names())
def test_oracle_matches_the_reference_edge_fixture(oracle, name):
    z, cfg, prob = load("edge/" + name, oracle)
    assert cfg.nsimu == 170 or int(z["stop_at"]) == cfg.nsimu + 1
    o = oracle.run_chain(cfg, prob, chain_id=int(z["chain_id"]))
    assert o.rc == 0 and not o.ram_downdate_fail
    _compare(o, z["chain"], z["sschain"], z["s2chain"] if "s2chain" in z.files else None, z["chaincmat"], z["chainmean"], z["rng_n"], prob, name)
    if name in REGIME:
        assert o.n_ss_nan >= REGIME[name][0] and o.n_ss_inf >= REGIME[name][1], (o.n_ss_nan, o.n_ss_inf)
        if cfg.method == 3:                                     # early rejection: the reference's own sschain shows the accepted NaN (and what follows it)
            ss = z["sschain"][:, 0]
            assert np.isnan(ss).sum() >= 3 and np.isinf(ss).any()
            assert "priors" not in name or o.erstayed >= 3      # ... and the prior alone rejected
        elif int(z["stop_at"]) == 0 and not cfg.doscam:         # (SCAM's trace holds the last component's alpha only)
            assert np.isnan(o.alpha).sum() >= REGIME[name][0]
    else:
        ss = z["sschain"][:, 0]                                 # the reference's own values are non-zero subnormals, all of them
        assert ep.is_subnormal(ss).all() and o.n_ss_nan == 0 and o.n_ss_inf == 0
    if "s2chain" in z.files:
        assert 0.1 < np.isinf(z["s2chain"]).mean() < 0.9
    if int(z["stop_at"]):
        # the reference stops at iteration stop_at; so does the oracle, on a NaN alpha; told to go on, it keeps the factor it had
        k = int(z["stop_at"])
        ckw = {f: getattr(cfg, f) for f, _ in oracle.Cfg._fields_ if f not in ("dodr", "doscam", "usesvd")}
        cfg170 = oracle.make_cfg(**dict(ckw, nsimu=170))
        o = oracle.run_chain(cfg170, prob, chain_id=int(z["chain_id"]))
        assert o.rc == -3000 and o.simuind == k and o.ram_downdate_fail == k and np.isnan(o.alpha[k - 1]) and np.isnan(o.alpha12)
        o = oracle.run_chain(cfg170, prob, chain_id=int(z["chain_id"]), continue_on_downdate_fail=True)
        assert o.rc == 0 and o.simuind == 170 and o.ram_downdate_fail == k and np.isfinite(o.R).all() and np.isfinite(o.theta).all()
        assert np.isnan(o.alpha[1:]).sum() >= 3


def test_subnormal_fixtures_are_the_unit_scale_chain(oracle):
    """sigma2 = t and Lam = t Lam0 with t a power of two: nothing but the size of ss depends on t unless something is flushed or misread.  The
    reference's runs at t = 2**-1030 and 2**-1060 have one run-length column and one stream position, which are the oracle's at t = 1."""
    z8, cfg, _ = load("edge/x8_sub20_am", oracle)
    z10, _, _ = load("edge/x10_sub20_am_1060", oracle)
    assert int(z8["chain_id"]) == int(z10["chain_id"])
    o = oracle.run_chain(cfg, oracle.Problem(**ep.subnormal(20, 1.0)), chain_id=int(z8["chain_id"]))
    for z in (z8, z10):
        assert int(z["rng_n"]) == o.rng_n
        np.testing.assert_array_equal(z["chain"][:, -1], o.chain[:, -1])
        assert 0.1 < 1.0 - (z["chain"].shape[0] - 1) / 169.0 < 0.95       # (a flushed ss = 0 accepts everything)


LIVE = [(n, c) for n in ("x1_ovf7_am", "x2_ovf13_dr", "x3_ovf20_ram", "x4_ovf12_scam", "x5_ovf9_er", "x6_ovf9_er_priors", "x7_ovf10_s2inf", "x8_sub20_am",
                         "x9_sub20_ram") for c in (8, 9, 10)]


@pytest.mark.parametrize("name,chain_id", LIVE)
def test_oracle_equals_reference_live_on_the_edge_problems(oracle, name, chain_id):
    """The fixtures' problems on three further chains each, against oracle/_ref where it is built."""
    from oracle import refrun as rr
    if not rr.available():
        pytest.skip("oracle/_ref/mcxref not built (needs /root/reference)")
    _, cfg, prob = load("edge/" + name, oracle)
    ckw = {f: getattr(cfg, f) for f, _ in oracle.Cfg._fields_ if f not in ("dodr", "doscam", "usesvd")}
    ckw["nsimu"] = 170
    cfg = oracle.make_cfg(**ckw)
    o = oracle.run_chain(cfg, prob, chain_id=chain_id)
    if o.ram_downdate_fail:                                     # the reference stops there: at that iteration, not before
        k = int(o.ram_downdate_fail)
        assert np.isnan(o.alpha[k - 1])
        assert rr.run_reference(oracle.make_cfg(**dict(ckw, nsimu=k)), prob, chain_id=chain_id, allow_stop=True).stopped
        cfg = oracle.make_cfg(**dict(ckw, nsimu=k - 1))
        o = oracle.run_chain(cfg, prob, chain_id=chain_id)
        assert not o.ram_downdate_fail
    if cfg.method != 1 and name.startswith("x8"):
        # (fewer accepted rows than parameters at a tick: the Cholesky factor of a singular covariance is the BLAS's rounding noise -- the
        #  ill-posed ticks of tests/test_oracle_fuzz_reference.py.  Chains 8 .. 10 of x8 have their rows; this guards the claim)
        assert o.chainind > 0
    r = rr.run_reference(cfg, prob, chain_id=chain_id, pinned_svd=bool(cfg.usesvd))
    _compare(o, r.chain, r.sschain, r.s2chain if cfg.updatesigma else None, r.chaincmat, r.chainmean, r.rng_n, prob, "%s chain %d" % (name, chain_id))
