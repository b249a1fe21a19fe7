"""Every chain of every per-chain kernel form that is not method = 'ram' -- adaptive Metropolis, delayed rejection, early rejection,
SCAM, the sigma2 update, the response-column target -- and of every form of the adaptation tick against the oracle, beyond eight tiles.

The other tests compare one to four chains of 66..130 with the oracle, on at most three tiles, and the remaining chains only between two
device forms (group against lane, tile_factor_kernel against adapt_post_kernel, blocked against lane SVD) -- which hand their history to
the SAME adapt_pre_kernel / adapt_cov_* / adapt_covb_* / adapt_post_kernel: an error of the tick that depends on where a chain sits
(the fold under the exec mask of whoever accepted, tile = (w / 8 / nblk) * 8 + w % 8 whose first term is zero below nine tiles, the
burn-in branch each lane takes from its own stay count, a ragged group of 4 NW chains, the gamma sampler's rejection loops) is the same on
both sides of every such comparison.  Here 583 chains from chain_id0 = 6 (nine full tiles and seven chains: a ragged tile, a sixteen-lane
group wave that ends with three chains and a quad wave with seven, tiles 8 and 9 in the second round of the XCD round-robin) run with a
cut at a tick and one right behind it, and EVERY chain's state, accept sequence, scalars, stream position, counters, factor(s) and
covariance must be the oracle's (MCMC_run.F90:41-107, MCMC_run_er.F90:46-104, MCMC_run_scam.F90:38-117, MCMC_adapt.F90:12-230,
matutils.F90:283-338), bit for bit.  The regime of every case is asserted from the oracle's results before the engine runs (_regime): a first-stage acceptance
rate of 0.1..0.5 for the Gaussian and response-column targets, so that lanes accept at different iterations; the last component's alpha for
SCAM; the high-acceptance regime for banana and for the sigma2 update below shape one, which allows no other; bounds that bite; the three
burn-in branches side by side.  (Pooled mode has one factor for all
chains and its restatement tests compare all of them; method = 'ram' is tests/test_gpu_ram_every_chain.py.)

fast=1 is mcmcx_config::scam_fast, the opt-in componentwise proposal cand_k = fma(zj, U(k,j), theta_k): the oracle restates it behind a
per-chain switch (oracle/mcx_oracle.h, tied to the reference's fixtures by tests/test_oracle_scam_fast.py), and every form that takes it --
the lane kernels at one to eight waves, scam_pooled_kernel<per-chain> with each lane's own column of E.Rf at three layouts of its waves,
the lane kernels that form falls back to under bounds and priors, step_kernel_cols<scam> -- is held to it on every chain like the rest.
A rounding-level tolerance cannot see a wrong column element in a ragged last block, a pad row that is not zero or an unfused multiply-add;
the accept sequence of some chain moves within a few hundred sub-steps of any of them."""
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import edge_problems as ep

pytestmark = pytest.mark.gpu

NCH, CHAIN_ID0 = 583, 6
SWITCHES = ("MCMCX_POOLED_MFMA_DR_MIN", "MCMCX_POOLED_SCALAR", "MCMCX_DR_BIG", "MCMCX_SCAM_POOLED_16", "MCMCX_SCAM_FAST_LANES", "MCMCX_SCAM_WAVES",
            "MCMCX_SVD_LANE", "MCMCX_COV_BATCH_ROWS", "MCMCX_RAM_WIDE", "MCMCX_POOLED_WAVES", "MCMCX_POOLED_KS", "MCMCX_COLS_PHASED", "MCMCX_HOST_MAPPED",
            "MCMCX_HOST_FUSE", "MCMCX_LDS_SCRATCH", "MCMCX_GROUP", "MCMCX_GROUP_DR2", "MCMCX_GROUP_GW", "MCMCX_RAM_GROUP", "MCMCX_TILE_FACTOR",
            "MCMCX_POOLED_PHASE_MFMA")
BOUNDED = (9, 10, 17, 20, 32, 33, 49)           # a third of the Gaussian problems: +-2.5 at these sizes without delayed rejection (and 32 with it)
BURN = dict(doburnin=1, burnintime=90, badaptint=20, greedy=1, scalelimit=0.45, scalefactor=2.0)
BURN_TICKS = (20, 40, 60)


def P(kind, d, **opt):
    """A problem: target kind, npar and what departs from the plain adaptive Metropolis run (hashable: the key of the oracle's cache)."""
    return (kind, d, tuple(sorted(opt.items())))


def _fast(prob):
    return int(dict(prob[2]).get("fast", 0))                    # mcmcx_config::scam_fast on the engine, scam_fast=True on the oracle's chains


def _bounded(prob):
    opt = dict(prob[2])
    return prob[0] == "gauss" and "edge" not in opt and bool(opt.get("bounded", prob[1] in BOUNDED and not opt.get("drscale")))


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _problem(prob):
    """(cfg keywords, problem keywords, chains, run cuts) of a problem.  Gaussian targets start from the target's own covariance, cmat0 = inv(lam),
    where a chain of the plain cases accepts one proposal in three to six (tests/test_gpu_ram_every_chain.py's construction; _regime has every case's range); banana keeps tests/test_gpu_group.py's start."""
    kind, d, opt = prob[0], prob[1], dict(prob[2])
    ckw = dict(nsimu=opt.get("nsimu", 170), method=opt.get("method", "dram"), adaptint=50, updatesigma=0, drscale=opt.get("drscale", 0.0))
    nch, cuts = opt.get("nch", NCH), (50, 51, 101, None)
    if kind == "cols":                                          # two response columns: tests/test_gpu_ram_every_chain.py's expdata problem,
        # with the proposal a tenth of what method = 'ram' starts from (tests/test_gpu_host_callbacks.py's scale for the other methods): at
        # the RAM file's scale a chain of MCMC_run accepts one proposal in 25, some chains none, and the tick keeps the old factor
        r = np.random.default_rng(31)
        x = np.arange(11.0)
        rates = np.array([0.1, 0.25])
        Y = np.vstack([9.0 * np.exp(-k * x) + r.standard_normal(11) * 0.3 for k in rates])
        pkw = dict(kind="expdata", npar=3, par0=np.concatenate([[9.0], rates]), cmat0=np.diag([0.02, 0.0002, 0.0002]),
                   sigma2=np.array([0.6, 0.9]), nobs=np.array([11, 14]), xdata=x, ydata=Y, lo=np.zeros(3))
        ckw.update(updatesigma=1, N0=1.0, S02=0.0)
        return ckw, pkw, nch, cuts
    if kind == "banana":
        pkw = dict(kind="banana", npar=d, par0=np.full(d, 0.05), cmat0=(2.0 / d) * np.eye(d), b=0.1)
        return ckw, pkw, nch, cuts
    r = np.random.default_rng(3000 + d)
    A = r.standard_normal((d, d)) / np.sqrt(d)
    lam = A @ A.T + np.eye(d)
    pkw = dict(kind="gauss", npar=d, par0=np.full(d, 0.1), cmat0=np.linalg.inv(lam), mu=np.linspace(-0.5, 0.5, d), lam=lam)
    if "edge" in opt:                                           # tests/edge_problems.py: "ovf:T:c" (the pair block), "ar1:T:c", "s2:T:c", "sub:e" (t = 2**-e)
        how, *arg = opt["edge"].split(":")
        if how == "sub":
            pkw = ep.subnormal(d, 2.0 ** -int(arg[0]))
        else:
            pkw = (ep.overflow if how == "ovf" else ep.overflow_ar1)(d, float(arg[0]), float(arg[1]))
        if how == "s2":
            ckw.update(ep.INF_SIGMA2)
            pkw.update(nobs=1)
    if _bounded(prob):
        # (with delayed rejection only the SECOND stage's exits are counted, MCMC_run.F90:49, and its proposals are a third as long: +-1.5)
        b = 1.5 if ckw["drscale"] else 2.5
        pkw.update(lo=np.full(d, -b), hi=np.full(d, b))
    if opt.get("priors"):                                       # every third parameter flat (tests/test_gpu_group.py), the others a unit Gaussian
        pkw.update(pri_mu=np.full(d, 0.1), pri_sig=np.where(np.arange(d) % 3 == 1, -1.0, 1.0))
    if "sigma2" in opt:                                         # (N0, nobs): the gamma sampler's shape (N0 + nobs) / 2 above and below one
        N0, nobs = opt["sigma2"]
        if N0 + nobs > 2:
            # sigma2 settles where N0 S02 + sigma2 npar = sigma2 (N0 + nobs - 2): S02 = 3 keeps it near one (0.14..13 over the chains), so the
            # target stays as wide as cmat0 and a chain accepts three proposals in ten.  (S02 = 0.3 lets it sink to 0.02 and the rate to 0.08.)
            ckw.update(updatesigma=1, N0=N0, S02=3.0)
            pkw.update(sigma2=1.0, nobs=nobs)
        else:
            # shape 0.6: an inverse gamma without a mean -- sigma2 runs up to 1e10, the target flattens and nearly every proposal is
            # accepted whatever S02 is.  A proposal a hundred times cmat0 still has the first stage reject one proposal in seven, so that the
            # second stage and the rejection loops of the shape-below-one sampler run in every wave at every iteration
            ckw.update(updatesigma=1, N0=N0, S02=0.3)
            pkw.update(sigma2=0.5, nobs=nobs, cmat0=100.0 * pkw["cmat0"])
    if opt.get("burnin"):                                       # burn-in ticks at 20, 40, 60, 80; the first AM tick at 140, then 150 and 160
        ckw.update(BURN)
        if not ckw["drscale"]:
            pkw["cmat0"] = 0.3 * pkw["cmat0"]
        cuts = (40, 41, 140, None)
    for k in ("adapthist", "initcmatn", "adaptend"):
        if k in opt:
            ckw[k] = opt[k]
    if "adapthist" in opt:                                      # the AP window's ticks: 100 and 150
        cuts = (100, 101, 150, None)
    if ckw["method"] == "scam" or "condmax" in opt:
        if "condmax" in opt:
            ckw["condmax"] = opt["condmax"]
        # (inv() returns a matrix whose triangles differ in the last bits.  The pinned dgesvd is defined for a symmetric matrix: the engine
        #  mirrors cmat0's upper triangle into it, the oracle hands it the matrix as it stands like the reference -- so the two are given
        #  one)
        pkw["cmat0"] = 0.5 * (pkw["cmat0"] + pkw["cmat0"].T)
    if ckw["nsimu"] < 101:
        cuts = (50, 51, None)
    return ckw, pkw, nch, cuts


_ORACLE = {}


def _pack(rs, nch, d, nsimu):
    """What the comparison needs of a problem's oracle chains, as read-only arrays over the chains."""
    assert len(rs) == nch and all(r.simuind == nsimu and r.rc == 0 for r in rs)
    o = dict(theta=np.array([r.theta for r in rs]), acc=np.array([r.accepted for r in rs], dtype=np.uint8),
             scal=np.array([[r.ss1, r.sspri1, r.sigma2, r.alpha12] for r in rs]), rng=np.array([r.rng_n for r in rs], dtype=np.uint64),
             ctr=np.array([[r.stayed, r.bndstayed, r.drtries, r.draccepted, r.erstayed] for r in rs], dtype=np.int64),
             nprop=np.array([r.nprop for r in rs], dtype=np.int64), ssinf=np.array([r.n_ss_inf for r in rs], dtype=np.int64),
             ssnan=np.array([r.n_ss_nan for r in rs], dtype=np.int64),
             R=np.array([r.R for r in rs]), qstd=np.array([r.qcovstd for r in rs]), R2=np.array([r.R2 for r in rs]), iC=np.array([r.iC for r in rs]),
             cmat=np.array([r.chaincmat for r in rs]), mean=np.array([r.chainmean for r in rs]), wsum=np.array([r.chainwsum for r in rs]),
             alpha=np.array([r.alpha for r in rs]), ss1v=np.array([r.ss1v for r in rs]), s2chain=np.array([r.s2chain for r in rs]).reshape(nch, nsimu, -1))
    assert o["theta"].shape == (nch, d) and o["acc"].shape == (nch, nsimu) and o["R"].shape == o["cmat"].shape == (nch, d, d)
    for v in o.values():
        v.setflags(write=False)
    return o


def _oracle_all(oracle, prob):
    """Every chain of a problem through the oracle: computed once per problem (the forms that share a problem share it), never changed.
    (The oracle keeps no state outside a chain: eight chains at a time.)"""
    if prob not in _ORACLE:
        ckw, pkw, nch, _ = _problem(prob)
        d, nsimu = int(pkw["npar"]), ckw["nsimu"]
        cfg = oracle.make_cfg(**ckw); pr = oracle.Problem(**pkw)
        oracle.lib()
        with ThreadPoolExecutor(8) as pool:
            rs = list(pool.map(lambda c: oracle.run_chain(cfg, pr, chain_id=CHAIN_ID0 + c, scam_fast=bool(_fast(prob))), range(nch)))
        _ORACLE[prob] = _pack(rs, nch, d, nsimu)
    return _ORACLE[prob]


def _regime(prob, o):
    """What makes the case worth running, from the oracle's chains alone.  Every problem passes one of the acceptance branches."""
    kind, d, opt = prob[0], prob[1], dict(prob[2])
    ckw, pkw, nch, _ = _problem(prob)
    nsimu = ckw["nsimu"]
    stayed, bnd, drtries, dracc, erstayed = o["ctr"].T
    rate = o["acc"][:, 1:].mean()                               # (row 0 is the start point)
    # the first stage's rate: with delayed rejection a first-stage rejection is a second-stage try
    rate1 = 1.0 - drtries.sum() / (nch * (nsimu - 1.0)) if ckw["drscale"] else rate
    below_one = "sigma2" in opt and sum(opt["sigma2"]) < 2
    if "edge" in opt:
        # no NaN and no infinity in a state, factor or covariance: the reference's fixtures (tests/golden/edge/) show none
        for k in ("theta", "R", "R2", "iC", "qstd", "cmat", "mean", "wsum"):
            assert np.isfinite(o[k]).all(), k
        tiles = [slice(t, t + 64) for t in range(0, nch - 63, 64)]
        scam = ckw["method"] == "scam"
        if opt["edge"].startswith("sub"):
            ss1 = o["scal"][:, 0]
            assert ep.is_subnormal(ss1).all() and len(np.unique(ss1)) == nch, (ss1.min(), ss1.max(), len(np.unique(ss1)))
            if scam:                                            # (an iteration of SCAM nearly always moves: the last component's alpha, as below)
                a = np.minimum(o["alpha"][:, 1:], 1.0).mean()
                assert rate > 0.9 and 0.5 < a < 0.9, (rate, a)
            else:
                assert 0.1 < rate1 < 0.5, rate1
            return
        ninf, nnan, nprop = o["ssinf"].sum(), o["ssnan"].sum(), float(o["nprop"].sum())
        print("%s: first-stage rate %.3f, ss = +inf %.4f, NaN %.4f of %d proposals" % (prob, rate1, ninf / nprop, nnan / nprop, nprop))
        assert all(o["ssnan"][t].any() for t in tiles) and all(o["ssinf"][t].any() for t in tiles)      # every full tile holds both
        if scam:
            assert ninf > 0 and nnan > 0
        else:
            assert 0.1 < rate1 < 0.75, rate1
            assert ninf >= 0.01 * nprop and nnan >= 0.005 * nprop, (ninf / nprop, nnan / nprop)
        if ckw["updatesigma"]:                                  # the gamma draw overflowed in part of the chains, not in all
            s2 = o["s2chain"][:, 1:, 0]
            print("sigma2 = +inf in %.3f of the draws" % np.isinf(s2).mean())
            assert not np.isnan(s2).any() and 0.05 < np.isinf(s2).mean() < 0.95 and all(np.isinf(s2[t]).any() and np.isfinite(s2[t]).any() for t in tiles)
        if ckw["drscale"]:
            assert dracc.sum() > nch and (drtries - dracc).sum() > nch
        return
    if ckw["method"] == "scam":
        # an iteration is npar one-dimensional steps and `accepted` says that one of them moved, which every iteration does.  The oracle's
        # alpha trace holds the LAST component's alpha of each iteration: a step as long as the target's own standard deviation along its
        # axis is accepted about seven times in ten, so the lanes of a wave diverge at every component
        a = np.minimum(o["alpha"][:, 1:], 1.0).mean()
        assert rate > 0.9 and 0.5 < a < 0.9, (rate, a)
    elif kind == "banana":
        assert 0.5 < rate < 0.95, rate                          # the high-acceptance regime
    elif opt.get("burnin"):
        for t in BURN_TICKS:                                    # MCMC_adapt.F90:60-102: every branch taken by a twentieth of the chains at every tick
            staypc = (o["acc"][:, 1:t] == 0).sum(axis=1) / float(t)
            shrink, grow = staypc > 1.0 - BURN["scalelimit"], staypc < BURN["scalelimit"]
            shares = (shrink.mean(), grow.mean(), (~shrink & ~grow).mean())
            assert min(shares) >= 0.05, (t, shares)
    elif below_one:
        assert 0.7 < rate1 < 0.95, rate1                        # (see _problem: the range this sampler allows)
    else:
        # Gaussian and response-column targets: lanes accept at different iterations, so the window kernels fold under mixed exec masks
        assert 0.1 < rate1 < 0.5, rate1
    if _bounded(prob):
        assert bnd.sum() > nch, bnd.sum()                       # the bounds bite: more than one counted proposal per chain lands outside
        if ckw["drscale"]:
            assert all(bnd[t:t + 64].sum() > 0 for t in range(0, nch - 63, 64))         # ... in every full tile
    if ckw["method"] == "er" and opt.get("priors"):
        assert erstayed.sum() > nch, erstayed.sum()             # the prior alone rejects, more than once per chain
    if ckw["drscale"]:
        assert dracc.sum() > nch and (drtries - dracc).sum() > nch          # second stages accepted and rejected
    if ckw["updatesigma"]:
        s2 = o["scal"][:, 2]
        assert len(np.unique(s2)) == nch                        # every chain its own sigma2
        if below_one:
            assert s2.max() > 1e6 * s2.min()                    # the heavy tail of shape 0.6


LANE, GRP, QUAD = dict(MCMCX_GROUP="0"), dict(MCMCX_GROUP="1", MCMCX_GROUP_GW="16"), dict(MCMCX_GROUP="1", MCMCX_GROUP_GW="4")
AM, LDSV, LDSR = "step_kernel<false, false, false>", "step_kernel_ldsv", "step_kernel_ldsr"


def _cases():
    C = []

    def add(label, prob, kernel, *envs):
        env = {}
        for e in envs:
            env.update(e)
        C.append(pytest.param(prob, kernel, env, id="%s-%s%d%s" % (label, prob[0], prob[1], "".join("_%s%s" % (k, v if not isinstance(v, tuple) else "") for k, v in prob[2]))))
    G = lambda d, **o: P("gauss", d, **o)
    # ---- lane AM: 7 (one ragged block of ten), 10, 11 (the second block of one column), 20, 50, 64 (seven blocks, the last of four) over the three forms
    add("lane", G(7), LDSR, LANE); add("lane", G(10), LDSR, LANE)
    add("lane", G(11), LDSV, LANE, dict(MCMCX_LDS_SCRATCH="1")); add("lane", G(50), LDSV, LANE)
    add("lane", G(20), AM, LANE, dict(MCMCX_LDS_SCRATCH="0")); add("lane", G(64), AM, LANE, dict(MCMCX_LDS_SCRATCH="0"))
    # ---- lane DR: the second stage's vectors in LDS / in global scratch
    add("lane", G(13, drscale=3.0), "step_kernel_dr", LANE, dict(MCMCX_DR_BIG="0"))
    add("lane", P("banana", 20, drscale=2.0), "step_kernel_dr_big", LANE, dict(MCMCX_DR_BIG="1"))
    add("lane", G(32, drscale=3.0, bounded=1), "step_kernel_dr", LANE, dict(MCMCX_DR_BIG="0"))
    # ---- group, sixteen lanes per chain, and the tick's factorisation in both forms on the same problem, against the same oracle:
    # tile_factor_kernel<1, 4> (16), <2, 4> (17, 32), <3, 2> (33, 48), <4, 1> (49, 64) against adapt_post_kernel's own
    for d in (16, 17, 32, 33, 48, 49, 64):
        for tf in ("1", "0"):
            add("group_tf" + tf, G(d), "group_step_kernel", GRP, dict(MCMCX_TILE_FACTOR=tf))
    add("group", G(50), "group_step_kernel", GRP)
    # with delayed rejection: dtrti2 / dlauu2
    for d in (17, 32):
        for tf in ("1", "0"):
            add("group_tf" + tf, G(d, drscale=3.0, bounded=int(d == 32)), "group_step_kernel<DR>", GRP, dict(MCMCX_TILE_FACTOR=tf))
    add("group", G(20, drscale=3.0), "group_step_kernel<DR>", GRP)
    add("group", P("banana", 20, drscale=2.0), "group_step_kernel<DR2>", GRP); add("group", G(24, drscale=2.0), "group_step_kernel<DR2>", GRP)
    # ---- quads
    for d in (1, 10, 16):
        add("quad", G(d), "group_step_kernel<quad>", QUAD)
    add("quad", G(13, drscale=3.0), "group_step_kernel<quad, DR>", QUAD); add("quad", G(15, drscale=2.0), "group_step_kernel<quad, DR2>", QUAD)
    # ---- early rejection: 9 with bounds and priors (the prior alone rejects: erstayed), 20
    er9, er20 = G(9, method="er", priors=1), G(20, method="er")
    add("lane", er9, LDSR, LANE); add("quad", er9, "group_step_kernel<quad>", QUAD)
    add("lane", er20, LDSV, LANE); add("group", er20, "group_step_kernel", GRP)
    # ---- the sigma2 update: the gamma sampler's shape above one, and below (N0 = 0.2, nobs = 1) with delayed rejection
    s7, s13 = G(7, sigma2=(1.0, 11)), G(13, drscale=3.0, sigma2=(0.2, 1))
    add("lane", s7, LDSR, LANE); add("group", s7, "group_step_kernel", GRP); add("quad", s7, "group_step_kernel<quad>", QUAD)
    add("lane", s13, "step_kernel_dr", LANE); add("group", s13, "group_step_kernel<DR>", GRP); add("quad", s13, "group_step_kernel<quad, DR>", QUAD)
    # ---- the tick's covariance: the AP window (every tick takes the batch branch) in blocks and row by row; initcmatn > 0 (the first tick
    # is a Welford tick); adaptend before the last tick (and the first tick's batch branch row by row)
    rows = dict(MCMCX_COV_BATCH_ROWS="1")
    add("group_blocks", G(11, adapthist=50), "group_step_kernel", GRP); add("group_rows", G(11, adapthist=50), "group_step_kernel", GRP, rows)
    add("lane_blocks", G(20, initcmatn=7), AM, LANE, dict(MCMCX_LDS_SCRATCH="0")); add("lane_rows", G(20, initcmatn=7), AM, LANE, dict(MCMCX_LDS_SCRATCH="0"), rows)
    add("group_blocks", G(50, adaptend=120), "group_step_kernel", GRP); add("group_rows", G(50, adaptend=120), "group_step_kernel", GRP, rows)
    # ---- the tick's schedule: shrink, grow and greedy restart in one wave
    b12, b12dr = G(12, burnin=1), G(12, burnin=1, drscale=2.0)
    add("lane", b12, LDSV, LANE); add("group", b12, "group_step_kernel", GRP)
    add("lane", b12dr, "step_kernel_dr", LANE); add("group", b12dr, "group_step_kernel<DR2>", GRP)
    # ---- SVD factors: the lane SVD, and the blocked one (svd_sweep_stream32_kernel<8>) at 135 chains with one tick.  The engine names no
    # tick form: npar 48 is the smallest the plan gives the blocked SVD (svd_blocked(), mcx_host_launch.hpp: 48 <= npar <= 256 unless
    # MCMCX_SVD_LANE is set) -- if that threshold moves up, move this size with it, or the case repeats svd_lane
    svd48 = G(48, condmax=1e8, nch=135, nsimu=60)
    add("svd_lane", G(12, condmax=1e8), LDSV, dict(MCMCX_SVD_LANE="1")); add("svd_lane", G(20, condmax=1e8), LDSV, dict(MCMCX_SVD_LANE="1"))
    add("svd_blocked", svd48, LDSV); add("svd_lane", svd48, LDSV, dict(MCMCX_SVD_LANE="1"))
    # ---- SCAM: one, two, four and eight waves per tile
    for nw, k in ((1, "scam_kernel"), (2, "scam_mw_kernel<2>"), (4, "scam_mw_kernel<4>"), (8, "scam_mw_kernel<8>")):
        add("scam%d" % nw, G(12, method="scam", nsimu=120), k, dict(MCMCX_SCAM_WAVES=str(nw)))
    # ---- two response columns in one launch
    add("cols", P("cols", 3), "step_kernel_cols"); add("cols", P("cols", 3, method="scam"), "step_kernel_cols<scam>")
    # ---- sums of squares that are +inf, NaN or subnormal (tests/edge_problems.py; T and c of every overflow problem chosen on the CPU so that the
    # oracle alone meets _regime's conditions).  The Metropolis decision is restated in every form: a NaN alpha draws no uniform and rejects
    # (MCMC_DRAM.F90:140-155), early rejection accepts a NaN proposal (MCMC_run_er.F90:72-78: the comparison is false)
    SUB = "sub:1030"
    lds0 = dict(MCMCX_LDS_SCRATCH="0")
    for e7, e50, e20 in (("ar1:10:0.3", "ovf:60:0.15", "ovf:25:0.3"), (SUB, SUB, SUB)):
        add("lane", G(7, edge=e7), LDSR, LANE); add("lane", G(50, edge=e50), LDSV, LANE); add("lane", G(20, edge=e20), AM, LANE, lds0)
        add("group", G(20, edge=e20), "group_step_kernel", GRP)
    for e in ("ovf:16:0.3", SUB):
        add("lane", G(13, drscale=3.0, edge=e), "step_kernel_dr", LANE, dict(MCMCX_DR_BIG="0"))
        add("quad", G(13, drscale=3.0, edge=e), "group_step_kernel<quad, DR>", QUAD)
    add("lane_big", G(13, drscale=3.0, edge="ovf:16:0.3"), "step_kernel_dr_big", LANE, dict(MCMCX_DR_BIG="1"))
    for e17, e24, e10 in (("ovf:21:0.3", "ovf:30:0.3", "ovf:12:0.3"), (SUB, SUB, SUB)):
        add("group", G(17, drscale=3.0, edge=e17), "group_step_kernel<DR>", GRP); add("group", G(24, drscale=2.0, edge=e24), "group_step_kernel<DR2>", GRP)
        add("quad", G(10, edge=e10), "group_step_kernel<quad>", QUAD)
    xer9, xer20 = G(9, method="er", priors=1, edge="ovf:11:0.3"), G(20, method="er", edge="ovf:25:0.3")
    add("lane", xer9, LDSR, LANE); add("quad", xer9, "group_step_kernel<quad>", QUAD); add("group", xer20, "group_step_kernel", GRP)
    xs10 = G(10, edge="s2:10:0.3")                              # sigma2 = +inf in a third of the gamma draws: (ss2 - ss1) / inf is 0 or NaN
    add("lane", xs10, LDSR, LANE); add("group", xs10, "group_step_kernel", GRP); add("quad", xs10, "group_step_kernel<quad>", QUAD)
    for e in ("ovf:15:0.5", SUB):
        xsc = G(12, method="scam", nsimu=120, edge=e)
        add("scam1", xsc, "scam_kernel", dict(MCMCX_SCAM_WAVES="1")); add("scam4", xsc, "scam_mw_kernel<4>", dict(MCMCX_SCAM_WAVES="4"))
    # ---- scam_fast, cand = fma(zj, U(:,j), theta), against the oracle's restatement of it.  The lane kernels at one, two, four and eight waves:
    f12 = G(12, method="scam", nsimu=120, fast=1)
    for nw, k in ((1, "scam_kernel"), (2, "scam_mw_kernel<2>"), (4, "scam_mw_kernel<4>"), (8, "scam_mw_kernel<8>")):
        add("fast_lanes%d" % nw, f12, k, dict(MCMCX_SCAM_FAST_LANES="1", MCMCX_SCAM_WAVES=str(nw)))
    # ... the matrix-core form the plan takes by itself, every lane with its own chain's column of E.Rf, at three layouts of its waves:
    # npar 12 is one ragged block (the four group waves alone), 40 three leftover blocks and no block wave, 67 four block waves and one
    # leftover block with a pad row (d4 = 68).  40 and 67 have one tick and a cut right behind it; 12 once more with the sigma2 update
    PC = "scam_pooled_kernel<per-chain>"
    add("fast_tile", f12, PC)
    add("fast_tile", G(40, method="scam", nsimu=60, fast=1), PC); add("fast_tile", G(67, method="scam", nsimu=60, fast=1), PC)
    add("fast_tile", G(12, method="scam", nsimu=120, fast=1, sigma2=(1.0, 11)), PC)
    # ... what that form falls back to: bounds and priors are not its business, so the plan names a lane kernel (ten tiles: eight waves each),
    # and both see the fast candidate
    add("fast_fallback", G(12, method="scam", fast=1, priors=1), "scam_mw_kernel<8>"); add("fast_fallback", G(12, method="scam", fast=1, bounded=1), "scam_mw_kernel<8>")
    add("fast_cols", P("cols", 3, method="scam", fast=1), "step_kernel_cols<scam>")
    # ... and the matrix-core target at +inf and NaN sums of squares: T and c of the reference-order case above meet _regime's edge conditions
    # under the fast oracle as they stand (+inf in 7.7 %, NaN in 1.1 % of the proposals, both in every full tile)
    add("fast_tile", G(12, method="scam", nsimu=120, fast=1, edge="ovf:15:0.5"), PC)
    return C


@pytest.mark.parametrize("prob,kernel,env", _cases())
def test_every_chain_of_a_form_equals_the_oracle(oracle, monkeypatch, prob, kernel, env):
    from mcmcf90_amd import engine_from_problem
    ckw, pkw, nch, cuts = _problem(prob)
    d, nsimu = int(pkw["npar"]), ckw["nsimu"]
    o = _oracle_all(oracle, prob)
    _regime(prob, o)                                            # ... before the engine is touched
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    cols = prob[0] == "cols"                                    # (the recorded chain is the engine's only view of the second column)
    e = engine_from_problem(ckw, pkw, nchains=nch, chain_id0=CHAIN_ID0, record_accept=1, record_chain=1 if cols else 0, scam_fast=_fast(prob))
    e.init()
    failures = _run_and_compare(e, o, ckw, nch, cuts, kernel, edge="edge" in dict(prob[2]), cols=cols)
    assert not failures, "; ".join(failures)


def _run_and_compare(e, o, ckw, nch, cuts, kernel, edge=False, cols=False, instance=None):
    """Run an initialised engine through the cuts, asserting the kernel after each; read every chain, close the engine, and compare every quantity
    on every chain with the oracle's (_pack).  Returns one line per quantity that differs, with the first failing chains.  (tests/test_gpu_accept_extremes.py
    runs its chains through this too: there o carries the expected status bits, and method = 'ram' keeps no covariance.  tests/test_gpu_group_instances.py
    names the template instance(s) behind the table entry as well.)"""
    nsimu, ram = ckw["nsimu"], ckw["method"] == "ram"
    for upto in cuts:
        e.run(upto)
        assert e.last_kernel() == kernel, e.last_kernel()
        assert instance is None or e.last_instance() == instance, e.last_instance()
    assert e.simuind == nsimu
    theta, masks, scal = e.theta(), e.accept_masks(), e.scalars()
    rng = np.array([e.rng(c)[0] for c in range(nch)], dtype=np.uint64)
    ctr = np.array([[k[n] for n in ("stayed", "bndstayed", "drtries", "draccepted", "erstayed", "status")] for k in (e.counters(c) for c in range(nch))], dtype=np.int64)
    ctr, status = ctr[:, :5], ctr[:, 5]
    R = np.array([e.R(c) for c in range(nch)])
    cov = None if ram else [e.chaincov(c) for c in range(nch)]
    qstd = np.array([e.qcovstd(c) for c in range(nch)]) if ckw["method"] == "scam" else None
    dr = [e.dr_state(c) for c in range(nch)] if ckw["drscale"] else None
    rec = [e.chain(c) for c in range(nch)] if cols else None
    e.close()
    c = np.arange(nch)
    assert masks.shape == (nsimu, (nch + 63) // 64)
    acc = ((masks[:, c // 64] >> (c % 64).astype(np.uint64)) & np.uint64(1)).astype(np.uint8).T         # [chain][iteration]
    # no chain is left out
    assert acc.shape == o["acc"].shape and theta.shape == o["theta"].shape and scal.shape == o["scal"].shape and R.shape == o["R"].shape
    assert rng.shape == o["rng"].shape and ctr.shape == o["ctr"].shape and (cov is None or len(cov) == nch) and (dr is None or len(dr) == nch)

    full = ckw["method"] == "scam" or ckw.get("condmax", 0.0) > 0.0     # an SVD factor is a full matrix
    tri = (lambda a: a) if full else (lambda a: np.triu(a))
    failures = []

    def check(name, got, want, nan_ok=False):
        # nan_ok: a NaN equals a NaN whatever its sign and payload (x86 and gfx950 generate different default NaNs).  Everything else bit for bit
        got, want = np.asarray(got), np.asarray(want)
        assert got.shape == want.shape, (name, got.shape, want.shape)
        eq = ep.same_bits_or_nan(got, want) if nan_ok else (_bits(got) == _bits(want)) if got.dtype.kind == "f" else (got == want)
        bad = np.flatnonzero(~eq.reshape(nch, -1).all(axis=1))
        if len(bad):
            failures.append("%s: %d chains, the first: %s" % (name, len(bad), bad[:12]))

    check("accept sequence", acc, o["acc"])
    check("theta", theta, o["theta"])
    for j, name in enumerate(("ss1", "sspri1", "sigma2", "alpha12")):
        if name != "alpha12" or ckw["method"] != "er":          # (MCMC_run_er computes no alpha)
            # (a NaN only where one can legitimately be, in the edge cases: alpha12, and ss1 under early rejection, which accepts a NaN proposal)
            check(name, scal[:, j], o["scal"][:, j], nan_ok=edge and (name == "alpha12" or (name == "ss1" and ckw["method"] == "er")))
    check("stream position", rng, o["rng"])
    for j, name in enumerate(("stayed", "bndstayed", "drtries", "draccepted", "erstayed")):
        check(name, ctr[:, j], o["ctr"][:, j])
    if "status" in o:
        check("status bits", status, o["status"])
    check("R", np.array([tri(a) for a in R]), np.array([tri(a) for a in o["R"]]))
    if qstd is not None:
        check("qcovstd", qstd, o["qstd"])
    if cov is not None:
        check("chaincmat", np.array([np.triu(k[0]) for k in cov]), np.array([np.triu(a) for a in o["cmat"]]))
        check("chainmean", np.array([k[1] for k in cov]), o["mean"])
        check("chainwsum", np.array([k[2] for k in cov]), o["wsum"])
    if rec is not None:                                         # one ss and one sigma2 per response column
        ny = o["ss1v"].shape[1]
        assert ny == 2 and len(rec) == nch
        check("ss of every column", np.array([k[1][-1, :ny] for k in rec]), o["ss1v"])
        check("sigma2 chain of every column", np.array([k[2] for k in rec]), o["s2chain"])
    if dr is not None:
        check("R2", np.array([tri(k[0]) for k in dr]), np.array([tri(a) for a in o["R2"]]))
        check("iC", np.array([np.triu(k[1]) for k in dr]), np.array([np.triu(a) for a in o["iC"]]))
    return failures
