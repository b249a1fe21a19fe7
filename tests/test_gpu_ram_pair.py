"""step_kernel_ram_wide's update-only waves store the factor once per two iterations (ram_update's SW_DEFER and ram_update_pair, DESIGN.md
section 5b): an iteration whose successor in the same launch adapts too sweeps the factor without storing it, and the successor applies both
rank-one updates in one pass; a successor with a downdate lane first flushes the deferred update (SW_FLUSH) and then takes the mixed sweeps.

Every case runs the engine twice, with the pairing on (the default) and with MCMCX_RAM_PAIR=0 (every update sweep stores, the parent's
path), and the oracle on every lane; EVERY chain's state, scalars (ss1, prior, sigma2, alpha12), packed factor, stream position
(n, saved, saved_y), counters (stayed, bndstayed, chainind, curcount, status) and accept sequence, and the run's downdate total, must be
equal bit for bit (==, no tolerance) between the two runs and to the oracle.  (pdesc, the next proposal's dtrmv order, has no accessor: a
wrong one changes the first proposal of the next launch, which the cut runs below continue from.)

The padding lanes of a ragged last tile are chains of their own (ids beyond nchains, started at par0) and take part in the wave's
`any lane downdates` test, so the oracle runs all 64 lanes of every tile and `_rule` below derives, from the oracle's per-iteration alpha12
alone, how many wave-iterations the rule sends to each sweep."""
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import edge_problems as ep

pytestmark = pytest.mark.gpu

KERNEL = "step_kernel_ram_wide"
SWITCHES = ("MCMCX_GROUP", "MCMCX_GROUP_GW", "MCMCX_RAM_GROUP", "MCMCX_RAM_WIDE", "MCMCX_RAM_PAIR", "MCMCX_LDS_SCRATCH", "MCMCX_COLS_PHASED")
ALPHATARGET = 0.234                              # the namelist default (mcmcinit.F90), which no case changes


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _gauss(d, start, seed=None):
    """The Gaussian target of tests/test_gpu_ram_every_chain.py.  start 'default': cmat0 = 0.01 I at the mode, bench.py's default start (high
    acceptance: updates); 'target': cmat0 = the target's covariance (RAM at its target rate from the start: most iterations downdate)."""
    r = np.random.default_rng(3000 + d if seed is None else seed)
    A = r.standard_normal((d, d)) / np.sqrt(d)
    lam = A @ A.T + np.eye(d)
    mu = np.linspace(-0.5, 0.5, d)
    if start == "default":
        return dict(kind="gauss", npar=d, par0=mu.copy(), cmat0=0.01 * np.eye(d), mu=mu, lam=lam)
    return dict(kind="gauss", npar=d, par0=np.full(d, 0.1), cmat0=np.linalg.inv(lam), mu=mu, lam=lam)


_ORACLE = {}


def _oracle_all(oracle, key, ckw, pkw, nch, chain_id0):
    """All lanes of all tiles (nch rounded up to 64) through the oracle, once per problem, never changed."""
    if key not in _ORACLE:
        d, nsimu, nl = pkw["npar"], ckw["nsimu"], (nch + 63) // 64 * 64
        cfg = oracle.make_cfg(**ckw); prob = oracle.Problem(**pkw)
        assert cfg.alphatarget == ALPHATARGET
        oracle.lib()
        with ThreadPoolExecutor(min(16, os.cpu_count() or 1)) as pool:
            rs = list(pool.map(lambda c: oracle.run_chain(cfg, prob, chain_id=chain_id0 + c, continue_on_downdate_fail=True), range(nl)))
        o = dict(theta=np.array([r.theta for r in rs]), acc=np.array([r.accepted for r in rs], dtype=np.uint8), R=np.array([r.R for r in rs]),
                 rng=np.array([r.rng_n for r in rs], dtype=np.uint64), saved=np.array([r.rng_saved for r in rs], dtype=np.int64),
                 saved_y=np.array([r.rng_saved_y for r in rs]), stayed=np.array([r.stayed for r in rs], dtype=np.int64),
                 bndstayed=np.array([r.bndstayed for r in rs], dtype=np.int64), fail=np.array([r.ram_downdate_fail != 0 for r in rs]),
                 scal=np.array([(r.ss1, r.sspri1, r.sigma2, r.alpha12) for r in rs]), alpha=np.array([r.alpha for r in rs]),
                 chainind=np.array([r.chainind for r in rs], dtype=np.int64))
        assert all(r.simuind == nsimu for r in rs) and o["alpha"].shape == (nl, nsimu)
        for v in o.values():
            v.setflags(write=False)
        _ORACLE[key] = o
    return _ORACLE[key]


def _rule(alpha, ckw, cuts):
    """From the oracle's alpha12 of every lane [lanes][nsimu] (row it - 1 = iteration it; iteration 1 is the start point): the wave-iterations
    the rule of step_body sends to (pair, flush + mixed, plain, defer, mixed without a flush), summed over tiles and launches.  A lane
    downdates at an adapting iteration unless alpha12 >= alphatarget (a NaN downdates); the launches are those of run(cuts...): 2 .. cuts[0],
    cuts[0] + 1 .. cuts[1], ..."""
    nsimu, doadapt = ckw["nsimu"], ckw.get("doadapt", 1)
    burn = ckw.get("burnintime", 0) if ckw.get("doburnin", 0) else 0
    adapts = lambda it: doadapt != 0 and not it < burn
    n = dict(pair=0, flush=0, plain=0, defer=0, mixed=0)
    ends = [nsimu if c is None else c for c in cuts]
    for t in range(0, alpha.shape[0], 64):
        anyd = ~np.all(alpha[t:t + 64] >= ALPHATARGET, axis=0)
        it0 = 2
        for it1 in ends:
            pending = False
            for it in range(it0, it1 + 1):
                if not adapts(it):
                    assert not pending
                    continue
                if anyd[it - 1]:
                    n["flush" if pending else "mixed"] += 1
                    pending = False
                elif pending:
                    n["pair"] += 1
                    pending = False
                elif it + 1 <= it1 and adapts(it + 1):
                    n["defer"] += 1
                    pending = True
                else:
                    n["plain"] += 1
            assert not pending                          # no launch ends with an update pending
            it0 = it1 + 1
    return n


def _engine_state(monkeypatch, ckw, pkw, nch, chain_id0, cuts, pair):
    from mcmcf90_amd import engine_from_problem
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("MCMCX_GROUP", "0")
    monkeypatch.setenv("MCMCX_RAM_GROUP", "0")
    if not pair:
        monkeypatch.setenv("MCMCX_RAM_PAIR", "0")
    e = engine_from_problem(ckw, pkw, nchains=nch, chain_id0=chain_id0, record_accept=1)
    e.init()
    for upto in cuts:
        e.run(upto)
        assert e.last_kernel() == KERNEL, e.last_kernel()
    assert e.simuind == ckw["nsimu"]
    masks = e.accept_masks()
    c = np.arange(nch)
    rng = [e.rng(k) for k in range(nch)]
    ctr = [e.counters(k) for k in range(nch)]
    s = dict(theta=e.theta(), scal=e.scalars(), R=np.array([np.triu(e.R(k)) for k in range(nch)]),
             acc=((masks[:, c // 64] >> (c % 64).astype(np.uint64)) & np.uint64(1)).astype(np.uint8).T,
             rng=np.array([r[0] for r in rng], dtype=np.uint64), saved=np.array([r[1] for r in rng], dtype=np.int64),
             saved_y=np.array([r[2] for r in rng]), downdates=e.totals()["downdates"])
    for k in ("stayed", "bndstayed", "chainind", "curcount", "status"):
        s[k] = np.array([q[k] for q in ctr], dtype=np.int64)
    e.close()
    return s


def _chains(bad):
    bad = np.flatnonzero(bad)
    return "%d chains, the first: %s" % (len(bad), bad[:12])


def _same_runs(a, b, what):
    for k in ("theta", "scal", "R", "saved_y"):
        bad = np.any((_bits(a[k]) != _bits(b[k])).reshape(len(a[k]), -1), axis=1)
        assert not bad.any(), "%s, %s: %s" % (what, k, _chains(bad))
    for k in ("acc", "rng", "saved", "stayed", "bndstayed", "chainind", "curcount", "status"):
        bad = np.any((a[k] != b[k]).reshape(len(a[k]), -1), axis=1)
        assert not bad.any(), "%s, %s: %s" % (what, k, _chains(bad))
    assert a["downdates"] == b["downdates"], what


def _same_as_oracle(s, o, nch, nan_alpha=False):
    what = "against the oracle"
    for k in ("theta", "R", "saved_y"):
        ov = np.array([np.triu(R) for R in o["R"][:nch]]) if k == "R" else o[k][:nch]
        bad = np.any((_bits(s[k]) != _bits(ov)).reshape(nch, -1), axis=1)
        if k == "saved_y":
            bad &= s["saved"] != 0                              # (the second deviate of a polar pair, where one is kept)
        assert not bad.any(), "%s, %s: %s" % (what, k, _chains(bad))
    for j, name in enumerate(("ss1", "prior", "sigma2", "alpha12")):
        # (a NaN equals a NaN whatever its sign and payload: x86 and gfx950 generate different default NaNs)
        bad = ~ep.same_bits_or_nan(s["scal"][:, j], o["scal"][:nch, j]) if nan_alpha else _bits(s["scal"][:, j]) != _bits(o["scal"][:nch, j])
        assert not bad.any(), "%s, %s: %s" % (what, name, _chains(bad))
    for k in ("acc", "rng", "saved", "stayed", "bndstayed", "chainind"):
        bad = np.any((s[k] != o[k][:nch]).reshape(nch, -1), axis=1)
        assert not bad.any(), "%s, %s: %s" % (what, k, _chains(bad))
    bad = (s["status"] & 1).astype(bool) != o["fail"][:nch]
    assert not bad.any(), "%s, failed-downdate flag: %s" % (what, _chains(bad))


def _check(oracle, monkeypatch, key, ckw, pkw, nch, cuts=(None,), chain_id0=0, cuts_off=None, want=None, nan_alpha=False):
    o = _oracle_all(oracle, key, ckw, pkw, nch, chain_id0)
    n = _rule(o["alpha"], ckw, cuts)
    print(key, "rule, wave-iterations:", n)
    if want:
        ok = want(n, o)                                         # the regime, from the oracle alone, before the engine is touched
        assert ok is None or ok, n
    on = _engine_state(monkeypatch, ckw, pkw, nch, chain_id0, cuts, True)
    off = _engine_state(monkeypatch, ckw, pkw, nch, chain_id0, cuts if cuts_off is None else cuts_off, False)
    _same_runs(on, off, "MCMCX_RAM_PAIR on / 0")
    _same_as_oracle(on, o, nch, nan_alpha)
    return on, n


# ---- 1. panel geometry: ram_update_pair's equal panels of at most ten columns (RW_PAIR) -- 3 x 7, 3 x 9, 4 x 10, 5 x 10 -- beside the 17-wide
# ones of the deferring sweep (2 x 11, 2 x 14, 3 x 14, 3 x 17); three tiles, the last one ragged at 2 lanes; the launch's last
# iteration once the second of a pair (nsimu 41: iterations 2 .. 41) and once unpaired (42)
@pytest.mark.parametrize("nsimu", (41, 42))
@pytest.mark.parametrize("d", (21, 27, 40, 50))
def test_panel_geometry(oracle, monkeypatch, d, nsimu):
    ckw = dict(nsimu=nsimu, method="ram", adaptint=100, updatesigma=0)

    def want(n, o):                                             # default start: updates only -- every iteration pairs, but an odd one out
        assert n["mixed"] == n["flush"] == 0 and n["pair"] == n["defer"] == 3 * ((nsimu - 1) // 2) and n["plain"] == 3 * ((nsimu - 1) % 2), n

    _check(oracle, monkeypatch, ("geom", d, nsimu), ckw, _gauss(d, "default"), 130, want=want)


# ---- 2. launch cuts on both parities, one launch of a single iteration: the state cannot depend on where the launches end
def test_launch_cuts(oracle, monkeypatch):
    ckw = dict(nsimu=40, method="ram", adaptint=100, updatesigma=0)
    pkw = _gauss(27, "default")
    whole, n = _check(oracle, monkeypatch, ("cuts", 27, 40), ckw, pkw, 64, cuts=(40,), want=lambda n, o: n["pair"] >= 19)
    cut = _engine_state(monkeypatch, ckw, pkw, 64, 0, (7, 8, 21, 40), True)
    _same_runs(whole, cut, "run(40) / run(7); run(8); run(21); run(40)")
    m = _rule(_ORACLE[("cuts", 27, 40)]["alpha"], ckw, (7, 8, 21, 40))
    assert (m["pair"], m["plain"]) == (18, 3), m                    # (launches 2..7, 8..8, 9..21, 22..40: 8..8 and two odd ones end unpaired)


# ---- 3. a pending update meets a downdate: defer -> flush -> mixed happens, and so does defer -> pair
def test_pending_meets_a_downdate(oracle, monkeypatch):
    """npar 21, three chains on one ragged tile -- whose 61 padding lanes are chains too and vote in `any lane downdates`, so with cmat0 = the
    target's covariance (about half of the LANES downdate at every iteration) no wave would ever pair, whatever the seed or the chain count.
    The regime in which a wave's vote is often false and often true is the one the headline run passes through: bench.py's default start,
    where the acceptance rate comes down to the target and the first lanes begin to downdate.  300 iterations of it; the oracle's alpha12
    of the tile's 64 lanes sends 111 wave-iterations to pair, 20 to flush + mixed and 22 to plain (COUNTS_3; launches of eleven iterations,
    CUTS_3: an update-only iteration is plain only where its launch ends), each required >= 10 before the engine is touched.  (The literal cmat0 = covariance case is test_target_regime_never_pairs.)"""
    ckw = dict(nsimu=300, method="ram", adaptint=100, updatesigma=0)

    def want(n, o):
        assert (n["pair"], n["flush"], n["plain"]) == COUNTS_3, n
        assert min(n["pair"], n["flush"], n["plain"]) >= 10, n

    _check(oracle, monkeypatch, ("pend", 21, 300), ckw, _gauss(21, "default"), 3, cuts=CUTS_3, want=want)


COUNTS_3, CUTS_3 = (111, 20, 22), tuple(range(12, 300, 11)) + (None,)


def test_target_regime_never_pairs(oracle, monkeypatch):
    """cmat0 = the target's covariance (bench.py --start target, the c4t fixtures), npar 21, three chains, 200 iterations: some lane of the 64
    downdates at every iteration but a few, so the rule takes the mixed sweeps throughout -- the run must be the parent's all the same."""
    ckw = dict(nsimu=200, method="ram", adaptint=100, updatesigma=0)
    _check(oracle, monkeypatch, ("target", 21, 200), ckw, _gauss(21, "target"), 3, want=lambda n, o: n["mixed"] >= 150)


# ---- 4. adaptation windows: the rule refuses to defer across the boundary
def test_burnin_ends_inside_the_launch(oracle, monkeypatch):
    ckw = dict(nsimu=60, method="ram", adaptint=100, updatesigma=0, doburnin=1, burnintime=21)

    def want(n, o):                                             # iterations 21 .. 60 adapt: twenty pairs, nothing before them
        assert n["pair"] == n["defer"] == 20 and n["plain"] == n["mixed"] == n["flush"] == 0, n

    _check(oracle, monkeypatch, ("burn", 27, 60), ckw, _gauss(27, "default"), 64, want=want)
    ckw = dict(ckw, nsimu=61)                                   # ... and forty-one: the last one unpaired
    _check(oracle, monkeypatch, ("burn", 27, 61), ckw, _gauss(27, "default"), 64, want=lambda n, o: (n["pair"], n["plain"]) == (20, 1))


def test_no_adaptation(oracle, monkeypatch):
    ckw = dict(nsimu=40, method="ram", adaptint=100, updatesigma=0, doadapt=0)
    _check(oracle, monkeypatch, ("noadapt", 27, 40), ckw, _gauss(27, "default"), 64, want=lambda n, o: not any(n.values()))


def test_failed_downdate(oracle, monkeypatch):
    """tests/test_gpu_ram_every_chain.py's `ovf:60:0.15` problem at npar 50 (sums of squares that overflow: a NaN alpha downdates, and its
    norm test fails): chains flagged ST_RAM_DOWNDATE_FAIL, their factor untouched, beside update-only stretches of the wave."""
    ckw = dict(nsimu=80, method="ram", adaptint=100, updatesigma=0)

    def want(n, o):
        assert o["fail"][:70].sum() >= 10 and n["mixed"] + n["flush"] >= 10, (o["fail"].sum(), n)

    _check(oracle, monkeypatch, ("ovf", 50, 80), ckw, ep.overflow(50, 60.0, 0.15), 70, cuts=(33, None), chain_id0=6, want=want, nan_alpha=True)


# ---- 5. bounds, a prior and the sigma2 update: have_p, stale alpha12 and the order of the draws
def test_bounds_prior_and_sigma2(oracle, monkeypatch):
    d = 27
    pkw = _gauss(d, "default")
    pkw.update(lo=pkw["mu"] - 0.4, hi=pkw["mu"] + 0.4, pri_mu=pkw["mu"] + 0.05, pri_sig=np.full(d, 2.0), sigma2=1.0, nobs=15)
    ckw = dict(nsimu=120, method="ram", adaptint=100, updatesigma=1, N0=50.0, S02=1.0)

    def want(n, o):                                             # (the oracle: 8477 proposals outside the box, 118 pairs)
        assert o["bndstayed"][:66].sum() > 66 and n["pair"] >= 100, (o["bndstayed"].sum(), n)

    _check(oracle, monkeypatch, ("bnd", d, 120), ckw, pkw, 66, cuts=(61, None), want=want)
