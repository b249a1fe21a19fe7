"""Per-chain start points (mcmcx_set_par0_all, mcmcx_set_par0_spread, mcmcx_start_info): chain c is the reference's single chain started at
its own start.  583 chains from chain_id0 = 6 (nine full tiles and a ragged one, tests/test_gpu_every_chain.py's layout); the oracle runs
every chain with a Problem whose par0 is that chain's start, and state, accept sequence, scalars, stream position, counters, factor and
chaincmat / chainmean / chainwsum must be the oracle's bit for bit.  The regime of every case is asserted from the oracle (or from
tests/start_ref.py) alone before the engine runs.

Case 1 (lane AM, initcmatn = 7: the first AM tick is a Welford update from chainmean) and case 2 (group kernel, burn-in with the greedy
restart) fail in the covariance's bits when adapt_pre_kernel restarts chainmean from the shared par0 instead of the chain's start; all of
the cases fail without the entry points."""
import ctypes as C
import math
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import start_ref as sr
import test_gpu_every_chain as ec

pytestmark = pytest.mark.gpu

NCH, CHAIN_ID0 = ec.NCH, ec.CHAIN_ID0
TILES = [slice(t, t + 64) for t in range(0, NCH - 63, 64)]


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _given(pkw, nch, seed=77):
    """par0 + 0.5 * (numpy normal): every chain its own start."""
    d = int(pkw["npar"])
    z = np.random.default_rng(seed).standard_normal((nch, d))
    if pkw.get("lo") is not None and pkw["kind"] == "expdata":
        # the response-column target evaluates its first point through the phase-cut path, which consults the box there as it does for
        # an out-of-box par0 today (no ss for a point outside): keep these starts inside lo = 0, par0 * exp(0.3 z)
        return np.asarray(pkw["par0"], dtype=np.float64) * np.exp(0.3 * z)
    return np.asarray(pkw["par0"], dtype=np.float64) + 0.5 * z


_ORACLE = {}


def _oracle_from(oracle, key, ckw, pkw, starts, chain_id0=CHAIN_ID0, fast=False):
    """Every chain through the oracle from its own start (a Problem of its own whose par0 is the start): once per case, never changed."""
    if key not in _ORACLE:
        nch, d, nsimu = len(starts), int(pkw["npar"]), ckw["nsimu"]
        cfg = oracle.make_cfg(**ckw)
        probs = [oracle.Problem(**dict(pkw, par0=starts[c])) for c in range(nch)]
        oracle.lib()
        ram = ckw.get("method") == "ram"
        with ThreadPoolExecutor(8) as pool:
            rs = list(pool.map(lambda c: oracle.run_chain(cfg, probs[c], chain_id=chain_id0 + c, scam_fast=fast, continue_on_downdate_fail=ram), range(nch)))
        assert all(r.simuind == nsimu and r.rc == 0 for r in rs)
        o = dict(theta=np.array([r.theta for r in rs]), acc=np.array([r.accepted for r in rs], dtype=np.uint8),
                 scal=np.array([[r.ss1, r.sspri1, r.sigma2, r.alpha12] for r in rs]), rng=np.array([r.rng_n for r in rs], dtype=np.uint64),
                 ctr=np.array([[r.stayed, r.bndstayed, r.drtries, r.draccepted, r.erstayed] for r in rs], dtype=np.int64),
                 R=np.array([r.R for r in rs]), qstd=np.array([r.qcovstd for r in rs]), R2=np.array([r.R2 for r in rs]), iC=np.array([r.iC for r in rs]),
                 cmat=np.array([r.chaincmat for r in rs]), mean=np.array([r.chainmean for r in rs]), wsum=np.array([r.chainwsum for r in rs]),
                 alpha=np.array([r.alpha for r in rs]), ss1v=np.array([r.ss1v for r in rs]), s2chain=np.array([r.s2chain for r in rs]).reshape(nch, nsimu, -1),
                 fail=np.array([r.ram_downdate_fail != 0 for r in rs]))
        assert o["theta"].shape == (nch, d) and o["acc"].shape == (nch, nsimu)
        for v in o.values():
            v.setflags(write=False)
        _ORACLE[key] = o
    return _ORACLE[key]


def _set_env(monkeypatch, env):
    for k in ec.SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def _compare(e, o, ckw, nch, cols=False):
    """Everything the engine shows of every chain against the oracle's dictionary, bit for bit (tests/test_gpu_every_chain.py's list)."""
    nsimu = ckw["nsimu"]
    assert e.simuind == nsimu
    theta, masks, scal = e.theta(), e.accept_masks(), e.scalars()
    rng = np.array([e.rng(c)[0] for c in range(nch)], dtype=np.uint64)
    cn = [e.counters(c) for c in range(nch)]
    ctr = np.array([[k[n] for n in ("stayed", "bndstayed", "drtries", "draccepted", "erstayed")] for k in cn], dtype=np.int64)
    R = np.array([e.R(c) for c in range(nch)])
    ram = ckw.get("method") == "ram"
    scam = ckw.get("method") == "scam"
    cov = None if ram else [e.chaincov(c) for c in range(nch)]
    qstd = np.array([e.qcovstd(c) for c in range(nch)]) if scam else None
    dr = [e.dr_state(c) for c in range(nch)] if ckw.get("drscale") else None
    rec = [e.chain(c) for c in range(nch)] if cols else None
    c = np.arange(nch)
    acc = ((masks[:, c // 64] >> (c % 64).astype(np.uint64)) & np.uint64(1)).astype(np.uint8).T
    assert acc.shape == o["acc"].shape and theta.shape == o["theta"].shape and R.shape == o["R"].shape
    full = scam or ckw.get("condmax", 0.0) > 0.0
    tri = (lambda a: a) if full else (lambda a: np.triu(a))
    failures = []

    def check(name, got, want):
        got, want = np.asarray(got), np.asarray(want)
        assert got.shape == want.shape, (name, got.shape, want.shape)
        eq = (_bits(got) == _bits(want)) if got.dtype.kind == "f" else (got == want)
        bad = np.flatnonzero(~eq.reshape(nch, -1).all(axis=1))
        if len(bad):
            failures.append("%s: %d chains, the first: %s" % (name, len(bad), bad[:12]))

    check("accept sequence", acc, o["acc"])
    check("theta", theta, o["theta"])
    for j, name in enumerate(("ss1", "sspri1", "sigma2", "alpha12")):
        if name != "alpha12" or ckw.get("method") not in ("er",):
            check(name, scal[:, j], o["scal"][:, j])
    check("stream position", rng, o["rng"])
    for j, name in enumerate(("stayed", "bndstayed", "drtries", "draccepted", "erstayed")):
        check(name, ctr[:, j], o["ctr"][:, j])
    check("R", np.array([tri(a) for a in R]), np.array([tri(a) for a in o["R"]]))
    if ram:
        check("downdate status", np.array([(k["status"] & 1) != 0 for k in cn]), o["fail"])
    if qstd is not None:
        check("qcovstd", qstd, o["qstd"])
    if cov is not None:
        check("chaincmat", np.array([np.triu(k[0]) for k in cov]), np.array([np.triu(a) for a in o["cmat"]]))
        check("chainmean", np.array([k[1] for k in cov]), o["mean"])
        check("chainwsum", np.array([k[2] for k in cov]), o["wsum"])
    if rec is not None:
        ny = o["ss1v"].shape[1]
        check("ss of every column", np.array([k[1][-1, :ny] for k in rec]), o["ss1v"])
        check("sigma2 chain of every column", np.array([k[2] for k in rec]), o["s2chain"])
    if dr is not None:
        check("R2", np.array([tri(k[0]) for k in dr]), np.array([tri(a) for a in o["R2"]]))
        check("iC", np.array([np.triu(k[1]) for k in dr]), np.array([np.triu(a) for a in o["iC"]]))
    assert not failures, "; ".join(failures)


def _run_given(oracle, monkeypatch, prob, kernel, env, samples=False, regime=None):
    """A problem of tests/test_gpu_every_chain.py with given starts: the oracle from each start, the regime, then the engine."""
    from mcmcf90_amd import engine_from_problem
    ckw, pkw, nch, cuts = ec._problem(prob)
    starts = _given(pkw, nch)
    o = _oracle_from(oracle, ("given", prob), ckw, pkw, starts, fast=bool(ec._fast(prob)))
    assert len(np.unique(starts[:, 0])) == nch
    (regime or ec._regime)(prob, o)                             # ... before the engine is touched
    _set_env(monkeypatch, env)
    cols = prob[0] == "cols"
    e = engine_from_problem(ckw, pkw, nchains=nch, chain_id0=CHAIN_ID0, record_accept=1, record_chain=1 if cols else 0, scam_fast=ec._fast(prob))
    e.setpar0_all(starts)
    if samples:
        e.set_samples(first=1, thin=1)
    e.init()
    assert (_bits(e.theta()) == _bits(starts)).all()            # mcmcx_get_theta right after init returns the starts
    assert e.start_info() == dict(mode="given", redrew=0, fell_back=0)
    for upto in cuts:
        e.run(upto)
        assert e.last_kernel() == kernel, e.last_kernel()
    if samples:                                                 # first = 1: sample 0 of the store is the start point
        its, a = e.samples(0, 1)
        assert list(its) == [1] and (_bits(a[0][:, :int(pkw["npar"])]) == _bits(starts)).all()
    try:
        _compare(e, o, ckw, nch, cols=cols)
    finally:
        e.close()


# ---------------------------------------------------------------- 1. given starts, lane AM, the first tick a Welford update from chainmean
def test_given_starts_lane_am_first_tick_from_chainmean(oracle, monkeypatch):
    prob = ec.P("gauss", 20, initcmatn=7)
    assert ec._problem(prob)[0]["initcmatn"] == 7 and ec._problem(prob)[0]["adaptint"] == 50 and ec._problem(prob)[0]["nsimu"] == 170
    _run_given(oracle, monkeypatch, prob, ec.AM, dict(ec.LANE, MCMCX_LDS_SCRATCH="0"), samples=True)


# ---------------------------------------------------------------- 2. given starts, group kernel with burn-in: the greedy restart
def _regime_greedy(prob, o):
    ec._regime(prob, o)                                         # every branch taken by a twentieth of the chains at every tick
    B = ec.BURN
    took = np.zeros(NCH, dtype=bool)
    for t in ec.BURN_TICKS:
        staypc = (o["acc"][:, 1:t] == 0).sum(axis=1) / float(t)
        took |= ~(staypc > 1.0 - B["scalelimit"]) & ~(staypc < B["scalelimit"])
    assert all(took[t].any() for t in TILES), [int(took[t].sum()) for t in TILES]      # the greedy branch, in every full tile


def test_given_starts_group_burnin_greedy_restart(oracle, monkeypatch):
    prob = ec.P("gauss", 12, burnin=1, initcmatn=7)
    _run_given(oracle, monkeypatch, prob, "group_step_kernel", ec.GRP, regime=_regime_greedy)


# ---------------------------------------------------------------- 3. spread with bounds, method = 'ram'
def _spread_problem(d, method="ram", nsimu=170):
    pkw = ec._problem(ec.P("gauss", d))[1]
    sd = np.sqrt(np.diag(pkw["cmat0"]))
    pkw = dict(pkw, lo=pkw["par0"] - 1.5 * sd, hi=pkw["par0"] + 1.5 * sd)
    return dict(nsimu=nsimu, method=method, adaptint=100, updatesigma=0), pkw


def _engine(ckw, pkw, nch, chain_id0=CHAIN_ID0, **extra):
    from mcmcf90_amd import engine_from_problem
    return engine_from_problem(ckw, pkw, nchains=nch, chain_id0=chain_id0, record_accept=1, **extra)


def test_spread_with_bounds_ram(oracle, monkeypatch):
    d = 7
    scale = math.sqrt(7.0) / 2.4
    ckw, pkw = _spread_problem(d)
    starts, tries, fell = sr.starts(oracle, NCH, pkw["par0"], pkw["cmat0"], scale, pkw["lo"], pkw["hi"], chain_id0=CHAIN_ID0)
    # the regime, from the restatement alone: every full tile holds a chain that redrew and one that did not, no chain fell back
    assert all((tries[t] > 1).any() and (tries[t] == 1).any() for t in TILES) and not fell.any()
    assert all(sr.inbounds(s, pkw["lo"], pkw["hi"]) for s in starts)
    o = _oracle_from(oracle, "spread_ram7", ckw, pkw, starts)
    rate = o["acc"][:, 1:].mean()
    assert 0.1 < rate < 0.5 and o["ctr"][:, 1].sum() > NCH, (rate, o["ctr"][:, 1].sum())      # near the target rate; the bounds bite
    _set_env(monkeypatch, {})
    e = _engine(ckw, pkw, NCH)
    e.setpar0_spread(scale)
    e.init()
    try:
        got = e.theta()
        bad = np.flatnonzero((_bits(got) != _bits(starts)).any(axis=1))
        assert not len(bad), (len(bad), bad[:12])
        assert e.start_info() == dict(mode="spread", redrew=sr.info(tries, fell)[0], fell_back=0)
        assert all(e.rng(c) == (0, 0, 0.0) for c in (0, 63, 64, NCH - 1))          # the sampling stream is not advanced
        for upto in (60, 61, None):
            e.run(upto)
        assert "ram" in e.last_kernel()
        _compare(e, o, ckw, NCH)
    finally:
        e.close()
    # a box nothing can meet: every chain falls back to par0's bits
    par0 = np.array(pkw["par0"]); par0[2] = -0.0
    lo, hi = np.array(pkw["lo"]), np.array(pkw["hi"])
    lo[1], hi[1] = 1.0, -1.0
    e = _engine(ckw, dict(pkw, par0=par0, lo=lo, hi=hi), 70)
    e.setpar0_spread(scale)
    e.init()
    try:
        assert (_bits(e.theta()) == _bits(np.tile(par0, (70, 1)))).all()
        assert e.start_info() == dict(mode="spread", redrew=70, fell_back=70)
    finally:
        e.close()


# ---------------------------------------------------------------- 4. pooled AM, spread
class _OwnStarts:
    """The oracle module with LiveChain handing chain c a Problem of its own whose par0 is the chain's start: what
    tests/test_gpu_pooled.py's _restate_pooled builds its chains through.  Everything else -- the moments' shift, the pooled state's
    initial mean -- keeps the shared par0 of the pkw the restatement is given."""

    def __init__(self, oracle, pkw, starts):
        self._o, self._probs = oracle, [oracle.Problem(**dict(pkw, par0=s)) for s in starts]

    def __getattr__(self, name):
        return getattr(self._o, name)

    def LiveChain(self, cfg, prob, chain_id=0, **kw):
        return self._o.LiveChain(cfg, self._probs[chain_id], chain_id=chain_id, **kw)


def test_pooled_am_spread(oracle, monkeypatch):
    import test_gpu_pooled as tp
    d, N, nsimu = 8, 130, 220
    scale = math.sqrt(8.0) / 2.4
    S = 0.5 ** np.abs(np.subtract.outer(np.arange(d), np.arange(d)))
    pkw = dict(kind="gauss", npar=d, par0=np.full(d, 0.3), cmat0=0.05 * np.eye(d), mu=np.linspace(-1, 1, d), lam=np.linalg.inv(S))
    ckw = dict(nsimu=nsimu, adaptint=50, updatesigma=0)
    starts, tries, fell = sr.starts(oracle, N, pkw["par0"], pkw["cmat0"], scale)
    assert (tries == 1).all() and len(np.unique(starts[:, 0])) == N
    chains, st, log = tp._restate_pooled(_OwnStarts(oracle, pkw, starts), ckw, pkw, N)
    assert [k for _, k in log] == ["am"] * 4, log
    _set_env(monkeypatch, {})
    e = _engine(ckw, pkw, N, chain_id0=0, pooled=1)
    e.setpar0_spread(scale)
    e.init()
    try:
        assert (_bits(e.theta()) == _bits(starts)).all() and e.start_info() == dict(mode="spread", redrew=0, fell_back=0)
        e.run(50); e.run()
        theta = np.array([ch.theta for ch in chains])
        np.testing.assert_array_equal(_bits(e.theta()), _bits(theta), err_msg=str(log))
        for c in range(N):
            np.testing.assert_array_equal(e.accepted(c), chains[c].accepted)
        cm, mean, W, R = e.pooled()
        assert W == st["W"]
        np.testing.assert_array_equal(_bits(np.triu(R)), _bits(np.triu(st["R"])))
        np.testing.assert_array_equal(_bits(mean), _bits(np.array(st["mean"])))
        assert e.totals()["stayed"] == sum(ch.stayed for ch in chains)
    finally:
        for ch in chains:
            ch.close()
        e.close()


# ---------------------------------------------------------------- 5. host callbacks, given starts
def test_host_callbacks_first_evaluation_at_each_chains_start(oracle, monkeypatch):
    from mcmcf90_amd import Engine, make_config
    d, N = 3, 70
    ckw, pkw, _, _ = ec._problem(ec.P("gauss", d))
    ckw = dict(ckw, nsimu=120)
    starts = _given(pkw, N)
    o = _oracle_from(oracle, "host3", ckw, pkw, starts)
    rate = o["acc"][:, 1:].mean()
    assert 0.1 < rate < 0.6, rate
    prob = oracle.Problem(**pkw)
    L = oracle.lib()
    tgt = prob.ctarget()
    L.mcxo_ssfun.restype = C.c_double; L.mcxo_priorfun.restype = C.c_double
    dp = C.POINTER(C.c_double)
    seen = []

    def ssfun(th):
        if len(seen) < N:
            seen.append(np.array(th, dtype=np.float64).copy())
        return L.mcxo_ssfun(C.byref(tgt), th.ctypes.data_as(dp))

    def priorfun(th):
        return L.mcxo_priorfun(C.byref(tgt), th.ctypes.data_as(dp))

    _set_env(monkeypatch, {})
    e = Engine(make_config(d, N, record_accept=1, chain_id0=CHAIN_ID0, **ckw))
    e.setpar0(pkw["par0"]); e.setcmat0(np.asarray(pkw["cmat0"], dtype=float).reshape(d, d)); e.setsigma2nobs(1.0, 1)
    e.set_target_host(ssfun, priorfun, None)
    e.setpar0_all(starts)
    e.init()
    try:
        assert len(seen) == N and (_bits(np.array(seen)) == _bits(starts)).all()       # the first evaluation, chain by chain, at the chain's start
        e.run(50); e.run(51); e.run()
        _compare(e, o, ckw, N)
    finally:
        e.close()


# ---------------------------------------------------------------- 6. sharding, refusals, the default path
def test_spread_does_not_depend_on_the_sharding(oracle, monkeypatch):
    d = 7
    ckw, pkw = _spread_problem(d, nsimu=20)
    _set_env(monkeypatch, {})
    got = []
    for nch, id0 in ((192, 0), (96, 0), (96, 96)):
        e = _engine(ckw, pkw, nch, chain_id0=id0)
        e.setpar0_all(np.tile(pkw["par0"], (nch, 1)))           # the later call wins
        e.setpar0_spread(1.3)
        e.init()
        got.append((e.theta(), e.start_info()))
        e.close()
    assert (_bits(got[0][0]) == _bits(np.vstack([got[1][0], got[2][0]]))).all()
    assert got[0][1]["redrew"] == got[1][1]["redrew"] + got[2][1]["redrew"] > 0 and got[0][1]["mode"] == "spread"
    want, tries, fell = sr.starts(oracle, 192, pkw["par0"], pkw["cmat0"], 1.3, pkw["lo"], pkw["hi"])
    assert (_bits(got[0][0]) == _bits(want)).all() and got[0][1]["redrew"] == sr.info(tries, fell)[0]


def test_refusals_return_minus_56_and_leave_the_handle_usable(oracle, monkeypatch):
    from mcmcf90_amd import _lib
    L = _lib.load()
    d, N = 7, 70
    ckw, pkw = _spread_problem(d, method="dram", nsimu=30)
    _set_env(monkeypatch, {})
    dp = C.POINTER(C.c_double)
    good = np.ascontiguousarray(np.tile(pkw["par0"], (N, 1)))

    def refused(rc, word):
        msg = L.mcmcx_last_error().decode()
        assert rc == -56 and word in msg, (rc, msg, word)

    refused(L.mcmcx_set_par0_all(None, good.ctypes.data_as(dp), N, d), "null handle")
    refused(L.mcmcx_set_par0_spread(None, 1.0), "null handle")
    e = _engine(ckw, pkw, N)
    refused(L.mcmcx_set_par0_all(e.h, None, N, d), "null array")
    refused(L.mcmcx_set_par0_all(e.h, good.ctypes.data_as(dp), N - 1, d), "nchains")
    refused(L.mcmcx_set_par0_all(e.h, good.ctypes.data_as(dp), N, d + 1), "npar")
    for v in (np.nan, np.inf, -np.inf):
        bad = good.copy(); bad[N - 1, d - 1] = v
        refused(L.mcmcx_set_par0_all(e.h, bad.ctypes.data_as(dp), N, d), "not finite")
    for s in (0.0, -1.0, np.nan, np.inf):
        refused(L.mcmcx_set_par0_spread(e.h, s), "scale")
    # none of these changed the handle: it starts every chain at par0, and neither call is taken after init
    e.init()
    assert e.start_info() == dict(mode="shared", redrew=0, fell_back=0) and (_bits(e.theta()) == _bits(good)).all()
    refused(L.mcmcx_set_par0_all(e.h, good.ctypes.data_as(dp), N, d), "after mcmcx_init")
    refused(L.mcmcx_set_par0_spread(e.h, 1.0), "after mcmcx_init")
    e.run()
    assert e.simuind == 30 and e.start_info()["mode"] == "shared"
    e.close()
    # the external target: refused at the call, or at init when the target was chosen later
    for first in ("target", "spread", "given"):
        e = _engine(ckw, pkw, N, external=True) if first == "target" else _engine(ckw, pkw, N)
        if first == "target":
            refused(L.mcmcx_set_par0_spread(e.h, 1.0), "mcmcx_set_target_external")
            refused(L.mcmcx_set_par0_all(e.h, good.ctypes.data_as(dp), N, d), "mcmcx_set_target_external")
            e.init()                                            # usable as before
            assert e.start_info()["mode"] == "shared"
        else:
            e.setpar0_spread(1.0) if first == "spread" else e.setpar0_all(good)
            e.set_target_external()
            refused(L.mcmcx_init(e.h), "mcmcx_set_target_external")
        e.close()
    # spread needs cmat0's Cholesky factor, whatever factor the proposals use
    cm = np.array(pkw["cmat0"]); cm[3, :] = 0.0; cm[:, 3] = 0.0
    for condmax in (0.0, 1e8):
        e = _engine(dict(ckw, condmax=condmax), dict(pkw, cmat0=cm), N)
        e.setpar0_spread(1.0)
        refused(L.mcmcx_init(e.h), "could not factor")
        e.close()


def test_a_run_with_neither_call_is_the_run_without_them(oracle, monkeypatch):
    """An engine that never touched the new entry points against the oracle with the shared par0: theta, the stream position, the factor
    (and the rest of _compare's list)."""
    prob = ec.P("gauss", 20, initcmatn=7, nch=135)
    ckw, pkw, nch, cuts = ec._problem(prob)
    o = ec._oracle_all(oracle, prob)
    ec._regime(prob, o)
    _set_env(monkeypatch, dict(ec.LANE, MCMCX_LDS_SCRATCH="0"))
    e = _engine(ckw, pkw, nch)
    e.init()
    try:
        assert e.start_info() == dict(mode="shared", redrew=0, fell_back=0)
        for upto in cuts:
            e.run(upto)
        _compare(e, dict(o, fail=np.zeros(nch, dtype=bool)), ckw, nch)
    finally:
        e.close()


# ---------------------------------------------------------------- extended: the other kernel forms from given starts, spread at a wave's edge
def _ext_cases():
    G = lambda d, **o: ec.P("gauss", d, **o)
    return [
        pytest.param(G(13, drscale=3.0), "step_kernel_dr", dict(ec.LANE, MCMCX_DR_BIG="0"), id="lane_dr13"),
        pytest.param(G(13, drscale=3.0), "group_step_kernel<DR>", ec.GRP, id="group_dr13"),
        pytest.param(G(10), "group_step_kernel<quad>", ec.QUAD, id="quad10"),
        pytest.param(G(12, method="scam", nsimu=120), "scam_mw_kernel<8>", dict(MCMCX_SCAM_WAVES="8"), id="scam12"),
        pytest.param(ec.P("cols", 3), "step_kernel_cols", {}, id="cols3"),
        pytest.param(G(12, condmax=1e8), ec.LDSV, dict(MCMCX_SVD_LANE="1"), id="svd_lane12"),
    ]


@pytest.mark.extended
@pytest.mark.parametrize("prob,kernel,env", _ext_cases())
def test_given_starts_other_forms(oracle, monkeypatch, prob, kernel, env):
    _run_given(oracle, monkeypatch, prob, kernel, env)


@pytest.mark.extended
@pytest.mark.parametrize("d", [64, 65])
def test_spread_on_both_sides_of_64_rows(oracle, monkeypatch, d):
    ckw, pkw = _spread_problem(d, method="dram", nsimu=60)
    ckw = dict(ckw, adaptint=50)
    nch = 135
    pkw = dict(pkw, lo=None, hi=np.asarray(pkw["par0"]) + np.where(np.arange(d) == d - 1, 0.0, np.inf))    # the last row of U0 decides
    starts, tries, fell = sr.starts(oracle, nch, pkw["par0"], pkw["cmat0"], 1.0, None, pkw["hi"], chain_id0=CHAIN_ID0)
    assert (tries > 1).any() and (tries == 1).any() and not fell.any()
    o = _oracle_from(oracle, ("spread", d), ckw, pkw, starts)
    _set_env(monkeypatch, {})
    e = _engine(ckw, pkw, nch)
    e.setpar0_spread(1.0)
    e.init()
    try:
        assert (_bits(e.theta()) == _bits(starts)).all() and e.start_info()["redrew"] == sr.info(tries, fell)[0]
        e.run(50); e.run()
        _compare(e, o, ckw, nch)
    finally:
        e.close()


# ---------------------------------------------------------------- extended: the Fortran shim's restart cycle and its drawn starts
_NML = """&mcmc
 method = 'dram'
 nsimu       = %d
 doadapt     = 1
 adaptint    = 100
 updatesigma = 1
 N0          = 1
 S02         = 0
 printint    = 0
/
&mcmcx
 devtarget = 'expdata'
 datafile  = 'data.dat'
 lowerfile = 'lower.dat'
 nchains   = 128
 %s
/
"""


def _shim_run(d, nsimu, extra):
    import subprocess
    fdir = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "mcmcf90_amd", "fortran")
    exe = os.path.join(fdir, "demo_main")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-s", "-C", fdir])
    open(os.path.join(d, "mcmcinit.nml"), "w").write(_NML % (nsimu, extra))
    p = subprocess.run([exe], cwd=d, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
    assert p.returncode == 0, p.stdout.decode(errors="replace")
    return np.loadtxt(os.path.join(d, "mcmclaststates.dat"), ndmin=2)


def _shim_files(d):
    x = np.arange(11.0)
    y = 9.0 * np.exp(-0.12 * x) + 0.3 * np.random.default_rng(5).standard_normal(11)
    with open(os.path.join(d, "data.dat"), "w") as f:
        for a, b in zip(x, y):
            f.write("  %g   %.2f\n" % (a, b))
    open(os.path.join(d, "mcmcpar.dat"), "w").write("10 0.1 \n")
    open(os.path.join(d, "mcmccov.dat"), "w").write("0.2 0 \n0 0.001 \n")
    open(os.path.join(d, "mcmcsigma2.dat"), "w").write("0.5\n11\n")
    open(os.path.join(d, "lower.dat"), "w").write("0 0\n")


@pytest.mark.extended
def test_fortran_restart_cycle_over_all_chains(oracle):
    """A shim program with nchains = 128 runs twice: the second run has startfile = 'mcmclaststates.dat' and nsimu = 1, and writes back the
    states it was given.  With startscale the states of an nsimu = 1 run are the restatement's starts."""
    import tempfile
    with tempfile.TemporaryDirectory() as d:
        _shim_files(d)
        first = _shim_run(d, 300, "")
        assert first.shape == (128, 2) and len(np.unique(first[:, 0])) > 100
        again = _shim_run(d, 1, "startfile = 'mcmclaststates.dat'")
        assert (_bits(again) == _bits(first)).all()
        spread = _shim_run(d, 1, "startscale = 2.0")
    want, tries, fell = sr.starts(oracle, 128, [10.0, 0.1], np.array([[0.2, 0.0], [0.0, 0.001]]), 2.0, lo=np.zeros(2))
    assert (_bits(spread) == _bits(want)).all() and (tries > 1).any() and not fell.any()


# ---------------------------------------------------------------- extended: a user target module, given starts, against the oracle
# The banana target of oracle/mcx_targets.h (mcxt_ss_banana) written as a user's device functions: the same fma chain, so the oracle's
# banana chains are what the module's chains must be, bit for bit.  data[0] = b.
_MODULE_SRC = r"""
#include "mcmcx_target.h"
__device__ void start_ss(const double *th, int npar, int ny, const void *data, double *ss)
{
    const double b = ((const double *)data)[0];
    double t1 = th[0] * th[0];
    double q = __builtin_fma(b, t1, th[1]) - 100.0 * b;
    double s = __builtin_fma(q, q, t1 / 100.0);
    for (int k = 2; k < npar; ++k) s = __builtin_fma(th[k], th[k], s);
    ss[0] = s;
}
__device__ double start_prior(const double *th, int npar, const void *data) { return 0.0; }
__device__ int start_bounds(const double *th, int npar, const void *data) { return 1; }
MCMCX_DEFINE_TARGET(start_target, start_ss, start_prior, start_bounds)
"""


@pytest.mark.extended
def test_given_starts_user_target_module(oracle, monkeypatch, tmp_path):
    import subprocess
    from mcmcf90_amd import Engine, make_config
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    prob = ec.P("banana", 8)
    ckw, pkw, nch, cuts = ec._problem(prob)
    starts = _given(pkw, nch)
    o = _oracle_from(oracle, ("given", prob), ckw, pkw, starts)
    rate = o["acc"][:, 1:].mean()                               # from the oracle alone: the lanes of a wave accept at different iterations
    assert 0.1 < rate < 0.9, rate
    src, hsaco = tmp_path / "start_target.hip", tmp_path / "start_target.hsaco"
    src.write_text(_MODULE_SRC)
    subprocess.check_call(["/opt/rocm/bin/hipcc", "--genco", "--offload-arch=gfx950", "-O2", "-ffp-contract=off",
                           "-I" + os.path.join(root, "include"), str(src), "-o", str(hsaco)])
    _set_env(monkeypatch, {})
    d = int(pkw["npar"])
    e = Engine(make_config(d, nch, record_accept=1, chain_id0=CHAIN_ID0, **ckw))
    e.setpar0(pkw["par0"]); e.setcmat0(np.asarray(pkw["cmat0"], dtype=float).reshape(d, d)); e.setsigma2nobs(1.0, 1)
    e.set_target_module(str(hsaco), "start_target", np.array([float(pkw["b"])]))
    e.setpar0_all(starts)
    e.init()
    try:
        assert (_bits(e.theta()) == _bits(starts)).all() and e.start_info()["mode"] == "given"
        for upto in cuts:
            e.run(upto)
        _compare(e, o, ckw, nch)
    finally:
        e.close()


# ---------------------------------------------------------------- extended: why the feature exists
# A frozen proposal (doadapt = 0) a tenth as wide as the unit Gaussian target in each of four parameters, 130 chains, 120 iterations,
# all kept: chosen on the CPU with the oracle and tests/diag_ref.py.  From the shared par0 = 0 the oracle's split-R-hat of the four theta
# fields is 2.08, 2.02, 2.12, 1.88 (every chain wanders, none has mixed); from starts spread with scale = 25 (standard deviation 3 per
# parameter, three times the target's) it is 6.23, 6.01, 6.47, 6.76 -- 3.0 to 3.6 times the shared-start figure: R-hat with a shared
# start does not see the distance the chains still have to cover.
RHAT = dict(d=4, c0=0.01, nsimu=120, N=130, scale=25.0, maxlag=16)
_RHAT_ORACLE = {}


def _rhat_problem():
    d = RHAT["d"]
    return (dict(nsimu=RHAT["nsimu"], doadapt=0, updatesigma=0),
            dict(kind="gauss", npar=d, par0=np.zeros(d), cmat0=RHAT["c0"] * np.eye(d), mu=np.zeros(d), lam=np.eye(d)))


def _rhat_oracle(oracle, mode):
    """The oracle's chains as the sample store holds them, X[ns][nfields][nc] (theta, ss, sspri = +0.0, sigma2 = 1), and their starts."""
    if mode not in _RHAT_ORACLE:
        ckw, pkw = _rhat_problem()
        d, N, nsimu = RHAT["d"], RHAT["N"], RHAT["nsimu"]
        starts = np.tile(pkw["par0"], (N, 1)) if mode == "shared" else sr.starts(oracle, N, pkw["par0"], pkw["cmat0"], RHAT["scale"])[0]
        cfg = oracle.make_cfg(**ckw)
        probs = [oracle.Problem(**dict(pkw, par0=starts[c])) for c in range(N)]
        oracle.lib()
        with ThreadPoolExecutor(8) as pool:
            rs = list(pool.map(lambda c: oracle.run_chain(cfg, probs[c], chain_id=c), range(N)))
        rows = []
        for r in rs:
            cnt = r.chain[:, d].astype(int)
            th, ss = np.repeat(r.chain[:, :d], cnt, axis=0), np.repeat(r.sschain[:, 0], cnt)
            assert len(th) == nsimu
            rows.append(np.concatenate([th, ss[:, None], np.zeros((nsimu, 1)), np.ones((nsimu, 1))], axis=1))
        X = np.ascontiguousarray(np.array(rows).transpose(1, 2, 0))
        X.setflags(write=False)
        _RHAT_ORACLE[mode] = (X, starts)
    return _RHAT_ORACLE[mode]


@pytest.mark.extended
def test_dispersed_starts_are_what_split_rhat_needs(oracle, monkeypatch):
    import diag_ref
    from mcmcf90_amd.engine import samples_diag
    d, N, maxlag = RHAT["d"], RHAT["N"], RHAT["maxlag"]
    ckw, pkw = _rhat_problem()
    rhat = {}
    for mode in ("shared", "spread"):
        rhat[mode] = diag_ref.summary_ref(_rhat_oracle(oracle, mode)[0], maxlag)[:d, 2]
    print("oracle split-R-hat: shared", rhat["shared"], "spread", rhat["spread"])
    # the conditions, on the oracle alone, before the engine runs
    assert (rhat["spread"] > 1.5).all() and (rhat["spread"] >= 1.2 * rhat["shared"]).all(), rhat
    _set_env(monkeypatch, {})
    for mode in ("shared", "spread"):
        X, starts = _rhat_oracle(oracle, mode)
        e = _engine(ckw, pkw, N, chain_id0=0)
        if mode == "spread":
            e.setpar0_spread(RHAT["scale"])
        e.set_samples(first=1, thin=1)
        e.init(); e.run()
        try:
            _, got_x = e.samples(layout=1)
            assert (_bits(got_x) == _bits(X)).all(), mode          # the store holds the oracle's chains
            got, want = e.samples_stats(0, None, maxlag), diag_ref.stats_ref(X, maxlag)
            bad = np.flatnonzero(_bits(got) != _bits(want))
            assert bad.size == 0, (mode, bad[:8])                   # the reduced stats vector: bit for bit
            table, ref = samples_diag(got, X.shape[1], maxlag), diag_ref.finish_ref(want, X.shape[1], maxlag)
            nb = int(((_bits(table) != _bits(ref)) & ~(np.isnan(table) & np.isnan(ref))).sum())
            print(mode, "engine R-hat", table[:d, 2], "table entries whose bits differ from diag_ref's:", nb)
            assert np.array_equal(np.isnan(table), np.isnan(ref)) and (_bits(table)[~np.isnan(ref)] == _bits(ref)[~np.isnan(ref)]).all(), (mode, nb)
        finally:
            e.close()
