"""Many fits in one run (mcmcx_set_target_expdata_all, mcmcx_chain_data_info): chain c is the reference's single chain on chain c's own
data set.  130 chains from chain_id0 = 6 (two full tiles and a third with two lanes), ndata = 7 (one case at ndata = 1), nycol 1, 2 and 3,
260 iterations with adaptint = 50; the oracle runs every chain with a Problem whose xdata / ydata (and, in one case, par0) are that chain's,
and theta, ss and sigma2 per column, sspri, alpha12, the eight counters, the stream position, the factor (R2, iC, qcovstd where the method
has them) and chaincmat / chainmean / chainwsum of EVERY chain must be the oracle's bit for bit.  Sample 0 and the last sample of the store
are the oracle's rows.  The regime of every case -- the chains of a tile really differ, bounds bite, second stages and early rejections
happen -- is asserted from the oracle alone before the engine runs.

Every case fails without the entry points (Engine.set_target_all raises: the symbol is missing)."""
import ctypes as C
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

NCH, CHAIN_ID0, NSIMU, ADAPTINT = 130, 6, 260, 50
TICKS = tuple(range(ADAPTINT, NSIMU, ADAPTINT))
SWITCHES = ("MCMCX_COLS_PHASED", "MCMCX_GROUP", "MCMCX_SCAM_WAVES", "MCMCX_LDS_SCRATCH", "MCMCX_DR_BIG", "MCMCX_RAM_GROUP")
TILES = [slice(0, 64), slice(64, 128), slice(128, 130)]
RATES = np.array([0.1, 0.25, 0.4])


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _data(ny, ndata, nch=NCH, x_per_chain=True, seed=11):
    """Per-chain true parameters, a per-chain grid and seeded noise: x[nch][ndata] (or [ndata]), y[nch][ny][ndata], truth[nch][1 + ny]."""
    r = np.random.default_rng(seed + 100 * ny + ndata)
    amp = 9.0 + 0.8 * r.standard_normal(nch)
    rate = RATES[:ny] * np.exp(0.15 * r.standard_normal((nch, ny)))
    if x_per_chain:
        x = np.linspace(0.0, 1.0, ndata)[None, :] * (5.0 + 3.0 * r.random(nch))[:, None] if ndata > 1 else 1.0 + r.random((nch, 1))
    else:
        x = np.linspace(0.0, 6.0, ndata) if ndata > 1 else np.array([1.5])
    xx = x if x_per_chain else np.broadcast_to(x, (nch, ndata))
    y = amp[:, None, None] * np.exp(-rate[:, :, None] * xx[:, None, :]) + 0.3 * r.standard_normal((nch, ny, ndata))
    return np.ascontiguousarray(x), np.ascontiguousarray(y), np.column_stack([amp, rate])


def _problem(ny, ndata, **over):
    d = 1 + ny
    pkw = dict(kind="expdata", npar=d, par0=np.concatenate([[9.0], RATES[:ny]]), cmat0=np.diag([0.02] + [0.0002] * ny),
               sigma2=np.array([0.6, 0.9, 0.7])[:ny], nobs=np.array([ndata, ndata + 3, ndata + 1])[:ny])
    pkw.update(over)
    return pkw


_ORACLE = {}


def _oracle(oracle, key, ckw, pkw, x, y, starts=None):
    """Every chain through the oracle on its own data (and from its own start): once per case, never changed."""
    if key in _ORACLE:
        return _ORACLE[key]
    nch, ny, d = y.shape[0], y.shape[1], int(pkw["npar"])
    cfg = oracle.make_cfg(**ckw)
    L = oracle.lib()
    L.mcxo_priorfun.restype = C.c_double
    probs = []
    for c in range(nch):
        kw = dict(pkw, xdata=x[c] if x.ndim == 2 else x, ydata=y[c] if ny > 1 else y[c, 0])
        if starts is not None:
            kw["par0"] = starts[c]
        probs.append(oracle.Problem(**kw))
    ram = ckw.get("method") == "ram"
    with ThreadPoolExecutor(8) as pool:
        rs = list(pool.map(lambda c: oracle.run_chain(cfg, probs[c], chain_id=CHAIN_ID0 + c, continue_on_downdate_fail=ram, marks=TICKS),
                           range(nch)))
    assert all(r.simuind == ckw["nsimu"] and r.rc == 0 for r in rs)
    us = bool(ckw.get("updatesigma"))
    s20 = np.asarray(pkw["sigma2"], dtype=np.float64)
    first, last = [], []
    for c, r in enumerate(rs):
        p0 = probs[c].par0
        pri0 = L.mcxo_priorfun(C.byref(probs[c].ctarget()), p0.ctypes.data_as(C.POINTER(C.c_double)))
        s2_0 = np.asarray(r.s2chain).reshape(-1, ny)[0] if us else s20
        first.append(np.concatenate([p0, r.sschain[0, :ny], [pri0], s2_0]))
        last.append(np.concatenate([r.theta, r.ss1v, [r.sspri1], r.sigma2v if us else s20]))
    o = dict(theta=np.array([r.theta for r in rs]), ssv=np.array([r.ss1v for r in rs]), s2v=np.array([r.sigma2v if us else s20 for r in rs]),
             scal=np.array([[r.ss1, r.sspri1, r.sigma2, r.alpha12] for r in rs]), rng=np.array([r.rng_n for r in rs], dtype=np.uint64),
             ctr=np.array([[r.stayed, r.bndstayed, r.draccepted, r.drtries, r.chainind,
                            (1 if r.ram_downdate_fail else 0) | (2 if (r.chol_failed and not ram) else 0), r.erstayed, int(r.chain[-1, d])]
                           for r in rs], dtype=np.int64),
             R=np.array([r.R for r in rs]), R2=np.array([r.R2 for r in rs]), iC=np.array([r.iC for r in rs]),
             qstd=np.array([r.qcovstd for r in rs]), cmat=np.array([r.chaincmat for r in rs]), mean=np.array([r.chainmean for r in rs]),
             wsum=np.array([r.chainwsum for r in rs]), acc=np.array([r.accepted for r in rs], dtype=np.uint8),
             samples=np.array([first, last]))
    for v in o.values():
        v.setflags(write=False)
    # the chains really differ: no two chains of a tile end at the same theta
    for t in TILES:
        th = o["theta"][t]
        assert len({tuple(_bits(row)) for row in th}) == len(th)
    _ORACLE[key] = o
    return o


CTR = ("stayed", "bndstayed", "draccepted", "drtries", "chainind", "status", "erstayed", "curcount")


def _state(e, ckw, nch):
    """Everything the engine shows of every chain."""
    method = ckw.get("method", "dram")
    g = dict(theta=e.theta(), scal=e.scalars(), rng=np.array([e.rng(c)[0] for c in range(nch)], dtype=np.uint64),
             ctr=np.array([[e.counters(c)[n] for n in CTR] for c in range(nch)], dtype=np.int64), R=np.array([e.R(c) for c in range(nch)]),
             samples=e.samples()[1], kept=e.samples_kept())
    if method == "scam":
        g["qstd"] = np.array([e.qcovstd(c) for c in range(nch)])
    if method != "ram":
        cov = [e.chaincov(c) for c in range(nch)]
        g.update(cmat=np.array([np.triu(k[0]) for k in cov]), mean=np.array([k[1] for k in cov]), wsum=np.array([k[2] for k in cov]))
    if ckw.get("drscale"):
        dr = [e.dr_state(c) for c in range(nch)]
        g.update(R2=np.array([np.triu(k[0]) for k in dr]), iC=np.array([np.triu(k[1]) for k in dr]))
    return g


def _compare(g, o, ckw, nch, ny):
    method = ckw.get("method", "dram")
    d = 1 + ny
    tri = (lambda a: np.asarray(a)) if method == "scam" else (lambda a: np.array([np.triu(m) for m in a]))
    failures = []

    def check(name, got, want):
        got, want = np.asarray(got), np.asarray(want)
        assert got.shape == want.shape, (name, got.shape, want.shape)
        eq = (_bits(got) == _bits(want)) if got.dtype.kind == "f" else (got == want)
        bad = np.flatnonzero(~eq.reshape(nch, -1).all(axis=1))
        if len(bad):
            failures.append("%s: %d chains, the first: %s" % (name, len(bad), bad[:12]))

    assert g["kept"][0] == 2 and g["kept"][1] == 1 and g["kept"][3] == d + 2 * ny + 1, g["kept"]
    check("theta", g["theta"], o["theta"])
    for j, name in enumerate(("ss1", "sspri1", "sigma2", "alpha12")):
        if name != "alpha12" or method != "er":                 # (MCMC_run_er never sets alpha12)
            check(name, g["scal"][:, j], o["scal"][:, j])
    last = g["samples"][1]
    check("ss of every column", last[:, d:d + ny], o["ssv"])
    check("sigma2 of every column", last[:, d + ny + 1:], o["s2v"])
    check("sample 0 of the store", g["samples"][0], o["samples"][0])
    check("the last sample of the store", last, o["samples"][1])
    check("stream position", g["rng"], o["rng"])
    for j, name in enumerate(CTR):
        check(name, g["ctr"][:, j], o["ctr"][:, j])
    check("R", tri(g["R"]), tri(o["R"]))
    if "qstd" in g:
        check("qcovstd", g["qstd"], o["qstd"])
    if "cmat" in g:
        check("chaincmat", g["cmat"], np.array([np.triu(a) for a in o["cmat"]]))
        check("chainmean", g["mean"], o["mean"])
        check("chainwsum", g["wsum"], o["wsum"])
    if "R2" in g:
        check("R2", g["R2"], np.array([np.triu(a) for a in o["R2"]]))
        check("iC", g["iC"], np.array([np.triu(a) for a in o["iC"]]))
    assert not failures, "; ".join(failures)


def _set_env(monkeypatch, env):
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def _engine(ckw, pkw, x, y, nch=NCH, starts=None, shared=False, samples=True):
    """An engine on per-chain data (shared = True: on ONE data set through set_target("expdata"), ydata [ny][ndata])."""
    from mcmcf90_amd import Engine, make_config
    d = int(pkw["npar"])
    e = Engine(make_config(d, nch, chain_id0=CHAIN_ID0, **ckw))
    e.setpar0(pkw["par0"]); e.setcmat0(np.asarray(pkw["cmat0"], dtype=np.float64).reshape(d, d)); e.setsigma2nobs(pkw["sigma2"], pkw["nobs"])
    if shared:
        e.set_target("expdata", xdata=x, ydata=y)
    else:
        e.set_target_all(x, y)
    if pkw.get("lo") is not None or pkw.get("hi") is not None:
        e.set_bounds(pkw.get("lo"), pkw.get("hi"))
    if pkw.get("pri_mu") is not None:
        e.set_priors(pkw["pri_mu"], pkw["pri_sig"])
    if starts is not None:
        e.setpar0_all(starts)
    if samples:
        e.set_samples(first=1, thin=ckw["nsimu"] - 1, capacity=2)
    return e


def _run(monkeypatch, env, ckw, pkw, x, y, kernel, starts=None, cuts=(ADAPTINT, ADAPTINT + 1, None)):
    _set_env(monkeypatch, env)
    e = _engine(ckw, pkw, x, y, nch=y.shape[0], starts=starts)
    try:
        e.init()
        info = e.chain_data_info()
        L64 = -(-y.shape[0] // 64) * 64
        assert info == dict(mode="xy_per_chain" if x.ndim == 2 else "y_per_chain", ndata=y.shape[2], nycol=y.shape[1],
                            bytes=8 * L64 * y.shape[2] * (y.shape[1] + (1 if x.ndim == 2 else 0))), info
        for upto in cuts:
            e.run(upto)
            if kernel is not None:
                assert e.last_kernel() == kernel, e.last_kernel()
        return _state(e, ckw, y.shape[0])
    finally:
        e.close()


def _same(a, b, what):
    for k in a:
        if k == "kept":
            assert a[k] == b[k], (what, k)
        else:
            assert a[k].shape == b[k].shape and a[k].dtype == b[k].dtype, (what, k)
            eq = (_bits(a[k]) == _bits(b[k])) if a[k].dtype.kind == "f" else (a[k] == b[k])
            assert eq.all(), (what, k, int((~eq).sum()))


PHASED = {"MCMCX_COLS_PHASED": "1"}


# ---------------------------------------------------------------- 1. dram with delayed rejection, sigma2 updated, bounds that bite
def test_dram_dr_two_columns_bounds_fused_and_phased(oracle, monkeypatch):
    ckw = dict(nsimu=NSIMU, method="dram", adaptint=ADAPTINT, updatesigma=1, N0=1.0, S02=0.0, drscale=2.0)
    pkw = _problem(2, 7, lo=np.array([0.0, 0.085, 0.0]))
    x, y, truth = _data(2, 7)
    o = _oracle(oracle, "dram_dr", ckw, pkw, x, y)
    # the regime, from the oracle alone: in every full tile second stages are tried and some accepted, and proposals leave the box
    for t in TILES[:2]:
        assert o["ctr"][t, 3].min() > 0 and o["ctr"][t, 2].sum() > 0 and o["ctr"][t, 1].sum() > 0, o["ctr"][t, 1:4].sum(axis=0)
    assert (o["ctr"][:, 1] > 0).sum() > NCH // 4
    fused = _run(monkeypatch, {}, ckw, pkw, x, y, "step_kernel_cols<pcd>")
    _compare(fused, o, ckw, NCH, 2)
    phased = _run(monkeypatch, PHASED, ckw, pkw, x, y, None)    # dev_eval_kernel<true> with use_stage2
    _same(fused, phased, "fused against phase-cut")


# ---------------------------------------------------------------- 2. ram, one column, every chain from its own start
def test_ram_one_column_given_starts(oracle, monkeypatch):
    ckw = dict(nsimu=NSIMU, method="ram", adaptint=ADAPTINT, updatesigma=0)
    pkw = _problem(1, 7, lo=np.zeros(2))
    x, y, truth = _data(1, 7)
    starts = truth * np.exp(0.02 * np.random.default_rng(5).standard_normal((NCH, 2)))     # near each fit's own mode
    o = _oracle(oracle, "ram", ckw, pkw, x, y, starts=starts)
    # the regime, from the oracle alone.  On seven observations the reference's RAM widens its factor until half the proposals leave the
    # box (rate 0.05, the rate parameter's proposal twenty times cmat0's) and most chains meet a failed downdate, after which the chain goes
    # on with the factor it has: every full tile mixes chains with the status bit and chains without, and every chain has moved
    rate, failed = o["acc"][:, 1:].mean(), o["ctr"][:, 5] == 1
    assert 0.02 < rate < 0.5 and (o["acc"][:, 1:].sum(axis=1) > 0).all() and o["ctr"][:, 1].sum() > NCH, (rate, o["ctr"][:, 1].sum())
    for t in TILES[:2]:
        assert 8 <= failed[t].sum() <= 56, failed[t].sum()
    g = _run(monkeypatch, {}, ckw, pkw, x, y, "step_kernel_cols<ram, pcd>", starts=starts)
    _compare(g, o, ckw, NCH, 1)


# ---------------------------------------------------------------- 3. early rejection with priors, three columns, x shared and y per chain
def test_er_priors_three_columns_shared_x_fused_and_phased(oracle, monkeypatch):
    ckw = dict(nsimu=NSIMU, method="er", adaptint=ADAPTINT, updatesigma=1, N0=1.0, S02=0.0)
    pkw = _problem(3, 7, pri_mu=np.array([9.0, 0.1, 0.25, 0.4]), pri_sig=np.array([1.0, -1.0, 0.05, 0.1]))
    x, y, truth = _data(3, 7, x_per_chain=False)
    assert x.shape == (7,)
    o = _oracle(oracle, "er", ckw, pkw, x, y)
    for t in TILES[:2]:                                         # rejected by the prior alone, and by the sum of squares, in every full tile
        assert o["ctr"][t, 6].sum() > 0 and (o["ctr"][t, 0] > o["ctr"][t, 6]).any()
    assert (o["scal"][:, 1] != 0.0).all()
    fused = _run(monkeypatch, {}, ckw, pkw, x, y, "step_kernel_cols<pcd>")
    _compare(fused, o, ckw, NCH, 3)
    phased = _run(monkeypatch, PHASED, ckw, pkw, x, y, None)    # dev_eval_kernel<true> with what = 1 / 2
    _same(fused, phased, "fused against phase-cut")


# ---------------------------------------------------------------- 4. scam, two columns
def test_scam_two_columns(oracle, monkeypatch):
    ckw = dict(nsimu=NSIMU, method="scam", adaptint=ADAPTINT, updatesigma=1, N0=1.0, S02=0.0)
    pkw = _problem(2, 7, lo=np.zeros(3))
    x, y, truth = _data(2, 7)
    o = _oracle(oracle, "scam", ckw, pkw, x, y)
    rate = o["acc"][:, 1:].mean()
    assert 0.2 < rate < 0.999, rate
    g = _run(monkeypatch, {}, ckw, pkw, x, y, "step_kernel_cols<scam, pcd>")
    _compare(g, o, ckw, NCH, 2)


# ---------------------------------------------------------------- 5. one observation per chain
def test_one_observation_per_chain(oracle, monkeypatch):
    ckw = dict(nsimu=NSIMU, method="dram", adaptint=ADAPTINT, updatesigma=0, drscale=0.0)
    pkw = _problem(1, 1)
    x, y, truth = _data(1, 1)
    assert x.shape == (NCH, 1) and y.shape == (NCH, 1, 1)
    o = _oracle(oracle, "ndata1", ckw, pkw, x, y)
    g = _run(monkeypatch, {}, ckw, pkw, x, y, "step_kernel_cols<pcd>")
    _compare(g, o, ckw, NCH, 1)


# ---------------------------------------------------------------- 6. the same data for every chain is the one-data-set run
@pytest.mark.parametrize("ny", [1, 2])
def test_same_data_for_every_chain_is_the_shared_run(monkeypatch, ny):
    ckw = dict(nsimu=120, method="dram", adaptint=ADAPTINT, updatesigma=1, N0=1.0, S02=0.0, drscale=2.0)
    pkw = _problem(ny, 7, lo=np.zeros(1 + ny))
    x, y, truth = _data(ny, 7, nch=1, x_per_chain=False)
    y1 = y[0]                                                   # [ny][ndata]
    _set_env(monkeypatch, {})
    e = _engine(ckw, pkw, x, y1, shared=True)
    try:
        e.init()
        assert e.chain_data_info() == dict(mode="shared", ndata=7, nycol=ny, bytes=0)
        e.run(ADAPTINT); e.run()
        assert e.last_kernel() == "step_kernel_cols"
        want = _state(e, ckw, NCH)
    finally:
        e.close()
    assert len({tuple(_bits(r)) for r in want["theta"]}) > NCH // 2          # (the chains of the shared run differ by their streams)
    for xs in (x, np.tile(x, (NCH, 1))):
        g = _run(monkeypatch, {}, ckw, pkw, xs, np.ascontiguousarray(np.broadcast_to(y1, (NCH,) + y1.shape)), "step_kernel_cols<pcd>",
                 cuts=(ADAPTINT, None))
        _same(want, g, "x per chain" if xs.ndim == 2 else "x shared")


# ---------------------------------------------------------------- 7. refusals, the getter, the last setter wins
def test_refusals_and_chain_data_info(monkeypatch):
    from mcmcf90_amd import Engine, McmcError, _lib, make_config
    L = _lib.load()
    dp = C.POINTER(C.c_double)
    ckw = dict(nsimu=30, method="dram", adaptint=ADAPTINT, updatesigma=0)
    pkw = _problem(2, 7)
    N = 70
    x, y, truth = _data(2, 7, nch=N)
    xp, yp = x.ctypes.data_as(dp), y.ctypes.data_as(dp)
    _set_env(monkeypatch, {})

    def refused(rc, code, word):
        msg = L.mcmcx_last_error().decode()
        assert rc == code and word in msg, (rc, msg, word)

    refused(L.mcmcx_set_target_expdata_all(None, N, 7, 2, xp, 1, yp), -58, "null handle")
    out4 = np.zeros(4, dtype=np.int64)
    o4 = out4.ctypes.data_as(C.POINTER(C.c_int64))
    refused(L.mcmcx_chain_data_info(None, o4), -40, "not inited")
    e = _engine(ckw, pkw, x[0], y[0], nch=N, shared=True, samples=False)
    refused(L.mcmcx_chain_data_info(e.h, o4), -40, "not inited")
    refused(L.mcmcx_set_target_expdata_all(e.h, N, 7, 2, None, 1, yp), -58, "null array")
    refused(L.mcmcx_set_target_expdata_all(e.h, N, 7, 2, xp, 1, None), -58, "null array")
    refused(L.mcmcx_set_target_expdata_all(e.h, N - 1, 7, 2, xp, 1, yp), -58, "nchains")
    refused(L.mcmcx_set_target_expdata_all(e.h, N, 0, 2, xp, 1, yp), -58, "ndata")
    for v in (-1, 2):
        refused(L.mcmcx_set_target_expdata_all(e.h, N, 7, 2, xp, v, yp), -58, "x_per_chain")
    refused(L.mcmcx_set_target_expdata_all(e.h, N, 7, 0, xp, 1, yp), -21, "nycol")
    refused(L.mcmcx_set_target_expdata_all(e.h, N, 7, 3, xp, 1, yp), -22, "npar")
    # none of these changed the handle: it runs on the one data set it was given
    e.init()
    assert e.chain_data_info() == dict(mode="shared", ndata=7, nycol=2, bytes=0)
    refused(L.mcmcx_chain_data_info(e.h, None), -1, "null")
    refused(L.mcmcx_set_target_expdata_all(e.h, N, 7, 2, xp, 1, yp), -58, "after mcmcx_init")
    e.run()
    assert e.simuind == 30 and e.last_kernel() == "step_kernel_cols"
    shared_theta = e.theta()
    e.close()
    # pooled mode
    e = Engine(make_config(3, N, pooled=1, **ckw))
    refused(L.mcmcx_set_target_expdata_all(e.h, N, 7, 2, xp, 1, yp), -58, "pooled")
    with pytest.raises(McmcError, match="pooled"):
        e.set_target_all(x, y)
    e.close()
    # the last target setter called wins, both ways
    e = _engine(ckw, pkw, x, y, nch=N, samples=False)
    e.set_target("expdata", xdata=x[0], ydata=y[0])
    e.init(); e.run()
    assert e.chain_data_info()["mode"] == "shared" and (_bits(e.theta()) == _bits(shared_theta)).all()
    e.close()
    e = _engine(ckw, pkw, x[0], y[0], nch=N, shared=True, samples=False)
    e.set_target_all(x, y)
    e.init(); e.run()
    assert e.chain_data_info() == dict(mode="xy_per_chain", ndata=7, nycol=2, bytes=8 * 128 * 7 * 3)
    assert e.last_kernel() == "step_kernel_cols<pcd>" and (_bits(e.theta()) != _bits(shared_theta)).any()
    e.close()
