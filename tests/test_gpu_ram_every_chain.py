"""Every chain of every method = 'ram' kernel form against the oracle, beyond eight ragged tiles.

The other RAM tests compare three to five chains of 66..70 with the oracle, on at most three tiles, and the remaining chains only
between two device forms: an error that depends on where a chain sits -- its row group in a wave that mixes update and downdate
lanes, its slot in a group_ram_kernel wave, a tile past the eighth (one round of the XCD round-robin) -- would pass, and so would
one that two forms share.  Here 583 chains (nine full tiles and seven chains: a ragged tile, and a ragged group wave of three
chains) run 150 iterations from cmat0 = inv(lam), where the chain sits near alphatarget and most iterations downdate, cut as
run(60), run(61), run(); and EVERY chain's state, accept sequence, factor, stream position, counters and status bit must be the
oracle's (MCMC_run_ram.F90:45-179, dchud.f:122-139, dchdd.f:141-179), bit for bit."""
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import edge_problems as ep

pytestmark = pytest.mark.gpu

NCH, NSIMU, CUTS, CHAIN_ID0 = 583, 150, (60, 61, None), 6
SWITCHES = ("MCMCX_GROUP", "MCMCX_GROUP_GW", "MCMCX_RAM_GROUP", "MCMCX_RAM_WIDE", "MCMCX_LDS_SCRATCH", "MCMCX_COLS_PHASED")
BOUNDED = (10, 12, 17, 20, 21, 33, 35, 57)      # a third of the cases: proposals outside the bounds leave alpha12 stale (MCMC_run_ram.F90:52-54)
SIGMA2 = (34,)                                  # the sigma2 update on one

# kernel form, what forces it, npar
CASES = [("step_kernel_ram_ldsr", dict(MCMCX_RAM_GROUP="0"), d) for d in (7, 10)] + \
        [("step_kernel<true, false, false>", dict(MCMCX_RAM_GROUP="0"), d) for d in (11, 20)] + \
        [("step_kernel<true, false, false>", dict(MCMCX_RAM_GROUP="0", MCMCX_RAM_WIDE="0"), 50)] + \
        [("step_kernel_ram_wide", dict(MCMCX_RAM_GROUP="0"), d) for d in (21, 34, 35, 50, 64)] + \
        [("group_ram_kernel", dict(MCMCX_RAM_GROUP="1"), d) for d in (16, 17, 32, 33, 56, 57, 64)] + \
        [("step_kernel_ram_fullr", dict(), 12), ("step_kernel_cols<ram>", dict(), 3)]
CASES = [k + (None,) for k in CASES]
# sums of squares that are +inf, NaN or subnormal (tests/edge_problems.py; "ovf:T:c" and "sub:e" as in tests/test_gpu_every_chain.py, T and c chosen on
# the CPU so that the oracle alone meets _regime's conditions).  A NaN alpha draws no uniform, rejects (MCMC_DRAM.F90:140-155) and reaches
# MCMC_adapt_ram as it is: a = NaN fails `a >= 0`, the downdate's norm test `norm < 1` fails on NaN and leaves the factor untouched
# (dchdd.f:150-153; the reference stops there, the engine and the oracle flag the chain and go on)
for _d, _edge in ((20, "ovf:25:0.3"), (50, "ovf:60:0.15"), (20, "sub:1030")):
    CASES += [("step_kernel<true, false, false>", dict(MCMCX_RAM_GROUP="0", MCMCX_RAM_WIDE="0"), _d, _edge), ("group_ram_kernel", dict(MCMCX_RAM_GROUP="1"), _d, _edge)]
CASES += [("step_kernel_ram_wide", dict(MCMCX_RAM_GROUP="0"), 50, "ovf:60:0.15")]


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _problem(kernel, d, edge=None):
    ckw = dict(nsimu=NSIMU, method="ram", adaptint=100, updatesigma=1 if d in SIGMA2 else 0)
    if kernel == "step_kernel_cols<ram>":                       # two response columns, the start of tests/test_gpu_fuzz.py's _draw_cols
        r = np.random.default_rng(31)
        x = np.arange(11.0)
        rates = np.array([0.1, 0.25])
        Y = np.vstack([9.0 * np.exp(-k * x) + r.standard_normal(11) * 0.3 for k in rates])
        pkw = dict(kind="expdata", npar=3, par0=np.concatenate([[9.0], rates]), cmat0=10.0 * np.diag([0.02, 0.0002, 0.0002]),
                   sigma2=np.array([0.6, 0.9]), nobs=np.array([11, 14]), xdata=x, ydata=Y, lo=np.zeros(3))
        return dict(ckw, N0=1.0, S02=0.0), pkw
    r = np.random.default_rng(3000 + d)
    A = r.standard_normal((d, d)) / np.sqrt(d)
    lam = A @ A.T + np.eye(d)
    pkw = dict(kind="gauss", npar=d, par0=np.full(d, 0.1), cmat0=np.linalg.inv(lam), mu=np.linspace(-0.5, 0.5, d), lam=lam)
    if edge:
        how, *arg = edge.split(":")
        return ckw, (ep.subnormal(d, 2.0 ** -int(arg[0])) if how == "sub" else ep.overflow(d, float(arg[0]), float(arg[1])))
    if d in BOUNDED:
        pkw.update(lo=np.full(d, -2.5), hi=np.full(d, 2.5))     # (the oracle: 2 to 16 proposals per chain land outside, rate 0.17..0.27)
    if d in SIGMA2:
        pkw.update(sigma2=0.8, nobs=15)
    if kernel == "step_kernel_ram_fullr":                       # the full SVD factor of a dense cmat0 through matmulx, dchud and dchdd
        ckw.update(condmax=1e8)
        # (inv() returns a matrix whose triangles differ in the last bits.  The pinned dgesvd is defined for a symmetric matrix: the engine
        #  mirrors cmat0's upper triangle into it, the oracle hands it the matrix as it stands like the reference -- so the two are given one)
        pkw["cmat0"] = 0.5 * (pkw["cmat0"] + pkw["cmat0"].T)
    return ckw, pkw


_ORACLE = {}


def _oracle_all(oracle, kernel, d, edge=None):
    """All 583 chains of a problem through the oracle: computed once per problem (npar 50 and 64 serve two forms), never changed."""
    key = (kernel in ("step_kernel_ram_fullr", "step_kernel_cols<ram>"), d, edge)
    if key not in _ORACLE:
        ckw, pkw = _problem(kernel, d, edge)
        cfg = oracle.make_cfg(**ckw); prob = oracle.Problem(**pkw)
        o = dict(theta=np.zeros((NCH, d)), acc=np.zeros((NCH, NSIMU), dtype=np.uint8), R=np.zeros((NCH, d, d)), rng=np.zeros(NCH, dtype=np.uint64),
                 stayed=np.zeros(NCH, dtype=np.int64), bndstayed=np.zeros(NCH, dtype=np.int64), fail=np.zeros(NCH, dtype=bool),
                 scal=np.zeros((NCH, 4)), ssinf=np.zeros(NCH, dtype=np.int64), ssnan=np.zeros(NCH, dtype=np.int64), nprop=np.zeros(NCH, dtype=np.int64))
        oracle.lib()
        # (the oracle keeps no state outside a chain and ctypes releases the GIL: a thread pool, as in tests/test_gpu_every_chain.py)
        with ThreadPoolExecutor(min(16, os.cpu_count() or 1)) as pool:
            rs = list(pool.map(lambda c: oracle.run_chain(cfg, prob, chain_id=CHAIN_ID0 + c, continue_on_downdate_fail=True), range(NCH)))
        assert len(rs) == NCH
        for c, r in enumerate(rs):
            assert r.simuind == NSIMU
            o["theta"][c], o["acc"][c], o["R"][c], o["rng"][c] = r.theta, r.accepted, r.R, r.rng_n
            o["stayed"][c], o["bndstayed"][c], o["fail"][c] = r.stayed, r.bndstayed, r.ram_downdate_fail != 0
            o["scal"][c], o["ssinf"][c], o["ssnan"][c], o["nprop"][c] = (r.ss1, r.sspri1, r.sigma2, r.alpha12), r.n_ss_inf, r.n_ss_nan, r.nprop
        for v in o.values():
            v.setflags(write=False)
        _ORACLE[key] = o
    return _ORACLE[key]


def _regime(pkw, d, edge, o):
    """The regime, from the oracle alone: near the target rate, where about three iterations in four downdate"""
    if pkw["kind"] != "gauss":
        return
    rate = o["acc"][:, 1:].mean()                               # (row 0 is the start point)
    if edge:
        # no NaN and no infinity in a state or factor (the reference's fixture tests/golden/edge/x3_ovf20_ram.npz shows none), whatever alpha was
        assert np.isfinite(o["theta"]).all() and np.isfinite(o["R"]).all()
        if edge.startswith("sub"):
            ss1 = o["scal"][:, 0]
            assert ep.is_subnormal(ss1).all() and len(np.unique(ss1)) == NCH, (ss1.min(), ss1.max(), len(np.unique(ss1)))
            assert 0.1 < rate < 0.5, rate
            return
        tiles = [slice(t, t + 64) for t in range(0, NCH - 63, 64)]
        ninf, nnan, nprop = o["ssinf"].sum(), o["ssnan"].sum(), float(o["nprop"].sum())
        print("d %d %s: rate %.3f, ss = +inf %.4f, NaN %.4f of %d proposals; chains flagged %d" % (d, edge, rate, ninf / nprop, nnan / nprop, nprop, o["fail"].sum()))
        assert 0.1 < rate < 0.75, rate
        assert ninf >= 0.01 * nprop and nnan >= 0.005 * nprop, (ninf / nprop, nnan / nprop)
        assert all(o["ssnan"][t].any() for t in tiles) and all(o["ssinf"][t].any() for t in tiles)      # every full tile holds both
        return
    assert 0.1 < rate < 0.5, rate
    if d in BOUNDED:
        assert o["bndstayed"].sum() > NCH                       # the bounds bite: more than one proposal per chain lands outside


@pytest.mark.parametrize("kernel,env,d,edge", CASES, ids=["%s-%d%s%s" % (k.split("<")[0] + ("_narrow" if "true" in k else "_ram" if "<ram>" in k else ""), d,
                                                                         "_wide0" if "MCMCX_RAM_WIDE" in e and not x else "", "_" + x if x else "") for k, e, d, x in CASES])
def test_every_chain_of_a_ram_form_equals_the_oracle(oracle, monkeypatch, kernel, env, d, edge):
    from mcmcf90_amd import engine_from_problem
    ckw, pkw = _problem(kernel, d, edge)
    o = _oracle_all(oracle, kernel, d, edge)
    _regime(pkw, d, edge, o)                                    # ... before the engine is touched
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    e = engine_from_problem(ckw, pkw, nchains=NCH, chain_id0=CHAIN_ID0, record_accept=1)
    e.init()
    for upto in CUTS:
        e.run(upto)
        assert e.last_kernel() == kernel, e.last_kernel()
    assert e.simuind == NSIMU
    theta, masks, scal = e.theta(), e.accept_masks(), e.scalars()
    assert masks.shape == (NSIMU, (NCH + 63) // 64)
    Rs = [e.R(c) for c in range(NCH)]
    rng = np.array([e.rng(c)[0] for c in range(NCH)], dtype=np.uint64)
    ctr = [e.counters(c) for c in range(NCH)]
    e.close()
    c = np.arange(NCH)
    acc = ((masks[:, c // 64] >> (c % 64).astype(np.uint64)) & np.uint64(1)).astype(np.uint8).T         # [chain][iteration]
    assert acc.shape == o["acc"].shape and theta.shape == o["theta"].shape and len(Rs) == len(ctr) == NCH     # no chain is left out

    def chains(bad):
        bad = np.flatnonzero(bad)
        return "%d chains, the first: %s" % (len(bad), bad[:12])

    bad = np.any(acc != o["acc"], axis=1)
    assert not bad.any(), "accept sequence: " + chains(bad)
    bad = np.any(_bits(theta) != _bits(o["theta"]), axis=1)
    assert not bad.any(), "theta: " + chains(bad)
    full = kernel == "step_kernel_ram_fullr"                    # the SVD form's factor is a full matrix
    bad = np.array([np.any(_bits(R if full else np.triu(R)) != _bits(Ro if full else np.triu(Ro))) for R, Ro in zip(Rs, o["R"])])
    assert not bad.any(), "R: " + chains(bad)
    bad = rng != o["rng"]
    assert not bad.any(), "stream position: " + chains(bad)
    bad = np.array([k["stayed"] for k in ctr]) != o["stayed"]
    assert not bad.any(), "stayed: " + chains(bad)
    bad = np.array([k["bndstayed"] for k in ctr]) != o["bndstayed"]
    assert not bad.any(), "bndstayed: " + chains(bad)
    bad = np.array([bool(k["status"] & 1) for k in ctr]) != o["fail"]
    assert not bad.any(), "failed-downdate flag: " + chains(bad)
    if edge:
        # ss1 bit for bit (a NaN proposal is never accepted); the last alpha too, except that a NaN equals a NaN whatever its sign and payload
        # (x86 and gfx950 generate different default NaNs)
        bad = _bits(scal[:, 0]) != _bits(o["scal"][:, 0])
        assert not bad.any(), "ss1: " + chains(bad)
        bad = ~ep.same_bits_or_nan(scal[:, 3], o["scal"][:, 3])
        assert not bad.any(), "alpha12: " + chains(bad)
