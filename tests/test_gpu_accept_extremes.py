"""Every per-chain kernel form at the two ends of the accept ballot -- chains that accept nothing in an adaptation window, chains that accept at
every iteration of it -- and the two side by side in one wave, on every chain, bit for bit, against the oracle.

tests/test_gpu_every_chain.py and tests/test_gpu_ram_every_chain.py run one regime: a first-stage acceptance rate of 0.1 .. 0.5, "so that lanes accept at
different iterations".  The branches written out for the ends are reached rarely or never there: adapt_pre_kernel's AM row list of the base row alone
with weight w - lastfreq (nr == 0), its AP walk-back over a run of unset ballots down to t2 > 1, covmat_window_td's only fold being the one after the
loop (cnt - adj), covmat_batch_td and covmat_rows given one row and dividing by wsum2 - 1, the burn-in branch at staypc = 1 and at staypc = 0, a
second-stage try at every iteration, alpha12 stale at every iteration of method = 'ram' and a downdate behind it; and at the other end a row per
iteration with every weight 1, hist and wacc rewritten in every slot while the ring wraps (wcap = 2 adaptint + 2 < nsimu), a fold at every q of the
64-iteration ballot chunks, alpha >= 1 and no uniform drawn, drtries = 0.  Whole tiles of either kind make __any(acc) false for a window, or
__any(upd) and __any(fl) true on all 64 lanes at every step -- the same in the sixteen-lane group waves, the quad waves and the accept bytes that
group_pack_kernel turns into ballots.

The chains are tests/box_problems.py's: a flat target in a box, a start per chain (Engine.setpar0_all), 583 chains from chain_id0 = 6.  A chain's
accept sequence is then a matter of geometry, and the oracle runs these chains as they stand (tests/test_box_cpu.py ties it to the reference in
these regimes).  box_problems.regime() is asserted from the oracle alone before the engine is touched, and tests/test_box_cpu.py asserts it for every
problem of this file without a GPU.  adaptint is 63, 64 and 65 over the cases: the first window ends before, on and behind a ballot chunk.
The comparison is tests/test_gpu_every_chain.py's (_run_and_compare), with the status bits added: a chain whose window holds too few distinct rows
has a covariance dpotrf refuses, keeps its factor (MCMC_adapt.F90:168-171) and carries ST_CHOL_FAIL; with method = 'ram' the oracle's
failed-downdate flag is bit 1.  No tolerance anywhere.

What follows from the regime: in every non-RAM case 221 .. 332 of the 583 chains carry ST_CHOL_FAIL at the end (none where initcmatn = 7 starts the
covariance from cmat0) -- about two chains in five never take a new factor and propose from cmat0's throughout, or from what burn-in scaled it to; the
new-factor path is the other chains'.  In the RAM cases 361 .. 373 chains fail their downdate at iteration 2 and run on under the engine's and the oracle's
flag-and-go-on convention, which the reference does not have (it stops there: tests/test_box_cpu.py).

Where the chains themselves bound the regime (box_problems.regime has the reasons): in the one window from the last burn-in tick to the first covariance
tick no tile is sure to hold a chain that accepts at every iteration (two to six chains of the 583 do), and the greedy restart is taken by 2 .. 4 % of
the chains at a burn-in tick; the RAM cases at npar 10 and 17 start from a chain_id0 of their own, at which tile 4 accepts nothing in the whole run."""
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import box_problems as bx
import test_gpu_every_chain as ec

pytestmark = pytest.mark.gpu

NCH, CHAIN_ID0 = 583, 6
ST_RAM_DOWNDATE_FAIL, ST_CHOL_FAIL = 1, 2


def B(d, adaptint, **opt):
    """A problem: npar, adaptint and what departs from the plain adaptive Metropolis run (hashable: the key of the oracle's cache)."""
    return (d, adaptint, tuple(sorted(opt.items())))


def _id0(prob):
    return dict(prob[2]).get("id0", CHAIN_ID0)


def _problem(oracle, prob):
    """(cfg keywords, problem keywords, every tick in order, burn-in ticks, run cuts) of a problem"""
    d, adaptint, opt = prob[0], prob[1], dict(prob[2])
    ckw = dict(nsimu=3 * adaptint + 8, method=opt.get("method", "dram"), adaptint=adaptint, updatesigma=0, drscale=opt.get("drscale", 0.0))
    if ckw["method"] == "ram":
        assert adaptint == 100
        ckw["nsimu"] = 150
        return ckw, bx.box(d), [], [], (100, 101, None)
    if opt.get("burnin"):
        ckw.update(ec.BURN)
    for k in ("adapthist", "initcmatn"):
        if k in opt:
            ckw[k] = opt[k]
    if "adapthist" in opt:                                      # the first tick is the first multiple of adaptint from adaptint + adapthist on
        ckw["nsimu"] = 4 * adaptint + 8
    burn, cov = bx.ticks(oracle.make_cfg(**ckw))
    tk = burn + cov
    assert len(tk) >= 2 and tk == sorted(tk) and ckw["nsimu"] >= 3 * adaptint + 8 > 2 * adaptint + 2
    return ckw, bx.box(d), tk, burn, (tk[0], tk[0] + 1, tk[1], None)


_ORACLE = {}


def oracle_all(oracle, prob):
    """Every chain of a problem through the oracle, each from its own start (a Problem per chain): once per problem, never changed.  The run pauses at
    every tick and notes the counters there (pyoracle.run_chain's marks)."""
    if prob not in _ORACLE:
        ckw, pkw, tk, _, _ = _problem(oracle, prob)
        d, nsimu, ram = int(pkw["npar"]), ckw["nsimu"], ckw["method"] == "ram"
        X, m = bx.starts(d, NCH)
        cfg = oracle.make_cfg(**ckw)
        probs = [oracle.Problem(**dict(pkw, par0=X[c])) for c in range(NCH)]
        oracle.lib()
        with ThreadPoolExecutor(min(16, os.cpu_count() or 1)) as pool:
            rs = list(pool.map(lambda c: oracle.run_chain(cfg, probs[c], chain_id=_id0(prob) + c, continue_on_downdate_fail=ram, marks=tk), range(NCH)))
        o = dict(ec._pack(rs, NCH, d, nsimu))
        o["fail"] = np.array([r.ram_downdate_fail != 0 for r in rs])
        o["status"] = np.array([ST_RAM_DOWNDATE_FAIL * int(r.ram_downdate_fail != 0) + ST_CHOL_FAIL * int(r.chol_failed) for r in rs], dtype=np.int64)
        o["marks"] = np.array([r.marks for r in rs], dtype=np.int64).reshape(NCH, len(tk), 5)
        o["X"], o["m"] = X, m
        for k in ("fail", "status", "marks", "X", "m"):
            o[k].setflags(write=False)
        _ORACLE[prob] = o
    return _ORACLE[prob]


def regime(oracle, prob, o):
    """box_problems.regime() on a problem's oracle chains"""
    ckw, pkw, tk, burn, _ = _problem(oracle, prob)
    if ckw["method"] == "ram":
        bx.regime(o["acc"], prob[0], tk, ram=True, fail=o["fail"])
        return
    bx.regime(o["acc"], prob[0], tk, drtries1=o["marks"][:, 0, 1] if ckw["drscale"] else None,
              burn=(burn, ec.BURN["scalelimit"]) if burn else None)


def _cases():
    C = []

    def add(label, prob, kernel, *envs):
        env = {}
        for e in envs:
            env.update(e)
        C.append(pytest.param(prob, kernel, env, id="%s-box%d_a%d%s" % (label, prob[0], prob[1], "".join("_%s%s" % kv for kv in prob[2]))))
    LANE, GRP, QUAD = ec.LANE, ec.GRP, ec.QUAD
    lds0, rows = dict(MCMCX_LDS_SCRATCH="0"), dict(MCMCX_COV_BATCH_ROWS="1")
    # ---- lane kernels.  The npar values are the smallest at which the form's blocks and seams exist and the corner still never accepts
    add("lane", B(10, 63), ec.LDSR, LANE)
    add("lane", B(11, 64), ec.LDSV, LANE, dict(MCMCX_LDS_SCRATCH="1")); add("lane", B(50, 65), ec.LDSV, LANE)
    add("lane", B(23, 64), ec.AM, LANE, lds0)                   # two blocks of ten and a ragged one of three
    w20 = B(20, 65, initcmatn=7)                                # the first tick is a Welford tick
    add("lane_blocks", w20, ec.AM, LANE, lds0); add("lane_rows", w20, ec.AM, LANE, lds0, rows)
    add("lane", B(13, 63, drscale=3.0), "step_kernel_dr", LANE, dict(MCMCX_DR_BIG="0"))
    add("lane", B(20, 64, drscale=2.0), "step_kernel_dr_big", LANE, dict(MCMCX_DR_BIG="1"))
    er20 = B(20, 63, method="er")
    add("lane", er20, ec.LDSV, LANE)
    b20, b20dr = B(20, 64, burnin=1), B(20, 65, burnin=1, drscale=2.0)     # shrink, grow and greedy restart are lanes of known kind
    add("lane", b20, ec.LDSV, LANE); add("lane", b20dr, "step_kernel_dr", LANE, dict(MCMCX_DR_BIG="0"))
    # ---- sixteen-lane groups
    for d, a in ((17, 65), (33, 63)):
        for tf in ("1", "0"):
            add("group_tf" + tf, B(d, a), "group_step_kernel", GRP, dict(MCMCX_TILE_FACTOR=tf))
    add("group", B(50, 65), "group_step_kernel", GRP)
    ap21 = B(21, 64, adapthist=70)                              # the AP window: every tick takes the batch branch
    add("group_blocks", ap21, "group_step_kernel", GRP); add("group_rows", ap21, "group_step_kernel", GRP, rows)
    add("group", B(17, 64, drscale=3.0), "group_step_kernel<DR>", GRP); add("group", B(24, 63, drscale=2.0), "group_step_kernel<DR2>", GRP)
    add("group", b20, "group_step_kernel", GRP); add("group", er20, "group_step_kernel", GRP)
    # ---- quads
    add("quad", B(10, 63), "group_step_kernel<quad>", QUAD); add("quad", B(13, 63, drscale=3.0), "group_step_kernel<quad, DR>", QUAD)
    # ---- method = 'ram', the switches of tests/test_gpu_ram_every_chain.py: out of bounds at every iteration leaves alpha12 stale, and a downdate follows
    # (after a run of downdates a corner chain's proposal is no longer isotropic, and one accept moves it off its walls: with ten walls tile 4
    #  accepts nothing in the whole run for one chain_id0 in five thousand, with seventeen for most but not for 6 -- the chain_id0 of these two
    #  was searched for on the CPU with the oracle, as the regime is a condition on the inputs)
    RAM_ID0 = {10: 5732, 17: 10}
    R = lambda d: B(d, 100, method="ram", **({"id0": RAM_ID0[d]} if d in RAM_ID0 else {}))
    nogroup = dict(MCMCX_RAM_GROUP="0")
    add("ram", R(10), "step_kernel_ram_ldsr", nogroup); add("ram", R(20), "step_kernel<true, false, false>", nogroup)
    add("ram", R(34), "step_kernel_ram_wide", nogroup); add("ram", R(50), "step_kernel_ram_wide", nogroup)
    add("ram", R(17), "group_ram_kernel", dict(MCMCX_RAM_GROUP="1")); add("ram", R(33), "group_ram_kernel", dict(MCMCX_RAM_GROUP="1"))
    return C


CASES = _cases()
PROBLEMS = sorted({p.values[0] for p in CASES}, key=repr)       # tests/test_box_cpu.py asserts the regime of each without a GPU


@pytest.mark.parametrize("prob,kernel,env", CASES)
def test_every_chain_at_the_ends_of_the_accept_ballot_equals_the_oracle(oracle, monkeypatch, prob, kernel, env):
    from mcmcf90_amd import engine_from_problem
    ckw, pkw, tk, _, cuts = _problem(oracle, prob)
    o = oracle_all(oracle, prob)
    regime(oracle, prob, o)                                     # ... before the engine is touched
    for k in ec.SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    e = engine_from_problem(ckw, pkw, nchains=NCH, chain_id0=_id0(prob), record_accept=1)
    e.setpar0_all(o["X"])
    e.init()
    failures = ec._run_and_compare(e, o, ckw, NCH, cuts, kernel)
    assert not failures, "; ".join(failures)
