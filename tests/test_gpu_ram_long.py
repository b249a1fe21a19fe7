"""BASELINE config 4 exactly as written -- method = 'ram', npar 50, cmat0 = 0.01 I, nsimu = 200 000 -- on the device against the real
reference's run (tests/golden/long/c4_gauss50_ram_200k.npz, oracle/gen_golden.py) and against the oracle.

No other RAM comparison with the reference is longer than 6000 iterations.  67 chains (a ragged second tile, a group wave of three
chains), the fixture's stream on chain 1, no recorded chain: the accept ballots give the run-length column, the thinned sample
store (every 1000th iteration) gives the states along the run.  group_ram_kernel, the engine's own choice at this size, runs all
200 000 iterations; step_kernel_ram_wide the first 20 000.  From cmat0 = 0.01 I the chain still accepts 86 % of its proposals at the
end (171 472 updates); the second fixture is the same run from the target's own covariance, at alphatarget throughout (152 867
downdates of one factor), all of it on group_ram_kernel."""
import time

import numpy as np
import pytest
from golden_util import load, accepted_from_runlen, state_at, LONG_RTOL

pytestmark = pytest.mark.gpu

NCH, THIN = 67, 1000
FIXTURE_CHAIN, LAST_CHAIN = 1, NCH - 1
SWITCHES = ("MCMCX_GROUP", "MCMCX_GROUP_GW", "MCMCX_RAM_GROUP", "MCMCX_RAM_WIDE", "MCMCX_LDS_SCRATCH")


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _kw(z):
    ckw = {k[4:]: z[k].item() for k in z.files if k.startswith("cfg_") and k[4:] not in ("dodr", "doscam", "usesvd")}
    pkw = {k[5:]: (z[k].item() if z[k].ndim == 0 else z[k]) for k in z.files if k.startswith("prob_")}
    return ckw, pkw


_ORACLE = {}


def _oracle_run(oracle, name, cfg, prob, chain_id, upto):
    """One oracle chain up to `upto`: computed once, never changed (4 s of CPU for the 200 000 iterations)."""
    if (name, chain_id, upto) not in _ORACLE:
        o = oracle.run_chain(cfg, prob, chain_id=chain_id, upto=upto)
        assert o.rc == 0 and not o.ram_downdate_fail and o.simuind == upto
        _ORACLE[(name, chain_id, upto)] = o
    return _ORACLE[(name, chain_id, upto)]


@pytest.mark.parametrize("name,kernel,env,upto", [("c4_gauss50_ram_200k", "group_ram_kernel", {}, 200000),
                                                  ("c4_gauss50_ram_200k", "step_kernel_ram_wide", dict(MCMCX_RAM_GROUP="0"), 20000),
                                                  # the same run from the target's own covariance, at alphatarget throughout: 152 867 downdates of
                                                  # one factor (a downdate iteration costs the kernel twice an update's time: 9.5 s for the run)
                                                  ("c4t_gauss50_ram_target_200k", "group_ram_kernel", {}, 200000)],
                         ids=["group_200k", "wide_20k", "target_start_group_200k"])
def test_config4_as_written_against_reference_and_oracle(oracle, monkeypatch, name, kernel, env, upto):
    from mcmcf90_amd import engine_from_problem
    z, cfg, prob = load("long/" + name, oracle)
    ckw, pkw = _kw(z)
    cid, d = int(z["chain_id"]), prob.npar
    assert cfg.nsimu == 200000 and upto % THIN == 0
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    e = engine_from_problem(ckw, pkw, nchains=NCH, chain_id0=cid - FIXTURE_CHAIN, record_accept=1)
    e.set_samples(first=THIN, thin=THIN)
    e.init()
    t0 = time.perf_counter()
    e.run(upto); e.sync()
    print("%s: %d iterations of %d chains in %.2f s" % (kernel, upto, NCH, time.perf_counter() - t0))
    assert e.last_kernel() == kernel, e.last_kernel()
    assert e.simuind == upto
    nkept = upto // THIN
    # --- against the real reference: the fixture's stream
    want = accepted_from_runlen(z["runlen"])
    assert len(want) == cfg.nsimu
    np.testing.assert_array_equal(e.accepted(FIXTURE_CHAIN), want[:upto])
    if upto == cfg.nsimu:
        assert e.rng(FIXTURE_CHAIN)[0] == int(z["rng_n"])
    its, S = e.samples()                                        # [kept][chain][theta, ss, sspri, sigma2]
    assert list(its) == list(z["thin_its"][:nkept]) and S.shape == (nkept, NCH, d + 3)
    scale = np.maximum(np.abs(z["rows_tail"]).max(axis=0), 1e-3)
    dev = np.max(np.abs(S[:, FIXTURE_CHAIN, :d] - z["thin_rows"][:nkept]) / scale)
    print("%s against the reference's thinned rows: %.3g" % (kernel, dev))
    assert dev < LONG_RTOL, dev
    theta = e.theta()
    if upto == cfg.nsimu:
        assert np.max(np.abs(theta[FIXTURE_CHAIN] - z["rows_tail"][-1]) / scale) < LONG_RTOL
    # --- against the oracle, bit for bit: the fixture's chain and the last one of the ragged tile
    for c in (FIXTURE_CHAIN, LAST_CHAIN):
        o = _oracle_run(oracle, name, cfg, prob, cid - FIXTURE_CHAIN + c, upto)
        np.testing.assert_array_equal(e.accepted(c), o.accepted)
        np.testing.assert_array_equal(_bits(theta[c]), _bits(o.theta))
        np.testing.assert_array_equal(_bits(np.triu(e.R(c))), _bits(np.triu(o.R)))
        assert e.rng(c)[0] == o.rng_n
        cnt = e.counters(c)
        assert (cnt["stayed"], cnt["bndstayed"], cnt["status"] & 1) == (o.stayed, o.bndstayed, 0)
        np.testing.assert_array_equal(_bits(S[:, c, :d]), _bits(state_at(o.chain[:, :-1], o.chain[:, -1], its)))
        np.testing.assert_array_equal(_bits(S[:, c, d]), _bits(state_at(o.sschain[:, 0], o.sschain[:, -1], its)))
    e.close()
