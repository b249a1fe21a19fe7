"""tests/box_problems.py on the CPU: the oracle against the REAL reference on chains that accept at every iteration, at one in thirty-two and never
(dev container only: needs oracle/_ref/mcxref; skipped elsewhere), and the regime of every problem of tests/test_gpu_accept_extremes.py from the oracle
alone, so that a GPU case's worth is known before a GPU is involved.

tests/test_oracle_fuzz_reference.py draws smooth targets: its chains accept a fifth to a half of their proposals.  The GPU file compares the engine with
the oracle where a window holds no accepted row, or nothing but accepted rows; here the oracle is tied to mcmcf90 itself there -- identical run-length
column, identical number of uniforms drawn, states to BLAS/libm rounding (that file's tolerance)."""
import numpy as np
import pytest

import box_problems as bx
import test_gpu_accept_extremes as ax
import test_gpu_every_chain as ec

D = 10
CONFIGS = {
    "dram": dict(),
    "dr2": dict(drscale=2.0),
    "er": dict(method="er"),
    "ap70": dict(adapthist=70, nsimu=264),
    "initcmatn0": dict(initcmatn=0),
    "burnin": dict(ec.BURN),
    "burnin_dr2": dict(ec.BURN, drscale=2.0),
}
KINDS = (0, 5, D)                                                # walls: the centre, five walls (one proposal in thirty-two lands inside), the corner
CHAINS = [(m, sgn) for m in KINDS for sgn in (+1.0, -1.0)]      # two chains of each kind


def _start(m, sgn):
    x = np.zeros(D)
    x[:m] = sgn * bx.EDGE
    return x


def _ckw(name):
    return dict(dict(nsimu=200, method="dram", adaptint=64, updatesigma=0), **CONFIGS[name])


def _agree(r, o, what):
    np.testing.assert_array_equal(r.chain[:, -1].astype(np.int64), o.chain[:, -1].astype(np.int64), err_msg=str(what))
    assert r.rng_n == o.rng_n, what
    scale = np.maximum(np.abs(o.chain[:, :-1]).max(axis=0), 1e-3)
    assert np.max(np.abs(r.chain[:, :-1] - o.chain[:, :-1]) / scale) < 1e-7, what


@pytest.mark.parametrize("name", list(CONFIGS))
def test_oracle_equals_reference_in_the_box(oracle, name):
    from oracle import refrun as rr
    if not rr.available():
        pytest.skip("oracle/_ref/mcxref not built (needs the reference's sources)")
    ckw = _ckw(name)
    cfg = oracle.make_cfg(**ckw)
    seen = []
    for k, (m, sgn) in enumerate(CHAINS):
        prob = oracle.Problem(**dict(bx.box(D), par0=_start(m, sgn)))
        o = oracle.run_chain(cfg, prob, chain_id=ax.CHAIN_ID0 + k)
        assert o.rc == 0 and o.simuind == ckw["nsimu"]
        r = rr.run_reference(cfg, prob, chain_id=ax.CHAIN_ID0 + k)
        _agree(r, o, (name, m, sgn))
        seen.append((m, int(o.accepted[1:64].sum())))
    # the chains are what they are meant to be: the centre accepts at every iteration of the first window, the corner (nearly) never
    assert all(n == 63 for m, n in seen if m == 0) and all(n <= 2 for m, n in seen if m == D), seen


@pytest.mark.parametrize("m,sgn", CHAINS + [(1, +1.0), (1, -1.0)])
def test_oracle_equals_reference_in_the_box_ram(oracle, m, sgn):
    """method = 'ram': full agreement on the chains the oracle does not flag; where it flags a failed downdate the reference has stopped
    (matutils.F90:719-722) -- the engine and the oracle flag the chain and go on, tests/test_gpu_parity.py pins that convention -- in choldowndate,
    at the oracle's iteration and stream position."""
    from oracle import refrun as rr
    if not rr.available():
        pytest.skip("oracle/_ref/mcxref not built (needs the reference's sources)")
    ckw = dict(nsimu=150, method="ram", adaptint=100, updatesigma=0)
    cfg = oracle.make_cfg(**ckw)
    prob = oracle.Problem(**dict(bx.box(D), par0=_start(m, sgn)))
    cid = ax.CHAIN_ID0 + m
    o = oracle.run_chain(cfg, prob, chain_id=cid, continue_on_downdate_fail=True)
    r = rr.run_reference(cfg, prob, chain_id=cid, allow_stop=True)
    if not o.ram_downdate_fail:
        assert hasattr(r, "chain"), r.stdout[-1500:]
        _agree(r, o, (m, sgn))
        return
    assert m > 0                                                # (the centre chain updates at every iteration: alpha = 1 is above the target)
    assert r.stopped and not hasattr(r, "chain"), "the reference goes on where the oracle's downdate fails"
    # ... in choldowndate and nowhere else (not a crash of another kind, which leaves no chain file either)
    assert "error in coldowndate" in r.stdout and "STOP" in r.stdout, r.stdout[-1500:]
    # ... at the oracle's iteration: the oracle run the reference's way stops there too, having drawn as many uniforms.  (A chain whose first
    # proposal leaves the box downdates with alpha12 still 0 and dchdd refuses: every flagged chain of a box stops at iteration 2, so there is no
    # prefix to compare -- a stop further on fails here and asks for that comparison)
    k = int(o.ram_downdate_fail)
    s = oracle.run_chain(cfg, prob, chain_id=cid)
    assert k == 2 and s.rc == -3000 and s.simuind == k and s.rng_n == r.rng_n, (k, s.rc, s.simuind, s.rng_n, r.rng_n)


@pytest.mark.parametrize("prob", ax.PROBLEMS, ids=["box%d_a%d%s" % (p[0], p[1], "".join("_%s%s" % kv for kv in p[2])) for p in ax.PROBLEMS])
def test_regime_of_every_gpu_problem_from_the_oracle_alone(oracle, prob):
    o = ax.oracle_all(oracle, prob)
    ax.regime(oracle, prob, o)
    X, m = o["X"], o["m"]
    d = prob[0]
    # the layout is box_problems.starts': the wall counts, the signs by groups of eight, the two whole tiles
    assert X.shape == (ax.NCH, d) and (m[192:256] == 0).all() and (m[256:320] == d).all()
    assert tuple(m[:8]) == (0, d, 1, min(d, 6), 0, d, 3, min(d, 8)) and tuple(m[576:583]) == (0, d, 1, min(d, 6), 0, d, 3)
    assert all(((X[c] != 0.0).sum() == m[c]) and (X[c, :m[c]] == (bx.EDGE if (c // 8) % 2 == 0 else -bx.EDGE)).all() for c in range(ax.NCH))
    assert (np.abs(X) < 1.0).all()
    # ss1 is zero on every chain, of either sign over the chains: an edge of its own for a bit comparison
    ss1 = o["scal"][:, 0]
    assert (ss1 == 0.0).all() and np.signbit(ss1).any() and not np.signbit(ss1).all()
