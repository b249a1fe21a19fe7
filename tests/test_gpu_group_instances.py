"""Every compiled instance of group_step_kernel<GW, D4, DRM, TK> (mcmcf90_amd/csrc/mcx_group.hpp) at both ends of its npar range, every chain
against the oracle, bit for bit.

The kernel's register arrays, static LDS and __launch_bounds__ are sized by its template parameters; its matrix-vector chains are hand-written DPP
blocks of 4, 8, 12 or 16 terms, the last one of D4 mod 16; with delayed rejection and D4 % GW != 0 the partly filled last slot of R lives in LDS and is
read back with immediate offsets; positions npar .. D4 - 1 are padding that has to stay zero through every chain.  mcmcx_last_kernel names one of six
GROUP_TABLE entries, each of which stands for four to twenty-five instances (launch_group_d4 / launch_group_inst, mcx_host_launch.hpp), and the other
group tests run a handful of sizes.  Here INSTANCES is the compiled set as a literal table -- tests/test_cabi_exports.py holds it to the kernel symbols
of the shipped code object, so a newly instantiated size fails until it has cases -- and each instance runs at hi = D4 (no padding) and at lo = the
first npar that rounds up to D4 (a pad of three, or seven above 32), asserting after every cut both the table name and the instance(s)
mcmcx_debug_last_instance reports: a moved planner threshold fails there.

A case is 135 chains from chain_id0 = 6 (two full tiles and seven chains: a ragged tile, a sixteen-lane wave that ends with three chains, a quad wave
with seven), nsimu = 110 with adaptint = 50, cut as run(50), run(51), run(): the factors are refilled into registers and LDS after each tick, and one
launch starts right behind a tick.  The comparison is tests/test_gpu_every_chain.py's (_run_and_compare): accept sequence, state, ss1 / sspri1 / sigma2 /
alpha12, stream position, the five counters, R, with delayed rejection R2 and iC, the covariance, the mean and the weight sum, on every chain.  No
tolerance anywhere.  The problems are that file's constructions as they stand (its bounds at npar 9, 17, 20, 32, 33 and 49 included), with mu = 0 at
npar 1; the oracle runs a problem's 135 chains once, and both group widths share them.  The regime is asserted from the oracle's chains alone before
the engine is created (_regime).

The general delayed-rejection form (DRM = 1) is one instance for all targets (TK = -1, "any"): it runs with the Gaussian and with the banana target.
The power-of-two form (DRM = 2) queues the general one behind it, which returns at once unless a factor left the exact range: both are named.

The expdata instances run at npar 2 only: mcmcx_set_target_expdata refuses any other npar ("expdata target needs npar = 2"), so the extra parameters
that tests/test_gpu_group.py::_problem can build never reach the engine, and npar 2 is both edges of what these instances can be given."""
import numpy as np
import pytest

import test_gpu_every_chain as ec
import test_gpu_group as tg

NCH, CHAIN_ID0 = 135, 6
CKW = dict(nsimu=110, method="dram", adaptint=50, updatesigma=0)
CUTS = (50, 51, None)
DR_GENERAL, DR_POW2 = 3.0, 2.0                                  # drscale of the general form and of the power-of-two form (npar <= 24)

# (GW, D4, DRM, TK, lo npar, hi npar): the instances launch_group_d4 can reach.  lo = D4 - 3 up to 32 and D4 - 7 above; at D4 = 4 the Gaussian
# target (and "any", which runs it) starts at npar 1, banana at 2 (its first two parameters are the banana); expdata has exactly two parameters
INSTANCES = (
    # ---- sixteen lanes per chain, no delayed rejection
    (16, 4, 0, "gauss", 1, 4), (16, 8, 0, "gauss", 5, 8), (16, 12, 0, "gauss", 9, 12), (16, 16, 0, "gauss", 13, 16),
    (16, 20, 0, "gauss", 17, 20), (16, 24, 0, "gauss", 21, 24), (16, 28, 0, "gauss", 25, 28), (16, 32, 0, "gauss", 29, 32),
    (16, 40, 0, "gauss", 33, 40), (16, 48, 0, "gauss", 41, 48), (16, 56, 0, "gauss", 49, 56), (16, 64, 0, "gauss", 57, 64),
    (16, 4, 0, "banana", 2, 4), (16, 8, 0, "banana", 5, 8), (16, 12, 0, "banana", 9, 12), (16, 16, 0, "banana", 13, 16),
    (16, 20, 0, "banana", 17, 20), (16, 24, 0, "banana", 21, 24), (16, 28, 0, "banana", 25, 28), (16, 32, 0, "banana", 29, 32),
    (16, 40, 0, "banana", 33, 40), (16, 48, 0, "banana", 41, 48), (16, 56, 0, "banana", 49, 56), (16, 64, 0, "banana", 57, 64),
    (16, 4, 0, "expdata", 2, 2),
    # ---- sixteen lanes, the general delayed-rejection form
    (16, 4, 1, "any", 1, 4), (16, 8, 1, "any", 5, 8), (16, 12, 1, "any", 9, 12), (16, 16, 1, "any", 13, 16),
    (16, 20, 1, "any", 17, 20), (16, 24, 1, "any", 21, 24), (16, 28, 1, "any", 25, 28), (16, 32, 1, "any", 29, 32),
    # ---- sixteen lanes, drscale a power of two
    (16, 4, 2, "gauss", 1, 4), (16, 8, 2, "gauss", 5, 8), (16, 12, 2, "gauss", 9, 12), (16, 16, 2, "gauss", 13, 16),
    (16, 20, 2, "gauss", 17, 20), (16, 24, 2, "gauss", 21, 24),
    (16, 4, 2, "banana", 2, 4), (16, 8, 2, "banana", 5, 8), (16, 12, 2, "banana", 9, 12), (16, 16, 2, "banana", 13, 16),
    (16, 20, 2, "banana", 17, 20), (16, 24, 2, "banana", 21, 24),
    (16, 4, 2, "expdata", 2, 2),
    # ---- quads
    (4, 4, 0, "gauss", 1, 4), (4, 8, 0, "gauss", 5, 8), (4, 12, 0, "gauss", 9, 12), (4, 16, 0, "gauss", 13, 16),
    (4, 4, 0, "banana", 2, 4), (4, 8, 0, "banana", 5, 8), (4, 12, 0, "banana", 9, 12), (4, 16, 0, "banana", 13, 16),
    (4, 4, 0, "expdata", 2, 2),
    (4, 4, 1, "any", 1, 4), (4, 8, 1, "any", 5, 8), (4, 12, 1, "any", 9, 12), (4, 16, 1, "any", 13, 16),
    (4, 4, 2, "gauss", 1, 4), (4, 8, 2, "gauss", 5, 8), (4, 12, 2, "gauss", 9, 12), (4, 16, 2, "gauss", 13, 16),
    (4, 4, 2, "banana", 2, 4), (4, 8, 2, "banana", 5, 8), (4, 12, 2, "banana", 9, 12), (4, 16, 2, "banana", 13, 16),
    (4, 4, 2, "expdata", 2, 2),
)
TK_CODE = {"gauss": 0, "banana": 1, "expdata": 2, "any": -1}  # the kernel's integer template argument (TGT_GAUSS ..; -1: read at run time)
TABLE_NAME = {(16, 0): "group_step_kernel", (16, 1): "group_step_kernel<DR>", (16, 2): "group_step_kernel<DR2>",
              (4, 0): "group_step_kernel<quad>", (4, 1): "group_step_kernel<quad, DR>", (4, 2): "group_step_kernel<quad, DR2>"}
# cmat0 = EXPDATA_CMAT0 * I for the expdata problem, chosen with the oracle alone so that every one of the 135 chains accepts and rejects:
# tests/test_gpu_group.py::_problem's own 0.01 does -- a first-stage rate of 0.643 without delayed rejection and 0.649 with drscale 2 (2921 second
# stages accepted, 2248 rejected), no chain without an accept and none without a rejection
EXPDATA_CMAT0 = 0.01


def compiled_set():
    """{(GW, D4, DRM, TK as the template's integer)}: what tests/test_cabi_exports.py compares with the code object's kernel symbols"""
    return {(gw, d4, drm, TK_CODE[tk]) for gw, d4, drm, tk, _, _ in INSTANCES}


def test_instance_table_covers_every_instance_at_both_edges():
    """The literal table itself (no device): every row's range is the whole range of npar that rounds up to its D4, with the exceptions the
    targets make at D4 = 4; no row twice; the delayed-rejection forms end where the launch switch ends them."""
    assert len(set(r[:4] for r in INSTANCES)) == len(INSTANCES) == len(compiled_set())
    for gw, d4, drm, tk, lo, hi in INSTANCES:
        assert gw in (4, 16) and drm in (0, 1, 2) and tk in TK_CODE and (tk == "any") == (drm == 1), (gw, d4, drm, tk)
        assert d4 % (4 if d4 <= 32 else 8) == 0 and 4 <= d4 <= (16 if gw == 4 else (64, 32, 24)[drm]), (gw, d4, drm, tk)
        if tk == "expdata":
            assert (d4, lo, hi) == (4, 2, 2)
            continue
        assert hi == d4, (gw, d4, drm, tk)
        want = d4 - 3 if d4 <= 32 else d4 - 7
        if d4 == 4 and tk == "banana":
            want = 2
        assert lo == want, (gw, d4, drm, tk, lo)
    # ... and a case exists for both ends of every row, the run-time-target form with both targets
    ran = {}
    for p in CASES:
        row, kind, d = p.values[0], p.values[1], p.values[2]
        ran.setdefault(row, set()).add((kind, d))
    for row in INSTANCES:
        gw, d4, drm, tk, lo, hi = row
        kinds = ("gauss", "banana") if tk == "any" else (tk,)
        assert ran.get(row) == {(k, max(lo, 2) if (k == "banana" and e == lo) else e) for k in kinds for e in (lo, hi)}, row


def test_last_instance_refuses_a_null_handle_or_buffer():
    """mcmcx_debug_last_instance without a device: a null h or buf is refused with -57 and nothing is written."""
    import ctypes as C
    from mcmcf90_amd import _lib
    L = _lib.load()
    buf = C.create_string_buffer(b"untouched", 64)
    assert L.mcmcx_debug_last_instance(None, buf, 64) == -57 and b"null argument" in L.mcmcx_last_error() and buf.value == b"untouched"
    assert L.mcmcx_debug_last_instance(None, None, 0) == -57


@pytest.mark.gpu
def test_last_instance_outside_the_group_step_kernels(monkeypatch):
    """Every entry that is one kernel reports its table name unchanged ("" before the first run); group_ram_kernel names its size; a len that does
    not hold the name and its terminator is refused with -57, the buffer untouched."""
    import ctypes as C
    from mcmcf90_amd import engine_from_problem
    for k in ec.SWITCHES:
        monkeypatch.delenv(k, raising=False)
    _, pkw = _problem(_prob("gauss", 17, 0.0))
    for env, method, kernel, inst in ((dict(MCMCX_GROUP="0"), "dram", ec.LDSV, ec.LDSV), (dict(MCMCX_RAM_GROUP="1"), "ram", "group_ram_kernel", "group_ram_kernel<32>")):
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        e = engine_from_problem(dict(CKW, method=method, nsimu=20), pkw, nchains=70, chain_id0=CHAIN_ID0)
        e.init()
        assert e.last_instance() == e.last_kernel() == ""
        e.run()
        assert (e.last_kernel(), e.last_instance()) == (kernel, inst)
        buf = C.create_string_buffer(b"untouched", 64)
        for n in (0, len(inst)):
            assert e.L.mcmcx_debug_last_instance(e.h, buf, n) == -57 and b"len too small" in e.L.mcmcx_last_error() and buf.value == b"untouched"
        assert e.L.mcmcx_debug_last_instance(e.h, buf, len(inst) + 1) == 0 and buf.value.decode() == inst
        e.close()


def _prob(kind, d, drscale):
    """The key of a problem (and of the oracle's cache): both group widths, and the instances that share a target and a size, share it."""
    return (kind, d, drscale)


def _problem(prob):
    """(cfg keywords, problem keywords).  Gaussian and banana: tests/test_gpu_every_chain.py::_problem as it stands -- par0 = 0.1, cmat0 = inv(lam),
    rng(3000 + d), bounds at that file's BOUNDED sizes without delayed rejection; par0 = 0.05, cmat0 = (2 / d) I, b = 0.1 -- with mu = 0 at npar 1
    (linspace(-0.5, 0.5, 1) puts the single mean at -0.5).  Expdata: tests/test_gpu_group.py::_problem(seed 42) with cmat0 = EXPDATA_CMAT0 I."""
    kind, d, drscale = prob
    ckw = dict(CKW, drscale=drscale)
    if kind == "expdata":
        pkw = tg._problem("expdata", 2, 42)
        pkw["cmat0"] = EXPDATA_CMAT0 * np.eye(2)
        return ckw, pkw
    _, pkw, _, _ = ec._problem(ec.P(kind, d, drscale=drscale))
    if kind == "gauss" and d == 1:
        pkw["mu"] = np.zeros(1)
    return ckw, pkw


_ORACLE = {}


def _oracle_all(oracle, prob):
    """A problem's 135 chains through the oracle: once per (target, npar, drscale), never changed (ec._pack makes the arrays read-only)."""
    if prob not in _ORACLE:
        from concurrent.futures import ThreadPoolExecutor
        ckw, pkw = _problem(prob)
        cfg = oracle.make_cfg(**ckw); pr = oracle.Problem(**pkw)
        oracle.lib()
        with ThreadPoolExecutor(8) as pool:
            rs = list(pool.map(lambda c: oracle.run_chain(cfg, pr, chain_id=CHAIN_ID0 + c), range(NCH)))
        _ORACLE[prob] = ec._pack(rs, NCH, int(pkw["npar"]), ckw["nsimu"])
    return _ORACLE[prob]


def _regime(prob, o):
    """What makes the case worth running, from the oracle's chains alone: lanes accept at different iterations (the first-stage rate strictly inside
    0.1 .. 0.5 for the Gaussian target and 0.25 .. 0.9 for banana), every chain accepts at least once and rejects at least once, and with delayed
    rejection more than one second stage per chain is accepted and more than one rejected.  Conditions on the inputs, not tolerances: a size that
    misses one gets another proposal scale.  Returns the first-stage rate."""
    kind, d, drscale = prob
    nsimu = CKW["nsimu"]
    stayed, bnd, drtries, dracc, erstayed = o["ctr"].T
    moves = o["acc"][:, 1:]                                     # (row 0 is the start point)
    rate1 = 1.0 - drtries.sum() / (NCH * (nsimu - 1.0)) if drscale else moves.mean()
    if kind == "gauss":
        assert 0.1 < rate1 < 0.5, (prob, rate1)
    elif kind == "banana":
        assert 0.25 < rate1 < 0.9, (prob, rate1)
    assert moves.any(axis=1).all() and (moves == 0).any(axis=1).all(), (prob, int((~moves.any(axis=1)).sum()), int(moves.all(axis=1).sum()))
    if drscale:
        assert dracc.sum() > NCH and (drtries - dracc).sum() > NCH, (prob, int(dracc.sum()), int((drtries - dracc).sum()))
    return rate1


def _instance_name(gw, d4, drm, tk):
    one = lambda m, t: "group_step_kernel<%d,%d,%d,%s>" % (gw, d4, m, t)
    return one(2, tk) + "+" + one(1, "any") if drm == 2 else one(drm, tk)


def _cases():
    C = []
    for row in INSTANCES:
        gw, d4, drm, tk, lo, hi = row
        for kind in (("gauss", "banana") if tk == "any" else (tk,)):
            for d in sorted({max(lo, 2) if kind == "banana" else lo, hi}):
                C.append(pytest.param(row, kind, d, id="gw%d_d4%d_drm%d_%s-%s%d" % (gw, d4, drm, tk, kind, d)))
    return C


CASES = _cases()
PROBLEMS = sorted({_prob(p.values[1], p.values[2], (0.0, DR_GENERAL, DR_POW2)[p.values[0][2]]) for p in CASES})


@pytest.mark.gpu
@pytest.mark.parametrize("row,kind,d", CASES)
def test_every_chain_of_an_instance_equals_the_oracle(oracle, monkeypatch, row, kind, d):
    from mcmcf90_amd import engine_from_problem
    gw, d4, drm, tk, lo, hi = row
    prob = _prob(kind, d, (0.0, DR_GENERAL, DR_POW2)[drm])
    ckw, pkw = _problem(prob)
    o = _oracle_all(oracle, prob)
    _regime(prob, o)                                            # ... before the engine is touched
    for k in ec.SWITCHES:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("MCMCX_GROUP", "1")
    monkeypatch.setenv("MCMCX_GROUP_GW", str(gw))
    e = engine_from_problem(ckw, pkw, nchains=NCH, chain_id0=CHAIN_ID0, record_accept=1)
    e.init()
    failures = ec._run_and_compare(e, o, ckw, NCH, CUTS, TABLE_NAME[(gw, drm)], instance=_instance_name(gw, d4, drm, tk))
    assert not failures, "; ".join(failures)
