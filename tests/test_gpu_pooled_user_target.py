"""Pooled adaptation (cfg.pooled = 1) for the USER's target: a target module (mcmcx_set_target_module) or host callbacks between the
engine's phase launches, every chain proposing from the one shared factor.

1. anchor: a module that restates the built-in banana target, run with pooled = 1, equals the built-in banana target with pooled = 1 (itself
   pinned to a numpy restatement in test_gpu_pooled.py) bit for bit -- in the lane form ("pooled_phase_kernel": the shared tables through
   the scalar cache) and in the matrix-core form ("pooled_phase_mfma_kernel"), so the two forms equal each other too; SCAM runs the per-chain
   phases on every chain's copy of the shared rotation ("host_phase_kernel<pooled scam>");
2. module == host callbacks == batched host callbacks in pooled mode (the configurations of test_gpu_user_module.py, nycol = 2 included);
3. two shards with the exchange hook == one engine;
4. random configurations, module against host callbacks;
5. no per-chain factor is allocated;
6. what is still refused says so."""
import ctypes as C
import os
import subprocess
import threading

import numpy as np
import pytest

from test_gpu_user_module import USER_SRC, CONFIGS, built  # noqa: F401  (built: the fixture that compiles USER_SRC both ways)

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
THIN = os.environ.get("MCMCX_THIN") == "1"

LANE, MFMA, SCAM = "pooled_phase_kernel", "pooled_phase_mfma_kernel", "host_phase_kernel<pooled scam>"

# oracle/mcx_targets.h: mcxt_ss_banana, operation for operation (two fma and a chain of fma); no prior, no bounds
BANANA_SRC = r"""
#include "mcmcx_target.h"
__device__ void banana_ss(const double *th, int npar, int ny, const void *data, double *ss)
{
    const double b = ((const double *)data)[0];
    double t1 = th[0] * th[0];
    double q = fma(b, t1, th[1]) - 100.0 * b;
    double s = fma(q, q, t1 / 100.0);
    for (int k = 2; k < npar; ++k) s = fma(th[k], th[k], s);
    ss[0] = s;
}
__device__ double banana_prior(const double *th, int npar, const void *data) { return 0.0; }
__device__ int banana_bounds(const double *th, int npar, const void *data) { return 1; }
MCMCX_DEFINE_TARGET(banana_target, banana_ss, banana_prior, banana_bounds)
"""


@pytest.fixture(scope="module")
def banana_module(tmp_path_factory):
    d = tmp_path_factory.mktemp("bananamod")
    src = d / "banana_target.hip"
    src.write_text(BANANA_SRC)
    hsaco = d / "banana_target.hsaco"
    subprocess.check_call(["/opt/rocm/bin/hipcc", "--genco", "--offload-arch=gfx950", "-O2", "-ffp-contract=off",
                           "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(hsaco)])
    return str(hsaco)


def _state(e, nch):
    cm, mean, w, R = e.pooled()
    return dict(theta=e.theta(), masks=e.accept_masks(), scal=e.scalars(), rng=[e.rng(c) for c in sorted({0, nch // 2, nch - 1})],
                cov=cm, mean=mean, W=w, R=R, totals=e.totals())


def _same(a, b, nch, what):
    """Bit for bit; the unused lanes of a ragged last tile never see a user callback and are masked out of the accept record."""
    for k in ("theta", "scal", "cov", "mean", "R"):
        assert np.array_equal(a[k].view(np.uint64), b[k].view(np.uint64)), (what, k)
    assert a["W"] == b["W"] and a["rng"] == b["rng"], (what, "W / rng")
    ma, mb = a["masks"].copy(), b["masks"].copy()
    if nch % 64:
        last = np.uint64((1 << (nch % 64)) - 1)
        ma[:, -1] &= last; mb[:, -1] &= last
    assert np.array_equal(ma, mb), (what, "accept masks")
    for k in ("stayed", "draccepted", "drtries", "proposals", "status"):
        assert a["totals"][k] == b["totals"][k], (what, k)


def _banana_problem(d, seed):
    rng = np.random.default_rng(seed)
    A = rng.standard_normal((d, d)) * 0.05
    cm = 0.02 * np.eye(d) + A @ A.T * 0.02
    return dict(kind="banana", npar=d, par0=np.concatenate([[0.5, 9.0], np.zeros(d - 2)]) if d > 2 else np.array([0.5, 9.0]),
                cmat0=0.5 * (cm + cm.T), b=0.1, sigma2=1.3, nobs=12)


ANCHOR = [
    # method, configuration, npar, chains, iterations
    ("dram", dict(adaptint=40), 5, 70, 130),
    ("dram", dict(adaptint=40), 20, 130, 130),
    ("dram", dict(adaptint=40, condmax=1.0e6), 20, 70, 130),
    ("dram", dict(adaptint=40), 50, 130, 130),
    ("dram", dict(adaptint=40), 64, 70, 130),
    ("dram", dict(adaptint=30), 20, 70000, 65),                       # 1094 tiles: more than one wave per SIMD of the chip, ragged
    ("dram", dict(adaptint=30, drscale=2.0, doburnin=1, burnintime=40, scalelimit=0.3), 5, 130, 130),
    ("dram", dict(adaptint=30, drscale=3.0, doburnin=1, burnintime=40, scalelimit=0.3), 20, 70, 130),
    ("dram", dict(adaptint=40, drscale=2.0, condmax=1.0e6), 50, 70, 130),
    ("dram", dict(adaptint=40, drscale=2.0), 64, 130, 130),
    ("er", dict(adaptint=40), 20, 130, 130),
    ("er", dict(adaptint=40, condmax=1.0e6), 50, 70, 130),
    ("ram", dict(adaptint=7), 5, 70, 130),
    ("ram", dict(adaptint=7, condmax=1.0e6), 20, 130, 130),
    ("ram", dict(adaptint=5), 50, 70, 130),
    ("ram", dict(adaptint=7), 64, 130, 131),
    ("scam", dict(adaptint=20), 5, 70, 70),
    ("scam", dict(adaptint=20), 20, 130, 50),
    ("scam", dict(adaptint=10), 50, 70, 25),
    ("scam", dict(adaptint=10), 64, 130, 25),
    # mcmcx_config::scam_fast through host_phase_kernel<5>'s proposal (the built-in side is tied to the oracle's restatement of the fast form
    # by test_gpu_pooled.py::test_pooled_scam_matches_restatement[banana-fast])
    ("scam", dict(adaptint=20, scam_fast=1), 20, 130, 50),
]


@pytest.mark.parametrize("ci", range(len(ANCHOR)))
def test_banana_module_equals_builtin_banana_in_pooled_mode(banana_module, monkeypatch, ci):
    from mcmcf90_amd import engine_from_problem, make_config, Engine
    method, kw, d, nch, nsimu = ANCHOR[ci]
    pkw = _banana_problem(d, ci)
    ckw = dict(nsimu=nsimu, method=method, updatesigma=1, **kw)
    monkeypatch.delenv("MCMCX_POOLED_PHASE_MFMA", raising=False)
    e = engine_from_problem(ckw, pkw, nchains=nch, pooled=1, record_accept=1, chain_id0=3)
    e.init(); e.run()
    ref = _state(e, nch)
    assert e.last_kernel() not in (LANE, MFMA, SCAM, ""), e.last_kernel()   # one of the single-launch pooled kernels
    e.close()
    # not vacuous: something was accepted and something rejected (SCAM: an iteration stays only when all its components do)
    assert ref["masks"].any() and (ref["totals"]["stayed"] > 0 or method == "scam")
    for form in (("scam",) if method == "scam" else ("0", "1")):
        if form != "scam":
            monkeypatch.setenv("MCMCX_POOLED_PHASE_MFMA", form)
        e = Engine(make_config(d, nch, pooled=1, record_accept=1, chain_id0=3, **ckw))
        e.setpar0(pkw["par0"]); e.setcmat0(pkw["cmat0"]); e.setsigma2nobs(pkw["sigma2"], pkw["nobs"])
        e.set_target_module(banana_module, "banana_target", np.array([pkw["b"]]))
        e.init(); e.run()
        assert e.last_kernel() == {"0": "pooled_phase_kernel", "1": "pooled_phase_mfma_kernel", "scam": "host_phase_kernel<pooled scam>"}[form], \
            e.last_kernel()
        got = _state(e, nch)
        e.close()
        _same(ref, got, nch, (method, d, nch, form))


def test_the_plan_takes_the_measured_form_by_itself(banana_module, monkeypatch):
    """Without the switch plan_kernels decides (mcx_host_launch.hpp: pooled_phase_mfma, the crossover of tools/pooled_phase_sweep.py)."""
    from mcmcf90_amd import make_config, Engine
    monkeypatch.delenv("MCMCX_POOLED_PHASE_MFMA", raising=False)
    for d, want in ((5, LANE), (50, MFMA)):
        pkw = _banana_problem(d, 1)
        e = Engine(make_config(d, 128, pooled=1, nsimu=20, adaptint=10))
        e.setpar0(pkw["par0"]); e.setcmat0(pkw["cmat0"])
        e.set_target_module(banana_module, "banana_target", np.array([0.1]))
        e.init(); e.run()
        assert e.last_kernel() == want, (d, e.last_kernel())
        e.close()


def _host_targets(e, H, batch):
    from mcmcf90_amd import _lib
    keep = (C.cast(H.host_ss, _lib.SSFUN_T), C.cast(H.host_prior, _lib.PRIORFUN_T), C.cast(H.host_bounds, _lib.CHECKBOUNDS_T),
            C.cast(H.host_ss_batch, _lib.SSFUN_BATCH_T))
    if batch:
        assert e.L.mcmcx_set_target_host_batch(e.h, keep[3], keep[1], keep[2], None, 3) == 0
    else:
        assert e.L.mcmcx_set_target_host(e.h, keep[0], keep[1], keep[2], None) == 0
    e._keep_cb = keep


@pytest.mark.parametrize("ci", range(len(CONFIGS)))
def test_module_equals_host_equals_host_batch_in_pooled_mode(built, monkeypatch, ci):
    from mcmcf90_amd import Engine, make_config
    hsaco, H = built
    kw = dict(CONFIGS[ci])
    ny = kw.pop("ny", 1)
    npar, nch = 5, 70
    nsimu = 60 if kw["method"] == "scam" else 150
    if kw["method"] == "ram":
        kw["adaptint"] = 9
    rng = np.random.default_rng(ci)
    data = np.concatenate([rng.uniform(0.5, 2.0, npar), [0.3]])
    H.set_data(data.ctypes.data_as(C.c_void_p))
    monkeypatch.setenv("MCMCX_POOLED_PHASE_MFMA", "1")                 # the module on the matrix cores, the host paths in the lane form

    def engine():
        e = Engine(make_config(npar, nch, nsimu=nsimu, updatesigma=1, record_accept=1, chain_id0=11, pooled=1, **kw))
        e.setpar0(np.full(npar, 0.1)); e.setcmat0(0.05 * np.eye(npar))
        e.setsigma2nobs(np.full(ny, 0.8), np.full(ny, 15))
        return e

    runs = {}
    e = engine(); e.set_target_module(hsaco, "user_target", data); e.init(); e.run()
    assert e.last_kernel() == ("host_phase_kernel<pooled scam>" if kw["method"] == "scam" else "pooled_phase_mfma_kernel"), e.last_kernel()
    runs["module"] = _state(e, nch); e.close()
    monkeypatch.setenv("MCMCX_POOLED_PHASE_MFMA", "0")
    for other in ("host", "batch"):
        e = engine(); _host_targets(e, H, other == "batch"); e.init(); e.run()
        assert e.last_kernel() == ("host_phase_kernel<pooled scam>" if kw["method"] == "scam" else "pooled_phase_kernel"), e.last_kernel()
        runs[other] = _state(e, nch); e.close()
        _same(runs["module"], runs[other], nch, (ci, other))
    assert runs["module"]["masks"].any()                               # something was accepted: the comparison is not vacuous


@pytest.mark.parametrize("form", ["0", "1"])
def test_two_shards_with_the_exchange_hook_equal_one_engine(banana_module, monkeypatch, form):
    import torch
    from mcmcf90_amd import make_config, Engine
    monkeypatch.setenv("MCMCX_POOLED_PHASE_MFMA", form)
    d, nsimu = 20, 200
    pkw = _banana_problem(d, 5)

    def engine(n, id0):
        e = Engine(make_config(d, n, pooled=1, nsimu=nsimu, adaptint=40, drscale=2.0 if form == "1" else 0.0, chain_id0=id0, updatesigma=1))
        e.setpar0(pkw["par0"]); e.setcmat0(pkw["cmat0"]); e.setsigma2nobs(1.3, 12)
        e.set_target_module(banana_module, "banana_target", np.array([0.1]))
        return e

    one = engine(256, 0); one.init(); one.run()
    assert one.last_kernel() == {"0": LANE, "1": MFMA}[form]
    ref_theta = one.theta(); ref = one.pooled(); one.close()
    mlen = 1 + d + d * (d + 1) // 2
    bufs = [torch.zeros(mlen, dtype=torch.float64, device="cuda") for _ in range(2)]
    engs = [engine(128, 128 * r) for r in range(2)]
    barrier = threading.Barrier(2)

    def make_hook(r):
        def hook():
            torch.cuda.synchronize()
            barrier.wait()
            if r == 0:
                tot = bufs[0] + bufs[1]
                bufs[0].copy_(tot); bufs[1].copy_(tot)
                torch.cuda.synchronize()
            barrier.wait()
        return hook

    errs = []

    def rank(r):
        try:
            engs[r].set_exchange(make_hook(r), bufs[r].data_ptr())
            engs[r].init(); engs[r].run()
        except Exception as ex:          # noqa: BLE001
            errs.append(ex)
            barrier.abort()

    ts = [threading.Thread(target=rank, args=(r,)) for r in range(2)]
    for t in ts:
        t.start()
    for t in ts:
        t.join(120)
    assert not errs, errs
    th = np.vstack([e.theta() for e in engs])
    assert np.array_equal(th.view(np.uint64), ref_theta.view(np.uint64))
    for e in engs:
        got = e.pooled()
        for a, b in zip(ref, got):
            assert np.array_equal(np.asarray(a), np.asarray(b))
        e.close()


def test_random_configurations_module_against_host_callbacks(built, monkeypatch):
    from mcmcf90_amd import Engine, make_config, McmcError
    hsaco, H = built
    gen = np.random.default_rng(20260817)
    ndraws = 20 if THIN else 40
    skipped, ran = 0, 0
    for draw in range(ndraws):
        method = ["dram", "dram", "ram", "er", "scam"][int(gen.integers(0, 5))]
        npar = int(gen.integers(2, 65))
        ny = int(gen.integers(1, 4))
        nch = int(gen.integers(2, 200))
        kw = dict(method=method, adaptint=int(gen.integers(5, 40)), updatesigma=int(gen.integers(0, 2)))
        if method == "dram":
            kw["drscale"] = float([0.0, 2.0, 3.0][int(gen.integers(0, 3))])
            if gen.integers(0, 2):
                kw.update(doburnin=1, burnintime=int(gen.integers(10, 50)), scalelimit=0.3)
        if method != "scam" and gen.integers(0, 3) == 0:
            kw["condmax"] = 1.0e8
        nsimu = int(gen.integers(12, 30)) if method == "scam" else int(gen.integers(60, 140))     # (SCAM: npar evaluations per iteration)
        if method == "scam":
            kw["adaptint"] = int(gen.integers(4, 10))
        form = ["0", "1"][int(gen.integers(0, 2))]
        data = np.concatenate([gen.uniform(0.5, 2.0, npar), [0.3]])
        H.set_data(data.ctypes.data_as(C.c_void_p))
        A = gen.standard_normal((npar, npar)) * 0.03
        cmat0 = 0.03 * np.eye(npar) + A @ A.T                          # well conditioned: the initial covariance always factors

        def engine():
            e = Engine(make_config(npar, nch, nsimu=nsimu, record_accept=1, chain_id0=int(draw), pooled=1, **kw))
            e.setpar0(np.full(npar, 0.1)); e.setcmat0(0.5 * (cmat0 + cmat0.T))
            e.setsigma2nobs(np.full(ny, 0.8), np.full(ny, 15))
            return e

        monkeypatch.setenv("MCMCX_POOLED_PHASE_MFMA", form)
        e = engine(); e.set_target_module(hsaco, "user_target", data)
        try:
            e.init()
        except McmcError as ex:
            assert "could not factor the initial covariance" in str(ex), ex     # -32, the one documented refusal a draw may meet
            skipped += 1; e.close()
            continue
        e.run()
        assert e.last_kernel() == (SCAM if method == "scam" else MFMA if form == "1" else LANE), e.last_kernel()
        a = _state(e, nch); e.close()
        monkeypatch.setenv("MCMCX_POOLED_PHASE_MFMA", "0")
        e = engine(); _host_targets(e, H, bool(draw & 1)); e.init(); e.run()
        b = _state(e, nch); e.close()
        _same(a, b, nch, (draw, method, npar, ny, nch, kw, form))
        ran += 1
    assert skipped * 10 <= ndraws, (skipped, ndraws)


def test_a_pooled_module_engine_allocates_no_per_chain_factor(banana_module):
    """npar 50, 262 144 chains, method = 'ram': the per-chain engine holds a packed triangle per chain (1275 doubles), the pooled one none.
    Device memory in use after init, by difference (hipMemGetInfo through torch)."""
    import torch
    from mcmcf90_amd import make_config, Engine
    d, n = 50, 262144
    pkw = _banana_problem(d, 2)
    used = {}
    for pooled in (1, 0):
        torch.cuda.synchronize()
        free0, _ = torch.cuda.mem_get_info()
        e = Engine(make_config(d, n, pooled=pooled, nsimu=10, method="ram", adaptint=5))
        e.setpar0(pkw["par0"]); e.setcmat0(pkw["cmat0"])
        e.set_target_module(banana_module, "banana_target", np.array([0.1]))
        e.init()
        free1, _ = torch.cuda.mem_get_info()
        used[pooled] = free0 - free1
        if pooled:
            e.run()
            assert e.last_kernel() == "pooled_phase_mfma_kernel"
        e.close()
    triangles = n * (d * (d + 1) // 2) * 8
    print("device memory after init: pooled %.3f GB, per chain %.3f GB, triangles %.3f GB" % (used[1] / 1e9, used[0] / 1e9, triangles / 1e9))
    assert used[0] - used[1] >= triangles, (used, triangles)


def test_what_is_still_refused_says_so():
    from mcmcf90_amd import make_config, Engine, McmcError, engine_from_problem
    e = Engine(make_config(4, 64, pooled=1, nsimu=10))
    e.setpar0(np.zeros(4)); e.set_target_external()
    with pytest.raises(McmcError, match="mcmcx_set_target_external: not in pooled mode"):
        e.init()
    e.close()
    x = np.linspace(0.0, 5.0, 12)
    for ny, msg in ((1, "pooled mode with method = 'scam': not on the device-resident response-column target"),
                    (2, "nycol > 1 in pooled mode: not with method = 'scam'")):
        y = np.stack([2.0 * np.exp(-0.5 * (j + 1) * x) for j in range(ny)])
        pkw = dict(kind="expdata", npar=1 + ny, par0=np.full(1 + ny, 1.0), cmat0=0.01 * np.eye(1 + ny), xdata=x, ydata=y,
                   sigma2=np.full(ny, 1.0), nobs=np.full(ny, 12))
        e = engine_from_problem(dict(nsimu=10, method="scam"), pkw, nchains=64, pooled=1)
        with pytest.raises(McmcError, match=msg):
            e.init()
        e.close()
    # host callbacks run on the calling thread, one engine after the other: several ranks of ONE process would wait for each other in
    # the first tick, so mcmcx_run_all refuses them before anything runs (two ranks of the host transport on the one GPU)
    import ctypes as C
    import uuid
    from mcmcf90_amd.engine import Comm
    key, comms, errs = "t" + uuid.uuid4().hex[:12], [None, None], []

    def make_comm(r):
        try:
            comms[r] = Comm(key, r, 2, 0, backend="host")
        except Exception as ex:          # noqa: BLE001
            errs.append(ex)

    ts = [threading.Thread(target=make_comm, args=(r,)) for r in range(2)]
    for t in ts:
        t.start()
    for t in ts:
        t.join(60)
    assert not errs and all(comms), errs
    engs = []
    for r in range(2):
        e = Engine(make_config(3, 64, pooled=1, nsimu=30, adaptint=10, chain_id0=64 * r))
        e.set_comm(comms[r]); e.setpar0(np.zeros(3)); e.set_target_host(lambda th: float(th @ th))
        e.init()
        engs.append(e)
    hs = (C.c_void_p * 2)(engs[0].h, engs[1].h)
    rc = engs[0].L.mcmcx_run_all(hs, 2, 30)
    assert rc == -8 and "one process per GPU" in engs[0].L.mcmcx_last_error().decode(), (rc, engs[0].L.mcmcx_last_error())
    assert engs[0].simuind == 1 and engs[1].simuind == 1               # nothing ran
    for e in engs:
        e.close()
    for c in comms:
        c.close()
    e = Engine(make_config(3, 1, pooled=1, nsimu=10))                  # one chain has no pooled covariance
    e.setpar0(np.zeros(3)); e.set_target_host(lambda th: float(th @ th))
    with pytest.raises(McmcError, match="at least 2 chains"):
        e.init()
    e.close()
