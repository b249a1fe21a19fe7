"""Pooled mode (the multi-chain extension named in BASELINE.json's north_star): all chains propose with ONE
factor, adapted every adaptint iterations from the pooled empirical covariance of the current states.  The
oracle side restates it with the single-chain C oracle (adaptation off, factor replaced from outside) plus the
moment tree / merge / Cholesky written out in Python floats in the engine's operation order: the states,
accept masks and the shared factor must agree bit for bit.  A second test splits the chains over two engines
that exchange their moment vectors through the exchange hook (the RCCL all-reduce of the multi-GPU run)."""
import ctypes as C
import os
import math
import threading
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


_libm = C.CDLL("libm.so.6")
_libm.fma.restype = C.c_double
_libm.fma.argtypes = [C.c_double, C.c_double, C.c_double]


def _fma(a, b, c):
    return _libm.fma(float(a), float(b), float(c))


def _tree(v):
    """Pairwise tree, adjacent partners first (the xor-butterfly inside a tile, then the tile tree)."""
    v = list(v)
    while len(v) > 1:
        v = [v[i] + v[i + 1] if i + 1 < len(v) else v[i] for i in range(0, len(v), 2)]
    return v[0]


def _pooled_moments(theta, par0, nchains):
    n, d = theta.shape
    T = (nchains + 63) // 64
    x = np.zeros((T * 64, d))
    x[:n] = theta - par0
    act = np.zeros(T * 64); act[:n] = 1.0
    cnt = _tree([_tree(act[t * 64:(t + 1) * 64]) for t in range(T)])
    s1 = [_tree([_tree(x[t * 64:(t + 1) * 64, j]) for t in range(T)]) for j in range(d)]
    s2 = {}
    for j in range(d):
        for i in range(j + 1):
            p = x[:, i] * x[:, j]
            s2[(i, j)] = _tree([_tree(p[t * 64:(t + 1) * 64]) for t in range(T)])
    return cnt, s1, s2


def _merge_and_factor(oracle, state, cnt, s1, s2, par0, d, first, cmat0, initcmatn):
    """pooled_adapt of mcx_api.hip in Python floats."""
    if first:
        state["W"] = float(initcmatn); state["C"] = {(i, j): float(cmat0[i, j]) for j in range(d) for i in range(j + 1)}
        state["mean"] = [float(v) for v in par0]
    n = cnt
    m1 = [s1[j] / n for j in range(d)]
    mb = [float(par0[j]) + m1[j] for j in range(d)]
    Cb = {(i, j): (s2[(i, j)] - n * m1[i] * m1[j]) / (n - 1.0) for j in range(d) for i in range(j + 1)}
    if not state["W"] > 0.0:
        state["C"], state["mean"], state["W"] = Cb, mb, n
    else:
        W = state["W"]; Wn = W + n
        dl = [mb[j] - state["mean"][j] for j in range(d)]
        f = W * n / Wn
        state["C"] = {(i, j): ((W - 1.0) * state["C"][(i, j)] + (n - 1.0) * Cb[(i, j)] + f * dl[i] * dl[j]) / (Wn - 1.0)
                      for j in range(d) for i in range(j + 1)}
        g = n / Wn
        state["mean"] = [state["mean"][j] + g * dl[j] for j in range(d)]
        state["W"] = Wn
    A = np.zeros((d, d), order="F")
    for (i, j), v in state["C"].items():
        A[i, j] = v; A[j, i] = v
    info = oracle.lib().mcxo_potrf_u(d, A.ctypes.data_as(C.POINTER(C.c_double)))
    if info == 0:
        sq = math.sqrt(float(d))
        state["R"] = np.array([[A[i, j] * 2.4 / sq if i <= j else 0.0 for j in range(d)] for i in range(d)])
    return state


def _setup(oracle, d, nsimu):
    ckw = dict(nsimu=nsimu, adaptint=100, updatesigma=0)
    S = 0.6 ** np.abs(np.subtract.outer(np.arange(d), np.arange(d)))
    pkw = dict(kind="gauss", npar=d, par0=np.full(d, 0.5), cmat0=0.02 * np.eye(d), mu=np.linspace(-1, 1, d),
               lam=np.linalg.inv(S))
    return ckw, pkw


def test_pooled_mode_matches_restatement(oracle):
    from mcmcf90_amd import engine_from_problem
    d, N, nsimu = 6, 150, 330
    ckw, pkw = _setup(oracle, d, nsimu)
    e = engine_from_problem(ckw, pkw, nchains=N, pooled=1, record_accept=1)
    e.init(); e.run()
    # ---- restatement
    cfg = oracle.make_cfg(**dict(ckw, doadapt=0))
    prob = oracle.Problem(**pkw)
    chains = [oracle.LiveChain(cfg, prob, chain_id=c) for c in range(N)]
    state = {}
    par0, cmat0 = np.asarray(pkw["par0"], float), np.asarray(pkw["cmat0"], float)
    for tick in (100, 200, 300, nsimu):
        for ch in chains:
            ch.run(tick)
        if tick % 100 == 0 and tick < nsimu:
            theta = np.array([ch.theta for ch in chains])
            cnt, s1, s2 = _pooled_moments(theta, par0, N)
            state = _merge_and_factor(oracle, state, cnt, s1, s2, par0, d, tick == 100, cmat0, 0)
            for ch in chains:
                ch.set_R(state["R"])
    theta = np.array([ch.theta for ch in chains])
    np.testing.assert_array_equal(_bits(e.theta()), _bits(theta))
    for c in (0, 63, 64, 149):
        np.testing.assert_array_equal(e.accepted(c), chains[c].accepted)
    cm, mean, W, R = e.pooled()
    assert W == state["W"] == 3 * N
    np.testing.assert_array_equal(_bits(np.triu(R)), _bits(np.triu(state["R"])))
    np.testing.assert_array_equal(_bits(mean), _bits(np.array(state["mean"])))
    for ch in chains:
        ch.close()
    e.close()


def test_pooled_mode_two_shards_with_exchange_hook(oracle):
    """256 chains on one engine == 2 x 128 chains on two engines whose moment vectors are summed by the exchange
    hook (what the RCCL all-reduce does on a multi-GPU node): identical states and identical shared factor."""
    import torch
    from mcmcf90_amd import engine_from_problem
    d, nsimu = 6, 260
    ckw, pkw = _setup(oracle, d, nsimu)
    one = engine_from_problem(ckw, pkw, nchains=256, pooled=1)
    one.init(); one.run()
    ref_theta = one.theta(); _, _, _, ref_R = one.pooled()
    one.close()

    mlen = 1 + d + d * (d + 1) // 2
    bufs = [torch.zeros(mlen, dtype=torch.float64, device="cuda") for _ in range(2)]
    engs = [engine_from_problem(ckw, pkw, nchains=128, chain_id0=128 * r, pooled=1) for r in range(2)]
    barrier = threading.Barrier(2)

    def make_hook(r):
        def hook():                      # the all-reduce: both ranks meet, rank 0 leaves the sum in both buffers
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
            engs[r].init()
            engs[r].run()                # ctypes drops the GIL inside mcmcx_run; the hook re-enters Python
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
    np.testing.assert_array_equal(_bits(th), _bits(ref_theta))
    for e in engs:
        np.testing.assert_array_equal(_bits(np.triu(e.pooled()[3])), _bits(np.triu(ref_R)))
        e.close()


def _scam_factor(oracle, state, d, condmax):
    """host_initial_svd(scam) of mcx_api.hip: pinned Jacobi SVD of the pooled covariance, singular-value floor, sqrt."""
    G = np.zeros((d, d), order="F")
    for (i, j), v in state["C"].items():
        G[i, j] = v; G[j, i] = v
    V = np.zeros((d, d), order="F"); sv = np.zeros(d)
    DP = C.POINTER(C.c_double)
    oracle.lib().mcxo_symsvd(d, G.ctypes.data_as(DP), V.ctypes.data_as(DP), sv.ctypes.data_as(DP))
    if sv[0] == 0.0:
        return state
    tol = sv[0] / condmax
    if sv[d - 1] <= tol:
        sv = np.where(sv < tol, tol, sv)
    state["U"] = np.array(V)                       # U[i, j] = V(i, j)
    state["std"] = np.array([math.sqrt(v) for v in sv])
    return state


@pytest.mark.parametrize("kind,fast", [pytest.param("gauss", 0, id="gauss"), pytest.param("banana", 0, id="banana"),
                                       pytest.param("gauss", 1, id="gauss-fast"), pytest.param("banana", 1, id="banana-fast")])
def test_pooled_scam_matches_restatement(oracle, kind, fast):
    """method='scam' with pooled=1: one rotation U / qcovstd for all chains, re-derived at every tick from the pooled
    covariance (scam_pooled_kernel: four waves per tile, U through the scalar cache).  fast: mcmcx_config::scam_fast against the oracle's
    restatement of it (LiveChain(scam_fast=True): cand = fma(zj, U(:,j), theta)); nothing else in the restatement changes."""
    from mcmcf90_amd import engine_from_problem
    d, N, nsimu = 7, 150, 230
    ckw = dict(nsimu=nsimu, adaptint=100, updatesigma=0, method="scam")
    if kind == "gauss":
        S = 0.6 ** np.abs(np.subtract.outer(np.arange(d), np.arange(d)))
        pkw = dict(kind="gauss", npar=d, par0=np.full(d, 0.5), cmat0=0.02 * np.eye(d), mu=np.linspace(-1, 1, d), lam=np.linalg.inv(S))
    else:
        pkw = dict(kind="banana", npar=d, par0=np.zeros(d), cmat0=0.05 * np.eye(d), b=0.1)
    e = engine_from_problem(ckw, pkw, nchains=N, pooled=1, record_accept=1, scam_fast=fast)
    e.init(); e.run()
    cfg = oracle.make_cfg(**dict(ckw, doadapt=0))
    prob = oracle.Problem(**pkw)
    chains = [oracle.LiveChain(cfg, prob, chain_id=c, scam_fast=bool(fast)) for c in range(N)]
    state = {}
    par0, cmat0 = np.asarray(pkw["par0"], float), np.asarray(pkw["cmat0"], float)
    for tick in (100, 200, nsimu):
        for ch in chains:
            ch.run(tick)
        if tick % 100 == 0 and tick < nsimu:
            theta = np.array([ch.theta for ch in chains])
            cnt, s1, s2 = _pooled_moments(theta, par0, N)
            state = _merge_and_factor(oracle, state, cnt, s1, s2, par0, d, tick == 100, cmat0, 0)
            state = _scam_factor(oracle, state, d, cfg.condmax)
            for ch in chains:
                ch.set_R(state["U"]); ch.set_qcovstd(state["std"])
    theta = np.array([ch.theta for ch in chains])
    np.testing.assert_array_equal(_bits(e.theta()), _bits(theta))
    for c in (0, 63, 64, 149):
        np.testing.assert_array_equal(e.accepted(c), chains[c].accepted)
    cm, mean, W, U = e.pooled()
    assert W == 2 * N
    np.testing.assert_array_equal(_bits(U), _bits(state["U"]))
    np.testing.assert_array_equal(_bits(e.qcovstd(0)), _bits(state["std"]))
    for ch in chains:
        ch.close()
    e.close()


@pytest.mark.parametrize("seed", range(18))
def test_pooled_scam_twelve_wave_layout_equals_the_sixteen_wave_layout(seed, monkeypatch):
    """scam_pooled12_kernel (npar 193..240: twelve block waves of 170 registers, a fifth slot on some of them -- the kernel behind bench.py's
    c5_pooled) against scam_pooled_kernel's sixteen-wave layout of the same configuration (MCMCX_SCAM_POOLED_16=1), which the restatement
    tests tie to the oracle: random npar over the whole range (every count of fifth slots, ragged last blocks), ragged tiles, bounds,
    priors, the sigma2 update, one pooled adaptation -- states, accept ballots, stream positions, the shared rotation, bit for bit.
    (Weak 4: the suite gave this kernel four runs.)"""
    from mcmcf90_amd import engine_from_problem
    r = np.random.default_rng(9100 + seed)
    d = int(r.integers(193, 241))
    N = int(r.choice([64, 70, 130]))
    A = r.standard_normal((d, d)) / np.sqrt(d)
    ckw = dict(nsimu=5, adaptint=3, updatesigma=int(r.integers(0, 2)), method="scam")
    pkw = dict(kind="gauss", npar=d, par0=np.full(d, 0.1), cmat0=0.01 * np.eye(d), mu=np.linspace(-0.5, 0.5, d), lam=A @ A.T + np.diag(np.linspace(0.5, 3.0, d)))
    if ckw["updatesigma"]:
        pkw.update(sigma2=0.7, nobs=30)
    if r.random() < 0.4:
        pkw.update(lo=np.full(d, -0.2), hi=np.full(d, 0.45))
    if r.random() < 0.4:
        pkw.update(pri_mu=np.zeros(d), pri_sig=np.where(np.arange(d) % 3 == 0, 0.0, 0.5))
    res = []
    for sixteen in (False, True):
        if sixteen:
            monkeypatch.setenv("MCMCX_SCAM_POOLED_16", "1")
        else:
            monkeypatch.delenv("MCMCX_SCAM_POOLED_16", raising=False)
        e = engine_from_problem(ckw, pkw, nchains=N, pooled=1, record_accept=1)
        e.init(); e.run()
        assert e.last_kernel() == ("scam_pooled_kernel" if sixteen else "scam_pooled12_kernel"), e.last_kernel()
        res.append((e.theta().copy(), e.accept_masks().copy(), [e.rng(c) for c in (0, N - 1)], e.pooled()[3].copy(), e.scalars().copy()))
        e.close()
    a, b = res
    assert np.array_equal(_bits(a[0]), _bits(b[0])) and np.array_equal(a[1], b[1]) and a[2] == b[2]
    np.testing.assert_array_equal(_bits(a[3]), _bits(b[3]))
    np.testing.assert_array_equal(_bits(a[4]), _bits(b[4]))


def _layout(d, extras, fast=0, extended=False):
    return pytest.param(d, extras, fast, id="%d-%s%s" % (d, extras, "-fast" if fast else ""), marks=[pytest.mark.extended] if extended else [])


@pytest.mark.slow
@pytest.mark.parametrize("d,extras,fast", [_layout(40, "s2"), _layout(64, ""), _layout(70, "bounds"), _layout(100, "priors"), _layout(130, ""), _layout(200, "bounds"),
                                           _layout(215, "", extended=True),
                                           # (230: twelve fifth slots -- 25 s of oracle chains; since round 6 the twelve-wave kernel has eighteen device-side cases over its
                                           #  whole npar range above, and 200 keeps its tie to the oracle in the default suite)
                                           _layout(230, "priors", extended=True), _layout(200, "sixteen", extended=True), _layout(250, "replicated"),
                                           # mcmcx_config::scam_fast on the same splits, against the restatement with the oracle's fast chains: 200 is
                                           # scam_pooled12_kernel, the kernel of bench.py's c5_pooled_fast row; with bounds the candidate makes its round trip
                                           # through global memory; 250 runs the per-chain lane kernels on copies of the one rotation
                                           _layout(40, "", 1), _layout(70, "", 1), _layout(130, "", 1), _layout(200, "", 1), _layout(200, "sixteen", 1, extended=True),
                                           _layout(100, "bounds", 1), _layout(250, "replicated", 1)])
def test_pooled_scam_wave_layouts(oracle, d, extras, fast, monkeypatch):
    """Every split of scam_pooled_kernel's output blocks over its waves: d=40 three leftover blocks and no block wave,
    64 four block waves and nothing left over, 70 / 100 four block waves + one / three leftover blocks, 130 eight + one;
    200 / 215 / 230: scam_pooled12_kernel, twelve block waves with four / eight / twelve fifth slots (the last one on the
    scalar wave, ragged last block), and 200 once more in the sixteen-wave layout; with the sigma2 update, box bounds and
    Gaussian priors (which make theta' round-trip through global memory).  250 (round 5): above npar 240 the tile's LDS vector does not
    fit; the engine copies the one rotation to every chain and runs the per-chain kernels on it (slower, not refused) -- the same chains."""
    if extras == "sixteen":
        monkeypatch.setenv("MCMCX_SCAM_POOLED_16", "1")
    from mcmcf90_amd import engine_from_problem
    N, nsimu, tick = (70, 8, 3) if d <= 240 else (66, 5, 3)
    rng = np.random.default_rng(d)
    A = rng.standard_normal((d, d)) / np.sqrt(d)
    lam = A @ A.T + np.diag(np.linspace(0.5, 3.0, d))
    ckw = dict(nsimu=nsimu, adaptint=tick, updatesigma=1 if extras == "s2" else 0, method="scam")
    pkw = dict(kind="gauss", npar=d, par0=np.full(d, 0.1), cmat0=0.01 * np.eye(d), mu=np.linspace(-0.5, 0.5, d), lam=lam)
    if extras == "s2":
        pkw.update(sigma2=0.7, nobs=30)
    if extras == "bounds":
        pkw.update(lo=np.full(d, -0.2), hi=np.full(d, 0.45))
    if extras == "priors":
        pkw.update(pri_mu=np.zeros(d), pri_sig=np.where(np.arange(d) % 3 == 0, 0.0, 0.5))
    e = engine_from_problem(ckw, pkw, nchains=N, pooled=1, record_accept=1, scam_fast=fast)
    e.init(); e.run()
    assert e.last_kernel() == ("scam_mw_kernel<8>" if d > 240 else "scam_pooled12_kernel" if (d >= 193 and extras != "sixteen") else "scam_pooled_kernel"), e.last_kernel()
    cfg = oracle.make_cfg(**dict(ckw, doadapt=0))
    prob = oracle.Problem(**pkw)
    chains = [oracle.LiveChain(cfg, prob, chain_id=c, scam_fast=bool(fast)) for c in range(N)]
    state = {}
    par0, cmat0 = np.asarray(pkw["par0"], float), np.asarray(pkw["cmat0"], float)
    for t in [t for t in (3, 6) if t < nsimu] + [nsimu]:
        for ch in chains:
            ch.run(t)
        if t < nsimu:
            theta = np.array([ch.theta for ch in chains])
            cnt, s1, s2 = _pooled_moments(theta, par0, N)
            state = _merge_and_factor(oracle, state, cnt, s1, s2, par0, d, t == 3, cmat0, 0)
            state = _scam_factor(oracle, state, d, cfg.condmax)
            for ch in chains:
                ch.set_R(state["U"]); ch.set_qcovstd(state["std"])
    theta = np.array([ch.theta for ch in chains])
    np.testing.assert_array_equal(_bits(e.theta()), _bits(theta))
    for c in (0, 63, 64, N - 1):
        np.testing.assert_array_equal(e.accepted(c), chains[c].accepted)
    if extras == "bounds":
        assert sum(e.counters(c)["bndstayed"] for c in range(N)) > 0
    np.testing.assert_array_equal(_bits(e.pooled()[3]), _bits(state["U"]))
    for ch in chains:
        ch.close()
    e.close()


def _check_pooled_scam_against_restatement(oracle, seed, scam_fast=0):
    """A random pooled SCAM configuration (one rotation for all chains, adapted from the pooled covariance every adaptint iterations) against the
    restatement of test_pooled_scam_wave_layouts: npar 2..64, ragged tiles, condmax floors, bounds, priors, the sigma2 update, a cut run.
    scam_fast: the engine's opt-in proposal against the oracle's fast chains."""
    from mcmcf90_amd import engine_from_problem
    r = np.random.default_rng(95000 + seed)
    d = int(r.choice([2, 3, 5, 8, 13, 16, 17, 24, 33, 40, 48, 64]))
    N = int(r.choice([66, 70, 130]))
    tick = int(r.choice([3, 4, 5]))
    nsimu = tick * int(r.integers(2, 4)) + int(r.integers(1, tick))          # never a multiple of the tick
    ckw = dict(nsimu=nsimu, adaptint=tick, updatesigma=int(r.random() < 0.3), method="scam")
    if r.random() < 0.3:
        ckw["condmax"] = float(r.choice([1e6, 50.0]))
    A = r.standard_normal((d, d)) / np.sqrt(d)
    pkw = dict(kind="gauss", npar=d, par0=np.full(d, 0.1), cmat0=float(r.choice([0.01, 0.3])) * np.eye(d), mu=np.linspace(-0.5, 0.5, d),
               lam=A @ A.T + np.diag(np.linspace(0.5, 3.0, d)))
    if ckw["updatesigma"]: pkw.update(sigma2=0.7, nobs=30)
    if r.random() < 0.3: pkw.update(lo=np.full(d, -0.8), hi=np.full(d, 0.9))
    if r.random() < 0.3: pkw.update(pri_mu=np.zeros(d), pri_sig=np.where(np.arange(d) % 3 == 0, 0.0, 0.5))
    e = engine_from_problem(ckw, pkw, nchains=N, pooled=1, record_accept=1, scam_fast=scam_fast)
    e.init(); e.run(int(r.integers(1, nsimu))); e.run()
    kernel = e.last_kernel()
    cfg = oracle.make_cfg(**dict(ckw, doadapt=0))
    prob = oracle.Problem(**pkw)
    chains = [oracle.LiveChain(cfg, prob, chain_id=c, scam_fast=bool(scam_fast)) for c in range(N)]
    try:
        state = {}
        par0, cmat0 = np.asarray(pkw["par0"], float), np.asarray(pkw["cmat0"], float)
        for t in list(range(tick, nsimu, tick)) + [nsimu]:
            for ch in chains:
                ch.run(t)
            if t < nsimu:
                theta = np.array([ch.theta for ch in chains])
                cnt, s1, s2 = _pooled_moments(theta, par0, N)
                state = _merge_and_factor(oracle, state, cnt, s1, s2, par0, d, t == tick, cmat0, 0)
                state = _scam_factor(oracle, state, d, cfg.condmax)
                for ch in chains:
                    ch.set_R(state["U"]); ch.set_qcovstd(state["std"])
        theta = np.array([ch.theta for ch in chains])
        np.testing.assert_array_equal(_bits(e.theta()), _bits(theta), err_msg=str(ckw))
        for c in (0, 63, 64, N - 1):
            np.testing.assert_array_equal(e.accepted(c), chains[c].accepted, err_msg=str(ckw))
        np.testing.assert_array_equal(_bits(e.pooled()[3]), _bits(state["U"]), err_msg=str(ckw))
    finally:
        for ch in chains:
            ch.close()
        e.close()
    return kernel


@pytest.mark.parametrize("seed", range(24))
def test_random_pooled_scam_configuration_matches_restatement(oracle, seed):
    _check_pooled_scam_against_restatement(oracle, seed)


@pytest.mark.parametrize("seed", range(100, 112))
def test_random_pooled_fast_scam_configuration_matches_restatement(oracle, seed):
    """A seed range of its own with mcmcx_config::scam_fast (the 24 seeds above and their draws stay as they are)."""
    _check_pooled_scam_against_restatement(oracle, seed, scam_fast=1)


@pytest.mark.parametrize("waves", [1, 2], ids=["one_wave_per_simd", "two_waves_per_simd"])
@pytest.mark.parametrize("d", [50, 70])
def test_pooled_am_matrix_core_kernel_sizes(oracle, d, waves, monkeypatch):
    """pooled_mfma_kernel at d = 50 (one pass of four output blocks, the bench's size) and d = 70 (two passes, products
    parked in a second LDS buffer): bit for bit the lane-per-chain kernel (MCMCX_POOLED_SCALAR=1) and the restatement.
    Both instances: 512 registers at one wave per SIMD, and pooled_mfma_kernel<false, true> -- 256 registers, part of the
    state spilled around the products -- which the engine takes by itself only from 2048 / 8192 tiles on (MCMCX_POOLED_WAVES)."""
    from mcmcf90_amd import engine_from_problem
    monkeypatch.setenv("MCMCX_POOLED_WAVES", str(waves))
    N, nsimu, tick = 2 * d + 10, 9, 4           # more chains than parameters, or the pooled covariance is singular
    rng = np.random.default_rng(d)
    A = rng.standard_normal((d, d)) / np.sqrt(d)
    lam = A @ A.T + np.diag(np.linspace(0.5, 3.0, d))
    ckw = dict(nsimu=nsimu, adaptint=tick, updatesigma=0)
    pkw = dict(kind="gauss", npar=d, par0=np.full(d, 0.1), cmat0=(0.5 / d) * np.eye(d), mu=np.linspace(-0.5, 0.5, d), lam=lam)
    e = engine_from_problem(ckw, pkw, nchains=N, pooled=1, record_accept=1)
    e.init(); e.run()
    assert e.last_kernel() == {1: "pooled_mfma_kernel<false>", 2: "pooled_mfma_kernel<false, true>"}[waves], e.last_kernel()
    monkeypatch.setenv("MCMCX_POOLED_SCALAR", "1")
    e2 = engine_from_problem(ckw, pkw, nchains=N, pooled=1, record_accept=1)
    e2.init(); e2.run()
    assert e2.last_kernel() == "step_kernel<false, false, true>", e2.last_kernel()
    np.testing.assert_array_equal(_bits(e.theta()), _bits(e2.theta()))
    np.testing.assert_array_equal(e.accept_masks(), e2.accept_masks())
    e2.close()
    cfg = oracle.make_cfg(**dict(ckw, doadapt=0))
    prob = oracle.Problem(**pkw)
    chains = [oracle.LiveChain(cfg, prob, chain_id=c) for c in range(N)]
    state = {}
    par0, cmat0 = np.asarray(pkw["par0"], float), np.asarray(pkw["cmat0"], float)
    for t in (4, 8, nsimu):
        for ch in chains:
            ch.run(t)
        if t < nsimu:
            theta = np.array([ch.theta for ch in chains])
            cnt, s1, s2 = _pooled_moments(theta, par0, N)
            state = _merge_and_factor(oracle, state, cnt, s1, s2, par0, d, t == 4, cmat0, 0)
            for ch in chains:
                ch.set_R(state["R"])
    theta = np.array([ch.theta for ch in chains])
    np.testing.assert_array_equal(_bits(e.theta()), _bits(theta))
    for ch in chains:
        ch.close()
    e.close()


# ---------------------------------------------------------------- pooled burn-in scaling / greedy / AP / RAM
def _init_state(oracle, d, par0, cmat0, initcmatn, drscale=0.0):
    st = {"W": float(initcmatn), "C": {(i, j): float(cmat0[i, j]) for j in range(d) for i in range(j + 1)},
          "mean": [float(v) for v in par0], "drscale": float(drscale)}
    return _factor(oracle, st, d)


def _factor(oracle, st, d):
    """pooled_factor: dpotf2 + 2.4/sqrt(d); the old factor stays when the covariance is not positive definite"""
    A = np.zeros((d, d), order="F")
    for (i, j), v in st["C"].items():
        A[i, j] = v; A[j, i] = v
    if oracle.lib().mcxo_potrf_u(d, A.ctypes.data_as(C.POINTER(C.c_double))) == 0:
        sq = math.sqrt(float(d))
        st["R"] = np.array([[A[i, j] * 2.4 / sq if i <= j else 0.0 for j in range(d)] for i in range(d)])
        if st.get("drscale", 0.0) > 0.0:                 # pooled_dr_fresh: R2 = R / drscale, iC = dpotri('U', R)
            st["R2"] = st["R"] / st["drscale"]
            B = np.asfortranarray(st["R"].copy())
            assert oracle.lib().mcxo_potri_u(d, B.ctypes.data_as(C.POINTER(C.c_double))) == 0
            st["iC"] = np.triu(B)
    return st


def _merge(st, cnt, s1, s2, par0, d, replace):
    """pooled_merge of mcx_api.hip in Python floats"""
    n = cnt
    m1 = [s1[j] / n for j in range(d)]
    mb = [float(par0[j]) + m1[j] for j in range(d)]
    Cb = {(i, j): (s2[(i, j)] - n * m1[i] * m1[j]) / (n - 1.0) for j in range(d) for i in range(j + 1)}
    if replace or not st["W"] > 0.0:
        st["C"], st["mean"], st["W"] = Cb, mb, n
    else:
        W = st["W"]; Wn = W + n
        dl = [mb[j] - st["mean"][j] for j in range(d)]
        f = W * n / Wn
        st["C"] = {(i, j): ((W - 1.0) * st["C"][(i, j)] + (n - 1.0) * Cb[(i, j)] + f * dl[i] * dl[j]) / (Wn - 1.0)
                   for j in range(d) for i in range(j + 1)}
        g = n / Wn
        st["mean"] = [st["mean"][j] + g * dl[j] for j in range(d)]
        st["W"] = Wn
    return st


def _restate_pooled(oracle, ckw, pkw, N, nranks=1):
    """The engine's pooled_tick, tick by tick, on N single-chain oracles that never adapt on their own."""
    d = int(pkw["npar"])
    cfg = oracle.make_cfg(**ckw)
    plain = oracle.make_cfg(**dict(ckw, doadapt=0, doburnin=0, method="er" if ckw.get("method") == "er" else "dram"))
    prob = oracle.Problem(**pkw)
    chains = [oracle.LiveChain(plain, prob, chain_id=c) for c in range(N)]
    par0, cmat0 = np.asarray(pkw["par0"], float), np.asarray(pkw["cmat0"], float).reshape(d, d)
    dr = cfg.drscale if cfg.drscale > 0.0 and ckw.get("method") != "er" else 0.0
    st = _init_state(oracle, d, par0, cmat0, cfg.initcmatn, dr)
    badapt = cfg.badaptint if cfg.badaptint > 0 else cfg.adaptint
    log = []
    for it in range(2, cfg.nsimu + 1):
        m1 = cfg.adaptint != 0 and it % cfg.adaptint == 0
        m2 = badapt != 0 and it % badapt == 0
        if not (m1 or m2) or (cfg.adaptend > 0 and it > cfg.adaptend):
            continue
        burn = it < cfg.burnintime and cfg.doburnin != 0 and m2
        am = (not burn) and it >= cfg.burnintime + cfg.adaptint + cfg.adapthist and cfg.doadapt != 0
        if not (burn or am):
            continue
        for ch in chains:
            ch.run(it)
        theta = np.array([ch.theta for ch in chains])
        cnt, s1, s2 = _pooled_moments(theta, par0, N)
        if burn:
            stayed = float(sum(ch.stayed for ch in chains))
            staypc = stayed / (cnt * float(it))
            sf = cfg.scalefactor
            if staypc > 1.0 - cfg.scalelimit:
                st["R"] = st["R"] / sf; log.append((it, "down"))
                if dr > 0.0: st["R2"] = st["R2"] / sf; st["iC"] = st["iC"] * sf * sf
            elif staypc < cfg.scalelimit:
                st["R"] = st["R"] * sf; log.append((it, "up"))
                if dr > 0.0: st["R2"] = st["R2"] * sf; st["iC"] = st["iC"] / sf / sf
            else:
                if cfg.greedy:
                    st.update(W=float(cfg.initcmatn), C={(i, j): float(cmat0[i, j]) for j in range(d) for i in range(j + 1)},
                              mean=[float(v) for v in par0])
                    st = _merge(st, cnt, s1, s2, par0, d, False)
                st = _factor(oracle, st, d); log.append((it, "greedy" if cfg.greedy else "refactor"))
        else:
            if it == cfg.burnintime + cfg.adaptint + cfg.adapthist:
                st.update(W=float(cfg.initcmatn), C={(i, j): float(cmat0[i, j]) for j in range(d) for i in range(j + 1)},
                          mean=[float(v) for v in par0])
            st = _merge(st, cnt, s1, s2, par0, d, cfg.adapthist > 1)
            st = _factor(oracle, st, d); log.append((it, "ap" if cfg.adapthist > 1 else "am"))
        for ch in chains:
            ch.set_R(st["R"])
            if dr > 0.0: ch.set_dr(st["R2"], st["iC"])
    for ch in chains:
        ch.run(cfg.nsimu)
    return chains, st, log


def _fuzz_npar(default):
    """the sizes a random pooled configuration draws from; POOLED_FUZZ_NPAR=41,45,... narrows tools/pooled_restate_fuzz.py to one kernel's range"""
    e = os.environ.get("POOLED_FUZZ_NPAR")
    return [int(x) for x in e.split(",")] if e else default


def _draw_pooled(seed):
    """A random pooled configuration: AM / delayed rejection / early rejection; burn-in scaling, greedy, AP window, adaptend, initcmatn; sigma2
    update, bounds, priors; Gaussian and banana targets; npar 2..64; ragged tiles (tools/pooled_restate_fuzz.py runs thousands of these)."""
    r = np.random.default_rng(91000 + seed)
    d = int(r.choice(_fuzz_npar([2, 3, 5, 8, 13, 16, 17, 20, 24, 31, 33, 48, 50, 64])))
    N = int(r.choice([66, 70, 130, 200]))
    nsimu = int(r.integers(150, 330))
    ckw = dict(nsimu=nsimu, adaptint=int(r.choice([40, 50, 100])), updatesigma=int(r.random() < 0.3))
    mode = r.choice(["am", "dr", "er"], p=[0.5, 0.3, 0.2])
    if mode == "dr": ckw["drscale"] = float(r.choice([1.5, 2.0, 3.0]))
    if mode == "er": ckw["method"] = "er"
    if r.random() < 0.4:
        ckw.update(doburnin=1, burnintime=int(r.integers(60, 200)), badaptint=int(r.choice([25, 50])), scalelimit=float(r.choice([0.05, 0.3, 0.45])), scalefactor=2.5)
        if r.random() < 0.4: ckw.update(greedy=1, initcmatn=7)
    if r.random() < 0.2: ckw["adapthist"] = int(r.choice([30, 60]))
    if r.random() < 0.2: ckw["adaptend"] = int(r.integers(100, nsimu))
    c0 = float(r.choice([1e-4, 0.05, 0.3, 2.0, 40.0])) / d
    kind = "banana" if (mode != "er" and r.random() < 0.3) else "gauss"
    if kind == "gauss":
        Aa = r.standard_normal((d, d)) / np.sqrt(d)
        pkw = dict(kind="gauss", npar=d, par0=np.full(d, 0.2), cmat0=c0 * np.eye(d), mu=np.linspace(-1, 1, d), lam=Aa @ Aa.T + np.eye(d))
    else:
        pkw = dict(kind="banana", npar=d, par0=np.zeros(d), cmat0=c0 * np.eye(d), b=0.1)
    if r.random() < 0.3: pkw.update(lo=np.full(d, -2.0), hi=np.full(d, 2.0))
    if r.random() < 0.3: pkw.update(pri_mu=np.zeros(d), pri_sig=np.where(np.arange(d) % 3 == 0, 0.0, 1.5))
    if ckw["updatesigma"]: pkw.update(sigma2=0.8, nobs=25)
    return ckw, pkw, N, int(r.integers(20, nsimu))


def _check_pooled_against_restatement(oracle, seed):
    from mcmcf90_amd import engine_from_problem
    ckw, pkw, N, cut = _draw_pooled(seed)
    e = engine_from_problem(ckw, pkw, nchains=N, pooled=1, record_accept=1)
    e.init(); e.run(cut); e.run()
    kernel = e.last_kernel()
    chains, st, log = _restate_pooled(oracle, ckw, pkw, N)
    try:
        theta = np.array([ch.theta for ch in chains])
        np.testing.assert_array_equal(_bits(e.theta()), _bits(theta), err_msg=str((ckw, log)))
        for c in (0, 63, 64, N - 1):
            np.testing.assert_array_equal(e.accepted(c), chains[c].accepted, err_msg=str(ckw))
        cm, mean, W, R = e.pooled()
        assert W == st["W"], ckw
        np.testing.assert_array_equal(_bits(np.triu(R)), _bits(np.triu(st["R"])), err_msg=str(ckw))
        np.testing.assert_array_equal(_bits(mean), _bits(np.array(st["mean"])), err_msg=str(ckw))
        assert e.totals()["stayed"] == sum(ch.stayed for ch in chains), ckw
    finally:
        for ch in chains:
            ch.close()
        e.close()
    return kernel


@pytest.mark.parametrize("seed", range(36))
def test_random_pooled_configuration_matches_restatement(oracle, seed):
    """Pooled mode has no reference (the reference has one chain): its parity is the tick-by-tick restatement on single-chain oracles.  Beyond
    the fixed cases of this file: random configurations (round 5; thousands more through tools/pooled_restate_fuzz.py, profiles/r05_e)."""
    _check_pooled_against_restatement(oracle, seed)


@pytest.mark.parametrize("name,extra,c0", [
    ("scale_up", dict(doburnin=1, burnintime=260, badaptint=50, scalelimit=0.3), 1e-4),       # nearly everything accepted
    ("scale_down", dict(doburnin=1, burnintime=260, badaptint=50, scalelimit=0.3), 40.0),     # nearly everything rejected
    ("refactor", dict(doburnin=1, burnintime=260, badaptint=50, scalelimit=0.05), 0.05),
    ("greedy", dict(doburnin=1, burnintime=260, badaptint=50, scalelimit=0.05, greedy=1, initcmatn=7), 0.05),
    ("ap", dict(adapthist=60), 0.05),
    ("adaptend", dict(adaptend=150), 0.05),
])
def test_pooled_burnin_greedy_ap_match_restatement(oracle, name, extra, c0):
    from mcmcf90_amd import engine_from_problem
    d, N, nsimu = 5, 130, 420
    ckw = dict(nsimu=nsimu, adaptint=100, updatesigma=0, **extra)
    S = 0.5 ** np.abs(np.subtract.outer(np.arange(d), np.arange(d)))
    pkw = dict(kind="gauss", npar=d, par0=np.full(d, 0.3), cmat0=c0 * np.eye(d), mu=np.linspace(-1, 1, d), lam=np.linalg.inv(S))
    e = engine_from_problem(ckw, pkw, nchains=N, pooled=1, record_accept=1)
    e.init(); e.run()
    chains, st, log = _restate_pooled(oracle, ckw, pkw, N)
    kinds = {k for _, k in log}
    want = {"scale_up": "up", "scale_down": "down", "refactor": "refactor", "greedy": "greedy", "ap": "ap", "adaptend": "am"}[name]
    assert want in kinds, log                                   # the branch the case is about was taken
    theta = np.array([ch.theta for ch in chains])
    np.testing.assert_array_equal(_bits(e.theta()), _bits(theta), err_msg=str(log))
    for c in (0, 63, 64, N - 1):
        np.testing.assert_array_equal(e.accepted(c), chains[c].accepted)
    cm, mean, W, R = e.pooled()
    assert W == st["W"]
    np.testing.assert_array_equal(_bits(np.triu(R)), _bits(np.triu(st["R"])))
    np.testing.assert_array_equal(_bits(mean), _bits(np.array(st["mean"])))
    for ch in chains:
        ch.close()
    e.close()


def _getter_after_tick(e, pkw, msg):
    """mcmcx_pooled_moments after a run whose last tick reduced a longer vector (kind 1: one more entry; kind 2: another layout) in the same
    workspace: the plain moments of the states as they are, in the documented tree (tests/moment_tree_ref.py)."""
    import moment_tree_ref as mt
    got = e.pooled_moments()
    np.testing.assert_array_equal(_bits(got), _bits(mt.pooled_moments_ref(e.theta(), np.asarray(pkw["par0"], float))), err_msg=msg)
    assert got[0] == e.nchains, msg


@pytest.mark.parametrize("name,extra,c0", [
    ("scale_up", dict(doburnin=1, burnintime=260, badaptint=50, scalelimit=0.3), 1e-4),
    ("greedy", dict(doburnin=1, burnintime=260, badaptint=50, scalelimit=0.15, greedy=1, initcmatn=7), 4e-3),
])
def test_pooled_burnin_rejection_count_over_two_tree_launches(oracle, name, extra, c0):
    """The burn-in tick's vector (moments_kernel kind 1: the moments followed by the pooled rejection count) reduced over 66 tiles -- two launches
    of the tile tree, a ragged last tile, a second group of two tiles -- against the tick-by-tick restatement; the rejection count steers the
    factor (an `up` / `down` in the log), and the getter afterwards reduces the shorter plain vector in the same workspace."""
    from mcmcf90_amd import engine_from_problem
    d, N, nsimu = 3, 4163, 230
    ckw = dict(nsimu=nsimu, adaptint=100, updatesigma=0, **extra)
    S = 0.5 ** np.abs(np.subtract.outer(np.arange(d), np.arange(d)))
    pkw = dict(kind="gauss", npar=d, par0=np.full(d, 0.3), cmat0=c0 * np.eye(d), mu=np.linspace(-1, 1, d), lam=np.linalg.inv(S))
    e = engine_from_problem(ckw, pkw, nchains=N, pooled=1, record_accept=1)
    e.init(); e.run()
    chains, st, log = _restate_pooled(oracle, ckw, pkw, N)
    msg = "%s; sampling kernel %s" % (log, e.last_kernel())
    kinds = {k for _, k in log}
    assert kinds & {"up", "down"}, msg                           # without one the kind-1 value steered nothing
    if name == "greedy":
        assert "greedy" in kinds, msg
    theta = np.array([ch.theta for ch in chains])
    np.testing.assert_array_equal(_bits(e.theta()), _bits(theta), err_msg=msg)
    for c in (0, 4095, 4096, N - 1):
        np.testing.assert_array_equal(e.accepted(c), chains[c].accepted, err_msg=msg)
    cm, mean, W, R = e.pooled()
    assert W == st["W"], msg
    np.testing.assert_array_equal(_bits(np.triu(R)), _bits(np.triu(st["R"])), err_msg=msg)
    np.testing.assert_array_equal(_bits(mean), _bits(np.array(st["mean"])), err_msg=msg)
    _getter_after_tick(e, pkw, msg)
    for ch in chains:
        ch.close()
    e.close()


@pytest.mark.parametrize("name,extra,c0,kind", [
    ("dr_am", dict(drscale=2.0), 0.3, "gauss"),                                                          # second stage with the shared R2, iC
    ("dr_banana", dict(drscale=3.0), 1.0, "banana"),
    ("dr_scale_down", dict(drscale=2.0, doburnin=1, burnintime=260, badaptint=50, scalelimit=0.3), 400.0, "gauss"),   # R2 / sf, iC * sf * sf
    ("dr_scale_up", dict(drscale=2.0, doburnin=1, burnintime=260, badaptint=50, scalelimit=0.3), 1e-6, "gauss"),
    ("dr_updatesigma", dict(drscale=2.0, updatesigma=1), 0.3, "gauss"),
    ("er", dict(method="er"), 0.05, "gauss"),                                                            # MCMC_run_er with the shared factor
    ("er_updatesigma", dict(method="er", updatesigma=1), 0.05, "gauss"),
    ("dr_am_global_scratch", dict(drscale=2.0), 0.3, "gauss"),           # npar 5 forced onto step_kernel_pooled_dr_big (MCMCX_DR_BIG=1)
    ("dr_am_37", dict(drscale=2.0), 0.3, "gauss"),                       # npar 37: still the LDS form (four waves per CU)
    ("dr_am_57", dict(drscale=2.0), 0.3, "gauss"),                       # npar 57: the engine's own choice of the global-scratch form
    ("dr_am_170", dict(drscale=2.0), 0.3, "gauss"),                      # npar 170: beyond what the LDS form could hold at all
    ("dr_am_130_priors", dict(drscale=2.0), 0.3, "gauss"),               # npar 130: the matrix-core form in two passes, priors and bounds
    ("dr_banana_24", dict(drscale=3.0), 1.0, "banana"),                  # a non-Gaussian target between the products
])
@pytest.mark.parametrize("scalar", [0, 1, 2], ids=["matrix_cores", "lane_kernels", "matrix_cores_two_waves"])
def test_pooled_delayed_rejection_and_er_match_restatement(oracle, name, extra, c0, kind, scalar, monkeypatch):
    """pooled = 1 with drscale > 0 (one R2 = R / drscale and one iC = dpotri(R) for every chain, recomputed at each pooled
    tick, scaled in place by the burn-in branch as MCMC_adapt.F90:66-78 does) and with method = 'er'.  Delayed rejection on the
    matrix cores (pooled_mfma_kernel<true>: both stages' proposals, the Gaussian target and the two quadratic forms as products
    against the shared tables) and in the lane-per-chain kernels, their quadratic-form vectors in LDS (npar <= 40) or global scratch."""
    from mcmcf90_amd import engine_from_problem
    d, N, nsimu = 5, 130, 420
    two_waves = scalar == 2                                     # pooled_mfma_kernel<false, true>: the instance without delayed rejection only
    if two_waves:
        if "dr" in name:
            pytest.skip("two waves per SIMD: the instance without delayed rejection")
        scalar = 0
        monkeypatch.setenv("MCMCX_POOLED_WAVES", "2")
    else:
        monkeypatch.setenv("MCMCX_POOLED_WAVES", "1")
    if scalar:
        monkeypatch.setenv("MCMCX_POOLED_SCALAR", "1")         # the lane-per-chain kernels (shared tables through the scalar cache)
    elif name == "dr_am_global_scratch":
        pytest.skip("a switch of the lane-per-chain kernels")
    else:
        monkeypatch.setenv("MCMCX_POOLED_MFMA_DR_MIN", "1")    # the matrix-core form at npar 5 too (the engine's own choice starts at 21)
    if name == "dr_am_global_scratch":
        monkeypatch.setenv("MCMCX_DR_BIG", "1")
    if name == "dr_am_37":
        d, N, nsimu = 37, 70, 230
    if name == "dr_am_57":
        d, N, nsimu = 57, 70, 230
    if name == "dr_am_170":
        d, N, nsimu = 170, 70, 120
        c0 = 0.3 / d
    if name == "dr_am_130_priors":
        d, N, nsimu = 130, 70, 120
        c0 = 0.3 / d
    if name == "dr_banana_24":
        d, N, nsimu = 24, 70, 230
    ckw = dict(dict(nsimu=nsimu, adaptint=100, updatesigma=0), **extra)
    S = 0.5 ** np.abs(np.subtract.outer(np.arange(d), np.arange(d)))
    if kind == "gauss":
        pkw = dict(kind="gauss", npar=d, par0=np.full(d, 0.3), cmat0=c0 * np.eye(d), mu=np.linspace(-1, 1, d), lam=np.linalg.inv(S))
        if "priors" in name:
            pkw.update(pri_mu=np.zeros(d), pri_sig=np.where(np.arange(d) % 3 == 0, 0.0, 2.0), lo=np.full(d, -3.0), hi=np.full(d, 3.0))
    else:
        pkw = dict(kind="banana", npar=d, par0=np.zeros(d), cmat0=c0 * np.eye(d), b=0.1)
    e = engine_from_problem(ckw, pkw, nchains=N, pooled=1, record_accept=1)
    e.init(); e.run()
    if "dr" in name:
        assert e.last_kernel() == ("pooled_mfma_kernel<true>" if (not scalar and d <= 140) else        # (its LDS ends at npar ~140)
                                   "step_kernel_pooled_dr" if (d <= 40 and name != "dr_am_global_scratch") else "step_kernel_pooled_dr_big")
    else:
        assert e.last_kernel() == ("step_kernel<false, false, true>" if scalar else "pooled_mfma_kernel<false, true>" if two_waves else "pooled_mfma_kernel<false>")
    chains, st, log = _restate_pooled(oracle, ckw, pkw, N)
    kinds = {k for _, k in log}
    if "scale_down" in name: assert "down" in kinds, log
    if "scale_up" in name: assert "up" in kinds, log
    theta = np.array([ch.theta for ch in chains])
    np.testing.assert_array_equal(_bits(e.theta()), _bits(theta), err_msg=str(log))
    for c in (0, 63, 64, N - 1):
        np.testing.assert_array_equal(e.accepted(c), chains[c].accepted)
    cm, mean, W, R = e.pooled()
    np.testing.assert_array_equal(_bits(np.triu(R)), _bits(np.triu(st["R"])))
    tot = e.totals()
    if "dr" in name:
        R2, iC = e.dr_state(0)
        np.testing.assert_array_equal(_bits(np.triu(R2)), _bits(np.triu(st["R2"])))
        np.testing.assert_array_equal(_bits(np.triu(iC)), _bits(np.triu(st["iC"])))
        assert tot["drtries"] == sum(ch.drtries for ch in chains) and tot["drtries"] > 0
        assert tot["draccepted"] == sum(ch.draccepted for ch in chains) and (tot["draccepted"] > 0 or d > 100)
    else:
        for c in (0, 63, 64, N - 1):
            assert e.counters(c)["erstayed"] == chains[c].erstayed
    assert tot["stayed"] == sum(ch.stayed for ch in chains)
    for ch in chains:
        ch.close()
    e.close()


@pytest.mark.parametrize("name,d,N,extra,kind", [
    ("am_17", 17, 130, dict(), "gauss"), ("am_50_ragged", 50, 130, dict(), "gauss"), ("am_64", 64, 200, dict(), "gauss"), ("am_33_s2", 33, 140, dict(updatesigma=1), "gauss"),
    ("er_48", 48, 140, dict(method="er"), "gauss"), ("er_20_s2_priors", 20, 130, dict(method="er", updatesigma=1), "gauss"),
    ("am_49_bounds_priors", 49, 140, dict(), "gauss"), ("banana_24", 24, 130, dict(), "banana"), ("am_50_record", 50, 130, dict(), "gauss"),
    ("burnin_up_32", 32, 130, dict(doburnin=1, burnintime=160, badaptint=50, scalelimit=0.3), "gauss"), ("svd_20", 20, 130, dict(condmax=1e8), "gauss"),
    # npar 41..64: the forty-row form too (every class of npar rounded up to four, odd and even counts of deviates beyond the cut)
    ("am_41", 41, 130, dict(), "gauss"), ("am_45_s2", 45, 140, dict(updatesigma=1), "gauss"), ("banana_53", 53, 130, dict(), "banana"),
    ("svd_57", 57, 130, dict(condmax=1e8), "gauss"), ("burnin_up_60", 60, 130, dict(doburnin=1, burnintime=160, badaptint=50, scalelimit=0.3), "gauss"),
    ("er_63_s2_priors", 63, 130, dict(method="er", updatesigma=1), "gauss"), ("am_52_bounds_record", 52, 200, dict(), "gauss"),
    ("am_51_s2_priors", 51, 130, dict(updatesigma=1), "gauss"),      # (49..52: the instantiation whose fourth output block is a 4 x 4 x 4 product)
])
def test_pooled_two_waves_per_simd_matches_restatement(oracle, name, d, N, extra, kind, monkeypatch):
    """pooled_mfma_kernel<false, true> -- the instance behind bench.py's c4_pooled: 256 registers, two waves per SIMD, part of the state spilled
    around the products; the engine's own choice from 2048 / 8192 tiles on, forced here on a small problem (MCMCX_POOLED_WAVES=2) -- gives the
    chain of pooled_mfma_kernel<false> bit for bit and the restatement's: two to four output blocks, odd and even npar (the cached second deviate),
    ragged tiles, the sigma2 update, early rejection, bounds and priors and a non-Gaussian target, the SVD factor (a full, non-triangular table),
    burn-in scaling, the history ring and accept masks of a recorded chain.  (Up to round 5 these cases ran the two-waves-per-tile and
    half-tile variants, which are no longer in the library: tools/variants/README.md.)
    At npar 41..64 a third run: pooled_mfma_ks_kernel (the LDS vector in two pieces of forty rows, eight tiles per CU; the engine's own choice
    from 2048 tiles on, MCMCX_POOLED_KS=1 here) -- the same chain again, bit for bit."""
    from mcmcf90_amd import engine_from_problem
    nsimu = 230
    ckw = dict(dict(nsimu=nsimu, adaptint=100, updatesigma=0, N0=1.0, S02=0.5), **extra)
    S = 0.5 ** np.abs(np.subtract.outer(np.arange(d), np.arange(d)))
    c0 = 1e-6 if "burnin_up" in name else 0.3 / d
    if kind == "gauss":
        pkw = dict(kind="gauss", npar=d, par0=np.full(d, 0.3), cmat0=c0 * np.eye(d), mu=np.linspace(-1, 1, d), lam=np.linalg.inv(S))
        if "priors" in name:
            pkw.update(pri_mu=np.zeros(d), pri_sig=np.where(np.arange(d) % 3 == 0, 0.0, 2.0))
        if "bounds" in name:
            pkw.update(lo=np.full(d, -1.5), hi=np.full(d, 1.5))
        if "s2" in name:
            pkw.update(sigma2=0.8, nobs=20)
    else:
        pkw = dict(kind="banana", npar=d, par0=np.zeros(d), cmat0=(1.0 / d) * np.eye(d), b=0.1)
    ekw = dict(record_chain=1) if "record" in name else {}
    res = []
    for waves in (("ks",) if 40 < d <= 64 else ()) + ("2", "1"):
        monkeypatch.setenv("MCMCX_POOLED_WAVES", "2" if waves == "ks" else waves)
        monkeypatch.setenv("MCMCX_POOLED_KS", "1" if waves == "ks" else "0")
        e = engine_from_problem(ckw, pkw, nchains=N, pooled=1, record_accept=1, **ekw)
        e.init(); e.run(57); e.run()
        assert e.last_kernel() == {"ks": "pooled_mfma_ks_kernel", "2": "pooled_mfma_kernel<false, true>", "1": "pooled_mfma_kernel<false>"}[waves], e.last_kernel()
        res.append(dict(theta=e.theta().copy(), masks=e.accept_masks().copy(), scal=e.scalars().copy(), rng=[e.rng(c) for c in (0, 31, 32, 63, 64, N - 1)],
                        ctr=[e.counters(c) for c in (0, 33, N - 1)], pooled=e.pooled(), tot=e.totals(),
                        chain=[e.chain(c) for c in (0, 35, N - 1)] if ekw else []))
        e.close()
    b = res[-1]
    for a in res[:-1]:
        assert np.array_equal(_bits(a["theta"]), _bits(b["theta"])) and np.array_equal(a["masks"], b["masks"]) and np.array_equal(_bits(a["scal"]), _bits(b["scal"]))
        assert a["rng"] == b["rng"] and a["ctr"] == b["ctr"] and a["tot"] == b["tot"]
        np.testing.assert_array_equal(_bits(a["pooled"][3]), _bits(b["pooled"][3]))
        for x, y in zip(a["chain"], b["chain"]):
            for u, v in zip(x, y):
                np.testing.assert_array_equal(_bits(u), _bits(v))
    a = res[0]
    if "svd" in name:
        return                                             # (the SVD factor's restatement lives in test_pooled_factor_with_condmax; here: the two kernels)
    chains, st, log = _restate_pooled(oracle, ckw, pkw, N)
    assert log
    theta = np.array([ch.theta for ch in chains])
    np.testing.assert_array_equal(_bits(a["theta"]), _bits(theta), err_msg=str(log))
    for i, c in enumerate((0, 31, 32, 63, 64, N - 1)):
        assert a["rng"][i][0] == chains[c].ch.contents.rng.n
    np.testing.assert_array_equal(_bits(np.triu(a["pooled"][3])), _bits(np.triu(st["R"])))
    assert a["tot"]["stayed"] == sum(ch.stayed for ch in chains)
    for ch in chains:
        ch.close()


@pytest.mark.parametrize("name,extra", [("am", dict()), ("dr_s2", dict(drscale=2.0, updatesigma=1)), ("er", dict(method="er")),
                                        ("burnin_dr", dict(drscale=3.0, doburnin=1, burnintime=160, badaptint=50, scalelimit=0.3))])
def test_pooled_mode_with_response_columns(oracle, name, extra):
    """pooled = 1 with nycol = 2 (round 5: the response-column target in pooled mode, step_kernel_cols with the shared factor / R2 / iC through
    the scalar cache): the sums over the columns in MCMC_alpha, MCMC_sscrit and MCMC_DR_alpha13 and one gamma draw per column on every chain,
    the pooled ticks as for one column -- restated tick by tick with two-column oracle chains."""
    from mcmcf90_amd import engine_from_problem
    N, nsimu = 130, 330
    r = np.random.default_rng(77)
    x = np.arange(11.0)
    rates = np.array([0.1, 0.25])
    Y = np.vstack([9.0 * np.exp(-k * x) + r.standard_normal(11) * 0.3 for k in rates])
    ckw = dict(dict(nsimu=nsimu, adaptint=100, updatesigma=0, N0=1.0, S02=0.8), **extra)
    pkw = dict(kind="expdata", npar=3, par0=np.concatenate([[9.0], rates]), cmat0=np.diag([0.02, 0.0002, 0.0002]),
               sigma2=np.array([0.5, 0.8]), nobs=np.array([11, 11]), xdata=x, ydata=Y, lo=np.zeros(3))
    e = engine_from_problem(ckw, pkw, nchains=N, pooled=1, record_accept=1)
    e.init(); e.run()
    assert e.last_kernel() == "step_kernel_cols", e.last_kernel()
    chains, st, log = _restate_pooled(oracle, ckw, pkw, N)
    assert log, "no pooled tick was taken"
    theta = np.array([ch.theta for ch in chains])
    np.testing.assert_array_equal(_bits(e.theta()), _bits(theta), err_msg=str(log))
    for c in (0, 63, 64, N - 1):
        np.testing.assert_array_equal(e.accepted(c), chains[c].accepted)
        assert e.rng(c)[0] == chains[c].ch.contents.rng.n
    cm, mean, W, R = e.pooled()
    assert W == st["W"]
    np.testing.assert_array_equal(_bits(np.triu(R)), _bits(np.triu(st["R"])))
    tot = e.totals()
    assert tot["stayed"] == sum(ch.stayed for ch in chains)
    if "dr" in name:
        R2, iC = e.dr_state(0)
        np.testing.assert_array_equal(_bits(np.triu(R2)), _bits(np.triu(st["R2"])))
        np.testing.assert_array_equal(_bits(np.triu(iC)), _bits(np.triu(st["iC"])))
        assert tot["drtries"] == sum(ch.drtries for ch in chains) and tot["draccepted"] == sum(ch.draccepted for ch in chains) and tot["drtries"] > 0
    for ch in chains:
        ch.close()
    e.close()


def _restate_pooled_ram(oracle, ckw, pkw, N, log=None):
    """pooled_ram_tick, tick by tick, on N single-chain oracles that never adapt on their own: returns (chains, final factor, initial state, floor hits).
    log, if given, collects (iteration, chains whose alpha was NaN, whether the factor was replaced) of every tick.
    A statistic that is not finite (one chain's NaN alpha is enough) is refused, as pooled_reduce refuses it (error -46): the restatement ends
    at that tick, the chains standing on its iteration, and only a caller that reads the log may meet it."""
    d, condmax = int(pkw["npar"]), float(ckw.get("condmax", 0.0))
    nsimu, adaptint, nu, target = int(ckw["nsimu"]), int(ckw["adaptint"]), float(ckw["nuparam"]), float(ckw["alphatarget"])
    plain = oracle.make_cfg(**dict(ckw, doadapt=0, method="dram"))
    prob = oracle.Problem(**pkw)
    chains = [oracle.LiveChain(plain, prob, chain_id=c) for c in range(N)]
    DP = C.POINTER(C.c_double)
    floored = []

    def svd_factor(S, scale):
        """covtor_svd: U sqrt(s) of the symmetric S with s floored at s_1 / condmax (times 2.4/sqrt(d) for MCMC_init's factor)"""
        G = np.asfortranarray(S.copy()); V = np.zeros((d, d), order="F"); sv = np.zeros(d)
        oracle.lib().mcxo_symsvd(d, G.ctypes.data_as(DP), V.ctypes.data_as(DP), sv.ctypes.data_as(DP))
        tol = sv[0] / condmax
        if sv[d - 1] <= tol:
            sv = np.where(sv < tol, tol, sv); floored.append(1)
        R0 = np.array([[math.sqrt(sv[i]) * V[k, i] for i in range(d)] for k in range(d)])
        return np.array([[R0[i, j] * 2.4 / math.sqrt(float(d)) for j in range(d)] for i in range(d)]) if scale else R0

    if condmax > 0.0:
        R = svd_factor(np.asarray(pkw["cmat0"], float), True)
        for ch in chains:
            ch.set_R(R)
        st = {"R": R.copy()}
    else:
        st = _init_state(oracle, d, np.asarray(pkw["par0"], float), np.asarray(pkw["cmat0"], float), 0)
        R = st["R"]
    T = (N + 63) // 64

    def tree_over_chains(vals):
        v = np.zeros(T * 64); v[:N] = vals
        return _tree([_tree(v[t * 64:(t + 1) * 64]) for t in range(T)])

    for it in range(adaptint, nsimu + 1, adaptint):
        for ch in chains:
            ch.run(it)
        rs = 1.0 / math.pow(float(np.float32(it)), nu)
        X = np.zeros((N, d)); sgn = np.zeros(N)
        for c, ch in enumerate(chains):
            u = ch.last_u
            su = 0.0
            for k in range(d):
                su = su + u[k] * u[k]
            a = rs * (ch.alpha12 - target)
            X[c] = [u[k] / su * a for k in range(d)]
            sgn[c] = 1.0 if a >= 0.0 else -1.0
        if not np.isfinite(X).all():
            assert log is not None, "pooled RAM refuses the tick of iteration %d: a non-finite statistic" % it
            log.append((it, sum(math.isnan(ch.alpha12) for ch in chains), False))
            return chains, R, st, floored
        cnt = tree_over_chains(np.ones(N))
        S = np.zeros((d, d))
        for j in range(d):
            for i in range(j + 1):
                acc = 0.0
                if condmax > 0.0:                      # proposals Rf z: the Gram matrix is Rf Rf'
                    for k in range(d):
                        acc = _fma(R[i, k], R[j, k], acc)
                else:
                    for k in range(i + 1):
                        acc = _fma(R[k, i], R[k, j], acc)
                S[i, j] = acc + tree_over_chains(sgn * (X[:, i] * X[:, j])) / cnt
                S[j, i] = S[i, j]
        if condmax > 0.0:
            R = svd_factor(S, False)
        else:
            Af = np.asfortranarray(S.copy())
            ok = oracle.lib().mcxo_potrf_u(d, Af.ctypes.data_as(C.POINTER(C.c_double))) == 0
            if ok:
                R = np.triu(np.array(Af))
            if log is not None:
                log.append((it, sum(math.isnan(ch.alpha12) for ch in chains), ok))
        for ch in chains:
            ch.set_R(R)
    for ch in chains:
        ch.run(nsimu)
    return chains, R, st, floored


@pytest.mark.parametrize("d,N,mfma,condmax", [(6, 150, 0, 0.0), (6, 150, 1, 0.0), (50, 200, 1, 0.0), (6, 150, 0, 1e8), (6, 150, 1, 25.0), (20, 130, 1, 1e8),
                                              (50, 200, 2, 0.0), (20, 130, 2, 1e8),           # mfma = 2: pooled_mfma_kernel<false, true> (two waves per SIMD)
                                              (33, 140, 2, 0.0), (64, 200, 2, 0.0), (17, 130, 2, 25.0),
                                              (50, 200, 3, 0.0), (64, 200, 3, 0.0), (45, 130, 3, 1e8), (57, 140, 3, 25.0)])    # 3: pooled_mfma_ks_kernel
def test_pooled_ram_matches_restatement(oracle, d, N, mfma, condmax, monkeypatch):
    """method = 'ram', pooled = 1: one factor for all chains; every adaptint iterations the chains' rank-one RAM
    statistics sign(a) x x' (MCMC_run_ram.F90:166-172) of that iteration are averaged over all chains and folded into
    the Gram matrix of the shared factor, which is refactored (pooled_ram_tick).  condmax > 0: the shared factor is
    covtor_svd's full matrix (matutils.F90:378-453), proposals are matmulx(Rf, z), the Gram matrix is Rf Rf' and the
    refactorisation goes through the pinned SVD with the singular-value floor (condmax = 25 makes it bite)."""
    from mcmcf90_amd import engine_from_problem
    if not mfma:
        monkeypatch.setenv("MCMCX_POOLED_SCALAR", "1")
    monkeypatch.setenv("MCMCX_POOLED_WAVES", "2" if mfma >= 2 else "1")
    monkeypatch.setenv("MCMCX_POOLED_KS", "1" if mfma == 3 else "0")
    nsimu, adaptint, nu, target = 130, 20, 0.7, 0.234
    ckw = dict(nsimu=nsimu, method="ram", adaptint=adaptint, updatesigma=0, nuparam=nu, alphatarget=target, condmax=condmax)
    rng = np.random.default_rng(d)
    A = rng.standard_normal((d, d)) / np.sqrt(d)
    cm0 = (0.5 / d) * (np.diag(10.0 ** np.linspace(-3, 0, d)) if 0.0 < condmax < 100.0 else np.eye(d))     # cond 1000 > condmax: the floor bites
    pkw = dict(kind="gauss", npar=d, par0=np.full(d, 0.2), cmat0=cm0, mu=np.zeros(d), lam=A @ A.T + np.eye(d))
    e = engine_from_problem(ckw, pkw, nchains=N, pooled=1, record_accept=1)
    e.init(); e.run()
    assert e.last_kernel() == {0: "step_kernel<false, false, true>", 1: "pooled_mfma_kernel<false>", 2: "pooled_mfma_kernel<false, true>",
                               3: "pooled_mfma_ks_kernel"}[mfma], e.last_kernel()
    chains, R, st, floored = _restate_pooled_ram(oracle, ckw, pkw, N)
    theta = np.array([ch.theta for ch in chains])
    np.testing.assert_array_equal(_bits(e.theta()), _bits(theta))
    for c in (0, 63, 64, N - 1):
        np.testing.assert_array_equal(e.accepted(c), chains[c].accepted)
    if condmax > 0.0:
        np.testing.assert_array_equal(_bits(e.pooled()[3]), _bits(R))
        assert floored or condmax > 100
    else:
        np.testing.assert_array_equal(_bits(np.triu(e.pooled()[3])), _bits(R))
    assert not np.array_equal(R, st["R"])                       # the factor did adapt
    for ch in chains:
        ch.close()
    e.close()


@pytest.mark.parametrize("condmax", [0.0, 1e8])
def test_pooled_ram_statistic_over_two_tree_launches(oracle, condmax):
    """The pooled RAM statistic (moments_kernel kind 2) reduced over 66 tiles -- two launches of the tile tree, a ragged last tile, a second group
    of two tiles -- with the Cholesky and the SVD factor, against the tick-by-tick restatement; the getter afterwards reduces the plain
    moments, a vector of another length, in the same workspace.  (The engine picks the sampling kernel: it is not the subject here.)"""
    from mcmcf90_amd import engine_from_problem
    d, N = 3, 4163
    nsimu, adaptint, nu, target = 130, 20, 0.7, 0.234
    ckw = dict(nsimu=nsimu, method="ram", adaptint=adaptint, updatesigma=0, nuparam=nu, alphatarget=target, condmax=condmax)
    rng = np.random.default_rng(d)
    A = rng.standard_normal((d, d)) / np.sqrt(d)
    pkw = dict(kind="gauss", npar=d, par0=np.full(d, 0.2), cmat0=(0.5 / d) * np.eye(d), mu=np.zeros(d), lam=A @ A.T + np.eye(d))
    e = engine_from_problem(ckw, pkw, nchains=N, pooled=1, record_accept=1)
    e.init(); e.run()
    msg = "condmax %g; sampling kernel %s" % (condmax, e.last_kernel())
    chains, R, st, floored = _restate_pooled_ram(oracle, ckw, pkw, N)
    theta = np.array([ch.theta for ch in chains])
    np.testing.assert_array_equal(_bits(e.theta()), _bits(theta), err_msg=msg)
    for c in (0, 4095, 4096, N - 1):
        np.testing.assert_array_equal(e.accepted(c), chains[c].accepted, err_msg=msg)
    if condmax > 0.0:
        np.testing.assert_array_equal(_bits(e.pooled()[3]), _bits(R), err_msg=msg)
    else:
        np.testing.assert_array_equal(_bits(np.triu(e.pooled()[3])), _bits(R), err_msg=msg)
    assert not np.array_equal(R, st["R"]), msg                  # the factor did adapt
    _getter_after_tick(e, pkw, msg)
    for ch in chains:
        ch.close()
    e.close()


def _draw_pooled_ram(seed):
    r = np.random.default_rng(93000 + seed)
    d = int(r.choice(_fuzz_npar([2, 5, 6, 13, 16, 17, 20, 33, 50, 64])))
    N = int(r.choice([66, 70, 130, 200]))
    condmax = float(r.choice([0.0, 0.0, 0.0, 1e8, 25.0]))
    ckw = dict(nsimu=int(r.integers(60, 160)), method="ram", adaptint=int(r.choice([10, 20, 50])), updatesigma=0, nuparam=float(r.choice([0.6, 0.7, 0.9])),
               alphatarget=float(r.choice([0.234, 0.4])), condmax=condmax)
    A = r.standard_normal((d, d)) / np.sqrt(d)
    scale = float(r.choice([0.02, 0.5, 5.0])) / d
    cm0 = scale * (np.diag(10.0 ** np.linspace(-3, 0, d)) if 0.0 < condmax < 100.0 else np.eye(d))
    pkw = dict(kind="gauss", npar=d, par0=np.full(d, 0.2), cmat0=cm0, mu=np.linspace(-0.5, 0.5, d), lam=A @ A.T + np.eye(d))
    if r.random() < 0.3: pkw.update(lo=np.full(d, -2.0), hi=np.full(d, 2.0))
    if r.random() < 0.3: pkw.update(pri_mu=np.zeros(d), pri_sig=np.where(np.arange(d) % 3 == 0, 0.0, 1.5))
    return ckw, pkw, N, int(r.integers(5, ckw["nsimu"]))


def _check_pooled_ram_against_restatement(oracle, seed):
    from mcmcf90_amd import engine_from_problem
    ckw, pkw, N, cut = _draw_pooled_ram(seed)
    e = engine_from_problem(ckw, pkw, nchains=N, pooled=1, record_accept=1)
    e.init(); e.run(cut); e.run()
    kernel = e.last_kernel()
    chains, R, st, floored = _restate_pooled_ram(oracle, ckw, pkw, N)
    try:
        theta = np.array([ch.theta for ch in chains])
        np.testing.assert_array_equal(_bits(e.theta()), _bits(theta), err_msg=str(ckw))
        for c in (0, 63, 64, N - 1):
            np.testing.assert_array_equal(e.accepted(c), chains[c].accepted, err_msg=str(ckw))
        if ckw["condmax"] > 0.0:
            np.testing.assert_array_equal(_bits(e.pooled()[3]), _bits(R), err_msg=str(ckw))
        else:
            np.testing.assert_array_equal(_bits(np.triu(e.pooled()[3])), _bits(R), err_msg=str(ckw))
    finally:
        for ch in chains:
            ch.close()
        e.close()
    return kernel


@pytest.mark.parametrize("seed", range(24))
def test_random_pooled_ram_configuration_matches_restatement(oracle, seed):
    """Pooled RAM (the bench's `c4_pooled` mode) on random configurations: npar 2..64, ragged tiles, adaptation every 10 / 20 / 50 iterations,
    Cholesky and SVD factors (with the floor biting), bounds, priors, the run cut in two calls -- against the tick-by-tick restatement."""
    _check_pooled_ram_against_restatement(oracle, seed)


@pytest.mark.parametrize("mfma,condmax,burn,drscale", [(1, 1e8, 0, 0.0), (0, 1e8, 0, 0.0), (1, 40.0, 0, 0.0), (0, 40.0, 1, 0.0),
                                                       (0, 1e8, 0, 2.0), (0, 40.0, 1, 2.0),      # + delayed rejection: R2 full, iC from R's upper triangle
                                                       (1, 1e8, 0, 2.0), (1, 40.0, 1, 2.0)])     # ... and its second stage on the matrix cores
def test_pooled_am_with_svd_factor_matches_restatement(oracle, mfma, condmax, burn, drscale, monkeypatch):
    """pooled = 1 with condmax > 0 (method dram): the shared factor is covtor_svd's full matrix U sqrt(s) 2.4/sqrt(d)
    (matutils.F90:378-453) of the pooled covariance, proposals are matmulx(R, z); condmax = 40 makes the singular-value
    floor bite, after which the covariance itself is replaced by R0 R0' (info = -1 branch)."""
    from mcmcf90_amd import engine_from_problem
    if not mfma:
        monkeypatch.setenv("MCMCX_POOLED_SCALAR", "1")
    else:
        monkeypatch.setenv("MCMCX_POOLED_MFMA_DR_MIN", "1")
    d, N, nsimu = 6, 140, 330
    ckw = dict(nsimu=nsimu, adaptint=100, updatesigma=0, condmax=condmax, drscale=drscale)
    if burn:
        ckw.update(doburnin=1, burnintime=160, badaptint=40, scalelimit=0.3)
    lam = np.diag(10.0 ** np.linspace(-1.5, 1.5, d))            # posterior variances over three decades
    pkw = dict(kind="gauss", npar=d, par0=np.full(d, 0.1), cmat0=(1e-4 if burn else 0.02) * np.eye(d), mu=np.zeros(d), lam=lam)
    e = engine_from_problem(ckw, pkw, nchains=N, pooled=1, record_accept=1)
    e.init(); e.run()
    cfg = oracle.make_cfg(**ckw)
    plain = oracle.make_cfg(**dict(ckw, doadapt=0, doburnin=0))
    prob = oracle.Problem(**pkw)
    chains = [oracle.LiveChain(plain, prob, chain_id=c) for c in range(N)]
    par0, cmat0 = np.asarray(pkw["par0"], float), np.asarray(pkw["cmat0"], float)
    DP = C.POINTER(C.c_double)
    floored_ticks = []

    def svd_factor(st, it):
        G = np.zeros((d, d), order="F")
        for (i, j), v in st["C"].items():
            G[i, j] = v; G[j, i] = v
        V = np.zeros((d, d), order="F"); sv = np.zeros(d)
        oracle.lib().mcxo_symsvd(d, G.ctypes.data_as(DP), V.ctypes.data_as(DP), sv.ctypes.data_as(DP))
        if sv[0] == 0.0:
            return st
        tol = sv[0] / condmax
        floored = bool(sv[d - 1] <= tol)
        if floored:
            sv = np.where(sv < tol, tol, sv); floored_ticks.append(it)
        R0 = np.array([[math.sqrt(sv[i]) * V[k, i] for i in range(d)] for k in range(d)])       # R0[k, i] = U(k,i) sqrt(s_i)
        if floored:
            newC = {}
            for j in range(d):
                for i in range(j + 1):
                    acc = 0.0
                    for k in range(d):
                        acc = _fma(R0[i, k], R0[j, k], acc)
                    newC[(i, j)] = acc
            st["C"] = newC
        sqd = math.sqrt(float(d))
        st["R"] = np.array([[R0[i, j] * 2.4 / sqd for j in range(d)] for i in range(d)])
        if drscale > 0.0:
            st["R2"] = st["R"] / drscale
            B = np.asfortranarray(np.triu(st["R"]))
            assert oracle.lib().mcxo_potri_u(d, B.ctypes.data_as(DP)) == 0
            st["iC"] = np.triu(B)
        return st

    st = {"W": 0.0, "C": {(i, j): float(cmat0[i, j]) for j in range(d) for i in range(j + 1)}, "mean": [float(v) for v in par0]}
    C0 = dict(st["C"])
    st = svd_factor(st, 0); st["C"] = C0                        # MCMC_init's factor; cmat0 itself stays
    badapt = cfg.badaptint if cfg.badaptint > 0 else cfg.adaptint
    for it in range(2, nsimu + 1):
        m1, m2 = it % cfg.adaptint == 0, it % badapt == 0
        burn_tick = it < cfg.burnintime and cfg.doburnin != 0 and m2
        am_tick = (not burn_tick) and (m1 or m2) and it >= cfg.burnintime + cfg.adaptint + cfg.adapthist
        if not (burn_tick or am_tick):
            continue
        for ch in chains:
            ch.run(it)
        theta = np.array([ch.theta for ch in chains])
        cnt, s1, s2 = _pooled_moments(theta, par0, N)
        if burn_tick:
            staypc = float(sum(ch.stayed for ch in chains)) / (cnt * float(it))
            sf = cfg.scalefactor
            if staypc > 1.0 - cfg.scalelimit:
                st["R"] = st["R"] / sf
                if drscale > 0.0: st["R2"] = st["R2"] / sf; st["iC"] = st["iC"] * sf * sf
            elif staypc < cfg.scalelimit:
                st["R"] = st["R"] * sf
                if drscale > 0.0: st["R2"] = st["R2"] * sf; st["iC"] = st["iC"] / sf / sf
            else:
                st = svd_factor(st, it)
        else:
            if it == cfg.burnintime + cfg.adaptint + cfg.adapthist:
                st.update(W=float(cfg.initcmatn), C={(i, j): float(cmat0[i, j]) for j in range(d) for i in range(j + 1)}, mean=[float(v) for v in par0])
            st = _merge(st, cnt, s1, s2, par0, d, False)
            st = svd_factor(st, it)
        for ch in chains:
            ch.set_R(st["R"])
            if drscale > 0.0: ch.set_dr(st["R2"], st["iC"])
    for ch in chains:
        ch.run(nsimu)
    if drscale > 0.0:
        R2, iC = e.dr_state(0)
        np.testing.assert_array_equal(_bits(R2), _bits(st["R2"]))
        np.testing.assert_array_equal(_bits(np.triu(iC)), _bits(np.triu(st["iC"])))
        assert e.totals()["drtries"] == sum(ch.drtries for ch in chains) > 0
    if condmax < 100:
        assert floored_ticks, "the floor never bit: the case does not test what it is about"
    theta = np.array([ch.theta for ch in chains])
    np.testing.assert_array_equal(_bits(e.theta()), _bits(theta))
    for c in (0, 63, 64, N - 1):
        np.testing.assert_array_equal(e.accepted(c), chains[c].accepted)
    cm, mean, W, R = e.pooled()
    np.testing.assert_array_equal(_bits(R), _bits(st["R"]))
    Cst = np.zeros((d, d))
    for (i, j), v in st["C"].items():
        Cst[i, j] = v; Cst[j, i] = v
    np.testing.assert_array_equal(_bits(np.triu(cm)), _bits(np.triu(Cst)))
    for ch in chains:
        ch.close()
    e.close()


# ---------------------------------------------------------------- sums of squares that are +inf, NaN or subnormal (tests/edge_problems.py)
def _edge_case(name):
    """(cfg keywords, problem keywords, chains, environment, kernel) of a pooled case on an overflowing ("ovf") or subnormal ("sub") Gaussian target.
    T and c of every overflow problem were chosen on the CPU so that the restatement's oracle chains alone meet _edge_regime's conditions.
    Chain counts and run lengths are those of the tests above for the same kernels."""
    import edge_problems as ep
    form, how = name.rsplit("_", 1)
    d, T, c = {"am24": (24, 30.0, 0.3), "am50": (50, 60.0, 0.15), "dr24": (24, 30.0, 0.3), "ram50ks": (50, 45.0, 0.15), "ram50w2": (50, 45.0, 0.15),
               "scam30": (30, 37.0, 0.5)}[form]
    pkw = ep.overflow(d, T, c, blk={"am50": 0.8, "ram50ks": 0.6, "ram50w2": 0.6}.get(form, 0.5)) if how == "ovf" else ep.subnormal(d, 2.0 ** -1030)
    env = dict(MCMCX_POOLED_WAVES="1", MCMCX_POOLED_KS="0")
    if form.startswith("ram"):
        ckw = dict(nsimu=130, method="ram", adaptint=20, updatesigma=0, nuparam=0.7, alphatarget=0.234, condmax=0.0)
        env = dict(MCMCX_POOLED_WAVES="2", MCMCX_POOLED_KS="1" if form.endswith("ks") else "0")
        return ckw, pkw, 200, env, "pooled_mfma_ks_kernel" if form.endswith("ks") else "pooled_mfma_kernel<false, true>"
    if form.startswith("scam"):
        pkw["cmat0"] = 0.5 * (pkw["cmat0"] + pkw["cmat0"].T)     # (the pinned dgesvd is defined for a symmetric matrix)
        return dict(nsimu=60, adaptint=25, updatesigma=0, method="scam"), pkw, 70, env, "scam_pooled_kernel"
    ckw = dict(nsimu=230, adaptint=100, updatesigma=0)
    if form.startswith("dr"):
        ckw["drscale"] = 2.0
        env["MCMCX_POOLED_MFMA_DR_MIN"] = "1"
        return ckw, pkw, 70, env, "pooled_mfma_kernel<true>"
    return ckw, pkw, 130, env, "pooled_mfma_kernel<false>"


def _edge_restate(oracle, name):
    """The restatement of a case: (chains, what the shared factor must be: {getter index or name: array}, the RAM tick log)"""
    ckw, pkw, N, _, _ = _edge_case(name)
    d = int(pkw["npar"])
    if ckw.get("method") == "ram":
        log = []
        chains, R, st, _ = _restate_pooled_ram(oracle, ckw, pkw, N, log=log)
        if not log[-1][2]:                                      # refused at the tick of iteration k: the run up to k - 1 is what there is to compare
            for ch in chains:
                ch.close()
            chains, R, st, _ = _restate_pooled_ram(oracle, dict(ckw, nsimu=log[-1][0] - 1), pkw, N)
        assert not np.array_equal(R, st["R"])                   # the factor did adapt
        return chains, {"R": np.triu(R)}, log
    if ckw.get("method") == "scam":
        cfg = oracle.make_cfg(**dict(ckw, doadapt=0))
        prob = oracle.Problem(**pkw)
        chains = [oracle.LiveChain(cfg, prob, chain_id=c) for c in range(N)]
        state, tick, nsimu = {}, ckw["adaptint"], ckw["nsimu"]
        par0, cmat0 = np.asarray(pkw["par0"], float), np.asarray(pkw["cmat0"], float)
        for t in list(range(tick, nsimu, tick)) + [nsimu]:
            for ch in chains:
                ch.run(t)
            if t < nsimu:
                theta = np.array([ch.theta for ch in chains])
                cnt, s1, s2 = _pooled_moments(theta, par0, N)
                state = _merge_and_factor(oracle, state, cnt, s1, s2, par0, d, t == tick, cmat0, 0)
                state = _scam_factor(oracle, state, d, cfg.condmax)
                for ch in chains:
                    ch.set_R(state["U"]); ch.set_qcovstd(state["std"])
        return chains, {"U": state["U"], "std": state["std"]}, None
    chains, st, log = _restate_pooled(oracle, ckw, pkw, N)
    assert log
    want = {"R": np.triu(st["R"])}
    if ckw.get("drscale", 0.0) > 0.0:
        want.update(R2=np.triu(st["R2"]), iC=np.triu(st["iC"]))
    return chains, want, None


def _edge_regime(name, chains, N, log, nsimu):
    """What makes a case worth running, from the restatement's oracle chains alone (the conditions of tests/test_gpu_every_chain.py's edge branch)."""
    import edge_problems as ep
    ckw = _edge_case(name)[0]
    scam, ram = ckw.get("method") == "scam", ckw.get("method") == "ram"
    cc = [ch.ch.contents for ch in chains]
    acc = np.array([ch.accepted for ch in chains])
    theta = np.array([ch.theta for ch in chains])
    assert acc.shape == (N, nsimu) and np.isfinite(theta).all()
    rate = acc[:, 1:].mean()
    rate1 = 1.0 - sum(c.drtries for c in cc) / (N * (nsimu - 1.0)) if ckw.get("drscale") else rate
    if name.endswith("sub"):
        ss1 = np.array([c.ss1 for c in cc])
        assert ep.is_subnormal(ss1).all() and len(np.unique(ss1)) == N, (ss1.min(), ss1.max(), len(np.unique(ss1)))
        if scam:                                                # (an iteration of SCAM nearly always moves: the last component's alpha, as tests/test_gpu_every_chain.py has it)
            a = np.minimum(np.array([np.ctypeslib.as_array(c.alpha_trace, shape=(nsimu,))[1:] for c in cc]), 1.0).mean()
            assert rate > 0.9 and 0.5 < a < 0.9, (rate, a)
        else:
            assert 0.1 < rate1 < 0.5, rate1
        if ram:
            assert len(log) == 6 and all(ok and not n for _, n, ok in log), log        # every tick adapted
        return
    ssinf, ssnan, nprop = (np.array([getattr(c, k) for c in cc], dtype=np.int64) for k in ("n_ss_inf", "n_ss_nan", "nprop"))
    tiles = [slice(t, t + 64) for t in range(0, N - 63, 64)]
    print("%s: first-stage rate %.3f, ss = +inf %.4f, NaN %.4f of %d proposals%s" % (name, rate1, ssinf.sum() / nprop.sum(), ssnan.sum() / nprop.sum(), nprop.sum(),
                                                                                    "; RAM ticks (iteration, NaN alphas, adapted): %s" % log if ram else ""))
    assert all(ssnan[t].any() for t in tiles) and all(ssinf[t].any() for t in tiles)
    if scam:
        assert ssinf.sum() > 0 and ssnan.sum() > 0
    else:
        assert 0.1 < rate1 < 0.75, rate1
        assert ssinf.sum() >= 0.01 * nprop.sum() and ssnan.sum() >= 0.005 * nprop.sum()
    if ram:
        # Pooled RAM folds every chain's sign(a) x x' into one statistic (pooled_ram_tick): ONE chain whose alpha is NaN at the tick's iteration
        # makes every entry NaN, and the engine refuses to go on (pooled_reduce: error -46).  A tick that adapted comes first, then the one
        # with a NaN alpha in a chain or two of two hundred
        assert len(log) >= 2 and all(ok and n == 0 for _, n, ok in log[:-1]) and not log[-1][2] and 0 < log[-1][1] < 5, log


EDGE_CASES = [f + "_" + h for f in ("am24", "am50", "dr24", "ram50ks", "ram50w2", "scam30") for h in ("ovf", "sub")]


@pytest.mark.parametrize("name", EDGE_CASES)
def test_pooled_matrix_core_kernels_at_infinite_nan_and_subnormal_sums_of_squares(oracle, name, monkeypatch):
    """The Gaussian target on the f64 matrix cores -- pooled_mfma_kernel (AM at npar 24 and 50, delayed rejection at 24), pooled RAM on
    pooled_mfma_ks_kernel and pooled_mfma_kernel<false, true> (50), scam_pooled_kernel (30) -- where a row of Lam v rounds to +-inf (ss = +inf, or
    NaN from inf - inf in two partial chains) and where every product is subnormal: the order is defined to equal mcxt_ss_gauss's fma chain, and a
    flush to zero or a wider internal accumulator would show here and nowhere else.  EVERY chain against the restatement: state, accept sequence,
    ss1 and the last alpha (a NaN equals a NaN whatever its sign and payload, everything else bit for bit), stream position; the shared factor.
    Pooled RAM at overflow: the run ends with error -46 at the first tick whose iteration has a NaN alpha in any chain;
    everything up to the iteration before is compared, then the refusal itself."""
    import edge_problems as ep
    from mcmcf90_amd import engine_from_problem, McmcError
    ckw, pkw, N, env, kernel = _edge_case(name)
    chains, want, log = _edge_restate(oracle, name)
    refused = log[-1][0] if log and not log[-1][2] else 0       # the iteration of the tick the engine must refuse
    nsimu = refused - 1 if refused else ckw["nsimu"]
    try:
        _edge_regime(name, chains, N, log, nsimu)               # ... before the engine is touched
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        e = engine_from_problem(ckw, pkw, nchains=N, pooled=1, record_accept=1)
        e.init(); e.run(min(57, nsimu - 2)); e.run(nsimu)
        assert e.last_kernel() == kernel, e.last_kernel()
        theta, masks, scal = e.theta(), e.accept_masks(), e.scalars()
        rng = np.array([e.rng(c)[0] for c in range(N)], dtype=np.uint64)
        got = {"R": np.triu(e.pooled()[3]), "U": e.pooled()[3]}
        if "std" in want:
            got["std"] = e.qcovstd(0)
        if "R2" in want:
            got["R2"], got["iC"] = (np.triu(a) for a in e.dr_state(0))
        tot = e.totals()
        if refused:
            with pytest.raises(McmcError, match="non-finite pooled statistic at iteration %d" % refused):
                e.run()
        e.close()
        c = np.arange(N)
        acc = ((masks[:, c // 64] >> (c % 64).astype(np.uint64)) & np.uint64(1)).astype(np.uint8).T
        np.testing.assert_array_equal(acc[:, :nsimu], np.array([ch.accepted for ch in chains]))
        np.testing.assert_array_equal(_bits(theta), _bits(np.array([ch.theta for ch in chains])))
        cc = [ch.ch.contents for ch in chains]
        assert ep.same_bits_or_nan(scal[:, 0], np.array([k.ss1 for k in cc])).all()
        assert ep.same_bits_or_nan(scal[:, 3], np.array([k.alpha12 for k in cc])).all()
        np.testing.assert_array_equal(rng, np.array([k.rng.n for k in cc], dtype=np.uint64))
        for k, v in want.items():
            assert np.isfinite(v).all(), k
            np.testing.assert_array_equal(_bits(got[k]), _bits(v), err_msg=k)
        assert tot["stayed"] == sum(k.stayed for k in cc)
        assert not tot["status"] & 2                            # (no tick was skipped for a Gram matrix that is not positive definite)
    finally:
        for ch in chains:
            ch.close()
