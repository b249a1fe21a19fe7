"""The sample store's posterior covariance on the f64 matrix cores (mcmcx_samples_cov / _dev / _finish, include/mcmcx.h).

The definition is sums in a fixed order, so the whole vector is compared on raw bits with the restatement (tests/cov_ref.py: libm's fma through
ctypes, about 1e6 per second -- every case says its count, chains x ns x pairs).  Through mcmcx_debug_samples_cov, which runs the same kernels
on a caller's array: data over forty decades, some seeds with +-inf and NaN (a NaN's payload is the adder's own, so NaNs are compared as
NaNs and everything else on bits), chain counts around a tile and at 66 tiles, field counts on both sides of every 16-row block edge of
form A and the first of form B, form B at 203 fields, ns = 1, and a given shift.  Through a run: windows of a whole and of a wrapped ring, the
three-column target, stores written by other kernel families, the host and the torch form, the run unmoved, the refusals, two engines adding
up, and the covariance of a Gaussian target within four Monte-Carlo standard errors, handed on to setcmat0."""
import ctypes as C

import numpy as np
import pytest

import cov_ref
from test_gpu_samples import FORMS, SWITCHES, _bits, _cols3, _engine, _final, _gauss, _same_final

pytestmark = pytest.mark.gpu
DP = C.POINTER(C.c_double)


def _dp(a):
    return None if a is None else a.ctypes.data_as(DP)


def _decades(seed, ns, nf, nch, specials=0):
    """[ns][nf][nch]: random signs, magnitudes 1e-20 .. 1e20; `specials` entries of +-inf and NaN, none of them in chain 0 of sample 0 (the
    default shift)"""
    rng = np.random.default_rng(seed)
    X = rng.choice([-1.0, 1.0], size=(ns, nf, nch)) * 10.0 ** rng.uniform(-20.0, 20.0, size=(ns, nf, nch))
    for k in range(specials):
        s, f, c = rng.integers(ns), rng.integers(nf), rng.integers(nch)
        if (s, c) != (0, 0):
            X[s, f, c] = (np.inf, -np.inf, np.nan)[k % 3]
    return X


def _debug(X, shift=None):
    from mcmcf90_amd import _lib
    L = _lib.load()
    ns, nf, nch = X.shape
    X = np.ascontiguousarray(X, dtype=np.float64)
    sh = None if shift is None else np.ascontiguousarray(shift, dtype=np.float64)
    out = np.full(cov_ref.vec_len(nf), 7.0)
    rc = L.mcmcx_debug_samples_cov(0, nch, nf, ns, _dp(X), _dp(sh), _dp(out))
    assert rc == 0, (rc, L.mcmcx_last_error())
    return out


def _same(got, want, what, only=None):
    """NaNs where the restatement has NaNs, equal bits everywhere else (`only`: the indices to look at)."""
    if only is not None:
        got, want = got[only], want[only]
    assert got.shape == want.shape, what
    gn, wn = np.isnan(got), np.isnan(want)
    assert np.array_equal(gn, wn), (what, np.flatnonzero(gn != wn)[:8])
    bad = np.flatnonzero((_bits(got) != _bits(want)) & ~wn)
    assert bad.size == 0, (what, bad[:8], got[bad[:8]], want[bad[:8]])


@pytest.mark.parametrize("nch,ns", [(1, 5), (63, 5), (64, 5), (65, 5), (583, 9), (4163, 4)])
def test_bits_over_chain_counts(nch, ns):
    """10 fields, 55 pairs: 4163 chains x 4 x 55 = 9.2e5 fma at the most; 4163 chains are 66 tiles, a second level of the tree.  Seeds with and
    without +-inf and NaN; the entry's NaN padding of the last tile must not show."""
    for seed, specials in ((nch, 0), (nch + 1, 6)) if nch < 4163 else ((nch, 3),):
        X = _decades(seed, ns, 10, nch, specials)
        got, want = _debug(X), cov_ref.cov_vector_ref(X)
        assert got[0] == float(ns * nch) and np.array_equal(_bits(got[1:11]), _bits(X[0, :, 0]))
        _same(got, want, (nch, seed))
        if specials == 0:
            assert np.isfinite(got).all()
        else:
            touched = np.unique(np.nonzero(~np.isfinite(X))[1])
            clean = [cov_ref.pair_index(j, k, 10) for j in range(10) for k in range(j, 10) if j not in touched and k not in touched]
            assert np.isfinite(got[21:][clean]).all() and not np.isfinite(got[11:21][touched]).any()


@pytest.mark.parametrize("nf", [1, 15, 16, 31, 32, 47, 48, 63, 64, 65])
def test_bits_over_field_counts(nf):
    """65 chains (two tiles, the second with one chain), ns = 5: 65 x 5 x 2145 pairs = 7.0e5 fma at 65 fields.  With the row of ones 15 fields
    fill one block, 16 open the second, ..., 63 are the last form A takes, 64 and 65 go to form B."""
    X = _decades(100 + nf, 5, nf, 65, specials=(4 if nf % 2 else 0))
    _same(_debug(X), cov_ref.cov_vector_ref(X), nf)


def test_bits_of_form_b_at_203_fields():
    """65 chains, ns = 4.  Bit-exact: all pairs with j or k in the last block (fields 192 .. 202), the block-diagonal pairs of the first and of a
    middle block, 1000 random pairs -- 3.4e3 pairs x 65 x 4 = 9.0e5 fma.  Every remaining pair against the longdouble reference within the
    derived bound 2 n u sum|z_j z_k|, so no pair is left out."""
    nf = 203
    X = _decades(203, 4, nf, 65)
    got = _debug(X)
    J, K = cov_ref.all_pairs(nf)
    rng = np.random.default_rng(7)
    pick = (K >= 192) | ((J < 16) & (K < 16)) | ((J >= 96) & (J < 112) & (K >= 96) & (K < 112))
    pick[rng.choice(J.size, 1000, replace=False)] = True
    want = cov_ref.cov_vector_ref(X, pairs=(J[pick], K[pick]))
    head = np.arange(1 + 2 * nf)
    _same(got, want, "n, shift, S", only=head)
    _same(got, want, "picked pairs", only=1 + 2 * nf + np.flatnonzero(pick))
    S, G, bS, bG = cov_ref.longdouble_ref(X)
    assert np.all(np.abs(got[1 + nf:1 + 2 * nf].astype(np.longdouble) - S) <= bS)
    err = np.abs(got[1 + 2 * nf:].astype(np.longdouble) - G)
    assert np.all(err <= bG), float((err / bG).max())


def test_one_sample_and_a_given_shift():
    """ns = 1; a shift given against the NULL shift: the same shift handed in gives the same bits, another one the restatement's."""
    X = _decades(5, 1, 17, 130)                                 # 130 x 1 x 153 = 2.0e4 fma
    a = _debug(X)
    _same(a, cov_ref.cov_vector_ref(X), "ns 1")
    assert np.array_equal(_bits(_debug(X, X[0, :, 0].copy())), _bits(a))
    X = _decades(6, 3, 17, 130)                                 # 6.0e4 fma, twice
    sh = np.random.default_rng(6).normal(size=17) * 1e3
    b = _debug(X, sh)
    _same(b, cov_ref.cov_vector_ref(X, sh), "given shift")
    assert np.array_equal(_bits(b[1:18]), _bits(sh)) and not np.array_equal(_bits(b[18:]), _bits(_debug(X)[18:]))


# ---------------------------------------------------------------- through a run
def _check(e, s0, ns, shift=None, torch_too=True):
    """Host and device form against the restatement of the same window; returns the vector."""
    _, X = e.samples(s0, ns, layout=1)                          # [ns][nfields][nchains]
    nf = X.shape[1]
    want = cov_ref.cov_vector_ref(X, shift)
    got = e.samples_cov_stats(s0, ns, shift)
    what = (e.nchains, nf, s0, ns, shift is not None)
    assert got.shape == want.shape == (e.L.mcmcx_samples_cov_len(e.h),), what
    _same(got, want, what)
    assert got[0] == float(X.shape[0] * e.nchains)
    if torch_too:
        t = e.samples_cov_stats_torch(s0, ns, shift)
        assert t.is_cuda and str(t.dtype) == "torch.float64"
        assert np.array_equal(_bits(t.cpu().numpy()), _bits(got)), (what, "device form")
    return got


def _shape_engine(nch, prob, capacity, nsimu=70, **kw):
    from mcmcf90_amd import engine_from_problem
    e = engine_from_problem(dict(dict(nsimu=nsimu, adaptint=15, updatesigma=1), **kw), prob, nchains=nch, chain_id0=2)
    e.set_samples(1, 1, capacity)
    e.init()
    e.run()
    return e


def test_bits_of_windows_of_a_whole_and_a_wrapped_ring():
    """npar 7 (10 fields) at 583 chains: 583 x 20 x 55 = 6.4e5 fma per window of twenty, three of them; then 583 x 21 x 55 across the wrap."""
    prob = _gauss(7, 27, sigma2=0.7, nobs=9)
    e = _shape_engine(583, prob, 70)
    assert e.samples_kept()[:2] == (70, 1)
    shift = np.random.default_rng(1).normal(size=10) * 0.3
    for k, s0 in enumerate((0, 3, 50)):
        _check(e, s0, 20, shift if k == 1 else None)
    e.close()
    e = _shape_engine(583, prob, 20)                            # retained sample s sits in slot (10 + s) % 20: the wrap is between 9 and 10
    assert e.samples_kept()[:2] == (20, 51)
    _check(e, 5, 9)
    _check(e, 7, 12, shift)
    e.close()


def test_bits_of_the_three_column_target():
    """11 fields, the E.ssv / E.s2v rows: 130 x 30 x 66 = 2.6e5 fma"""
    e = _shape_engine(130, _cols3(), 70)
    assert e.samples_kept()[3] == 11
    _check(e, 40, 30)
    r = e.samples_cov(s0=40, ns=30, fields="all")
    assert r["fields"] == ["theta[0]", "theta[1]", "theta[2]", "theta[3]", "ss[0]", "ss[1]", "ss[2]", "sspri", "sigma2[0]", "sigma2[1]",
                           "sigma2[2]"] and r["n"] == 30 * 130 and r["cov"].shape == (11, 11)
    _, X = e.samples(40, 30, layout=1)
    flat = X.transpose(1, 0, 2).reshape(11, -1)
    vary = np.flatnonzero(flat.std(axis=1) > 0)
    assert np.allclose(r["mean"], flat.mean(axis=1), rtol=1e-9, atol=0.0)
    assert np.allclose(r["cov"][np.ix_(vary, vary)], np.cov(flat)[np.ix_(vary, vary)], rtol=1e-6, atol=0.0)
    t = e.samples_cov(s0=40, ns=30, shift="mean")               # the default: the theta block
    assert t["fields"] == r["fields"][:4] and np.allclose(t["cov"], r["cov"][:4, :4], rtol=1e-9, atol=0.0)
    e.close()


@pytest.mark.parametrize("name", ["ram_group", "pooled_mfma"])
def test_bits_of_stores_written_by_other_kernel_families(name, monkeypatch):
    """The covariance does not depend on the family, but the store's rows come from different writers.  70 x 24 x 120 = 2.0e5 fma (npar 12),
    130 x 12 x 276 = 4.3e5 (npar 20)."""
    env, ckw, _, nch, kernel, _ = FORMS[name]
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    e = _engine(name, None, (3, 2, 24))
    assert e.run() == 0 and e.last_kernel() == kernel
    assert e.samples_kept()[0] == 24
    if name == "ram_group":
        _check(e, 0, 24)
    else:
        _check(e, 11, 12)
    e.close()


def test_the_run_is_unmoved(monkeypatch):
    """Two engines cut at the same iterations, one calling the covariance mid-run (its scratch allocated then)."""
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("MCMCX_GROUP", "0")
    chains = [0, 63, 64, 129]
    finals = []
    for call in (True, False):
        e = _engine("lane_am", None, (3, 7, None))
        assert e.run(50) == 0
        if call:
            a = e.samples_cov_stats()
        assert e.run(90) == 0
        if call:
            b = e.samples_cov_stats(1, 8, shift=np.zeros(10))
            t = e.samples_cov_stats_torch(0, None)
            assert a.size == b.size == t.numel() == 76
        assert e.run() == 0
        finals.append((_final(e, chains, False), _bits(e.samples()[1])))
        e.close()
    _same_final(finals[0][0], finals[1][0], "a covariance in the middle of the run")
    assert np.array_equal(finals[0][1], finals[1][1])


def test_refusals_launch_nothing():
    from mcmcf90_amd import engine_from_problem
    prob = _gauss(2, 22, sigma2=0.7, nobs=9)
    e = engine_from_problem(dict(nsimu=40, adaptint=15, updatesigma=1), prob, nchains=65, chain_id0=2)
    L = e.L
    n = 1 + 10 + 15
    buf = np.full(n, 7.0)
    p = _dp(buf)
    e.set_samples(1, 3, 5)
    assert L.mcmcx_samples_cov(e.h, 0, 4, None, p) == -51 and b"inited" in L.mcmcx_last_error()
    assert L.mcmcx_samples_cov_len(e.h) == n
    e.init()
    e.run()
    before = _bits(e.samples()[1])
    assert e.samples_kept()[0] == 5
    for s0, ns in ((0, 0), (0, -4), (-1, 4), (2, 4), (0, 6), (5, 1), (2 ** 31 - 1, 4), (1, 2 ** 31 - 1)):
        for fn, out in ((L.mcmcx_samples_cov, p), (L.mcmcx_samples_cov_dev, C.c_void_p(8))):      # refused before the pointer is looked at
            rc = fn(e.h, s0, ns, None, out)
            assert rc == -51 and len(L.mcmcx_last_error()) > 0, (s0, ns, rc)
    assert L.mcmcx_samples_cov(e.h, 0, 4, None, None) == -51 and b"null output" in L.mcmcx_last_error()
    assert L.mcmcx_samples_cov_dev(e.h, 0, 4, None, None) == -51
    assert np.all(buf == 7.0)
    assert np.array_equal(_bits(e.samples()[1]), before)
    _check(e, 0, 5)                                             # still usable
    _check(e, 4, 1)
    assert np.array_equal(_bits(e.samples()[1]), before)        # and the covariance writes nothing into the ring either
    e.close()
    e = engine_from_problem(dict(nsimu=40, adaptint=15, updatesigma=1), prob, nchains=65, chain_id0=2)
    e.init()
    e.run()
    assert L.mcmcx_samples_cov(e.h, 0, 4, None, p) == -51 and b"no samples are kept" in L.mcmcx_last_error()
    e.close()


def test_vectors_of_two_engines_add_up():
    """Chains 0 .. 127 and 128 .. 255 in two engines (chain_id0 0 and 128) with one shift: the sum of their vectors against the longdouble
    reference of one engine that runs all 256, within the forward bound of any summation order."""
    from mcmcf90_amd import engine_from_problem
    prob = _gauss(7, 27, sigma2=0.7, nobs=9)
    ckw = dict(nsimu=60, adaptint=20, updatesigma=1)

    def eng(nch, id0):
        e = engine_from_problem(ckw, prob, nchains=nch, chain_id0=id0)
        e.set_samples(21, 1, 40)
        e.init()
        e.run()
        return e
    whole = eng(256, 0)
    _, X = whole.samples(layout=1)
    whole.close()
    shift = X[0, :, 0].copy()
    parts = []
    for id0 in (0, 128):
        e = eng(128, id0)
        assert np.array_equal(_bits(e.samples(layout=1)[1]), _bits(X[:, :, id0:id0 + 128])), "the halves are the whole engine's chains"
        parts.append(e.samples_cov_stats(0, 40, shift))
        e.close()
    total = parts[0] + parts[1]
    total[1:11] = shift
    assert total[0] == 40 * 256
    S, G, bS, bG = cov_ref.longdouble_ref(X, shift)
    assert np.all(np.abs(total[11:21].astype(np.longdouble) - S) <= bS)
    assert np.all(np.abs(total[21:].astype(np.longdouble) - G) <= bG)


def test_covariance_of_a_gaussian_target_and_the_next_run():
    """4163 chains on a Gaussian with known covariance S; thirty samples, every twentieth iteration from 320 on.  Each entry of the theta
    block within four Monte-Carlo standard errors: for a Gaussian var(C_jk) = (S_jj S_kk + S_jk^2) / n_eff, with n_eff the smaller of the two
    fields' ESS from samples_summary (the ESS of the means; the products decorrelate faster, so this is on the safe side of n_eff).  Then
    the result is the next run's cmat0 -- the reference's mcmccovf.dat cycle."""
    from mcmcf90_amd import engine_from_problem
    d = 4
    rng = np.random.default_rng(12)
    A = rng.standard_normal((d, d))
    S = A @ A.T / d + 0.5 * np.eye(d)
    prob = dict(kind="gauss", npar=d, par0=np.array([0.3, -0.2, 0.1, 0.0]), cmat0=(2.4 ** 2 / d) * S, mu=np.array([0.5, -1.0, 0.25, 2.0]),
                lam=np.linalg.inv(S))
    ckw = dict(nsimu=900, adaptint=100, updatesigma=0)
    e = engine_from_problem(ckw, prob, nchains=4163, chain_id0=0)
    e.set_samples(320, 20, 30)
    e.init()
    assert e.run() == 0 and e.samples_kept()[0] == 30
    r = e.samples_cov(shift="mean")
    assert r["fields"] == ["theta[%d]" % i for i in range(d)] and r["n"] == 30 * 4163
    ess = e.samples_summary(maxlag=14)["ess"][:d]
    assert np.all(ess > 1000.0)
    se = np.sqrt((np.outer(np.diag(S), np.diag(S)) + S * S) / np.minimum.outer(ess, ess))
    dev = np.abs(r["cov"] - S) / se
    print("deviations in standard errors", np.round(dev, 2).tolist(), "ess", np.round(ess).tolist())
    assert np.all(dev < 4.0), dev
    assert np.all(np.abs(r["mean"] - prob["mu"]) < 4.0 * np.sqrt(np.diag(S) / ess))
    assert np.allclose(np.diag(r["corr"]), 1.0) and np.all(np.linalg.eigvalsh(r["cov"]) > 0)
    e.close()
    e2 = engine_from_problem(dict(nsimu=50, adaptint=100, updatesigma=0), dict(prob, cmat0=np.eye(d)), nchains=65, chain_id0=0)
    e2.setcmat0(r["cov"])
    e2.init()
    assert e2.run() == 0
    e2.close()


def test_readers_share_one_scratch_back_to_back():
    """The summary, the order statistics and counts and the covariance carve their work areas out of ONE grow-only scratch of the engine.
    The asynchronous forms are issued back to back with nothing synchronised in between -- counts with one threshold (the smallest scratch),
    stats at maxlag 0, cov, order statistics at 32 ranks (a regrow while the earlier calls are still queued), stats at maxlag 3 -- each into
    a tensor of its own; after ONE sync every tensor holds the bits of the host form of the same call made alone on a second engine with
    the same seed.  70 chains (two tiles, the second ragged), npar 3, a ring of 8 under 20 kept iterations (wrapped)."""
    import torch
    from mcmcf90_amd import engine_from_problem

    def eng():
        e = engine_from_problem(dict(nsimu=20, adaptint=7, updatesigma=1), _gauss(3, 31, sigma2=0.6, nobs=11), nchains=70, chain_id0=4)
        e.set_samples(1, 1, 8)
        e.init()
        assert e.run() == 0 and e.samples_kept()[:2] == (8, 13)
        return e

    a, b = eng(), eng()
    nf = a.samples_kept()[3]
    assert nf == 6
    x = np.full((nf, 1), 0.05)
    ranks = np.linspace(0, 8 * 70 - 1, 32).astype(np.int64)
    L, h = a.L, a.h

    def dev(*shape, dtype=torch.float64):
        return torch.empty(shape, dtype=dtype, device="cuda:%d" % a.cfg.device)
    # every tensor first: an allocation between two calls may synchronise the device
    t_cnt, t_s0, t_cov = dev(nf, 1, 2, dtype=torch.int64), dev(L.mcmcx_samples_stats_len(h, 0)), dev(L.mcmcx_samples_cov_len(h))
    t_os, t_s3 = dev(nf, 32), dev(L.mcmcx_samples_stats_len(h, 3))
    ptr = lambda t: C.c_void_p(t.data_ptr())
    assert L.mcmcx_samples_counts_dev(h, 0, 8, 1, _dp(x), ptr(t_cnt)) == 0
    assert L.mcmcx_samples_stats_dev(h, 0, 8, 0, None, ptr(t_s0)) == 0
    assert L.mcmcx_samples_cov_dev(h, 0, 8, None, ptr(t_cov)) == 0
    assert L.mcmcx_samples_order_stats_dev(h, 0, 8, 32, ranks.ctypes.data_as(C.POINTER(C.c_int64)), ptr(t_os)) == 0
    assert L.mcmcx_samples_stats_dev(h, 0, 8, 3, None, ptr(t_s3)) == 0
    a.sync()
    assert np.array_equal(t_cnt.cpu().numpy(), b.samples_counts(x, 0, 8)), "counts"
    _same(t_s0.cpu().numpy(), b.samples_stats(0, 8, 0), "stats, maxlag 0")
    _same(t_cov.cpu().numpy(), b.samples_cov_stats(0, 8), "cov")
    _same(t_os.cpu().numpy().ravel(), b.samples_order_stats(ranks, 0, 8).ravel(), "order statistics")
    _same(t_s3.cpu().numpy(), b.samples_stats(0, 8, 3), "stats, maxlag 3")
    a.close(); b.close()
