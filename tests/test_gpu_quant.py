"""Exact order statistics, tail counts and quantiles of the sample store, reduced on the device (mcmcx_samples_order_stats / _counts /
_quantiles, include/mcmcx.h).

Nothing here depends on an order of summation, so everything is compared bit for bit: order statistics as raw uint64 with np.sort of the
keys of Engine.samples(layout=1) of the same window (tests/quant_ref.py), counts as integers.  Shapes: chain counts around a tile and at 66
tiles (seventeen blocks of four waves), field counts 4, 10, 11 and 65, windows of 1, 2 and 70 samples, s0 > 0, a wrapped ring with the window
across the wrap; rank lists with 0 and n - 1, a repeated rank, unsorted order, nr = 1 and nr = 32.  Iteration 1 holds par0 in every chain (a tie
of nchains values) and sspri is constant (every digit wave-uniform).  Adversarial arrays go through mcmcx_debug_order_stats."""
import ctypes as C

import numpy as np
import pytest

import quant_ref
from test_gpu_samples import FORMS, SWITCHES, _bits, _cols3, _engine, _final, _gauss, _same_final

pytestmark = pytest.mark.gpu
NSIMU = 70                                                      # first = 1, thin = 1: seventy kept iterations
PROBS = (0.0, 0.025, 0.25, 1.0 / 3.0, 0.5, 0.975, 1.0)


def _shape_engine(nch, prob, capacity, **kw):
    from mcmcf90_amd import engine_from_problem
    e = engine_from_problem(dict(dict(nsimu=NSIMU, adaptint=15, updatesigma=1), **kw), prob, nchains=nch, chain_id0=2)
    e.set_samples(1, 1, capacity)
    e.init()
    e.run()
    return e


def _rank_lists(n, seed):
    """Unsorted with 0, n - 1 and a repeat; nr = 1; nr = 32."""
    rng = np.random.default_rng(seed)
    return [np.array([n - 1, 0, n // 2, n // 2, (7 * n) // 10, n // 40], dtype=np.int64), np.array([n // 3], dtype=np.int64),
            np.concatenate([[n - 1, 0], rng.integers(0, n, 30)]).astype(np.int64)]


def _check_os(e, s0, ns, ranks, X=None):
    if X is None:
        X = e.samples(s0, ns, layout=1)[1]                      # [ns][nfields][nchains]
    want = quant_ref.order_stats_ref(X, ranks)
    got = e.samples_order_stats(ranks, s0, ns)
    what = (e.nchains, X.shape[1], s0, ns, list(ranks[:6]))
    assert got.shape == want.shape == (X.shape[1], len(ranks)), what
    bad = np.argwhere(_bits(got) != _bits(want))
    assert bad.size == 0, (what, bad[:4], got[tuple(bad[0])], want[tuple(bad[0])])
    return got


def _thresholds(X, os_):
    """[nfields][nq]: window values (ties are hit), points between two values, below the minimum, above the maximum."""
    flat = np.moveaxis(X, 1, 0).reshape(X.shape[1], -1)
    lo, hi = flat.min(axis=1), flat.max(axis=1)
    mid = 0.5 * (os_[:, 0] + os_[:, -1])
    return np.stack([os_[:, 0], os_[:, os_.shape[1] // 2], os_[:, -1], mid, np.nextafter(mid, np.inf), np.nextafter(lo, -np.inf),
                     np.nextafter(hi, np.inf), lo, hi], axis=1)


def _check_counts(e, s0, ns, X, ranks, os_):
    x = _thresholds(X, os_)
    want = quant_ref.counts_ref(X, x)
    got = e.samples_counts(x, s0, ns)
    what = (e.nchains, X.shape[1], s0, ns)
    assert got.dtype == np.int64 and got.shape == want.shape == x.shape + (2,), what
    assert np.array_equal(got, want), (what, np.argwhere(got != want)[:4])
    n = X.shape[0] * X.shape[2]
    assert np.all(got[:, 5] == 0) and np.all(got[:, 6] == n), (what, "below the minimum, above the maximum")
    c = e.samples_counts(os_, s0, ns)                           # lt(os(r)) <= r < le(os(r))
    r = np.asarray(ranks)[None, :]
    assert np.all(c[:, :, 0] <= r) and np.all(r < c[:, :, 1]), what
    return got


def _check_window(e, s0, ns, seed, counts=True, lists=(0, 1, 2)):
    X = e.samples(s0, ns, layout=1)[1]
    n = ns * e.nchains
    rl = _rank_lists(n, seed)
    for k in lists:
        got = _check_os(e, s0, ns, rl[k], X)
        if counts and k == lists[0]:
            _check_counts(e, s0, ns, X, rl[k], got)


FULL = [(0, 70), (0, 1), (0, 2), (3, 9), (61, 9), (1, 1)]       # a ring that holds all seventy kept iterations; (0, *) includes iteration 1
WRAP = [(0, 20), (5, 9), (16, 4), (9, 5), (9, 2)]               # a ring of twenty under seventy: slot (10 + s) % 20, the wrap between 9 and 10


def _run_windows(e, wins):
    for k, (s0, ns) in enumerate(wins):
        _check_window(e, s0, ns, 10 + k, lists=(0, 1, 2) if k < 2 else (k % 3,))


@pytest.mark.parametrize("nch", [1, 63, 64, 65, 583, 4163])
def test_order_stats_and_counts_over_chain_counts(nch):
    """npar 7 (nfields 10); theta[3] is centred at zero, so both signs occur; sspri is constant; iteration 1 is par0 in every chain."""
    prob = _gauss(7, 27, sigma2=0.7, nobs=9)
    e = _shape_engine(nch, prob, NSIMU)
    assert e.samples_kept()[:2] == (NSIMU, 1)
    X = e.samples(0, 70, layout=1)[1]
    if nch > 1:
        assert (X[:, 3] < 0).any() and (X[:, 3] > 0).any(), "both signs"
    assert np.all(_bits(X[0, :7]) == _bits(X[0, :7, :1])) and np.all(_bits(X[:, 8]) == _bits(X[0, 8, 0])), "the tie and the constant field"
    _run_windows(e, FULL)
    e.close()
    e = _shape_engine(nch, prob, 20)
    assert e.samples_kept()[:2] == (20, 51)
    _run_windows(e, WRAP)
    e.close()


@pytest.mark.parametrize("name,nch", [("npar1", 65), ("npar1", 4163), ("cols3", 130), ("npar62", 583)])
def test_order_stats_and_counts_over_field_counts(name, nch):
    """nfields 4 (npar 1: the target is centred at zero), 11 (the three-column target: E.ssv / E.s2v rows), 65."""
    prob = {"npar1": _gauss(1, 21, sigma2=0.7, nobs=9), "cols3": _cols3(), "npar62": _gauss(62, 82, sigma2=0.7, nobs=9)}[name]
    e = _shape_engine(nch, prob, NSIMU)
    assert e.samples_kept()[3] == {"npar1": 4, "cols3": 11, "npar62": 65}[name]
    _run_windows(e, FULL[:4])
    e.close()
    e = _shape_engine(nch, prob, 20)
    _run_windows(e, WRAP[:3])
    e.close()


@pytest.mark.parametrize("name", ["ram_group", "pooled_mfma", "host"])
def test_order_stats_of_stores_written_by_other_kernel_families(name, monkeypatch):
    env, ckw, _, nch, kernel, _ = FORMS[name]
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    e = _engine(name, None, (3, 2, 24))
    assert e.run() == 0 and e.last_kernel() == kernel
    assert e.samples_kept()[0] == 24
    _run_windows(e, [(0, 24), (2, 21), (11, 5)])
    e.close()


# ---- adversarial arrays through mcmcx_debug_order_stats
def _debug_os(values, ranks):
    from mcmcf90_amd import _lib
    L = _lib.load()
    v = np.ascontiguousarray(values, dtype=np.float64)
    r = np.ascontiguousarray(ranks, dtype=np.int64)
    out = np.zeros(r.size)
    rc = L.mcmcx_debug_order_stats(0, v.size, v.ctypes.data_as(C.POINTER(C.c_double)), r.size, r.ctypes.data_as(C.POINTER(C.c_int64)),
                                   out.ctypes.data_as(C.POINTER(C.c_double)))
    assert rc == 0, L.mcmcx_last_error()
    return out


def _adversarial(kind, n, rng):
    u = np.uint64
    if kind == "equal":
        return np.full(n, -3.25)
    if kind == "last_byte":                                     # the top 56 bits shared, the last byte differs
        return (u(0x400921FB54442D00) | rng.integers(0, 256, n).astype(u)).view(np.float64)
    if kind == "zeros":
        return np.where(rng.integers(0, 2, n) == 1, 0.0, -0.0)
    if kind == "inf":
        return rng.choice(np.array([np.inf, -np.inf, 1.0, -1.0, 0.0]), n)
    if kind == "nan":                                           # NaNs of both signs and several payloads among numbers
        pool = np.array([0x7FF8000000000000, 0xFFF8000000000000, 0x7FF0000000000001, 0xFFFFFFFFFFFFFFFF, 0x7FFFFFFFFFFFFFFF,
                         0x3FF0000000000000, 0xBFF0000000000000, 0x7FF0000000000000, 0xFFF0000000000000], dtype=u).view(np.float64)
        return pool[rng.integers(0, pool.size, n)]
    if kind == "denormal":
        b = rng.integers(0, 2 ** 52, n).astype(u) | (rng.integers(0, 2, n).astype(u) << u(63))
        b[: min(n, 4)] = np.array([1, 0x8000000000000001, 0, 0x8000000000000000], dtype=u)[: min(n, 4)]
        return b.view(np.float64)
    if kind == "all_exponents":
        return ((rng.integers(0, 2, n).astype(u) << u(63)) | (rng.integers(0, 2048, n).astype(u) << u(52))
                | rng.integers(0, 2 ** 52, n).astype(u)).view(np.float64)
    raise KeyError(kind)


@pytest.mark.parametrize("kind", ["equal", "last_byte", "zeros", "inf", "nan", "denormal", "all_exponents"])
def test_adversarial_arrays(kind):
    rng = np.random.default_rng(len(kind))
    for n in (1, 64, 65, 4163):
        v = _adversarial(kind, n, rng)
        for ranks in _rank_lists(n, n):
            got = _debug_os(v, ranks)
            want = quant_ref.order_stats_1d(v, ranks)
            assert np.array_equal(_bits(got), _bits(want)), (kind, n, list(ranks[:6]))


@pytest.mark.parametrize("kind", ["last_byte", "nan", "all_exponents"])
def test_every_rank_of_a_small_array_is_the_full_sort(kind):
    rng = np.random.default_rng(7)
    for n in (65, 200):
        v = _adversarial(kind, n, rng)
        got = np.concatenate([_debug_os(v, np.arange(r0, min(r0 + 32, n))[::-1]) for r0 in range(0, n, 32)])
        want = np.concatenate([quant_ref.order_stats_1d(v, np.arange(r0, min(r0 + 32, n))[::-1]) for r0 in range(0, n, 32)])
        assert np.array_equal(_bits(got), _bits(want)), (kind, n)


def test_a_wave_takes_more_than_one_tile():
    """700 000 values are 10 938 tiles: more than the 2560 blocks of four waves the grid is capped at for one field, so a wave loops over
    tiles and a block's LDS counters take several tiles' values.  The padding lanes of the last tile hold the smallest key there is."""
    rng = np.random.default_rng(11)
    n = 700000
    v = rng.standard_normal(n)
    v[:1000] = 0.5
    ranks = _rank_lists(n, 3)[2]
    got = _debug_os(v, ranks)
    assert np.array_equal(_bits(got), _bits(quant_ref.order_stats_1d(v, ranks)))


# ---- counts add up, quantiles, the summary, the torch form
def test_counts_of_two_engines_add_up_exactly():
    """Chains 0 .. 127 and 128 .. 255 in two engines (chain_id0 0 and 128): their counts add up to the 256-chain engine's -- integers, no
    tolerance."""
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
    X = whole.samples(layout=1)[1]
    os_ = whole.samples_order_stats([0, 256 * 40 // 2, 256 * 40 - 1])
    x = _thresholds(X, os_)
    total = whole.samples_counts(x)
    assert np.array_equal(total, quant_ref.counts_ref(X, x))
    whole.close()
    parts = []
    for id0 in (0, 128):
        e = eng(128, id0)
        assert np.array_equal(_bits(e.samples(layout=1)[1]), _bits(X[:, :, id0:id0 + 128])), "the halves are the whole engine's chains"
        parts.append(e.samples_counts(x))
        e.close()
    assert np.array_equal(parts[0] + parts[1], total)


def test_quantiles_summary_and_torch_form():
    e = _shape_engine(583, _cols3(), NSIMU)
    before = e.samples_summary(s0=10, ns=40, maxlag=8)
    for s0, ns in ((10, 40), (0, 70), (0, 1), (69, 1)):
        X = e.samples(s0, ns, layout=1)[1]
        want = quant_ref.quantiles_ref(X, PROBS)
        got = e.samples_quantiles(PROBS, s0, ns)
        assert got.shape == want.shape == (11, len(PROBS)) and np.array_equal(_bits(got), _bits(want)), (s0, ns)
        flat = np.moveaxis(X, 1, 0).reshape(11, -1)
        assert np.array_equal(got[:, 0], flat.min(axis=1)) and np.array_equal(got[:, -1], flat.max(axis=1))
        assert np.allclose(got, np.quantile(flat, PROBS, axis=1).T, rtol=1e-13, atol=1e-13 * np.abs(flat).max()), "numpy's own quantile"
    s = e.samples_summary(s0=10, ns=40, maxlag=8, probs=PROBS)
    assert set(s) == set(before) | {"probs", "quantiles"} and sorted(before) == sorted(
        ["mean", "sd", "rhat", "ess", "mcse", "W", "Bn", "truncated", "fields", "iterations"])
    for k in before:
        same = s[k] == before[k] if k == "fields" else np.array_equal(_bits(s[k]), _bits(before[k]))     # bits: a constant field's NaNs
        assert same, k
    assert np.array_equal(s["probs"], np.array(PROBS))
    assert np.array_equal(_bits(s["quantiles"]), _bits(quant_ref.quantiles_ref(e.samples(10, 40, layout=1)[1], PROBS)))
    n = 40 * 583
    for ranks in _rank_lists(n, 5):
        t = e.samples_order_stats_torch(ranks, 10, 40)
        assert t.is_cuda and str(t.dtype) == "torch.float64" and tuple(t.shape) == (11, len(ranks))
        assert np.array_equal(_bits(t.cpu().numpy()), _bits(e.samples_order_stats(ranks, 10, 40)))
    e.close()


def test_counts_dev_form():
    import torch
    e = _shape_engine(130, _gauss(7, 27, sigma2=0.7, nobs=9), NSIMU)
    X = e.samples(5, 30, layout=1)[1]
    for nq in (1, 2, 5, 8, 9, 32):                              # every instantiation of the counts kernel, on both sides of its bound
        rng = np.random.default_rng(nq)
        flat = np.moveaxis(X, 1, 0).reshape(10, -1)
        x = np.ascontiguousarray(np.stack([rng.choice(flat[f], nq) for f in range(10)]))
        x[:, ::3] += 1e-3 * rng.standard_normal(x[:, ::3].shape)
        want = quant_ref.counts_ref(X, x)
        assert np.array_equal(e.samples_counts(x, 5, 30), want), nq
        t = torch.full((10, nq, 2), -1, dtype=torch.int64, device="cuda:%d" % e.cfg.device)
        assert e.L.mcmcx_samples_counts_dev(e.h, 5, 30, nq, x.ctypes.data_as(C.POINTER(C.c_double)), C.c_void_p(t.data_ptr())) == 0
        e.sync()
        assert np.array_equal(t.cpu().numpy(), want), nq
    e.close()


def test_the_run_is_unmoved(monkeypatch):
    """Two engines cut at the same iterations, one calling order statistics and counts mid-run (the scratch grows at the second call)."""
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("MCMCX_GROUP", "0")
    chains = [0, 63, 64, 129]
    finals = []
    for ask in (True, False):
        e = _engine("lane_am", None, (3, 7, None))
        assert e.run(50) == 0
        if ask:
            n = e.samples_kept()[0] * e.nchains
            a = e.samples_order_stats([0, n - 1])
            c = e.samples_counts(a)
        assert e.run(90) == 0
        if ask:
            n = 8 * e.nchains
            b = e.samples_order_stats(np.arange(32) * (n // 32), 1, 8)
            t = e.samples_order_stats_torch([n // 2], 1, 8)
            q = e.samples_quantiles([0.025, 0.5, 0.975])
            c2 = e.samples_counts(b, 1, 8)
            assert a.shape == (10, 2) and c.shape == (10, 2, 2) and b.shape == (10, 32) and t.shape == (10, 1) and q.shape == (10, 3)
            assert c2.shape == (10, 32, 2)
        assert e.run() == 0
        finals.append((_final(e, chains, False), _bits(e.samples()[1])))
        e.close()
    _same_final(finals[0][0], finals[1][0], "order statistics and counts in the middle of the run")
    assert np.array_equal(finals[0][1], finals[1][1])


def test_refusals_launch_nothing():
    from mcmcf90_amd import engine_from_problem
    prob = _gauss(2, 22, sigma2=0.7, nobs=9)
    e = engine_from_problem(dict(nsimu=40, adaptint=15, updatesigma=1), prob, nchains=65, chain_id0=2)
    L = e.L
    dp, lp = C.POINTER(C.c_double), C.POINTER(C.c_int64)
    out = np.full(5 * 32, 7.0)
    cnt = np.full(5 * 32 * 2, 7, dtype=np.int64)
    ranks = np.zeros(32, dtype=np.int64)
    x = np.zeros(5 * 32)
    op, cp, rp, xp = out.ctypes.data_as(dp), cnt.ctypes.data_as(lp), ranks.ctypes.data_as(lp), x.ctypes.data_as(dp)
    dev = C.c_void_p(8)                                         # refused before the pointer is looked at

    def all_refused(s0, ns, nr, what):
        for rc in (L.mcmcx_samples_order_stats(e.h, s0, ns, nr, rp, op), L.mcmcx_samples_order_stats_dev(e.h, s0, ns, nr, rp, dev),
                   L.mcmcx_samples_counts(e.h, s0, ns, nr, xp, cp), L.mcmcx_samples_counts_dev(e.h, s0, ns, nr, xp, dev),
                   L.mcmcx_samples_quantiles(e.h, s0, ns, min(nr, 16) if nr <= 32 else nr, xp, op)):
            assert rc == -50 and len(L.mcmcx_last_error()) > 0, (what, s0, ns, nr, rc)

    e.set_samples(1, 3, 5)
    all_refused(0, 1, 2, "before init")
    assert b"inited" in L.mcmcx_last_error()
    e.init()
    e.run()
    before = _bits(e.samples()[1])
    assert e.samples_kept()[0] == 5
    for s0, ns in ((0, 0), (0, -4), (-1, 2), (2, 4), (0, 6), (5, 1), (2 ** 31 - 1, 1), (1, 2 ** 31 - 1)):
        all_refused(s0, ns, 2, "window")
    n = 5 * 65
    for bad in (n, -1, 2 ** 40):
        ranks[:] = 0
        ranks[1] = bad
        for rc in (L.mcmcx_samples_order_stats(e.h, 0, 5, 2, rp, op), L.mcmcx_samples_order_stats_dev(e.h, 0, 5, 2, rp, dev)):
            assert rc == -50 and b"rank" in L.mcmcx_last_error(), bad
    ranks[:] = 0
    for nr in (0, 33):
        all_refused(0, 5, nr, "nr")
    assert L.mcmcx_samples_quantiles(e.h, 0, 5, 17, xp, op) == -50 and b"at most 16" in L.mcmcx_last_error()
    x[0] = 1.5
    assert L.mcmcx_samples_quantiles(e.h, 0, 5, 1, xp, op) == -50 and b"probability" in L.mcmcx_last_error()
    x[0] = 0.0
    assert L.mcmcx_samples_order_stats_dev(e.h, 0, 5, 2, rp, None) == -50 and L.mcmcx_samples_counts_dev(e.h, 0, 5, 2, xp, None) == -50
    assert np.all(out == 7.0) and np.all(cnt == 7)
    assert np.array_equal(_bits(e.samples()[1]), before)
    _check_window(e, 0, 5, 1)                                   # still usable
    _check_window(e, 1, 4, 2)
    assert np.array_equal(_bits(e.samples()[1]), before)        # and a select writes nothing into the ring either
    e.close()
    e = engine_from_problem(dict(nsimu=40, adaptint=15, updatesigma=1), prob, nchains=65, chain_id0=2)
    e.init()
    e.run()
    all_refused(0, 1, 2, "sampling off")
    assert b"no samples are kept" in L.mcmcx_last_error()
    assert np.all(out == 7.0) and np.all(cnt == 7)
    e.close()
