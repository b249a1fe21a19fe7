"""The sample store's convergence summary, reduced on the device (mcmcx_samples_stats / _dev / mcmcx_samples_diag, include/mcmcx.h).

The definition is sums in a fixed order, so the stats vector is compared on raw bits with the numpy restatement (tests/diag_ref.py) fed from
Engine.samples(layout=1) of the same ring, and the table at 1e-13 (the finish is the same IEEE operations on both sides; log10 is libm's).
Shapes: chain counts around a tile and at 66 tiles (a second level of moments_tree_kernel), field counts that are and are not multiples of the
four rows a block takes, windows of 4, 5 (middle dropped) and 9 samples, the whole ring, s0 > 0, a wrapped ring with the window across the
wrap, maxlag on each side of every instantiation's bound (W = 1, 9, 17, 33 hold K <= 0, 8, 16, 32) and larger than n_h - 1, shift given and
NULL, and stores written by different kernel families.  Then: the run is unmoved, the refusals, and stats vectors of two engines add up."""
import ctypes as C

import numpy as np
import pytest

import diag_ref
from test_gpu_samples import FORMS, SWITCHES, _bits, _cols3, _engine, _final, _gauss, _same_final

pytestmark = pytest.mark.gpu
RTOL = 1e-13
NSIMU = 70                                                      # first = 1, thin = 1: seventy kept iterations


def _shape_engine(nch, prob, capacity, **kw):
    from mcmcf90_amd import engine_from_problem
    e = engine_from_problem(dict(dict(nsimu=NSIMU, adaptint=15, updatesigma=1), **kw), prob, nchains=nch, chain_id0=2)
    e.set_samples(1, 1, capacity)
    e.init()
    e.run()
    return e


def _check(e, s0, ns, maxlag, shift=None, torch_too=True):
    """Host and device form against the restatement of the same window; returns the stats vector."""
    from mcmcf90_amd.engine import samples_diag
    _, X = e.samples(s0, ns, layout=1)                          # [ns][nfields][nchains]
    nf = X.shape[1]
    want = diag_ref.stats_ref(X, maxlag, shift)
    got = e.samples_stats(s0, ns, maxlag, shift)
    what = (e.nchains, nf, s0, ns, maxlag, shift is not None)
    assert got.shape == want.shape == (e.L.mcmcx_samples_stats_len(e.h, maxlag),), what
    bad = np.flatnonzero(_bits(got) != _bits(want))
    assert bad.size == 0, (what, bad[:8], got[bad[:8]], want[bad[:8]])
    nh = ns // 2
    K = min(maxlag, nh - 1)
    assert (got[0], got[1], got[2]) == (2.0 * e.nchains, nh, K)
    per = got[3:].reshape(nf, maxlag + 4)
    assert np.array_equal(_bits(per[:, 4 + K:]), np.zeros((nf, maxlag - K), dtype=np.uint64)), (what, "slots beyond K are +0.0")
    if shift is None:
        assert np.array_equal(_bits(per[:, 0]), _bits(X[0, :, 0])), (what, "shift")
    if torch_too:
        t = e.samples_stats_torch(s0, ns, maxlag, shift)
        assert t.is_cuda and str(t.dtype) == "torch.float64"
        assert np.array_equal(_bits(t.cpu().numpy()), _bits(got)), (what, "device form")
    table, ref = samples_diag(got, nf, maxlag), diag_ref.finish_ref(want, nf, maxlag)
    assert np.array_equal(np.isnan(table), np.isnan(ref)), what
    assert np.allclose(table, ref, rtol=RTOL, atol=0.0, equal_nan=True), what
    return got


# (s0, ns, maxlag, shift given) on a ring that holds all seventy kept iterations
FULL_CASES = [(0, 70, 32, False), (0, 70, 17, True), (0, 70, 16, False), (0, 70, 9, False), (0, 70, 8, True), (0, 70, 7, False),
              (0, 70, 1, False), (0, 70, 0, True), (0, 4, 5, False), (0, 5, 2, True), (3, 9, 32, False), (61, 9, 3, True), (1, 69, 32, True)]
# ... on a ring of twenty under seventy kept iterations: retained sample s sits in slot (10 + s) % 20, the wrap is between 9 and 10
WRAP_CASES = [(0, 20, 8, False), (0, 20, 32, True), (5, 9, 3, False), (7, 12, 16, True), (16, 4, 0, False), (9, 5, 1, False)]


def _shift_for(e, seed):
    nf = e.samples_kept()[3]
    return np.random.default_rng(seed).normal(size=nf) * 0.3


def _run_cases(e, cases, torch_every=3):
    for k, (s0, ns, maxlag, given) in enumerate(cases):
        _check(e, s0, ns, maxlag, _shift_for(e, k) if given else None, torch_too=(k % torch_every == 0))


@pytest.mark.parametrize("nch", [1, 63, 64, 65, 583, 4163])
def test_stats_bits_over_chain_counts(nch):
    """npar 7 (nfields 10, not a multiple of four); 4163 chains are 66 tiles: two levels of moments_tree_kernel."""
    prob = _gauss(7, 27, sigma2=0.7, nobs=9)
    e = _shape_engine(nch, prob, NSIMU)
    assert e.samples_kept()[:2] == (NSIMU, 1)
    _run_cases(e, FULL_CASES)
    e.close()
    e = _shape_engine(nch, prob, 20)
    assert e.samples_kept()[:2] == (20, 51)
    _run_cases(e, WRAP_CASES)
    e.close()


@pytest.mark.parametrize("name,nch", [("npar1", 65), ("npar1", 4163), ("cols3", 130), ("npar62", 65), ("npar62", 583)])
def test_stats_bits_over_field_counts(name, nch):
    """nfields 4 (one block row), 11 (the three-column target: E.ssv / E.s2v rows), 65 (seventeen block rows, the last with one field)."""
    prob = {"npar1": _gauss(1, 21, sigma2=0.7, nobs=9), "cols3": _cols3(), "npar62": _gauss(62, 82, sigma2=0.7, nobs=9)}[name]
    nf = {"npar1": 4, "cols3": 11, "npar62": 65}[name]
    e = _shape_engine(nch, prob, NSIMU)
    assert e.samples_kept()[3] == nf
    _run_cases(e, FULL_CASES[::2] if name == "npar62" else FULL_CASES)
    e.close()
    e = _shape_engine(nch, prob, 20)
    _run_cases(e, WRAP_CASES)
    e.close()


@pytest.mark.parametrize("name", ["lane_am", "ram_group", "group_quad", "pooled_mfma", "host"])
def test_stats_bits_of_stores_written_by_other_kernel_families(name, monkeypatch):
    """The summary does not depend on the family, but the store's rows come from different writers."""
    env, ckw, _, nch, kernel, _ = FORMS[name]
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    e = _engine(name, None, (3, 2, 24))                         # iterations 3, 5, ...: nsimu 120 keeps 59, nsimu 60 keeps 29; a ring of 24
    assert e.run() == 0 and e.last_kernel() == kernel
    n = e.samples_kept()[0]
    assert n == 24
    _run_cases(e, [(0, 24, 16, False), (2, 21, 9, True), (0, 24, 0, False), (11, 5, 1, True)], torch_every=2)
    e.close()


def test_summary_names_its_rows():
    e = _shape_engine(65, _cols3(), NSIMU)
    s = e.samples_summary(s0=10, ns=40, maxlag=8)
    assert s["fields"] == ["theta[0]", "theta[1]", "theta[2]", "theta[3]", "ss[0]", "ss[1]", "ss[2]", "sspri", "sigma2[0]", "sigma2[1]",
                           "sigma2[2]"]
    assert list(s["iterations"]) == list(range(11, 51))
    _, X = e.samples(10, 40, layout=1)
    ref = diag_ref.summary_ref(X, 8)
    for j, k in enumerate(diag_ref.COLUMNS):
        assert s[k].shape == (11,) and np.allclose(s[k], ref[:, j], rtol=RTOL, atol=0.0, equal_nan=True), k
    assert np.allclose(s["mean"], X[np.r_[0:20, 20:40]].mean(axis=(0, 2)), rtol=1e-10)
    e.close()


def test_the_run_is_unmoved(monkeypatch):
    """Two engines cut at the same iterations, one calling samples_stats twice mid-run (growing its scratch the second time)."""
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("MCMCX_GROUP", "0")
    chains = [0, 63, 64, 129]
    finals = []
    for summarise in (True, False):
        e = _engine("lane_am", None, (3, 7, None))
        assert e.run(50) == 0
        if summarise:
            a = e.samples_stats(0, None, 2)
        assert e.run(90) == 0
        if summarise:
            b = e.samples_stats(1, 8, 32, shift=np.zeros(10))
            t = e.samples_stats_torch(0, None, 0)
            assert a.size == 3 + 10 * 6 and b.size == 3 + 10 * 36 and t.numel() == 3 + 10 * 4
        assert e.run() == 0
        finals.append((_final(e, chains, False), _bits(e.samples()[1])))
        e.close()
    _same_final(finals[0][0], finals[1][0], "a summary in the middle of the run")
    assert np.array_equal(finals[0][1], finals[1][1])


def test_refusals_launch_nothing():
    from mcmcf90_amd import engine_from_problem
    prob = _gauss(2, 22, sigma2=0.7, nobs=9)
    e = engine_from_problem(dict(nsimu=40, adaptint=15, updatesigma=1), prob, nchains=65, chain_id0=2)
    L = e.L
    n = 3 + 5 * 8
    buf = np.full(n, 7.0)
    p = buf.ctypes.data_as(C.POINTER(C.c_double))
    e.set_samples(1, 3, 5)
    assert L.mcmcx_samples_stats(e.h, 0, 4, 4, None, p) == -49 and b"inited" in L.mcmcx_last_error()
    assert L.mcmcx_samples_stats_len(e.h, 4) == n
    for bad in (-1, 33):
        assert L.mcmcx_samples_stats_len(e.h, bad) == -49
    e.init()
    e.run()
    before = _bits(e.samples()[1])
    assert e.samples_kept()[0] == 5
    for s0, ns, maxlag in ((0, 3, 4), (0, 0, 4), (0, -4, 4), (-1, 4, 4), (2, 4, 4), (0, 6, 4), (5, 4, 4), (0, 4, -1), (0, 4, 33),
                           (2 ** 31 - 1, 4, 4), (1, 2 ** 31 - 1, 4)):
        for fn, out in ((L.mcmcx_samples_stats, p), (L.mcmcx_samples_stats_dev, C.c_void_p(8))):     # refused before the pointer is looked at
            rc = fn(e.h, s0, ns, maxlag, None, out)
            assert rc == -49 and len(L.mcmcx_last_error()) > 0, (s0, ns, maxlag, rc)
    assert L.mcmcx_samples_stats(e.h, 0, 4, 4, None, None) == -49 and b"null output" in L.mcmcx_last_error()
    assert L.mcmcx_samples_stats_dev(e.h, 0, 4, 4, None, None) == -49
    assert np.all(buf == 7.0)
    assert np.array_equal(_bits(e.samples()[1]), before)
    _check(e, 0, 5, 4)                                          # still usable
    _check(e, 1, 4, 0)
    assert np.array_equal(_bits(e.samples()[1]), before)        # and a summary writes nothing into the ring either
    e.close()
    e = engine_from_problem(dict(nsimu=40, adaptint=15, updatesigma=1), prob, nchains=65, chain_id0=2)
    e.init()
    e.run()
    assert L.mcmcx_samples_stats(e.h, 0, 4, 4, None, p) == -49 and b"no samples are kept" in L.mcmcx_last_error()
    e.close()


def test_stats_vectors_of_two_engines_add_up():
    """Chains 0 .. 127 and 128 .. 255 in two engines (chain_id0 0 and 128) with a common shift: the sum of their stats vectors, finished by
    samples_diag, against the restatement of one engine that runs all 256 -- another summation order over the chains, so 1e-12, not bits."""
    from mcmcf90_amd import engine_from_problem
    from mcmcf90_amd.engine import samples_diag
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
        parts.append(_check(e, 0, 40, 16, shift))
        e.close()
    total = parts[0] + parts[1]
    total[1:3] = parts[0][1:3]                                  # n_h and K are the window's, not sums
    per = total[3:].reshape(10, 20)
    per[:, 0] = shift
    assert total[0] == 512.0
    table, ref = samples_diag(total, 10, 16), diag_ref.summary_ref(X, 16, shift)
    assert np.array_equal(table[:, 7], ref[:, 7])
    # sspri is constant (this target has no prior) and equal to its shift: every sum is exactly zero on both sides, R-hat and ESS are 0 / 0
    const = [s == "sspri" for s in ("theta",) * 7 + ("ss", "sspri", "sigma2")]
    assert np.array_equal(np.isnan(table), np.isnan(ref)) and not np.isnan(table[np.logical_not(const)]).any()
    assert np.allclose(table, ref, rtol=1e-12, atol=0.0, equal_nan=True), np.nanmax(np.abs(table / ref - 1.0))
