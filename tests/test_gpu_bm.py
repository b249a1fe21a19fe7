"""The sample store's batch-means covariance on the f64 matrix cores (mcmcx_samples_cov_bm / _dev, include/mcmcx.h) and its finishes on a run.

The definition is sums in a fixed order, so the whole vector is compared on raw bits with the restatement (tests/bm_ref.py on tests/cov_ref.py:
libm's fma through ctypes, about 1e6 per second -- every case says its count, lanes x batches x pairs).  Through mcmcx_debug_samples_cov_bm,
which runs the same kernels on a caller's array: data over forty decades, some seeds with +-inf and NaN (NaNs are compared as NaNs,
everything else on bits), chain counts around a tile and at 66 tiles, windows with a remainder, of one batch and of one sample per batch,
field counts on both sides of the block edges of form A and into form B, form B at 203 fields, a given shift -- and at batch = 1 the bits of
mcmcx_debug_samples_cov of the same array, the shipped covariance.  Through a run: windows of a whole and of a wrapped ring, the three-column
target, the host, the device and the torch form, the run unmoved, the refusals, two engines adding up, and the two finishes on a Gaussian
target."""
import ctypes as C

import numpy as np
import pytest

import bm_ref
import cov_ref
from test_gpu_samples import SWITCHES, _bits, _cols3, _engine, _final, _gauss, _same_final

pytestmark = pytest.mark.gpu
DP = C.POINTER(C.c_double)
WINDOWS = ((5, 1), (7, 2), (8, 8), (9, 4), (6, 6))             # (ns, batch): a remainder (7, 2), (9, 4); nb = 1 and batch = ns (8, 8), (6, 6)


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


def _debug(X, batch, shift=None):
    """The batch-means vector of X through the debug entry; batch = None: mcmcx_debug_samples_cov's cov vector"""
    from mcmcf90_amd import _lib
    L = _lib.load()
    ns, nf, nch = X.shape
    X = np.ascontiguousarray(X, dtype=np.float64)
    sh = None if shift is None else np.ascontiguousarray(shift, dtype=np.float64)
    out = np.full(cov_ref.vec_len(nf), 7.0)
    if batch is None:
        rc = L.mcmcx_debug_samples_cov(0, nch, nf, ns, _dp(X), _dp(sh), _dp(out))
    else:
        rc = L.mcmcx_debug_samples_cov_bm(0, nch, nf, ns, batch, _dp(X), _dp(sh), _dp(out))
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


@pytest.mark.parametrize("nch", [1, 63, 64, 65, 583, 4163])
def test_bits_over_chain_counts_and_windows(nch):
    """10 fields, 55 pairs.  Up to 65 chains every window of WINDOWS with and without +-inf and NaN (128 lanes x 5 batches x 55 = 3.5e4 fma at
    the most); 583 chains (640 lanes) every window once, 12 batches in all: 4.2e5; 4163 chains -- 66 tiles, a second level of the tree --
    the window (9, 4): 4224 x 2 x 55 = 4.6e5.  The entry's NaN padding of the last tile must not show."""
    windows = WINDOWS if nch < 4163 else ((9, 4),)
    for k, (ns, batch) in enumerate(windows):
        for seed, specials in ((nch + k, 0), (nch + 100 + k, 6)) if nch <= 65 else ((nch + k, 3 * (k % 2)),):
            X = _decades(seed, ns, 10, nch, specials)
            got, want = _debug(X, batch), bm_ref.bm_vector_ref(X, batch)
            assert got[0] == float((ns // batch) * nch) and np.array_equal(_bits(got[1:11]), _bits(X[0, :, 0]))
            _same(got, want, (nch, ns, batch, seed))
            if specials == 0:
                assert np.isfinite(got).all()


@pytest.mark.parametrize("nch", [1, 63, 64, 65, 583, 4163])
def test_batch_one_has_the_bits_of_the_covariance(nch):
    """batch = 1 against mcmcx_debug_samples_cov of the same array: no restatement in between, the shipped covariance's kernels on one side
    and bm_tile_kernel on the other.  ns = 5, 10 fields; with and without +-inf and NaN; a given shift too."""
    for seed, specials in ((nch, 0), (nch + 1, 6)):
        X = _decades(seed, 5, 10, nch, specials)
        a, b = _debug(X, 1), _debug(X, None)
        _same(a, b, (nch, seed))
        assert a[0] == b[0] == 5.0 * nch
        if specials == 0:
            assert np.array_equal(_bits(a), _bits(b))
    sh = np.random.default_rng(nch).normal(size=10) * 1e3
    assert np.array_equal(_bits(_debug(X[:, :, :], 1, sh)[:11]), _bits(_debug(X, None, sh)[:11]))
    _same(_debug(X, 1, sh), _debug(X, None, sh), (nch, "given shift"))


@pytest.mark.parametrize("nf", [1, 15, 16, 47, 48, 63, 64, 65])
def test_bits_over_field_counts(nf):
    """65 chains (two tiles, the second with one chain), ns = 6, batch = 3: 128 lanes x 2 x 2145 pairs = 5.5e5 fma at 65 fields.  With the row
    of ones 15 fields fill one block, 16 open the second, 47 / 48 the fourth, 63 are the last form A takes, 64 and 65 go to form B.  And
    batch = 1 against the covariance at the same field count."""
    X = _decades(100 + nf, 6, nf, 65, specials=(4 if nf % 2 else 0))
    _same(_debug(X, 3), bm_ref.bm_vector_ref(X, 3), nf)
    _same(_debug(X, 1), _debug(X, None), (nf, "batch 1"))


def test_bits_of_form_b_at_203_fields():
    """65 chains, ns = 5, batch = 2 (two batches and a remainder).  Bit-exact: all pairs with j or k in the last block (fields 192 .. 202), the
    block-diagonal pairs of the first and of a middle block, 300 random pairs -- 2.8e3 pairs x 128 lanes x 2 = 7.1e5 fma.  Every remaining
    pair against the longdouble reference within the derived bound, so no pair is left out; and batch = 1 against the covariance."""
    nf = 203
    X = _decades(203, 5, nf, 65)
    got = _debug(X, 2)
    J, K = cov_ref.all_pairs(nf)
    rng = np.random.default_rng(7)
    pick = (K >= 192) | ((J < 16) & (K < 16)) | ((J >= 96) & (J < 112) & (K >= 96) & (K < 112))
    pick[rng.choice(J.size, 300, replace=False)] = True
    want = bm_ref.bm_vector_ref(X, 2, pairs=(J[pick], K[pick]))
    head = np.arange(1 + 2 * nf)
    assert got[0] == 2.0 * 65
    _same(got, want, "n, shift, S", only=head)
    _same(got, want, "picked pairs", only=1 + 2 * nf + np.flatnonzero(pick))
    S, G, bS, bG = bm_ref.longdouble_ref(X, 2)
    assert np.all(np.abs(got[1 + nf:1 + 2 * nf].astype(np.longdouble) - S) <= bS)
    err = np.abs(got[1 + 2 * nf:].astype(np.longdouble) - G)
    assert np.all(err <= bG), float((err / bG).max())
    assert np.array_equal(_bits(_debug(X, 1)), _bits(_debug(X, None)))


def test_a_given_shift_against_the_default():
    """The default shift handed in gives the same bits, another one the restatement's."""
    X = _decades(6, 7, 17, 130)                                 # 192 lanes x 3 x 153 = 8.8e4 fma, twice
    a = _debug(X, 2)
    _same(a, bm_ref.bm_vector_ref(X, 2), "default shift")
    assert np.array_equal(_bits(_debug(X, 2, X[0, :, 0].copy())), _bits(a))
    sh = np.random.default_rng(6).normal(size=17) * 1e3
    b = _debug(X, 2, sh)
    _same(b, bm_ref.bm_vector_ref(X, 2, sh), "given shift")
    assert np.array_equal(_bits(b[1:18]), _bits(sh)) and not np.array_equal(_bits(b[18:]), _bits(a[18:]))


# ---------------------------------------------------------------- through a run
def _check(e, batch, s0, ns, shift=None):
    """Host, device and torch form against the restatement of the same window; returns the vector."""
    import torch
    _, X = e.samples(s0, ns, layout=1)                          # [ns][nfields][nchains]
    want = bm_ref.bm_vector_ref(X, batch, shift)
    got = e.samples_cov_bm_stats(batch, s0, ns, shift)
    what = (e.nchains, X.shape[1], batch, s0, ns, shift is not None)
    assert got.shape == want.shape == (e.L.mcmcx_samples_cov_len(e.h),), what
    _same(got, want, what)
    assert got[0] == float((X.shape[0] // batch) * e.nchains)
    t = e.samples_cov_bm_stats_torch(batch, s0, ns, shift)
    assert t.is_cuda and str(t.dtype) == "torch.float64"
    assert np.array_equal(_bits(t.cpu().numpy()), _bits(got)), (what, "torch form")
    d = torch.full((got.size,), 7.0, dtype=torch.float64, device=t.device)
    sh = None if shift is None else np.ascontiguousarray(shift, dtype=np.float64)
    assert e.L.mcmcx_samples_cov_bm_dev(e.h, int(s0), int(X.shape[0]), int(batch), _dp(sh), C.c_void_p(d.data_ptr())) == 0
    e.sync()
    assert np.array_equal(_bits(d.cpu().numpy()), _bits(got)), (what, "device form")
    return got


def _shape_engine(nch, prob, capacity, nsimu=70, **kw):
    from mcmcf90_amd import engine_from_problem
    e = engine_from_problem(dict(dict(nsimu=nsimu, adaptint=15, updatesigma=1), **kw), prob, nchains=nch, chain_id0=2)
    e.set_samples(1, 1, capacity)
    e.init()
    e.run()
    return e


def test_bits_of_windows_of_a_whole_and_a_wrapped_ring():
    """npar 7 (10 fields) at 583 chains: 640 lanes x 55 pairs x (5 + 2 + 1) batches = 2.8e5 fma over the whole ring's windows, then 640 x 55 x
    (4 + 3 + 1) across the wrap; batch = 1 is the covariance of the same window."""
    prob = _gauss(7, 27, sigma2=0.7, nobs=9)
    e = _shape_engine(583, prob, 70)
    assert e.samples_kept()[:2] == (70, 1)
    shift = np.random.default_rng(1).normal(size=10) * 0.3
    _check(e, 4, 0, 20)
    _check(e, 8, 3, 20, shift)                                  # a remainder of four
    _check(e, 20, 50, 20)
    assert np.array_equal(_bits(e.samples_cov_bm_stats(1, 3, 20, shift)), _bits(e.samples_cov_stats(3, 20, shift)))
    e.close()
    e = _shape_engine(583, prob, 20)                            # retained sample s sits in slot (10 + s) % 20: the wrap is between 9 and 10
    assert e.samples_kept()[:2] == (20, 51)
    _check(e, 2, 5, 9)                                          # batches 5-6, 7-8, 9-10 (across the wrap), 11-12
    _check(e, 4, 7, 12, shift)
    _check(e, 20, 0, 20)
    assert np.array_equal(_bits(e.samples_cov_bm_stats(1, 5, 9)), _bits(e.samples_cov_stats(5, 9)))
    e.close()


def test_bits_of_the_three_column_target():
    """11 fields, the E.ssv / E.s2v rows: 192 lanes x 6 x 66 = 7.6e4 fma; sspri is constant (a flat prior): selected it warns, left out the
    finishes are finite."""
    e = _shape_engine(130, _cols3(), 70)
    assert e.samples_kept()[3] == 11
    _check(e, 5, 40, 30)
    r = e.samples_mess(40, 30, fields="all")
    assert r["warn"] == 1 and np.isnan(r["mess"]) and r["batch"] == 5 and len(r["fields"]) == 11
    keep = [j for j in range(11) if j != 7]
    r = e.samples_mess(40, 30, fields=keep)
    m = e.samples_mpsrf(40, 30, fields=keep)
    assert r["warn"] == 0 and np.isfinite(r["mess"]) and r["n"] == 30 * 130 and "sspri" not in r["fields"]
    assert m["warn"] == 0 and np.isfinite(m["mpsrf"]) and m["M"] == 260 and m["n_h"] == 15
    e.close()


def test_the_run_is_unmoved(monkeypatch):
    """Two engines cut at the same iterations, one calling the batch-means covariance mid-run (its scratch allocated then)."""
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("MCMCX_GROUP", "0")
    chains = [0, 63, 64, 129]
    finals = []
    for call in (True, False):
        e = _engine("lane_am", None, (3, 7, None))
        assert e.run(50) == 0
        if call:
            a = e.samples_cov_bm_stats(2)
        assert e.run(90) == 0
        if call:
            b = e.samples_cov_bm_stats(3, 1, 8, shift=np.zeros(10))
            t = e.samples_cov_bm_stats_torch(1, 0, None)
            assert a.size == b.size == t.numel() == 76
            s = e.samples_summary(multivariate=True)
            assert np.isfinite(s["mess"]) and np.isfinite(s["mpsrf"]) and s["ess_bm"].shape == (7,)
        assert e.run() == 0
        finals.append((_final(e, chains, False), _bits(e.samples()[1])))
        e.close()
    _same_final(finals[0][0], finals[1][0], "a batch-means covariance in the middle of the run")
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
    assert L.mcmcx_samples_cov_bm(e.h, 0, 4, 2, None, p) == -55 and b"inited" in L.mcmcx_last_error()
    e.init()
    e.run()
    before = _bits(e.samples()[1])
    assert e.samples_kept()[0] == 5
    cases = [(s0, ns, 1) for s0, ns in ((0, 0), (0, -4), (-1, 4), (2, 4), (0, 6), (5, 1), (2 ** 31 - 1, 4), (1, 2 ** 31 - 1))]
    cases += [(0, 4, 0), (0, 4, 5), (0, 4, -1), (1, 4, 2 ** 31 - 1), (0, 5, 6)]
    for s0, ns, batch in cases:
        for fn, out in ((L.mcmcx_samples_cov_bm, p), (L.mcmcx_samples_cov_bm_dev, C.c_void_p(8))):     # refused before the pointer is looked at
            rc = fn(e.h, s0, ns, batch, None, out)
            assert rc == -55 and len(L.mcmcx_last_error()) > 0, (s0, ns, batch, rc)
    assert L.mcmcx_samples_cov_bm(e.h, 0, 4, 2, None, None) == -55 and b"null output" in L.mcmcx_last_error()
    assert L.mcmcx_samples_cov_bm_dev(e.h, 0, 4, 2, None, None) == -55
    assert np.all(buf == 7.0)
    assert np.array_equal(_bits(e.samples()[1]), before)
    _check(e, 2, 0, 5)                                          # still usable
    _check(e, 1, 4, 1)
    _check(e, 5, 0, 5)
    assert np.array_equal(_bits(e.samples()[1]), before)        # and the reader writes nothing into the ring either
    e.close()
    e = engine_from_problem(dict(nsimu=40, adaptint=15, updatesigma=1), prob, nchains=65, chain_id0=2)
    e.init()
    e.run()
    assert L.mcmcx_samples_cov_bm(e.h, 0, 4, 2, None, p) == -55 and b"no samples are kept" in L.mcmcx_last_error()
    e.close()


def test_vectors_of_two_half_engines_add_up():
    """Chains 0 .. 127 and 128 .. 255 in two engines (chain_id0 0 and 128) with one shift and one batch: the sum of their vectors against the
    longdouble reference of one engine that runs all 256, within the forward bound; and the finishes of the sums are the whole's."""
    from mcmcf90_amd import engine_from_problem
    from mcmcf90_amd.engine import samples_mess, samples_mpsrf
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
    shift = X[0, :, 0].copy()
    wc, wb5, wb20 = whole.samples_cov_stats(0, 40, shift), whole.samples_cov_bm_stats(5, 0, 40, shift), whole.samples_cov_bm_stats(20, 0, 40, shift)
    whole.close()
    parts = []
    for id0 in (0, 128):
        e = eng(128, id0)
        parts.append((e.samples_cov_stats(0, 40, shift), e.samples_cov_bm_stats(5, 0, 40, shift), e.samples_cov_bm_stats(20, 0, 40, shift)))
        e.close()
    tot = [a + b for a, b in zip(*parts)]
    for v in tot:
        v[1:11] = shift
    assert tot[0][0] == 40 * 256 and tot[1][0] == 8 * 256 and tot[2][0] == 2 * 256
    for batch, v in ((5, tot[1]), (20, tot[2])):
        S, G, bS, bG = bm_ref.longdouble_ref(X, batch, shift)
        assert np.all(np.abs(v[11:21].astype(np.longdouble) - S) <= bS) and np.all(np.abs(v[21:].astype(np.longdouble) - G) <= bG)
    sel = list(range(7)) + [7, 9]                               # theta, ss, sigma2 (sspri is constant)
    a, b = samples_mess(tot[0], tot[1], 10, 5, sel), samples_mess(wc, wb5, 10, 5, sel)
    assert a["warn"] == b["warn"] == 0 and abs(a["mess"] - b["mess"]) <= 1e-9 * b["mess"]
    a, b = samples_mpsrf(tot[0], tot[2], 10, 20, sel), samples_mpsrf(wc, wb20, 10, 20, sel)
    assert a["warn"] == b["warn"] == 0 and a["M"] == 512 and abs(a["mpsrf"] - b["mpsrf"]) <= 1e-9 * b["mpsrf"]


def test_mess_and_mpsrf_of_a_gaussian_target_run():
    """583 chains on a correlated Gaussian, forty samples, every tenth iteration from 200 on.  Asserted is what is exact: finiteness, mpsrf
    at least every parameter's split-R-hat (the Rayleigh quotient at e_j; mpsrf is samples_summary's rhat for one field within 1e-9), the
    dict's bookkeeping -- not mess <= n, which does not hold in general.  The values are printed (DESIGN.md 5i-2 records them)."""
    from mcmcf90_amd import engine_from_problem
    d = 4
    rng = np.random.default_rng(12)
    A = rng.standard_normal((d, d))
    S = A @ A.T / d + 0.5 * np.eye(d)
    prob = dict(kind="gauss", npar=d, par0=np.array([0.3, -0.2, 0.1, 0.0]), cmat0=(2.4 ** 2 / d) * S, mu=np.array([0.5, -1.0, 0.25, 2.0]),
                lam=np.linalg.inv(S))
    e = engine_from_problem(dict(nsimu=600, adaptint=100, updatesigma=0), prob, nchains=583, chain_id0=0)
    e.set_samples(200, 10, 40)
    e.init()
    assert e.run() == 0 and e.samples_kept()[0] == 40
    s = e.samples_summary(maxlag=8, multivariate=True)
    plain = e.samples_summary(maxlag=8)
    assert set(s) - set(plain) == {"mess", "mess_batch", "ess_bm", "mpsrf"}
    for k in plain:
        assert np.array_equal(np.asarray(s[k]), np.asarray(plain[k])) or np.array_equal(_bits(s[k]), _bits(plain[k])), k
    r = e.samples_mess()
    m = e.samples_mpsrf()
    print("mess %.1f of n %d at batch %d, ess_bm %s, ess %s; mpsrf %.5f, rhat %s" % (r["mess"], r["n"], r["batch"], np.round(r["ess_bm"]).tolist(),
          np.round(s["ess"][:d]).tolist(), m["mpsrf"], np.round(s["rhat"][:d], 5).tolist()))
    assert r["warn"] == 0 and r["batch"] == 6 and r["n"] == 36 * 583 and r["fields"] == ["theta[%d]" % i for i in range(d)]
    assert np.isfinite(r["mess"]) and r["mess"] > 0 and np.isfinite(r["ess_bm"]).all() and abs(s["mess"] - r["mess"]) <= 1e-9 * r["mess"]
    assert m["warn"] == 0 and np.isfinite(m["mpsrf"]) and m["M"] == 2 * 583 and m["n_h"] == 20 and abs(s["mpsrf"] - m["mpsrf"]) <= 1e-9
    assert m["mpsrf"] >= s["rhat"][:d].max() * (1.0 - 1e-12)
    for j in range(d):
        one = e.samples_mpsrf(fields=[j])
        assert abs(one["mpsrf"] - s["rhat"][j]) <= 1e-9, (j, one["mpsrf"], s["rhat"][j])
    odd = e.samples_mpsrf(0, 39)                                # an odd window loses its last sample
    assert odd["n_h"] == 19 and np.isfinite(odd["mpsrf"])
    e.close()
