"""The summary of an elementwise function of the sample store, reduced on the device (mcmcx_samples_stats_of / _dev / mcmcx_debug_samples_stats,
include/mcmcx.h): tail ESS, folded split-R-hat, the MCSE of the sd.

The definition is the summary's own sums of u(x), so the stats vector is compared on raw bits with the numpy restatement
(tests/diag_xf_ref.py).  The debug entry lays a caller's array out as a store: chain counts around a tile, at ten tiles and at 66 (a second
level of moments_tree_kernel), five fields (not a multiple of the four rows a block takes), windows of 4, 5 (middle dropped), 9 and 70
samples, maxlag on each side of every instantiation's bound, shift given and NULL, and the values a run cannot put into the ring.  Then an
engine's ring, whole and wrapped: bits, the identity, the indicator's exact count, the tail summary, the refusals, the run unmoved and the
asynchronous forms back to back on the shared scratch."""
import ctypes as C

import numpy as np
import pytest

import diag_ref
import diag_xf_ref
import quant_ref
from diag_xf_ref import FOLD, IDENTITY, LE, SQUARE
from test_diag_xf_cpu import NAN_NEG, NAN_POS
from test_gpu_diag import NSIMU, _shape_engine
from test_gpu_samples import SWITCHES, _bits, _cols3, _engine, _final, _same_final

pytestmark = pytest.mark.gpu
RTOL = 1e-13
DP = C.POINTER(C.c_double)
KINDS = (LE, FOLD, SQUARE)
MAXLAGS = (0, 8, 9, 16, 17, 32)


def _dp(a):
    return None if a is None else a.ctypes.data_as(DP)


def _debug(X, maxlag, kind, a, shift=None):
    from mcmcf90_amd import _lib
    L = _lib.load()
    ns, nf, nch = X.shape
    X = np.ascontiguousarray(X, dtype=np.float64)
    a = None if a is None else np.ascontiguousarray(a, dtype=np.float64)
    sh = None if shift is None else np.ascontiguousarray(shift, dtype=np.float64)
    out = np.full(diag_ref.stats_len(nf, maxlag), 7.0)
    rc = L.mcmcx_debug_samples_stats(0, nch, nf, ns, _dp(X), maxlag, kind, _dp(a), _dp(sh), _dp(out))
    assert rc == 0, (rc, L.mcmcx_last_error())
    return out


def _same_bits(got, want, what):
    assert got.shape == want.shape, what
    bad = np.flatnonzero(_bits(got) != _bits(want))
    assert bad.size == 0, (what, bad[:8], got[bad[:8]], want[bad[:8]])


def _values(seed, ns, nf, nch):
    """Correlated along the window (so that the lag sums are no noise), a field each near and far from zero, a per chain: quantiles in the
    body and in the tails, one below every value (a constant indicator)."""
    rng = np.random.default_rng(seed)
    X = rng.normal(size=(ns, nf, nch))
    for i in range(1, ns):
        X[i] = 0.6 * X[i - 1] + 0.8 * X[i]
    X += np.array([0.0, 10.0, -3.0, 0.5, 1e3])[:nf, None]
    a = np.array([np.quantile(X[:, f], q) for f, q in zip(range(nf), (0.05, 0.5, 0.95, 0.3, 0.0))])
    a[4] -= 1.0
    return X, a


@pytest.mark.parametrize("nch", [1, 63, 65, 583])
@pytest.mark.parametrize("ns", [4, 5, 9, 70])
def test_debug_entry_bits_of_every_kind(nch, ns):
    """Every kind at every maxlag, with the shift given and NULL."""
    X, a = _values(1000 * ns + nch, ns, 5, nch)
    shift = np.random.default_rng(ns).normal(size=5) * 0.3
    for kind in KINDS:
        for maxlag in MAXLAGS:
            for given in (True, False):
                sh = shift if given else None
                got, want = _debug(X, maxlag, kind, a, sh), diag_xf_ref.stats_ref(X, kind, a, maxlag, sh)
                _same_bits(got, want, (nch, ns, kind, maxlag, given))
                if not given:
                    assert np.array_equal(_bits(got[3:].reshape(5, maxlag + 4)[:, 0]), _bits(diag_xf_ref.u_ref(X[:1, :, :1], kind, a).ravel()))


def test_debug_entry_bits_above_one_tree_level():
    """4163 chains are 66 tiles: two levels of moments_tree_kernel."""
    X, a = _values(4163, 9, 5, 4163)
    for kind, maxlag, given in ((LE, 3, False), (FOLD, 0, True), (SQUARE, 32, False)):
        sh = np.full(5, 0.25) if given else None
        _same_bits(_debug(X, maxlag, kind, a, sh), diag_xf_ref.stats_ref(X, kind, a, maxlag, sh), (kind, maxlag))


def _same(got, want, what):
    """NaNs where the restatement has NaNs, equal bits everywhere else."""
    assert got.shape == want.shape, what
    gn, wn = np.isnan(got), np.isnan(want)
    assert np.array_equal(gn, wn), (what, np.flatnonzero(gn != wn)[:8])
    bad = np.flatnonzero((_bits(got) != _bits(want)) & ~wn)
    assert bad.size == 0, (what, bad[:8], got[bad[:8]], want[bad[:8]])


# a_f for the adversarial arrays: fields 0 and 1 finite (every kind's bits are compared there), then an infinity, a NaN, an ordinary value
ADVERSARIAL_A = {"plus": [0.0, 5e-324, np.inf, NAN_POS, 0.7], "minus": [-0.0, -5e-324, -np.inf, NAN_NEG, -0.7]}


@pytest.mark.parametrize("sign", sorted(ADVERSARIAL_A))
def test_debug_entry_adversarial_values(sign):
    """+-0, +-inf, NaNs of both signs, denormals and values equal to a_f scattered over 65 chains and 9 samples; a_f itself a zero, a
    denormal, an infinity, a NaN and an ordinary value, of either sign (the key compare takes another path for an a_f with its sign set).
    The entry fills the 63 padding lanes with (positive) NaNs: under kind 1 with a = +NaN a kernel that counted them would show a sum of
    half means above what 65 chains allow."""
    nch, ns, nf = 65, 9, 5
    rng = np.random.default_rng(77)
    a = np.array(ADVERSARIAL_A[sign])
    special = [0.0, -0.0, np.inf, -np.inf, NAN_POS, NAN_NEG, 5e-324, -5e-324, 2.2250738585072009e-308, -2.2250738585072009e-308, 0.7, -0.7]
    finite = [v for v in special if np.isfinite(v)]
    X = rng.normal(size=(ns, nf, nch))
    for f in range(nf):
        pick = finite if f < 2 else special
        for _ in range(40):
            X[rng.integers(ns), f, rng.integers(nch)] = pick[rng.integers(len(pick))]
        X[rng.integers(ns), f, rng.integers(nch)] = a[f]
    X[1, 2, 5], X[2, 2, 6], X[1, 3, 7] = NAN_POS, NAN_NEG, NAN_NEG   # above +inf, below -inf, equal to the negative a_3: inside half 0
    zero = np.zeros(nf)
    for kind in KINDS:
        for maxlag in (0, 3, 32):
            for sh in (zero, None):
                got, want = _debug(X, maxlag, kind, a, sh), diag_xf_ref.stats_ref(X, kind, a, maxlag, sh)
                _same(got, want, (kind, maxlag, sh is None))
                assert not np.isnan(want[3:].reshape(nf, maxlag + 4)[:2]).any(), "the finite fields are compared on bits"
    got = _debug(X, 3, LE, a, zero)
    _same_bits(got, diag_xf_ref.stats_ref(X, LE, a, 3, zero), "kind 1 has no NaN to excuse")
    s1 = got[3:].reshape(nf, 7)[:, 1]                           # the sum over chains of the two half means, each k / 4
    assert np.all(s1 <= 2.0 * nch) and np.all(s1 >= 0.0), s1
    if sign == "plus":
        assert s1[3] == 2.0 * nch and 0.0 < s1[2] < 2.0 * nch, s1                  # everything <= +NaN; all but the +NaNs <= +inf
    else:
        assert 0.0 < s1[3] < s1[2] < 0.25 * nch, s1                                # only -NaNs <= -NaN; they and the -infs <= -inf


# ------------------------------------------------------------------ an engine's ring: cols3 (nfields 11), 130 chains
@pytest.fixture(scope="module")
def rings():
    """(whole, wrapped): a ring that holds all seventy kept iterations and one of twenty under them (retained sample s in slot
    (10 + s) % 20: windows across 9 | 10 straddle the wrap)."""
    whole, wrapped = _shape_engine(130, _cols3(), NSIMU), _shape_engine(130, _cols3(), 20)
    assert whole.samples_kept()[:2] == (NSIMU, 1) and wrapped.samples_kept()[:2] == (20, 51) and whole.samples_kept()[3] == 11
    yield whole, wrapped
    whole.close()
    wrapped.close()


def _engine_check(e, s0, ns, maxlag, kind, given, torch_too):
    _, X = e.samples(s0, ns, layout=1)
    a = e.samples_quantiles([0.05, 0.5, 0.95], s0, ns)[:, kind - 1]
    assert np.array_equal(_bits(a), _bits(quant_ref.quantiles_ref(X, [0.05, 0.5, 0.95])[:, kind - 1]))
    sh = np.random.default_rng(s0 + ns).normal(size=11) * 0.3 if given else None
    want = diag_xf_ref.stats_ref(X, kind, a, maxlag, sh)
    got = e.samples_stats_of(kind, a, s0, ns, maxlag, sh)
    _same_bits(got, want, (s0, ns, maxlag, kind, given))
    if torch_too:
        t = e.samples_stats_of_torch(kind, a, s0, ns, maxlag, sh)
        assert t.is_cuda and str(t.dtype) == "torch.float64"
        assert np.array_equal(_bits(t.cpu().numpy()), _bits(got)), (s0, ns, maxlag, kind, "device form")


def test_engine_bits_whole_and_wrapped_ring(rings):
    whole, wrapped = rings
    for k, (s0, ns, maxlag, given) in enumerate([(0, 70, 32, False), (0, 70, 8, True), (3, 9, 17, False), (1, 69, 16, True), (61, 9, 0, True)]):
        for kind in KINDS:
            _engine_check(whole, s0, ns, maxlag, kind, given, torch_too=(k + kind) % 3 == 0)
    for k, (s0, ns, maxlag, given) in enumerate([(0, 20, 8, False), (5, 9, 3, True), (7, 12, 16, False), (9, 5, 1, True)]):
        for kind in KINDS:
            _engine_check(wrapped, s0, ns, maxlag, kind, given, torch_too=(k + kind) % 2 == 0)


def test_identity_is_the_summary_itself(rings):
    for e, (s0, ns) in zip(rings, ((2, 40), (7, 12))):
        for maxlag, sh in ((0, None), (9, None), (32, np.linspace(-1.0, 1.0, 11))):
            plain = e.samples_stats(s0, ns, maxlag, sh)
            assert np.array_equal(_bits(e.samples_stats_of(IDENTITY, None, s0, ns, maxlag, sh)), _bits(plain)), (maxlag, "a = None")
            assert np.array_equal(_bits(e.samples_stats_of(IDENTITY, np.full(11, 0.5), s0, ns, maxlag, sh)), _bits(plain)), (maxlag, "a given")
            assert np.array_equal(_bits(e.samples_stats_of_torch(IDENTITY, None, s0, ns, maxlag, sh).cpu().numpy()), _bits(plain))


def test_the_indicator_counts_exactly(rings):
    """ns = 8 and a shift of zeros: S1 n_h is samples_counts' le over the window, exactly."""
    for e, s0 in zip(rings, (11, 6)):
        q = e.samples_quantiles([0.05, 0.5, 1.0], s0, 8)
        le = e.samples_counts(q, s0, 8)[:, :, 1]
        for k in range(3):
            st = e.samples_stats_of(LE, q[:, k], s0, 8, 3, np.zeros(11))
            assert np.array_equal(st[3:].reshape(11, 7)[:, 1] * 4.0, le[:, k].astype(np.float64)), (s0, k)
        assert np.all(le[:, 2] == 8 * 130)


def test_tail_summary_is_the_composition(rings):
    """Every new key against the same composition done with the restatements on samples(layout=1); the eight old keys unchanged."""
    from mcmcf90_amd.engine import DIAG_COLUMNS
    probs = [0.025, 0.5, 0.9]
    for e, (s0, ns, maxlag) in zip(rings, ((10, 40, 8), (3, 16, 16))):
        old, s = e.samples_summary(s0, ns, maxlag, probs=probs), e.samples_summary(s0, ns, maxlag, probs=probs, tail=True)
        assert set(s) == set(old) | {"ess_tail", "truncated_tail", "rhat_folded", "ess_sd", "mcse_sd", "ess_quantiles"}
        assert set(e.samples_summary(s0, ns, maxlag, tail=True)) == set(s) - {"probs", "quantiles", "ess_quantiles"}
        for k in DIAG_COLUMNS + ("quantiles", "probs", "iterations"):
            assert np.array_equal(_bits(s[k]), _bits(old[k])) if k != "iterations" else np.array_equal(s[k], old[k]), k
        assert s["fields"] == old["fields"]
        _, X = e.samples(s0, ns, layout=1)
        q = quant_ref.quantiles_ref(X, [0.05, 0.5, 0.95])
        plain = diag_ref.summary_ref(X, maxlag)
        assert np.array_equal(_bits(plain[:, 0]), _bits(s["mean"])), "the square's parameter is the table's mean"
        zero = np.zeros(11)
        lo, hi = (diag_xf_ref.summary_ref(X, LE, q[:, j], maxlag, zero) for j in (0, 2))
        fold, sq = diag_xf_ref.summary_ref(X, FOLD, q[:, 1], maxlag), diag_xf_ref.summary_ref(X, SQUARE, plain[:, 0], maxlag)
        with np.errstate(all="ignore"):
            want = dict(ess_tail=np.minimum(lo[:, 3], hi[:, 3]), truncated_tail=np.maximum(lo[:, 7], hi[:, 7]), rhat_folded=fold[:, 2],
                        ess_sd=sq[:, 3], mcse_sd=sq[:, 4] / (2.0 * plain[:, 1]),
                        ess_quantiles=np.stack([diag_xf_ref.summary_ref(X, LE, quant_ref.quantiles_ref(X, probs)[:, j], maxlag, zero)[:, 3]
                                                for j in range(3)], axis=1))
        for k, w in want.items():
            assert s[k].shape == w.shape and np.array_equal(np.isnan(s[k]), np.isnan(w)), k
            assert np.allclose(s[k], w, rtol=RTOL, atol=0.0, equal_nan=True), (k, s[k], w)
        moving = [f for f, name in enumerate(s["fields"]) if name != "sspri"]      # no prior: sspri is constant, its indicators too
        assert np.isfinite(s["rhat_folded"][moving]).all() and np.isfinite(s["ess_tail"][moving]).all()


def test_refusals_launch_nothing(rings):
    from mcmcf90_amd import engine_from_problem
    whole, _ = rings
    L = whole.L
    n = L.mcmcx_samples_stats_len(whole.h, 4)
    buf, a = np.full(n, 7.0), np.zeros(11)
    p, ap = _dp(buf), _dp(a)
    before = _bits(whole.samples()[1])
    good = whole.samples_stats_of(LE, a, 0, 8, 4)
    forms = ((L.mcmcx_samples_stats_of, p), (L.mcmcx_samples_stats_of_dev, C.c_void_p(8)))   # refused before the pointer is looked at
    for fn, out in forms:
        for s0, ns, maxlag, kind, av in ((0, 3, 4, 1, ap), (0, 0, 4, 2, ap), (-1, 4, 4, 3, ap), (67, 4, 4, 1, ap), (0, 71, 4, 0, None),
                                         (0, 8, -1, 1, ap), (0, 8, 33, 2, ap), (0, 8, 4, -1, ap), (0, 8, 4, 4, ap), (0, 8, 4, 1, None),
                                         (0, 8, 4, 2, None), (0, 8, 4, 3, None), (2 ** 31 - 1, 4, 4, 1, ap), (1, 2 ** 31 - 1, 4, 1, ap)):
            rc = fn(whole.h, s0, ns, maxlag, kind, av, None, out)
            assert rc == -53 and len(L.mcmcx_last_error()) > 0, (s0, ns, maxlag, kind, rc)
        assert fn(whole.h, 0, 8, 4, 1, ap, None, None) == -53 and b"null output" in L.mcmcx_last_error()
    assert np.all(buf == 7.0) and np.array_equal(_bits(whole.samples()[1]), before)
    assert np.array_equal(_bits(whole.samples_stats_of(LE, a, 0, 8, 4)), _bits(good)), "still usable, and the same"
    prob = _cols3()
    e = engine_from_problem(dict(nsimu=20, adaptint=15, updatesigma=1), prob, nchains=65, chain_id0=2)
    e.set_samples(1, 1, 20)
    for fn, out in forms:
        assert fn(e.h, 0, 8, 4, 1, ap, None, out) == -53 and b"inited" in L.mcmcx_last_error()
    e.close()
    e = engine_from_problem(dict(nsimu=20, adaptint=15, updatesigma=1), prob, nchains=65, chain_id0=2)
    e.init()
    e.run()
    for fn, out in forms:
        assert fn(e.h, 0, 8, 4, 1, ap, None, out) == -53 and b"no samples are kept" in L.mcmcx_last_error()
    e.close()
    assert np.all(buf == 7.0)


def test_the_run_is_unmoved(monkeypatch):
    """Two engines cut at the same iterations, one calling transformed summaries mid-run (its scratch allocated, then grown)."""
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("MCMCX_GROUP", "0")
    chains = [0, 63, 64, 129]
    finals = []
    for summarise in (True, False):
        e = _engine("lane_am", None, (3, 7, None))
        assert e.run(50) == 0
        if summarise:
            a = e.samples_stats_of(LE, np.zeros(10), 0, None, 2)
        assert e.run(90) == 0
        if summarise:
            b = e.samples_stats_of(FOLD, np.zeros(10), 1, 8, 32, shift=np.zeros(10))
            t = e.samples_stats_of_torch(SQUARE, np.ones(10), 0, None, 0)
            s = e.samples_summary(maxlag=4, tail=True)
            assert a.size == 3 + 10 * 6 and b.size == 3 + 10 * 36 and t.numel() == 3 + 10 * 4 and s["ess_tail"].shape == (10,)
        assert e.run() == 0
        finals.append((_final(e, chains, False), _bits(e.samples()[1])))
        e.close()
    _same_final(finals[0][0], finals[1][0], "transformed summaries in the middle of the run")
    assert np.array_equal(finals[0][1], finals[1][1])


@pytest.mark.parametrize("which", [0, 1])
def test_dev_forms_back_to_back_on_the_shared_scratch(rings, which):
    """Three asynchronous calls of different kinds, lag counts and scratch sizes issued with nothing synchronised in between: their tile
    rows, shift and a lie at the same place of the one scratch, and the stream's order alone keeps them apart."""
    import torch
    e = rings[which]
    s0, ns = ((4, 60), (7, 12))[which]
    L = e.L
    q = e.samples_quantiles([0.05, 0.5], s0, ns)
    mean = e.samples_summary(s0, ns, 0)["mean"]
    calls = [(LE, np.ascontiguousarray(q[:, 0]), 32, np.zeros(11)), (FOLD, np.ascontiguousarray(q[:, 1]), 0, None),
             (SQUARE, np.ascontiguousarray(mean), 9, None)]
    want = [e.samples_stats_of(kind, a, s0, ns, maxlag, sh) for kind, a, maxlag, sh in calls]
    e.sync()
    outs = [torch.full((w.size,), 7.0, dtype=torch.float64, device="cuda:%d" % e.cfg.device) for w in want]
    for (kind, a, maxlag, sh), t in zip(calls, outs):
        assert L.mcmcx_samples_stats_of_dev(e.h, s0, ns, maxlag, kind, _dp(a), _dp(sh), C.c_void_p(t.data_ptr())) == 0
    e.sync()
    for (kind, _, maxlag, _), t, w in zip(calls, outs, want):
        assert np.array_equal(_bits(t.cpu().numpy()), _bits(w)), (kind, maxlag)
