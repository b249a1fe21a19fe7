"""The summary of a step function of the sample store, reduced on the device (mcmcx_samples_stats_step / _dev /
mcmcx_debug_samples_stats_step, include/mcmcx.h): rank-normalised split-R-hat and bulk ESS.

The definition is the summary's own sums of u(x) = table[cell(x)], so the stats vector is compared on raw bits with the numpy restatement
(tests/diag_step_ref.py).  The debug entry lays a caller's array out as a store: chain counts on both sides of a tile (the padding lanes
hold NaN), five fields (not a multiple of the four a block takes), windows of 4, 5 (middle dropped), 9 and 40 samples, a maxlag for every
instantiation, bin counts 1, 2, around the search's power of two and at the LDS cap, shift given and NULL, and the values a run cannot
put into the ring.  Then the indicator that already exists, an engine's ring, whole and wrapped: bits, the device form, the
rank-normalised summary against its composition, the refusals, the run unmoved and the asynchronous forms back to back on the shared
scratch."""
import ctypes as C

import numpy as np
import pytest

import diag_ref
import diag_step_ref
import diag_xf_ref
import quant_ref
from test_diag_xf_cpu import NAN_NEG, NAN_POS
from test_gpu_diag_xf import rings  # noqa: F401  (the module's fixture: a whole ring and a wrapped one, 130 chains, 11 fields)
from test_gpu_samples import SWITCHES, _bits, _cols3, _engine, _final, _same_final

pytestmark = pytest.mark.gpu
DP = C.POINTER(C.c_double)
NCHAINS, WINDOWS, MAXLAGS, NBINS = (1, 64, 65, 130), (4, 5, 9, 40), (0, 3, 8, 16, 32), (1, 2, 63, 64, 65, 510)
COMBOS = [(m, b) for m in MAXLAGS for b in NBINS]


def _dp(a):
    return None if a is None else a.ctypes.data_as(DP)


def _debug(X, maxlag, edges, table, shift=None):
    from mcmcf90_amd import _lib
    L = _lib.load()
    ns, nf, nch = X.shape
    X, edges, table = (np.ascontiguousarray(a, dtype=np.float64) for a in (X, edges, table))
    sh = None if shift is None else np.ascontiguousarray(shift, dtype=np.float64)
    out = np.full(diag_ref.stats_len(nf, maxlag), 7.0)
    rc = L.mcmcx_debug_samples_stats_step(0, nch, nf, ns, _dp(X), maxlag, edges.shape[1] - 1, _dp(edges), _dp(table), _dp(sh), _dp(out))
    assert rc == 0, (rc, L.mcmcx_last_error())
    return out


def _same_bits(got, want, what):
    assert got.shape == want.shape, what
    bad = np.flatnonzero(_bits(got) != _bits(want))
    assert bad.size == 0, (what, bad[:8], got[bad[:8]], want[bad[:8]])


def _values(seed, ns, nf, nch):
    """Correlated along the window (so that the lag sums are no noise), fields near and far from zero."""
    rng = np.random.default_rng(seed)
    X = rng.normal(size=(ns, nf, nch))
    for i in range(1, ns):
        X[i] = 0.6 * X[i - 1] + 0.8 * X[i]
    return X + np.array([0.0, 10.0, -3.0, 0.5, 1e3])[:nf, None]


def _edges_table(seed, X, nbins):
    """Edges at quantiles of the field's values (every cell is hit where there are values enough), some of them values themselves and
    some equal to a neighbour; a table of normals."""
    rng = np.random.default_rng(seed)
    nf = X.shape[1]
    edges = np.stack([np.quantile(X[:, f], np.linspace(0.02, 0.98, nbins + 1)) for f in range(nf)])
    for f in range(nf):
        v = X[:, f].ravel()
        k = rng.integers(0, nbins + 1, size=max(1, nbins // 4))
        edges[f, k] = v[rng.integers(0, v.size, size=k.size)]
    edges = np.sort(edges, axis=1)
    if nbins >= 2:
        edges[:, 1] = edges[:, 0]
    return edges, rng.normal(size=(nf, nbins + 2))


@pytest.mark.parametrize("nch", NCHAINS)
@pytest.mark.parametrize("ns", WINDOWS)
def test_debug_entry_bits(nch, ns):
    """Every (maxlag, nbins) pair once per window length, dealt over the four chain counts; the shift given and NULL in turn."""
    X = _values(1000 * ns + nch, ns, 5, nch)
    shift = np.random.default_rng(ns).normal(size=5) * 0.3
    for j, (maxlag, nbins) in enumerate(COMBOS):
        if j % len(NCHAINS) != NCHAINS.index(nch):
            continue
        edges, table = _edges_table(j, X, nbins)
        sh = shift if (j // len(NCHAINS) + WINDOWS.index(ns)) % 2 else None
        got, want = _debug(X, maxlag, edges, table, sh), diag_step_ref.stats_ref(X, edges, table, maxlag, sh)
        _same_bits(got, want, (nch, ns, maxlag, nbins, sh is not None))
        if sh is None:
            assert np.array_equal(_bits(got[3:].reshape(5, maxlag + 4)[:, 0]), _bits(diag_step_ref.u_ref(X[:1, :, :1], edges, table).ravel()))


def test_every_pair_of_maxlag_and_nbins_is_dealt():
    """The deal above reaches every pair at every window length, and with 40 samples every instantiation (K = 0, 3, 8, 16, 19)."""
    dealt = {(ns, COMBOS[j]) for ns in WINDOWS for nch in NCHAINS for j in range(len(COMBOS)) if j % len(NCHAINS) == NCHAINS.index(nch)}
    assert dealt == {(ns, c) for ns in WINDOWS for c in COMBOS}
    assert sorted({min(m, 40 // 2 - 1) for m in MAXLAGS}) == [0, 3, 8, 16, 19]


def _same(got, want, what):
    """NaNs where the restatement has NaNs, equal bits everywhere else."""
    assert got.shape == want.shape, what
    gn, wn = np.isnan(got), np.isnan(want)
    assert np.array_equal(gn, wn), (what, np.flatnonzero(gn != wn)[:8])
    bad = np.flatnonzero((_bits(got) != _bits(want)) & ~wn)
    assert bad.size == 0, (what, bad[:8], got[bad[:8]], want[bad[:8]])


def test_debug_entry_adversarial_values():
    """+-0, +-inf, NaNs of both signs, denormals and values equal to an edge scattered over 65 chains and 9 samples; edges that are
    zeros of both signs, denormals, infinities and equal neighbours; table entries that are NaN and +-inf.  Fields 0 and 1 have finite
    tables: every value, the NaNs included, is looked up to a finite number and the bits are compared.  The entry fills the 63 padding
    lanes with (positive) NaNs: they belong to the last cell of every field, which in field 1 lies at or above +inf and holds 1e6 -- a
    kernel that did not mask them would show it in every sum."""
    nch, ns, nf = 65, 9, 5
    rng = np.random.default_rng(78)
    special = [0.0, -0.0, np.inf, -np.inf, NAN_POS, NAN_NEG, 5e-324, -5e-324, 2.2250738585072009e-308, -2.2250738585072009e-308, 0.7, -0.7]
    edges = np.array([[-np.inf, -0.7, -5e-324, -0.0, 0.0, 5e-324, 0.7, np.inf],
                      [-0.7, -0.7, -0.7, -0.0, -0.0, 0.7, 0.7, np.inf],
                      [-np.inf, -np.inf, -1.0, 0.0, 0.0, 1.0, np.inf, np.inf],
                      [-2.0, -1.0, -0.5, 0.0, 0.5, 1.0, 2.0, 3.0],
                      [0.0] * 8])
    table = rng.normal(size=(nf, 9))
    table[1, 8] = 1e6
    table[2, 0], table[2, 5], table[2, 8] = -np.inf, NAN_POS, np.inf
    table[3, 2], table[3, 6] = NAN_NEG, np.inf
    table[4, 0], table[4, 8] = NAN_POS, -0.0
    X = rng.normal(size=(ns, nf, nch))
    for f in range(nf):
        for _ in range(60):
            X[rng.integers(ns), f, rng.integers(nch)] = special[rng.integers(len(special))]
    zero = np.zeros(nf)
    for maxlag in (0, 3, 32):
        for sh in (zero, None):
            got, want = _debug(X, maxlag, edges, table, sh), diag_step_ref.stats_ref(X, edges, table, maxlag, sh)
            _same(got, want, (maxlag, sh is None))
            per = want[3:].reshape(nf, maxlag + 4)
            assert not np.isnan(per[:2]).any() and np.isnan(per[2:4, 1:3]).all(), "fields 0 and 1 are compared on bits, 2 and 3 hold NaN"


def test_the_indicator_that_already_exists(rings):  # noqa: F811
    """Both edges at the successor of a_f in the key order and the table (1, +0, +0): u is the indicator key(x) <= key(a_f), and the
    vector has the bits of kind 1 of mcmcx_samples_stats_of at a -- on a caller's array and on an engine's window alike."""
    from mcmcf90_amd import _lib
    L = _lib.load()

    def as_double(word):
        return float(np.array([word & 0xFFFFFFFFFFFFFFFF], dtype=np.uint64).view(np.float64)[0])

    def successor(a):
        """the double whose key is key(a) + 1: the key as a double's bits, through the inverse map"""
        return as_double(L.mcmcx_debug_quant_key(as_double(L.mcmcx_debug_quant_key(float(a), 0) + 1), 1))
    X = _values(9, 9, 5, 65)
    a = np.array([np.quantile(X[:, f], q) for f, q in enumerate((0.05, 0.5, 0.95, 0.3, 0.7))])
    a[1], a[3] = X[4, 1, 7], -0.0                               # a value itself; the zero whose successor is +0.0
    X[2, 3, 5], X[3, 3, 6] = -0.0, 0.0
    s = np.array([successor(v) for v in a])
    assert np.array_equal(quant_ref.key(s), quant_ref.key(a) + np.uint64(1)) and s[3] == 0.0 and not np.signbit(s[3])
    edges, table = np.stack([s, s], axis=1), np.tile([1.0, 0.0, 0.0], (5, 1))
    for maxlag, sh in ((0, None), (3, np.zeros(5)), (32, None)):
        out = np.full(diag_ref.stats_len(5, maxlag), 7.0)
        Xc = np.ascontiguousarray(X)
        assert L.mcmcx_debug_samples_stats(0, 65, 5, 9, _dp(Xc), maxlag, 1, _dp(a), _dp(sh), _dp(out)) == 0
        _same_bits(_debug(X, maxlag, edges, table, sh), out, ("kind 1", maxlag))
        _same_bits(out, diag_xf_ref.stats_ref(X, diag_xf_ref.LE, a, maxlag, sh), ("kind 1 itself", maxlag))
    for e, (s0, ns, maxlag) in zip(rings, ((2, 40, 8), (7, 12, 16))):
        q = e.samples_quantiles([0.3], s0, ns)[:, 0]
        moving = np.array([successor(v) for v in q])
        got = e.samples_stats_step(np.stack([moving, moving], axis=1), np.tile([1.0, 0.0, 0.0], (11, 1)), s0, ns, maxlag)
        _same_bits(got, e.samples_stats_of(diag_xf_ref.LE, q, s0, ns, maxlag), ("kind 1 on the ring", s0, ns))


# ------------------------------------------------------------------ an engine's ring: cols3 (nfields 11), 130 chains
def _engine_check(e, s0, ns, maxlag, cells, given, torch_too):
    from mcmcf90_amd.engine import samples_rank_scores
    _, X = e.samples(s0, ns, layout=1)
    edges = e.samples_rank_edges(cells, s0, ns)
    assert np.array_equal(_bits(edges), _bits(diag_step_ref.rank_edges_ref(X, cells)))
    table = samples_rank_scores(e.samples_hist(edges, s0, ns))
    sh = np.random.default_rng(s0 + ns).normal(size=11) * 0.3 if given else None
    got = e.samples_stats_step(edges, table, s0, ns, maxlag, sh)
    _same_bits(got, diag_step_ref.stats_ref(X, edges, table, maxlag, sh), (s0, ns, maxlag, cells, given))
    if torch_too:
        t = e.samples_stats_step_torch(edges, table, s0, ns, maxlag, sh)
        assert t.is_cuda and str(t.dtype) == "torch.float64"
        assert np.array_equal(_bits(t.cpu().numpy()), _bits(got)), (s0, ns, maxlag, cells, "device form")


def test_engine_bits_whole_and_wrapped_ring(rings):  # noqa: F811
    whole, wrapped = rings
    for s0, ns, maxlag, cells, given in ((0, 70, 32, 128, False), (0, 70, 8, 512, True), (3, 9, 16, 3, False), (61, 9, 0, 64, True)):
        _engine_check(whole, s0, ns, maxlag, cells, given, torch_too=True)
    for s0, ns, maxlag, cells, given in ((0, 20, 8, 128, False), (5, 9, 3, 17, True), (7, 12, 16, 65, False), (9, 5, 1, 4, True)):
        _engine_check(wrapped, s0, ns, maxlag, cells, given, torch_too=True)


def test_rank_summary_is_the_composition(rings):  # noqa: F811
    """Every new key, bit for bit, against the same composition made in numpy from the restatements on samples(layout=1); without
    `rank` the summary has the keys and the bits it had."""
    from mcmcf90_amd.engine import DIAG_COLUMNS
    new = {"rhat_rank", "ess_bulk_rank", "truncated_rank", "rhat_max"}
    for e, (s0, ns, maxlag, cells) in zip(rings, ((10, 40, 8, 128), (3, 16, 16, 16))):
        old, s = e.samples_summary(s0, ns, maxlag), e.samples_summary(s0, ns, maxlag, rank=True, rank_cells=cells)
        assert set(old) == set(DIAG_COLUMNS) | {"fields", "iterations"} and set(s) == set(old) | new
        _, X = e.samples(s0, ns, layout=1)
        plain = diag_ref.summary_ref(X, maxlag)
        for j, k in enumerate(DIAG_COLUMNS):
            assert np.array_equal(_bits(s[k]), _bits(old[k])), k
            assert np.array_equal(np.isnan(old[k]), np.isnan(plain[:, j])) and np.allclose(old[k], plain[:, j], rtol=1e-13, atol=0.0, equal_nan=True), k
        assert s["fields"] == old["fields"] and np.array_equal(s["iterations"], old["iterations"])
        want = diag_step_ref.rank_summary_ref(X, maxlag, cells)
        for k in sorted(new):
            assert s[k].shape == (11,), k
            _same(s[k], want[k], (k, s[k], want[k]))
        moving = [f for f, name in enumerate(s["fields"]) if name != "sspri"]      # no prior: sspri is constant, one cell
        const = s["fields"].index("sspri")
        assert np.isfinite(s["rhat_rank"][moving]).all() and np.isfinite(s["ess_bulk_rank"][moving]).all()
        assert np.isnan(s["rhat_rank"][const]) and np.isnan(s["ess_bulk_rank"][const]) and np.isnan(s["rhat_max"][const])
        assert np.all(s["rhat_max"][moving] >= s["rhat_rank"][moving])
    e = rings[1]
    assert set(e.samples_summary(3, 16, 4, tail=True, rank=True, rank_cells=16)) == set(e.samples_summary(3, 16, 4, tail=True)) | new


def test_refusals_launch_nothing(rings):  # noqa: F811
    from mcmcf90_amd import engine_from_problem
    whole, _ = rings
    L = whole.L
    n = L.mcmcx_samples_stats_len(whole.h, 4)
    buf = np.full(n, 7.0)
    edges, table = np.tile([0.0, 1.0, 1.0], (11, 1)), np.ones((11, 4))
    dec, nan = edges.copy(), edges.copy()
    dec[10, 2], nan[7, 0] = 0.5, np.nan                          # in rows that are looked at once nfields is known
    p, ep, tp = _dp(buf), _dp(edges), _dp(table)
    before = _bits(whole.samples()[1])
    good = whole.samples_stats_step(edges, table, 0, 8, 4)
    forms = ((L.mcmcx_samples_stats_step, p), (L.mcmcx_samples_stats_step_dev, C.c_void_p(8)))   # refused before the pointer is looked at
    for fn, out in forms:
        for s0, ns, maxlag, nbins, ed, tb in ((0, 3, 4, 2, ep, tp), (0, 0, 4, 2, ep, tp), (-1, 4, 4, 2, ep, tp), (67, 4, 4, 2, ep, tp),
                                             (0, 71, 4, 2, ep, tp), (0, 8, -1, 2, ep, tp), (0, 8, 33, 2, ep, tp), (0, 8, 4, 0, ep, tp),
                                             (0, 8, 4, -1, ep, tp), (0, 8, 4, 511, ep, tp), (0, 8, 4, 2, None, tp), (0, 8, 4, 2, ep, None),
                                             (0, 8, 4, 2, _dp(dec), tp), (0, 8, 4, 2, _dp(nan), tp), (2 ** 31 - 1, 4, 4, 2, ep, tp),
                                             (1, 2 ** 31 - 1, 4, 2, ep, tp)):
            rc = fn(whole.h, s0, ns, maxlag, nbins, ed, tb, None, out)
            assert rc == -54 and len(L.mcmcx_last_error()) > 0, (s0, ns, maxlag, nbins, rc)
        assert fn(whole.h, 0, 8, 4, 2, ep, tp, None, None) == -54 and b"null output" in L.mcmcx_last_error()
        assert fn(None, 0, 8, 4, 2, ep, tp, None, out) == -54 and b"null handle" in L.mcmcx_last_error()
    assert np.all(buf == 7.0) and np.array_equal(_bits(whole.samples()[1]), before)
    assert np.array_equal(_bits(whole.samples_stats_step(edges, table, 0, 8, 4)), _bits(good)), "still usable, and the same"
    prob = _cols3()
    e = engine_from_problem(dict(nsimu=20, adaptint=15, updatesigma=1), prob, nchains=65, chain_id0=2)
    e.set_samples(1, 1, 20)
    for fn, out in forms:
        assert fn(e.h, 0, 8, 4, 2, ep, tp, None, out) == -54 and b"inited" in L.mcmcx_last_error()
    e.close()
    e = engine_from_problem(dict(nsimu=20, adaptint=15, updatesigma=1), prob, nchains=65, chain_id0=2)
    e.init()
    e.run()
    for fn, out in forms:
        assert fn(e.h, 0, 8, 4, 2, ep, tp, None, out) == -54 and b"no samples are kept" in L.mcmcx_last_error()
    e.close()
    assert np.all(buf == 7.0)


def test_the_run_is_unmoved(monkeypatch):
    """Two engines cut at the same iterations, one calling step summaries mid-run (its scratch allocated, then grown)."""
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("MCMCX_GROUP", "0")
    chains = [0, 63, 64, 129]
    finals = []
    for summarise in (True, False):
        e = _engine("lane_am", None, (3, 7, None))
        assert e.run(50) == 0
        if summarise:
            a = e.samples_stats_step(np.tile([0.0, 1.0], (10, 1)), np.tile([0.0, 1.0, 0.0], (10, 1)), 0, None, 2)
        assert e.run(90) == 0
        if summarise:
            ed = e.samples_rank_edges(512)
            b = e.samples_stats_step(ed, np.tile(np.arange(512.0), (10, 1)), 1, 8, 32, shift=np.zeros(10))
            t = e.samples_stats_step_torch(ed[:, :64], np.ones((10, 65)), 0, None, 0)
            s = e.samples_summary(maxlag=4, rank=True, rank_cells=32)
            assert a.size == 3 + 10 * 6 and b.size == 3 + 10 * 36 and t.numel() == 3 + 10 * 4 and s["rhat_rank"].shape == (10,)
        assert e.run() == 0
        finals.append((_final(e, chains, False), _bits(e.samples()[1])))
        e.close()
    _same_final(finals[0][0], finals[1][0], "step summaries in the middle of the run")
    assert np.array_equal(finals[0][1], finals[1][1])


@pytest.mark.parametrize("which", [0, 1])
def test_dev_forms_back_to_back_on_the_shared_scratch(rings, which):  # noqa: F811
    """Three asynchronous calls of different bin counts, lag counts and scratch sizes issued with nothing synchronised in between: their
    tile rows, shift, keys and table lie at the same place of the one scratch, and the stream's order alone keeps them apart."""
    import torch
    from mcmcf90_amd.engine import samples_rank_scores
    e = rings[which]
    s0, ns = ((4, 60), (7, 12))[which]
    L = e.L
    calls = []
    for cells, maxlag, sh in ((512, 32, np.zeros(11)), (3, 0, None), (65, 9, None)):
        edges = e.samples_rank_edges(cells, s0, ns)
        calls.append((edges, samples_rank_scores(e.samples_hist(edges, s0, ns)), maxlag, sh))
    want = [e.samples_stats_step(ed, tb, s0, ns, maxlag, sh) for ed, tb, maxlag, sh in calls]
    e.sync()
    outs = [torch.full((w.size,), 7.0, dtype=torch.float64, device="cuda:%d" % e.cfg.device) for w in want]
    for (ed, tb, maxlag, sh), t in zip(calls, outs):
        assert L.mcmcx_samples_stats_step_dev(e.h, s0, ns, maxlag, ed.shape[1] - 1, _dp(ed), _dp(tb), _dp(sh), C.c_void_p(t.data_ptr())) == 0
    e.sync()
    for (ed, _, maxlag, _), t, w in zip(calls, outs, want):
        assert np.array_equal(_bits(t.cpu().numpy()), _bits(w)), (ed.shape, maxlag)
