"""Marginal and pairwise joint histograms of the sample store, counted on the device (mcmcx_samples_hist / _hist2, include/mcmcx.h).

A histogram is a vector of integers, so everything is compared without a tolerance with tests/hist_ref.py (np.searchsorted on the keys).
The kernels' own shapes go through mcmcx_debug_samples_hist: chain counts around a tile and 583 (ten tiles, three blocks of four waves),
every bin count around the 64 lanes of a wave and the two maxima, five window samples in chunks of two, a single hot cell, the values a
run cannot produce, 700 000 values so that a wave loops over tiles.  Then a real engine with a wrapped ring, the additivity over engines,
the asynchronous forms on the shared scratch, the run unmoved and the refusals that need an engine."""
import ctypes as C

import numpy as np
import pytest

import hist_ref
from test_gpu_samples import SWITCHES, _bits, _engine, _final, _gauss, _same_final
from test_hist_cpu import SPECIAL

pytestmark = pytest.mark.gpu
DP, LP, IP = C.POINTER(C.c_double), C.POINTER(C.c_int64), C.POINTER(C.c_int32)
PAIRS = [(0, 1), (2, 2), (1, 0), (0, 1)]                         # a j == k pair and a repeated one


def _debug(values, edges, pairs=None, chunk=0, one=True):
    """(1-D table or None, 2-D tables or None) of values[ns][nfields][nchains] through the kernels' debug entry."""
    from mcmcf90_amd import _lib
    L = _lib.load()
    v = np.ascontiguousarray(values, dtype=np.float64)
    e = np.ascontiguousarray(edges, dtype=np.float64)
    ns, nf, nc = v.shape
    nb = e.shape[1] - 1
    assert e.shape == (nf, nb + 1)
    out1 = np.full((nf, nb + 2), -1, dtype=np.int64) if one else None
    pr = np.ascontiguousarray(pairs, dtype=np.int32) if pairs is not None else None
    out2 = np.full((len(pr), nb + 2, nb + 2), -1, dtype=np.int64) if pr is not None else None
    rc = L.mcmcx_debug_samples_hist(0, nc, nf, ns, v.ctypes.data_as(DP), nb, e.ctypes.data_as(DP), 0 if pr is None else len(pr),
                                    None if pr is None else pr.ctypes.data_as(IP), chunk, None if out1 is None else out1.ctypes.data_as(LP),
                                    None if out2 is None else out2.ctypes.data_as(LP))
    assert rc == 0, L.mcmcx_last_error()
    return out1, out2


def _edges3(nbins, rng):
    """Three fields' edges: uniform ones, ones with equal neighbours between infinite ends, random ones around some of the values."""
    from mcmcf90_amd.engine import samples_hist_edges
    # rounded to a tenth: equal neighbours, and values that sit on them (+ 0.0: np.sort does not tell a rounded -0.0 from +0.0)
    e1 = np.sort(np.round(rng.standard_normal(nbins + 1), 1) + 0.0)
    e1[0], e1[-1] = -np.inf, np.inf
    if nbins == 1:
        e1[0] = 0.3
    return np.stack([samples_hist_edges(-2.5, 2.5, nbins), e1, np.sort(rng.standard_normal(nbins + 1)) * 0.5])


def _values3(ns, nch, rng):
    """[ns][3][nch] standard normals; field 1 rounded to a tenth (values equal to its edges), the specials spread over field 0 and 2."""
    X = rng.standard_normal((ns, 3, nch))
    X[:, 1] = np.round(X[:, 1], 1)
    k = min(SPECIAL.size, nch)
    X[0, 0, :k] = SPECIAL[:k]
    X[ns - 1, 2, nch - k:] = SPECIAL[:k]
    return X


def _check(X, edges, pairs, chunk, what):
    n = X.shape[0] * X.shape[2]
    h1, h2 = _debug(X, edges, pairs, chunk)
    assert np.array_equal(h1, hist_ref.hist_ref(X, edges)), (what, "1-D")
    assert np.all(h1.sum(axis=1) == n), (what, "the cells of a field sum to n: the NaN padding shows up nowhere")
    if pairs is not None:
        assert np.array_equal(h2, hist_ref.hist2_ref(X, pairs, edges)), (what, "2-D")
        for p, (j, k) in enumerate(pairs):
            assert np.array_equal(h2[p].sum(axis=1), h1[j]) and np.array_equal(h2[p].sum(axis=0), h1[k]), (what, "margins", p)
    return h1, h2


@pytest.mark.parametrize("nch", [1, 63, 64, 65, 583])
def test_debug_entry_against_the_restatement(nch):
    """ns = 5 in window chunks of 2 (three blocks along z, the last with one sample); nbins on both sides of a wave's 64 lanes and at
    the maxima.  2-D tables only up to 96 bins."""
    rng = np.random.default_rng(nch)
    X = _values3(5, nch, rng)
    for nbins in (1, 2, 63, 64, 65, 1024):
        e = _edges3(nbins, rng)
        h1, _ = _debug(X, e, None, 2)
        assert np.array_equal(h1, hist_ref.hist_ref(X, e)), (nch, nbins)
        assert np.all(h1.sum(axis=1) == 5 * nch), (nch, nbins)
    for nbins in (1, 2, 95, 96):
        _check(X, _edges3(nbins, rng), PAIRS, 2, (nch, nbins))
    e = _edges3(64, rng)                                        # the default chunk, and one longer than the window
    for chunk in (0, 1, 7):
        _check(X, e, PAIRS, chunk, (nch, "chunk", chunk))


def test_all_values_in_one_cell():
    """Every lane of every wave adds to one LDS counter: the middle, the first, the last cell, and positive NaNs."""
    edges = np.tile(np.linspace(-1.0, 1.0, 17), (2, 1))
    for val, cell in ((0.3, 11), (-5.0, 0), (1.0, 17), (-1.0, 1), (np.float64("nan"), 17), (np.inf, 17), (-np.inf, 0)):
        X = np.full((5, 2, 583), val)
        h1, h2 = _check(X, edges, [(0, 1), (1, 1)], 2, val)
        assert h1[0, cell] == 5 * 583 and h2[0, cell, cell] == 5 * 583 and h2[1, cell, cell] == 5 * 583, (val, cell)


def test_adversarial_values_and_edges():
    """Both zeros, both infinities, NaNs of both signs, denormals, values equal to an edge, equal edges: in every lane position."""
    from test_hist_cpu import EDGE_SETS
    rng = np.random.default_rng(5)
    for edges in EDGE_SETS:
        pool = np.concatenate([SPECIAL, edges])
        X = pool[rng.integers(0, pool.size, (3, 2, 130))]
        e = np.stack([edges, edges])
        h1, _ = _check(X, e, [(0, 1), (0, 0)], 0, edges)
        neg_nan = int((np.isnan(X[:, 0]) & np.signbit(X[:, 0])).sum())
        pos_nan = int((np.isnan(X[:, 0]) & ~np.signbit(X[:, 0])).sum())
        assert neg_nan > 0 and pos_nan > 0 and h1[0, 0] >= neg_nan and h1[0, -1] >= pos_nan
    e = np.tile(EDGE_SETS[0], (2, 1))                           # -0.0 and +0.0 are two edges: the zeros land in two cells
    X = np.where(rng.integers(0, 2, (3, 2, 130)) == 1, 0.0, -0.0)
    h1, _ = _check(X, e, [(0, 1)], 0, "zeros")
    assert h1[0, 2] == int(np.signbit(X[:, 0]).sum()) and h1[0, 3] == int((~np.signbit(X[:, 0])).sum()) and h1[0, 2] + h1[0, 3] == 390


def test_a_wave_takes_more_than_one_tile():
    """700 000 chains of two fields are 10 938 tiles: more than the 1280 blocks of four waves the grid is capped at for two fields or
    one pair, so a wave loops over tiles and a block's LDS counters take several tiles' values."""
    from mcmcf90_amd.engine import samples_hist_edges
    rng = np.random.default_rng(11)
    X = rng.standard_normal((1, 2, 700000))
    X[0, 1] += 0.5 * X[0, 0]
    X[0, 0, :1000] = 0.5
    e = np.stack([samples_hist_edges(-3.0, 3.0, 64), samples_hist_edges(-2.0, 4.0, 64)])
    h1, h2 = _check(X, e, [(0, 1)], 0, "700 000")
    assert h1[0].max() < 700000 and (h2[0] > 0).sum() > 1000


# ---- on a real engine
def _hist_engine(nch, id0=2, capacity=20, nsimu=70):
    from mcmcf90_amd import engine_from_problem
    e = engine_from_problem(dict(nsimu=nsimu, adaptint=15, updatesigma=1), _gauss(7, 27, sigma2=0.7, nobs=9), nchains=nch, chain_id0=id0)
    e.set_samples(1, 1, capacity)
    e.init()
    e.run()
    return e


def _data_edges(X, nbins):
    """[nfields][nbins + 1] uniform edges between the 2 % and 98 % points of every field (a constant field: one unit around it)."""
    from mcmcf90_amd.engine import samples_hist_edges
    flat = np.moveaxis(X, 1, 0).reshape(X.shape[1], -1)
    rows = []
    for f in range(flat.shape[0]):
        lo, hi = np.quantile(flat[f], [0.02, 0.98])
        if not lo < hi:
            lo, hi = lo - 1.0, lo + 1.0
        rows.append(samples_hist_edges(lo, hi, nbins))
    return np.stack(rows)


@pytest.fixture(scope="module")
def wrapped():
    """583 chains, a ring of twenty under seventy kept iterations: window sample w in slot (10 + w) % 20."""
    e = _hist_engine(583)
    assert e.samples_kept()[:2] == (20, 51)
    X = e.samples(layout=1)[1]
    X.setflags(write=False)
    yield e, X
    e.close()


def test_engine_histograms_against_the_restatement(wrapped):
    e, X = wrapped
    pairs = [(0, 1), (3, 9), (8, 8), (6, 2), (0, 1)]
    for s0, ns in ((0, 20), (5, 9), (16, 4), (9, 2), (19, 1)):   # the whole ring, across the wrap between 9 and 10, on either side
        W = X[s0:s0 + ns]
        for nbins in (31, 200):
            ed = _data_edges(X, nbins)
            got = e.samples_hist(ed, s0, ns)
            assert got.dtype == np.int64 and got.shape == (10, nbins + 2)
            assert np.array_equal(got, hist_ref.hist_ref(W, ed)), (s0, ns, nbins)
            assert np.all(got.sum(axis=1) == ns * 583)
            if nbins == 31:                                      # 32 edges are one call of the counts
                lt = e.samples_counts(ed, s0, ns)[:, :, 0]
                assert np.array_equal(np.cumsum(got, axis=1)[:, :-1], lt), (s0, ns, "running sums are lt at the edges")
                got2 = e.samples_hist2(pairs, ed, s0, ns)
                assert got2.dtype == np.int64 and np.array_equal(got2, hist_ref.hist2_ref(W, pairs, ed)), (s0, ns)
                for p, (j, k) in enumerate(pairs):
                    assert np.array_equal(got2[p].sum(axis=1), got[j]) and np.array_equal(got2[p].sum(axis=0), got[k]), (s0, ns, p)
    ed = _data_edges(X, 48)
    t1, t2 = e.samples_hist_torch(ed, 5, 9), e.samples_hist2_torch(pairs, ed, 5, 9)
    assert t1.is_cuda and str(t1.dtype) == "torch.int64" and tuple(t1.shape) == (10, 50) and tuple(t2.shape) == (5, 50, 50)
    assert np.array_equal(t1.cpu().numpy(), e.samples_hist(ed, 5, 9)) and np.array_equal(t2.cpu().numpy(), e.samples_hist2(pairs, ed, 5, 9))
    from mcmcf90_amd.engine import samples_hist_density
    d = samples_hist_density(e.samples_hist(ed), ed)
    assert np.array_equal(_bits(d), _bits(hist_ref.density_ref(hist_ref.hist_ref(X, ed), ed)))
    assert np.allclose((d * np.diff(ed, axis=1)).sum(axis=1)[:7], 0.96, atol=0.01), "96 % of a parameter's values lie inside its edges"


def test_histograms_of_two_engines_add_up_exactly():
    """Chains 0 .. 127 and 128 .. 255 in two engines (chain_id0 0 and 128): their tables add up to the 256-chain engine's."""
    whole = _hist_engine(256, 0, 40, 60)
    X = whole.samples(layout=1)[1]
    ed = _data_edges(X, 40)
    pairs = [(0, 6), (7, 9), (2, 2)]
    t1, t2 = whole.samples_hist(ed), whole.samples_hist2(pairs, ed)
    assert np.array_equal(t1, hist_ref.hist_ref(X, ed)) and np.array_equal(t2, hist_ref.hist2_ref(X, pairs, ed))
    whole.close()
    p1, p2 = [], []
    for id0 in (0, 128):
        e = _hist_engine(128, id0, 40, 60)
        assert np.array_equal(_bits(e.samples(layout=1)[1]), _bits(X[:, :, id0:id0 + 128])), "the halves are the whole engine's chains"
        p1.append(e.samples_hist(ed))
        p2.append(e.samples_hist2(pairs, ed))
        e.close()
    assert np.array_equal(p1[0] + p1[1], t1) and np.array_equal(p2[0] + p2[1], t2)


def test_dev_forms_back_to_back_on_the_shared_scratch(wrapped):
    """Four asynchronous calls with different edge tables and one other reader between them, one synchronisation: every call's edge keys
    sit at the same place of the one scratch, and the stream's order alone keeps them apart."""
    import torch
    e, X = wrapped
    dev = "cuda:%d" % e.cfg.device
    pairs = np.array([(0, 1), (5, 5), (9, 3)], dtype=np.int32)
    eds = [_data_edges(X, nb) for nb in (1024, 17, 96, 5)]
    outs = [torch.full((10, 1026), -1, dtype=torch.int64, device=dev), torch.full((10, 19), -1, dtype=torch.int64, device=dev),
            torch.full((3, 98, 98), -1, dtype=torch.int64, device=dev), torch.full((3, 7, 7), -1, dtype=torch.int64, device=dev)]
    stats = torch.empty(e.L.mcmcx_samples_stats_len(e.h, 0), dtype=torch.float64, device=dev)
    L, h = e.L, e.h
    assert L.mcmcx_samples_hist_dev(h, 0, 20, 1024, eds[0].ctypes.data_as(DP), C.c_void_p(outs[0].data_ptr())) == 0
    assert L.mcmcx_samples_hist_dev(h, 5, 9, 17, eds[1].ctypes.data_as(DP), C.c_void_p(outs[1].data_ptr())) == 0
    assert L.mcmcx_samples_stats_dev(h, 0, 20, 0, None, C.c_void_p(stats.data_ptr())) == 0
    assert L.mcmcx_samples_hist2_dev(h, 0, 20, 3, pairs.ctypes.data_as(IP), 96, eds[2].ctypes.data_as(DP), C.c_void_p(outs[2].data_ptr())) == 0
    assert L.mcmcx_samples_hist2_dev(h, 16, 4, 3, pairs.ctypes.data_as(IP), 5, eds[3].ctypes.data_as(DP), C.c_void_p(outs[3].data_ptr())) == 0
    e.sync()
    assert np.array_equal(outs[0].cpu().numpy(), hist_ref.hist_ref(X, eds[0]))
    assert np.array_equal(outs[1].cpu().numpy(), hist_ref.hist_ref(X[5:14], eds[1]))
    assert np.array_equal(outs[2].cpu().numpy(), hist_ref.hist2_ref(X, pairs, eds[2]))
    assert np.array_equal(outs[3].cpu().numpy(), hist_ref.hist2_ref(X[16:20], pairs, eds[3]))
    assert np.array_equal(_bits(stats.cpu().numpy()), _bits(e.samples_stats(0, 20, 0)))


def test_the_run_is_unmoved(monkeypatch):
    """Two engines cut at the same iterations, one calling the histograms mid-run (the scratch grows at the second call)."""
    from mcmcf90_amd.engine import samples_hist_edges
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("MCMCX_GROUP", "0")
    chains = [0, 63, 64, 129]
    finals = []
    for ask in (True, False):
        e = _engine("lane_am", None, (3, 7, None))
        assert e.run(50) == 0
        if ask:
            ed = np.tile(samples_hist_edges(-3.0, 3.0, 8), (10, 1))
            a, b = e.samples_hist(ed), e.samples_hist2([(0, 1)], ed)
            assert a.shape == (10, 10) and b.shape == (1, 10, 10) and np.all(a.sum(axis=1) == e.samples_kept()[0] * e.nchains)
        assert e.run(90) == 0
        if ask:
            ed = np.tile(samples_hist_edges(-3.0, 3.0, 96), (10, 1))
            a, b = e.samples_hist_torch(ed, 1, 8), e.samples_hist2_torch([(0, 1), (2, 9)], ed, 1, 8)
            c = e.samples_hist(np.tile(samples_hist_edges(-3.0, 3.0, 1024), (10, 1)))
            assert a.shape == (10, 98) and b.shape == (2, 98, 98) and c.shape == (10, 1026)
        assert e.run() == 0
        finals.append((_final(e, chains, False), _bits(e.samples()[1])))
        e.close()
    _same_final(finals[0][0], finals[1][0], "histograms in the middle of the run")
    assert np.array_equal(finals[0][1], finals[1][1])


def test_refusals_launch_nothing():
    from mcmcf90_amd import engine_from_problem
    prob = _gauss(2, 22, sigma2=0.7, nobs=9)
    e = engine_from_problem(dict(nsimu=40, adaptint=15, updatesigma=1), prob, nchains=65, chain_id0=2)
    L = e.L
    out = np.full(5 * 98 * 98, 7, dtype=np.int64)
    edges = np.tile(np.linspace(-1.0, 1.0, 9), (5, 1))
    pairs = np.array([(0, 1), (4, 4)], dtype=np.int32)
    op, ep, pp, dev = out.ctypes.data_as(LP), edges.ctypes.data_as(DP), pairs.ctypes.data_as(IP), C.c_void_p(8)

    def all_refused(s0, ns, what, word=None):
        for rc in (L.mcmcx_samples_hist(e.h, s0, ns, 8, ep, op), L.mcmcx_samples_hist_dev(e.h, s0, ns, 8, ep, dev),
                   L.mcmcx_samples_hist2(e.h, s0, ns, 2, pp, 8, ep, op), L.mcmcx_samples_hist2_dev(e.h, s0, ns, 2, pp, 8, ep, dev)):
            assert rc == -52 and len(L.mcmcx_last_error()) > 0, (what, s0, ns, rc)
            assert word is None or word in L.mcmcx_last_error(), (what, L.mcmcx_last_error())

    e.set_samples(1, 3, 5)
    all_refused(0, 1, "before init", b"inited")
    e.init()
    e.run()
    before = _bits(e.samples()[1])
    assert e.samples_kept()[0] == 5
    for s0, ns in ((0, 0), (0, -4), (-1, 2), (2, 4), (0, 6), (5, 1), (2 ** 31 - 1, 1), (1, 2 ** 31 - 1)):
        all_refused(s0, ns, "window")
    edges[4, 3] = -2.0                                           # the LAST field's row: refused once nfields is known
    all_refused(0, 5, "edges", b"of field 4 decrease")
    edges[4, 3] = np.nan
    all_refused(0, 5, "edges", b"of field 4 is a NaN")
    edges[4, 3] = -0.25
    for bad in ((5, 0), (0, 5), (-1, 0)):
        pairs[1] = bad
        for rc in (L.mcmcx_samples_hist2(e.h, 0, 5, 2, pp, 8, ep, op), L.mcmcx_samples_hist2_dev(e.h, 0, 5, 2, pp, 8, ep, dev)):
            assert rc == -52 and b"pair 1 names field" in L.mcmcx_last_error(), bad
    pairs[1] = (4, 4)
    assert np.all(out == 7)
    assert np.array_equal(_bits(e.samples()[1]), before)
    X = e.samples(layout=1)[1]                                   # still usable
    assert np.array_equal(e.samples_hist(edges), hist_ref.hist_ref(X, edges))
    assert np.array_equal(e.samples_hist2(pairs, edges, 1, 4), hist_ref.hist2_ref(X[1:5], pairs, edges))
    assert np.array_equal(_bits(e.samples()[1]), before)         # and a histogram writes nothing into the ring either
    with pytest.raises(Exception, match="edges must be"):
        e.samples_hist(edges[:4])
    e.close()
    e = engine_from_problem(dict(nsimu=40, adaptint=15, updatesigma=1), prob, nchains=65, chain_id0=2)
    e.init()
    e.run()
    all_refused(0, 1, "sampling off", b"no samples are kept")
    assert np.all(out == 7)
    e.close()
