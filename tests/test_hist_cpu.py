"""The sample store's histograms without a device (mcmcx_samples_hist / _hist2 / _hist_edges / _hist_density, include/mcmcx.h): the numpy
restatement tests/hist_ref.py against the definition's own words on small arrays, the uniform edges bit for bit, the density finish, every
refusal that the arguments alone decide, and the new kernels' rows of the build's resource report."""
import ctypes as C
import os

import numpy as np

import hist_ref
from mcmcf90_amd import _lib
from mcmcf90_amd.engine import McmcError, samples_hist_density, samples_hist_edges

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = np.uint64
NBINS = (1, 2, 63, 64, 65, 1024)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _f(words):
    return np.array(words, dtype=U).view(np.float64)


NEG_NAN, POS_NAN = _f([0xFFF8000000000000])[0], _f([0x7FF8000000000000])[0]
# both zeros, both infinities, NaNs of both signs and two payloads, the smallest denormals and the largest, numbers around the edges
SPECIAL = np.concatenate([_f([0xFFF8000000000000, 0xFFFFFFFFFFFFFFFF, 0x7FF8000000000000, 0x7FF0000000000001, 1, 0x8000000000000001,
                              0x000FFFFFFFFFFFFF, 0x800FFFFFFFFFFFFF]),
                          [0.0, -0.0, np.inf, -np.inf, 1.0, -1.0, 0.5, np.nextafter(0.5, 0), np.nextafter(0.5, 1), 2.0, -2.0, 1e300, -1e300]])
EDGE_SETS = [
    np.array([-1.0, -0.0, 0.0, 0.5, 0.5, 1.0]),                 # both zeros as edges, an empty bin
    np.array([-np.inf, -1.0, 0.5, np.inf]),                     # infinite outer edges
    np.array([0.5, 0.5]),                                       # one empty bin
    _f([0x8000000000000001, 0x8000000000000000, 0, 1]),         # -denormal, -0, +0, +denormal
    np.array([-2.0, 2.0]),
    np.array([np.inf, np.inf, np.inf]),
    np.array([-np.inf, -np.inf]),
]


def test_the_restatement_is_the_definition():
    """searchsorted(side='right') on the keys against a loop that counts the edges not above the value, on the adversarial values."""
    rng = np.random.default_rng(1)
    for edges in EDGE_SETS:
        assert hist_ref.edges_ok(edges)
        v = np.concatenate([SPECIAL, edges, rng.standard_normal(40)])
        got, want = hist_ref.cells(v, edges), hist_ref.cells_loop(v, edges)
        assert np.array_equal(got, want), (edges, v[got != want])
        assert got.min() >= 0 and got.max() <= edges.size
    e = EDGE_SETS[0]                                             # the words of the definition, one by one
    c = lambda x: int(hist_ref.cells(np.array([x]), e)[0])       # noqa: E731
    assert c(-3.0) == 0 and c(-1.0) == 1 and c(np.nextafter(-1.0, -2)) == 0, "left-closed"
    assert c(-0.0) == 2 and c(0.0) == 3, "-0.0 lies below +0.0"
    assert c(0.5) == 5 and c(np.nextafter(0.5, 0)) == 3, "a value on two equal edges passes the empty bin"
    assert c(1.0) == 6 and c(np.nextafter(1.0, 0)) == 5 and c(np.inf) == 6, "right-open, the last bin too"
    assert c(POS_NAN) == 6 and c(NEG_NAN) == 0, "NaNs at the two ends"
    assert not hist_ref.edges_ok([0.0, -0.0]) and not hist_ref.edges_ok([0.0, np.nan]) and not hist_ref.edges_ok([1.0, 0.5])


def test_tables_of_the_restatement():
    """The cells of a field sum to n, the running sums are lt at the edges (tests/quant_ref.py), the 2-D margins are the 1-D tables."""
    import quant_ref
    rng = np.random.default_rng(2)
    X = rng.standard_normal((5, 3, 67))
    X[0, 0, :SPECIAL.size] = SPECIAL
    X[1, 2, :8] = 0.25
    edges = np.stack([np.linspace(-2, 2, 9), np.array([-np.inf, -1, -0.0, 0.0, 0.25, 0.25, 1, 3, np.inf]), np.linspace(0.25, 0.75, 9)])
    h = hist_ref.hist_ref(X, edges)
    assert h.shape == (3, 10) and h.dtype == np.int64 and np.all(h.sum(axis=1) == 5 * 67)
    lt = quant_ref.counts_ref(X, edges)[:, :, 0]
    assert np.array_equal(np.cumsum(h, axis=1)[:, :-1], lt)
    pairs = [(0, 1), (2, 2), (1, 0), (0, 1)]
    h2 = hist_ref.hist2_ref(X, pairs, edges)
    assert h2.shape == (4, 10, 10)
    for p, (j, k) in enumerate(pairs):
        assert np.array_equal(h2[p].sum(axis=1), h[j]) and np.array_equal(h2[p].sum(axis=0), h[k]), p
    assert np.array_equal(h2[1], np.diag(h[2])) and np.array_equal(h2[2], h2[0].T) and np.array_equal(h2[3], h2[0])


def test_uniform_edges_bit_for_bit():
    rng = np.random.default_rng(3)
    cases = 0
    for nbins in NBINS:
        for _ in range(40):
            a, b = (rng.choice([-1.0, 1.0]) * 10.0 ** rng.uniform(-300, 300) * rng.uniform(1, 10) for _ in range(2))
            if rng.integers(0, 4) == 0:
                b = a * (1 + rng.uniform(1e-15, 1e-3))           # a narrow range far from zero: many edges round to equal values
            lo, hi = min(a, b), max(a, b)
            if not lo < hi:
                continue
            got = samples_hist_edges(lo, hi, nbins)
            want = hist_ref.uniform_edges_ref(lo, hi, nbins)
            assert got.shape == (nbins + 1,) and np.array_equal(_bits(got), _bits(want)), (lo, hi, nbins)
            assert got[0] == lo and got[-1] == hi and hist_ref.edges_ok(got) and np.all(np.diff(got) >= 0), (lo, hi, nbins)
            cases += 1
    assert cases > 200
    assert np.array_equal(samples_hist_edges(-1.0, 1.0, 4), [-1.0, -0.5, 0.0, 0.5, 1.0])
    L = _lib.load()
    out = np.full(1026, 7.0)
    op = out.ctypes.data_as(C.POINTER(C.c_double))
    for lo, hi, nb, word in ((0.0, 1.0, 0, b"bins"), (0.0, 1.0, 1025, b"bins"), (0.0, 1.0, -1, b"bins"), (np.nan, 1.0, 4, b"finite"),
                             (0.0, np.inf, 4, b"finite"), (-np.inf, 0.0, 4, b"finite"), (1.0, 1.0, 4, b"below"), (2.0, 1.0, 4, b"below"),
                             (-1.7e308, 1.7e308, 4, b"non-decreasing")):
        assert L.mcmcx_samples_hist_edges(lo, hi, nb, op) == -52 and word in L.mcmcx_last_error(), (lo, hi, nb, L.mcmcx_last_error())
    assert L.mcmcx_samples_hist_edges(0.0, 1.0, 4, None) == -52 and b"null output" in L.mcmcx_last_error()
    try:
        samples_hist_edges(1.0, 0.0, 3)
        raise AssertionError("not refused")
    except McmcError as ex:
        assert "below" in str(ex)


def test_density_finish():
    rng = np.random.default_rng(4)
    edges = np.stack([np.linspace(-1, 1, 8), np.array([-3.0, -1.0, -1.0, 0.0, 0.5, 0.5, 0.5, 4.0]), rng.standard_normal(8).cumsum()])
    edges[2].sort()
    counts = rng.integers(0, 10 ** 12, (3, 9)).astype(np.int64)
    counts[1, 2] = 0                                             # an empty bin of no width: 0 / 0
    got, want = samples_hist_density(counts, edges), hist_ref.density_ref(counts, edges)
    assert got.shape == (3, 7) and np.array_equal(_bits(got), _bits(want))
    assert np.isnan(got[1, 1]) and np.isinf(got[1, 4]) and np.isinf(got[1, 5]), "an empty-width bin gives the IEEE answer"
    # what the density means: inside the edges it integrates to the share of the values that lie there
    inside = counts[0, 1:-1].sum() / counts[0].sum()
    assert abs((got[0] * np.diff(edges[0])).sum() - inside) < 1e-14
    L = _lib.load()
    dp, lp = C.POINTER(C.c_double), C.POINTER(C.c_int64)
    out = np.full(64, 7.0)
    cp, ep, op = counts.ctypes.data_as(lp), edges.ctypes.data_as(dp), out.ctypes.data_as(dp)
    assert L.mcmcx_samples_hist_density(None, ep, 3, 7, op) == -52 and L.mcmcx_samples_hist_density(cp, None, 3, 7, op) == -52
    assert L.mcmcx_samples_hist_density(cp, ep, 3, 7, None) == -52 and b"null argument" in L.mcmcx_last_error()
    assert L.mcmcx_samples_hist_density(cp, ep, 0, 7, op) == -52 and b"nfields" in L.mcmcx_last_error()
    for nb in (0, 1025):
        assert L.mcmcx_samples_hist_density(cp, ep, 3, nb, op) == -52 and b"bins" in L.mcmcx_last_error()
    assert np.all(out == 7.0)


def test_refusals_that_need_no_device():
    """-52 for everything the arguments alone decide, before the handle (here: none) or a device is looked at."""
    L = _lib.load()
    dp, lp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int64), C.POINTER(C.c_int32)
    out = np.full(4096, 7, dtype=np.int64)
    edges = np.tile(np.linspace(0.0, 1.0, 1026), (3, 1))
    pairs = np.zeros((65, 2), dtype=np.int32)
    op, ep, pp, dev = out.ctypes.data_as(lp), edges.ctypes.data_as(dp), pairs.ctypes.data_as(ip), C.c_void_p(8)
    h = None

    def err():
        return L.mcmcx_last_error()
    # a null handle, after the arguments passed
    for rc in (L.mcmcx_samples_hist(h, 0, 1, 4, ep, op), L.mcmcx_samples_hist_dev(h, 0, 1, 4, ep, dev),
               L.mcmcx_samples_hist2(h, 0, 1, 1, pp, 4, ep, op), L.mcmcx_samples_hist2_dev(h, 0, 1, 1, pp, 4, ep, dev)):
        assert rc == -52 and b"null handle" in err()
    # null output, edge table, pair list
    assert L.mcmcx_samples_hist(h, 0, 1, 4, ep, None) == -52 and b"null output" in err()
    assert L.mcmcx_samples_hist_dev(h, 0, 1, 4, ep, None) == -52 and b"null output" in err()
    assert L.mcmcx_samples_hist(h, 0, 1, 4, None, op) == -52 and b"null edge table" in err()
    assert L.mcmcx_samples_hist2(h, 0, 1, 1, pp, 4, ep, None) == -52 and b"null output" in err()
    assert L.mcmcx_samples_hist2_dev(h, 0, 1, 1, pp, 4, ep, None) == -52 and b"null output" in err()
    assert L.mcmcx_samples_hist2(h, 0, 1, 1, pp, 4, None, op) == -52 and b"null edge table" in err()
    assert L.mcmcx_samples_hist2(h, 0, 1, 1, None, 4, ep, op) == -52 and b"null pair list" in err()
    # nbins and npairs out of range: 1024 and 96 bins, 64 pairs pass (and meet the null handle)
    for nb in (0, -1, 1025):
        for rc in (L.mcmcx_samples_hist(h, 0, 1, nb, ep, op), L.mcmcx_samples_hist_dev(h, 0, 1, nb, ep, dev)):
            assert rc == -52 and b"outside 1 .. 1024" in err(), nb
    for nb in (0, -1, 97, 1024):
        for rc in (L.mcmcx_samples_hist2(h, 0, 1, 1, pp, nb, ep, op), L.mcmcx_samples_hist2_dev(h, 0, 1, 1, pp, nb, ep, dev)):
            assert rc == -52 and b"outside 1 .. 96" in err(), nb
    for npairs in (0, -1, 65):
        for rc in (L.mcmcx_samples_hist2(h, 0, 1, npairs, pp, 4, ep, op), L.mcmcx_samples_hist2_dev(h, 0, 1, npairs, pp, 4, ep, dev)):
            assert rc == -52 and b"outside 1 .. 64" in err(), npairs
    assert L.mcmcx_samples_hist(h, 0, 1, 1024, ep, op) == -52 and b"null handle" in err()
    assert L.mcmcx_samples_hist2(h, 0, 1, 64, pp, 96, ep, op) == -52 and b"null handle" in err()
    # bad edges: a NaN, a decreasing pair, +0.0 before -0.0 (the first field's row needs no nfields)
    for bad, word in (([0.0, np.nan, 1.0], b"NaN"), ([0.0, 1.0, 0.5], b"decrease"), ([0.0, -0.0, 1.0], b"decrease"), ([np.inf, -np.inf, 0.0],
                                                                                                                 b"decrease")):
        b = np.array(bad)
        bp = b.ctypes.data_as(dp)
        for rc in (L.mcmcx_samples_hist(h, 0, 1, 2, bp, op), L.mcmcx_samples_hist_dev(h, 0, 1, 2, bp, dev),
                   L.mcmcx_samples_hist2(h, 0, 1, 1, pp, 2, bp, op), L.mcmcx_samples_hist2_dev(h, 0, 1, 1, pp, 2, bp, dev)):
            assert rc == -52 and word in err(), (bad, err())
    ok = np.array([-np.inf, -0.0, 0.0, 0.0, np.inf])            # equal neighbours and infinities are edges
    assert L.mcmcx_samples_hist(h, 0, 1, 4, ok.ctypes.data_as(dp), op) == -52 and b"null handle" in err()
    # the debug entry knows nfields: every row of the edge table, the pair indices -- all before it looks for a device
    v = np.zeros((2, 3, 5))
    vp = v.ctypes.data_as(dp)
    e3 = np.tile(np.linspace(0.0, 1.0, 5), (3, 1))
    e3p = e3.ctypes.data_as(dp)

    def dbg(values=vp, nch=5, nf=3, ns=2, nb=4, ed=e3p, npairs=1, pr=pp, chunk=0, o1=op, o2=op):
        return L.mcmcx_debug_samples_hist(0, nch, nf, ns, values, nb, ed, npairs, pr, chunk, o1, o2)
    assert dbg(values=None) == -52 and b"null values" in err()
    assert dbg(o1=None, o2=None) == -52 and b"null output" in err()
    assert dbg(ed=None) == -52 and b"null edge table" in err()
    assert dbg(pr=None) == -52 and b"null pair list" in err()
    assert dbg(nb=0) == -52 and dbg(nb=97) == -52 and b"outside 1 .. 96" in err()
    assert dbg(nb=1025, ed=ep, o2=None) == -52 and b"outside 1 .. 1024" in err()
    assert dbg(npairs=0) == -52 and dbg(npairs=65) == -52 and b"outside 1 .. 64" in err()
    for kw in (dict(nch=0), dict(nf=0), dict(ns=0), dict(chunk=-1)):
        assert dbg(**kw) == -52, kw
    e3[2, 3] = 0.1                                              # the last field's row decreases
    assert dbg() == -52 and b"of field 2 decrease" in err()
    assert dbg(o2=None) == -52 and b"of field 2 decrease" in err()
    e3[2, 3] = np.nan
    assert dbg() == -52 and b"of field 2 is a NaN" in err()
    e3[2, 3] = 0.75
    tmp = np.zeros(4096, dtype=np.int64)                         # with a device these calls run
    tp = tmp.ctypes.data_as(lp)
    for j, k in ((3, 0), (0, 3), (-1, 0), (0, -1), (2 ** 31 - 1, 0)):
        pairs[1] = (j, k)
        assert dbg(npairs=2) == -52 and b"pair 1 names field" in err(), (j, k)
        assert dbg(npairs=1, o1=tp, o2=tp) in (0, -10), "the second pair is not looked at: what is left is the device"
        assert dbg(npairs=2, o1=tp, o2=None) in (0, -10), "nor any pair without a 2-D table"
    pairs[1] = (2, 2)
    assert dbg(npairs=2, o1=tp, o2=tp) in (0, -10)
    assert np.all(out == 7)


def test_histogram_kernels_use_no_scratch():
    """The build's report of the shipped code object (its sha is checked by tests/test_evidence_is_current.py): both kernels of
    mcx_hist.hpp without scratch and without a vector or scalar spill, their LDS dynamic (none static), at more than one wave per SIMD."""
    rows = {}
    for line in open(os.path.join(ROOT, "profiles", "kernel_resources.txt")):
        if line.startswith("hist"):
            f = line.split()
            rows[f[0]] = dict(zip(("vgpr", "agpr", "sgpr", "scratch", "vspill", "sspill", "lds", "wg", "waves"), map(int, f[1:])))
    assert sorted(rows) == ["hist2_kernel", "hist_kernel"]
    for name, r in rows.items():
        assert r["scratch"] == r["vspill"] == r["sspill"] == r["agpr"] == r["lds"] == 0, (name, r)
        assert r["wg"] == 256 and r["waves"] >= 4, (name, r)
