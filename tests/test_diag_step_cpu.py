"""The summary of a step function of the sample store without a GPU (mcmcx_samples_stats_step, mcmcx_samples_rank_scores; include/mcmcx.h):
the numpy restatement (tests/diag_step_ref.py) against a scalar loop, the library's table of normal scores against its restatement, what
the rank-normalised diagnostics read where the plain ones are blind (chains of Cauchy draws that differ in location) and how far 128 cells
lie from the exact rank normalisation, ties, a constant field, and the refusals that need no device."""
import ctypes as C
import functools

import numpy as np
import pytest

import diag_ref
import diag_step_ref
import hist_ref
from mcmcf90_amd import _lib
from test_diag_xf_cpu import NAN_NEG, NAN_POS, SPECIALS, _bits

DP = C.POINTER(C.c_double)
LP = C.POINTER(C.c_int64)
MAXBINS = 510


def _scores(counts, nbins=None, rc_only=False):
    L = _lib.load()
    c = np.ascontiguousarray(counts, dtype=np.int64)
    out = np.full(c.shape, 7.0)
    rc = L.mcmcx_samples_rank_scores(c.ctypes.data_as(LP), c.shape[0], c.shape[1] - 2 if nbins is None else nbins, out.ctypes.data_as(DP))
    if rc_only:
        return rc, out
    assert rc == 0, (rc, L.mcmcx_last_error())
    return out


def test_restatement_against_a_scalar_loop():
    """u_ref against the definition value by value: +-0, +-inf, both NaN signs, denormals, values equal to an edge; equal edges, +-inf
    edges; table entries that are NaN and +-inf."""
    v = np.array(SPECIALS)
    X = np.broadcast_to(v[None, None, :], (2, 3, v.size)).copy()
    X[1] = X[1, :, ::-1]
    edges = np.array([[-np.inf, -1.0, -0.0, 0.0, 0.0, 5e-324, 1.0, np.inf],
                      [-1e300, -1.0, -1.0, -1.0, 0.3, 0.3, 1.0, np.nextafter(1.0, 2.0)],
                      [0.0] * 8])
    assert hist_ref.edges_ok(edges)
    table = np.arange(27, dtype=np.float64).reshape(3, 9)
    table[0, 3], table[1, 0], table[2, 8], table[2, 0] = NAN_POS, np.inf, -np.inf, NAN_NEG
    got, want = diag_step_ref.u_ref(X, edges, table), diag_step_ref.u_loop(X, edges, table)
    assert np.array_equal(_bits(got), _bits(want))
    assert np.array_equal(_bits(got[0, 2]), _bits(np.where(hist_ref.cells(v, edges[2]) == 8, -np.inf, NAN_NEG))), "eight equal edges: two cells"
    k, j = 0, 1                                                 # +0.0 and -0.0 in SPECIALS: cells 5 and 3 of field 0, whose entry 3 is a NaN
    assert hist_ref.cells(v[j], edges[0]) == 3 and hist_ref.cells(v[k], edges[0]) == 5, "-0.0 lies below +0.0"
    assert np.isnan(got[0, 0, j]) and got[0, 0, k] == 5.0


def test_rank_scores_against_the_restatement():
    """Counts of every kind -- uniform, one hot cell, empty cells at the ends and inside, one value, 10**8 values in 512 cells, a bin
    count of 1 -- against the restatement: empty cells +0.0, everything else bit for bit.  The library's AS241 and the standard
    library's are the same operations on the same p in the same order and turned out bit-equal, so that is what is demanded (the
    issue's bound was 4 ulp); equal p give equal scores and distinct p distinct ones."""
    rng = np.random.default_rng(5)
    cases = [np.full((1, 3), 1), np.array([[0, 1, 0]]), np.array([[5, 0, 0, 0, 7]]), np.array([[0, 0, 3, 0, 3, 0, 0]]),
             rng.integers(0, 50, size=(5, 130)), rng.multinomial(10 ** 8, np.full(512, 1.0 / 512), size=2),
             np.array([[1, 0, 2 ** 40, 0, 1]]), (rng.integers(0, 3, size=(3, 512)) * rng.integers(0, 2, size=(3, 512)) + np.eye(3, 512, dtype=np.int64))]
    for c in cases:
        c = np.asarray(c, dtype=np.int64)
        got, want, p = _scores(c), diag_step_ref.rank_scores_ref(c), diag_step_ref.rank_p(c)
        assert np.array_equal(_bits(got[c == 0]), _bits(np.zeros(int((c == 0).sum())))), "empty cells give +0.0"
        assert np.all((p[c > 0] > 0.0) & (p[c > 0] < 1.0))
        bad = np.flatnonzero(_bits(got).ravel() != _bits(want).ravel())
        assert bad.size == 0, (c.shape, bad[:8], got.ravel()[bad[:8]], want.ravel()[bad[:8]])
        for f in range(c.shape[0]):
            s = got[f][c[f] > 0]
            assert np.all(np.diff(s) > 0.0), "monotone over the cells that are not empty"


def test_rank_scores_are_symmetric_and_cover_every_branch():
    """Symmetric counts give antisymmetric scores; n = 10**12 in the outer cells reaches AS241's third branch (r > 5).  The bound:
    mirrored cells have p and p' with p + p' = 1 before rounding; p' near 1 carries 1.1e-16 of rounding, which moves its score by
    1.1e-16 / phi(z), below 2e-13 for |z| <= 3.5 (n is about 500 here), and p as much again at most: 1e-12 covers both."""
    rng = np.random.default_rng(6)
    half = rng.integers(0, 9, size=(4, 64))
    c = np.concatenate([half, half[:, ::-1]], axis=1)
    s = _scores(c)
    assert np.abs(s).max() <= 3.5 and np.abs(s + s[:, ::-1]).max() <= 1e-12, np.abs(s + s[:, ::-1]).max()
    assert np.array_equal(s > 0.0, s[:, ::-1] < 0.0)
    c = np.array([[1, 10 ** 12, 1, 10 ** 12, 1]])
    s = _scores(c)[0]
    assert s[0] < -6.5 and s[4] > 6.5 and s[2] == 0.0 and np.array_equal(_bits(s), _bits(diag_step_ref.rank_scores_ref(c)[0]))
    assert abs(_scores(np.array([[1, 0, 0]]))[0, 0]) == 0.0     # one value: p = 1 / 2


def test_rank_scores_refusals():
    L = _lib.load()
    good = np.ones((2, 5), dtype=np.int64)
    out = np.full((2, 5), 7.0)
    gp, op = good.ctypes.data_as(LP), out.ctypes.data_as(DP)
    for args in ((None, 2, 3, op), (gp, 2, 3, None), (gp, 0, 3, op), (gp, -1, 3, op), (gp, 2, 0, op), (gp, 2, MAXBINS + 1, op)):
        assert L.mcmcx_samples_rank_scores(*args) == -54 and len(L.mcmcx_last_error()) > 0, args[1:3]
    for bad in (np.array([[1, -1, 1, 1, 1], [1, 1, 1, 1, 1]]), np.array([[1, 1, 1, 1, 1], [0, 0, 0, 0, 0]])):
        rc, o = _scores(bad, rc_only=True)
        assert rc == -54 and np.all(o == 7.0), "refused before anything is written"
    assert np.all(out == 7.0)
    assert _scores(np.ones((1, MAXBINS + 2), dtype=np.int64)).shape == (1, 512)


def test_step_entries_refuse_without_a_device():
    """What the arguments alone decide is refused with -54 before a handle or a device is looked at."""
    L = _lib.load()
    X, out = np.zeros((4, 1, 2)), np.full(3 + 5, 7.0)
    e, t = np.array([0.0, 1.0]), np.zeros(3)
    xp, op, ep, tp = (a.ctypes.data_as(DP) for a in (X, out, e, t))
    dec, nan = np.array([1.0, 0.0]).ctypes.data_as(DP), np.array([0.0, np.nan]).ctypes.data_as(DP)
    zero = np.array([0.0, -0.0]).ctypes.data_as(DP)
    for nbins, ed, tb, o in ((1, ep, tp, None), (1, None, tp, op), (1, ep, None, op), (0, ep, tp, op), (MAXBINS + 1, ep, tp, op),
                            (1, dec, tp, op), (1, nan, tp, op), (1, zero, tp, op)):
        assert L.mcmcx_debug_samples_stats_step(0, 2, 1, 4, xp, 1, nbins, ed, tb, None, o) == -54, nbins
        assert L.mcmcx_samples_stats_step(None, 0, 4, 1, nbins, ed, tb, None, o) == -54, nbins
        assert L.mcmcx_samples_stats_step_dev(None, 0, 4, 1, nbins, ed, tb, None, C.c_void_p(8) if o else None) == -54, nbins
    assert L.mcmcx_samples_stats_step(None, 0, 4, 1, 1, ep, tp, None, op) == -54 and b"null handle" in L.mcmcx_last_error()
    for nch, nf, ns, maxlag in ((0, 1, 4, 1), (2, 0, 4, 1), (2, 1, 3, 1), (2, 1, 4, -1), (2, 1, 4, 33)):
        assert L.mcmcx_debug_samples_stats_step(0, nch, nf, ns, xp, maxlag, 1, ep, tp, None, op) == -54
    assert L.mcmcx_debug_samples_stats_step(0, 2, 1, 4, None, 1, 1, ep, tp, None, op) == -54
    assert np.all(out == 7.0)


# ------------------------------------------------------------------ what the numbers read: [64][3][200], maxlag 16, seeds 1 .. 8
MAXLAG = 16


@functools.lru_cache(maxsize=None)
def _case(seed):
    """Fields: Cauchy draws with every second chain shifted by 1, Cauchy draws, AR(1) with coefficient 0.7.  -> (plain table, 128-cell
    rank summary, exact rank-normalised table)."""
    rng = np.random.default_rng(seed)
    shifted = rng.standard_cauchy((64, 200))
    shifted[:, ::2] += 1
    cauchy = rng.standard_cauchy((64, 200))
    ar = rng.normal(size=(64, 200))
    for i in range(1, 64):
        ar[i] = 0.7 * ar[i - 1] + np.sqrt(1.0 - 0.49) * ar[i]
    X = np.stack([shifted, cauchy, ar], axis=1)
    return diag_ref.summary_ref(X, MAXLAG), diag_step_ref.rank_summary_ref(X, MAXLAG, 128), diag_step_ref.exact_rank_summary_ref(X, MAXLAG)


@pytest.mark.parametrize("seed", range(1, 9))
def test_rank_rhat_sees_what_the_plain_one_does_not(seed):
    """Chains of Cauchy draws that differ in location by 1: the plain split-R-hat reads 1.000 (measured 0.9998 .. 1.0006), the
    rank-normalised one over 128 cells 1.023 .. 1.027."""
    plain, cells, _ = _case(seed)
    print("seed %d: plain rhat %.6f, 128-cell rank rhat %.6f" % (seed, plain[0, 2], cells["rhat_rank"][0]))
    assert cells["rhat_rank"][0] >= 1.015
    assert plain[0, 2] <= 1.005
    assert cells["rhat_max"][0] >= cells["rhat_rank"][0]


@pytest.mark.parametrize("seed", range(1, 9))
def test_128_cells_against_the_exact_rank_normalisation(seed):
    """R-hat within 2e-3 (measured at most 5e-4) and ESS within 5 % (measured at most 2.5 %) of the exact rank-normalised ones (scipy's
    average ranks and ndtri), on all three fields."""
    _, cells, exact = _case(seed)
    for f, name in enumerate(("shifted Cauchy", "Cauchy", "AR(1) 0.7")):
        dr, de = abs(cells["rhat_rank"][f] - exact[f, 2]), abs(cells["ess_bulk_rank"][f] / exact[f, 3] - 1.0)
        print("seed %d %-14s rhat %.6f exact %.6f (%.1e)  ess %.1f exact %.1f (%.2f %%)"
              % (seed, name, cells["rhat_rank"][f], exact[f, 2], dr, cells["ess_bulk_rank"][f], exact[f, 3], 100.0 * de))
        assert dr <= 2e-3, (name, dr)
        assert de <= 0.05, (name, de)


def test_ties_finish_and_a_constant_field_gives_nan():
    """Normals rounded to one decimal (some sixty distinct values in 12 800: most of the 127 edges are equal to a neighbour, most cells
    empty) finish without a NaN; a constant field falls into one cell and gives NaN in every new column."""
    rng = np.random.default_rng(11)
    X = np.stack([np.round(rng.normal(size=(64, 200)), 1), np.full((64, 200), 2.5)], axis=1)
    s = diag_step_ref.rank_summary_ref(X, MAXLAG, 128)
    edges = diag_step_ref.rank_edges_ref(X, 128)
    counts = hist_ref.hist_ref(X, edges)
    assert hist_ref.edges_ok(edges) and (counts[0] == 0).sum() > 60 and counts[1, -1] == 64 * 200
    lib = diag_step_ref.rank_summary_ref(X, MAXLAG, 128, scores=_scores)
    for k in ("rhat_rank", "ess_bulk_rank", "truncated_rank", "rhat_max"):
        assert np.isfinite(s[k][0]) and np.isnan(s[k][1]) == (k != "truncated_rank"), (k, s[k])
        assert np.array_equal(_bits(s[k]), _bits(lib[k])), "the library's scores give the same table"
    assert 0.99 < s["rhat_rank"][0] < 1.01 and s["ess_bulk_rank"][0] > 64 * 200 * 0.5
    exact = diag_step_ref.exact_rank_summary_ref(X[:, :1], MAXLAG)
    assert abs(s["rhat_rank"][0] - exact[0, 2]) <= 2e-3, "every tie group is a cell of its own: the average-rank convention itself"


def test_fold_scores_are_the_restatement():
    """mcmcf90_amd.engine.samples_fold_scores against tests/diag_step_ref.py, ties of |centre - median| among them."""
    from mcmcf90_amd.engine import samples_fold_scores, samples_rank_scores
    rng = np.random.default_rng(12)
    edges = np.sort(rng.normal(size=(3, 21)), axis=1)
    edges[1] = np.arange(-10.0, 11.0)                           # symmetric about the centre 0: pairs of cells tie
    edges[2, 5:9] = edges[2, 5]
    counts = rng.integers(0, 40, size=(3, 22))
    centre = np.array([0.1, 0.0, -0.3])
    got, want = samples_fold_scores(counts, edges, centre), diag_step_ref.fold_scores_ref(counts, edges, centre)
    assert np.array_equal(_bits(got), _bits(want))
    assert np.array_equal(_bits(got[1, 1:11]), _bits(got[1, 20:10:-1])), "cells at the same distance share a score"
    assert np.array_equal(_bits(samples_rank_scores(counts)), _bits(diag_step_ref.rank_scores_ref(counts)))
