"""The sample store's order statistics and quantiles without a GPU: the key map's host build (mcmcx_debug_quant_key) and
mcmcx_samples_quantile_ranks against the numpy restatement of include/mcmcx.h's definition (tests/quant_ref.py), the restated finish against
numpy's own quantile, the refusals that need no device, and the build's resource report of the new kernels."""
import ctypes as C
import os

import numpy as np
import pytest

import quant_ref
from mcmcf90_amd import _lib
from mcmcf90_amd.engine import McmcError, samples_quantile_ranks

DBL_MAX = np.finfo(np.float64).max
DENORM_MIN = np.float64(5e-324)
NS = (1, 2, 3, 64, 4081, 2 ** 40)
PS = (0.0, 0.025, 0.25, 1.0 / 3.0, 0.5, 0.975, 1.0)


def _specials():
    nan_pos = np.array([0x7FF8000000000000, 0x7FF8000000000001, 0x7FFFFFFFFFFFFFFF], dtype=np.uint64).view(np.float64)
    nan_neg = np.array([0xFFF8000000000000, 0xFFF8000000000001, 0xFFFFFFFFFFFFFFFF], dtype=np.uint64).view(np.float64)
    return np.concatenate([[0.0, -0.0, np.inf, -np.inf, DENORM_MIN, -DENORM_MIN, DBL_MAX, -DBL_MAX, 1.0, -1.0], nan_pos, nan_neg])


def _random_doubles(rng, n):
    """Doubles over all exponents: random sign, exponent field and mantissa (NaN and inf patterns among them)."""
    b = (rng.integers(0, 2, n).astype(np.uint64) << np.uint64(63)) | (rng.integers(0, 2048, n).astype(np.uint64) << np.uint64(52)) \
        | rng.integers(0, 2 ** 52, n).astype(np.uint64)
    return b.view(np.float64)


def _lib_key(x, inverse):
    L = _lib.load()
    return np.array([L.mcmcx_debug_quant_key(C.c_double(float(v)), inverse) for v in x], dtype=np.int64).view(np.uint64)


def test_key_map_and_its_inverse_against_the_restatement():
    rng = np.random.default_rng(3)
    x = np.concatenate([_specials(), _random_doubles(rng, 4000)])
    # a signalling NaN may be quieted where a double is passed by value: the library is asked about quiet NaNs and everything else
    b = quant_ref.bits(x)
    snan = ((b >> np.uint64(52)) & np.uint64(0x7FF) == np.uint64(0x7FF)) & ((b & np.uint64(0x000FFFFFFFFFFFFF)) != 0) \
        & ((b & np.uint64(0x0008000000000000)) == 0)
    x = x[~snan]
    want = quant_ref.key(x)
    assert np.array_equal(_lib_key(x, 0), want)
    # the inverse returns the bits: restated, and through the library where the key's own pattern is no signalling NaN
    assert np.array_equal(quant_ref.bits(quant_ref.unkey(want)), quant_ref.bits(x))
    kd = want.view(np.float64)
    kb = want
    ok = ~(((kb >> np.uint64(52)) & np.uint64(0x7FF) == np.uint64(0x7FF)) & ((kb & np.uint64(0x000FFFFFFFFFFFFF)) != 0)
           & ((kb & np.uint64(0x0008000000000000)) == 0))
    assert ok.sum() > 3000
    assert np.array_equal(_lib_key(kd[ok], 1), quant_ref.bits(x)[ok])


def test_key_order_is_the_stated_total_order():
    rng = np.random.default_rng(4)
    x = np.concatenate([_specials(), _random_doubles(rng, 4000)])
    finite = x[~np.isnan(x)]
    by_key = finite[np.argsort(quant_ref.key(finite), kind="stable")]
    want = np.sort(finite)
    assert np.array_equal(by_key, want)                          # equal as values: np.sort does not order -0.0 against +0.0
    z = by_key[by_key == 0.0]
    assert z.size >= 2 and np.all(np.diff(np.signbit(z).astype(int)) <= 0), "-0.0 lies below +0.0"
    k = quant_ref.key(x)
    neg_nan, pos_nan = np.isnan(x) & np.signbit(x), np.isnan(x) & ~np.signbit(x)
    assert neg_nan.any() and pos_nan.any()
    assert k[neg_nan].max() < quant_ref.key(np.array([-np.inf]))[0] and k[pos_nan].min() > quant_ref.key(np.array([np.inf]))[0]


@pytest.mark.parametrize("n", NS)
def test_quantile_ranks_against_the_restatement(n):
    ranks, frac = samples_quantile_ranks(n, PS)
    wr, wf = quant_ref.quantile_ranks_ref(n, PS)
    assert ranks.dtype == np.int64 and np.array_equal(ranks, wr), (n, ranks, wr)
    assert np.array_equal(quant_ref.bits(frac), quant_ref.bits(wf)), (n, frac, wf)
    assert ranks.min() >= 0 and ranks.max() <= n - 1 and np.all(ranks[:, 0] <= ranks[:, 1])
    assert tuple(ranks[0]) == (0, min(1, n - 1)) and tuple(ranks[-1]) == (n - 1, n - 1) and frac[0] == 0.0 and frac[-1] == 0.0


def test_quantile_ranks_refusals():
    L = _lib.load()
    r, f = np.zeros(2, dtype=np.int64), np.zeros(1)
    rp, fp = r.ctypes.data_as(C.POINTER(C.c_int64)), f.ctypes.data_as(C.POINTER(C.c_double))
    for p in (-1e-300, 1.0000000000000002, np.nan, np.inf, -np.inf):
        pa = np.array([p])
        assert L.mcmcx_samples_quantile_ranks(10, 1, pa.ctypes.data_as(C.POINTER(C.c_double)), rp, fp) == -50, p
        assert len(L.mcmcx_last_error()) > 0
    pa = np.array([0.5])
    pp = pa.ctypes.data_as(C.POINTER(C.c_double))
    for n in (0, -1):
        assert L.mcmcx_samples_quantile_ranks(n, 1, pp, rp, fp) == -50
    assert L.mcmcx_samples_quantile_ranks(10, 0, pp, rp, fp) == -50
    assert L.mcmcx_samples_quantile_ranks(10, 1, None, rp, fp) == -50
    assert L.mcmcx_samples_quantile_ranks(10, 1, pp, None, fp) == -50
    assert L.mcmcx_samples_quantile_ranks(10, 1, pp, rp, None) == -50
    assert np.all(r == 0) and np.all(f == 0.0)
    with pytest.raises(McmcError):
        samples_quantile_ranks(10, [0.5, 1.5])


def test_the_finish_against_numpy_quantile():
    """The restated finish, fed from sorted random data, against np.quantile(method="linear"), at 4 ulp of max(|a|, |b|): numpy's lerp
    switches form at g >= 0.5, so bit equality is not promised.  Largest difference seen here: 1 ulp, over the 45 cases."""
    rng = np.random.default_rng(5)
    worst, cases = 0.0, 0
    for n in (1, 2, 3, 64, 4081):
        for scale in (1.0, 1e-200, 1e150):
            v = np.sort(rng.standard_normal(n) * scale)
            for p in (0.025, 1.0 / 3.0, 0.975):
                (lo, hi), = quant_ref.quantile_ranks_ref(n, [p])[0]
                g = quant_ref.quantile_ranks_ref(n, [p])[1][0]
                got = float(np.ravel(quant_ref.finish_ref(v[lo], v[hi], g))[0])
                want = float(np.quantile(v, p, method="linear"))
                ulp = np.spacing(max(abs(v[lo]), abs(v[hi])))
                worst = max(worst, abs(got - want) / ulp)
                cases += 1
                assert abs(got - want) <= 4.0 * ulp, (n, scale, p, got, want)
    assert cases == 45
    print("largest difference: %.2f ulp over %d cases" % (worst, cases))


def test_refusals_that_need_no_device():
    L = _lib.load()
    out = np.full(64, 7.0)
    cnt = np.full(64, 7, dtype=np.int64)
    ranks = np.zeros(33, dtype=np.int64)
    x = np.zeros(64)
    dp, lp = C.POINTER(C.c_double), C.POINTER(C.c_int64)
    op, cp, rp, xp = out.ctypes.data_as(dp), cnt.ctypes.data_as(lp), ranks.ctypes.data_as(lp), x.ctypes.data_as(dp)
    # a null handle
    assert L.mcmcx_samples_order_stats(None, 0, 1, 1, rp, op) == -50 and b"null handle" in L.mcmcx_last_error()
    assert L.mcmcx_samples_order_stats_dev(None, 0, 1, 1, rp, C.c_void_p(8)) == -50
    assert L.mcmcx_samples_counts(None, 0, 1, 1, xp, cp) == -50
    assert L.mcmcx_samples_counts_dev(None, 0, 1, 1, xp, C.c_void_p(8)) == -50
    assert L.mcmcx_samples_quantiles(None, 0, 1, 1, xp, op) == -50
    # null arrays and nr of 0 and 33: what the arguments alone decide is refused before the handle is looked at
    h = None
    assert L.mcmcx_samples_order_stats(h, 0, 1, 1, None, op) == -50 and b"null argument" in L.mcmcx_last_error()
    assert L.mcmcx_samples_order_stats(h, 0, 1, 1, rp, None) == -50 and b"null output" in L.mcmcx_last_error()
    assert L.mcmcx_samples_order_stats_dev(h, 0, 1, 1, rp, None) == -50 and b"null output" in L.mcmcx_last_error()
    assert L.mcmcx_samples_counts(h, 0, 1, 1, None, cp) == -50 and b"null argument" in L.mcmcx_last_error()
    assert L.mcmcx_samples_counts(h, 0, 1, 1, xp, None) == -50 and b"null output" in L.mcmcx_last_error()
    assert L.mcmcx_samples_quantiles(h, 0, 1, 1, None, op) == -50 and b"null argument" in L.mcmcx_last_error()
    assert L.mcmcx_samples_quantiles(h, 0, 1, 1, xp, None) == -50 and b"null output" in L.mcmcx_last_error()
    for nr in (0, 33, -1):
        for rc in (L.mcmcx_samples_order_stats(h, 0, 1, nr, rp, op), L.mcmcx_samples_order_stats_dev(h, 0, 1, nr, rp, C.c_void_p(8)),
                   L.mcmcx_samples_counts(h, 0, 1, nr, xp, cp), L.mcmcx_samples_counts_dev(h, 0, 1, nr, xp, C.c_void_p(8)),
                   L.mcmcx_samples_quantiles(h, 0, 1, nr, xp, op)):
            assert rc == -50 and b"outside 1 .. 32" in L.mcmcx_last_error(), nr
    # the debug entry checks its arguments before it looks for a device
    v = np.zeros(4)
    vp = v.ctypes.data_as(dp)
    assert L.mcmcx_debug_order_stats(0, 4, None, 1, rp, op) == -50
    assert L.mcmcx_debug_order_stats(0, 4, vp, 1, None, op) == -50
    assert L.mcmcx_debug_order_stats(0, 4, vp, 1, rp, None) == -50
    for nr in (0, 33):
        assert L.mcmcx_debug_order_stats(0, 4, vp, nr, rp, op) == -50
    assert L.mcmcx_debug_order_stats(0, 0, vp, 1, rp, op) == -50
    ranks[0] = 4
    assert L.mcmcx_debug_order_stats(0, 4, vp, 1, rp, op) == -50 and b"rank 4" in L.mcmcx_last_error()
    ranks[0] = -1
    assert L.mcmcx_debug_order_stats(0, 4, vp, 1, rp, op) == -50
    assert np.all(out == 7.0) and np.all(cnt == 7)


def test_order_statistic_kernels_keep_their_counts_in_registers():
    """The build's report of the shipped code object (its sha is checked by tests/test_evidence_is_current.py): every kernel of
    mcx_quant.hpp without scratch and without a vector or scalar spill -- quant_counts_kernel<NQ>'s 2 NQ counters and NQ thresholds are
    registers only while their indices are compile-time ones -- and the histogram pass with its LDS at more than one wave per SIMD."""
    rows = {}
    for line in open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "kernel_resources.txt")):
        if line.startswith("quant_"):
            f = line.split()
            rows[f[0]] = dict(zip(("vgpr", "agpr", "sgpr", "scratch", "vspill", "sspill", "lds", "wg", "waves"), map(int, f[1:])))
    assert sorted(rows) == ["quant_counts_kernel<2>", "quant_counts_kernel<32>", "quant_counts_kernel<8>", "quant_counts_zero_kernel",
                            "quant_hist_kernel", "quant_init_kernel", "quant_out_kernel", "quant_pick_kernel"]
    for name, r in rows.items():
        assert r["scratch"] == r["vspill"] == r["sspill"] == r["agpr"] == 0, (name, r)
        assert r["waves"] >= 2, (name, r)
    assert rows["quant_hist_kernel"]["waves"] >= 4
