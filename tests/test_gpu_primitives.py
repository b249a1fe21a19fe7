"""Device primitives against the oracle, bit for bit (through the C ABI debug probes)."""
import ctypes as C
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _bits(a):
    return np.asarray(a, dtype=np.float64).view(np.uint64)


def _dev_math(op, a, b=None):
    from mcmcf90_amd import _lib
    L = _lib.load()
    a = np.ascontiguousarray(a, dtype=np.float64)
    out = np.zeros_like(a)
    dp = C.POINTER(C.c_double)
    bb = np.ascontiguousarray(b, dtype=np.float64) if b is not None else None
    rc = L.mcmcx_debug_math(op, a.size, a.ctypes.data_as(dp), bb.ctypes.data_as(dp) if bb is not None else None,
                            out.ctypes.data_as(dp))
    assert rc == 0, L.mcmcx_last_error()
    return out


def test_log_exp_sqrt_div_bitexact(oracle):
    L = oracle.lib()
    rng = np.random.default_rng(7)
    xs = np.concatenate([rng.random(200000), 10.0 ** rng.uniform(-300, 300, 20000), 1 + rng.uniform(-1e-6, 1e-6, 5000),
                         [1.0, 0.5, 2.0, 5e-324, 2.2250738585072014e-308, 0.0, np.inf]])
    ref = np.array([L.mcxo_log(float(x)) for x in xs])
    np.testing.assert_array_equal(_bits(_dev_math(0, xs)), _bits(ref))
    ts = np.concatenate([-rng.random(200000) * 708.0, rng.uniform(-760, 720, 20000), rng.uniform(-1e-3, 1e-3, 5000),
                         [0.0, -np.inf, np.inf, -708.3964185322641]])
    ref = np.array([L.mcxo_exp(float(t)) for t in ts])
    np.testing.assert_array_equal(_bits(_dev_math(1, ts)), _bits(ref))
    # sqrt and division must be IEEE correctly rounded like the host's
    ys = np.concatenate([rng.random(300000) * 10.0 ** rng.integers(-30, 30, 300000), [0.0, 1.0, 2.0, 4.0, 1e-310]])
    np.testing.assert_array_equal(_bits(_dev_math(2, ys)), _bits(np.sqrt(ys)))
    a = rng.standard_normal(300000) * 10.0 ** rng.integers(-20, 20, 300000)
    b = rng.standard_normal(300000) * 10.0 ** rng.integers(-20, 20, 300000)
    np.testing.assert_array_equal(_bits(_dev_math(3, a, b)), _bits(a / b))


def _decades(rng, n, lo=-20, hi=20):
    """n doubles of both signs over the decades 1e`lo` .. 1e`hi`"""
    return rng.standard_normal(n) * 10.0 ** rng.integers(lo, hi, n)


def test_fma_probe_bitexact():
    """dfma (op 4 returns fma(x, y, x)) against the C library's correctly rounded fma: random operands over 40 decades, and y within a few
    ulps .. 1e-6 of -1, where x y nearly cancels x and an unfused multiply-add loses every bit."""
    libm = C.CDLL("libm.so.6")
    libm.fma.restype = C.c_double
    libm.fma.argtypes = [C.c_double] * 3
    rng = np.random.default_rng(17)
    x = np.concatenate([_decades(rng, 50000), _decades(rng, 20000)])
    eps = np.concatenate([10.0 ** rng.uniform(-16, -6, 15000) * rng.choice([-1.0, 1.0], 15000), rng.integers(-4, 5, 5000) * 2.0 ** -53])
    y = np.concatenate([_decades(rng, 50000), -1.0 + eps])
    ref = np.array([libm.fma(float(p), float(q), float(p)) for p, q in zip(x, y)])
    unfused = x * y + x
    assert (_bits(ref[50000:]) != _bits(unfused[50000:])).mean() > 0.5        # the cancellation cases do tell a fused from an unfused form
    np.testing.assert_array_equal(_bits(_dev_math(4, x, y)), _bits(ref))


def test_rotg_probe_bitexact(oracle):
    """d_rotg (op 5 returns r + c 3 + s 7) against the oracle's classic netlib drotg: random pairs over 40 decades and both signs, zeros on either
    side, |a| == |b| in every sign combination (roe takes b on a tie), operands whose squares overflow / underflow without the scaling, a subnormal
    next to a normal number, neighbouring doubles.  No infinities or NaNs: classic drotg does not define them."""
    L = oracle.lib()
    rng = np.random.default_rng(19)
    a, b = 2.5, 0.75
    tiny, sub = 2.2250738585072014e-308, 5e-324
    edge = [(0.0, 0.0), (a, 0.0), (0.0, b), (-a, 0.0), (0.0, -b), (a, a), (a, -a), (-a, a), (-a, -a), (1e300, 1e300), (1e-300, 1e-300),
            (-1e300, 1e300), (1e-300, -1e-300), (sub, 1.0), (1.0, sub), (3e-310, tiny), (tiny, -3e-310), (sub, sub), (sub, -3 * sub),
            (np.nextafter(b, 1.0), b), (b, np.nextafter(b, 1.0)), (-np.nextafter(a, 0.0), a), (a, -np.nextafter(a, 9.0))]
    xs = np.concatenate([_decades(rng, 50000), [p for p, _ in edge]])
    ys = np.concatenate([_decades(rng, 50000), [q for _, q in edge]])
    ref = np.zeros(xs.size)
    for i in range(xs.size):
        da, db, c, s = C.c_double(xs[i]), C.c_double(ys[i]), C.c_double(), C.c_double()
        L.mcxo_rotg(C.byref(da), C.byref(db), C.byref(c), C.byref(s))
        ref[i] = da.value + c.value * 3.0 + s.value * 7.0
    assert np.all(np.isfinite(ref))
    np.testing.assert_array_equal(_bits(_dev_math(5, xs, ys)), _bits(ref))


def _dev_rng(kind, n, a=0.0, b=0.0, seed=11, chain=22):
    from mcmcf90_amd import _lib
    L = _lib.load()
    out = np.zeros(n)
    used = C.c_uint64()
    rc = L.mcmcx_debug_rng(seed, chain, kind, n, a, b, out.ctypes.data_as(C.POINTER(C.c_double)), C.byref(used))
    assert rc == 0, L.mcmcx_last_error()
    return out, used.value


def test_rng_streams_bitexact(oracle):
    L = oracle.lib()
    for kind, n, a, b in ((0, 5001, 0, 0), (1, 5001, 0, 0), (2, 2000, 6.0, 0.37)):
        g = oracle.Rng(); g.key[0] = 11; g.key[1] = 22
        if kind == 0:
            import subprocess  # noqa: F401  (uniforms via normal path below)
        ref = []
        for _ in range(n):
            if kind == 1:
                ref.append(L.mcxo_normal(C.byref(g)))
            elif kind == 2:
                ref.append(L.mcxo_gamma(C.byref(g), a, b))
        got, used = _dev_rng(kind, n, a, b)
        if kind == 0:
            assert used == n
            assert np.all((got >= 0) & (got < 1))
            # uniforms are checked through the normals (same stream) and against the Philox KAT on the CPU side
            continue
        np.testing.assert_array_equal(_bits(got), _bits(np.array(ref)))
        assert used == g.n


@pytest.mark.parametrize("a,b", [(0.5, 1.0), (0.3, 2.0), (0.999999, 0.37), (1.0, 0.37), (2000.5, 1e-3)])
def test_gamma_stream_shapes_below_and_at_one_bitexact(oracle, a, b):
    """rng_gamma on the a < 1 route of random_gamma (mcmcrand.F90:102-105: one uniform first, gammar_mt(1 + a, b) * u**(1/a), the route
    MCMC_DRAM.F90:201 takes when n0 + nobs < 2), on both sides of a = 1 and at a large shape: values and stream position against mcxo_gamma."""
    L = oracle.lib()
    n = 2000
    g = oracle.Rng(); g.key[0] = 11; g.key[1] = 22
    ref = np.array([L.mcxo_gamma(C.byref(g), a, b) for _ in range(n)])
    assert np.all(ref > 0.0) and np.all(np.isfinite(ref))
    if a < 1.0:
        assert g.n > 3 * n                                   # the extra uniform of every draw was taken
    got, used = _dev_rng(2, n, a, b)
    np.testing.assert_array_equal(_bits(got), _bits(ref))
    assert used == g.n
