"""The thinned sample store's rule and arithmetic, without a GPU (mcmcx_set_samples, include/mcmcx.h): which iterations a ring of
`capacity` samples retains, how many doubles a chain's sample has, and where a row of the store lives -- the last one through the host
build of the very function the store's kernels index with, at sizes whose element offset passes 2**31 and 2**32."""
import ctypes as C

import pytest

from mcmcf90_amd.engine import sample_iterations, sample_nfields, sample_store_offset


def _brute(first, thin, capacity, simuind):
    ring = []
    for i in range(1, simuind + 1):
        if i >= first and (i - first) % thin == 0:
            ring.append(i)
            if len(ring) > capacity:
                ring.pop(0)                                     # the oldest sample is overwritten
    return ring


def test_sample_iterations_equals_a_loop_over_the_iterations():
    wrapped = empty = 0
    for first in range(1, 7):
        for thin in range(1, 6):
            for capacity in range(1, 5):
                for simuind in range(1, 26):
                    want = _brute(first, thin, capacity, simuind)
                    assert sample_iterations(first, thin, capacity, simuind) == want, (first, thin, capacity, simuind)
                    empty += not want
                    wrapped += len([i for i in range(first, simuind + 1, thin)]) > 2 * capacity
    assert empty > 0 and wrapped > 0                            # first > simuind, and rings that wrapped more than once, were among them


def test_sampling_off_keeps_nothing():
    assert sample_iterations(1, 0, 4, 100) == []
    assert sample_iterations(1, 3, 0, 100) == []


def _nfields(npar, nycol):
    return len(["theta"] * npar + ["ss"] * nycol + ["sspri"] + ["sigma2"] * nycol)


@pytest.mark.parametrize("npar,nycol", [(1, 1), (2, 1), (7, 1), (50, 1), (4, 3), (4096, 4096)])
def test_nfields(npar, nycol):
    assert sample_nfields(npar, nycol) == npar + 2 * nycol + 1 == _nfields(npar, nycol)
    assert sample_nfields(npar) == npar + 3


def test_store_offset_beyond_the_int_range():
    """capacity x ntiles x nfields x 64 elements: 100 samples of 262 144 chains at npar 50 are 1.39e9 doubles, 1000 of them pass 2**32.
    The library's function (size_t throughout) against Python's integers."""
    from mcmcf90_amd import _lib
    L = _lib.load()
    cases = [(0, 1, 4, 0, 0), (2, 3, 10, 1, 9), (99, 4096, 53, 4095, 52), (154, 4096, 53, 0, 0), (155, 4096, 53, 0, 0),
             (999, 4096, 53, 4095, 52), (40, 16384, 12289, 16383, 12288), (2 ** 20, 2 ** 15, 12289, 7, 5)]
    past31 = past32 = 0
    for slot, ntiles, nfields, tile, field in cases:
        want = sample_store_offset(slot, ntiles, nfields, tile, field)
        assert want == ((slot * ntiles + tile) * nfields + field) * 64
        assert want < 2 ** 63
        got = L.mcmcx_debug_samples_offset(slot, ntiles, nfields, tile, field)
        assert got == want, (slot, ntiles, nfields, tile, field, got, want)
        past31 += want >= 2 ** 31
        past32 += want >= 2 ** 32
        assert C.c_int32(want & 0xFFFFFFFF).value != want or want < 2 ** 31          # (what an int-typed index would have made of it)
    assert past31 >= 4 and past32 >= 3
