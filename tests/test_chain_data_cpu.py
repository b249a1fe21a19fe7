"""Many fits in one run, the parts that need no device: the shape checks of Engine.set_target_all (chain_data_arrays raises ValueError
before any library call) and the three kernel-table entries of the per-chain-data instances."""
import numpy as np
import pytest


def _arrays(*a):
    from mcmcf90_amd.engine import chain_data_arrays
    return chain_data_arrays(*a)


def test_good_shapes():
    y = np.arange(5 * 2 * 7, dtype=np.float64).reshape(5, 2, 7)
    x, yy, nycol, xpc = _arrays(5, 3, np.arange(7.0), y)
    assert (nycol, xpc) == (2, 0) and x.shape == (7,) and yy.shape == (5, 2, 7) and yy.flags.c_contiguous and np.array_equal(yy, y)
    x, yy, nycol, xpc = _arrays(5, 3, np.ones((5, 7)), y)
    assert (nycol, xpc) == (2, 1) and x.shape == (5, 7) and x.flags.c_contiguous
    # one column as (nchains, ndata)
    x, yy, nycol, xpc = _arrays(5, 2, np.arange(7.0), y[:, 0, :])
    assert (nycol, xpc) == (1, 0) and yy.shape == (5, 1, 7) and np.array_equal(yy[:, 0, :], y[:, 0, :])
    # nchains == ndata: the number of dimensions decides, not the lengths
    x, yy, nycol, xpc = _arrays(7, 2, np.arange(7.0), np.ones((7, 7)))
    assert (nycol, xpc) == (1, 0)
    x, yy, nycol, xpc = _arrays(7, 2, np.ones((7, 7)), np.ones((7, 1, 7)))
    assert (nycol, xpc) == (1, 1)
    # one observation
    x, yy, nycol, xpc = _arrays(5, 3, np.ones((5, 1)), np.ones((5, 2, 1)))
    assert (nycol, xpc) == (2, 1) and yy.shape == (5, 2, 1)


def test_input_is_converted():
    """Non-contiguous and integer input: contiguous float64 copies of the same values."""
    y = np.arange(5 * 7 * 2).reshape(5, 7, 2)                   # integers
    yt = y.transpose(0, 2, 1)                                   # (5, 2, 7), not contiguous
    assert not yt.flags.c_contiguous
    x = np.arange(14)[::2]
    xx, yy, nycol, xpc = _arrays(5, 3, x, yt)
    assert xx.dtype == np.float64 and yy.dtype == np.float64 and xx.flags.c_contiguous and yy.flags.c_contiguous
    assert np.array_equal(xx, np.arange(0.0, 14.0, 2.0)) and np.array_equal(yy, yt.astype(np.float64)) and (nycol, xpc) == (2, 0)
    xx, _, _, xpc = _arrays(5, 3, np.asfortranarray(np.arange(35).reshape(5, 7)), yt)
    assert xpc == 1 and xx.flags.c_contiguous and np.array_equal(xx, np.arange(35.0).reshape(5, 7))
    xx, yy, _, _ = _arrays(2, 2, [0, 1, 2], [[1, 2, 3], [4, 5, 6]])      # lists
    assert yy.shape == (2, 1, 3) and yy.dtype == np.float64


@pytest.mark.parametrize("nchains,npar,xshape,yshape,word", [
    (6, 3, (7,), (5, 2, 7), "chains"),                          # a wrong chain count
    (5, 4, (7,), (5, 2, 7), "npar"),                            # npar != 1 + nycol
    (5, 2, (7,), (5, 2, 7), "npar"),
    (5, 3, (7,), (5, 7), "npar"),                               # one column given where the model has two
    (5, 3, (7,), (7,), "ydata must be"),                        # a 1-D ydata
    (5, 3, (7,), (5, 2, 7, 1), "ydata must be"),
    (5, 3, (8,), (5, 2, 7), "xdata must be"),
    (5, 3, (4, 7), (5, 2, 7), "xdata must be"),
    (5, 3, (5, 7, 1), (5, 2, 7), "xdata must be"),
    (5, 3, (0,), (5, 2, 0), "at least one"),
    (5, 1, (7,), (5, 0, 7), "at least one"),
])
def test_bad_shapes_raise_before_any_library_call(monkeypatch, nchains, npar, xshape, yshape, word):
    from mcmcf90_amd import _lib

    def no_library(*a, **k):
        raise AssertionError("chain_data_arrays loaded the library")
    monkeypatch.setattr(_lib, "load", no_library)
    with pytest.raises(ValueError, match=word):
        _arrays(nchains, npar, np.ones(xshape), np.ones(yshape))


def test_kernel_table_lists_the_per_chain_data_instances():
    from mcmcf90_amd.engine import kernel_table
    tab = kernel_table()
    names = [n for _, n in tab]
    for fam, name, sibling in (("step", "step_kernel_cols<ram, pcd>", "step_kernel_cols<ram>"), ("step", "step_kernel_cols<pcd>", "step_kernel_cols"),
                               ("scam", "step_kernel_cols<scam, pcd>", "step_kernel_cols<scam>")):
        assert (fam, name) in tab
        assert names.index(name) < names.index(sibling)         # ahead of its shared-data sibling: the first entry that holds is taken
    assert names.index("step_kernel_cols<ram, pcd>") < names.index("step_kernel_cols<pcd>")


def test_abi_exports_the_two_entry_points():
    from mcmcf90_amd import _lib
    assert {"mcmcx_set_target_expdata_all", "mcmcx_chain_data_info"} <= set(_lib.SYMBOLS)
    L = _lib.load()
    assert L.mcmcx_set_target_expdata_all and L.mcmcx_chain_data_info
    assert L.mcmcx_chain_data_info(None, None) == -40           # a getter: no device, no handle
