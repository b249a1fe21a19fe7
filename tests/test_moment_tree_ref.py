"""The numpy restatement of the pooled moment tree (tests/moment_tree_ref.py) against the definition written out with Python lists, and against an
emulation of the device's launch scheme (groups of 64 tiles, six levels per launch, stride 1, 64, 4096: moments_tree_kernel and the host loop of
pooled_moments_launch) at the tile counts tests/test_gpu_moment_tree.py runs -- so a disagreement on the GPU is the kernel's, not the reference's.
The same emulation with one mistake built in shows that those tile counts can tell each of the mistakes from the tree."""
import numpy as np
import pytest

import moment_tree_ref as mt

TILES = [63, 64, 65, 66, 127, 129, 192, 4096, 4097, 4161]


def _per_tile(T, ln=4, seed=0):
    r = np.random.default_rng(1000 * T + seed)
    return r.standard_normal((T, ln)) * 10.0 ** r.integers(-3, 4, (T, ln))


def _list_tree(v):
    v = list(v)
    while len(v) > 1:
        v = [v[i] + v[i + 1] if i + 1 < len(v) else v[i] for i in range(0, len(v), 2)]
    return v[0]


def _launch_scheme(per_tile, mistake=None):
    """moments_tree_kernel launch by launch on a workspace with one stale tile behind the last one (what a longer vector of an earlier call leaves)."""
    T, ln = per_tile.shape
    ws = np.vstack([per_tile, np.full((1, ln), 3.25)])
    stride = 1
    while True:
        groups = (T + 64 * stride - 1) // (64 * stride)
        if mistake == "groups" and groups > 1:
            groups = T // (64 * stride)                                   # an off-by-one: the ragged last group is never launched
        for g in range(groups):
            t0 = g * 64 * stride if mistake != "stride" else g * 64       # "stride": the group's first tile forgets the stride
            idx = [t0 + i * stride for i in range(64)]
            # the kernel guards twice: a missing tile is loaded as +0.0, and its addition is skipped.  Either guard alone gives the same bits
            # (x + 0.0 is x), so "stale" breaks both: the load reads one tile past ntiles and the addition asks for tile i, not i + s
            limit = T + 1 if mistake == "stale" else T
            a = [ws[t].copy() if t < limit else np.zeros(ln) for t in idx]
            s = 1
            while s < 64:
                for i in range(0, 64 - s, 2 * s):
                    if mistake == "sequential":
                        continue
                    if idx[i if mistake == "stale" else i + s] < T:
                        a[i] = a[i] + a[i + s]
                s *= 2
            if mistake == "sequential":
                for i in range(1, 64):
                    if idx[i] < T:
                        a[0] = a[0] + a[i]
            ws[t0] = a[0]
        if groups <= 1:
            break
        stride *= 64
    return ws[0]


@pytest.mark.parametrize("T", [1, 2, 3, 5, 7, 64, 65, 129, 192, 300])
def test_numpy_tree_is_the_list_tree(T):
    v = _per_tile(T)
    want = np.array([_list_tree(v[:, k]) for k in range(v.shape[1])])
    np.testing.assert_array_equal(mt.bits(mt.tile_tree(v)), mt.bits(want))
    lanes = _per_tile(64 * T - 37, seed=1)
    padded = np.vstack([lanes, np.zeros((37, lanes.shape[1]))]).reshape(T, 64, -1)
    want = np.array([[_list_tree(padded[t, :, k]) for k in range(lanes.shape[1])] for t in range(T)])
    np.testing.assert_array_equal(mt.bits(mt.tile_sums(lanes)), mt.bits(want))


def test_terms_are_indexed_by_column_then_row():
    th = np.array([[1.5, -2.0, 0.25], [0.5, 4.0, -1.0]])
    par0 = np.array([0.5, 1.0, 0.25])
    t = mt.chain_terms(th, par0)
    x = th - par0
    assert t.shape == (2, mt.moment_len(3)) and np.all(t[:, 0] == 1.0) and np.array_equal(t[:, 1:4], x)
    for j in range(3):
        for i in range(j + 1):
            assert np.array_equal(t[:, 4 + j * (j + 1) // 2 + i], x[:, i] * x[:, j])


@pytest.mark.parametrize("T", TILES)
def test_launch_scheme_is_the_documented_tree(T):
    v = _per_tile(T)
    np.testing.assert_array_equal(mt.bits(_launch_scheme(v)), mt.bits(mt.tile_tree(v)))


@pytest.mark.parametrize("mistake", ["groups", "stride", "stale", "sequential"])
def test_the_tile_counts_expose_each_mistake(mistake):
    caught = [T for T in TILES if not np.array_equal(mt.bits(_launch_scheme(_per_tile(T), mistake)), mt.bits(mt.tile_tree(_per_tile(T))))]
    assert caught, mistake
    if mistake == "sequential":
        assert caught == TILES
