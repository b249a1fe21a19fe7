"""The pooled moment vector of a set of chain states, restated in numpy from its documented definition (the comments above moments_kernel and
moments_tree_kernel in mcmcf90_amd/csrc/mcx_moments.hpp) -- NOT from the kernels' launch scheme (64 tiles per group, six levels per launch):

    terms of a chain     [1, x_j, x_i x_j (i <= j, at index j (j + 1) / 2 + i)],  x = theta - par0
    inside a tile        the 64 lanes by an adjacent-pairs tree; a lane without a chain contributes +0.0
    over the T tiles     for s = 1, 2, 4, ...: for t = 0, 2 s, 4 s, ... with t + s < T: v[t] += v[t + s]   (no partner: no addition)

Every addition is one IEEE operation of numpy, so a device that adds the same operands on the same sides gives the same bits."""
import math
import numpy as np


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def moment_len(d):
    return 1 + d + d * (d + 1) // 2


def chain_terms(theta, par0):
    """[n][1 + d + d (d + 1) / 2]: the terms every chain contributes."""
    x = np.asarray(theta, dtype=np.float64) - np.asarray(par0, dtype=np.float64)
    n, d = x.shape
    out = np.empty((n, moment_len(d)))
    out[:, 0] = 1.0
    out[:, 1:1 + d] = x
    for j in range(d):
        for i in range(j + 1):
            out[:, 1 + d + j * (j + 1) // 2 + i] = x[:, i] * x[:, j]
    return out


def tile_sums(terms):
    """[T][len]: the 64 lanes of every tile in the adjacent-pairs tree (lane l + lane l ^ 1 first); the last tile's missing lanes are +0.0."""
    n, ln = terms.shape
    T = (n + 63) // 64
    v = np.zeros((T * 64, ln))
    v[:n] = terms
    v = v.reshape(T, 64, ln)
    while v.shape[1] > 1:
        v = v[:, 0::2, :] + v[:, 1::2, :]
    return v[:, 0, :]


def tile_tree(per_tile):
    """The fixed pairwise tree over tiles, adjacent tiles first; a tile without a partner is carried up unchanged (the tile axis is never padded)."""
    v = np.array(per_tile, dtype=np.float64)
    T, s = v.shape[0], 1
    while s < T:
        b = v[s::2 * s]
        v[0:2 * s * len(b):2 * s] += b
        s *= 2
    return v[0].copy()


def running_sum(per_tile):
    """What a sequential sum over tiles would give (acc = acc + per_tile[t]): the order the tree must be told apart from."""
    acc = np.array(per_tile[0], dtype=np.float64)
    for t in range(1, len(per_tile)):
        acc = acc + per_tile[t]
    return acc


def pooled_moments_ref(theta, par0):
    return tile_tree(tile_sums(chain_terms(theta, par0)))


def exact_sums(terms):
    """(fsum of every column, fsum of its absolute values): the correctly rounded sums of the terms as they stand."""
    ex = np.array([math.fsum(terms[:, k]) for k in range(terms.shape[1])])
    ab = np.array([math.fsum(np.abs(terms[:, k])) for k in range(terms.shape[1])])
    return ex, ab


def pairwise_bound(nchains, abs_sums):
    """Error bound of a pairwise sum of 64 T products against the exact sum: one rounding per level of the tree and one for the product."""
    T = (nchains + 63) // 64
    return (math.ceil(math.log2(64 * T)) + 1) * 2.0 ** -53 * abs_sums
