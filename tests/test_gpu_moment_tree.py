"""The pooled moment vector above one launch level of its tile tree, bit for bit.

moments_kernel sums every 64-chain tile; moments_tree_kernel finishes the fixed pairwise tree over tiles six levels per launch, the host
(pooled_moments_launch) repeating it with stride 1, 64, 4096 until one group is left.  Pooled mode, the multi-GPU exchange and "the same bits
for any shard count" rest on that tree, so it is compared here with the numpy restatement of its DEFINITION (tests/moment_tree_ref.py, which
knows nothing of groups of 64) at tile counts that need two and three launches, ragged at every level, with one and two x-blocks of
the tree kernel -- and the inputs are shown to be able to tell the tree from a sequential sum."""
import functools
import numpy as np
import pytest

import moment_tree_ref as mt

pytestmark = pytest.mark.gpu

# (tiles T, npar d, nchains): 64 T - 37 chains (a ragged last tile) unless noted
CASES = [
    (63, 3, None), (64, 3, None),                    # one launch: the last group not full, a full group
    (65, 3, None), (66, 3, None), (127, 3, None),    # two launches: a lone tile in group 1, two tiles there, a second group one tile short,
    (129, 3, None), (192, 3, None), (4096, 3, None),     # a lone tile in group 2, three groups whose third has no partner, a full second level
    (4097, 3, None), (4161, 3, None),                # three launches (4161 = 4096 + 64 + 1: a lone tile at every level)
    (64, 3, 64 * 64),                                # no inactive lane anywhere
    (66, 22, None), (192, 22, None),                 # 276 moments: two x-blocks of the tree kernel, the second ragged
]
_ids = ["T%d-d%d%s" % (T, d, "-full" if n else "") for T, d, n in CASES]


def _problem(d):
    """A unit Gaussian the chains start half a standard deviation away from, with a proposal small enough that most of them move at once."""
    ckw = dict(nsimu=8, doadapt=0, updatesigma=0)
    pkw = dict(kind="gauss", npar=d, par0=0.5 - 0.75 * np.arange(d) / d, cmat0=(0.02 / d) * np.eye(d), mu=np.zeros(d), lam=np.eye(d))
    return ckw, pkw


def _run(d, nchains, chain_id0=0):
    from mcmcf90_amd import engine_from_problem
    ckw, pkw = _problem(d)
    e = engine_from_problem(ckw, pkw, nchains=nchains, chain_id0=chain_id0)
    e.init(); e.run()
    return e, pkw["par0"]


@functools.lru_cache(maxsize=None)
def _case(T, d, nchains):
    """One engine run per case, shared by the tests below: the states, the engine's moments (asked for twice) and the restatement's."""
    n = nchains or 64 * T - 37
    assert (n + 63) // 64 == T
    e, par0 = _run(d, n)
    th = e.theta()
    got, again, kernel = e.pooled_moments(), e.pooled_moments(), e.last_kernel()
    e.close()
    terms = mt.chain_terms(th, par0)
    per_tile = mt.tile_sums(terms)
    exact, absum = mt.exact_sums(terms)
    moved = int(np.any(th != par0, axis=1).sum())
    return dict(n=n, th=th, par0=par0, got=got, again=again, kernel=kernel, ref=mt.tile_tree(per_tile), seq=mt.running_sum(per_tile),
                exact=exact, bound=mt.pairwise_bound(n, absum), moved=moved)


@pytest.mark.parametrize("T,d,nchains", CASES, ids=_ids)
def test_inputs_tell_the_tree_from_a_running_sum(T, d, nchains):
    """What holds of the restatement alone, whatever the device computed: the count, the pairwise-summation bound against the exact sums, and that
    these states distinguish the tree's order from a sequential sum over tiles in at least a third of the entries."""
    c = _case(T, d, nchains)
    assert c["ref"][0] == c["n"]
    assert c["moved"] > c["n"] // 2, "most chains never moved: %d of %d" % (c["moved"], c["n"])
    err = np.abs(c["ref"] - c["exact"])
    assert np.all(err <= c["bound"]), (err / c["bound"]).max()
    differ = int((mt.bits(c["ref"])[1:] != mt.bits(c["seq"])[1:]).sum())
    print("T=%d d=%d: %d of %d entries differ from a running sum; worst error %.3f of the bound" % (T, d, differ, len(c["ref"]) - 1,
                                                                                                    (err[1:] / c["bound"][1:]).max()))
    assert 3 * differ >= len(c["ref"]) - 1, (differ, len(c["ref"]) - 1)


@pytest.mark.parametrize("T,d,nchains", CASES, ids=_ids)
def test_pooled_moments_are_the_documented_tree(T, d, nchains):
    c = _case(T, d, nchains)
    msg = "T=%d d=%d nchains=%d, sampling kernel %s" % (T, d, c["n"], c["kernel"])
    assert len(c["got"]) == mt.moment_len(d)
    np.testing.assert_array_equal(mt.bits(c["got"]), mt.bits(c["ref"]), err_msg=msg)
    assert c["got"][0] == c["n"], msg
    np.testing.assert_array_equal(mt.bits(c["again"]), mt.bits(c["got"]), err_msg=msg)       # the tree ran in place on the workspace
    err = np.abs(c["got"] - c["exact"])
    assert np.all(err <= c["bound"]), (msg, (err / c["bound"]).max())                        # the value, not only the order


def test_restatement_agrees_with_the_python_tree_at_65_tiles():
    """The list-based tree the pooled-mode restatements use (tests/test_gpu_pooled.py) and the numpy one, on the same states."""
    from test_gpu_pooled import _pooled_moments
    c = _case(65, 3, None)
    cnt, s1, s2 = _pooled_moments(c["th"], c["par0"], c["n"])
    flat = [cnt] + list(s1) + [s2[(i, j)] for j in range(3) for i in range(j + 1)]
    np.testing.assert_array_equal(mt.bits(np.array(flat)), mt.bits(c["ref"]))


def test_shards_of_64_tiles_add_up_to_one_engine():
    """The power-of-two aligned blocks the comment above moments_tree_kernel promises: three engines of 4096 chains (64 tiles, one full group
    each) against one engine of 8192 and one of 12288 chains, whose trees go through a second launch."""
    d = 3
    ms, ths = [], []
    for r in range(3):
        e, par0 = _run(d, 4096, chain_id0=4096 * r)
        ms.append(e.pooled_moments()); ths.append(e.theta())
        e.close()
    for nsh in (2, 3):
        e, _ = _run(d, 4096 * nsh)
        m, th = e.pooled_moments(), e.theta()
        e.close()
        np.testing.assert_array_equal(mt.bits(np.vstack(ths[:nsh])), mt.bits(th))               # streams keyed by chain id
        parts = ms[0] + ms[1] if nsh == 2 else (ms[0] + ms[1]) + ms[2]
        np.testing.assert_array_equal(mt.bits(parts), mt.bits(m))
        np.testing.assert_array_equal(mt.bits(m), mt.bits(mt.pooled_moments_ref(th, par0)))
        assert m[0] == 4096 * nsh


@pytest.mark.parametrize("T", [66, 4097])
def test_device_destination_gets_the_last_launch_only(T):
    """mcmcx_pooled_moments_dev: the tree kernel writes `dst` in its last launch (one group left) and nowhere past the vector."""
    import torch
    d, n = 3, 64 * T - 37
    ln = mt.moment_len(d)
    e, par0 = _run(d, n)
    t = torch.full((2 * ln,), float("nan"), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    e.pooled_moments_dev(t.data_ptr())
    e.sync()
    dev = t.cpu().numpy()
    host, th = e.pooled_moments(), e.theta()
    e.close()
    assert len(host) == ln
    np.testing.assert_array_equal(mt.bits(dev[:ln]), mt.bits(host))
    np.testing.assert_array_equal(mt.bits(host), mt.bits(mt.pooled_moments_ref(th, par0)))
    assert np.all(np.isnan(dev[ln:])), dev[ln:]
