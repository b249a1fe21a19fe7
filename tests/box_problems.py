"""A flat target in a box, with a start point per chain: chains whose accept sequence is a matter of geometry.

No new target: the built-in ss = v' Lam v with Lam = 0 is 0 everywhere (+0.0 or -0.0), so alpha is 1 wherever the proposal lands inside the box
-1 <= theta_k <= 1 and the Metropolis decision draws no uniform; outside the box the proposal is rejected before the target is looked at
(MCMC_run.F90:49-56).  cmat0 = 1e-4 I: a proposal is a hundredth of the box wide, so from the centre it always lands inside.  A chain that starts
with m coordinates at sgn (1 - 2**-40) -- inside, and closer to the wall than any proposal is short -- lands inside only if all m components move
away from their walls: a fraction 2**-m of its proposals.  m = 0 accepts at every iteration until the adapted proposal has grown to the size of
the box, m = npar >= 20 never within a test's length, m = 1 .. 8 in between; starts() lays the three kinds side by side in every wave, and gives
one tile wholly to each extreme.

Everything here is a function of its arguments, so the CPU tests (the oracle against the reference, the regime of every GPU case from the oracle
alone) and the GPU tests (the engine against the oracle) run the very same inputs.
"""
import numpy as np

EDGE = 1.0 - 2.0 ** -40
ALL_ACCEPT_TILE, NONE_ACCEPT_TILE = 3, 4


def box(d):
    """The problem keywords (oracle.Problem / engine_from_problem)."""
    return dict(kind="gauss", npar=d, par0=np.zeros(d), cmat0=1e-4 * np.eye(d), mu=np.zeros(d), lam=np.zeros((d, d)),
                lo=np.full(d, -1.0), hi=np.full(d, 1.0))


def walls(d, c):
    """The wall count of chain c."""
    if c // 64 == ALL_ACCEPT_TILE:
        return 0
    if c // 64 == NONE_ACCEPT_TILE:
        return d
    return (0, d, 1, min(d, 6), 0, d, 3, min(d, 8))[c % 8]


def starts(d, nch):
    """(X[nch, d], m[nch]): chain c starts with its first m[c] coordinates at sgn (1 - 2**-40), sgn = +1 where (c // 8) % 2 == 0, the rest at 0."""
    m = np.array([walls(d, c) for c in range(nch)], dtype=np.int64)
    X = np.zeros((nch, d))
    for c in range(nch):
        X[c, :m[c]] = EDGE if (c // 8) % 2 == 0 else -EDGE
    return X, m


def ticks(cfg):
    """The iterations at which MCMC_adapt acts (MCMC_adapt.F90:30-58 and the two branches' conditions, :60 and :105), from an oracle configuration
    (make_cfg has applied the reference's defaults and checks): (burn-in ticks, covariance ticks)."""
    burn, cov = [], []
    for it in range(2, cfg.nsimu + 1):
        if (cfg.doadapt == 0 and cfg.doburnin == 0) or (cfg.adaptend > 0 and it > cfg.adaptend):
            continue
        m1 = it % cfg.adaptint if cfg.adaptint != 0 else 1
        m2 = it % cfg.badaptint if cfg.badaptint != 0 else 1
        if m1 != 0 and m2 != 0:
            continue
        if it < cfg.burnintime and cfg.doburnin != 0 and m2 == 0:
            burn.append(it)
        elif it >= cfg.burnintime + cfg.adaptint + cfg.adapthist and cfg.doadapt != 0:
            cov.append(it)
    return burn, cov


def windows(tk):
    """[(first, last)] iteration of every window: the iterations between two ticks, the first window starting at iteration 2."""
    return [(a + 1, b) for a, b in zip([1] + list(tk[:-1]), tk)]


def _full_tiles(nch, but=()):
    return [t for t in range(nch // 64) if t not in but]


def regime(acc, d, tk, ram=False, drtries1=None, burn=None, fail=None):
    """What makes a case worth running: conditions on the inputs, from the oracle's accept sequences acc[chain, iteration] (column 0 is the
    start point) and counters alone.  tk: every tick of the run in order (ticks()).  drtries1: with delayed rejection, every chain's drtries at
    the first tick.  burn: (burn-in ticks, scalelimit).  ram: method = 'ram', with fail[chain] the oracle's failed-downdate flag."""
    acc = np.asarray(acc)
    nch = acc.shape[0]
    mixed = _full_tiles(nch, (ALL_ACCEPT_TILE, NONE_ACCEPT_TILE))
    assert len(mixed) >= 2 and nch > 64 * (NONE_ACCEPT_TILE + 1)
    t3, t4 = (slice(64 * t, 64 * t + 64) for t in (ALL_ACCEPT_TILE, NONE_ACCEPT_TILE))
    if ram:
        for t in mixed:
            a = acc[64 * t:64 * t + 64]
            assert a[:, 1:31].all(axis=1).any(), ("no chain whose first 30 iterations all accept", t)
            assert (~a[:, 1:].any(axis=1)).any(), ("no chain that accepts nothing in the whole run", t)
        assert not acc[t4, 1:].any(), "tile 4 accepts"
        assert fail.any() and not fail.all(), fail.sum()
        return
    wins = windows(tk)
    assert len(wins) >= 2, tk
    for a, b in wins:
        n, L = acc[:, a - 1:b].sum(axis=1), b - a + 1
        # (burn-in doubles a centre chain's proposal at each of its ticks: behind the last one it is a sixteenth of the box wide per coordinate,
        #  and the one window from there to the first covariance tick is eighty iterations long -- two to six of the 583 chains stay inside
        #  throughout it, not one in every tile.  In that window alone the always-accepting kind is not asked for; the covariance ticks behind it
        #  take the proposal back to the chain's own size and every window holds the three kinds again)
        every = burn is None or a != burn[0][-1] + 1
        for t in mixed:
            k = n[64 * t:64 * t + 64]
            assert (k == 0).any() and ((k == L).any() or not every) and ((k > 0) & (k < L)).any(), ("a kind is missing", (a, b), t, (k == 0).sum(), (k == L).sum())
    a, b = wins[0]
    n, L = acc[:, a - 1:b].sum(axis=1), b - a + 1
    assert (n[t3] == L).all(), ("tile 3 does not accept at every iteration of the first window", (n[t3] != L).sum())
    none4 = int((n[t4] == 0).sum())
    assert none4 == 64 if d >= 20 else none4 >= 48, ("tile 4 accepts in the first window", none4)
    assert (n == 1).any(), "no chain with exactly one accept in the first window"
    if drtries1 is not None:
        assert (drtries1 == 0).any() and (drtries1 == L).any(), ((drtries1 == 0).sum(), (drtries1 == L).sum())
    if burn is not None:
        bticks, scalelimit = burn
        assert len(bticks) >= 2
        for t in bticks:                                        # MCMC_adapt.F90:60-102: every branch taken at every tick
            staypc = (acc[:, 1:t] == 0).sum(axis=1) / float(t)
            shrink, grow = staypc > 1.0 - scalelimit, staypc < scalelimit
            shares = (shrink.mean(), grow.mean(), (~shrink & ~grow).mean())
            # shrink and grow by a twentieth of the chains, tests/test_gpu_every_chain.py's condition.  The greedy restart needs a stay share
            # within scalelimit of one half, which in a box only the one-wall chains can have: a tenth of the chains, of which Binomial(19, 1/2) puts
            # half there at the first tick and fewer later, as a chain that has moved off its wall accepts more than half -- a twentieth of all
            # chains is out of this layout's reach, a fiftieth (a fifth of the one-wall chains) is asked for
            assert min(shares[:2]) >= 0.05 and shares[2] >= 0.02, (t, shares)
