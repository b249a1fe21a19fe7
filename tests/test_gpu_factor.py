"""The adaptation tick's own factorisation on edge covariances, every compiled form (mcmcx_debug_calculate_R; the matrices:
tests/factor_cases.py).

An engine run feeds MCMC_calculate_R's Cholesky branch -- dpotf2, the 2.4 / sqrt(npar) scaling, with delayed rejection dpotri and
R2 = R / drscale -- covariances of smooth chains: dense, positive definite, nearly equal on all lanes.  Here the lane form
(calculate_R / potri_packed in adapt_post_kernel<false,*>), the four tile_factor_kernel instances and potri_packed on an SVD factor
(adapt_post_kernel<true,*>) get failures at the first pivot, the last and at the seams of their blocks, pivots of +0, -0, NaN and +inf,
exact zeros that meet infinities in dtrmv and dgemv, subnormal input -- and chains of one wave, one 16-lane group and one workgroup that
succeed, fail at different pivots, or do not recompute at all.  The probe launches through the function the tick ends in, so the
instance, the grid and the LDS size are the engine's.

One engine per layout: a Gaussian target, 83 chains (one full tile and a ragged one; a ragged last workgroup for every NW), no iteration
run, one probe call.  Reference: the oracle's mcxo_calculate_R on the same matrix with the same configuration.  Per chain:

    need, oracle info == 0   triu(R), and with delayed rejection triu(R2) and triu(iC), bit for bit -- where an entry is a NaN, NaN-ness
                             and payload, the sign left open (the device's default NaN is positive, x86's negative) --, info 0, the
                             status unchanged
    need, oracle info > 0    info the oracle's, status bit 2 (ST_CHOL_FAIL), R, R2, iC bit for bit what they were before the call
    need == 0                everything as before the call, info the sentinel

The chains of a layout go round five kinds -- succeeding, failing at pivot 1, failing at a seam, failing at the last pivot, need = 0 --
so that any four neighbours differ.  Every layout holds zero_meets_inf, subn and diagonal among its succeeding chains; a case runs as
many layouts (an engine and a probe call each) as it takes for the delayed-rejection case to hold every succeeding family and for the
two cases of a form to hold every failing one -- one up to npar 17, two above (test_layouts_hold_every_family).

Out of reach: the upper end of adapt_post_kernel<false,true> (npar 4096: the matrices alone take 4 GB per buffer).  After a successful
dpotf2 dpotri's zero-diagonal event cannot happen (a positive pivot's root, scaled, is not zero), so ST_POTRI_FAIL is pinned on the one
form that reaches it, the SVD instance with delayed rejection."""
import numpy as np
import pytest

import factor_cases as fc
from svd_cases import bits

pytestmark = pytest.mark.gpu

NMAT = 83
ST_CHOL_FAIL, ST_POTRI_FAIL = 2, 4
_REF = {}


def _engine(monkeypatch, d, nch, tile, drscale, condmax=0.0):
    from mcmcf90_amd import engine_from_problem
    monkeypatch.delenv("MCMCX_GROUP", raising=False)
    if tile is None:
        monkeypatch.delenv("MCMCX_TILE_FACTOR", raising=False)
    else:
        monkeypatch.setenv("MCMCX_TILE_FACTOR", str(tile))
    ckw = dict(nsimu=60, adaptint=50, updatesigma=0, drscale=drscale, condmax=condmax)
    pkw = dict(kind="gauss", npar=d, par0=np.zeros(d), cmat0=(0.5 / d) * np.eye(d), mu=np.zeros(d), lam=np.eye(d))
    e = engine_from_problem(ckw, pkw, nchains=nch)
    e.init()
    return e, ckw, pkw


def _oracle(oracle, d, A, key, ckw, pkw):
    k = (d, key, ckw["drscale"], ckw["condmax"])
    if k not in _REF:
        _REF[k] = oracle.calculate_R(oracle.make_cfg(**ckw), A, cmat0=pkw["cmat0"])
    return _REF[k]


def _state(e, chains, dr):
    out = {}
    for c in chains:
        R2, iC = e.dr_state(c) if dr else (None, None)
        out[c] = (e.R(c), R2, iC, e.counters(c)["status"])
    return out


def _same(a, b, nan_sign_open):
    return fc.same_bits_nan_sign_open(a, b) if nan_sign_open else fc.same_bits(a, b)


def _check(oracle, monkeypatch, d, names, need, tile, drscale, want_forms, mats=None):
    """One engine, one probe call on cases(d)[names] (or mats); every chain against the oracle and against its own state before the
    call.  Returns {chain: (R, R2, iC, status, info)}."""
    from mcmcf90_amd.engine import INFO_SENTINEL
    n = len(names)
    A = np.stack([fc.cases(d)[k][0] for k in names]) if mats is None else np.stack(mats)
    e, ckw, pkw = _engine(monkeypatch, d, n, tile, drscale)
    try:
        dr = drscale > 0.0
        before = _state(e, range(n), dr)
        cov0 = e.chaincov(0)[0]
        info, forms = e.debug_calculate_R(A, need=need)
        assert forms == want_forms, (forms, want_forms)
        after = _state(e, range(n), dr)
        out = {}
        for c, k in enumerate(names):
            R, R2, iC, st = after[c]
            R0, R20, iC0, st0 = before[c]
            out[c] = (R, R2, iC, st, int(info[c]))
            what = (d, c, k, tile, drscale)
            if need is not None and not need[c]:
                assert info[c] == INFO_SENTINEL and st == st0 and fc.same_bits(R, R0), what
                assert not dr or (fc.same_bits(R2, R20) and fc.same_bits(iC, iC0)), what
                assert fc.same_bits(e.chaincov(c)[0], cov0), what
                continue
            o = _oracle(oracle, d, A[c], k, ckw, pkw)
            assert info[c] == o.info, what + (int(info[c]), o.info)
            if o.info == 0:
                assert st == st0, what
                assert _same(np.triu(R), np.triu(o.R), True), what
                assert not dr or (_same(np.triu(R2), np.triu(o.R2), True) and _same(np.triu(iC), np.triu(o.iC), True)), what
            else:
                assert o.info > 0 and st == st0 | ST_CHOL_FAIL, what + (st,)
                assert fc.same_bits(R, R0) and (not dr or (fc.same_bits(R2, R20) and fc.same_bits(iC, iC0))), what
        return out
    finally:
        e.close()


PINNED = ("zero_meets_inf", "subn", "diagonal")          # in every layout: they decide the zero skips of dtrmv and dgemv
_KINDS = {}


def _kinds(oracle, d):
    """{kind: [family names]} by the oracle's dpotf2 on every family of cases(d): 0 succeeding (the pinned three first), 1 failing at
    pivot 1, 2 failing at a seam (any pivot that is neither the first nor the last; where npar has none, any failure), 3 failing at
    the last pivot.  The seam failures are ordered seam-major within a kind of pivot (neg_at at every seam, then zero_at, ...), so
    that a slice holds every seam."""
    if d not in _KINDS:
        import ctypes as C
        L = oracle.lib()
        kinds = {0: [], 1: [], 2: [], 3: []}
        for k, (A, want) in fc.cases(d).items():
            W = np.asfortranarray(np.array(A))
            info = int(L.mcxo_potrf_u(d, W.ctypes.data_as(C.POINTER(C.c_double))))
            assert want is None or want == info, (d, k)
            kinds[0 if info == 0 else 1 if info == 1 else 3 if info == d else 2].append(k)
        if not kinds[2]:
            kinds[2] = kinds[1] + kinds[3]
        if d == 1:
            kinds[3] = kinds[1]
        fam = ("neg_at", "zero_at", "negzero_at", "nan_diag", "nan_off")
        kinds[2].sort(key=lambda k: fam.index(k.split("(")[0]) if k.split("(")[0] in fam else len(fam))
        kinds[0] = [k for k in PINNED if k in kinds[0]] + [k for k in kinds[0] if k not in PINNED]
        _KINDS[d] = kinds
    return _KINDS[d]


def _slots(nmat, q):
    return len(range(q, nmat, 5))


def _layout(oracle, d, rot, nmat=NMAT):
    """names[nmat], need[nmat]: chain m is of kind m % 5 (_kinds; 4 = need 0, on dense), so that any four neighbours differ.  The
    succeeding chains are the pinned families and then a window of the others; every failing kind is a window of its families.  `rot`
    moves each window on by its own length, wrapping: layouts rot = 0 .. n - 1 together hold the first n windows."""
    kinds = _kinds(oracle, d)
    pick = {}
    for q in range(4):
        v, n = kinds[q], _slots(nmat, q)
        pin = [k for k in v if k in PINNED] if q == 0 else []
        rest = [k for k in v if k not in pin]
        w = max(n - len(pin), 0)
        pick[q] = iter((pin + [rest[(rot * w + i) % len(rest)] for i in range(w)] if rest else pin * n)[:n] if n else [])
    names, need = [], []
    for m in range(nmat):
        q = m % 5
        names.append(next(pick[q]) if q < 4 else "dense")
        need.append(0 if q == 4 else 1)
    return names, np.array(need, dtype=np.uint8)


def _nrounds(oracle, d, nmat=NMAT):
    """Layouts per (form, drscale) case: enough that the delayed-rejection case alone holds every succeeding family (only there does
    dpotri run) and that the two cases of a form together hold every failing family (which never reaches dpotri)."""
    kinds = _kinds(oracle, d)
    up = lambda a, b: -(-a // b) if a > 0 else 1
    npin = len([k for k in kinds[0] if k in PINNED])
    n = up(len(kinds[0]) - npin, max(_slots(nmat, 0) - npin, 1))
    for q in (1, 2, 3):
        n = max(n, up(len(kinds[q]), 2 * _slots(nmat, q)))
    return n


def _layouts(oracle, d, drscale):
    """the layouts of one (form, drscale) case: rounds 0 .. n - 1 with delayed rejection, n .. 2 n - 1 without"""
    n = _nrounds(oracle, d)
    return [_layout(oracle, d, r + (0 if drscale else n)) for r in range(n)]


POST, POSTG, TF = "adapt_post_kernel<false,false>", "adapt_post_kernel<false,true>", "tile_factor_kernel<%d,%d>"
# what plan_adapt's thresholds give each (switch, npar), written out: a moved threshold fails here
INSTANCES = {(1, 1): TF % (1, 4), (1, 2): TF % (1, 4), (1, 15): TF % (1, 4), (1, 16): TF % (1, 4),
             (1, 17): TF % (2, 4), (1, 31): TF % (2, 4), (1, 32): TF % (2, 4),
             (1, 33): TF % (3, 2), (1, 47): TF % (3, 2), (1, 48): TF % (3, 2),
             (1, 49): TF % (4, 1), (1, 63): TF % (4, 1), (1, 64): TF % (4, 1),
             (0, 1): POST, (0, 7): POST, (0, 8): POST, (0, 9): POST, (0, 15): POST, (0, 16): POST, (0, 17): POST, (0, 25): POST, (0, 63): POST,
             (0, 64): POST, (0, 65): POST, (0, 320): POST, (None, 321): POSTG}


def _forms(tile, d):
    name = INSTANCES[(tile, d)]
    return POST + ":3+" + name if tile == 1 else name


def test_instance_table_covers_every_instance_at_both_edges():
    """The literal table itself: each of the six forms at the first and the last npar of its range (the range of
    adapt_post_kernel<false,true> ends at npar 4096, out of reach)."""
    lo_hi = {}
    for (tile, d), name in INSTANCES.items():
        lo, hi = lo_hi.get(name, (d, d))
        lo_hi[name] = (min(lo, d), max(hi, d))
    assert lo_hi == {TF % (1, 4): (1, 16), TF % (2, 4): (17, 32), TF % (3, 2): (33, 48), TF % (4, 1): (49, 64), POST: (1, 320),
                     POSTG: (321, 321)}


def _params(sizes):
    """with delayed rejection (drscale = 2) and without (the whole file takes a few seconds: nothing here needs the extended marker)"""
    return [(d, dr) for d in sizes for dr in (2.0, 0.0)]


TILE_SIZES = [d for (t, d) in INSTANCES if t == 1]
LANE_SIZES = [d for (t, d) in INSTANCES if t == 0 and d <= 65]


@pytest.mark.parametrize("d", sorted(set(TILE_SIZES + LANE_SIZES)))
def test_layouts_hold_every_family(oracle, d):
    """What the cases below rely on, checked on the layouts themselves (no device): every layout holds the pinned families that exist at
    this npar -- zero_meets_inf from npar 4 on --; the delayed-rejection layouts of a size hold every succeeding family; the layouts of
    both cases of a form together hold every family of tests/factor_cases.py, so every kind of pivot stands at every seam in each form;
    and any four neighbouring chains are of four different kinds."""
    kinds = _kinds(oracle, d)
    dr, nodr = _layouts(oracle, d, 2.0), _layouts(oracle, d, 0.0)
    for names, need in dr + nodr + [_layout(oracle, d, 0, nmat=37)]:
        assert {k for k in PINNED if k in fc.cases(d)} <= set(names[0::5]), d
        assert (d < 4) == ("zero_meets_inf" not in names), d
        assert list(need) == [0 if m % 5 == 4 else 1 for m in range(len(names))]
        for m, k in enumerate(names):
            assert m % 5 == 4 or k in kinds[m % 5], (d, m, k)
    assert set(kinds[0]) <= {k for names, _ in dr for k in names}, d
    assert set(fc.cases(d)) <= {k for names, _ in dr + nodr for k in names}, d


@pytest.mark.parametrize("d,drscale", _params(TILE_SIZES))
def test_tile_forms(oracle, monkeypatch, d, drscale):
    """tile_factor_kernel<1,4>, <2,4>, <3,2>, <4,1> at both edges of their ranges and between: the 16-lane groups of a wave and the
    waves of a workgroup hold chains of all five kinds -- act / ok / go, __any(go), the flg[] hand-over to the cooperative write-back."""
    for names, need in _layouts(oracle, d, drscale):
        _check(oracle, monkeypatch, d, names, need, 1, drscale, _forms(1, d))


@pytest.mark.parametrize("d,drscale", _params(LANE_SIZES))
def test_lane_form(oracle, monkeypatch, d, drscale):
    """calculate_R and potri_packed in adapt_post_kernel<false,false>: npar mod 8 = 1, 7, 0 for the eight-wide clamped trips, both sides
    of the 8 x 8 block seams, a wave's lanes of all five kinds."""
    for names, need in _layouts(oracle, d, drscale):
        _check(oracle, monkeypatch, d, names, need, 0, drscale, _forms(0, d))


@pytest.mark.parametrize("tile,d", [(0, 320), (None, 321)])
def test_lane_form_at_the_lds_threshold(oracle, monkeypatch, tile, d):
    """npar 320 is the last size whose work vector fits LDS, 321 the first in global scratch (adapt_post_kernel<false,true>): dpotf2 only
    (a lane runs ~npar^3 / 3 dependent fmas), on dense, a failure in the middle and the zero matrix, and a chain that does not recompute."""
    names = ["dense", "neg_at(%d)" % (d // 2), "zero", "dense"]
    dense = np.array(fc.svd_cases.cases(d)["dense"])
    neg = dense.copy(); neg[d // 2, d // 2] = -1.0
    out = _check(oracle, monkeypatch, d, names, np.array([1, 1, 1, 0], dtype=np.uint8), tile, 0.0, _forms(tile, d),
                 mats=[dense, neg, np.zeros((d, d)), dense])
    assert [out[c][4] for c in range(3)] == [0, d // 2 + 1, 1]


@pytest.mark.parametrize("d", [16, 32, 48, 64])
def test_tile_lane_and_host_forms_agree(oracle, monkeypatch, d):
    """R, R2, iC and info bit for bit between tile_factor_kernel and the lane form -- no allowance at all between two device forms -- and
    the host's statement (the sign of a NaN open: a host compiler's)."""
    from mcmcf90_amd.engine import debug_host_calculate_R
    names, need = _layout(oracle, d, 0, nmat=37)
    need[:] = 1
    a = _check(oracle, monkeypatch, d, names, need, 1, 2.0, _forms(1, d))
    b = _check(oracle, monkeypatch, d, names, need, 0, 2.0, POST)
    for c, k in enumerate(names):
        for x, y in zip(a[c][:3], b[c][:3]):
            assert fc.same_bits(x, y), (d, c, k)
        assert a[c][3:] == b[c][3:], (d, c, k)
        Rh, iCh, ih, ih2 = debug_host_calculate_R(fc.cases(d)[k][0])
        assert ih == a[c][4] and ih2 == 0, (d, c, k)
        if ih == 0:
            assert fc.same_bits_nan_sign_open(Rh, np.triu(a[c][0])) and fc.same_bits_nan_sign_open(iCh, np.triu(a[c][2])), (d, c, k)


@pytest.mark.parametrize("which", ["nobody recomputes", "everybody fails"])
def test_whole_workgroups(oracle, monkeypatch, which):
    """A whole workgroup of need = 0 (tile_factor_kernel's first __syncthreads_or return) and a whole workgroup of failing chains (its
    return before dpotri), next to workgroups with work: npar 17, sixteen chains per workgroup, so chains 16 .. 31 are one."""
    d = 17
    names, need = _layout(oracle, d, 0)
    fails = [k for k, (A, want) in fc.cases(d).items() if want]
    for c in range(16, 32):
        if which == "nobody recomputes":
            need[c] = 0
        else:
            names[c], need[c] = fails[c % len(fails)], 1
    _check(oracle, monkeypatch, d, names, need, 1, 2.0, _forms(1, d))
    _check(oracle, monkeypatch, d, names, need, 0, 2.0, _forms(0, d))


def _svd_mats(d):
    return [("dense", fc.cases(d)["dense"][0]), ("lowrank", fc.cases(d)["lowrank"][0]), ("zero", np.zeros((d, d))),
            ("ascending", np.diag(np.arange(1.0, d + 1)))]


def _check_svd(oracle, monkeypatch, d, want_post):
    """The SVD instance with delayed rejection: dense, lowrank (floored: the rewritten covariance is compared), zero (info = npar, status
    bit 2, everything kept) and an ascending diagonal, whose U is a permutation with a zero on its diagonal: dpotri's event.  The
    reference has stopped there (the oracle returns -2000 - info2), so the project's own statement decides: status bit 4, iC keeps its
    previous bits, R is the new factor and R2 = R / drscale.  The four twice over, so that a wave holds every outcome more than once."""
    mats = _svd_mats(d) * 2
    n = len(mats)
    e, ckw, pkw = _engine(monkeypatch, d, n, None, 2.0, condmax=1e10)
    try:
        before = _state(e, range(n), True)
        info, forms = e.debug_calculate_R(np.stack([m for _, m in mats]))
        assert forms.startswith(want_post), forms
        after = _state(e, range(n), True)
        for c, (k, A) in enumerate(mats):
            o = _oracle(oracle, d, A, k, ckw, pkw)
            R, R2, iC, st = after[c]
            R0, R20, iC0, st0 = before[c]
            what = (d, c, k)
            if k == "zero":
                assert o.info == d and info[c] == d and st == st0 | ST_CHOL_FAIL, what
                assert fc.same_bits(R, R0) and fc.same_bits(R2, R20) and fc.same_bits(iC, iC0), what
            elif k == "ascending":
                assert o.info == -2001 and info[c] == 0 and st == st0 | ST_POTRI_FAIL, what + (o.info, int(info[c]), st)
                assert fc.same_bits(R, o.R), what                                      # the new factor
                assert fc.same_bits(R2, o.R / 2.0), what                               # R2 = R / drscale
                assert fc.same_bits(iC, iC0), what                                     # the inverse it had
            else:
                assert o.info == 0 and info[c] == 0 and st == st0, what
                assert o.floored == (1 if k == "lowrank" else 0), what
                assert fc.same_bits(R, o.R) and fc.same_bits(R2, o.R2) and fc.same_bits(np.triu(iC), np.triu(o.iC)), what
                assert fc.same_bits(np.triu(e.chaincov(c)[0]), np.triu(o.cmat)), what
        return forms
    finally:
        e.close()


@pytest.mark.parametrize("d", [2, 8, 9, 17])
def test_svd_instance_with_delayed_rejection(oracle, monkeypatch, d):
    assert _check_svd(oracle, monkeypatch, d, "adapt_post_kernel<true,false>") == "adapt_post_kernel<true,false>"


@pytest.mark.extended
def test_blocked_svd_instance_with_delayed_rejection(oracle, monkeypatch):
    """npar 48: the factorisation cut around the blocked SVD (phases 1 and 2 of adapt_post_kernel<true,false>)"""
    forms = _check_svd(oracle, monkeypatch, 48, "adapt_post_kernel<true,false>:1+")
    assert forms == "adapt_post_kernel<true,false>:1+svd_sweep_stream32_kernel<8>+svd_applyv_stream32_kernel<4>+adapt_post_kernel<true,false>:2"


def test_refusals_launch_nothing_and_write_nothing(monkeypatch):
    """-57 for a null argument, a len too small, an engine that is not initialised, pooled, method = 'ram' or without adaptation; the
    engine's factors, covariance and status, the caller's info and forms are as before."""
    import ctypes as C
    from mcmcf90_amd import engine_from_problem, _lib
    L = _lib.load()
    d, n = 5, 3
    DP, IP, UP = C.POINTER(C.c_double), C.POINTER(C.c_int32), C.POINTER(C.c_uint8)
    pkw = dict(kind="gauss", npar=d, par0=np.zeros(d), cmat0=(0.5 / d) * np.eye(d), mu=np.zeros(d), lam=np.eye(d))
    A = np.ascontiguousarray(np.stack([fc.cases(d)["dense"][0]] * n))

    def call(e, null=None, ln=128, h=True):
        info = np.full(n, 7, dtype=np.int32); buf = C.create_string_buffer(b"\x55" * 127, 128)
        rc = L.mcmcx_debug_calculate_R(e.h if h else None, None if null == "cmat" else A.ctypes.data_as(DP), None,
                                       None if null == "info" else info.ctypes.data_as(IP), buf, ln)
        assert rc == -57 and np.all(info == 7) and buf.raw[:127] == b"\x55" * 127, (null, ln, rc, L.mcmcx_last_error())
        return L.mcmcx_last_error()

    monkeypatch.setenv("MCMCX_TILE_FACTOR", "1")
    e = engine_from_problem(dict(nsimu=60, adaptint=50, updatesigma=0, drscale=2.0), pkw, nchains=n)
    assert b"not initialised" in call(e)
    e.init()
    before = (_state(e, range(n), True), [e.chaincov(c)[0] for c in range(n)])
    assert b"null" in call(e, h=False) and b"null" in call(e, null="cmat") and b"null" in call(e, null="info")
    want = POST + ":3+" + TF % (1, 4)
    assert b"len" in call(e, ln=len(want)) and b"len" in call(e, ln=0)
    after = (_state(e, range(n), True), [e.chaincov(c)[0] for c in range(n)])
    for c in range(n):
        for x, y in zip(before[0][c][:3], after[0][c][:3]):
            assert fc.same_bits(x, y)
        assert before[0][c][3] == after[0][c][3] and fc.same_bits(before[1][c], after[1][c])
    info, forms = e.debug_calculate_R(A)                    # ... and the same engine accepts the call with the buffer one byte longer
    assert forms == want and np.all(info == 0)
    e.close()
    for ckw, extra, frag in ((dict(method="ram"), {}, b"ram"), (dict(doadapt=0, doburnin=0), {}, b"no adaptation"), ({}, dict(pooled=1), b"pooled")):
        e = engine_from_problem(dict(nsimu=60, adaptint=50, updatesigma=0, **ckw), pkw, nchains=n, **extra)
        e.init()
        assert frag in call(e), frag
        e.close()
