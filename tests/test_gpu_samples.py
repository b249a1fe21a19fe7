"""Thinned samples of all chains, kept on the device (mcmcx_set_samples / mcmcx_get_samples / mcmcx_get_samples_dev, include/mcmcx.h).

The feature is a copy, so every comparison is on raw bits.  Per kernel family (FORMS), one run with sampling on against
1. the recorded chain of the same run (record_chain: the history ring, decoded on the host -- an independent path),
2. an engine without sampling that is stepped to every kept iteration (run(i), theta(), scalars()) -- after checking that stepping
   itself leaves that engine where one call leaves a third,
3. that third engine: sampling does not move the run (state, scalars, stream positions, factors, counters, totals, the kernel run).
Then the two kernels' shapes (chain counts around a tile, npar around the transposing read's field block, windows of chains and of
samples, both layouts, host and device form, the ring wrapped and not), and the refusals."""
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SWITCHES = ("MCMCX_GROUP", "MCMCX_GROUP_GW", "MCMCX_RAM_GROUP", "MCMCX_SCAM_WAVES", "MCMCX_POOLED_WAVES", "MCMCX_POOLED_PHASE_MFMA",
            "MCMCX_RAM_WIDE", "MCMCX_LDS_SCRATCH", "MCMCX_DR_BIG", "MCMCX_HOST_FUSE", "MCMCX_COLS_PHASED")


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _gauss(d, seed, **kw):
    rng = np.random.default_rng(seed)
    A = rng.standard_normal((d, d)) / np.sqrt(d)
    return dict(dict(kind="gauss", npar=d, par0=np.full(d, 0.05), cmat0=(0.5 / d) * np.eye(d), mu=np.linspace(-1, 1, d) if d > 1 else np.zeros(1),
                     lam=A @ A.T + np.eye(d)), **kw)


def _banana(d):
    return dict(kind="banana", npar=d, par0=np.full(d, 0.05), cmat0=(2.0 / d) * np.eye(d), b=0.1)


def _cols3():
    x = np.linspace(0.0, 6.0, 21)
    rng = np.random.default_rng(5)
    y = np.stack([1.5 * np.exp(-k * x) + 0.05 * rng.standard_normal(x.size) for k in (0.4, 0.7, 1.1)])
    return dict(kind="expdata", npar=4, par0=np.array([1.4, 0.5, 0.6, 1.0]), cmat0=0.002 * np.eye(4), xdata=x, ydata=y,
                sigma2=np.full(3, 0.01), nobs=np.full(3, x.size))


_HOST_LAM = np.array([[2.0, 0.3, 0.0], [0.3, 1.0, 0.2], [0.0, 0.2, 1.5]])


def _host_ss(th):
    return float(th @ (_HOST_LAM @ th))


def _host_ss2(th):                                              # two response columns
    return np.array([_host_ss(th), float(th @ th) + 0.5 * th[0]])


def _host_prior(th):
    return float(((th - 0.1) / 2.0) @ ((th - 0.1) / 2.0))


# name -> switches, configuration, problem (or "host" / "module"), chains, the kernel mcmcx_last_kernel must name, (first, thin)
# thin = 7 divides no adaptint here; "lane_am_tick" keeps exactly the adaptation ticks (thin == adaptint)
FORMS = {
    "lane_am": (dict(MCMCX_GROUP="0"), dict(nsimu=120, adaptint=50, updatesigma=1), _gauss(7, 1, sigma2=0.8, nobs=12), 130,
                "step_kernel_ldsr", (3, 7)),
    "lane_am_tick": (dict(MCMCX_GROUP="0"), dict(nsimu=120, adaptint=10, updatesigma=1), _gauss(7, 1, sigma2=0.8, nobs=12), 130,
                     "step_kernel_ldsr", (10, 10)),
    "lane_dr": (dict(MCMCX_GROUP="0"), dict(nsimu=120, adaptint=50, drscale=2.0, updatesigma=0), _banana(5), 130, "step_kernel_dr", (3, 7)),
    "group_quad": (dict(MCMCX_GROUP="1", MCMCX_GROUP_GW="4"), dict(nsimu=120, adaptint=50, updatesigma=0), _gauss(10, 2), 130,
                   "group_step_kernel<quad>", (1, 7)),
    "group_dr": (dict(MCMCX_GROUP="1"), dict(nsimu=120, adaptint=50, drscale=3.0, updatesigma=0), _gauss(20, 3), 130,
                 "group_step_kernel<DR>", (3, 7)),
    "ram_lane": (dict(MCMCX_GROUP="0"), dict(nsimu=120, method="ram", adaptint=100, updatesigma=0), _gauss(7, 4), 130,
                 "step_kernel_ram_ldsr", (3, 7)),
    "ram_group": (dict(MCMCX_RAM_GROUP="1"), dict(nsimu=120, method="ram", adaptint=100, updatesigma=0), _gauss(12, 5), 70,
                  "group_ram_kernel", (3, 7)),
    "ram_wide": (dict(MCMCX_GROUP="0", MCMCX_RAM_WIDE="1"), dict(nsimu=100, method="ram", adaptint=100, updatesigma=0), _gauss(21, 6), 70,
                 "step_kernel_ram_wide", (3, 7)),
    "scam": (dict(MCMCX_SCAM_WAVES="1"), dict(nsimu=60, method="scam", adaptint=25, updatesigma=0), _gauss(6, 7), 70, "scam_kernel", (3, 7)),
    "pooled_mfma": (dict(MCMCX_POOLED_WAVES="1"), dict(nsimu=120, adaptint=50, updatesigma=0, pooled=1), _gauss(20, 8), 130,
                    "pooled_mfma_kernel<false>", (3, 7)),
    "pooled_scam": (dict(), dict(nsimu=50, method="scam", adaptint=20, updatesigma=0, pooled=1), _gauss(20, 9), 130, "scam_pooled_kernel",
                    (3, 7)),
    "host": (dict(), dict(nsimu=60, adaptint=25, updatesigma=1), "host", 66, "", (3, 7)),
    "host_pooled": (dict(), dict(nsimu=60, adaptint=25, updatesigma=1, pooled=1), "host", 66, "pooled_phase_kernel", (3, 7)),
    # host callbacks with nycol = 2: the per-column vectors E.ssv / E.s2v through host_phase_kernel
    "host_ny2": (dict(), dict(nsimu=60, adaptint=25, drscale=2.0, updatesigma=1), "host2", 66, "", (3, 7)),
    "module_ny2": (dict(), dict(nsimu=100, adaptint=40, drscale=2.0, updatesigma=1), "module", 70, "", (3, 7)),
    "cols3": (dict(), dict(nsimu=120, adaptint=50, updatesigma=1), _cols3(), 130, "step_kernel_cols", (3, 7)),
    # the response-column target with its phases in separate launches (no table entry names them: "")
    "cols3_phased": (dict(MCMCX_COLS_PHASED="1"), dict(nsimu=120, adaptint=50, updatesigma=1), _cols3(), 130, "", (3, 7)),
}


@pytest.fixture(scope="module")
def user_module(tmp_path_factory):
    """tests/test_gpu_user_module.py's target source, compiled the way its own fixture compiles the code object."""
    from test_gpu_user_module import USER_SRC
    d = tmp_path_factory.mktemp("samplesmod")
    src = d / "user_target.hip"
    src.write_text(USER_SRC)
    hsaco = d / "user_target.hsaco"
    subprocess.check_call(["/opt/rocm/bin/hipcc", "--genco", "--offload-arch=gfx950", "-O2", "-ffp-contract=off",
                           "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(hsaco)])
    return str(hsaco)


def _engine(name, user_module, samples=None):
    """A form's engine, inited; samples = (first, thin, capacity) or None."""
    from mcmcf90_amd import Engine, engine_from_problem, make_config
    _, ckw, prob, nch, _, _ = FORMS[name]
    if prob in ("host", "host2"):
        e = Engine(make_config(3, nch, record_chain=1, chain_id0=5, **ckw))
        e.setpar0(np.array([0.2, -0.1, 0.3])); e.setcmat0(0.3 * np.eye(3))
        if prob == "host":
            e.setsigma2nobs(0.9, 14)
        else:
            e.setsigma2nobs(np.array([0.9, 1.4]), np.array([14, 9]))
        e.set_target_host(_host_ss if prob == "host" else _host_ss2, priorfun=_host_prior,
                          checkbounds=lambda th: bool(np.all(np.abs(th) < 4.0)))
    elif prob == "module":
        npar, ny = 5, 2
        data = np.concatenate([np.random.default_rng(11).uniform(0.5, 2.0, npar), [0.3]])
        e = Engine(make_config(npar, nch, record_chain=1, chain_id0=5, **ckw))
        e.setpar0(np.full(npar, 0.1)); e.setcmat0(0.05 * np.eye(npar)); e.setsigma2nobs(np.full(ny, 0.8), np.full(ny, 15))
        e.set_target_module(user_module, "user_target", data)
    else:
        e = engine_from_problem(ckw, prob, nchains=nch, record_chain=1, chain_id0=5)
    if samples is not None:
        e.set_samples(*samples)
    e.init()
    return e


def _final(e, chains, pooled):
    out = dict(theta=_bits(e.theta()), scal=_bits(e.scalars()), rng=[e.rng(c) for c in chains], ctr=[e.counters(c) for c in chains],
               totals=e.totals(), kernel=e.last_kernel(), simuind=e.simuind)
    out["R"] = [_bits(x) for x in e.pooled()[:2]] + [e.pooled()[2], _bits(e.pooled()[3])] if pooled else [_bits(e.R(c)) for c in chains]
    return out


def _same_final(a, b, what):
    for k in ("theta", "scal"):
        assert np.array_equal(a[k], b[k]), (what, k)
    for k in ("rng", "ctr", "totals", "kernel", "simuind"):
        assert a[k] == b[k], (what, k, a[k], b[k])
    for x, y in zip(a["R"], b["R"]):
        assert np.array_equal(x, y), (what, "factor")


@pytest.mark.parametrize("name", list(FORMS))
def test_samples_of_every_kernel_family(name, user_module, monkeypatch):
    from mcmcf90_amd.engine import sample_iterations, sample_nfields
    env, ckw, prob, nch, kernel, (first, thin) = FORMS[name]
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    nsimu, pooled = ckw["nsimu"], bool(ckw.get("pooled"))
    assert thin == ckw["adaptint"] or ckw["adaptint"] % thin != 0
    chains = sorted({0, 63, 64, nch - 1})                       # the first, the last, one on each side of a tile boundary
    kept = sample_iterations(first, thin, nsimu, nsimu)

    # A: one call, sampling on
    A = _engine(name, user_module, (first, thin, None))
    assert A.run() == 0
    assert A.last_kernel() == kernel, A.last_kernel()
    d, ny = A.npar, getattr(A, "nycol", 1)
    n, oldest, th, nf = A.samples_kept()
    assert (n, oldest, th, nf) == (len(kept), kept[0], thin, sample_nfields(d, ny))
    its, S = A.samples()                                        # [ns][nchains][nfields]
    assert list(its) == kept and S.shape == (len(kept), nch, nf)
    fa = _final(A, chains, pooled)

    # 1. against the recorded chain of the same run: run-length rows expanded to one row per iteration
    for c in chains:
        ch, ss, s2 = A.chain(c)
        th_it = np.repeat(ch[:, :d], ch[:, d].astype(int), axis=0)
        ss_it = np.repeat(ss[:, :ny], ss[:, ny].astype(int), axis=0)
        assert len(th_it) == len(ss_it) == nsimu
        s2 = np.asarray(s2).reshape(nsimu, ny)
        for s, i in enumerate(kept):
            assert np.array_equal(_bits(S[s, c, :d]), _bits(th_it[i - 1])), (name, "theta", c, i)
            assert np.array_equal(_bits(S[s, c, d:d + ny]), _bits(ss_it[i - 1])), (name, "ss", c, i)
            if ckw["updatesigma"]:
                assert np.array_equal(_bits(S[s, c, d + ny + 1:]), _bits(s2[i - 1])), (name, "sigma2", c, i)
    if not ckw["updatesigma"]:                                  # no s2chain then: sigma2 stays what MCMC_setsigma2nobs gave
        s20 = np.atleast_1d(np.asarray(prob["sigma2"] if isinstance(prob, dict) and "sigma2" in prob else 1.0, dtype=np.float64))
        assert np.array_equal(_bits(S[:, :, d + ny + 1:]), _bits(np.broadcast_to(s20, (len(kept), nch, ny))))
    A.close()

    # C: one call, no sampling.  3. sampling does not move the run
    Cc = _engine(name, user_module)
    assert Cc.run() == 0
    fc = _final(Cc, chains, pooled)
    Cc.close()
    _same_final(fa, fc, (name, "sampling on against off"))

    # 2. B: no sampling, stepped to every kept iteration
    B = _engine(name, user_module)
    stepped = []
    for i in kept:
        assert B.run(i) == 0 and B.simuind == i
        stepped.append((B.theta(), B.scalars()))
    assert B.run() == 0
    fb = _final(B, chains, pooled)
    B.close()
    _same_final(fb, fc, (name, "stepping against one call: a defect of the engine's launch cut, not of the sample store"))
    for s, (i, (theta, scal)) in enumerate(zip(kept, stepped)):
        assert np.array_equal(_bits(S[s, :, :d]), _bits(theta)), (name, "theta", i)
        assert np.array_equal(_bits(S[s, :, d]), _bits(scal[:, 0])), (name, "ss (column 1)", i)
        assert np.array_equal(_bits(S[s, :, d + ny]), _bits(scal[:, 1])), (name, "sspri", i)
        assert np.array_equal(_bits(S[s, :, d + ny + 1]), _bits(scal[:, 2])), (name, "sigma2 (column 1)", i)


# ---------------------------------------------------------------- the two kernels' shapes
NSIMU, FIRST, THIN = 40, 1, 3                                   # keeps 1, 4, ..., 40: fourteen samples


def _shape_engine(nch, d, samples=None):
    from mcmcf90_amd import engine_from_problem
    e = engine_from_problem(dict(nsimu=NSIMU, adaptint=15, updatesigma=1), _gauss(d, 20 + d, sigma2=0.7, nobs=9), nchains=nch, chain_id0=2)
    if samples is not None:
        e.set_samples(*samples)
    e.init()
    return e


_STEPPED = {}


def _stepped(nch, d):
    """[14][nch][npar + 3] from an engine without sampling, stepped to every kept iteration: computed once per shape, never changed."""
    from mcmcf90_amd.engine import sample_iterations
    if (nch, d) not in _STEPPED:
        e = _shape_engine(nch, d)
        rows = []
        for i in sample_iterations(FIRST, THIN, NSIMU, NSIMU):
            e.run(i)
            rows.append(np.concatenate([e.theta(), e.scalars()[:, :3]], axis=1))
        e.close()
        ref = np.stack(rows)
        ref.setflags(write=False)
        _STEPPED[(nch, d)] = ref
    return _STEPPED[(nch, d)]


def _windows(nch):
    w = {(0, nch), (nch - 1, 1)}
    if nch > 1:
        w.add((1, 1))
    if nch == 130:
        w |= {(63, 2), (60, 70)}
    return sorted(w)


def _check_windows(e, ref_retained, nch, sample_windows, torch_too):
    """Both layouts of every (sample window, chain window) against the stepped reference; layout 1 = layout 0 transposed; device = host."""
    for s0, ns in sample_windows:
        for c0, nc in _windows(nch):
            want = ref_retained[s0:s0 + ns, c0:c0 + nc]
            its, a0 = e.samples(s0, ns, c0, nc, layout=0)
            _, a1 = e.samples(s0, ns, c0, nc, layout=1)
            assert a0.shape == want.shape and np.array_equal(_bits(a0), _bits(want)), (s0, ns, c0, nc)
            assert np.array_equal(_bits(a1), _bits(a0.transpose(0, 2, 1))), (s0, ns, c0, nc, "layout 1")
            if torch_too:
                for layout, host in ((0, a0), (1, a1)):
                    it2, t = e.samples_torch(s0, ns, c0, nc, layout=layout)
                    assert t.is_cuda and str(t.dtype) == "torch.float64" and list(it2) == list(its)
                    assert np.array_equal(_bits(t.cpu().numpy()), _bits(host)), (s0, ns, c0, nc, layout, "device form")


# npar 62 is the smallest whose nfields = npar + 3 = 65 passes the transposing read's block of 64 fields (mcx_samples.hpp: SAMP_FB): its
# loop over field blocks runs twice, the second time for one field
@pytest.mark.parametrize("d", [1, 2, 7, 50, 62])
@pytest.mark.parametrize("nch", [1, 63, 64, 65, 130])
def test_sample_kernels_over_chain_counts_and_npar(nch, d):
    """A ring of five under fourteen kept iterations (wrapped twice): retained samples 9 .. 13 sit in slots 4, 0, 1, 2, 3, so the windows
    (0, 2) and (0, 5) straddle the wrap point."""
    from mcmcf90_amd.engine import sample_iterations
    ref = _stepped(nch, d)
    e = _shape_engine(nch, d, (FIRST, THIN, 5))
    e.run()
    kept = sample_iterations(FIRST, THIN, 5, NSIMU)
    assert e.samples_kept() == (5, kept[0], THIN, d + 3) and kept == [28, 31, 34, 37, 40]
    _check_windows(e, ref[-5:], nch, [(0, 5), (0, 1), (4, 1), (0, 2), (2, 3)], torch_too=(nch in (65, 130) or d == 62))
    assert list(e.samples()[0]) == kept
    e.close()


@pytest.mark.parametrize("capacity", [1, 3, 100])
def test_ring_capacities(capacity):
    """capacity 1 and 3 under fourteen kept iterations (more than 2 x capacity), and a ring larger than the kept count."""
    from mcmcf90_amd.engine import sample_iterations
    nch, d = 130, 7
    ref = _stepped(nch, d)
    e = _shape_engine(nch, d, (FIRST, THIN, capacity))
    e.run()
    kept = sample_iterations(FIRST, THIN, capacity, NSIMU)
    n = min(capacity, 14)
    assert e.samples_kept() == (n, kept[0], THIN, d + 3) and len(kept) == n
    wins = [(s0, ns) for s0 in range(n) for ns in range(1, n - s0 + 1)] if n <= 3 else [(0, n), (0, 1), (n - 1, 1), (5, 4)]
    _check_windows(e, ref[-n:], nch, wins, torch_too=True)
    e.close()


def test_first_iteration_is_the_start_point():
    """first = 1: the state mcmcx_init leaves -- par0 and the init evaluation's ss -- is sample 0, stored at init."""
    nch, d = 65, 7
    e = _shape_engine(nch, d, (1, THIN, 100))
    assert e.simuind == 1 and e.samples_kept() == (1, 1, THIN, d + 3)
    its, S = e.samples()
    assert list(its) == [1] and S.shape == (1, nch, d + 3)
    assert np.array_equal(_bits(S[0, :, :d]), _bits(np.broadcast_to(_gauss(d, 20 + d)["par0"], (nch, d))))
    assert np.array_equal(_bits(S[0, :, d:]), _bits(e.scalars()[:, :3]))
    assert np.array_equal(_bits(S[0]), _bits(_stepped(nch, d)[0]))
    e.close()


def test_first_beyond_nsimu_keeps_nothing():
    nch, d = 65, 2
    e = _shape_engine(nch, d, (NSIMU + 1, 1, 4))
    e.run()
    assert e.samples_kept() == (0, NSIMU + 1, 1, d + 3)
    for layout, shape in ((0, (0, nch, d + 3)), (1, (0, d + 3, nch))):
        its, S = e.samples(layout=layout)
        assert len(its) == 0 and S.shape == shape
        assert tuple(e.samples_torch(layout=layout)[1].shape) == shape
    e.close()


def test_sampling_off_by_default_and_switched_off_again():
    e = _shape_engine(65, 2)
    e.run()
    assert e.samples_kept()[0] == 0
    e.close()
    e = _shape_engine(65, 2, (1, 0, 0))
    e.run()
    assert e.samples_kept()[0] == 0
    e.close()


@pytest.mark.parametrize("k", [2, 17, 39])
def test_two_calls_keep_what_one_call_keeps(k):
    """run(k), run(nsimu) with k not a kept iteration: the launch is cut at k too, the store is the one call's."""
    from mcmcf90_amd.engine import sample_iterations
    nch, d = 130, 7
    assert k not in sample_iterations(FIRST, THIN, NSIMU, NSIMU)
    e = _shape_engine(nch, d, (FIRST, THIN, 100))
    e.run(k)
    n_k = len(sample_iterations(FIRST, THIN, 100, k))
    assert e.samples_kept()[0] == n_k
    assert np.array_equal(_bits(e.samples()[1]), _bits(_stepped(nch, d)[:n_k]))
    e.run()
    its, S = e.samples()
    assert list(its) == sample_iterations(FIRST, THIN, 100, NSIMU)
    assert np.array_equal(_bits(S), _bits(_stepped(nch, d)))
    e.close()


# ---------------------------------------------------------------- refusals: argument checks on the host, before any launch
def test_refusals_leave_the_engine_usable():
    import ctypes as C
    from mcmcf90_amd import engine_from_problem
    from mcmcf90_amd.engine import McmcError
    nch, d = 65, 2
    pkw = _gauss(d, 20 + d, sigma2=0.7, nobs=9)
    e = engine_from_problem(dict(nsimu=NSIMU, adaptint=15, updatesigma=1), pkw, nchains=nch, chain_id0=2)
    L = e.L
    for bad in ((0, 1, 4), (-3, 1, 4), (1, -1, 4), (1, 2, 0), (1, 2, -5)):
        rc = L.mcmcx_set_samples(e.h, *bad)
        assert rc == -47 and b"mcmcx_set_samples" in L.mcmcx_last_error(), (bad, rc)
    e.set_samples(FIRST, THIN, 5)
    e.init()
    rc = L.mcmcx_set_samples(e.h, 1, 1, 4)
    assert rc == -47 and b"after mcmcx_init" in L.mcmcx_last_error()
    with pytest.raises(McmcError):
        e.set_samples(1, 1, 4)
    e.run()
    buf = np.zeros(5 * nch * (d + 3))
    p = buf.ctypes.data_as(C.POINTER(C.c_double))
    for s0, ns, c0, nc, layout in ((-1, 1, 0, 1, 0), (0, 6, 0, 1, 0), (5, 1, 0, 1, 0), (0, 0, 0, 1, 0), (0, 1, -1, 1, 0), (0, 1, 0, nch + 1, 0),
                                   (0, 1, nch, 1, 0), (0, 1, 0, 0, 1), (0, 1, 0, 1, 2), (0, 1, 0, 1, -1), (2 ** 31 - 1, 2, 0, 1, 0),
                                   (0, 1, 2 ** 31 - 1, 2, 1)):
        for fn, out in ((L.mcmcx_get_samples, p), (L.mcmcx_get_samples_dev, C.c_void_p(8))):   # (refused before the pointer is looked at)
            rc = fn(e.h, s0, ns, c0, nc, layout, out)
            assert rc == -48 and len(L.mcmcx_last_error()) > 0, (s0, ns, c0, nc, layout, rc)
    assert L.mcmcx_get_samples(e.h, 0, 1, 0, 1, 0, None) < 0
    assert np.array_equal(_bits(e.samples()[1]), _bits(_stepped(nch, d)[-5:]))       # still usable, and unharmed
    e.close()
    # sampling off: nothing to read
    e = _shape_engine(nch, d)
    assert L.mcmcx_get_samples(e.h, 0, 1, 0, 1, 0, p) == -48
    e.close()


def test_refused_with_the_external_target():
    from mcmcf90_amd import engine_from_problem
    pkw = _gauss(2, 22)
    e = engine_from_problem(dict(nsimu=NSIMU), pkw, nchains=65, external=True)
    assert e.L.mcmcx_set_samples(e.h, 1, 2, 4) == -47 and b"external" in e.L.mcmcx_last_error()
    assert e.L.mcmcx_set_samples(e.h, 1, 0, 0) == 0             # switching it off is no request to sample
    e.init()                                                    # usable: MCMC_run1's arithmetic
    assert e.run1_propose(1, pkw["par0"]).shape == (65, 2)
    e.close()
    e = engine_from_problem(dict(nsimu=NSIMU), pkw, nchains=65)
    e.set_samples(1, 2, 4)
    e.set_target_external()                                     # the other order: mcmcx_init refuses
    assert e.L.mcmcx_init(e.h) == -47 and b"external" in e.L.mcmcx_last_error()
    e.close()
