"""User targets where the sum of squares or the prior is +inf or NaN (tests/edge_problems.py has the built-in target's side of this).

1. A target module that restates oracle/mcx_targets.h's mcxt_ss_gauss operation for operation, on the npar 20 overflow problem (ss = +inf in one
   proposal in eight, NaN in one in thirty): bit for bit the built-in Gaussian target -- per chain (the per-chain phase kernels, which carry no
   name in the kernel table: last_kernel() is "") and pooled in both phase forms (pooled_phase_kernel, pooled_phase_mfma_kernel).  The built-in
   target's chains are the oracle's (tests/test_gpu_every_chain.py), so this ties the user-target phases to the reference's decision at NaN.
2. A source with a hole, compiled for the device and for the host: ss = +inf where th[0] > 1, ss = NaN where th[1] > 1, the prior +inf where
   th[2] > 1, chosen by comparisons only (the values themselves come in through the data pointer, so neither compiler folds them).  For the
   dram, drscale, ram, er and scam configurations: module == host callbacks == batched host callbacks.  That every region was proposed into in
   every tile is counted by the host functions themselves (with delayed rejection: by first-stage proposals; the host run is then cut at every
   iteration, which changes nothing: it still equals the module's uncut run bit for bit)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import edge_problems as ep

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# oracle/mcx_targets.h: mcxt_ss_gauss, operation for operation.  data = mu[npar], lam[npar][npar] (row major)
GAUSS_SRC = r"""
#include "mcmcx_target.h"
__device__ void gauss_ss(const double *th, int d, int ny, const void *data, double *out)
{
    const double *mu = (const double *)data, *lam = mu + d;
    double ss = 0.0;
    for (int t0 = 0; t0 < d; t0 += 16)
        for (int k = 0; k < 4 && t0 + k < d; ++k) {
            double q = 0.0;
            for (int r = 0; r < 4; ++r) {
                const int i = t0 + k + 4 * r;
                if (i >= d) break;
                const double *row = lam + (long)i * d;
                double y = 0.0;
                for (int j = 0; j < d; ++j) y = fma(row[j], th[j] - mu[j], y);
                const double vi = th[i] - mu[i];
                q = (r == 0) ? y * vi : fma(y, vi, q);
            }
            ss = (t0 == 0 && k == 0) ? q : ss + q;
        }
    out[0] = ss;
}
__device__ double gauss_prior(const double *th, int npar, const void *data) { return 0.0; }
__device__ int gauss_bounds(const double *th, int npar, const void *data) { return 1; }
MCMCX_DEFINE_TARGET(gauss_target, gauss_ss, gauss_prior, gauss_bounds)
"""

# one source, two compilers (tests/test_gpu_user_module.py's pattern): arithmetic only, -ffp-contract=off.  data = w[npar], +inf, NaN.
# The host side counts, per tile of 64 chains, the proposals that fell into each region: host_bounds is called once per chain and pass, in chain
# order, before that chain's prior and sum of squares (mcx_host_callbacks.hpp).  Every pass visits every chain (the start point, an iteration's
# proposal, early rejection's, one SCAM component's), so the call count names the chain -- except delayed rejection's second-stage pass, which
# visits only the chains whose first stage rejected.  There the test runs one iteration per call and says so (begin_iteration): the first nch
# calls of an iteration are the first stage's, in chain order, and what follows is the second stage's, counted without a tile.
HOLE_SRC = r"""
#ifdef __HIPCC__
#include "mcmcx_target.h"
#define FN __device__
#else
#define FN
#endif
FN void user_ss(const double *th, int npar, int ny, const void *data, double *ss)
{
    const double *w = (const double *)data;
    double s = 0.0;
    for (int k = 0; k < npar; ++k) s = s + w[k] * (th[k] * th[k]);
    if (th[0] > 1.0) s = w[npar];                             /* +inf */
    if (th[1] > 1.0) s = w[npar + 1];                         /* NaN */
    ss[0] = s;
}
FN double user_prior(const double *th, int npar, const void *data)
{
    const double *w = (const double *)data;
    if (th[2] > 1.0) return w[npar];                          /* +inf */
    return 0.0;
}
FN int user_bounds(const double *th, int npar, const void *data) { return 1; }
#ifdef __HIPCC__
MCMCX_DEFINE_TARGET(hole_target, user_ss, user_prior, user_bounds)
#else
static const void *g_data;
static long g_nch, g_calls, g_iter_calls, g_by_iteration;
long g_hits[3][8];                                            /* [ss = +inf, ss = NaN, prior = +inf][tile]: passes over all chains */
long g_any[3];                                                /* ... every pass */
long g_stage2[3];                                             /* ... second-stage passes */
void set_data(const void *d, long nch)
{
    g_data = d; g_nch = nch; g_calls = 0; g_iter_calls = 0; g_by_iteration = 0;
    for (int r = 0; r < 3; ++r) { g_any[r] = 0; g_stage2[r] = 0; for (int t = 0; t < 8; ++t) g_hits[r][t] = 0; }
}
void begin_iteration(void) { g_by_iteration = 1; g_iter_calls = 0; }
long n_bounds_calls(void) { return g_calls; }
static void note(const double *th)
{
    const int stage2 = g_by_iteration && g_iter_calls >= g_nch;
    const long chain = g_iter_calls % g_nch;
    for (int r = 0; r < 3; ++r) if (th[r] > 1.0) { g_any[r]++; if (stage2) g_stage2[r]++; else g_hits[r][chain / 64]++; }
    g_iter_calls++; g_calls++;
}
void host_ss(const double *th, int npar, int ny, double *ss, void *user) { user_ss(th, npar, ny, g_data, ss); }
double host_prior(const double *th, int npar, void *user) { return user_prior(th, npar, g_data); }
int host_bounds(const double *th, int npar, void *user) { note(th); return user_bounds(th, npar, g_data); }
void host_ss_batch(const double *th, int npar, int n, int ny, double *ss, void *user)
{ for (int i = 0; i < n; ++i) user_ss(th + (long)i * npar, npar, ny, g_data, ss + (long)i * ny); }
#endif
"""


def _genco(d, name, text):
    src = d / (name + ".hip")
    src.write_text(text)
    hsaco = d / (name + ".hsaco")
    subprocess.check_call(["/opt/rocm/bin/hipcc", "--genco", "--offload-arch=gfx950", "-O2", "-ffp-contract=off",
                           "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(hsaco)])
    return str(hsaco)


@pytest.fixture(scope="module")
def gauss_module(tmp_path_factory):
    return _genco(tmp_path_factory.mktemp("gaussmod"), "gauss_target", GAUSS_SRC)


@pytest.fixture(scope="module")
def hole(tmp_path_factory):
    d = tmp_path_factory.mktemp("holemod")
    hsaco = _genco(d, "hole_target", HOLE_SRC)
    (d / "hole_target.c").write_text(HOLE_SRC)
    so = d / "libhole_host.so"
    subprocess.check_call(["gcc", "-O2", "-ffp-contract=off", "-shared", "-fPIC", str(d / "hole_target.c"), "-o", str(so)])
    H = C.CDLL(str(so))
    H.set_data.argtypes = [C.c_void_p, C.c_long]
    H.n_bounds_calls.restype = C.c_long
    H.begin_iteration.restype = None
    return hsaco, H


def _state(e, nch, pooled):
    s = dict(theta=e.theta(), masks=e.accept_masks(), scal=e.scalars(), rng=np.array([e.rng(c)[0] for c in range(nch)], dtype=np.uint64), totals=e.totals())
    if pooled:
        s["R"] = e.pooled()[3]
    return s


def _same(a, b, nch, what):
    """Bit for bit, except that a NaN equals a NaN whatever its sign and payload in the scalars (ss1, sspri1, sigma2, alpha12); the unused lanes
    of a ragged last tile never see a user callback and are masked out of the accept record."""
    assert np.array_equal(a["theta"].view(np.uint64), b["theta"].view(np.uint64)), (what, "theta")
    assert np.isfinite(a["theta"]).all(), (what, "a state is not finite")
    assert ep.same_bits_or_nan(a["scal"], b["scal"]).all(), (what, "scalars")
    assert np.array_equal(a["rng"], b["rng"]), (what, "stream position")
    ma, mb = a["masks"].copy(), b["masks"].copy()
    if nch % 64:
        last = np.uint64((1 << (nch % 64)) - 1)
        ma[:, -1] &= last; mb[:, -1] &= last
    assert np.array_equal(ma, mb), (what, "accept masks")
    for k in ("stayed", "draccepted", "drtries", "proposals"):
        assert a["totals"][k] == b["totals"][k], (what, k)
    if "R" in a:
        assert np.isfinite(a["R"]).all() and np.array_equal(a["R"].view(np.uint64), b["R"].view(np.uint64)), (what, "shared factor")


@pytest.mark.parametrize("name,kw", [("am", dict()), ("dr", dict(drscale=3.0)), ("er", dict(method="er"))])
@pytest.mark.parametrize("pooled", [0, 1], ids=["per_chain", "pooled"])
def test_gauss_module_equals_the_builtin_target_at_overflow(gauss_module, monkeypatch, pooled, name, kw):
    from mcmcf90_amd import engine_from_problem, make_config, Engine
    d, nch, nsimu = 20, 130, 130
    pkw = ep.overflow(d, 25.0, 0.3)
    ckw = dict(dict(nsimu=nsimu, adaptint=40, updatesigma=0), **kw)
    monkeypatch.delenv("MCMCX_POOLED_PHASE_MFMA", raising=False)
    # the built-in target's side: the lane-per-chain forms tests/test_gpu_every_chain.py checks against the oracle at this problem's kind, and the
    # matrix-core form of pooled mode
    for k, v in dict(MCMCX_GROUP="0", MCMCX_DR_BIG="0", MCMCX_POOLED_WAVES="1", MCMCX_POOLED_KS="0", MCMCX_POOLED_MFMA_DR_MIN="1").items():
        monkeypatch.setenv(k, v)
    monkeypatch.delenv("MCMCX_LDS_SCRATCH", raising=False)
    e = engine_from_problem(ckw, pkw, nchains=nch, pooled=pooled, record_accept=1, chain_id0=6)
    e.init(); e.run()
    want = {(0, "am"): "step_kernel_ldsv", (0, "dr"): "step_kernel_dr", (0, "er"): "step_kernel_ldsv",
            (1, "am"): "pooled_mfma_kernel<false>", (1, "dr"): "pooled_mfma_kernel<true>", (1, "er"): "pooled_mfma_kernel<false>"}[(pooled, name)]
    assert e.last_kernel() == want, e.last_kernel()
    ref = _state(e, nch, pooled)
    e.close()
    # the regime, from the built-in target's run: both kinds of proposal decided the last iteration of some chain (alpha 0: ss = +inf, there
    # is no other way to -708 here), something was accepted and something rejected
    a12 = ref["scal"][:, 3]
    if name != "er":                                            # (MCMC_run_er computes no alpha: its accepted NaN shows in ss1)
        assert np.isnan(a12).any() and (a12 == 0.0).any(), (np.isnan(a12).sum(), (a12 == 0.0).sum())
    else:
        assert np.isnan(ref["scal"][:, 0]).any()
    assert ref["masks"].any() and ref["totals"]["stayed"] > nch
    data = np.concatenate([pkw["mu"], np.asarray(pkw["lam"]).ravel()])
    for form in (("0", "1") if pooled else ("",)):
        if pooled:
            monkeypatch.setenv("MCMCX_POOLED_PHASE_MFMA", form)
        e = Engine(make_config(d, nch, pooled=pooled, record_accept=1, chain_id0=6, **ckw))
        e.setpar0(pkw["par0"]); e.setcmat0(pkw["cmat0"]); e.setsigma2nobs(pkw["sigma2"], 1)
        e.set_target_module(gauss_module, "gauss_target", data)
        e.init(); e.run()
        assert e.last_kernel() == {"": "", "0": "pooled_phase_kernel", "1": "pooled_phase_mfma_kernel"}[form], e.last_kernel()
        got = _state(e, nch, pooled)
        e.close()
        _same(ref, got, nch, (name, pooled, form))


HOLE_CONFIGS = [("dram", dict(method="dram", drscale=0.0, adaptint=40)), ("drscale", dict(method="dram", drscale=2.0, adaptint=40)), ("ram", dict(method="ram")),
                ("er", dict(method="er", adaptint=40)), ("scam", dict(method="scam", adaptint=25))]


@pytest.mark.parametrize("name,kw", HOLE_CONFIGS, ids=[n for n, _ in HOLE_CONFIGS])
def test_module_equals_host_callbacks_on_a_target_with_a_hole(hole, name, kw):
    from mcmcf90_amd import Engine, make_config, _lib
    hsaco, H = hole
    npar, nch = 5, 130
    nsimu = 60 if kw["method"] == "scam" else 150
    data = np.concatenate([[1.0, 1.4, 0.8, 1.2, 0.9], [np.inf, np.nan]])

    def engine():
        H.set_data(data.ctypes.data_as(C.c_void_p), nch)
        e = Engine(make_config(npar, nch, nsimu=nsimu, updatesigma=0, record_accept=1, chain_id0=11, **kw))
        e.setpar0(np.full(npar, 0.1)); e.setcmat0(0.3 * np.eye(npar))
        e.setsigma2nobs(np.full(1, 0.8), np.full(1, 15))
        return e

    runs = {}
    e = engine(); e.set_target_module(hsaco, "hole_target", data); e.init(); e.run()
    assert e.last_kernel() == "", e.last_kernel()               # (the per-chain phase kernels carry no name in the kernel table)
    runs["module"] = _state(e, nch, 0); e.close()
    keep = (C.cast(H.host_ss, _lib.SSFUN_T), C.cast(H.host_prior, _lib.PRIORFUN_T), C.cast(H.host_bounds, _lib.CHECKBOUNDS_T), C.cast(H.host_ss_batch, _lib.SSFUN_BATCH_T))
    e = engine()
    assert e.L.mcmcx_set_target_host(e.h, keep[0], keep[1], keep[2], None) == 0
    if name == "drscale":                                       # one iteration per call, so that the host side can tell the two stages' passes apart
        H.begin_iteration(); e.init()
        for k in range(2, nsimu + 1):
            H.begin_iteration(); e.run(k)
    else:
        e.init(); e.run()
    runs["host"] = _state(e, nch, 0)
    erstayed = np.array([e.counters(c)["erstayed"] for c in range(nch)])
    e.close()
    # what the host functions counted during that run: every region was proposed into in every tile, the ragged one of two chains included
    hits = np.array((C.c_long * 24).in_dll(H, "g_hits")).reshape(3, 8)
    anyhit = np.array((C.c_long * 3).in_dll(H, "g_any"))
    stage2 = np.array((C.c_long * 3).in_dll(H, "g_stage2"))
    print("%s: proposals with ss = +inf %d, ss = NaN %d, prior = +inf %d (in second stages %s); per tile %s" % (name, anyhit[0], anyhit[1], anyhit[2], stage2.tolist(),
                                                                                                          hits[:, :3].tolist()))
    # the passes the counts rest on: the start point and one per iteration (one per component with SCAM) over all chains; with delayed
    # rejection the second stage's besides, one call per try
    passes = 1 + (nsimu - 1) * (npar if kw["method"] == "scam" else 1)
    assert H.n_bounds_calls() == nch * passes + runs["host"]["totals"]["drtries"], (H.n_bounds_calls(), nch * passes, runs["host"]["totals"]["drtries"])
    assert (hits[:, :3] > 0).all() and not hits[:, 3:].any(), hits
    assert hits.sum() + stage2.sum() == anyhit.sum()
    if name == "drscale":                                       # (per tile: first-stage proposals; the second stage's, a third as long, over the whole run)
        assert (stage2 > 0).all(), stage2
    else:
        assert not stage2.any()
    if name == "er":
        # ... in every full tile: only the prior's +inf can reject on the prior here (it is zero elsewhere); it does unless the chain sits on
        # ss1 = NaN, where the threshold is NaN and nothing is rejected
        assert all(erstayed[t:t + 64].sum() > 0 for t in (0, 64)) and 0 < erstayed.sum() <= anyhit[2], (erstayed.sum(), anyhit)
    e = engine()
    assert e.L.mcmcx_set_target_host_batch(e.h, keep[3], keep[1], keep[2], None, 3) == 0
    e.init(); e.run()
    runs["batch"] = _state(e, nch, 0); e.close()
    for other in ("host", "batch"):
        _same(runs["module"], runs[other], nch, (name, other))
    m = runs["module"]
    assert m["masks"].any() and m["totals"]["stayed"] > 0 or name == "scam"
    if name != "er":
        assert np.isfinite(m["scal"][:, :2]).all()              # no chain sits on a non-finite ss or prior: such a proposal is never accepted
    else:
        assert np.isnan(m["scal"][:, 0]).any()                  # early rejection accepts NaN (MCMC_run_er.F90:72-78): some chain ends on it
