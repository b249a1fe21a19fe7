"""`&mcmcx pooled = 1` from a Fortran program with the user's own target: (1) `devtarget = 'module'` -- device code built with
include/mcmcx_target.h -- and (2) the user's Fortran ssfunction left on the host (the unmodified demo_user program).  Both run
`mcmc_main` to the end and write mcmclaststates.dat / mcmcpooledmean.dat / mcmcpooledcov.dat, and both are compared with the same
configuration through the C ABI.  (1): every chain's last state bit for bit (the files round-trip a double); the pooled mean and
covariance equal the C ABI's only up to the re-derivation -- the test forms them from `mcmcx_pooled_moments` with the shim's
expressions, in numpy instead of Fortran (a contracted multiply-add apart at most).  (2): the Fortran ssfunction uses the Fortran
runtime's exp, so its C twin -- the same model as host callbacks through `mcmcx_set_target_host`, pooled = 1 -- agrees at the libm
rounding level, the tolerance test_gpu_fortran_shim.py uses for this program (rtol 1e-9); the batched form of the same Fortran callbacks
(`hostbatch = 1`) must be the same run bit for bit."""
import os
import subprocess

import numpy as np
import pytest
from golden_util import load

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FDIR = os.path.join(ROOT, "mcmcf90_amd", "fortran")

POLY = '''#include "mcmcx_target.h"
__device__ void p_ss(const double *th, int npar, int ny, const void *data, double *ss)
{ const double *w = (const double *)data; double s = 0.0; for (int k = 0; k < npar; ++k) { double q = th[k] - w[k]; s = s + w[npar + k] * (q * q); } ss[0] = s; }
__device__ double p_prior(const double *th, int npar, const void *data) { return 0.0; }
__device__ int p_bounds(const double *th, int npar, const void *data) { return th[0] > -4.0 ? 1 : 0; }
MCMCX_DEFINE_TARGET(poly_target, p_ss, p_prior, p_bounds)
'''


def _programs():
    for exe in ("demo_main", "demo_user"):
        if not os.path.exists(os.path.join(FDIR, exe)):
            subprocess.check_call(["make", "-s", "-C", FDIR])
    return os.path.join(FDIR, "demo_main"), os.path.join(FDIR, "demo_user")


def _cov_from_moments(pm, n):
    mean = pm[1:1 + n] / pm[0]
    cov = np.zeros((n, n))
    for j in range(n):
        for i in range(j + 1):
            cov[i, j] = cov[j, i] = (pm[1 + n + j * (j + 1) // 2 + i] - pm[0] * mean[i] * mean[j]) / (pm[0] - 1.0)
    return mean, cov


def test_fortran_program_with_a_module_target_in_pooled_mode(tmp_path):
    demo_main, _ = _programs()
    src = tmp_path / "poly.hip"
    src.write_text(POLY)
    hsaco = tmp_path / "poly.hsaco"
    subprocess.check_call(["/opt/rocm/bin/hipcc", "--genco", "--offload-arch=gfx950", "-O2", "-ffp-contract=off",
                           "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(hsaco)])
    data = np.array([0.5, -0.25, 1.0, 2.0, 0.7, 1.3])                    # centres (3), weights (3)
    nch = 130
    d = tmp_path / "mod"; d.mkdir()
    (d / "mcmcinit.nml").write_text("&mcmc\n method = 'dram'\n nsimu = 400\n adaptint = 50\n drscale = 2\n updatesigma = 0\n verbosity = 0\n/\n"
                                    "&mcmcx\n devtarget = 'module'\n modulefile = '%s'\n modulekernel = 'poly_target'\n moduledatafile = 'w.dat'\n"
                                    " nchains = %d\n pooled = 1\n/\n" % (hsaco, nch))
    (d / "w.dat").write_text(" ".join(repr(float(v)) for v in data) + "\n")
    (d / "mcmcpar.dat").write_text("0 0 0\n"); (d / "mcmccov.dat").write_text("0.1 0 0\n0 0.1 0\n0 0 0.1\n")
    p = subprocess.run([demo_main], cwd=d, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
    assert p.returncode == 0, p.stdout.decode(errors="replace")
    last = np.loadtxt(d / "mcmclaststates.dat", ndmin=2)
    pmean = np.loadtxt(d / "mcmcpooledmean.dat", ndmin=1)
    pcov = np.loadtxt(d / "mcmcpooledcov.dat", ndmin=2)
    from mcmcf90_amd import Engine, make_config
    e = Engine(make_config(3, nch, nsimu=400, adaptint=50, drscale=2.0, updatesigma=0, pooled=1))
    e.setpar0(np.zeros(3)); e.setcmat0(0.1 * np.eye(3)); e.setsigma2nobs(1.0, 1)
    e.set_target_module(str(hsaco), "poly_target", data)
    e.init(); e.run()
    assert e.last_kernel() == "pooled_phase_kernel", e.last_kernel()     # npar 3: the lane form
    theta = e.theta()
    mean, cov = _cov_from_moments(e.pooled_moments(), 3)
    shared = e.pooled()[3]
    e.close()
    np.testing.assert_array_equal(last, theta)                           # the same pooled run, chain for chain
    # the shim forms mean and covariance from the same moment vector with the same expressions; a compiler may contract one
    # multiply-add of them: a few ulp of terms of the covariance's own size (the chains are spread around the mean)
    np.testing.assert_allclose(pmean, mean, rtol=1e-13, atol=1e-15)
    np.testing.assert_allclose(pcov, cov, rtol=1e-11)
    assert not np.allclose(shared, np.linalg.cholesky(0.1 * np.eye(3)).T * 2.4 / np.sqrt(3.0))   # the shared factor was adapted


def test_fortran_program_with_its_own_host_callbacks_in_pooled_mode(oracle, tmp_path):
    _, demo_user = _programs()
    z, cfg, prob = load("c1_shipped_nml", oracle)
    nml = ("&mcmc\n method = 'dram'\n nsimu = 600\n verbosity = 0\n doadapt = 1\n adaptint = 100\n drscale = 2\n updatesigma = 1\n N0 = 1\n S02 = 0\n"
           " chainfile = 'chain.dat'\n ssfile = 'sschain.dat'\n s2file = 's2chain.dat'\n/\n")
    outs = []
    for extra in ("&mcmcx\n nchains = 70\n pooled = 1\n/\n", "&mcmcx\n nchains = 70\n pooled = 1\n hostbatch = 1\n hostthreads = 3\n/\n",
                  "&mcmcx\n nchains = 70\n/\n"):
        d = tmp_path / ("h%d" % len(outs)); d.mkdir()
        (d / "mcmcinit.nml").write_text(nml + extra)
        with open(d / "data.dat", "w") as f:
            for x, y in zip(z["prob_xdata"], z["prob_ydata"]):
                f.write("  %g   %.2f\n" % (x, y))
        (d / "mcmcpar.dat").write_text("10 0.1 \n"); (d / "mcmccov.dat").write_text("0.2 0 \n0 0.001 \n"); (d / "mcmcsigma2.dat").write_text("0.5\n11\n")
        p = subprocess.run([demo_user], cwd=d, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
        assert p.returncode == 0, p.stdout.decode(errors="replace")
        outs.append((np.loadtxt(d / "mcmclaststates.dat", ndmin=2), np.loadtxt(d / "mcmcpooledmean.dat", ndmin=1),
                     np.loadtxt(d / "mcmcpooledcov.dat", ndmin=2)))
    last, pmean, pcov = outs[0]
    assert last.shape == (70, 2)
    np.testing.assert_array_equal(last, outs[1][0])                      # the batched callbacks: the same pooled run
    np.testing.assert_array_equal(pcov, outs[1][2])
    np.testing.assert_allclose(pmean, last.mean(axis=0), rtol=1e-12)     # (the tolerances of test_gpu_fortran_shim.py for these files)
    np.testing.assert_allclose(pcov, np.cov(last.T), rtol=1e-9)
    assert not np.array_equal(last, outs[2][0])                          # ... and not the per-chain run
    # ---- the C twin: the same model (demo_user.F90: ss = sum((y - theta1 exp(-theta2 x))**2), all parameters positive) as host callbacks
    # through the C ABI with pooled = 1, data as data.dat holds them.  numpy's exp against the Fortran runtime's: libm rounding level
    x = np.array([float("%g" % v) for v in z["prob_xdata"]]); y = np.array([float("%.2f" % v) for v in z["prob_ydata"]])
    from mcmcf90_amd import Engine, make_config
    e = Engine(make_config(2, 70, method="dram", nsimu=600, doadapt=1, adaptint=100, drscale=2.0, updatesigma=1, N0=1.0, S02=0.0, pooled=1))
    e.setpar0(np.array([10.0, 0.1])); e.setcmat0(np.array([[0.2, 0.0], [0.0, 0.001]])); e.setsigma2nobs(0.5, 11)
    e.set_target_host(lambda th: float(np.sum((y - th[0] * np.exp(-th[1] * x)) ** 2)), checkbounds=lambda th: bool(np.all(th > 0.0)))
    e.init(); e.run()
    assert e.last_kernel() == "pooled_phase_kernel", e.last_kernel()
    theta = e.theta()
    mean, cov = _cov_from_moments(e.pooled_moments(), 2)
    mean = mean + np.array([10.0, 0.1])                                  # (the moments are about par0)
    shared = e.pooled()[3]
    e.close()
    np.testing.assert_allclose(last, theta, rtol=1e-9)
    np.testing.assert_allclose(pmean, mean, rtol=1e-9)
    sd = np.sqrt(np.diag(cov))
    np.testing.assert_allclose(pcov / np.outer(sd, sd), cov / np.outer(sd, sd), rtol=1e-9, atol=1e-9)   # (an entry's scale: |c_ij| <= sd_i sd_j)
    assert not np.allclose(shared, np.linalg.cholesky(np.array([[0.2, 0.0], [0.0, 0.001]])).T * 2.4 / np.sqrt(2.0))   # adapted
