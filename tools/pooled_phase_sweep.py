"""Pooled mode with a user target module: the lane form (pooled_phase_kernel) against the matrix-core form (pooled_phase_mfma_kernel) of the
proposal phases, forced through MCMCX_POOLED_PHASE_MFMA = 0 / 1, alternating on one device.  The module is the test module of
tests/test_gpu_user_module.py.  Evidence for plan_kernels' rule pooled_phase_mfma (mcx_host_launch.hpp); run on the GPU box from the
repository root:

    python tools/pooled_phase_sweep.py [--reps 3] > phase_form_sweep.txt
"""
import argparse
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def build_module(tmp):
    from test_gpu_user_module import USER_SRC
    src = os.path.join(tmp, "user_target.hip")
    open(src, "w").write(USER_SRC)
    out = os.path.join(tmp, "user_target.hsaco")
    subprocess.check_call(["/opt/rocm/bin/hipcc", "--genco", "--offload-arch=gfx950", "-O2", "-ffp-contract=off", "-I" + os.path.join(ROOT, "include"),
                           src, "-o", out])
    return out


def device_line():
    """The card a table was measured on (mcmcx_device_info)."""
    import ctypes as C
    from mcmcf90_amd import _lib
    buf = C.create_string_buffer(256)
    _lib.load().mcmcx_device_info(0, buf, 256)
    return "# device: " + buf.value.decode()


def run_once(hsaco, d, n, nsimu, form, pooled=1, **kw):
    """Seconds per iteration of iterations 2..nsimu (the ticks included), and the kernel form that ran."""
    from mcmcf90_amd import Engine, make_config
    if form is None:
        os.environ.pop("MCMCX_POOLED_PHASE_MFMA", None)
    else:
        os.environ["MCMCX_POOLED_PHASE_MFMA"] = str(form)
    cfg = dict(method="dram", adaptint=50, updatesigma=1)
    cfg.update(kw)
    e = Engine(make_config(d, n, nsimu=nsimu, pooled=pooled, **cfg))
    e.setpar0(np.full(d, 0.1)); e.setcmat0(0.05 * np.eye(d)); e.setsigma2nobs(0.8, 15)
    e.set_target_module(hsaco, "user_target", np.concatenate([np.linspace(0.5, 2.0, d), [0.3]]))
    e.init()
    e.run(11); e.sync()                                    # warm-up: code objects loaded, the first proposal made
    t0 = time.perf_counter()
    e.run(); e.sync()
    dt = time.perf_counter() - t0
    k = e.last_kernel()
    e.close()
    return dt / (nsimu - 11), k


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--npar", type=int, nargs="*", default=[10, 20, 50, 64])
    ap.add_argument("--chains", type=int, nargs="*", default=[1024, 65536, 1048576])
    a = ap.parse_args()
    with tempfile.TemporaryDirectory() as tmp:
        hsaco = build_module(tmp)
        print(device_line())
        print("# us per iteration (module evaluation and ticks included), median of %d alternating runs; dr: drscale = 2" % a.reps)
        print("%5s %8s %3s %12s %12s %8s" % ("npar", "chains", "dr", "lane", "mfma", "lane/mfma"))
        for d in a.npar:
            for n in a.chains:
                for dr in (0.0, 2.0):
                    nsimu = 211 if n <= 65536 else 111
                    t = {0: [], 1: []}
                    for _ in range(a.reps):
                        for form in (0, 1):
                            s, k = run_once(hsaco, d, n, nsimu, form, drscale=dr)
                            assert k == ("pooled_phase_mfma_kernel" if form else "pooled_phase_kernel"), k
                            t[form].append(s)
                    lane, mfma = np.median(t[0]) * 1e6, np.median(t[1]) * 1e6
                    print("%5d %8d %3d %12.1f %12.1f %8.2f" % (d, n, int(dr > 0), lane, mfma, lane / mfma), flush=True)


if __name__ == "__main__":
    main()
