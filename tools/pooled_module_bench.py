"""A user target module (the test module of tests/test_gpu_user_module.py) at npar 50: pooled adaptation (pooled = 1, one shared factor,
the plan's own phase form) against per-chain adaptation (pooled = 0: a packed factor per chain), alternating on one device.  The
per-chain path is the parent's code: this tool runs it from the same build.  Run on the GPU box from the repository root:

    python tools/pooled_module_bench.py [--reps 3] > pooled_module_bench.txt
"""
import argparse
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from pooled_phase_sweep import build_module, device_line, run_once  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--npar", type=int, default=50)
    ap.add_argument("--chains", type=int, nargs="*", default=[65536, 1048576])
    a = ap.parse_args()
    with tempfile.TemporaryDirectory() as tmp:
        hsaco = build_module(tmp)
        print(device_line())
        print("# proposals/s over iterations 12..111 (module evaluation included), median of %d alternating runs; ticks: adaptint = 25 (the" % a.reps)
        print("# adaptation's four ticks inside the timed iterations); none: adaptint = 1000 (no tick in the run: the sampling iterations alone)")
        print("%5s %8s %6s %6s %14s %14s %8s  %s" % ("npar", "chains", "method", "ticks", "pooled", "per chain", "ratio", "pooled form"))
        for n in a.chains:
            for method in ("dram", "ram"):
                for ticks in (True, False):
                    kw = dict(method=method, adaptint=25 if ticks else 1000)
                    t = {0: [], 1: []}
                    form = ""
                    for _ in range(a.reps):
                        for pooled in (1, 0):
                            s, k = run_once(hsaco, a.npar, n, 111, None, pooled=pooled, **kw)
                            t[pooled].append(s)
                            if pooled:
                                form = k
                    rp, rc = n / np.median(t[1]), n / np.median(t[0])
                    print("%5d %8d %6s %6s %14.4g %14.4g %8.2f  %s" % (a.npar, n, method, "yes" if ticks else "none", rp, rc, rp / rc, form),
                          flush=True)


if __name__ == "__main__":
    main()
