"""What the sample store's batch-means covariance costs (mcmcx_samples_cov_bm_dev) beside the covariance (mcmcx_samples_cov_dev, whose
kernels are instruction for instruction the parent commit's): on BASELINE configuration c3's shape (262 144 chains, npar 20: form A, two
blocks) and the headline's (c4, 1 048 576 chains, npar 50: form A, four blocks), with the largest ring that fits a share of the free
device memory beside the state, over the whole ring and over a window of 16 samples.  The calls ALTERNATE within one session -- cov, bm at
batch 1, 8 and ns / 2, and round again --, wall time of a synchronised call, median of --reps rounds after one warm round; `spread` is the
covariance's own (max - min) / median over the rounds, `bm/cov` the ratio of the medians.  The batch-means kernel reads the same bytes once and
issues 1 / batch of the MFMAs, so the expectation is a ratio of one within the spread.  Evidence for DESIGN.md section 5i-2; run on the GPU
box from the repository root:

    python tools/bm_cost.py [--reps 5] [--workloads c3 c4] > bm_cost.txt
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CHAINS = {"c3": 262144, "c4": 1048576}                          # bench.py's DEFAULT_CHAINS
WARM = 11


def measure(wl, reps, frac):
    import torch
    from mcmcf90_amd import engine_from_problem
    from mcmcf90_amd.engine import sample_nfields
    from mcmcf90_amd.workloads import problem
    n = CHAINS[wl]
    ckw, pkw, _ = problem(wl, 100)
    nf = sample_nfields(pkw["npar"])
    slot = 8 * nf * (-(-n // 64) * 64)
    e = engine_from_problem(ckw, pkw, nchains=n)                 # the state's size is not known before init
    e.init(); e.sync()
    free, total = torch.cuda.mem_get_info()
    e.close()
    cap = max(16, int(frac * free / slot))
    ckw, pkw, _ = problem(wl, WARM + cap)
    e = engine_from_problem(ckw, pkw, nchains=n)
    e.set_samples(first=WARM + 1, thin=1, capacity=cap)
    e.init()
    e.run(); e.sync()
    assert e.samples_kept()[0] == cap
    print("# %s: %d chains, nfields %d, a slot %.1f MB, ring of %d slots = %.2f GB, kernel %s" % (wl, n, nf, slot / 1e6, cap, cap * slot / 1e9,
                                                                                              e.last_kernel()), flush=True)
    print("%3s %6s %-12s %10s %12s %15s %8s %8s" % ("wl", "ns", "call", "window GB", "ms (median)", "min .. max", "TB/s", "bm/cov"))
    for ns in (cap, 16):
        gb = ns * slot / 1e9
        calls = [("cov", lambda: e.samples_cov_stats_torch(0, ns))]
        for b in dict.fromkeys((1, 8, ns // 2)):                 # (ns = 16: ns / 2 is 8)
            calls.append(("bm batch %d" % b, lambda b=b: e.samples_cov_bm_stats_torch(b, 0, ns)))
        ts = {name: [] for name, _ in calls}
        for r in range(reps + 1):                                # round 0 warms: the scratch, the code objects
            for name, fn in calls:
                e.sync()
                t0 = time.perf_counter()
                fn()
                if r:
                    ts[name].append(time.perf_counter() - t0)
        cov = float(np.median(ts["cov"]))
        for name, _ in calls:
            t = ts[name]
            med = float(np.median(t))
            tail = "spread %.3f" % ((max(t) - min(t)) / med) if name == "cov" else "%8.3f" % (med / cov)
            print("%3s %6d %-12s %10.3f %12.3f %6.3f .. %-6.3f %8.2f %s" % (wl, ns, name, gb, med * 1e3, min(t) * 1e3, max(t) * 1e3,
                                                                          gb / med / 1e3, tail), flush=True)
    e.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--workloads", nargs="*", default=["c3", "c4"])
    ap.add_argument("--mem-fraction", type=float, default=0.5, help="share of the device memory free beside the state that the ring takes")
    a = ap.parse_args()
    # torch bundles its own HIP runtime under the same soname as the library's: whichever is loaded first serves the whole process
    # (tests/conftest.py, bench.py).  torch first, or it finds no device.
    import torch
    torch.zeros(1, device="cuda")
    from samples_cost import device_line
    print(device_line())
    for wl in a.workloads:
        measure(wl, a.reps, a.mem_fraction)


if __name__ == "__main__":
    main()
