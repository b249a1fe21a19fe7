"""What a transformed summary pass costs (mcmcx_samples_stats_of_dev, kinds 1 .. 3) beside the summary itself (mcmcx_samples_stats_dev) in the
SAME session: tools/summary_cost.py's shapes and ring (c3: 262 144 chains, npar 20; c4, the headline: 1 048 576 chains, npar 50), the whole
ring and a window of 16 samples, maxlag 0, 8 and 32.  Per cell the four calls alternate -- identity, LE, FOLD, SQUARE, identity, .. --
--reps times after one warm round; each is the `_dev` form plus one synchronisation.  Printed: the median per kind in ms and its ratio to
the identity's median, with the identity's own min .. max as the spread to read the ratios against.  a is the window's mean (the cost does
not depend on it).  With --tail also samples_summary(tail=True) beside tail=False, end to end.  Evidence for DESIGN.md section 5g; run on
the GPU box from the repository root:

    python tools/summary_xf_cost.py [--reps 5] [--workloads c3 c4] [--tail] > summary_xf_cost.txt
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

NAMES = ("identity", "le", "fold", "square")


def measure(wl, reps, frac, tail):
    import torch
    from mcmcf90_amd import engine_from_problem
    from mcmcf90_amd.engine import sample_nfields, samples_diag
    from mcmcf90_amd.workloads import problem
    from summary_cost import CHAINS, MAXLAGS, WARM
    n = CHAINS[wl]
    ckw, pkw, _ = problem(wl, 100)
    nf = sample_nfields(pkw["npar"])
    slot = 8 * nf * (-(-n // 64) * 64)
    e = engine_from_problem(ckw, pkw, nchains=n)                 # what is free beside the state (tools/summary_cost.py)
    e.init(); e.sync()
    free, _ = torch.cuda.mem_get_info()
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
    print("%3s %6s %6s %10s | %9s %15s | %s" % ("wl", "ns", "maxlag", "window GB", "identity", "min .. max", "   ".join("%6s ms  ratio" % k for k in NAMES[1:])))
    for ns in (cap, 16):
        a = samples_diag(e.samples_stats(0, ns, 0), nf, 0)[:, 0].copy()
        calls = [lambda m: e.samples_stats_torch(0, ns, m)] + [(lambda m, k=k: e.samples_stats_of_torch(k, a, 0, ns, m)) for k in (1, 2, 3)]
        for maxlag in MAXLAGS:
            ts = [[] for _ in calls]
            for r in range(reps + 1):                            # round 0 warms: the scratch, the code objects
                for k, call in enumerate(calls):
                    e.sync()
                    t0 = time.perf_counter()
                    call(maxlag)
                    if r:
                        ts[k].append(time.perf_counter() - t0)
            med = [float(np.median(t)) * 1e3 for t in ts]
            print("%3s %6d %6d %10.3f | %9.3f %6.3f .. %-6.3f | %s" % (wl, ns, maxlag, ns * slot / 1e9, med[0], min(ts[0]) * 1e3, max(ts[0]) * 1e3,
                  "   ".join("%9.3f %6.3f" % (m, m / med[0]) for m in med[1:])), flush=True)
    if tail:
        for ns in (cap, 16):
            for maxlag in (8,):
                ts = {False: [], True: []}
                for r in range(reps + 1):
                    for flag in (False, True):
                        e.sync()
                        t0 = time.perf_counter()
                        e.samples_summary(0, ns, maxlag, tail=flag)
                        if r:
                            ts[flag].append(time.perf_counter() - t0)
                print("# %s: samples_summary over %d samples, maxlag %d: tail=False %.3f ms, tail=True %.3f ms (medians of %d, alternating)"
                      % (wl, ns, maxlag, np.median(ts[False]) * 1e3, np.median(ts[True]) * 1e3, reps), flush=True)
    e.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--workloads", nargs="*", default=["c3", "c4"])
    ap.add_argument("--mem-fraction", type=float, default=0.5, help="share of the device memory free beside the state that the ring takes")
    ap.add_argument("--tail", action="store_true", help="also time samples_summary(tail=True) beside tail=False")
    a = ap.parse_args()
    # torch first, or it finds no device (tools/summary_cost.py says why)
    import torch
    torch.zeros(1, device="cuda")
    from samples_cost import device_line
    print(device_line())
    for wl in a.workloads:
        measure(wl, a.reps, a.mem_fraction, a.tail)


if __name__ == "__main__":
    main()
