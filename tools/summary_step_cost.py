"""What a step summary pass costs (mcmcx_samples_stats_step_dev: two nine-step searches in LDS and a table read per value) beside the
summary itself (mcmcx_samples_stats_dev) in the SAME session: tools/summary_cost.py's shapes and ring (c3: 262 144 chains, npar 20; c4, the
headline: 1 048 576 chains, npar 50), the whole ring and a window of 16 samples, maxlag 0, 8 and 32, nbins 30, 126 and 510.  Per cell the
four calls alternate -- identity, 30, 126, 510 bins, identity, .. -- --reps times after one warm round; each is the `_dev` form plus one
synchronisation (the step form also stages its keys and table).  Printed: the median per call in ms and its ratio to the identity's
median, with the identity's own min .. max as the spread to read the ratios against.  The edges are the order statistics of the
16-sample window that cut it into nbins + 2 cells, the table their normal scores (the cost depends on neither).  With --rank also
samples_summary(rank=True) beside rank=False, end to end.  Evidence for DESIGN.md section 5g-3; run on the GPU box from the repository
root:

    python tools/summary_step_cost.py [--reps 5] [--workloads c3 c4] [--rank] > summary_step_cost.txt

The counters, in a run of their own (no tracing beside them), then per dispatch of the summary's kernels:

    rocprofv3 --pmc SQ_INSTS_VALU SQ_INSTS_LDS SQ_ACTIVE_INST_LDS SQ_LDS_BANK_CONFLICT SQ_WAVE_CYCLES SQ_BUSY_CYCLES --output-format csv -d DIR -o pmc \\
        -- python tools/summary_step_cost.py --reps 1 --workloads c3 --mem-fraction 0.1
    python tools/summary_step_cost.py --pmc-stats DIR/.../pmc_counter_collection.csv
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

NBINS = (30, 126, 510)


def measure(wl, reps, frac, rank):
    import torch
    from mcmcf90_amd import engine_from_problem
    from mcmcf90_amd.engine import sample_nfields, samples_rank_scores
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
    print("%3s %6s %6s %10s | %9s %15s | %s" % ("wl", "ns", "maxlag", "window GB", "identity", "min .. max",
                                                "   ".join("%3d: ms  ratio" % b for b in NBINS)))
    steps = []
    for b in NBINS:
        edges = e.samples_rank_edges(b + 2, 0, 16)
        steps.append((edges, samples_rank_scores(e.samples_hist(edges, 0, 16))))
    zero = np.zeros(nf)
    for ns in (cap, 16):
        calls = [lambda m: e.samples_stats_torch(0, ns, m, zero)] + [(lambda m, ed=ed, tb=tb: e.samples_stats_step_torch(ed, tb, 0, ns, m, zero))
                                                                      for ed, tb in steps]
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
                  "   ".join("%8.3f %6.3f" % (m, m / med[0]) for m in med[1:])), flush=True)
    if rank:
        for ns in (cap, 16):
            ts = {False: [], True: []}
            for r in range(reps + 1):
                for flag in (False, True):
                    e.sync()
                    t0 = time.perf_counter()
                    e.samples_summary(0, ns, 8, rank=flag)
                    if r:
                        ts[flag].append(time.perf_counter() - t0)
            print("# %s: samples_summary over %d samples, maxlag 8, 128 cells: rank=False %.3f ms, rank=True %.3f ms (medians of %d, alternating)"
                  % (wl, ns, np.median(ts[False]) * 1e3, np.median(ts[True]) * 1e3, reps), flush=True)
    e.close()


def pmc_stats(path):
    """diag_tile_kernel / diag_step_tile_kernel dispatches of a rocprofv3 --pmc counter_collection.csv: every counter summed per dispatch."""
    import csv
    acc, names = {}, {}
    for r in csv.DictReader(open(path)):
        k = r.get("Kernel_Name", "")
        if "diag_tile_kernel" in k or "diag_step_tile_kernel" in k:
            d = int(r["Dispatch_Id"])
            acc.setdefault(d, {})
            acc[d][r["Counter_Name"]] = acc[d].get(r["Counter_Name"], 0.0) + float(r["Counter_Value"])
            names[d] = k
    for d in sorted(acc):
        print("dispatch %7d %-38s %s" % (d, names[d][:38], "  ".join("%s %.4g" % (c, v) for c, v in sorted(acc[d].items()))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--workloads", nargs="*", default=["c3", "c4"])
    ap.add_argument("--mem-fraction", type=float, default=0.5, help="share of the device memory free beside the state that the ring takes")
    ap.add_argument("--rank", action="store_true", help="also time samples_summary(rank=True) beside rank=False")
    ap.add_argument("--pmc-stats", help="a rocprofv3 --pmc counter_collection.csv of a run of this tool: the counters per dispatch")
    a = ap.parse_args()
    if a.pmc_stats:
        pmc_stats(a.pmc_stats)
        return
    # torch first, or it finds no device (tools/summary_cost.py says why)
    import torch
    torch.zeros(1, device="cuda")
    from samples_cost import device_line
    print(device_line())
    for wl in a.workloads:
        measure(wl, a.reps, a.mem_fraction, a.rank)


if __name__ == "__main__":
    main()
