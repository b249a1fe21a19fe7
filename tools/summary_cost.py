"""What the sample store's convergence summary costs (mcmcx_samples_stats_dev): on BASELINE configuration c3's shape (262 144 chains, npar 20)
and the headline's (c4, method = 'ram', 1 048 576 chains, npar 50), with the largest ring that fits a share of the free device memory beside
the state, the `_dev` form at maxlag 0, 8 and 32 over the whole ring and over a window of 16 samples: wall time of a synchronised call
(median of --reps after one warm call), the window's bytes per second (the window counted ONCE; the kernel reads it twice), against the
keep kernel's 5.3 - 5.5 TB/s.  Beside it the route a user had before: samples_torch(layout=1) of the 16-sample window plus the same table in
torch, as time and peak device memory.  Evidence for DESIGN.md section 5g; run on the GPU box from the repository root:

    python tools/summary_cost.py [--reps 3] [--workloads c3 c4] > summary_cost.txt

The kernels' OWN durations come from a kernel trace of one such run, which --trace-stats turns into bytes/s per instantiation:

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o kt -- python tools/summary_cost.py --reps 1 --workloads c4 --no-torch
    python tools/summary_cost.py --trace-stats DIR/.../kt_kernel_stats.csv

and whether a wave's second pass over its rows is served by L2 from a counter run of its own:

    rocprofv3 --pmc FETCH_SIZE --output-format csv -d DIR -o pmc -- python tools/summary_cost.py --reps 1 --workloads c4 --no-torch
    python tools/summary_cost.py --pmc-stats DIR/.../pmc_counter_collection.csv
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CHAINS = {"c3": 262144, "c4": 1048576}                           # bench.py's DEFAULT_CHAINS
WARM = 11
MAXLAGS = (0, 8, 32)


def torch_table(X, maxlag):
    """The same table from a [ns][nfields][nc] tensor with torch's own reductions (no fixed order): mean, sd, rhat, ess, mcse."""
    import math
    import torch
    ns, nf, nc = X.shape
    nh = ns // 2
    K = min(maxlag, nh - 1)
    H = torch.stack([X[:nh], X[ns - nh:]])                       # [2][n_h][nf][nc]
    m = H.mean(dim=1)                                            # [2][nf][nc]
    Z = H - m[:, None]
    M = 2 * nc
    G = torch.stack([(Z[:, :nh - t] * Z[:, t:]).sum(dim=(0, 1, 3)) for t in range(K + 1)])           # [K + 1][nf]
    W = G[0] / (M * (nh - 1))
    Bn = m.var(dim=(0, 2), unbiased=True)
    varp = W * (nh - 1) / nh + Bn
    rho = 1.0 - (W - G / (M * nh)) / varp
    rho[0] = 1.0
    P = (rho[0:2 * ((K + 1) // 2):2] + rho[1:2 * ((K + 1) // 2):2]) if K > 0 else rho[:0]
    keep = torch.cumprod((P > 0).to(P.dtype), dim=0)
    P = torch.cummin(torch.where(keep > 0, P, torch.full_like(P, float("inf"))), dim=0).values if len(P) else P
    tau = -1.0 + 2.0 * (torch.where(keep > 0, P, torch.zeros_like(P))).sum(dim=0) if len(P) else torch.full((nf,), float("nan"), device=X.device)
    tau = torch.clamp(tau, min=1.0 / math.log10(M * nh))
    ess = M * nh / tau
    sd = varp.sqrt()
    return torch.stack([m.mean(dim=(0, 2)), sd, (varp / W).sqrt(), ess, sd / ess.sqrt()], dim=1)


def measure(wl, reps, frac, use_torch):
    import torch
    from mcmcf90_amd import engine_from_problem
    from mcmcf90_amd.engine import sample_nfields, samples_diag
    from mcmcf90_amd.workloads import problem
    n = CHAINS[wl]
    ckw, pkw, _ = problem(wl, 100)
    nf = sample_nfields(pkw["npar"])
    slot = 8 * nf * (-(-n // 64) * 64)
    # the state's size is not known before init: a first engine without a ring tells what is free beside it
    e = engine_from_problem(ckw, pkw, nchains=n)
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
    print("# %s: %d chains, nfields %d, a slot %.1f MB, ring of %d slots = %.2f GB (%.0f %% of the %.1f GB free beside the state), kernel %s"
          % (wl, n, nf, slot / 1e6, cap, cap * slot / 1e9, 100 * frac, free / 1e9, e.last_kernel()), flush=True)
    print("%3s %6s %6s %10s %12s %12s %10s" % ("wl", "ns", "maxlag", "window GB", "ms (median)", "min .. max", "TB/s"))
    rows = {}
    for ns in (cap, 16):
        for maxlag in MAXLAGS:
            e.samples_stats_torch(0, ns, maxlag)                 # warm: the scratch, the code object
            ts = []
            for _ in range(reps):
                e.sync()
                t0 = time.perf_counter()
                t = e.samples_stats_torch(0, ns, maxlag)         # the _dev form + one synchronisation
                ts.append(time.perf_counter() - t0)
            med = float(np.median(ts))
            rows[(ns, maxlag)] = (med, t)
            print("%3s %6d %6d %10.3f %12.3f %5.3f .. %-5.3f %10.2f" % (wl, ns, maxlag, ns * slot / 1e9, med * 1e3, min(ts) * 1e3, max(ts) * 1e3,
                                                                    ns * slot / med / 1e12), flush=True)
    if use_torch:
        ns, maxlag = 16, 8
        torch.cuda.synchronize(); torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        ts = []
        for _ in range(reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            X = e.samples_torch(0, ns, layout=1)[1]
            tab = torch_table(X, maxlag)
            torch.cuda.synchronize()
            ts.append(time.perf_counter() - t0)
            del X
        peak = torch.cuda.max_memory_allocated() - base
        ours = samples_diag(rows[(ns, maxlag)][1].cpu().numpy(), nf, maxlag)
        with np.errstate(invalid="ignore", divide="ignore"):                  # a constant field is 0 / 0 in both tables
            err = np.nanmax(np.abs(tab.cpu().numpy() / ours[:, :5] - 1.0))
        print("# %s: samples_torch(layout=1) of %d samples + the table in torch (maxlag %d): %.1f ms (min %.1f, max %.1f), peak device memory "
              "%.2f GB beside the ring; the summary: %.3f ms, scratch %.1f MB; largest relative difference of the two tables %.1e"
              % (wl, ns, maxlag, np.median(ts) * 1e3, min(ts) * 1e3, max(ts) * 1e3, peak / 1e9, rows[(ns, maxlag)][0] * 1e3,
                 8 * (-(-n // 64)) * nf * (32 + 3) / 1e6, err), flush=True)
    e.close()


def trace_stats(path):
    """diag_tile_kernel / moments_tree_kernel lines of a rocprofv3 kernel_stats.csv."""
    import csv
    for r in csv.DictReader(open(path)):
        if "diag_" in r["Name"] or "moments_tree" in r["Name"] or "samples_" in r["Name"]:
            print("%-40s calls %5s average %10.1f us min %10.1f max %10.1f" % (r["Name"][:40], r["Calls"], float(r["AverageNs"]) / 1e3,
                                                                             float(r["MinNs"]) / 1e3, float(r["MaxNs"]) / 1e3))


def pmc_stats(path):
    """diag_tile_kernel dispatches of a `rocprofv3 --pmc FETCH_SIZE` counter_collection.csv (a run of its own, no tracing): bytes that came
    in through L2 per dispatch, 2 x FETCH_SIZE KiB on gfx950 (tools/profile_summary.py).  Against the window's bytes: 1 x = the second pass
    of a wave found its rows in L2, 2 x = it did not."""
    import csv
    acc, names = {}, {}
    for r in csv.DictReader(open(path)):
        if "diag_tile_kernel" in r.get("Kernel_Name", "") and r["Counter_Name"] == "FETCH_SIZE":
            d = int(r["Dispatch_Id"])
            acc[d] = acc.get(d, 0.0) + float(r["Counter_Value"])
            names[d] = r["Kernel_Name"]
    for d in sorted(acc):
        print("dispatch %6d %-40s read through L2 %10.3f GB" % (d, names[d][:40], 2.0 * acc[d] * 1024.0 / 1e9))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--workloads", nargs="*", default=["c3", "c4"])
    ap.add_argument("--mem-fraction", type=float, default=0.5, help="share of the device memory free beside the state that the ring takes")
    ap.add_argument("--no-torch", action="store_true")
    ap.add_argument("--trace-stats", help="a rocprofv3 kernel_stats.csv of a run of this tool: print the summary kernels' durations and stop")
    ap.add_argument("--pmc-stats", help="a rocprofv3 --pmc FETCH_SIZE counter_collection.csv of a run of this tool: bytes read per dispatch")
    a = ap.parse_args()
    if a.trace_stats:
        trace_stats(a.trace_stats)
        return
    if a.pmc_stats:
        pmc_stats(a.pmc_stats)
        return
    # torch bundles its own HIP runtime under the same soname as the library's: whichever is loaded first serves the whole process
    # (tests/conftest.py, bench.py).  torch first, or it finds no device.
    import torch
    torch.zeros(1, device="cuda")
    from samples_cost import device_line
    print(device_line())
    for wl in a.workloads:
        measure(wl, a.reps, a.mem_fraction, not a.no_torch)


if __name__ == "__main__":
    main()
