"""What the sample store's order statistics and counts cost (mcmcx_samples_order_stats_dev / mcmcx_samples_counts_dev): on BASELINE
configuration c3's shape (262 144 chains, npar 20) and the headline's (c4, method = 'ram', 1 048 576 chains, npar 50), with the largest ring
that fits a share of the free device memory beside the state, over the whole ring and over a window of 16 samples: wall time of a
synchronised call (median of --reps after one warm call) of the select at nr = 2 (one interval), 6 and 32 and of the counts pass at nq = 2.
The yardstick, in the same session: mcmcx_samples_stats_dev at maxlag = 0 over the same window, which reads the window twice -- so HALF its
time is what one pass over the window costs a kernel of this shape, and a select is eight passes: `pass/yard` is (select time / 8) against
(yardstick time / 2).  Beside it the route a user had before: samples_torch(layout=1) of the 16-sample window plus, one field at a time, a
torch sort and the same interpolation (torch.quantile refuses inputs above 16 M elements), as time and peak device memory.  Evidence for DESIGN.md section 5h; run on the GPU box from the repository root:

    python tools/quantile_cost.py [--reps 3] [--workloads c3 c4] > quantile_cost.txt

The kernels' OWN durations come from a kernel trace of one such run:

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o kt -- python tools/quantile_cost.py --reps 1 --workloads c4 --no-torch
    python tools/quantile_cost.py --trace-stats DIR/.../kt_kernel_stats.csv

and what bounds a pass from a counter run of its own (no tracing beside it):

    rocprofv3 --pmc SQ_INSTS_VALU SQ_INSTS_SALU SQ_INSTS_LDS SQ_ACTIVE_INST_LDS SQ_WAVE_CYCLES SQ_BUSY_CYCLES --output-format csv -d DIR -o pmc \
        -- python tools/quantile_cost.py --reps 1 --workloads c3 --no-torch --mem-fraction 0.1
    python tools/quantile_cost.py --pmc-stats DIR/.../pmc_counter_collection.csv
"""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CHAINS = {"c3": 262144, "c4": 1048576}                           # bench.py's DEFAULT_CHAINS
WARM = 11
NRS = (2, 6, 32)
PROBS = (0.025, 0.5, 0.975)


def _timed(fn, reps, sync):
    fn()                                                         # warm: the scratch, the code object
    ts = []
    for _ in range(reps):
        sync()
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts)), min(ts), max(ts)


def measure(wl, reps, frac, use_torch):
    import torch
    from mcmcf90_amd import engine_from_problem
    from mcmcf90_amd.engine import sample_nfields, samples_quantile_ranks
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
    print("# %s: %d chains, nfields %d, a slot %.1f MB, ring of %d slots = %.2f GB (%.0f %% of the %.1f GB free beside the state), kernel %s"
          % (wl, n, nf, slot / 1e6, cap, cap * slot / 1e9, 100 * frac, free / 1e9, e.last_kernel()), flush=True)
    print("%3s %6s %-12s %10s %12s %15s %10s %10s" % ("wl", "ns", "call", "window GB", "ms (median)", "min .. max", "TB/s pass", "pass/yard"))
    cnt = torch.empty((nf, 2, 2), dtype=torch.int64, device="cuda:%d" % e.cfg.device)
    for ns in (cap, 16):
        gb = ns * slot / 1e9
        yard, lo, hi = _timed(lambda: e.samples_stats_torch(0, ns, 0), reps, e.sync)
        print("%3s %6d %-12s %10.3f %12.3f %6.3f .. %-6.3f %10.2f %10s" % (wl, ns, "stats lag 0", gb, yard * 1e3, lo * 1e3, hi * 1e3,
                                                                          2 * gb / yard / 1e3, "(2 passes)"), flush=True)
        for nr in NRS:
            ranks = (np.arange(nr, dtype=np.int64) * 2 + 1) * (ns * n // (2 * nr))
            if nr == 2:
                ranks = samples_quantile_ranks(ns * n, [0.025, 0.975])[0][:, 0]
            med, lo, hi = _timed(lambda: e.samples_order_stats_torch(ranks, 0, ns), reps, e.sync)
            print("%3s %6d %-12s %10.3f %12.3f %6.3f .. %-6.3f %10.2f %10.2f" % (wl, ns, "select nr %d" % nr, gb, med * 1e3, lo * 1e3, hi * 1e3,
                                                                               8 * gb / med / 1e3, (med / 8) / (yard / 2)), flush=True)
        x = np.ascontiguousarray(e.samples_order_stats(samples_quantile_ranks(ns * n, [0.025, 0.975])[0][:, 0], 0, ns))

        def counts():
            e._chk(e.L.mcmcx_samples_counts_dev(e.h, 0, ns, 2, x.ctypes.data_as(C.POINTER(C.c_double)), C.c_void_p(cnt.data_ptr())))
            e.sync()
        med, lo, hi = _timed(counts, reps, e.sync)
        print("%3s %6d %-12s %10.3f %12.3f %6.3f .. %-6.3f %10.2f %10.2f" % (wl, ns, "counts nq 2", gb, med * 1e3, lo * 1e3, hi * 1e3,
                                                                           gb / med / 1e3, med / (yard / 2)), flush=True)
    if use_torch:
        ns = 16
        ours, _, _ = _timed(lambda: e.samples_quantiles(PROBS, 0, ns), reps, e.sync)
        try:
            torch.cuda.synchronize(); torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            ts = []
            for _ in range(reps):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                X = e.samples_torch(0, ns, layout=1)[1]          # [ns][nfields][nc]
                p = torch.tensor(PROBS, dtype=torch.float64, device=X.device)
                q = torch.empty((nf, len(PROBS)), dtype=torch.float64, device=X.device)
                for f in range(nf):                              # one field at a time: torch.quantile refuses more than 16 M elements,
                    v = torch.sort(X[:, f, :].reshape(-1)).values                      # so a sort and the same interpolation
                    pos = p * (v.numel() - 1)
                    lo_ = pos.floor().long()
                    hi_ = torch.clamp(lo_ + 1, max=v.numel() - 1)
                    q[f] = v[lo_] + (v[hi_] - v[lo_]) * (pos - lo_)
                    del v
                torch.cuda.synchronize()
                ts.append(time.perf_counter() - t0)
                del X
            peak = torch.cuda.max_memory_allocated() - base
            err = np.nanmax(np.abs(q.cpu().numpy() - e.samples_quantiles(PROBS, 0, ns)))
            print("# %s: samples_torch(layout=1) of %d samples + a sort per field in torch (%d quantiles): %.1f ms (min %.1f, max %.1f), peak "
                  "device memory %.2f GB beside the ring; samples_quantiles: %.3f ms, scratch %.2f MB; largest difference of the two %.1e"
                  % (wl, ns, len(PROBS), np.median(ts) * 1e3, min(ts) * 1e3, max(ts) * 1e3, peak / 1e9, ours * 1e3,
                     8 * nf * 2 * len(PROBS) * 260 / 1e6, err), flush=True)
        except RuntimeError as ex:                               # it may not fit at all: that is the result
            print("# %s: the torch route over %d samples did not run: %s; samples_quantiles: %.3f ms" % (wl, ns, str(ex).splitlines()[0][:200],
                                                                                                   ours * 1e3), flush=True)
    e.close()


def trace_stats(path):
    """quant_* / diag_tile_kernel lines of a rocprofv3 kernel_stats.csv."""
    import csv
    for r in csv.DictReader(open(path)):
        if "quant_" in r["Name"] or "diag_tile" in r["Name"]:
            print("%-44s calls %5s average %10.1f us min %10.1f max %10.1f" % (r["Name"][:44], r["Calls"], float(r["AverageNs"]) / 1e3,
                                                                             float(r["MinNs"]) / 1e3, float(r["MaxNs"]) / 1e3))


def pmc_stats(path):
    """quant_hist_kernel / quant_counts_kernel / diag_tile_kernel dispatches of a rocprofv3 --pmc counter_collection.csv: every counter summed
    per dispatch; a select's eight passes are eight consecutive quant_hist_kernel dispatches."""
    import csv
    acc, names = {}, {}
    for r in csv.DictReader(open(path)):
        k = r.get("Kernel_Name", "")
        if "quant_hist" in k or "quant_counts_kernel" in k or "diag_tile" in k:
            d = int(r["Dispatch_Id"])
            acc.setdefault(d, {})
            acc[d][r["Counter_Name"]] = acc[d].get(r["Counter_Name"], 0.0) + float(r["Counter_Value"])
            names[d] = k
    for d in sorted(acc):
        print("dispatch %7d %-34s %s" % (d, names[d][:34], "  ".join("%s %.4g" % (c, v) for c, v in sorted(acc[d].items()))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--workloads", nargs="*", default=["c3", "c4"])
    ap.add_argument("--mem-fraction", type=float, default=0.5, help="share of the device memory free beside the state that the ring takes")
    ap.add_argument("--no-torch", action="store_true")
    ap.add_argument("--trace-stats", help="a rocprofv3 kernel_stats.csv of a run of this tool: print the kernels' durations and stop")
    ap.add_argument("--pmc-stats", help="a rocprofv3 --pmc counter_collection.csv of a run of this tool: the counters per dispatch")
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
