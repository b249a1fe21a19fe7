"""What the sample store's histograms cost (mcmcx_samples_hist_dev / mcmcx_samples_hist2_dev): on BASELINE configuration c3's shape
(262 144 chains, npar 20) and the headline's (c4, method = 'ram', 1 048 576 chains, npar 50), with the largest ring that fits a share of the
free device memory beside the state, over the whole ring and over a window of 16 samples: wall time of a synchronised call (median of --reps
after one warm call) of the 1-D pass at 32, 256 and 1024 bins (every field) and of the 2-D pass at 64 bins for 1 and 16 pairs.  The edges are
uniform between the 0.5 % and 99.5 % points of every field (mcmcx_samples_quantiles of the 16-sample window).  The yardsticks, in the same
session: mcmcx_samples_stats_dev at maxlag = 0 over the same window, which reads the window twice -- so HALF its time is what one pass over
the window costs a kernel of this shape -- and mcmcx_samples_counts_dev at nq = 32, the route to a 31-bin histogram there was before.
`x half` is a call's time against half the stats call's; a 2-D call reads 2 x pairs of the nfields rows, `x rows` scales the half yardstick
to those.  Evidence for DESIGN.md section 5j; run on the GPU box from the repository root:

    python tools/hist_cost.py [--reps 3] [--workloads c3 c4] > hist_cost.txt

What bounds a pass comes from a counter run of its own (no tracing beside it):

    rocprofv3 --pmc SQ_INSTS_VALU SQ_INSTS_LDS SQ_ACTIVE_INST_LDS SQ_LDS_BANK_CONFLICT SQ_WAVE_CYCLES SQ_BUSY_CYCLES --output-format csv -d DIR -o pmc \\
        -- python tools/hist_cost.py --reps 1 --workloads c3 --mem-fraction 0.1
    python tools/hist_cost.py --pmc-stats DIR/.../pmc_counter_collection.csv
"""
import argparse
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from quantile_cost import CHAINS, WARM, _timed  # noqa: E402

BINS = (32, 256, 1024)
NPAIRS = (1, 16)
DP, IP = C.POINTER(C.c_double), C.POINTER(C.c_int32)


def measure(wl, reps, frac):
    import torch
    from mcmcf90_amd import engine_from_problem
    from mcmcf90_amd.engine import sample_nfields, samples_hist_edges
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
    print("%3s %6s %-16s %10s %12s %15s %10s %8s %8s" % ("wl", "ns", "call", "window GB", "ms (median)", "min .. max", "TB/s read", "x half",
                                                       "x rows"))
    q = e.samples_quantiles([0.005, 0.995], cap - 16, 16)
    lo, hi = q[:, 0].copy(), q[:, 1].copy()
    flat = ~(lo < hi)                                            # a constant field (sspri under a flat prior)
    lo[flat], hi[flat] = lo[flat] - 1.0, lo[flat] + 1.0
    dev = "cuda:%d" % e.cfg.device
    line = "%3s %6d %-16s %10.3f %12.3f %6.3f .. %-6.3f %10.2f %8s %8s"
    for ns in (cap, 16):
        gb = ns * slot / 1e9
        yard, a, b = _timed(lambda: e.samples_stats_torch(0, ns, 0), reps, e.sync)
        print(line % (wl, ns, "stats lag 0", gb, yard * 1e3, a * 1e3, b * 1e3, 2 * gb / yard / 1e3, "(2 passes)", ""), flush=True)
        half = yard / 2
        x32 = np.ascontiguousarray(np.stack([samples_hist_edges(lo[f], hi[f], 31) for f in range(nf)]))
        cnt = torch.empty((nf, 32, 2), dtype=torch.int64, device=dev)

        def counts():
            e._chk(e.L.mcmcx_samples_counts_dev(e.h, 0, ns, 32, x32.ctypes.data_as(DP), C.c_void_p(cnt.data_ptr())))
            e.sync()
        med, a, b = _timed(counts, reps, e.sync)
        print(line % (wl, ns, "counts nq 32", gb, med * 1e3, a * 1e3, b * 1e3, gb / med / 1e3, "%.2f" % (med / half), ""), flush=True)
        for nb in BINS:
            ed = np.ascontiguousarray(np.stack([samples_hist_edges(lo[f], hi[f], nb) for f in range(nf)]))
            out = torch.empty((nf, nb + 2), dtype=torch.int64, device=dev)

            def hist():
                e._chk(e.L.mcmcx_samples_hist_dev(e.h, 0, ns, nb, ed.ctypes.data_as(DP), C.c_void_p(out.data_ptr())))
                e.sync()
            med, a, b = _timed(hist, reps, e.sync)
            assert int(out.sum()) == nf * ns * n
            print(line % (wl, ns, "hist %d bins" % nb, gb, med * 1e3, a * 1e3, b * 1e3, gb / med / 1e3, "%.2f" % (med / half), ""), flush=True)
        ed = np.ascontiguousarray(np.stack([samples_hist_edges(lo[f], hi[f], 64) for f in range(nf)]))
        for npairs in NPAIRS:
            pairs = np.ascontiguousarray([(p % nf, (p + 1 + p // nf) % nf) for p in range(npairs)], dtype=np.int32)
            out = torch.empty((npairs, 66, 66), dtype=torch.int64, device=dev)

            def hist2():
                e._chk(e.L.mcmcx_samples_hist2_dev(e.h, 0, ns, npairs, pairs.ctypes.data_as(IP), 64, ed.ctypes.data_as(DP),
                                                   C.c_void_p(out.data_ptr())))
                e.sync()
            med, a, b = _timed(hist2, reps, e.sync)
            assert int(out.sum()) == npairs * ns * n
            rows = gb * 2 * npairs / nf
            print(line % (wl, ns, "hist2 %d pairs" % npairs, gb, med * 1e3, a * 1e3, b * 1e3, rows / med / 1e3, "%.2f" % (med / half),
                          "%.2f" % (med / (half * 2 * npairs / nf))), flush=True)
    e.close()


def pmc_stats(path):
    """hist_kernel / hist2_kernel / quant_counts_kernel / diag_tile_kernel dispatches of a rocprofv3 --pmc counter_collection.csv: every
    counter summed per dispatch."""
    import csv
    acc, names = {}, {}
    for r in csv.DictReader(open(path)):
        k = r.get("Kernel_Name", "")
        if "hist_kernel" in k or "hist2_kernel" in k or "quant_counts_kernel" in k or "diag_tile" in k:
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
    ap.add_argument("--pmc-stats", help="a rocprofv3 --pmc counter_collection.csv of a run of this tool: the counters per dispatch")
    a = ap.parse_args()
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
        measure(wl, a.reps, a.mem_fraction)


if __name__ == "__main__":
    main()
