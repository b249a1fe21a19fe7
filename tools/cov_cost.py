"""What the sample store's posterior covariance costs (mcmcx_samples_cov_dev): on BASELINE configuration c3's shape (262 144 chains, npar 20:
form A, two blocks), the headline's (c4, 1 048 576 chains, npar 50: form A, four blocks, ten accumulators) and config 5's (65 536 chains,
npar 200: form B, pooled as bench.py runs it), with the largest ring that fits a share of the free device memory beside the state, over the whole ring and over a window
of 16 samples; and `few`: 64 chains of c3's problem over a ring of 4096 -- one wave walks the whole window, so that case is latency
(reported, not built for).  Wall time of a synchronised call, median of --reps after one warm call.  The yardstick, in the same session:
mcmcx_samples_stats_dev at maxlag = 0 over the same window, which reads the window twice -- HALF its time is what one streaming pass over
the window costs a kernel of this shape (the yardstick DESIGN.md section 5h used); `cov/yard` is the covariance's time against that half.
Beside it the route a user had before: samples_torch(layout=1) of the 16-sample window and a matmul, as time, peak device memory and
relative difference (torch picks its own order of summation).  Evidence for DESIGN.md section 5i; run on the GPU box from the repository
root:

    python tools/cov_cost.py [--reps 3] [--workloads c3 c4 c5 few] > cov_cost.txt

What bounds a pass comes from a counter run of its own (no tracing beside it):

    rocprofv3 --pmc SQ_INSTS_VALU SQ_INSTS_SALU SQ_INSTS_LDS SQ_LDS_BANK_CONFLICT SQ_INSTS_MFMA SQ_BUSY_CYCLES --output-format csv -d DIR -o pmc \\
        -- python tools/cov_cost.py --reps 1 --workloads c4 --no-torch --mem-fraction 0.1
    python tools/cov_cost.py --pmc-stats DIR/.../pmc_counter_collection.csv
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CHAINS = {"c3": 262144, "c4": 1048576, "c5": 65536, "few": 64}   # bench.py's DEFAULT_CHAINS; few: one tile
WARM = 11
FEW_RING = 4096


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
    from mcmcf90_amd.engine import sample_nfields, samples_cov_finish, samples_cov_len
    from mcmcf90_amd.workloads import problem
    n = CHAINS[wl]
    base = "c3" if wl == "few" else wl
    ckw, pkw, _ = problem(base, 100)
    if wl == "c5":
        ckw["pooled"] = 1
    nf = sample_nfields(pkw["npar"])
    slot = 8 * nf * (-(-n // 64) * 64)
    if wl == "few":
        cap, free = FEW_RING, 0.0
    else:
        e = engine_from_problem(ckw, pkw, nchains=n)             # the state's size is not known before init
        e.init(); e.sync()
        free, total = torch.cuda.mem_get_info()
        e.close()
        cap = max(16, int(frac * free / slot))
    ckw, pkw, _ = problem(base, WARM + cap)
    if wl == "c5":
        ckw["pooled"] = 1                                        # the shape bench.py runs config 5 in; the writer does not matter to the reader
    e = engine_from_problem(ckw, pkw, nchains=n)
    e.set_samples(first=WARM + 1, thin=1, capacity=cap)
    e.init()
    e.run(); e.sync()
    assert e.samples_kept()[0] == cap
    ntiles = -(-n // 64)
    print("# %s: %d chains, nfields %d, a slot %.1f MB, ring of %d slots = %.2f GB, cov scratch %.1f MB, kernel %s"
          % (wl, n, nf, slot / 1e6, cap, cap * slot / 1e9, 8 * (ntiles * (nf + nf * (nf + 1) // 2) + nf + samples_cov_len(nf)) / 1e6,
             e.last_kernel()), flush=True)
    print("%3s %6s %-12s %10s %12s %15s %10s %10s" % ("wl", "ns", "call", "window GB", "ms (median)", "min .. max", "TB/s", "cov/yard"))
    for ns in (cap, 16):
        gb = ns * slot / 1e9
        yard, lo, hi = _timed(lambda: e.samples_stats_torch(0, ns, 0), reps, e.sync)
        print("%3s %6d %-12s %10.3f %12.3f %6.3f .. %-6.3f %10.2f %10s" % (wl, ns, "stats lag 0", gb, yard * 1e3, lo * 1e3, hi * 1e3,
                                                                          2 * gb / yard / 1e3, "(2 passes)"), flush=True)
        med, lo, hi = _timed(lambda: e.samples_cov_stats_torch(0, ns), reps, e.sync)
        print("%3s %6d %-12s %10.3f %12.3f %6.3f .. %-6.3f %10.2f %10.2f" % (wl, ns, "cov", gb, med * 1e3, lo * 1e3, hi * 1e3,
                                                                           gb / med / 1e3, med / (yard / 2)), flush=True)
    if use_torch and wl != "few":
        ns = 16
        ours, _, _ = _timed(lambda: e.samples_cov_stats_torch(0, ns), reps, e.sync)
        try:
            torch.cuda.synchronize(); torch.cuda.reset_peak_memory_stats()
            base_mem = torch.cuda.memory_allocated()
            ts = []
            for _ in range(reps):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                X = e.samples_torch(0, ns, layout=1)[1]          # [ns][nfields][nc]
                Zt = X.permute(1, 0, 2).reshape(nf, -1)
                Zt = Zt - Zt[:, :1]                              # the default shift: chain 0 of window sample 0
                S = Zt.sum(dim=1)
                Cm = (Zt @ Zt.T - torch.outer(S, S) / Zt.shape[1]) / (Zt.shape[1] - 1)
                torch.cuda.synchronize()
                ts.append(time.perf_counter() - t0)
                del X, Zt
            peak = torch.cuda.max_memory_allocated() - base_mem
            cov = samples_cov_finish(e.samples_cov_stats(0, ns), nf)[1]
            ref = Cm.cpu().numpy()
            scale = np.sqrt(np.outer(np.diag(cov), np.diag(cov)))
            with np.errstate(all="ignore"):
                rel = np.nanmax(np.where(scale > 0, np.abs(ref - cov) / scale, 0.0))
            print("# %s: samples_torch(layout=1) of %d samples + a matmul in torch: %.1f ms (min %.1f, max %.1f), peak device memory %.2f GB "
                  "beside the ring; samples_cov_stats_torch: %.3f ms; largest difference of the two covariances relative to "
                  "sqrt(C_jj C_kk): %.1e" % (wl, ns, np.median(ts) * 1e3, min(ts) * 1e3, max(ts) * 1e3, peak / 1e9, ours * 1e3, rel), flush=True)
        except RuntimeError as ex:                               # it may not fit at all: that is the result
            print("# %s: the torch route over %d samples did not run: %s; samples_cov_stats_torch: %.3f ms"
                  % (wl, ns, str(ex).splitlines()[0][:200], ours * 1e3), flush=True)
    e.close()


def pmc_stats(path):
    """cov_tile_kernel / diag_tile_kernel dispatches of a rocprofv3 --pmc counter_collection.csv: every counter summed per dispatch."""
    import csv
    acc, names = {}, {}
    for r in csv.DictReader(open(path)):
        k = r.get("Kernel_Name", "")
        if "cov_tile" in k or "diag_tile" in k:
            d = int(r["Dispatch_Id"])
            acc.setdefault(d, {})
            acc[d][r["Counter_Name"]] = acc[d].get(r["Counter_Name"], 0.0) + float(r["Counter_Value"])
            names[d] = k
    for d in sorted(acc):
        print("dispatch %7d %-34s %s" % (d, names[d][:34], "  ".join("%s %.4g" % (c, v) for c, v in sorted(acc[d].items()))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--workloads", nargs="*", default=["c3", "c4", "c5", "few"])
    ap.add_argument("--mem-fraction", type=float, default=0.5, help="share of the device memory free beside the state that the ring takes")
    ap.add_argument("--no-torch", action="store_true")
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
        measure(wl, a.reps, a.mem_fraction, not a.no_torch)


if __name__ == "__main__":
    main()
