"""What keeping thinned samples costs (mcmcx_set_samples): wall time per iteration of BASELINE configurations c2, c3 and c4 (method = 'ram',
the headline) at bench.py's chain counts with thin = off / 100 / 10 / 1, alternating on one device, medians and spread of --reps runs, each
as a ratio to "off" on the same build; and the keep kernel's rate, from the difference thin = 1 makes per iteration against the bytes a keep
moves (2 x 8 x nfields per chain, read + write).  Evidence for DESIGN.md's "Thinned samples"; run on the GPU box from the repository root:

    python tools/samples_cost.py [--reps 3] > samples_cost.txt

The difference of wall times holds the added launch boundary as well as the copy.  The keep kernel's OWN duration comes from a kernel trace of
one such run, which --keep-stats turns into bytes/s:

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o kt -- python tools/samples_cost.py --reps 1 --workloads c4 --thin 10
    python tools/samples_cost.py --keep-stats DIR/.../kt_kernel_stats.csv --workloads c4
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# configuration -> chains (bench.py's DEFAULT_CHAINS), iterations of a run
RUNS = {"c2": (65536, 2011), "c3": (262144, 1011), "c4": (1048576, 211)}
WARM = 11


def device_line():
    import ctypes as C
    from mcmcf90_amd import _lib
    buf = C.create_string_buffer(256)
    _lib.load().mcmcx_device_info(0, buf, 256)
    return "# device: " + buf.value.decode()


def run_once(wl, thin, chains=None, nsimu=None):
    """Seconds per iteration of iterations WARM + 1 .. nsimu (ticks and keeps included), the kernel that ran, samples kept in that range."""
    from mcmcf90_amd import engine_from_problem
    from mcmcf90_amd.workloads import problem
    n, ns = RUNS[wl]
    n, ns = chains or n, nsimu or ns
    ckw, pkw, _ = problem(wl, ns)
    e = engine_from_problem(ckw, pkw, nchains=n)
    if thin:
        e.set_samples(first=WARM + thin, thin=thin, capacity=2)       # a ring of two: the store's size does not depend on thin
    e.init()
    e.run(WARM); e.sync()
    t0 = time.perf_counter()
    e.run(); e.sync()
    dt = time.perf_counter() - t0
    kept = len(range(WARM + thin, ns + 1, thin)) if thin else 0
    k, nf = e.last_kernel(), e.samples_kept()[3]
    e.close()
    return dt / (ns - WARM), k, kept, nf


def keep_stats(path, wl):
    """samples_keep_kernel's line of a rocprofv3 kernel_stats.csv (a trace of ONE configuration) as durations and bytes/s."""
    import csv
    from mcmcf90_amd.engine import sample_nfields
    from mcmcf90_amd.workloads import problem
    nlanes = -(-RUNS[wl][0] // 64) * 64
    nbytes = 2 * 8 * sample_nfields(problem(wl, 10)[1]["npar"]) * nlanes
    for r in csv.DictReader(open(path)):
        if "samples_keep_kernel" in r["Name"]:
            avg, lo, hi = float(r["AverageNs"]), float(r["MinNs"]), float(r["MaxNs"])
            print("%s: samples_keep_kernel %s calls, %.1f MB each; average %.1f us (min %.1f, max %.1f) -> %.2f TB/s average, %.2f at best, of "
                  "6.29 TB/s" % (wl, r["Calls"], nbytes / 1e6, avg / 1e3, lo / 1e3, hi / 1e3, nbytes / avg / 1e3, nbytes / lo / 1e3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--workloads", nargs="*", default=["c2", "c3", "c4"])
    ap.add_argument("--thin", type=int, nargs="*", default=[0, 100, 10, 1])
    ap.add_argument("--keep-stats", help="a rocprofv3 kernel_stats.csv of a run of ONE of --workloads: print the keep kernel's rate and stop")
    a = ap.parse_args()
    if a.keep_stats:
        keep_stats(a.keep_stats, a.workloads[0])
        return
    print(device_line())
    print("# us per iteration, median of %d alternating runs (min .. max); ratio = median / median of thin = off" % a.reps)
    print("%3s %8s %-28s %5s %6s %10s %22s %7s" % ("wl", "chains", "kernel", "thin", "kept", "us/it", "min .. max", "ratio"))
    for wl in a.workloads:
        t = {th: [] for th in a.thin}
        info = {}
        for _ in range(a.reps):
            for th in a.thin:
                s, k, kept, nf = run_once(wl, th)
                t[th].append(s * 1e6)
                info[th] = (k, kept, nf)
        off = np.median(t[0]) if 0 in t else float("nan")
        for th in a.thin:
            k, kept, nf = info[th]
            print("%3s %8d %-28s %5s %6d %10.2f %10.2f .. %-9.2f %7.3f" % (wl, RUNS[wl][0], k[:28], th or "off", kept, np.median(t[th]), min(t[th]),
                                                                       max(t[th]), np.median(t[th]) / off), flush=True)
        if 0 in t and 1 in t:
            nlanes = -(-RUNS[wl][0] // 64) * 64
            nbytes = 2 * 8 * info[1][2] * nlanes
            extra = (np.median(t[1]) - off) * 1e-6
            print("#   a keep moves %.1f MB; thin = 1 adds %.2f us per iteration -> %.2f TB/s, launch and the cut's factor reload included"
                  % (nbytes / 1e6, extra * 1e6, nbytes / extra / 1e12 if extra > 0 else float("nan")), flush=True)


if __name__ == "__main__":
    main()
