"""What a data set per chain costs (mcmcx_set_target_expdata_all): proposals/s of bench.py's c1x configuration (262 144 chains, nycol = 2,
ndata = 11, dram with drscale = 2 and updatesigma = 1) in three forms, alternating on one device, --reps runs each:

    shared   one data set for all chains (mcmcx_set_target_expdata_cols): step_kernel_cols, the data through scalar loads
    y        y per chain, x shared: step_kernel_cols<pcd>, 2 x 11 x 8 = 176 B of vector loads per evaluation and lane
    xy       x and y per chain: 176 + 2 x 88 = 352 B issued per evaluation (x_i is loaded once per column), 264 B distinct

Every chain is given the SAME data, so the three forms do identical arithmetic and end in identical states (checked: theta's bits of the
first run of each form).  Evidence for DESIGN.md section 5f-3; run on the GPU box from the repository root:

    python tools/chain_data_cost.py [--reps 5] > chain_data_cost.txt
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CHAINS, NSIMU, WARM = 262144, 311, 11
FORMS = ("shared", "y", "xy")


def device_line():
    import ctypes as C
    from mcmcf90_amd import _lib
    buf = C.create_string_buffer(256)
    _lib.load().mcmcx_device_info(0, buf, 256)
    return "# device: " + buf.value.decode()


def run_once(form, chains, nsimu):
    """(proposals/s over iterations WARM + 1 .. nsimu, ticks included; the kernel that ran; bytes of the per-chain tables; theta)."""
    from mcmcf90_amd import engine_from_problem
    from mcmcf90_amd.workloads import problem
    ckw, pkw, ppi = problem("c1x", nsimu)
    e = engine_from_problem(ckw, pkw, nchains=chains)
    if form != "shared":
        x, y = np.asarray(pkw["xdata"], dtype=np.float64), np.asarray(pkw["ydata"], dtype=np.float64)
        e.set_target_all(np.tile(x, (chains, 1)) if form == "xy" else x, np.ascontiguousarray(np.broadcast_to(y, (chains,) + y.shape)))
    e.init()
    e.run(WARM); e.sync()
    t0 = time.perf_counter()
    e.run(); e.sync()
    dt = time.perf_counter() - t0
    k, nbytes, theta = e.last_kernel(), e.chain_data_info()["bytes"], e.theta()
    e.close()
    return chains * ppi * (nsimu - WARM) / dt, k, nbytes, theta


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--chains", type=int, default=CHAINS)
    ap.add_argument("--nsimu", type=int, default=NSIMU)
    a = ap.parse_args()
    print(device_line())
    print("# c1x: %d chains, nycol 2, ndata 11, dram drscale 2, updatesigma 1; proposals/s over iterations %d .. %d (delayed rejection's "
          "second tries not counted), %d alternating runs" % (a.chains, WARM + 1, a.nsimu, a.reps))
    rate = {f: [] for f in FORMS}
    info, first = {}, {}
    for rep in range(a.reps):
        for f in FORMS:
            r, k, nbytes, theta = run_once(f, a.chains, a.nsimu)
            rate[f].append(r)
            info[f] = (k, nbytes)
            if rep == 0:
                first[f] = theta.view(np.uint64)
    same = all(np.array_equal(first["shared"], first[f]) for f in FORMS)
    base = np.median(rate["shared"])
    print("%-7s %-24s %10s %12s %26s %8s %7s" % ("form", "kernel", "tables MB", "median", "min .. max", "spread", "ratio"))
    for f in FORMS:
        v = np.array(rate[f])
        print("%-7s %-24s %10.1f %12.4g %12.4g .. %-11.4g %7.1f%% %7.3f" % (f, info[f][0], info[f][1] / 1e6, np.median(v), v.min(), v.max(),
                                                                             100.0 * (v.max() - v.min()) / np.median(v), np.median(v) / base))
    print("# final theta of the three forms bit-identical: %s" % same)
    print("# raw: " + "; ".join("%s %s" % (f, " ".join("%.5g" % r for r in rate[f])) for f in FORMS), flush=True)
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
