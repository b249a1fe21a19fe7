"""Pooled mode's phase forms (a user module or host callbacks between the engine's launches) are entries of the kernel-selection tables
like every other sampling kernel: listed by mcmcx_debug_kernel_table (no device needed), named by mcmcx_last_kernel after a run, their base
names kernels of the build's resource report, and MCMCX_POOLED_PHASE_MFMA is one of the switches plan_kernels reads."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mcmcf90_amd", "csrc")


def test_the_kernel_table_lists_the_pooled_phase_forms():
    from mcmcf90_amd.engine import kernel_table
    tab = kernel_table()
    assert ("step", "pooled_phase_kernel") in tab
    assert ("step", "pooled_phase_mfma_kernel") in tab
    assert ("scam", "host_phase_kernel<pooled scam>") in tab
    assert {f for f, _ in tab} == {"step", "group", "scam"}


def test_the_resource_report_has_every_instance_at_the_occupancy_it_declares():
    rows = [l.split() for l in open(os.path.join(ROOT, "profiles", "kernel_resources.txt")) if l.startswith("pooled_phase_")]
    names = {" ".join(r[:-9]) for r in rows}
    for k in ("pooled_phase_kernel<0, -1>", "pooled_phase_kernel<1, 0>", "pooled_phase_kernel<2, 0>", "pooled_phase_kernel<4, 0>",
              "pooled_phase_mfma_kernel<-1, false>", "pooled_phase_mfma_kernel<1, false>", "pooled_phase_mfma_kernel<1, true>",
              "pooled_phase_mfma_kernel<2, false>", "pooled_phase_mfma_kernel<4, false>"):
        assert k in names, (k, sorted(names))
    for r in rows:
        if r[0].startswith("pooled_phase_mfma_kernel"):
            assert int(r[-1]) >= 2 and int(r[-5]) == 0 and int(r[-6]) == 0, r       # two waves per SIMD, no scratch, no spilled VGPRs


def test_the_switch_is_read_by_the_plan_only():
    hits = []
    for f in sorted(os.listdir(CSRC)):
        text = open(os.path.join(CSRC, f)).read()
        if re.search(r'"MCMCX_POOLED_PHASE_MFMA"', text):
            hits.append(f)
    assert hits == ["mcx_host_engine.hpp"], hits                          # mcx_switches::read, called by plan_kernels
    launch = open(os.path.join(CSRC, "mcx_host_launch.hpp")).read()
    assert "sw.pooled_phase_mfma" in launch
