"""The adaptation's SVD kernels on edge matrices, every compiled instance (mcmcx_debug_symsvd; the matrices: tests/svd_cases.py).

An engine run feeds these kernels the covariances of a few hundred iterations of smooth chains, seventy nearly equal matrices at a time.
Here the blocked kernels of mcx_svd.hpp (form 2, through the plan and launch functions the adaptation tick itself calls) and the lane form
symsvd_dev (form 1) get exact zeros in gamma, ties among the singular values, rank-deficient and ill-scaled input, the 60-sweep cap,
non-finite results, masked-out matrices, and neighbours that converge in different sweeps -- at both edges of every instance's npar
range and at every npar mod 8.  Every comparison is bit for bit with the oracle's routine (mcxo_symsvd) on the same arrays: V, s (the
bits of NaNs included) and the number of sweeps a matrix rotated in.

Left out: the lane form above npar 256, where the engine also runs it -- one factorisation there takes tens of seconds;
tests/test_gpu_fullsize.py::test_c5_illcond200_scam_replicas_two_ticks[lane_svd] remains the check of the lane form at a large size."""
import numpy as np
import pytest

from svd_cases import FAMILIES, bits, cases, check_refusals, oracle_svd, same_bits_up_to_nan_sign

pytestmark = pytest.mark.gpu

SENT = -7.25           # the caller's fill of V_out / s_out, and -3 of sweeps_out: what a row with need == 0 must keep


def _probe(form, d, names, need=None):
    from mcmcf90_amd.engine import debug_symsvd
    A = np.stack([cases(d)[n] for n in names])
    return debug_symsvd(form, A, need=need, fill=SENT, sweeps_fill=-3)


def _check(oracle, form, d, names, need=None):
    """One probe call on cases(d)[names]; every row against the oracle, or against the sentinel where need == 0.  Returns forms."""
    V, s, sw, forms = _probe(form, d, names, need)
    nd = np.ones(len(names), dtype=bool) if need is None else np.asarray(need, dtype=bool)
    ref = oracle_svd(oracle, d, [n for n, k in zip(names, nd) if k])
    ref = iter(ref)
    for m, n in enumerate(names):
        if not nd[m]:
            assert sw[m] == -3 and np.all(V[m] == SENT) and np.all(s[m] == SENT), (form, d, m, n)
            continue
        Vo, so, swo = next(ref)
        assert sw[m] == swo, (form, d, m, n, int(sw[m]), swo)
        if form == 0 and n == "huge":                           # host code: the sign of a NaN is the host compiler's (tests/test_svd_cpu.py)
            assert same_bits_up_to_nan_sign(s[m], so) and same_bits_up_to_nan_sign(V[m], Vo), (form, d, m, n)
            continue
        assert np.array_equal(bits(s[m]), bits(so)), (form, d, m, n)
        assert np.array_equal(bits(V[m]), bits(Vo)), (form, d, m, n)
    return forms


# what plan_svd's thresholds give each npar, written out: a moved threshold fails here
S32, ST, AV = "svd_sweep_stream32_kernel<%d>", "svd_sweep_stream_kernel<%d>", "svd_applyv_stream32_kernel<%d>"
INSTANCES = {48: (S32 % 8, AV % 4), 49: (S32 % 8, AV % 4), 63: (S32 % 8, AV % 4), 64: (S32 % 8, AV % 4),
             65: (S32 % 16, AV % 8), 127: (S32 % 16, AV % 8), 128: (S32 % 16, AV % 8),
             129: (S32 % 25, AV % 13), 199: (S32 % 25, AV % 13), 200: (S32 % 25, AV % 13),
             201: (ST % 26, AV % 13), 207: (ST % 26, AV % 13), 208: (ST % 26, AV % 13),
             209: (ST % 32, AV % 16), 255: (ST % 32, AV % 16), 256: (ST % 32, AV % 16)}


def test_instance_table_covers_every_instance_at_both_edges():
    """The literal table itself: five sweep and four replay instances, each at the first and the last npar of its range."""
    lo_hi = {}
    for d, (sweep, replay) in INSTANCES.items():
        for name in (sweep, replay):
            lo, hi = lo_hi.get(name, (d, d))
            lo_hi[name] = (min(lo, d), max(hi, d))
    assert lo_hi == {S32 % 8: (48, 64), S32 % 16: (65, 128), S32 % 25: (129, 200), ST % 26: (201, 208), ST % 32: (209, 256),
                     AV % 4: (48, 64), AV % 8: (65, 128), AV % 13: (129, 208), AV % 16: (209, 256)}


@pytest.mark.parametrize("d", sorted(INSTANCES))
def test_blocked_every_instance_at_both_edges(oracle, d):
    """One probe call per npar.  Up to 129 nine matrices in an order that puts chains converging in different sweeps (0 for identity,
    diag_rep and zero, 7 .. 40 for the others) next to each other: a chain in state 2 is skipped by the sweep and by the replay while its
    neighbours go on.  From 199 on five, the last with need = 0 (state 0: no kernel may touch its row)."""
    if d <= 129:
        names, need = ["dense", "identity", "few", "block", "diag_rep", "ill", "lowrank", "rank1", "zero"], None
    else:
        names, need = ["dense", "few", "block", "diag_rep", "identity"], [1, 1, 1, 1, 0]
    forms = _check(oracle, 2, d, names, need)
    assert forms == "+".join(INSTANCES[d])


@pytest.mark.parametrize("mask", ["all", "none", "alternating", "last"])
@pytest.mark.parametrize("nmat", [1, 7, 8, 9, 13])
def test_blocked_matrix_counts_and_need_masks(oracle, nmat, mask):
    """npar 65, matrix counts around the replay's unit of eight chains (its grid is 32 ceil(n / 8) one-wave workgroups, a chain's four
    placed by block index), the families cycled, and four need masks; with none needed the call succeeds and writes nothing."""
    d = 65
    names = [FAMILIES[m % len(FAMILIES)] for m in range(nmat)]
    need = {"all": np.ones(nmat), "none": np.zeros(nmat), "alternating": np.arange(nmat) % 2, "last": np.arange(nmat) == nmat - 1}[mask]
    forms = _check(oracle, 2, d, names, need.astype(np.uint8))
    assert forms == "+".join(INSTANCES[d])


@pytest.mark.parametrize("name,d", [("small", 48), ("small", 129), ("small", 201), ("small", 209), ("ones", 129), ("tiny", 48), ("huge", 48),
                                    ("huge", 65)])
def test_blocked_sweep_cap_and_ill_scaled(oracle, name, d):
    """The 60-sweep cap next to a chain that stops after a few sweeps: the named matrix is still in state 1 when svd_finish_kernel runs,
    dense went to state 2 long before.  small / tiny: alpha * beta underflows; huge: it overflows and the results are non-finite (NaN bits
    compared); ones at npar 129: a rank-one matrix whose rotations never die out."""
    ref = oracle_svd(oracle, d, [name, "dense"])
    assert ref[0][2] == 60 and ref[1][2] < 20, (ref[0][2], ref[1][2])
    if name == "huge":
        assert not np.all(np.isfinite(ref[0][0]))
    forms = _check(oracle, 2, d, [name, "dense"])
    assert forms == "+".join(INSTANCES[d])


@pytest.mark.parametrize("d", [1, 2, 3, 7, 8, 9, 15, 16, 17, 31, 47, 48])
def test_lane_form_mixed_waves(oracle, d):
    """symsvd_dev, seventy matrices = two tiles, the second ragged: the families cycled (all but tiny), so that every wave holds lanes that
    rotate a given pair and lanes that do not (the wave-uniform __any(rot) branch, and alpha carried over where nobody rotates), lanes that
    converged long ago, and lanes at the sweep cap; the need mask alternates in the second tile."""
    fam = [n for n in FAMILIES if n != "tiny"]
    names = [fam[m % len(fam)] for m in range(70)]
    need = np.ones(70, dtype=np.uint8)
    need[64:] = np.arange(6) % 2
    forms = _check(oracle, 1, d, names, need)
    assert forms == "symsvd_dev"


def test_three_forms_agree(oracle):
    """npar 48, every family: the host's statement, the lane form and the blocked kernels, each against the oracle -- hence each other.
    (The two device forms to the bit, NaNs included; the host's NaNs of huge up to their sign.)"""
    names = list(FAMILIES)
    assert _check(oracle, 0, 48, names) == "host_symsvd"
    assert _check(oracle, 1, 48, names) == "symsvd_dev"
    assert _check(oracle, 2, 48, names) == "+".join(INSTANCES[48])


def test_refusals_launch_nothing(oracle):
    """Every refusal of the probe with a device present: -1, its message, nothing written -- and the probe works afterwards."""
    check_refusals()
    assert _check(oracle, 2, 48, ["dense", "zero"]) == "+".join(INSTANCES[48])
