"""Edge matrices for the three statements of the pinned SVD (oracle/mcx_svd.h): host_symsvd, symsvd_dev and the blocked kernels of
mcx_svd.hpp, all reached through mcmcx_debug_symsvd.  cases(d) is an ordered dict of symmetric d x d float64 matrices from
np.random.default_rng(1000 + d); every family is symmetrised with (S + S.T) / 2.  What a family is for:

    identity, zero   no rotation at all
    diag_rep         diag(2.., 2.., 0.5.., 0..): ties and a null space, "first maximum wins" alone decides V's column order
    dense            A A' + diag(10**linspace(-1, 2, d)): the engine tests' matrix
    lowrank, rank1   rank-deficient: exact and near zeros among the column norms
    few              the sample covariance of 5 draws (rank 4): an adaptation after 5 iterations
    block            a dense top-left half, a diagonal rest: gamma is exactly 0 for half of all pairs
    ill              condition 1e14
    ones             all ones: from npar 129 on the routine reaches its 60-sweep cap
    small            dense * 1e-100: alpha * beta underflows to 0, the tolerance vanishes, the cap
    tiny             dense * 1e-160: subnormal column norms, the cap
    huge             dense * 1e160: alpha * beta overflows, non-finite results, the cap

oracle_svd runs the oracle's routine on a list of matrices (threads: ctypes releases the interpreter lock, a call at npar 256 takes
seconds) and keeps every result for the session, so that tests sharing a matrix share its reference."""
import collections
import ctypes as C
from concurrent.futures import ThreadPoolExecutor

import numpy as np

FAMILIES = ("identity", "zero", "diag_rep", "dense", "lowrank", "rank1", "few", "block", "ill", "ones", "small", "tiny", "huge")
ILL_SCALED = ("small", "tiny", "huge")
_CASES = {}
_REF = {}


def _sym(S):
    return (S + S.T) / 2


def cases(d):
    if d in _CASES:
        return _CASES[d]
    rng = np.random.default_rng(1000 + d)
    out = collections.OrderedDict()
    out["identity"] = np.eye(d)
    out["zero"] = np.zeros((d, d))
    q = d // 4
    out["diag_rep"] = np.diag(np.concatenate([np.full(q, 2.0), np.full(q, 2.0), np.full(q, 0.5), np.zeros(d - 3 * q)]))
    A = rng.standard_normal((d, d)) / np.sqrt(d)
    dense = _sym(A @ A.T + np.diag(10.0 ** np.linspace(-1, 2, d)))
    out["dense"] = dense
    X = rng.standard_normal((d, max(1, d // 3)))
    out["lowrank"] = _sym(X @ X.T / d)
    x = rng.standard_normal(d)
    out["rank1"] = _sym(np.outer(x, x))
    Y = rng.standard_normal((5, d))
    Yc = Y - Y.mean(axis=0)
    out["few"] = _sym(Yc.T @ Yc / 4.0)
    h = d // 2
    blk = np.zeros((d, d))
    if h > 0:
        B = rng.standard_normal((h, h))
        blk[:h, :h] = B @ B.T / h
    r = d - h
    blk[h:, h:] = np.diag(np.concatenate([np.full(r // 2, 3.0), np.full(r - r // 2, 1.0)]))
    out["block"] = _sym(blk)
    Q, _ = np.linalg.qr(rng.standard_normal((d, d)))
    out["ill"] = _sym((Q * 10.0 ** np.linspace(0, -14, d)) @ Q.T)
    out["ones"] = np.ones((d, d))
    out["small"] = _sym(dense * 1e-100)
    out["tiny"] = _sym(dense * 1e-160)
    out["huge"] = _sym(dense * 1e160)
    assert tuple(out) == FAMILIES
    for k, v in out.items():
        assert v.shape == (d, d) and np.array_equal(v, v.T), k
        v.setflags(write=False)
    _CASES[d] = out
    return out


def _dp(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def _one(L, A):
    d = A.shape[0]
    G = np.asfortranarray(A.copy()); V = np.zeros((d, d), order="F"); s = np.zeros(d)
    sweeps = L.mcxo_symsvd(d, _dp(G), _dp(V), _dp(s))
    V = np.array(V); V.setflags(write=False); s.setflags(write=False)
    return V, s, int(sweeps)


def oracle_svd(oracle, d, names):
    """[(V, s, sweeps)] of mcxo_symsvd for cases(d)[name], name in names; computed once per (d, name), read-only."""
    L = oracle.lib()
    cs = cases(d)
    todo = [n for n in dict.fromkeys(names) if (d, n) not in _REF]
    if todo:
        with ThreadPoolExecutor(max_workers=min(8, len(todo))) as ex:
            for n, r in zip(todo, ex.map(lambda n: _one(L, cs[n]), todo)):
                _REF[(d, n)] = r
    return [_REF[(d, n)] for n in names]


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same_bits_up_to_nan_sign(a, b):
    """Bit for bit, except that two NaNs may differ in their sign bit (payloads compared).  For host code only: an x86 add of two NaNs
    returns its first operand's, and which of fabs(zeta) (a positive NaN) and sqrt(1 + zeta * zeta) (a negative one: x86's default NaN)
    comes first is each compiler's choice, so the oracle's build and the library's host build may differ there and nowhere else."""
    a, b = bits(a), bits(b)
    nan = np.isnan(a.view(np.float64)) & np.isnan(b.view(np.float64))
    return bool(np.all((a == b) | (nan & ((a ^ b) == np.uint64(1 << 63)))))


def refusal_cases():
    """(form, d, nmat, null argument or None, len, fragment of the message): every refusal of mcmcx_debug_symsvd"""
    return [(0, 4, 2, "A", 64, b"null"), (0, 4, 2, "V", 64, b"null"), (0, 4, 2, "s", 64, b"null"), (1, 4, 2, "A", 64, b"null"),
            (2, 48, 2, "s", 64, b"null"), (0, 0, 2, None, 64, b"d outside"), (1, -3, 2, None, 64, b"d outside"), (0, 4, 0, None, 64, b"nmat"),
            (2, 48, -1, None, 64, b"nmat"), (3, 4, 2, None, 64, b"form"), (-1, 4, 2, None, 64, b"form"), (2, 47, 2, None, 64, b"48 .. 256"),
            (2, 257, 2, None, 64, b"48 .. 256"), (2, 4, 2, None, 64, b"48 .. 256"), (0, 4, 2, None, len("host_symsvd"), b"len"),
            (0, 4, 2, None, 0, b"len"), (1, 4, 2, None, len("symsvd_dev"), b"len"),
            (2, 201, 2, None, len("svd_sweep_stream_kernel<26>+svd_applyv_stream32_kernel<13>"), b"len")]


def check_refusals():
    """Each refusal returns -1 with its message and writes nothing (tests/test_svd_cpu.py without a device; tests/test_gpu_svd.py where one is there to launch on)."""
    from mcmcf90_amd import _lib
    L = _lib.load()
    dp = C.POINTER(C.c_double)
    for form, d, nmat, null, ln, frag in refusal_cases():
        n = max(nmat, 1) * max(d, 1) ** 2
        A = np.full(n, 0.5); V = np.full(n, 7.0); s = np.full(n, 7.0); sw = np.full(max(nmat, 1), 7, dtype=np.int32)
        buf = C.create_string_buffer(b"\x55" * 127, 128)
        rc = L.mcmcx_debug_symsvd(0, form, d, nmat, None if null == "A" else A.ctypes.data_as(dp), None,
                                  None if null == "V" else V.ctypes.data_as(dp), None if null == "s" else s.ctypes.data_as(dp),
                                  sw.ctypes.data_as(C.POINTER(C.c_int32)), buf, ln)
        assert rc == -1 and frag in L.mcmcx_last_error(), (form, d, nmat, null, ln, rc, L.mcmcx_last_error())
        assert np.all(V == 7.0) and np.all(s == 7.0) and np.all(sw == 7) and buf.raw[:127] == b"\x55" * 127, (form, d, nmat, null, ln)
