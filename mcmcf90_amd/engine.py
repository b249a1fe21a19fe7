"""Host-side mirror of mcmcf90's user surface on top of the C ABI.

`McmcConfig` carries the numeric members of namelist /mcmc/ (mcmcinit.F90:74-82) with the reference's
defaults (:184-230); `Engine` follows the call sequence of a reference driver program:
MCMC_setpar0 / MCMC_setcmat0 / MCMC_setsigma2nobs (MCMC_init.F90:168-347, testcases/mcmcrun3.F90:18-23),
then mcmc_main() = init + run (mcmc_main.F90:12-44), then the chain/sschain/s2chain arrays.
Every call goes through libmcmcx.so; nothing is computed in Python.
"""
import ctypes as C
import numpy as np
from . import _lib

METHODS = {"dram": 0, "ram": 1, "scam": 2, "er": 3}


class McmcError(RuntimeError):
    pass


def _dp(a):
    return a.ctypes.data_as(C.POINTER(C.c_double)) if a is not None else None


def _f64(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64))


def make_config(npar, nchains=1, **kw):
    c = _lib.Config()
    _lib.load().mcmcx_config_defaults(C.byref(c))
    c.npar, c.nchains = int(npar), int(nchains)
    for k, v in kw.items():
        if k == "method" and isinstance(v, str):
            v = METHODS[v]
        if not hasattr(c, k):
            raise KeyError(k)
        setattr(c, k, v)
    return c


def chain_data_arrays(nchains, npar, xdata, ydata):
    """(x, y, nycol, x_per_chain) for Engine.set_target_all: y as a contiguous float64 (nchains, nycol, ndata) from ydata (nchains, nycol,
    ndata) or (nchains, ndata), x as a contiguous float64 (ndata,) -- x_per_chain = 0 -- or (nchains, ndata) -- 1.  Raises ValueError on
    shapes that do not fit nchains, npar = 1 + nycol or each other; no library call."""
    x, y = _f64(xdata), _f64(ydata)
    nchains, npar = int(nchains), int(npar)
    if y.ndim == 2:
        if npar != 2:
            raise ValueError("ydata is (nchains, ndata): one response column needs npar = 2, got npar = %d" % npar)
        y = y.reshape(y.shape[0], 1, y.shape[1])
    if y.ndim != 3:
        raise ValueError("ydata must be (nchains, nycol, ndata) or (nchains, ndata), got %s" % (y.shape,))
    if y.shape[0] != nchains:
        raise ValueError("ydata holds %d data sets, the engine has %d chains" % (y.shape[0], nchains))
    nycol, ndata = y.shape[1], y.shape[2]
    if nycol < 1 or ndata < 1:
        raise ValueError("ydata must hold at least one column and one observation, got %s" % (y.shape,))
    if npar != 1 + nycol:
        raise ValueError("the model has npar = 1 + nycol parameters: npar = %d, nycol = %d" % (npar, nycol))
    if x.shape == (ndata,):
        return x, y, nycol, 0
    if x.shape == (nchains, ndata):
        return x, y, nycol, 1
    raise ValueError("xdata must be (ndata,) = (%d,) or (nchains, ndata) = (%d, %d), got %s" % (ndata, nchains, ndata, x.shape))


def sample_iterations(first, thin, capacity, simuind):
    """The iterations a sample store retains once the run stands at `simuind` (mcmcx_set_samples' rule, stated once): iteration i,
    1 <= i <= simuind, is kept when i >= first and (i - first) % thin == 0, and the ring holds the last `capacity` of those.
    thin = 0 (sampling off) and first > simuind keep nothing."""
    first, thin, capacity, simuind = int(first), int(thin), int(capacity), int(simuind)
    if thin <= 0 or capacity < 1 or simuind < first:
        return []
    n = (simuind - first) // thin + 1
    r = min(n, capacity)
    return [first + (n - r + j) * thin for j in range(r)]


def sample_nfields(npar, nycol=1):
    """Doubles per chain and sample: theta[npar], ss[nycol], sspri, sigma2[nycol]."""
    return int(npar) + 2 * int(nycol) + 1


def sample_store_offset(slot, ntiles, nfields, tile, field):
    """Element offset of a 64-chain row in the device store, [slot][ntiles][nfields][64] doubles (mcx_samples.hpp: samples_row)."""
    return ((int(slot) * int(ntiles) + int(tile)) * int(nfields) + int(field)) * 64


DIAG_MAXLAG = 32
DIAG_COLUMNS = ("mean", "sd", "rhat", "ess", "mcse", "W", "Bn", "truncated")
XF_IDENTITY, XF_LE, XF_FOLD, XF_SQUARE = 0, 1, 2, 3            # Engine.samples_stats_of's kinds (MCMCX_XF_*)


def samples_stats_len(nfields, maxlag):
    """Doubles of a stats vector: [M, n_h, K, then per field: shift, S1, S2, G_0 .. G_maxlag] (mcmcx_samples_stats, include/mcmcx.h)."""
    return 3 + int(nfields) * (int(maxlag) + 4)


def samples_diag(stats, nfields, maxlag):
    """[nfields][8] -- mean, sd, rhat, ess, mcse, W, Bn, truncated -- from a stats vector (one engine's, or the sum of several engines'
    that used the same shift): mcmcx_samples_diag, pure host arithmetic, no engine and no device."""
    L = _lib.load()
    st = _f64(stats)
    if st.size != samples_stats_len(nfields, maxlag):
        raise McmcError("samples_diag: %d doubles given, nfields %d and maxlag %d make %d" % (st.size, nfields, maxlag,
                                                                                            samples_stats_len(nfields, maxlag)))
    table = np.zeros((int(nfields), 8))
    if L.mcmcx_samples_diag(_dp(st), int(nfields), int(maxlag), _dp(table)) < 0:
        raise McmcError(L.mcmcx_last_error().decode())
    return table


def samples_cov_len(nfields):
    """Doubles of a cov vector: [n, shift[nfields], S[nfields], G packed by rows of the upper triangle] (mcmcx_samples_cov, include/mcmcx.h)."""
    nf = int(nfields)
    return 1 + 2 * nf + nf * (nf + 1) // 2


def samples_cov_finish(vec, nfields):
    """(mean[nfields], cov[nfields][nfields], corr[nfields][nfields]) from a cov vector (one engine's, or the sum of several engines' that
    used the same shift): mcmcx_samples_cov_finish, pure host arithmetic, no engine and no device.  A constant field has a NaN row and
    column in corr."""
    L = _lib.load()
    v = _f64(vec)
    nf = int(nfields)
    if v.size != samples_cov_len(nf):
        raise McmcError("samples_cov_finish: %d doubles given, nfields %d makes %d" % (v.size, nf, samples_cov_len(nf)))
    mean, cov, corr = np.zeros(nf), np.zeros((nf, nf)), np.zeros((nf, nf))
    if L.mcmcx_samples_cov_finish(_dp(v), nf, _dp(mean), _dp(cov), _dp(corr)) < 0:
        raise McmcError(L.mcmcx_last_error().decode())
    return mean, cov, corr                                      # symmetric: column-major is row-major


def _sel(sel, nfields, who):
    """a field selection as a contiguous int32 array"""
    idx = np.ascontiguousarray(np.asarray(sel, dtype=np.int32).ravel())
    if idx.size < 1 or idx.size > int(nfields):
        raise McmcError("%s: %d fields selected of %d" % (who, idx.size, int(nfields)))
    return idx


def _two_vectors(cov_vec, bm_vec, nfields, who):
    cv, bv = _f64(cov_vec), _f64(bm_vec)
    for v in (cv, bv):
        if v.size != samples_cov_len(nfields):
            raise McmcError("%s: %d doubles given, nfields %d makes %d" % (who, v.size, int(nfields), samples_cov_len(nfields)))
    return cv, bv


def samples_mess(cov_vec, bm_vec, nfields, batch, sel):
    """dict: `mess`, the multivariate effective sample size of the fields `sel` (Vats, Flegal, Jones 2019, replicated batch means), `n`,
    `logdet_lambda`, `logdet_sigma`, `ess_bm` [nsel] (the univariate batch-means ESS of each selected field) and `warn` (1: a matrix was
    not positive definite -- a constant field was selected -- and the results are NaN) from a cov vector and the batch-means vector of the
    same nb x batch samples (one engine's each, or sums over engines): mcmcx_samples_mess, pure host, no engine and no device."""
    L = _lib.load()
    nf = int(nfields)
    cv, bv = _two_vectors(cov_vec, bm_vec, nf, "samples_mess")
    idx = _sel(sel, nf, "samples_mess")
    out4, ess = np.zeros(4), np.zeros(idx.size)
    rc = L.mcmcx_samples_mess(_dp(cv), _dp(bv), nf, int(batch), int(idx.size), idx.ctypes.data_as(C.POINTER(C.c_int32)), _dp(out4), _dp(ess))
    if rc < 0:
        raise McmcError(L.mcmcx_last_error().decode())
    return {"mess": out4[0], "n": out4[1], "logdet_lambda": out4[2], "logdet_sigma": out4[3], "ess_bm": ess, "warn": int(rc)}


def samples_mpsrf(cov_vec, bm_vec, nfields, n_h, sel):
    """dict: `mpsrf`, the multivariate split-R-hat of the fields `sel` (Brooks and Gelman 1998, without coda's (M + 1) / M: with one field it
    is samples_diag's rhat), `lambda1`, `M` (split chains), `n_h`, `W` and `Bn` [nsel][nsel], and `warn` (1: W was not positive definite,
    mpsrf is NaN) from the cov vector of a window of 2 n_h samples and the batch-means vector of the same window with batch = n_h:
    mcmcx_samples_mpsrf, pure host, no engine and no device."""
    L = _lib.load()
    nf = int(nfields)
    cv, bv = _two_vectors(cov_vec, bm_vec, nf, "samples_mpsrf")
    idx = _sel(sel, nf, "samples_mpsrf")
    out4, W, Bn = np.zeros(4), np.zeros((idx.size, idx.size)), np.zeros((idx.size, idx.size))
    rc = L.mcmcx_samples_mpsrf(_dp(cv), _dp(bv), nf, int(n_h), int(idx.size), idx.ctypes.data_as(C.POINTER(C.c_int32)), _dp(out4), _dp(W),
                               _dp(Bn))
    if rc < 0:
        raise McmcError(L.mcmcx_last_error().decode())
    return {"mpsrf": out4[0], "lambda1": out4[1], "M": out4[2], "n_h": out4[3], "W": W, "Bn": Bn, "warn": int(rc)}      # symmetric


QUANT_MAXR = 32


def _lp(a):
    return a.ctypes.data_as(C.POINTER(C.c_int64))


def _i64(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.int64))


def samples_quantile_ranks(n, probs):
    """(ranks[nq][2], frac[nq]) of the quantiles at `probs` among n values (Hyndman-Fan type 7: pos = p (n - 1), lo = floor(pos),
    hi = min(lo + 1, n - 1), g = pos - lo): mcmcx_samples_quantile_ranks, pure host arithmetic, no engine and no device."""
    L = _lib.load()
    p = _f64(probs).ravel()
    ranks, frac = np.zeros((p.size, 2), dtype=np.int64), np.zeros(p.size)
    if L.mcmcx_samples_quantile_ranks(int(n), int(p.size), _dp(p), _lp(ranks), _dp(frac)) < 0:
        raise McmcError(L.mcmcx_last_error().decode())
    return ranks, frac


HIST_MAXBINS, HIST2_MAXBINS, HIST2_MAXPAIRS = 1024, 96, 64


def samples_hist_edges(lo, hi, nbins):
    """nbins + 1 uniform edges of one field, e_i = lo + (hi - lo) * (i / nbins) and e_nbins = hi: mcmcx_samples_hist_edges, pure host
    arithmetic, no engine and no device."""
    L = _lib.load()
    e = np.zeros(max(int(nbins), 0) + 1)
    if L.mcmcx_samples_hist_edges(float(lo), float(hi), int(nbins), _dp(e)) < 0:
        raise McmcError(L.mcmcx_last_error().decode())
    return e


def samples_hist_density(counts, edges):
    """[nfields][nbins] densities from 1-D counts[nfields][nbins + 2] (one engine's, or the sum of several engines') and their
    edges[nfields][nbins + 1]: count_b / (n (e_b - e_{b-1})), n the sum of the field's cells, the two outer cells included --
    mcmcx_samples_hist_density, pure host arithmetic, no engine and no device."""
    L = _lib.load()
    c, e = _i64(counts), _f64(edges)
    if c.ndim != 2 or e.ndim != 2 or c.shape[0] != e.shape[0] or c.shape[1] != e.shape[1] + 1 or e.shape[1] < 2:
        raise McmcError("samples_hist_density: counts must be [nfields][nbins + 2] and edges [nfields][nbins + 1], got %s and %s"
                        % (c.shape, e.shape))
    d = np.zeros((c.shape[0], e.shape[1] - 1))
    if L.mcmcx_samples_hist_density(_lp(c), _dp(e), int(c.shape[0]), int(e.shape[1] - 1), _dp(d)) < 0:
        raise McmcError(L.mcmcx_last_error().decode())
    return d


STEP_MAXBINS = 510                                              # Engine.samples_stats_step's bin count (MCMCX_STEP_MAXBINS)


def samples_rank_scores(counts):
    """[nfields][nbins + 2] normal scores from 1-D counts[nfields][nbins + 2] (samples_hist: one engine's, or the sum of several
    engines'): a cell with count_b > 0 gets Phi^-1(((2 before_b + count_b + 1) / 2 - 3/8) / (n + 1/4)), the score of the average rank
    of its values in Blom's form (Phi^-1: Wichura's AS241, PPND16), an empty cell +0.0 -- mcmcx_samples_rank_scores, pure host
    arithmetic, no engine and no device.  With the counts' edges it is the table of `Engine.samples_stats_step` for the rank-normalised
    split-R-hat and bulk ESS."""
    L = _lib.load()
    c = _i64(counts)
    if c.ndim != 2 or c.shape[1] < 3:
        raise McmcError("samples_rank_scores: counts must be [nfields][nbins + 2], got %s" % (c.shape,))
    out = np.zeros(c.shape)
    if L.mcmcx_samples_rank_scores(_lp(c), int(c.shape[0]), int(c.shape[1] - 2), _dp(out)) < 0:
        raise McmcError(L.mcmcx_last_error().decode())
    return out


def samples_fold_scores(counts, edges, centre):
    """The step table of the rank-normalised FOLDED values |x - centre[f]| over the cells of x: cell b of field f stands at
    c_0 = e_0, c_b = (e_{b-1} + e_b) / 2 (1 <= b <= nbins), c_{nbins+1} = e_nbins; d_b = |c_b - centre[f]|; cells of equal d_b form one
    group, the groups in ascending order of d_b (np.unique) are ranked with their summed counts as samples_rank_scores ranks cells, and a
    cell gets its group's score.  counts[nfields][nbins + 2], edges[nfields][nbins + 1], centre[nfields] -> [nfields][nbins + 2]."""
    c, e, m = _i64(counts), _f64(edges), _f64(centre).ravel()
    if c.ndim != 2 or e.ndim != 2 or c.shape[0] != e.shape[0] or c.shape[1] != e.shape[1] + 1 or e.shape[1] < 2 or m.size != c.shape[0]:
        raise McmcError("samples_fold_scores: counts must be [nfields][nbins + 2], edges [nfields][nbins + 1] and centre [nfields], "
                        "got %s, %s and %s" % (c.shape, e.shape, m.shape))
    out = np.zeros(c.shape)
    with np.errstate(all="ignore"):
        for f in range(c.shape[0]):
            pos = np.concatenate([e[f, :1], (e[f, :-1] + e[f, 1:]) * 0.5, e[f, -1:]])
            uniq, inv = np.unique(np.fabs(pos - m[f]), return_inverse=True)
            group = np.zeros(max(uniq.size, 3), dtype=np.int64)          # a bin count of 1 at least; an empty group changes nothing
            np.add.at(group, inv, c[f])
            out[f] = samples_rank_scores(group[None, :])[0][inv]
    return out


def sample_field_names(npar, nycol=1):
    """Names of a sample's fields, in the store's order."""
    ny = int(nycol)
    return (["theta[%d]" % i for i in range(int(npar))] + (["ss"] if ny == 1 else ["ss[%d]" % j for j in range(ny)]) + ["sspri"]
            + (["sigma2"] if ny == 1 else ["sigma2[%d]" % j for j in range(ny)]))


class Comm:
    """The node's communicator (include/mcmcx.h, "several GPUs of one node"): one process per GPU, RCCL underneath
    (backend "rccl"), or the host-staged transport for ranks that share one GPU (backend "host")."""
    BACKENDS = {"rccl": 0, "host": 1}

    def __init__(self, key, rank, nranks, device, backend="rccl"):
        self.L = _lib.load()
        self.h = C.c_void_p()
        rc = self.L.mcmcx_comm_create(str(key).encode(), int(rank), int(nranks), int(device), self.BACKENDS[backend], C.byref(self.h))
        if rc < 0:
            raise McmcError(self.L.mcmcx_last_error().decode())
        self.rank, self.size = int(rank), int(nranks)

    def _chk(self, rc):
        if rc < 0:
            raise McmcError(self.L.mcmcx_last_error().decode())

    def barrier(self):
        self._chk(self.L.mcmcx_comm_barrier(self.h))

    def allreduce(self, values, op="sum"):
        """Sum / maximum of a few host doubles over the ranks."""
        a = np.ascontiguousarray(np.atleast_1d(values), dtype=np.float64).copy()
        self._chk(self.L.mcmcx_comm_allreduce_host(self.h, _dp(a), a.size, 1 if op == "max" else 0))
        return a

    def close(self):
        if self.h:
            self.L.mcmcx_comm_destroy(self.h)
            self.h = C.c_void_p()


class Engine:
    def __init__(self, cfg):
        self.L = _lib.load()
        self.cfg = cfg
        self.h = C.c_void_p()
        self._chk(self.L.mcmcx_create(C.byref(cfg), C.byref(self.h)))
        self.npar, self.nchains, self.nsimu = cfg.npar, cfg.nchains, cfg.nsimu

    def _chk(self, rc):
        if rc < 0:
            raise McmcError(self.L.mcmcx_last_error().decode())
        return rc

    def close(self):
        if self.h:
            self.L.mcmcx_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # --- MCMC_setpar0 / MCMC_setcmat0 / MCMC_setsigma2nobs
    def setpar0(self, par0):
        a = _f64(par0)
        self._chk(self.L.mcmcx_set_par0(self.h, _dp(a), a.size))

    def setpar0_all(self, par0_all):
        """Every chain its own start point: par0_all[nchains, npar] (mcmcx_set_par0_all).  Before init; setpar0 is still required."""
        a = np.ascontiguousarray(np.asarray(par0_all, dtype=np.float64))
        if a.ndim != 2:
            raise McmcError("setpar0_all: par0_all must be [nchains][npar]")
        self._chk(self.L.mcmcx_set_par0_all(self.h, _dp(a), a.shape[0], a.shape[1]))

    def setpar0_spread(self, scale=1.0):
        """Start points drawn on the device at init, par0 + scale U0'z per chain (mcmcx_set_par0_spread; tests/start_ref.py restates the
        draw).  scale = 1: one draw of the initial proposal; sqrt(npar) / 2.4: N(par0, cmat0)."""
        self._chk(self.L.mcmcx_set_par0_spread(self.h, float(scale)))

    def start_info(self):
        """After init: how the chains were started (mcmcx_start_info)."""
        a = np.zeros(3, dtype=np.int64)
        self._chk(self.L.mcmcx_start_info(self.h, a.ctypes.data_as(C.POINTER(C.c_int64))))
        return dict(mode=("shared", "given", "spread")[int(a[0])], redrew=int(a[1]), fell_back=int(a[2]))

    def setcmat0(self, cmat0):
        a = np.asfortranarray(np.asarray(cmat0, dtype=np.float64))
        self._chk(self.L.mcmcx_set_cmat0(self.h, a.ctypes.data_as(C.POINTER(C.c_double)), a.shape[0]))

    def setsigma2nobs(self, sigma2, nobs):
        """Scalars, or vectors of length nycol (one error variance per response column of ssfunction)."""
        s = _f64(np.atleast_1d(sigma2)); n = np.ascontiguousarray(np.atleast_1d(nobs), dtype=np.int32)
        assert len(s) == len(n)
        self.nycol = len(s)
        self._chk(self.L.mcmcx_set_sigma2nobs(self.h, _dp(s), n.ctypes.data_as(C.POINTER(C.c_int32)), len(s)))

    # --- the device-resident user callbacks
    def set_target(self, kind, mu=None, lam=None, b=0.1, xdata=None, ydata=None):
        if kind == "gauss":
            self._chk(self.L.mcmcx_set_target_gauss(self.h, _dp(_f64(mu)), _dp(_f64(lam))))
        elif kind == "banana":
            self._chk(self.L.mcmcx_set_target_banana(self.h, float(b)))
        elif kind == "expdata":
            x, y = _f64(xdata), np.ascontiguousarray(np.asarray(ydata, dtype=np.float64))
            if y.ndim == 2:                                   # response columns: y[nycol][ndata]
                self._chk(self.L.mcmcx_set_target_expdata_cols(self.h, x.size, y.shape[0], _dp(x), _dp(y.ravel())))
            else:
                self._chk(self.L.mcmcx_set_target_expdata(self.h, x.size, _dp(x), _dp(y)))
        else:
            raise KeyError(kind)

    def set_target_all(self, xdata, ydata):
        """Many fits in one run (mcmcx_set_target_expdata_all): the "expdata" model with a data set per chain.  ydata is
        (nchains, nycol, ndata), or (nchains, ndata) for one column; xdata is (ndata,), shared, or (nchains, ndata).  Before init."""
        x, y, nycol, x_per_chain = chain_data_arrays(self.nchains, self.npar, xdata, ydata)
        self._chk(self.L.mcmcx_set_target_expdata_all(self.h, y.shape[0], y.shape[2], nycol, _dp(x), x_per_chain, _dp(y)))

    def chain_data_info(self):
        """After init: whose data the chains fit (mcmcx_chain_data_info); `bytes` are the per-chain device tables'."""
        a = np.zeros(4, dtype=np.int64)
        self._chk(self.L.mcmcx_chain_data_info(self.h, a.ctypes.data_as(C.POINTER(C.c_int64))))
        return dict(mode=("shared", "y_per_chain", "xy_per_chain")[int(a[0])], ndata=int(a[1]), nycol=int(a[2]), bytes=int(a[3]))

    def set_target_host(self, ssfun, priorfun=None, checkbounds=None, ssfun_er=None):
        """User callbacks on the host, like the reference's link-time ssfunction / priorfun / checkbounds:
        ssfun(theta) -> float, priorfun(theta) -> float, checkbounds(theta) -> bool, theta a numpy vector;
        ssfun_er(theta, sscrit) -> float is the early-rejection form used by method='er' (default: ssfun)."""
        n = self.npar

        def _ss(th, npar, ny, out, user):
            v = np.atleast_1d(ssfun(np.ctypeslib.as_array(th, shape=(n,)).copy()))
            for j in range(ny):
                out[j] = float(v[j])

        def _pri(th, npar, user):
            return float(priorfun(np.ctypeslib.as_array(th, shape=(n,)).copy()))

        def _cb(th, npar, user):
            return 1 if checkbounds(np.ctypeslib.as_array(th, shape=(n,)).copy()) else 0

        self._cb_keep = (_lib.SSFUN_T(_ss), _lib.PRIORFUN_T(_pri) if priorfun else _lib.PRIORFUN_T(),
                         _lib.CHECKBOUNDS_T(_cb) if checkbounds else _lib.CHECKBOUNDS_T())
        self._chk(self.L.mcmcx_set_target_host(self.h, self._cb_keep[0], self._cb_keep[1], self._cb_keep[2], None))
        if ssfun_er is not None:
            def _ss_er(th, npar, ny, crit, out, user):
                v = np.atleast_1d(ssfun_er(np.ctypeslib.as_array(th, shape=(n,)).copy(), crit))
                for j in range(ny):
                    out[j] = float(v[j])
            self._er_keep = _lib.SSFUN_ER_T(_ss_er)
            self._chk(self.L.mcmcx_set_target_host_er(self.h, self._er_keep))

    def set_target_host_batch(self, ssfun_batch, priorfun=None, checkbounds=None, nthreads=1):
        """Batched user callback: ssfun_batch(theta[n, npar]) -> ss[n] or ss[n, ny], called once per stage (or from
        `nthreads` threads on disjoint slices)."""
        n = self.npar

        def _ssb(th, npar, nb, ny, out, user):
            a = np.ctypeslib.as_array(th, shape=(nb, n)).copy()
            v = np.asarray(ssfun_batch(a), dtype=np.float64).reshape(nb, ny)
            np.ctypeslib.as_array(out, shape=(nb, ny))[:, :] = v

        def _pri(th, npar, user):
            return float(priorfun(np.ctypeslib.as_array(th, shape=(n,)).copy()))

        def _cb(th, npar, user):
            return 1 if checkbounds(np.ctypeslib.as_array(th, shape=(n,)).copy()) else 0

        self._cbb_keep = (_lib.SSFUN_BATCH_T(_ssb), _lib.PRIORFUN_T(_pri) if priorfun else _lib.PRIORFUN_T(),
                          _lib.CHECKBOUNDS_T(_cb) if checkbounds else _lib.CHECKBOUNDS_T())
        self._chk(self.L.mcmcx_set_target_host_batch(self.h, self._cbb_keep[0], self._cbb_keep[1], self._cbb_keep[2], None, int(nthreads)))

    def set_target_module(self, code_object, kernel_name, userdata=None):
        """The user's ssfunction / priorfun / checkbounds as device code (include/mcmcx_target.h): `code_object` is the
        hipcc --genco output, userdata a bytes-like object or a float64 array copied to the device."""
        buf = None if userdata is None else np.ascontiguousarray(userdata)
        self._chk(self.L.mcmcx_set_target_module(self.h, str(code_object).encode(), str(kernel_name).encode(),
                                                 None if buf is None else buf.ctypes.data_as(C.c_void_p), 0 if buf is None else buf.nbytes))

    def set_bounds(self, lo=None, hi=None):
        lo = _f64(lo) if lo is not None else None
        hi = _f64(hi) if hi is not None else None
        self._chk(self.L.mcmcx_set_bounds(self.h, _dp(lo), _dp(hi)))

    def set_priors(self, mu, sig):
        self._chk(self.L.mcmcx_set_priors(self.h, _dp(_f64(mu)), _dp(_f64(sig))))

    # --- mcmc_main_one: MCMC_run1 / MCMC_run1_er, the arithmetic of one invocation (MCMC_run1.F90:131-199); all chains at once
    def set_target_external(self):
        """Every evaluation of ssfunction / priorfun / checkbounds is the caller's: init evaluates nothing, run refuses."""
        self._chk(self.L.mcmcx_set_target_external(self.h))

    def _rows(self, a, k):
        return None if a is None else np.ascontiguousarray(np.broadcast_to(np.asarray(a, dtype=np.float64).reshape(-1, k), (self.nchains, k)))

    def run1_decide(self, drstage, oldpar1, ssprev1, sspri1, newpar, ss, sspri, oldpar2=None, ssprev2=None, sspri2=None, alpha12=None):
        """(alpha[nchains], reject[nchains]): MCMC_alpha(oldpar1 -> newpar) in stage 1, MCMC_DR_alpha13(oldpar2, oldpar1, newpar)
        in stage 2 with drscale > 0, then MCMC_reject.  Vectors [nchains][npar] / [nchains][nycol] / [nchains] (or one row for all)."""
        n, ny = self.npar, getattr(self, "nycol", 1)
        A = [self._rows(oldpar2, n), self._rows(ssprev2, ny), self._rows(sspri2, 1), self._rows(oldpar1, n), self._rows(ssprev1, ny),
             self._rows(sspri1, 1), self._rows(alpha12, 1), self._rows(newpar, n), self._rows(ss, ny), self._rows(sspri, 1)]
        alpha = np.zeros(self.nchains); rej = np.zeros(self.nchains, dtype=np.int32)
        self._chk(self.L.mcmcx_run1_decide(self.h, int(drstage), *[_dp(a) for a in A], _dp(alpha), rej.ctypes.data_as(C.POINTER(C.c_int32))))
        return alpha, rej.astype(bool)

    def run1_propose(self, stage, from_):
        out = np.zeros((self.nchains, self.npar))
        self._chk(self.L.mcmcx_run1_propose(self.h, int(stage), _dp(self._rows(from_, self.npar)), _dp(out)))
        return out

    def run1_sscrit(self, ssprev1, sspri1):
        out = np.zeros(self.nchains)
        self._chk(self.L.mcmcx_run1_sscrit(self.h, _dp(self._rows(ssprev1, getattr(self, "nycol", 1))), _dp(self._rows(sspri1, 1)), _dp(out)))
        return out

    # --- mcmc_main
    def set_stream(self, hip_stream):
        """Run on the caller's HIP stream (e.g. torch.cuda.Stream().cuda_stream) instead of the engine's own; before init."""
        self._chk(self.L.mcmcx_set_stream(self.h, C.c_void_p(int(hip_stream))))

    def init(self):
        self._chk(self.L.mcmcx_init(self.h))

    def run(self, upto=None):
        """Returns 0, or 2 (MCMCX_INTERRUPTED) when a caught signal ended the run early (see mcmcx_run)."""
        return self._chk(self.L.mcmcx_run(self.h, self.nsimu if upto is None else int(upto)))

    def sync(self):
        self._chk(self.L.mcmcx_sync(self.h))

    @property
    def simuind(self):
        return self.L.mcmcx_simuind(self.h)

    # --- results
    def counters(self, chain=0):
        a = np.zeros(8, dtype=np.int32)
        self._chk(self.L.mcmcx_get_counters(self.h, chain, a.ctypes.data_as(C.POINTER(C.c_int32))))
        return dict(stayed=int(a[0]), bndstayed=int(a[1]), draccepted=int(a[2]), drtries=int(a[3]),
                    chainind=int(a[4]), status=int(a[5]), erstayed=int(a[6]), curcount=int(a[7]))

    def totals(self):
        a = np.zeros(7, dtype=np.int64)
        self._chk(self.L.mcmcx_get_totals_n(self.h, a.ctypes.data_as(C.POINTER(C.c_int64)), a.size))
        return dict(stayed=int(a[0]), bndstayed=int(a[1]), draccepted=int(a[2]), drtries=int(a[3]), proposals=int(a[4]),
                    downdates=int(a[5]), status=int(a[6]))

    def theta(self):
        a = np.zeros((self.nchains, self.npar))
        self._chk(self.L.mcmcx_get_theta(self.h, _dp(a)))
        return a

    def scalars(self):
        a = np.zeros((self.nchains, 4))
        self._chk(self.L.mcmcx_get_scalars(self.h, _dp(a)))
        return a          # ss1, sspri1, sigma2, alpha12

    def rng(self, chain=0):
        n, s, y = C.c_uint64(), C.c_int32(), C.c_double()
        self._chk(self.L.mcmcx_get_rng(self.h, chain, C.byref(n), C.byref(s), C.byref(y)))
        return n.value, s.value, y.value

    def R(self, chain=0):
        a = np.zeros((self.npar, self.npar), order="F")
        self._chk(self.L.mcmcx_get_R(self.h, chain, a.ctypes.data_as(C.POINTER(C.c_double))))
        return np.array(a)

    def qcovstd(self, chain=0):
        a = np.zeros(self.npar)
        self._chk(self.L.mcmcx_get_qcovstd(self.h, chain, _dp(a)))
        return a

    def dr_state(self, chain=0):
        r2 = np.zeros((self.npar, self.npar), order="F"); ic = np.zeros((self.npar, self.npar), order="F")
        dp = C.POINTER(C.c_double)
        self._chk(self.L.mcmcx_get_dr(self.h, chain, r2.ctypes.data_as(dp), ic.ctypes.data_as(dp)))
        return np.array(r2), np.array(ic)

    def chaincov(self, chain=0):
        a = np.zeros((self.npar, self.npar), order="F"); m = np.zeros(self.npar); w = C.c_double()
        self._chk(self.L.mcmcx_get_chaincov(self.h, chain, a.ctypes.data_as(C.POINTER(C.c_double)), _dp(m), C.byref(w)))
        return np.array(a), m, w.value

    def debug_calculate_R(self, cmat, need=None):
        """Test probe (mcmcx_debug_calculate_R): the tick's own factorisation on the covariances cmat[nchains, npar, npar] (symmetric), in
        the instances this engine's plan chose.  Returns (info[nchains] -- INFO_SENTINEL where need == 0 --, forms); R, R2, iC, the status
        and the covariance are read with R(), dr_state(), counters(), chaincov().  Raises McmcError on a refusal (-57)."""
        a = np.ascontiguousarray(np.swapaxes(np.asarray(cmat, dtype=np.float64), 1, 2))
        assert a.shape == (self.nchains, self.npar, self.npar), a.shape
        nd = None if need is None else np.ascontiguousarray(np.asarray(need, dtype=np.uint8))
        info = np.zeros(self.nchains, dtype=np.int32)
        buf = C.create_string_buffer(256)
        self._chk(self.L.mcmcx_debug_calculate_R(self.h, _dp(a), None if nd is None else nd.ctypes.data_as(C.POINTER(C.c_uint8)),
                                                 info.ctypes.data_as(C.POINTER(C.c_int32)), buf, 256))
        return info, buf.value.decode()

    def accepted(self, chain=0):
        a = np.zeros(self.simuind, dtype=np.uint8)
        self._chk(self.L.mcmcx_get_accepted(self.h, chain, a.ctypes.data_as(C.POINTER(C.c_uint8))))
        return a

    def accept_masks(self):
        nt = C.c_int32()
        self._chk(self.L.mcmcx_get_accept_masks(self.h, None, C.byref(nt)))
        a = np.zeros((self.simuind, nt.value), dtype=np.uint64)
        self._chk(self.L.mcmcx_get_accept_masks(self.h, a.ctypes.data_as(C.POINTER(C.c_uint64)), C.byref(nt)))
        return a

    def chain(self, chain=0):
        n, ny = self.simuind, getattr(self, "nycol", 1)
        ch = np.zeros((n, self.npar + 1)); ss = np.zeros((n, ny + 1)); s2 = np.zeros((n, ny)); nr = C.c_int32()
        self._chk(self.L.mcmcx_get_chain(self.h, chain, _dp(ch), _dp(ss), _dp(s2), C.byref(nr)))
        return ch[:nr.value], ss[:nr.value], (s2[:, 0] if ny == 1 else s2)

    # --- thinned samples of all chains, kept on the device (mcmcx_set_samples)
    def set_samples(self, first=1, thin=1, capacity=None):
        """Keep iteration i when i >= first and (i - first) % thin == 0, in a ring of `capacity` samples (None: as many as the rule
        keeps up to nsimu); thin = 0 switches sampling off.  Before init."""
        if capacity is None:
            capacity = max(1, len(sample_iterations(first, thin, self.nsimu + 1, self.nsimu))) if thin > 0 else 0
        self._chk(self.L.mcmcx_set_samples(self.h, int(first), int(thin), int(capacity)))

    def samples_kept(self):
        """(n, oldest_iteration, thin, nfields): retained sample s (0 = oldest) is iteration oldest_iteration + s * thin."""
        o, t, f = C.c_int32(), C.c_int32(), C.c_int32()
        n = self.L.mcmcx_samples_kept(self.h, C.byref(o), C.byref(t), C.byref(f))
        return int(n), o.value, t.value, f.value

    def _window(self, s0, ns):
        """(ns, oldest_iteration, thin, nfields) of a reader's window; ns = None: every retained sample from s0 on."""
        n, oldest, thin, nf = self.samples_kept()
        return (n - s0 if ns is None else int(ns)), oldest, thin, nf

    def _shift(self, shift, nf, who):
        """shift as a contiguous array of nfields values, or None"""
        if shift is None:
            return None
        sh = _f64(shift)
        if sh.size != nf:
            raise McmcError("%s: shift has %d values, a sample has %d fields" % (who, sh.size, nf))
        return sh

    def _dev(self, shape, call):
        """A tensor on the engine's device filled by the asynchronous form `call(pointer)` of a getter, synchronised."""
        import torch
        t = torch.empty(shape, dtype=torch.float64, device="cuda:%d" % self.cfg.device)
        self._chk(call(C.c_void_p(t.data_ptr())))
        self.sync()
        return t

    def _sample_shape(self, s0, ns, c0, nc, layout):
        """(ns, nc, iterations[ns], shape) of what samples / samples_torch return"""
        ns, oldest, thin, nf = self._window(s0, ns)
        nc = self.nchains - c0 if nc is None else int(nc)
        its = np.array([oldest + (s0 + j) * thin for j in range(max(ns, 0))], dtype=np.int64)
        shape = (ns, nc, nf) if layout == 0 else (ns, nf, nc)
        return ns, nc, its, shape

    def samples(self, s0=0, ns=None, c0=0, nc=None, layout=0):
        """(iterations[ns], array): retained samples s0 .. s0 + ns - 1 of chains c0 .. c0 + nc - 1 as [ns][nc][nfields] (layout 0) or
        [ns][nfields][nc] (layout 1); the fields of a chain are theta, ss per column, sspri, sigma2 per column."""
        ns, nc, its, shape = self._sample_shape(s0, ns, c0, nc, layout)
        a = np.zeros(shape)
        if ns == 0 or nc == 0:
            return its, a
        self._chk(self.L.mcmcx_get_samples(self.h, int(s0), ns, int(c0), nc, int(layout), _dp(a)))
        return its, a

    def samples_torch(self, s0=0, ns=None, c0=0, nc=None, layout=0):
        """The same window as a float64 torch tensor on the engine's device: the copy never leaves device memory."""
        ns, nc, its, shape = self._sample_shape(s0, ns, c0, nc, layout)
        if ns == 0 or nc == 0:
            import torch
            return its, torch.empty(shape, dtype=torch.float64, device="cuda:%d" % self.cfg.device)
        return its, self._dev(shape, lambda p: self.L.mcmcx_get_samples_dev(self.h, int(s0), ns, int(c0), nc, int(layout), p))

    # --- convergence summary of the retained samples, reduced on the device (mcmcx_samples_stats)
    def samples_stats(self, s0=0, ns=None, maxlag=16, shift=None):
        """The stats vector of retained samples s0 .. s0 + ns - 1 of all chains (include/mcmcx.h has the definition): additive over engines
        that were given the same `shift`; `samples_diag` finishes it."""
        ns, _, _, nf = self._window(s0, ns)
        sh = self._shift(shift, nf, "samples_stats")
        a = np.zeros(self._chk(self.L.mcmcx_samples_stats_len(self.h, int(maxlag))))
        self._chk(self.L.mcmcx_samples_stats(self.h, int(s0), ns, int(maxlag), _dp(sh), _dp(a)))
        return a

    def samples_stats_torch(self, s0=0, ns=None, maxlag=16, shift=None):
        """The same vector as a float64 torch tensor on the engine's device, filled by the asynchronous form and synchronised."""
        ns, _, _, nf = self._window(s0, ns)
        sh = self._shift(shift, nf, "samples_stats_torch")
        return self._dev(self._chk(self.L.mcmcx_samples_stats_len(self.h, int(maxlag))),
                         lambda p: self.L.mcmcx_samples_stats_dev(self.h, int(s0), ns, int(maxlag), _dp(sh), p))

    # --- the summary of an elementwise function of the retained samples (mcmcx_samples_stats_of)
    def _stats_of_args(self, kind, a, s0, ns, shift, who):
        """(ns, a, shift) of a transformed summary: a and shift as contiguous arrays of nfields values, or None"""
        ns, _, _, nf = self._window(s0, ns)
        av = None if a is None else _f64(a)
        if av is not None and av.size != nf:
            raise McmcError("%s: a has %d values, a sample has %d fields" % (who, av.size, nf))
        return ns, av, self._shift(shift, nf, who)

    def samples_stats_of(self, kind, a=None, s0=0, ns=None, maxlag=16, shift=None):
        """The stats vector `samples_stats` would return if every stored value x of field f were u_f(x): kind XF_IDENTITY x (a is not
        looked at), XF_LE 1.0 where key(x) <= key(a[f]) else 0.0 (the order of samples_counts' le), XF_FOLD |x - a[f]|,
        XF_SQUARE (x - a[f])^2.  shift = None: u_f of chain 0 in window sample 0.  `samples_diag` finishes it; additive over engines
        that were given the same kind, a and shift."""
        ns, av, sh = self._stats_of_args(kind, a, s0, ns, shift, "samples_stats_of")
        out = np.zeros(self._chk(self.L.mcmcx_samples_stats_len(self.h, int(maxlag))))
        self._chk(self.L.mcmcx_samples_stats_of(self.h, int(s0), ns, int(maxlag), int(kind), _dp(av), _dp(sh), _dp(out)))
        return out

    def samples_stats_of_torch(self, kind, a=None, s0=0, ns=None, maxlag=16, shift=None):
        """The same vector as a float64 torch tensor on the engine's device, filled by the asynchronous form and synchronised."""
        ns, av, sh = self._stats_of_args(kind, a, s0, ns, shift, "samples_stats_of_torch")
        return self._dev(self._chk(self.L.mcmcx_samples_stats_len(self.h, int(maxlag))),
                         lambda p: self.L.mcmcx_samples_stats_of_dev(self.h, int(s0), ns, int(maxlag), int(kind), _dp(av), _dp(sh), p))

    # --- the summary of a step function of the retained samples (mcmcx_samples_stats_step)
    def _stats_step_args(self, edges, table, s0, ns, shift, who):
        """(ns, edges[nfields][nbins + 1], table[nfields][nbins + 2], shift) of a step summary"""
        ns, _, _, nf = self._window(s0, ns)
        ed, tb = _f64(edges), _f64(table)
        if ed.ndim != 2 or ed.shape[0] != nf or ed.shape[1] < 2 or tb.shape != (nf, ed.shape[1] + 1):
            raise McmcError("%s: edges must be [nfields = %d][nbins + 1] and table [nfields][nbins + 2], got %s and %s"
                            % (who, nf, ed.shape, tb.shape))
        return ns, ed, tb, self._shift(shift, nf, who)

    def samples_stats_step(self, edges, table, s0=0, ns=None, maxlag=16, shift=None):
        """The stats vector `samples_stats` would return if every stored value x of field f were table[f][cell_f(x)], cell_f(x) the
        cell of `samples_hist` among edges[f] (the number of edges whose key is not above x's, 0 .. nbins + 1; at most STEP_MAXBINS
        bins).  shift = None: u_f of chain 0 in window sample 0.  `samples_diag` finishes it; additive over engines that were given the
        same edges, table and shift.  With edges at order statistics and `samples_rank_scores` of their counts as the table it is the
        rank-normalised summary; with a table of zeros and ones the summary of an interval's indicator."""
        ns, ed, tb, sh = self._stats_step_args(edges, table, s0, ns, shift, "samples_stats_step")
        out = np.zeros(self._chk(self.L.mcmcx_samples_stats_len(self.h, int(maxlag))))
        self._chk(self.L.mcmcx_samples_stats_step(self.h, int(s0), ns, int(maxlag), int(ed.shape[1] - 1), _dp(ed), _dp(tb), _dp(sh),
                                                  _dp(out)))
        return out

    def samples_stats_step_torch(self, edges, table, s0=0, ns=None, maxlag=16, shift=None):
        """The same vector as a float64 torch tensor on the engine's device, filled by the asynchronous form and synchronised."""
        ns, ed, tb, sh = self._stats_step_args(edges, table, s0, ns, shift, "samples_stats_step_torch")
        return self._dev(self._chk(self.L.mcmcx_samples_stats_len(self.h, int(maxlag))),
                         lambda p: self.L.mcmcx_samples_stats_step_dev(self.h, int(s0), ns, int(maxlag), int(ed.shape[1] - 1), _dp(ed),
                                                                       _dp(tb), _dp(sh), p))

    def samples_rank_edges(self, rank_cells=128, s0=0, ns=None):
        """edges[nfields][rank_cells - 1] that cut the window's n = ns x nchains values of every field into rank_cells cells of (nearly)
        equal counts: the order statistics at the 0-based ranks (k n) // rank_cells, k = 1 .. rank_cells - 1, in
        ceil((rank_cells - 1) / QUANT_MAXR) calls of samples_order_stats."""
        ns, _, _, nf = self._window(s0, ns)
        B = int(rank_cells)
        if B < 3 or B > STEP_MAXBINS + 2:
            raise McmcError("samples_rank_edges: rank_cells must lie in 3 .. %d, got %d" % (STEP_MAXBINS + 2, B))
        ranks = [(k * ns * self.nchains) // B for k in range(1, B)]
        return np.concatenate([self.samples_order_stats(ranks[i:i + QUANT_MAXR], s0, ns) for i in range(0, B - 1, QUANT_MAXR)], axis=1)

    # --- exact order statistics, tail counts and quantiles of the retained samples (mcmcx_samples_order_stats)
    def samples_order_stats(self, ranks, s0=0, ns=None):
        """[nfields][nr]: the values whose keys are the ranks[k]-th smallest (0-based) among the ns x nchains values of each field in
        retained samples s0 .. s0 + ns - 1 (include/mcmcx.h has the key order: -0.0 below +0.0, NaNs at the two ends)."""
        ns, _, _, nf = self._window(s0, ns)
        r = _i64(ranks).ravel()
        a = np.zeros((nf, r.size))
        self._chk(self.L.mcmcx_samples_order_stats(self.h, int(s0), ns, int(r.size), _lp(r), _dp(a)))
        return a

    def samples_order_stats_torch(self, ranks, s0=0, ns=None):
        """The same as a float64 torch tensor on the engine's device, filled by the asynchronous form and synchronised."""
        ns, _, _, nf = self._window(s0, ns)
        r = _i64(ranks).ravel()
        return self._dev((nf, r.size), lambda p: self.L.mcmcx_samples_order_stats_dev(self.h, int(s0), ns, int(r.size), _lp(r), p))

    def samples_counts(self, x, s0=0, ns=None):
        """int64 [nfields][nq][2]: how many window values of field f have a key below (lt) and not above (le) that of x[f][q].  Exact
        and additive over engines that hold disjoint chains."""
        ns, _, _, nf = self._window(s0, ns)
        xs = _f64(x)
        if xs.ndim != 2 or xs.shape[0] != nf:
            raise McmcError("samples_counts: x must be [nfields = %d][nq], got %s" % (nf, xs.shape))
        a = np.zeros((nf, xs.shape[1], 2), dtype=np.int64)
        self._chk(self.L.mcmcx_samples_counts(self.h, int(s0), ns, int(xs.shape[1]), _dp(xs), _lp(a)))
        return a

    def samples_quantiles(self, probs, s0=0, ns=None):
        """[nfields][nq]: the quantiles at `probs` (numpy's default, linear interpolation between two order statistics) of every
        field over the window; at most QUANT_MAXR / 2 probabilities per call."""
        ns, _, _, nf = self._window(s0, ns)
        p = _f64(probs).ravel()
        a = np.zeros((nf, p.size))
        self._chk(self.L.mcmcx_samples_quantiles(self.h, int(s0), ns, int(p.size), _dp(p), _dp(a)))
        return a

    def samples_summary(self, s0=0, ns=None, maxlag=16, shift=None, probs=None, tail=False, rank=False, rank_cells=128, multivariate=False):
        """dict of arrays over the fields: mean, sd, rhat, ess, mcse, W, Bn, truncated; `fields` names the rows, `iterations` are the
        window's.  truncated = 1: the lag window ended before the autocorrelation did, ess is an upper bound.  With `probs` also the
        keys `probs` and `quantiles` ([nfields][nq], samples_quantiles of the same window).

        tail=True adds the diagnostics of the intervals and of the sd, each a summary of an elementwise function of the samples
        (samples_stats_of) at the same maxlag, with q05, q50, q95 from samples_quantiles of the same window:
          ess_tail        the smaller ess of the indicators x <= q05 and x <= q95 (XF_LE, a shift of zeros); NaN if either is
          truncated_tail  the larger of their two `truncated` flags
          rhat_folded     rhat of |x - q50| (XF_FOLD): chains that agree in location and differ in scale show here, not in rhat
          ess_sd, mcse_sd ess of (x - mean)^2 (XF_SQUARE at the table's mean), and its mcse / (2 sd): the delta method on the
                          variance, sd = sqrt(var) so d sd = d var / (2 sd)
          ess_quantiles   with `probs`, [nfields][nq]: the ess of the indicator x <= quantiles[f][q]; the MCSE of P(x <= q) is
                          sqrt(p (1 - p) / ess)
        An indicator that is constant over the window (a quantile at the window's extreme) gives NaN.  Cost on top of tail=False:
        4 + nq summary passes over the window and one quantile call.  `shift` applies to the plain table only.

        rank=True adds the rank-normalised diagnostics of Vehtari et al. (2021) -- Stan's and ArviZ's `Rhat` and `ess_bulk`, which
        mean something for a heavy-tailed field too, where rhat and ess above do not --, rank-normalised over rank_cells cells: every
        value is replaced by the normal score of the average rank of its cell (ties as the average-rank convention treats them; at 128
        cells within 5e-4 of the exact rank-normalised R-hat and 2.5 % of its ESS).  The recipe: edges = samples_rank_edges, counts =
        samples_hist, table = samples_rank_scores, then samples_stats_step with a shift of zeros at the same maxlag.
          rhat_rank       the rank-normalised split-R-hat
          ess_bulk_rank, truncated_rank   the rank-normalised bulk ESS and its `truncated` flag
          rhat_max        the larger of rhat_rank and the rank-normalised folded R-hat, the same summary with the table
                          samples_fold_scores at the window's median (samples_quantiles): the scores of |x - median| over the cells of x
        A field that is constant over the window falls into one cell and gives NaN.  Cost on top of rank=False:
        ceil((rank_cells - 1) / 32) order-statistics calls (a radix select each: eight passes over the window), one histogram pass,
        one quantile call and two summary passes (each reads the window twice, as every summary does).

        multivariate=True adds the joint diagnostics of the parameter block, at the table's mean as the shift (samples_mess and
        samples_mpsrf have the definitions):
          mess            the multivariate effective sample size of theta at batch = floor(sqrt(ns)); `mess_batch` is that batch
          ess_bm          [npar]: the univariate batch-means ESS of every parameter at the same batch
          mpsrf           the multivariate split-R-hat of theta: at least every parameter's rhat
        Cost on top of multivariate=False: four passes over the window (two covariances, two batch-means covariances)."""
        ns, oldest, thin, nf = self._window(s0, ns)
        table = samples_diag(self.samples_stats(s0, ns, maxlag, shift), nf, maxlag)
        out = {k: table[:, j].copy() for j, k in enumerate(DIAG_COLUMNS)}
        out["fields"] = sample_field_names(self.npar, getattr(self, "nycol", 1))
        out["iterations"] = oldest + (int(s0) + np.arange(max(ns, 0), dtype=np.int64)) * thin
        if probs is not None:
            out["probs"] = _f64(probs).ravel().copy()
            out["quantiles"] = self.samples_quantiles(out["probs"], s0, ns)
        if tail:
            def of(kind, a, sh=None):
                return samples_diag(self.samples_stats_of(kind, a, s0, ns, maxlag, sh), nf, maxlag)
            ESS, MCSE, RHAT, TRUNC = (DIAG_COLUMNS.index(k) for k in ("ess", "mcse", "rhat", "truncated"))
            zero = np.zeros(nf)
            q = self.samples_quantiles([0.05, 0.5, 0.95], s0, ns)
            lo, hi = of(XF_LE, q[:, 0], zero), of(XF_LE, q[:, 2], zero)
            out["ess_tail"] = np.minimum(lo[:, ESS], hi[:, ESS])
            out["truncated_tail"] = np.maximum(lo[:, TRUNC], hi[:, TRUNC])
            out["rhat_folded"] = of(XF_FOLD, q[:, 1])[:, RHAT].copy()
            sq = of(XF_SQUARE, out["mean"])
            out["ess_sd"] = sq[:, ESS].copy()
            out["mcse_sd"] = sq[:, MCSE] / (2.0 * out["sd"])
            if probs is not None:
                qs = out["quantiles"]
                out["ess_quantiles"] = np.stack([of(XF_LE, qs[:, k], zero)[:, ESS] for k in range(qs.shape[1])], axis=1)
        if rank:
            ESS, RHAT, TRUNC = (DIAG_COLUMNS.index(k) for k in ("ess", "rhat", "truncated"))
            zero = np.zeros(nf)
            edges = self.samples_rank_edges(rank_cells, s0, ns)
            counts = self.samples_hist(edges, s0, ns)
            r = samples_diag(self.samples_stats_step(edges, samples_rank_scores(counts), s0, ns, maxlag, zero), nf, maxlag)
            out["rhat_rank"], out["ess_bulk_rank"], out["truncated_rank"] = r[:, RHAT].copy(), r[:, ESS].copy(), r[:, TRUNC].copy()
            fold = samples_fold_scores(counts, edges, self.samples_quantiles([0.5], s0, ns)[:, 0])
            rf = samples_diag(self.samples_stats_step(edges, fold, s0, ns, maxlag, zero), nf, maxlag)
            out["rhat_max"] = np.maximum(out["rhat_rank"], rf[:, RHAT])
        if multivariate:
            m = self.samples_mess(s0, ns, None, "theta", out["mean"])
            out["mess"], out["mess_batch"], out["ess_bm"] = m["mess"], m["batch"], m["ess_bm"]
            out["mpsrf"] = self.samples_mpsrf(s0, ns, "theta", out["mean"])["mpsrf"]
        return out

    # --- marginal and pairwise joint histograms of the retained samples (mcmcx_samples_hist / _hist2)
    def _hist_args(self, s0, ns, edges, pairs, who):
        """(ns, nfields, edges[nfields][nbins + 1], pairs[npairs][2] or None) of a histogram call"""
        ns, _, _, nf = self._window(s0, ns)
        ed = _f64(edges)
        if ed.ndim != 2 or ed.shape[0] != nf or ed.shape[1] < 2:
            raise McmcError("%s: edges must be [nfields = %d][nbins + 1], got %s" % (who, nf, ed.shape))
        if pairs is None:
            return ns, nf, ed, None
        pr = np.ascontiguousarray(np.asarray(pairs, dtype=np.int32))
        if pr.ndim != 2 or pr.shape[1] != 2:
            raise McmcError("%s: pairs must be [npairs][2], got %s" % (who, pr.shape))
        return ns, nf, ed, pr

    def samples_hist(self, edges, s0=0, ns=None):
        """int64 [nfields][nbins + 2]: how many of the ns x nchains values of field f in retained samples s0 .. s0 + ns - 1 lie in each
        cell of edges[f] (include/mcmcx.h has the definition: cell 0 below the first edge, cell b = [e_{b-1}, e_b), cell nbins + 1 at or
        above the last).  Exact and additive over engines that hold disjoint chains; `samples_hist_density` finishes it."""
        ns, nf, ed, _ = self._hist_args(s0, ns, edges, None, "samples_hist")
        a = np.zeros((nf, ed.shape[1] + 1), dtype=np.int64)
        self._chk(self.L.mcmcx_samples_hist(self.h, int(s0), ns, int(ed.shape[1] - 1), _dp(ed), _lp(a)))
        return a

    def samples_hist_torch(self, edges, s0=0, ns=None):
        """The same as an int64 torch tensor on the engine's device, filled by the asynchronous form and synchronised."""
        import torch
        ns, nf, ed, _ = self._hist_args(s0, ns, edges, None, "samples_hist_torch")
        return self._dev((nf, ed.shape[1] + 1),
                         lambda p: self.L.mcmcx_samples_hist_dev(self.h, int(s0), ns, int(ed.shape[1] - 1), _dp(ed), p)).view(torch.int64)

    def samples_hist2(self, pairs, edges, s0=0, ns=None):
        """int64 [npairs][nbins + 2][nbins + 2]: for every pair (j, k) of field indices the number of (sample, chain) points of the
        window with field j in cell a of edges[j] and field k in cell b of edges[k], at [a][b]; at most HIST2_MAXBINS bins and
        HIST2_MAXPAIRS pairs per call.  Exact and additive over engines that hold disjoint chains."""
        ns, nf, ed, pr = self._hist_args(s0, ns, edges, pairs, "samples_hist2")
        a = np.zeros((pr.shape[0], ed.shape[1] + 1, ed.shape[1] + 1), dtype=np.int64)
        self._chk(self.L.mcmcx_samples_hist2(self.h, int(s0), ns, int(pr.shape[0]), pr.ctypes.data_as(C.POINTER(C.c_int32)),
                                             int(ed.shape[1] - 1), _dp(ed), _lp(a)))
        return a

    def samples_hist2_torch(self, pairs, edges, s0=0, ns=None):
        """The same as an int64 torch tensor on the engine's device, filled by the asynchronous form and synchronised."""
        import torch
        ns, nf, ed, pr = self._hist_args(s0, ns, edges, pairs, "samples_hist2_torch")
        return self._dev((pr.shape[0], ed.shape[1] + 1, ed.shape[1] + 1),
                         lambda p: self.L.mcmcx_samples_hist2_dev(self.h, int(s0), ns, int(pr.shape[0]), pr.ctypes.data_as(C.POINTER(C.c_int32)),
                                                                  int(ed.shape[1] - 1), _dp(ed), p)).view(torch.int64)

    # --- posterior covariance of the retained samples, on the matrix cores (mcmcx_samples_cov)
    def samples_cov_stats(self, s0=0, ns=None, shift=None):
        """The cov vector of retained samples s0 .. s0 + ns - 1 of all chains (include/mcmcx.h has the definition): additive over engines
        that were given the same `shift`; `samples_cov_finish` finishes it."""
        ns, _, _, nf = self._window(s0, ns)
        sh = self._shift(shift, nf, "samples_cov_stats")
        a = np.zeros(self._chk(self.L.mcmcx_samples_cov_len(self.h)))
        self._chk(self.L.mcmcx_samples_cov(self.h, int(s0), ns, _dp(sh), _dp(a)))
        return a

    def samples_cov_stats_torch(self, s0=0, ns=None, shift=None):
        """The same vector as a float64 torch tensor on the engine's device, filled by the asynchronous form and synchronised."""
        ns, _, _, nf = self._window(s0, ns)
        sh = self._shift(shift, nf, "samples_cov_stats_torch")
        return self._dev(self._chk(self.L.mcmcx_samples_cov_len(self.h)),
                         lambda p: self.L.mcmcx_samples_cov_dev(self.h, int(s0), ns, _dp(sh), p))

    def samples_cov(self, s0=0, ns=None, shift=None, fields="theta"):
        """dict: `mean`, `cov`, `corr` of the window over all chains, `n` = ns x nchains, `fields` the names of the rows.  fields="theta"
        (the default) keeps the parameter block -- its `cov` is a valid `setcmat0` of the next run --, "all" every field of the store.
        shift="mean" first takes the mean from samples_stats(maxlag=0) (two halves: a window of four samples at least)."""
        nf = self.samples_kept()[3]
        if fields not in ("theta", "all"):
            raise McmcError("samples_cov: fields must be 'theta' or 'all'")
        if isinstance(shift, str):
            if shift != "mean":
                raise McmcError("samples_cov: shift must be None, 'mean' or an array")
            shift = samples_diag(self.samples_stats(s0, ns, 0), nf, 0)[:, 0].copy()
        vec = self.samples_cov_stats(s0, ns, shift)
        mean, cov, corr = samples_cov_finish(vec, nf)
        k = self.npar if fields == "theta" else nf
        names = sample_field_names(self.npar, getattr(self, "nycol", 1))
        return {"fields": names[:k], "mean": mean[:k].copy(), "cov": cov[:k, :k].copy(), "corr": corr[:k, :k].copy(), "n": int(vec[0])}

    # --- batch-means covariance of the retained samples and its finishes (mcmcx_samples_cov_bm, mcmcx_samples_mess / _mpsrf)
    def samples_cov_bm_stats(self, batch, s0=0, ns=None, shift=None):
        """The batch-means vector of retained samples s0 .. s0 + ns - 1 of all chains (include/mcmcx.h has the definition): the cov
        vector of the means of batches of `batch` consecutive samples, additive over engines that were given the same `shift` and
        `batch`; `samples_mess` and `samples_mpsrf` finish it beside a cov vector, `samples_cov_finish` gives the batch means' moments."""
        ns, _, _, nf = self._window(s0, ns)
        sh = self._shift(shift, nf, "samples_cov_bm_stats")
        a = np.zeros(self._chk(self.L.mcmcx_samples_cov_len(self.h)))
        self._chk(self.L.mcmcx_samples_cov_bm(self.h, int(s0), ns, int(batch), _dp(sh), _dp(a)))
        return a

    def samples_cov_bm_stats_torch(self, batch, s0=0, ns=None, shift=None):
        """The same vector as a float64 torch tensor on the engine's device, filled by the asynchronous form and synchronised."""
        ns, _, _, nf = self._window(s0, ns)
        sh = self._shift(shift, nf, "samples_cov_bm_stats_torch")
        return self._dev(self._chk(self.L.mcmcx_samples_cov_len(self.h)),
                         lambda p: self.L.mcmcx_samples_cov_bm_dev(self.h, int(s0), ns, int(batch), _dp(sh), p))

    def _joint_args(self, s0, ns, fields, shift, who):
        """(ns, nfields, selection, shift) of a joint diagnostic"""
        ns, _, _, nf = self._window(s0, ns)
        if isinstance(fields, str):
            if fields not in ("theta", "all"):
                raise McmcError("%s: fields must be 'theta', 'all' or a list of field indices" % who)
            fields = range(self.npar if fields == "theta" else nf)
        if isinstance(shift, str):
            if shift != "mean":
                raise McmcError("%s: shift must be None, 'mean' or an array" % who)
            shift = samples_diag(self.samples_stats(s0, ns, 0), nf, 0)[:, 0].copy()
        return ns, nf, _sel(list(fields), nf, who), shift

    def samples_mess(self, s0=0, ns=None, batch=None, fields="theta", shift="mean"):
        """The multivariate effective sample size of the window for the mean VECTOR of `fields` ("theta", "all" or field indices; leave
        a field out that is constant over the window): the module function samples_mess's dict with `batch` and `fields` added.  batch =
        floor(sqrt(ns)) by default; the window is trimmed to nb x batch samples for both vectors.  shift="mean" takes the mean of
        samples_stats(maxlag=0) first."""
        ns, nf, idx, shift = self._joint_args(s0, ns, fields, shift, "samples_mess")
        b = int(np.floor(np.sqrt(ns))) if batch is None else int(batch)
        if b < 1 or b > ns:
            raise McmcError("samples_mess: a batch of %d samples in a window of %d" % (b, ns))
        used = (ns // b) * b
        out = samples_mess(self.samples_cov_stats(s0, used, shift), self.samples_cov_bm_stats(b, s0, used, shift), nf, b, idx)
        out["batch"], out["fields"] = b, [sample_field_names(self.npar, getattr(self, "nycol", 1))[j] for j in idx]
        return out

    def samples_mpsrf(self, s0=0, ns=None, fields="theta", shift="mean"):
        """The multivariate split-R-hat of the window over `fields`: the module function samples_mpsrf's dict with `fields` added; an odd
        window loses its last sample.  It is at least the split-R-hat of every selected field, and can be far above all of them."""
        ns, nf, idx, shift = self._joint_args(s0, ns, fields, shift, "samples_mpsrf")
        nh = ns // 2
        if nh < 2:
            raise McmcError("samples_mpsrf: a window of %d samples, four at least" % ns)
        out = samples_mpsrf(self.samples_cov_stats(s0, 2 * nh, shift), self.samples_cov_bm_stats(nh, s0, 2 * nh, shift), nf, nh, idx)
        out["fields"] = [sample_field_names(self.npar, getattr(self, "nycol", 1))[j] for j in idx]
        return out

    def pooled_moments(self):
        n = self.L.mcmcx_pooled_moments_len(self.h)
        a = np.zeros(n)
        self._chk(self.L.mcmcx_pooled_moments(self.h, _dp(a)))
        return a

    def pooled_moments_dev(self, dev_ptr):
        """Pooled moments straight into device memory (e.g. a torch tensor's data_ptr()); async on the engine stream."""
        self._chk(self.L.mcmcx_pooled_moments_dev(self.h, C.c_void_p(int(dev_ptr))))

    def set_comm(self, comm):
        """Attach the node's communicator (before init): pooled-mode ticks and allreduce_moments span all ranks."""
        self._comm = comm
        self._chk(self.L.mcmcx_set_comm(self.h, comm.h if comm is not None else None))

    def allreduce_moments(self, fetch=True):
        """Pooled moments of the chains of ALL ranks (collective).  fetch=False leaves them on the device (async)."""
        if not fetch:
            self._chk(self.L.mcmcx_allreduce_moments(self.h, None))
            return None
        a = np.zeros(self.L.mcmcx_pooled_moments_len(self.h))
        self._chk(self.L.mcmcx_allreduce_moments(self.h, _dp(a)))
        return a

    def set_exchange(self, fn, dev_ptr):
        """Pooled mode over several GPUs: fn() must all-reduce (sum) the device buffer at dev_ptr in place."""
        self._xkeep = _lib.EXCHANGE_T(lambda user: fn())
        self._chk(self.L.mcmcx_set_exchange(self.h, self._xkeep, None, C.c_void_p(int(dev_ptr))))

    def pooled(self):
        n = self.npar
        cm = np.zeros((n, n), order="F"); R = np.zeros((n, n), order="F"); m = np.zeros(n); w = C.c_double()
        dp = C.POINTER(C.c_double)
        self._chk(self.L.mcmcx_get_pooled(self.h, cm.ctypes.data_as(dp), _dp(m), C.byref(w), R.ctypes.data_as(dp)))
        return np.array(cm), m, w.value, np.array(R)

    def debug_set_factor(self, R, qcovstd=None):
        """Test probe: every chain's SVD proposal factor replaced by R[i, j] (scam: the rotation U) and qcovstd."""
        a = np.asfortranarray(np.asarray(R, dtype=np.float64))
        q = None if qcovstd is None else _f64(qcovstd)
        self._chk(self.L.mcmcx_debug_set_factor(self.h, a.ctypes.data_as(C.POINTER(C.c_double)), _dp(q)))

    def last_kernel(self):
        """Name of the sampling kernel the last run() launched (mcmcx_last_kernel)."""
        return (self.L.mcmcx_last_kernel(self.h) or b"").decode()

    def last_instance(self):
        """Test probe (mcmcx_debug_last_instance): the template instance(s) the last run() launched for the step, joined by '+' --
        'group_step_kernel<16,20,2,gauss>+group_step_kernel<16,20,1,any>', 'group_ram_kernel<32>'; elsewhere last_kernel()'s name."""
        buf = C.create_string_buffer(256)
        self._chk(self.L.mcmcx_debug_last_instance(self.h, buf, 256))
        return buf.value.decode()

    def kernel_time(self, reset=False):
        ms, nl, ns = C.c_double(), C.c_int64(), C.c_int64()
        self._chk(self.L.mcmcx_kernel_time(self.h, C.byref(ms), C.byref(nl), C.byref(ns), int(reset)))
        return ms.value, nl.value, ns.value


def kernel_table():
    """[(family, name), ...]: every entry of the engine's kernel-selection tables (mcmcx_debug_kernel_table); no device needed."""
    L = _lib.load()
    n = L.mcmcx_debug_kernel_table(-1, None, 0)
    out = []
    for i in range(n):
        buf = C.create_string_buffer(128)
        L.mcmcx_debug_kernel_table(i, buf, 128)
        fam, name = buf.value.decode().split(":", 1)
        out.append((fam, name))
    return out


def debug_symsvd(form, A, need=None, device=0, fill=0.0, sweeps_fill=-1):
    """Test probe (mcmcx_debug_symsvd): the pinned SVD of the symmetric matrices A[nmat, d, d] in the host's statement (form 0, no device),
    the lane form (1) or the blocked kernels (2).  Returns (V[nmat, d, d] with the singular vectors as columns, s[nmat, d], sweeps[nmat],
    forms); rows of matrices with need == 0 keep `fill` / `sweeps_fill`.  Raises RuntimeError on a refusal."""
    L = _lib.load()
    A = np.asarray(A, dtype=np.float64)
    nmat, d = A.shape[0], A.shape[-1]
    a = np.ascontiguousarray(np.swapaxes(A, 1, 2))                  # [m][column][row]: column-major d x d per matrix
    V = np.full((nmat, d, d), fill, dtype=np.float64); s = np.full((nmat, d), fill, dtype=np.float64)
    sweeps = np.full(nmat, sweeps_fill, dtype=np.int32)
    nd = None if need is None else np.ascontiguousarray(np.asarray(need, dtype=np.uint8))
    buf = C.create_string_buffer(256)
    rc = L.mcmcx_debug_symsvd(device, form, d, nmat, _dp(a), None if nd is None else nd.ctypes.data_as(C.POINTER(C.c_uint8)), _dp(V), _dp(s),
                              sweeps.ctypes.data_as(C.POINTER(C.c_int32)), buf, 256)
    if rc != 0:
        raise RuntimeError("mcmcx_debug_symsvd: %d %s" % (rc, (L.mcmcx_last_error() or b"").decode()))
    return np.swapaxes(V, 1, 2), s, sweeps, buf.value.decode()


INFO_SENTINEL = -77          # MCMCX_DEBUG_INFO_SENTINEL


def debug_host_calculate_R(A, with_inverse=True, fill=0.0):
    """Test probe (mcmcx_debug_host_calculate_R): the host's host_initial_R + host_potri on the symmetric A[d, d], no device.  Returns
    (R[d, d] upper, iC[d, d] upper, info, info2); what a failure leaves unwritten keeps `fill`.  Raises RuntimeError on a refusal."""
    L = _lib.load()
    A = np.asarray(A, dtype=np.float64)
    d = A.shape[-1]
    a = np.ascontiguousarray(A.T)
    R = np.full((d, d), fill); iC = np.full((d, d), fill)
    info = np.zeros(2, dtype=np.int32)
    rc = L.mcmcx_debug_host_calculate_R(d, _dp(a), _dp(R), _dp(iC) if with_inverse else None, info.ctypes.data_as(C.POINTER(C.c_int32)))
    if rc != 0:
        raise RuntimeError("mcmcx_debug_host_calculate_R: %d %s" % (rc, (L.mcmcx_last_error() or b"").decode()))
    return R.T.copy(), iC.T.copy(), int(info[0]), int(info[1])


def engine_from_problem(cfg_kw, prob_kw, nchains=1, **extra):
    """Build an Engine from the same (cfg, problem) dictionaries the oracle / golden fixtures use."""
    pk = dict(prob_kw)
    npar = int(pk["npar"])
    extra = dict(extra)
    comm = extra.pop("comm", None)
    external = extra.pop("external", False)          # MCMC_run1: the caller evaluates the target
    cfg = make_config(npar, nchains, **cfg_kw, **extra)
    e = Engine(cfg)
    if comm is not None:
        e.set_comm(comm)
    e.setpar0(pk["par0"])
    e.setcmat0(np.asarray(pk["cmat0"], dtype=np.float64).reshape(npar, npar))
    e.setsigma2nobs(pk.get("sigma2", 1.0), pk.get("nobs", 1))
    if external:
        e.set_target_external()
        return e
    e.set_target(str(pk["kind"]), mu=pk.get("mu"), lam=pk.get("lam"), b=float(pk.get("b", 0.1)),
                 xdata=pk.get("xdata"), ydata=pk.get("ydata"))
    if pk.get("lo") is not None or pk.get("hi") is not None:
        e.set_bounds(pk.get("lo"), pk.get("hi"))
    if pk.get("pri_mu") is not None:
        e.set_priors(pk["pri_mu"], pk["pri_sig"])
    return e
