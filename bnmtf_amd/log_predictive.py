"""Log pointwise predictive density and WAIC from the stored samples of a Gibbs run, on the device.

    m = bnmf_gibbs_optimised(R, M, K, priors, ...); m.initialise(); m.run(iterations)          # likewise bnmtf_gibbs_optimised
    Q = log_predictive(m, E_test, burn_in, thinning)          # E_test: an Entries of the model's shape with the true values
    Q.lppd()                                                  # the held-out log pointwise predictive density, sum_e lpd_e
    W = log_predictive(m, None, burn_in, thinning)            # None: the model's own training entries
    W.waic(), W.p_waic(), W.se()                              # WAIC = -2 (lppd - p_waic), its effective parameters, its standard error

Per entry e = (i, j) with value r_e and per selected sample t = 0 .. T - 1 -- range(burn_in, stored, thinning), the rule of
approx_expectation -- the Gaussian log-likelihood l_t = c_t - h_t (r_e - p_t)^2 with p_t = U_t[i] . V_t[j], or (F_t[i] S_t) . G_t[j],
c_t = (log tau_t - log 2 pi) / 2 and h_t = tau_t / 2.  Then

    lpd_e      = log( (1 / T) sum_t exp l_t )                 # Q.lpd
    mean_e     = (1 / T) sum_t l_t                            # Q.mean
    variance_e = sum_t (l_t - mean_e)^2 / (T - 1)             # Q.variance: p_WAIC2 of Gelman, Hwang and Vehtari (2014); nan with T = 1

and lppd = sum_e lpd_e, p_waic = sum_e variance_e, the pointwise elpd_e = lpd_e - variance_e and WAIC = -2 sum_e elpd_e.

The work -- n K T multiply-adds with gathers, and an exp per entry and sample -- runs in bnmtf_log_predictive_samples
(csrc/api_log_predictive.inc, kernel_log_predictive.hip), which takes the samples in chunks and hands back, per entry, l of the first
sample, the sums of (l_t - l_first) and of its square, max_t l_t and sum_t exp(l_t - max); c and h are formed here in NumPy fp64 and
the two logarithms and the divisions that finish the statistics are made here.  Nothing of size I x J is made beyond what the model
holds.  from_samples is the same on plain arrays.  Everything that is refused is refused before the first device call."""
import ctypes as C

import numpy as np

from . import _lib
from ._postfit import device_of, kind_of, refuse, stored_samples
from .entries import Entries
from .predictive import _operands

LOG_2PI = float(np.log(2.0 * np.pi))


class LogPredictive(object):
    """What log_predictive returns: rows, cols (int32 [n], as given), values, lpd, mean, variance (fp64 [n]) and count (T); see the
    module's text."""

    def __init__(self, rows, cols, values, lpd, mean, variance, count):
        self.rows, self.cols, self.values, self.lpd, self.mean, self.variance, self.count = rows, cols, values, lpd, mean, variance, int(count)

    def __len__(self):
        return len(self.rows)

    def __repr__(self):
        return "LogPredictive(%d entries, %d samples)" % (len(self), self.count)

    def _needs_two(self, what):
        if self.count < 2:
            refuse("LogPredictive: " + what, "the variance of the log-likelihood over the samples needs at least two of them (%d selected)" % self.count)

    def lppd(self):
        """sum_e lpd_e: the log pointwise predictive density of the list"""
        return float(np.sum(self.lpd))

    def p_waic(self):
        """sum_e variance_e: the effective number of parameters (p_WAIC2)"""
        self._needs_two("p_waic")
        return float(np.sum(self.variance))

    def pointwise(self):
        """elpd_e = lpd_e - variance_e, fp64 [n]"""
        self._needs_two("pointwise")
        return self.lpd - self.variance

    def waic(self):
        """-2 (lppd - p_waic), on the deviance scale: lower is better"""
        self._needs_two("waic")
        return -2.0 * (self.lppd() - self.p_waic())

    def se(self):
        """sqrt(n Var_e(-2 elpd_e)), the variance over the entries with divisor n - 1: the standard error of waic()"""
        self._needs_two("se")
        if len(self) < 2:
            refuse("LogPredictive: se", "the spread over the entries needs at least two of them")
        return float(np.sqrt(len(self) * np.var(-2.0 * self.pointwise(), ddof=1)))


def _compute(who, factors, taus, shape, rows, cols, values, indices, device, chunk_samples):
    I, J, K, L, rows, cols, A, S, B, c_first, c_step, T, taus = _operands(who, factors, taus, shape, rows, cols, indices, chunk_samples)
    values = np.ascontiguousarray(values, dtype=np.float64)
    if values.ndim != 1 or len(values) != len(rows):
        refuse(who, "values holds the true value of every entry: %d entries, values of shape %s" % (len(rows), values.shape))
    if not np.isfinite(values).all():
        e = int(np.flatnonzero(~np.isfinite(values))[0])
        refuse(who, "the value of entry %d (%d, %d) is not finite: %s" % (e, rows[e], cols[e], values[e]))
    if not (np.isfinite(taus) & (taus > 0)).all():
        refuse(who, "every selected tau is finite and positive")
    c = np.ascontiguousarray(0.5 * (np.log(taus) - LOG_2PI))
    h = np.ascontiguousarray(0.5 * taus)

    n = len(rows)
    l_first, sum_d, sum_d2, l_max, sum_exp = [np.zeros(n) for _ in range(5)]
    _lib.check(_lib.lib().bnmtf_log_predictive_samples(int(device), I, J, K, L, C.c_uint64(n), _lib.ptr(rows), _lib.ptr(cols), _lib.ptr(values),
                                                       _lib.ptr(A), _lib.ptr(S), _lib.ptr(B), C.c_uint64(c_first), C.c_uint64(c_step), T,
                                                       int(chunk_samples), _lib.ptr(c), _lib.ptr(h),
                                                       _lib.ptr(l_first), _lib.ptr(sum_d), _lib.ptr(sum_d2), _lib.ptr(l_max), _lib.ptr(sum_exp)))
    lpd = l_max + np.log(sum_exp) - np.log(float(T))
    mean = l_first + sum_d / T
    # shifted by the first sample, as _postfit.shifted_moments: a spread far below the mean survives fp64
    variance = np.maximum(0.0, (sum_d2 - sum_d * sum_d / T) / (T - 1)) if T > 1 else np.full(n, np.nan)
    return LogPredictive(rows, cols, values, lpd, mean, variance, T)


def from_samples(factors, taus, shape, rows, cols, values, indices, *, device=0, chunk_samples=0):
    """log_predictive on plain arrays.  factors, taus, shape, rows, cols, indices, chunk_samples: as predictive.from_samples; values:
    the true value of every entry, taken in fp64.  Returns a LogPredictive."""
    return _compute("log_predictive.from_samples", factors, taus, shape, rows, cols, values, indices, device, chunk_samples)


def _training_entries(model):
    """(rows, cols, values in fp64) of the entries the model was fitted to: an Entries-built model's list as it is, a dense-built
    model's R[M != 0] in row-major order"""
    if isinstance(model.R, Entries):
        return model.R.rows, model.R.cols, model.R.values
    Mb = np.asarray(model.M) != 0
    rows, cols = np.nonzero(Mb)
    return rows, cols, np.asarray(model.R, dtype=np.float64)[Mb]


def log_predictive(model, at, burn_in, thinning, *, device=None):
    """The log predictive density of the values of `at` under the stored samples range(burn_in, stored, thinning), per entry, with
    the mean and the variance of the log-likelihood over the same samples: a LogPredictive (see the module's text).  model: a
    bnmf_gibbs_optimised or bnmtf_gibbs_optimised that has run with store_samples=True, either layout, any rank; at: an Entries of
    the model's shape whose values are the true values (taken in fp64 as held), any order, repeats allowed, or None: the model's
    own training entries; device: defaults to the model's."""
    who = type(model).__name__ + ": log_predictive"
    kind = kind_of(model)
    if kind == 'variational':
        refuse(who, "a variational model has no posterior samples to average the likelihood over; it has variational_predictive, the "
                    "closed-form predictive mean and variance under q (bnmf_gibbs_optimised and bnmtf_gibbs_optimised are taken)")
    if kind in ('icm', 'np'):
        refuse(who, "a point estimate has no posterior samples (bnmf_gibbs_optimised and bnmtf_gibbs_optimised are taken)")
    if kind != 'gibbs':
        refuse(who, "not a bnmf_gibbs_optimised or bnmtf_gibbs_optimised")
    names, stored, burn_in, thinning = stored_samples(who, model, burn_in, thinning)
    shape = (int(model.I), int(model.J))
    if at is None:
        rows, cols, values = _training_entries(model)
    elif isinstance(at, Entries):
        if tuple(at.shape) != shape:
            refuse(who, "the Entries and the model's matrix have different shapes: %s and %s" % (tuple(at.shape), shape))
        rows, cols, values = at.rows, at.cols, at.values
    else:
        refuse(who, "at is an Entries whose values are the true values at its entries, or None for the training entries: a density "
                    "needs values, which %s does not carry" % ("a pair (rows, cols)" if isinstance(at, (tuple, list)) else type(at).__name__))
    return _compute(who, [getattr(model, a) for a in names], model.all_tau, shape, rows, cols, values, range(burn_in, stored, thinning),
                    device_of(model, device), 0)


log_predictive.from_samples = from_samples          # (the package exports the function under the module's name: bnmtf_amd.log_predictive.from_samples)
