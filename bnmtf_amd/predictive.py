"""Posterior predictive mean and variance at a list of entries, from the stored samples of a Gibbs run, on the device (DESIGN.md
section 2.8).

    m = bnmf_gibbs_optimised(R, M, K, priors, ...); m.initialise(); m.run(iterations)          # likewise bnmtf_gibbs_optimised
    P = posterior_predictive(m, at, burn_in, thinning)        # at: an Entries of the model's shape (values ignored), or (rows, cols)
    P.mean, P.variance        # fp64 [n], in the order given: over the samples range(burn_in, iterations, thinning) -- the rule of
                              # approx_expectation -- of p_t = U_t[i] . V_t[j], or (F_t[i] S_t) . G_t[j]; the variance's divisor is T
    P.noise                   # the mean of 1 / tau_t over the same samples
    P.std()                   # sqrt(variance + noise): the spread of a new observation; std(noise=False): of the model's mean

The work -- n K T multiply-adds with gathers -- runs in bnmtf_predictive_samples (csrc/api_predictive.inc, kernel_predictive.hip),
which takes the samples in chunks and hands back, per entry, p of the first sample and the sums of (p_t - p_first) and of its
square; the two divisions that finish the statistics are made here.  Nothing of size I x J is made anywhere.  from_samples is the
same on plain arrays.  Everything that is refused is refused before the first device call."""
import ctypes as C

import numpy as np

from . import _lib
from ._postfit import device_of, entry_lists, kind_of, refuse, shifted_moments, stored_samples
from .entries import Entries

MAX_RANK = 256          # K and L of bnmtf_predictive_samples


class Predictive(object):
    """What posterior_predictive returns: rows, cols (int32 [n], as given), mean, variance (fp64 [n]), noise (float), count (T)."""

    def __init__(self, rows, cols, mean, variance, noise, count):
        self.rows, self.cols, self.mean, self.variance, self.noise, self.count = rows, cols, mean, variance, float(noise), int(count)

    def __len__(self):
        return len(self.rows)

    def __repr__(self):
        return "Predictive(%d entries, %d samples)" % (len(self), self.count)

    def std(self, noise=True):
        """sqrt(variance + noise): the predictive standard deviation of an observation; noise=False: of the noise-free product."""
        return np.sqrt(self.variance + self.noise) if noise else np.sqrt(self.variance)


def _progression(who, indices, stored):
    """(first, step, T) of `indices`, which must be first, first + step, ... with step >= 1, inside the stored samples"""
    idx = np.asarray(list(indices) if isinstance(indices, range) else indices)
    if idx.ndim != 1 or idx.size == 0:
        refuse(who, "no sample selected (%d stored)" % stored)
    if not np.issubdtype(idx.dtype, np.integer):
        refuse(who, "the sample indices are integers, not %s" % idx.dtype)
    first, step = int(idx[0]), int(idx[1] - idx[0]) if idx.size > 1 else 1
    if step < 1 or (idx.size > 1 and not (np.diff(idx) == step).all()):
        refuse(who, "the sample indices must be an arithmetic progression first, first + step, ... with step >= 1 "
                    "(the device call takes first and step)")
    if first < 0 or int(idx[-1]) >= stored:
        refuse(who, "sample indices %d .. %d lie outside the %d stored samples" % (first, int(idx[-1]), stored))
    return first, step, int(idx.size)


def _operands(who, factors, taus, shape, rows, cols, indices, chunk_samples):
    """What bnmtf_predictive_samples and bnmtf_log_predictive_samples are handed, checked: (I, J, K, L, rows, cols, A, S, B, first,
    step, T, the selected taus in fp64)"""
    if len(factors) not in (2, 3):
        refuse(who, "factors is (all_A, all_B) or (all_A, all_S, all_B), not %d arrays" % len(factors))
    I, J = int(shape[0]), int(shape[1])
    stored = len(factors[0])
    if stored == 0:
        refuse(who, "no stored samples")
    if any(len(f) != stored for f in factors):
        refuse(who, "the sample arrays hold different numbers of samples: %s" % ", ".join(str(len(f)) for f in factors))
    first, step, T = _progression(who, indices, stored)
    rows, cols = entry_lists(who, (I, J), rows, cols)
    if int(chunk_samples) < 0:
        refuse(who, "chunk_samples >= 0 (0: the library's default), not %d" % chunk_samples)
    # the samples in their own precision; what is no contiguous fp32 array is cast -- its selected samples only
    stop = first + (T - 1) * step + 1
    if all(isinstance(f, np.ndarray) and f.dtype == np.float32 and f.flags["C_CONTIGUOUS"] for f in factors):
        arrays, c_first, c_step = list(factors), first, step
    else:
        arrays = [np.ascontiguousarray(f[first:stop:step] if isinstance(f, np.ndarray) else [f[i] for i in range(first, stop, step)],
                                       dtype=np.float32) for f in factors]
        c_first, c_step = 0, 1
    A, S, B = arrays[0], (arrays[1] if len(arrays) == 3 else None), arrays[-1]
    if any(a.ndim != 3 for a in arrays):
        refuse(who, "every sample array is three-dimensional [samples][rows][columns], not %s" % ", ".join(str(a.shape) for a in arrays))
    K = A.shape[2]
    L = S.shape[2] if S is not None else 0
    W = L if S is not None else K
    if A.shape[1] != I or B.shape[1] != J or B.shape[2] != W or (S is not None and S.shape[1] != K):
        refuse(who, "sample arrays of shapes %s do not belong to a %d x %d matrix" % (", ".join(str(a.shape[1:]) for a in arrays), I, J))
    if not (1 <= K <= MAX_RANK) or (S is not None and not (1 <= L <= MAX_RANK)):
        refuse(who, "ranks 1 .. %d (K=%d, L=%d)" % (MAX_RANK, K, L))
    taus = np.asarray(taus, dtype=np.float64)
    if taus.ndim != 1 or len(taus) < stop:
        refuse(who, "taus holds a value per stored sample, not %s" % (taus.shape,))
    return I, J, int(K), int(L), rows, cols, A, S, B, c_first, c_step, int(T), taus[first:stop:step]


def _compute(who, factors, taus, shape, rows, cols, indices, device, chunk_samples):
    I, J, K, L, rows, cols, A, S, B, c_first, c_step, T, taus = _operands(who, factors, taus, shape, rows, cols, indices, chunk_samples)
    noise = float(np.mean(1.0 / taus))
    n = len(rows)
    p_first, sum_d, sum_d2 = np.zeros(n), np.zeros(n), np.zeros(n)
    _lib.check(_lib.lib().bnmtf_predictive_samples(int(device), I, J, K, L, C.c_uint64(n), _lib.ptr(rows), _lib.ptr(cols),
                                                   _lib.ptr(A), _lib.ptr(S), _lib.ptr(B), C.c_uint64(c_first), C.c_uint64(c_step), T,
                                                   int(chunk_samples), _lib.ptr(p_first), _lib.ptr(sum_d), _lib.ptr(sum_d2)))
    mean, variance = shifted_moments(p_first, sum_d, sum_d2, T)
    return Predictive(rows, cols, mean, variance, noise, T)


def from_samples(factors, taus, shape, rows, cols, indices, *, device=0, chunk_samples=0):
    """posterior_predictive on plain arrays.  factors: (all_A, all_B) -- [samples][I][K], [samples][J][K] -- or (all_A, all_S, all_B)
    -- [.][I][K], [.][K][L], [.][J][L]; taus [samples]; shape (I, J); rows, cols: the entries; indices: the samples to use, an
    arithmetic progression first, first + step, ... (a range); chunk_samples: samples per upload and launch (0: the library's
    default; the result's bits do not depend on it).  Returns a Predictive."""
    return _compute("predictive.from_samples", factors, taus, shape, rows, cols, indices, device, chunk_samples)


def posterior_predictive(model, at, burn_in, thinning, *, device=None):
    """Mean and variance of the model's prediction at the entries `at` over the stored samples range(burn_in, stored, thinning),
    and the mean noise variance 1 / tau over the same samples: a Predictive (see the module's text).  model: a
    bnmf_gibbs_optimised or bnmtf_gibbs_optimised that has run with store_samples=True, either layout, any rank; at: an Entries of
    the model's shape (its values are ignored) or (rows, cols), any order, repeats allowed; device: defaults to the model's."""
    who = type(model).__name__ + ": posterior_predictive"
    kind = kind_of(model)
    if kind == 'variational':
        refuse(who, "a variational model has no posterior samples: its predictive variance is a closed form of q, not a sample "
                    "statistic, and is out of scope here (bnmf_gibbs_optimised and bnmtf_gibbs_optimised are taken)")
    if kind in ('icm', 'np'):
        refuse(who, "a point estimate has no posterior samples (bnmf_gibbs_optimised and bnmtf_gibbs_optimised are taken)")
    if kind != 'gibbs':
        refuse(who, "not a bnmf_gibbs_optimised or bnmtf_gibbs_optimised")
    names, stored, burn_in, thinning = stored_samples(who, model, burn_in, thinning)
    shape = (int(model.I), int(model.J))
    if isinstance(at, Entries):
        if tuple(at.shape) != shape:
            refuse(who, "the Entries and the model's matrix have different shapes: %s and %s" % (tuple(at.shape), shape))
        rows, cols = at.rows, at.cols
    else:
        try:
            rows, cols = at
        except (TypeError, ValueError):
            refuse(who, "at is an Entries or a pair (rows, cols), not %s" % type(at).__name__)
    return _compute(who, [getattr(model, a) for a in names], model.all_tau, shape, rows, cols, range(burn_in, stored, thinning),
                    device_of(model, device), 0)
