"""Predictive mean and variance at a list of entries of a variational model, the closed form of its q, on the device (DESIGN.md
section 2.8a).

    m = bnmf_vb_optimised(R, M, K, priors, ...); m.initialise(); m.run(iterations)     # likewise bnmf_vb_observed, bnmtf_vb_optimised,
                                                                                       # bnmtf_vb_observed: either layout, any rank
    P = variational_predictive(m, at)         # at: an Entries of the model's shape (values ignored), or (rows, cols)
    P.mean, P.variance        # fp64 [n], in the order given: E_q and Var_q of U[i] . V[j], or (F[i] S) . G[j]
    P.noise                   # E_q[1 / tau] = beta_s / (alpha_s - 1)
    P.std()                   # sqrt(variance + noise): the spread of a new observation; std(noise=False): of the model's mean

Under the mean-field q every entry of every factor is independent.  With f, a the mean and variance (exp*, var*) of row i of the
first factor, s, b of S and g, c of row j of the last:

    two factors   mean = sum_k f_k g_k                 variance = sum_k [ a_k g_k^2 + c_k f_k^2 + a_k c_k ]
    three         mean = sum_l P_l g_l,  P = f S       variance = sum_k a_k H_k^2 + sum_l [ c_l (P_l^2 + u_l) + (g_l^2 + c_l) w_l ]
                  H = S g,  u_l = sum_k a_k s_kl^2,  w_l = sum_k b_kl (f_k^2 + a_k)

(E[X^2] expanded with E[F_k F_k'] = f_k f_k' + [k = k'] a_k and likewise for S and G has eight terms; one is mean^2, these are the
other seven).  Every term is a product of non-negative numbers: nothing cancels.  The work runs in bnmtf_predictive_moments
(csrc/api_predictive_q.inc, kernel_predictive_q.hip); nothing of size I x J is made anywhere.

from_moments is the same on plain arrays; a variance of None marks a factor that is fixed.  That takes what fold_in returns:

    F = fold_in(m, new_rows, iterations)                                               # F.mean, F.variance [r][K], F.other = E[V]
    Q = variational_predictive.from_moments(((F.mean, F.variance), (F.other, None)), (r, J), rows, cols)
    Q.variance                # sum_k F.variance[i, k] * F.other[j, k]^2: how sure the folded-in rows' predictions are

Everything that is refused is refused before the first device call."""
import ctypes as C

import numpy as np

from . import _lib
from ._postfit import device_of, entry_lists, kind_of, refuse
from .entries import Entries
from .predictive import Predictive

MAX_RANK = 256          # K and L of bnmtf_predictive_moments (BNMTF_PREDICTIVE_Q_MAX_RANK)


class VariationalPredictive(Predictive):
    """What variational_predictive returns: rows, cols (int32 [n], as given), mean, variance (fp64 [n]), noise (float; nan when
    alpha_s / beta_s were not given), count = 0 (no samples: a closed form of q)."""

    def __init__(self, rows, cols, mean, variance, noise):
        super(VariationalPredictive, self).__init__(rows, cols, mean, variance, noise, 0)

    def __repr__(self):
        return "VariationalPredictive(%d entries, closed form of q)" % len(self)


def _noise(who, alpha_s, beta_s):
    if alpha_s is None and beta_s is None:
        return float('nan')
    if alpha_s is None or beta_s is None:
        refuse(who, "alpha_s and beta_s come together: q(tau) = Gamma(alpha_s, beta_s)")
    alpha_s, beta_s = float(alpha_s), float(beta_s)
    if not (np.isfinite(alpha_s) and np.isfinite(beta_s) and beta_s > 0):
        refuse(who, "q(tau) = Gamma(alpha_s, beta_s) needs finite alpha_s and beta_s > 0 (alpha_s=%r, beta_s=%r)" % (alpha_s, beta_s))
    if alpha_s <= 1:
        refuse(who, "the noise E_q[1 / tau] = beta_s / (alpha_s - 1) exists for alpha_s > 1 only (alpha_s=%r)" % alpha_s)
    return beta_s / (alpha_s - 1.0)


def _compute(who, factors, shape, rows, cols, alpha_s, beta_s, device):
    try:
        pairs = [tuple(p) for p in factors]
    except TypeError:
        pairs = None
    if pairs is None or len(pairs) not in (2, 3) or any(len(p) != 2 for p in pairs):
        refuse(who, "factors is ((EA, VA), (EB, VB)) or ((EA, VA), (ES, VS), (EB, VB)): a (mean, variance) pair per factor, the "
                    "variance None for a fixed factor")
    I, J = int(shape[0]), int(shape[1])
    if I < 1 or J < 1:
        refuse(who, "a matrix of at least one row and one column, not %d x %d" % (I, J))
    means = [_lib.f64(p[0]) for p in pairs]
    variances = [None if p[1] is None else _lib.f64(p[1]) for p in pairs]
    if any(m.ndim != 2 for m in means):
        refuse(who, "every factor is two-dimensional, not %s" % ", ".join(str(m.shape) for m in means))
    for m, v in zip(means, variances):
        if v is not None and v.shape != m.shape:
            refuse(who, "a factor's mean and variance have different shapes: %s and %s" % (m.shape, v.shape))
    tri = len(means) == 3
    K = means[0].shape[1]
    L = means[1].shape[1] if tri else 0
    W = L if tri else K
    if means[0].shape[0] != I or means[-1].shape != (J, W) or (tri and means[1].shape[0] != K):
        refuse(who, "factor arrays of shapes %s do not fit each other and the %d x %d matrix" % (", ".join(str(m.shape) for m in means), I, J))
    if not (1 <= K <= MAX_RANK) or (tri and not (1 <= L <= MAX_RANK)):
        refuse(who, "ranks 1 .. %d (K=%d, L=%d)" % (MAX_RANK, K, L))
    for m, v in zip(means, variances):
        if not np.isfinite(m).all():
            refuse(who, "a factor holds a mean that is not finite")
        if v is not None and not (np.isfinite(v).all() and (v >= 0).all()):
            refuse(who, "a factor holds a variance that is negative or not finite")
    rows, cols = entry_lists(who, (I, J), rows, cols)
    noise = _noise(who, alpha_s, beta_s)

    n = len(rows)
    mean, variance = np.zeros(n), np.zeros(n)
    ES, VS = (means[1], variances[1]) if tri else (None, None)
    _lib.check(_lib.lib().bnmtf_predictive_moments(int(device), I, J, int(K), int(L), C.c_uint64(n), _lib.ptr(rows), _lib.ptr(cols),
                                                   _lib.ptr(means[0]), _lib.ptr(variances[0]), _lib.ptr(ES), _lib.ptr(VS),
                                                   _lib.ptr(means[-1]), _lib.ptr(variances[-1]), _lib.ptr(mean), _lib.ptr(variance)))
    return VariationalPredictive(rows, cols, mean, variance, noise)


def from_moments(factors, shape, rows, cols, *, alpha_s=None, beta_s=None, device=0):
    """variational_predictive on plain arrays.  factors: ((EA, VA), (EB, VB)) -- [I][K], [J][K] -- or ((EA, VA), (ES, VS), (EB, VB))
    -- [I][K], [K][L], [J][L] --, the mean and the variance of every factor under q, a variance of None for a factor that is fixed;
    shape (I, J); rows, cols: the entries; alpha_s, beta_s: q(tau) = Gamma(alpha_s, beta_s), both or neither (noise is then nan).
    With the result F of fold_in, ((F.mean, F.variance), (F.other, None)) gives the variance of the folded-in rows' predictions
    (axis=1: ((F.other, None), (F.mean, F.variance))).  Returns a VariationalPredictive."""
    return _compute("variational_predictive.from_moments", factors, shape, rows, cols, alpha_s, beta_s, device)


def variational_predictive(model, at, *, device=None):
    """Mean and variance under q of the model's prediction at the entries `at`, and the noise variance E_q[1 / tau]: a
    VariationalPredictive (see the module's text).  model: a bnmf_vb_optimised, bnmf_vb_observed, bnmtf_vb_optimised or
    bnmtf_vb_observed that has been initialised (and, usually, run), either layout, any rank; at: an Entries of the model's shape
    (its values are ignored) or (rows, cols), any order, repeats allowed; device: defaults to the model's."""
    who = type(model).__name__ + ": variational_predictive"
    kind = kind_of(model)
    if kind == 'gibbs':
        refuse(who, "a Gibbs model has samples, not a q: posterior_predictive(model, at, burn_in, thinning) gives their mean and variance")
    if kind in ('icm', 'np'):
        refuse(who, "a point estimate has no q and no predictive variance (bnmf_vb_optimised, bnmf_vb_observed, bnmtf_vb_optimised "
                    "and bnmtf_vb_observed are taken)")
    if kind != 'variational':
        refuse(who, "not a bnmf_vb_optimised, bnmf_vb_observed, bnmtf_vb_optimised or bnmtf_vb_observed")
    names = [(p + f) for f in model._FACTORS for p in ("exp", "var")]
    if not all(hasattr(model, a) for a in names):
        refuse(who, "no q yet (%s): initialise() has not been called" % ", ".join(a for a in names if not hasattr(model, a)))
    if not (hasattr(model, "alpha_s") and hasattr(model, "beta_s")):
        refuse(who, "no alpha_s / beta_s yet: neither initialise(), update_tau() nor run() has set q(tau)")
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
    factors = [(getattr(model, "exp" + f), getattr(model, "var" + f)) for f in model._FACTORS]
    return _compute(who, factors, shape, rows, cols, model.alpha_s, model.beta_s, device_of(model, device))


variational_predictive.from_moments = from_moments
