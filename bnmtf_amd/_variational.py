"""What the variational classes of both factorisations share: bnmf_vb_optimised / bnmf_vb_observed (R ~ U.V^T) and
bnmtf_vb_optimised / bnmtf_vb_observed (R ~ F.S.G^T) differ in how many factors they carry and in which C entry points they name,
and every one of those entry points takes the q parameters -- mu, tau, exp, var of each factor -- as consecutive pointer arguments in
one order.  So the priors, the q hand-over, run() behind its argument checks, the single updates, exp_square_diff and the
model-quality methods are written here once, over the factor tuple.

A model class supplies
    _FACTORS    the factor names in C argument order
    _NAMES      mu, tau, exp, var of each factor, in that order: the q parameters as every state call takes them
    _DENSE      its entry points on the dense layout: set_state, get_state, run, update, exp_square_diff, run_many -- and set_tau
                where exptau can go up without the q parameters, esd_rest where exp_square_diff has further outputs
    _OBSERVED   ... on the observed-entry layout (the *_vb_observed subclass): set_state, get_state, run, update, exp_square_diff,
                and the _observed functions create, metric_sums
    _KEEPS_DEVICE_STATE     whether the hand-over remembers what the device holds (see there)
    _ONES_IN_PUSH, _ONES_IN_ESD     the attributes _push / exp_square_diff fill with ones when nobody has set them
    _factor_shapes()        the factors' shapes
and keeps what is its own: the constructor's checks of R, M and the ranks, initialise, train, run's argument checks (the
tri-factorisation's update orders), the named one-line updates, the ELBO, and the column blocks of bnmf_vb_optimised."""
import ctypes as C
import math

import numpy as np

from . import _lib
from ._base import DeviceModel, broadcast_lambda, information_criterion, metrics_from_sums, performances
from .distributions import TN_vector_expectation, TN_vector_variance, _moments, gamma_expectation, gamma_expectation_log


def q_names(factors):
    return tuple(p + f for f in factors for p in ("mu", "tau", "exp", "var"))


class Variational(DeviceModel):
    _FACTORS = _NAMES = _DENSE = _OBSERVED = None
    _layout = 'dense'               # (an instance on the observed-entry layout carries its own)
    # True: _push uploads only what changed since the device last gave or took the q parameters, and the device keeps what it
    # carries between its half sweeps -- run(a); run(b) is the trajectory of run(a + b).  False (the dense tri-factorisation):
    # every _push uploads, and the device rebuilds what it derives from the q parameters.
    _KEEPS_DEVICE_STATE = True
    _ONES_IN_PUSH = _ONES_IN_ESD = ()

    def _factor_shapes(self):
        raise NotImplementedError

    def _shapes(self):
        return [s for s in self._factor_shapes() for _ in range(4)]

    def _entries(self):
        return self._OBSERVED if self._layout == 'observed' else self._DENSE

    def _entry(self, name):
        """The library's `name` call for this model's factorisation and layout."""
        return getattr(_lib.lib(), self._entries()[name])

    def _blocked(self):
        return getattr(self, "_blocks", None) is not None

    def _init_priors(self, priors, device, verbose, rank, world, comm_id):
        """The constructor behind the checks of R, M and the ranks: alpha, beta, the factors' prior rates, the device."""
        self.alpha, self.beta = float(priors['alpha']), float(priors['beta'])
        for f, shape in zip(self._FACTORS, self._factor_shapes()):
            setattr(self, "lambda" + f, broadcast_lambda(priors["lambda" + f], shape, "lambda" + f))
        self.verbose = verbose
        # (VB draws nothing on the device: the key is unused, 0 on every rank; rank / world / comm_id: the factors' rows over several GPUs)
        self._init_device(0, device, rank, world, comm_id)

    def _lambda_arrays(self):
        lam = [getattr(self, "lambda" + f) for f in self._FACTORS]
        return lam[0], lam[-1], lam[1] if len(lam) == 3 else None

    def _own(self, A, S, B):
        """The factors (A, S, B) in this model's order, its own expectations standing in for a None."""
        given = (A, S, B) if len(self._FACTORS) == 3 else (A, B)
        return [getattr(self, "exp" + f) if g is None else g for f, g in zip(self._FACTORS, given)]

    def _exp_asb(self):
        """(E[A], E[S] or None, E[B]) as the metric calls shared by both factorisations take them."""
        e = [getattr(self, "exp" + f) for f in self._FACTORS]
        return e[0], e[1] if len(e) == 3 else None, e[-1]

    # -- state hand-over --------------------------------------------------------
    def _fill(self, names):
        """The reference's tests set only some of the q parameters: those of `names` nobody has set become ones."""
        for n, s in zip(self._NAMES, self._shapes()):
            if n in names and not hasattr(self, n):
                setattr(self, n, np.ones(s))

    def _push(self):
        self._fill(self._ONES_IN_PUSH)
        exptau = float(getattr(self, "exptau", 1.0))
        blocked = self._blocked()
        if self._KEEPS_DEVICE_STATE:
            # _device_state = (handle, exptau, arrays): what the device holds (in fp32; a push of the same arrays would give it the
            # same).  Nothing touched the q parameters or exptau since: no upload.  Only exptau moved (update_tau / update_exp_tau
            # between two device calls), and the layout has a call for it alone: the q parameters on the device stay.
            held = getattr(self, "_device_state", None)
            tau_alone = not blocked and "set_tau" in self._entries()
            if (held is not None and held[0] is (None if blocked else self._h) and (held[1] == exptau or tau_alone)
                    and all(np.array_equal(getattr(self, n), a) for n, a in zip(self._NAMES, held[2]))):
                if held[1] != exptau:
                    _lib.check(self._entry("set_tau")(self._handle(), exptau))
                    self._device_state = (held[0], exptau, held[2])
                return
            if blocked:
                self._blocks.push(exptau)
                self._device_state = (None, exptau, [np.array(getattr(self, n), dtype=float) for n in self._NAMES])
                return
            self._device_state = None
        arrs = [_lib.f64(getattr(self, n)) for n in self._NAMES]
        _lib.check(self._entry("set_state")(self._handle(), *[_lib.ptr(a) for a in arrs], exptau))
        if self._KEEPS_DEVICE_STATE:
            self._device_state = (self._h, exptau, [np.array(a, dtype=float) for a in arrs])

    def _pull(self):
        if self._blocked():
            got = self._blocks.pull()
            for n in self._NAMES:
                setattr(self, n, got[n])
            self._device_state = (None, float(getattr(self, "exptau", 1.0)), [got[n].copy() for n in self._NAMES])
            return
        arrs = [np.zeros(s) for s in self._shapes()]
        _lib.check(self._entry("get_state")(self._handle(), *[_lib.ptr(a) for a in arrs]))
        held = getattr(self, "_device_state", None)
        for n, a in zip(self._NAMES, arrs):
            setattr(self, n, a)
        if self._KEEPS_DEVICE_STATE:
            # exptau: a single update leaves the device's as it was pushed -- where it can go up alone the next _push sends it
            # again, elsewhere the record keeps it; behind a run() _run_finish fills in the one formed from the device's beta_s
            kept = None if held is None or "set_tau" in self._entries() else held[1]
            self._device_state = (self._h, kept, [a.copy() for a in arrs])

    # -- run ----------------------------------------------------------------------
    def _run(self, it, Mt, *orders):
        """run() behind the class's argument checks: the state and the held-out mask onto the device, one device call for all
        iterations (orders: what it takes ahead of its outputs), the records."""
        self._push()
        self._set_heldout(Mt)
        exptau = np.zeros(it); perf = np.zeros((it, 3)); terms = np.zeros((it, 10)); times = np.zeros(it)
        self._run_device(it, *orders, exptau, perf, terms, times)
        self._finish_heldout(it)
        self._run_finish(it, exptau, perf, terms, times)

    def _run_finish(self, it, exptau, perf, terms, times):
        """What run() does behind the device call (batch.run_many: behind the call that ran this model among others)."""
        self._pull()
        self.all_exp_tau = list(exptau)
        self.all_times = list(times)
        self.all_performances = performances(perf)
        self._take_elbo_terms(terms)
        if it > 0:
            self.alpha_s = self.alpha + self.size_Omega / 2.0
            self.beta_s = terms[-1, 1]
            self.update_exp_tau()
            if getattr(self, "_device_state", None) is not None:      # alpha_s / beta_s from the device's own beta_s: the exptau it holds
                self._device_state = (self._device_state[0], float(self.exptau), self._device_state[2])
        if self.verbose:
            for i in range(it):
                print(self._iteration_line(i, perf))
        return

    def _take_elbo_terms(self, terms):
        """Per iteration: exp_square_diff, beta_s, then the (quad, log erfc, log tau, lambda E) sums of the first and of the last
        factor."""
        self.all_elbo_terms = terms

    def _iteration_line(self, i, perf):
        return "Iteration %s. MSE: %s. R^2: %s. Rp: %s." % (i + 1, perf[i, 0], perf[i, 1], perf[i, 2])

    # -- updates ----------------------------------------------------------------
    def update_tau(self):
        """bnmf_vb_optimised.py:181-183, bnmtf_vb_optimised.py:231-233."""
        self.alpha_s = self.alpha + self.size_Omega / 2.0
        self.beta_s = self.beta + 0.5 * self.exp_square_diff()

    def update_exp_tau(self):
        """:213-215, :286-288."""
        self.exptau = gamma_expectation(self.alpha_s, self.beta_s)
        self.explogtau = gamma_expectation_log(self.alpha_s, self.beta_s)

    def exp_square_diff(self):
        """:185-187, :235-239 (fp64 on the device)."""
        self._fill(self._ONES_IN_ESD)
        self._push()
        if self._blocked():
            return self._blocks.esd(self.expU, self.expV)[0]
        out = C.c_double()
        _lib.check(self._entry("exp_square_diff")(self._handle(), C.byref(out), *self._entries().get("esd_rest", ())))
        return out.value

    def _update(self, *which_index_moments):
        """One update_<factor> on the device: (which factor, its column -- for the tri-factorisation k and l --, moments too?)."""
        self._push()
        if self._blocked():
            self._blocks.update(*which_index_moments)
        else:
            _lib.check(self._entry("update")(self._handle(), *[int(a) for a in which_index_moments]))
        self._pull()

    def _update_exp(self, f, index):
        """update_exp_<f>: the truncated-normal moments of q at `index` -- a column, or one entry of S."""
        mu, tau = getattr(self, "mu" + f)[index], getattr(self, "tau" + f)[index]
        entry = np.ndim(mu) == 0            # (the reference hands a single entry over as one-element lists)
        if entry:
            mu, tau = [mu], [tau]
        e = TN_vector_expectation(mu, tau)
        getattr(self, "exp" + f)[index] = e[0] if entry else e
        v = TN_vector_variance(mu, tau)
        getattr(self, "var" + f)[index] = v[0] if entry else v

    def _initial_moments(self):
        """update_exp_<f> of every column of every factor, as initialise ends: the moments are element-wise -- one device call per
        factor instead of two per column (a model search builds dozens of models and their set-up was most of its wall time)."""
        for f, shape in zip(self._FACTORS, self._factor_shapes()):
            e, v = _moments(np.ravel(np.broadcast_to(getattr(self, "mu" + f), shape)), np.ravel(getattr(self, "tau" + f)))
            setattr(self, "exp" + f, e.reshape(shape))
            setattr(self, "var" + f, v.reshape(shape))

    # -- prediction / model quality ----------------------------------------------
    def predict(self, M_pred):
        """:219-224, :292-297."""
        return metrics_from_sums(self._metric_sums(M_pred, *self._exp_asb()))

    def quality(self, metric):
        """:247-262, :320-337."""
        return information_criterion(metric, tuple, self.log_likelihood,
                                     lambda: metrics_from_sums(self._metric_sums(None, *self._exp_asb()))['MSE'],
                                     sum(rows * columns for rows, columns in self._factor_shapes()), self.size_Omega, self.elbo)

    def log_likelihood(self):
        """:264-266, :339-342."""
        s = self._metric_sums(None, *self._exp_asb())
        sse = s[2] - 2.0 * s[5] + s[4]
        return self.size_Omega / 2. * (self.explogtau - math.log(2 * math.pi)) - self.exptau / 2. * sse
