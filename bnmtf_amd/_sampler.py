"""What the Gibbs and ICM classes of both factorisations share: bnmf_gibbs_optimised / nmf_icm (R ~ U.V^T) and
bnmtf_gibbs_optimised / nmtf_icm (R ~ F.S.G^T) differ in how many factors they carry and in which C entry points they name, and
every one of those entry points takes the factors as consecutive pointer arguments in one order.  So the state hand-over, run()
on every path (one handle, column blocks, layout='observed'), the posterior means and the model-quality methods are written here
once, over the factor tuple.

A model class supplies
    _FACTORS    the factor names in C argument order
    _PRIORS     the names of their prior rates, in the same order
    _DENSE      its entry points on the dense layout: set_state, get_state, run, cond_params, run_many
    _OBSERVED   ... with layout='observed': set_state, get_state, run, cond_params, and the _observed functions create, metric_sums
    _BLOCKS_KEEP_STATE   whether its blocks hold the state between calls (see there)
    _shapes()   the factors' shapes
and keeps what is its own: the constructor, initialise, describe, the blocked branch of _handle, _cond and the accessors of the
conditionals, and log_likelihood, whose arguments are named after the factors."""
import ctypes as C
import math

import numpy as np

from . import _lib, _observed
from ._base import DeviceModel, check_binary, information_criterion, metrics_from_sums, performances


class GibbsSampler(_observed.ObservedLayout, DeviceModel):
    _FACTORS = _PRIORS = _DENSE = _OBSERVED = None
    # A blocked model (a rank above 64: _blocked.py) keeps its state in one of two ways.  True (ColumnBlocks): _push hands it to
    # the blocks, which hold it between calls, and a blocked run records it as the device's.  False (TriBlocks): the state lives
    # on the host between the phases of an iteration -- _push has nothing to do, and a blocked run makes the blocks' handles itself.
    _BLOCKS_KEEP_STATE = None

    def _shapes(self):
        raise NotImplementedError

    def _entry(self, name):
        """The library's `name` call for this model's factorisation and layout."""
        return getattr(_lib.lib(), (self._OBSERVED if self._layout == 'observed' else self._DENSE)[name])

    def _asb(self, factors):
        """(A, S, B) as the calls shared by both factorisations take them (bnmtf_create, bnmtf_metric_sums): S is None without one."""
        return (factors[0], factors[1] if len(factors) == 3 else None, factors[-1])

    def _own(self, A, S, B):
        """The factors (A, S, B) in this model's order, its own standing in for a None."""
        given = (A, S, B) if len(self._FACTORS) == 3 else (A, B)
        return [getattr(self, n) if g is None else g for n, g in zip(self._FACTORS, given)]

    def _factors(self):
        return [getattr(self, n) for n in self._FACTORS]

    def _lambda_arrays(self):
        A, S, B = self._asb([getattr(self, n) for n in self._PRIORS])
        return A, B, S

    def close(self):
        if getattr(self, "_blocks", None) is not None:
            self._blocks.close()
        super(GibbsSampler, self).close()

    def _handle(self):
        if self._layout == 'observed':
            if self._h is None:
                self._draw_seed()
                self._h = self._OBSERVED["create"](self)
            return self._h
        return super(GibbsSampler, self)._handle()

    def train(self, init, iterations):
        """bnmf_gibbs_optimised.py:94-96, bnmtf_gibbs_optimised.py:100-102 (as written there: initialise(init=init) is not a
        valid keyword of the tri-factorisation's initialise and raises TypeError in the reference too)."""
        self.initialise(init=init)
        return self.run(iterations)

    # -- state hand-over --------------------------------------------------------
    def _device_holds(self, handle, tau):
        """Is (the factors, tau) what `handle` was last given or gave?  Then nothing touched them since: no upload -- and the
        device keeps what it carries between its half sweeps, so run(a); run(b) is the chain of run(a + b)."""
        held = getattr(self, "_device_state", None)
        return (held is not None and held[0] is handle and tau == held[-1]
                and all(np.array_equal(f, h) for f, h in zip(self._factors(), held[1:-1])))

    def _push(self):
        tau = float(getattr(self, "tau", 1.0))
        if self._blocks is not None:
            if self._BLOCKS_KEEP_STATE and not self._device_holds(None, tau):
                factors = [np.asarray(f, dtype=float) for f in self._factors()]
                self._blocks.push(*factors, tau)
                self._device_state = (None,) + tuple(np.array(f, dtype=float) for f in factors) + (tau,)
            return
        if self._device_holds(self._h, tau):
            return
        self._device_state = None
        factors = [_lib.f64(f) for f in self._factors()]
        _lib.check(self._entry("set_state")(self._handle(), *[_lib.ptr(f) for f in factors], tau))

    def _pull(self):
        factors = [np.zeros(s) for s in self._shapes()]
        tau = C.c_double()
        _lib.check(self._entry("get_state")(self._handle(), *[_lib.ptr(f) for f in factors], C.byref(tau)))
        self._take_state(factors, tau.value)

    def _take_state(self, factors, tau):
        """What the device holds at the end of a call becomes the model's state."""
        for n, f in zip(self._FACTORS, factors):
            setattr(self, n, f)
        self.tau = tau
        self._device_state = (self._h,) + tuple(f.copy() for f in factors) + (tau,)

    # -- run ----------------------------------------------------------------------
    def run(self, iterations, update='draw', store_samples=True, expectation=None, *, M_test=None):
        """bnmf_gibbs_optimised.py:121-157, bnmtf_gibbs_optimised.py:138-180.  One device call runs all iterations; samples, tau,
        metrics and cumulative times come back afterwards.  store_samples=False skips the hand-off of the samples
        (device-resident benchmark mode); update='mode' runs the ICM harness; expectation=(burn_in, thinning) also accumulates
        the posterior means of exactly that approx_expectation(burn_in, thinning) on the device (what the model-selection drivers
        need: with store_samples=False no sample ever crosses to the host).  M_test (a 0/1 matrix shaped like R -- with
        layout='observed' of the two-factor classes an Entries, the held-out entries with their values --; it may overlap
        M): the held-out MSE / R^2 / Rp of the state every iteration ends with are computed on the device and kept in
        all_performances_test; without it no such attribute exists after the call."""
        update = _lib.UPDATE_MODE if update == 'mode' else _lib.UPDATE_DRAW
        if self._layout == 'observed':
            bufs = self._run_observed(iterations, update, store_samples, expectation, M_test)
            return self._run_finish(bufs, store_samples)
        Mt = self._check_heldout(M_test)
        if self._blocks is not None:
            return self._run_blocked(iterations, update, store_samples, expectation)
        bufs = self._run_prepare(iterations, store_samples, expectation)
        self._set_heldout(Mt)
        _lib.check(self._entry("run")(self._handle(), bufs[0], update, *[_lib.ptr(b) for b in bufs[1:]]))
        self._finish_heldout(bufs[0])
        return self._run_finish(bufs, store_samples)

    def _buffers(self, it, keep):
        """The output arrays of one device call, in its argument order: (iterations, the factors' samples, tau, perf, times).
        The sample arrays are page-locked: the device-to-host copy of iteration t overlaps the sweeps of iteration t+1."""
        samples = tuple(_lib.sample_buffer((it,) + s) if keep else None for s in self._shapes())
        return (it,) + samples + (np.zeros(it), np.zeros((it, 3)), np.zeros(it))

    def _run_observed(self, iterations, update, store_samples, expectation, M_test):
        """run() with layout='observed': one device call (bnmf_obs_run / bnmtf_otri_run) runs all iterations -- per iteration the
        half sweeps on the entry lists (between them the tri-factorisation's dense S system from the column list) and the
        end-of-iteration kernel; samples, tau, metrics and times come back as from the dense layout's call."""
        Et = self._check_heldout(M_test)
        if expectation is not None:
            _observed.refuse(self, "run(expectation=)")
        it = int(iterations)
        self._push()
        self._set_heldout(Et)
        self._dev_expect = None
        bufs = self._buffers(it, store_samples and update != _lib.UPDATE_ICM)
        _lib.check(self._entry("run")(self._handle(), it, int(update), *[_lib.ptr(b) for b in bufs[1:]]))
        self._finish_heldout(it)
        return bufs

    def _run_blocked(self, iterations, update, store_samples, expectation, minimum_TN=0.0, icm=False):
        """run() of a model wider than 64 columns: the blocks' half sweeps in turn (_blocked.py); tau by the update rule's own
        law -- a Gamma(alpha_s, beta_s) draw keyed like the single-handle loop's (seed, iteration); mode updates (the deterministic
        harness) take its mean, ICM the Gamma mode (nmf_icm.py:137, nmtf_icm.py:160)."""
        from .distributions import gamma_draw
        it = int(iterations)
        self._push()
        blocks = self._blocks
        shapes = self._shapes()
        samples = [np.zeros((it,) + s, dtype=np.float32) if store_samples else None for s in shapes]
        self._dev_expect = None
        self._host_expect = None              # (a run without expectation= leaves no means of an earlier chain behind)
        acc = None
        if expectation is not None:
            burn_in, thinning = int(expectation[0]), int(expectation[1])
            assert 0 <= burn_in < it and thinning >= 1, "expectation=(burn_in, thinning) needs 0 <= burn_in < iterations, thinning >= 1"
            acc = {"sums": [np.zeros(s) for s in shapes], "tau": 0.0, "n": 0, "sel": set(range(burn_in, it, thinning))}
        alpha_s = self.alpha_s()
        if not self._BLOCKS_KEEP_STATE:
            blocks._prepare()

        def tau_rule(iteration, sse):
            beta_s = self.beta + 0.5 * sse
            if icm:
                return (alpha_s - 1.0) / beta_s
            if update == _lib.UPDATE_MODE:          # the deterministic harness: the mean, as the single-handle loop takes it (csrc finish_kernel)
                return alpha_s / beta_s
            return gamma_draw(alpha_s, beta_s, seed=self._seed, it=iteration, device=self._device)

        def store(i, *factors):
            for all_f, f in zip(samples, factors):
                all_f[i] = f

        def each(i, *state):
            if i in acc["sel"]:
                for s, f in zip(acc["sums"], state[:-1]):
                    s += f
                acc["tau"] += state[-1]; acc["n"] += 1

        taus, perf, times = blocks.run(it, update, tau_rule, minimum_TN=minimum_TN, store=store if store_samples else None,
                                       each=each if acc is not None else None)
        if it > 0:
            for n, f in zip(self._FACTORS + ("tau",), blocks.last):
                setattr(self, n, f)
            if self._BLOCKS_KEEP_STATE:
                self._device_state = (None,) + tuple(f.copy() for f in self._factors()) + (float(self.tau),)
        if acc is not None and acc["n"] > 0:
            self._host_expect = ((burn_in, thinning),) + tuple(s / acc["n"] for s in acc["sums"]) + (acc["tau"] / acc["n"],)
        return self._record(it, samples, store_samples, taus, perf, times)

    def _run_prepare(self, iterations, store_samples, expectation):
        """State on the device, expectation switch, output arrays of one run() call: run() in two halves, so that
        bnmtf_amd.run_many can put many models' device part into one call."""
        self._refuse_if_observed("run_many")
        it = int(iterations)
        self._push()
        self._set_expectation(expectation, it)
        return self._buffers(it, store_samples)

    def _run_finish(self, bufs, store_samples, state=None):
        if state is None:
            self._pull()
        else:                       # (run_many fetched the final states of the whole batch with one synchronisation)
            self._take_state(state[:-1], float(state[-1][0]))
        # the samples are what the device drew: fp32 (the reference's arrays are fp64; every reduction below sums in fp64)
        return self._record(bufs[0], bufs[1:-3], store_samples, *bufs[-3:])

    def _record(self, it, samples, store_samples, taus, perf, times):
        """all_<factor>, all_tau, all_times, all_performances of a run(), and what run() returns."""
        for n, a, s in zip(self._FACTORS, samples, self._shapes()):
            setattr(self, "all_" + n, a if store_samples else np.zeros((0,) + s))
        self._record_iterations(it, taus, perf, times)
        return tuple(getattr(self, "all_" + n) for n in self._FACTORS) + (self.all_tau,)

    def _record_iterations(self, it, taus, perf, times):
        self.all_tau = taus
        self.all_times = list(times)
        self.all_performances = performances(perf)
        if self.verbose:
            for i in range(it):
                print("Iteration %s. MSE: %s. R^2: %s. Rp: %s." % (i + 1, perf[i, 0], perf[i, 1], perf[i, 2]))

    # -- posterior means ----------------------------------------------------------
    def _device_expectation(self, burn_in, thinning):
        if self._blocks is not None:           # (the blocked run keeps the posterior sums on the host)
            he = getattr(self, "_host_expect", None)
            if he is not None and he[0] == (int(burn_in), int(thinning)) and len(getattr(self, "all_" + self._FACTORS[0], ())) == 0:
                return self._asb(he[1:-1]) + (he[-1],)
            return None
        return super(GibbsSampler, self)._device_expectation(burn_in, thinning)

    def approx_expectation(self, burn_in, thinning):
        """bnmf_gibbs_optimised.py:182-187, bnmtf_gibbs_optimised.py:216-223: from the device's sums when the last run()
        accumulated them, else from the stored samples (host fp64, accepts lists)."""
        dev = self._device_expectation(burn_in, thinning)
        if dev is not None:
            return tuple(x for x in dev if x is not None)
        stored = [getattr(self, "all_" + n) for n in self._FACTORS]
        indices = range(burn_in, len(stored[0]), thinning)
        means = tuple(np.array([a[i] for i in indices], dtype=np.float64).sum(axis=0) / float(len(indices)) for a in stored)
        exp_tau = sum([self.all_tau[i] for i in indices]) / float(len(indices))
        return means + (exp_tau,)

    # -- metrics ------------------------------------------------------------------
    def _metric_sums(self, M_pred, A, S, B):
        if self._layout == 'observed':          # the list-metric kernel: the host turns the mask into a list
            return self._OBSERVED["metric_sums"](self, M_pred, *self._own(A, S, B))
        if self._blocks is not None:
            if M_pred is not None:
                check_binary(M_pred, "M_pred")
            return self._blocks.metric_sums(M_pred, *self._own(A, S, B))
        return super(GibbsSampler, self)._metric_sums(M_pred, A, S, B)

    def _metrics(self, M_pred, factors):
        """MSE / R^2 / Rp of the product of `factors` over M_pred (None: the training entries); the product and the masked sums
        run on the device in fp64."""
        return metrics_from_sums(self._metric_sums(M_pred, *self._asb(factors)))

    def predict(self, M_pred, burn_in, thinning):
        """bnmf_gibbs_optimised.py:191-197, bnmtf_gibbs_optimised.py:226-232."""
        return self._metrics(M_pred, self.approx_expectation(burn_in, thinning)[:-1])

    def predict_while_running(self):
        """:199-204, :234-239."""
        return self._metrics(None, self._factors())

    def _n_parameters(self):
        return sum(rows * columns for rows, columns in self._shapes())

    def quality(self, metric, burn_in, thinning):
        """:227-245, :262-280."""
        return information_criterion(metric, lambda: self.approx_expectation(burn_in, thinning), self.log_likelihood,
                                     lambda *exp: self._metrics(None, exp[:-1])['MSE'], self._n_parameters(), self.size_Omega)

    def _log_likelihood(self, factors, tau):
        """:247-251, :282-285."""
        s = self._metric_sums(None, *self._asb(factors))
        sse = s[2] - 2.0 * s[5] + s[4]
        return self.size_Omega / 2. * (math.log(tau) - math.log(2 * math.pi)) - tau / 2. * sse

    # Parameters of the conditional posterior of tau, evaluated on the device
    def alpha_s(self):
        return self.alpha + self.size_Omega / 2.0

    def beta_s(self):
        """bnmf_gibbs_optimised.py:164-165, bnmtf_gibbs_optimised.py:192-193."""
        if self._blocks is not None or self._layout == 'observed':           # from the full-width masked SSE
            s = self._metric_sums(None, *self._asb([np.asarray(f, dtype=float) for f in self._factors()]))
            return self.beta + 0.5 * (s[2] - 2.0 * s[5] + s[4])
        self._push()
        out = C.c_double()
        _lib.check(_lib.lib().bnmtf_beta_s(self._handle(), C.byref(out)))
        return out.value


class ICMRules(object):
    """Iterated Conditional Modes on a sampler class (nmf_icm.py, nmtf_icm.py), ahead of it in the MRO: run() with the ICM update
    rule and minimum_TN, and predict / quality / log_likelihood of the point estimate the model holds."""

    def run(self, iterations, minimum_TN=0., *, M_test=None):
        """nmf_icm.py:114-150, nmtf_icm.py:132-173.  One device call runs all iterations; returns None like the reference.
        M_test: the held-out metrics of the point estimate every iteration ends with, in all_performances_test (see
        GibbsSampler.run)."""
        if self._layout == 'observed':          # (the ICM rules on the observed-entry kernels)
            Et = self._check_heldout(M_test)
            _lib.check(_lib.lib().bnmtf_set_minimum_tn(self._handle(), float(minimum_TN)))
            bufs = self._run_observed(iterations, _lib.UPDATE_ICM, False, None, Et)
            return self._finish_icm(bufs[0], *bufs[-3:])
        Mt = self._check_heldout(M_test)
        it = int(iterations)
        if self._blocks is not None:            # ranks above 64: blocks (_blocked.py), the same updates with the Gamma mode for tau
            self._run_blocked(it, _lib.UPDATE_ICM, False, None, minimum_TN=float(minimum_TN), icm=True)
            return
        self._push()
        self._set_heldout(Mt)
        bufs = self._buffers(it, False)
        _lib.check(_lib.lib().bnmtf_set_minimum_tn(self._handle(), float(minimum_TN)))
        _lib.check(self._entry("run")(self._handle(), it, _lib.UPDATE_ICM, *[_lib.ptr(b) for b in bufs[1:]]))
        self._finish_heldout(it)
        return self._finish_icm(it, *bufs[-3:])

    def _finish_icm(self, it, taus, perf, times):
        """Behind the device call of run(), either layout: the point estimate and the per-iteration records."""
        self._pull()
        self._record_iterations(it, taus, perf, times)

    def predict(self, M_pred):
        """nmf_icm.py:173-178, nmtf_icm.py:218-223: metrics of the current point estimate on M_pred."""
        return self._metrics(M_pred, self._factors())

    def quality(self, metric):
        """:201-217, :246-264."""
        return information_criterion(metric, tuple, self.log_likelihood, lambda: self._metrics(None, self._factors())['MSE'],
                                     self._n_parameters(), self.size_Omega)

    def log_likelihood(self):
        """:219-222, :266-269."""
        return self._log_likelihood(self._factors(), self.tau)
