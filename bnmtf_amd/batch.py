"""Independent models in one device call.

    bnmtf_amd.run_many(models, iterations)      # every model ends as if its own run(iterations) had been called

The reference fits the candidates of a model search -- folds x ranks x restarts -- one after the other
(code/cross_validation/line_search_cross_validation.py:54-131, line_search_bnmf.py:53-76) or in a process pool
(parallel_matrix_cross_validation.py:40-74).  Small BNMF and BNMTF Gibbs models run on the device as ONE block each
(csrc/kernel_small.hip), so a list of them is one launch per kind; models that do not qualify are run in turn.  Variational models
(bnmf_vb_optimised, any size its 8-wave kernels serve) walk their iterations in lock-step: every kernel of an iteration is ONE
launch for all of them (csrc/many.h, api_many.inc: bnmf_vb_run_many), each model ending with the bits of its own run().  So do the
variational tri-factorisations (bnmtf_vb_optimised: their run(iterations)), of any shapes and ranks together: every launch site of
an iteration is ONE launch for all of them (csrc/api_trivb_many.inc: bnmtf_vb_run_many); their update orders are drawn from
Python's `random` model by model, in list order, before the device call -- as the models' own run() calls one after the other
would draw them.  Models wider than 64 columns (column blocks, _blocked.py: several handles per model) of any of these kinds are
run by their own run().
The non-probabilistic models (nmf_np.NMF, nmtf_np.NMTF: their run(iterations)) walk their iterations in lock-step too, NMF and
NMTF of any shapes and ranks together: every launch site of an iteration is ONE launch for all of them (csrc/api_np_many.inc:
bnmtf_np_run_many).  ICM models (nmf_icm: their own run(), update rule and minimum_TN) are not taken: ReplicaPool runs them one by one."""
import ctypes as C
import time

import numpy as np

from . import _lib


def takes(model):
    """Is `model` one that run_many fits as its own run() would?  (A Gibbs class itself -- or a subclass that keeps its run().)"""
    return _kind(model) is not None


def _kind(model):
    from .bnmf_gibbs import bnmf_gibbs_optimised
    from .bnmtf_gibbs import bnmtf_gibbs_optimised
    if isinstance(model, bnmf_gibbs_optimised) and type(model).run is bnmf_gibbs_optimised.run:
        return "bnmf"
    if isinstance(model, bnmtf_gibbs_optimised) and type(model).run is bnmtf_gibbs_optimised.run:
        return "bnmtf"
    from .bnmf_vb import bnmf_vb_optimised
    if isinstance(model, bnmf_vb_optimised) and type(model).run is bnmf_vb_optimised.run:
        return "vb"
    from .bnmtf_vb import bnmtf_vb_optimised
    if isinstance(model, bnmtf_vb_optimised) and type(model).run is bnmtf_vb_optimised.run:
        return "trivb"
    from .nmf_np import NMF
    from .nmtf_np import NMTF
    # (taken once initialise() has given it its factors: run() of a model without them fails its assertion, run_many refuses it)
    if isinstance(model, NMF) and type(model).run is NMF.run and all(hasattr(model, f) for f in "UV"):
        return "np"
    if isinstance(model, NMTF) and type(model).run is NMTF.run and all(hasattr(model, f) for f in "FSG"):
        return "np"
    return None


def run_many(models, iterations, update='draw', store_samples=True, expectation=None, orders=None):
    """run(iterations, update, store_samples, expectation) of every model in `models` (bnmf_gibbs_optimised and / or
    bnmtf_gibbs_optimised instances), with the models of the one-launch path that share a device and a kind sharing a single
    launch; bnmf_vb_optimised instances (their run(iterations)): the models of a device walk their iterations in lock-step, one
    launch per kernel for all of them (csrc/api_many.inc).  A Gibbs model wider than 64 columns (column blocks) is run by its own
    run(iterations, update, store_samples, expectation).  bnmtf_vb_optimised instances (their run(iterations)): the models of a
    device walk their iterations in lock-step, one launch per launch site for all of them (csrc/api_trivb_many.inc); their update
    orders are drawn with _draw_orders, model by model in list order, before the device call -- Python's `random` ends as after
    their run() calls one after the other.  orders (optional): a list as long as `models` whose entry for a bnmtf_vb_optimised is
    the [iterations][K L + K + L] orders of its run(iterations, orders) (None: drawn here), None for every other model.  NMF / NMTF
    instances (their run(iterations); update, store_samples and expectation do not apply): the models of a device walk their
    iterations in lock-step, one launch per launch site for all of them (csrc/api_np_many.inc).  Returns the list of the runs'
    results, in the order of `models`."""
    models = list(models)
    if not models:
        return []
    if not all(takes(m) for m in models):
        # (nmf_icm inherits the Gibbs class and overrides run(): its update rule, minimum_TN and Gamma mode are not what the
        # batched entry point runs -- it would come back fitted by Gibbs draws)
        raise TypeError("run_many takes models whose run() is bnmf_gibbs_optimised.run, bnmtf_gibbs_optimised.run, "
                        "bnmf_vb_optimised.run, bnmtf_vb_optimised.run, NMF.run or NMTF.run, the last two initialised (got %s)"
                        % sorted({type(m).__name__ for m in models if not takes(m)}))
    if orders is not None and len(orders) != len(models):
        raise ValueError("run_many: %d orders for %d models" % (len(orders), len(models)))
    if int(iterations) == 0:                  # run(0) changes nothing (the C entry points return before they fill the final states)
        return [None for _ in models]
    out = [None] * len(models)
    upd = _lib.UPDATE_MODE if update == 'mode' else _lib.UPDATE_DRAW
    tri = [i for i, m in enumerate(models) if _kind(m) == "trivb"]
    # (the shuffles of every tri-factorisation first, in list order: what their run() calls one after the other draw)
    tri_orders = [models[i]._draw_orders(int(iterations)) if orders is None or orders[i] is None
                  else np.ascontiguousarray(orders[i], dtype=np.int32) for i in tri]
    _run_many_vb([m for m in models if _kind(m) == "vb"], int(iterations))
    _run_many_trivb([models[i] for i in tri], tri_orders, int(iterations))
    _run_many_np([m for m in models if _kind(m) == "np"], int(iterations))
    for i, m in enumerate(models):
        if _kind(m) in ("bnmf", "bnmtf") and m._blocks is not None:
            out[i] = m.run(iterations, update, store_samples, expectation)
    for kind in ("bnmf", "bnmtf"):
        idx = [i for i, m in enumerate(models) if _kind(m) == kind and m._blocks is None]
        if not idx:
            continue
        ms = [models[i] for i in idx]
        bufs = [m._run_prepare(iterations, store_samples, expectation) for m in ms]
        n = len(ms)
        arr = lambda xs: (C.c_void_p * n)(*[None if x is None else x.ctypes.data for x in xs])
        hs = (C.c_void_p * n)(*[m._handle().value for m in ms])
        if kind == "bnmf":
            states = [(np.zeros((m.I, m.K)), np.zeros((m.J, m.K)), np.zeros(1)) for m in ms]      # what every model ends with
            _lib.check(_lib.lib().bnmf_gibbs_run_many(hs, n, bufs[0][0], upd, arr([b[1] for b in bufs]), arr([b[2] for b in bufs]),
                                                      arr([b[3] for b in bufs]), arr([b[4] for b in bufs]), arr([b[5] for b in bufs]),
                                                      arr([s[0] for s in states]), arr([s[1] for s in states]), arr([s[2] for s in states])))
        else:
            states = [(np.zeros((m.I, m.K)), np.zeros((m.K, m.L)), np.zeros((m.J, m.L)), np.zeros(1)) for m in ms]
            _lib.check(_lib.lib().bnmtf_gibbs_run_many(hs, n, bufs[0][0], upd, arr([b[1] for b in bufs]), arr([b[2] for b in bufs]),
                                                       arr([b[3] for b in bufs]), arr([b[4] for b in bufs]), arr([b[5] for b in bufs]),
                                                       arr([b[6] for b in bufs]),
                                                       arr([s[0] for s in states]), arr([s[1] for s in states]), arr([s[2] for s in states]),
                                                       arr([s[3] for s in states])))
        for i, m, b, st in zip(idx, ms, bufs, states):
            out[i] = m._run_finish(b, store_samples, state=st)
    return out


def _run_many_vb(ms, it):
    """bnmf_vb_optimised.run(it) of every model of `ms` (bnmf_vb_optimised.py:121-153): per device one bnmf_vb_run_many call;
    models wider than 64 columns (column blocks) run on their own."""
    by_device = {}
    for m in ms:
        if m._blocks is not None:
            m.run(it)
        else:
            by_device.setdefault(m._device, []).append(m)
    for group in by_device.values():
        n = len(group)
        for m in group:
            m._push()
        hs = (C.c_void_p * n)(*[m._handle().value for m in group])
        exptau = np.zeros((n, it)); perf = np.zeros((n, it, 3)); terms = np.zeros((n, it, 10)); times = np.zeros((n, it))
        info = np.zeros(2, dtype=np.int32)
        t0 = time.perf_counter()
        _lib.check(_lib.lib().bnmf_vb_run_many(hs, n, it, _lib.ptr(exptau), _lib.ptr(perf), _lib.ptr(terms), _lib.ptr(times), _lib.ptr(info)))
        dt = time.perf_counter() - t0
        for i, m in enumerate(group):
            m._run_finish(it, exptau[i], perf[i], terms[i], times[i])
            m._many_info = (int(info[0]), int(info[1]), dt)     # models that shared launches, argument-list uploads, seconds of the device call


def _run_many_trivb(ms, orders, it):
    """bnmtf_vb_optimised.run(it, orders) of every model of `ms` (bnmtf_vb_optimised.py:160-205) with its orders: per device one
    bnmtf_vb_run_many call."""
    by_device = {}
    for m, o in zip(ms, orders):
        assert o.shape == (it, m.K * m.L + m.K + m.L), (o.shape, it, m.K, m.L)
        by_device.setdefault(m._device, []).append((m, o))
    for group in by_device.values():
        n = len(group)
        for m, _ in group:
            m._push()
        hs = (C.c_void_p * n)(*[m._handle().value for m, _ in group])
        ords = (C.c_void_p * n)(*[o.ctypes.data for _, o in group])
        exptau = np.zeros((n, it)); perf = np.zeros((n, it, 3)); terms = np.zeros((n, it, 10)); times = np.zeros((n, it))
        info = np.zeros(2, dtype=np.int32)
        t0 = time.perf_counter()
        _lib.check(_lib.lib().bnmtf_vb_run_many(hs, n, it, ords, _lib.ptr(exptau), _lib.ptr(perf), _lib.ptr(terms), _lib.ptr(times), _lib.ptr(info)))
        dt = time.perf_counter() - t0
        for i, (m, _) in enumerate(group):
            m._run_finish(it, exptau[i], perf[i], terms[i], times[i])
            m._many_info = (int(info[0]), int(info[1]), dt)     # models that shared launches, argument-list uploads, seconds of the device call


def _run_many_np(ms, it):
    """NMF.run(it) / NMTF.run(it) of every model of `ms` (nmf_np.py:87-107, nmtf_np.py:116-144): per device one bnmtf_np_run_many
    call, NMF and NMTF together."""
    by_device = {}
    for m in ms:
        by_device.setdefault(m._device, []).append(m)
    for group in by_device.values():
        n = len(group)
        for m in group:
            m._run_prepare(it)
        hs = (C.c_void_p * n)(*[m._handle().value for m in group])
        perf = np.zeros((n, it, 3)); idiv = np.zeros((n, it)); times = np.zeros((n, it))
        info = np.zeros(2, dtype=np.int32)
        t0 = time.perf_counter()
        _lib.check(_lib.lib().bnmtf_np_run_many(hs, n, it, _lib.ptr(perf), _lib.ptr(idiv), _lib.ptr(times), _lib.ptr(info)))
        dt = time.perf_counter() - t0
        for i, m in enumerate(group):
            m._run_finish(it, perf[i], idiv[i], times[i])
            m._many_info = (int(info[0]), int(info[1]), dt)     # models that shared launches, argument-list uploads, seconds of the device call
