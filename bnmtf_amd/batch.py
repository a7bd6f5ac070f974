"""Independent models in one device call.

    bnmtf_amd.run_many(models, iterations)      # every model ends as if its own run(iterations) had been called

The reference fits the candidates of a model search -- folds x ranks x restarts -- one after the other
(code/cross_validation/line_search_cross_validation.py:54-131, line_search_bnmf.py:53-76) or in a process pool
(parallel_matrix_cross_validation.py:40-74).  Here a list of them shares launches, in one of two ways:

  one launch      small BNMF and BNMTF Gibbs models run on the device as ONE block each (csrc/kernel_small.hip): the models of a
                  device and a kind are one launch; models that do not qualify are run in turn.
  lock-step       bnmf_vb_optimised, bnmtf_vb_optimised, nmf_np.NMF and nmtf_np.NMTF models (their run(iterations)) walk their
                  iterations together: every launch site of an iteration is ONE launch for the models of a device and a family
                  (csrc/many.h, api_many.inc; the families: _LOCKSTEP), models of any shapes and ranks together, NMF with NMTF.
                  Each model ends with the bits of its own run().

Held-out curves: run_many(..., M_tests=[mask or None per model]) gives every model with a mask the all_performances_test of its own
run(M_test=mask).  In the lock-step families the held-out kernels join the shared launches (list forms of csrc/kernel_heldout.hip,
behind the iteration's last site; models with and without a mask mix, and the argument lists stay the same from the first
iteration on).  The one-launch kernel has no per-iteration hook: a Gibbs model with a mask is run by its own run(M_test=), its
neighbours without one stay in the one-launch batch.  Without M_tests a model that still carries the mask of an earlier
run(M_test=) is refused.

Models wider than 64 columns (column blocks, _blocked.py: several handles per model) are run by their own run().  ICM models
(nmf_icm: their own run(), update rule and minimum_TN) are not taken: ReplicaPool runs them one by one.  A model in column blocks
keeps no held-out record: given a mask it raises the BnmtfError of its run(M_test=)."""
import ctypes as C
import time

import numpy as np

from . import _lib


def takes(model):
    """Is `model` one that run_many fits as its own run() would?  (A Gibbs class itself -- or a subclass that keeps its run().)"""
    return _kind(model) is not None


def _kinds():
    """kind -> (class whose run() run_many stands in for, the attributes an instance must have been given)"""
    from .bnmf_gibbs import bnmf_gibbs_optimised
    from .bnmtf_gibbs import bnmtf_gibbs_optimised
    from .bnmf_vb import bnmf_vb_optimised
    from .bnmtf_vb import bnmtf_vb_optimised
    from .nmf_np import NMF
    from .nmtf_np import NMTF
    # (NMF / NMTF: taken once initialise() has given them their factors -- run() of a model without them fails its assertion)
    return (("bnmf", bnmf_gibbs_optimised, ""), ("bnmtf", bnmtf_gibbs_optimised, ""), ("vb", bnmf_vb_optimised, ""),
            ("trivb", bnmtf_vb_optimised, ""), ("np", NMF, "UV"), ("np", NMTF, "FSG"))


def _kind(model):
    # (the two Gibbs classes share one run(), _sampler.GibbsSampler's: isinstance tells them apart, and `run is cls.run` keeps out a
    # subclass that brings its own -- nmf_icm / nmtf_icm, whose run() is _sampler.ICMRules')
    for kind, cls, needs in _kinds():
        if isinstance(model, cls) and type(model).run is cls.run and all(hasattr(model, f) for f in needs):
            return kind
    return None


def run_many(models, iterations, update='draw', store_samples=True, expectation=None, orders=None, M_tests=None):
    """Every model of `models` (see `takes`) as after its own run(): run(iterations, update, store_samples, expectation) for the
    Gibbs models, run(iterations) for the others (update, store_samples and expectation do not apply to them).  How they share
    launches: the module's docstring.  The update orders of the bnmtf_vb_optimised models are drawn with _draw_orders, model by
    model in list order, before any device call -- Python's `random` ends as after their run() calls one after the other.  orders
    (optional): a list as long as `models` whose entry for a bnmtf_vb_optimised is the [iterations][K L + K + L] orders of its
    run(iterations, orders) (None: drawn here), None for every other model.  M_tests (optional): a list as long as `models`, per
    model None or the held-out mask of its run(..., M_test=) -- validated for all models before any device call; afterwards a model
    with a mask has its all_performances_test, one without has none.  Returns the list of the runs' results, in the order of
    `models`."""
    models = list(models)
    if not models:
        return []
    if not all(takes(m) for m in models):
        # (nmf_icm inherits the Gibbs class and overrides run(): its update rule, minimum_TN and Gamma mode are not what the
        # batched entry point runs -- it would come back fitted by Gibbs draws)
        raise TypeError("run_many takes models whose run() is bnmf_gibbs_optimised.run, bnmtf_gibbs_optimised.run, "
                        "bnmf_vb_optimised.run, bnmtf_vb_optimised.run, NMF.run or NMTF.run, the last two initialised (got %s)"
                        % sorted({type(m).__name__ for m in models if not takes(m)}))
    for i, m in enumerate(models):
        if getattr(m, "_layout", "dense") == 'observed':
            raise _lib.BnmtfError("run_many: model %d has layout='observed' (batched launches and pools take models of the dense "
                                  "layout: run it on its own)" % i)
    if orders is not None and len(orders) != len(models):
        raise ValueError("run_many: %d orders for %d models" % (len(orders), len(models)))
    if M_tests is not None:
        M_tests = list(M_tests)
        if len(M_tests) != len(models):
            raise ValueError("run_many: %d M_tests for %d models" % (len(M_tests), len(models)))
        masks = [m._check_heldout(Mt) for m, Mt in zip(models, M_tests)]      # (every model's, before any device call)
    else:
        for i, m in enumerate(models):
            held = getattr(m, "_heldout", None)
            if held is not None and held[0] is m._h:
                raise _lib.BnmtfError("run_many: model %d has a held-out mask (the M_test of an earlier run()): give run_many its "
                                      "M_tests, or clear the mask with a run() without M_test" % i)
        masks = None
    if int(iterations) == 0:                  # run(0) changes nothing (the C entry points return before they fill the final states)
        return [None for _ in models]
    out = [None] * len(models)
    upd = _lib.UPDATE_MODE if update == 'mode' else _lib.UPDATE_DRAW
    tri = [i for i, m in enumerate(models) if _kind(m) == "trivb"]
    # (the shuffles of every tri-factorisation first, in list order: what their run() calls one after the other draw)
    tri_orders = [models[i]._draw_orders(int(iterations)) if orders is None or orders[i] is None
                  else np.ascontiguousarray(orders[i], dtype=np.int32) for i in tri]
    of = lambda idx: None if masks is None else [masks[i] for i in idx]
    for kind in ("vb", "trivb", "np"):
        idx = tri if kind == "trivb" else [i for i, m in enumerate(models) if _kind(m) == kind]
        _run_lockstep(kind, [models[i] for i in idx], int(iterations), tri_orders if kind == "trivb" else None, masks=of(idx))
    alone = lambda i: models[i]._blocks is not None or (masks is not None and masks[i] is not None)
    for i, m in enumerate(models):
        if _kind(m) in ("bnmf", "bnmtf") and alone(i):       # (a mask: the one-launch kernel has no per-iteration hook)
            out[i] = m.run(iterations, update, store_samples, expectation, M_test=None if masks is None else masks[i])
    for kind in ("bnmf", "bnmtf"):
        idx = [i for i, m in enumerate(models) if _kind(m) == kind and not alone(i)]
        if not idx:
            continue
        ms = [models[i] for i in idx]
        bufs = [m._run_prepare(iterations, store_samples, expectation) for m in ms]
        if masks is not None:
            for m in ms:
                m._set_heldout(None)          # (a mask left by an earlier run(M_test=): off the handle)
        n = len(ms)
        arr = lambda xs: (C.c_void_p * n)(*[None if x is None else x.ctypes.data for x in xs])
        hs = (C.c_void_p * n)(*[m._handle().value for m in ms])
        states = [tuple(np.zeros(s) for s in m._shapes()) + (np.zeros(1),) for m in ms]      # what every model ends with: its factors, tau
        # the entry point takes, per output array of run() and then per array of the final state, the models' pointers: both in
        # the order of the class's factor tuple (_sampler.py)
        outputs = zip(*[b[1:] for b in bufs])
        entry = getattr(_lib.lib(), ms[0]._DENSE["run_many"])
        _lib.check(entry(hs, n, bufs[0][0], upd, *[arr(col) for col in outputs], *[arr(col) for col in zip(*states)]))
        for i, m, b, st in zip(idx, ms, bufs, states):
            out[i] = m._run_finish(b, store_samples, state=st)
    return out


# The lock-step families: kind -> (what puts a model's state on the device, the C entry point, the trailing shapes of its
# model-major [models][iterations] output arrays, in the order the entry point and the models' _run_finish take them; the batch's
# clock follows them).  bnmf_vb_optimised.py:121-153, bnmtf_vb_optimised.py:160-205, nmf_np.py:87-107, nmtf_np.py:116-144.
_VARIATIONAL = (lambda m, it: m._push(), None, ((), (3,), (10,)))                      # exptau, perf, the ELBO's terms; the entry point:
_LOCKSTEP = {                                                                          # the run_many of the models' _DENSE table
    "vb": _VARIATIONAL,
    "trivb": _VARIATIONAL,
    "np": (lambda m, it: m._run_prepare(it), "bnmtf_np_run_many", ((3,), ())),         # perf, the I-divergence
}


def _run_lockstep(kind, ms, it, orders=None, masks=None):
    """run(it) of every model of `ms`, all of one lock-step family: per device one call of the family's entry point (orders: per
    model the update orders its run(it, orders) would take, for the family whose entry point takes them); models in column blocks
    run on their own.  masks: None (the handles are left as they are), or per model None or the checked mask of its
    run(it, M_test=) -- set on the handle (None: cleared) before the call, finished into all_performances_test behind it."""
    prepare, entry, shapes = _LOCKSTEP[kind]
    by_device = {}
    for i, m in enumerate(ms):
        if getattr(m, "_blocks", None) is not None:
            m.run(it)                     # (in column blocks no mask passes _check_heldout)
        else:
            by_device.setdefault(m._device, []).append(i)
    for idx in by_device.values():
        group = [ms[i] for i in idx]
        n = len(group)
        for i, m in zip(idx, group):
            prepare(m, it)
            if masks is not None:
                m._set_heldout(masks[i])
        args = [(C.c_void_p * n)(*[m._handle().value for m in group]), n, it]
        if orders is not None:
            for i in idx:
                assert orders[i].shape == (it, ms[i].K * ms[i].L + ms[i].K + ms[i].L), (orders[i].shape, it, ms[i].K, ms[i].L)
            args.append((C.c_void_p * n)(*[orders[i].ctypes.data for i in idx]))
        outs = [np.zeros((n, it) + shape) for shape in shapes] + [np.zeros((n, it))]
        info = np.zeros(2, dtype=np.int32)
        t0 = time.perf_counter()
        _lib.check(getattr(_lib.lib(), entry or group[0]._DENSE["run_many"])(*args, *[_lib.ptr(o) for o in outs], _lib.ptr(info)))
        dt = time.perf_counter() - t0
        for j, m in enumerate(group):
            if masks is not None:
                m._finish_heldout(it)
            m._run_finish(it, *[o[j] for o in outs])
            m._many_info = (int(info[0]), int(info[1]), dt)     # models that shared launches, argument-list uploads, seconds of the device call
