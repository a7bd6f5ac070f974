"""layout='observed' of bnmf_gibbs_optimised / nmf_icm, of bnmtf_gibbs_optimised / nmtf_icm and of nmf_np.NMF / nmtf_np.NMTF,
bnmf_vb_observed and bnmtf_vb_observed: the host side of the observed-entry layout.

The device keeps the residual R_ij - U_i.V_j -- for the non-probabilistic models the product P_ij itself -- on the OBSERVED entries
(csrc/kernel_obs.hip, kernel_obs_vb.hip, kernel_obs_np.hip), so cost and device memory follow the number of observed entries: the
layout for matrices that are mostly missing.  The three classes on the two-factor handle (bnmf_gibbs_optimised, nmf_icm,
bnmf_vb_observed) take the matrix as dense NumPy arrays R, M or as an Entries (entries.py: lists, nothing of size I x J on the
host either), and an Entries as run()'s M_test for a held-out curve; for the other classes R and M stay dense at the Python
boundary.  This module turns either form into the entry lists the library takes, owns the bnmtf_obs_create / bnmtf_otri_create /
bnmtf_onp_create handle of a model and states what the layout does not run."""
import ctypes as C

import numpy as np

from . import _lib
from ._base import check_binary, check_R_M
from .entries import Entries

LAYOUTS = ('dense', 'observed')
MAX_RANK = 256          # BNMTF_OBS_MAX_RANK: nothing ties a rank to a lane, one handle takes them all
MAX_RANK_TRI = 32       # BNMTF_OTRI_MAX_RANK: the tri-factorisation's S step is the dense K.L x K.L system, one 32 x 32 tile per column Gram


def check_layout(layout):
    assert layout in LAYOUTS, "Unknown layout: %s. Should be 'dense' or 'observed'." % (layout,)


# what the layout does not run -> why: every refusal's one text
REFUSALS = {
    "set_sweep_path": "it has one sweep kernel; BNMTF_OBS_LONG=1 forces its long form",
    "set_small_path": "the one-launch path belongs to the dense layout",
    "set_profiling": "the per-kernel event brackets belong to the dense layout",
    "masked_sums": "the sums over the missing entries belong to the dense layout's matrix-core product",
    "column_maxima": "the fixed-point grid belongs to the dense layout's matrix-core product",
    "run(M_test=)": "a 0/1 mask belongs to the dense layout: pass the held-out entries with their values as an Entries",
    "run(expectation=)": "the posterior sums on the device belong to the dense layout; approx_expectation averages the stored samples",
    "run_many": "batched launches take models of the dense layout",
}

HELDOUT_TWO_FACTOR = ("held-out curves on this layout are built for the two-factor models bnmf_gibbs_optimised, nmf_icm and "
                      "bnmf_vb_observed, which take the held-out entries as an Entries; use predict(M_test) after the run")


def refuse(model, what, why=None):
    raise _lib.BnmtfError("%s: %s is not available with layout='observed' (%s)" % (type(model).__name__, what, REFUSALS[what] if why is None else why))


class ObservedLayout(object):
    """What a model on the layout answers without the device, and what it refuses before any device call.  Ahead of the dense
    class in the MRO of every class that can run layout='observed': a method answers when self._layout == 'observed' and hands on
    to the dense class otherwise (the Gibbs / ICM classes take either layout; the two *_vb_observed classes only this one)."""

    def _refuse_if_observed(self, what):
        if self._layout == 'observed':
            refuse(self, what)

    def set_sweep_path(self, fast=True):
        self._refuse_if_observed("set_sweep_path")
        return super(ObservedLayout, self).set_sweep_path(fast)

    def set_small_path(self, on='auto'):
        self._refuse_if_observed("set_small_path")
        return super(ObservedLayout, self).set_small_path(on)

    def set_profiling(self, enable=True, kernel=None, every=1):
        self._refuse_if_observed("set_profiling")
        return super(ObservedLayout, self).set_profiling(enable, kernel, every)

    def is_small(self):
        return False if self._layout == 'observed' else super(ObservedLayout, self).is_small()

    def omega_counts(self):
        if self._layout != 'observed':
            return super(ObservedLayout, self).omega_counts()
        rows, cols, _ = entries_of(self)
        return len(rows), np.bincount(rows, minlength=self.I).astype(np.uint32), np.bincount(cols, minlength=self.J).astype(np.uint32)

    def _check_heldout(self, M_test):
        """run()'s M_test on this layout, before any device call: None, or an Entries of the model's shape with at least one entry
        (it may overlap the training entries); a dense mask is the dense layout's."""
        if self._layout != 'observed':
            return super(ObservedLayout, self)._check_heldout(M_test)
        if M_test is None:
            return None
        if hasattr(self, "L"):
            refuse(self, "run(M_test=)", HELDOUT_TWO_FACTOR)
        if not isinstance(M_test, Entries):
            refuse(self, "run(M_test=)")
        assert M_test.shape == (self.I, self.J), "Input matrix R is not of the same size as the held-out entries M_test: %s and %s respectively." \
            % ((self.I, self.J), M_test.shape)
        assert len(M_test) > 0, "The held-out entries M_test are empty."
        return M_test

    def _set_heldout(self, Et):
        """The list of _check_heldout onto the handle (bnmtf_set_heldout_entries) -- or, with None, a list left there by an
        earlier run() off it."""
        if self._layout != 'observed':
            return super(ObservedLayout, self)._set_heldout(Et)
        held = getattr(self, "_heldout", None)
        if Et is None:
            if held is not None and held[0] is self._h:
                _lib.check(_lib.lib().bnmtf_set_heldout_entries(self._handle(), C.c_uint64(0), None, None, None))
            self._heldout = None
            if hasattr(self, "all_performances_test"):
                del self.all_performances_test
            return
        vals = Et.values32()
        _lib.check(_lib.lib().bnmtf_set_heldout_entries(self._handle(), C.c_uint64(len(Et)), _lib.ptr(Et.rows), _lib.ptr(Et.cols), _lib.ptr(vals)))
        self._heldout = (self._h, len(Et))


class ObservedVB(ObservedLayout):
    """... and of the two variational classes, ahead of the dense class (a _variational.Variational) in their MRO: the layout's
    handle and list metric, as the class's _OBSERVED table names them, and the hooks of the dense layout's masked product.
    Everything else -- the q hand-over too -- is the dense class's code on the _OBSERVED entry points."""

    def _handle(self):
        if self._h is None:
            self._h = self._OBSERVED["create"](self)
        return self._h

    def _metric_sums(self, M_pred, A, S, B):
        return self._OBSERVED["metric_sums"](self, M_pred, *self._own(A, S, B))

    def masked_sums(self, which):
        refuse(self, "masked_sums")

    def column_maxima(self, which):
        refuse(self, "column_maxima")


class ObservedNP(object):
    """The layout switch of nmf_np.NMF and nmtf_np.NMTF, ahead of nmf_np.NPDevice in their MRO as ObservedLayout is ahead of
    DeviceModel: with self._layout == 'observed' the handle is bnmtf_onp_create's, the device calls are the bnmtf_onp_* ones and
    the sums of predict() / compute_I_div() come from the list metric; everything else -- initialise, run, train, the single
    updates, the push-only-if-changed hand-over -- is NPDevice's own code.  With 'dense' every method hands on."""

    def _init_layout(self, layout, world):
        """The constructor's first step: the keyword, and what the layout does not run, before anything touches a device."""
        check_layout(layout)
        self._layout = layout
        if layout == 'observed':
            for name in ("K", "L"):
                v = getattr(self, name, None)
                if v is not None and not (1 <= int(v) <= MAX_RANK):
                    raise _lib.BnmtfError("%s: %s = %s is outside what layout='observed' runs (1 <= %s <= %d on one handle; "
                                          "DESIGN.md section 2.7, limits)" % (type(self).__name__, name, v, name, MAX_RANK))
            if int(world) != 1:
                refuse(self, "world = %s" % world, "the observed-entry layout runs on one GPU: world = 1")

    def _handle(self):
        if self._layout != 'observed':
            return super(ObservedNP, self)._handle()
        if self._h is None:
            Mb = check_binary(self.M, "M")
            rows, cols, vals = entry_list(self.R, Mb)
            self._train_list = (rows, cols, vals)
            h = C.c_void_p()
            _lib.check(_lib.lib().bnmtf_onp_create(int(self.I), int(self.J), int(self.K), int(getattr(self, "L", 0)), C.c_uint64(len(rows)),
                                                   _lib.ptr(rows), _lib.ptr(cols), _lib.ptr(vals), int(self._device), C.byref(h)))
            self._h = h
        return self._h

    def _entry(self, name):
        """The bnmtf_onp_* call that stands in for the dense layout's `name` (the two-factor names: S is null, V is `which` 2)."""
        if self._layout != 'observed':
            return super(ObservedNP, self)._entry(name)
        lib = _lib.lib              # (resolved at the call: naming an entry point is no device call)
        return {"bnmf_np_run": lambda *a: lib().bnmtf_onp_run(*a), "bnmtf_np_run": lambda *a: lib().bnmtf_onp_run(*a),
                "bnmf_np_set_state": lambda h, U, V: lib().bnmtf_onp_set_state(h, U, None, V),
                "bnmtf_np_set_state": lambda *a: lib().bnmtf_onp_set_state(*a),
                "bnmf_np_get_state": lambda h, U, V: lib().bnmtf_onp_get_state(h, U, None, V),
                "bnmtf_np_get_state": lambda *a: lib().bnmtf_onp_get_state(*a),
                "bnmf_np_update": lambda h, which, k: lib().bnmtf_onp_update(h, 2 * which, k, k),
                "bnmtf_np_update": lambda *a: lib().bnmtf_onp_update(*a)}[name]

    def _check_heldout(self, M_test):
        if self._layout != 'observed':
            return super(ObservedNP, self)._check_heldout(M_test)
        if M_test is not None:
            refuse(self, "run(M_test=)", HELDOUT_TWO_FACTOR)
        return None

    def _sums(self, M_pred=None):
        """The eight sums of metrics_from_np_sums over M_pred (None: the training entries) for the factors the device holds."""
        if self._layout != 'observed':
            return super(ObservedNP, self)._sums(M_pred)
        self._push()
        out = np.zeros(8)
        if M_pred is None:
            _lib.check(_lib.lib().bnmtf_onp_metrics(self._handle(), C.c_uint64(0), None, None, None, _lib.ptr(out)))
            return out
        Mp = np.asarray(M_pred)
        assert Mp.shape == (self.I, self.J), "M_pred has the wrong shape: %s instead of %s." % (Mp.shape, (self.I, self.J))
        check_binary(Mp, "M_pred")
        rows, cols, vals = entry_list(self.R, Mp)
        if len(rows):                           # (an empty mask: the dense layout's sums of nothing)
            _lib.check(_lib.lib().bnmtf_onp_metrics(self._handle(), C.c_uint64(len(rows)), _lib.ptr(rows), _lib.ptr(cols), _lib.ptr(vals), _lib.ptr(out)))
        return out


def check_constructor(model, world):
    """What the layout does not run, said at construction: several GPUs, and ranks beyond one handle's (no column blocks here)."""
    if not (1 <= int(model.K) <= MAX_RANK):
        raise _lib.BnmtfError("%s: K = %s is outside what layout='observed' runs (1 <= K <= %d on one handle; DESIGN.md section 2.7, limits)"
                              % (type(model).__name__, model.K, MAX_RANK))
    if world != 1:
        refuse(model, "world = %s" % world, "the observed-entry layout runs on one GPU: world = 1")


def check_constructor_tri(model, world):
    """The same for the tri-factorisation: K and L within the dense S system's one tile per Gram (no blocks of S on this layout)."""
    for name, v in (("K", model.K), ("L", model.L)):
        if not (1 <= int(v) <= MAX_RANK_TRI):
            raise _lib.BnmtfError("%s: %s = %s is outside what layout='observed' runs (1 <= K, L <= %d: the S step is the dense K.L x K.L "
                                  "system, one 32 x 32 tile per column Gram, and this layout has no blocks of S; DESIGN.md section 2.7, limits)"
                                  % (type(model).__name__, name, v, MAX_RANK_TRI))
    if world != 1:
        refuse(model, "world = %s" % world, "the observed-entry layout runs on one GPU: world = 1")


def build_lists(I, J, rows, cols, values):
    """The row list and the column list the device holds for the entries (rows, cols, values), given in any order: the library's
    own host builder (bnmtf_obs_build_lists, the first half of bnmtf_obs_create; no GPU needed).  Returns row_ptr [I + 1],
    row_col, row_val, col_ptr [J + 1], col_row, col_val; raises BnmtfError for what bnmtf_obs_create refuses."""
    rows = np.ascontiguousarray(rows, dtype=np.int32); cols = np.ascontiguousarray(cols, dtype=np.int32)
    values = np.ascontiguousarray(values, dtype=np.float32)
    n = len(rows)
    out = dict(row_ptr=np.zeros(I + 1, dtype=np.uint32), row_col=np.zeros(n, dtype=np.uint32), row_val=np.zeros(n, dtype=np.float32),
               col_ptr=np.zeros(J + 1, dtype=np.uint32), col_row=np.zeros(n, dtype=np.uint32), col_val=np.zeros(n, dtype=np.float32))
    _lib.check(_lib.lib().bnmtf_obs_build_lists(int(I), int(J), C.c_uint64(n), _lib.ptr(rows), _lib.ptr(cols), _lib.ptr(values),
                                                *[_lib.ptr(out[k]) for k in ("row_ptr", "row_col", "row_val", "col_ptr", "col_row", "col_val")]))
    return out


def entry_list(R, Mask):
    """(rows, cols, values) of the entries of the 0/1 matrix Mask in row-major order: what the library's list calls take."""
    Mb = np.asarray(Mask) != 0
    rows, cols = np.nonzero(Mb)
    return (np.ascontiguousarray(rows, dtype=np.int32), np.ascontiguousarray(cols, dtype=np.int32),
            np.ascontiguousarray(np.asarray(R)[Mb], dtype=np.float32))


def take_R_M(model, R, M, layout='observed'):
    """The constructor's first step on the three classes that take either form: R and M onto the model with check_R_M's
    assertions, and ((I, J), size_Omega).  Dense arrays as ever; an Entries (then M is None) only with layout='observed'."""
    if isinstance(R, Entries):
        if layout != 'observed':
            raise _lib.BnmtfError("%s: an Entries is taken with layout='observed'; layout='dense' takes R and M as dense arrays "
                                  "(Entries.to_dense() gives them)" % type(model).__name__)
        if M is not None:
            raise _lib.BnmtfError("%s: with an Entries as R the mask is the list itself: M must be None" % type(model).__name__)
        model.R, model.M = R, None
        R.check_rows_columns()
        return R.shape, len(R)
    model.R = np.array(R, dtype=float)
    model.M = np.array(M, dtype=float)
    check_R_M(model.R, model.M)
    return model.R.shape, model.M.sum()


def refuse_entries(model, *given):
    """The classes that do not take an Entries yet say so at construction."""
    if any(isinstance(g, Entries) for g in given):
        raise _lib.BnmtfError("%s: an Entries is taken by the models on the two-factor handle of layout='observed' only "
                              "(bnmf_gibbs_optimised, nmf_icm, bnmf_vb_observed); this class takes R and M as dense arrays"
                              % type(model).__name__)


def entries_of(model, M_pred=None, name="M"):
    """(rows, cols, values in fp32) of a model's training entries (M_pred None), or of M_pred -- an Entries, whose values are the
    true values at its entries, or a 0/1 matrix that picks them from the model's dense R: the one place where either form of
    input becomes the lists the library takes: row major, the fp32 cast entry_list's."""
    if M_pred is None:
        if isinstance(model.R, Entries):
            return model.R.row_major()
        return entry_list(model.R, check_binary(model.M, name))
    if isinstance(M_pred, Entries):
        assert M_pred.shape == tuple(model.R.shape), "Input matrix R is not of the same size as the entries %s: %s and %s respectively." \
            % (name, tuple(model.R.shape), M_pred.shape)
        return M_pred.row_major()
    if isinstance(model.R, Entries):
        raise _lib.BnmtfError("%s: a model built from an Entries holds no dense R to pick the values of a 0/1 mask from: pass %s "
                              "as an Entries with the true values at its entries" % (type(model).__name__, name))
    Mp = np.asarray(M_pred)
    check_binary(Mp, name)
    assert Mp.shape == model.R.shape, "Input matrix R is not of the same size as the indicator matrix %s: %s and %s respectively." % (name, model.R.shape, Mp.shape)
    return entry_list(model.R, Mp)


def _create(model, create, ranks, lambdas):
    """The handle `create` gives for a model's entries, seed and device, with its ranks and prior rates."""
    rows, cols, vals = entries_of(model)
    model._train_list = (rows, cols, vals)
    lams = [_lib.f64(l) for l in lambdas]
    h = C.c_void_p()
    _lib.check(create(int(model.I), int(model.J), *ranks, C.c_uint64(len(rows)), _lib.ptr(rows), _lib.ptr(cols), _lib.ptr(vals),
                      *[_lib.ptr(l) for l in lams], float(model.alpha), float(model.beta), C.c_uint64(model._seed & (2 ** 64 - 1)),
                      int(model._device), C.byref(h)))
    return h


def create_handle(model):
    """The bnmtf_obs_create handle of a model (its R, M, priors, seed, device)."""
    return _create(model, _lib.lib().bnmtf_obs_create, (int(model.K),), (model.lambdaU, model.lambdaV))


def create_tri_handle(model):
    """The bnmtf_otri_create handle of a tri-factorisation (its R, M, priors, seed, device)."""
    return _create(model, _lib.lib().bnmtf_otri_create, (int(model.K), int(model.L)), (model.lambdaF, model.lambdaS, model.lambdaG))


def _pred_list(model, M_pred):
    """The entry list of M_pred (None: the training entries) for the metric calls."""
    if M_pred is None:
        return model._train_list
    return entries_of(model, M_pred, "M_pred")


def _list_metric(model, M_pred, call, factors):
    """The six sums the library's `call` gives for the factors (fp64) over the entries of M_pred (None: the training entries)."""
    given = None if M_pred is None else _pred_list(model, M_pred)      # (what it refuses: before any device call)
    h, call = model._handle(), getattr(_lib.lib(), call)
    rows, cols, vals = _pred_list(model, None) if given is None else given
    out = np.zeros(6)
    if len(rows) == 0:                      # (an empty mask: the dense layout's sums of nothing)
        return out
    factors = [_lib.f64(f) for f in factors]
    _lib.check(call(h, C.c_uint64(len(rows)), _lib.ptr(rows), _lib.ptr(cols), _lib.ptr(vals), *[_lib.ptr(f) for f in factors], _lib.ptr(out)))
    return out


def tri_metric_sums(model, M_pred, F, S, G):
    """The six sums of metrics_from_sums of (F.S).G^T over the entries of M_pred (None: the training entries): F.S and the dot
    products in fp64 (bnmtf_otri_metric_sums), never the sweeps' fp32 effective factor."""
    return _list_metric(model, M_pred, "bnmtf_otri_metric_sums", (F, S, G))


def metric_sums(model, M_pred, A, B):
    """The six sums of metrics_from_sums of A.B^T over the entries of M_pred (None: the training entries), on the device in fp64."""
    return _list_metric(model, M_pred, "bnmf_obs_metric_sums", (A, B))
