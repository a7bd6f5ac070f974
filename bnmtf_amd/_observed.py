"""layout='observed' of bnmf_gibbs_optimised / nmf_icm and of bnmtf_gibbs_optimised / nmtf_icm, bnmf_vb_observed and
bnmtf_vb_observed: the host side of the observed-entry layout.

The device keeps the residual R_ij - U_i.V_j on the OBSERVED entries (csrc/kernel_obs.hip, kernel_obs_vb.hip), so cost and device memory follow the
number of observed entries: the layout for matrices that are mostly missing.  R and M stay dense NumPy arrays at the Python
boundary; this module turns the mask into the entry lists the library takes, owns the bnmtf_obs_create / bnmtf_otri_create handle of a model and
states what the layout does not run."""
import ctypes as C

import numpy as np

from . import _lib

LAYOUTS = ('dense', 'observed')
MAX_RANK = 256          # BNMTF_OBS_MAX_RANK: nothing ties a rank to a lane, one handle takes them all
MAX_RANK_TRI = 32       # BNMTF_OTRI_MAX_RANK: the tri-factorisation's S step is the dense K.L x K.L system, one 32 x 32 tile per column Gram


def check_layout(layout):
    assert layout in LAYOUTS, "Unknown layout: %s. Should be 'dense' or 'observed'." % (layout,)


def refuse(model, what, why):
    raise _lib.BnmtfError("%s: %s is not available with layout='observed' (%s)" % (type(model).__name__, what, why))


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


def create_handle(model):
    """The bnmtf_obs_create handle of a model (its R, M, priors, seed, device)."""
    Mb = model.M != 0
    assert (model.M == Mb).all(), "The indicator matrix M must contain only 0 and 1."
    rows, cols, vals = entry_list(model.R, Mb)
    model._train_list = (rows, cols, vals)
    lr, lc = _lib.f64(model.lambdaU), _lib.f64(model.lambdaV)
    h = C.c_void_p()
    _lib.check(_lib.lib().bnmtf_obs_create(int(model.I), int(model.J), int(model.K), C.c_uint64(len(rows)), _lib.ptr(rows), _lib.ptr(cols),
                                           _lib.ptr(vals), _lib.ptr(lr), _lib.ptr(lc), float(model.alpha), float(model.beta),
                                           C.c_uint64(model._seed & (2 ** 64 - 1)), int(model._device), C.byref(h)))
    return h


def create_tri_handle(model):
    """The bnmtf_otri_create handle of a tri-factorisation (its R, M, priors, seed, device)."""
    Mb = model.M != 0
    assert (model.M == Mb).all(), "The indicator matrix M must contain only 0 and 1."
    rows, cols, vals = entry_list(model.R, Mb)
    model._train_list = (rows, cols, vals)
    lf, ls, lg = _lib.f64(model.lambdaF), _lib.f64(model.lambdaS), _lib.f64(model.lambdaG)
    h = C.c_void_p()
    _lib.check(_lib.lib().bnmtf_otri_create(int(model.I), int(model.J), int(model.K), int(model.L), C.c_uint64(len(rows)), _lib.ptr(rows),
                                            _lib.ptr(cols), _lib.ptr(vals), _lib.ptr(lf), _lib.ptr(ls), _lib.ptr(lg), float(model.alpha),
                                            float(model.beta), C.c_uint64(model._seed & (2 ** 64 - 1)), int(model._device), C.byref(h)))
    return h


def _pred_list(model, M_pred):
    """The entry list of M_pred (None: the training entries) for the metric calls."""
    if M_pred is None:
        return model._train_list
    Mp = np.asarray(M_pred)
    assert ((Mp == 0) | (Mp == 1)).all(), "The indicator matrix M_pred must contain only 0 and 1."
    assert Mp.shape == model.R.shape, "Input matrix R is not of the same size as the indicator matrix M_pred: %s and %s respectively." % (model.R.shape, Mp.shape)
    return entry_list(model.R, Mp)


def tri_metric_sums(model, M_pred, F, S, G):
    """The six sums of metrics_from_sums of (F.S).G^T over the entries of M_pred (None: the training entries): F.S and the dot
    products in fp64 (bnmtf_otri_metric_sums), never the sweeps' fp32 effective factor."""
    h = model._handle()
    rows, cols, vals = _pred_list(model, M_pred)
    out = np.zeros(6)
    if len(rows) == 0:                      # (an empty mask: the dense layout's sums of nothing)
        return out
    F, S, G = _lib.f64(F), _lib.f64(S), _lib.f64(G)
    _lib.check(_lib.lib().bnmtf_otri_metric_sums(h, C.c_uint64(len(rows)), _lib.ptr(rows), _lib.ptr(cols), _lib.ptr(vals), _lib.ptr(F), _lib.ptr(S),
                                                 _lib.ptr(G), _lib.ptr(out)))
    return out


def metric_sums(model, M_pred, A, B):
    """The six sums of metrics_from_sums of A.B^T over the entries of M_pred (None: the training entries), on the device in fp64."""
    h = model._handle()
    rows, cols, vals = _pred_list(model, M_pred)
    out = np.zeros(6)
    if len(rows) == 0:                      # (an empty mask: the dense layout's sums of nothing)
        return out
    A, B = _lib.f64(A), _lib.f64(B)
    _lib.check(_lib.lib().bnmf_obs_metric_sums(h, C.c_uint64(len(rows)), _lib.ptr(rows), _lib.ptr(cols), _lib.ptr(vals), _lib.ptr(A), _lib.ptr(B), _lib.ptr(out)))
    return out
