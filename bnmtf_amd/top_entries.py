"""The n highest (or lowest) predicted missing entries per row, selected on the device.

    T = top_entries(model, n, burn_in=.., thinning=..)       # a Gibbs model; every other class: top_entries(model, n)
    T.rows      # int32 [r]     the rows asked for, in the order given (rows=None: 0 .. I - 1)
    T.cols      # int32 [r][n]  per row the n best columns, best first; -1 where the row has fewer than n candidates
    T.scores    # fp64  [r][n]  their scores; nan where cols is -1
    T.counts    # int32 [r]     valid slots per row = min(n, J - excluded columns of that row)
    T.entries() # (rows, cols) of the valid slots as two flat int32 lists, row by row: what posterior_predictive(model, at=...)
                # and Entries take

The score of (i, j) is the entry of the matrix the class's own predict() evaluates: A[i] . B[j], or (F[i] S) . G[j], with the
factors predict() uses -- approx_expectation(burn_in, thinning)[:-1] of a Gibbs class, expU, expV / expF, expS, expG of a
variational one, the current point estimate of the ICM and the non-probabilistic classes.  It ranks by the product of the means,
not by the mean of the products over the samples.  The candidates of a row are the columns outside `exclude`: 'observed' (the
model's training entries), None (every column), or an Entries of the model's shape / a pair (rows, cols), repeats allowed.  The
order is total, so the answer is unique: higher score first (largest=False: lower first), equal scores: lower column first,
-0.0 equal to 0.0.  axis=1: for each COLUMN the n best rows -- the same call on the swapped problem; T.rows then holds column
indices and T.cols row indices, and entries() gives them back as (rows, cols) of the matrix.

The work -- r J K multiply-adds with a selection -- runs in bnmtf_top_entries (csrc/api_top.inc, kernel_top.hip); nothing of size
I x J is made on the host or the device.  The call reads host attributes and the training entries only and uses no model handle
(a Gibbs model whose last run() was given expectation=(burn_in, thinning) answers approx_expectation from its handle, as for predict()).
from_factors is the same on plain arrays.  Everything that is refused is refused before the first device call."""
import ctypes as C

import numpy as np

from . import _lib, _observed
from ._postfit import device_of, entry_lists, factors_fit, index_list, model_factors, refuse
from .entries import Entries

MAX_N = 128             # BNMTF_TOP_MAX_N
MAX_RANK = 256          # K and L of bnmtf_top_entries


class TopEntries(object):
    """What top_entries returns: rows [r], cols [r][n], scores [r][n], counts [r] (see the module's text); axis as asked for."""

    def __init__(self, rows, cols, scores, counts, axis=0):
        self.rows, self.cols, self.scores, self.counts, self.axis = rows, cols, scores, counts, int(axis)

    def __len__(self):
        return int(self.counts.sum())

    def __repr__(self):
        return "TopEntries(%d rows, n=%d, %d entries)" % (len(self.rows), self.cols.shape[1], len(self))

    def entries(self):
        """(rows, cols) of the valid slots, flat int32 lists, row by row and best first within a row; with axis=1 the pairs are
        turned back, so that they are (rows, cols) of the matrix either way."""
        valid = self.cols >= 0
        own = np.ascontiguousarray(np.repeat(self.rows, self.cols.shape[1]).reshape(self.cols.shape)[valid], dtype=np.int32)
        other = np.ascontiguousarray(self.cols[valid], dtype=np.int32)
        return (other, own) if self.axis == 1 else (own, other)


def _exclusion(who, shape, exclude):
    """(ex_rows, ex_cols) as int32 lists inside the matrix, or two empty ones"""
    if exclude is None:
        return np.zeros(0, dtype=np.int32), np.zeros(0, dtype=np.int32)
    if isinstance(exclude, Entries):
        if tuple(exclude.shape) != tuple(shape):
            refuse(who, "the excluded Entries and the matrix have different shapes: %s and %s" % (tuple(exclude.shape), tuple(shape)))
        return exclude.rows, exclude.cols
    if isinstance(exclude, str):
        refuse(who, "exclude is 'observed' (a model's training entries), None, an Entries or a pair (rows, cols), not %r" % exclude)
    try:
        er, ec = exclude
    except (TypeError, ValueError):
        refuse(who, "exclude is 'observed' (a model's training entries), None, an Entries or a pair (rows, cols), not %s" % type(exclude).__name__)
    return entry_lists(who, shape, er, ec, noun="excluded ", bits=32, empty=True)


def _compute(who, factors, n, rows, exclude, largest, device, split, axis=0):
    if len(factors) not in (2, 3):
        refuse(who, "factors is (A, B) or (A, S, B), not %d arrays" % len(factors))
    arrays = [np.ascontiguousarray(f, dtype=np.float64) for f in factors]
    if any(a.ndim != 2 for a in arrays):
        refuse(who, "every factor is two-dimensional, not %s" % ", ".join(str(a.shape) for a in arrays))
    A, S, B = arrays[0], (arrays[1] if len(arrays) == 3 else None), arrays[-1]
    I, K = A.shape
    J, W = B.shape
    L = S.shape[1] if S is not None else 0
    if I < 1 or J < 1 or (S is None and W != K) or (S is not None and (S.shape[0] != K or W != L)):
        refuse(who, "factor arrays of shapes %s do not fit each other: (A [I][K], B [J][K]) or (A [I][K], S [K][L], B [J][L])"
                % ", ".join(str(a.shape) for a in arrays))
    if not (1 <= K <= MAX_RANK) or (S is not None and not (1 <= L <= MAX_RANK)):
        refuse(who, "ranks 1 .. %d (K=%d, L=%d)" % (MAX_RANK, K, L))
    try:
        n_int = int(n)
    except (TypeError, ValueError):
        refuse(who, "n is an integer 1 .. %d (BNMTF_TOP_MAX_N), not %r" % (MAX_N, n))
    if n_int != n or not (1 <= n_int <= MAX_N):
        refuse(who, "n is an integer 1 .. %d (BNMTF_TOP_MAX_N), not %r" % (MAX_N, n))
    split = int(split)
    if split < 0 or split > 1024:
        refuse(who, "0 <= split <= 1024 column segments per row (0: the library chooses), not %d" % split)
    for name, a in (("A", A), ("S", S), ("B", B)):
        if a is not None and not np.isfinite(a).all():
            refuse(who, "factor %s holds a value that is not finite (the total order needs finite scores)" % name)
    if rows is None:
        sel = np.arange(I, dtype=np.int32)
    else:
        sel = index_list(who, "rows", rows)
        if sel.size == 0:
            refuse(who, "rows is empty (None: all rows)")
        bad = (sel < 0) | (sel >= I)
        if bad.any():
            e = int(np.flatnonzero(bad)[0])
            refuse(who, "rows[%d] = %d lies outside the %d rows" % (e, sel[e], I))
        uniq, first = np.unique(sel, return_index=True)
        if len(uniq) != len(sel):
            twice = int(sel[np.setdiff1d(np.arange(len(sel)), first)[0]])
            refuse(who, "rows holds distinct indices: %d occurs twice" % twice)
        sel = np.ascontiguousarray(sel, dtype=np.int32)
    er, ec = _exclusion(who, (I, J), exclude)

    r = len(sel)
    cols = np.zeros((r, n_int), dtype=np.int32)
    scores = np.zeros((r, n_int))
    counts = np.zeros(r, dtype=np.int32)
    _lib.check(_lib.lib().bnmtf_top_entries(int(device), int(I), int(J), int(K), int(L), _lib.ptr(A), _lib.ptr(S), _lib.ptr(B),
                                            C.c_uint64(r), _lib.ptr(sel) if rows is not None else None,
                                            C.c_uint64(len(er)), _lib.ptr(er) if len(er) else None, _lib.ptr(ec) if len(er) else None,
                                            n_int, 1 if largest else 0, split, _lib.ptr(cols), _lib.ptr(scores), _lib.ptr(counts)))
    return TopEntries(sel, cols, scores, counts, axis)


def from_factors(factors, n, *, rows=None, exclude=None, largest=True, device=0, split=0):
    """top_entries on plain arrays.  factors: (A [I][K], B [J][K]) or (A [I][K], S [K][L], B [J][L]), any real dtype (taken as
    fp64); exclude: None, an Entries of shape (I, J) or a pair (rows, cols); split: column segments per row, each taken by a wave
    of its own (0: the library chooses; the answer's bytes do not depend on it).  Returns a TopEntries."""
    if isinstance(exclude, str):
        refuse("top_entries.from_factors", "exclude is None, an Entries or a pair (rows, cols): plain factors have no training entries (%r)" % exclude)
    return _compute("top_entries.from_factors", factors, n, rows, exclude, largest, device, split)


def top_entries(model, n, *, burn_in=None, thinning=None, rows=None, axis=0, largest=True, exclude='observed', device=None):
    """Per row of the model's matrix (rows: a 1-D array of distinct rows in any order; None: all) the n <= 128 candidates its
    predict() scores highest (largest=False: lowest): a TopEntries (see the module's text).  model: any class the package
    exports, either layout, Entries-built or dense-built, blocked ranks included; burn_in, thinning: required for the Gibbs
    classes, refused for every other; exclude: 'observed' -- the model's training entries --, None, an Entries of the model's
    shape or (rows, cols); axis=1: for each column the n best rows (T.rows then holds column indices, T.cols row indices);
    device: defaults to the model's."""
    who = type(model).__name__ + ": top_entries"
    if axis not in (0, 1):
        refuse(who, "axis is 0 (per row the best columns) or 1 (per column the best rows), not %r" % (axis,))
    factors = model_factors(who, model, burn_in, thinning)
    shape = (int(model.I), int(model.J))
    factors_fit(who, factors, shape[0], shape[1], each_other=False)           # (_compute checks the inner dimensions, with its own text)
    if isinstance(exclude, str):
        if exclude != 'observed':
            refuse(who, "exclude is 'observed' (the model's training entries), None, an Entries or a pair (rows, cols), not %r" % exclude)
        er, ec = _observed.entries_of(model)[:2]
    else:
        er, ec = _exclusion(who, shape, exclude)
    if axis == 1:                       # the swapped problem: (B, A), or (G, S^T, F), and the exclusion transposed
        factors = [factors[-1]] + ([np.asarray(factors[1]).T] if len(factors) == 3 else []) + [factors[0]]
        er, ec = ec, er
    return _compute(who, factors, n, rows, (er, ec), largest, device_of(model, device), 0, axis)


top_entries.from_factors = from_factors          # (the package exports the function under the module's name: bnmtf_amd.top_entries.from_factors)
