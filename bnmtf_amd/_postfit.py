"""What the calls on a fitted model share (posterior_predictive, variational_predictive, top_entries, fold_in; DESIGN.md sections 2.8 - 2.10): which kind
of class a model is, the factors its predict() multiplies, the checks of stored samples, of factor shapes and of entry lists, and
the finish of the shifted moments.  Everything here runs on the host and refuses with a BnmtfError '<who>: <why>'."""
import numpy as np

from ._lib import BnmtfError


def refuse(who, why):
    raise BnmtfError("%s: %s" % (who, why))


def integer(who, name, v, low):
    """v as an int, which it must equal, and >= low"""
    try:
        i = int(v)
    except (TypeError, ValueError):
        refuse(who, "%s is an integer >= %d, not %r" % (name, low, v))
    if i != v or i < low:
        refuse(who, "%s is an integer >= %d, not %r" % (name, low, v))
    return i


def kind_of(model):
    """'gibbs', 'icm', 'variational' or 'np'; None: not a model of this package"""
    from ._sampler import GibbsSampler, ICMRules
    from ._variational import Variational
    from .nmf_np import NPDevice
    if isinstance(model, GibbsSampler):
        return 'icm' if isinstance(model, ICMRules) else 'gibbs'
    return 'variational' if isinstance(model, Variational) else 'np' if isinstance(model, NPDevice) else None


def device_of(model, device):
    return getattr(model, "_device", 0) if device is None else device


def stored_samples(who, model, burn_in, thinning):
    """(names of the sample arrays, how many are stored, burn_in, thinning as ints) of a Gibbs model whose samples
    range(burn_in, stored, thinning) exist"""
    names = ["all_" + f for f in model._FACTORS]
    if not all(hasattr(model, a) for a in names + ["all_tau"]):
        refuse(who, "no stored samples: run() has not been called")
    stored = len(getattr(model, names[0]))
    if stored == 0:
        refuse(who, "no stored samples: the last run() was called with store_samples=False")
    burn_in, thinning = int(burn_in), int(thinning)
    if thinning < 1:
        refuse(who, "thinning >= 1, not %d" % thinning)
    if not (0 <= burn_in < stored):
        refuse(who, "burn_in must lie below the number of stored samples (burn_in=%d, %d stored)" % (burn_in, stored))
    return names, stored, burn_in, thinning


def model_factors(who, model, burn_in, thinning):
    """the factors the class's predict() multiplies, in the order (A, B) or (A, S, B)"""
    kind = kind_of(model)
    if kind != 'gibbs':
        if kind is None:
            refuse(who, "not a model of this package")
        if burn_in is not None or thinning is not None:
            refuse(who, "burn_in and thinning select the samples of a Gibbs model (bnmf_gibbs_optimised, bnmtf_gibbs_optimised); "
                        "this class has one estimate and takes neither")
        if kind == 'variational':
            names = ["exp" + f for f in model._FACTORS]
            if not all(hasattr(model, a) for a in names):
                refuse(who, "no factors yet: initialise() has not been called")
            return [getattr(model, a) for a in names]
        try:
            return list(model._factors())
        except AttributeError:
            refuse(who, "no factors yet: initialise() has not been called")
    if burn_in is None or thinning is None:
        refuse(who, "burn_in and thinning are required for a Gibbs model: they select the samples whose mean is ranked "
                    "(approx_expectation(burn_in, thinning))")
    burn_in, thinning = stored_samples(who, model, burn_in, thinning)[2:]
    # what predict(M_pred, burn_in, thinning) multiplies: the mean of the stored samples, formed on the host in fp64 (only a model
    # whose last run() was given expectation=(burn_in, thinning) answers from its handle's sums instead, as it does for predict())
    return list(model.approx_expectation(burn_in, thinning)[:-1])


def factors_fit(who, factors, I, J, each_other):
    """the outer factors are [I][.] and [J][.]; each_other: and every inner dimension meets its neighbour's"""
    shapes = [np.shape(f) for f in factors]
    fit = len(shapes[0]) == 2 and len(shapes[-1]) == 2 and shapes[0][0] == I and shapes[-1][0] == J
    if fit and each_other:
        fit = all(len(s) == 2 for s in shapes) and (shapes[0][1] == shapes[1][1] if len(shapes) == 2 else
                                                    shapes[0][1] == shapes[1][0] and shapes[1][1] == shapes[2][1])
    if not fit:
        refuse(who, "factor arrays of shapes %s do not fit each other and the %d x %d matrix" % (", ".join(str(s) for s in shapes), I, J))


def index_list(who, name, a):
    a = np.asarray(a)
    if a.ndim != 1:
        refuse(who, "%s is one-dimensional, not %d-dimensional" % (name, a.ndim))
    if a.size and not np.issubdtype(a.dtype, np.integer):
        refuse(who, "%s holds integers, not %s" % (name, a.dtype))
    return a


def entry_lists(who, shape, rows, cols, noun="", bits=31, empty=False):
    """(rows, cols) as contiguous int32 lists of equal length inside the matrix.  noun: what the texts put before 'entry'
    ('excluded ': the lists are then 'the excluded rows', 'the excluded cols'); at most 2^bits - 1 entries; empty: whether a list
    without entries is taken"""
    lists = ("the " if noun else "") + noun
    rows, cols = index_list(who, lists + "rows", rows), index_list(who, lists + "cols", cols)
    if len(rows) != len(cols):
        refuse(who, "%srows and cols have different lengths: %d and %d" % (lists, len(rows), len(cols)))
    if len(rows) == 0 and not empty:
        refuse(who, "the list of entries is empty")
    if len(rows) >= 2 ** bits:
        refuse(who, "at most 2^%d - 1 %sentries (%d given)" % (bits, noun, len(rows)))
    bad = (rows < 0) | (rows >= shape[0]) | (cols < 0) | (cols >= shape[1])
    if bad.any():
        e = int(np.flatnonzero(bad)[0])
        refuse(who, "%sentry %d (%d, %d) lies outside the %d x %d matrix" % (noun, e, rows[e], cols[e], shape[0], shape[1]))
    return np.ascontiguousarray(rows, dtype=np.int32), np.ascontiguousarray(cols, dtype=np.int32)


def shifted_moments(first, sum_d, sum_d2, count):
    """(mean, variance) from the first value and the sums of (x - first) and of its square over `count` values: shifted by the
    first, a spread far below the mean survives fp64"""
    md = sum_d / count
    return first + md, np.maximum(0.0, sum_d2 / count - md * md)
