"""Entries: the observed entries of an I x J matrix as lists -- what a mostly-missing matrix is on the host, as the observed-entry
layout is what it is on the device.

    E = Entries((I, J), rows, cols, values)
    BNMF = bnmf_gibbs_optimised(E, None, K, priors, layout='observed')      # likewise nmf_icm, and bnmf_vb_observed(E, None, K, priors)
    BNMF.run(iterations, M_test=E_test)                                     # held-out curve: all_performances_test
    BNMF.predict(E_test, burn_in, thinning)                                 # E_test's values are the true values at its entries

Taken in place of the dense pair (R, M) by the three classes on the two-factor handle of this layout, as M_test of their run()
and as M_pred of their predict().  Nothing of size I x J is allocated on that path: host memory follows the number of entries."""
import numpy as np


class Entries(object):
    """The entries (rows[e], cols[e]) of a matrix of `shape`, in any order, with their values.  Held as contiguous int32 / int32 /
    fp64 arrays; the device takes the values in fp32, cast as _observed.entry_list casts a dense R.  An entry given twice, or a
    row or column without one, is found where it is found for dense input: by the library when the handle is made, and -- the
    empty rows and columns -- by the model's constructor."""

    def __init__(self, shape, rows, cols, values):
        try:
            shape = tuple(int(s) for s in shape)
        except TypeError:
            raise ValueError("Entries: shape is (I, J), not %r" % (shape,))
        if len(shape) != 2 or shape[0] < 1 or shape[1] < 1:
            raise ValueError("Entries: shape is (I, J) with I, J >= 1, not %r" % (shape,))
        lists = []
        for name, a in (("rows", rows), ("cols", cols)):
            a = np.asarray(a)
            if a.ndim != 1:
                raise ValueError("Entries: %s is one-dimensional, not %d-dimensional" % (name, a.ndim))
            if a.size and not np.issubdtype(a.dtype, np.integer):
                raise ValueError("Entries: %s holds integers, not %s" % (name, a.dtype))
            lists.append(a)
        values = np.ascontiguousarray(values, dtype=np.float64)
        if values.ndim != 1:
            raise ValueError("Entries: values is one-dimensional, not %d-dimensional" % values.ndim)
        if not (len(lists[0]) == len(lists[1]) == len(values)):
            raise ValueError("Entries: rows, cols and values have different lengths: %d, %d and %d" % (len(lists[0]), len(lists[1]), len(values)))
        for name, a, extent in (("rows", lists[0], shape[0]), ("cols", lists[1], shape[1])):
            if a.size and (a.min() < 0 or a.max() >= extent):
                e = int(np.flatnonzero((a < 0) | (a >= extent))[0])
                raise ValueError("Entries: entry %d (%d, %d) lies outside the %d x %d matrix" % (e, lists[0][e], lists[1][e], shape[0], shape[1]))
        if not np.isfinite(values).all():
            e = int(np.flatnonzero(~np.isfinite(values))[0])
            raise ValueError("Entries: the value of entry %d (%d, %d) is not finite: %s" % (e, lists[0][e], lists[1][e], values[e]))
        self.shape = shape
        self.rows = np.ascontiguousarray(lists[0], dtype=np.int32)
        self.cols = np.ascontiguousarray(lists[1], dtype=np.int32)
        self.values = values

    def __len__(self):
        return len(self.rows)

    def __repr__(self):
        return "Entries(%d x %d, %d entries)" % (self.shape[0], self.shape[1], len(self))

    @classmethod
    def from_dense(cls, R, M):
        """The entries of the 0/1 matrix M with R's values, in row-major order: the order and values of _observed.entry_list."""
        R, Mb = np.asarray(R), np.asarray(M) != 0
        if R.ndim != 2 or R.shape != Mb.shape:
            raise ValueError("Entries.from_dense: R and M are two-dimensional and of one shape, not %s and %s" % (R.shape, Mb.shape))
        rows, cols = np.nonzero(Mb)
        return cls(R.shape, rows, cols, R[Mb])

    def to_dense(self):
        """(R, M) as fp64 I x J arrays, R zero where M is: for tests and small cases."""
        R, M = np.zeros(self.shape), np.zeros(self.shape)
        R[self.rows, self.cols] = self.values
        M[self.rows, self.cols] = 1.0
        return R, M

    def counts(self):
        """(n, entries per row, entries per column), the counts as uint32: omega_counts() of a model built from these entries."""
        return (len(self), np.bincount(self.rows, minlength=self.shape[0]).astype(np.uint32),
                np.bincount(self.cols, minlength=self.shape[1]).astype(np.uint32))

    def values32(self):
        """The values as the device takes them: fp32, the cast entry_list makes of a dense R."""
        return np.ascontiguousarray(self.values, dtype=np.float32)

    def row_major(self):
        """(rows, cols, values in fp32) in row-major order -- entry_list's order, whatever order the entries were given in: the
        lists the library's calls are handed, so that a sum over them does not depend on the order of the input."""
        key = self.rows.astype(np.int64) * self.shape[1] + self.cols
        if len(key) < 2 or (key[1:] > key[:-1]).all():
            return self.rows, self.cols, self.values32()
        order = np.argsort(key, kind='stable')
        return np.ascontiguousarray(self.rows[order]), np.ascontiguousarray(self.cols[order]), np.ascontiguousarray(self.values[order], dtype=np.float32)

    def check_rows_columns(self):
        """check_R_M's assertions on a list: no row and no column without an entry (the same texts)."""
        _, per_row, per_col = self.counts()
        empty = np.flatnonzero(per_row == 0)
        assert len(empty) == 0, "Fully unobserved row in R, row %s." % empty[0]
        empty = np.flatnonzero(per_col == 0)
        assert len(empty) == 0, "Fully unobserved column in R, column %s." % empty[0]
