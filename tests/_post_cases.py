"""Shared by tests/test_post_cases_cpu.py and tests/test_post_exact_gpu.py: the relayout and the Gram behind every half sweep and
every state upload of a dense-layout model (csrc/kernel_post.hip: post_kernel, gram_reduce_kernel, gram_cast_kernel) -- a NumPy face
of the library's read-only diagnostic entry bnmtf_post_dump, a NumPy model that restates every output of the two kernels from the
factor they read, in the kernels' own order of additions, the two value families, and the seeded cases with the launch-shape
classes each of them is there for.

Everything the kernels compute is an fp64 sum of products of two fp32 numbers (exact in fp64: 24 + 24 significand bits), so the
fused multiply-add of the device is the multiplication and the addition of NumPy, and a restatement that adds in the same order
gives the same bits:

  layouts   XT[k][r] = X[r][k]; XT2[kp][r][c] = X[r][2 kp + c]; S2T like XT from S2; XS[k][r] = (X[r][k], S2[r][k]); zero from
            `rows` to ldT and in the padding columns K .. KP - 1 (the buffers start as zeros, X's padding columns are zeros)
  Gram      per block of 32 rows acc = acc + a b over r = 0 .. 31 in row order (rows beyond the factor are zeros); stride g adds
            the blocks g, g + 32, ... in order; the 32 strides are added in order.  Only the 4 x 4 tiles on and above the diagonal
            are formed (tri_tile: packed tile p -> (ty, tx)); a tile above the diagonal is stored a second time, mirrored.
            C32 = float32(C64)
  colsum    per block and column four row groups r = grp, grp + 4, ..., combined (d0 + d1) + (d2 + d3); across blocks group grp of
            16 adds the blocks grp + 128 i + 16 u, i outer, u = 0 .. 7 (a block beyond nblk: + 0.0, which changes nothing); the 16
            groups are added in order.  colsum2 the same from S2
  own rows  (several GPUs: a rank forms the Gram of its own rows [own0, own1) only) blocks from own0 // 32, rows outside the range
            count as zeros, nblk counted from that first block

Family X: small integers times a power of two per column -- every partial and every final sum is exact (bounded below), so the
expected Gram and column sums are X^T X and X.sum(0) themselves, in whatever order: this pins the coverage, every row and every
block exactly once.  Family G: values over six decades with zeros, an all-zero column and a huge column -- the sums round, and the
device must return the ordered model's bits."""
from types import SimpleNamespace

import numpy as np

from bnmtf_amd import _lib

RB = 32                     # kPostRows
U64 = 2.0 ** -53            # unit roundoff of fp64

# ------------------------------------------------------------------------------------------------ the diagnostic entry
DUMP_INFO = ("rows", "KP", "W", "ldT", "nblk", "vb", "xs", "umax", "n0", "n")
DUMP_ARRAYS = (("X", np.float32), ("S2", np.float32), ("XT", np.float32), ("XT2", np.float32), ("S2T", np.float32), ("XS", np.float32),
               ("C64", np.float64), ("C32", np.float32), ("colsum", np.float64), ("colsum2", np.float64))
DUMP_INFO_LEN = 20          # BNMTF_POST_INFO_LEN
OUTPUTS = ("XT", "XT2", "S2T", "XS", "C64", "C32", "colsum", "colsum2")


def raw_dump(h, which, info, arrays):
    return _lib.lib().bnmtf_post_dump(h, int(which), _lib.ptr(info), *[_lib.ptr(a) for a in arrays])


def post_dump(h, which):
    """Direction `which` (0 rows, 1 cols) of handle h: the scalars (DUMP_INFO) and the ten arrays in their shapes (None where the
    handle has none).  Two calls: the sizes, then the data."""
    assert len(DUMP_INFO) + len(DUMP_ARRAYS) == DUMP_INFO_LEN
    info = np.zeros(DUMP_INFO_LEN, dtype=np.int64)
    _lib.check(raw_dump(h, which, info, [None] * len(DUMP_ARRAYS)))
    arrays = [np.full(int(s), np.nan, dtype=dt) if s else None for (_, dt), s in zip(DUMP_ARRAYS, info[len(DUMP_INFO):])]
    info2 = np.zeros(DUMP_INFO_LEN, dtype=np.int64)
    _lib.check(raw_dump(h, which, info2, arrays))
    assert (info == info2).all()
    d = SimpleNamespace(**{k: int(v) for k, v in zip(DUMP_INFO, info)}, **{name: a for (name, _), a in zip(DUMP_ARRAYS, arrays)})
    shapes = dict(X=(d.rows, d.KP), S2=(d.rows, d.KP), XT=(d.KP, d.ldT), XT2=(d.KP // 2, d.ldT, 2), S2T=(d.KP, d.ldT),
                  XS=(d.KP, d.ldT, 2), C64=(d.KP, d.KP), C32=(d.KP, d.KP))
    for name, shape in shapes.items():
        if getattr(d, name) is not None:
            setattr(d, name, getattr(d, name).reshape(shape))
    assert d.nblk == -(-d.rows // RB) and d.ldT >= d.rows and d.ldT % 256 == 0
    return d


# ------------------------------------------------------------------------------------------------ the model
FAULTS = ("last_row_of_a_partial_block_dropped", "block_left_out_of_a_stride", "stride_summed_twice", "clamped_term_counted",
          "second_batch_skipped", "mirror_from_the_next_row", "tri_tile_off_by_one_at_a_row_change", "xt2_pairs_swapped",
          "xs_second_half_from_the_next_row", "own0_excluded", "padding_column_counted")


def tri_tile(p, NT):
    """tile p of the packed upper triangle -> (ty, tx): row y of tiles holds (y, y) .. (y, NT - 1)"""
    y, rem = 0, p
    while rem >= NT - y:
        rem -= NT - y
        y += 1
    return y, y + rem


def _seq_sum(terms):
    """terms[0] + terms[1] + ... in order, from +0.0, along axis 0"""
    acc = np.zeros(terms.shape[1:], dtype=np.float64)
    for t in terms:
        acc = acc + t
    return acc


def tiles(X, own0, own1, fault=None):
    """The tiles of the Gram blocks as doubles [nblk][32][KP] -- rows outside [own0, own1) and beyond the factor are zeros -- and
    the first block."""
    rows, KP = X.shape
    blk0 = own0 // RB
    nblk = (-(-own1 // RB) - blk0) if own1 > own0 else 0
    lo = own0 + 1 if fault == "own0_excluded" else own0
    T = np.zeros((nblk * RB, KP), dtype=np.float64)
    r0 = blk0 * RB
    hi = min(own1, rows)
    if fault == "last_row_of_a_partial_block_dropped" and rows % RB and hi == rows:
        hi -= 1
    if hi > lo:
        T[lo - r0:hi - r0] = X[lo:hi].astype(np.float64)
    return T.reshape(nblk, RB, KP), blk0


def column_sums(T, W=None, fault=None):
    """colsum [KP] of the tiles T [nblk][32][KP]: post_body's four row groups, gram_reduce_body's 16 block groups."""
    nblk, _, KP = T.shape
    d = [_seq_sum(T[:, g::4, :].transpose(1, 0, 2)) for g in range(4)]              # [nblk][KP] each, rows g, g + 4, ... in order
    part = (d[0] + d[1]) + (d[2] + d[3])
    nbatch = max(-(-nblk // 128), 1)
    if fault == "second_batch_skipped":
        nbatch = 1
    padded = np.zeros((nbatch * 128, KP), dtype=np.float64)
    n = min(nblk, nbatch * 128)
    padded[:n] = part[:n]
    if fault == "clamped_term_counted" and nblk:
        # the last batch of a group that does not take the unrolled path loads a term beyond the last block clamped to it
        for grp in range(16):
            for b0 in range(grp, nblk, 128):
                if not b0 + 112 < nblk:
                    for u in range(8):
                        if b0 + 16 * u >= nblk:
                            padded[b0 + 16 * u] = part[nblk - 1]
    groups = padded.reshape(nbatch, 8, 16, KP)                                        # block = 128 i + 16 u + grp
    acc = np.zeros((16, KP), dtype=np.float64)
    for i in range(nbatch):
        for u in range(8):
            acc = acc + groups[i, u]
    out = _seq_sum(acc)
    if fault == "padding_column_counted" and W is not None and 0 < W < KP:
        out[W] = out[W - 1]
    return out


def partials(T):
    """post_body: the Gram partial of every block [nblk][KP][KP], acc = acc + a b in row order"""
    nblk, _, KP = T.shape
    P = np.zeros((nblk, KP, KP), dtype=np.float64)
    for r in range(RB):
        P += T[:, r, :, None] * T[:, r, None, :]
    return P


def gram_total(P, fault=None):
    """gram_reduce_body: stride g adds the blocks g, g + 32, ... in order, then the 32 strides are added in order"""
    nblk, KP, _ = P.shape
    S = np.zeros((32, KP, KP), dtype=np.float64)
    for i in range(-(-nblk // 32)):
        chunk = P[32 * i:32 * i + 32]
        if fault == "block_left_out_of_a_stride" and i == (nblk - 1) // 32 and i > 0:
            chunk = chunk.copy(); chunk[0] = 0.0                                      # the last block of stride 0
        S[:len(chunk)] = S[:len(chunk)] + chunk
    tot = _seq_sum(S)
    if fault == "stride_summed_twice":
        tot = tot + S[0]
    return tot


def gram_scatter(tot, fault=None):
    """Only the tiles on and above the diagonal are formed: packed entry t = 16 tile + 4 i + j -> (4 ty + i, 4 tx + j), and the
    mirror of a tile above the diagonal"""
    KP = tot.shape[0]
    NT = KP // 4
    NU = NT * (NT + 1) // 2
    C = np.zeros((KP, KP), dtype=np.float64)
    for p in range(NU):
        ty, tx = tri_tile(p, NT)
        val = tot[4 * ty:4 * ty + 4, 4 * tx:4 * tx + 4]
        if fault == "tri_tile_off_by_one_at_a_row_change" and tx == NT - 1 and p + 1 < NU:
            continue                               # (the tile lands on its successor's place, which the successor then overwrites)
        C[4 * ty:4 * ty + 4, 4 * tx:4 * tx + 4] = val
        if ty != tx:
            if fault == "mirror_from_the_next_row":
                val = val[[1, 2, 3, 3], :]
            C[4 * tx:4 * tx + 4, 4 * ty:4 * ty + 4] = val.T
    return C


def gram(T, fault=None):
    """C64 [KP][KP] of the tiles T [nblk][32][KP]"""
    return gram_scatter(gram_total(partials(T), fault), fault)


def layouts(X, S2, ldT, fault=None):
    rows, KP = X.shape
    out = {}
    XT = np.zeros((KP, ldT), dtype=np.float32); XT[:, :rows] = X.T
    XT2 = np.zeros((KP // 2, ldT, 2), dtype=np.float32)
    pairs = X.reshape(rows, KP // 2, 2).transpose(1, 0, 2)
    XT2[:, :rows, :] = pairs[:, :, ::-1] if fault == "xt2_pairs_swapped" else pairs
    out["XT"], out["XT2"] = XT, XT2
    if S2 is not None:
        S2T = np.zeros((KP, ldT), dtype=np.float32); S2T[:, :rows] = S2.T
        XS = np.zeros((KP, ldT, 2), dtype=np.float32)
        XS[:, :rows, 0] = X.T
        XS[:, :rows, 1] = S2[np.minimum(np.arange(rows) + 1, rows - 1)].T if fault == "xs_second_half_from_the_next_row" else S2.T
        out["S2T"], out["XS"] = S2T, XS
    return out


def model(X, S2=None, ldT=None, W=None, own=None, fault=None):
    """Every output of the relayout and the Gram of factor X [rows][KP] (fp32, as dumped), VB: with S2.  own = (own0, own1): the
    Gram and the column sums over those rows only (the layouts are always those of the whole factor)."""
    X = np.ascontiguousarray(X, dtype=np.float32)
    rows, KP = X.shape
    if ldT is None:
        ldT = (((rows + 31) // 32 * 32 + 32) + 255) // 256 * 256
    own0, own1 = own if own is not None else (0, rows)
    out = layouts(X, S2, ldT, fault)
    T, _ = tiles(X, own0, own1, fault)
    out["C64"] = gram(T, fault)
    with np.errstate(over="ignore"):
        out["C32"] = out["C64"].astype(np.float32)
    out["colsum"] = column_sums(T, W, fault)
    if S2 is not None:
        T2, _ = tiles(np.ascontiguousarray(S2, dtype=np.float32), own0, own1, fault)
        out["colsum2"] = column_sums(T2, W, fault)
    return out


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    as_int = {4: np.uint32, 8: np.uint64}[a.dtype.itemsize]
    return np.array_equal(a.view(as_int), b.view(as_int))


def differences(got, want, names=OUTPUTS):
    """One line per output of `names` that `want` holds and `got` does not return bit for bit."""
    lines = []
    for name in names:
        w = want.get(name)
        g = got.get(name) if isinstance(got, dict) else getattr(got, name, None)
        if w is None:
            continue
        if g is None:
            lines.append("%s: not returned" % name)
        elif not same_bits(np.asarray(g), w):
            g = np.asarray(g)
            bad = np.argwhere(g.view({4: np.uint32, 8: np.uint64}[g.dtype.itemsize]) != w.view({4: np.uint32, 8: np.uint64}[w.dtype.itemsize])) \
                if g.shape == w.shape else []
            first = tuple(bad[0]) if len(bad) else None
            lines.append("%s: %d of %d elements differ; first at %s: expected %r, got %r" % (
                name, len(bad), w.size, first, None if first is None else w[first], None if first is None else g[first]))
    return lines


# ------------------------------------------------------------------------------------------------ the value families
FAMILIES = ("X", "G")
# family X: entries n 2^e, 0 <= n <= 15, |e| <= 3 per column; VB: var = m 2^(2 e), 0 <= m <= 15, so S2 = (m + n^2) 2^(2 e) with
# m + n^2 <= 240 is exact in fp32 however var + exp^2 is rounded.  Over at most MAX_ROWS rows a Gram entry is 2^(ea + eb) times an
# integer <= 8225 * 15 * 15 = 1 850 625 < 2^21 and a column sum of S2 2^(2 e) times one <= 8225 * 240 = 1 974 000 < 2^21: every
# partial sum is such an integer too (all terms are non-negative), far inside the 53 bits of fp64 -- and inside the 24 of C32.
MAX_ROWS, N_MAX, E_MAX = 8225, 15, 3
assert MAX_ROWS * N_MAX * N_MAX < 2 ** 21 and MAX_ROWS * (N_MAX + N_MAX * N_MAX) < 2 ** 21


def family_X(rows, K, seed, vb=False):
    """(exp, var or None) [rows][K] fp64 holding fp32 values.  The first and the last two rows and the rows on either side of
    every block edge are non-zero in every column."""
    assert rows <= MAX_ROWS
    rs = np.random.RandomState(seed)
    e = rs.randint(-E_MAX, E_MAX + 1, K)
    n = rs.randint(0, N_MAX + 1, (rows, K))
    edge = np.unique(np.clip(np.concatenate([[0, rows - 1, rows - 2], np.arange(0, rows, RB), np.arange(RB - 1, rows, RB)]), 0, rows - 1))
    n[edge] = 1 + (n[edge] + edge[:, None] + np.arange(K)[None, :]) % N_MAX
    ex = n * 2.0 ** e
    var = None
    if vb:
        m = rs.randint(0, N_MAX + 1, (rows, K))
        m[edge] = 1 + (m[edge] + 2 * edge[:, None] + np.arange(K)[None, :]) % N_MAX
        var = m * 4.0 ** e
    return ex, var


def family_G(rows, K, seed, vb=False):
    """Values over six decades, a tenth of them zeros, column 1 all zeros (K >= 3), column K - 1 larger by 2^40 (K >= 2)."""
    rs = np.random.RandomState(seed + 1000003)

    def draw():
        v = 10.0 ** rs.uniform(-3, 3, (rows, K)) * (rs.rand(rows, K) >= 0.1)
        v[[0, rows - 1]] = np.maximum(v[[0, rows - 1]], 0.5)          # (no zeros in the first and the last row)
        if K >= 3:
            v[:, 1] = 0.0
        if K >= 2:
            v[:, K - 1] *= 2.0 ** 40
        return v.astype(np.float32).astype(np.float64)
    ex = draw()
    return ex, (draw() if vb else None)


def family(name, rows, K, seed, vb=False):
    return (family_X if name == "X" else family_G)(rows, K, seed, vb)


def padded(a, KP):
    """[rows][K] -> the device's [rows][KP] fp32 (zeros in the padding columns)"""
    out = np.zeros((a.shape[0], KP), dtype=np.float32)
    out[:, :a.shape[1]] = a
    return out


def bound_ratios(X, out, samples=24, seed=0):
    """Family G against the plain sums: any order of n - 1 additions of n exact terms stays within gamma sum |terms| of their sum,
    gamma = (n - 1) u / (1 - (n - 1) u) (Higham, Accuracy and Stability of Numerical Algorithms, 4.2).  The terms are exact (a
    product of two fp32 numbers has 48 bits), padding rows add zeros, and n <= rows + 128 covers the tile's 32 rows, the strides
    and the groups.  The plain sum comes from math.fsum, correctly rounded: one more u.  Returns the largest |model - plain sum| /
    bound over every column sum and over `samples` Gram entries (the diagonal and the last column among them).  Measured over
    the cases of test_post_cases_cpu.py: at most 0.02 (the one-block cases, where n is mostly the allowance of 128), 0.0004 to
    0.001 from 4000 rows on -- blocked sums of non-negative terms stay far inside a bound made for any order and any signs."""
    import math
    Xd = X.astype(np.float64)
    rows, KP = Xd.shape
    n = rows + 128
    gamma = (n - 1) * U64 / (1 - (n - 1) * U64) + U64
    worst = 0.0

    def ratio(terms, got):
        exact, scale = math.fsum(terms), math.fsum(np.abs(terms))
        if scale == 0.0:
            assert got == 0.0
            return 0.0
        return abs(got - exact) / (gamma * scale)
    for k in range(KP):
        worst = max(worst, ratio(Xd[:, k], out["colsum"][k]))
    rs = np.random.RandomState(seed)
    picks = [(0, 0), (KP - 1, KP - 1), (0, KP - 1)] + [tuple(rs.randint(0, KP, 2)) for _ in range(samples)]
    for a, b in picks:
        worst = max(worst, ratio(Xd[:, a] * Xd[:, b], out["C64"][a, b]))
    return worst


# ------------------------------------------------------------------------------------------------ the cases
NBLK = (1, 2, 15, 16, 17, 31, 32, 33, 64, 65, 112, 113, 120, 128, 129, 144, 241, 257)
MODS = (0, 1, 31)
KS = {32: (1, 2, 31, 32), 64: (33, 63, 64)}
OTHER = 24                  # the other extent of the matrix: small, and with BNMTF_SMALL=0 the handle runs the multi-launch kernels


def rows_of(nblk, mod):
    return RB * (nblk - 1) + (mod if mod else RB)


def clamped_live_terms(nblk):
    """live terms (blocks < nblk) of every batch of the column-sum block that takes the clamped path, over the 16 groups"""
    out = set()
    for grp in range(16):
        for b0 in range(grp, nblk, 128):
            if not b0 + 112 < nblk:
                out.add(sum(1 for u in range(8) if b0 + 16 * u < nblk))
    return out


def unrolled_groups(nblk, batch):
    return sum(1 for grp in range(16) if grp + 128 * batch < nblk and grp + 128 * batch + 112 < nblk)


def edges(rows, K, KP=None, own=None):
    """The launch-shape classes a factor of `rows` rows and K columns exercises (own: the own-rows form of a rank)."""
    KP = KP or (32 if K <= 32 else 64)
    own0, own1 = own if own is not None else (0, rows)
    nblk = -(-own1 // RB) - own0 // RB if own1 > own0 else 0
    e = {"rows_mod_32=%d" % (rows % RB), "K=%d" % K, "NT=%d" % (KP // 4)}
    if rows % RB:
        e.add("partial_last_block")
    if K < KP:
        e.add("padding_columns")
    if K < KP:
        e.add("snapW<KP")
    if K > 4:
        e.add("off_diagonal_tile_live")
    if K > KP - 4:
        e.add("last_tile_column_live")
    if 0 < nblk < 16:
        e.add("colsum_groups_without_work")
    u0 = unrolled_groups(nblk, 0)
    if u0 == 1:
        e.add("first_batch_unrolled_for_group_0_only")
    if 1 < u0 < 16:
        e.add("first_batch_unrolled_for_some_groups")
    if u0 == 16:
        e.add("first_batch_unrolled_for_all_groups")
    live = clamped_live_terms(nblk)
    e |= {"clamped_batch_with_%d_live" % n for n in live}
    if not live and nblk:
        e.add("no_clamped_batch")
    if nblk > 128:
        e.add("second_batch")
    if unrolled_groups(nblk, 1):
        e.add("second_batch_unrolled")
    if nblk > 256:
        e.add("third_batch")
    terms = {len(range(g, nblk, 32)) for g in range(32)}
    e |= {"stride_of_%d_terms" % t for t in terms}
    if own is not None:
        e.add("own_rows_form")
        if own0 % RB:
            e.add("own0_inside_a_block")
        if own1 % RB and own1 < rows:
            e.add("own1_inside_a_block")
        if nblk == 0:
            e.add("no_own_rows")
    return e


# what the faults of FAULTS need to show: the classes a case must have (any one of them) for the fault to move a checked output
FAULT_EDGES = {
    "last_row_of_a_partial_block_dropped": ("partial_last_block",),
    "block_left_out_of_a_stride": ("stride_of_2_terms", "stride_of_3_terms", "stride_of_4_terms", "stride_of_5_terms", "stride_of_8_terms", "stride_of_9_terms"),
    "stride_summed_twice": ("NT=8", "NT=16"),
    "clamped_term_counted": tuple("clamped_batch_with_%d_live" % n for n in range(1, 8)),
    "second_batch_skipped": ("second_batch",),
    "mirror_from_the_next_row": ("off_diagonal_tile_live",),
    "tri_tile_off_by_one_at_a_row_change": ("last_tile_column_live",),
    "xt2_pairs_swapped": ("NT=8", "NT=16"),
    "xs_second_half_from_the_next_row": ("vb",),
    "own0_excluded": ("own_rows_form",),
    "padding_column_counted": ("padding_columns",),
}


class Case(object):
    def __init__(self, nblk, mod, K, which, seed):
        self.nblk, self.mod, self.K, self.which, self.seed = nblk, mod, K, which, seed
        self.rows = rows_of(nblk, mod)
        self.KP = 32 if K <= 32 else 64
        self.I, self.J = (self.rows, OTHER) if which == 0 else (OTHER, self.rows)
        self.id = "%s%d_nblk%d_K%d" % ("rows" if which == 0 else "cols", self.rows, nblk, K)
        self.edges = edges(self.rows, K, self.KP)

    def mask(self):
        rs = np.random.RandomState(self.seed + 17)
        M = (rs.rand(self.I, self.J) >= 0.3).astype(np.float64)
        M[0, :] = 1; M[:, 0] = 1
        return M

    def data(self):
        return np.random.RandomState(self.seed + 29).rand(self.I, self.J)

    def factors(self, fam, vb=False):
        """((exp, var) of the factor under test, (exp, var) of the other factor) in family fam"""
        return family(fam, self.rows, self.K, self.seed, vb), family(fam, OTHER, self.K, self.seed + 1, vb)


def _cases():
    out = []
    for i, nblk in enumerate(NBLK):
        for c, (KP, which) in enumerate(((32, 0), (64, 1), (32, 1), (64, 0))):
            ks = KS[KP]
            out.append(Case(nblk, MODS[(i + c) % 3], ks[(i + c // 2) % len(ks)], which, 100 * i + c))
    return out


CASES = _cases()
# the column-sum block's edges: what the variational cases (colsum2, S2T, XS; the maxima block beside it) run at
COLSUM_NBLK = (15, 16, 113, 120, 128, 129, 241, 257)
VB_CASES = [c for c in CASES if c.nblk in COLSUM_NBLK and (c.KP, c.which) in ((32, 0), (64, 1))]
TRI_CASES = [c for c in CASES if c.nblk in (17, 65, 129) and (c.KP, c.which) == (32, 0)]
TRIVB_CASES = TRI_CASES[:2]

# every class the cases must reach, at both paddings and in both directions
REQUIRED = ("rows_mod_32=0", "rows_mod_32=1", "rows_mod_32=31", "partial_last_block", "padding_columns", "snapW<KP",
            "colsum_groups_without_work", "first_batch_unrolled_for_group_0_only", "first_batch_unrolled_for_some_groups",
            "first_batch_unrolled_for_all_groups", "no_clamped_batch", "clamped_batch_with_1_live", "clamped_batch_with_4_live",
            "clamped_batch_with_5_live", "clamped_batch_with_7_live", "second_batch", "second_batch_unrolled", "third_batch",
            "stride_of_1_terms", "stride_of_2_terms", "stride_of_9_terms", "off_diagonal_tile_live", "last_tile_column_live")
# ... and every K in both directions of its own padding
REQUIRED_K = {"K=%d" % K: KP for KP, ks in KS.items() for K in ks}


def coverage(cases=None):
    """{class: {(KP, which), ...}} over the cases"""
    table = {}
    for c in (CASES if cases is None else cases):
        for e in c.edges:
            table.setdefault(e, set()).add((c.KP, c.which))
    return table


# ------------------------------------------------------------------------------------------------ sharded (own-rows form)
def shard_range(n, rank, world):
    """bnmtf_shard_range restated (the GPU test takes the ranges from the library and compares): rank r holds the units
    [n r // world, n (r + 1) // world).  With world <= n, which bnmtf_create insists on, no rank is left without units: the
    nblk = 0 launch of gram_reduce_kernel cannot be reached through the public constructor."""
    first = n * rank // world
    return first, n * (rank + 1) // world - first


# (I, J, K, world): shard starts inside a block in both directions, at both paddings
SHARDED = ((77, 45, 5, 2), (131, 70, 40, 3))
assert all(shard_range(n, r, w)[1] >= 1 for n in range(1, 200) for w in range(1, n + 1) for r in range(w))
