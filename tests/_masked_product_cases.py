"""Cases of the exact tests of the variational sweep's masked product (csrc/kernel_maskgemm.hip: out[u][c] = sum over the
MISSING inner indices r of unit u of x[r][c], x = [S2 | E^2] of the other factor) and a NumPy model of what the device returns
through the hook bnmf_vb_masked_sums, bit for bit.  The GPU side: test_masked_product_exact_gpu.py; the pins of the cases
themselves: test_masked_product_cases_cpu.py.

The kernel's arithmetic is integer until one fp32 combine per inner slice (slab), so the result is a deterministic function of
its inputs:
  planes()        vb_colmax_kernel + vb_planes_kernel: column c on a grid of 22 bits below 2^e_c > max_r x[r][c], an element
                  n = rint(x 2^(22 - e_c)) as three balanced base-256 digits;
  slab_digit_sums the three integer digit sums of every (unit, column) per slab s = inner rows [s mipw, (s + 1) mipw);
  combine()       fmaf(D0, 65536, fmaf(D1, 256, D2)) in fp32 -- two single roundings --, then ldexp by e_c - 22 (exact);
  device_sums()   the slabs added in slab order in fp32, from 0.f (bnmf_vb_masked_sums, slab_sum_ordered).
geometry() restates the launch: n_pad / inner_pad from build_dir (csrc/api.hip), msplit / mipw from ensure_vb
(csrc/api_models.inc), the block grid, the XCD remap and the wrap-round start of maskgemm_kernel.  The GPU test compares it with
what the handle reports (describe(): masked_product[...]) before it compares values.

Value families, set through expU / varU / expV / varV (the device forms S2 = fp32(var + fp32(exp exp)); so does operand()):
  X  split-independent and exact.  Column k: exp = i 2^t, var = v 2^(2t), integers i <= 15, v >= 0, q = v + i^2 <= 255, t = t_k
     in [-40, 40]; one pinned row per column (a different row in every column) holds i = 15, v = 30 at t_k + o_k, o_k in
     {0, 3, 5, 7}: the column's maximum 255 2^(2 (t + o)) puts the grid step at 2^(2t + 2o - 14), every element on the grid, and
     -- the four offsets -- the elements into different digit planes.  Every partial and total sum is (an integer below 2^24)
     2^(2t) (asserted per case on the CPU: sum_bound), so the expected value is the exact fp64 product miss @ x whatever the
     split, with no model in between.
  G  general: exp = 10^U(-4, 1), var = 10^U(-6, 0) as tests/test_bnmf_vb_gpu.py, 5 % zeros, and (K >= 5) an all-zero column, a
     column whose maxima are exact powers of two, a column scaled by 2^60 and one by 2^-60.  Every value is a normal fp32;
     subnormal moments are out of scope (v_ldexp_f32 and the conversions may flush them).  K < KP in every case: padding
     columns exist.  Expected: device_sums(), bit for bit.
X proves the product (every step counted once, the right mask word against the right digit rows); G proves the combine, the
exponents and the slab order.

Masks: 30-50 % missing at random, and (I, J >= 3) row 0 / column 0 with every entry missing but one, row 1 / column 1 with none
missing, entry (I - 1, J - 1) missing.  A unit with EVERY entry missing cannot exist in a model: the constructor refuses a fully
unobserved row or column as the reference does (check_R_M), so the fullest unit keeps one observed entry -- in the unit without
missing entries of the other direction.  No inner extent is a multiple of 32 except where the step count needs it.
"""
import numpy as np

NSET = 6                       # maskgemm_kernel's operand ring: sets of one step each
TWO24 = 1 << 24


def _ru(x, q):
    return -(-x // q) * q


def geometry(n, m, K):
    """The masked product's launch for a direction of n units, m inner rows, K factor columns."""
    KP = 32 if K <= 32 else 64
    n_pad = _ru(max(n, 1), 128)
    # build_dir: the contraction's split fixes the padded inner extent
    tw = 2 if KP == 64 and n_pad <= 2048 else 4
    split = min(max(1, 256 // (n_pad // (32 * tw))), max(1, m // 256))
    ipw = _ru(-(-m // (split * 4)), 32)
    inner_pad = split * 4 * ipw
    # ensure_vb: inner slices of the masked product
    ncg = 2 * KP // 32                      # waves per unit group
    ugpb = 4 // ncg                         # unit groups (128 units) per block
    nug = n_pad // 128
    nx = -(-nug // ugpb)
    msplit = 1
    while msplit < 8 and nx * msplit * 2 <= 256 and inner_pad % (32 * msplit * 2) == 0:
        msplit *= 2
    mipw = inner_pad // msplit
    nb = nx * msplit
    return dict(KP=KP, n_pad=n_pad, inner_pad=inner_pad, msplit=msplit, mipw=mipw, nsteps=mipw // 32, ncg=ncg, ugpb=ugpb, nug=nug,
                nx=nx, nb=nb, remap=nb % 8 == 0 and 8 % msplit == 0, dead=ugpb == 2 and nug % 2 == 1)


def block_of(g, blockidx):
    """maskgemm_kernel: block id -> (unit-group slot bx, inner slice s)"""
    bx, s = blockidx % g["nx"], blockidx // g["nx"]
    if g["remap"]:
        per = 8 // g["msplit"]
        xcd, li = blockidx & 7, blockidx >> 3
        s, bx = xcd // per, li * per + xcd % per
    return bx, s


def start_step(g, bx):
    """the step a block's walk of its slice starts at"""
    return (bx * 11) % g["nsteps"]


def step_class(nsteps):
    if nsteps < NSET:
        return "below the ring (%d steps)" % nsteps
    q, r = divmod(nsteps, NSET)
    return "%d ring%s%s (%d steps)" % (q, "s" if q > 1 else "", " + %d" % r if r else "", nsteps)


# ------------------------------------------------------------------ cases
class Case:
    def __init__(self, I, J, K, rows, cols, note=""):
        self.I, self.J, self.K, self.note = I, J, K, note
        self.expect = {"rows": rows, "cols": cols}           # (msplit, nsteps) of each direction

    @property
    def id(self):
        return "%dx%dx%d" % (self.I, self.J, self.K)

    @property
    def seed(self):
        return (self.I * 7919 + self.J * 104729 + self.K * 31) % (2 ** 31)

    def shape(self, d):
        """(n units, m inner rows) of a direction"""
        return (self.I, self.J) if d == "rows" else (self.J, self.I)

    def geometry(self, d):
        return geometry(*self.shape(d), self.K)

    @property
    def claims(self):
        """a case without a missing entry checks that nothing is counted; it cannot see a defect of the product"""
        return min(self.I, self.J) >= 3


DIRS = ("rows", "cols")
FAMILIES = ("X", "G")

# (I, J, K), then (msplit, nsteps) of the rows' product (n = I, m = J) and of the columns' (n = J, m = I)
CASES = [
    Case(1, 1, 1, (4, 1), (4, 1), "nothing missing; dead pair, no remap"),
    # KP = 64 (NCG = 4)
    Case(385, 1025, 40, (8, 6), (8, 2), "one ring; nx = 4 | nx = 9"),
    Case(130, 2049, 40, (8, 12), (8, 1), "two rings | nx = 17, one step"),
    Case(129, 3329, 40, (4, 39), (8, 1), "six rings + 3, a block of one real unit | nx = 27"),
    Case(257, 3328, 40, (8, 13), (4, 3), "two rings + 1, nx = 3 | nx = 26, remap at msplit 4"),
    Case(257, 1792, 40, (8, 7), (4, 3), "one ring + 1"),
    Case(257, 1280, 40, (8, 5), (4, 3), "one short of the ring"),
    Case(8321, 513, 40, (2, 12), (4, 75), "msplit 2, nx = 66, no remap | nx = 5, no remap, a long walk"),
    Case(16513, 257, 40, (1, 12), (8, 84), "msplit 1, nx = 130, no remap | a long walk"),
    # KP = 32 (NCG = 2: two unit groups per block)
    Case(641, 1793, 7, (4, 21), (8, 3), "nx = 3, no remap, three rings + 3 | dead pair"),
    Case(129, 129, 7, (8, 1), (8, 1), "one step per slab"),
    Case(257, 385, 7, (8, 2), (4, 3), "dead pair | nx = 2"),
    Case(257, 1280, 7, (8, 5), (4, 3), "dead pair"),
    Case(257, 1025, 7, (8, 6), (4, 3), "dead pair, one ring | dead pair, no remap"),
    Case(513, 1792, 7, (8, 7), (8, 3), "dead pair, one ring + 1, nx = 3"),
    Case(257, 2049, 7, (8, 12), (4, 3), "dead pair, two rings"),
    Case(257, 3328, 7, (8, 13), (4, 3), "dead pair, two rings + 1 | nx = 13, no remap"),
    Case(16641, 129, 7, (2, 4), (4, 195), "msplit 2, dead pair, nx = 66, no remap | a long walk"),
    Case(33000, 129, 7, (1, 8), (8, 192), "msplit 1, nx = 129, no remap | the longest walk"),
]

# what the cases must cover between them, per KP where the kernel's instantiation can get there (test_masked_product_cases_cpu.py)
NSTEPS_CLASSES = (1, 2, 5, 6, 7, 12, 13)
MSPLIT_CLASSES = (1, 2, 4, 8)
# a dead wave pair needs two unit groups per block: NCG = 2, i.e. KP = 32.  Everything else is reached for both KP below
# 4.5 10^6 matrix entries.
UNREACHABLE = {(64, "dead pair, nsteps >= 6"): "KP = 64 runs one unit group per block (NCG = 4): no wave pair without units"}


def mask(case):
    """M [I][J] (1 = observed) of a case"""
    I, J = case.I, case.J
    rs = np.random.RandomState(case.seed)
    frac = rs.uniform(0.3, 0.5)
    M = (rs.rand(I, J) >= frac).astype(np.float64)
    if min(I, J) >= 3:
        M[0, :] = 0; M[:, 0] = 0                 # the fullest units: one observed entry each ...
        M[1, :] = 1; M[:, 1] = 1                 # ... in the units without a missing entry
        M[I - 1, J - 1] = 0                      # the last unit's last inner index
    else:
        M[:] = 1
    assert M.sum(0).min() >= 1 and M.sum(1).min() >= 1
    return M


_OFFSETS = (0, 3, 5, 7)


def moments(case, fam):
    """(expU, varU, expV, varV) of a family, fp64 arrays of fp32 values"""
    rs = np.random.RandomState(case.seed + (17 if fam == "X" else 29))
    out = []
    for rows in (case.I, case.J):
        K = case.K
        if fam == "X":
            t = rs.randint(-40, 41, K)
            i = rs.randint(0, 16, (rows, K))
            v = (rs.rand(rows, K) * (256 - i * i)).astype(np.int64)           # v + i^2 <= 255
            ex = np.ldexp(i.astype(np.float64), t[None, :])
            var = np.ldexp(v.astype(np.float64), 2 * t[None, :])
            for k in range(K):                                               # the pinned element: the column's maximum
                p, o = (k * 7919 + 3) % rows, _OFFSETS[k % 4]
                ex[p, k] = np.ldexp(15.0, t[k] + o); var[p, k] = np.ldexp(30.0, 2 * (t[k] + o))
        else:
            ex = 10.0 ** rs.uniform(-4, 1, (rows, K)); var = 10.0 ** rs.uniform(-6, 0, (rows, K))
            zero = rs.rand(rows, K) < 0.05
            ex[zero] = 0; var[zero] = 0
            if K >= 5:
                ex[:, 1] = 0; var[:, 1] = 0                                   # an all-zero column
                ex[:, 2] = 10.0 ** rs.uniform(-4, 0, rows); var[:, 2] = 10.0 ** rs.uniform(-6, 0, rows)
                p = (5 * 7919 + 3) % rows
                ex[p, 2] = 2.0; var[p, 2] = 4.0                               # maxima 8 (S2) and 4 (E^2): exact powers of two
        ex = ex.astype(np.float32).astype(np.float64); var = var.astype(np.float32).astype(np.float64)
        if fam == "G" and K >= 5:                                            # (exact scalings of the fp32 values)
            ex[:, 3] = np.ldexp(ex[:, 3], 30); var[:, 3] = np.ldexp(var[:, 3], 60)
            ex[:, 4] = np.ldexp(ex[:, 4], -30); var[:, 4] = np.ldexp(var[:, 4], -60)
        tiny = np.finfo(np.float32).tiny
        for a in (ex, var, ex * ex):
            assert np.all((a == 0) | (a >= tiny)) and np.all(a < 2.0 ** 120)   # normal fp32, squares included
        out += [ex, var]
    return tuple(out)


def operand(ex, var):
    """[S2 | E^2] as the device holds it: fp32(var + fp32(exp exp)), fp32(exp exp) -- [rows][2 K] float32"""
    e = np.asarray(ex).astype(np.float32); v = np.asarray(var).astype(np.float32)
    e2 = e * e
    return np.concatenate([v + e2, e2], axis=1)


def problem(case, fam, d, M=None, mom=None):
    """(miss [n][m] bool, x [m][2 K] float32) of one direction's product"""
    M = mask(case) if M is None else M
    eU, vU, eV, vV = moments(case, fam) if mom is None else mom
    if d == "rows":
        return M == 0, operand(eV, vV)
    return M.T == 0, operand(eU, vU)


# ------------------------------------------------------------------ the device's arithmetic
def column_exponents(x):
    """e_c: 2^e > the column's largest element (its exponent field + 1; a zero column: 0)"""
    bits = np.asarray(x, dtype=np.float32).max(0).view(np.uint32)
    return np.where(bits != 0, ((bits >> 23) & 255).astype(np.int64) - 126, 0)


def planes(x, e=None):
    """vb_colmax_kernel + vb_planes_kernel: x [rows][cols] non-negative fp32 -> (e[cols], d0, d1, d2 int8-range arrays, n)."""
    x = np.asarray(x, dtype=np.float32)
    if e is None:
        e = column_exponents(x)
    n = np.rint(np.ldexp(x.astype(np.float64), (22 - e)[None, :])).astype(np.int64)  # 0 .. 2^22 (ldexpf + v_cvt_i32_f32, RNE)
    d2 = ((n + 128) & 255) - 128
    n1 = (n - d2) >> 8
    d1 = ((n1 + 128) & 255) - 128
    d0 = (n1 - d1) >> 8
    return e, d0, d1, d2, n


def combine(D0, D1, D2, e):
    """a slab's value from its digit sums: fmaf(D0, 65536, fmaf(D1, 256, D2)) in fp32, scaled by 2^(e - 22)"""
    f = [np.asarray(D).astype(np.float32) for D in (D0, D1, D2)]                          # v_cvt_f32_i32 (exact below 2^24)
    inner = (f[1].astype(np.float64) * 256.0 + f[2].astype(np.float64)).astype(np.float32)     # exact in fp64, one rounding
    tot = (f[0].astype(np.float64) * 65536.0 + inner.astype(np.float64)).astype(np.float32)    # the outer FMA: one rounding
    return np.ldexp(tot, (np.asarray(e) - 22)[None, :].astype(np.int32)).astype(np.float32)


def masked_sums(miss, x):
    """maskgemm_kernel with ONE slab: (values, the three digit sums)"""
    e, d0, d1, d2, _ = planes(x)
    mi = miss.astype(np.int64)
    D0, D1, D2 = mi @ d0, mi @ d1, mi @ d2
    return combine(D0, D1, D2, e), (D0, D1, D2)


def _matmul_int(mi, d):
    """exact integer product through fp64 (every sum far below 2^53)"""
    return np.rint(mi @ d.astype(np.float64)).astype(np.int64)


def slab_digit_sums(miss, digits, g):
    """D [msplit][3][n][cols]: the digit sums of slab s = inner rows [s mipw, (s + 1) mipw) (rows >= m: zero planes, zero bits)"""
    m = miss.shape[1]
    out = []
    for s in range(g["msplit"]):
        a, b = min(s * g["mipw"], m), min((s + 1) * g["mipw"], m)
        mi = miss[:, a:b].astype(np.float64)
        out.append([_matmul_int(mi, d[a:b]) for d in digits])
    return np.array(out)


def add_slabs(slabs, order=None):
    """the slabs in slab order, in fp32, from 0.f"""
    acc = np.zeros_like(slabs[0], dtype=np.float32)
    for s in (range(len(slabs)) if order is None else order):
        acc = (acc + slabs[s]).astype(np.float32)
    return acc


def device_sums(miss, x, g, e=None, parts=False):
    """What bnmf_vb_masked_sums returns for one direction: [n][cols] float32 (cols = 2 K: asq | vsq)"""
    e, d0, d1, d2, _ = planes(x, e)
    D = slab_digit_sums(miss, (d0, d1, d2), g)
    slabs = [combine(D[s][0], D[s][1], D[s][2], e) for s in range(g["msplit"])]
    out = add_slabs(slabs)
    return (out, e, (d0, d1, d2), D, slabs) if parts else out


def exact_sums(miss, x):
    """the fp64 product (family X: exactly representable, the expected value itself)"""
    return miss.astype(np.float64) @ np.asarray(x).astype(np.float64)


def sum_bound(miss, x):
    """Family X: the largest sum of a (unit, column), in units of the column's smallest power of two that divides every element
    -- below 2^24 means that every partial sum of the product, in any order and under any split, is an exact fp32."""
    x = np.asarray(x).astype(np.float64)
    worst = 0
    for c in range(x.shape[1]):
        col = x[:, c]
        nz = col[col > 0]
        if nz.size == 0:
            continue
        mant, ex = np.frexp(nz)
        # the exponent of the lowest set bit of each element: mantissas have at most 24 bits
        low = ex - 24 + np.array([(int(v) & -int(v)).bit_length() - 1 for v in np.ldexp(mant, 24).astype(np.int64)])
        unit = low.min()
        q = np.ldexp(col, -int(unit))
        assert np.all(q == np.rint(q))
        worst = max(worst, float((miss.astype(np.float64) @ q).max()))
    return worst


def expected(case, fam, d, M=None, mom=None):
    """(asq, vsq) [n][K] float32 the hook must return, and the geometry"""
    miss, x = problem(case, fam, d, M, mom)
    g = case.geometry(d)
    if fam == "X":
        ref = exact_sums(miss, x)
        out = ref.astype(np.float32)
        assert np.array_equal(out.astype(np.float64), ref)
    else:
        out = device_sums(miss, x, g)
    return out[:, :case.K], out[:, case.K:], g


# ------------------------------------------------------------------ defects (test_masked_product_cases_cpu.py)
class View:
    """One direction's product with its parts kept, for the defects below."""

    def __init__(self, case, fam, d, M=None, mom=None):
        self.case, self.fam, self.d = case, fam, d
        self.miss, self.x = problem(case, fam, d, M, mom)
        self.n, self.m = self.miss.shape
        self.g = case.geometry(d)
        self.out, self.e, self.digits, self.D, self.slabs = device_sums(self.miss, self.x, self.g, parts=True)

    def units(self, bx):
        """the real units of block bx"""
        a = bx * self.g["ugpb"] * 128
        return np.arange(a, min(a + self.g["ugpb"] * 128, self.n))

    def rows(self, s, step):
        """the real inner rows of step `step` of slab s (step = nsteps: the step behind the slab)"""
        a = s * self.g["mipw"] + 32 * step
        return np.arange(min(a, self.m), min(a + 32, self.m))

    def partial(self, units, mrows, drows=None):
        """[3][units][cols]: the mask bits of rows mrows against the digit rows drows (the same rows unless given)"""
        drows = mrows if drows is None else drows
        k = min(len(mrows), len(drows))
        mi = self.miss[np.ix_(units, mrows[:k])].astype(np.float64)
        return np.array([_matmul_int(mi, d[drows[:k]]) for d in self.digits])

    def with_slab(self, units, s, D3):
        """the output of `units` with the digit sums of slab s replaced by D3 [3][units][cols]"""
        slabs = [sl[units] for sl in self.slabs]
        slabs[s] = combine(D3[0], D3[1], D3[2], self.e)
        return add_slabs(slabs)

    def changed(self, units, s, delta):
        """does adding delta to slab s's digit sums of `units` change an output element?"""
        D3 = self.D[s][:, units, :] + delta
        return bool(np.any(self.with_slab(units, s, D3).view(np.uint32) != self.out[units].view(np.uint32)))

    def block_slots(self):
        """the block slots the defects are tried in: the first three (their walks start at steps 0, 11, 22 mod nsteps), a middle one, the last"""
        nx = self.g["nx"]
        return sorted({0, min(1, nx - 1), min(2, nx - 1), nx // 2, nx - 1})

    def blocks(self):
        """(bx, s) to try: every slab; the block slots of block_slots() that hold real units and real rows"""
        for s in range(self.g["msplit"]):
            for bx in self.block_slots():
                if len(self.units(bx)) and len(self.rows(s, 0)):
                    yield bx, s

    def sites(self):
        """(bx, s, walk position i, step) to try: every slab; the block slots of block_slots(); every position of a short
        walk, of a long one the positions round the ring's edges and the ends -- where the block holds real units and the step real rows"""
        g = self.g
        ns = g["nsteps"]
        pos = range(ns) if ns <= 2 * NSET + 1 else sorted({0, 1, NSET - 2, NSET - 1, NSET, NSET + 1, 2 * NSET - 1, 2 * NSET, 2 * NSET + 1, ns - 2, ns - 1})
        for s in range(g["msplit"]):
            for bx in self.block_slots():
                if len(self.units(bx)) == 0:
                    continue
                g0 = start_step(g, bx)
                for i in pos:
                    step = (g0 + i) % ns
                    if len(self.rows(s, step)):
                        yield bx, s, i, step


def defect_step_skipped(v, bx, s, i, step):
    u = v.units(bx)
    return v.changed(u, s, -v.partial(u, v.rows(s, step)))


def defect_step_twice(v, bx, s, i, step):
    u = v.units(bx)
    return v.changed(u, s, v.partial(u, v.rows(s, step)))


def defect_stale_ring_set(v, bx, s, i, step):
    """the step's digit planes from the set that was not reloaded: those of the walk's step NSET - 1 earlier"""
    if i < NSET - 1:
        return None
    u = v.units(bx)
    old = (start_step(v.g, bx) + i - (NSET - 1)) % v.g["nsteps"]
    mr, dr = v.rows(s, step), v.rows(s, old)
    return v.changed(u, s, v.partial(u, mr, dr) - v.partial(u, mr))        # (digit rows >= m: zero planes)


def defect_wrap_off_by_one(v, bx, s):
    """at(): `g > nsteps` for `g >= nsteps` -- a walk that starts at g0 > 0 reads the step behind its slice instead of step 0"""
    if start_step(v.g, bx) == 0 or len(v.rows(s, 0)) == 0:
        return None
    u = v.units(bx)
    behind = v.rows(s, v.g["nsteps"])
    delta = -v.partial(u, v.rows(s, 0))
    if len(behind):
        # (the mask words and the digit rows of the next slab's first step: both operands move together)
        delta = delta + v.partial(u, behind)
    return v.changed(u, s, delta)


def defect_plane_dropped(v, bx, s, plane):
    u = v.units(bx)
    D3 = v.D[s][:, u, :].copy()
    if not D3[plane].any():
        return None
    D3[plane] = 0
    return bool(np.any(v.with_slab(u, s, D3).view(np.uint32) != v.out[u].view(np.uint32)))


def defect_next_tiles_mask(v, bx, s):
    """the first unit tile of the block reads the mask words of the tile behind it (units + 32; zero behind n)"""
    u = v.units(bx)[:32]
    src = u + 32
    a, b = min(s * v.g["mipw"], v.m), min((s + 1) * v.g["mipw"], v.m)
    mi = np.zeros((len(u), b - a))
    ok = src < v.n
    mi[ok] = v.miss[src[ok], a:b]
    D3 = np.array([_matmul_int(mi, d[a:b]) for d in v.digits])
    if np.array_equal(D3, v.D[s][:, u, :]):
        return None
    return bool(np.any(v.with_slab(u, s, D3).view(np.uint32) != v.out[u].view(np.uint32)))


def defect_pads_counted(v):
    """mask bits at inner indices >= m and of units >= n set: the output the hook would return (the digit rows >= m are zero --
    vb_planes_kernel -- and the hook returns the units below n)"""
    g = v.g
    missp = np.ones((g["n_pad"], g["inner_pad"]), dtype=bool)
    missp[:v.n, :v.m] = v.miss
    xp = np.zeros((g["inner_pad"], v.x.shape[1]), dtype=np.float32)
    xp[:v.m] = v.x
    return device_sums(missp, xp, g, e=v.e)[:v.n]


def defect_slab_order_reversed(v):
    return bool(np.any(add_slabs(v.slabs, order=range(v.g["msplit"] - 1, -1, -1)).view(np.uint32) != v.out.view(np.uint32)))


def defect_exponent_one_too_large(v):
    nz = v.x.max(0) > 0
    return bool(np.any(device_sums(v.miss, v.x, v.g, e=v.e + nz.astype(np.int64)).view(np.uint32) != v.out.view(np.uint32)))


def first_mismatch(case, fam, d, which, got, want, g):
    """The report of a failed comparison: the first differing (unit, column) of asq | vsq, where it sits in the launch, the two values"""
    bad = np.argwhere(got.view(np.uint32) != want.view(np.uint32))
    u, c = (int(t) for t in bad[0])
    bx = u // (128 * g["ugpb"])
    blocks = [b for b in range(g["nb"]) if block_of(g, b)[0] == bx]
    return ("%s family %s %s (which = %d): %d of %d elements differ; first at unit %d, column %d (%s[%d]): expected %r (bits %08x), got %r (bits %08x).  "
            "The unit sits in tile %d of unit group %d, block slot bx = %d (blocks %s, one per slab 0..%d), whose walk starts at step %d of %d: %s; "
            "msplit = %d, mipw = %d, n_pad = %d, inner_pad = %d, remap = %s, dead pair = %s" % (
                case.id, fam, d, which, len(bad), got.size, u, c, "asq" if c < case.K else "vsq", c % case.K,
                float(want[u, c]), int(want.view(np.uint32)[u, c]), float(got[u, c]), int(got.view(np.uint32)[u, c]),
                (u % 128) // 32, u // 128, bx, blocks, g["msplit"] - 1, start_step(g, bx), g["nsteps"], step_class(g["nsteps"]),
                g["msplit"], g["mipw"], g["n_pad"], g["inner_pad"], g["remap"], g["dead"]))
