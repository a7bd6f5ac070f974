"""The relayout and the Gram behind every half sweep and every state upload (csrc/kernel_post.hip: post_kernel, gram_reduce_kernel,
gram_cast_kernel; the list forms post_many / gram_reduce_many) held to their bits at every launch shape.

Every statement goes through the library's read-only entry bnmtf_post_dump (what the kernels read: X, S2; what they wrote: XT, XT2,
S2T, XS, C64, C32, colsum, colsum2) and tests/_post_cases.py's NumPy model of the dumped inputs (its docstring: the order of the
additions, the two value families, the cases; test_post_cases_cpu.py: what the cases cover and which faults they would see).  No
tolerance anywhere: every output, every element, bit for bit.

  * after a state upload: bnmf_gibbs at every case and both families; bnmtf_gibbs (F and G); bnmf_vb on the pair-panel path (XS
    written) and on the masked-sum path (no XS, the maxima block beside the column-sum block) at the column-sum block's edges;
    bnmtf_vb
  * after run(3): the outputs are the model of the FINAL factor (the last relayout is ordered behind the last sweep), the two-stream
    order of the Gibbs loop gives the bits of the one-stream order, the last stored sample is the dumped factor (the packed rows,
    snapW < KP), and the same call gives the same bits again
  * sharded (in-process ranks): the Gram of a rank's own rows, summed over the ranks, and the layouts of the gathered factor
  * list forms: three variational models of different shapes in one run_many call, each against its own run()"""
import threading

import numpy as np
import pytest

import _post_cases as C
from bnmtf_amd import _lib, bnmf_gibbs_optimised, bnmf_vb_optimised, bnmtf_gibbs_optimised, bnmtf_vb_optimised, nmf_icm, run_many

pytestmark = pytest.mark.gpu

PRI = dict(alpha=1., beta=1., lambdaU=0.1, lambdaV=0.1)
PRI3 = dict(alpha=1., beta=1., lambdaF=0.1, lambdaS=0.1, lambdaG=0.1)
# every switch that chooses a path of the kernels under test, or the path that bypasses them: a test sets the ones it names
SWITCHES = ("BNMTF_SMALL", "BNMTF_VB_PATH", "BNMTF_TAIL", "BNMTF_EXCHANGE", "BNMTF_FORCE_COMM", "BNMTF_VB_GENERIC", "BNMTF_HANDOVER")
IDS = [c.id for c in C.CASES]


@pytest.fixture(autouse=True)
def _multi_launch_path(monkeypatch):
    for s in SWITCHES:
        monkeypatch.delenv(s, raising=False)
    monkeypatch.setenv("BNMTF_SMALL", "0")          # (read at create: no one-launch arena, the multi-launch kernels run)


def _ran_multi_launch(b):
    desc = b.describe()
    assert not b.is_small() and "small[" not in desc, desc


def _check(d, label, vb=False, xs=None, exact=False):
    """The dump d against the model of its own inputs: the lines of what differs."""
    assert d.vb == int(vb), (label, d.vb)
    assert not d.X[:, d.W:].any(), label                                  # the padding columns the model counts on
    if vb:
        assert not d.S2[:, d.W:].any(), label
    if xs is not None:
        assert (d.xs, d.umax) == (int(xs), int(not xs)), (label, d.xs, d.umax)
    want = C.model(d.X, d.S2 if vb else None, ldT=d.ldT, W=d.W)
    if vb and not d.xs:
        assert d.XS is None
        del want["XS"]
    if exact:                                                              # family X: the plain sums themselves
        Xd = d.X.astype(np.float64)
        assert np.array_equal(want["C64"], Xd.T @ Xd) and np.array_equal(want["colsum"], Xd.sum(0))
        if vb:
            assert np.array_equal(want["colsum2"], d.S2.astype(np.float64).sum(0))
    return ["%s: %s" % (label, line) for line in C.differences(d, want)]


def _place(case, a, b):
    """(the factor under test, the other one) -> (rows factor, cols factor)"""
    return (a, b) if case.which == 0 else (b, a)


# ------------------------------------------------------------------------------------------------ after a state upload
@pytest.mark.parametrize("case", C.CASES, ids=IDS)
def test_bnmf_gibbs_state_upload(case):
    b = bnmf_gibbs_optimised(case.data(), case.mask(), case.K, PRI, verbose=False, seed=3)
    fails = []
    for fam in C.FAMILIES:
        (ex, _), (oex, _) = case.factors(fam)
        b.U, b.V = _place(case, ex, oex)
        b.tau = 1.0
        b._push()
        _ran_multi_launch(b)
        d = C.post_dump(b._handle(), case.which)
        assert (d.rows, d.KP, d.W, d.nblk, d.n0, d.n) == (case.rows, case.KP, case.K, case.nblk, 0, case.rows)
        assert C.same_bits(d.X, C.padded(ex, case.KP))
        fails += _check(d, "%s family %s" % (case.id, fam), exact=fam == "X")
        o = C.post_dump(b._handle(), 1 - case.which)                      # the other factor: one block
        assert (o.rows, o.nblk) == (C.OTHER, 1)
        fails += _check(o, "%s family %s, the other factor" % (case.id, fam), exact=fam == "X")
    b.close()
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("which", [0, 1], ids=["F", "G"])
@pytest.mark.parametrize("case", C.TRI_CASES, ids=[c.id for c in C.TRI_CASES])
def test_bnmtf_gibbs_state_upload(case, which):
    K, L = (case.K, 7) if which == 0 else (7, case.K)
    I, J = (case.rows, C.OTHER) if which == 0 else (C.OTHER, case.rows)
    rs = np.random.RandomState(case.seed)
    M = (rs.rand(I, J) >= 0.3).astype(np.float64); M[0, :] = 1; M[:, 0] = 1
    b = bnmtf_gibbs_optimised(rs.rand(I, J), M, K, L, PRI3, verbose=False, seed=3)
    fails = []
    for fam in C.FAMILIES:
        F, _ = C.family(fam, I, K, case.seed)
        G, _ = C.family(fam, J, L, case.seed + 1)
        b.F, b.S, b.G, b.tau = F, np.ones((K, L)), G, 1.0
        b._push()
        _ran_multi_launch(b)
        d = C.post_dump(b._handle(), which)
        assert (d.rows, d.W, d.nblk) == (case.rows, case.K, case.nblk)
        assert C.same_bits(d.X, C.padded(F if which == 0 else G, d.KP))
        fails += _check(d, "%s %s family %s" % (case.id, "FG"[which], fam), exact=fam == "X")
    b.close()
    assert not fails, "\n".join(fails)


def _vb_moments(case, fam):
    (ex, var), (oex, ovar) = case.factors(fam, vb=True)
    return _place(case, ex, oex) + _place(case, var, ovar), ex, var


@pytest.mark.parametrize("path", ["pairs", "masked"])
@pytest.mark.parametrize("case", C.VB_CASES, ids=[c.id for c in C.VB_CASES])
def test_bnmf_vb_state_upload(monkeypatch, case, path):
    monkeypatch.setenv("BNMTF_VB_PATH", path)                              # (read when the model's layout is built)
    b = bnmf_vb_optimised(case.data(), case.mask(), case.K, PRI, verbose=False)
    fails = []
    for fam in C.FAMILIES:
        (b.expU, b.expV, b.varU, b.varV), ex, var = _vb_moments(case, fam)
        b.muU, b.tauU = np.ones((case.I, case.K)), np.ones((case.I, case.K))
        b.muV, b.tauV = np.ones((case.J, case.K)), np.ones((case.J, case.K))
        b.exptau = 1.0
        b._push()
        _ran_multi_launch(b)
        d = C.post_dump(b._handle(), case.which)
        assert (d.rows, d.KP, d.W, d.nblk) == (case.rows, case.KP, case.K, case.nblk)
        assert C.same_bits(d.X, C.padded(ex, case.KP))
        if fam == "X":                                                     # S2 = var + exp^2 was formed without a rounding
            assert np.array_equal(d.S2.astype(np.float64), C.padded(var, case.KP).astype(np.float64) + d.X.astype(np.float64) ** 2)
        fails += _check(d, "%s %s family %s" % (case.id, path, fam), vb=True, xs=path == "pairs", exact=fam == "X")
        o = C.post_dump(b._handle(), 1 - case.which)
        fails += _check(o, "%s %s family %s, the other factor" % (case.id, path, fam), vb=True, xs=path == "pairs", exact=fam == "X")
    b.close()
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("case", C.TRIVB_CASES, ids=[c.id for c in C.TRIVB_CASES])
def test_bnmtf_vb_state_upload(case):
    K, L = case.K, 5
    I, J = case.rows, C.OTHER
    b = bnmtf_vb_optimised(case.data(), case.mask(), K, L, PRI3, verbose=False)
    fails = []
    for fam in C.FAMILIES:
        b.expF, b.varF = C.family(fam, I, K, case.seed, vb=True)
        b.expG, b.varG = C.family(fam, J, L, case.seed + 1, vb=True)
        b.expS, b.varS = np.ones((K, L)), np.ones((K, L))
        b.exptau = 1.0
        b._push()
        _ran_multi_launch(b)
        for which, (ex, rows) in enumerate(((b.expF, I), (b.expG, J))):
            d = C.post_dump(b._handle(), which)
            assert d.rows == rows and C.same_bits(d.X, C.padded(ex, d.KP))
            fails += _check(d, "%s %s family %s" % (case.id, "FG"[which], fam), vb=True, exact=fam == "X")
    b.close()
    assert not fails, "\n".join(fails)


# ------------------------------------------------------------------------------------------------ after run(3)
RUN_I, RUN_J = 333, 257                # 11 and 9 blocks, the last ones of 13 rows and of 1 row


def _run_data(K):
    from bnmtf_amd.synthetic import generate_bnmf
    R, M, _, _ = generate_bnmf(RUN_I, RUN_J, K, 0.2, seed_data=11, seed_mask=12)
    rs = np.random.RandomState(5)
    return R, M, rs.exponential(1.0, (RUN_I, K)), rs.exponential(1.0, (RUN_J, K))


def _dumps(b):
    return [C.post_dump(b._handle(), w) for w in (0, 1)]


def _alive(d, K):
    """The chain did not collapse: a Gram that is wrong takes the sweeps that read it to zeros or NaNs, of which any Gram is
    trivially the model."""
    live = d.X[:, :K]
    assert np.isfinite(live).all() and np.count_nonzero(live) > live.size // 4, (np.isfinite(live).all(), np.count_nonzero(live), live.size)


def _same_dump(a, b):
    return [n for n, _ in C.DUMP_ARRAYS if (getattr(a, n) is None) != (getattr(b, n) is None)
            or (getattr(a, n) is not None and not C.same_bits(getattr(a, n), getattr(b, n)))]


@pytest.mark.parametrize("update", ["mode", "draw"])
@pytest.mark.parametrize("K", [31, 33])
def test_bnmf_gibbs_run_leaves_the_model_of_its_last_factor(monkeypatch, K, update):
    R, M, U0, V0 = _run_data(K)
    runs = {}
    for tail in ("overlap", "overlap", "serial"):                          # (read at create)
        monkeypatch.setenv("BNMTF_TAIL", tail)
        b = bnmf_gibbs_optimised(R, M, K, PRI, verbose=False, seed=9)
        b.U, b.V, b.tau = U0.copy(), V0.copy(), 0.7
        b.run(3, update=update)
        _ran_multi_launch(b)
        assert "tail=%s" % tail in b.describe(), b.describe()
        ds = _dumps(b)
        fails = []
        for w, (d, last) in enumerate(zip(ds, (b.all_U[-1], b.all_V[-1]))):
            fails += _check(d, "K=%d %s tail=%s factor %d" % (K, update, tail, w))
            assert d.W == K < d.KP
            _alive(d, K)
            assert C.same_bits(np.ascontiguousarray(d.X[:, :K]), np.ascontiguousarray(last, dtype=np.float32)), \
                "the last stored sample of factor %d is not the factor the device holds" % w
        assert not fails, "\n".join(fails)
        runs.setdefault(tail, []).append(ds)
        b.close()
    for w in (0, 1):
        assert not _same_dump(runs["overlap"][0][w], runs["overlap"][1][w]), "the same call twice, factor %d" % w
        assert not _same_dump(runs["overlap"][0][w], runs["serial"][0][w]), "BNMTF_TAIL=overlap against serial, factor %d" % w


@pytest.mark.parametrize("path", ["pairs", "masked"])
@pytest.mark.parametrize("K", [31, 33])
def test_bnmf_vb_run_leaves_the_model_of_its_last_factor(monkeypatch, K, path):
    monkeypatch.setenv("BNMTF_VB_PATH", path)
    R, M, _, _ = _run_data(K)
    runs = []
    for _ in range(2):
        b = bnmf_vb_optimised(R, M, K, PRI, verbose=False)
        b.initialise('exp')
        b.run(3)
        _ran_multi_launch(b)
        assert "vb_sweep=%s" % path in b.describe(), b.describe()
        ds = _dumps(b)
        fails = []
        for w, (d, ex) in enumerate(zip(ds, (b.expU, b.expV))):
            fails += _check(d, "K=%d %s factor %d" % (K, path, w), vb=True, xs=path == "pairs")
            _alive(d, K)
            assert np.array_equal(d.X[:, :K].astype(np.float64), ex)
        assert not fails, "\n".join(fails)
        runs.append(ds)
        b.close()
    for w in (0, 1):
        assert not _same_dump(runs[0][w], runs[1][w]), "the same call twice, factor %d" % w


# ------------------------------------------------------------------------------------------------ sharded
def _threads(world, work):
    out, err = [None] * world, [None] * world

    def run(rank):
        try:
            out[rank] = work(rank)
        except Exception as e:      # noqa: BLE001 -- reported by the main thread
            err[rank] = e

    ts = [threading.Thread(target=run, args=(r,)) for r in range(world)]
    for t in ts:
        t.start()
    for t in ts:
        t.join(timeout=120)
    assert not any(t.is_alive() for t in ts), "a rank hung"
    assert all(e is None for e in err), err
    return out


@pytest.mark.parametrize("exchange", ["streams", "serial"])
@pytest.mark.parametrize("I,J,K,world", C.SHARDED)
def test_sharded_own_rows_gram_and_gathered_layouts(monkeypatch, I, J, K, world, exchange):
    """Family X through a run: ICM updates on data that are negative throughout take every mode to the lower clamp (minimum_TN = 2^-1),
    so the factors the sweeps write are 1/2 in every live column -- every Gram entry is rows / 4 and every column sum rows / 2,
    exact in any order of the ranks' partial sums (the all-reduce's order is not this test's subject), and a row counted twice, or
    by no rank, or a block taken from the wrong start moves them.  The shard starts lie inside a block of 32 rows."""
    if exchange == "serial":
        monkeypatch.setenv("BNMTF_EXCHANGE", "serial")
    rs = np.random.RandomState(I + world)
    M = (rs.rand(I, J) >= 0.2).astype(np.float64); M[0, :] = 1; M[:, 0] = 1
    R = -1.0 - rs.rand(I, J)
    cid = (b"BNMTFLOC" + b"post%d%s" % (world, exchange.encode())).ljust(128, b"\0")
    U0, _ = C.family_X(I, K, 1); V0, _ = C.family_X(J, K, 2)

    def work(rank):
        b = nmf_icm(R, M, K, PRI, verbose=False, seed=7, rank=rank, world=world, comm_id=cid)
        b.U, b.V, b.tau = U0.copy(), V0.copy(), 1.0
        b.run(2, minimum_TN=0.5)
        ds = _dumps(b)
        b.close()
        return ds

    ranks = _threads(world, work)
    inside = 0
    for rank, ds in enumerate(ranks):
        for w, (d, n) in enumerate(zip(ds, (I, J))):
            first, count = _lib_shard_range(n, rank, world)
            assert (first, count) == C.shard_range(n, rank, world) == (d.n0, d.n) and count >= 1
            inside += int(first % 32 != 0)
            KP = d.KP
            X = np.zeros((n, KP), dtype=np.float32); X[:, :K] = 0.5
            assert C.same_bits(d.X, X), "rank %d factor %d: the gathered factor" % (rank, w)
            want = C.model(X, ldT=d.ldT, W=K)                              # (exact: the whole factor's sums in any order)
            assert np.array_equal(want["C64"][:K, :K], np.full((K, K), n / 4.0)) and np.array_equal(want["colsum"][:K], np.full(K, n / 2.0))
            fails = ["rank %d factor %d: %s" % (rank, w, line) for line in C.differences(d, want)]
            assert not fails, "\n".join(fails)
    assert inside >= 2 * (world - 1)                                       # every later rank starts inside a block, both directions


def _lib_shard_range(n, rank, world):
    import ctypes
    first, count = ctypes.c_int64(), ctypes.c_int64()
    _lib.check(_lib.lib().bnmtf_shard_range(n, rank, world, ctypes.byref(first), ctypes.byref(count)))
    return first.value, count.value


# ------------------------------------------------------------------------------------------------ list forms
MANY = ((333, 70, 31), (97, 257, 33), (160, 129, 5))


def _vb_model(I, J, K):
    rs = np.random.RandomState(I + K)
    M = (rs.rand(I, J) >= 0.25).astype(np.float64); M[0, :] = 1; M[:, 0] = 1
    b = bnmf_vb_optimised(rs.rand(I, J) * 3, M, K, PRI, verbose=False)
    b.initialise('exp')
    return b


def test_the_list_forms_write_what_the_single_launches_write():
    alone = []
    for shape in MANY:
        b = _vb_model(*shape)
        b.run(3)
        alone.append(_dumps(b))
        b.close()
    ms = [_vb_model(*shape) for shape in MANY]
    run_many(ms, 3)
    fails = []
    for i, (m, shape) in enumerate(zip(ms, MANY)):
        _ran_multi_launch(m)
        assert m._many_info[0] == len(MANY), "model %d: %d models shared launches (post_many, gram_reduce_many)" % (i, m._many_info[0])
        for w, d in enumerate(_dumps(m)):
            fails += _check(d, "model %d %s factor %d" % (i, shape, w), vb=True)
            fails += ["model %d %s factor %d: %s differs from the model run alone" % (i, shape, w, n) for n in _same_dump(d, alone[i][w])]
        m.close()
    assert not fails, "\n".join(fails)


# ------------------------------------------------------------------------------------------------ the hook itself
def test_the_dump_reads_only_and_refuses_what_has_no_buffers(monkeypatch):
    case = C.CASES[0]
    b = bnmf_gibbs_optimised(case.data(), case.mask(), case.K, PRI, verbose=False, seed=3)
    (ex, _), (oex, _) = case.factors("G")
    b.U, b.V = _place(case, ex, oex); b.tau = 1.0
    b._push()
    first, again = C.post_dump(b._handle(), case.which), C.post_dump(b._handle(), case.which)
    assert not _same_dump(first, again) and first.S2 is None and first.XS is None and first.colsum2 is None
    info = np.zeros(C.DUMP_INFO_LEN, dtype=np.int64)
    assert C.raw_dump(b._handle(), 2, info, [None] * len(C.DUMP_ARRAYS)) != 0
    b.close()
    monkeypatch.delenv("BNMTF_SMALL")                                       # a model on the one-launch path: no such buffers
    s = bnmf_gibbs_optimised(np.random.RandomState(1).rand(40, 30), np.ones((40, 30)), 4, PRI, verbose=False, seed=3)
    s.initialise()
    s._push()
    assert s.is_small()
    assert C.raw_dump(s._handle(), 0, info, [None] * len(C.DUMP_ARRAYS)) == -5, "BNMTF_ESTATE expected"
    s.close()
