"""nmf_np.NMF and nmtf_np.NMTF with layout='observed' (csrc/kernel_obs_np.hip, api_obs_np.inc) on the
device, against the fp64 restatement of the reference's updates (tests/_np_restatement.py, pinned to the reference by
tests/golden/np.npz) at every launch shape of tests/_obs_np_cases.py, against the dense layout, and bit for bit against itself:
the long form, a second run, run(2); run(3), the columns one by one.

The tolerances are the project's own for these models (tests/test_np_shapes_gpu.py): TOL_ONE = 1e-5 for one iteration or one
update, TOL_DRIFT = 2e-5 for five iterations -- ten times the worst fp32-against-fp64 error measured for the dense kernels,
nothing measured on this code.  Every test records its errors (record_property)."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import bnmtf_amd
from bnmtf_amd import NMF, NMTF, _lib, bnmf_gibbs_optimised, bnmtf_gibbs_optimised

import _np_restatement as NR
import _obs_np_cases as OC

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL_ONE = 1e-5             # one iteration / one update: factors and metrics
TOL_DRIFT = 2e-5           # five iterations
TOL_F64 = 1e-9             # predict() / compute_I_div(): fp64 on both sides from the same fp32 factors, only the order of the sums differs


def f32(X):
    return np.asarray(X, dtype=np.float32).astype(np.float64)


def run_capturing_idiv(model, iterations, capsys):
    model.verbose = True
    model.run(iterations)
    model.verbose = False
    lines = [l for l in capsys.readouterr().out.splitlines() if l.startswith("Iteration ")]
    assert len(lines) == iterations
    return np.array([float(l.split("I-divergence: ")[1].split(". MSE")[0]) for l in lines])


def metric_errors(model, idiv, ref, it=0):
    got = {"MSE": model.all_performances["MSE"][it], "R^2": model.all_performances["R^2"][it], "Rp": model.all_performances["Rp"][it],
           "I_div": idiv[it]}
    return {m: abs(got[m] - ref[m]) / abs(ref[m]) for m in got}


def check(errs, tol, record_property, prefix=""):
    for name, e in errs.items():
        record_property(prefix + name, "%.3e" % e)
    bad = {n: e for n, e in errs.items() if not e <= tol}
    assert not bad, (bad, tol)


# ---------------------------------------------------------------- one iteration at every launch shape
@pytest.mark.parametrize("shape", sorted(OC.NMF_SHAPES))
def test_nmf_iteration_at_every_launch_shape(shape, capsys, record_property):
    M, K = OC.NMF_SHAPES[shape]()
    assert M.sum(axis=0).min() > 0 and M.sum(axis=1).min() > 0
    R, U0, V0 = OC.nmf_problem(M, K)
    n = OC.nmf_model(R, M, K, U0, V0, layout='observed')
    idiv = run_capturing_idiv(n, 1, capsys)
    U, V = NR.ref_nmf_iteration(R, M, U0, V0)
    errs = {"U": NR.rel_err(n.U, U), "V": NR.rel_err(n.V, V)}
    errs.update(metric_errors(n, idiv, NR.metrics(R, M, U @ V.T)))
    assert len(n.all_times) == 1 and n.all_times[0] > 0
    n.close()
    check(errs, TOL_ONE, record_property)


@pytest.mark.parametrize("case", sorted(OC.NMTF_SHAPES))
def test_nmtf_iteration_at_every_case(case, capsys, record_property):
    M, K, L = OC.NMTF_SHAPES[case]()
    R, F0, S0, G0 = OC.nmtf_problem(M, K, L)
    t = OC.nmtf_model(R, M, K, L, F0, S0, G0, layout='observed')
    idiv = run_capturing_idiv(t, 1, capsys)
    F, S, G = NR.ref_nmtf_iteration(R, M, F0, S0, G0)
    errs = {"F": NR.rel_err(t.F, F), "S": NR.rel_err(t.S, S), "G": NR.rel_err(t.G, G)}
    errs.update(metric_errors(t, idiv, NR.metrics(R, M, F @ S @ G.T)))
    t.close()
    check(errs, TOL_ONE, record_property)


# ---------------------------------------------------------------- single updates at the first and the last column
@pytest.mark.parametrize("shape", sorted(OC.NMF_SHAPES))
def test_nmf_single_updates(shape, record_property):
    """update_U / update_V at columns 0 and K - 1, each from the same start: only its own column moves, to the restatement's value."""
    M, K = OC.NMF_SHAPES[shape]()
    R, U0, V0 = OC.nmf_problem(M, K)
    n = OC.nmf_model(R, M, K, U0, V0, layout='observed')
    errs = {}
    for k in sorted({0, K - 1}):
        for name, call, ref in (("U", n.update_U, NR.update_U), ("V", n.update_V, NR.update_V)):
            n.U, n.V = U0.copy(), V0.copy()
            call(k)
            got = getattr(n, name)
            errs["%s%d" % (name, k)] = NR.rel_err(got[:, k], ref(R, M, U0, V0, k)[:, k])
            rest = np.arange(K) != k
            assert np.array_equal(got[:, rest], f32(U0 if name == "U" else V0)[:, rest])
            assert np.array_equal(n.V if name == "U" else n.U, f32(V0 if name == "U" else U0))
    n.close()
    check(errs, TOL_ONE, record_property)


@pytest.mark.parametrize("case", sorted(OC.NMTF_SHAPES))
def test_nmtf_single_updates(case, record_property):
    M, K, L = OC.NMTF_SHAPES[case]()
    R, F0, S0, G0 = OC.nmtf_problem(M, K, L)
    t = OC.nmtf_model(R, M, K, L, F0, S0, G0, layout='observed')
    errs = {}
    calls = [("F", (k,), lambda k=k: NR.update_F(R, M, F0, S0, G0, k), (slice(None), k)) for k in sorted({0, K - 1})]
    calls += [("G", (l,), lambda l=l: NR.update_G(R, M, F0, S0, G0, l), (slice(None), l)) for l in sorted({0, L - 1})]
    calls += [("S", (k, l), lambda k=k, l=l: NR.update_S(R, M, F0, S0, G0, k, l), (k, l)) for k, l in sorted({(0, 0), (0, L - 1), (K - 1, 0), (K - 1, L - 1)})]
    for which, args, ref, idx in calls:
        t.F, t.S, t.G = F0.copy(), S0.copy(), G0.copy()
        getattr(t, "update_" + which)(*args)
        errs["%s%s" % (which, list(args))] = NR.rel_err(np.atleast_1d(getattr(t, which)[idx]), np.atleast_1d(ref()[idx]))
        for other, X0 in (("F", F0), ("S", S0), ("G", G0)):
            keep = np.ones(X0.shape, dtype=bool)
            if other == which:
                keep[idx] = False
            assert np.array_equal(getattr(t, other)[keep], f32(X0)[keep]), (which, args, other)
    t.close()
    check(errs, TOL_ONE, record_property)


# ---------------------------------------------------------------- five iterations, and the metrics of the end point
def _pred_masks(M, seed):
    rs = np.random.RandomState(seed)
    overlap = ((rs.rand(*M.shape) < 0.3) | ((M != 0) & (rs.rand(*M.shape) < 0.3))).astype(float)
    disjoint = ((M == 0) & (rs.rand(*M.shape) < 0.5)).astype(float)
    assert (overlap * M).sum() > 0 and (overlap * (1 - M)).sum() > 0 and disjoint.sum() > 0 and (disjoint * M).sum() == 0
    return overlap, disjoint


def _endpoint_errors(model, R, M, P):
    errs = {}
    overlap, disjoint = _pred_masks(M, 3)
    for name, Mp in (("train", M), ("overlap", overlap), ("disjoint", disjoint)):
        got, ref = model.predict(Mp), NR.metrics(R32(R), Mp, P)
        for m in ("MSE", "R^2", "Rp"):
            errs["%s_%s" % (name, m)] = abs(got[m] - ref[m]) / abs(ref[m])
    ref = NR.metrics(R32(R), M, P)["I_div"]
    errs["I_div"] = abs(model.compute_I_div() - ref) / abs(ref)
    return errs


def R32(R):
    return f32(R)              # (the device holds R in fp32)


def test_five_iterations_of_nmf_and_the_end_points_metrics(capsys, record_property):
    M, K = OC.NMF_SHAPES["row_counts"]()
    R, U0, V0 = OC.nmf_problem(M, K)
    n = OC.nmf_model(R, M, K, U0, V0, layout='observed')
    idiv = run_capturing_idiv(n, 5, capsys)
    U, V = U0, V0
    for _ in range(5):
        U, V = NR.ref_nmf_iteration(R, M, U, V)
    errs = {"U": NR.rel_err(n.U, U), "V": NR.rel_err(n.V, V)}
    errs.update(metric_errors(n, idiv, NR.metrics(R, M, U @ V.T), it=4))
    assert [len(n.all_performances[m]) for m in ("MSE", "R^2", "Rp")] == [5, 5, 5] and len(n.all_times) == 5
    check(errs, TOL_DRIFT, record_property)
    check(_endpoint_errors(n, R, M, n.U @ n.V.T), TOL_F64, record_property, "end_")
    n.close()


def test_five_iterations_of_nmtf_and_the_end_points_metrics(capsys, record_property):
    M, K, L = OC.NMTF_SHAPES["row_counts_K7_L3"]()
    R, F0, S0, G0 = OC.nmtf_problem(M, K, L)
    t = OC.nmtf_model(R, M, K, L, F0, S0, G0, layout='observed')
    idiv = run_capturing_idiv(t, 5, capsys)
    F, S, G = F0, S0, G0
    for _ in range(5):
        F, S, G = NR.ref_nmtf_iteration(R, M, F, S, G)
    errs = {"F": NR.rel_err(t.F, F), "S": NR.rel_err(t.S, S), "G": NR.rel_err(t.G, G)}
    errs.update(metric_errors(t, idiv, NR.metrics(R, M, F @ S @ G.T), it=4))
    check(errs, TOL_DRIFT, record_property)
    check(_endpoint_errors(t, R, M, t.F @ t.S @ t.G.T), TOL_F64, record_property, "end_")
    t.close()


# ---------------------------------------------------------------- against the dense layout on the device
def test_nmf_agrees_with_the_dense_layout(record_property):
    M, K = OC.NMF_SHAPES["K31"]()
    R, U0, V0 = OC.nmf_problem(M, K)
    res = []
    for layout in ("dense", "observed"):
        n = OC.nmf_model(R, M, K, U0, V0, layout=layout)
        n.run(1)
        res.append((n.U, n.V, n.all_performances))
        n.close()
    (Ud, Vd, pd), (Uo, Vo, po) = res
    assert sorted(pd) == sorted(po) and all(len(pd[m]) == len(po[m]) == 1 for m in pd)
    check({"U": NR.rel_err(Uo, Ud), "V": NR.rel_err(Vo, Vd)}, 2 * TOL_ONE, record_property)


def test_nmtf_agrees_with_the_dense_layout(record_property):
    M, K, L = OC.NMTF_SHAPES["col_counts_K7_L3"]()
    R, F0, S0, G0 = OC.nmtf_problem(M, K, L)
    res = []
    for layout in ("dense", "observed"):
        t = OC.nmtf_model(R, M, K, L, F0, S0, G0, layout=layout)
        t.run(1)
        res.append((t.F, t.S, t.G, t.all_performances))
        t.close()
    (Fd, Sd, Gd, pd), (Fo, So, Go, po) = res
    assert sorted(pd) == sorted(po) and all(len(pd[m]) == len(po[m]) == 1 for m in pd)
    check({"F": NR.rel_err(Fo, Fd), "S": NR.rel_err(So, Sd), "G": NR.rel_err(Go, Gd)}, 2 * TOL_ONE, record_property)


# ---------------------------------------------------------------- bit for bit
_CHILD = """
import sys, numpy as np
sys.path[:0] = [%r, %r]
import _obs_np_cases as OC
out = OC.bits_runs()
from bnmtf_amd import NMF
M, K = OC.NMF_SHAPES["row_counts"]()
R, U0, V0 = OC.nmf_problem(M, K)
n = OC.nmf_model(R, M, K, U0, V0, layout='observed')
n._push()
import ctypes as C
buf = C.create_string_buffer(2048)
from bnmtf_amd import _lib
_lib.check(_lib.lib().bnmtf_describe(n._handle(), buf, 2048))
assert ("force_long=%s" in buf.value.decode()), buf.value
np.savez(sys.argv[1], **out)
"""


def _child_run(tmp_path, force_long, tag):
    env = dict(os.environ)
    env.pop("BNMTF_OBS_LONG", None)
    if force_long:
        env["BNMTF_OBS_LONG"] = "1"
    out = str(tmp_path / ("run_%s.npz" % tag))
    subprocess.run([sys.executable, "-c", _CHILD % (ROOT, os.path.join(ROOT, "tests"), "1" if force_long else "0"), out], check=True, env=env, cwd=ROOT, timeout=300)
    return np.load(out)


def test_long_form_and_register_form_give_the_same_bits(tmp_path):
    """BNMTF_OBS_LONG=1 (every unit down the long form) in a fresh child process against the default, two iterations on the
    row-count and column-count masks and one NMTF case: factors, per-iteration metrics and the I-divergence."""
    a = _child_run(tmp_path, False, "a")
    b = _child_run(tmp_path, True, "long")
    assert sorted(a.files) == sorted(b.files) and len(a.files) == 4 * len(OC.BITS_NMF) + 5 * len(OC.BITS_NMTF)
    for k in a.files:
        assert a[k].tobytes() == b[k].tobytes(), k


def _nmf(name="col_counts"):
    M, K = OC.NMF_SHAPES[name]()
    R, U0, V0 = OC.nmf_problem(M, K)
    return K, lambda: OC.nmf_model(R, M, K, U0, V0, layout='observed')


def _nmtf(name="row_counts_K3_L11"):
    M, K, L = OC.NMTF_SHAPES[name]()
    R, F0, S0, G0 = OC.nmtf_problem(M, K, L)
    return K, L, lambda: OC.nmtf_model(R, M, K, L, F0, S0, G0, layout='observed')


def _state(m):
    return [np.array(f) for f in m._factors()]


def _same(a, b):
    return all(x.tobytes() == y.tobytes() for x, y in zip(a, b))


@pytest.mark.parametrize("kind", ["nmf", "nmtf"])
def test_two_runs_and_split_runs_give_the_same_bits(kind):
    make = _nmf()[-1] if kind == "nmf" else _nmtf()[-1]
    ends, perfs = [], []
    for parts in ((5,), (5,), (2, 3)):
        m = make()
        perf = []
        for p in parts:
            m.run(p)
            perf += list(m.all_performances["MSE"])
        ends.append(_state(m)); perfs.append(perf)
        m.close()
    assert _same(ends[0], ends[1]) and _same(ends[0], ends[2])
    assert perfs[0] == perfs[1] == perfs[2]


def test_the_columns_one_by_one_are_the_iteration_nmf():
    K, make = _nmf()
    a = make(); a.run(1)
    b = make()
    for k in range(K):
        b.update_U(k)
    for k in range(K):
        b.update_V(k)
    assert _same(_state(a), _state(b))
    a.close(); b.close()


def test_the_entries_and_columns_one_by_one_are_the_iteration_nmtf():
    K, L, make = _nmtf()
    a = make(); a.run(1)
    b = make()
    for k in range(K):
        for l in range(L):
            b.update_S(k, l)
    for k in range(K):
        b.update_F(k)
    for l in range(L):
        b.update_G(l)
    assert _same(_state(a), _state(b))
    a.close(); b.close()


def test_get_state_after_set_state_returns_the_fp32_rounded_input():
    rs = np.random.RandomState(4)
    for make, shapes in ((_nmf("K33")[-1], None), (_nmtf("row_counts_K33_L5")[-1], None)):
        m = make()
        start = [rs.rand(*f.shape) + 0.1 for f in m._factors()]
        names = ("U", "V") if len(start) == 2 else ("F", "S", "G")
        for nme, x in zip(names, start):
            setattr(m, nme, x.copy())
        m._push(); m._pull()
        for got, x in zip(m._factors(), start):
            assert np.array_equal(got, f32(x)) and not np.array_equal(got, x)
        m.close()


# ---------------------------------------------------------------- the shapes can tell a misplaced edge entry from rounding
def test_a_dropped_entry_shows():
    """On the restatement alone: without the last entry of the longest unit that unit's row moves by far more than TOL_ONE."""
    for name in ("row_counts", "K31"):
        M, K = OC.NMF_SHAPES[name]()
        R, U0, V0 = OC.nmf_problem(M, K)
        i = int(np.argmax(M.sum(axis=1)))
        j = int(np.flatnonzero(M[i])[-1])
        M2 = M.copy(); M2[i, j] = 0
        assert M2.sum(axis=0).min() > 0 and M2.sum(axis=1).min() > 0
        full, dropped = NR.ref_half(R, M, U0, V0), NR.ref_half(R, M2, U0, V0)
        assert NR.rel_err(dropped[i], full[i]) > 10 * TOL_ONE, (name, NR.rel_err(dropped[i], full[i]))
        assert np.array_equal(np.delete(dropped, i, axis=0), np.delete(full, i, axis=0))


# ---------------------------------------------------------------- handle kinds
def test_the_handle_kinds_refuse_each_other_and_the_model_still_runs():
    lib = bnmtf_amd.lib()
    K, make = _nmf("K2")
    n = make(); n._push()
    h = n._handle()
    A = np.ones((n.I, K)); B = np.ones((n.J, K))
    assert lib.bnmf_obs_run(h, 1, _lib.UPDATE_MODE, None, None, None, None, None) == -1
    assert b"not a handle of bnmtf_obs_create" in lib.bnmtf_last_error()
    assert lib.bnmtf_otri_run(h, 1, _lib.UPDATE_MODE, None, None, None, None, None, None) == -1
    assert b"not a handle of bnmtf_otri_create" in lib.bnmtf_last_error()
    assert lib.bnmf_vbo_set_state(h, *[_lib.ptr(A)] * 4, *[_lib.ptr(B)] * 4, 1.0) == -1
    assert b"not a handle of bnmtf_obs_create" in lib.bnmtf_last_error()
    pri2 = dict(alpha=1., beta=1., lambdaU=0.5, lambdaV=0.5); pri3 = dict(alpha=1., beta=1., lambdaF=0.5, lambdaS=0.5, lambdaG=0.5)
    g = bnmf_gibbs_optimised(n.R, n.M, K, pri2, verbose=False, layout='observed')
    t = bnmtf_gibbs_optimised(n.R, n.M, K, 3, pri3, verbose=False, layout='observed')
    for other in (g, t):
        assert lib.bnmtf_onp_run(other._handle(), 1, None, None, None) == -1
        assert b"not a handle of bnmtf_onp_create" in lib.bnmtf_last_error()
        other.close()
    ref = make(); ref.run(2)
    n.run(2)
    assert _same(_state(n), _state(ref))
    n.close(); ref.close()
