"""bnmf_gibbs_run on one GPU with its relayout / Gram / end-of-iteration kernels on a second stream beside the contractions
(api.hip: TailOverlap) against the same loop with every kernel on the compute stream in program order (BNMTF_TAIL=serial, read
when the handle is created).  Left to itself the library takes the second stream where the contraction is long enough to pay
for it (8192 x 8192), so at this file's sizes the default is the serial order: every case therefore runs three times -- the
second stream forced (BNMTF_TAIL=overlap), the default, and BNMTF_TAIL=serial.

The orderings run the same kernels on the same operands: nothing that is added is reordered, so every output is compared
with np.array_equal -- the tolerance is zero.  What could differ is a reader that got ahead of its join (a sweep reading a
layout, a Gram or tau that the tail stream has not written yet; a sample slot copied or overwritten too early; the posterior
sums reading a factor the next sweep is already overwriting), which shows as different bits in the samples, the tau / metric
series, the posterior means or the state the call leaves behind.  (At the headline size, where the default IS the second stream,
the outputs of bench.py --dump-outputs were compared with the previous build's: profiles/README.md, tail_overlap_*.)"""
import numpy as np
import pytest

from bnmtf_amd import bnmf_gibbs_optimised
from bnmtf_amd.nmf_icm import nmf_icm

pytestmark = pytest.mark.gpu

PRI = dict(alpha=1., beta=1., lambdaU=1., lambdaV=1.)       # (the start, Exp(lambda), on the data's scale: a mode update is then not max(0, mu) = 0 everywhere)

# name -> (I, J, K, missing fraction per row from .. to, switches read at bnmtf_create)
SHAPES = {
    # 16-wave sweeps on both directions, q handed over between them, the rows sweep's pre-pass every fourth iteration
    "k64_wide_handover": (640, 800, 64, 0.0, 0.9, {"BNMTF_WIDE": "1", "BNMTF_HANDOVER": "1", "BNMTF_HANDOVER_REFRESH": "4"}),
    "k32": (512, 384, 32, 0.05, 0.3, {}),
    "ragged": (517, 391, 20, 0.05, 0.5, {}),               # I, J not multiples of 32 or 128
}
N_ITERS = (1, 2, 19)        # 19: sample groups of eight close inside the run, and the slots of the first group are re-used (16 deep)


def _data(name):
    I, J, K, lo, hi, _ = SHAPES[name]
    rs = np.random.RandomState(I + J + K)
    R = rs.exponential(1.0, (I, K)) @ rs.exponential(1.0, (J, K)).T + rs.randn(I, J)
    M = np.ones((I, J))
    for i in range(I):
        M[i, rs.choice(J, int((lo + (hi - lo) * rs.rand()) * J), replace=False)] = 0
    M[rs.randint(I, size=J), np.arange(J)] = 1          # no empty column
    return R, M, K


def _chain(monkeypatch, tail, name, update, store, expectation, calls):
    """the seeded model in a fresh handle, run() once per entry of `calls`; everything a caller can see afterwards"""
    if tail == "default":
        monkeypatch.delenv("BNMTF_TAIL", raising=False)
    else:
        monkeypatch.setenv("BNMTF_TAIL", tail)
    env = SHAPES[name][5]
    for k in ("BNMTF_WIDE", "BNMTF_HANDOVER", "BNMTF_HANDOVER_REFRESH"):
        if k in env:
            monkeypatch.setenv(k, env[k])
        else:
            monkeypatch.delenv(k, raising=False)
    R, M, K = _data(name)
    cls = nmf_icm if update == "icm" else bnmf_gibbs_optimised
    b = cls(R, M, K, PRI, verbose=False, seed=11)
    try:
        d = b.describe()                                 # (creates the handle: the switch is read here)
        assert {"overlap": "tail=overlap", "serial": "tail=serial", "default": "tail=serial(auto)"}[tail] in d.split() , d
        if env.get("BNMTF_HANDOVER") == "1":
            assert "sweep_nw=16" in d and "handover=1" in d, d
        b.set_small_path(False)
        assert not b.is_small()
        np.random.seed(3); b.initialise("random")
        out = []
        for n in calls:
            if update == "icm":
                b.run(n, minimum_TN=0.1)
                res = {}
            else:
                exp = expectation if (expectation is not None and expectation[0] < n) else None
                b.run(n, update=update, store_samples=store, expectation=exp)
                res = {"all_U": np.array(b.all_U), "all_V": np.array(b.all_V)}
                if exp is not None:
                    A, _, B, tau = b._device_expectation(*exp)
                    res.update(exp_U=A, exp_V=B, exp_tau=np.array(tau))
                if store:
                    assert res["all_U"].shape == (n, b.I, K) and np.isfinite(res["all_U"]).all() and np.isfinite(res["all_V"]).all()
                    if update == "draw":        # (a draw is positive; a mode update can be max(0, mu) = 0)
                        assert np.abs(res["all_U"][-1]).max() > 0 and np.abs(res["all_V"][-1]).max() > 0
            res.update(all_tau=np.array(b.all_tau), MSE=np.array(b.all_performances["MSE"]), R2=np.array(b.all_performances["R^2"]),
                       Rp=np.array(b.all_performances["Rp"]), U=np.array(b.U), V=np.array(b.V), tau=np.array(b.tau))
            times = np.array(b.all_times)
            assert times.shape == (n,) and (np.diff(times) >= 0).all() and times[0] >= 0 and times[-1] > 0, (tail, times)
            assert np.isfinite(res["all_tau"]).all() and np.isfinite(res["MSE"]).all()
            out.append(res)
        return out
    finally:
        b.close()


def _same(monkeypatch, name, update, store, expectation, calls):
    se = _chain(monkeypatch, "serial", name, update, store, expectation, calls)
    for other in ("overlap", "default"):
        ov = _chain(monkeypatch, other, name, update, store, expectation, calls)
        for k, (a, b) in enumerate(zip(ov, se)):
            assert sorted(a) == sorted(b)
            for key in a:
                # (equal_nan: a metric that is 0 / 0 in both runs -- Rp of a constant prediction -- is the same result)
                assert np.array_equal(a[key], b[key], equal_nan=True), (other, name, update, store, expectation, calls, "call %d" % k, key)


@pytest.mark.parametrize("n_iter", N_ITERS)
@pytest.mark.parametrize("expectation", [None, (1, 2)])
@pytest.mark.parametrize("store", [True, False])
@pytest.mark.parametrize("update", ["draw", "mode"])
@pytest.mark.parametrize("name", sorted(SHAPES))
def test_overlapped_tail_equals_the_serial_order(monkeypatch, name, update, store, expectation, n_iter):
    _same(monkeypatch, name, update, store, expectation, [n_iter])


@pytest.mark.parametrize("n_iter", N_ITERS)
@pytest.mark.parametrize("name", sorted(SHAPES))
def test_overlapped_tail_equals_the_serial_order_icm(monkeypatch, name, n_iter):
    _same(monkeypatch, name, "icm", False, None, [n_iter])


@pytest.mark.parametrize("store", [True, False])
@pytest.mark.parametrize("name", sorted(SHAPES))
def test_two_calls_in_a_row_on_one_handle(monkeypatch, name, store):
    """the second call starts from what the first one left on the device: the q hand-over regions, tau, both streams drained"""
    _same(monkeypatch, name, "draw", store, (2, 3), [5, 11])


def test_describe_names_the_mode(monkeypatch):
    R, M, K = _data("k32")
    for env, want in ((None, "tail=serial(auto)"), ("serial", "tail=serial"), ("overlap", "tail=overlap")):
        if env is None:
            monkeypatch.delenv("BNMTF_TAIL", raising=False)
        else:
            monkeypatch.setenv("BNMTF_TAIL", env)
        b = bnmf_gibbs_optimised(R, M, K, PRI, verbose=False, seed=1)
        try:
            assert want in b.describe().split(), b.describe()
        finally:
            b.close()
