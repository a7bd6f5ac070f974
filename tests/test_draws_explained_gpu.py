"""Every truncated-normal draw of every Gibbs kernel form, explained by the oracle's candidate sequence (tests/_draw_explainer.py).

A run of three iterations from a fixed state returns its samples; conditioned on them, (mu, tau_p) of each single draw is an fp64
function of numbers the run returned, so each draw is checked on its own -- nothing cascades, every iteration counts, and the
paths a kernel takes once in forty or once in 250 draws (candidates past its first batch) are held like the first candidate.
Per case: (1) no unexplained draw, (2) the draws with a one-element admissible set are the oracle's accepted candidate (counted
separately), (3) at most 1 % ambiguous draws, (5) tau of every iteration = gamma_unit / beta_s(the device's own sample) to 2e-5;
per kernel form (4) the coverage counts of _draw_cases.coverage_failures.  The inputs (tests/_draw_cases.py) are steered so that
the long candidate walks, both regimes and the regime switch occur; tests/test_draw_explainer_cpu.py holds them to the same
counts on the oracle's own chain, and the explainer to its mutations, without a GPU.

Recorded numbers of an MI355X run: profiles/draws_explained.json (summaries() below makes them) -- 1.32 M draws over the 31
cases of the default build, none unexplained, at most 0.34 % ambiguous in a case, value errors at most 0.12 of the derived
tolerance (0.05 outside the K = 130 column blocks), tau within 1e-7."""
import contextlib
import os

import numpy as np
import pytest

from bnmtf_amd import _lib, bnmf_gibbs_optimised, bnmtf_gibbs_optimised
from bnmtf_amd._blocked import block_ranges

import _draw_cases as C
import _draw_explainer as X

pytestmark = pytest.mark.gpu

SWITCHES = ("BNMTF_UNIT", "BNMTF_FAST_NW", "BNMTF_WIDE", "BNMTF_HANDOVER", "BNMTF_TWIN", "BNMTF_TURNS", "BNMTF_OBS_LONG", "BNMTF_SSYS")


@contextlib.contextmanager
def _switches(env):
    """the case's kernel-form switches (read when the model is built), every other one of them unset; restored afterwards"""
    saved = {k: os.environ.get(k) for k in SWITCHES}
    try:
        for k in SWITCHES:
            os.environ.pop(k, None)
        os.environ.update(env)
        yield
    finally:
        for k, v in saved.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


def _check_form(case, b):
    """the intended kernel form runs, as the existing tests of each form assert it"""
    d = b.describe()
    form, path, env = case["form"], case["path"], case["env"]
    if path == "small":
        assert b.is_small() and "small[" in d, d
        return
    if path == "blocks":
        assert ("blocks of F" in d) if form == "wide_tri" else ("column blocks %s" % (block_ranges(case["shape"][2]),) in d), d
        return
    if path == "obs":
        assert "layout=observed" in d and ("force_long=1" in d) == ("BNMTF_OBS_LONG" in env), d
        if form == "obs_long":
            assert "long_form_units=0/0" not in d or "force_long=1" in d, d
        else:
            assert "long_form_units=0/0" in d, d
        return
    assert not b.is_small(), d
    if form == "unit":
        assert "unit_sweep[rows=1" in d, d
    elif form == "pairs":
        assert "unit_sweep[rows=0" in d and ("sweep_nw=%s" % env["BNMTF_FAST_NW"] in d if "BNMTF_FAST_NW" in env else "sweep_nw=16" not in d), d
    elif form == "wide":
        assert "sweep_nw=16" in d and "twin=0" in d and "turns=0" in d and ("handover=1" in d) == (env["BNMTF_HANDOVER"] == "1"), d
    elif form == "twin":
        assert "twin=1" in d and "sweep_nw=8" in d, d
    elif form == "turns":
        assert "turns=1" in d and "sweep_nw=16" in d, d
    elif form == "ssys":
        assert "ssys[on=1" in d, d
    elif form == "rowwise":
        assert "ssys[on=0]" in d, d


_RUNS = {}


def explained(case):
    """the case's run on the device and its explanation (once per session; the coverage tests sum over a form's cases)"""
    if case["id"] in _RUNS:
        return _RUNS[case["id"]]
    R, M, init, lams = C.case_inputs(case)
    tri = len(init) == 4
    with _switches(case["env"]):
        if tri:
            K, L = init[1].shape
            b = bnmtf_gibbs_optimised(R, M, K, L, dict(alpha=1.0, beta=1.0, lambdaF=lams[0].copy(), lambdaS=lams[1].copy(), lambdaG=lams[2].copy()),
                                      verbose=False, seed=C.SEED)
            b.F, b.S, b.G, b.tau = init[0].copy(), init[1].copy(), init[2].copy(), init[3]
        else:
            kw = dict(layout="observed") if case["path"] == "obs" else {}
            b = bnmf_gibbs_optimised(R, M, init[0].shape[1], dict(alpha=1.0, beta=1.0, lambdaU=lams[0].copy(), lambdaV=lams[1].copy()),
                                     verbose=False, seed=C.SEED, **kw)
            b.U, b.V, b.tau = init[0].copy(), init[1].copy(), init[2]
        if case["path"] in ("small", "multi", "generic"):
            b.set_small_path("always" if case["path"] == "small" else False)
        if case["path"] == "generic":
            b.set_sweep_path(False)
        b.run(C.ITERATIONS, store_samples=True)
        _check_form(case, b)
        if tri:
            e = X.explain_bnmtf_run(R, M, lams[0], lams[1], lams[2], 1.0, 1.0, C.SEED, init, np.asarray(b.all_F), np.asarray(b.all_S),
                                    np.asarray(b.all_G), np.asarray(b.all_tau))
        else:
            e = X.explain_bnmf_run(R, M, lams[0], lams[1], 1.0, 1.0, C.SEED, init, np.asarray(b.all_U), np.asarray(b.all_V), np.asarray(b.all_tau))
        b.close()
    _RUNS[case["id"]] = e
    return e


def _skip_experiment(case):
    if case["experiment"] and not _lib.lib().bnmtf_has_experiments():
        pytest.skip("the %s kernel is an experiment: make EXPERIMENTS=1" % case["form"])


@pytest.mark.parametrize("case", C.BNMF_CASES + C.BNMTF_CASES, ids=lambda c: c["id"])
def test_every_draw_is_a_candidate_the_oracle_admits(case):
    _skip_experiment(case)
    e = explained(case)
    s = e.summary()
    print("%s: draws %d, unexplained %d, unique %d, ambiguous %.3f %%, err max normal %s tail %s, tau rel %.2e, accepted index %s"
          % (case["id"], s["draws"], s["unexplained"], s["unique"], 100 * s["ambiguous_share"], s["err_max_normal"], s["err_max_tail"],
             s["tau_rel_max"], s["accepted_index_histogram"]))
    if e.unexplained:
        for o in e.offenders(10):
            print("  unexplained:", o)
    assert e.unexplained == 0                                                    # 1 (and 2: the unique draws among them)
    assert s["unique"] + e.ambiguous == e.draws
    assert e.ambiguous <= C.AMBIGUITY_CAP * e.draws                              # 3
    assert max(e.tau_rel) <= X.TAU_REL, e.tau_rel                                # 5
    if case["kw"].get("zero_col", -1) >= 0:                                      # the dead column: tau_p = 0, the guarded 0
        k = case["kw"]["zero_col"]
        dead = (e["factor"] == "U") & (e["col"] == k)
        assert (e["cand"][dead] == -1).all() and (e["x"][dead] == 0.0).all()


@pytest.mark.parametrize("tri,form", [(False, f) for f in C.forms(C.BNMF_CASES)] + [(True, f) for f in C.forms(C.BNMTF_CASES)])
def test_form_coverage(tri, form):
    cases = C.forms(C.BNMTF_CASES if tri else C.BNMF_CASES)[form]
    for c in cases:
        _skip_experiment(c)
    results = [explained(c) for c in cases]
    batch = (1 if form.startswith("small") else 4) if tri else C.BATCH[form]
    blocks = [block_ranges(c["shape"][2]) for c in cases] if form == "blocks" else None
    fails = C.coverage_failures(form, batch, results, tri=tri, blocks=blocks)
    print("%s: past the first batch (%d) %d, index >= 8: %d%s" % (form, batch, sum(r.past(batch) for r in results), sum(r.past(8) for r in results),
                                                                  ", S index >= 4: %d" % sum(r.past(4, ("S",)) for r in results) if tri else ""))
    assert not fails, fails


def summaries():
    """per-case records of the cases run so far in this process, for profiles/draws_explained.json"""
    return {c["id"]: dict(form=c["form"], shape=list(c["shape"][:4 if len(c["shape"]) == 4 else 3]), **_RUNS[c["id"]].summary())
            for c in C.BNMF_CASES + C.BNMTF_CASES if c["id"] in _RUNS}
