"""Pins of the exact contraction cases (tests/_contraction_cases.py; the GPU side: test_contraction_exact_gpu.py), on the CPU:
  (a) every case is exact: its launch is the one it targets, every output's sum of |split terms| is below 2^24, and the three
      products the kernel drops are zero on it;
  (b) the cases would see a wrong kernel: dropping any one of the six retained products, reading one inner step twice at
      every wave's slice end, or dropping any one inner slice changes a checked output;
  (c) the cases cover every instantiation x (nsteps mod 3), split = 1, a clamped split, zero pads and whole pad slices.
The emulation rounds to nearest even at each level of the split, as the kernel's v_cvt_pk_bf16_f32 does; products and sums are
fp64 (exact on these grids)."""
import numpy as np
import pytest

from _contraction_cases import (CASES, DROPPED, HEAVY, LAM, PRODUCTS, TWO24, exact, instantiation, launch, operands,
                                problems, split3)


def _walk(case):
    """(direction, family, the direction's View, X, exact numer, num, budget) of every checked state of the case"""
    for p in problems(case):
        for st in p.states:
            v, X, Y = operands(p, st)
            numer, num, _, budget, _ = exact(v, X, Y)
            yield st[0], p.fam, v, X, numer, num, budget


def _moves(numer, num, delta):
    """does changing the exact num by delta change a checked fp32 output?"""
    return bool(np.any((num + delta - LAM).astype(np.float32) != numer))


def _product(sb, sx, a, b):
    if not sx[a].any() or not sb[b].any():
        return None
    return sb[b].astype(np.float64) @ sx[a].astype(np.float64)


@pytest.mark.parametrize("case", CASES, ids=[c.id for c in CASES])
def test_case_sits_on_its_launch_and_is_exact(case):
    for d in case.dirs():
        assert case.launch(d) == case.expect[d], (d, case.launch(d))
    for d, fam, v, X, numer, num, budget in _walk(case):
        assert budget.max() < TWO24, (d, fam, budget.max())
        assert np.all(num == np.rint(num)) and np.abs(num).max() < TWO24, (d, fam)
        sb, sx = v.split, split3(X)
        for a, b in DROPPED:
            c = _product(sb, sx, a, b)
            assert c is None or not c.any(), (d, fam, "dropped a%s.b%s is not zero" % (a, b))


def test_every_retained_product_moves_a_checked_output_at_every_instantiation():
    seen = {}
    for case in CASES:
        if case.I * case.J > HEAVY:
            continue
        for d, fam, v, X, numer, num, _ in _walk(case):
            inst = instantiation(case.launch(d))
            sb, sx = v.split, split3(X)
            for a, b in PRODUCTS:
                c = _product(sb, sx, a, b)
                if c is not None and _moves(numer, num, -c):
                    seen.setdefault(inst, set()).add((a, b))
    assert set(seen) == {(1, 4), (2, 2), (2, 4)}
    for inst, got in seen.items():
        assert got == set(PRODUCTS), (inst, set(PRODUCTS) - got)


@pytest.mark.parametrize("case", CASES, ids=[c.id for c in CASES])
def test_a_step_read_twice_or_a_dropped_slice_moves_a_checked_output(case):
    want, seen = set(), set()
    for d in case.dirs():
        p = case.launch(d)
        m = case.J if d == "rows" else case.I
        if p["ipw"] - 16 < m:
            want.add((d, "tail"))                       # (a wave's last step holds real rows)
        want |= {(d, s) for s in range(p["split"]) if s * 4 * p["ipw"] < m}      # every inner slice that holds real rows
    for d, _, v, X, numer, num, _ in _walk(case):
        p = case.launch(d)
        ipw, m = p["ipw"], v.Rt.shape[1]

        def part(rows):
            rows = rows[rows < m]
            return v.Rt[:, rows] @ X[rows].astype(np.float64)

        # the ring's tail re-reading the last step of every wave's slice
        if (d, "tail") not in seen and _moves(numer, num, part(np.concatenate(
                [np.arange((w + 1) * ipw - 16, (w + 1) * ipw) for w in range(p["split"] * 4)]))):
            seen.add((d, "tail"))
        # one inner slice (four waves' rows) lost
        for s in range(p["split"]):
            if (d, s) in want and (d, s) not in seen and _moves(numer, num, -part(np.arange(s * 4 * ipw, (s + 1) * 4 * ipw))):
                seen.add((d, s))
    assert want == seen, sorted(want - seen, key=str)


def test_cases_cover_the_launch_matrix():
    cells, flags = set(), set()
    for case in CASES:
        for d in case.dirs():
            p = case.launch(d)
            n, m = (case.I, case.J) if d == "rows" else (case.J, case.I)
            cells.add((instantiation(p), p["nsteps"] % 3))
            unclamped = max(1, 256 // (p["n_pad"] // (32 * p["tw"])))
            flags.add("split=1" if p["split"] == 1 else "split>1")
            if p["split"] < unclamped:
                flags.add("clamped split")
            if p["n_pad"] > n:
                flags.add("pad units")
            if p["split"] * 4 * p["ipw"] > m:
                flags.add("pad rows")
            if p["split"] * 4 * p["ipw"] - m >= 4 * p["ipw"]:
                flags.add("whole pad slices")
            if p["KP"] == 64 and p["n_pad"] in (2048, 2176):
                flags.add("tw switch %d" % p["n_pad"])
            if "C" in case.fams and p["KP"] == 64 and case.K > 32:
                flags.add("both factor tiles")
    assert cells == {(i, r) for i in ((1, 4), (2, 2), (2, 4)) for r in (0, 1, 2)}, cells
    assert flags >= {"split=1", "split>1", "clamped split", "pad units", "pad rows", "whole pad slices", "tw switch 2048",
                     "tw switch 2176", "both factor tiles"}, flags


def test_split3_emulation():
    x = np.float32(1 + 2 ** -8 + 2 ** -9 + 2 ** -17 + 2 ** -23)
    s = split3(np.array([x]))
    assert s["h"][0] + s["m"][0] + s["l"][0] == x
    t = split3(np.array([1 + 2 ** -8, 1 + 3 * 2 ** -8], np.float32))   # ties round to even (truncation would keep 1 + 2^-7)
    assert list(t["h"]) == [1.0, 1 + 2 ** -6] and list(t["m"]) == [2 ** -8, -2 ** -8]
    rs = np.random.RandomState(0)
    v = rs.uniform(-4, 4, 10000).astype(np.float32)
    s = split3(v)
    for t in "hml":                                        # every term is a bf16
        assert not np.any(s[t].view(np.uint32) & 0xFFFF)
    assert np.array_equal((s["h"].astype(np.float64) + s["m"] + s["l"]).astype(np.float32), v)
    assert launch(8192, 8192, 64) == dict(KP=64, tw=4, n_pad=8192, split=4, ipw=512, nsteps=32)
