"""Pins of the exact masked-product cases (tests/_masked_product_cases.py; the GPU side: test_masked_product_exact_gpu.py), on
the CPU:
  (a) every case sits on the launch it targets, family X is exact there (every sum an integer below 2^24 on its grid: the
      slab-aware model and the fp64 product agree to the bit) and every digit sum fits the int32 accumulators and converts to
      fp32 exactly, as the model assumes;
  (b) the cases would see a wrong kernel: each defect of DEFECTS below, applied to the model, changes an output element of
      every case that claims it -- at every place it is tried, not only somewhere;
  (c) between them the cases cover the launch classes of CLASSES, per instantiation (KP = 32: NCG = 2, KP = 64: NCG = 4), or the
      class is declared unreachable with its reason.
test_survey_lists_every_case prints, per case and direction, the classes it covers and the defects it detects (pytest -s).

Two defects are invisible by construction and the test says so instead of claiming them:
  * a reversed slab order to family X: every partial sum of X is exact, so no order of additions can change it (that is what
    makes X independent of the split); to family G below four slabs: fp32 addition commutes, a + b = b + a;
  * mask bits counted at inner indices >= m or for units >= n: the digit rows >= m are zero (vb_planes_kernel) and the hook returns
    the units below n, so either guard alone keeps the result -- the model with every pad bit set returns the same bits.
"""
import functools

import numpy as np
import pytest

import _masked_product_cases as C
from _masked_product_cases import CASES, DIRS, FAMILIES, NSET, TWO24, View

CLAIMING = [c for c in CASES if c.claims]


@functools.lru_cache(maxsize=None)
def _views(case):
    M = C.mask(case)
    return {(fam, d): View(case, fam, d, M, mom) for fam in FAMILIES for mom in [C.moments(case, fam)] for d in DIRS}


def _fold(acc, key, r):
    """r: True (seen), False (missed), None (not applicable there)"""
    if r is not None:
        acc.setdefault(key, []).append(bool(r))


@functools.lru_cache(maxsize=None)
def _survey(case):
    """{(defect, family, direction): [the outcome at every place it was tried]}"""
    acc = {}
    for (fam, d), v in _views(case).items():
        for bx, s, i, step in v.sites():
            _fold(acc, ("step skipped", fam, d), C.defect_step_skipped(v, bx, s, i, step))
            _fold(acc, ("step twice", fam, d), C.defect_step_twice(v, bx, s, i, step))
            _fold(acc, ("stale ring set", fam, d), C.defect_stale_ring_set(v, bx, s, i, step))
        for bx, s in v.blocks():
            for p in range(3):
                _fold(acc, ("plane %d dropped" % p, fam, d), C.defect_plane_dropped(v, bx, s, p))
            _fold(acc, ("next tile's mask", fam, d), C.defect_next_tiles_mask(v, bx, s))
            _fold(acc, ("wrap off by one", fam, d), C.defect_wrap_off_by_one(v, bx, s))
        _fold(acc, ("slab order reversed", fam, d), C.defect_slab_order_reversed(v))
        _fold(acc, ("exponent + 1", fam, d), C.defect_exponent_one_too_large(v))
        _fold(acc, ("pads counted", fam, d), not np.array_equal(C.defect_pads_counted(v).view(np.uint32), v.out.view(np.uint32)))
    return acc


# defect -> (the families that must see it, where: a predicate on the direction's geometry)
DEFECTS = {
    "step skipped": ("XG", lambda g: True),
    "step twice": ("XG", lambda g: True),
    "stale ring set": ("XG", lambda g: g["nsteps"] >= NSET),
    "plane 0 dropped": ("XG", lambda g: True),
    "plane 1 dropped": ("XG", lambda g: True),
    "plane 2 dropped": ("XG", lambda g: True),
    "next tile's mask": ("XG", lambda g: True),
    "wrap off by one": ("XG", lambda g: g["nx"] >= 2 and g["nsteps"] >= 2 and 11 % g["nsteps"] != 0),      # (slot 1 starts at 11 mod nsteps)
    # (four slabs or more -- fp32 addition commutes -- of three steps or more: below that a slab's sum of the general family stays
    # under 2^24 grid steps, nothing is rounded and no order can matter)
    "slab order reversed": ("G", lambda g: g["msplit"] >= 4 and g["nsteps"] >= 3),
    "exponent + 1": ("G", lambda g: True),
}


@pytest.mark.parametrize("case", CASES, ids=[c.id for c in CASES])
def test_case_sits_on_its_launch_and_is_exact(case):
    for d in DIRS:
        g = case.geometry(d)
        assert (g["msplit"], g["nsteps"]) == case.expect[d], (d, g)
        assert g["mipw"] % 32 == 0 and g["msplit"] * g["mipw"] == g["inner_pad"] >= case.shape(d)[1] and g["n_pad"] >= case.shape(d)[0]
        # every block id maps to its own (slot, slab), and the pairs fill the grid
        assert sorted(C.block_of(g, b) for b in range(g["nb"])) == [(bx, s) for bx in range(g["nx"]) for s in range(g["msplit"])]
    assert case.K < case.geometry("rows")["KP"]                                   # padding columns exist
    for (fam, d), v in _views(case).items():
        # the accumulators: int32, and exact as fp32 where combine() converts them
        assert np.abs(v.D).max(initial=0) < min(2 ** 31, TWO24), (fam, d)
        for dig, lo, hi in zip(v.digits, (0, -128, -128), (64, 127, 127)):
            assert dig.min() >= lo and dig.max() <= hi                            # int8 operands
        if fam == "X":
            assert C.sum_bound(v.miss, v.x) < TWO24, (d, C.sum_bound(v.miss, v.x))
            ref = C.exact_sums(v.miss, v.x)
            assert np.array_equal(v.out.astype(np.float64), ref), d               # the model IS the exact product, whatever the split
            for k in range(1, v.g["msplit"] + 1):                                 # ... and so is every partial sum over the slabs
                part = C.add_slabs(v.slabs[:k])
                a = min(k * v.g["mipw"], v.m)
                assert np.array_equal(part.astype(np.float64), C.exact_sums(v.miss[:, :a], v.x[:a])), (d, k)
        else:
            tiny = np.finfo(np.float32).tiny
            assert np.all((v.x == 0) | (v.x >= tiny))                             # normal fp32 (subnormals: out of scope)
            assert np.all((v.out == 0) | (v.out >= tiny))
    if not case.claims:
        for v in _views(case).values():
            assert not v.miss.any() and not v.out.any()


def test_the_masks_hold_the_edge_units():
    for case in CLAIMING:
        M = C.mask(case)
        assert M[0].sum() == 1 and M[:, 0].sum() == 1                             # every entry missing but one (the constructor refuses none)
        assert M[1].all() and M[:, 1].all()                                       # none missing
        assert M[-1, -1] == 0                                                     # the last unit's last inner index, in both directions
        frac = 1 - M[2:, 2:].mean()
        assert 0.29 < frac < 0.51, frac
    assert sum(1 for c in CLAIMING for d in DIRS if c.shape(d)[1] % 32) >= len(CLAIMING)      # inner extents off the 32-row step
    assert any(c.shape(d)[1] % 32 == 0 for c in CLAIMING for d in DIRS)


def test_the_family_values_are_what_the_docstring_says():
    case = next(c for c in CASES if c.id == "513x1792x7")
    eU, vU, eV, vV = C.moments(case, "G")
    x = C.operand(eV, vV)
    K = case.K
    assert not x[:, 1].any() and not x[:, K + 1].any()                            # an all-zero column
    assert x[:, 2].max() == 8.0 and x[:, K + 2].max() == 4.0                      # maxima that are exact powers of two
    assert 2.0 ** 50 < x[:, 3].max() < 2.0 ** 70 and 2.0 ** -70 < x[:, 4].max() < 2.0 ** -50
    assert (x == 0).mean() > 0.03
    e = C.column_exponents(x)
    assert e[1] == 0 and e[2] == 4 and e[K + 2] == 3
    eU, vU, eV, vV = C.moments(case, "X")
    x = C.operand(eV, vV).astype(np.float64)
    assert np.array_equal(x[:, :K], vV + eV * eV)                                 # S2 = var + exp^2 without a rounding
    e, d0, d1, d2, n = C.planes(x)
    assert np.array_equal(np.ldexp(n.astype(np.float64), (e - 22)[None, :]), x)   # every element ON its column's grid
    assert d0.any() and d1.any() and d2.any()
    assert len({int(np.argmax(x[:, k])) for k in range(K)}) == K                  # the pinned maxima: a different row per column


@pytest.mark.parametrize("case", CLAIMING, ids=[c.id for c in CLAIMING])
def test_every_claimed_defect_moves_an_output_wherever_it_is_tried(case):
    got = _survey(case)
    for name, (fams, where) in DEFECTS.items():
        for d in DIRS:
            if not where(case.geometry(d)):
                continue
            for fam in fams:
                r = got.get((name, fam, d))
                assert r, "%s: %s is never tried in family %s, %s" % (case.id, name, fam, d)
                assert all(r), "%s: %s goes unseen at %d of %d places in family %s, %s" % (case.id, name, r.count(False), len(r), fam, d)
    for d in DIRS:
        for fam in FAMILIES:
            assert got[("pads counted", fam, d)] == [False]                       # invisible by construction (module docstring)
        assert got[("slab order reversed", "X", d)] == [False]                    # X is exact under any order
        if case.geometry(d)["msplit"] <= 2 or case.shape(d)[1] <= case.geometry(d)["mipw"] * 2:
            assert got[("slab order reversed", "G", d)] == [False]                # a + b = b + a


def test_every_defect_is_claimed_at_both_instantiations():
    claimed = {32: set(), 64: set()}
    for case in CLAIMING:
        for d in DIRS:
            g = case.geometry(d)
            claimed[g["KP"]] |= {name for name, (_, where) in DEFECTS.items() if where(g)}
    assert claimed[32] == claimed[64] == set(DEFECTS)


def _classes(case, d):
    g = case.geometry(d)
    out = {"nsteps %d" % g["nsteps"] if g["nsteps"] in C.NSTEPS_CLASSES else "nsteps other", "msplit %d" % g["msplit"],
           "remap" if g["remap"] else "no remap"}
    starts = {C.start_step(g, bx) for bx in range(g["nx"])} - {0}
    if g["nx"] >= 3 and len(starts) >= 2:
        out.add("nx >= 3, distinct starts")
    if g["dead"] and g["nsteps"] >= NSET:
        out.add("dead pair, nsteps >= 6")
    elif g["dead"]:
        out.add("dead pair")
    return out


CLASSES = ["nsteps %d" % k for k in C.NSTEPS_CLASSES] + ["msplit %d" % k for k in C.MSPLIT_CLASSES] + [
    "remap", "no remap", "nx >= 3, distinct starts", "dead pair, nsteps >= 6"]


def test_cases_cover_the_launch_classes():
    seen = {32: set(), 64: set()}
    for case in CLAIMING:
        for d in DIRS:
            seen[case.geometry(d)["KP"]] |= _classes(case, d)
    for KP in (32, 64):
        for cl in CLASSES:
            assert (cl in seen[KP]) != ((KP, cl) in C.UNREACHABLE), "KP = %d: %s is %s" % (
                KP, cl, "declared unreachable but covered" if cl in seen[KP] else "neither covered nor declared unreachable")
    # the declared reason, checked: no KP = 64 launch has a wave pair without units
    assert not any(C.geometry(n, 257, 40)["dead"] for n in range(1, 3000, 64))
    assert all(KP in (32, 64) and cl in CLASSES for KP, cl in C.UNREACHABLE)


def test_survey_lists_every_case():
    lines = []
    for case in CASES:
        for d in DIRS:
            g = case.geometry(d)
            n, m = case.shape(d)
            line = "%-14s %-4s n=%-5d m=%-5d KP=%d n_pad=%-5d inner_pad=%-5d msplit=%d mipw=%-5d nsteps=%-3d nx=%-3d | %s" % (
                case.id, d, n, m, g["KP"], g["n_pad"], g["inner_pad"], g["msplit"], g["mipw"], g["nsteps"], g["nx"], ", ".join(sorted(_classes(case, d))))
            if case.claims:
                got = _survey(case)
                det = [name + "[" + "".join(f for f in FAMILIES if got.get((name, f, d)) and all(got[(name, f, d)])) + "]" for name in DEFECTS]
                line += " | detects: " + ", ".join(x for x in det if not x.endswith("[]"))
                assert len([x for x in det if not x.endswith("[]")]) >= 7, line              # (the seven that apply to every launch)
            else:
                line += " | nothing missing: checks that nothing is counted"
            lines.append(line)
    print("\n" + "\n".join(lines))
    assert len(lines) == 2 * len(CASES)
