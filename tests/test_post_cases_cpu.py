"""What tests/test_post_exact_gpu.py rests on, held without a GPU: the NumPy model of the relayout and the Gram
(tests/_post_cases.py) is the plain X^T X and X.sum(0) where the sums are exact and within the fp64 forward bound where they
round; the cases reach every launch-shape class at both paddings and in both directions; and one fault at a time in the model
moves a checked output on every case that claims the class the fault lives in -- so a kernel with that fault cannot return the
model's bits there."""
import os
import re

import numpy as np
import pytest

import _post_cases as C
from bnmtf_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IDS = [c.id for c in C.CASES]


def _X(case, fam, vb=False):
    (ex, var), _ = case.factors(fam, vb)
    X = C.padded(ex, case.KP)
    S2 = None
    if vb:
        S2 = (C.padded(var, case.KP) + X * X).astype(np.float32)
        if fam == "X":
            assert np.array_equal(S2.astype(np.float64), C.padded(var, case.KP).astype(np.float64) + X.astype(np.float64) ** 2)
    return X, S2


@pytest.mark.parametrize("case", C.CASES, ids=IDS)
def test_family_X_the_model_is_the_plain_sums(case):
    vb = case in C.VB_CASES
    X, S2 = _X(case, "X", vb)
    out = C.model(X, S2, W=case.K)
    Xd = X.astype(np.float64)
    assert np.array_equal(out["C64"], Xd.T @ Xd) and np.array_equal(out["C64"], out["C64"].T)
    assert np.array_equal(out["C32"].astype(np.float64), out["C64"])                  # (below 2^24: the fp32 copy is exact too)
    assert np.array_equal(out["colsum"], Xd.sum(0))
    assert np.abs(out["C64"]).max() < 2.0 ** (21 + 2 * C.E_MAX)
    if vb:
        assert np.array_equal(out["colsum2"], S2.astype(np.float64).sum(0))
    # the layouts hold every element once, zeros elsewhere
    assert np.array_equal(out["XT"][:, :case.rows], X.T) and not out["XT"][:, case.rows:].any() and not out["XT"][case.K:].any()
    assert np.array_equal(out["XT2"][:, :, 0], out["XT"][0::2]) and np.array_equal(out["XT2"][:, :, 1], out["XT"][1::2])
    if vb:
        assert np.array_equal(out["XS"][:, :, 0], out["XT"]) and np.array_equal(out["XS"][:, :, 1], out["S2T"])
        assert np.array_equal(out["S2T"][:, :case.rows], S2.T)


@pytest.mark.parametrize("case", C.CASES[::3], ids=IDS[::3])
def test_family_G_the_model_is_within_the_forward_bound(case):
    X, _ = _X(case, "G")
    out = C.model(X, W=case.K)
    assert np.array_equal(out["C64"], out["C64"].T)
    assert np.isfinite(out["C32"]).all()
    if case.K >= 3:
        assert not out["C64"][1].any() and out["colsum"][1] == 0.0                    # the all-zero column
    ratio = C.bound_ratios(X, out, seed=case.seed)
    print("%s: largest deviation / forward bound = %.3g" % (case.id, ratio))
    assert ratio <= 1.0, ratio
    if case.rows > 64 and case.K > 1:                # the Gram's sums do round: the same rows in another order give other bits
        assert not np.array_equal(out["C64"], C.model(np.ascontiguousarray(X[::-1]), W=case.K)["C64"])


def test_the_cases_reach_every_class_at_both_paddings_and_in_both_directions():
    table = C.coverage()
    every = {(KP, w) for KP in (32, 64) for w in (0, 1)}
    for e in C.REQUIRED:
        assert table.get(e) == every, (e, table.get(e))
    for e, KP in C.REQUIRED_K.items():
        assert table.get(e) == {(KP, 0), (KP, 1)}, (e, table.get(e))
    assert {c.nblk for c in C.CASES} == set(C.NBLK) and len(IDS) == len(set(IDS))
    assert max(c.rows for c in C.CASES) <= C.MAX_ROWS
    # what the issue's list of block counts is there for, restated from the kernel's loop bounds
    assert C.clamped_live_terms(1) == {1} and C.clamped_live_terms(64) == {4} and C.clamped_live_terms(65) == {4, 5}
    assert C.clamped_live_terms(128) == set() and C.clamped_live_terms(113) == {7} and C.unrolled_groups(113, 0) == 1
    assert C.unrolled_groups(120, 0) == 8 and C.unrolled_groups(128, 0) == 16 and C.unrolled_groups(112, 0) == 0
    assert C.unrolled_groups(241, 1) == 1 and C.unrolled_groups(257, 1) == 16 and C.clamped_live_terms(129) == {1}
    # a clamped batch never has eight live terms: a batch whose eighth term is a block takes the unrolled path
    assert all(8 not in C.clamped_live_terms(n) for n in range(1, 300))
    # the variational and the tri-factorisation cases: the column-sum block's edges, both paddings
    vb = C.coverage(C.VB_CASES)
    for e in ("colsum_groups_without_work", "first_batch_unrolled_for_group_0_only", "first_batch_unrolled_for_all_groups", "no_clamped_batch",
              "clamped_batch_with_7_live", "clamped_batch_with_1_live", "second_batch", "second_batch_unrolled", "third_batch"):
        assert {KP for KP, _ in vb[e]} == {32, 64}, e
    assert len(C.TRI_CASES) == 3 and len(C.TRIVB_CASES) == 2 and all(c.K <= 32 for c in C.TRI_CASES)


def test_the_model_restates_the_kernels_constants():
    src = open(os.path.join(ROOT, "bnmtf_amd", "csrc", "kernel_post.hip")).read()
    hdr = open(os.path.join(ROOT, "bnmtf_amd", "csrc", "kernels.h")).read()
    assert re.search(r"constexpr int kPostRows = %d;" % C.RB, hdr)
    assert "for (int b = g; b < nblk; b += 32)" in src and "for (int b0 = grp; b0 < nblk; b0 += 8 * 16)" in src
    assert "if (b0 + 16 * 7 < nblk)" in src and "for (int r = grp; r < RB; r += 4)" in src
    assert "(dred[tid] + dred[64 + tid]) + (dred[128 + tid] + dred[192 + tid])" in src
    # tri_tile: the packed upper triangle row by row
    for NT in (8, 16):
        want = [(y, x) for y in range(NT) for x in range(y, NT)]
        assert [C.tri_tile(p, NT) for p in range(len(want))] == want


def test_the_dump_is_declared_bound_and_sized_alike():
    hdr = open(os.path.join(ROOT, "include", "bnmtf_hip.h")).read()
    assert re.search(r"^BNMTF_API int bnmtf_post_dump\(", hdr, flags=re.M) and "bnmtf_post_dump" in _lib.EXPORTS
    assert int(re.search(r"#define BNMTF_POST_INFO_LEN (\d+)", hdr).group(1)) == C.DUMP_INFO_LEN == len(C.DUMP_INFO) + len(C.DUMP_ARRAYS)
    assert len(_lib._SIGS["bnmtf_post_dump"][0]) == 3 + len(C.DUMP_ARRAYS)


def _claims(case_edges, fault):
    return any(e in case_edges for e in C.FAULT_EDGES[fault])


@pytest.mark.parametrize("case", C.CASES, ids=IDS)
def test_a_fault_in_the_model_moves_an_output_where_the_case_claims_its_class(case):
    vb = case in C.VB_CASES
    seen = []
    for fam in C.FAMILIES:
        X, S2 = _X(case, fam, vb)
        T, _ = C.tiles(X, 0, case.rows)
        P = C.partials(T)
        tot = C.gram_total(P)
        good = dict(C64=C.gram_scatter(tot), colsum=C.column_sums(T, case.K), **C.layouts(X, S2, 256 * (case.rows // 256 + 2)))
        case_edges = case.edges | ({"vb"} if vb else set())
        for fault in C.FAULTS:
            if not _claims(case_edges, fault):
                continue
            if fault in ("last_row_of_a_partial_block_dropped",):
                Tf, _ = C.tiles(X, 0, case.rows, fault)
                moved = not C.same_bits(C.column_sums(Tf, case.K), good["colsum"]) and not C.same_bits(C.gram(Tf), good["C64"])
            elif fault in ("block_left_out_of_a_stride", "stride_summed_twice"):
                moved = not C.same_bits(C.gram_scatter(C.gram_total(P, fault)), good["C64"])
            elif fault in ("mirror_from_the_next_row", "tri_tile_off_by_one_at_a_row_change"):
                moved = not C.same_bits(C.gram_scatter(tot, fault), good["C64"])
            elif fault in ("clamped_term_counted", "second_batch_skipped", "padding_column_counted"):
                moved = not C.same_bits(C.column_sums(T, case.K, fault), good["colsum"])
            else:
                bad = C.layouts(X, S2, 256 * (case.rows // 256 + 2), fault)
                name = "XT2" if fault == "xt2_pairs_swapped" else "XS"
                moved = not C.same_bits(bad[name], good[name])
            seen.append(fault)
            assert moved, (case.id, fam, fault)
    assert "stride_summed_twice" in seen and "xt2_pairs_swapped" in seen


def test_every_fault_is_claimed_by_cases_at_both_paddings():
    for fault in C.FAULTS:
        if fault == "own0_excluded":
            continue                                                                   # (the sharded shapes: below)
        pool = C.VB_CASES if fault == "xs_second_half_from_the_next_row" else C.CASES
        hit = {c.KP for c in pool if _claims(c.edges | {"vb"}, fault)}
        assert hit == {32, 64}, (fault, hit)


@pytest.mark.parametrize("I,J,K,world", C.SHARDED)
def test_the_own_rows_forms_of_the_ranks_add_up_to_the_whole_factor(I, J, K, world):
    inside = set()
    for which, n in enumerate((I, J)):
        KP = 32 if K <= 32 else 64
        ex, _ = C.family_X(n, K, seed=which + 7)
        X = C.padded(ex, KP)
        whole = C.model(X, W=K)
        C64 = np.zeros((KP, KP)); colsum = np.zeros(KP)
        for rank in range(world):
            first, count = C.shard_range(n, rank, world)
            assert count >= 1
            own = (first, first + count)
            part = C.model(X, W=K, own=own)
            C64 += part["C64"]; colsum += part["colsum"]
            assert C.same_bits(part["XT"], whole["XT"])                                # (the layouts are the gathered factor's)
            e = C.edges(n, K, KP, own)
            inside |= {x for x in e if x.startswith("own")}
            if first > 0:
                bad = C.model(X, W=K, own=own, fault="own0_excluded")
                assert not C.same_bits(bad["C64"], part["C64"]) and not C.same_bits(bad["colsum"], part["colsum"])
        assert np.array_equal(C64, whole["C64"]) and np.array_equal(colsum, whole["colsum"])
        empty = C.model(X, W=K, own=(n // 2, n // 2))                                  # a rank without rows (nblk = 0): zeros
        assert not empty["C64"].any() and not empty["C32"].any() and not empty["colsum"].any()
        assert "no_own_rows" in C.edges(n, K, KP, (n // 2, n // 2))
    assert {"own_rows_form", "own0_inside_a_block", "own1_inside_a_block"} <= inside
