"""The dense-rows GEMM checker (gemm_rows.py) on the CPU: for every case a correct fp32 result passes
the element-wise bound, every subtly wrong kernel that changes the case's result at all is caught, the
rules that say which launch configs take a case are self-consistent, and the fp32 emulation of the
kernel's statistics merge stays inside the bounds that the GPU test grants the row_parts reader.  Runs
without a GPU; test_gpu_gemm_rows.py applies the same checks to the kernels.

Bounds of the merged statistics (row_parts: the fp32 (mean, M2) of a row's ng = K / 64 groups of 64
columns, merged by RowParts::merge), first order in u = 2^-24, with conv_geometry's factor 2 for
operations not known to round to nearest (a supposition):

  mean.  Each group mean arrives rounded to fp32 (1 u of |mean_g| <= mean|x_g|).  A chan_add64 step
  computes mean + d * (64 / tot): a subtraction, a division, a multiplication and an addition, whose
  first-order errors are each at most u times a quantity bounded by the running |mean| or |d| * 64 / tot
  <= the 64 / tot share of (|mean_g| + |mean|).  Summed over the ng - 1 steps (the shares 64 / tot are
  the weights of the final mean) and the one or two symmetric merges this is at most (ng + 2) u times
  the row's mean |x|; doubled: |mean - mean_64| <= 2 (ng + 2) u mean|x|.

  M2.  All terms added into M2 are non-negative (the groups' M2 and d^2 * n_a n_b / n), so the
  accumulation is a sum of ng group terms and ng - 1 between-group terms without cancellation: a
  relative error of at most (ng + 6) u -- ng for the additions in any order, 1 for the stored group
  values, and 5 for the roundings inside a between-group term (d * d, the count product, the division,
  the product, and d's own rounding twice since it is squared, less the one already counted) --
  doubled: |M2 / K - var_64| <= 2 (ng + 6) u var_64.  The error of d that comes from the running mean's
  error is of second order in the result as long as the between-group terms are a small share of M2,
  which holds for rows whose groups have the same mean up to sampling noise (the share is 1 / 64).

  rstd = rsqrt(M2 / K + eps): half the relative error of its argument, ((ng + 6) u, the division by K
  and the eps addition within the 6), plus the device rsqrtf.  The installed HIP documentation carries no
  ulp table for rsqrtf, so 2 ulp = 2 * 2^-23 relative is SUPPOSED here (gemm_rows.RSQRT_ULPS).
"""
import numpy as np
import pytest
import torch

import conv_geometry as cg
import gemm_rows as gr

PRECISIONS = pytest.mark.parametrize("split", [False, True], ids=["bf16", "fp32"])
GEMM_MUTANTS = {"one_product", "last_row_is_row0", "bias_group_shift", "k_tail_early", "slice_twice"}
ACT_MUTANTS = {"clip_swapped", "gelu_tanh"}
FOLD_MUTANTS = {"col_sum_wrong_column", "mean_of_next_row", "overflow_groups_skipped"}


def test_grid_keeps_its_edges():
    """The grid keeps the properties the kernels branch on (a reminder for whoever edits CASES)."""
    cs = gr.CASES
    assert len(set(cs)) == len(cs) == 10
    ms = {c[0] * c[1] for c in cs}
    assert {1, 32, 33, 65, 129, 257} <= ms
    assert all(c[0] * c[1] <= 300 and c[2] <= 1152 and c[3] <= 320 for c in cs)
    assert any(c[2] % 64 and c[2] % 8 == 0 for c in cs) and any(c[2] % 8 for c in cs) and any(c[3] % 8 for c in cs)
    assert any(c[2] // 64 > 16 for c in cs), "more than 8 statistics groups per thread at TPR = 2"
    assert any(c[2] // 64 < 4 and c[2] % 64 == 0 for c in cs), "fewer groups than threads per row"
    assert {c[2] for c in gr.FOLD_CASES} == set(gr.FOLD_KS)
    assert any(c[1] > 1 and c[0] > 2 for c in cs), "live batches 1, B - 1, B differ"


@PRECISIONS
@pytest.mark.parametrize("case", gr.CASES, ids=gr.case_id)
def test_bound_passes_fp32_and_catches_mutants(case, split):
    p = gr.problem(case, split)
    ref, S = p["ref"], p["S"]
    assert tuple(ref.shape) == (case[0], case[1], 1, case[3])
    for splits in (1, 3, 4, 8):
        T = gr.bound(case, splits, split) * S
        assert cg.check(ref.float(), ref, T, "float64 reference through fp32") < 0.1
    # an fp32 matmul on the pre-rounded operands, standing in for the kernel
    y = (p["x"].float() @ p["w"].float().t() + p["bias"].float()).reshape(ref.shape)
    T = gr.bound(case, 1, split) * S
    assert cg.check(y, ref, T, "fp32 CPU matmul") < 0.1
    # the epilogue pass and its stored outputs, the reference rounded to storage
    Tv = gr.bound(case, 1, split, extra=1) * p["Sv"] + cg.storage(p["v"], split)
    Tu = gr.bound(case, 1, split, extra=3) * p["Su"] + cg.storage(p["u"], split)
    assert cg.check(cg.preround(p["v"], split), p["v"], Tv, "stored v") <= 1.0
    assert cg.check(cg.preround(p["u"], split), p["u"], Tu, "stored u") <= 1.0
    live = []
    for name, m in gr.mutants(p, case).items():
        if torch.equal(m, ref):
            continue  # a no-op for this case (one row, one 8-channel group in the last N tile, ...)
        live.append(name)
        with pytest.raises(AssertionError, match="outside the bound"):
            cg.check(m, ref, gr.bound(case, 3 if name == "slice_twice" else 1, split) * S, name)
    assert set(live) <= GEMM_MUTANTS and len(live) >= 3, live
    assert {"one_product", "k_tail_early", "slice_twice"} <= set(live)  # the sharpest: they apply to every case
    # activations: Clip is 1-Lipschitz, so the pre-activation's tolerance holds
    for name, (m, r) in gr.activation_mutants(p).items():
        if name == "clip_swapped":
            assert cg.check(r.float(), r, T, "clip reference through fp32") < 0.1
            frac = float((p["ref"] < p["clip_lo"]).double().mean()), float((p["ref"] > p["clip_hi"]).double().mean())
            assert p["clip_lo"] < p["clip_hi"] and (ref.numel() < 64 or all(0.2 < f < 0.45 for f in frac)), frac
            with pytest.raises(AssertionError, match="outside the bound"):
                cg.check(m, r, T, name)
        else:
            assert gr.gelu_error(r.float(), ref) < gr.GELU_BAR / 4  # fp32 rounding of the reference
            if ref.abs().max() > 0.5:
                assert gr.gelu_error(m, ref) > 100 * gr.GELU_BAR, name  # tanh-GELU: 1e-4 .. 5e-4 off
        live.append(name)


def test_bound_is_sharp_enough():
    """Loosened 100x the bound lets the single missing product pass: the margin is below 100."""
    case, split = gr.CASES[8], False  # K = 1152: a product is the smallest share of S
    p = gr.problem(case, split)
    m = gr.mutants(p, case)["one_product"]
    cg.check(m, p["ref"], 100 * gr.bound(case, 1, split) * p["S"], "one_product under 100 x T")
    with pytest.raises(AssertionError, match="outside the bound"):
        cg.check(m, p["ref"], gr.bound(case, 1, split) * p["S"], "one_product")


@PRECISIONS
@pytest.mark.parametrize("offset", gr.FOLD_OFFSETS)
@pytest.mark.parametrize("case", gr.FOLD_CASES, ids=gr.case_id)
def test_fold_reference_and_mutants(case, offset, split):
    f = gr.fold_problem(case, offset, split)
    M, K, N = case[0] * case[1], case[2], case[3]
    assert float((f["mean"].abs() / torch.sqrt(f["var"])).median()) >= 0.9 * offset  # the offsets are real
    for splits in (1, 2):
        T = gr.fold_tolerance(f, case, splits, split)
        assert cg.check(f["ref"].float(), f["ref"], T, "fold reference through fp32") < 0.1
        # the planner's fp32 operands (rounded statistics and column sums) in float64 arithmetic
        y = gr.fold_model(f, case, mean=f["row_stats"][:, 0].double(), rstd=f["row_stats"][:, 1].double(),
                          col_sum=f["col_sum"])
        assert cg.check(y, f["ref"], T, "fold with fp32 statistics") < 0.5
    live = _live_fold_mutants(f, case, split)
    assert {"col_sum_wrong_column", "mean_of_next_row"} <= set(live) <= FOLD_MUTANTS, live
    assert ("overflow_groups_skipped" in live) == (K // 64 > 16)  # more than 8 groups per thread at TPR = 2


def _live_fold_mutants(f, case, split):
    """The fold mutants that change the case's result; each must fail the check."""
    live = []
    for name, m in gr.fold_mutants(f, case).items():
        overflow = name == "overflow_groups_skipped"
        if (case[2] // 64 <= 16) if overflow else torch.equal(m, f["ref"]):
            continue
        live.append(name)
        with pytest.raises(AssertionError, match="outside the bound"):
            if overflow:
                # statistics of 16 of the 18 groups are a fair sample of the row: the outputs move by a per
                # cent, which the accumulation bound of K = 1152 at a 10 sigma offset hides -- the sharper
                # check is the GPU test's: row_parts against row_stats, the statistics terms alone
                y0 = gr.fold_model(f, case, mean=f["row_stats"][:, 0].double(), rstd=f["row_stats"][:, 1].double())
                cg.check(m, y0, gr._rows(gr.stats_terms(f, case), case), name)
            else:
                cg.check(m, f["ref"], gr.fold_tolerance(f, case, 1, split), name)
    return live


@pytest.mark.parametrize("tpr", [2, 4])
@pytest.mark.parametrize("offset", gr.FOLD_OFFSETS)
@pytest.mark.parametrize("case", gr.FOLD_CASES, ids=gr.case_id)
def test_merged_statistics_bound(case, offset, tpr):
    """merge_parts_f32 (the kernel's merge order in fp32) against float64 statistics of the stored rows,
    inside the bounds derived in the module docstring; and the row_parts tolerance holds for the fold
    evaluated with the merged statistics."""
    f = gr.fold_problem(case, offset, True)
    K = case[2]
    mean, m2, cnt = gr.merge_parts_f32(f["parts"].numpy(), tpr)
    assert float(cnt) == K
    dmean, rel_m2, rho = gr.merged_stats_bounds(f, K)
    mean64, var64 = f["mean"], f["var"]
    e_mean = (torch.from_numpy(mean.astype(np.float64)) - mean64).abs()
    assert bool((e_mean <= dmean).all()), float((e_mean / dmean).max())
    var = torch.from_numpy(m2.astype(np.float64)) / K
    e_var = (var - var64).abs() / var64
    assert float(e_var.max()) <= rel_m2, float(e_var.max()) / rel_m2
    rstd32 = (np.float32(1.0) / np.sqrt((m2 / np.float32(K) + np.float32(gr.LN_EPS)).astype(np.float32))).astype(np.float32)
    e_rstd = (torch.from_numpy(rstd32.astype(np.float64)) - f["rstd"]).abs() / f["rstd"]
    assert float(e_rstd.max()) <= rho, float(e_rstd.max()) / rho
    print("merge %s offset %g tpr %d: mean %.3f, M2 %.3f, rstd %.3f of their bounds"
          % (gr.case_id(case), offset, tpr, float((e_mean / dmean).max()), float(e_var.max()) / rel_m2,
             float(e_rstd.max()) / rho))
    y = gr.fold_model(f, case, mean=torch.from_numpy(mean.astype(np.float64)),
                      rstd=torch.from_numpy(rstd32.astype(np.float64)), col_sum=f["col_sum"])
    assert cg.check(y, f["ref"], gr.fold_tolerance(f, case, 1, True, row_parts=True), "fold with merged statistics") < 0.5
    # the two deliveries of the statistics differ by the statistics terms alone
    y0 = gr.fold_model(f, case, mean=f["row_stats"][:, 0].double(), rstd=f["row_stats"][:, 1].double(), col_sum=f["col_sum"])
    assert cg.check(y, y0, gr._rows(gr.stats_terms(f, case), case), "row_parts against row_stats") <= 1.0


def test_group64_stats_and_producer_bound():
    """group64_stats_f64 is the statistic; the fp32 round-trip of exact group statistics is far inside
    the producer's bound (test_gpu_gemm_rows.py derives it)."""
    g = torch.Generator().manual_seed(7)
    v = torch.randn(5, 192, generator=g).double() + 3.0
    st = gr.group64_stats_f64(v)
    assert tuple(st.shape) == (5, 3, 2)
    assert torch.allclose(st[..., 0], v.reshape(5, 3, 64).mean(-1))
    assert torch.allclose(st[..., 1], v.reshape(5, 3, 64).var(-1, unbiased=False) * 64)
    assert float(((st.float().double() - st).abs()[..., 1] / st[..., 1]).max()) < 2 * 70 * gr.U / 100


def test_expected_cfgs_rules():
    """The config rules against a few hand-worked launches (kernels.h TileCfg, the launchers' guards)."""
    E = gr.expected_cfgs
    all_dma_bf16 = [c for c in range(4, 24) if c != 16]  # 6 stages of 128x128 do not fit
    assert E((3, 43, 320, 136), False, 1) == [0, 1, 2, 3] + all_dma_bf16
    # fp32: doubled stages -- 128x128: 2 stages; 128x64, 64x128: 3; 64x64: 4; plus the wide tile
    assert E((3, 43, 320, 136), True, 3) == [0, 1, 2, 3, 4, 5, 6, 7, 9, 10, 11, 15, 20, 21, 22, 23, 28]
    assert E((1, 1, 256, 8), False, 1) == [0, 1, 2, 3] + all_dma_bf16 + [32]
    assert 32 not in E((1, 1, 256, 8), False, 3) and 32 in E((4, 8, 256, 40), True, 1)
    assert 32 not in E((3, 11, 256, 72), False, 1)
    assert E((6, 5, 72, 64), True, 1) == [0, 1, 2, 3] == E((2, 9, 20, 12), False, 1)
    assert E((2, 9, 20, 12), False, 3) == []
    assert E((3, 43, 320, 136), True, 1, stats_out=True) == [] and E((2, 35, 128, 128), False, 2, stats_out=True)
    assert E((2, 35, 128, 128), False, 1, row_parts=True) == []
    assert 28 in E((2, 35, 128, 128), True, 2, row_parts=True)
    assert E((4, 8, 256, 40), True, 1, row_parts=True) == [c for c in E((4, 8, 256, 40), True, 1) if c != 32]
    assert E((5, 13, 64, 64), False, 3, tail=True) == [] and 7 in E((2, 35, 128, 128), False, 3, tail=True)
    assert E((3, 43, 320, 136), False, 1, sk=True) == [4, 5, 6, 7, 20, 21, 22, 23]
    assert E((3, 43, 320, 136), True, 1, sk=True) == [4, 5, 6, 7, 20, 21, 22, 23]
    assert all(c not in E(case, s, 1) for case in gr.CASES for s in (False, True) for c in (24, 25, 26, 27, 29, 30, 31, 39))


def test_every_mutant_applies_somewhere():
    seen = set()
    for case in gr.CASES:
        p = gr.problem(case, False)
        seen |= {n for n, m in gr.mutants(p, case).items() if not torch.equal(m, p["ref"])}
        seen |= {n for n, (m, r) in gr.activation_mutants(p).items() if not torch.equal(m, r)}
    for case in gr.FOLD_CASES:
        f = gr.fold_problem(case, 10.0, True)
        seen |= set(_live_fold_mutants(f, case, True))
    assert seen == GEMM_MUTANTS | ACT_MUTANTS | FOLD_MUTANTS, seen ^ (GEMM_MUTANTS | ACT_MUTANTS | FOLD_MUTANTS)
