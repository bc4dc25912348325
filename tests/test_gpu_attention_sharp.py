"""The streaming attention kernel (csrc/kernels/transformer.hip attention_stream_kernel) element by
element against float64, on the grid, input families and derived bound of attention_oracle.py.

Sharp pass: every case x family x {bf16, fp32}; each launch writes into a buffer pre-filled with a
sentinel bit pattern that is wider and longer than the result -- every element of the result block
must lie inside the bound and every sentinel outside it must survive (both planes in fp32 mode).
Pitches and offsets: q, k, v in three buffers of three pitches at non-zero 8-column offsets with NaN
in every unused column, the output at a 4-column offset in rows of H D + 4 and H D + 24 elements, the
bias table's pad columns at 1e30: bit for bit the dense layout's result.  Block mappings: on the cases
the XCD map takes, the natural mapping (variant 2) and contiguous pair ranges (variant 3) give the
default's bits in every mode, two-tile staging (variant 1) in the unmasked mode, groups of one through
the GQA mode (variant 4) where that mode applies.

Largest |err| / T of the sharp pass observed on an MI355X, per mode over all its cases and families
(T: attention_oracle.bound_of; pytest -s prints these lines, and one per case, family and precision):
  none            bf16 0.6741   fp32 0.0258
  bias_shared     bf16 0.6778   fp32 0.0147
  bias_per_head   bf16 0.6734   fp32 0.0169
  causal          bf16 0.7729   fp32 0.0843
  causal_bias     bf16 0.8305   fp32 0.0964
  keymask         bf16 0.7125   fp32 0.0193
  keymask_holes   bf16 0.7074   fp32 0.0176
  keymask_bias    bf16 0.6692   fp32 0.0209
The bf16 figures are the two 2^-8 terms (P rounded to bf16, the stored output rounded to bf16), which
round-to-nearest nearly reaches; the CPU model of the same arithmetic sits at 0.5.  The fp32 figures
show how much of that bound is worst-case accumulation (2 n u Sx over 3 D products) that a real sum
does not reach: a tenth at most, in the causal cases of head dim 32 with 192 pairs.  No constant of
the bound was changed after these runs.  Every bitwise comparison below held.
"""
import math

import pytest

import attention_oracle as ao
from conftest import gpu_available

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not gpu_available(), reason="needs a GPU")]

PRECISIONS = pytest.mark.parametrize("split", [False, True], ids=["bf16", "fp32"])
SENTINEL = 0x7FA5  # a bf16 NaN: an element the kernel skipped fails the bound as well
WORST = {}         # (mode, split) -> largest |err| / T seen by the sharp pass


@pytest.fixture(scope="module")
def K():
    from die_amd.ops import kernels

    return kernels


def _mapped(case):
    nqb, gy, gz = ao.launch_grid(case)
    return (gy * gz) % 8 == 0


def _place(K, t, split, ld, col, fill):
    """[B, S, Hx, D] float64 storage values -> ([planes, B * S, ld] bf16 on the GPU with the block at
    column `col` and `fill` everywhere else, the address of the block's first element)."""
    import torch

    B, S, Hx, D = t.shape
    R, W = B * S, Hx * D
    rows = t.float().reshape(R, W)
    planes = K.split_planes(rows) if split else rows.to(torch.bfloat16)[None]
    buf = torch.full((planes.shape[0], R, ld), fill, dtype=torch.bfloat16, device="cuda")
    buf[:, :, col:col + W] = planes.cuda()
    return buf, buf.data_ptr() + 2 * col


DENSE = dict(ldq=0, cq=0, ldk=0, ck=0, ldv=0, cv=0, ldo=0, co=0, bias_pad=0.0)


def _run(K, p, ldq=0, cq=0, ldk=0, ck=0, ldv=0, cv=0, ldo=0, co=0, bias_pad=0.0):
    """One launch of problem p in the given layout (pitch 0: the block's own width) into a
    sentinel-filled buffer.  Asserts that nothing outside the result block was written; returns the
    block's raw bits [planes, B * S, C] int16 (GPU) and its values [B, S, H, D] float64 (CPU)."""
    import torch

    B, H, Hkv, D, S, mode = p["case"]
    split = p["split"]
    C, Ckv, R = H * D, Hkv * D, B * S
    ldq, ldk, ldv, ldo = ldq or C, ldk or Ckv, ldv or Ckv, ldo or C
    nan = float("nan")
    qb, qp = _place(K, p["q"], split, ldq, cq, nan)
    kb, kp = _place(K, p["k"], split, ldk, ck, nan)
    vb, vp = _place(K, p["v"], split, ldv, cv, nan)
    npl = 2 if split else 1
    guard = 3 * ldo + 8
    flat = torch.full((guard + npl * R * ldo + guard,), SENTINEL, dtype=torch.int16, device="cuda")
    table = None if p["table"] is None else p["table"].cuda()
    vis = None if p["vis"] is None else p["vis"].cuda()
    K.attention_launch(qp, kp, vp, flat.data_ptr() + 2 * (guard + co), B, S, H, D, ldq, ldk, ldv, ldo, p["scale"],
                       split=split, bias=table, causal=ao.is_causal(mode), key_mask=vis,
                       kv_heads=Hkv if Hkv != H else None, bias_pad=bias_pad)
    torch.cuda.synchronize()
    body = flat[guard:guard + npl * R * ldo].view(npl, R, ldo)
    bits = body[:, :, co:co + C].clone()
    body[:, :, co:co + C] = SENTINEL
    stray = int((flat != SENTINEL).sum())
    assert stray == 0, "%d elements written outside the result block" % stray
    vals = bits.view(torch.bfloat16).double()
    vals = (vals[0] + vals[1]) if split else vals[0]
    return bits, vals.reshape(B, S, H, D).cpu()


# ---- sharp pass -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", ao.CASES, ids=ao.case_id)
def test_sharp(K, case):
    # wider (8 more columns per row) and longer (guard rows at both ends) than the result
    C = case[1] * case[3]
    for split in (False, True):
        for family in ao.FAMILIES:
            p = ao.problem(case, family, split)
            _, got = _run(K, p, ldo=C + 8)
            what = "%s %s %s" % (ao.case_id(case), family, "fp32" if split else "bf16")
            worst = ao.check(got, p["O"], p["T"], what)
            print("%s: |err| / T <= %.4f" % (what, worst))
            key = (case[5], split)
            WORST[key] = max(WORST.get(key, 0.0), worst)


# ---- pitches and offsets ----------------------------------------------------------------------------------

def _one_case_per_mode():
    cs = [next(c for c in ao.CASES if c[5] == m and c[1] == c[2] and _mapped(c)) for m in ao.MODES]
    cs.append(next(c for c in ao.CASES if c[1] != c[2] and c[5] == "causal" and _mapped(c)))
    cs.append(next(c for c in ao.CASES if c[1] != c[2] and c[5] == "keymask" and _mapped(c)))
    cs.append(next(c for c in ao.CASES if c[3] == 80 and c[5] == "none"))  # H D + 4 = 244
    return cs


@PRECISIONS
@pytest.mark.parametrize("case", _one_case_per_mode(), ids=ao.case_id)
def test_pitches_and_offsets(K, case, split):
    import torch

    B, H, Hkv, D, S, mode = case
    C, Ckv = H * D, Hkv * D
    p = ao.problem(case, "randn", split)
    dense, _ = _run(K, p)
    for extra in (4, 24):
        assert (C + extra) % 8 == (4 if extra == 4 else 0)
        bits, got = _run(K, p, ldq=C + 24, cq=8, ldk=Ckv + 40, ck=16, ldv=Ckv + 16, cv=8, ldo=C + extra, co=4, bias_pad=1e30)
        assert torch.equal(bits, dense), (ao.case_id(case), extra)
    ao.check(got, p["O"], p["T"], ao.case_id(case))


# ---- block mappings ---------------------------------------------------------------------------------------

@PRECISIONS
@pytest.mark.parametrize("case", [c for c in ao.CASES if _mapped(c)], ids=ao.case_id)
def test_block_mappings_agree_bitwise(K, case, split):
    import torch

    B, H, Hkv, D, S, mode = case
    p = ao.problem(case, "randn", split)
    variants = [2, 3]
    if mode == "none" and Hkv == H:
        variants.append(1)  # two-tile staging: the unmasked multi-head kernel only
    if Hkv == H and D in (64, 128) and not ao.has_bias(mode):
        variants.append(4)  # groups of one through the GQA mode
    base, got = _run(K, p)
    ao.check(got, p["O"], p["T"], ao.case_id(case))
    try:
        for v in variants:
            K.set_attention_variant(v)
            bits, _ = _run(K, p)
            assert torch.equal(bits, base), (ao.case_id(case), v)
    finally:
        K.set_attention_variant(0)


def test_mapped_cases_cover_every_mode():
    assert {c[5] for c in ao.CASES if _mapped(c) and c[1] == c[2]} == set(ao.MODES)


def test_report():
    """Prints the sharp pass's maxima (pytest -s); they are all below 1 or test_sharp failed."""
    for (mode, split), w in sorted(WORST.items()):
        print("sharp pass  %-14s %s  %.4f" % (mode, "fp32" if split else "bf16", w))
    assert all(w <= 1.0 and math.isfinite(w) for w in WORST.values())
