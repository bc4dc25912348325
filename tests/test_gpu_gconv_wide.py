"""The wide-group MFMA grouped 3x3 conv kernel (csrc/kernels/gconv_wide.hip) through ops.kernels.grouped_conv_wide
against a float64 F.conv2d(..., groups=C // w), element by element under the law of tests/conv_geometry.py:
T = eps * S, eps = 2 * (9 w + 3 + extra) * 2^-24 (+ 2^-16 in fp32 mode), S the same conv on |x|, |w|, |bias| (+ |res|),
stored outputs add the storage rounding of the reference; SiLU / HardSwish scale eps by max |f'| (ACT_LAW).
One missing tap is about S / (9 w) >= S / 576; eps <= 1.3e-4.
C = 3 w: three groups, and C = 72 / 120 / 168 for the widths that are no multiple of 16.

Worst |err| / T measured on an MI355X over all the cases below: 0.973 in bf16 mode (stored bf16 outputs: half an
ulp is up to 2^-8 |ref| at the bottom of a binade, which is the storage term itself), 0.093 in fp32 mode."""
import functools

import pytest

from conftest import gpu_available
from conv_geometry import check, preround, storage

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not gpu_available(), reason="needs a GPU")]

WIDTHS = [24, 40, 48, 56, 64]
# (H, W, stride, (top, left, bottom, right))
GEOMS = [(9, 11, 1, (1, 1, 1, 1)),   # ragged 8x8 tiles on both axes
         (5, 7, 1, (1, 1, 1, 1)),    # map smaller than a tile
         (12, 10, 2, (0, 0, 1, 1)),  # TF "SAME" stride 2: begin pad != end pad
         (11, 9, 2, (1, 1, 1, 1)),   # odd map at stride 2, halo 17 wide
         (9, 8, 1, (2, 1, 0, 1)),    # four different pads
         (1, 1, 1, (1, 1, 1, 1)),    # every tap but the centre is padding
         (17, 9, 1, (1, 1, 1, 1))]   # with 128 groups: 12 tiles for the 8 blocks of a group, the stationary weights reused
MANY = len(GEOMS) - 1
EPILOGUES = [dict(bias=True, want_f32=True), dict(bias=False), dict(bias=True, act=1),
             dict(bias=True, clip=(-0.5, 0.75)), dict(bias=True, residual=True),
             dict(bias=True, act=1, residual=True, want_f32=True), dict(bias=True, live=2, want_f32=True),
             dict(bias=True, act=4, want_f32=True), dict(bias=True, act=5, residual=True)]
# SiLU / HardSwish f behind a pre-activation v with |v - v_ref| <= eps S: |f(v) - f(v_ref)| <= max |f'| eps S, and
# |f(v)| <= |v| <= S, so the roundings of evaluating f count as `extra` terms.  act -> (max |f'|, extra):
#   SiLU: max |f'| = 1.0998; v * rcp(1 + exp(-v)) with the fast exp (argument -v log2 e rounded once: a relative
#     error of |v| 2^-24 log 2 in exp(-v), under 12 * 2^-24 for |v| <= 12; exp2, add, rcp and the product one
#     rounding each): 16;  HardSwish: max |f'| = 1.5 (at v -> 3); fma, clamp, product: 2
ACT_LAW = {4: (1.1, 16), 5: (1.5, 2)}
FILL = -7.0  # sentinel in the output buffers (exact in bf16)


@functools.lru_cache(maxsize=None)
def _problem(gi, w, split, B, residual):
    """Operands the storage holds exactly (float64, CPU), the pre-activation reference and S; shared, read only."""
    import torch
    import torch.nn.functional as F

    H, W, s, (t, l, b, r) = GEOMS[gi]
    G = 128 if gi == MANY else 3
    C = G * w
    g = torch.Generator().manual_seed(100 * gi + w)
    x = preround(torch.randn(B, C, H, W, generator=g), split)
    wt = preround(torch.randn(C, w, 3, 3, generator=g) / (9 * w) ** 0.5, split)
    bias = torch.randn(C, generator=g).float().double()

    def conv(xx, ww, bb):
        return F.conv2d(F.pad(xx, (l, r, t, b)), ww, bb, stride=s, groups=G).permute(0, 2, 3, 1).contiguous()

    ref, ref0 = conv(x, wt, bias), conv(x, wt, None)
    S, S0 = conv(x.abs(), wt.abs(), bias.abs()), conv(x.abs(), wt.abs(), None)
    res = preround(torch.randn(ref.shape, generator=g), split) if residual else None
    return dict(x=x, w=wt, bias=bias, res=res, ref=ref, ref0=ref0, S=S, S0=S0, C=C)


def _run(gi, w, split, epi):
    """Runs one case and checks every element; returns the largest |err| / T."""
    import torch
    import torch.nn.functional as F

    from die_amd.ops import kernels as K

    B = 3 if "live" in epi else 2
    live = epi.get("live", B)
    p = _problem(gi, w, split, B, bool(epi.get("residual")))
    s, pads = GEOMS[gi][2], GEOMS[gi][3]
    has_bias, act = bool(epi.get("bias")), epi.get("act", 0)
    ref, S = (p["ref"], p["S"]) if has_bias else (p["ref0"], p["S0"])
    ref = {0: ref, 1: ref.clamp(min=0), 4: F.silu(ref), 5: F.hardswish(ref)}[act]
    if epi.get("clip"):
        ref = ref.clamp(*epi["clip"])
    lip, extra = ACT_LAW.get(act, (1.0, 0))
    if p["res"] is not None:
        ref, S, extra = ref + p["res"], S + p["res"].abs(), extra + 1
    eps = lip * (2.0 * (9 * w + 3 + extra) * 2.0 ** -24 + (2.0 ** -16 if split else 0.0))
    dev = "cuda"
    xin = p["x"].float().permute(0, 2, 3, 1).contiguous().to(dev)
    out, of = K.grouped_conv_wide(xin if split else xin.to(torch.bfloat16), p["w"].float().to(dev),
                                  p["bias"].float().to(dev) if has_bias else None, pads=pads, stride=s,
                                  clip=epi.get("clip"), relu=act,
                                  residual=None if p["res"] is None else p["res"].float().to(dev), split=split,
                                  want_f32=bool(epi.get("want_f32")), live=epi.get("live"), fill=FILL, groups=p["C"] // w)
    torch.cuda.synchronize()
    what = (GEOMS[gi], w, split, epi)
    vals = (K.join_planes(out) if split else out.float()).cpu()
    worst = check(vals[:live], ref[:live], eps * S[:live] + storage(ref[:live], split), what)
    if of is not None:
        worst = max(worst, check(of.cpu()[:live], ref[:live], eps * S[:live], what))
    if live < B:  # samples past the live count keep the sentinel, in every plane and in the f32 output
        assert bool((out[..., live:, :, :, :] == FILL).all()) and bool((of[live:] == FILL).all()), what
    print("gconv_wide %s worst |err|/T %.3f" % (what, worst))
    return worst


@pytest.mark.parametrize("gi", range(MANY))
@pytest.mark.parametrize("split", [False, True])
@pytest.mark.parametrize("w", WIDTHS)
def test_against_float64(native, w, split, gi):
    _run(gi, w, split, EPILOGUES[(gi + WIDTHS.index(w)) % len(EPILOGUES)])


@pytest.mark.parametrize("gi", [1, 2])
@pytest.mark.parametrize("split", [False, True])
@pytest.mark.parametrize("w", WIDTHS)
def test_every_epilogue(native, w, split, gi):
    for epi in EPILOGUES:
        _run(gi, w, split, epi)


@pytest.mark.parametrize("split", [False, True])
@pytest.mark.parametrize("w", [24, 40])  # two waves per bundle; three bundles and a wave that only loads
def test_block_walks_several_tiles(native, w, split):
    _run(MANY, w, split, EPILOGUES[5])


@pytest.mark.parametrize("case", [dict(C=64, cw=16), dict(C=64, cw=32), dict(C=144, cw=72), dict(C=80, cw=20),
                                  dict(C=48, cw=24, Cout=96), dict(C=48, cw=24, k=5), dict(C=48, cw=24, dilation=2),
                                  dict(C=48, cw=24, stride=3)],
                         ids=["w16", "w32", "w72", "w20", "cpg_ne_opg", "5x5", "dilation2", "stride3"])
def test_out_of_scope_is_invalid_value(native, case):
    """hipErrorInvalidValue (1) from the launcher's own check, before any launch: the outputs keep their sentinel"""
    import json

    import torch

    from die_amd import native as nat

    C, cw, k, Cout = case["C"], case["cw"], case.get("k", 3), case.get("Cout", case["C"])
    x = torch.randn(1, 8, 8, C, device="cuda").to(torch.bfloat16)
    wp = torch.zeros(Cout * 2 * 672, dtype=torch.bfloat16, device="cuda")
    out = torch.full((1, 8, 8, Cout), FILL, dtype=torch.bfloat16, device="cuda")
    of = torch.full((1, 8, 8, Cout), FILL, dtype=torch.float32, device="cuda")
    geom = dict(B=1, H=8, W=8, Cin=C, Ho=8, Wo=8, Cout=Cout, groups=C // cw, KH=k, KW=k, stride=case.get("stride", 1),
                dil=case.get("dilation", 1), pad_h=1, pad_w=1, act=0, split=0)
    rc = nat.kernels().die_kern_gconv_wide(json.dumps(geom).encode(), x.data_ptr(), wp.data_ptr(), 0, 0, 0, out.data_ptr(),
                                           of.data_ptr(), 0, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert rc == 1 and bool((out == FILL).all()) and bool((of == FILL).all()), (case, rc)
