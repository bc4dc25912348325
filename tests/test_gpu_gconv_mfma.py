"""The MFMA grouped 3x3 conv kernel (csrc/kernels/gconv_mfma.hip) through ops.kernels.grouped_conv_mfma against
a float64 F.conv2d(..., groups=C // w), element by element under the law of tests/conv_geometry.py: T = eps * S,
eps = 2 * (9 w + 3 + extra) * 2^-24 (+ 2^-16 in fp32 mode), S the same conv on |x|, |w|, |bias| (+ |res|), stored
outputs add the storage rounding of the reference.  One missing tap is about S / (9 w) >= S / 288; eps <= 5e-5.

Worst |err| / T measured on an MI355X over all the cases below: 0.991 in bf16 mode (stored bf16 outputs:
half an ulp is up to 2^-8 |ref| at the bottom of a binade, which is the storage term itself), 0.228 in fp32 mode."""
import functools

import pytest

from conftest import gpu_available
from conv_geometry import check, preround, storage

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not gpu_available(), reason="needs a GPU")]

# (H, W, C, C for w = 32, stride, (top, left, bottom, right))
GEOMS = [(9, 11, 64, 64, 1, (1, 1, 1, 1)),     # ragged 8x8 tiles on both axes, one full chunk
         (5, 7, 80, 96, 1, (1, 1, 1, 1)),      # map smaller than a tile, partial trailing chunk
         (12, 10, 128, 128, 2, (0, 0, 1, 1)),  # TF "SAME" stride 2, two chunks, weights kept across chunks' tiles
         (11, 9, 64, 64, 2, (1, 1, 1, 1)),     # odd map at stride 2, halo 17 wide
         (9, 8, 64, 64, 1, (2, 1, 0, 1)),      # four different pads
         (1, 1, 64, 64, 1, (1, 1, 1, 1))]      # every tap but the centre is padding
EPILOGUES = [dict(bias=True, want_f32=True), dict(bias=False), dict(bias=True, relu=True),
             dict(bias=True, clip=(-0.5, 0.75)), dict(bias=True, residual=True),
             dict(bias=True, relu=True, residual=True, want_f32=True), dict(bias=True, live=2, want_f32=True)]
FILL = -7.0  # sentinel in the output buffers (exact in bf16)


@functools.lru_cache(maxsize=None)
def _problem(gi, w, split, B, residual):
    """Operands the storage holds exactly (float64, CPU), the pre-activation reference and S; shared, read only."""
    import torch
    import torch.nn.functional as F

    H, W, C, C32, s, (t, l, b, r) = GEOMS[gi]
    C = C32 if w == 32 else C
    g = torch.Generator().manual_seed(100 * gi + w)
    x = preround(torch.randn(B, C, H, W, generator=g), split)
    wt = preround(torch.randn(C, w, 3, 3, generator=g) / (9 * w) ** 0.5, split)
    bias = torch.randn(C, generator=g).float().double()

    def conv(xx, ww, bb):
        return F.conv2d(F.pad(xx, (l, r, t, b)), ww, bb, stride=s, groups=C // w).permute(0, 2, 3, 1).contiguous()

    ref, ref0 = conv(x, wt, bias), conv(x, wt, None)
    S, S0 = conv(x.abs(), wt.abs(), bias.abs()), conv(x.abs(), wt.abs(), None)
    res = preround(torch.randn(ref.shape, generator=g), split) if residual else None
    return dict(x=x, w=wt, bias=bias, res=res, ref=ref, ref0=ref0, S=S, S0=S0, C=C)


def _run(gi, w, split, epi):
    """Runs one case and checks every element; returns the largest |err| / T."""
    import torch

    from die_amd.ops import kernels as K

    B = 3 if "live" in epi else 2
    live = epi.get("live", B)
    p = _problem(gi, w, split, B, bool(epi.get("residual")))
    s, pads = GEOMS[gi][4], GEOMS[gi][5]
    has_bias = bool(epi.get("bias"))
    ref, S = (p["ref"], p["S"]) if has_bias else (p["ref0"], p["S0"])
    if epi.get("relu"):
        ref = ref.clamp(min=0)
    if epi.get("clip"):
        ref = ref.clamp(*epi["clip"])
    extra = 0
    if p["res"] is not None:
        ref, S, extra = ref + p["res"], S + p["res"].abs(), 1
    eps = 2.0 * (9 * w + 3 + extra) * 2.0 ** -24 + (2.0 ** -16 if split else 0.0)
    dev = "cuda"
    xin = p["x"].float().permute(0, 2, 3, 1).contiguous().to(dev)
    out, of = K.grouped_conv_mfma(xin if split else xin.to(torch.bfloat16), p["w"].float().to(dev),
                                  p["bias"].float().to(dev) if has_bias else None, pads=pads, stride=s,
                                  clip=epi.get("clip"), relu=bool(epi.get("relu")),
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
    print("gconv_mfma %s worst |err|/T %.3f" % (what, worst))
    return worst


@pytest.mark.parametrize("gi", range(len(GEOMS)))
@pytest.mark.parametrize("split", [False, True])
@pytest.mark.parametrize("w", [4, 8, 16, 32])
def test_against_float64(native, w, split, gi):
    _run(gi, w, split, EPILOGUES[(gi + [4, 8, 16, 32].index(w)) % len(EPILOGUES)])


@pytest.mark.parametrize("gi", [1, 2])
@pytest.mark.parametrize("split", [False, True])
@pytest.mark.parametrize("w", [4, 8, 16, 32])
def test_every_epilogue(native, w, split, gi):
    for epi in EPILOGUES:
        _run(gi, w, split, epi)


@pytest.mark.parametrize("case", [dict(C=64, cw=2), dict(C=128, cw=64), dict(C=64, cw=8, Cout=128), dict(C=64, cw=8, k=5),
                                  dict(C=64, cw=8, dilation=2), dict(C=64, cw=8, stride=3), dict(C=72, cw=8)],
                         ids=["w2", "w64", "cpg_ne_opg", "5x5", "dilation2", "stride3", "c72_w8"])
def test_out_of_scope_is_invalid_value(native, case):
    """hipErrorInvalidValue (1) from the launcher's own check, before any launch: the outputs keep their sentinel"""
    import json

    import torch

    from die_amd import native as nat

    C, cw, k, Cout = case["C"], case["cw"], case.get("k", 3), case.get("Cout", case["C"])
    x = torch.randn(1, 8, 8, C, device="cuda").to(torch.bfloat16)
    wp = torch.zeros(Cout * 288, dtype=torch.bfloat16, device="cuda")
    out = torch.full((1, 8, 8, Cout), FILL, dtype=torch.bfloat16, device="cuda")
    of = torch.full((1, 8, 8, Cout), FILL, dtype=torch.float32, device="cuda")
    geom = dict(B=1, H=8, W=8, Cin=C, Ho=8, Wo=8, Cout=Cout, groups=C // cw, KH=k, KW=k, stride=case.get("stride", 1),
                dil=case.get("dilation", 1), pad_h=1, pad_w=1, act=0, split=0)
    rc = nat.kernels().die_kern_gconv_mfma(json.dumps(geom).encode(), x.data_ptr(), wp.data_ptr(), 0, 0, 0, out.data_ptr(),
                                           of.data_ptr(), 0, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert rc == 1 and bool((out == FILL).all()) and bool((of == FILL).all()), (case, rc)
