"""The SiLU (4) and HardSwish (5) epilogue codes in every conv kernel family, against the float64 conv on the
STORED operands followed by the float64 activation.  One small shape per family, with an M tail (162 = 2 x 9 x 9
pixels, or 5 rows) and channels that do not fill the tile (40).  Bars: rel-L2 < 2e-5 split in every family;
bf16 < 5e-3 for conv_igemm (tests/test_gpu_kernels.py) and < 1e-2 for the grouped / depthwise kernels
(tests/test_gpu_dwconv.py)."""
import pytest

from conftest import gpu_available

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not gpu_available(), reason="needs a GPU")]

# conv_igemm: name -> (Cin, k, rows-only, launch config = tile + 4 * variant, splits, fused split-K)
IGEMM = {"register_staged": (24, 3, False, 3, 1, True), "lds_dma": (64, 1, False, 7, 1, True),
         "fused_splitk": (64, 3, False, 3, 2, True), "separate_splitk": (64, 3, False, 3, 2, False),
         "skinny": (256, 1, True, 32, 1, True)}  # K a multiple of the 8 waves' 32-wide steps
# grouped kernels: name -> (C, groups, k, stride)
GROUPED = {"grouped_conv": (40, 5, 3, 1), "grouped_conv_mfma": (48, 6, 3, 1), "dwconv_tiled": (40, 40, 5, 1),
           "dwconv_poly": (40, 40, 3, 2)}


def _act(v, act):
    import torch.nn.functional as F

    return F.silu(v) if act == 4 else F.hardswish(v)


def _stored(t, split):
    import torch

    from die_amd.ops import kernels as K

    return (K.join_planes(K.split_planes(t)) if split else t.to(torch.bfloat16).float()).double()


def _rel(got, ref):
    return float((got.double() - ref).norm() / ref.norm())


@pytest.mark.parametrize("split", [False, True])
@pytest.mark.parametrize("act", [4, 5])
@pytest.mark.parametrize("family", list(IGEMM))
def test_conv_igemm(native, family, act, split):
    import torch
    import torch.nn.functional as F

    from die_amd.ops import kernels as K

    Cin, k, rows, cfg, splits, fused = IGEMM[family]
    g = torch.Generator(device="cuda").manual_seed(7)
    x = torch.randn((5, 1, 1, Cin) if rows else (2, 9, 9, Cin), device="cuda", generator=g)
    w = torch.randn(40, Cin, k, k, device="cuda", generator=g) / (Cin * k * k) ** 0.5 * 2
    bias = torch.randn(40, device="cuda", generator=g)
    out, _ = K.conv2d_nhwc(x if split else x.to(torch.bfloat16), w, bias, pad=k // 2, relu=act, tile=cfg, splits=splits,
                           fused_splitk=fused, split=split)
    assert out is not None, "the config does not take this shape"
    torch.cuda.synchronize()
    ref = _act(F.conv2d(_stored(x, split).permute(0, 3, 1, 2), _stored(w, split), bias.double(), padding=k // 2), act)
    err = _rel(out.float().permute(0, 3, 1, 2), ref)
    print(family, act, split, "rel-L2 %.3g" % err)
    assert err < (2e-5 if split else 5e-3), err


@pytest.mark.parametrize("split", [False, True])
@pytest.mark.parametrize("act", [4, 5])
@pytest.mark.parametrize("family", list(GROUPED))
def test_grouped_kernels(native, family, act, split):
    import torch
    import torch.nn.functional as F

    from die_amd.ops import kernels as K

    C, groups, k, stride = GROUPED[family]
    g = torch.Generator(device="cuda").manual_seed(9)
    x = torch.randn(2, 9, 9, C, device="cuda", generator=g)
    w = torch.randn(C, C // groups, k, k, device="cuda", generator=g) / (C // groups * k * k) ** 0.5 * 2
    bias = torch.randn(C, device="cuda", generator=g)
    pads = (k // 2,) * 4
    if family == "grouped_conv":
        vals = K.grouped_conv(x, w, bias, stride, pads, groups, relu=act, split=split).float()
    else:
        fn = {"grouped_conv_mfma": K.grouped_conv_mfma, "dwconv_tiled": K.depthwise_conv, "dwconv_poly": K.depthwise_conv_poly}[family]
        out, _ = fn(x, w, bias, pads, stride, relu=act, split=split, groups=groups)
        vals = K.join_planes(out) if split else out.float()
    torch.cuda.synchronize()
    wq = w.double() if family != "grouped_conv_mfma" else _stored(w, split)  # fp32 weights but in the MFMA kernel
    ref = _act(F.conv2d(_stored(x, split).permute(0, 3, 1, 2), wq, bias.double(), stride=stride, padding=k // 2, groups=groups), act)
    err = _rel(vals.permute(0, 3, 1, 2), ref)
    print(family, act, split, "rel-L2 %.3g" % err)
    assert err < (2e-5 if split else 1e-2), err
