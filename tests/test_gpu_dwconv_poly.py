"""The polyphase tiled depthwise conv kernel (csrc/kernels/dwconv_poly.hip) through
ops.kernels.depthwise_conv_poly, in its three classes (3x3 stride 1, 3x3 stride 2, 5x5 stride 2): bit for bit the
output of gconv_kernel on the same inputs, and the bars of tests/test_gpu_dwconv.py against a float64 torch
conv2d (rel-L2 2e-5 split, 1e-2 bf16).  Maps: smaller than a tile, one tile exactly, partial tiles on both
edges, both tile widths, odd and even widths (the two column-parity planes differ in length); channel counts
with a partial 32-channel slice; symmetric, zero, TF "SAME" and asymmetric pads."""
import itertools

import pytest

from conftest import gpu_available
from test_gpu_dwconv import EPILOGUES, FILL, B, _check

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not gpu_available(), reason="needs a GPU")]

CLASSES = [(3, 1), (3, 2), (5, 2)]
MAPS = [(1, 1), (2, 2), (5, 7), (9, 16), (14, 14), (17, 33)]
CHANNELS = [8, 24, 40]


def _pads(k):  # top, left, bottom, right
    return [(k // 2,) * 4, (0, 0, 0, 0), (0, 0, 1, 1), (2, 1, 0, 2)]


def _case(k, stride, H, W, C, pads, epi, split, seed):
    """Runs both kernels and the float64 reference; returns what test_gpu_dwconv._check takes, or None when the
    window does not fit the padded map."""
    import torch

    from die_amd.ops import kernels as K

    if H + pads[0] + pads[2] < k or W + pads[1] + pads[3] < k:
        return None
    g = torch.Generator(device="cuda").manual_seed(seed)
    x = torch.randn(B, C, H, W, device="cuda", generator=g)
    w = torch.randn(C, 1, k, k, device="cuda", generator=g) * 0.3
    b = torch.randn(C, device="cuda", generator=g) if epi.get("bias") else None
    ref = torch.nn.functional.conv2d(torch.nn.functional.pad(x.double(), (pads[1], pads[3], pads[0], pads[2])), w.double(),
                                     None if b is None else b.double(), stride=stride, groups=C)
    r = torch.randn(ref.shape, device="cuda", generator=g) if epi.get("residual") else None
    if epi.get("relu"):
        ref = ref.clamp(min=0)
    if epi.get("clip"):
        ref = ref.clamp(*epi["clip"])
    if r is not None:
        ref = ref + r.double()
    kw = dict(pads=pads, stride=stride, clip=epi.get("clip"), relu=bool(epi.get("relu")), split=split,
              want_f32=bool(epi.get("want_f32")), live=epi.get("live"), fill=FILL,
              residual=None if r is None else r.permute(0, 2, 3, 1).contiguous())
    xh = x.permute(0, 2, 3, 1).contiguous()
    t, tf = K.depthwise_conv_poly(xh, w, b, **kw)
    o, of = K.depthwise_conv(xh, w, b, tiled=False, **kw)
    torch.cuda.synchronize()
    vals = (K.join_planes(t) if split else t.float()).permute(0, 3, 1, 2).double()
    return t, o, tf, of, vals, ref


@pytest.mark.parametrize("k,stride", CLASSES)
@pytest.mark.parametrize("split", [False, True])
def test_poly_equals_gconv_and_torch(native, k, stride, split):
    n = 0
    for i, ((H, W), C, pads) in enumerate(itertools.product(MAPS, CHANNELS, _pads(k))):
        epi = EPILOGUES[i % len(EPILOGUES)]
        out = _case(k, stride, H, W, C, pads, epi, split, seed=1000 * k + 100 * stride + i)
        if out is None:
            continue
        _check(out, split, (k, stride, H, W, C, pads, epi))
        n += 1
    # left out: windows that do not fit the padded map, 3 of the 24 (map, pads) pairs at k = 3 (1x1 and 2x2 without
    # pads, 1x1 with SAME pads) and 6 at k = 5 (1x1 and 2x2 with anything but the symmetric pads), times 3 widths
    assert n == {3: 63, 5: 54}[k], n


@pytest.mark.parametrize("k,stride", CLASSES)
@pytest.mark.parametrize("split", [False, True])
@pytest.mark.parametrize("shape", [(17, 33, 40, (2, 1, 0, 2)), (14, 14, 24, (0, 0, 1, 1)), (5, 7, 8, None)])
def test_every_epilogue(native, k, stride, split, shape):
    H, W, C, pads = shape
    pads = pads or (k // 2,) * 4
    for j, epi in enumerate(EPILOGUES):
        out = _case(k, stride, H, W, C, pads, epi, split, seed=77 * k + 7 * stride + j)
        _check(out, split, (k, stride, H, W, C, pads, epi))


def test_out_of_scope_is_invalid_value(native):
    """window / stride classes outside the scope, dilation, a rectangular window, grouping and a channel count that
    is no multiple of 8: hipErrorInvalidValue (1) from the launcher's own check, before any launch"""
    import torch

    from die_amd import native as nat
    from die_amd.ops import kernels as K

    x = torch.randn(1, 12, 12, 16, device="cuda")

    def w(c, k):
        return torch.randn(c, 1, k, k, device="cuda")

    bad = [dict(w=w(16, 5), stride=1), dict(w=w(16, 7), stride=2), dict(w=w(16, 3), dilation=2),
           dict(w=torch.randn(16, 1, 3, 5, device="cuda")), dict(w=w(16, 3), groups=8),
           dict(w=w(12, 3), x=torch.randn(1, 12, 12, 12, device="cuda"))]
    for case in bad:
        kw = dict(case)
        xx = kw.pop("x", x)
        with pytest.raises(nat.NativeError, match=r"hipError 1\b"):
            K.depthwise_conv_poly(xx, kw.pop("w"), None, pads=(3, 3, 3, 3), **kw)
    torch.cuda.synchronize()
    # and a call inside the scope goes through
    out, _ = K.depthwise_conv_poly(x, w(16, 3), None, pads=(1, 1, 1, 1), stride=2)
    torch.cuda.synchronize()
    assert out.shape == (1, 6, 6, 16) and bool(torch.isfinite(out.float()).all())
