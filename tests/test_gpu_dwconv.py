"""The tiled depthwise conv kernel (csrc/kernels/dwconv.hip) through ops.kernels.depthwise_conv: bit for
bit the output of gconv_kernel on the same inputs (same tap order, same fp32 expression, a zero halo
adds exact zeros), and the bars of the grouped-conv kernel test (tests/test_gpu_op_coverage.py) against a
float64 torch conv2d.  Shapes: maps smaller than a tile, exactly one tile wide / high, partial tiles on
both edges, both tile widths (maps up to 8 wide take the narrow one); channel counts with a partial
32-channel slice and widths 32 / 64 do not divide; symmetric, zero and asymmetric pads."""
import itertools

import pytest

from conftest import gpu_available

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not gpu_available(), reason="needs a GPU")]

MAPS = [(1, 1), (2, 2), (5, 7), (7, 7), (14, 14), (17, 9)]
CHANNELS = [8, 24, 96, 136]
PADS = [(3, 3, 3, 3), (0, 0, 0, 0), (2, 4, 3, 1)]  # top, left, bottom, right
B = 3
# epilogues of GConvArgs; every (shape, pads) case takes one in turn, test_every_epilogue takes them all
EPILOGUES = [dict(bias=True), dict(bias=False), dict(bias=True, relu=True), dict(bias=True, clip=(-0.5, 0.75)),
             dict(bias=True, residual=True), dict(bias=True, relu=True, residual=True, want_f32=True),
             dict(bias=False, want_f32=True), dict(bias=True, live=2, want_f32=True)]
FILL = -7.0  # sentinel in the output buffers (exact in bf16)


def _case(k, H, W, C, pads, epi, split, seed):
    """Runs both kernels and the float64 reference; returns (tiled planes, gconv planes, tiled f32, gconv f32,
    stored values as float64 NCHW, reference) or None when the window does not fit the padded map."""
    import torch

    from die_amd.ops import kernels as K

    Ho, Wo = H + pads[0] + pads[2] - k + 1, W + pads[1] + pads[3] - k + 1
    if Ho < 1 or Wo < 1:
        return None
    g = torch.Generator(device="cuda").manual_seed(seed)
    x = torch.randn(B, C, H, W, device="cuda", generator=g)
    w = torch.randn(C, 1, k, k, device="cuda", generator=g) * 0.3
    b = torch.randn(C, device="cuda", generator=g) if epi.get("bias") else None
    r = torch.randn(B, C, Ho, Wo, device="cuda", generator=g) if epi.get("residual") else None
    ref = torch.nn.functional.conv2d(torch.nn.functional.pad(x.double(), (pads[1], pads[3], pads[0], pads[2])), w.double(),
                                     None if b is None else b.double(), groups=C)
    if epi.get("relu"):
        ref = ref.clamp(min=0)
    if epi.get("clip"):
        ref = ref.clamp(*epi["clip"])
    if r is not None:
        ref = ref + r.double()
    kw = dict(pads=pads, clip=epi.get("clip"), relu=bool(epi.get("relu")), split=split, want_f32=bool(epi.get("want_f32")),
              live=epi.get("live"), fill=FILL, residual=None if r is None else r.permute(0, 2, 3, 1).contiguous())
    xh = x.permute(0, 2, 3, 1).contiguous()
    t, tf = K.depthwise_conv(xh, w, b, tiled=True, **kw)
    o, of = K.depthwise_conv(xh, w, b, tiled=False, **kw)
    torch.cuda.synchronize()
    vals = (K.join_planes(t) if split else t.float()).permute(0, 3, 1, 2).double()
    return t, o, tf, of, vals, ref


def _check(out, split, what):
    import torch

    t, o, tf, of, vals, ref = out
    live = what[-1].get("live", B)
    assert torch.equal(t.view(torch.int16), o.view(torch.int16)), ("tiled != gconv", what)
    if tf is not None:
        assert torch.equal(tf.view(torch.int32), of.view(torch.int32)), ("tiled f32 != gconv f32", what)
        ferr = float((tf[:live].permute(0, 3, 1, 2).double() - ref[:live]).norm() / ref[:live].norm().clamp(min=1e-30))
        assert ferr < (2e-5 if split else 1e-2), (ferr, what)
    err = float((vals[:live] - ref[:live]).norm() / ref[:live].norm().clamp(min=1e-30))
    assert err < (2e-5 if split else 1e-2), (err, what)
    if live < B:  # samples past the live count keep the sentinel, in every plane and in the f32 output
        assert bool((t[..., live:, :, :, :] == FILL).all()) and bool((tf[live:] == FILL).all()), what
        assert bool((t[..., :live, :, :, :] != FILL).any())


@pytest.mark.parametrize("k", [5, 7])
@pytest.mark.parametrize("split", [False, True])
def test_tiled_equals_gconv_and_torch(native, k, split):
    n = 0
    for i, ((H, W), C, pads) in enumerate(itertools.product(MAPS, CHANNELS, PADS)):
        epi = EPILOGUES[i % len(EPILOGUES)]
        out = _case(k, H, W, C, pads, epi, split, seed=1000 * k + i)
        if out is None:
            continue
        _check(out, split, (k, H, W, C, pads, epi))
        n += 1
    # left out: windows that do not fit the padded map (zero pads on the small maps, 7x7 on 1x1 with pads 2 + 3)
    assert n == {5: 64, 7: 56}[k], n


@pytest.mark.parametrize("k", [5, 7])
@pytest.mark.parametrize("split", [False, True])
@pytest.mark.parametrize("shape", [(17, 9, 136, (2, 4, 3, 1)), (14, 14, 96, (3, 3, 3, 3)), (2, 2, 24, (3, 3, 3, 3))])
def test_every_epilogue(native, k, split, shape):
    H, W, C, pads = shape
    for j, epi in enumerate(EPILOGUES):
        out = _case(k, H, W, C, pads, epi, split, seed=77 * k + j)
        _check(out, split, (k, H, W, C, pads, epi))


def test_out_of_scope_is_invalid_value(native):
    """stride, dilation, window size, channel count and grouping outside the scope: hipErrorInvalidValue (1)
    from the launcher's own check, before any launch"""
    import torch

    from die_amd import native as nat
    from die_amd.ops import kernels as K

    x = torch.randn(1, 8, 8, 16, device="cuda")

    def w(c, k):
        return torch.randn(c, 1, k, k, device="cuda")

    bad = [dict(w=w(16, 7), stride=2), dict(w=w(16, 7), dilation=2), dict(w=w(16, 3)), dict(w=w(16, 6)), dict(w=w(16, 9)),
           dict(w=torch.randn(16, 1, 5, 7, device="cuda")), dict(w=w(16, 7), groups=8),
           dict(w=w(12, 7), x=torch.randn(1, 8, 8, 12, device="cuda"))]
    for case in bad:
        kw = dict(case)
        xx = kw.pop("x", x)
        with pytest.raises(nat.NativeError, match=r"hipError 1\b"):
            K.depthwise_conv(xx, kw.pop("w"), None, pads=(4, 4, 4, 4), **kw)
    torch.cuda.synchronize()
    # and the same call inside the scope goes through
    out, _ = K.depthwise_conv(x, w(16, 7), None, pads=(3, 3, 3, 3))
    torch.cuda.synchronize()
    assert out.shape == (1, 8, 8, 16) and bool(torch.isfinite(out.float()).all())
