"""The float64 references of test_gpu_generic_kernels.py (generic_refs.py) against torch on the CPU,
wherever torch implements the same operator, so that a kernel and its reference cannot be wrong in
the same way.  Needs no GPU."""
import pytest
import torch
import torch.nn.functional as F

import generic_refs as G

PAIRS = [(G.RESIZE_SIZES[i], G.RESIZE_SIZES[(i + 1) % len(G.RESIZE_SIZES)]) for i in range(len(G.RESIZE_SIZES))]


def _image(B, H, W, C, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(B, H, W, C, generator=g, dtype=torch.float64)


def _nchw(x):
    return x.permute(0, 3, 1, 2)


@pytest.mark.parametrize("hs,ws", PAIRS)
def test_nearest_asymmetric_floor_is_torch_nearest(hs, ws):
    (H, Ho), (W, Wo) = hs, ws
    x = _image(2, H, W, 3, 1)
    ref = G.resize_nearest_ref(x, Ho, Wo, Ho / H, Wo / W, G.COORDS.index("asymmetric"), G.NEAREST.index("floor"))
    want = F.interpolate(_nchw(x), size=(Ho, Wo), mode="nearest").permute(0, 2, 3, 1)
    assert torch.equal(ref, want), (hs, ws)


@pytest.mark.parametrize("hs,ws", PAIRS)
def test_linear_align_corners_is_torch_bilinear(hs, ws):
    (H, Ho), (W, Wo) = hs, ws
    x = _image(2, H, W, 3, 2)
    ref = G.resize_linear_ref(x, Ho, Wo, Ho / H, Wo / W, G.COORDS.index("align_corners"))
    want = F.interpolate(_nchw(x), size=(Ho, Wo), mode="bilinear", align_corners=True).permute(0, 2, 3, 1)
    assert (ref - want).abs().max().item() < 1e-12, (hs, ws)


@pytest.mark.parametrize("hs,ws", [p for p in PAIRS if p[0][1] > 1 and p[1][1] > 1])
@pytest.mark.parametrize("coord", ["half_pixel", "pytorch_half_pixel"])
def test_linear_half_pixel_is_torch_bilinear(hs, ws, coord):
    (H, Ho), (W, Wo) = hs, ws
    x = _image(2, H, W, 3, 3)
    ref = G.resize_linear_ref(x, Ho, Wo, Ho / H, Wo / W, G.COORDS.index(coord))
    want = F.interpolate(_nchw(x), size=(Ho, Wo), mode="bilinear", align_corners=False).permute(0, 2, 3, 1)
    assert (ref - want).abs().max().item() < 1e-12, (hs, ws)


def test_output_of_one_pixel():
    # out == 1: half_pixel samples the centre, pytorch_half_pixel and align_corners pixel 0
    x = _image(1, 4, 4, 1, 4)
    hp = G.resize_linear_ref(x, 1, 1, 0.25, 0.25, G.COORDS.index("half_pixel"))
    assert torch.allclose(hp[0, 0, 0], x[0, 1:3, 1:3].mean(dim=(0, 1)), atol=1e-15)
    for name in ("pytorch_half_pixel", "align_corners"):
        assert torch.equal(G.resize_linear_ref(x, 1, 1, 0.25, 0.25, G.COORDS.index(name))[0, 0, 0], x[0, 0, 0])


def test_nearest_modes_on_exact_ties_and_between():
    src = torch.tensor([-0.5, -0.25, 0.0, 0.49, 0.5, 0.51, 1.5, 2.5, 3.0, 9.0], dtype=torch.float64)
    want = {"round_prefer_floor": [0, 0, 0, 0, 0, 1, 1, 2, 3, 4], "round_prefer_ceil": [0, 0, 0, 0, 1, 1, 2, 3, 3, 4],
            "floor": [0, 0, 0, 0, 0, 0, 1, 2, 3, 4], "ceil": [0, 0, 0, 1, 1, 1, 2, 3, 3, 4]}
    for k, name in enumerate(G.NEAREST):
        assert G.nearest_index(src, k, 5).tolist() == want[name], name


def test_float32_coordinates_pick_the_same_pixels():
    """The zero-exclusion condition of the GPU test: on every listed size pair the coordinates computed
    in float32 from the float32 scale (what the kernel does) and in float64 from the exact ratio
    out / in (the reference) select the same source index in every coordinate and nearest mode, so
    no output pixel needs to be left out of the comparison."""
    checked, gap = 0, 0.0
    for n_in, n_out in G.RESIZE_SIZES:
        for coord in range(len(G.COORDS)):
            s32 = G.resize_src(n_in, n_out, G.resize_scale(n_in, n_out), coord, torch.float32)
            s64 = G.resize_src(n_in, n_out, n_out / n_in, coord, torch.float64)
            gap = max(gap, (s32.double() - s64).abs().max().item())
            for nearest in range(len(G.NEAREST)):
                a, b = G.nearest_index(s32, nearest, n_in), G.nearest_index(s64, nearest, n_in)
                assert torch.equal(a, b), (n_in, n_out, G.COORDS[coord], G.NEAREST[nearest], a.tolist(), b.tolist())
                checked += n_out
    assert checked == 4 * 5 * sum(o for _, o in G.RESIZE_SIZES)
    assert gap < 1e-6, gap


def test_asymmetric_times_two_lands_on_ties():
    for n_in, n_out in ((5, 10), (7, 14)):
        s = G.resize_src(n_in, n_out, G.resize_scale(n_in, n_out), G.COORDS.index("asymmetric"))
        assert torch.equal(s[1::2] - torch.floor(s[1::2]), torch.full((n_out // 2,), 0.5, dtype=torch.float64))
        lo, hi = G.nearest_index(s, 0, n_in), G.nearest_index(s, 1, n_in)
        assert torch.equal(hi[1:-1:2], lo[1:-1:2] + 1)  # the last odd output clamps to the edge in both


@pytest.mark.parametrize("t,l,Ho,Wo", [(0, 0, 5, 8), (1, 2, 6, 9), (3, 0, 7, 5)])
def test_pad_is_torch_pad(t, l, Ho, Wo):
    x = _image(2, 3, 5, 4, 5)
    want = F.pad(_nchw(x), (l, Wo - 5 - l, t, Ho - 3 - t)).permute(0, 2, 3, 1)
    assert torch.equal(G.pad_insert_ref(x, Ho, Wo, t, l), want)


@pytest.mark.parametrize("sy,sx,p", [(1, 1, 0), (2, 2, 1), (2, 3, 0)])
def test_zero_insertion_turns_conv_transpose_into_a_conv(sy, sx, p):
    k = 3
    x = _image(2, 3, 5, 4, 6)
    g = torch.Generator().manual_seed(7)
    w = torch.randn(4, 6, k, k, generator=g, dtype=torch.float64)  # [Cin, Cout, k, k]
    want = F.conv_transpose2d(_nchw(x), w, stride=(sy, sx), padding=p)
    e = k - 1 - p
    z = G.pad_insert_ref(x, (3 - 1) * sy + 1 + 2 * e, (5 - 1) * sx + 1 + 2 * e, e, e, sy, sx)
    got = F.conv2d(_nchw(z), w.flip(2, 3).transpose(0, 1))
    assert (got - want).abs().max().item() < 1e-12


def test_generic_kernel_entries_resolve(native):
    """The C-ABI entries behind the wrappers of ops/kernels.py exist and have their signatures declared."""
    L = native.kernels()
    for name in ("rows_prep", "input_prep_wide", "copy_cols", "binary_rows", "unary_rows", "where_rows", "resize_nhwc",
                 "pad_nhwc", "rows_to_f32", "nhwc_to_nchw_strided", "bmm_rows", "pool2d", "gap"):
        fn = getattr(L, "die_kern_" + name)
        assert fn.argtypes, name
