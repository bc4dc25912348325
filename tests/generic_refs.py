"""Plain float64 references for the generic image kernels (csrc/kernels/generic.hip), written from the
ONNX operator definitions and shared by test_generic_refs.py (which checks them against torch on
the CPU) and test_gpu_generic_kernels.py (which checks the kernels against them).

Images are NHWC torch tensors on any device."""
import torch

COORDS = ("half_pixel", "asymmetric", "align_corners", "pytorch_half_pixel", "tf_half_pixel_for_nn")
NEAREST = ("round_prefer_floor", "round_prefer_ceil", "floor", "ceil")

# (input size, output size) of one axis; test cases take H from pair i and W from pair i + 1, so the
# two scales of a case differ
RESIZE_SIZES = ((5, 10), (7, 14), (8, 4), (12, 6), (7, 10), (5, 8), (9, 4), (6, 5), (4, 1), (1, 5), (3, 7), (16, 4),
                (6, 9))


def resize_scale(n_in, n_out):
    """The op's scale as the engine carries it: float32(out / in), returned as a Python float.  That
    is what a kernel gets; the float64 references take the exact ratio n_out / n_in."""
    return float(torch.tensor(n_out / n_in, dtype=torch.float64).to(torch.float32))


def resize_src(n_in, n_out, scale, coord, dtype=torch.float64, device="cpu"):
    """Source coordinate of every output index along one axis (ONNX Resize,
    coordinate_transformation_mode `coord` as an index into COORDS), with the arithmetic carried out
    in `dtype`: float64 for the reference, float32 for what a single-precision kernel computes."""
    o = torch.arange(n_out, dtype=dtype, device=device)
    s = torch.tensor(scale, dtype=dtype, device=device)
    half = torch.tensor(0.5, dtype=dtype, device=device)
    name = COORDS[coord]
    if name == "half_pixel":
        return (o + half) / s - half
    if name == "asymmetric":
        return o / s
    if name == "align_corners":
        if n_out == 1:
            return torch.zeros_like(o)
        return o * torch.tensor(n_in - 1, dtype=dtype, device=device) / torch.tensor(n_out - 1, dtype=dtype, device=device)
    if name == "pytorch_half_pixel":
        return (o + half) / s - half if n_out > 1 else torch.zeros_like(o)
    return (o + half) / s  # tf_half_pixel_for_nn


def nearest_index(src, nearest, n_in):
    """ONNX nearest_mode (index into NEAREST) of source coordinates, clamped to the axis."""
    x = src.to(torch.float64)
    name = NEAREST[nearest]
    if name == "round_prefer_floor":  # a tie x.5 goes down
        i = torch.ceil(x - 0.5)
    elif name == "round_prefer_ceil":  # a tie x.5 goes up
        i = torch.floor(x + 0.5)
    elif name == "floor":
        i = torch.floor(x)
    else:
        i = torch.ceil(x)
    return i.to(torch.int64).clamp(0, n_in - 1)


def resize_nearest_ref(x, Ho, Wo, scale_h, scale_w, coord, nearest, dtype=torch.float64):
    """Nearest Resize of [..., H, W, C]: a pure gather, any dtype of x (also raw bit planes)."""
    H, W = x.shape[-3], x.shape[-2]
    iy = nearest_index(resize_src(H, Ho, scale_h, coord, dtype, x.device), nearest, H)
    ix = nearest_index(resize_src(W, Wo, scale_w, coord, dtype, x.device), nearest, W)
    return x.index_select(-3, iy).index_select(-2, ix)


def _linear_taps(n_in, n_out, scale, coord, device):
    s = resize_src(n_in, n_out, scale, coord, torch.float64, device)
    f = torch.floor(s)
    i0 = f.to(torch.int64)
    return i0.clamp(0, n_in - 1), (i0 + 1).clamp(0, n_in - 1), s - f


def resize_linear_ref(x, Ho, Wo, scale_h, scale_w, coord):
    """Bilinear Resize of float64 [B, H, W, C]; neighbours outside the image take the edge pixel."""
    x = x.to(torch.float64)
    H, W = x.shape[1], x.shape[2]
    y0, y1, ay = _linear_taps(H, Ho, scale_h, coord, x.device)
    x0, x1, ax = _linear_taps(W, Wo, scale_w, coord, x.device)
    ax = ax.view(1, 1, Wo, 1)
    ay = ay.view(1, Ho, 1, 1)
    r0, r1 = x.index_select(1, y0), x.index_select(1, y1)
    top = r0.index_select(2, x0) * (1 - ax) + r0.index_select(2, x1) * ax
    bot = r1.index_select(2, x0) * (1 - ax) + r1.index_select(2, x1) * ax
    return top * (1 - ay) + bot * ay


def pad_insert_ref(x, Ho, Wo, t, l, sy=1, sx=1):
    """Zeros [..., Ho, Wo, C] with the pixels of x [..., H, W, C] at (t + sy * h, l + sx * w): ONNX Pad
    (constant 0) for sy = sx = 1, and the zero insertion of a ConvTranspose for larger strides."""
    H, W = x.shape[-3], x.shape[-2]
    y = torch.zeros(x.shape[:-3] + (Ho, Wo, x.shape[-1]), dtype=x.dtype, device=x.device)
    y[..., t:t + (H - 1) * sy + 1:sy, l:l + (W - 1) * sx + 1:sx, :] = x
    return y
