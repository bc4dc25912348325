"""Geometry grid and element-wise error bound for the implicit-GEMM conv kernels (a plain helper
module: test_conv_geometry_bound.py runs it on the CPU, test_gpu_conv_geometry.py on the kernels).

The cases are rectangular images and kernels, pads that differ per side, dilation and stride -- the
geometries where swapping H / W, pad_h / pad_w, KH / KW or ignoring `dil` changes the result.  Every
output element is compared with a float64 reference under a tolerance T = eps * S, S being the same
conv on |x|, |w|, |bias| (the sum of the magnitudes of everything added into that element):

  bf16 mode, operands already rounded to bf16, f32 output: the products are exact in fp32, so only the
  fp32 accumulation of K + splits + 2 terms rounds; in any order that is at most (K + splits + 2) *
  2^-24 * S (Higham, Accuracy and Stability of Numerical Algorithms, section 4.2).  eps takes twice
  that, because the MFMA's internal accumulation is not known to round to nearest (the factor 2 is a
  supposition, not a measurement).
  fp32 mode: the operands are rounded to what the hi / lo planes hold; the kernel drops the lo * lo
  products, |lo| <= 2^-8 |v|, which adds 2^-16.
  A stored output adds the storage rounding of the reference value: 2^-8 |ref| for bf16, 2^-16 |ref|
  for the split planes.

One missing product is about S / K, i.e. 1/1600 to 1/60 of S at these sizes, while eps <= 2e-4.
"""
import functools

import torch
import torch.nn.functional as F

# (B, H, W, Cin, Cout, KH, KW, stride, (top, left, bottom, right), dil)
CASES = [
    (2, 9, 13, 64, 64, 3, 3, 1, (1, 1, 1, 1), 1),    # 3x3/s1/p1, non-square: variants 6 / 9, ragged 8x8 tiles per axis
    (2, 10, 12, 64, 64, 1, 7, 1, (0, 3, 0, 3), 1),   # 1x7, pad_h != pad_w
    (2, 10, 12, 64, 40, 7, 1, 1, (3, 0, 3, 0), 1),   # 7x1, ragged N
    (2, 11, 9, 64, 64, 3, 3, 1, (2, 2, 2, 2), 2),    # dilated 3x3 with H == Ho: only dil keeps variants 6 / 9 away
    (3, 9, 7, 24, 40, 3, 3, 1, (2, 2, 2, 2), 2),     # dilation on the register path, ragged K (216) and N
    (2, 12, 10, 64, 64, 3, 3, 2, (0, 0, 1, 1), 1),   # TF "SAME" stride 2: begin pad != end pad
    (2, 11, 8, 128, 64, 3, 3, 2, (2, 1, 0, 1), 2),   # stride, dilation, four different pads; two K-steps per tap
    (2, 9, 11, 64, 64, 5, 5, 1, (2, 2, 2, 2), 1),    # 25 taps
    (3, 7, 9, 64, 64, 1, 1, 1, (1, 1, 1, 1), 1),     # padded 1x1: not dense, one tap
    (3, 7, 9, 64, 64, 1, 1, 2, (0, 0, 0, 0), 1),     # strided 1x1, odd non-square
    (2, 8, 12, 32, 64, 2, 2, 2, (0, 0, 0, 0), 1),    # patchify, non-square
    (2, 9, 13, 16, 12, 4, 4, 4, (0, 0, 0, 0), 1),    # patchify with rows / columns left over, N % 8 != 0
    (2, 9, 11, 4, 64, 3, 5, 1, (1, 2, 1, 2), 1),     # 4-wide loads, rectangular kernel, K = 60
]


def case_id(case):
    B, H, W, Cin, Cout, KH, KW, s, pads, d = case
    return "b%d_%dx%d_c%d_n%d_k%dx%d_s%d_p%d%d%d%d_d%d" % ((B, H, W, Cin, Cout, KH, KW, s) + tuple(pads) + (d,))


def out_hw(case):
    B, H, W, Cin, Cout, KH, KW, s, (t, l, b, r), d = case
    return (H + t + b - d * (KH - 1) - 1) // s + 1, (W + l + r - d * (KW - 1) - 1) // s + 1


def preround(v, split):
    """What the kernel's storage holds of v, as float64: bf16, or hi + lo of the split planes."""
    if not split:
        return v.float().to(torch.bfloat16).double()
    from die_amd.ops import kernels as K

    return K.join_planes(K.split_planes(v.float())).double()


def reference(x, w, bias, case):
    """float64 conv of x [B, Cin, H, W] with w [Cout, Cin, KH, KW] -> NHWC [B, Ho, Wo, Cout]."""
    s, (t, l, b, r), d = case[7], case[8], case[9]
    y = F.conv2d(F.pad(x.double(), (l, r, t, b)), w.double(), None if bias is None else bias.double(), stride=s,
                 dilation=d)
    return y.permute(0, 2, 3, 1).contiguous()


def abs_reference(x, w, bias, case):
    """S: the same conv on the magnitudes."""
    return reference(x.abs(), w.abs(), None if bias is None else bias.abs(), case)


def bound(case, splits=1, split=False, extra=0):
    """eps of T = eps * S: twice the worst-case fp32 accumulation of K + splits + 2 (+ extra: further
    terms an epilogue adds) terms, plus the dropped lo * lo products in fp32 mode."""
    K = case[5] * case[6] * case[3]
    eps = 2.0 * (K + splits + 2 + extra) * 2.0 ** -24
    if split:
        eps += 2.0 ** -16
    return eps


def storage(ref, split):
    """Storage rounding of a stored (not f32) output around the reference value."""
    return (2.0 ** -16 if split else 2.0 ** -8) * ref.abs()


def check(got, ref, T, what=""):
    """Assert |got - ref| <= T for every element of the NHWC tensors; returns the largest |err| / T."""
    got = got.double()
    assert got.shape == ref.shape, (what, tuple(got.shape), tuple(ref.shape))
    err = (got - ref).abs()
    bad = ~(err <= T)  # NaN fails
    ratio = torch.where(T > 0, err / T.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, float("inf")),
                                                                      torch.zeros_like(err)))
    ratio = torch.nan_to_num(ratio, nan=float("inf"))
    if bool(bad.any()):
        flat = int(ratio.flatten().argmax())
        idx = []
        for n in reversed(ref.shape):
            idx.append(flat % n)
            flat //= n
        idx = tuple(reversed(idx))
        raise AssertionError("%s: %d of %d elements outside the bound; worst (b, oh, ow, n) = %s: got %r, ref %r, "
                             "|err| %.3e, T %.3e" % (what, int(bad.sum()), bad.numel(), idx, float(got[idx]),
                                                     float(ref[idx]), float(err[idx]), float(T[idx])))
    return float(ratio.max())


@functools.lru_cache(maxsize=None)
def problem(case, split):
    """The case's operands (CPU, float64 values the kernel's storage holds exactly), its references and
    S, computed once and shared; callers must not modify them.
    x [B, Cin, H, W], w [Cout, Cin, KH, KW], res [B, Ho, Wo, Cout] rounded to the storage format; bias,
    scale2, shift2 fp32 values."""
    B, H, W, Cin, Cout, KH, KW, s, pads, d = case
    g = torch.Generator().manual_seed(1000 + CASES.index(case))
    Ho, Wo = out_hw(case)
    x = preround(torch.randn(B, Cin, H, W, generator=g), split)
    w = preround(torch.randn(Cout, Cin, KH, KW, generator=g) / (Cin * KH * KW) ** 0.5, split)
    bias = torch.randn(Cout, generator=g).double()
    res = preround(torch.randn(B, Ho, Wo, Cout, generator=g), split)
    scale2 = (torch.rand(Cout, generator=g) + 0.5).float().double()
    shift2 = torch.randn(Cout, generator=g).float().double()
    bias = bias.float().double()
    ref = reference(x, w, bias, case)
    S = abs_reference(x, w, bias, case)
    # epilogue pass: v = relu(conv + bias + res), u = relu(v * scale2 + shift2)
    v = torch.relu(ref + res)
    Sv = S + res.abs()
    u = torch.relu(v * scale2 + shift2)
    Su = Sv * scale2.abs() + shift2.abs()
    return dict(x=x, w=w, bias=bias, res=res, scale2=scale2, shift2=shift2, ref=ref, S=S, v=v, Sv=Sv, u=u, Su=Su)


# ---- a model of what the kernel computes from its geometry fields, for the mutation test ----------

def kernel_model(x, w, bias, case, pad_h=None, pad_w=None, dil=None):
    """float64 result of a kernel that offsets by (pad_h, pad_w), steps taps by `dil`, reads pixels
    outside the image as zero and writes the case's Ho x Wo outputs -- equal to reference() for the
    case's own fields, and what a kernel with a wrong field would give otherwise."""
    B, H, W, Cin, Cout, KH, KW, s, (t, l, b, r), d = case
    pad_h = t if pad_h is None else pad_h
    pad_w = l if pad_w is None else pad_w
    dil = d if dil is None else dil
    Ho, Wo = out_hw(case)
    bot = max(0, (Ho - 1) * s - pad_h + dil * (KH - 1) + 1 - H)
    right = max(0, (Wo - 1) * s - pad_w + dil * (KW - 1) + 1 - W)
    y = F.conv2d(F.pad(x.double(), (pad_w, right, pad_h, bot)), w.double(), bias.double(), stride=s, dilation=dil)
    return y[:, :, :Ho, :Wo].permute(0, 2, 3, 1).contiguous()


def mutants(x, w, bias, case):
    """name -> the result of a subtly wrong kernel (some are no-ops for a case: compare with the reference)."""
    B, H, W, Cin, Cout, KH, KW, s, (t, l, b, r), d = case
    out = {}
    out["flipx"] = kernel_model(x, w.flip(3), bias, case)
    out["flipy"] = kernel_model(x, w.flip(2), bias, case)
    # (ky, kx) order of the weight packing: k = kx * KH + ky read as ky * KW + kx
    out["tap_order"] = kernel_model(x, w.transpose(2, 3).contiguous().reshape(w.shape), bias, case)
    out["swap_pads"] = kernel_model(x, w, bias, case, pad_h=l, pad_w=t)
    out["end_as_begin"] = kernel_model(x, w, bias, case, pad_h=b, pad_w=r)
    out["pad_w_plus_1"] = kernel_model(x, w, bias, case, pad_w=l + 1)
    out["no_dil"] = kernel_model(x, w, bias, case, dil=1)
    w1 = w.clone()
    w1[Cout // 2, Cin // 2, KH // 2, KW // 2] = 0  # one product missing in the elements of one channel
    out["one_tap"] = kernel_model(x, w1, bias, case)
    xr = x.clone()
    xr[:, :, H - 1, :] = 0  # bounds test off by one: the last input row reads as padding
    out["last_row"] = kernel_model(xr, w, bias, case)
    xc = x.clone()
    xc[:, :, :, W - 1] = 0
    out["last_col"] = kernel_model(xc, w, bias, case)
    return out
