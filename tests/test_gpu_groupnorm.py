"""The GroupNorm / InstanceNorm kernel (csrc/kernels/groupnorm.hip) through ops.kernels.group_norm, against
torch's group_norm in float64 on the STORED input values with the activation applied in float64; the bars
are those of the depthwise test (tests/test_gpu_dwconv.py): rel-L2 < 2e-5 split, < 1e-2 bf16.  Every case
runs B = 3 samples into a sentinel-filled output, with large finite values in the stored pad channels of
the input (they must reach neither the statistics nor the output).  Shapes: maps from 1x1 (one block, one
pixel) to 64x64 (64 statistics blocks per sample to merge); groups of 8, 1, 6, 12, 5, 3 and 10 channels (a
16-byte chunk of 8 channels straddles groups in most of them), a single group, InstanceNorm, and logical
channels below the stored ones."""
import itertools

import pytest

from conftest import gpu_available

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not gpu_available(), reason="needs a GPU")]

B = 3
MAPS = [(1, 1), (2, 2), (5, 7), (17, 9)]
SHAPES = [(8, 8, 1), (8, 8, 8), (24, 24, 3), (24, 24, 4), (24, 24, 2), (20, 24, 4), (20, 24, 20), (96, 96, 32),
          (320, 320, 32)]  # (Cl, C, G)
BIG = ((64, 64), (64, 64, 32), 2)  # map, shape, batch
# (gamma, beta, act, eps): every case takes one in turn
PARAMS = [(True, True, None, 1e-5), (True, False, "relu", 1e-3), (False, False, "silu", 1e-5), (True, True, "silu", 1e-3),
          (True, True, "relu", 1e-5), (False, False, None, 1e-3)]
FILL = -7.0  # sentinel in the output buffer (exact in bf16)
PAD = 1.0e4  # in the stored pad channels of the input


def _inputs(H, W, shape, batch, seed, mean=0.0):
    import torch

    Cl, C, G = shape
    g = torch.Generator(device="cuda").manual_seed(seed)
    x = torch.randn(batch, H, W, C, device="cuda", generator=g) * 1.5 + 0.3 + mean
    x[..., Cl:] = PAD
    gamma = torch.rand(Cl, device="cuda", generator=g) + 0.5
    beta = torch.randn(Cl, device="cuda", generator=g)
    return x, gamma, beta


def _stored(x, split):
    import torch

    from die_amd.ops import kernels as K

    return K.join_planes(K.split_planes(x)) if split else x.to(torch.bfloat16).float()


def _reference(x, shape, gamma, beta, act, eps, split):
    import torch

    Cl, C, G = shape
    xs = _stored(x, split)[..., :Cl].permute(0, 3, 1, 2).double()
    ref = torch.nn.functional.group_norm(xs, G, None if gamma is None else gamma.double(),
                                         None if beta is None else beta.double(), eps)
    if act == "relu":
        ref = ref.clamp(min=0)
    if act == "silu":
        ref = ref * torch.sigmoid(ref)
    return ref  # [B, Cl, H, W]


def _run(x, shape, gamma, beta, act, eps, split, **kw):
    import torch

    from die_amd.ops import kernels as K

    Cl, C, G = shape
    out = K.group_norm(x, G, gamma, beta, eps, act=act, split=split, fill=FILL, Cl=Cl, **kw)
    torch.cuda.synchronize()
    return out


def _values(out, split):
    from die_amd.ops import kernels as K

    return (K.join_planes(out) if split else out.float()).double()  # [B, H, W, C]


def _err(out, ref, shape, split, live=None):
    """rel-L2 of the logical channels of the first `live` samples; an all-zero reference must be met exactly"""
    Cl = shape[0]
    vals = _values(out, split)[..., :Cl].permute(0, 3, 1, 2)[:live]
    ref = ref[:live]
    if float(ref.norm()) == 0.0:
        return 0.0 if bool((vals == 0).all()) else float("inf")
    return float((vals - ref).norm() / ref.norm())


def _check(out, ref, shape, split, what, live=None):
    import torch

    Cl, C, G = shape
    assert bool(torch.isfinite(out.float()).all()), what
    err = _err(out, ref, shape, split, live)
    print(what, "rel-L2 %.3g" % err)
    assert err < (2e-5 if split else 1e-2), (err, what)
    if Cl < C:  # pad channels: exactly 0 in every plane
        assert bool((out[..., :live, :, :, Cl:] == 0).all()), what


@pytest.mark.parametrize("split", [False, True])
def test_against_torch_float64(native, split):
    import torch

    n = 0
    cases = [(m, s, B) for m, s in itertools.product(MAPS, SHAPES)] + [BIG]
    for i, ((H, W), shape, batch) in enumerate(cases):
        hg, hb, act, eps = PARAMS[i % len(PARAMS)]
        x, gamma, beta = _inputs(H, W, shape, batch, seed=100 + i)
        gamma, beta = gamma if hg else None, beta if hb else None
        out = _run(x, shape, gamma, beta, act, eps, split)
        ref = _reference(x, shape, gamma, beta, act, eps, split)
        what = (H, W, shape, batch, hg, hb, act, eps, split)
        _check(out, ref, shape, split, what)
        assert bool((out != FILL).all()) or act is None, what  # every element was written
        n += 1
    assert n == len(MAPS) * len(SHAPES) + 1 == 37, n


@pytest.mark.parametrize("split", [False, True])
@pytest.mark.parametrize("shape", [(8, 8, 8), (20, 24, 20)])
def test_one_pixel_instance_norm_is_act_of_beta(native, split, shape):
    """1x1 map, a group per channel: the variance is exactly 0 and x - mean is exactly 0, so the output is
    act(beta) as stored -- finite, and exactly 0 without a beta"""
    import torch

    Cl = shape[0]
    for act, eps in itertools.product([None, "relu", "silu"], [1e-5, 1e-3]):
        x, gamma, beta = _inputs(1, 1, shape, B, seed=7)
        out = _run(x, shape, gamma, beta, act, eps, split)
        want = beta.double()
        want = want.clamp(min=0) if act == "relu" else want * torch.sigmoid(want) if act == "silu" else want
        ref = want.view(1, Cl, 1, 1).expand(B, Cl, 1, 1)
        _check(out, ref, shape, split, ("1x1", shape, act, eps, split))
        out = _run(x, shape, gamma, None, act, eps, split)
        assert bool((out == 0).all()), (shape, act, eps, split)


@pytest.mark.parametrize("split", [False, True])
@pytest.mark.parametrize("act", [None, "relu", "silu"])
@pytest.mark.parametrize("params", ["both", "gamma", "neither"])
def test_parameters_and_activations(native, split, act, params):
    H, W, shape = 5, 7, (20, 24, 4)
    for eps in (1e-5, 1e-3):
        x, gamma, beta = _inputs(H, W, shape, B, seed=31)
        gamma, beta = (None if params == "neither" else gamma), (beta if params == "both" else None)
        out = _run(x, shape, gamma, beta, act, eps, split)
        _check(out, _reference(x, shape, gamma, beta, act, eps, split), shape, split, (params, act, eps, split))


@pytest.mark.parametrize("split", [False, True])
@pytest.mark.parametrize("case", [((5, 7), (24, 24, 4), B), ((17, 9), (20, 24, 4), B), BIG])
def test_live_batch_invariance_repeatability(native, split, case):
    import torch

    (H, W), shape, batch = case
    x, gamma, beta = _inputs(H, W, shape, batch, seed=55)
    full = _run(x, shape, gamma, beta, "silu", 1e-5, split)
    again = _run(x, shape, gamma, beta, "silu", 1e-5, split)
    assert torch.equal(full.view(torch.int16), again.view(torch.int16)), "two runs differ"
    live = batch - 1
    part = _run(x, shape, gamma, beta, "silu", 1e-5, split, live=live)
    # samples past the live count keep the sentinel in every plane; the others have the bits of the full run
    assert bool((part[..., live:, :, :, :] == FILL).all())
    assert torch.equal(part[..., :live, :, :, :].contiguous().view(torch.int16),
                       full[..., :live, :, :, :].contiguous().view(torch.int16))
    # sample 1 alone (B = 1) has the bits of its slice of the batch
    alone = _run(x[1:2].contiguous(), shape, gamma, beta, "silu", 1e-5, split)
    assert torch.equal(alone.view(torch.int16), full[..., 1:2, :, :, :].contiguous().view(torch.int16))


@pytest.mark.parametrize("split", [False, True])
@pytest.mark.parametrize("case", [((5, 7), (24, 24, 4), B), BIG])
def test_large_mean(native, split, case):
    """x = 100 + randn: a sum-of-squares variance (E[x^2] - mean^2 in fp32) loses the variance's digits here;
    the (count, mean, M2) statistics stay inside the same bars"""
    import torch

    (H, W), shape, batch = case
    Cl, C, G = shape
    g = torch.Generator(device="cuda").manual_seed(77)
    x = 100.0 + torch.randn(batch, H, W, C, device="cuda", generator=g)
    gamma = torch.rand(Cl, device="cuda", generator=g) + 0.5
    beta = torch.randn(Cl, device="cuda", generator=g)
    out = _run(x, shape, gamma, beta, None, 1e-5, split)
    _check(out, _reference(x, shape, gamma, beta, None, 1e-5, split), shape, split, ("large mean", case, split))


def test_bad_arguments_are_invalid_value(native):
    """Cl % G != 0, C % 8 != 0 and a too-small workspace: hipErrorInvalidValue (1) from the launcher's own
    check, nothing launched -- the output keeps the sentinel"""
    import torch

    from die_amd import native as nat
    from die_amd.ops import kernels as K

    def attempt(x, G, **kw):
        out = torch.empty(x.shape, dtype=torch.bfloat16, device="cuda")
        with pytest.raises(nat.NativeError, match=r"hipError 1\b"):
            K.group_norm(x, G, fill=FILL, out=out, **kw)
        torch.cuda.synchronize()
        assert bool((out == FILL).all())

    x = torch.randn(2, 4, 4, 24, device="cuda")
    attempt(x, 5)                                   # 24 % 5
    attempt(x, 3, Cl=20)                            # 20 % 3
    attempt(torch.randn(2, 4, 4, 12, device="cuda"), 4)  # C % 8
    need = nat.kernels().die_groupnorm_workspace_bytes(2, 16, 24, 4)
    assert need > 0
    attempt(x, 4, ws_bytes=need - 8)                # a workspace one float2 short
    attempt(x, 4, ws_bytes=0)
    out = K.group_norm(x, 4, fill=FILL)             # and the same call with good arguments goes through
    torch.cuda.synchronize()
    assert bool((out != FILL).all()) and bool(torch.isfinite(out.float()).all())
