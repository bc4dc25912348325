"""The squeeze-excitation kernels (csrc/kernels/se.hip) through ops.kernels.se_block, against the ONNX expression
in float64 on the STORED input values:
    gate = act2(W2 act1(W1 mean_hw(x) + b1) + b2),  y = x * gate
Bars: those of tests/test_gpu_grn.py for y (rel-L2 < 2e-5 split, < 1e-2 bf16, on the whole output and per
channel) and 2e-5 for the f32 gate in both modes (fp32 arithmetic on stored values in both).  Every case runs
B = 3 samples into sentinel-filled outputs.  Channels: one 16-byte chunk (8), a partial wave (24), 33 chunks that
do not divide the 256 threads (264), more chunks than threads (2056: two column tiles); hidden widths from fewer
rows than waves (1) to many per wave (240); one 56x56 map with the slice count forced to 1 and to > 1."""
import itertools

import pytest

from conftest import gpu_available

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not gpu_available(), reason="needs a GPU")]

B = 3
MAPS = [(1, 1), (3, 5), (7, 7), (14, 14)]
CHANNELS = [8, 24, 264, 2056]
HIDDEN = [1, 4, 10, 240]
ACTS = [("silu", "sigmoid"), ("relu", "hardsigmoid"), ("hardswish", "hardsigmoid")]  # B0, MobileNetV3, and a spare
FILL = -(2.0 ** 100)  # exact in bf16 and f32, far from every value a case can produce


def _inputs(H, W, C, Cr, seed, batch=B):
    import torch

    g = torch.Generator(device="cuda").manual_seed(seed)
    r = lambda *s: torch.randn(*s, device="cuda", generator=g)
    return (r(batch, H, W, C) * 1.5 + 0.3, r(Cr, C) / C ** 0.5, r(Cr) * 0.5, r(C, Cr) / Cr ** 0.5, r(C) * 0.5)


def _stored(x, split):
    import torch

    from die_amd.ops import kernels as K

    return K.join_planes(K.split_planes(x)) if split else x.to(torch.bfloat16).float()


def _reference(x, w1, b1, w2, b2, act1, act2, split, alpha=1.0 / 6.0, beta=0.5):
    """(y [B, H, W, C], gate [B, C]) in float64 on the stored x"""
    import torch
    import torch.nn.functional as F

    xs = _stored(x, split).double()
    h = xs.mean(dim=(1, 2)) @ w1.double().t() + b1.double()
    h = {"relu": F.relu, "silu": F.silu, "hardswish": F.hardswish}[act1](h)
    z = h @ w2.double().t() + b2.double()
    gate = torch.sigmoid(z) if act2 == "sigmoid" else (alpha * z + beta).clamp(0, 1)
    return xs * gate[:, None, None, :], gate


def _rel(d, r):
    if float(r.norm()) == 0.0:
        return 0.0 if float(d.norm()) == 0.0 else float("inf")
    return float(d.norm() / r.norm())


def _check(out, gate, ref, split, what):
    import torch

    from die_amd.ops import kernels as K

    vals = (K.join_planes(out) if split else out.float()).double()
    bar = 2e-5 if split else 1e-2
    err, gerr = _rel(vals - ref[0], ref[0]), _rel(gate.double() - ref[1], ref[1])
    d, r = (vals - ref[0]).flatten(0, 2).norm(dim=0), ref[0].flatten(0, 2).norm(dim=0)
    worst = float(torch.where(r > 0, d / r.clamp(min=1e-300), (d > 0).double() * float("inf")).nan_to_num(0.0, posinf=float("inf")).max())
    print(what, "y rel-L2 %.3g, worst channel %.3g, gate %.3g" % (err, worst, gerr))
    assert bool(torch.isfinite(out.float()).all()) and bool((out != FILL).all()) and bool((gate != FILL).all()), what
    assert err < bar and worst < bar and gerr < 2e-5, (err, worst, gerr, what)


def _run(args, act1, act2, split, **kw):
    import torch

    from die_amd.ops import kernels as K

    kw.setdefault("fill", FILL)
    out = K.se_block(*args, act1, act2, split=split, **kw)
    torch.cuda.synchronize()
    return out


def _bits(t):
    import torch

    return t.contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


@pytest.mark.parametrize("split", [False, True])
@pytest.mark.parametrize("i,shape", list(enumerate(itertools.product(MAPS, CHANNELS))))
def test_against_the_onnx_expression_in_float64(native, i, shape, split):
    """the hidden width and the act pair move on with the case; every fourth case has no b1, every fifth no b2"""
    import torch

    (H, W), C = shape
    Cr, (act1, act2) = HIDDEN[(i + i // len(CHANNELS)) % len(HIDDEN)], ACTS[i % len(ACTS)]
    x, w1, b1, w2, b2 = _inputs(H, W, C, Cr, seed=500 + i)
    got = _run((x, w1, None if i % 4 == 1 else b1, w2, None if i % 5 == 2 else b2), act1, act2, split)
    ref = _reference(x, w1, torch.zeros_like(b1) if i % 4 == 1 else b1, w2, torch.zeros_like(b2) if i % 5 == 2 else b2, act1, act2, split)
    _check(*got, ref, split, (H, W, C, Cr, act1, act2, split))


@pytest.mark.parametrize("split", [False, True])
@pytest.mark.parametrize("slices", [1, 7, 64, 0])
def test_slices_of_a_large_map(native, split, slices):
    """56 x 56 x 264: one block per sample, slices whose last one is short, the cap, and the launcher's choice;
    a non-default HardSigmoid"""
    args = _inputs(56, 56, 264, 10, seed=77)
    out, gate = _run(args, "relu", "hardsigmoid", split, slices=slices, alpha=0.2, beta=0.4)
    _check(out, gate, _reference(*args, "relu", "hardsigmoid", split, 0.2, 0.4), split, ("56x56", slices, split))


@pytest.mark.parametrize("split", [False, True])
@pytest.mark.parametrize("case", [(3, 5, 24, 4, 0), (14, 14, 2056, 10, 0), (56, 56, 264, 240, 5)])
def test_live_batch_repeatability_in_place(native, split, case):
    import torch

    from die_amd.ops import kernels as K

    H, W, C, Cr, slices = case
    args = _inputs(H, W, C, Cr, seed=91)
    full, gate = _run(args, "silu", "sigmoid", split, slices=slices)
    # the same counters again: they went back to 0 and the sums are added in a fixed order
    again, gate2 = _run(args, "silu", "sigmoid", split, slices=slices)
    assert torch.equal(_bits(full), _bits(again)) and torch.equal(_bits(gate), _bits(gate2)), "two runs differ"
    live = B - 1
    part, pgate = _run(args, "silu", "sigmoid", split, slices=slices, live=live)
    assert bool((part[..., live:, :, :, :] == FILL).all()) and bool((pgate[live:] == FILL).all())
    assert torch.equal(_bits(part[..., :live, :, :, :]), _bits(full[..., :live, :, :, :]))
    assert torch.equal(_bits(pgate[:live]), _bits(gate[:live]))
    # in place: out = the stored planes of x
    planes = K.split_planes(args[0]) if split else args[0].to(torch.bfloat16).contiguous()
    same, _ = _run((planes,) + args[1:], "silu", "sigmoid", split, slices=slices, out=planes, fill=None)
    assert same.data_ptr() == planes.data_ptr() and torch.equal(_bits(planes), _bits(full))


@pytest.mark.parametrize("bad", [dict(C=12), dict(C=4104), dict(Cr=1025), dict(act1=2), dict(act2=2), dict(slices=-1)])
def test_out_of_scope_is_invalid_value(native, bad):
    """hipErrorInvalidValue (1) from the launcher's own check, nothing launched: y and the gate keep the sentinel"""
    import torch

    from die_amd import native as nat
    from die_amd.ops import kernels as K

    C, Cr = bad.get("C", 24), bad.get("Cr", 4)
    args = _inputs(2, 2, C, Cr, seed=5, batch=2)
    out = torch.empty(args[0].shape, dtype=torch.bfloat16, device="cuda")
    with pytest.raises(nat.NativeError, match=r"hipError 1\b"):
        K.se_block(*args, bad.get("act1", "relu"), bad.get("act2", "sigmoid"), slices=bad.get("slices", 0), out=out, fill=FILL)
    torch.cuda.synchronize()
    assert bool((out == FILL).all())
