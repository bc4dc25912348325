"""The Global Response Normalization kernel (csrc/kernels/grn.hip) through ops.kernels.grn, against the ONNX
expression of ConvNeXt-V2's GRN in float64 on the STORED input values:
    G = sqrt(sum_{h,w} x^2),  nx = G / (mean_c G + eps),  y = gamma * (x * nx) + beta + x
The bars are those of tests/test_gpu_groupnorm.py and tests/test_gpu_dwconv.py: rel-L2 < 2e-5 split, < 1e-2
bf16 -- applied to the whole output AND to every channel on its own, so that a small channel is not hidden
behind a large one.  Every case runs B = 3 samples into a sentinel-filled output.  Shapes: maps from 1x1 to
17x9, channels from one 16-byte chunk (8) over 20 chunks (160, which do not divide the 256 threads) to 2056
and 3072 (more chunks than a block has threads: two column tiles), and one 56x56x384 map whose statistics
are merged from many blocks."""
import itertools
import json

import pytest

from conftest import gpu_available

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not gpu_available(), reason="needs a GPU")]

B = 3
MAPS = [(1, 1), (2, 2), (5, 7), (17, 9)]
CHANNELS = [8, 24, 160, 384, 2056, 3072]
BIG = ((56, 56), 384, 2)  # map, channels, batch
# (gamma, beta, eps): the cases take them in turn
PARAMS = [(True, True, 1e-6), (True, False, 1e-3), (False, False, 1e-6), (True, True, 1e-3), (True, False, 1e-6),
          (False, False, 1e-3)]
FILL = -(2.0 ** 100)  # sentinel in the output buffer: exact in bf16 and far from every value a case can produce


def _bar(split):
    return 2e-5 if split else 1e-2


def _inputs(H, W, C, batch, seed):
    import torch

    g = torch.Generator(device="cuda").manual_seed(seed)
    x = torch.randn(batch, H, W, C, device="cuda", generator=g) * 1.5 + 0.3
    gamma = torch.rand(C, device="cuda", generator=g) + 0.5
    beta = torch.randn(C, device="cuda", generator=g)
    return x, gamma, beta


def _stored(x, split):
    import torch

    from die_amd.ops import kernels as K

    return K.join_planes(K.split_planes(x)) if split else x.to(torch.bfloat16).float()


def _reference(x, gamma, beta, eps, split):
    """the ONNX expression in float64 on the stored values; [B, H, W, C]"""
    import torch

    xs = _stored(x, split).double()
    G = torch.sqrt((xs * xs).sum(dim=(1, 2), keepdim=True))
    nx = G / (G.mean(dim=-1, keepdim=True) + eps)
    y = xs * nx
    if gamma is None:
        y = torch.zeros_like(y)  # a missing gamma is 0
    else:
        y = gamma.double() * y
    if beta is not None:
        y = y + beta.double()
    return y + xs


def _run(x, gamma, beta, eps, split, **kw):
    import torch

    from die_amd.ops import kernels as K

    kw.setdefault("fill", FILL)
    out = K.grn(x, gamma, beta, eps, split=split, **kw)
    torch.cuda.synchronize()
    return out


def _values(out, split):
    from die_amd.ops import kernels as K

    return (K.join_planes(out) if split else out.float()).double()  # [B, H, W, C]


def _rel(d, r):
    """rel-L2; an all-zero reference must be met exactly"""
    if float(r.norm()) == 0.0:
        return 0.0 if float(d.norm()) == 0.0 else float("inf")
    return float(d.norm() / r.norm())


def _check(out, ref, split, what):
    import torch

    assert bool(torch.isfinite(out.float()).all()), what
    vals = _values(out, split)
    err = _rel(vals - ref, ref)
    d = (vals - ref).flatten(0, 2).norm(dim=0)  # per channel over (B, H, W)
    r = ref.flatten(0, 2).norm(dim=0)
    per = torch.where(r > 0, d / r.clamp(min=1e-300), torch.where(d > 0, torch.full_like(d, float("inf")), torch.zeros_like(d)))
    worst = float(per.max())
    print(what, "rel-L2 %.3g, worst channel %.3g (channel %d)" % (err, worst, int(per.argmax())))
    assert err < _bar(split), (err, what)
    assert worst < _bar(split), (worst, int(per.argmax()), what)


def _cases():
    cases = [(m, C, B) for m, C in itertools.product(MAPS, CHANNELS)] + [BIG]
    # the parameter form moves on by one with every map, so that a channel count meets several forms
    return [(m, C, batch) + PARAMS[(i + i // len(CHANNELS)) % len(PARAMS)] for i, (m, C, batch) in enumerate(cases)]


@pytest.mark.parametrize("split", [False, True])
def test_against_the_onnx_expression_in_float64(native, split):
    n = 0
    for i, ((H, W), C, batch, hg, hb, eps) in enumerate(_cases()):
        x, gamma, beta = _inputs(H, W, C, batch, seed=300 + i)
        gamma, beta = gamma if hg else None, beta if hb else None
        out = _run(x, gamma, beta, eps, split)
        _check(out, _reference(x, gamma, beta, eps, split), split, (H, W, C, batch, hg, hb, eps, split))
        assert bool((out != FILL).all()), (H, W, C)  # every element was written
        n += 1
    assert n == len(MAPS) * len(CHANNELS) + 1 == 25, n


@pytest.mark.parametrize("split", [False, True])
@pytest.mark.parametrize("shape", [(5, 7, 24), (2, 2, 2056), (17, 9, 384)])
def test_zero_parameters_return_the_input(native, split, shape):
    """gamma = 0 and beta = 0, as arrays or both missing: a = 1 exactly and fma(x, 1, 0) = x, so the joined
    output is the joined stored input"""
    import torch

    H, W, C = shape
    x, _, _ = _inputs(H, W, C, B, seed=9)
    want = _stored(x, split).double()
    zeros = torch.zeros(C, device="cuda")
    for gamma, beta in ((zeros, zeros), (None, None)):
        out = _run(x, gamma, beta, 1e-6, split)
        assert torch.equal(_values(out, split), want), (shape, split, gamma is None)


@pytest.mark.parametrize("split", [False, True])
@pytest.mark.parametrize("shape", [(1, 1, 8), (5, 7, 160), (17, 9, 3072)])
def test_all_zero_sample_gives_beta(native, split, shape):
    """G = 0 in every channel: nx = 0 / (0 + eps) = 0, y = beta as stored, no NaN; the other samples are as ever"""
    import torch

    H, W, C = shape
    for eps in (1e-6, 1e-3):
        x, gamma, beta = _inputs(H, W, C, B, seed=11)
        x[1] = 0.0
        out = _run(x, gamma, beta, eps, split)
        assert bool(torch.isfinite(out.float()).all())
        want = _stored(beta.view(1, 1, C).expand(H, W, C).contiguous(), split).double()
        assert torch.equal(_values(out, split)[1], want), (shape, split, eps)
        _check(out, _reference(x, gamma, beta, eps, split), split, ("zero sample", shape, split, eps))


@pytest.mark.parametrize("split", [False, True])
@pytest.mark.parametrize("shape", [(5, 7, 160), (17, 9, 2056)])
def test_channel_imbalance(native, split, shape):
    """one channel scaled by 1e3 and one by 1e-3: the per-channel bar holds for both"""
    H, W, C = shape
    x, gamma, beta = _inputs(H, W, C, B, seed=13)
    x[..., 3] *= 1e3
    x[..., C - 5] *= 1e-3
    for b in (beta, None):
        out = _run(x, gamma, b, 1e-6, split)
        _check(out, _reference(x, gamma, b, 1e-6, split), split, ("imbalance", shape, split, b is not None))


def _bits(t):
    import torch

    return t.contiguous().view(torch.int16)


@pytest.mark.parametrize("split", [False, True])
@pytest.mark.parametrize("case", [((2, 2), 24, B), ((5, 7), 160, B), ((17, 9), 2056, B), BIG])
def test_live_batch_invariance_repeatability(native, split, case):
    import torch

    (H, W), C, batch = case
    x, gamma, beta = _inputs(H, W, C, batch, seed=55)
    full = _run(x, gamma, beta, 1e-6, split)
    again = _run(x, gamma, beta, 1e-6, split)
    assert torch.equal(_bits(full), _bits(again)), "two runs differ"
    live = batch - 1
    part = _run(x, gamma, beta, 1e-6, split, live=live)
    # samples past the live count keep the sentinel in every plane; the others have the bits of the full run
    assert bool((part[..., live:, :, :, :] == FILL).all())
    assert torch.equal(_bits(part[..., :live, :, :, :]), _bits(full[..., :live, :, :, :]))
    # every sample alone (B = 1) has the bits of its slice of the batch
    for i in range(batch):
        alone = _run(x[i:i + 1].contiguous(), gamma, beta, 1e-6, split)
        assert torch.equal(_bits(alone), _bits(full[..., i:i + 1, :, :, :])), i
    # ... and in every other position of the batch
    perm = list(range(1, batch)) + [0]
    moved = _run(x[perm].contiguous(), gamma, beta, 1e-6, split)
    for k, i in enumerate(perm):
        assert torch.equal(_bits(moved[..., k, :, :, :]), _bits(full[..., i, :, :, :])), (k, i)


@pytest.mark.parametrize("split", [False, True])
@pytest.mark.parametrize("case", [((2, 2), 24, B), ((17, 9), 160, B), ((5, 7), 3072, B), BIG])
def test_in_place(native, split, case):
    """out = x: the same bits as out of place"""
    import torch

    from die_amd.ops import kernels as K

    (H, W), C, batch = case
    x, gamma, beta = _inputs(H, W, C, batch, seed=71)
    planes = K.split_planes(x) if split else x.to(torch.bfloat16).contiguous()
    apart = _run(planes, gamma, beta, 1e-6, split)
    before = planes.clone()
    same = _run(planes, gamma, beta, 1e-6, split, out=planes, fill=None)
    assert same.data_ptr() == planes.data_ptr() and not torch.equal(_bits(planes), _bits(before))
    assert torch.equal(_bits(planes), _bits(apart))


def test_bad_arguments_are_invalid_value(native):
    """C % 8 != 0, HW < 1, a misaligned x / out / gamma / beta / ws, a missing or too-small workspace:
    hipErrorInvalidValue (1) from the launcher's own check, nothing launched -- the output keeps the sentinel"""
    import torch

    from die_amd import native as nat
    from die_amd.ops import kernels as K

    L = nat.kernels()
    Bn, H, W, C = 2, 4, 4, 24
    x = torch.randn(Bn, H, W, C, device="cuda")

    def attempt(xx, **kw):
        out = torch.empty(xx.shape, dtype=torch.bfloat16, device="cuda")
        with pytest.raises(nat.NativeError, match=r"hipError 1\b"):
            K.grn(xx, fill=FILL, out=out, **kw)
        torch.cuda.synchronize()
        assert bool((out == FILL).all())

    attempt(torch.randn(2, 4, 4, 12, device="cuda"))  # C % 8
    need = int(L.die_grn_workspace_bytes(Bn, H * W, C))
    assert need > 0 and L.die_grn_workspace_bytes(Bn, H * W, 12) == 0 and L.die_grn_workspace_bytes(Bn, 0, C) == 0
    attempt(x, ws_bytes=need - 4)  # a workspace one float short
    attempt(x, ws_bytes=0)

    # the raw entry point: pointers moved off their alignment, a null workspace, HW = 0
    xin = x.to(torch.bfloat16).contiguous()
    spare = torch.zeros(64, dtype=torch.bfloat16, device="cuda")  # room behind the shifted pointers
    xbuf = torch.cat([xin.flatten(), spare])
    obuf = torch.full((xin.numel() + 64,), FILL, dtype=torch.bfloat16, device="cuda")
    gamma = torch.ones(C + 4, device="cuda")
    beta = torch.zeros(C + 4, device="cuda")
    ws = torch.zeros(need // 4 + 16, dtype=torch.float32, device="cuda")

    def raw(dx=0, do=0, dg=0, db=0, dw=0, no_ws=False, **geom):
        g = dict(B=Bn, HW=H * W, C=C, eps=1e-6, split=0, ws_bytes=need)
        g.update(geom)
        rc = L.die_kern_grn(json.dumps(g).encode(), xbuf.data_ptr() + dx, gamma.data_ptr() + dg, beta.data_ptr() + db,
                            obuf.data_ptr() + do, 0 if no_ws else ws.data_ptr() + dw, 0, K._stream())
        torch.cuda.synchronize()
        return rc

    for kw in (dict(dx=8), dict(do=8), dict(dg=2), dict(db=2), dict(dw=8), dict(no_ws=True), dict(HW=0), dict(C=20)):
        assert raw(**kw) == 1, kw
        assert bool((obuf == FILL).all()), kw
    assert raw() == 0  # and the same call with good arguments goes through
    assert bool((obuf[:xin.numel()] != FILL).all()) and bool((obuf[xin.numel():] == FILL).all())
    ref = _reference(x, gamma[:C], beta[:C], 1e-6, False)
    _check(obuf[:xin.numel()].view(Bn, H, W, C), ref, False, "raw call")
