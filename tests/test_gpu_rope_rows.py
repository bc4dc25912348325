"""rope_rows (csrc/kernels/transformer.hip): the rotate-half rotary embedding of head rows against
float64 numpy on the stored inputs (bf16 values; hi + lo planes in fp32 mode).  Bars: the project's
for stored rows -- 2e-5 rel-L2 in fp32 (split) mode, 3e-2 for bf16 (tests/test_gpu_pool_tokens.py).
The rotation is two products and a sum in fp32 per element, far inside both."""
import numpy as np
import pytest

from conftest import gpu_available

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not gpu_available(), reason="needs a GPU")]

HEAD_DIMS = (32, 64, 80, 128)
HEADS = (1, 3)
SEQS = (1, 33, 160)
BATCHES = (1, 5)
F32_BAR, BF16_BAR = 2e-5, 3e-2
SENTINEL = -7.0  # exact in bf16, its lo plane is 0


def _tables(S, D, theta=10000.0):
    from die_amd.models import generic as G

    return G.rope_tables(S, D, theta)


def _buffers(B, S, H, D, fused, split, seed, ldy_extra=0):
    """x rows [B*S, ldx] with the block at columns [col, col + H*D) (fused: the K block of a [Q | K | V]
    buffer), everything else the sentinel; a sentinel-filled y [B*S, H*D + ldy_extra].  Returns
    (xbuf, ybuf, col, stored block float64 [B, S, H, D])."""
    import torch

    from die_amd.ops import kernels as K

    W, rows = H * D, B * S
    ldx, col = (3 * W, W) if fused else (W, 0)
    x = torch.full((rows, ldx), SENTINEL, dtype=torch.float32)
    x[:, col:col + W] = torch.from_numpy(np.random.default_rng(seed).standard_normal((rows, W)).astype(np.float32))
    y = torch.full((rows, W + ldy_extra), SENTINEL, dtype=torch.float32)
    if split:
        xbuf, ybuf = K.split_planes(x.cuda()), K.split_planes(y.cuda())
        stored = K.join_planes(xbuf).cpu().double().numpy()
    else:
        xbuf, ybuf = x.cuda().to(torch.bfloat16), y.cuda().to(torch.bfloat16)
        stored = xbuf.cpu().double().numpy()
    return xbuf, ybuf, col, stored[:, col:col + W].reshape(B, S, H, D)


def _ref(block, cos, sin):
    """block [B, S, H, D] float64, cos / sin [S, D]: the index law of the kernel's contract."""
    h2 = block.shape[-1] // 2
    c, s = cos.astype(np.float64)[None, :, None, :], sin.astype(np.float64)[None, :, None, :]
    out = np.empty_like(block)
    out[..., :h2] = block[..., :h2] * c[..., :h2] - block[..., h2:] * s[..., :h2]
    out[..., h2:] = block[..., h2:] * c[..., h2:] + block[..., :h2] * s[..., h2:]
    return out


def _values(buf, split):
    from die_amd.ops import kernels as K

    return (K.join_planes(buf) if split else buf.float()).cpu().double().numpy()


def _rel(a, b):
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))


@pytest.mark.parametrize("D", HEAD_DIMS)
@pytest.mark.parametrize("split", [False, True])
def test_rotation_against_float64(native, D, split):
    import torch

    from die_amd.ops import kernels as K

    worst = 0.0
    for S in SEQS:
        cos, sin = (torch.from_numpy(t).cuda() for t in _tables(S, D))
        for B in BATCHES:
            for H in HEADS:
                for fused in (False, True):
                    xbuf, ybuf, col, block = _buffers(B, S, H, D, fused, split, seed=S * 11 + B * 3 + H)
                    before = xbuf.clone()
                    K.rope_rows(xbuf, cos, sin, B, S, H, D, col=col, split=split, ybuf=ybuf)
                    torch.cuda.synchronize()
                    got = _values(ybuf, split).reshape(B, S, H, D)
                    ref = _ref(block, cos.cpu().numpy(), sin.cpu().numpy())
                    err = _rel(got, ref)
                    worst = max(worst, err)
                    what = "B%d S%d H%d D%d fused %d %s" % (B, S, H, D, fused, "fp32" if split else "bf16")
                    assert np.isfinite(got).all() and err <= (F32_BAR if split else BF16_BAR), (what, err)
                    assert torch.equal(xbuf, before), what  # out of place: x and the columns around the block untouched
    print("D%d %s worst rel-L2 %.2e" % (D, "fp32" if split else "bf16", worst))


@pytest.mark.parametrize("split", [False, True])
def test_random_tables_pin_the_index_law(native, split):
    """Tables whose halves differ (nothing a real RoPE would store): y[j] uses cos / sin at j, y[j + D/2]
    at j + D/2, each with the partner element of x."""
    import torch

    from die_amd.ops import kernels as K

    B, S, H, D = 2, 33, 3, 80
    rng = np.random.default_rng(5)
    cos = torch.from_numpy(rng.standard_normal((S, D)).astype(np.float32)).cuda()
    sin = torch.from_numpy(rng.standard_normal((S, D)).astype(np.float32)).cuda()
    xbuf, ybuf, col, block = _buffers(B, S, H, D, True, split, seed=9)
    K.rope_rows(xbuf, cos, sin, B, S, H, D, col=col, split=split, ybuf=ybuf)
    got = _values(ybuf, split).reshape(B, S, H, D)
    err = _rel(got, _ref(block, cos.cpu().numpy(), sin.cpu().numpy()))
    print("random tables %s rel-L2 %.2e" % ("fp32" if split else "bf16", err))
    assert err <= (F32_BAR if split else BF16_BAR), err
    # the law with the halves of the tables swapped is a different function
    swapped = _ref(block, np.roll(cos.cpu().numpy(), D // 2, axis=1), np.roll(sin.cpu().numpy(), D // 2, axis=1))
    assert _rel(got, swapped) > 0.5


@pytest.mark.parametrize("split", [False, True])
def test_sentinels_around_the_output_block_survive(native, split):
    """y rows wider than H*D: the columns past the block keep their sentinel, in both planes."""
    import torch

    from die_amd.ops import kernels as K

    B, S, H, D = 5, 33, 3, 32
    cos, sin = (torch.from_numpy(t).cuda() for t in _tables(S, D))
    xbuf, ybuf, col, block = _buffers(B, S, H, D, True, split, seed=2, ldy_extra=16)
    y0 = ybuf.clone()
    K.rope_rows(xbuf, cos, sin, B, S, H, D, col=col, split=split, ybuf=ybuf)
    torch.cuda.synchronize()
    assert torch.equal(ybuf[..., H * D:], y0[..., H * D:])
    got = _values(ybuf, split)[:, :H * D].reshape(B, S, H, D)
    assert _rel(got, _ref(block, cos.cpu().numpy(), sin.cpu().numpy())) <= (F32_BAR if split else BF16_BAR)


@pytest.mark.parametrize("D", HEAD_DIMS)
@pytest.mark.parametrize("split", [False, True])
def test_identity_tables_return_x_bit_for_bit(native, D, split):
    import torch

    from die_amd.ops import kernels as K

    B, S, H = 5, 33, 3
    cos = torch.ones((S, D), dtype=torch.float32, device="cuda")
    sin = torch.zeros((S, D), dtype=torch.float32, device="cuda")
    xbuf, ybuf, col, _ = _buffers(B, S, H, D, True, split, seed=4)
    if split:  # the canonical planes of the stored values (hi = bf16(v), lo = v - hi exactly): what a kernel's store writes
        xbuf = K.split_planes(K.join_planes(xbuf))
    K.rope_rows(xbuf, cos, sin, B, S, H, D, col=col, split=split, ybuf=ybuf)
    torch.cuda.synchronize()
    assert torch.equal(ybuf, xbuf[..., col:col + H * D].contiguous())


@pytest.mark.parametrize("split", [False, True])
def test_bad_arguments_launch_nothing(native, split):
    """hipErrorInvalidValue (1) from the argument checks alone; a sentinel-filled y stays as it was."""
    import torch

    from die_amd.ops import kernels as K

    B, S, H = 2, 8, 2
    planes = (2,) if split else ()

    def buf(rows, ld):
        return torch.full(planes + (rows, ld), SENTINEL, dtype=torch.bfloat16, device="cuda")

    def tables(D):
        return (torch.ones((S, D), dtype=torch.float32, device="cuda"), torch.zeros((S, D), dtype=torch.float32, device="cuda"))

    def rejected(xbuf, ybuf, D, col=0, cos=None, sin=None):
        c, s = tables(D)
        y0 = ybuf.clone()
        rc, _ = K.rope_rows(xbuf, c if cos is None else cos, s if sin is None else sin, B, S, H, D, col=col, split=split,
                            ybuf=ybuf, check=False)
        torch.cuda.synchronize()
        assert rc == 1, rc
        assert torch.equal(ybuf, y0)

    rows, D = B * S, 64
    W = H * D
    for bad_d in (48, 16, 256):  # head dims the attention launcher does not take
        rejected(buf(rows, max(H * bad_d, 8)), buf(rows, max(H * bad_d, 8)), bad_d)
    rejected(buf(rows, W - 8), buf(rows, W), D)        # ldx < H*D
    rejected(buf(rows, W), buf(rows, W - 8), D)        # ldy < H*D
    rejected(buf(rows, W + 4), buf(rows, W), D)        # ldx not a multiple of 8
    rejected(buf(rows, W), buf(rows, W + 4), D)        # ldy not a multiple of 8
    rejected(buf(rows, W + 8), buf(rows, W), D, col=4)  # x 8 bytes off a 16-byte boundary
    flat = torch.full((planes + (rows * W + 8,)), SENTINEL, dtype=torch.bfloat16, device="cuda")
    if not split:  # a y 8 bytes off a 16-byte boundary
        rejected(buf(rows, W), flat[4:4 + rows * W].view(rows, W), D)
    c, s = tables(D)
    off = torch.ones((S * D + 1,), dtype=torch.float32, device="cuda")[1:].view(S, D)  # tables 4 bytes off
    rejected(buf(rows, W), buf(rows, W), D, cos=off)
    rejected(buf(rows, W), buf(rows, W), D, sin=off)
    # overlapping x / y: the same buffer, and y inside a fused x buffer
    x = buf(rows, W)
    y0 = x.clone()
    rc, _ = K.rope_rows(x, c, s, B, S, H, D, split=split, ybuf=x, check=False)
    torch.cuda.synchronize()
    assert rc == 1 and torch.equal(x, y0)
