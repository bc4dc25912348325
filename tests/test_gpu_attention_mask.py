"""The streaming attention kernel's masked modes (csrc/kernels/transformer.hip: BIAS, CAUSAL) against
torch given the same bias tensor: bf16 vs torch fp32 at rel-L2 < 2e-2 and fp32 (split) vs float64 at
<= 1e-5, the bars of tests/test_gpu_transformer.py for this kernel."""
import functools
import math

import pytest

from conftest import gpu_available

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not gpu_available(), reason="needs a GPU")]

KINDS = ["shared", "per_head", "key_only", "causal", "causal_per_head", "band"]


@pytest.fixture(scope="module")
def K():
    from die_amd.ops import kernels

    return kernels


@functools.lru_cache(maxsize=None)
def _qkv(S, H, D, B=2):
    import torch

    g = torch.Generator(device="cuda").manual_seed(S * 131 + H * 17 + D)
    return torch.randn(B, S, 3 * H * D, device="cuda", generator=g)


@functools.lru_cache(maxsize=None)
def _mask(kind, S, H):
    """(bias argument or None, causal flag, the full additive term [1 or H, S, S] for the reference)."""
    import torch

    g = torch.Generator(device="cuda").manual_seed(S * 7 + H + len(kind))
    i = torch.arange(S, device="cuda")
    tri = torch.where(i[None, :] <= i[:, None], 0.0, -math.inf)  # [S, S]: key j visible to query i iff j <= i
    if kind == "shared":
        b = torch.randn(S, S, device="cuda", generator=g)
        return b, False, b[None]
    if kind == "per_head":  # distinct heads: a wrong head stride fails
        b = torch.randn(H, S, S, device="cuda", generator=g) + torch.arange(H, device="cuda")[:, None, None] * i[None, None, :] / S
        return b, False, b
    if kind == "key_only":
        row = torch.randn(S, device="cuda", generator=g)
        row[S - S // 4:] = -10000.0
        b = row[None, :].expand(S, S).contiguous()
        return b, False, b[None]
    if kind == "causal":
        return None, True, tri[None]
    if kind == "causal_per_head":
        b = torch.randn(H, S, S, device="cuda", generator=g)
        return b, True, b + tri
    if kind == "band":  # from query 41 on, the first 32-key tile is entirely -inf
        b = torch.where((i[:, None] - i[None, :]).abs() <= 8, 0.0, -math.inf)
        return b, False, b[None]
    raise KeyError(kind)


def _ref(qkv, H, scale, term, dtype):
    import torch

    B, S, C3 = qkv.shape
    C = C3 // 3
    D = C // H
    q, k, v = (qkv[..., i * C:(i + 1) * C].to(dtype).reshape(B, S, H, D).transpose(1, 2) for i in range(3))
    p = torch.softmax(q @ k.transpose(-1, -2) * scale + term.to(dtype), -1)
    return (p @ v).transpose(1, 2).reshape(B, S, C)


def _rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


def _check(K, S, H, D, kind):
    import torch

    qkv = _qkv(S, H, D)
    C = H * D
    bias, causal, term = _mask(kind, S, H)
    scale = 1.0 / math.sqrt(D)
    qb = qkv.bfloat16()
    out = K.attention(qb[..., :C], qb[..., C:2 * C], qb[..., 2 * C:], H, scale, bias=bias, causal=causal)
    e16 = _rel(out, _ref(qb.float(), H, scale, term, torch.float32))
    got = K.attention_qkv_split(qkv, H, scale, bias=bias, causal=causal)
    e32 = _rel(got, _ref(qkv, H, scale, term, torch.float64))
    print("S=%d H=%d D=%d %s: bf16 %.2e split %.2e" % (S, H, D, kind, e16, e32))
    assert torch.isfinite(out.float()).all() and torch.isfinite(got).all()
    assert e16 < 2e-2, e16
    assert e32 <= 1e-5, e32


# 17: one partial tile; 33: the diagonal crosses into a partial second tile; 64 / 65: tile edge;
# 129: a second query block holding one row (block tile limit, clamped idle rows); 197, 300: many tiles
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("S", [17, 33, 64, 65, 129, 197, 300])
def test_masked_attention_sequence_lengths(K, S, kind):
    _check(K, S, 3, 64, kind)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("D", [32, 80, 96, 128])
def test_masked_attention_head_dims(K, D, kind):
    _check(K, 129, 2, D, kind)


@pytest.mark.parametrize("S", [33, 129, 300])
def test_causal_flag_equals_explicit_triangle_bitwise(K, S):
    """A skipped tile contributes alpha = 1, p = 0, so the flag (tile skip, block tile limit, diagonal
    element mask) and a -inf strict upper triangle passed as a bias agree bit for bit."""
    import torch

    H, D = 3, 64
    C = H * D
    qkv = _qkv(S, H, D)
    tri = _mask("causal", S, H)[2][0].contiguous()
    qb = qkv.bfloat16()
    q, k, v = qb[..., :C], qb[..., C:2 * C], qb[..., 2 * C:]
    assert torch.equal(K.attention(q, k, v, H, causal=True), K.attention(q, k, v, H, bias=tri))
    assert torch.equal(K.attention_qkv_split(qkv, H, causal=True), K.attention_qkv_split(qkv, H, bias=tri))
    # ... and with a per-head table under both
    b = _mask("per_head", S, H)[0]
    assert torch.equal(K.attention(q, k, v, H, bias=b, causal=True), K.attention(q, k, v, H, bias=b + tri))
    assert torch.equal(K.attention_qkv_split(qkv, H, bias=b, causal=True),
                       K.attention_qkv_split(qkv, H, bias=b + tri))


@pytest.mark.parametrize("S,D", [(65, 64), (129, 128), (197, 32)])
def test_zero_bias_equals_unmasked_bitwise(K, S, D):
    import torch

    H = 2
    C = H * D
    qkv = _qkv(S, H, D)
    qb = qkv.bfloat16()
    q, k, v = qb[..., :C], qb[..., C:2 * C], qb[..., 2 * C:]
    for zeros in (torch.zeros(S, S, device="cuda"), torch.zeros(H, S, S, device="cuda")):
        assert torch.equal(K.attention(q, k, v, H, bias=zeros), K.attention(q, k, v, H))
        assert torch.equal(K.attention_qkv_split(qkv, H, bias=zeros), K.attention_qkv_split(qkv, H))


def test_masked_attention_repeats_bitwise(K):
    import torch

    S, H, D = 197, 3, 64
    qkv = _qkv(S, H, D)
    b = _mask("causal_per_head", S, H)[0]
    assert torch.equal(K.attention_qkv_split(qkv, H, bias=b, causal=True),
                       K.attention_qkv_split(qkv, H, bias=b, causal=True))


def test_masked_attention_rejects_bad_arguments(K):
    """A bias whose row pitch is not S rounded up to 32, or whose head count is neither 1 nor H, is an
    error from the launcher (nothing is launched)."""
    import torch

    from die_amd import native

    B, S, H, D = 1, 40, 2, 64
    C = H * D
    x = torch.zeros(B, S, C, device="cuda", dtype=torch.bfloat16)
    out = torch.empty_like(x)
    bias = torch.zeros(3 * S * 64, device="cuda")
    L = native.kernels()
    st = torch.cuda.current_stream().cuda_stream

    def call(bias_heads, Sp, ptr=bias.data_ptr()):
        return L.die_kern_attention(native.geometry(dict(
            q=x.data_ptr(), k=x.data_ptr(), v=x.data_ptr(), out=out.data_ptr(), B=B, S=S, H=H, D=D, ldq=C, ldk=C, ldv=C,
            ldo=C, scale=0.125, split=0, bias=ptr, bias_heads=bias_heads, Sp=Sp, causal=0)), st)

    assert call(1, 64) == 0 and call(H, 64) == 0
    assert call(1, 40) != 0 and call(1, 96) != 0  # Sp must be 64 for S = 40
    assert call(3, 64) != 0 and call(0, 64) != 0  # heads: 1 or H when a bias is given
    assert call(1, 64, ptr=0) != 0
    torch.cuda.synchronize()
    with pytest.raises((native.NativeError, ValueError, AssertionError)):
        K.attention(x, x, x, H, bias=torch.zeros(3, S, S, device="cuda"))
    with pytest.raises((native.NativeError, ValueError, AssertionError)):
        K.attention(x, x, x, H, bias=torch.zeros(S + 1, S + 1, device="cuda"))
