"""The streaming attention kernel's KEYMASK mode (csrc/kernels/transformer.hip): a per-sample key
mask -- the request's padding -- given as the key data embed_tokens writes (kvis rows of 0 / -inf,
kend = 1 + the last visible key), alone and with a BIAS table.  Against torch with an explicit
masked_fill at the bars of tests/test_gpu_attention_mask.py (bf16 vs torch fp32 < 2e-2, fp32 split vs
float64 <= 1e-5), and bit for bit against the BIAS mode given the same mask as a table, against the
unmasked kernel when every key is visible, and for the neighbours of an all-pad sample."""
import functools
import math

import pytest

from conftest import gpu_available

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not gpu_available(), reason="needs a GPU")]

B = 4


@pytest.fixture(scope="module")
def K():
    from die_amd.ops import kernels

    return kernels


@functools.lru_cache(maxsize=None)
def _qkv(S, H, D, Bn=B):
    import torch

    g = torch.Generator(device="cuda").manual_seed(S * 131 + H * 17 + D + Bn)
    return torch.randn(Bn, S, 3 * H * D, device="cuda", generator=g)


@functools.lru_cache(maxsize=None)
def _visible(S, holes=False):
    """bool [4, S]: visible lengths 1, min(S, 32), S, min(S, 45); holes: pad ids inside the lengths too."""
    import torch

    vis = torch.zeros(B, S, dtype=torch.bool, device="cuda")
    for b, n in enumerate((1, min(S, 32), S, min(S, 45))):
        vis[b, :n] = True
    if holes:
        vis[1, 3] = False                 # inside the first tile
        vis[2, 5:S - 2:7] = False         # all along a full-length row
        vis[2, S - 1] = True
        vis[3, min(S, 45) // 2] = False
    return vis


@functools.lru_cache(maxsize=None)
def _table(S, H):
    import torch

    g = torch.Generator(device="cuda").manual_seed(S * 7 + H)
    i = torch.arange(S, device="cuda")
    return torch.randn(H, S, S, device="cuda", generator=g) + torch.arange(H, device="cuda")[:, None, None] * i[None, None, :] / S


def _ref(qkv, H, scale, vis, table, dtype):
    import torch

    Bn, S, C3 = qkv.shape
    C = C3 // 3
    D = C // H
    q, k, v = (qkv[..., i * C:(i + 1) * C].to(dtype).reshape(Bn, S, H, D).transpose(1, 2) for i in range(3))
    sc = q @ k.transpose(-1, -2) * scale
    if table is not None:
        sc = sc + table.to(dtype)
    sc = sc.masked_fill(~vis[:, None, None, :], -math.inf)
    return (torch.softmax(sc, -1) @ v).transpose(1, 2).reshape(Bn, S, C)


def _rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


def _check(K, S, H, D, holes=False, with_table=False):
    import torch

    qkv = _qkv(S, H, D)
    C = H * D
    vis = _visible(S, holes)
    table = _table(S, H) if with_table else None
    scale = 1.0 / math.sqrt(D)
    qb = qkv.bfloat16()
    out = K.attention(qb[..., :C], qb[..., C:2 * C], qb[..., 2 * C:], H, scale, bias=table, key_mask=vis)
    e16 = _rel(out, _ref(qb.float(), H, scale, vis, table, torch.float32))
    got = K.attention_qkv_split(qkv, H, scale, bias=table, key_mask=vis)
    e32 = _rel(got, _ref(qkv, H, scale, vis, table, torch.float64))
    print("S=%d H=%d D=%d holes=%s table=%s: bf16 %.2e split %.2e" % (S, H, D, holes, with_table, e16, e32))
    assert torch.isfinite(out.float()).all() and torch.isfinite(got).all()
    assert e16 < 2e-2, e16
    assert e32 <= 1e-5, e32


# 17: one partial tile; 33: a partial second tile; 64 / 65: tile edge; 129: a second query block
# holding one row; 300: many tiles.  Visible lengths 1 (first tile, one key), 32 (tile edge: one tile
# walked), S (all tiles), 45 (mid-tile: two tiles walked, the second masked by the row).
@pytest.mark.parametrize("S", [17, 33, 64, 65, 129, 300])
def test_keymask_sequence_lengths(K, S):
    _check(K, S, 3, 64)


def test_keymask_with_holes(K):
    _check(K, 129, 3, 64, holes=True)


@pytest.mark.parametrize("D", [32, 80, 96, 128])
def test_keymask_head_dims(K, D):
    _check(K, 129, 3, D)


@pytest.mark.parametrize("S", [33, 129])
def test_keymask_with_bias_table(K, S):
    _check(K, S, 3, 64, holes=True, with_table=True)


@pytest.mark.parametrize("S", [33, 129, 300])
def test_keymask_equals_bias_mode_bitwise(K, S):
    """B = 1: the key mask as a [S, S] table through the BIAS mode gives the same bits -- a tile the
    key-mask mode does not walk contributes alpha = 1, p = 0 in the BIAS mode."""
    import torch

    H, D = 3, 64
    C = H * D
    for n, holes in ((1, False), (min(S, 32), False), (min(S, 45), True), (S, True)):
        qkv = _qkv(S, H, D, 1)
        vis = torch.zeros(1, S, dtype=torch.bool, device="cuda")
        vis[0, :n] = True
        if holes and n > 4:
            vis[0, 2:n - 1:5] = False
        table = torch.where(vis[0], 0.0, -math.inf)[None, :].expand(S, S).contiguous()
        qb = qkv.bfloat16()
        q, k, v = qb[..., :C], qb[..., C:2 * C], qb[..., 2 * C:]
        assert torch.equal(K.attention(q, k, v, H, key_mask=vis), K.attention(q, k, v, H, bias=table)), (S, n)
        assert torch.equal(K.attention_qkv_split(qkv, H, key_mask=vis), K.attention_qkv_split(qkv, H, bias=table)), (S, n)


@pytest.mark.parametrize("S,D", [(65, 64), (129, 128), (300, 32)])
def test_all_visible_equals_unmasked_bitwise(K, S, D):
    import torch

    H = 2
    C = H * D
    qkv = _qkv(S, H, D)
    vis = torch.ones(B, S, dtype=torch.bool, device="cuda")
    qb = qkv.bfloat16()
    q, k, v = qb[..., :C], qb[..., C:2 * C], qb[..., 2 * C:]
    assert torch.equal(K.attention(q, k, v, H, key_mask=vis), K.attention(q, k, v, H))
    assert torch.equal(K.attention_qkv_split(qkv, H, key_mask=vis), K.attention_qkv_split(qkv, H))


@pytest.mark.parametrize("with_table", [False, True])
def test_all_pad_sample_is_zero_and_leaves_its_neighbours_alone(K, with_table):
    import torch

    S, H, D = 129, 3, 64
    C = H * D
    qkv = _qkv(S, H, D, 3)
    table = _table(S, H) if with_table else None
    vis = torch.ones(3, S, dtype=torch.bool, device="cuda")
    vis[0, :] = False
    vis[1, 40:] = False
    qb = qkv.bfloat16()
    out = K.attention(qb[..., :C], qb[..., C:2 * C], qb[..., 2 * C:], H, bias=table, key_mask=vis)
    got = K.attention_qkv_split(qkv, H, bias=table, key_mask=vis)
    assert (out[0] == 0).all() and (got[0] == 0).all()
    # samples 1 and 2 run without the all-pad sample
    qb2, qkv2, vis2 = qb[1:].contiguous(), qkv[1:].contiguous(), vis[1:].contiguous()
    out2 = K.attention(qb2[..., :C], qb2[..., C:2 * C], qb2[..., 2 * C:], H, bias=table, key_mask=vis2)
    got2 = K.attention_qkv_split(qkv2, H, bias=table, key_mask=vis2)
    assert torch.equal(out[1:], out2) and torch.equal(got[1:], got2)
    assert torch.isfinite(out.float()).all() and torch.isfinite(got).all()


def test_key_data_pair_from_embed_tokens_feeds_attention(K):
    """The (kvis, kend) pair embed_tokens writes is the key_mask argument as it is."""
    import torch

    S, H, D = 65, 3, 64
    C = H * D
    qkv = _qkv(S, H, D)
    vis = _visible(S, True)
    ids = torch.where(vis, 5.0, 0.0)
    _, kvis, kend = K.embed_tokens(ids, torch.zeros(8, 8, device="cuda"), pad_test=0)
    qb = qkv.bfloat16()
    q, k, v = qb[..., :C], qb[..., C:2 * C], qb[..., 2 * C:]
    assert torch.equal(K.attention(q, k, v, H, key_mask=(kvis, kend)), K.attention(q, k, v, H, key_mask=vis))


def test_keymask_launcher_rejects_bad_arguments(K):
    """Key mask + causal, a misaligned kvis, a wrong Sp and one of the pair missing are errors from the
    launcher (nothing is launched)."""
    import torch

    from die_amd import native

    Bn, S, H, D = 2, 40, 2, 64
    C = H * D
    x = torch.zeros(Bn, S, C, device="cuda", dtype=torch.bfloat16)
    out = torch.empty_like(x)
    kvis = torch.zeros(Bn * 64 + 4, device="cuda")
    kend = torch.full((Bn,), S, device="cuda", dtype=torch.int32)
    L = native.kernels()
    st = torch.cuda.current_stream().cuda_stream

    def call(Sp=64, causal=0, kv=kvis.data_ptr(), ke=kend.data_ptr()):
        return L.die_kern_attention(native.geometry(dict(
            q=x.data_ptr(), k=x.data_ptr(), v=x.data_ptr(), out=out.data_ptr(), B=Bn, S=S, H=H, D=D, ldq=C, ldk=C, ldv=C,
            ldo=C, scale=0.125, split=0, bias=0, bias_heads=0, Sp=Sp, causal=causal, kvis=kv, kend=ke)), st)

    assert call() == 0
    assert call(causal=1) != 0
    assert call(kv=kvis.data_ptr() + 4) != 0  # 16-byte loads
    assert call(Sp=40) != 0 and call(Sp=96) != 0  # Sp must be 64 for S = 40
    assert call(ke=0) != 0 and call(kv=0) != 0  # both or neither
    assert call(kv=0, ke=0, Sp=0) == 0  # neither: the unmasked kernel
    torch.cuda.synchronize()
    with pytest.raises((native.NativeError, ValueError, AssertionError)):
        K.attention(x, x, x, H, causal=True, key_mask=torch.ones(Bn, S, dtype=torch.bool, device="cuda"))
    with pytest.raises((native.NativeError, ValueError, AssertionError)):
        K.attention(x, x, x, H, key_mask=torch.ones(Bn, S + 1, dtype=torch.bool, device="cuda"))
