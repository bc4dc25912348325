"""The streaming attention kernel's GQA mode (csrc/kernels/transformer.hip): K and V with fewer heads
than Q, a block per (image, kv head) pair whose four waves take four (query tile, head of the group)
items.  Against torch at the bars of tests/test_gpu_attention_mask.py / test_gpu_attention_keymask.py
(bf16 vs torch fp32 < 2e-2, fp32 split vs float64 <= 1e-5), and bit for bit against the per-head kernel
given K / V physically repeated to H heads: per-row arithmetic does not depend on the block a row
lands in."""
import functools
import math

import pytest

from conftest import gpu_available

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not gpu_available(), reason="needs a GPU")]

MODES = ("none", "causal", "key_mask")
# (H, Hkv, D): groups of 2, MQA over 4, groups of 3 (a block's items straddle query tiles), MQA over 3
# (odd, one pair per image); head dim 128: groups of 3 and MQA over 2
HEADS = [(4, 2, 64), (4, 1, 64), (6, 2, 64), (3, 1, 64), (6, 2, 128), (2, 1, 128)]


@pytest.fixture(scope="module")
def K():
    from die_amd.ops import kernels

    return kernels


@functools.lru_cache(maxsize=None)
def _qkv(S, H, Hkv, D, Bn):
    """Packed rows [Bn, S, (H + 2 Hkv) D] fp32: Q | K | V."""
    import torch

    g = torch.Generator(device="cuda").manual_seed(S * 131 + H * 17 + Hkv * 5 + D + Bn)
    return torch.randn(Bn, S, (H + 2 * Hkv) * D, device="cuda", generator=g)


def _repeated(qkv, H, Hkv, D):
    """The multi-head twin [Bn, S, 3 H D]: every K / V head repeated over its group."""
    import torch

    Bn, S, _ = qkv.shape
    C, Ckv, G = H * D, Hkv * D, H // Hkv
    k = qkv[..., C:C + Ckv].reshape(Bn, S, Hkv, D).repeat_interleave(G, dim=2).reshape(Bn, S, C)
    v = qkv[..., C + Ckv:].reshape(Bn, S, Hkv, D).repeat_interleave(G, dim=2).reshape(Bn, S, C)
    return torch.cat([qkv[..., :C], k, v], dim=-1).contiguous()


@functools.lru_cache(maxsize=None)
def _visible(S, Bn):
    """bool [Bn, S]: visible lengths 1, 32, S, 45 (Bn = 3: 1, S, 45) plus the holes of the key-mask test."""
    import torch

    vis = torch.zeros(4, S, dtype=torch.bool, device="cuda")
    for b, n in enumerate((1, min(S, 32), S, min(S, 45))):
        vis[b, :n] = True
    vis[1, 3] = False                 # inside the first tile
    vis[2, 5:S - 2:7] = False         # all along a full-length row
    vis[2, S - 1] = True
    vis[3, min(S, 45) // 2] = False
    return vis if Bn == 4 else vis[[0, 2, 3]].contiguous()


def _ref(qkv_rep, H, scale, mode, vis, dtype):
    import torch

    Bn, S, C3 = qkv_rep.shape
    C = C3 // 3
    D = C // H
    q, k, v = (qkv_rep[..., i * C:(i + 1) * C].to(dtype).reshape(Bn, S, H, D).transpose(1, 2) for i in range(3))
    sc = q @ k.transpose(-1, -2) * scale
    if mode == "causal":
        sc = sc.masked_fill(~torch.ones(S, S, dtype=torch.bool, device=sc.device).tril(), -math.inf)
    if mode == "key_mask":
        sc = sc.masked_fill(~vis[:, None, None, :], -math.inf)
    return (torch.softmax(sc, -1) @ v).transpose(1, 2).reshape(Bn, S, C)


def _rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


def _kw(mode, vis):
    return dict(causal=mode == "causal", key_mask=vis if mode == "key_mask" else None)


# 17: one partial tile; 33: a partial second tile; 64 / 65: tile edge; 129: five query tiles, so
# 5 G items -- idle waves in the last block for every G here; 300: many tiles and blocks.
@pytest.mark.parametrize("S", [17, 33, 64, 65, 129, 300])
@pytest.mark.parametrize("H,Hkv,D", HEADS)
def test_gqa_against_torch_and_the_per_head_kernel(K, S, H, Hkv, D):
    import torch

    C, Ckv = H * D, Hkv * D
    scale = 1.0 / math.sqrt(D)
    for Bn in (4, 3):  # Hkv * Bn a multiple of 8 (Hkv = 2, Bn = 4): the XCD map is on; Bn = 3: off
        qkv = _qkv(S, H, Hkv, D, Bn)
        rep = _repeated(qkv, H, Hkv, D)
        qb, rb = qkv.bfloat16(), rep.bfloat16()
        vis = _visible(S, Bn)
        for mode in MODES:
            kw = _kw(mode, vis)
            # bf16: K / V as column blocks of the packed buffer, and as tensors of their own
            out = K.attention(qb[..., :C], qb[..., C:C + Ckv], qb[..., C + Ckv:], H, scale, kv_heads=Hkv, **kw)
            sep = K.attention(qb[..., :C].contiguous(), qb[..., C:C + Ckv].contiguous(), qb[..., C + Ckv:].contiguous(), H,
                              scale, kv_heads=Hkv, **kw)
            got = K.attention_qkv_split(qkv, H, scale, kv_heads=Hkv, **kw)
            e16 = _rel(out, _ref(rb.float(), H, scale, mode, vis, torch.float32))
            e32 = _rel(got, _ref(rep, H, scale, mode, vis, torch.float64))
            print("S=%d H=%d Hkv=%d D=%d B=%d %s: bf16 %.2e split %.2e" % (S, H, Hkv, D, Bn, mode, e16, e32))
            assert torch.isfinite(out.float()).all() and torch.isfinite(got).all()
            assert e16 < 2e-2, (Bn, mode, e16)
            assert e32 <= 1e-5, (Bn, mode, e32)
            assert torch.equal(out, sep), (Bn, mode)
            # bit for bit: the per-head kernel on K / V repeated to H heads
            assert torch.equal(out, K.attention(rb[..., :C], rb[..., C:2 * C], rb[..., 2 * C:], H, scale, **kw)), (Bn, mode)
            assert torch.equal(got, K.attention_qkv_split(rep, H, scale, **kw)), (Bn, mode)


@pytest.mark.parametrize("S,H,D", [(65, 4, 64), (129, 3, 64), (300, 2, 128)])
def test_groups_of_one_through_the_gqa_mode_equal_the_per_head_kernel(K, S, H, D):
    """Variant 4 sends kv_heads == H through the GQA mapping (G = 1: a block's four waves are four
    query tiles of one head, the per-head mapping itself)."""
    import torch

    C = H * D
    qkv = _qkv(S, H, H, D, 4)
    qb = qkv.bfloat16()
    q, k, v = qb[..., :C], qb[..., C:2 * C], qb[..., 2 * C:]
    vis = _visible(S, 4)
    for mode in MODES:
        kw = _kw(mode, vis)
        want, want32 = K.attention(q, k, v, H, **kw), K.attention_qkv_split(qkv, H, **kw)
        # kv_heads = H through the new entry point is the old launch
        assert torch.equal(K.attention(q, k, v, H, kv_heads=H, **kw), want), mode
        assert torch.equal(K.attention_qkv_split(qkv, H, kv_heads=H, **kw), want32), mode
        K.set_attention_variant(4)
        try:
            got, got32 = K.attention(q, k, v, H, kv_heads=H, **kw), K.attention_qkv_split(qkv, H, kv_heads=H, **kw)
        finally:
            K.set_attention_variant(0)
        assert torch.equal(got, want) and torch.equal(got32, want32), mode


def test_all_pad_sample_is_zero_and_leaves_its_neighbours_alone(K):
    import torch

    S, H, Hkv, D = 129, 4, 2, 64
    C, Ckv = H * D, Hkv * D
    qkv = _qkv(S, H, Hkv, D, 3)
    vis = torch.ones(3, S, dtype=torch.bool, device="cuda")
    vis[0, :] = False
    vis[1, 40:] = False
    qb = qkv.bfloat16()
    out = K.attention(qb[..., :C], qb[..., C:C + Ckv], qb[..., C + Ckv:], H, key_mask=vis, kv_heads=Hkv)
    got = K.attention_qkv_split(qkv, H, key_mask=vis, kv_heads=Hkv)
    assert (out[0] == 0).all() and (got[0] == 0).all()
    qb2, qkv2, vis2 = qb[1:].contiguous(), qkv[1:].contiguous(), vis[1:].contiguous()
    out2 = K.attention(qb2[..., :C], qb2[..., C:C + Ckv], qb2[..., C + Ckv:], H, key_mask=vis2, kv_heads=Hkv)
    got2 = K.attention_qkv_split(qkv2, H, key_mask=vis2, kv_heads=Hkv)
    assert torch.equal(out[1:], out2) and torch.equal(got[1:], got2)
    assert torch.isfinite(out.float()).all() and torch.isfinite(got).all()


def test_gqa_launcher_rejects_bad_arguments(K):
    """H % Hkv != 0, a bias table, head dim 80, causal + key mask and a misaligned K are errors from the
    launcher (nothing is launched)."""
    import torch

    from die_amd import native

    Bn, S = 2, 40
    x = torch.zeros(Bn * S * 6 * 128 + 8, device="cuda", dtype=torch.bfloat16)
    out = torch.empty_like(x)
    table = torch.zeros(6 * S * 64, device="cuda")
    kvis = torch.zeros(Bn * 64, device="cuda")
    kend = torch.full((Bn,), S, device="cuda", dtype=torch.int32)
    L = native.kernels()
    st = torch.cuda.current_stream().cuda_stream

    def call(H=4, Hkv=2, D=64, bias=0, bias_heads=0, Sp=0, causal=0, kv=0, ke=0, koff=0):
        ldkv = (Hkv if Hkv > 0 else H) * D
        return L.die_kern_attention(native.geometry(dict(
            q=x.data_ptr(), k=x.data_ptr() + koff, v=x.data_ptr(), out=out.data_ptr(), B=Bn, S=S, H=H, D=D, ldq=H * D,
            ldk=ldkv, ldv=ldkv, ldo=H * D, scale=0.125, split=0, bias=bias, bias_heads=bias_heads, Sp=Sp, causal=causal,
            kvis=kv, kend=ke, kv_heads=Hkv)), st)

    assert call() == 0 and call(causal=1) == 0
    assert call(Sp=64, kv=kvis.data_ptr(), ke=kend.data_ptr()) == 0
    assert call(H=6, Hkv=4) != 0 and call(H=4, Hkv=3) != 0          # H % Hkv
    assert call(H=4, Hkv=5) != 0 and call(H=4, Hkv=-1) != 0
    assert call(bias=table.data_ptr(), bias_heads=1, Sp=64) != 0       # no bias table in the GQA mode
    assert call(bias=table.data_ptr(), bias_heads=4, Sp=64) != 0
    assert call(D=80) != 0 and call(D=32) != 0 and call(D=96) != 0     # head dim 64 / 128 only
    assert call(D=128) == 0
    assert call(Sp=64, causal=1, kv=kvis.data_ptr(), ke=kend.data_ptr()) != 0  # causal + key mask
    assert call(koff=8) != 0                                           # K not 16-byte aligned
    assert call(H=4, Hkv=4, bias=table.data_ptr(), bias_heads=1, Sp=64) == 0  # kv_heads = H: the per-head launch
    assert call(H=4, Hkv=0) == 0
    torch.cuda.synchronize()
    q = torch.zeros(Bn, S, 256, device="cuda", dtype=torch.bfloat16)
    kv_ = torch.zeros(Bn, S, 128, device="cuda", dtype=torch.bfloat16)
    with pytest.raises((native.NativeError, ValueError, AssertionError)):
        K.attention(q, kv_, kv_, 4, causal=True, key_mask=torch.ones(Bn, S, dtype=torch.bool, device="cuda"), kv_heads=2)
    with pytest.raises((native.NativeError, ValueError, AssertionError)):
        K.attention(q, kv_, kv_, 4, bias=torch.zeros(S, S, device="cuda"), kv_heads=2)
