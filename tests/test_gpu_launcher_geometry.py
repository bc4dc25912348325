"""The JSON entry points of the token-model launchers (csrc/capi/capi_kernels.cpp die_kern_attention,
die_kern_embed_tokens, die_kern_pool_tokens): the keys of the geometry are the members of the
launcher's argument struct, a missing key is the member's default and an unknown key is an error, not
a default.  And the two defaults the Python wrappers lean on: kv_heads = 0 is the multi-head launch,
ld_in = 0 the single-input embedding kernel, whose rows the packed-row kernel reproduces."""
import pytest

from conftest import gpu_available

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not gpu_available(), reason="needs a GPU")]


@pytest.fixture(scope="module")
def K():
    from die_amd.ops import kernels

    return kernels


def test_geometry_keys_and_defaults(K):
    import torch

    from die_amd import native

    L = native.kernels()
    st = torch.cuda.current_stream().cuda_stream
    B, S, H, D = 2, 40, 4, 64
    C = H * D
    g = torch.Generator(device="cuda").manual_seed(7)
    q, k, v = (torch.randn(B, S, C, device="cuda", generator=g).to(torch.bfloat16) for _ in range(3))
    out = torch.empty_like(q)
    attn = dict(q=q.data_ptr(), k=k.data_ptr(), v=v.data_ptr(), out=out.data_ptr(), B=B, S=S, H=H, D=D, ldq=C, ldk=C,
                ldv=C, ldo=C, scale=0.125)
    V, Dm = 50, 24
    ids = torch.randint(0, V, (B, S), device="cuda", generator=g).float()
    table = torch.randn(V, C, device="cuda", generator=g)
    rows = torch.empty(B, S, C, device="cuda", dtype=torch.bfloat16)
    embed = dict(ids=ids.data_ptr(), table=table.data_ptr(), ldt=C, out=rows.data_ptr(), B=B, S=S, V=V, C=C)
    pooled = torch.empty(B, C, device="cuda")
    pool = dict(x=q.data_ptr(), out_f32=pooled.data_ptr(), B=B, S=S, C=C, D=C)
    for fn, geom, typo in ((L.die_kern_attention, attn, "kvheads"), (L.die_kern_embed_tokens, embed, "ldin"),
                           (L.die_kern_pool_tokens, pool, "normalise")):
        assert fn(native.geometry(geom), st) == 0  # the keys left out are the members' defaults
        assert fn(native.geometry(dict(geom, **{typo: 0})), st) != 0
    torch.cuda.synchronize()

    want = K.attention(q, k, v, H)
    assert torch.equal(K.attention(q, k, v, H, kv_heads=H), want)
    got = torch.empty_like(want)
    K.attention_launch(q.data_ptr(), k.data_ptr(), v.data_ptr(), got.data_ptr(), B, S, H, D, C, C, C, C, 0.125, kv_heads=0)
    assert torch.equal(got, want) and torch.equal(out, want)

    small = torch.randn(V, Dm, device="cuda", generator=g)
    dense = K.embed_tokens(ids, small)[0]
    packed = K.embed_tokens(ids, small, packed=dict(S=S, ids=0, types=None, mask=None))[0]
    assert tuple(dense.shape) == (B, S, Dm) and torch.equal(dense, packed)
