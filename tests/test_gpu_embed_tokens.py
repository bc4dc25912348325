"""The embedding-lookup kernel (csrc/kernels/transformer.hip embed_tokens_kernel) against torch:
rows = table[idx(id)] + pos + type summed in fp32 -- bf16 mode bit-equal to torch's bf16 rounding of
that fp32 sum, fp32 (split) mode within the split format's 2^-16 -- the pad columns of a width that is
not a multiple of 8, the per-sample key data (kvis, kend) the attention key mask reads, and the index
clamp."""
import functools
import math

import pytest

from conftest import gpu_available

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not gpu_available(), reason="needs a GPU")]

B = 3


@pytest.fixture(scope="module")
def K():
    from die_amd.ops import kernels

    return kernels


@functools.lru_cache(maxsize=None)
def _case(V, D, S):
    """ids [B, S] with pads (id 0) -- sample 0 right-padded with a hole, sample 1 all pad, sample 2
    full -- a table, positions and a type row."""
    import torch

    g = torch.Generator(device="cuda").manual_seed(V * 1009 + D * 31 + S)
    ids = torch.randint(1, V, (B, S), device="cuda", generator=g).float()
    ids[0, S - S // 3:] = 0
    if S > 4:
        ids[0, 2] = 0  # a hole
    ids[1, :] = 0
    table = torch.randn(V, D, device="cuda", generator=g)
    pos = torch.randn(S, D, device="cuda", generator=g)
    typ = torch.randn(D, device="cuda", generator=g)
    return ids, table, pos, typ


def _ref_rows(ids, table, pos, typ):
    ref = table[ids.long()]  # fp32, the kernel's order of additions
    if pos is not None:
        ref = ref + pos
    if typ is not None:
        ref = ref + typ
    return ref


def _ref_keys(ids, S):
    import torch

    Sp = (S + 31) // 32 * 32
    vis = ids != 0
    kvis = torch.full((B, Sp), -math.inf, device="cuda")
    kvis[:, :S] = torch.where(vis, 0.0, -math.inf)
    kend = torch.tensor([int(v.nonzero().max()) + 1 if v.any() else 0 for v in vis], dtype=torch.int32, device="cuda")
    return kvis, kend


@pytest.mark.parametrize("extras", ["pos+type", "pos", "none"])
@pytest.mark.parametrize("S", [1, 48])
@pytest.mark.parametrize("D", [20, 128, 768])
@pytest.mark.parametrize("V", [37, 1000])
def test_embed_tokens_values_and_key_data(K, V, D, S, extras):
    import torch

    ids, table, pos, typ = _case(V, D, S)
    pos = pos if "pos" in extras else None
    typ = typ if "type" in extras else None
    ref = _ref_rows(ids, table, pos, typ)
    Dp = (D + 7) // 8 * 8
    rows, kvis, kend = K.embed_tokens(ids, table, pos, typ, pad_test=0)
    assert rows.shape == (B, S, Dp) and rows.dtype == torch.bfloat16
    assert torch.equal(rows[..., :D], ref.bfloat16())  # bit-equal: one fp32 sum, one rounding
    assert (rows[..., D:] == 0).all()  # pad columns up to the stored pitch
    got = K.embed_tokens(ids, table, pos, typ, pad_test=("eq", 0), split=True)[0]
    assert got.shape == (B, S, Dp) and (got[..., D:] == 0).all()
    rel = ((got[..., :D] - ref).abs() / ref.abs().clamp_min(1e-30)).max()
    assert float(rel) <= 2.0 ** -16, float(rel)
    wk, we = _ref_keys(ids, S)
    assert torch.equal(kvis, wk) and torch.equal(kend, we)
    assert kend.dtype == torch.int32 and int(kend[1]) == 0 and int(kend[2]) == S  # all-pad row, full row
    # without a pad test there is no key data
    rows2, k2, e2 = K.embed_tokens(ids, table, pos, typ)
    assert k2 is None and e2 is None and torch.equal(rows2, rows)


def test_pad_tests_greater_and_less(K):
    """visible = not (id op value): the three compares the planner roots a key mask in."""
    import torch

    ids, table, _, _ = _case(37, 128, 48)
    S = 48
    for test, vis in ((("gt", 20), ids <= 20), (("lt", 5), ids >= 5), (("eq", 7), ids != 7)):
        _, kvis, kend = K.embed_tokens(ids, table, pad_test=test)
        assert torch.equal(kvis[:, :S] == 0, vis), test
        want = [int(v.nonzero().max()) + 1 if v.any() else 0 for v in vis]
        assert kend.tolist() == want, test


def test_ids_are_read_as_fp32_not_bf16(K):
    """Ids above 256 are not bf16 values (8 significant bits): 999 must not come out as row 1000."""
    import torch

    V, D = 1000, 128
    table = torch.arange(V, device="cuda", dtype=torch.float32)[:, None].expand(V, D).contiguous()
    ids = torch.tensor([[257.0, 513.0, 999.0, 998.0]], device="cuda")
    rows = K.embed_tokens(ids, table, split=True)[0]
    assert rows[0, :, 0].tolist() == [257.0, 513.0, 999.0, 998.0]


def test_index_clamp_stays_inside_the_table(K):
    """Out-of-range ids clamp to rows 0 and V - 1.  The table handed to the kernel is the middle of a
    larger allocation with sentinel rows on both sides, so a kernel that does not clamp reads a
    sentinel (and the test fails) instead of leaving the allocation."""
    import torch

    V, D, G = 37, 128, 8
    full = torch.full((V + 2 * G, D), 12345.0, device="cuda")
    g = torch.Generator(device="cuda").manual_seed(3)
    full[G:G + V] = torch.randn(V, D, device="cuda", generator=g)
    table = full[G:G + V]  # read in place: a view with 16-byte aligned rows
    assert table.data_ptr() == full.data_ptr() + G * D * 4
    inf, nan = float("inf"), float("nan")
    ids = torch.tensor([[-1.0, float(V), float(V + 3), -0.0, 0.9, V - 0.5, 1e9, inf, -inf, nan, -3e38, 3e38]], device="cuda")
    want = torch.tensor([0, V - 1, V - 1, 0, 0, V - 1, V - 1, V - 1, 0, 0, 0, V - 1], device="cuda")
    for split in (False, True):
        rows = K.embed_tokens(ids, table, split=split)[0]
        assert not (rows.float() == 12345.0).any()
        ref = table[want][None]
        if split:
            assert float(((rows - ref).abs() / ref.abs().clamp_min(1e-30)).max()) <= 2.0 ** -16
        else:
            assert torch.equal(rows, ref.bfloat16())


def test_embed_tokens_rejects_bad_arguments(K):
    import torch

    from die_amd import native

    L = native.kernels()
    st = torch.cuda.current_stream().cuda_stream
    Bn, S, V, C = 2, 40, 16, 32
    ids = torch.zeros(Bn, S, device="cuda")
    table = torch.zeros(V, C, device="cuda")
    out = torch.empty(Bn, S, C, device="cuda", dtype=torch.bfloat16)
    kvis = torch.empty(Bn, 64, device="cuda")
    kend = torch.empty(Bn, device="cuda", dtype=torch.int32)

    def call(C=C, ldt=C, Sp=64, kv=kvis.data_ptr(), ke=kend.data_ptr(), tab=table.data_ptr(), op=0):
        return L.die_kern_embed_tokens(native.geometry(dict(
            ids=ids.data_ptr(), table=tab, ldt=ldt, pos=0, ttab=0, out=out.data_ptr(), B=Bn, S=S, V=V, C=C, split=0, kvis=kv,
            kend=ke, Sp=Sp, pad_op=op, pad_c=0.0, pad_neg=1, pad_trunc=0)), st)

    assert call() == 0
    assert call(C=20) != 0 and call(ldt=16) != 0 and call(ldt=34) != 0  # stored width % 8, table pitch
    assert call(Sp=40) != 0 and call(Sp=96) != 0  # Sp must be 64 for S = 40
    assert call(ke=0) != 0 and call(kv=0) != 0  # key data: both or neither
    assert call(kv=0, ke=0, Sp=0) == 0
    assert call(tab=table.data_ptr() + 4) != 0 and call(op=3) != 0
    torch.cuda.synchronize()
