"""The embedding kernel of models with attention_mask / token_type_ids graph inputs
(csrc/kernels/transformer.hip embed_inputs_kernel) against torch.  Every sample is one packed request
row [K * S] holding the ids, the mask and the type ids as segments, so each is read with the row pitch
K * S, not S:  rows = table[idx(ids)] + pos + type_table[idx(types)] summed in fp32 in that order --
bf16 mode bit-equal to torch's bf16 rounding of that sum, fp32 (split) mode within the split format's
2^-16 -- and the key data (kvis, kend) comes from the mask segment, not from the ids."""
import functools
import math

import pytest

from conftest import gpu_available

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not gpu_available(), reason="needs a GPU")]

B, V = 3, 37
ORDERS = {"ids|mask|types": ("ids", "mask", "types"), "mask|types|ids": ("mask", "types", "ids")}


@pytest.fixture(scope="module")
def K():
    from die_amd.ops import kernels

    return kernels


@functools.lru_cache(maxsize=None)
def _case(D, S, T):
    """Segments [B, S] and the tables.  The mask: sample 0 right-padded with a hole, sample 1 all
    hidden, sample 2 full.  The ids disagree with it on purpose: one VISIBLE token has id 0 and every
    HIDDEN token a non-zero id, so key data taken from an `id != 0` test would be wrong."""
    import torch

    g = torch.Generator(device="cuda").manual_seed(D * 31 + S * 7 + T)
    ids = torch.randint(1, V, (B, S), device="cuda", generator=g).float()
    mask = torch.ones(B, S, device="cuda")
    mask[0, S - S // 3:] = 0
    if S > 4:
        mask[0, 2] = 0  # a hole
        ids[0, 1] = 0  # visible, id 0
    mask[1, :] = 0
    ids[2, S - 1] = 0  # visible, id 0 (the only key of sample 2 when S = 1)
    types = torch.randint(0, T, (B, S), device="cuda", generator=g).float()
    table = torch.randn(V, D, device="cuda", generator=g)
    pos = torch.randn(S, D, device="cuda", generator=g)
    ttab = torch.randn(T, D, device="cuda", generator=g)
    return dict(ids=ids, mask=mask, types=types), table, pos, ttab


def _pack(seg, order, S):
    import torch

    rows = torch.cat([seg[r] for r in order], dim=1).contiguous()
    return rows, dict(S=S, **{r: order.index(r) * S if r in order else None for r in ("ids", "types", "mask")})


def _ref_keys(vis, S):
    import torch

    Sp = (S + 31) // 32 * 32
    kvis = torch.full((vis.shape[0], Sp), -math.inf, device="cuda")
    kvis[:, :S] = torch.where(vis, 0.0, -math.inf)
    kend = torch.tensor([int(v.nonzero().max()) + 1 if v.any() else 0 for v in vis], dtype=torch.int32, device="cuda")
    return kvis, kend


@pytest.mark.parametrize("order", list(ORDERS))
@pytest.mark.parametrize("T", [1, 2, 3])
@pytest.mark.parametrize("S", [1, 33, 48])
@pytest.mark.parametrize("D", [20, 128])
def test_embed_inputs_values_and_key_data(K, D, S, T, order):
    import torch

    seg, table, pos, ttab = _case(D, S, T)
    rows_in, packed = _pack(seg, ORDERS[order], S)
    assert rows_in.shape == (B, 3 * S)
    ref = table[seg["ids"].long()] + pos + ttab[seg["types"].long()]  # fp32, the kernel's order of additions
    Dp = (D + 7) // 8 * 8
    rows, kvis, kend = K.embed_tokens(rows_in, table, pos, type_table=ttab, packed=packed)
    assert rows.shape == (B, S, Dp) and rows.dtype == torch.bfloat16
    assert torch.equal(rows[..., :D], ref.bfloat16())  # bit-equal: one fp32 sum, one rounding
    assert (rows[..., D:] == 0).all()  # pad columns up to the stored pitch
    got = K.embed_tokens(rows_in, table, pos, type_table=ttab, packed=packed, split=True)[0]
    assert got.shape == (B, S, Dp) and (got[..., D:] == 0).all()
    rel = ((got[..., :D] - ref).abs() / ref.abs().clamp_min(1e-30)).max()
    assert float(rel) <= 2.0 ** -16, float(rel)
    wk, we = _ref_keys(seg["mask"] != 0, S)
    assert torch.equal(kvis, wk) and torch.equal(kend, we)
    assert kend.dtype == torch.int32 and int(kend[1]) == 0 and int(kend[2]) == S  # all hidden, full
    assert not torch.equal(kvis, _ref_keys(seg["ids"] != 0, S)[0])  # the ids would have given other key data


def test_mask_values_other_than_zero_and_one(K):
    """Non-zero is visible: 2, -1 and 0.5 count as 1; with the truncated test (an integer-declared
    mask input) 0.5 is trunc(0.5) = 0, hidden.  NaN compares unequal to 0: visible."""
    import torch

    S = 8
    seg, table, pos, ttab = _case(128, 48, 2)
    ids = seg["ids"][:1, :S].contiguous()
    mask = torch.tensor([[2.0, -1.0, 0.5, 0.0, -0.0, 1.0, -0.5, 0.0]], device="cuda")
    for trunc, vis in ((False, [1, 1, 1, 0, 0, 1, 1, 0]), (True, [1, 1, 0, 0, 0, 1, 0, 0])):
        _, kvis, kend = K.embed_tokens(ids, table, mask=mask, mask_trunc=trunc)
        assert (kvis[0, :S] == 0).int().tolist() == vis, trunc
        assert (kvis[0, S:] == -math.inf).all()
        assert int(kend[0]) == max(i + 1 for i, v in enumerate(vis) if v)


def test_type_index_clamp_stays_inside_the_table(K):
    """Type ids -1, T and NaN clamp to rows 0, T - 1 and 0.  The type table is the middle of a larger
    allocation with sentinel rows on both sides: a kernel that does not clamp reads a sentinel."""
    import torch

    D, G = 128, 8
    for T in (1, 2, 3):
        full = torch.full((T + 2 * G, D), 12345.0, device="cuda")
        g = torch.Generator(device="cuda").manual_seed(T)
        full[G:G + T] = torch.randn(T, D, device="cuda", generator=g)
        ttab = full[G:G + T]  # read in place: a view with 16-byte aligned rows
        assert ttab.data_ptr() == full.data_ptr() + G * D * 4
        table = torch.zeros(V, D, device="cuda")
        nan, inf = float("nan"), float("inf")
        types = torch.tensor([[-1.0, float(T), nan, 0.0, T - 1.0, 1e9, -inf, inf, T + 3.0]], device="cuda")
        want = torch.tensor([0, T - 1, 0, 0, T - 1, T - 1, 0, T - 1, T - 1], device="cuda")
        ids = torch.ones_like(types)
        for split in (False, True):
            rows = K.embed_tokens(ids, table, types=types, type_table=ttab, split=split)[0]
            assert not (rows.float() == 12345.0).any()
            ref = ttab[want][None]
            if split:
                assert float(((rows - ref).abs() / ref.abs().clamp_min(1e-30)).max()) <= 2.0 ** -16
            else:
                assert torch.equal(rows, ref.bfloat16())


@pytest.mark.parametrize("S,D", [(1, 20), (33, 128), (48, 20)])
def test_no_mask_no_types_is_the_single_input_kernel(K, S, D):
    """Without a mask and a type input the packed entry point gives the bits of the single-input one:
    rows, and key data from the pad test on the ids (read with the row pitch)."""
    import torch

    seg, table, pos, ttab = _case(D, S, 2)
    ids = seg["ids"]
    old = K.embed_tokens(ids, table, pos, ttab[0], pad_test=0)
    for split in (False, True):
        want = K.embed_tokens(ids, table, pos, ttab[0], pad_test=0, split=split)
        # the ids as the middle segment of a wider row: pitch 3 S
        rows_in = torch.cat([seg["mask"], ids, seg["types"]], dim=1).contiguous()
        got = K.embed_tokens(rows_in, table, pos, ttab[0], pad_test=0, split=split, packed=dict(S=S, ids=S))
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], old[1]) and torch.equal(got[2], old[2])


def test_embed_inputs_rejects_bad_arguments(K):
    import torch

    from die_amd import native

    L = native.kernels()
    st = torch.cuda.current_stream().cuda_stream
    Bn, S, C, T = 2, 40, 32, 2
    rows_in = torch.zeros(Bn, 3 * S, device="cuda")
    table = torch.zeros(V, C, device="cuda")
    ttab = torch.zeros(T + 1, C, device="cuda")
    out = torch.full((Bn, S, C), 7.0, device="cuda", dtype=torch.bfloat16)
    kvis = torch.full((Bn, 64), 7.0, device="cuda")
    kend = torch.full((Bn,), 7, device="cuda", dtype=torch.int32)
    base = rows_in.data_ptr()

    def call(ld=3 * S, types=base + 4 * 2 * S, mask=base + 4 * S, tt=ttab.data_ptr(), T=T, ldtt=C, kv=kvis.data_ptr(),
             ke=kend.data_ptr(), Sp=64):
        return L.die_kern_embed_tokens(native.geometry(dict(
            ids=base, types=types, mask=mask, ld_in=ld, table=table.data_ptr(), ldt=C, pos=0, ttab=tt, ldtt=ldtt, T=T,
            out=out.data_ptr(), B=Bn, S=S, V=V, C=C, split=0, kvis=kv, kend=ke, Sp=Sp, pad_op=0, pad_c=0.0, pad_neg=1,
            pad_trunc=0)), st)

    bad = [call(ld=S - 1), call(T=0), call(T=-1), call(tt=ttab.data_ptr() + 4), call(tt=0), call(ldtt=16), call(ldtt=34),
           call(ke=0), call(kv=0), call(kv=0, ke=0, Sp=0), call(Sp=40)]  # (a mask without key data has no reader)
    torch.cuda.synchronize()
    assert all(rc != 0 for rc in bad), bad
    # nothing was launched: the outputs still hold their fill
    assert (out == 7.0).all() and (kvis == 7.0).all() and (kend == 7).all()
    assert call() == 0 and call(ld=S, types=0, mask=0, tt=0, T=0) == 0  # ld_in = S is the lower bound
    torch.cuda.synchronize()
    assert (out == 0).all() and (kvis[:, :S] == -math.inf).all()  # table of zeros; mask of zeros: all hidden
