"""pool_tokens (csrc/kernels/transformer.hip): the masked mean over a request's visible tokens and the
L2 normalisation after it, against float64 numpy on the stored inputs (bf16 rows; hi + lo planes in
fp32 mode).  fp32 output bar 2e-5 rel-L2 in both modes (docs/DESIGN.md section 3, one layer: an fp32
sum of <= 160 terms and one division sit well inside it), bf16 rows 3e-2 (the project's bf16 bar)."""
import numpy as np
import pytest

from conftest import gpu_available

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not gpu_available(), reason="needs a GPU")]

SEQS = (1, 31, 32, 33, 48, 160)
DIMS = (8, 36, 128, 200)  # 36 is stored as 40; 200 = four column blocks, the last partial
BATCHES = (1, 5)
F32_BAR, BF16_BAR, NORM_BAR = 2e-5, 3e-2, 1e-5


def _visible(B, S):
    """Lengths of models/generic.py synthetic_lengths (1, 32, S, 45, 33 in turn) clamped to S, a hole
    in every third sample."""
    from die_amd.models import generic as G

    vis = np.zeros((B, S), bool)
    for i, n in enumerate(G.synthetic_lengths("sbert_ids_hf", B)):
        n = min(n, S)
        vis[i, :n] = True
        if i % 3 == 2 and n >= 3:
            vis[i, n // 2] = False
    return vis


def _rows(B, S, D, split, seed):
    """(device input [B, S, C], its stored values as float64 [B, S, D]); pad columns hold 0."""
    import torch

    from die_amd.ops import kernels as K

    C = (D + 7) // 8 * 8
    x = torch.zeros((B, S, C), dtype=torch.float32)
    x[:, :, :D] = torch.from_numpy(np.random.default_rng(seed).standard_normal((B, S, D)).astype(np.float32)) + 0.25
    if split:
        xin = x.cuda()
        stored = K.join_planes(K.split_planes(xin)).cpu().double().numpy()
    else:
        xin = x.cuda().to(torch.bfloat16)
        stored = xin.cpu().double().numpy()
    return xin, stored[:, :, :D]


def _ref(stored, vis, clip_min, normalize, eps):
    w = np.ones(stored.shape[:2]) if vis is None else vis.astype(np.float64)
    cnt = w.sum(1, keepdims=True)
    v = (stored * w[:, :, None]).sum(1) / np.maximum(np.maximum(cnt, clip_min), 1e-300)
    v[cnt[:, 0] == 0] = 0.0
    if normalize:
        n = np.maximum(np.linalg.norm(v, axis=1, keepdims=True), eps)
        v = np.where(n > 0, v / np.where(n > 0, n, 1.0), 0.0)
    return v


def _rel(a, b):
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))


def _check(got_rows, got32, ref, D, split, normalize, what):
    g32 = got32.cpu().double().numpy()
    assert g32.shape == ref.shape and np.isfinite(g32).all(), what
    err = _rel(g32, ref)
    rows = got_rows.float().cpu().double().numpy()
    assert (rows[:, D:] == 0).all(), what  # stored pad columns
    rerr = _rel(rows[:, :D], ref)
    nerr = float(np.abs(np.linalg.norm(g32, axis=1) - 1.0).max()) if normalize else 0.0
    print(what, "fp32 out rel-L2 %.2e, rows rel-L2 %.2e, | |v| - 1 | %.2e" % (err, rerr, nerr))
    assert err <= F32_BAR, (what, err)
    assert rerr <= (F32_BAR if split else BF16_BAR), (what, rerr)
    assert nerr <= NORM_BAR, (what, nerr)


@pytest.mark.parametrize("D", DIMS)
@pytest.mark.parametrize("split", [False, True])
def test_masked_mean_and_normalisation_against_float64(native, D, split):
    import torch

    from die_amd.ops import kernels as K

    for B in BATCHES:
        counters = torch.zeros((B,), dtype=torch.int32, device="cuda")
        for S in SEQS:
            x, stored = _rows(B, S, D, split, seed=S * 7 + B)
            vis = _visible(B, S)
            km = K.key_mask_data(torch.from_numpy(vis).cuda())
            # every S: plain masked mean with no clip, and the full op; the mixed pairs at one S
            cases = [(0.0, False), (1e-9, True)] + ([(1e-9, False), (0.0, True)] if S == 33 else [])
            for clip_min, normalize in cases:
                what = "B%d S%d D%d %s clip %g norm %d" % (B, S, D, "fp32" if split else "bf16", clip_min, normalize)
                rows, out32 = K.pool_tokens(x, km, clip_min=clip_min, normalize=normalize, eps=1e-12, split=split, dim=D,
                                            counters=counters)
                _check(rows, out32, _ref(stored, vis, clip_min, normalize, 1e-12), D, split, normalize, what)
                # the hand-off sums in slice order: a second launch is bitwise equal, on the same tickets
                rows2, out32b = K.pool_tokens(x, km, clip_min=clip_min, normalize=normalize, eps=1e-12, split=split,
                                              dim=D, counters=counters)
                assert torch.equal(out32, out32b) and torch.equal(rows, rows2), what
                assert int(counters.abs().sum()) == 0, what  # left at 0 for the next launch


@pytest.mark.parametrize("split", [False, True])
def test_all_pad_sample_gives_zeros_and_leaves_its_neighbours(native, split):
    import torch

    from die_amd.ops import kernels as K

    B, S, D = 5, 48, 200
    x, stored = _rows(B, S, D, split, seed=11)
    vis = _visible(B, S)
    base = K.pool_tokens(x, K.key_mask_data(torch.from_numpy(vis).cuda()), clip_min=0.0, normalize=True, split=split, dim=D)
    vis0 = vis.copy()
    vis0[2] = False  # no visible token at all: kend = 0
    for clip_min in (0.0, 1e-9):
        rows, out32 = K.pool_tokens(x, K.key_mask_data(torch.from_numpy(vis0).cuda()), clip_min=clip_min, normalize=True,
                                    split=split, dim=D)
        assert (out32[2] == 0).all() and (rows[2] == 0).all()
        keep = [0, 1, 3, 4]
        assert torch.equal(out32[keep], base[1][keep]) and torch.equal(rows[keep], base[0][keep])
        _check(rows, out32, _ref(stored, vis0, clip_min, True, 1e-12), D, split, False, "all-pad sample, clip %g" % clip_min)


@pytest.mark.parametrize("split", [False, True])
@pytest.mark.parametrize("S,D", [(33, 36), (160, 200), (1, 128)])
def test_unmasked_mean(native, split, S, D):
    from die_amd.ops import kernels as K

    x, stored = _rows(5, S, D, split, seed=5)
    for normalize in (False, True):
        rows, out32 = K.pool_tokens(x, None, normalize=normalize, split=split, dim=D)
        _check(rows, out32, _ref(stored, None, 0.0, normalize, 1e-12), D, split, normalize,
               "unmasked S%d D%d norm %d" % (S, D, normalize))


@pytest.mark.parametrize("split", [False, True])
@pytest.mark.parametrize("D", DIMS)
def test_row_normalisation_alone(native, split, D):
    """S = 1, no mask: v / max(|v|, eps) of each row; a zero row gives zeros (0 / 0 guarded), a row
    shorter than eps is divided by eps."""
    import torch

    from die_amd.ops import kernels as K

    x, stored = _rows(5, 1, D, split, seed=9)
    x[3] = 0
    stored[3] = 0
    rows, out32 = K.pool_tokens(x, None, normalize=True, eps=0.0, split=split, dim=D)
    assert (out32[3] == 0).all() and (rows[3] == 0).all() and bool(torch.isfinite(out32).all())
    ref = _ref(stored, None, 0.0, True, 0.0)
    keep = [0, 1, 2, 4]
    _check(rows[keep], out32[keep], ref[keep], D, split, True, "S1 D%d" % D)
    big = 1e3  # eps above every row's length: plain division by eps
    _, out_eps = K.pool_tokens(x, None, normalize=True, eps=big, split=split, dim=D)
    assert _rel(out_eps.cpu().double().numpy(), stored[:, 0] / big) <= F32_BAR


def test_bad_arguments_launch_nothing(native):
    import torch

    from die_amd import native as N
    from die_amd.ops import kernels as K

    x = torch.zeros((2, 4, 16), dtype=torch.bfloat16, device="cuda")
    with pytest.raises(N.NativeError):
        K.pool_tokens(x, None, dim=17)  # more logical than stored columns
    with pytest.raises(N.NativeError):
        K.pool_tokens(x, None, clip_min=-1.0)
    kvis, kend = K.key_mask_data(torch.ones((2, 4), dtype=torch.bool, device="cuda"))
    with pytest.raises(N.NativeError):
        K.pool_tokens(x, (kvis[:, :16].contiguous(), kend))  # Sp is not S rounded up to 32
    wide = torch.zeros((2, 4, 128), dtype=torch.bfloat16, device="cuda")
    with pytest.raises(N.NativeError):  # a normalised row over two column blocks needs B tickets
        K.pool_tokens(wide, None, normalize=True, counters=torch.zeros((1,), dtype=torch.int32, device="cuda"))
