"""layernorm_rows in its RMS mode (csrc/kernels/transformer.hip) against float64 numpy on the stored
inputs (bf16 values; hi + lo planes in fp32 mode): y = x * rsqrt(mean(x^2) + eps) * gamma, no mean, no
beta.  Bars: the project's for stored rows -- 2e-5 rel-L2 in fp32 (split) mode, 3e-2 for bf16
(tests/test_gpu_pool_tokens.py); an fp32 sum of <= 2560 squares and a product sit well inside.
Every row carries a mean of +3, so a mean subtracted by mistake shows as an error of order 1."""
import numpy as np
import pytest

from conftest import gpu_available

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not gpu_available(), reason="needs a GPU")]

WIDTHS = (128, 200, 768, 2560)  # one chunk per lane, a partial last lane, the 32-lane ViT shape, the block-per-row kernel
ROWS = (1, 5, 257)
F32_BAR, BF16_BAR = 2e-5, 3e-2
EPS = 1e-6


def _inputs(rows, C, Cl, split, seed):
    """(device x [rows, C] with the pad columns holding 5 -- out of the statistics whatever they hold --,
    gamma [C] with zeros in the pad columns, stored x float64 [rows, Cl], gamma float64 [Cl])."""
    import torch

    from die_amd.ops import kernels as K

    rng = np.random.default_rng(seed)
    x = torch.full((rows, C), 5.0, dtype=torch.float32)
    x[:, :Cl] = torch.from_numpy((3.0 + rng.standard_normal((rows, Cl))).astype(np.float32))
    g = np.zeros(C, np.float32)
    g[:Cl] = 1.0 + 0.1 * rng.standard_normal(Cl)
    if split:
        xin = x.cuda()
        stored = K.join_planes(K.split_planes(xin)).cpu().double().numpy()
    else:
        xin = x.cuda().to(torch.bfloat16)
        stored = xin.cpu().double().numpy()
    return xin, torch.from_numpy(g).cuda(), stored[:, :Cl], g[:Cl].astype(np.float64)


def _ref(stored, g):
    inv = 1.0 / np.sqrt((stored ** 2).mean(1, keepdims=True) + float(np.float32(EPS)))
    return stored * inv * g, inv[:, 0]


def _rel(a, b):
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))


@pytest.mark.parametrize("C,Cl", [(c, c) for c in WIDTHS] + [(40, 36)])
@pytest.mark.parametrize("split", [False, True])
def test_rmsnorm_against_float64(native, C, Cl, split):
    from die_amd.ops import kernels as K

    for rows in ROWS:
        x, g, stored, g64 = _inputs(rows, C, Cl, split, seed=C + rows)
        ref, inv = _ref(stored, g64)
        got = K.layernorm_rows(x, g, None, eps=EPS, split=split, cl=Cl, rms=True).float().cpu().double().numpy()
        err = _rel(got[:, :Cl], ref)
        what = "rows %d C %d Cl %d %s" % (rows, C, Cl, "fp32" if split else "bf16")
        print(what, "rel-L2 %.2e" % err)
        assert np.isfinite(got).all() and err <= (F32_BAR if split else BF16_BAR), (what, err)
        assert (got[:, Cl:] == 0).all(), what  # stored pad columns are written 0
        # statistics mode: (0, rstd) per row, fp32 in both modes
        st = K.layernorm_rows(x, g, None, eps=EPS, split=split, cl=Cl, rms=True, stats=True).cpu().double().numpy()
        assert st.shape == (rows, 2) and (st[:, 0] == 0).all(), what
        serr = _rel(st[:, 1], inv)
        print(what, "rstd rel-L2 %.2e" % serr)
        assert serr <= F32_BAR, (what, serr)


@pytest.mark.parametrize("C", (128, 768, 2560))
@pytest.mark.parametrize("split", [False, True])
def test_measurement_variants_agree_in_rms_mode(native, C, split):
    """variant 1 (16 lanes x 6 chunks, C <= 768) and 2 (block per row) compute the same function."""
    from die_amd.ops import kernels as K

    x, g, stored, g64 = _inputs(5, C, C, split, seed=C)
    ref, _ = _ref(stored, g64)
    for variant in ((1, 2) if C <= 768 else (2,)):
        got = K.layernorm_rows(x, g, None, eps=EPS, split=split, variant=variant, rms=True).float().cpu().double().numpy()
        assert _rel(got, ref) <= (F32_BAR if split else BF16_BAR), (C, variant)


@pytest.mark.parametrize("C,Cl", [(c, c) for c in WIDTHS] + [(40, 36)])
@pytest.mark.parametrize("split", [False, True])
def test_layernorm_mode_is_unchanged_bit_for_bit(native, C, Cl, split):
    """rms = 0 through the new entry point equals the entry point that existed before, bit for bit, and
    differs from the RMS result (the rows have a mean)."""
    import torch

    from die_amd.ops import kernels as K

    x, g, _, _ = _inputs(257, C, Cl, split, seed=C + 1)
    beta = torch.from_numpy((0.1 * np.random.default_rng(C).standard_normal(C)).astype(np.float32)).cuda()
    beta[Cl:] = 0
    new = K.layernorm_rows(x, g, beta, eps=1e-5, split=split, cl=Cl, rms=False)
    if Cl == C:  # the earlier entry point has no logical-width argument
        old = K.layernorm(x, g, beta, eps=1e-5, split=split)
        assert torch.equal(new, old)
    rms = K.layernorm_rows(x, g, beta, eps=1e-5, split=split, cl=Cl, rms=True)
    assert not torch.equal(new, rms)
    # LayerNorm against float64 here too: the mean is subtracted in this mode
    xs = (K.join_planes(K.split_planes(x)) if split else x.float()).cpu().double().numpy()[:, :Cl]
    mu = xs.mean(1, keepdims=True)
    ref = (xs - mu) / np.sqrt(((xs - mu) ** 2).mean(1, keepdims=True) + 1e-5) * g.cpu().double().numpy()[:Cl] \
        + beta.cpu().double().numpy()[:Cl]
    assert _rel(new.float().cpu().double().numpy()[:, :Cl], ref) <= (F32_BAR if split else BF16_BAR)
