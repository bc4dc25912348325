"""Shape grid, float64 references and element-wise bounds for the dense-rows GEMM path of the conv
kernels (a plain helper module: test_gemm_rows_bound.py runs it on the CPU, test_gpu_gemm_rows.py on
the kernels).  Dense rows = a 1x1 / stride 1 / no-pad conv, x[M][K] . W[N][K]^T: MODE 0 of the
register-staged and LDS-DMA loops, the 256x128 wide tile (cfg 28), the skinny GEMM (cfg 32), the
LayerNorm fold (row_stats / row_parts + col_sum), the statistics epilogue (stats_out), the GELU and
Clip epilogues and the panel-major tile orders.

The check is conv_geometry's: every output element against float64 under T = eps * S, S the same
product on the magnitudes; preround / check / storage / bound are that module's, used through a case
tuple with KH = KW = 1 and Cin = K, so eps = 2 * (K + splits + 2 + extra) * 2^-24 (+ 2^-16 in fp32
mode).

A case is (B, S, K, N), launched as x[B, S, 1, K] (H = S, W = 1, M = B * S), so that the device-side
live batch counts samples of S rows."""
import functools
import math

import numpy as np
import torch

import conv_geometry as cg

U = 2.0 ** -24  # fp32 unit roundoff

# (B, S, K, N): the smallest shapes at which each path of the dense-rows code can go wrong
CASES = [
    (1, 1, 256, 8),      # one row, one 8-channel group: skinny takes it, the N tile nearly empty
    (4, 8, 256, 40),     # M = 32: skinny's last legal M; N < 64, N % 8 == 0
    (3, 11, 256, 72),    # M = 33: skinny must refuse; ragged second N tile
    (5, 13, 64, 64),     # M = 65: one K-step (splits clamp to 1), one row into the second 64-row tile
    (3, 43, 320, 136),   # M = 129: 5 K-steps (splits 3 -> 2 + 2 + 1, splits 4 -> 3 slices), ragged M and N tiles
    (257, 1, 128, 264),  # one row past the wide tile; 5 N-tiles of 64, 3 of 128: partial last panel at orders 3 / 4
    (6, 5, 72, 64),      # K % 64 != 0, Cin % 8 == 0: register dense path only, Kpad = 128
    (2, 9, 20, 12),      # Cin % 8 != 0 (4-wide loads), N % 8 != 0 (register epilogue), no split-K
    (7, 10, 1152, 64),   # 18 statistics groups: 9 per thread at TPR = 2, the row_parts overflow loop
    (2, 35, 128, 128),   # 2 statistics groups: fewer than TPR at 64-row tiles (empty runs); stats_out at 2 groups
]

FOLD_KS = (64, 128, 320, 1152)
FOLD_OFFSETS = (0.0, 10.0, 30.0)  # row DC offsets, in row sigmas
FOLD_CASES = [c for c in CASES if c[2] in FOLD_KS]
LN_EPS = float(np.float32(1e-5))

TILES = [(128, 128), (128, 64), (64, 128), (64, 64)]  # kernels.h TileCfg: cfg = tile + 4 * variant
LDS_BYTES = 160 * 1024
NUM_CFGS = 40
CFG_WIDE, CFG_SKINNY = 28, 32

# The GELU epilogue against float64 0.5 v (1 + erf(v / sqrt 2)) of the kernel's own fp32 pre-activation
# v: |err| / max(1, |v|).  Measured on an MI355X over all cases, both precisions: 1.13e-7 (the device
# erfc polynomial, a reciprocal, an exp2 and the few fp32 operations around them); asserted: 4x that,
# rounded up to a power of two.
GELU_MEASURED = 1.13e-7
GELU_BAR = 2.0 ** -21  # 4.77e-7 >= 4 * 1.13e-7


def case_id(case):
    return "m%dx%d_k%d_n%d" % case


def conv_case(case):
    """The conv_geometry case tuple of a dense-rows case (for conv_geometry.bound)."""
    B, S, K, N = case
    return (B, S, 1, K, N, 1, 1, 1, (0, 0, 0, 0), 1)


def bound(case, splits=1, split=False, extra=0):
    return cg.bound(conv_case(case), splits, split, extra)


def _rows(t, case):
    """[M, N] -> the NHWC shape the kernel writes, [B, S, 1, N]."""
    return t.reshape(case[0], case[1], 1, -1)


def gelu_erf(v):
    return 0.5 * v * (1.0 + torch.erf(v / math.sqrt(2.0)))


def gelu_tanh(v):
    return 0.5 * v * (1.0 + torch.tanh(math.sqrt(2.0 / math.pi) * (v + 0.044715 * v ** 3)))


@functools.lru_cache(maxsize=None)
def problem(case, split):
    """The case's operands (CPU, float64 values the kernel's storage holds exactly), references and S,
    computed once and shared; callers must not modify them.
    x [M, K], w [N, K], res [B, S, 1, N] rounded to the storage format; bias, scale2, shift2 fp32 values;
    ref, S, v, Sv, u, Su as conv_geometry.problem gives them, [B, S, 1, N]."""
    B, S, K, N = case
    M = B * S
    g = torch.Generator().manual_seed(2000 + CASES.index(case))
    x = cg.preround(torch.randn(M, K, generator=g), split)
    w = cg.preround(torch.randn(N, K, generator=g) / K ** 0.5, split)
    bias = torch.randn(N, generator=g).float().double()
    res = _rows(cg.preround(torch.randn(M, N, generator=g), split), case)
    scale2 = (torch.rand(N, generator=g) + 0.5).float().double()
    shift2 = torch.randn(N, generator=g).float().double()
    ref = _rows(x @ w.t() + bias, case)
    S_ = _rows(x.abs() @ w.abs().t() + bias.abs(), case)
    v = torch.relu(ref + res)
    Sv = S_ + res.abs()
    u = torch.relu(v * scale2 + shift2)
    Su = Sv * scale2.abs() + shift2.abs()
    # Clip edges: about a third of the outputs clip on each side
    srt = ref.flatten().sort().values
    clip_lo = float(np.float32(srt[srt.numel() // 3]))
    clip_hi = float(np.float32(srt[(2 * srt.numel()) // 3]))
    if not clip_lo < clip_hi:  # one row x 8 channels can tie
        clip_lo, clip_hi = clip_lo - 0.25, clip_hi + 0.25
    return dict(x=x, w=w, bias=bias, res=res, scale2=scale2, shift2=shift2, ref=ref, S=S_, v=v, Sv=Sv, u=u, Su=Su,
                clip_lo=clip_lo, clip_hi=clip_hi)


# ---- which launch configs take a case (kernels.h TileCfg, launch_cfg / launch_wide / launch_tile_skinny,
# ---- the guards of conv_igemm), written from those rules and not by running the kernels ----------------

def expected_cfgs(case, split, splits, *, stats_out=False, row_parts=False, sk=False, tail=False):
    """The launch configs that take the dense-rows case at `splits` K-slices (either reduction form).
    sk / tail: a stream-K / tail split-K launch (the LDS-DMA loops only; tail needs >= 2 K-steps)."""
    B, S, K, N = case
    M = B * S
    if K % 4:
        return []  # 4-wide loads at the least
    if splits > 1 and N % 8:
        return []  # split-K partials are 8-channel groups
    if stats_out and N % 64:
        return []  # whole 64-column groups
    if row_parts and (not split or N % 8 or K % 64):
        return []
    nk = (K + 63) // 64
    if tail and (splits < 2 or min(splits, nk) < 2):
        return []  # nothing to cut
    if sk and (N % 8 or row_parts or stats_out or tail):
        return []
    cfgs = []
    if not (sk or tail):
        cfgs += [0, 1, 2, 3]  # variant 0, the register-staged loop: any shape
    if K % 64 == 0:  # LDS-DMA loops: whole 64-wide K-steps of real data
        for variant, stages in ((1, 2), (2, 3), (3, 4), (4, 6), (5, 1)):
            if sk and stages > 2:
                continue  # stream-K: the 1- and 2-stage loops
            for tile, (bm, bn) in enumerate(TILES):
                if stages * (bm + bn) * 64 * 2 * (2 if split else 1) <= LDS_BYTES:
                    cfgs.append(tile + 4 * variant)
        if split and N % 8 == 0 and not (sk or tail):
            cfgs.append(CFG_WIDE)  # the 256 x 128 wide tile: fp32 dense rows
    # variants 6 and 9 (cfgs 24-27, 36-39) are 3x3 kernels; variant 7 / 8 have tile 0 only
    if (M <= 32 and K % 256 == 0 and N % 8 == 0 and splits == 1 and not (stats_out or row_parts or sk or tail)):
        cfgs.append(CFG_SKINNY)
    return sorted(cfgs)


def tile_rows(cfg):
    """BM of a config: the rows of one output tile."""
    if cfg == CFG_WIDE:
        return 256
    if cfg == CFG_SKINNY:
        return 1  # the skinny kernel stores row by row
    return TILES[cfg % 4][0]


# ---- LayerNorm fold --------------------------------------------------------------------------------------

def group64_stats_f64(v):
    """[M, N] float64 -> [M, N / 64, 2]: (mean, M2) of every row's 64-column groups."""
    g = v.reshape(v.shape[0], -1, 64)
    mean = g.mean(-1)
    return torch.stack([mean, ((g - mean[..., None]) ** 2).sum(-1)], -1)


@functools.lru_cache(maxsize=None)
def fold_problem(case, offset, split):
    """LayerNorm folded into the rows GEMM, y = LN(x) W^T + b as rstd (x W'^T - mean col_sum) + b':
    x [M, K] the stored rows (DC offset of `offset` row sigmas, random sign, so that the cancellation is
    real), W' = W gamma rounded to storage, b' = b + W beta (fp32), col_sum = sum_k W' of the stored
    values (fp32), row_stats (mean, rstd) computed in float64 from the stored rows and rounded to fp32,
    parts [M, K / 64, 2] the fp32 (mean, M2) per 64-column group, ref the float64 result (float64
    statistics and column sums: their fp32 roundings are in the tolerance) and S its magnitude sum."""
    B, S, K, N = case
    M = B * S
    g = torch.Generator().manual_seed(3000 + 10 * CASES.index(case) + int(offset))
    sigma = 0.7
    xr = torch.randn(M, K, generator=g) * sigma + torch.randn(M, 1, generator=g) * 0.3
    sign = torch.where(torch.rand(M, 1, generator=g) < 0.5, -1.0, 1.0)
    x = cg.preround(xr + sign * offset * sigma, split)
    gamma = (1.0 + 0.1 * torch.randn(K, generator=g)).double()
    beta = (0.1 * torch.randn(K, generator=g)).double()
    W = (torch.randn(N, K, generator=g) / K ** 0.5).double()
    b = (0.1 * torch.randn(N, generator=g)).double()
    wg = cg.preround((W * gamma).float(), split)
    fb = (b + W @ beta).float().double()
    cs64 = wg.sum(1)
    col_sum = cs64.float().double()
    mean = x.mean(1)
    var = x.var(1, unbiased=False)
    rstd = 1.0 / torch.sqrt(var + LN_EPS)
    row_stats = torch.stack([mean, rstd], 1).float()
    parts = group64_stats_f64(x).float()
    ref = rstd[:, None] * (x @ wg.t() - mean[:, None] * cs64[None]) + fb
    sabs = wg.abs().sum(1)
    S_ = rstd[:, None] * (x.abs() @ wg.abs().t() + mean.abs()[:, None] * sabs[None]) + fb.abs()
    return dict(x=x, wg=wg, fb=fb, col_sum=col_sum, mean=mean, rstd=rstd, var=var, row_stats=row_stats, parts=parts,
                ref=_rows(ref, case), S=_rows(S_, case), sabs=sabs, xabs_mean=x.abs().mean(1))


def fold_model(f, case, *, mean=None, rstd=None, col_sum=None):
    """float64 fold result with some statistics replaced (the mutants, and the row_parts result from
    merged statistics)."""
    mean = f["mean"] if mean is None else mean
    rstd = f["rstd"] if rstd is None else rstd
    cs = f["wg"].sum(1) if col_sum is None else col_sum
    return _rows(rstd[:, None] * (f["x"] @ f["wg"].t() - mean[:, None] * cs[None]) + f["fb"], case)


def _chan_add64(mean, m2, cnt, gx, gy):
    f = np.float32
    d = gx - mean
    tot = f(cnt + f(64.0))
    mean = mean + d * f(f(64.0) / tot)
    m2 = m2 + (gy + d * d * f(f(cnt * f(64.0)) / tot))
    return mean.astype(f), m2.astype(f), tot


def _chan_sym(a, b):
    f = np.float32
    (mean, m2, cnt), (mean_o, m2_o, cnt_o) = a, b
    tot = f(cnt + cnt_o)
    d = mean_o - mean
    inv = f(1.0) / tot if tot > 0 else f(0.0)
    m2n = (m2 + m2_o) + d * d * f(f(cnt * cnt_o) * inv)
    meann = (cnt * mean + cnt_o * mean_o) * inv
    return meann.astype(f), m2n.astype(f), tot


def merge_parts_f32(parts, tpr, skip_overflow=False):
    """numpy float32 emulation of the kernel's row_parts reader (conv_igemm_impl.h RowParts::merge):
    each of `tpr` threads merges its contiguous run of the row's groups left to right (chan_add64), then
    the runs meet by the DPP steps 0xB1 (lane ^ 1) and, at tpr == 4, 0x4E (lane ^ 2) with the symmetric
    chan_sym.  parts [M, ng, 2] -> (mean [M], M2 [M]) float32.  The operation order is the kernel's, the
    contraction of multiply-adds into FMAs is the compiler's: this is a model for the error bound, not for
    the bits.  skip_overflow: the mutant that drops groups past the 8 a thread holds in registers."""
    f = np.float32
    p = np.asarray(parts, dtype=f)
    M, ng = p.shape[0], p.shape[1]
    runs = []
    for sub in range(tpr):
        g0, g1 = sub * ng // tpr, (sub + 1) * ng // tpr
        if g1 > g0:
            mean, m2, cnt = p[:, g0, 0].copy(), p[:, g0, 1].copy(), f(64.0)
        else:
            mean, m2, cnt = np.zeros(M, f), np.zeros(M, f), f(0.0)
        for j in range(g0 + 1, g1):
            if skip_overflow and j >= g0 + 8:
                break
            mean, m2, cnt = _chan_add64(mean, m2, cnt, p[:, j, 0], p[:, j, 1])
        runs.append((mean, m2, cnt))
    runs = [_chan_sym(runs[i], runs[i ^ 1]) for i in range(tpr)]  # 0xB1: quad_perm [1, 0, 3, 2]
    if tpr == 4:
        runs = [_chan_sym(runs[i], runs[i ^ 2]) for i in range(4)]  # 0x4E: quad_perm [2, 3, 0, 1]
    return runs[0]


def merged_stats_bounds(f, K):
    """Per-row bounds of the merged statistics against float64 (derived in test_gemm_rows_bound.py):
    (dmean, absolute; rho, relative, of rstd)."""
    ng = K // 64
    dmean = 2.0 * (ng + 2) * U * f["xabs_mean"]
    rel_m2 = 2.0 * (ng + 6) * U
    rho = 0.5 * rel_m2 + RSQRT_ULPS * 2.0 ** -23
    return dmean, rel_m2, rho


RSQRT_ULPS = 2.0  # supposed error of the device rsqrtf in ulps (no figure in the installed documentation)


def fold_tolerance(f, case, splits, split, row_parts=False):
    """T of the folded GEMM: (bound + 6 * 2^-24) * S_fold -- the 6: the roundings of mean, rstd and
    col_sum to fp32, and the multiply, subtract and multiply of the fold -- and, for row_parts, the
    merged-statistics terms rstd * dmean * sum|W'| and rho * S_fold."""
    T = (bound(case, splits, split) + 6.0 * U) * f["S"]
    if row_parts:
        T = T + _rows(stats_terms(f, case), case)
    return T


def stats_terms(f, case):
    """[M, N]: how far the merged statistics alone may move a folded output."""
    dmean, _, rho = merged_stats_bounds(f, case[2])
    S2 = f["S"].reshape(-1, case[3])
    return (f["rstd"] * dmean)[:, None] * f["sabs"][None] + rho * S2


# ---- subtly wrong kernels, modelled in float64 ---------------------------------------------------------

def mutants(p, case, splits=3):
    """name -> (result of a subtly wrong kernel, the reference it must be checked against), plain GEMM
    with bias.  Some are no-ops for a case (compare with the reference)."""
    B, S, K, N = case
    M = B * S
    x, w, bias = p["x"], p["w"], p["bias"]
    ref = p["ref"]
    out = {}
    w1 = w.clone()
    w1[N // 2, K // 2] = 0  # one product missing in the elements of one channel
    out["one_product"] = _rows(x @ w1.t() + bias, case)
    y = ref.reshape(M, N).clone()
    y[M - 1] = y[0]  # the clamped row index of a tail row (mm = mvalid ? m : 0) leaking into a valid row
    out["last_row_is_row0"] = _rows(y, case)
    n0 = (N - 1) // 64 * 64  # the last 64-wide N tile
    b2 = bias.clone()
    b2[n0 + 8:] = bias[n0:N - 8]  # bias of 8-channel group g applied to group g + 1
    out["bias_group_shift"] = _rows(x @ w.t() + b2, case)
    xt = x.clone()
    xt[:, K - 8:] = 0  # the K tail read as zeros one 8-element chunk early
    out["k_tail_early"] = _rows(xt @ w.t() + bias, case)
    nk = (K + 63) // 64
    per = -(-nk // min(splits, nk))
    s0, s1 = (per * 64, min(K, 2 * per * 64)) if nk > per else (0, K)
    out["slice_twice"] = _rows(x @ w.t() + x[:, s0:s1] @ w[:, s0:s1].t() + bias, case)
    return out


def k_tail_model(p, case, cut=8):
    """(result, S) of a kernel that reads K - cut columns of the rows (the weights are whole)."""
    x = p["x"].clone()
    x[:, case[2] - cut:] = 0
    return (_rows(x @ p["w"].t() + p["bias"], case), _rows(x.abs() @ p["w"].abs().t() + p["bias"].abs(), case))


def activation_mutants(p):
    """name -> (mutant, reference): Clip with lo / hi swapped, tanh-GELU for erf-GELU."""
    lo, hi = p["clip_lo"], p["clip_hi"]
    ref = p["ref"]
    swapped = torch.minimum(torch.maximum(ref, torch.tensor(hi, dtype=ref.dtype)), torch.tensor(lo, dtype=ref.dtype))
    return {"clip_swapped": (swapped, ref.clamp(lo, hi)), "gelu_tanh": (gelu_tanh(ref), gelu_erf(ref))}


def gelu_error(got, v):
    """max |got - gelu(v)| / max(1, |v|) against float64 erf-GELU of v."""
    v = v.double()
    return float(((got.double() - gelu_erf(v)).abs() / v.abs().clamp_min(1.0)).max())


def fold_mutants(f, case):
    """name -> result of a folded GEMM with one statistic wrong."""
    K = case[2]
    cs = f["wg"].sum(1)
    out = {"col_sum_wrong_column": fold_model(f, case, col_sum=torch.roll(cs, -8)),
           "mean_of_next_row": fold_model(f, case, mean=torch.roll(f["mean"], -1))}
    # TPR = 2 (the 128- and 256-row tiles): a thread's run exceeds its 8 registers from 17 groups on
    mean, m2, cnt = merge_parts_f32(f["parts"].numpy(), 2, skip_overflow=True)
    rstd = 1.0 / torch.sqrt(torch.from_numpy(m2.astype(np.float64)) / float(cnt) + LN_EPS)
    out["overflow_groups_skipped"] = fold_model(f, case, mean=torch.from_numpy(mean.astype(np.float64)), rstd=rstd)
    return out
