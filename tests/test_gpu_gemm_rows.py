"""The dense-rows GEMM path of the conv kernels (x[M][K] . W[N][K]^T: MODE 0 of both main loops, the
wide tile cfg 28, the skinny GEMM cfg 32, the LayerNorm fold, the statistics epilogue, GELU / Clip, the
panel-major tile orders, the live batch, stream-K and tail split-K) on the grid of gemm_rows.py, every
launch config, element by element against float64 under T = eps * S (conv_geometry.bound through
gemm_rows.bound).  Every launch pre-fills its outputs with NaN, so an unvisited tile fails; which
configs take a case is asserted from the rules of kernels.h and the launchers (gemm_rows.expected_cfgs),
so a wrong guard cannot pass as "not applicable"; every test ends with the split-K counters at zero.

Largest |err| / T observed on an MI355X over all cases and configs (pytest -s prints them):
  sharp pass            bf16 0.0228   fp32 0.1371
  epilogue pass         bf16 0.9896   fp32 0.1863
  Clip                  bf16 0.0091   fp32 0.1371
  tile orders           bf16 0.0058   fp32 0.0509
  live batch            bf16 0.0228   fp32 0.1371
  stream-K / tail       bf16 0.0075   fp32 0.1022
  fold, row_stats       bf16 0.0072   fp32 0.0806
  fold, row_parts                     fp32 0.0776   (row_parts against row_stats: 0.0779 of the statistics terms)
  statistics producer   mean 0.0053   M2 0.0202
The bf16 epilogue figure is the storage term, as in test_gpu_conv_geometry.py: 2^-8 |ref| is bf16's unit
roundoff, which round-to-nearest reaches, so stored bf16 outputs sit close to 1 by construction.
GELU (relu = 2) against float64 erf-GELU of the kernel's own fp32 pre-activation, |err| / max(1, |v|):
measured 1.129e-07 on an MI355X; asserted gemm_rows.GELU_BAR = 2^-21 = 4.8e-7 (4x the measured figure, rounded
up to a power of two: the error of the device erfc varies over its argument range and 1e5 samples do not
find its maximum).  tanh-GELU of the same v is 1e-4 .. 5e-4 off and fails that bar (asserted).

Statistics producer (stats_out: (mean, M2) of every 64-column group of the launch's own f32 output v).
mean: 64 values summed in a fixed tree (7 additions inside a lane, three pairwise halvings across lanes)
-- any summation order of 64 terms is within 63 u of sum|v|, the scalings by 1/8 and 1/2 are exact, the
stored value rounds once: 66 u mean|v| with the group's mean |v|, doubled as everywhere (the supposition
of conv_geometry): |mean - mean_64| <= 2 * 66 * u * mean|v|.  M2: a sum of 64 + 7 non-negative terms
(the squared deviations and the between-lane terms d^2 n / 2), each formed with a few roundings: relative
2 * 70 * u; the deviations are taken from the computed mean, which adds 64 * dmean^2, of second order.

Live batch: rows of live samples equal the launch without `live` bit for bit for the forms whose K cuts
do not depend on the number of tiles (plain, uniform split-K, the wide and skinny kernels).  Tail split-K
and stream-K choose which tiles are cut, and where, from the number of LIVE tiles (that is their purpose),
so there the bits are compared with the same launch on a batch of `live` samples, which has the same
tiles (N-fastest order for both, as the heuristic order looks at the batch), and the rows with float64.
"""
import pytest

import conv_geometry as cg
import gemm_rows as gr
from conftest import gpu_available

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not gpu_available(), reason="needs a GPU")]

PRECISIONS = pytest.mark.parametrize("split", [False, True], ids=["bf16", "fp32"])
NAN = float("nan")


def _prec(split):
    return "fp32" if split else "bf16"


def _report(line):
    print(line)  # pytest -s: the figures quoted in the docstring above


def _device_problem(case, split, batch=None, **kw):
    """(ConvProblem on the GPU, the shared CPU problem moved to the GPU).  batch: the first samples only."""
    import torch

    from die_amd.ops import kernels as K

    B, S, Kd, N = case
    p = {k: (v.cuda() if torch.is_tensor(v) else v) for k, v in gr.problem(case, split).items()}
    Bb = B if batch is None else batch
    x = p["x"].reshape(B, S, 1, Kd)[:Bb].contiguous()
    x = x.float() if split else x.to(torch.bfloat16)  # exact: the values are what the storage holds
    if "res" in kw:
        kw["res"] = p["res"].float() if split else p["res"].to(torch.bfloat16)
    for name in ("scale2", "shift2"):
        if name in kw:
            kw[name] = p[name].float()
    pr = K.ConvProblem(x, p["w"].float().reshape(N, Kd, 1, 1), bias=p["bias"].float(), split=split, **kw)
    return pr, p


def _fill(pr):
    pr.out.fill_(NAN)
    if pr.out2 is not None:
        pr.out2.fill_(NAN)


def _clean(pr):
    assert int(pr.counters.abs().sum().item()) == 0, "split-K counters left non-zero"


@PRECISIONS
@pytest.mark.parametrize("case", gr.CASES, ids=gr.case_id)
def test_gemm_rows_sharp(native, case, split):
    """Bias only, f32 output: every config x (splits 1; 3 fused; 3 two-kernel; 4 fused)."""
    import torch

    pr, p = _device_problem(case, split, out_f32=True, max_splits=4)
    ref, S = p["ref"], p["S"]
    worst, outs = 0.0, {}
    for splits, fused in ((1, True), (3, True), (3, False), (4, True)):
        T = gr.bound(case, splits, split) * S
        ran = []
        for cfg in range(gr.NUM_CFGS):
            _fill(pr)
            rc = pr.launch(cfg, splits, fused)
            if rc == 1:
                continue  # hipErrorInvalidValue: the config does not take this shape
            assert rc == 0, (cfg, splits, fused, rc)
            torch.cuda.synchronize()
            # cfg 28 and cfg 32 are checked against float64 like the rest; their K order is their own
            worst = max(worst, cg.check(pr.out, ref, T, "cfg %d splits %d fused %d" % (cfg, splits, fused)))
            ran.append(cfg)
            if splits == 1:
                outs[cfg] = pr.out.clone()
        assert ran == gr.expected_cfgs(case, split, splits), (splits, fused, ran)
    _clean(pr)
    # variants 0-5 on one tile accumulate K in the same order: bit-identical
    for cfg, out in outs.items():
        if cfg < 24:
            assert torch.equal(out, outs[cfg % 4]), "cfg %d differs from cfg %d in bits" % (cfg, cfg % 4)
    _report("sharp %s %s: ran %s at splits 1; max |err|/T %.4f"
            % (gr.case_id(case), _prec(split), gr.expected_cfgs(case, split, 1), worst))


@PRECISIONS
@pytest.mark.parametrize("case", gr.CASES, ids=gr.case_id)
def test_gemm_rows_epilogue(native, case, split):
    """bias + residual + ReLU and the dual store relu(v * scale2 + shift2): the stored out and out2, every
    config (the N = 12 case: the ragged-N register epilogue with residual and dual store)."""
    import torch

    pr, p = _device_problem(case, split, relu=True, res=True, scale2=True, shift2=True, relu2=True, max_splits=1)
    Tv = gr.bound(case, 1, split, extra=1) * p["Sv"] + cg.storage(p["v"], split)
    Tu = gr.bound(case, 1, split, extra=3) * p["Su"] + cg.storage(p["u"], split)
    ran, worst = [], 0.0
    for cfg in range(gr.NUM_CFGS):
        _fill(pr)
        rc = pr.launch(cfg, 1)
        if rc == 1:
            continue
        assert rc == 0, (cfg, rc)
        torch.cuda.synchronize()
        out, out2 = pr.results()
        worst = max(worst, cg.check(out, p["v"], Tv, "cfg %d out" % cfg), cg.check(out2, p["u"], Tu, "cfg %d out2" % cfg))
        ran.append(cfg)
    assert ran == gr.expected_cfgs(case, split, 1), ran
    _clean(pr)
    _report("epilogue %s %s: max |err|/T %.4f" % (gr.case_id(case), _prec(split), worst))


@PRECISIONS
@pytest.mark.parametrize("case", gr.CASES, ids=gr.case_id)
def test_gemm_rows_activations(native, case, split):
    """Clip (relu = 3, clip_lo / clip_hi through the geometry JSON) and erf-GELU (relu = 2) on one config
    of variant 0, one of variant 1 and the skinny kernel."""
    import torch

    pr, p = _device_problem(case, split, out_f32=True, max_splits=1)
    ref, S = p["ref"], p["S"]
    T = gr.bound(case, 1, split) * S  # Clip is 1-Lipschitz: the pre-activation's tolerance
    lo, hi = p["clip_lo"], p["clip_hi"]
    clipped = ref.clamp(lo, hi)
    want = [c for c in (3, 4, gr.CFG_SKINNY) if c in gr.expected_cfgs(case, split, 1)]
    assert 3 in want
    w_clip, w_gelu = 0.0, 0.0
    for cfg in (3, 4, gr.CFG_SKINNY):
        _fill(pr)
        rc = pr.launch(cfg, 1, extra=dict(relu=3, clip_lo=lo, clip_hi=hi))
        assert rc == (0 if cfg in want else 1), (cfg, rc)
        if rc:
            continue
        torch.cuda.synchronize()
        w_clip = max(w_clip, cg.check(pr.out, clipped, T, "cfg %d Clip" % cfg))
        if ref.numel() >= 64:
            got = pr.out
            assert 0.2 < float((got == lo).double().mean()) < 0.45 and 0.2 < float((got == hi).double().mean()) < 0.45
        # GELU: the kernel's own pre-activation first (same accumulation order, the same bits), then the
        # activation alone against float64
        _fill(pr)
        assert pr.launch(cfg, 1, extra=dict(relu=0)) == 0
        torch.cuda.synchronize()
        v = pr.out.clone()
        _fill(pr)
        assert pr.launch(cfg, 1, extra=dict(relu=2)) == 0
        torch.cuda.synchronize()
        assert not bool(torch.isnan(pr.out).any())
        e = gr.gelu_error(pr.out, v)
        w_gelu = max(w_gelu, e)
        assert e <= gr.GELU_BAR, "cfg %d GELU: |err| / max(1, |v|) = %.3e" % (cfg, e)
        if float(v.abs().max()) > 0.5:
            assert gr.gelu_error(gr.gelu_tanh(v.double()), v) > gr.GELU_BAR  # the bar tells the two GELUs apart
    _clean(pr)
    _report("activations %s %s: Clip max |err|/T %.4f; GELU max |err|/max(1,|v|) %.3e"
            % (gr.case_id(case), _prec(split), w_clip, w_gelu))


@PRECISIONS
@pytest.mark.parametrize("case", [c for c in gr.CASES if c[3] >= 136], ids=gr.case_id)
def test_gemm_rows_tile_orders(native, case, split):
    """XCD tile orders 0..4 (3 / 4: N in 2 / 4 panels, the last one narrower here): every config, each
    order inside the bound and all five the same bits (a wrong panel map leaves a tile at NaN or computes
    one twice and another never)."""
    import torch

    pr, p = _device_problem(case, split, out_f32=True, max_splits=1)
    T = gr.bound(case, 1, split) * p["S"]
    worst = 0.0
    for cfg in gr.expected_cfgs(case, split, 1):
        first = None
        for order in range(5):
            _fill(pr)
            assert pr.launch(cfg, 1, order=order) == 0, (cfg, order)
            torch.cuda.synchronize()
            worst = max(worst, cg.check(pr.out, p["ref"], T, "cfg %d order %d" % (cfg, order)))
            if first is None:
                first = pr.out.clone()
            assert torch.equal(pr.out, first), "cfg %d: order %d differs from order 0 in bits" % (cfg, order)
    _clean(pr)
    _report("orders %s %s: max |err|/T %.4f" % (gr.case_id(case), _prec(split), worst))


def _ws_splits(case, P=8):
    """max_splits that makes the workspace hold a stream-K launch of P blocks on 64x64 tiles."""
    return max(3, -(-P * 2 * 64 * 64 // (case[0] * case[1] * case[3])))


# form name -> (cfg, splits, launch keywords, the K cuts depend on the number of live tiles)
_LIVE_FORMS = [
    ("plain", 3, 1, {}, False),
    ("split-K", 7, 3, {}, False),
    ("tail", 7, 3, dict(extra=dict(tail=4)), True),
    ("stream-K", 7, 1, dict(sk=8), True),
    ("wide", gr.CFG_WIDE, 1, {}, False),
    ("skinny", gr.CFG_SKINNY, 1, {}, False),
]


def _form_applies(case, split, cfg, splits, kw):
    tail, sk = "extra" in kw, "sk" in kw
    return cfg in gr.expected_cfgs(case, split, splits, sk=sk, tail=tail)


@PRECISIONS
@pytest.mark.parametrize("case", [c for c in gr.CASES if c[1] > 1], ids=gr.case_id)
def test_gemm_rows_live_batch(native, case, split):
    """ConvArgs::live with several rows per sample (Ml = live * S): live in {1, B - 1, B}."""
    import torch

    B, S, Kd, N = case
    M = B * S
    pr, p = _device_problem(case, split, out_f32=True, max_splits=_ws_splits(case))
    ref, Sm = p["ref"].reshape(M, N), p["S"].reshape(M, N)
    worst, done = 0.0, []
    for name, cfg, splits, kw, cuts_follow_live in _LIVE_FORMS:
        order = 1 if cuts_follow_live else 0
        _fill(pr)
        rc = pr.launch(cfg, splits, True, order=order, **kw)
        assert rc == (0 if _form_applies(case, split, cfg, splits, kw) else 1), (name, rc)
        if rc:
            continue
        torch.cuda.synchronize()
        full = pr.out.reshape(M, N).clone()
        eps = gr.bound(case, 8 if "sk" in kw else splits, split)
        worst = max(worst, cg.check(full, ref, eps * Sm, name))
        for live in sorted({1, B - 1, B} - {0}):
            lv = torch.tensor([live], dtype=torch.int64, device="cuda")
            _fill(pr)
            extra = dict(kw.get("extra", {}), live=int(lv.data_ptr()))
            assert pr.launch(cfg, splits, True, order=order, extra=extra, sk=kw.get("sk", 0)) == 0, (name, live)
            torch.cuda.synchronize()
            got = pr.out.reshape(M, N)
            rows = live * S
            worst = max(worst, cg.check(got[:rows], ref[:rows], eps * Sm[:rows], "%s live %d" % (name, live)))
            if cuts_follow_live and live < B:
                sub, _ = _device_problem(case, split, batch=live, out_f32=True, max_splits=_ws_splits((live, S, Kd, N)))
                sub.out.fill_(NAN)
                assert sub.launch(cfg, splits, True, order=order, **kw) == 0, (name, live)
                torch.cuda.synchronize()
                want = sub.out.reshape(rows, N)
                _clean(sub)
            else:
                want = full[:rows]
            assert torch.equal(got[:rows], want), "%s live %d: live rows differ in bits" % (name, live)
            # tiles that hold padding samples only are skipped: their rows keep the sentinel
            bm = gr.tile_rows(cfg)
            skipped = -(-rows // bm) * bm
            assert bool(torch.isnan(got[skipped:]).all()), "%s live %d: a skipped tile was written" % (name, live)
        done.append(name)
    _clean(pr)
    assert "plain" in done
    _report("live %s %s: forms %s; max |err|/T %.4f" % (gr.case_id(case), _prec(split), done, worst))


@PRECISIONS
@pytest.mark.parametrize("case", [c for c in gr.CASES if c[2] % 64 == 0 and c[3] % 8 == 0], ids=gr.case_id)
def test_gemm_rows_streamk_and_tail(native, case, split):
    """Stream-K (8 blocks) and tail split-K (tail 4, 3 slices) on the 2-stage LDS-DMA ring of the 64x64
    tile, dense rows; each launch repeated once with equal bits."""
    import torch

    cfg, P = 3 + 4 * 1, 8
    assert cfg in gr.expected_cfgs(case, split, 1, sk=True)
    pr, p = _device_problem(case, split, out_f32=True, max_splits=_ws_splits(case, P))
    ref, S = p["ref"], p["S"]

    def twice(what, eps, *a, **kw):
        outs = []
        for _ in range(2):
            _fill(pr)
            assert pr.launch(*a, **kw) == 0, what
            torch.cuda.synchronize()
            outs.append(pr.out.clone())
        assert torch.equal(outs[0], outs[1]), what + ": not repeatable"
        _clean(pr)
        return cg.check(outs[0], ref, eps * S, what)

    w1 = twice("stream-K", gr.bound(case, P, split), cfg, 1, True, sk=P)  # a tile has at most P contributors
    w2 = 0.0
    if cfg in gr.expected_cfgs(case, split, 3, tail=True):
        w2 = twice("tail split-K", gr.bound(case, 3, split), cfg, 3, True, extra=dict(tail=4))
    else:
        assert case[2] == 64
        _fill(pr)
        assert pr.launch(cfg, 3, True, extra=dict(tail=4)) == 1  # one K-step cannot be cut
    _clean(pr)
    _report("streamk/tail %s %s: max |err|/T %.4f %.4f" % (gr.case_id(case), _prec(split), w1, w2))


def _fold_device(case, offset, split):
    import torch

    from die_amd.ops import kernels as K

    B, S, Kd, N = case
    f = {k: (v.cuda() if torch.is_tensor(v) else v) for k, v in gr.fold_problem(case, offset, split).items()}
    x = f["x"].reshape(B, S, 1, Kd)
    x = x.float() if split else x.to(torch.bfloat16)
    pr = K.ConvProblem(x, f["wg"].float().reshape(N, Kd, 1, 1), bias=f["fb"].float(), out_f32=True, max_splits=2, split=split)
    # col_sum followed by its first 8 values again: a pointer 8 floats in reads the columns rolled by 8
    cs = torch.zeros((N + 8 + 127) // 128 * 128, dtype=torch.float32, device="cuda")
    cs[:N] = f["col_sum"].float()
    cs[N:N + 8] = f["col_sum"][:8].float()
    return pr, f, cs, f["row_stats"].contiguous(), f["parts"].contiguous()


@PRECISIONS
@pytest.mark.parametrize("offset", gr.FOLD_OFFSETS)
@pytest.mark.parametrize("case", gr.FOLD_CASES, ids=gr.case_id)
def test_gemm_rows_layernorm_fold(native, case, offset, split):
    """LayerNorm folded into the GEMM, statistics delivered as row_stats (both precisions) and merged by
    the kernel from row_parts (fp32): every config at splits 1, 2 fused and 2 two-kernel (row_parts_direct)."""
    import torch

    pr, f, cs, row_stats, parts = _fold_device(case, offset, split)
    common = dict(col_sum=int(cs.data_ptr()), ln_eps=gr.LN_EPS)
    terms = gr._rows(gr.stats_terms(f, case), case)
    w_stats = w_parts = w_diff = 0.0
    for splits, fused in ((1, True), (2, True), (2, False)):
        T = gr.fold_tolerance(f, case, splits, split)
        Tp = T + terms
        ran, ran_p = [], []
        for cfg in range(gr.NUM_CFGS):
            _fill(pr)
            rc = pr.launch(cfg, splits, fused, extra=dict(common, row_stats=int(row_stats.data_ptr())))
            if rc == 1:
                continue
            assert rc == 0, (cfg, splits, fused, rc)
            torch.cuda.synchronize()
            a = pr.out.clone()
            w_stats = max(w_stats, cg.check(a, f["ref"], T, "row_stats cfg %d splits %d fused %d" % (cfg, splits, fused)))
            ran.append(cfg)
            if not split:
                continue
            _fill(pr)
            rc = pr.launch(cfg, splits, fused, extra=dict(common, row_parts=int(parts.data_ptr())))
            if rc == 1:
                continue
            assert rc == 0, (cfg, splits, fused, rc)
            torch.cuda.synchronize()
            what = "cfg %d splits %d fused %d" % (cfg, splits, fused)
            w_parts = max(w_parts, cg.check(pr.out, f["ref"], Tp, "row_parts " + what))
            # the GEMM part is the same bits: the two outputs differ by the statistics terms alone
            w_diff = max(w_diff, cg.check(pr.out, a.double(), terms, "row_parts against row_stats, " + what))
            ran_p.append(cfg)
        assert ran == gr.expected_cfgs(case, split, splits), (splits, fused, ran)
        if split:
            assert ran_p == gr.expected_cfgs(case, split, splits, row_parts=True), (splits, fused, ran_p)
    _clean(pr)
    _report("fold %s offset %g %s: row_stats max |err|/T %.4f; row_parts %.4f; row_parts - row_stats %.4f of the "
            "statistics terms" % (gr.case_id(case), offset, _prec(split), w_stats, w_parts, w_diff))


@PRECISIONS
@pytest.mark.parametrize("case", [c for c in gr.CASES if c[3] % 64 == 0], ids=gr.case_id)
def test_gemm_rows_stats_producer(native, case, split):
    """stats_out with the residual add: (mean, M2) of every 64-column group of the launch's own f32 output."""
    import torch

    B, S, Kd, N = case
    M = B * S
    pr, p = _device_problem(case, split, res=True, out_f32=True, max_splits=2)
    st = torch.zeros(M, N // 64, 2, dtype=torch.float32, device="cuda")
    Tv = gr.bound(case, 2, split, extra=1) * (p["S"] + p["res"].abs())
    w_mean = w_m2 = 0.0
    for splits, fused in ((1, True), (2, True), (2, False)):
        ran = []
        for cfg in range(gr.NUM_CFGS):
            _fill(pr)
            st.fill_(NAN)
            rc = pr.launch(cfg, splits, fused, extra=dict(stats_out=int(st.data_ptr())))
            if rc == 1:
                continue
            assert rc == 0, (cfg, splits, fused, rc)
            torch.cuda.synchronize()
            what = "cfg %d splits %d fused %d" % (cfg, splits, fused)
            cg.check(pr.out, p["ref"] + p["res"], Tv, what)
            v = pr.out.reshape(M, N).double()
            want = gr.group64_stats_f64(v)
            got = st.double()
            assert not bool(torch.isnan(got).any()), what + ": a group was not written"
            dmean = 2.0 * 66 * gr.U * v.abs().reshape(M, -1, 64).mean(-1)
            e_mean = (got[..., 0] - want[..., 0]).abs()
            assert bool((e_mean <= dmean).all()), (what, float((e_mean / dmean).max()))
            Tm2 = 2.0 * 70 * gr.U * want[..., 1] + 64.0 * dmean ** 2
            e_m2 = (got[..., 1] - want[..., 1]).abs()
            assert bool((e_m2 <= Tm2).all()), (what, float((e_m2 / Tm2).max()))
            w_mean, w_m2 = max(w_mean, float((e_mean / dmean).max())), max(w_m2, float((e_m2 / Tm2).max()))
            ran.append(cfg)
        assert ran == gr.expected_cfgs(case, split, splits, stats_out=True), (splits, fused, ran)
    _clean(pr)
    _report("producer %s %s: mean %.4f, M2 %.4f of their bounds" % (gr.case_id(case), _prec(split), w_mean, w_m2))


@PRECISIONS
def test_gemm_rows_check_sees_a_short_k(native, split):
    """The check on the kernels themselves: launched with K shortened by 8 (Kpad and the row pitch as they
    are, so every read stays inside the rows), the register-staged dense loop computes the "K tail one
    chunk early" model and fails the check against the true reference."""
    import torch

    case = gr.CASES[4]
    pr, p = _device_problem(case, split, out_f32=True, max_splits=1)
    cpu = gr.problem(case, split)
    model, Sm = (t.cuda() for t in gr.k_tail_model(cpu, case))
    assert not torch.equal(model, p["ref"])
    eps = gr.bound(case, 1, split)
    for cfg in range(8):
        _fill(pr)
        rc = pr.launch(cfg, 1, extra=dict(K=case[2] - 8))
        assert rc == (0 if cfg < 4 else 1), (cfg, rc)  # the LDS-DMA loops need whole K-steps of real data
        if rc:
            continue
        torch.cuda.synchronize()
        cg.check(pr.out, model, eps * Sm, "cfg %d with K - 8" % cfg)
        with pytest.raises(AssertionError, match="outside the bound"):
            cg.check(pr.out, p["ref"], eps * p["S"], "cfg %d with K - 8" % cfg)
    _clean(pr)


@PRECISIONS
def test_gemm_rows_check_sees_a_shifted_col_sum(native, split):
    """... and with the col_sum pointer 8 floats into its (padded) buffer the fold computes the "col_sum of
    the wrong column" model and fails the check against the true reference."""
    import torch

    case, offset = gr.CASES[9], 10.0
    pr, f, cs, row_stats, parts = _fold_device(case, offset, split)
    c = f["col_sum"]
    model = gr.fold_model(f, case, mean=f["row_stats"][:, 0].double(), rstd=f["row_stats"][:, 1].double(),
                          col_sum=torch.roll(c, -8))
    Sm = gr._rows(f["rstd"][:, None] * (f["x"].abs() @ f["wg"].abs().t() + f["mean"].abs()[:, None]
                                        * torch.roll(f["sabs"], -8)[None]) + f["fb"].abs(), case)
    eps = gr.bound(case, 1, split) + 6.0 * gr.U
    for cfg in (3, 7, gr.CFG_WIDE):
        _fill(pr)
        rc = pr.launch(cfg, 1, extra=dict(col_sum=int(cs.data_ptr()) + 32, ln_eps=gr.LN_EPS, row_stats=int(row_stats.data_ptr())))
        assert rc == (0 if cfg in gr.expected_cfgs(case, split, 1) else 1), (cfg, rc)
        if rc:
            continue
        torch.cuda.synchronize()
        cg.check(pr.out, model, eps * Sm, "cfg %d with col_sum + 8" % cfg)
        with pytest.raises(AssertionError, match="outside the bound"):
            cg.check(pr.out, f["ref"], gr.fold_tolerance(f, case, 1, split), "cfg %d with col_sum + 8" % cfg)
    _clean(pr)
