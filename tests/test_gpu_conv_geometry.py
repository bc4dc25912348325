"""The implicit-GEMM conv kernels on rectangular, dilated and unevenly padded geometry (the grid of
conv_geometry.py), every launch config, element by element against float64.

Sharp pass: bias only, f32 output, every config at splits 1 and 3 (fused and two-kernel reduction).
Epilogue pass: bias + residual + ReLU + dual store, the stored outputs.  Stream-K and tail split-K on
one LDS-DMA config.  Which configs take a case is asserted from the rules of kernels.h, so a wrong
guard cannot pass as "not applicable".  Then one engine-level graph with the same geometries, which
guards the planner's weight packing, pads / auto_pad arithmetic and the dilation hand-off.

Largest |err| / T observed on an MI355X over all cases and configs (T: conv_geometry.bound, eps * S per
element, plus the storage term for stored outputs):
  sharp pass          bf16 0.0093   fp32 0.1125
  stream-K / tail     bf16 0.0084   fp32 0.0914
  epilogue pass       bf16 0.9834   fp32 0.1906
The sharp pass leaves the factor 2 of eps untested (a hundredth of T in bf16).  The bf16 epilogue
figure is the storage term, not the kernel: 2^-8 |ref| is bf16's unit roundoff, which round-to-nearest
reaches for a value just above a power of two, so stored bf16 outputs sit close to 1 by construction
(the accumulation part stays as small as in the sharp pass).
All applicable configs of variants 0-5 on one tile agree bit for bit at splits = 1; that is asserted.
"""
import numpy as np
import pytest

import conv_geometry as cg
from conftest import gpu_available

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not gpu_available(), reason="needs a GPU")]

TILES = [(128, 128), (128, 64), (64, 128), (64, 64)]  # kernels.h TileCfg: cfg = tile + 4 * variant
LDS_BYTES = 160 * 1024
PRECISIONS = pytest.mark.parametrize("split", [False, True], ids=["bf16", "fp32"])


def expected_cfgs(case, split):
    """The launch configs that take the case at splits = 1, by the rules of kernels.h / the launchers."""
    B, H, W, Cin, Cout, KH, KW, s, (t, l, b, r), d = case
    Ho, Wo = cg.out_hw(case)
    assert not (KH == 1 and KW == 1 and s == 1 and t == 0 and l == 0 and H == Ho and W == Wo), "no dense rows here"
    K = KH * KW * Cin
    implicit = Cin % 64 == 0  # LDS-DMA rings: a 64-wide K-step never straddles a tap
    patchify = (not implicit and KH == s and KW == s and s > 1 and d == 1 and (t, l) == (0, 0) and (KW * Cin) % 64 == 0
                and K % 64 == 0 and Ho == (H - KH) // s + 1 and Wo == (W - KW) // s + 1)
    cfgs = [0, 1, 2, 3]  # variant 0 (register-staged): any shape
    if implicit or patchify:
        for variant, stages in ((1, 2), (2, 3), (3, 4), (4, 6), (5, 1)):
            if patchify and stages > 3:
                continue
            for tile, (bm, bn) in enumerate(TILES):
                if stages * (bm + bn) * 64 * 2 * (2 if split else 1) <= LDS_BYTES:
                    cfgs.append(tile + 4 * variant)
    # variants 6 / 9 (spatially tiled and four-tile 3x3 kernels, tile 3): 3x3 / s1 / p1 / dil 1, H == Ho, W == Wo
    if (KH, KW, s, d, t, l) == (3, 3, 1, 1, 1, 1) and (H, W) == (Ho, Wo) and Cin % 64 == 0 and Cout % 8 == 0:
        cfgs += [27, 39]
    # variants 7 (cfg 28) and 8 (cfg 32) take dense rows only
    return sorted(cfgs)


def _device_problem(case, split, **kw):
    """(ConvProblem on the GPU, the shared CPU problem moved to the GPU)."""
    import torch

    from die_amd.ops import kernels as K

    p = {k: v.cuda() for k, v in cg.problem(case, split).items()}
    x = p["x"].permute(0, 2, 3, 1).contiguous()
    x = x.float() if split else x.to(torch.bfloat16)  # exact: the values are what the storage holds
    if "res" in kw:
        kw["res"] = p["res"].float() if split else p["res"].to(torch.bfloat16)
    for name in ("scale2", "shift2"):
        if name in kw:
            kw[name] = p[name].float()
    pr = K.ConvProblem(x, p["w"].float(), bias=p["bias"].float(), stride=case[7], pad=case[8], dil=case[9], split=split,
                       **kw)
    return pr, p


def _report(line):
    print(line)  # pytest -s: the figures quoted in the docstring above


@PRECISIONS
@pytest.mark.parametrize("case", cg.CASES, ids=cg.case_id)
def test_conv_geometry_sharp(native, case, split):
    """Bias-only epilogue, f32 output: every config x (splits 1, splits 3 fused, splits 3 two-kernel)."""
    import torch

    from die_amd.ops import kernels as K

    pr, p = _device_problem(case, split, out_f32=True, max_splits=3)
    ref, S = p["ref"], p["S"]
    want = expected_cfgs(case, split)
    worst, outs = 0.0, {}
    for splits, fused in ((1, True), (3, True), (3, False)):
        T = cg.bound(case, splits, split) * S
        ran = []
        for cfg in range(K.NUM_CFGS):
            pr.out.fill_(float("nan"))
            rc = pr.launch(cfg, splits, fused)
            if rc == 1:
                continue  # hipErrorInvalidValue: the config does not take this shape
            assert rc == 0, (cfg, splits, fused, rc)
            torch.cuda.synchronize()
            worst = max(worst, cg.check(pr.out, ref, T, "cfg %d splits %d fused %d" % (cfg, splits, fused)))
            ran.append(cfg)
            if splits == 1:
                outs[cfg] = pr.out.clone()
        # split-K needs 8-channel groups (N % 8 == 0); the configs that take the shape are the same
        assert ran == (want if splits == 1 or case[4] % 8 == 0 else []), (splits, fused, ran, want)
    assert int(pr.counters.abs().sum().item()) == 0
    # variants 0-5 on one tile accumulate K in the same order: bit-identical
    for cfg, out in outs.items():
        if cfg < 24:
            assert torch.equal(out, outs[cfg % 4]), "cfg %d differs from cfg %d in bits" % (cfg, cfg % 4)
    _report("sharp %s %s: ran %s; not applicable: the other %d; max |err|/T %.4f"
            % (cg.case_id(case), "fp32" if split else "bf16", want, K.NUM_CFGS - len(want), worst))


@PRECISIONS
@pytest.mark.parametrize("case", cg.CASES, ids=cg.case_id)
def test_conv_geometry_epilogue(native, case, split):
    """bias + residual + ReLU and the dual store relu(v * scale2 + shift2): the stored out and out2."""
    import torch

    from die_amd.ops import kernels as K

    pr, p = _device_problem(case, split, relu=True, res=True, scale2=True, shift2=True, relu2=True, max_splits=1)
    # one more term (the residual) in v; a multiply and an add more in u
    Tv = cg.bound(case, 1, split, extra=1) * p["Sv"] + cg.storage(p["v"], split)
    Tu = cg.bound(case, 1, split, extra=3) * p["Su"] + cg.storage(p["u"], split)
    ran, worst = [], 0.0
    for cfg in range(K.NUM_CFGS):
        pr.out.fill_(float("nan"))
        pr.out2.fill_(float("nan"))
        rc = pr.launch(cfg, 1)
        if rc == 1:
            continue
        assert rc == 0, (cfg, rc)
        torch.cuda.synchronize()
        out, out2 = pr.results()
        worst = max(worst, cg.check(out, p["v"], Tv, "cfg %d out" % cfg), cg.check(out2, p["u"], Tu, "cfg %d out2" % cfg))
        ran.append(cfg)
    assert ran == expected_cfgs(case, split), ran
    _report("epilogue %s %s: max |err|/T %.4f" % (cg.case_id(case), "fp32" if split else "bf16", worst))


@PRECISIONS
@pytest.mark.parametrize("case", [c for c in cg.CASES if c[3] % 64 == 0], ids=cg.case_id)
def test_conv_geometry_streamk_and_tail(native, case, split):
    """Stream-K (8 blocks) and tail split-K (tail 4, 3 slices) on the 2-stage LDS-DMA ring of the 64x64 tile."""
    import torch

    cfg = 3 + 4 * 1
    assert cfg in expected_cfgs(case, split)
    Ho, Wo = cg.out_hw(case)
    P = 8
    ws_splits = max(3, -(-P * 2 * 64 * 64 // (case[0] * Ho * Wo * case[4])))  # stream-K: 2 slabs per block
    pr, p = _device_problem(case, split, out_f32=True, max_splits=ws_splits)
    ref, S = p["ref"], p["S"]
    pr.out.fill_(float("nan"))
    assert pr.launch(cfg, 1, True, sk=P) == 0
    torch.cuda.synchronize()
    w1 = cg.check(pr.out, ref, cg.bound(case, P, split) * S, "stream-K")  # a tile has at most P contributors
    assert int(pr.counters.abs().sum().item()) == 0
    pr.out.fill_(float("nan"))
    rc = pr.launch(cfg, 3, True, extra=dict(tail=4))
    w2 = 0.0
    if pr.geom["Kpad"] // 64 >= 2:
        assert rc == 0, rc
        torch.cuda.synchronize()
        w2 = cg.check(pr.out, ref, cg.bound(case, 3, split) * S, "tail split-K")
    else:
        assert rc == 1, rc  # one K-step cannot be cut: the launcher refuses a tail launch without split-K
    assert int(pr.counters.abs().sum().item()) == 0
    _report("streamk/tail %s %s: max |err|/T %.4f %.4f" % (cg.case_id(case), "fp32" if split else "bf16", w1, w2))


@pytest.mark.parametrize("field", ["swap_pads", "end_as_begin", "no_dil"])
def test_conv_geometry_check_sees_a_wrong_field(native, field):
    """The check on the kernels themselves: launched with one geometry field wrong (pads swapped, end
    pads as begin pads, dilation dropped -- every read stays bounds-checked), the register-staged and
    the LDS-DMA loop compute what conv_geometry.kernel_model says of that field, and fail the check."""
    import torch

    case = cg.CASES[6]  # stride 2, dilation 2, four different pads
    t, l, b, r = case[8]
    wrong = dict(swap_pads=dict(pad_h=l, pad_w=t), end_as_begin=dict(pad_h=b, pad_w=r), no_dil=dict(dil=1))[field]
    pr, p = _device_problem(case, False, out_f32=True, max_splits=1)
    eps = cg.bound(case, 1, False)
    model = cg.kernel_model(p["x"], p["w"], p["bias"], case, **wrong)
    Sm = cg.kernel_model(p["x"].abs(), p["w"].abs(), p["bias"].abs(), case, **wrong)
    assert not torch.equal(model, p["ref"])
    for cfg in (3, 3 + 4 * 1):
        pr.out.fill_(float("nan"))
        assert pr.launch(cfg, 1, extra=wrong) == 0
        torch.cuda.synchronize()
        cg.check(pr.out, model, eps * Sm, "cfg %d with %s" % (cfg, field))
        with pytest.raises(AssertionError, match="outside the bound"):
            cg.check(pr.out, p["ref"], eps * p["S"], "cfg %d with %s" % (cfg, field))


# ---- one engine-level graph ------------------------------------------------------------------------

# name, cin, cout, (KH, KW), stride, Conv attributes
_LAYERS = [
    ("conv1", 3, 32, (3, 3), 2, dict(pads=[0, 0, 1, 1])),
    ("conv2", 32, 64, (1, 7), 1, dict(pads=[0, 3, 0, 3])),
    ("conv3", 64, 64, (7, 1), 1, dict(pads=[3, 0, 3, 0])),
    ("conv4", 64, 64, (3, 3), 1, dict(pads=[2, 2, 2, 2], dilations=[2, 2])),
    ("conv5", 64, 64, (5, 5), 2, dict(auto_pad="SAME_UPPER")),
]
_IMAGE = (3, 20, 28)
_CLASSES = 10


def _geometry_weights(seed=0):
    rng = np.random.default_rng(seed)
    w = {}
    for name, cin, cout, (kh, kw), _, _ in _LAYERS:
        w[name + ".weight"] = (rng.standard_normal((cout, cin, kh, kw)) * (2.0 / (cin * kh * kw)) ** 0.5).astype(np.float32)
        w[name + ".bias"] = (0.1 * rng.standard_normal(cout)).astype(np.float32)
    w["fc.weight"] = (rng.standard_normal((_CLASSES, 64)) / 8.0).astype(np.float32)
    w["fc.bias"] = (0.1 * rng.standard_normal(_CLASSES)).astype(np.float32)
    return w


def _geometry_onnx(w):
    from die_amd.utils.onnx_writer import GraphBuilder

    g = GraphBuilder(name="conv_geometry")
    h = g.input("image", ["N"] + list(_IMAGE))
    for name, _, _, (kh, kw), s, attrs in _LAYERS:
        h = g.node("Conv", [h, g.init(name + ".weight", w[name + ".weight"]), g.init(name + ".bias", w[name + ".bias"])],
                   name=name, kernel_shape=[kh, kw], strides=[s, s], **attrs)
        h = g.node("Relu", [h], name=name + "_relu")
    h = g.node("Flatten", [g.node("GlobalAveragePool", [h], name="gap")], name="flatten", axis=1)
    y = g.node("Gemm", [h, g.init("fc.weight", w["fc.weight"]), g.init("fc.bias", w["fc.bias"])], name="fc", transB=1)
    g.output(y, ["N", _CLASSES])
    return g.model_proto(opset=13)


def _geometry_torch(w, x):
    """float64 forward of the same graph, the pads written out (SAME_UPPER: the odd pixel at the end)."""
    import torch
    import torch.nn.functional as F

    h = torch.from_numpy(x).double()
    for name, _, _, (kh, kw), s, attrs in _LAYERS:
        d = attrs.get("dilations", [1, 1])[0]
        if attrs.get("auto_pad") == "SAME_UPPER":
            pads = []
            for size, k in ((h.shape[2], kh), (h.shape[3], kw)):
                total = max(0, (-(-size // s) - 1) * s + (k - 1) * d + 1 - size)
                pads.append((total // 2, total - total // 2))
            (t, b), (l, r) = pads
        else:
            t, l, b, r = attrs["pads"]
        h = F.conv2d(F.pad(h, (l, r, t, b)), torch.from_numpy(w[name + ".weight"]).double(),
                     torch.from_numpy(w[name + ".bias"]).double(), stride=s, dilation=d)
        h = torch.relu(h)
    h = h.mean(dim=(2, 3))
    return (h @ torch.from_numpy(w["fc.weight"]).double().t() + torch.from_numpy(w["fc.bias"]).double()).numpy()


def _rel_l2(a, b):
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))


@pytest.mark.parametrize("precision,bar", [("fp32", 1e-4), ("bf16", 2e-2)])
def test_gpu_conv_geometry_model(native, tmp_path, precision, bar):
    """3x20x28 -> 3x3/s2 pads [0,0,1,1] -> 1x7 -> 7x1 -> dilated 3x3 -> 5x5/s2 SAME_UPPER -> GAP -> Gemm
    on the HIP engine vs torch float64 and the CPU executor, per sample and per logit."""
    w = _geometry_weights()
    path = str(tmp_path / "conv_geometry.onnx")
    with open(path, "wb") as f:
        f.write(_geometry_onnx(w))
    eng = native.Engine(path, device="hip", max_batch=8, precision=precision)
    try:
        for B in (1, 5, 8):
            x = np.random.default_rng(B).standard_normal((B,) + _IMAGE).astype(np.float32)
            ref = _geometry_torch(w, x)
            got = eng.run(x.reshape(B, -1)).astype(np.float64)
            assert got.shape == ref.shape
            assert _rel_l2(got, ref) <= bar, (B, _rel_l2(got, ref))
            # per logit, so that one wrong output cannot hide in the norm
            worst = np.abs(got - ref).max(axis=1) / np.abs(ref).max(axis=1)
            assert (worst <= bar).all(), (B, worst)
            if precision == "fp32":
                cpu = native.cpu_run(path, x).astype(np.float64)
                assert _rel_l2(cpu, ref) <= 1e-4, (B, _rel_l2(cpu, ref))
                assert _rel_l2(got, cpu) <= 1e-4, (B, _rel_l2(got, cpu))
                assert (np.abs(got - cpu).max(axis=1) <= 1e-4 * np.abs(cpu).max(axis=1)).all()
    finally:
        eng.close()
