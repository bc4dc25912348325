"""Squeeze-excitation on the planner (no GPU): the tiny EfficientNet-B0 / MobileNetV3 models of
models/mbconv_se.py plan, in both precisions, with one `se` op per SE block and every activation in an epilogue
(no unary / binary op); fuse_se = False brings the unfused chain back; chains outside the pattern keep the
lowering they had.  Numerics on the device: tests/test_gpu_se.py (kernel), tests/test_gpu_mbconv_se.py."""
import numpy as np
import pytest

ARCHS = ["efficientnet_b0", "mobilenet_v3_large"]


def _tiny(tmp_path, arch):
    from die_amd.models import mbconv_se as ms

    cfg = ms.tiny_config(arch)
    path = str(tmp_path / (arch + ".onnx"))
    open(path, "wb").write(ms.build_onnx(cfg)[0])
    return ms, cfg, path


def _kinds(native, path, precision, **kw):
    return [o["kind"] for o in native.plan_summary(path, 2, precision=precision, **kw)["ops"]]


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
@pytest.mark.parametrize("arch", ARCHS)
def test_tiny_models_plan_with_one_se_op_per_block(native, tmp_path, arch, precision):
    ms, cfg, path = _tiny(tmp_path, arch)
    r = native.plan_report(path, precision)
    assert r["supported"] and not r["unsupported"] and r["blocked"] == 0, r["text"]
    ops = native.plan_summary(path, 2, precision=precision)["ops"]
    se = [o for o in ops if o["kind"] == "se"]
    assert [(o["C"], o["Cr"], o["rows"]) for o in se] == [(C, Cr, s * s) for s, C, Cr in ms.se_shapes(cfg)] and len(se) >= 2
    b0 = arch == "efficientnet_b0"
    assert {(o["act1"], o["act2"]) for o in se} == ({(4, 0)} if b0 else {(1, 1)})
    kinds = [o["kind"] for o in ops]
    # MobileNetV3's classifier has a HardSwish behind a Linear: Gemm epilogues are not in this change's scope
    assert not set(kinds) & {"binary", "affine"} and kinds.count("unary") == (0 if b0 else 1), kinds
    acts = {o["act"] for o in ops if o["kind"] in ("conv", "gconv")}
    assert acts == ({0, 4} if b0 else {0, 1, 5}), acts
    off = _kinds(native, path, precision, fuse_se=False)
    assert "se" not in off and "binary" in off and off.count("gap") == len(se) + 1


def test_full_size_models_plan(native, tmp_path):
    """the mark rule: blocks of at most 9600 (fp32) / 2400 (bf16) FC weights are fused, the others keep the chain"""
    from die_amd.models import mbconv_se as ms

    for arch, n_se in (("efficientnet_b0", 16), ("mobilenet_v3_large", 8)):
        cfg = ms.MbconvSeConfig(arch)
        path = str(tmp_path / (arch + ".onnx"))
        open(path, "wb").write(ms.build_onnx(cfg)[0])
        assert len(ms.se_shapes(cfg)) == n_se
        for precision, cap in (("fp32", 9600), ("bf16", 2400)):
            kinds = _kinds(native, path, precision)
            on = sum(C * Cr <= cap for _, C, Cr in ms.se_shapes(cfg))
            assert 0 < on < n_se and kinds.count("se") == on and kinds.count("binary") == n_se - on, (arch, precision)


@pytest.mark.parametrize("variant", ["gate_read_twice", "pool_read_twice", "x_read_by_a_third", "padded_x", "gemm_form"])
def test_chains_outside_the_pattern_keep_their_lowering(native, tmp_path, variant):
    """each still plans, without an se op and without a report line"""
    from die_amd.utils.onnx_writer import GraphBuilder

    rng = np.random.default_rng(1)
    C = 20 if variant == "padded_x" else 24  # 20 channels are stored as 24
    g = GraphBuilder(name=variant)
    for name, shape in (("c.w", (C, 8, 3, 3)), ("se1.w", (4, C, 1, 1)), ("se1.b", (4,)), ("se2.w", (C, 4, 1, 1)), ("se2.b", (C,)),
                        ("fc1.w", (4, C)), ("fc2.w", (C, 4))):
        g.init(name, rng.normal(0, 0.3, shape).astype(np.float32))
    x = g.node("Relu", [g.node("Conv", [g.input("x", ["N", 8, 8, 8]), "c.w"], name="c", kernel_shape=[3, 3], pads=[1] * 4)], name="r")
    pool = g.node("GlobalAveragePool", [x], name="pool")
    if variant == "gemm_form":
        z = g.node("Gemm", [g.node("Flatten", [pool], name="fl", axis=1), "fc1.w"], name="fc1", transB=1)
        z = g.node("Gemm", [g.node("Relu", [z], name="fr"), "fc2.w"], name="fc2", transB=1)
        gate = g.node("Reshape", [g.node("Sigmoid", [z], name="gate"), g.const(np.array([0, C, 1, 1], np.int64), "shp")], name="rs")
    else:
        z = g.node("Relu", [g.node("Conv", [pool, "se1.w", "se1.b"], name="se1", kernel_shape=[1, 1])], name="se_relu")
        gate = g.node("Sigmoid", [g.node("Conv", [z, "se2.w", "se2.b"], name="se2", kernel_shape=[1, 1])], name="gate")
    y = g.node("Mul", [x, gate], name="scale")
    if variant == "gate_read_twice":
        y = g.node("Mul", [y, gate], name="scale2")
    if variant == "pool_read_twice":
        y = g.node("Add", [y, pool], name="plus_pool")
    if variant == "x_read_by_a_third":
        y = g.node("Add", [y, x], name="plus_x")
    g.output(y, ["N", C, 8, 8])
    path = str(tmp_path / (variant + ".onnx"))
    open(path, "wb").write(g.model_proto(opset=14, ir_version=7))
    for precision in ("fp32", "bf16"):
        r = native.plan_report(path, precision)
        assert r["supported"] and not r["unsupported"], r["text"]
        kinds = _kinds(native, path, precision)
        assert "se" not in kinds and "gap" in kinds and "binary" in kinds, kinds


def test_option_round_trips(native, tmp_path):
    ms, cfg, path = _tiny(tmp_path, "mobilenet_v3_large")
    for on in (True, False):
        eng = native.Engine(path, device="cpu", max_batch=2, fuse_se=on)
        try:
            assert eng.refresh_info()["options"]["fuse_se"] is on
        finally:
            eng.close()
