"""ResNeXt on the planner (no GPU): every grouped 3x3 of a bottleneck is one gconv op marked for the MFMA
kernel (kernels/gconv_mfma.hip; every (width, stride) class of its scope is marked, profiles/gconv_mfma.md),
and everything outside that scope stays unmarked.  Numerics on the device: tests/test_gpu_gconv_mfma.py
(kernel), tests/test_gpu_resnext.py (engine)."""
import numpy as np
import pytest


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
@pytest.mark.parametrize("size", ["tiny", "full"])
def test_every_grouped_3x3_is_one_marked_gconv(native, tmp_path, size, precision):
    from die_amd.models import resnext as rx

    cfg = rx.tiny_resnext_config() if size == "tiny" else rx.ResNeXtConfig()
    path = str(tmp_path / "resnext.onnx")
    open(path, "wb").write(rx.build_onnx(cfg)[0])
    r = native.plan_report(path, precision)
    assert r["supported"] and not r["unsupported"] and r["blocked"] == 0, r["text"]
    ops = native.plan_summary(path, 2, precision=precision)["ops"]
    gc = [o for o in ops if o["kind"] == "gconv"]
    want = rx.grouped_convs(cfg)
    assert [o["name"] for o in gc] == ["block%d.conv2" % i for i in range(len(want))]
    assert [(o["groups"], o["stride"], o["KH"]) for o in gc] == [(c["groups"], c["stride"], 3) for c in want]
    assert all(o["mfma"] and not o["tiled"] and not o["residual"] for o in gc), gc
    assert {c["C"] // c["groups"] for c in want} == {4, 8, 16, 32} and sum(c["stride"] == 2 for c in want) == 3


def test_marks_follow_the_kernel_scope(native, tmp_path):
    from die_amd.utils.onnx_writer import GraphBuilder

    g = GraphBuilder(name="gconv_marks")
    rng = np.random.default_rng(0)
    h = g.node("Relu", [g.input("x", ["N", 128, 8, 8])], name="in_relu")
    # name: (groups, window, stride, dilation, expected mark)
    convs = {"w8_s1": (16, 3, 1, 1, True), "w16_s2": (8, 3, 2, 1, True), "depthwise": (128, 3, 1, 1, False),
             "cpg2": (64, 3, 1, 1, False), "w64": (2, 3, 1, 1, False), "dilated": (16, 3, 1, 2, False),
             "five": (16, 5, 1, 1, False)}
    for name, (groups, k, stride, dil, _) in convs.items():
        g.init(name + ".w", rng.normal(0, 0.2, (128, 128 // groups, k, k)).astype(np.float32))
        h = g.node("Conv", [h, name + ".w"], name=name, kernel_shape=[k, k], strides=[stride, stride],
                   dilations=[dil, dil], pads=[dil * (k // 2)] * 4, group=groups)
    g.output(h, ["N", 128, 4, 4])
    path = str(tmp_path / "marks.onnx")
    open(path, "wb").write(g.model_proto(opset=17, ir_version=8))
    for precision in ("fp32", "bf16"):
        ops = native.plan_summary(path, 2, precision=precision)["ops"]
        assert {o["name"]: o["mfma"] for o in ops if o["kind"] == "gconv"} == {n: c[4] for n, c in convs.items()}


def test_mobilenet_has_no_mfma_mark(native, tmp_path):
    from die_amd.models import mobilenet as mb

    path = str(tmp_path / "mobilenet.onnx")
    open(path, "wb").write(mb.build_onnx(mb.tiny_mobilenet_config())[0])
    gc = [o for o in native.plan_summary(path, 2, precision="fp32")["ops"] if o["kind"] == "gconv"]
    assert gc and not any(o["mfma"] for o in gc), gc
