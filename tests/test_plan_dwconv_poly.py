"""The polyphase depthwise kernel on the planner (no GPU): depthwise convs of the (window, stride) classes that
are turned on (3x3 stride 1 / 2, 5x5 stride 2: profiles/dwconv_poly.md) carry the `poly` mark, the `tiled`
marks stay where they were, EfficientNet-Lite0 has no unmarked depthwise conv, and EngineOptions::poly_dwconv
round-trips.  Numerics on the device: tests/test_gpu_dwconv_poly.py (kernel), tests/test_gpu_efficientnet_lite.py."""
import numpy as np
import pytest

ON = {(3, 1), (3, 2), (5, 2)}  # the classes kern::dwconv_poly_class_on turns on


def test_marks_follow_the_enabled_classes(native, tmp_path):
    from die_amd.utils.onnx_writer import GraphBuilder

    g = GraphBuilder(name="dw_marks")
    rng = np.random.default_rng(0)
    h = g.node("Relu", [g.input("x", ["N", 32, 64, 64])], name="in_relu")
    # name: (window, stride, dilation, groups)
    convs = {"dw3_s1": (3, 1, 1, 32), "dw3_s2": (3, 2, 1, 32), "dw5_s2": (5, 2, 1, 32), "dw5_s1": (5, 1, 1, 32),
             "dw7_s2": (7, 2, 1, 32), "dw3_dil": (3, 1, 2, 32), "g3_w2": (3, 1, 1, 16)}
    for name, (k, stride, dil, groups) in convs.items():
        g.init(name + ".w", rng.normal(0, 0.2, (32, 32 // groups, k, k)).astype(np.float32))
        h = g.node("Conv", [h, name + ".w"], name=name, kernel_shape=[k, k], strides=[stride, stride],
                   dilations=[dil, dil], pads=[dil * (k // 2)] * 4, group=groups)
    g.output(h, ["N", 32, 8, 8])
    path = str(tmp_path / "marks.onnx")
    open(path, "wb").write(g.model_proto(opset=17, ir_version=8))
    for precision in ("fp32", "bf16"):
        ops = {o["name"]: o for o in native.plan_summary(path, 2, precision=precision)["ops"] if o["kind"] == "gconv"}
        assert {n: o["poly"] for n, o in ops.items()} == {
            n: (c[3] == 32 and c[2] == 1 and (c[0], c[1]) in ON) for n, c in convs.items()}
        assert {n for n, o in ops.items() if o["tiled"]} == {"dw5_s1"}
        assert not any(o["mfma"] for o in ops.values())


@pytest.mark.parametrize("size", ["tiny", "full"])
def test_lite0_depthwise_convs_are_all_marked(native, tmp_path, size):
    from die_amd.models import efficientnet_lite as el

    cfg = el.tiny_efficientnet_lite_config() if size == "tiny" else el.EfficientNetLiteConfig()
    path = str(tmp_path / "lite0.onnx")
    open(path, "wb").write(el.build_onnx(cfg)[0])
    r = native.plan_report(path, "fp32")
    assert r["supported"] and not r["unsupported"] and r["blocked"] == 0, r["text"]
    gc = [o for o in native.plan_summary(path, 2, precision="fp32")["ops"] if o["kind"] == "gconv"]
    assert len(gc) == 16 and {(o["KH"], o["stride"]) for o in gc} == ON | {(5, 1)}
    for o in gc:
        assert o["tiled"] == ((o["KH"], o["stride"]) == (5, 1)), o
        assert o["poly"] == ((o["KH"], o["stride"]) in ON), o


def test_option_round_trips(native, tmp_path):
    from die_amd.models import efficientnet_lite as el

    cfg = el.tiny_efficientnet_lite_config()
    path = str(tmp_path / "lite0.onnx")
    open(path, "wb").write(el.build_onnx(cfg)[0])
    x = el.synthetic_input(2, cfg)
    outs = []
    for on in (True, False):
        eng = native.Engine(path, device="cpu", max_batch=2, poly_dwconv=on)
        try:
            assert eng.refresh_info()["options"]["poly_dwconv"] is on
            outs.append(eng.run(x.reshape(2, -1)))
        finally:
            eng.close()
    assert np.array_equal(outs[0], outs[1])  # the CPU executor does not look at the option
