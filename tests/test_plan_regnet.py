"""RegNet on the planner (no GPU): every grouped 3x3 of a block is one gconv op marked for the wide-group MFMA
kernel (kernels/gconv_wide.hip: group widths 24 / 40 / 48 / 56 / 64, any group count), RegNetY's SE blocks are
`se` ops where that op's class rule is on, and everything outside the kernel's scope stays unmarked.  Numerics on
the device: tests/test_gpu_gconv_wide.py (kernel), tests/test_gpu_regnet.py (engine)."""
import numpy as np
import pytest


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
@pytest.mark.parametrize("model", ["tiny_x", "tiny_y", "regnet_y_1_6gf"])
def test_every_grouped_3x3_is_one_wide_gconv(native, tmp_path, model, precision):
    from die_amd.models import regnet as rn

    cfg = rn.CONFIGS[model]() if model in rn.CONFIGS else rn.tiny_regnet_config(se=model == "tiny_y")
    path = str(tmp_path / "regnet.onnx")
    open(path, "wb").write(rn.build_onnx(cfg)[0])
    r = native.plan_report(path, precision)
    assert r["supported"] and not r["unsupported"] and r["blocked"] == 0, r["text"]
    ops = native.plan_summary(path, 2, precision=precision)["ops"]
    gc = [o for o in ops if o["kind"] == "gconv"]
    want = rn.grouped_convs(cfg)
    assert [o["name"] for o in gc] == ["block%d.conv2" % i for i in range(len(want))]
    assert [(o["groups"], o["stride"], o["KH"]) for o in gc] == [(c["groups"], c["stride"], 3) for c in want]
    assert all(o["wide"] and not o["mfma"] and not o["tiled"] and not o["poly"] for o in gc), gc
    # an SE block is one `se` op where the planner's class rule turns it on (C * Cr <= 9600 in fp32 mode, 2400 in
    # bf16: profiles/se_mbconv.md), and the pool + conv + elementwise chain elsewhere
    limit = 9600 if precision == "fp32" else 2400
    assert sum(o["kind"] == "se" for o in ops) == sum(0 < c["C"] * c["se"] <= limit for c in want)
    if model.startswith("tiny"):
        assert {c["C"] // c["groups"] for c in want} == {24, 40, 48, 56, 64}
        assert any(c["C"] % 16 for c in want) and sum(c["stride"] == 2 for c in want) == 3


def test_wide_marks_follow_the_kernel_scope(native, tmp_path):
    from die_amd.utils.onnx_writer import GraphBuilder

    g = GraphBuilder(name="gconv_wide_marks")
    rng = np.random.default_rng(0)
    # name: (channels, groups, window, stride, dilation, expected mark); a 1x1 conv changes the channel count
    convs = {"w24_s1": (192, 8, 3, 1, 1, True), "w64_s2": (192, 3, 3, 2, 1, True), "w32": (192, 6, 3, 1, 1, False),
             "w16": (192, 12, 3, 1, 1, False), "depthwise": (192, 192, 3, 1, 1, False), "dilated": (192, 8, 3, 1, 2, False),
             "five": (192, 8, 5, 1, 1, False), "w56_c168": (168, 3, 3, 1, 1, True), "w72": (144, 2, 3, 1, 1, False)}
    h, cin = g.node("Relu", [g.input("x", ["N", 192, 8, 8])], name="in_relu"), 192
    for name, (C, groups, k, stride, dil, _) in convs.items():
        if C != cin:
            g.init(name + ".pw", rng.normal(0, 0.1, (C, cin, 1, 1)).astype(np.float32))
            h, cin = g.node("Conv", [h, name + ".pw"], name=name + "_pw", kernel_shape=[1, 1]), C
        g.init(name + ".w", rng.normal(0, 0.2, (C, C // groups, k, k)).astype(np.float32))
        h = g.node("Conv", [h, name + ".w"], name=name, kernel_shape=[k, k], strides=[stride, stride],
                   dilations=[dil, dil], pads=[dil * (k // 2)] * 4, group=groups)
    g.output(h, ["N", 144, 4, 4])
    path = str(tmp_path / "marks.onnx")
    open(path, "wb").write(g.model_proto(opset=17, ir_version=8))
    for precision in ("fp32", "bf16"):
        ops = native.plan_summary(path, 2, precision=precision)["ops"]
        assert {o["name"]: o["wide"] for o in ops if o["kind"] == "gconv"} == {n: c[5] for n, c in convs.items()}
