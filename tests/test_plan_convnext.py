"""ConvNeXt on the planner (no GPU): the two channels-last transposes of a block are views of the NHWC
buffer, so a block is a depthwise conv, a row LayerNorm (or its statistics) and two rows GEMMs with the
GELU and the residual in their epilogues; the layer-scale Mul is folded into the second GEMM; the
channels-first LayerNorm of older exports is the same layernorm op on the image's rows; and each form
outside that is rejected with a report line naming the node.  Numerics on the device:
tests/test_gpu_dwconv.py (kernel), tests/test_gpu_convnext.py (engine)."""
import numpy as np
import pytest

SPECS = ["timm", "channels_first_ln", "reduce_mean_head"]
PRECISIONS = ["fp32", "bf16"]


@pytest.fixture(scope="module")
def cn_models(native, tmp_path_factory):
    from die_amd.models import convnext as cn

    d = tmp_path_factory.mktemp("convnext_plan")
    out = {}
    for spec in SPECS:
        cfg = cn.tiny_convnext_config(**cn.SPECS[spec])
        blob, _ = cn.build_onnx(cfg)
        p = str(d / (spec + ".onnx"))
        open(p, "wb").write(blob)
        out[spec] = (p, cfg)
    return out


def _plan(native, path, precision, **kw):
    r = native.plan_report(path, precision)
    assert r["supported"] and not r["unsupported"] and r["blocked"] == 0, r["text"]
    return native.plan_summary(path, 8, precision=precision, **kw)


def _blocks(cfg):
    return ["stages.%d.blocks.%d." % (s, i) for s, d in enumerate(cfg.depths) for i in range(d)]


@pytest.mark.parametrize("spec", SPECS)
@pytest.mark.parametrize("precision", PRECISIONS)
def test_report_is_empty(native, cn_models, spec, precision):
    """Before this lowering every block's Transpose was "unsupported transpose" and the model was cut into
    HIP and CPU pieces."""
    r = native.plan_report(cn_models[spec][0], precision)
    assert r["supported"] and not r["unsupported"] and r["blocked"] == 0 and r["text"] == "", r["text"]
    assert all(seg["device"] == "hip" for seg in native.hybrid_partition(cn_models[spec][0], 8, precision))


@pytest.mark.parametrize("spec", SPECS)
@pytest.mark.parametrize("precision", PRECISIONS)
def test_block_is_four_ops(native, cn_models, spec, precision):
    path, cfg = cn_models[spec]
    ops = _plan(native, path, precision)["ops"]
    kinds = [o["kind"] for o in ops]
    # nothing elementwise, no copy, no transpose anywhere: the transposes and the layer scale left no op
    assert set(kinds) <= {"input_prep", "conv", "layernorm", "gconv", "gap"}, kinds
    assert not any("layer_scale" in o["name"] or "to_nhwc" in o["name"] or "to_nchw" in o["name"] for o in ops)
    for p in _blocks(cfg):
        i = next(k for k, o in enumerate(ops) if o["name"] == p + "dwconv")
        dw, ln, g1, g2 = ops[i:i + 4]
        C = dw["groups"]
        rows = ln["rows"]
        assert dw["kind"] == "gconv" and dw["KH"] == 7 and dw["stride"] == 1 and not dw["residual"]
        assert ln["kind"] == "layernorm" and ln["name"] == p + "norm" and not ln["rms"]
        assert g1["kind"] == "conv" and g1["name"].endswith(p + "pwconv1/MatMul"), g1
        assert (g1["K"], g1["N"], g1["act"], g1["rows"], g1["residual"]) == (C, 4 * C, 2, rows, False), g1  # GELU epilogue
        assert g2["kind"] == "conv" and g2["name"] == p + "pwconv2/MatMul"
        assert (g2["K"], g2["N"], g2["act"], g2["rows"], g2["residual"]) == (4 * C, C, 0, rows, True), g2
        # the LayerNorm reads the conv's buffer in place (the transpose copied nothing), the GEMMs chain, and
        # the shortcut is the NHWC buffer the depthwise conv read
        assert ln["bufs"]["in"] == dw["bufs"]["out"]
        assert g1["bufs"]["in"] == (dw["bufs"]["out"] if g1["layernorm_folded"] else ln["bufs"]["out"])
        assert g2["bufs"]["in"] == g1["bufs"]["out"] and g2["bufs"]["in2"] == dw["bufs"]["in"]
    # launches: stem (prep, conv, LN), 4 per block, 2 per downsample, head (pool, LN, FC)
    assert len(ops) == 3 + 4 * sum(cfg.depths) + 2 * (len(cfg.depths) - 1) + 3, kinds


@pytest.mark.parametrize("spec", SPECS)
@pytest.mark.parametrize("precision", PRECISIONS)
def test_layer_scale_leaves_no_op(native, cn_models, spec, precision):
    """x (W2 gamma) + b2 gamma at plan time: the Mul is no affine / binary op, and the only GEMMs are the stem,
    two per block, one per downsample and the FC."""
    path, cfg = cn_models[spec]
    kinds = [o["kind"] for o in _plan(native, path, precision)["ops"]]
    assert kinds.count("conv") == 1 + 2 * sum(cfg.depths) + (len(cfg.depths) - 1) + 1, kinds
    assert not {"affine", "binary", "unary", "copy_cols"} & set(kinds), kinds


def test_layer_scale_with_a_second_reader_is_kept(native, tmp_path):
    """the GEMM's unscaled output has another reader (here: the graph's second use), so the Mul stays an op"""
    def body(g, x, rng):
        h = _dw(g, x, rng, 16, 7, 1, 3, "dw")
        v = g.node("Transpose", [h], name="to_nhwc", perm=[0, 2, 3, 1])
        g.init("fc.w", rng.normal(0, 0.2, (16, 16)).astype(np.float32))
        g.init("gamma", rng.uniform(0.5, 1.5, 16).astype(np.float32))
        m = g.node("MatMul", [v, "fc.w"], name="fc")
        s = g.node("Mul", [m, "gamma"], name="layer_scale")
        y = g.node("Add", [s, m], name="both")
        return g.node("Transpose", [y], name="to_nchw", perm=[0, 3, 1, 2]), [16, 8, 8]

    ops = _plan(native, _graph(tmp_path, "ls_kept", body), "fp32")["ops"]
    assert [o["kind"] for o in ops].count("conv") == 1
    assert [o["kind"] for o in ops if o["name"] == "layer_scale"] == ["affine"], ops


@pytest.mark.parametrize("spec", SPECS)
def test_fold_layernorm_takes_the_block_norm_not_the_downsample_norm(native, cn_models, spec):
    """fold_layernorm (fp32): pwconv1 is a rows GEMM and the only reader of the block's LayerNorm, so the norm
    becomes a statistics op where the pass's own conditions hold (K a multiple of 64: no K padding).  One
    output pixel of the 2x2 stride-2 downsample conv spans four rows with four different statistics: never
    folded.  Off, or in bf16: nothing is folded."""
    path, cfg = cn_models[spec]
    ops = _plan(native, path, "fp32", fold_layernorm=True)["ops"]
    by = {o["name"]: o for o in ops}
    for s, (depth, C) in enumerate(zip(cfg.depths, cfg.dims)):
        for i in range(depth):
            p = "stages.%d.blocks.%d." % (s, i)
            ln = by[p + "norm"]
            g1 = next(o for o in ops if o["name"].endswith(p + "pwconv1/MatMul"))
            assert ln["stats_only"] == (C % 64 == 0) and g1["layernorm_folded"] == (C % 64 == 0), (p, ln, g1)
    down = [o for o in ops if "downsample.norm" in o["name"]]
    assert len(down) == len(cfg.depths) - 1 and not any(o["stats_only"] for o in down), down
    for o in ops:
        if o["kind"] == "conv" and "downsample.conv" in o["name"]:
            assert not o["layernorm_folded"] and o["KH"] == 2 and o["stride"] == 2, o
    for kw, precision in (({"fold_layernorm": False}, "fp32"), ({"fold_layernorm": True}, "bf16")):
        ops = _plan(native, path, precision, **kw)["ops"]
        assert not any(o["kind"] == "layernorm" and o["stats_only"] for o in ops)
        assert not any(o["kind"] == "conv" and o["layernorm_folded"] for o in ops)


@pytest.mark.parametrize("spec", SPECS)
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("fuse_gap_fc", [False, True])
def test_head_layernorm_is_one_row_and_feeds_the_fc(native, cn_models, spec, precision, fuse_gap_fc):
    path, cfg = cn_models[spec]
    s = _plan(native, path, precision, fuse_gap_fc=fuse_gap_fc, fold_layernorm=False)
    ops = s["ops"]
    gap, ln, fc = ops[-3:]
    # the pooled vector has the LayerNorm as its reader: the pool + FC fusion must leave it alone
    assert [gap["kind"], ln["kind"], fc["kind"]] == ["gap", "layernorm", "conv"], [o["kind"] for o in ops[-4:]]
    assert ln["rows"] == 1 and not ln["stats_only"] and "head.norm" in ln["name"]
    assert ln["bufs"]["in"] == gap["bufs"]["out"] and fc["bufs"]["in"] == ln["bufs"]["out"]
    assert (fc["K"], fc["rows"]) == (cfg.dims[-1], 1) and fc["name"] == "head.fc"
    assert s["output_shape"] == [1, cfg.num_classes]
    # stem and downsample norms run over the image's rows
    stem = next(o for o in ops if o["name"].startswith("stem.norm"))
    assert stem["kind"] == "layernorm" and stem["rows"] == (cfg.image // 4) ** 2


@pytest.mark.parametrize("spec", SPECS)
def test_eligible_convs_carry_the_tiled_mark(native, cn_models, spec):
    path, cfg = cn_models[spec]
    dws = [o for o in _plan(native, path, "fp32")["ops"] if o["kind"] == "gconv"]
    assert len(dws) == sum(cfg.depths) and all(o["tiled"] for o in dws), dws


# ---- small hand-built graphs ----------------------------------------------------------------------------

def _graph(tmp_path, name, body, C=16, hw=8, out_dims=None):
    """input [N, C, hw, hw] -> Relu (an NHWC activation: a grouped conv does not read the graph input) ->
    body(g, x, rng) -> output"""
    from die_amd.utils.onnx_writer import GraphBuilder

    g = GraphBuilder(name=name)
    rng = np.random.default_rng(0)
    x = g.node("Relu", [g.input("x", ["N", C, hw, hw])], name="in_relu")
    y, dims = body(g, x, rng)
    g.output(y, ["N"] + dims)
    p = str(tmp_path / (name + ".onnx"))
    open(p, "wb").write(g.model_proto(opset=17, ir_version=8))
    return p


def _dw(g, x, rng, C, k, stride, pad, name):
    g.init(name + ".w", rng.normal(0, 0.2, (C, 1, k, k)).astype(np.float32))
    g.init(name + ".b", rng.normal(0, 0.1, C).astype(np.float32))
    return g.node("Conv", [x, name + ".w", name + ".b"], name=name, kernel_shape=[k, k], strides=[stride, stride],
                  pads=[pad] * 4, group=C)


def test_mobilenet_style_depthwise_convs_are_not_marked(native, tmp_path):
    """3x3, strided and dilated depthwise convs stay with gconv_kernel; 5x5 and 7x7 stride 1 are marked."""
    def body(g, x, rng):
        h = _dw(g, x, rng, 16, 3, 1, 1, "dw3")
        h = _dw(g, h, rng, 16, 5, 1, 2, "dw5")
        h = _dw(g, h, rng, 16, 7, 1, 3, "dw7")
        g.init("dil.w", rng.normal(0, 0.2, (16, 1, 5, 5)).astype(np.float32))
        h = g.node("Conv", [h, "dil.w"], name="dw5_dilated", kernel_shape=[5, 5], dilations=[2, 2], pads=[4] * 4, group=16)
        g.init("grp.w", rng.normal(0, 0.2, (16, 2, 7, 7)).astype(np.float32))
        h = g.node("Conv", [h, "grp.w"], name="grouped7", kernel_shape=[7, 7], pads=[3] * 4, group=8)
        h = _dw(g, h, rng, 16, 7, 2, 3, "dw7_s2")
        return h, [16, 4, 4]

    p = _graph(tmp_path, "dw_marks", body)
    for precision in PRECISIONS:
        ops = _plan(native, p, precision)["ops"]
        marks = {o["name"]: o["tiled"] for o in ops if o["kind"] == "gconv"}
        assert marks == {"dw3": False, "dw5": True, "dw7": True, "dw5_dilated": False, "grouped7": False,
                         "dw7_s2": False}, marks


def test_mobilenet_plan_has_no_tiled_conv(native, tmp_path):
    from die_amd.models import mobilenet as mb

    blob, _ = mb.build_onnx(mb.tiny_mobilenet_config())
    p = str(tmp_path / "mbv2.onnx")
    open(p, "wb").write(blob)
    dws = [o for o in _plan(native, p, "fp32")["ops"] if o["kind"] == "gconv"]
    assert dws and not any(o["tiled"] for o in dws)


def _ln(g, x, rng, C, name, axis=-1):
    g.init(name + ".w", rng.uniform(0.8, 1.2, C).astype(np.float32))
    g.init(name + ".b", rng.normal(0, 0.05, C).astype(np.float32))
    return g.node("LayerNormalization", [x, name + ".w", name + ".b"], name=name, axis=axis, epsilon=1e-6)


def _rejected(native, path, node):
    for precision in PRECISIONS:
        r = native.plan_report(path, precision)
        assert not r["supported"], r
        assert any(it["node"] == node for it in r["unsupported"]), r["text"]
        assert node in r["text"]
    return r


def test_other_image_permutes_are_rejected(native, tmp_path):
    for perm in ([0, 3, 2, 1], [0, 2, 1, 3], [0, 1, 3, 2]):
        def body(g, x, rng):
            h = _dw(g, x, rng, 16, 7, 1, 3, "dw")
            h = g.node("Transpose", [h], name="odd_permute", perm=perm)
            return g.node("Relu", [h], name="relu"), [8, 8, 16]

        r = _rejected(native, _graph(tmp_path, "perm%d%d%d" % tuple(perm[1:]), body), "odd_permute")
        assert "unsupported transpose" in r["text"]


def test_back_transpose_needs_the_view(native, tmp_path):
    """Transpose(0,3,1,2) of an image (not of an [N,H,W,C] view) is some other permute"""
    def body(g, x, rng):
        h = _dw(g, x, rng, 16, 7, 1, 3, "dw")
        h = g.node("Transpose", [h], name="not_a_view", perm=[0, 3, 1, 2])
        return g.node("Relu", [h], name="relu"), [8, 16, 8]

    _rejected(native, _graph(tmp_path, "backonly", body), "not_a_view")


def test_view_as_graph_output_is_rejected(native, tmp_path):
    def direct(g, x, rng):
        h = _dw(g, x, rng, 16, 7, 1, 3, "dw")
        return g.node("Transpose", [h], name="to_nhwc", perm=[0, 2, 3, 1]), [8, 8, 16]

    r = _rejected(native, _graph(tmp_path, "view_out", direct), "to_nhwc")
    assert "graph output" in r["text"]

    def after_ln(g, x, rng):
        h = _dw(g, x, rng, 16, 7, 1, 3, "dw")
        h = g.node("Transpose", [h], name="to_nhwc", perm=[0, 2, 3, 1])
        return _ln(g, h, rng, 16, "norm_out"), [8, 8, 16]

    r = _rejected(native, _graph(tmp_path, "view_ln_out", after_ln), "norm_out")
    assert "graph output" in r["text"]


def test_layernorm_over_another_axis_is_rejected(native, tmp_path):
    def on_view(g, x, rng):  # axis 2 (W) of the [N, H, W, C] view
        h = _dw(g, x, rng, 8, 7, 1, 3, "dw")
        h = g.node("Transpose", [h], name="to_nhwc", perm=[0, 2, 3, 1])
        h = _ln(g, h, rng, 8, "norm_w", axis=2)
        return g.node("Transpose", [h], name="to_nchw", perm=[0, 3, 1, 2]), [8, 8, 8]

    _rejected(native, _graph(tmp_path, "ln_axis2", on_view, C=8), "norm_w")

    def on_image(g, x, rng):  # decomposed, over axis 2 (H) of the NCHW image
        h = _dw(g, x, rng, 8, 7, 1, 3, "dw")
        two = g.const(np.array(2.0, np.float32), "two")
        eps = g.const(np.array(1e-6, np.float32), "eps")
        mu = g.node("ReduceMean", [h], name="mean_h", axes=[2], keepdims=1)
        d = g.node("Sub", [h, mu], name="sub")
        var = g.node("ReduceMean", [g.node("Pow", [d, two], name="pow")], name="var", axes=[2], keepdims=1)
        sd = g.node("Sqrt", [g.node("Add", [var, eps], name="add_eps")], name="sqrt")
        return g.node("Div", [d, sd], name="div"), [8, 8, 8]

    r = _rejected(native, _graph(tmp_path, "ln_axis_h", on_image, C=8), "mean_h")
    assert "channel axis" in r["text"]


def test_channels_first_layernorm_alone(native, tmp_path):
    """the decomposed form over axis 1 of an image is one layernorm op over its rows, also away from ConvNeXt"""
    def body(g, x, rng):
        h = _dw(g, x, rng, 16, 7, 1, 3, "dw")
        two = g.const(np.array(2.0, np.float32), "two")
        eps = g.const(np.array(1e-6, np.float32), "eps")
        wc = g.const(rng.uniform(0.8, 1.2, (16, 1, 1)).astype(np.float32), "w")
        bc = g.const(rng.normal(0, 0.05, (16, 1, 1)).astype(np.float32), "b")
        mu = g.node("ReduceMean", [h], name="cf_norm", axes=[1], keepdims=1)
        d = g.node("Sub", [h, mu], name="sub")
        var = g.node("ReduceMean", [g.node("Pow", [d, two], name="pow")], name="var", axes=[1], keepdims=1)
        sd = g.node("Sqrt", [g.node("Add", [var, eps], name="add_eps")], name="sqrt")
        y = g.node("Add", [g.node("Mul", [g.node("Div", [d, sd], name="div"), wc], name="scale"), bc], name="shift")
        return y, [16, 8, 8]

    p = _graph(tmp_path, "cf_ln", body)
    for precision in PRECISIONS:
        s = _plan(native, p, precision)
        assert [o["kind"] for o in s["ops"]] == ["input_prep", "affine", "gconv", "layernorm", "to_nchw_f32"]
        assert s["ops"][3]["rows"] == 64 and s["output_shape"] == [1, 16, 8, 8]
