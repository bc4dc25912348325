"""ConvNeXt-V2 on the planner (no GPU): the exported Global Response Normalization chain (ReduceL2 over the
spatial axes, ReduceMean over the channels, Add(eps), Div, Mul, Mul, Add, Add) is one `grn` op on the
[N,H,W,C] rows view between the two rows GEMMs of a block, in both export forms (timm: parameters [C] and
Add(bias, .) -> Add(x, .); HF: parameters [1,1,1,C] and Add(., bias) -> Add(., x)); the channels-first form
is the same op on an image; and each form outside that is rejected with a report line naming the node.
Numerics on the device: tests/test_gpu_grn.py (kernel), tests/test_gpu_convnextv2.py (engine)."""
import numpy as np
import pytest

SPECS = ["timm", "hf"]
PRECISIONS = ["fp32", "bf16"]


@pytest.fixture(scope="module")
def v2_models(native, tmp_path_factory):
    from die_amd.models import convnextv2 as v2

    d = tmp_path_factory.mktemp("convnextv2_plan")
    out = {}
    for spec in SPECS:
        cfg = v2.tiny_convnextv2_config(**v2.SPECS[spec])
        blob, _ = v2.build_onnx(cfg)
        p = str(d / (spec + ".onnx"))
        open(p, "wb").write(blob)
        out[spec] = (p, cfg)
    return out


def _plan(native, path, precision, **kw):
    r = native.plan_report(path, precision)
    assert r["supported"] and not r["unsupported"] and r["blocked"] == 0, r["text"]
    return native.plan_summary(path, 8, precision=precision, **kw)


@pytest.mark.parametrize("spec", SPECS)
@pytest.mark.parametrize("precision", PRECISIONS)
def test_report_is_empty(native, v2_models, spec, precision):
    """Before this lowering every block's ReduceL2 was rejected by the F.normalize lowering and the model was
    cut into HIP and CPU pieces."""
    r = native.plan_report(v2_models[spec][0], precision)
    assert r["supported"] and not r["unsupported"] and r["blocked"] == 0 and r["text"] == "", r["text"]
    assert all(seg["device"] == "hip" for seg in native.hybrid_partition(v2_models[spec][0], 8, precision))


@pytest.mark.parametrize("spec", SPECS)
@pytest.mark.parametrize("precision", PRECISIONS)
def test_block_is_five_ops(native, v2_models, spec, precision):
    path, cfg = v2_models[spec]
    ops = _plan(native, path, precision)["ops"]
    kinds = [o["kind"] for o in ops]
    # nothing is left over from the chain: no elementwise op, no reduction, no copy
    assert set(kinds) <= {"input_prep", "conv", "layernorm", "gconv", "grn", "gap"}, kinds
    assert not {"binary", "unary", "affine", "pool_tokens"} & set(kinds), kinds
    assert kinds.count("grn") == sum(cfg.depths)
    assert not any(t in o["name"] for o in ops for t in ("/mean", "/add_eps", "/div", "/mul_x", "/scale", "/shift", "grn/residual"))
    size = cfg.image // 4
    for s, (depth, C) in enumerate(zip(cfg.depths, cfg.dims)):
        for i in range(depth):
            p = "stages.%d.blocks.%d." % (s, i)
            k = next(k for k, o in enumerate(ops) if o["name"] == p + "dwconv")
            dw, ln, g1, grn, g2 = ops[k:k + 5]
            assert [o["kind"] for o in (dw, ln, g1, grn, g2)] == ["gconv", "layernorm", "conv", "grn", "conv"], p
            rows = size * size
            assert g1["name"].endswith(p + "pwconv1/MatMul") and (g1["K"], g1["N"], g1["act"], g1["rows"]) == (C, 4 * C, 2, rows), g1
            assert grn["name"] == p + "grn/norm" and (grn["C"], grn["rows"]) == (4 * C, rows), grn
            assert grn["eps"] == pytest.approx(cfg.grn_eps, rel=1e-6) and grn["gamma"] and grn["beta"]
            # it reads pwconv1's output, writes a buffer of its own and has a workspace; pwconv2 reads its
            # output and still takes the block's shortcut in its residual epilogue
            assert grn["bufs"]["in"] == g1["bufs"]["out"] and grn["bufs"]["out"] != grn["bufs"]["in"]
            assert grn["bufs"]["out2"][1] > grn["bufs"]["out2"][0]
            assert g2["name"] == p + "pwconv2/MatMul" and g2["bufs"]["in"] == grn["bufs"]["out"]
            assert (g2["K"], g2["N"], g2["act"], g2["rows"], g2["residual"]) == (4 * C, C, 0, rows, True), g2
            assert g2["bufs"]["in2"] == dw["bufs"]["in"]
        size //= 2
    # launches: stem (prep, conv, LN), 5 per block, 2 per downsample, head (pool, LN, FC)
    assert len(ops) == 3 + 5 * sum(cfg.depths) + 2 * (len(cfg.depths) - 1) + 3, kinds


@pytest.mark.parametrize("precision", PRECISIONS)
def test_both_forms_plan_the_same_parameters(native, v2_models, precision):
    """[C] and [1,1,1,C] parameters, either Add order: the same ops, buffers and parameter blob"""
    a = native.plan_dump(v2_models["timm"][0], 8, precision=precision).splitlines()
    b = native.plan_dump(v2_models["hf"][0], 8, precision=precision).splitlines()
    assert a == b and sum("grn/norm" in ln for ln in a) == sum(v2_models["timm"][1].depths)


@pytest.mark.parametrize("spec", SPECS)
def test_fold_layernorm_still_takes_the_block_norm(native, v2_models, spec):
    """GRN sits behind pwconv1, so the block LayerNorm is still read by pwconv1 alone: statistics only in
    fp32 where the pass's conditions hold (K a multiple of 64), untouched in bf16 or with the pass off"""
    path, cfg = v2_models[spec]
    ops = _plan(native, path, "fp32", fold_layernorm=True)["ops"]
    by = {o["name"]: o for o in ops}
    for s, (depth, C) in enumerate(zip(cfg.depths, cfg.dims)):
        for i in range(depth):
            p = "stages.%d.blocks.%d." % (s, i)
            g1 = next(o for o in ops if o["name"].endswith(p + "pwconv1/MatMul"))
            assert by[p + "norm"]["stats_only"] == (C % 64 == 0) and g1["layernorm_folded"] == (C % 64 == 0), p
    assert any(o["kind"] == "layernorm" and o["stats_only"] for o in ops)
    for kw, precision in (({"fold_layernorm": False}, "fp32"), ({"fold_layernorm": True}, "bf16")):
        ops = _plan(native, path, precision, **kw)["ops"]
        assert not any(o["kind"] == "layernorm" and o["stats_only"] for o in ops)
        assert [o["kind"] for o in ops].count("grn") == sum(cfg.depths)


# ---- small hand-built graphs ----------------------------------------------------------------------------

def _graph(tmp_path, name, body, C=16, hw=4):
    """input [N, C, hw, hw] -> Relu (an NHWC activation) -> body(g, x, rng) -> output"""
    from die_amd.utils.onnx_writer import GraphBuilder

    g = GraphBuilder(name=name)
    rng = np.random.default_rng(0)
    x = g.node("Relu", [g.input("x", ["N", C, hw, hw])], name="in_relu")
    y, dims = body(g, x, rng)
    g.output(y, ["N"] + dims)
    p = str(tmp_path / (name + ".onnx"))
    open(p, "wb").write(g.model_proto(opset=17, ir_version=8))
    return p


def _conv1x1(g, x, rng, cin, cout, name):
    g.init(name + ".w", rng.normal(0, 0.2, (cout, cin, 1, 1)).astype(np.float32))
    g.init(name + ".b", rng.normal(0, 0.1, cout).astype(np.float32))
    return g.node("Conv", [x, name + ".w", name + ".b"], name=name, kernel_shape=[1, 1])


def _grn(g, x, rng, C, shape, spatial, channel, name="grn", **kw):
    """the chain of models/convnextv2.py with random parameters of the given shape"""
    from die_amd.models import convnextv2 as v2

    w = g.const(rng.uniform(0.5, 1.5, C).astype(np.float32).reshape(shape), name + ".w")
    b = g.const(rng.normal(0, 0.05, C).astype(np.float32).reshape(shape), name + ".b")
    eps = g.const(np.array(1e-6, np.float32), name + ".eps")
    return v2.grn_nodes(g, x, w, b, eps, name, spatial=spatial, channel=channel, **kw)


@pytest.mark.parametrize("shape,spatial,channel,spec", [
    ((1, 16, 1, 1), (2, 3), 1, "timm"), ((16, 1, 1), (2, 3), 1, "hf"), ((1, 16, 1, 1), (-2, -1), -3, "hf")])
@pytest.mark.parametrize("precision", PRECISIONS)
def test_channels_first_form_is_one_op_on_the_image(native, tmp_path, shape, spatial, channel, spec, precision):
    """timm's channels_last=False: axes [2,3] and the mean over axis 1 of the NCHW value, parameters [1,C,1,1] or
    [C,1,1] -- the same NHWC buffer, the same op, between two convs"""
    def body(g, x, rng):
        h = _conv1x1(g, x, rng, 16, 16, "conv_a")
        h = _grn(g, h, rng, 16, shape, spatial, channel, spec=spec)
        return _conv1x1(g, h, rng, 16, 8, "conv_b"), [8, 4, 4]

    s = _plan(native, _graph(tmp_path, "cf_grn", body), precision)
    assert [o["kind"] for o in s["ops"]] == ["input_prep", "affine", "conv", "grn", "conv", "to_nchw_f32"], s["ops"]
    a, grn, b = s["ops"][2:5]
    assert (grn["C"], grn["rows"]) == (16, 16) and grn["bufs"]["in"] == a["bufs"]["out"] and b["bufs"]["in"] == grn["bufs"]["out"]


@pytest.mark.parametrize("weight,bias", [(False, True), (True, False), (False, False)])
def test_parameters_may_be_absent(native, tmp_path, weight, bias):
    from die_amd.models import convnextv2 as v2

    def body(g, x, rng):
        h = g.node("Transpose", [x], name="to_nhwc", perm=[0, 2, 3, 1])
        w = g.const(rng.uniform(0.5, 1.5, 16).astype(np.float32), "w") if weight else None
        b = g.const(rng.normal(0, 0.05, 16).astype(np.float32), "b") if bias else None
        h = v2.grn_nodes(g, h, w, b, g.const(np.array(1e-3, np.float32), "eps"), "grn", "hf")
        return g.node("Transpose", [h], name="to_nchw", perm=[0, 3, 1, 2]), [16, 4, 4]

    ops = _plan(native, _graph(tmp_path, "absent", body), "fp32")["ops"]
    grn = [o for o in ops if o["kind"] == "grn"]
    assert len(grn) == 1 and grn[0]["beta"] == bias and grn[0]["eps"] == pytest.approx(1e-3, rel=1e-6), ops
    assert not {"binary", "unary"} & {o["kind"] for o in ops} and [o["kind"] for o in ops].count("affine") == 1


def test_axes_as_inputs(native, tmp_path):
    """opset 18: the axes of ReduceL2 and ReduceMean are inputs; Add(eps, .) and Mul(nx, x) in the other order"""
    from die_amd.utils.onnx_writer import GraphBuilder

    g = GraphBuilder(name="axes_inputs")
    rng = np.random.default_rng(0)
    x = g.node("Relu", [g.input("x", ["N", 16, 4, 4])], name="in_relu")
    v = g.node("Transpose", [x], name="to_nhwc", perm=[0, 2, 3, 1])
    G = g.node("ReduceL2", [v, g.const(np.array([1, 2], np.int64), "spatial")], name="grn/norm", keepdims=1)
    mu = g.node("ReduceMean", [G, g.const(np.array([3], np.int64), "channel")], name="grn/mean", keepdims=1)
    nx = g.node("Div", [G, g.node("Add", [g.const(np.array(1e-6, np.float32), "eps"), mu], name="grn/add_eps")], name="grn/div")
    y = g.node("Mul", [nx, v], name="grn/mul_x")
    w, b = rng.uniform(0.5, 1.5, (1, 1, 1, 16)).astype(np.float32), rng.normal(0, 0.05, 16).astype(np.float32)
    y = g.node("Mul", [y, g.const(w, "w")], name="grn/scale")
    y = g.node("Add", [g.const(b, "b"), y], name="grn/shift")
    y = g.node("Add", [y, v], name="grn/residual")
    g.output(g.node("Transpose", [y], name="to_nchw", perm=[0, 3, 1, 2]), ["N", 16, 4, 4])
    p = str(tmp_path / "axes_inputs.onnx")
    open(p, "wb").write(g.model_proto(opset=18, ir_version=8))
    for precision in PRECISIONS:
        ops = _plan(native, p, precision)["ops"]
        assert [o["kind"] for o in ops] == ["input_prep", "affine", "grn", "to_nchw_f32"], ops
        assert (ops[2]["C"], ops[2]["rows"], ops[2]["gamma"], ops[2]["beta"]) == (16, 16, True, True)
    # and the CPU executor, the oracle of the engine tests, computes the expression on this form too
    xs = rng.standard_normal((2, 16, 4, 4)).astype(np.float32)
    got = native.cpu_run(p, xs)
    r = np.maximum(xs, 0).transpose(0, 2, 3, 1).astype(np.float64)
    Gn = np.sqrt((r * r).sum(axis=(1, 2), keepdims=True))
    ref = (w * (r * (Gn / (Gn.mean(axis=-1, keepdims=True) + 1e-6))) + b + r).transpose(0, 3, 1, 2)
    assert got.shape == ref.shape and float(np.linalg.norm(got - ref) / np.linalg.norm(ref)) < 1e-5


def _reject_bodies():
    """case -> (body, channels of the input, the node the report names, a word of its reason)"""
    from die_amd.models import convnextv2 as v2

    def chain(g, x, rng, C=16, axes=(1, 2), keepdims=1, mean_axis=-1, eps=None, w="vec", b="vec", residual=None,
              extra=None):
        """the HF chain on the [N, H, W, C] view of x, node by node, so that one piece can be bent"""
        v = g.node("Transpose", [x], name="to_nhwc", perm=[0, 2, 3, 1])
        G = g.node("ReduceL2", [v], name="grn/norm", axes=list(axes), keepdims=keepdims)
        mu = g.node("ReduceMean", [G], name="grn/mean", axes=[mean_axis], keepdims=1)
        eps = eps if eps is not None else g.const(np.array(1e-6, np.float32), "eps")
        nx = g.node("Div", [G, g.node("Add", [mu, eps], name="grn/add_eps")], name="grn/div")
        y = m = g.node("Mul", [v, nx], name="grn/mul_x")
        wv = {"vec": lambda: g.const(rng.uniform(0.5, 1.5, C).astype(np.float32), "w"),
              "scalar": lambda: g.const(np.array([1.5], np.float32), "w")}[w]()
        y = g.node("Mul", [wv, y], name="grn/scale")
        bv = {"vec": lambda: g.const(rng.normal(0, 0.05, C).astype(np.float32), "b"),
              "computed": lambda: g.node("Identity", [g.const(np.zeros(C, np.float32), "b0")], name="bias_of")}[b]()
        y = g.node("Add", [y, bv], name="grn/shift")
        y = g.node("Add", [y, v if residual is None else residual(g, x)], name="grn/residual")
        if extra == "mul_x":
            y = g.node("Add", [y, g.node("Neg", [m], name="side")], name="sum")
        if extra == "norm":
            y = g.node("Mul", [y, G], name="times_norm")
        return g.node("Transpose", [y], name="to_nchw", perm=[0, 3, 1, 2]), [C, 4, 4]

    def other_view(g, x):
        return g.node("Transpose", [g.node("Neg", [x], name="neg")], name="other_to_nhwc", perm=[0, 2, 3, 1])

    def image_mean_h(g, x, rng):  # channels-first, the mean over H instead of the channels
        h = _grn(g, x, rng, 16, (1, 16, 1, 1), (2, 3), 2)
        return g.node("Relu", [h], name="out_relu"), [16, 4, 4]

    def image_axes(g, x, rng):  # channels-first, the norm over (C, H)
        h = _grn(g, x, rng, 16, (1, 16, 1, 1), (1, 2), 1)
        return g.node("Relu", [h], name="out_relu"), [16, 4, 4]

    return {
        "axes_h_c": (lambda g, x, rng: chain(g, x, rng, axes=(1, 3)), 16, "grn/norm", "two spatial axes"),
        "keepdims0": (lambda g, x, rng: chain(g, x, rng, keepdims=0), 16, "grn/norm", "keepdims 1"),
        "mean_over_h": (lambda g, x, rng: chain(g, x, rng, mean_axis=1), 16, "grn/mean", "channel axis"),
        "eps_vector": (lambda g, x, rng: chain(g, x, rng, eps=g.const(np.full(16, 1e-6, np.float32), "eps_vec")), 16,
                       "grn/add_eps", "scalar constant"),
        "scalar_weight": (lambda g, x, rng: chain(g, x, rng, w="scalar"), 16, "grn/scale", "one value per channel"),
        "computed_bias": (lambda g, x, rng: chain(g, x, rng, b="computed"), 16, "grn/shift", "initializer"),
        "mul_x_read_twice": (lambda g, x, rng: chain(g, x, rng, extra="mul_x"), 16, "grn/mul_x", "another reader"),
        "norm_read_thrice": (lambda g, x, rng: chain(g, x, rng, extra="norm"), 16, "grn/norm", "another reader"),
        "other_residual": (lambda g, x, rng: chain(g, x, rng, residual=other_view), 16, "grn/residual", "adds back"),
        "pad_channels": (lambda g, x, rng: chain(g, x, rng, C=12), 12, "grn/norm", "multiple of 8"),
        "image_mean_over_h": (image_mean_h, 16, "grn/mean", "channel axis"),
        "image_axes_c_h": (image_axes, 16, "grn/norm", "two spatial axes"),
    }


@pytest.mark.parametrize("case", sorted(_reject_bodies()))
@pytest.mark.parametrize("precision", PRECISIONS)
def test_rejections_name_the_node(native, tmp_path, case, precision):
    body, C, node, word = _reject_bodies()[case]
    path = _graph(tmp_path, case, body, C=C)
    r = native.plan_report(path, precision)  # reports, never throws
    assert not r["supported"], case
    lines = [u for u in r["unsupported"] if u["node"] == node or (" " + node + ":") in u["error"]]
    assert lines and any(word in u["error"] for u in lines), (node, word, r["text"])
    with pytest.raises(native.NativeError):
        native.plan_summary(path, 8, precision=precision)


def test_inner_tensor_as_a_graph_output_is_rejected(native, tmp_path):
    from die_amd.models import convnextv2 as v2
    from die_amd.utils.onnx_writer import GraphBuilder

    g = GraphBuilder(name="inner_output")
    x = g.node("Relu", [g.input("x", ["N", 16, 4, 4])], name="in_relu")
    v = g.node("Transpose", [x], name="to_nhwc", perm=[0, 2, 3, 1])
    y = v2.grn_nodes(g, v, None, None, g.const(np.array(1e-6, np.float32), "eps"), "grn", "hf")
    g.output(g.node("Transpose", [y], name="to_nchw", perm=[0, 3, 1, 2]), ["N", 16, 4, 4])
    g.output("grn/div", ["N", 1, 1, 16])  # a node's output carries the node's name
    p = str(tmp_path / "inner_output.onnx")
    open(p, "wb").write(g.model_proto(opset=17, ir_version=8))
    r = native.plan_report(p, "fp32")
    assert not r["supported"]
    assert any("grn/div" in u["error"] and "graph output" in u["error"] for u in r["unsupported"]), r["text"]


def test_f_normalize_messages_are_unchanged(native, tmp_path):
    """a ReduceL2 over ONE axis of a view keeps the F.normalize lowering's report line"""
    def body(g, x, rng):
        v = g.node("Transpose", [x], name="to_nhwc", perm=[0, 2, 3, 1])
        n = g.node("ReduceL2", [v], name="row_norm", axes=[-1], keepdims=1)
        y = g.node("Div", [v, n], name="normalised")
        return g.node("Transpose", [y], name="to_nchw", perm=[0, 3, 1, 2]), [16, 4, 4]

    r = native.plan_report(_graph(tmp_path, "l2_rows", body), "fp32")
    lines = [u for u in r["unsupported"] if u["node"] == "row_norm"]
    assert lines and ("F.normalize" in lines[0]["error"] or "rank-2 rows" in lines[0]["error"]), r["text"]
