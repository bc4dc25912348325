"""GroupNorm / InstanceNorm on the planner (no GPU): InstanceNormalization, GroupNormalization in both
parameter forms and torch's Reshape -> InstanceNormalization -> Reshape [-> Mul] [-> Add] export each
lower to one groupnorm op on the NHWC image, a trailing Relu / SiLU becomes the op's act, and each form
outside that is rejected with a report line naming the node while device="auto" still serves the model.
Numerics on the device: tests/test_gpu_groupnorm.py (kernel), tests/test_gpu_groupnorm_models.py (engine)."""
import numpy as np
import pytest

NAMES = ["gn_resnet", "gn_resnet_node", "gn_decoder", "inorm_net"]
PRECISIONS = ["fp32", "bf16"]


@pytest.fixture(scope="module")
def gn_models(native, tmp_path_factory):
    from die_amd.models import groupnorm as M

    d = tmp_path_factory.mktemp("groupnorm_plan")
    out = {}
    for name in NAMES:
        blob, _ = M.BUILDERS[name](0)
        p = str(d / (name + ".onnx"))
        open(p, "wb").write(blob)
        out[name] = p
    return out


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("precision", PRECISIONS)
def test_report_is_empty(native, gn_models, name, precision):
    """Before this lowering every InstanceNormalization / GroupNormalization node was unsupported (and the
    CPU executor behind the hybrid fallback could not run them either)."""
    r = native.plan_report(gn_models[name], precision)
    assert r["supported"] and not r["unsupported"] and r["blocked"] == 0 and r["text"] == "", r["text"]
    assert all(seg["device"] == "hip" for seg in native.hybrid_partition(gn_models[name], 8, precision))


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("precision", PRECISIONS)
def test_one_op_per_normalisation(native, gn_models, name, precision):
    from die_amd.models import groupnorm as M

    s = native.plan_summary(gn_models[name], 8, precision=precision)
    ops = s["ops"]
    norms = [(o["groups"], o["channels"], o["act"]) for o in ops if o["kind"] == "groupnorm"]
    assert norms == M.EXPECTED_NORMS[name], norms
    for o in ops:
        if o["kind"] == "groupnorm":
            assert o["stored_channels"] == (o["channels"] + 7) // 8 * 8 and o["bufs"]["out2"][1] > o["bufs"]["out2"][0]
    # nothing left of the Reshapes, the Mul / Add parameters, the ReLUs or the Sigmoid / Mul of SiLU
    allowed = {"input_prep", "conv", "groupnorm", "affine", "gap", "resize", "bf16_to_f32", "to_nchw_f32"}
    assert {o["kind"] for o in ops} <= allowed, [o["kind"] for o in ops]
    for o in ops:
        assert not any(t in o["name"] for t in ("/group", "/ungroup", "/scale", "/shift", "sigmoid", "silu", "relu")), o
    # the only elementwise ops are the residual adds of gn_resnet (with the block's last ReLU)
    affine = [o["name"] for o in ops if o["kind"] == "affine"]
    assert affine == (["stage%d.add" % i for i in range(3)] if name.startswith("gn_resnet") else []), affine
    assert len(ops) == {"gn_resnet": 33, "gn_resnet_node": 33, "gn_decoder": 11, "inorm_net": 8}[name], len(ops)


def test_both_resnet_forms_plan_the_same_parameters(native, gn_models):
    """per-group parameters are expanded to per channel at plan time, and the export's Mul / Add fold into them:
    the two graphs give the same ops with the same parameter blob"""
    a = native.plan_dump(gn_models["gn_resnet"], 8, precision="fp32").splitlines()
    b = native.plan_dump(gn_models["gn_resnet_node"], 8, precision="fp32").splitlines()

    def strip(lines):  # op names differ (the chain is named after its inner node)
        return [" ".join(t for t in ln.split(" ") if not t.startswith("name=")) for ln in lines if not ln.startswith("plan")]

    assert strip(a) == strip(b)
    fnv = [next(t for t in ln[-1].split(" ") if t.startswith("params_fnv1a=")) for ln in (a, b)]
    assert fnv[0] == fnv[1], fnv


def test_decoder_output_is_the_image(native, gn_models):
    s = native.plan_summary(gn_models["gn_decoder"], 8, precision="fp32")
    assert s["output_shape"] == [1, 3, 16, 16] and s["ops"][-1]["kind"] == "to_nchw_f32"
    s = native.plan_summary(gn_models["inorm_net"], 8, precision="fp32")
    assert s["output_shape"] == [1, 8, 12, 12]
    stored = [o["stored_channels"] for o in s["ops"] if o["kind"] == "groupnorm"]
    assert stored == [16, 24, 8], stored  # the 20-channel layer is stored as 24


# ---- rejections -----------------------------------------------------------------------------------------

def _chain(g, x, G, back, inner_extra=None):
    r = g.node("Reshape", [x, g.const(np.array([0, G, -1], np.int64))], name="group")
    n = g.node("InstanceNormalization", [r, g.const(np.ones(G, np.float32)), g.const(np.zeros(G, np.float32))],
               name="inner_norm", epsilon=1e-5)
    y = g.node("Reshape", [n, g.const(np.array(back, np.int64))], name="ungroup")
    return r, n, y


def _reject_models():
    """name -> (builder(g) -> output dims, input dims, the node the report must name)"""
    def not_divisible(g, x):  # 24 channels in 16 groups: the Reshape is valid ONNX (groups straddle channels)
        _, _, y = _chain(g, x, 16, [0, 24, 2, 4])
        g.output(g.node("Relu", [y], name="relu"), ["N", 24, 2, 4])

    def inner_read_twice(g, x):
        _, n, y = _chain(g, x, 4, [0, 16, 4, 4])
        side = g.node("Reshape", [g.node("Relu", [n], name="side_relu"), g.const(np.array([0, 16, 4, 4], np.int64))], name="side")
        g.output(g.node("Add", [y, side], name="sum"), ["N", 16, 4, 4])

    def grouped_read_twice(g, x):
        r, _, y = _chain(g, x, 4, [0, 16, 4, 4])
        side = g.node("Reshape", [g.node("Neg", [r], name="neg"), g.const(np.array([0, 16, 4, 4], np.int64))], name="side")
        g.output(g.node("Add", [y, side], name="sum"), ["N", 16, 4, 4])

    def other_back_shape(g, x):
        _, _, y = _chain(g, x, 4, [0, 8, 8, 4])
        g.output(g.node("Relu", [y], name="relu"), ["N", 8, 8, 4])

    def computed_scale(g, x):
        sc = g.node("Identity", [g.const(np.full(16, 1.5, np.float32))], name="scale_of")
        y = g.node("GroupNormalization", [x, sc, g.const(np.zeros(16, np.float32))], name="gn", num_groups=4, epsilon=1e-5)
        g.output(y, ["N", 16, 4, 4])

    def nhwc_view(g, x):
        t = g.node("Transpose", [g.node("Relu", [x], name="relu")], name="to_nhwc", perm=[0, 2, 3, 1])
        y = g.node("GroupNormalization", [t, g.const(np.ones(4, np.float32)), g.const(np.zeros(4, np.float32))], name="gn_view",
                   num_groups=2, epsilon=1e-5)
        g.output(g.node("Transpose", [y], name="to_nchw", perm=[0, 3, 1, 2]), ["N", 16, 4, 4])

    def rows(g, x):
        y = g.node("InstanceNormalization", [x, g.const(np.ones(6, np.float32)), g.const(np.zeros(6, np.float32))],
                   name="rows_norm", epsilon=1e-5)
        g.output(y, ["N", 6, 16])

    return {
        "not_divisible": (not_divisible, [24, 2, 4], "group"),
        "inner_read_twice": (inner_read_twice, [16, 4, 4], "inner_norm"),
        "grouped_read_twice": (grouped_read_twice, [16, 4, 4], "group"),
        "other_back_shape": (other_back_shape, [16, 4, 4], "ungroup"),
        "computed_scale": (computed_scale, [16, 4, 4], "gn"),
        "nhwc_view": (nhwc_view, [16, 4, 4], "gn_view"),
        "rows": (rows, [6, 16], "rows_norm"),
    }


@pytest.mark.parametrize("case", sorted(_reject_models()))
def test_rejected_with_a_report_line_and_still_served(native, tmp_path, case):
    from conftest import gpu_available

    from die_amd.utils.onnx_writer import GraphBuilder

    build, dims, offender = _reject_models()[case]
    g = GraphBuilder(name="reject_" + case)
    build(g, g.input("x", ["N"] + dims))
    p = str(tmp_path / (case + ".onnx"))
    g.save(p, opset=21)
    r = native.plan_report(p, "fp32")
    assert not r["supported"], case
    named = [it for it in r["unsupported"] if it["node"] == offender or ("%s %s" % (it["op"], offender)) in it["error"] or
             (" " + offender + " ") in it["error"] or (" " + offender + ":") in it["error"]]
    assert named, (offender, r["text"])
    # ... and the model is still served: by the CPU executor without a GPU, by the hybrid partition with one
    eng = native.Engine(p, device="auto", max_batch=4)
    try:
        name = eng.refresh_info()["name"]
        assert name != "hip" and (gpu_available() or name == "cpu"), name
        x = np.random.default_rng(4).standard_normal([3] + dims).astype(np.float32)
        got = eng.run(x.reshape(3, -1))
        ref = native.cpu_run(p, x).reshape(3, -1)
        # the bar of the HIP engine in fp32 against the CPU executor (tests/test_gpu_fuzz.py); exact on the CPU
        err = float(np.linalg.norm(got - ref) / np.linalg.norm(ref))
        assert err <= 2e-4, (case, err)
    finally:
        eng.close()
