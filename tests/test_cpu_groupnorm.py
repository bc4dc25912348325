"""CPU executor (the oracle of the GPU tests) on InstanceNormalization / GroupNormalization: one-node and
chain graphs against torch's group_norm / instance_norm in float64 (rel-L2 < 1e-6, the bar of the other
fp32 CPU-op tests), gn_resnet against gn_resnet_node, and every model of models/groupnorm.py against its
torch forward at the 1e-5 bar of tests/test_op_coverage.py.  No GPU."""
import numpy as np
import pytest

NAMES = ["gn_resnet", "gn_resnet_node", "gn_decoder", "inorm_net"]


def _rel(got, ref):
    return float(np.linalg.norm(got.astype(np.float64) - ref) / max(np.linalg.norm(ref), 1e-30))


def _run(native, tmp_path, g, x, opset=17):
    p = str(tmp_path / (g.name + ".onnx"))
    g.save(p, opset=opset)
    return native.cpu_run(p, x)


def _data(shape, C, n, seed):
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal(shape) * 1.5 + 0.7).astype(np.float32)
    return x, rng.uniform(0.5, 1.5, n).astype(np.float32), rng.normal(0, 0.3, n).astype(np.float32)


@pytest.mark.parametrize("shape", [(3, 6, 5, 7), (2, 20, 1, 1), (2, 4, 9)])
def test_instance_norm_node(native, tmp_path, shape):
    """rank 4, a 1x1 map (variance 0: the output is the bias) and rank 3"""
    import torch

    from die_amd.utils.onnx_writer import GraphBuilder

    C = shape[1]
    x, w, b = _data(shape, C, C, 3)
    g = GraphBuilder(name="inorm_r%d_%d" % (len(shape), shape[-1]))
    xi = g.input("x", ["N"] + list(shape[1:]))
    y = g.node("InstanceNormalization", [xi, g.const(w), g.const(b)], name="inorm", epsilon=1e-3)
    g.output(y, ["N"] + list(shape[1:]))
    got = _run(native, tmp_path, g, x)
    xt, wt, bt = (torch.from_numpy(a).double() for a in (x, w, b))
    if shape[2:] == (1, 1):  # torch's instance_norm refuses a single spatial element; a group per channel is the same
        ref = torch.nn.functional.group_norm(xt, C, wt, bt, eps=1e-3).numpy()
    else:
        ref = torch.nn.functional.instance_norm(xt, weight=wt, bias=bt, eps=1e-3).numpy()
    assert got.shape == shape and _rel(got, ref) < 1e-6, _rel(got, ref)
    if shape[2:] == (1, 1):
        np.testing.assert_allclose(got, np.broadcast_to(b.reshape(1, C, 1, 1), shape), atol=1e-6)


@pytest.mark.parametrize("form", ["per_group", "per_channel", "groups_equal_channels"])
def test_group_norm_node(native, tmp_path, form):
    """opset 18 (scale / bias [G]) and opset 21 ([C]), told apart by the length; G = C means the same in both"""
    import torch

    from die_amd.utils.onnx_writer import GraphBuilder

    C, G = (12, 12) if form == "groups_equal_channels" else (12, 4)
    shape = (3, C, 5, 3)
    x, w, b = _data(shape, C, G if form == "per_group" else C, 5)
    g = GraphBuilder(name="gn_" + form)
    xi = g.input("x", ["N"] + list(shape[1:]))
    y = g.node("GroupNormalization", [xi, g.const(w), g.const(b)], name="gn", epsilon=1e-5, num_groups=G)
    g.output(y, ["N"] + list(shape[1:]))
    got = _run(native, tmp_path, g, x, opset=18 if form == "per_group" else 21)
    wc, bc = (np.repeat(w, C // G), np.repeat(b, C // G)) if form == "per_group" else (w, b)
    ref = torch.nn.functional.group_norm(torch.from_numpy(x).double(), G, torch.from_numpy(wc).double(),
                                         torch.from_numpy(bc).double(), 1e-5).numpy()
    assert got.shape == shape and _rel(got, ref) < 1e-6, _rel(got, ref)


def test_group_norm_large_mean(native, tmp_path):
    """mean 100, unit variance: fp64 accumulation of the centred squares, not E[x^2] - mean^2"""
    import torch

    from die_amd.utils.onnx_writer import GraphBuilder

    shape = (2, 8, 16, 16)
    x = (100 + np.random.default_rng(9).standard_normal(shape)).astype(np.float32)
    g = GraphBuilder(name="gn_large_mean")
    xi = g.input("x", ["N", 8, 16, 16])
    y = g.node("GroupNormalization", [xi, g.const(np.ones(8, np.float32)), g.const(np.zeros(8, np.float32))], name="gn",
               epsilon=1e-5, num_groups=2)
    g.output(y, ["N", 8, 16, 16])
    got = _run(native, tmp_path, g, x, opset=21)
    ref = torch.nn.functional.group_norm(torch.from_numpy(x).double(), 2, eps=1e-5).numpy()
    assert _rel(got, ref) < 1e-6, _rel(got, ref)


def test_torch_export_chain(native, tmp_path):
    """Reshape [0, G, -1] -> InstanceNormalization (general per-group scale / bias) -> Reshape back -> Mul -> Add"""
    import torch

    from die_amd.utils.onnx_writer import GraphBuilder

    C, G, H, W = 20, 4, 3, 5
    x, w, b = _data((3, C, H, W), C, C, 11)
    rng = np.random.default_rng(12)
    s, t = rng.uniform(0.5, 1.5, G).astype(np.float32), rng.normal(0, 0.3, G).astype(np.float32)
    g = GraphBuilder(name="gn_chain")
    xi = g.input("x", ["N", C, H, W])
    r = g.node("Reshape", [xi, g.const(np.array([0, G, -1], np.int64))], name="group")
    n = g.node("InstanceNormalization", [r, g.const(s), g.const(t)], name="inorm", epsilon=1e-5)
    y = g.node("Reshape", [n, g.node("Shape", [xi], name="shape_of")], name="ungroup")
    y = g.node("Add", [g.node("Mul", [y, g.const(w.reshape(C, 1, 1))], name="scale"), g.const(b.reshape(C, 1, 1))], name="shift")
    g.output(y, ["N", C, H, W])
    got = _run(native, tmp_path, g, x)
    gamma = np.repeat(s, C // G).astype(np.float64) * w
    beta = np.repeat(t, C // G).astype(np.float64) * w + b
    ref = torch.nn.functional.group_norm(torch.from_numpy(x).double(), G, torch.from_numpy(gamma), torch.from_numpy(beta),
                                         1e-5).numpy()
    assert _rel(got, ref) < 1e-6, _rel(got, ref)


@pytest.fixture(scope="module")
def gn_models(native, tmp_path_factory):
    from die_amd.models import groupnorm as M

    d = tmp_path_factory.mktemp("groupnorm_cpu")
    out = {}
    for name in NAMES:
        blob, w = M.BUILDERS[name](0)
        p = str(d / (name + ".onnx"))
        open(p, "wb").write(blob)
        out[name] = (p, w)
    return out


def test_resnet_forms_agree(native, gn_models):
    """the export chain and the GroupNormalization nodes (per group / per channel) are the same function"""
    from die_amd.models import groupnorm as M

    x = M.synthetic_input("gn_resnet", 3)
    a = native.cpu_run(gn_models["gn_resnet"][0], x)
    b = native.cpu_run(gn_models["gn_resnet_node"][0], x)
    assert a.shape == (3, 10) and _rel(a, b.astype(np.float64)) < 1e-6, _rel(a, b.astype(np.float64))
    assert (a.argmax(1) == b.argmax(1)).all()


@pytest.mark.parametrize("name", NAMES)
def test_models_match_torch(native, gn_models, name):
    import torch

    from die_amd.models import groupnorm as M

    path, w = gn_models[name]
    x = M.synthetic_input(name, 3)
    got = native.cpu_run(path, x)
    with torch.no_grad():
        ref = M.torch_forward(name, w, x).numpy()
    assert got.shape == ref.shape, (got.shape, ref.shape)
    err = _rel(got, ref.astype(np.float64))
    assert err < 1e-5, (name, err)
