"""CPU executor (the oracle of the GPU tests) on the rotary / RMSNorm models: `rope_bert`,
`rope_bert_nshd`, `llama_enc` and `llama_enc_rmsnode` against an independent numpy float64 forward
written here from the generators' weights, and the single nodes RMSNormalization /
SimplifiedLayerNormalization alone.  No GPU."""
import math

import numpy as np
import pytest

NAMES = ["rope_bert", "rope_bert_nshd", "llama_enc", "llama_enc_rmsnode"]


@pytest.fixture(scope="module")
def rope_models(native, tmp_path_factory):
    from die_amd.models import generic as G

    d = tmp_path_factory.mktemp("rope_cpu")
    out = {}
    for name in NAMES:
        blob, weights = G.BUILDERS[name](0)
        p = str(d / (name + ".onnx"))
        open(p, "wb").write(blob)
        out[name] = (p, {k: np.asarray(v, np.float64) for k, v in weights.items() if np.asarray(v).dtype == np.float32})
    return out


# ---- the float64 forward ------------------------------------------------------------------------------

def _tables(S, hd, theta):
    """cos / sin [S, hd] in float64, re-derived (not read from the model): angle = s * theta^(-2i/hd)."""
    inv = theta ** (-2.0 * np.arange(hd // 2) / hd)
    ang = np.arange(S)[:, None] * inv[None, :]
    return np.cos(np.concatenate([ang, ang], 1)), np.sin(np.concatenate([ang, ang], 1))


def _rope(x, cos, sin):
    """x [N, H, S, hd]: pairs (j, j + hd/2) rotated by the angle of position s."""
    h2 = x.shape[-1] // 2
    rot = np.concatenate([-x[..., h2:], x[..., :h2]], axis=-1)
    return x * cos + rot * sin


def _softmax(s):
    e = np.exp(s - s.max(-1, keepdims=True))
    return e / e.sum(-1, keepdims=True)


def _heads(x, H):
    N, S, D = x.shape
    return x.reshape(N, S, H, D // H).transpose(0, 2, 1, 3)


def _merge(x):
    N, H, S, hd = x.shape
    return x.transpose(0, 2, 1, 3).reshape(N, S, H * hd)


def _ln(x, w, b, eps=1e-5):
    mu = x.mean(-1, keepdims=True)
    var = ((x - mu) ** 2).mean(-1, keepdims=True)
    return (x - mu) / np.sqrt(var + eps) * w + b


def _erf(x):
    return np.vectorize(math.erf)(x)


def _rope_bert_ref(name, w, x, rotate=True):
    from die_amd.models import generic as G

    s = G.SPECS[name]
    S, D, H = s["seq"], s["dim"], s["heads"]
    hd = D // H
    # the stored tables are the float32 roundings of these; the model computes with the stored ones
    cos, sin = w["rope.cos"].reshape(S, hd), w["rope.sin"].reshape(S, hd)
    c64, s64 = _tables(S, hd, s["theta"])
    assert np.abs(cos - c64).max() < 1e-7 and np.abs(sin - s64).max() < 1e-7
    if not rotate:
        cos, sin = np.ones_like(cos), np.zeros_like(sin)
    h = x.astype(np.float64).reshape(-1, S, D)
    for i in range(s["layers"]):
        p = "layer%d." % i
        lin = lambda a, n: a @ w[p + n + ".weight"] + w[p + n + ".bias"]
        q = _rope(_heads(lin(h, "query"), H), cos, sin)
        k = _rope(_heads(lin(h, "key"), H), cos, sin)
        v = _heads(lin(h, "value"), H)
        ctx = _merge(_softmax(q @ k.transpose(0, 1, 3, 2) / math.sqrt(hd)) @ v)
        h = _ln(lin(ctx, "attn_out") + h, w[p + "ln1.weight"], w[p + "ln1.bias"])
        m = lin(h, "intermediate")
        m = m * 0.5 * (1.0 + _erf(m / math.sqrt(2.0)))
        h = _ln(lin(m, "output") + h, w[p + "ln2.weight"], w[p + "ln2.bias"])
    return h.mean(1) @ w["classifier.weight"].T + w["classifier.bias"]


def _llama_ref(name, w, ids):
    from die_amd.models import generic as G

    s = G.SPECS[name]
    S, D, H, eps = s["seq"], s["dim"], s["heads"], float(np.float32(s["eps"]))
    hd = D // H
    cos, sin = w["rope.cos"].reshape(S, hd), w["rope.sin"].reshape(S, hd)
    rms = lambda a, n: a / np.sqrt((a ** 2).mean(-1, keepdims=True) + eps) * w[n + ".weight"]
    vis = (ids > 0).astype(np.float64)
    h = w["embed_tokens.weight"][ids.astype(np.int64)]
    key_term = (1.0 - vis)[:, None, None, :] * -10000.0
    for i in range(s["layers"]):
        p = "layer%d." % i
        a = rms(h, p + "input_norm")
        q = _rope(_heads(a @ w[p + "q_proj.weight"], H), cos, sin)
        k = _rope(_heads(a @ w[p + "k_proj.weight"], H), cos, sin)
        v = _heads(a @ w[p + "v_proj.weight"], H)
        ctx = _merge(_softmax(q @ k.transpose(0, 1, 3, 2) / math.sqrt(hd) + key_term) @ v)
        h = h + ctx @ w[p + "o_proj.weight"]
        a = rms(h, p + "post_attention_norm")
        g = a @ w[p + "gate_proj.weight"]
        h = h + (g / (1.0 + np.exp(-g)) * (a @ w[p + "up_proj.weight"])) @ w[p + "down_proj.weight"]
    h = rms(h, "norm")
    mean = (h * vis[:, :, None]).sum(1) / np.maximum(vis.sum(1, keepdims=True), 1e-9)
    return mean / np.linalg.norm(mean, axis=1, keepdims=True)


def _ref(name, w, x):
    return _rope_bert_ref(name, w, x) if name.startswith("rope_bert") else _llama_ref(name, w, x)


# ---- the models ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", NAMES)
def test_cpu_executor_matches_the_float64_forward(native, rope_models, name):
    """The bar of tests/test_cpu_ops_pooling.py for a whole tail: 2e-6 absolute on outputs of order 1
    (unit-length embeddings; the classifiers' logits are scaled by their largest magnitude)."""
    from die_amd.models import generic as G

    path, w = rope_models[name]
    x = G.synthetic_input(name, 5)
    got = native.cpu_run(path, x)
    ref = _ref(name, w, x)
    assert got.shape == ref.shape and np.isfinite(got).all()
    scale = max(1.0, float(np.abs(ref).max()))
    err = float(np.abs(got - ref).max())
    print(name, "max abs err %.3g (scale %.3g)" % (err, scale))
    assert err <= 2e-6 * scale, (err, scale)
    if name.startswith("llama"):
        np.testing.assert_allclose(np.linalg.norm(got.astype(np.float64), axis=1), 1.0, atol=1e-6)


def test_rotation_depends_on_the_position(native, rope_models):
    """The float64 forward without the rotation is a different function: the check above is not blind to RoPE."""
    from die_amd.models import generic as G

    path, w = rope_models["rope_bert"]
    x = G.synthetic_input("rope_bert", 2)
    got = native.cpu_run(path, x)
    assert np.abs(got - _rope_bert_ref("rope_bert", w, x, rotate=False)).max() > 1e-3


def test_decomposed_and_node_rmsnorm_agree(native, rope_models):
    """The same weights: the two spellings differ by fp32 rounding of the normalisation only."""
    from die_amd.models import generic as G

    x = G.synthetic_input("llama_enc", 5)
    a = native.cpu_run(rope_models["llama_enc"][0], x)
    b = native.cpu_run(rope_models["llama_enc_rmsnode"][0], x)
    assert sorted(rope_models["llama_enc"][1]) == sorted(rope_models["llama_enc_rmsnode"][1])
    np.testing.assert_allclose(a, b, rtol=0, atol=2e-6)


# ---- the single nodes ----------------------------------------------------------------------------------

def _rms_ref(x, w, eps, axis):
    x64 = x.astype(np.float64)
    axes = tuple(range(axis % x.ndim, x.ndim))
    inv = 1.0 / np.sqrt((x64 ** 2).mean(axis=axes, keepdims=True) + float(np.float32(eps)))
    return x64 * inv * w.astype(np.float64), inv


@pytest.mark.parametrize("op", ["RMSNormalization", "SimplifiedLayerNormalization"])
@pytest.mark.parametrize("shape,axis", [((5, 12), -1), ((5, 12), 1), ((3, 7, 10), -1), ((3, 7, 10), 2), ((3, 7, 10), 1)])
def test_rmsnorm_nodes(native, tmp_path, op, shape, axis):
    from die_amd.utils.onnx_writer import GraphBuilder

    rng = np.random.default_rng(len(shape) + 7)
    x = (3.0 + rng.standard_normal(shape)).astype(np.float32)  # a mean the op must not subtract
    a = axis % len(shape)
    w = (1.0 + 0.1 * rng.standard_normal(shape[a:])).astype(np.float32)
    g = GraphBuilder(name="rms")
    y = g.node(op, [g.input("x", ["N"] + list(shape[1:])), g.init("w", w)], name="norm", axis=axis, epsilon=1e-6)
    g.output(y, ["N"] + list(shape[1:]))
    p = str(tmp_path / "rms.onnx")
    open(p, "wb").write(g.model_proto(opset=23))
    got = native.cpu_run(p, x)
    ref, _ = _rms_ref(x, w, 1e-6, axis)
    assert got.shape == x.shape
    np.testing.assert_allclose(got, ref, rtol=3e-6, atol=0)


def test_simplified_layernorm_second_output_is_inv_std(native, tmp_path):
    """The optional second output, consumed: y2 = x * inv_std (the unscaled normalisation)."""
    from die_amd.utils.onnx_writer import GraphBuilder

    rng = np.random.default_rng(11)
    x = (3.0 + rng.standard_normal((4, 6, 16))).astype(np.float32)
    w = (1.0 + 0.1 * rng.standard_normal(16)).astype(np.float32)
    g = GraphBuilder(name="sln2")
    xin = g.input("x", ["N", 6, 16])
    outs = g.node("SimplifiedLayerNormalization", [xin, g.init("w", w)], outputs=["y", "inv_std"], name="norm", axis=-1,
                  epsilon=1e-6)
    inv = outs[1] if isinstance(outs, (list, tuple)) else "inv_std"
    g.output(g.node("Mul", [xin, inv], name="renorm"), ["N", 6, 16])
    p = str(tmp_path / "sln2.onnx")
    open(p, "wb").write(g.model_proto(opset=17))
    got = native.cpu_run(p, x)
    _, inv_ref = _rms_ref(x, w, 1e-6, -1)
    np.testing.assert_allclose(got, x.astype(np.float64) * inv_ref, rtol=3e-6, atol=0)
