"""CPU executor (the oracle of the GPU tests) on the grouped-query attention models `gqa_enc`,
`mqa_causal` and `gqa_hd128`: HF's repeat_kv runs as Unsqueeze -> Expand -> Reshape on a rank-5
activation.  Against an independent numpy float64 forward written here from the generators' weights
(K / V heads indexed h // G, nothing repeated), and against the `expand_kv` multi-head twins, at the
bar of tests/test_cpu_rope_rmsnorm.py.  No GPU."""
import math

import numpy as np
import pytest

NAMES = ["gqa_enc", "mqa_causal", "gqa_hd128"]


@pytest.fixture(scope="module")
def gqa_models(native, tmp_path_factory):
    from die_amd.models import generic as G

    d = tmp_path_factory.mktemp("gqa_cpu")
    out = {}
    for name in NAMES:
        for twin in (False, True):
            blob, weights = G.BUILDERS[name](0, expand_kv=twin)
            p = str(d / (name + ("_mha" if twin else "") + ".onnx"))
            open(p, "wb").write(blob)
            out[name, twin] = (p, {k: np.asarray(v, np.float64) for k, v in weights.items()
                                   if np.asarray(v).dtype == np.float32})
    return out


@pytest.fixture(scope="module")
def cpu_outputs(native, gqa_models):
    """One CPU-executor run per model and twin, shared by the tests."""
    from die_amd.models import generic as G

    out = {}
    for name in NAMES:
        x = G.synthetic_input(name, 5)
        out[name] = (x, native.cpu_run(gqa_models[name, False][0], x), native.cpu_run(gqa_models[name, True][0], x))
    return out


def _rope(x, cos, sin):
    h2 = x.shape[-1] // 2
    return x * cos + np.concatenate([-x[..., h2:], x[..., :h2]], axis=-1) * sin


def _softmax(s):
    e = np.exp(s - s.max(-1, keepdims=True))
    return e / e.sum(-1, keepdims=True)


def _heads(x, H):
    N, S, D = x.shape
    return x.reshape(N, S, H, D // H).transpose(0, 2, 1, 3)


def _ln(x, w, b, eps=1e-5):
    mu = x.mean(-1, keepdims=True)
    var = ((x - mu) ** 2).mean(-1, keepdims=True)
    return (x - mu) / np.sqrt(var + eps) * w + b


_erf = np.vectorize(math.erf)


def _gqa_attention(q, k, v, G, term):
    """q [N, H, S, hd], k / v [N, Hkv, S, hd]: head h attends to K / V head h // G; term: added to the scores."""
    N, H, S, hd = q.shape
    ctx = np.empty((N, S, H, hd))
    for h in range(H):
        sc = q[:, h] @ k[:, h // G].transpose(0, 2, 1) / math.sqrt(hd)
        ctx[:, :, h] = _softmax(sc + term) @ v[:, h // G]
    return ctx.reshape(N, S, H * hd)


def _ref(name, w, x):
    from die_amd.models import generic as G_

    s = G_.SPECS[name]
    S, D, H, Hkv, body = s["seq"], s["dim"], s["heads"], s["kv_heads"], s["body"]
    hd, G = D // H, H // Hkv
    bias = body != "llama"
    lin = lambda a, n: a @ w[n + ".weight"] + (w[n + ".bias"] if bias else 0.0)
    if body != "gpt":
        cos, sin = w["rope.cos"].reshape(S, hd), w["rope.sin"].reshape(S, hd)
    if body == "llama":
        eps = float(np.float32(s["eps"]))
        norm = lambda a, n: a / np.sqrt((a ** 2).mean(-1, keepdims=True) + eps) * w[n + ".weight"]
        vis = (x > 0).astype(np.float64)
        h = w["embed_tokens.weight"][x.astype(np.int64)]
        term = ((1.0 - vis) * -10000.0)[:, None, :]
    else:
        norm = lambda a, n: _ln(a, w[n + ".weight"], w[n + ".bias"])
        h = x.astype(np.float64).reshape(-1, S, D)
        # the export's Where(tril, scores, -1e4) REPLACES the masked scores; exp(-1e4 - max) is 0 in float32 and float64 alike
        term = np.where(np.tril(np.ones((S, S), bool)), 0.0, -np.inf)[None] if body == "gpt" else 0.0

    def attention(a, p):
        q, k, v = _heads(lin(a, p + "q_proj"), H), _heads(lin(a, p + "k_proj"), Hkv), _heads(lin(a, p + "v_proj"), Hkv)
        assert k.shape[1] == Hkv and k.shape[-1] == hd
        if body != "gpt":
            q, k = _rope(q, cos, sin), _rope(k, cos, sin)
        return lin(_gqa_attention(q, k, v, G, term), p + "o_proj")

    def ffn(a, p):
        if body == "llama":
            g = a @ w[p + "gate_proj.weight"]
            return (g / (1.0 + np.exp(-g)) * (a @ w[p + "up_proj.weight"])) @ w[p + "down_proj.weight"]
        m = lin(a, p + "intermediate")
        return lin(m * 0.5 * (1.0 + _erf(m / math.sqrt(2.0))), p + "output")

    for i in range(s["layers"]):
        p = "layer%d." % i
        if body == "rope_bert":
            h = norm(attention(h, p) + h, p + "ln1")
            h = norm(ffn(h, p) + h, p + "ln2")
        else:
            h = h + attention(norm(h, p + "norm1"), p)
            h = h + ffn(norm(h, p + "norm2"), p)
    if body != "rope_bert":
        h = norm(h, "norm_f")
    if body == "llama":
        mean = (h * vis[:, :, None]).sum(1) / np.maximum(vis.sum(1, keepdims=True), 1e-9)
        return mean / np.linalg.norm(mean, axis=1, keepdims=True)
    return h.mean(1) @ w["classifier.weight"].T + w["classifier.bias"]


@pytest.mark.parametrize("name", NAMES)
def test_cpu_executor_matches_the_float64_forward(gqa_models, cpu_outputs, name):
    """2e-6 absolute on outputs of order 1 (unit-length embeddings; the classifiers' logits are scaled by
    their largest magnitude): the bar of tests/test_cpu_rope_rmsnorm.py."""
    x, got, _ = cpu_outputs[name]
    ref = _ref(name, gqa_models[name, False][1], x)
    assert got.shape == ref.shape and np.isfinite(got).all()
    scale = max(1.0, float(np.abs(ref).max()))
    err = float(np.abs(got - ref).max())
    print(name, "max abs err %.3g (scale %.3g)" % (err, scale))
    assert err <= 2e-6 * scale, (err, scale)
    if name == "gqa_enc":
        np.testing.assert_allclose(np.linalg.norm(got.astype(np.float64), axis=1), 1.0, atol=1e-6)


@pytest.mark.parametrize("name", NAMES)
def test_cpu_executor_matches_the_expand_kv_twin(cpu_outputs, name):
    """The twin repeats the K / V projection columns instead of the heads: the same function."""
    _, got, twin = cpu_outputs[name]
    assert got.shape == twin.shape
    scale = max(1.0, float(np.abs(twin).max()))
    err = float(np.abs(got - twin).max())
    print(name, "max abs err vs twin %.3g (scale %.3g)" % (err, scale))
    assert err <= 2e-6 * scale, (err, scale)


def test_the_group_index_matters(gqa_models, cpu_outputs):
    """The float64 forward with every head reading K / V head 0 is a different function: the checks
    above are not blind to which stored head a query head reads."""
    from die_amd.models import generic as G_

    name = "gqa_hd128"
    x, got, _ = cpu_outputs[name]
    w = dict(gqa_models[name, False][1])
    s = G_.SPECS[name]
    hd = s["dim"] // s["heads"]
    for i in range(s["layers"]):  # head 1's columns := head 0's
        for n in ("k_proj", "v_proj"):
            for sfx in (".weight", ".bias"):
                a = w["layer%d.%s%s" % (i, n, sfx)].copy()
                a[..., hd:2 * hd] = a[..., :hd]
                w["layer%d.%s%s" % (i, n, sfx)] = a
    ref = _ref(name, w, x)
    assert float(np.abs(got - ref).max()) > 1e-3
