"""Token-id models on the planner (no GPU): the graph input [N, S] holds token ids, a Gather embeds
them and the attention mask is the request's own padding, computed from the ids.  The planner lowers
the lookup (+ positions + token type) to one embed_tokens op reading the fp32 input in place, and the
mask to the attention op's key_mask flag.  Also here: the id -> table row rule on the host, and the
CPU executor (the oracle of the GPU tests) against a float64 torch forward on padded rows.
Numerics on the device: tests/test_gpu_embed_tokens.py, tests/test_gpu_attention_keymask.py (kernels)
and tests/test_gpu_token_models.py (engine)."""
import math

import numpy as np
import pytest

NAMES = ["bert_ids", "bert_ids_hf"]


@pytest.fixture(scope="module")
def token_models(native, tmp_path_factory):
    from die_amd.models import generic as G

    d = tmp_path_factory.mktemp("token_ids")
    out = {}
    for name in NAMES:
        for int_input in (False, True):
            blob, weights = G.build_token_encoder(0, spec=name, int_input=int_input)
            p = str(d / ("%s_%d.onnx" % (name, int_input)))
            open(p, "wb").write(blob)
            out[name, int_input] = (p, weights)
    return out


def _plan(native, path, precision):
    r = native.plan_report(path, precision)
    assert r["supported"] and not r["unsupported"], r["text"]
    return native.plan_summary(path, 8, precision=precision)


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_token_models_plan_with_one_embed_op_and_key_masked_attention(native, token_models, name, precision):
    from die_amd.models import generic as G

    spec = G.SPECS[name]
    s = _plan(native, token_models[name, False][0], precision)
    kinds = [o["kind"] for o in s["ops"]]
    assert kinds.count("embed_tokens") == 1 and "rows_prep" not in kinds, kinds
    # the mask is part of the attention op: nothing stands in for the compare / where / add nodes
    assert not {"where", "binary", "unary", "softmax"} & set(kinds), kinds
    assert s["input_shape"] == [1, spec["seq"]]
    emb = next(o for o in s["ops"] if o["kind"] == "embed_tokens")
    assert (emb["vocab"], emb["seq"], emb["dim"]) == (spec["vocab"], spec["seq"], spec["dim"])
    assert emb["positions"] and emb["token_type"] == (name == "bert_ids_hf") and emb["key_data"]
    # visible = not (trunc(id) == 0) for bert_ids, id > 0 for bert_ids_hf
    if name == "bert_ids":
        assert (emb["pad_op"], emb["pad_value"], emb["pad_negated"], emb["pad_truncated"]) == ("equal", 0.0, True, True)
    else:
        assert (emb["pad_op"], emb["pad_value"], emb["pad_negated"], emb["pad_truncated"]) == ("greater", 0.0, False, False)
    att = [o for o in s["ops"] if o["kind"] == "attention"]
    assert len(att) == spec["layers"]
    for o in att:
        assert o["key_mask"] is True and o["causal"] is False, o
        assert o["bias_heads"] == (spec["heads"] if name == "bert_ids_hf" else 0), o
        # the key data buffers stay live from the embed op to the last attention
        assert o["bufs"]["in4"] == emb["bufs"]["out2"] and o["bufs"]["in5"] == emb["bufs"]["out3"]


@pytest.mark.parametrize("name", NAMES)
def test_declared_int64_input_plans_the_same(native, token_models, name):
    a = _plan(native, token_models[name, False][0], "fp32")
    b = _plan(native, token_models[name, True][0], "fp32")
    assert [(o["kind"], o["name"]) for o in a["ops"]] == [(o["kind"], o["name"]) for o in b["ops"]]
    assert a["input_shape"] == b["input_shape"]
    ea, eb = (next(o for o in s["ops"] if o["kind"] == "embed_tokens") for s in (a, b))
    for key in ("vocab", "seq", "dim", "positions", "token_type", "key_data", "pad_op", "pad_value", "pad_negated"):
        assert ea[key] == eb[key], key
    assert eb["pad_truncated"] is True  # a declared integer input: both engines truncate the fed floats
    for oa, ob in zip(a["ops"], b["ops"]):
        if oa["kind"] == "attention":
            assert (oa["key_mask"], oa["bias_heads"], oa["causal"]) == (ob["key_mask"], ob["bias_heads"], ob["causal"])


# ---- rejections: one minimal graph each ---------------------------------------------------------------

def _tiny(tmp_path, name, gather_axis=0, table_is_init=True, mask_axes=(1, 2), causal=False, pooled_mask=False,
          fill=-np.inf):
    """ids [N, 8] -> Gather -> one single-head attention with Where(Unsqueeze(ids == 0), -inf, scores)
    -> mean over tokens -> Gemm, with one thing wrong per caller."""
    from die_amd.utils.onnx_writer import INT64, GraphBuilder

    rng = np.random.default_rng(0)
    S, D, V = 8, 32, 16
    g = GraphBuilder(name=name)
    x = g.input("input_ids", ["N", S])
    ids = g.node("Cast", [x], name="ids_int", to=INT64)
    table = g.init("table", rng.standard_normal((V, D)).astype(np.float32))
    if not table_is_init:
        table = g.node("Identity", [table], name="table_copy")
    h = g.node("Gather", [table, ids], name="lookup", axis=gather_axis)
    hidden = g.node("Equal", [ids, g.const(np.array(0, np.int64), "pad")], name="is_pad")
    mask = g.node("Unsqueeze", [hidden, g.const(np.array(mask_axes, np.int64), "axes")], name="pad_mask")
    heads = g.const(np.array([0, 0, 1, D], np.int64), "heads_shape")

    def proj(nm, perm):
        w = g.init(nm + ".weight", (rng.standard_normal((D, D)) / math.sqrt(D)).astype(np.float32))
        t = g.node("Reshape", [g.node("MatMul", [h, w], name=nm), heads], name=nm + "_heads")
        return g.node("Transpose", [t], name=nm + "_perm", perm=perm)

    q, k, v = proj("q", [0, 2, 1, 3]), proj("k", [0, 2, 3, 1]), proj("v", [0, 2, 1, 3])
    sc = g.node("Div", [g.node("MatMul", [q, k], name="scores"), g.const(np.array(math.sqrt(D), np.float32), "sqrt_d")],
                name="scale")
    fill = g.const(np.array(fill, np.float32), "fill")
    if causal:
        sc = g.node("Where", [g.init("tril", np.tril(np.ones((1, 1, S, S), np.bool_))), sc, fill], name="causal")
    sc = g.node("Softmax", [g.node("Where", [mask, fill, sc], name="key_mask")], name="softmax", axis=-1)
    c = g.node("Transpose", [g.node("MatMul", [sc, v], name="context")], name="ctx_perm", perm=[0, 2, 1, 3])
    c = g.node("Reshape", [c, g.const(np.array([0, 0, D], np.int64), "merge_shape")], name="ctx_merge")
    pooled = g.node("ReduceMean", [c], name="mean_pool", axes=[1], keepdims=0)
    if pooled_mask:  # masked mean pooling: the visibility value leaves the attention pattern
        cnt = g.node("ReduceSum", [g.node("Cast", [g.node("Not", [hidden], name="visible")], name="visible_f", to=1),
                                   g.const(np.array([1], np.int64), "count_axes")], name="visible_count", keepdims=1)
        pooled = g.node("Div", [pooled, cnt], name="masked_mean")
    w = g.init("fc.weight", rng.standard_normal((3, D)).astype(np.float32))
    y = g.node("Gemm", [pooled, w, g.init("fc.bias", np.zeros(3, np.float32))], name="fc", transB=1)
    g.output(y, ["N", 3])
    p = str(tmp_path / (name + ".onnx"))
    open(p, "wb").write(g.model_proto(opset=17))
    return p


def test_tiny_token_graph_plans(native, tmp_path):
    """The base of the rejection graphs is itself supported (each rejection below changes one thing)."""
    s = _plan(native, _tiny(tmp_path, "ok"), "fp32")
    assert [o["kind"] for o in s["ops"]].count("embed_tokens") == 1
    assert all(o["key_mask"] for o in s["ops"] if o["kind"] == "attention")


@pytest.mark.parametrize("case,kwargs,node,words", [
    ("causal", dict(causal=True), "ctx_merge", "causal"),
    ("pooling", dict(pooled_mask=True), "visible_count", "key mask"),
    ("axis", dict(gather_axis=1), "lookup", "axis 0"),
    ("table", dict(table_is_init=False), "lookup", "initializer"),
    ("shape", dict(mask_axes=(1,)), "key_mask", "[N, 1, 1, S]"),
])
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_rejections_name_the_node(native, tmp_path, case, kwargs, node, words, precision):
    path = _tiny(tmp_path, case, **kwargs)
    r = native.plan_report(path, precision)  # reports, never throws
    assert not r["supported"]
    lines = [u for u in r["unsupported"] if u["node"] == node]
    assert lines and words in lines[0]["error"], r["text"]
    with pytest.raises(native.NativeError):
        native.plan_summary(path, 8, precision=precision)


def test_finite_fill_above_the_bar_is_rejected(native, tmp_path):
    """The fill rule is the constant masks' one: <= -1e4 is taken as -inf, a finite fill above it is a
    value and is rejected."""
    r = native.plan_report(_tiny(tmp_path, "fill", fill=-100.0), "fp32")
    assert not r["supported"]
    assert any(u["node"] == "key_mask" and "fill" in u["error"] for u in r["unsupported"]), r["text"]
    assert native.plan_report(_tiny(tmp_path, "fill_ok", fill=-1e4), "fp32")["supported"]


# ---- the id -> table row rule -------------------------------------------------------------------------

def test_host_index_function(native):
    idx = native.kernels().die_token_index
    V = 1000
    inf = float("inf")
    want = {-1.0: 0, -0.0: 0, 0.0: 0, 0.9: 0, 1.0: 1, 1.9: 1, -0.9: 0, float(V - 1): V - 1, float(V): V - 1,
            V - 0.5: V - 1, V - 1.5: V - 2, 1e9: V - 1, inf: V - 1, -inf: 0, float("nan"): 0, 3e38: V - 1, -3e38: 0}
    for x, w in want.items():
        assert idx(x, V) == w, (x, idx(x, V), w)
    assert idx(5.0, 1) == 0 and idx(0.0, 1) == 0  # a one-row table
    # every bit pattern class: denormals, the largest finite values, NaN payloads
    for bits in (0x00000001, 0x80000001, 0x7F7FFFFF, 0xFF7FFFFF, 0x7FC00001, 0xFFC00000, 0x7F800001):
        x = float(np.array([bits], np.uint32).view(np.float32)[0])
        assert 0 <= idx(x, V) <= V - 1


# ---- the oracle itself on padded rows -------------------------------------------------------------------

def _torch_forward(name, w, ids):
    """float64 forward of models/generic.py build_token_encoder from its weight dict, with an explicit
    masked_fill of the padded keys."""
    import torch

    from die_amd.models import generic as G

    s = G.SPECS[name]
    S, D, H, L = s["seq"], s["dim"], s["heads"], s["layers"]
    hd = D // H
    t = {k: torch.from_numpy(np.asarray(v)).double() for k, v in w.items() if np.asarray(v).dtype.kind == "f"}
    ids = torch.from_numpy(ids).long()
    B = ids.shape[0]
    h = t["embeddings.word"][ids] + t["embeddings.position"]
    if name == "bert_ids_hf":
        h = h + t["embeddings.token_type"]
    ln = lambda v, p: torch.nn.functional.layer_norm(v, (D,), t[p + ".weight"], t[p + ".bias"], 1e-5)  # noqa: E731
    lin = lambda v, p: v @ t[p + ".weight"] + t[p + ".bias"]  # noqa: E731
    h = ln(h, "embeddings.ln")
    pad = (ids == s["pad"])[:, None, None, :]  # [B, 1, 1, S]
    for i in range(L):
        p = "layer%d." % i
        q, k, v = (lin(h, p + n).reshape(B, S, H, hd).transpose(1, 2) for n in ("query", "key", "value"))
        sc = q @ k.transpose(-1, -2) / math.sqrt(hd)
        if name == "bert_ids_hf":
            sc = sc + t[p + "rel_bias"]
        sc = sc.masked_fill(pad, -math.inf)
        c = (torch.softmax(sc, -1) @ v).transpose(1, 2).reshape(B, S, D)
        h = ln(lin(c, p + "attn_out") + h, p + "ln1")
        m = lin(h, p + "intermediate")
        m = m * 0.5 * (1.0 + torch.erf(m / math.sqrt(2.0)))
        h = ln(lin(m, p + "output") + h, p + "ln2")
    return (h[:, 0] @ t["classifier.weight"].T + t["classifier.bias"]).numpy()


@pytest.mark.parametrize("int_input", [False, True])
@pytest.mark.parametrize("name", NAMES)
def test_cpu_executor_matches_torch_on_padded_rows(native, token_models, name, int_input):
    from die_amd.models import generic as G

    path, w = token_models[name, int_input]
    B = 5
    x = G.synthetic_input(name, B, seed=B)
    S = G.SPECS[name]["seq"]
    lengths = G.synthetic_lengths(name, B)
    assert lengths == [1, 32, S, 45, 33] and x.dtype == np.float32 and x.shape == (B, S)
    assert all((x[i, n:] == 0).all() and x[i, 0] >= 1 for i, n in enumerate(lengths))
    assert (x[2, :lengths[2]] == 0).sum() == 1  # every third sample has a hole
    got = native.cpu_run(path, x).reshape(B, -1)
    ref = _torch_forward(name, w, x)
    err = float(np.linalg.norm(got - ref) / np.linalg.norm(ref))
    print(name, int_input, "cpu executor vs torch float64 rel-L2 %.2e" % err)
    assert err <= 1e-5, err
