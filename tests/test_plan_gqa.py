"""Grouped-query attention on the planner (no GPU): HF's repeat_kv (Unsqueeze -> Expand -> Reshape on a
K / V heads view) defines a heads view of the same buffer with a group size, the attention op carries
kv_heads, no op and no copy is emitted for the repeat, and each unsupported variant is rejected with a
report line that names a node.  Numerics: tests/test_cpu_gqa.py (CPU executor),
tests/test_gpu_attention_gqa.py (kernel), tests/test_gpu_gqa_models.py (engine)."""
import numpy as np
import pytest

NAMES = ["gqa_enc", "mqa_causal", "gqa_hd128"]


@pytest.fixture(scope="module")
def gqa_models(native, tmp_path_factory):
    from die_amd.models import generic as G

    d = tmp_path_factory.mktemp("gqa_plan")
    out = {}
    for name in NAMES:
        for twin in (False, True):
            p = str(d / (name + ("_mha" if twin else "") + ".onnx"))
            open(p, "wb").write(G.BUILDERS[name](0, expand_kv=twin)[0])
            out[name, twin] = p
    return out


def _plan(native, path, precision):
    r = native.plan_report(path, precision)
    assert r["supported"] and not r["unsupported"] and r["blocked"] == 0, r["text"]
    return native.plan_summary(path, 8, precision=precision)


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_gqa_models_plan_with_kv_heads(native, gqa_models, name, precision):
    """Before the repeat_kv lowering the report named the Unsqueeze of the heads view."""
    from die_amd.models import generic as G

    spec = G.SPECS[name]
    s = _plan(native, gqa_models[name, False], precision)
    ops = s["ops"]
    kinds = [o["kind"] for o in ops]
    attn = [o for o in ops if o["kind"] == "attention"]
    assert len(attn) == spec["layers"], kinds
    hd = spec["dim"] // spec["heads"]
    for o in attn:
        assert (o["heads"], o["kv_heads"], o["head_dim"]) == (spec["heads"], spec["kv_heads"], hd), o
        assert o["causal"] == (name == "mqa_causal") and o["key_mask"] == (name == "gqa_enc") and o["bias_heads"] == 0, o
    # RoPE on Q and on the kv_heads-head K; nothing copies or expands K / V
    ropes = [o for o in ops if o["kind"] == "rope"]
    assert len(ropes) == (0 if name == "mqa_causal" else 2 * spec["layers"]), kinds
    assert sorted(o["heads"] for o in ropes[:2]) == ([] if name == "mqa_causal" else [spec["kv_heads"], spec["heads"]])
    assert not {"copy_cols", "bmm", "softmax", "where"} & set(kinds), kinds
    for o in ops:
        assert "repeat" not in o["name"], o
    # the twin plans to the same op kinds: the repeat adds no op
    t = _plan(native, gqa_models[name, True], precision)
    assert [o["kind"] for o in t["ops"]] == kinds
    for o in t["ops"]:
        if o["kind"] == "attention":
            assert o["kv_heads"] == o["heads"] == spec["heads"], o
    # the attention does the same MACs; the K / V projections do less
    assert [o["gflop"] for o in attn] == [o["gflop"] for o in t["ops"] if o["kind"] == "attention"]
    assert s["gflop"] < t["gflop"] if "gflop" in s else True


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_mqa_causal_reads_column_blocks_of_one_fused_gemm(native, gqa_models, precision):
    from die_amd.models import generic as G

    spec = G.SPECS["mqa_causal"]
    D, hd = spec["dim"], spec["dim"] // spec["heads"]
    s = _plan(native, gqa_models["mqa_causal", False], precision)
    ops = s["ops"]
    for i, o in enumerate(ops):
        if o["kind"] != "attention":
            continue
        qkv = [p for p in ops[:i] if p["kind"] == "conv" and p["name"].endswith("+qkv")][-1]
        assert qkv["N"] == D + 2 * hd, qkv
        b = o["bufs"]
        assert b["in"] == b["in2"] == b["in3"] == qkv["bufs"]["out"], (b, qkv)
        assert o["cols"] == [0, D, D + hd] and o["lds"] == [D + 2 * hd] * 3, o
    assert sum(1 for p in ops if p["kind"] == "conv" and p["name"].endswith("+qkv")) == spec["layers"]


# ---- minimal graphs: one thing wrong per caller ---------------------------------------------------------

def _tiny_gqa(tmp_path, name, D=256, H=4, Hkv=2, S=8, gk=None, gv=None, repeat_q=False, before_transpose=False,
              expand_shape=None, unsqueeze_axis=2, extra_reader=False, bias=False, causal_keymask=False, q_heads=None):
    """embeddings [N, S*D] -> Q [H heads] / K / V [Hkv heads] -> repeat_kv on K and V -> attention -> mean over
    the tokens."""
    from die_amd.utils.onnx_writer import GraphBuilder

    rng = np.random.default_rng(0)
    hd = D // H
    G = H // Hkv
    gk = G if gk is None else gk
    gv = G if gv is None else gv
    g = GraphBuilder(name=name)
    x = g.input("embeddings", ["N", S * D])
    h = g.node("Reshape", [x, g.const(np.array([0, S, D], np.int64), "seq_shape")], name="to_tokens")
    i64 = lambda v, n: g.const(np.array(v, np.int64), n)

    def linear(name_, width):
        w = g.init(name_ + ".weight", (rng.standard_normal((D, width)) / np.sqrt(D)).astype(np.float32))
        return g.node("MatMul", [h, w], name=name_)

    def heads(v, p, n):
        return g.node("Reshape", [v, i64([0, 0, n, hd], "hs")], name=p + "_heads")

    def perm(v, p):
        return g.node("Transpose", [v], name=p + "_perm", perm=[0, 2, 1, 3])

    def repeat(v, p, n, G_):
        if before_transpose:  # [N, S, n, hd] -> [N, S, n, G, hd] -> [N, S, n * G, hd]
            u = g.node("Unsqueeze", [v, i64([3], "ax")], name=p + "_repeat/unsqueeze")
            e = g.node("Expand", [u, i64([1, S, n, G_, hd], "es")], name=p + "_repeat/expand")
            return g.node("Reshape", [e, i64([0, S, n * G_, hd], "ms")], name=p + "_repeat/merge")
        u = g.node("Unsqueeze", [v, i64([unsqueeze_axis], "ax")], name=p + "_repeat/unsqueeze")
        shape = expand_shape if expand_shape is not None else [1, n, G_, S, hd]
        e = g.node("Expand", [u, i64(shape, "es")], name=p + "_repeat/expand")
        return g.node("Reshape", [e, i64([0, n * G_, S, hd], "ms")], name=p + "_repeat/merge")

    Hq = q_heads or H
    q = heads(linear("query", (Hq // 2 if repeat_q else Hq) * hd), "q", Hq // 2 if repeat_q else Hq)
    k = heads(linear("key", Hkv * hd), "k", Hkv)
    v = heads(linear("value", Hkv * hd), "v", Hkv)
    if before_transpose:
        q, k, v = perm(q, "q"), perm(repeat(k, "k", Hkv, gk), "k"), perm(repeat(v, "v", Hkv, gv), "v")
    else:
        q, k, v = perm(q, "q"), repeat(perm(k, "k"), "k", Hkv, gk), repeat(perm(v, "v"), "v", Hkv, gv)
        if repeat_q:
            q = repeat(q, "q", Hq // 2, 2)
    extra = g.node("ReduceMean", [g.node("Reshape", [g.node("Transpose", [v], name="v_back", perm=[0, 2, 1, 3]),
                                                     i64([0, 0, D], "vm")], name="v_merge")], name="v_mean", axes=[1],
                   keepdims=0) if extra_reader else None
    sc = g.node("Div", [g.node("MatMul", [q, g.node("Transpose", [k], name="k_t", perm=[0, 1, 3, 2])], name="scores"),
                        g.const(np.array(np.sqrt(hd), np.float32), "sqrt_d")], name="scale")
    if bias:
        sc = g.node("Add", [sc, g.init("rel_bias", rng.standard_normal((1, Hq, S, S)).astype(np.float32))], name="rel_bias/Add")
    sc = g.node("Softmax", [sc], name="softmax", axis=-1)
    ctx = g.node("Reshape", [g.node("Transpose", [g.node("MatMul", [sc, v], name="context")], name="ctx_perm", perm=[0, 2, 1, 3]),
                             i64([0, 0, Hq * hd], "merge_shape")], name="ctx_merge")
    out = g.node("ReduceMean", [ctx], name="mean_pool", axes=[1], keepdims=0)
    if extra is not None:
        out = g.node("Add", [out, extra], name="sum")
    g.output(out, ["N", Hq * hd])
    p = str(tmp_path / (name + ".onnx"))
    open(p, "wb").write(g.model_proto(opset=17))
    return p


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
@pytest.mark.parametrize("kwargs,kv", [(dict(), 2), (dict(Hkv=1), 1), (dict(expand_shape=[1, 1, 2, 1, 1]), 2),
                                        (dict(Hkv=4), 4)])
def test_tiny_gqa_graph_lowers_to_one_attention(native, tmp_path, precision, kwargs, kv):
    """The builder of the rejections below, with nothing wrong (Hkv = 4: a repeat over groups of one)."""
    s = _plan(native, _tiny_gqa(tmp_path, "tiny_ok", **kwargs), precision)
    kinds = [o["kind"] for o in s["ops"]]
    assert kinds == ["rows_prep", "conv", "conv", "conv", "attention", "gap", "bf16_to_f32"], kinds
    assert s["ops"][4]["kv_heads"] == kv and s["ops"][4]["heads"] == 4


@pytest.mark.parametrize("case,kwargs,node,words", [
    ("groups_differ", dict(Hkv=1, gk=4, gv=2), "context", "one group size"),
    ("q_repeated", dict(repeat_q=True), "scores", "first operand"),
    ("before_transpose", dict(before_transpose=True), "k_repeat/unsqueeze", "before the head Transpose"),
    ("other_axis", dict(unsqueeze_axis=1), "k_repeat/unsqueeze", "axes [2]"),
    ("other_dims", dict(expand_shape=[1, 2, 2, 8, 128]), "k_repeat/expand", "expands axis 2 alone"),
    ("expand_seq", dict(S=1, expand_shape=[1, 2, 2, 4, 64]), "k_repeat/expand", "expands axis 2 alone"),
    ("extra_reader", dict(extra_reader=True), "v_repeat/merge", "is read by Reshape v_merge"),
    ("group_mismatch", dict(q_heads=6, D=384, Hkv=2, gk=2, gv=2, H=6), "scores", "Q has 6 heads and K 4"),
    ("bias_table", dict(bias=True), "ctx_merge", "bias table"),
    ("head_dim", dict(D=128), "ctx_merge", "head dim 64 or 128"),
])
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_gqa_rejections_name_the_node(native, tmp_path, case, kwargs, node, words, precision):
    path = _tiny_gqa(tmp_path, case, **kwargs)
    r = native.plan_report(path, precision)  # reports, never throws
    assert not r["supported"]
    lines = [u for u in r["unsupported"] if u["node"] == node and words in u["error"]]
    assert lines, r["text"]
    with pytest.raises(native.NativeError):
        native.plan_summary(path, 8, precision=precision)
