"""Rotary position embeddings and RMSNorm on the planner (no GPU): the seven exported RoPE nodes on a
heads view lower to one rope op per Q / K whose output the attention reads, the decomposed torch
RMSNorm and the single-node forms lower to the layernorm op in its rms mode, and each unsupported
variant is rejected with a report line that names a node of the pattern.  Numerics on the device:
tests/test_gpu_rope_rows.py, tests/test_gpu_rmsnorm_rows.py (kernels), tests/test_gpu_rope_models.py
(engine)."""
import numpy as np
import pytest

NAMES = ["rope_bert", "rope_bert_nshd", "llama_enc", "llama_enc_rmsnode"]

# op kinds of models that existed before RoPE / RMSNorm, as the planner lowered them then (fp32, max batch 8)
KINDS_BEFORE = {
    "bert": ["rows_prep", "conv", "attention", "conv", "layernorm", "conv", "conv", "layernorm", "conv", "attention",
             "conv", "layernorm", "conv", "conv", "layernorm", "gap", "conv", "bf16_to_f32"],
    "gpt_causal": ["rows_prep", "layernorm", "conv", "attention", "conv", "conv", "conv", "conv", "attention", "conv", "conv",
                   "conv", "layernorm", "gap", "conv", "bf16_to_f32"],  # pre-LN: most LayerNorms folded into their GEMMs
    "sbert_ids_hf": ["embed_tokens", "layernorm", "conv", "attention", "conv", "layernorm", "conv", "conv", "layernorm",
                     "conv", "attention", "conv", "layernorm", "conv", "conv", "layernorm", "pool_tokens"],
}


@pytest.fixture(scope="module")
def rope_models(native, tmp_path_factory):
    from die_amd.models import generic as G

    d = tmp_path_factory.mktemp("rope_plan")
    out = {}
    for name in NAMES + sorted(KINDS_BEFORE):
        p = str(d / (name + ".onnx"))
        open(p, "wb").write(G.build_onnx(name))
        out[name] = p
    return out


def _plan(native, path, precision):
    r = native.plan_report(path, precision)
    assert r["supported"] and not r["unsupported"], r["text"]
    return native.plan_summary(path, 8, precision=precision)


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_models_are_supported(native, rope_models, name, precision):
    """Before this lowering the report listed the rotation's Slice / Mul / Concat nodes (and the
    RMSNorm's ReduceMean) and the model left the GPU."""
    r = native.plan_report(rope_models[name], precision)
    assert r["supported"] and not r["unsupported"] and r["blocked"] == 0, r["text"]


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_rope_ops_feed_the_attention(native, rope_models, name, precision):
    from die_amd.models import generic as G

    spec = G.SPECS[name]
    s = _plan(native, rope_models[name], precision)
    ops = s["ops"]
    kinds = [o["kind"] for o in ops]
    ropes = [o for o in ops if o["kind"] == "rope"]
    assert len(ropes) == 2 * spec["layers"], kinds
    hd = spec["dim"] // spec["heads"]
    for o in ropes:
        assert (o["heads"], o["head_dim"], o["seq"]) == (spec["heads"], hd, spec["seq"]), o
        assert o["layout"] == spec.get("layout", "nhsd"), o
        assert o["ld_in"] >= spec["dim"] and o["col"] % spec["dim"] == 0 and o["col"] + spec["dim"] <= o["ld_in"], o
        assert o["bufs"]["in"] != o["bufs"]["out"]
    # nothing of the rotation is left as an elementwise / copy op
    for o in ops:
        if o["kind"] in ("unary", "binary", "copy_cols", "affine", "where"):
            assert "rope" not in o["name"], o
    if name.startswith("rope_bert"):
        assert not {"unary", "binary", "copy_cols"} & set(kinds), kinds
    # every attention reads the two rope outputs just before it for Q and K, and an unrotated buffer for V
    attn = [i for i, o in enumerate(ops) if o["kind"] == "attention"]
    assert len(attn) == spec["layers"]
    for i in attn:
        before = [o for o in ops[:i] if o["kind"] == "rope"][-2:]
        q = next(o for o in before if "q_rope" in o["name"])
        k = next(o for o in before if "k_rope" in o["name"])
        b = ops[i]["bufs"]
        assert b["in"] == q["bufs"]["out"] and b["in2"] == k["bufs"]["out"], (b, q, k)
        assert b["in3"] not in (q["bufs"]["out"], k["bufs"]["out"])
    if name.startswith("rope_bert"):  # fused QKV GEMM: both rope ops read its buffer at their column block, V reads it too
        for i in attn:
            q, k = [o for o in ops[:i] if o["kind"] == "rope"][-2:]
            assert q["bufs"]["in"] == k["bufs"]["in"] == ops[i]["bufs"]["in3"]
            assert (q["ld_in"], q["col"], k["col"]) == (3 * spec["dim"], 0, spec["dim"])


@pytest.mark.parametrize("name", ["llama_enc", "llama_enc_rmsnode"])
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_llama_norms_are_rms_layernorm_ops(native, rope_models, name, precision):
    from die_amd.models import generic as G

    spec = G.SPECS[name]
    s = _plan(native, rope_models[name], precision)
    kinds = [o["kind"] for o in s["ops"]]
    lns = [o for o in s["ops"] if o["kind"] == "layernorm"]
    assert len(lns) == 2 * spec["layers"] + 1, kinds
    assert all(o["rms"] and not o["stats_only"] for o in lns), lns
    assert kinds.count("embed_tokens") == 1 and kinds.count("pool_tokens") == 1 and kinds[-1] == "pool_tokens", kinds
    emb = next(o for o in s["ops"] if o["kind"] == "embed_tokens")
    assert emb["key_data"] and not emb["positions"] and not emb["token_type"], emb
    assert all(o["key_mask"] for o in s["ops"] if o["kind"] == "attention")
    # the RMSNorm chain left no pow / reduce / sqrt ops; the SwiGLU is a sigmoid and two multiplies per layer
    assert kinds.count("unary") == spec["layers"] and kinds.count("binary") == 2 * spec["layers"], kinds
    assert not {"gap", "affine", "softmax"} & set(kinds), kinds
    assert s["output_shape"] == [1, spec["dim"]] and s["input_shape"] == [1, spec["seq"]]
    # no folding of an RMSNorm into its GEMM readers
    assert not any(o["kind"] == "conv" and (o["layernorm_folded"] or o["stats_from_producer"]) for o in s["ops"])


@pytest.mark.parametrize("name", sorted(KINDS_BEFORE))
def test_models_from_before_lower_as_before(native, rope_models, name):
    s = _plan(native, rope_models[name], "fp32")
    assert [o["kind"] for o in s["ops"]] == KINDS_BEFORE[name]
    assert not any(o["kind"] == "layernorm" and o["rms"] for o in s["ops"])


def test_vit_layernorms_are_not_rms(native, models):
    path = models["get_vit"]("tiny")[0]
    for precision in ("fp32", "bf16"):
        s = native.plan_summary(path, 8, precision=precision)
        lns = [o for o in s["ops"] if o["kind"] == "layernorm"]
        assert lns and not any(o["rms"] for o in lns)
        assert "rope" not in [o["kind"] for o in s["ops"]]


# ---- minimal graphs: RoPE ------------------------------------------------------------------------------

def _tiny_rope(tmp_path, name, D=128, H=2, S=8, lo=None, hi=None, step=1, table="init", table_shape=None, partial=False):
    """embeddings [N, S*D] -> Q / K / V projections -> heads [N, H, S, hd] -> rotation of Q and K -> attention
    -> mean over the tokens; one thing wrong per caller."""
    from die_amd.models import generic as G
    from die_amd.utils.onnx_writer import GraphBuilder

    rng = np.random.default_rng(0)
    hd = D // H
    g = GraphBuilder(name=name)
    x = g.input("embeddings", ["N", S * D])
    h = g.node("Reshape", [x, g.const(np.array([0, S, D], np.int64), "seq_shape")], name="to_tokens")
    heads_shape = g.const(np.array([0, 0, H, hd], np.int64), "heads_shape")
    i64 = lambda v, n: g.const(np.array([v], np.int64), n)
    rot = hd // 2 if partial else hd  # columns the rotation covers
    c, s = G.rope_tables(S, rot)
    shape = table_shape or (1, 1, S, rot)
    if table_shape is not None:
        c, s = np.resize(c, shape), np.resize(s, shape)
    cos, sin = g.init("rope.cos", c.reshape(shape)), g.init("rope.sin", s.reshape(shape))
    if table == "computed":  # a table that a node produces (a position_ids lookup in a cache)
        pos = g.const(np.arange(S, dtype=np.int64), "positions")
        cos = g.node("Gather", [g.init("rope.cos_cache", c.reshape(S, rot)), pos], name="cos_lookup", axis=0)
        sin = g.node("Gather", [g.init("rope.sin_cache", s.reshape(S, rot)), pos], name="sin_lookup", axis=0)

    def linear(name_):
        w = g.init(name_ + ".weight", (rng.standard_normal((D, D)) / np.sqrt(D)).astype(np.float32))
        b = g.init(name_ + ".bias", np.zeros(D, np.float32))
        return g.node("Add", [g.node("MatMul", [h, w], name=name_ + "/MatMul"), b], name=name_ + "/Add")

    def rope(v, p):
        if partial:  # rotate the first half of the head, pass the second through
            keep = g.node("Slice", [v, i64(rot, "p0"), i64(hd, "p1"), i64(-1, "pax")], name=p + "rope/pass_part")
            v = g.node("Slice", [v, i64(0, "r0"), i64(rot, "r1"), i64(-1, "rax")], name=p + "rope/rot_part")
        l0, l1 = lo or (0, rot // 2)
        h0, h1 = hi or (rot // 2, rot)
        a = g.node("Slice", [v, i64(l0, "l0"), i64(l1, "l1"), i64(-1, "lax"), i64(step, "lst")], name=p + "rope/lo")
        b = g.node("Slice", [v, i64(h0, "h0"), i64(h1, "h1"), i64(-1, "hax"), i64(step, "hst")], name=p + "rope/hi")
        r = g.node("Concat", [g.node("Neg", [b], name=p + "rope/neg"), a], name=p + "rope/rotate_half", axis=-1)
        y = g.node("Add", [g.node("Mul", [v, cos], name=p + "rope/cos"), g.node("Mul", [r, sin], name=p + "rope/sin")],
                   name=p + "rope/add")
        return g.node("Concat", [y, keep], name=p + "rope/join", axis=-1) if partial else y

    q = rope(g.node("Transpose", [g.node("Reshape", [linear("query"), heads_shape], name="q_heads")], name="q_perm",
                    perm=[0, 2, 1, 3]), "q_")
    k = rope(g.node("Transpose", [g.node("Reshape", [linear("key"), heads_shape], name="k_heads")], name="k_perm",
                    perm=[0, 2, 1, 3]), "k_")
    k = g.node("Transpose", [k], name="k_t", perm=[0, 1, 3, 2])
    v = g.node("Transpose", [g.node("Reshape", [linear("value"), heads_shape], name="v_heads")], name="v_perm",
               perm=[0, 2, 1, 3])
    sc = g.node("Softmax", [g.node("Div", [g.node("MatMul", [q, k], name="scores"),
                                           g.const(np.array(np.sqrt(hd), np.float32), "sqrt_d")], name="scale")],
                name="softmax", axis=-1)
    ctx = g.node("Reshape", [g.node("Transpose", [g.node("MatMul", [sc, v], name="context")], name="ctx_perm", perm=[0, 2, 1, 3]),
                             g.const(np.array([0, 0, D], np.int64), "merge_shape")], name="ctx_merge")
    g.output(g.node("ReduceMean", [ctx], name="mean_pool", axes=[1], keepdims=0), ["N", D])
    p = str(tmp_path / (name + ".onnx"))
    open(p, "wb").write(g.model_proto(opset=17))
    return p


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_tiny_rope_graph_lowers_to_two_rope_ops(native, tmp_path, precision):
    """The builder of the rejections below, with nothing wrong."""
    s = _plan(native, _tiny_rope(tmp_path, "tiny_ok"), precision)
    kinds = [o["kind"] for o in s["ops"]]
    assert kinds == ["rows_prep", "conv", "rope", "rope", "attention", "gap", "bf16_to_f32"], kinds


@pytest.mark.parametrize("case,kwargs,words", [
    ("interleaved", dict(lo=(0, 64), hi=(1, 64), step=2), "interleaved"),
    ("halves_apart", dict(lo=(0, 24), hi=(24, 64)), "[hd/2, hd)"),
    ("partial", dict(partial=True), "partial"),
    ("computed_tables", dict(table="computed"), "must be an initializer"),
    ("table_shape", dict(table_shape=(1, 1, 1, 64)), "does not broadcast"),
    ("head_dim", dict(D=96), "head dim 48"),
])
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_rope_rejections_name_a_node_of_the_pattern(native, tmp_path, case, kwargs, words, precision):
    path = _tiny_rope(tmp_path, case, **kwargs)
    r = native.plan_report(path, precision)  # reports, never throws
    assert not r["supported"]
    lines = [u for u in r["unsupported"] if u["node"].startswith("q_rope/") and words in u["error"]]
    assert lines, r["text"]
    with pytest.raises(native.NativeError):
        native.plan_summary(path, 8, precision=precision)


# ---- minimal graphs: RMSNorm ---------------------------------------------------------------------------

def _tiny_rms(tmp_path, name, D=64, S=6, head="pow", exponent=2.0, axes=(-1,), eps="scalar", eps_first=False,
              norm="div", x_first=True, weight=True, weight_first=False, extra_reader=False, node=None, second_used=False):
    """embeddings [N, S*D] -> [N, S, D] -> RMSNorm in one of its spellings -> mean over the tokens."""
    from die_amd.utils.onnx_writer import GraphBuilder

    rng = np.random.default_rng(0)
    g = GraphBuilder(name=name)
    x = g.input("embeddings", ["N", S * D])
    h = g.node("Reshape", [x, g.const(np.array([0, S, D], np.int64), "seq_shape")], name="to_tokens")
    w = g.init("norm.weight", (1.0 + 0.1 * rng.standard_normal(D)).astype(np.float32))
    one = g.const(np.array(1.0, np.float32), "one")
    extra = None
    if node is not None:
        outs = ["norm_out", "norm_inv_std"] if second_used else ["norm_out"]
        y = g.node(node, [h, w], outputs=outs, name="norm", axis=-1, epsilon=1e-6)
        if second_used:
            y, extra = y[0], y[1]
    else:
        sq = g.node("Pow", [h, g.const(np.array(exponent, np.float32), "exponent")], name="norm/pow") if head == "pow" else \
            g.node("Mul", [h, h], name="norm/pow")
        ms = g.node("ReduceMean", [sq], name="norm/mean", axes=list(axes), keepdims=1)
        e = g.const(np.full(D, 1e-6, np.float32) if eps == "vector" else np.array(1e-6, np.float32), "eps")
        rt = g.node("Sqrt", [g.node("Add", [e, ms] if eps_first else [ms, e], name="norm/add_eps")], name="norm/sqrt")
        if norm == "div":
            y = g.node("Div", [h, rt], name="norm/normalize")
        else:
            inv = g.node("Reciprocal", [rt], name="norm/rsqrt") if norm == "reciprocal" else \
                g.node("Div", [one, rt], name="norm/rsqrt")
            y = g.node("Mul", [h, inv] if x_first else [inv, h], name="norm/normalize")
        if weight:
            y = g.node("Mul", [w, y] if weight_first else [y, w], name="norm/scale")
        if extra_reader:
            extra = ms
    out = g.node("ReduceMean", [y], name="mean_pool", axes=[1], keepdims=0)
    if extra is not None:  # a second reader of the mean of squares / of the inv_std output
        out = g.node("Add", [out, g.node("ReduceMean", [g.node("Mul", [y, extra], name="rescaled")], name="mean_pool2", axes=[1],
                                         keepdims=0)], name="sum")
    g.output(out, ["N", D])
    p = str(tmp_path / (name + ".onnx"))
    open(p, "wb").write(g.model_proto(opset=17))
    return p


@pytest.mark.parametrize("case,kwargs", [
    ("div", dict()),
    ("square_mul", dict(head="mul")),
    ("eps_first", dict(eps_first=True)),
    ("reciprocal", dict(norm="reciprocal")),
    ("reciprocal_swapped", dict(norm="reciprocal", x_first=False)),
    ("one_over", dict(norm="one_over", weight_first=True)),
    ("one_over_swapped", dict(norm="one_over", x_first=False)),
    ("no_weight", dict(weight=False)),
    ("rms_node", dict(node="RMSNormalization")),
    ("simplified_node", dict(node="SimplifiedLayerNormalization")),
])
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_rmsnorm_spellings_are_one_rms_layernorm_op(native, tmp_path, case, kwargs, precision):
    s = _plan(native, _tiny_rms(tmp_path, case, **kwargs), precision)
    kinds = [o["kind"] for o in s["ops"]]
    assert kinds == ["rows_prep", "layernorm", "gap", "bf16_to_f32"], kinds
    assert s["ops"][1]["rms"] and not s["ops"][1]["stats_only"]


@pytest.mark.parametrize("case,kwargs,node,words", [
    ("exponent", dict(exponent=3.0), "norm/pow", "exponent must be 2"),
    ("axes", dict(axes=(1, 2)), "norm/pow", "last axis"),
    ("eps_vector", dict(eps="vector"), "norm/pow", "scalar constant"),
    ("pad_columns", dict(D=36), "norm/pow", "C % 8"),
    ("second_reader", dict(extra_reader=True), "norm/pow", "read by the Add of eps alone"),
    ("inv_std_used", dict(node="SimplifiedLayerNormalization", second_used=True), "norm", "must be unused"),
])
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_rmsnorm_rejections_name_the_node(native, tmp_path, case, kwargs, node, words, precision):
    path = _tiny_rms(tmp_path, case, **kwargs)
    r = native.plan_report(path, precision)
    assert not r["supported"]
    lines = [u for u in r["unsupported"] if u["node"] == node]
    assert lines and words in lines[0]["error"], r["text"]
    with pytest.raises(native.NativeError):
        native.plan_summary(path, 8, precision=precision)
