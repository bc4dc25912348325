"""Token models with attention_mask / token_type_ids graph inputs on the planner (no GPU): the two
lookups (+ positions) lower to ONE embed_tokens op reading the packed request rows in place, the
mask input roots the key-mask machinery (attention key_mask, masked mean pooling), roles come from
use in either declaration order, and everything the planner does not take is rejected with a report
line naming the input or node -- such a model then runs whole on the CPU engine, never partitioned.
Numerics: tests/test_cpu_multi_input.py (oracle), tests/test_gpu_embed_inputs.py (kernel),
tests/test_gpu_multi_input_models.py (engine)."""
import math

import numpy as np
import pytest

NAMES = ["bert_hf3", "sbert_hf2", "bert_hf3_maskfirst"]


@pytest.fixture(scope="module")
def paths(native, tmp_path_factory):
    from die_amd.models import generic as G

    d = tmp_path_factory.mktemp("multi_input_plan")
    out = {}
    for name in NAMES:
        out[name] = str(d / (name + ".onnx"))
        open(out[name], "wb").write(G.build_onnx(name))
    return out


def _plan(native, path, precision):
    r = native.plan_report(path, precision)
    assert r["supported"] and not r["unsupported"], r["text"]
    return native.plan_summary(path, 8, precision=precision)


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_multi_input_models_plan_with_one_embed_op_and_key_masked_attention(native, paths, name, precision):
    from die_amd.models import generic as G

    spec = G.SPECS[name]
    order, S = spec["inputs"], spec["seq"]
    K = len(order)
    s = _plan(native, paths[name], precision)
    kinds = [o["kind"] for o in s["ops"]]
    assert kinds.count("embed_tokens") == 1 and "rows_prep" not in kinds, kinds
    assert not {"where", "binary", "unary", "softmax", "gather_rows"} & set(kinds[:2]), kinds
    assert s["input_shape"] == [1, K, S]
    emb = next(o for o in s["ops"] if o["kind"] == "embed_tokens")
    assert (emb["seq"], emb["dim"], emb["row_pitch"]) == (S, spec["dim"], K * S)
    assert emb["positions"] and emb["token_type"] and emb["key_data"]
    # visible = not (mask == 0), on the truncated value for the INT64 declarations; read from the mask segment
    assert (emb["pad_op"], emb["pad_value"], emb["pad_negated"]) == ("equal", 0.0, True)
    assert emb["pad_truncated"] == spec["int_input"]
    assert emb["mask_offset"] == order.index("mask") * S
    # roles: the earlier-declared Gather index is the ids (its table gives `vocab`), the other the types
    roles = {e["name"]: (e["role"], e["offset"], e["numel"]) for e in s["inputs"]}
    assert roles["attention_mask"] == ("mask", order.index("mask") * S, S)
    if name == "bert_hf3":
        assert roles["input_ids"] == ("ids", 0, S) and roles["token_type_ids"] == ("types", 2 * S, S)
        assert (emb["vocab"], emb["type_rows"], emb["ids_offset"], emb["types_offset"]) == (spec["vocab"], 2, 0, 2 * S)
    elif name == "bert_hf3_maskfirst":  # declared mask, types, ids: token_type_ids is the earlier Gather index
        assert roles["token_type_ids"] == ("ids", S, S) and roles["input_ids"] == ("types", 2 * S, S)
        assert (emb["vocab"], emb["type_rows"], emb["ids_offset"], emb["types_offset"]) == (2, spec["vocab"], S, 2 * S)
    else:  # no type input: the constant type row
        assert roles["input_ids"] == ("ids", 0, S) and len(roles) == 2
        assert (emb["vocab"], emb["type_rows"], emb["types_offset"]) == (spec["vocab"], 0, -1)
    att = [o for o in s["ops"] if o["kind"] == "attention"]
    assert len(att) == spec["layers"]
    for o in att:
        assert o["key_mask"] is True and o["causal"] is False and o["bias_heads"] == spec["heads"], o
        assert o["bufs"]["in4"] == emb["bufs"]["out2"] and o["bufs"]["in5"] == emb["bufs"]["out3"]
    pools = [o for o in s["ops"] if o["kind"] == "pool_tokens"]
    if name == "sbert_hf2":
        assert len(pools) == 1 and pools[0]["masked"] is True and pools[0]["normalize"] is True
        assert pools[0]["bufs"]["in4"] == emb["bufs"]["out2"]
    else:
        assert not pools


def test_single_input_plans_report_their_one_input(native, tmp_path):
    from die_amd.models import generic as G

    for name, role in (("bert_ids_hf", "ids"), ("bert", "activations")):
        p = str(tmp_path / (name + ".onnx"))
        open(p, "wb").write(G.build_onnx(name))
        s = native.plan_summary(p, 8)
        assert [(e["role"], e["offset"], e["numel"]) for e in s["inputs"]] == [(role, 0, int(np.prod(G.input_shape(name))))]
        emb = [o for o in s["ops"] if o["kind"] == "embed_tokens"]
        assert all("row_pitch" not in o for o in emb)  # the single-input launch


# ---- rejections ---------------------------------------------------------------------------------------

def _tiny(variant):
    """A one-layer, two-head token classifier (S = 8, D = 64, vocab 11) with input_ids and
    attention_mask [N, 8] INT64, in the shape of bert_hf3 -- and one thing wrong with it."""
    from die_amd.utils.onnx_writer import INT64, GraphBuilder

    S, D, H, V = 8, 64, 2, 11
    hd = D // H
    rng = np.random.default_rng(0)
    w = lambda *shape: (0.3 * rng.standard_normal(shape)).astype(np.float32)  # noqa: E731
    g = GraphBuilder(name=variant)
    c = lambda v, n, t=np.int64: g.const(np.array(v, t), n)  # noqa: E731
    if variant == "not_a_token_model":  # float features gated by a second input: no Gather anywhere
        x = g.input("features", ["N", S])
        gate = g.input("attention_mask", ["N", S])
        y = g.node("Gemm", [g.node("Mul", [x, gate], name="gated"), g.init("fc.weight", w(3, S))], name="classifier", transB=1)
        g.output(y, ["N", 3])
        return g.model_proto(opset=17)
    ids = g.input("input_ids", ["N", S], elem_type=INT64)
    mask_dims = {"other_length": ["N", 6], "other_rank": ["N", 1, S]}.get(variant, ["N", S])
    mask = g.input("attention_mask", mask_dims, elem_type=INT64)
    h = g.node("Gather", [g.init("embeddings.word", w(V, D)), ids], name="embeddings.lookup", axis=0)
    h = g.node("Add", [h, g.init("embeddings.position", w(1, S, D))], name="embeddings.add_position")
    if variant == "extra_input":  # a third input that is neither ids nor a mask: scaled into the rows
        extra = g.input("token_weights", ["N", S])
        e = g.node("Unsqueeze", [g.node("Relu", [extra], name="weights_relu"), c([-1], "last")], name="weights_col")
        h = g.node("Mul", [h, e], name="weighted_rows")
    if variant == "four_inputs":
        for k in range(2):
            g.input("more%d" % k, ["N", S], elem_type=INT64)
    key_src = ids if variant == "both_ways" else mask  # both_ways: the ids index the Gather AND are the mask
    if variant == "other_rank":
        m = g.node("Unsqueeze", [key_src, c([1], "axis1")], name="extended_mask")
    else:
        m = g.node("Unsqueeze", [key_src, c([1, 2], "axes12")], name="extended_mask")
    m = g.node("Cast", [m], name="extended_mask_f", to=1)
    key_term = g.node("Mul", [g.node("Sub", [c(1.0, "one", np.float32), m], name="inverted_mask"),
                              c(-10000.0, "mask_value", np.float32)], name="additive_mask")

    def linear(inp, name):
        return g.node("Add", [g.node("MatMul", [inp, g.init(name + ".weight", w(D, D))], name=name + "/MatMul"),
                              g.init(name + ".bias", w(D))], name=name + "/Add")

    heads, merge = c([0, 0, H, hd], "heads_shape"), c([0, 0, D], "merge_shape")
    q = g.node("Transpose", [g.node("Reshape", [linear(h, "query"), heads], name="q_heads")], name="q_perm", perm=[0, 2, 1, 3])
    k = g.node("Transpose", [g.node("Reshape", [linear(h, "key"), heads], name="k_heads")], name="k_perm", perm=[0, 2, 3, 1])
    v = g.node("Transpose", [g.node("Reshape", [linear(h, "value"), heads], name="v_heads")], name="v_perm", perm=[0, 2, 1, 3])
    sc = g.node("Div", [g.node("MatMul", [q, k], name="scores"), c(math.sqrt(hd), "sqrt_d", np.float32)], name="scale")
    if variant == "mask_and_causal":
        sc = g.node("Where", [g.init("causal_mask", np.tril(np.ones((1, 1, S, S), np.bool_))), sc,
                              c(-1e4, "causal_fill", np.float32)], name="causal")
    sc = g.node("Softmax", [g.node("Add", [sc, key_term], name="mask/Add")], name="softmax", axis=-1)
    ctx = g.node("Reshape", [g.node("Transpose", [g.node("MatMul", [sc, v], name="context")], name="ctx_perm", perm=[0, 2, 1, 3]),
                             merge], name="ctx_merge")
    cls = g.node("Gather", [ctx, c(0, "cls_index")], name="cls_token", axis=1)
    y = g.node("Gemm", [cls, g.init("classifier.weight", w(3, D)), g.init("classifier.bias", w(3))], name="classifier", transB=1)
    g.output(y, ["N", 3])
    return g.model_proto(opset=17)


REJECTED = {  # variant -> (what the report line must name, request numel, runs on the CPU executor)
    "other_length": ("attention_mask", 14, False),  # (6 mask values do not broadcast onto 8 keys: it loads, no more)
    "other_rank": ("attention_mask", 16, True),
    "extra_input": ("token_weights", 24, True),
    "both_ways": ("input_ids", 16, True),
    "mask_and_causal": ("ctx_merge", 16, True),  # unchanged: reported where the attention materialises
    "not_a_token_model": ("attention_mask", 16, True),
    "four_inputs": ("more1", 32, True),
}


def test_the_tiny_model_itself_plans(native, tmp_path):
    p = str(tmp_path / "tiny.onnx")
    open(p, "wb").write(_tiny("ok"))
    s = _plan(native, p, "fp32")
    assert s["input_shape"] == [1, 2, 8] and [o["kind"] for o in s["ops"]].count("embed_tokens") == 1
    assert all(o["key_mask"] for o in s["ops"] if o["kind"] == "attention")


@pytest.mark.parametrize("variant", list(REJECTED))
def test_rejections_name_the_offender_and_fall_to_the_cpu_engine(native, tmp_path, variant):
    offender, numel, runs = REJECTED[variant]
    p = str(tmp_path / (variant + ".onnx"))
    open(p, "wb").write(_tiny(variant))
    r = native.plan_report(p, "fp32")
    assert not r["supported"] and r["unsupported"], variant
    print(variant, r["text"])
    assert any(offender in it["node"] or offender in it["error"] for it in r["unsupported"]), r["text"]
    with pytest.raises(native.NativeError):
        native.plan_summary(p, 8)
    with pytest.raises(native.NativeError):  # never partitioned into HIP + CPU pieces
        native.hybrid_partition(p, 8)
    assert native.model_inputs(p)["input_numel"] == numel
    eng = native.Engine(p, device="auto", max_batch=4)
    try:
        assert eng.refresh_info()["name"] == "cpu" and eng.input_numel == numel
        if runs:
            x = np.ones((2, numel), np.float32)
            y = eng.run(x)
            assert y.shape == (2, 3) and np.isfinite(y).all()
    finally:
        eng.close()


def test_a_second_ids_derived_pad_test_next_to_a_mask_input_is_two_pad_tests(native, tmp_path):
    """The attention takes the mask input, the pooling a mask recomputed from the ids: rejected like
    two different pad tests of a single-input model."""
    from die_amd.models import generic as G

    blob, _ = G.build_token_encoder(spec="sbert_hf2", inputs=("ids", "mask"))
    ok = str(tmp_path / "ok.onnx")
    open(ok, "wb").write(blob)
    assert native.plan_report(ok, "fp32")["supported"]
    orig = G._sentence_head

    def ids_derived_head(g, spec, h, is_pad, mask_f, mask_in=None):
        import numpy as np

        vis = g.node("Greater", ["input_ids", g.const(np.array(0, np.float32), "pad_id")], name="ids_visible")
        return orig(g, spec, h, None, None, vis)

    G._sentence_head = ids_derived_head
    try:
        blob, _ = G.build_token_encoder(spec="sbert_hf2", inputs=("ids", "mask"))
    finally:
        G._sentence_head = orig
    p = str(tmp_path / "two_tests.onnx")
    open(p, "wb").write(blob)
    r = native.plan_report(p, "fp32")
    assert not r["supported"] and any("pad test" in it["error"] for it in r["unsupported"]), r["text"]
