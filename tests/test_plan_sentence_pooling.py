"""Sentence embedders on the planner (no GPU): the masked mean over the visible tokens and the L2
normalisation after it lower to one pool_tokens op reading the key data the embed_tokens op writes;
an L2 normalisation of other rank-2 rows is a pool_tokens op with one token.  Also the rejections,
one minimal graph each.  Numerics on the device: tests/test_gpu_pool_tokens.py (kernel) and
tests/test_gpu_sentence_models.py (engine)."""
import numpy as np
import pytest

NAMES = ["sbert_ids", "sbert_ids_hf", "sbert_cls"]
# (masked, normalize, clip_min, eps, seq) of the one pool_tokens op
EXPECT = {"sbert_ids": (True, True, 1e-9, 1e-12, 48), "sbert_ids_hf": (True, True, 1e-9, 0.0, 160),
          "sbert_cls": (False, True, 0.0, 0.0, 1)}


@pytest.fixture(scope="module")
def sentence_models(native, tmp_path_factory):
    from die_amd.models import generic as G

    d = tmp_path_factory.mktemp("sentence_plan")
    out = {}
    for name in NAMES:
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
def test_sentence_models_plan_with_one_pool_tokens_op(native, sentence_models, name, precision):
    from die_amd.models import generic as G

    spec = G.SPECS[name]
    s = _plan(native, sentence_models[name], precision)
    kinds = [o["kind"] for o in s["ops"]]
    assert kinds.count("pool_tokens") == 1 and kinds.count("embed_tokens") == 1, kinds
    # the whole tail is that op, and it writes the fp32 output itself
    assert not {"binary", "unary", "where", "gap", "bf16_to_f32"} & set(kinds), kinds
    assert kinds[-1] == "pool_tokens"
    assert s["output_shape"] == [1, spec["dim"]] and s["input_shape"] == [1, spec["seq"]]
    op = next(o for o in s["ops"] if o["kind"] == "pool_tokens")
    emb = next(o for o in s["ops"] if o["kind"] == "embed_tokens")
    masked, normalize, clip_min, eps, seq = EXPECT[name]
    assert (op["masked"], op["normalize"], op["seq"], op["dim"]) == (masked, normalize, seq, spec["dim"]), op
    assert op["clip_min"] == pytest.approx(clip_min, rel=1e-6) and op["eps"] == pytest.approx(eps, rel=1e-6), op
    assert emb["key_data"]  # every body here has key-masked attention
    if masked:
        assert op["bufs"]["in4"] == emb["bufs"]["out2"] and op["bufs"]["in5"] == emb["bufs"]["out3"]
    else:
        assert "in4" not in op["bufs"] and "in5" not in op["bufs"]
    assert "out" not in op["bufs"]  # no bf16 round trip: fp32 straight into the output buffer
    for o in s["ops"]:
        if o["kind"] == "attention":
            assert o["key_mask"] and o["bufs"]["in4"] == emb["bufs"]["out2"]


# ---- minimal graphs -----------------------------------------------------------------------------------

def _tiny(tmp_path, name, sum_axis=1, count_use="div", divide=True, clip_max=None, norm=None, mask_seq=None,
          second_test=False):
    """ids [N, 8] -> Gather -> LayerNormalization -> masked mean over the visible tokens (the expanded
    sentence-transformers form), no attention; one thing wrong per caller."""
    from die_amd.utils.onnx_writer import INT64, GraphBuilder

    rng = np.random.default_rng(0)
    S, D, V = 8, 32, 16
    g = GraphBuilder(name=name)
    x = g.input("input_ids", ["N", S])
    ids = g.node("Cast", [x], name="ids_int", to=INT64)
    h = g.node("Gather", [g.init("table", rng.standard_normal((V, D)).astype(np.float32)), ids], name="lookup", axis=0)
    h = g.node("LayerNormalization", [h, g.init("ln.weight", np.ones(D, np.float32)), g.init("ln.bias", np.zeros(D, np.float32))],
               name="ln", axis=-1, epsilon=1e-5)
    vis = g.node("Not", [g.node("Equal", [ids, g.const(np.array(0, np.int64), "pad")], name="is_pad")], name="visible")
    last = g.const(np.array([-1], np.int64), "last_axis")
    tokens = g.const(np.array([1], np.int64), "token_axis")
    m = g.node("Unsqueeze", [vis, last], name="pool_mask")
    m = g.node("Expand", [m, g.const(np.array([1, mask_seq or S, D], np.int64), "mask_shape")], name="pool_mask_expanded")
    m = g.node("Cast", [m], name="pool_mask_f", to=1)
    summed = g.node("ReduceSum", [g.node("Mul", [h, m], name="masked_states"),
                                  g.const(np.array([sum_axis], np.int64), "sum_axis")], name="masked_sum", keepdims=0)
    cm = m
    if second_test:  # the count over another pad test (ids > 1)
        v2 = g.node("Greater", [ids, g.const(np.array(1, np.int64), "pad2")], name="visible2")
        cm = g.node("Cast", [g.node("Expand", [g.node("Unsqueeze", [v2, last], name="pool_mask2"),
                                               g.const(np.array([1, S, D], np.int64), "mask_shape2")], name="pool_mask2_expanded")],
                    name="pool_mask2_f", to=1)
    count = g.node("ReduceSum", [cm, tokens], name="visible_count", keepdims=0)
    clip_in = [count, g.const(np.array(1e-9, np.float32), "count_min")]
    if clip_max is not None:
        clip_in.append(g.const(np.array(clip_max, np.float32), "count_max"))
    count = g.node("Clip", clip_in, name="count_clamp")
    if not divide:
        y = summed if count_use == "none" else g.node("Add", [summed, count], name="sum_plus_count")
    elif count_use == "div":
        y = g.node("Div", [summed, count], name="mean_pool")
    else:  # the count divides something that is not a masked sum
        y = g.node("Div", [g.node("ReduceMean", [h], name="plain_mean", axes=[1], keepdims=0), count], name="mean_pool")
    if norm is not None:
        y = g.node("LpNormalization", [y], name="normalize", **norm)
    g.output(y, ["N", D])
    p = str(tmp_path / (name + ".onnx"))
    open(p, "wb").write(g.model_proto(opset=17))
    return p


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_pooling_alone_makes_the_embedding_write_the_key_data(native, tmp_path, precision):
    """No attention in the model: the pooling op is the key data's first and only reader."""
    s = _plan(native, _tiny(tmp_path, "pool_only"), precision)
    kinds = [o["kind"] for o in s["ops"]]
    assert kinds == ["embed_tokens", "layernorm", "pool_tokens"], kinds
    emb, op = s["ops"][0], s["ops"][2]
    assert emb["key_data"] and (emb["pad_op"], emb["pad_value"], emb["pad_negated"], emb["pad_truncated"]) == ("equal", 0.0, True, True)
    assert op["masked"] and not op["normalize"] and op["seq"] == 8 and op["dim"] == 32
    assert op["clip_min"] == pytest.approx(1e-9, rel=1e-6)
    assert op["bufs"]["in4"] == emb["bufs"]["out2"] and op["bufs"]["in5"] == emb["bufs"]["out3"]
    assert s["output_shape"] == [1, 32]


def test_normalisation_joins_the_pooled_vector(native, tmp_path):
    s = _plan(native, _tiny(tmp_path, "pool_norm", norm=dict(axis=-1, p=2)), "fp32")
    ops = [o for o in s["ops"] if o["kind"] == "pool_tokens"]
    assert len(ops) == 1 and ops[0]["masked"] and ops[0]["normalize"] and ops[0]["eps"] == 0.0


@pytest.mark.parametrize("case,kwargs,node,words", [
    ("mul_reader", dict(sum_axis=2), "masked_states", "ReduceSum(axis 1"),
    ("count_use", dict(count_use="mean"), "visible_count", "key mask"),
    ("count_other_test", dict(second_test=True), "mean_pool", "pad test"),
    ("sum_pooling", dict(divide=False, count_use="none"), "masked_sum", "divided"),
    ("sum_plus_count", dict(divide=False, count_use="add"), "masked_sum", "divided"),
    ("clip_max", dict(clip_max=100.0), "count_clamp", "max"),
    ("norm_p", dict(norm=dict(axis=-1, p=1)), "normalize", "p = 2"),
    ("norm_axis", dict(norm=dict(axis=0, p=2)), "normalize", "last axis"),
    ("mask_length", dict(mask_seq=4), "pool_mask_expanded", "[N, S, D]"),
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


def test_mask_of_another_length_than_the_rows(native, tmp_path):
    """Rows regrouped to 4 tokens of 64 against the mask of the 8 ids."""
    from die_amd.utils.onnx_writer import INT64, GraphBuilder

    rng = np.random.default_rng(0)
    S, D, V = 8, 32, 16
    g = GraphBuilder(name="mask_len")
    x = g.input("input_ids", ["N", S])
    ids = g.node("Cast", [x], name="ids_int", to=INT64)
    h = g.node("Gather", [g.init("table", rng.standard_normal((V, D)).astype(np.float32)), ids], name="lookup", axis=0)
    h = g.node("Reshape", [h, g.const(np.array([0, S // 2, 2 * D], np.int64), "regroup")], name="regrouped")
    m = g.node("Cast", [g.node("Unsqueeze", [g.node("Greater", [ids, g.const(np.array(0, np.int64), "pad")], name="visible"),
                                             g.const(np.array([-1], np.int64), "last_axis")], name="pool_mask")],
               name="pool_mask_f", to=1)
    tokens = g.const(np.array([1], np.int64), "token_axis")
    summed = g.node("ReduceSum", [g.node("Mul", [h, m], name="masked_states"), tokens], name="masked_sum", keepdims=0)
    count = g.node("ReduceSum", [m, tokens], name="visible_count", keepdims=0)
    g.output(g.node("Div", [summed, count], name="mean_pool"), ["N", 2 * D])
    p = str(tmp_path / "mask_len.onnx")
    open(p, "wb").write(g.model_proto(opset=17))
    r = native.plan_report(p, "fp32")
    assert not r["supported"]
    lines = [u for u in r["unsupported"] if u["node"] == "masked_states"]
    assert lines and "length 8 is not the rows' 4" in lines[0]["error"], r["text"]


def test_synthetic_lengths_never_give_an_all_pad_sample():
    """The oracle of the GPU tests stays free of NaN (ONNX: 0 / 0 for a sample with no visible token)."""
    from die_amd.models import generic as G

    for name in NAMES:
        x = G.synthetic_input(name, 16, seed=3)
        assert ((x != 0).sum(1) >= 1).all() and (x[:, 0] != 0).all()
        assert min(G.synthetic_lengths(name, 16)) >= 1
