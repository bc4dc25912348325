"""Attention with a constant additive bias or mask between Q K^T and the Softmax, on the planner
(no GPU): Add(scores, table) and Where(mask, scores, fill) fold into one dense table per attention
op, which the planner classifies (causal flag, per-head / shared table, nothing left) and hands to
the masked streaming kernel.  Numerics on the device: tests/test_gpu_attention_mask.py (kernel) and
tests/test_gpu_masked_models.py (engine)."""
import math

import numpy as np
import pytest

MASKED = ["gpt_causal", "bert_relpos", "bert_window", "bert_keymask"]
# model -> (causal, bias heads: 0 none, 1 shared, "H" per head)
EXPECT = {"gpt_causal": (True, 0), "bert_relpos": (False, "H"), "bert_window": (False, 1), "bert_keymask": (False, 1)}


@pytest.fixture(scope="module")
def masked_models(native, tmp_path_factory):
    from die_amd.models import generic as G

    d = tmp_path_factory.mktemp("masked")
    out = {}
    for name in MASKED:
        blob, weights = G.BUILDERS[name]()
        p = str(d / (name + ".onnx"))
        open(p, "wb").write(blob)
        out[name] = (p, weights)
    return out


def _variant(tmp_path, name, spec, score_ops):
    from die_amd.models import generic as G

    blob, weights = G.build_masked_encoder(0, spec=spec, score_ops=score_ops)
    p = str(tmp_path / (name + ".onnx"))
    open(p, "wb").write(blob)
    return p, weights


def _scaled(g, v, p, hd):
    return g.node("Div", [v, g.const(np.array(math.sqrt(hd), np.float32), "sqrt_d")], name=p + "scale")


def _attention_ops(native, path, precision):
    r = native.plan_report(path, precision)
    assert r["supported"], r["text"]
    s = native.plan_summary(path, 8, precision=precision)
    kinds = [o["kind"] for o in s["ops"]]
    # the chain is ONE attention op per layer: no where / binary / softmax op stands in for the mask
    assert "where" not in kinds and "binary" not in kinds and "softmax" not in kinds, kinds
    return [o for o in s["ops"] if o["kind"] == "attention"]


@pytest.mark.parametrize("name", MASKED)
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_masked_models_plan_as_one_attention_per_layer(native, masked_models, name, precision):
    from die_amd.models import generic as G

    att = _attention_ops(native, masked_models[name][0], precision)
    spec = G.SPECS[name]
    assert len(att) == spec["layers"]
    causal, heads = EXPECT[name]
    for o in att:
        assert o["causal"] is causal, o
        assert o["bias_heads"] == (spec["heads"] if heads == "H" else heads), o
    if name == "gpt_causal":  # causal attention does half the MACs: 4 hd nh S (S + 1) / 2
        S, D = spec["seq"], spec["dim"]
        assert att[0]["gflop"] == pytest.approx(4.0 * D * S * (S + 1) / 2 / 1e9, rel=1e-6)


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_alibi_is_causal_with_a_per_head_table(native, tmp_path, precision):
    """Per-head slopes and the -inf triangle in ONE Add: the planner splits it into the causal flag
    and the lower-triangle table."""
    from die_amd.models import generic as G

    spec = G.SPECS["bert_relpos"]
    S, H, hd = spec["seq"], spec["heads"], spec["dim"] // spec["heads"]
    i = np.arange(S)
    dist = (i[:, None] - i[None, :]).astype(np.float32)
    slopes = 2.0 ** -(np.arange(1, H + 1, dtype=np.float32) * 8 / H)
    table = np.where(dist >= 0, -slopes[:, None, None] * dist, -np.inf).astype(np.float32)[None]

    def ops(g, v, p, layer):
        return g.node("Add", [_scaled(g, v, p, hd), g.init(p + "alibi", table)], name=p + "alibi/Add")

    path, _ = _variant(tmp_path, "alibi", "bert_relpos", ops)
    for o in _attention_ops(native, path, precision):
        assert o["causal"] is True and o["bias_heads"] == H, o
        assert o["bias_masked"] == 0  # the triangle became the flag
        assert o["bias_sum"] == pytest.approx(float(np.tril(table[0]).sum(dtype=np.float64)), rel=1e-5)


def test_equal_heads_share_one_slice(native, tmp_path):
    from die_amd.models import generic as G

    spec = G.SPECS["bert_relpos"]
    S, H, hd = spec["seq"], spec["heads"], spec["dim"] // spec["heads"]
    one = np.random.default_rng(5).standard_normal((1, 1, S, S)).astype(np.float32)
    table = np.ascontiguousarray(np.broadcast_to(one, (1, H, S, S)))

    def ops(g, v, p, layer):
        return g.node("Add", [g.init(p + "table", table), _scaled(g, v, p, hd)], name=p + "table/Add")  # B + scores

    path, _ = _variant(tmp_path, "equal_heads", "bert_relpos", ops)
    for o in _attention_ops(native, path, "fp32"):
        assert o["causal"] is False and o["bias_heads"] == 1, o
        assert o["bias_sum"] == pytest.approx(float(one.sum(dtype=np.float64)), rel=1e-5)


def test_stacked_adds_and_a_late_scale_fold_into_one_table(native, tmp_path):
    """Add(A) -> Div(sqrt d) -> Add(B) -> Mul(0.5): one table (A / sqrt d + B) * 0.5; the [S, 1] and
    [1, S] broadcast forms; a Where with an all-true mask changes nothing."""
    from die_amd.models import generic as G

    spec = G.SPECS["bert_relpos"]
    S, H, hd = spec["seq"], spec["heads"], spec["dim"] // spec["heads"]
    rng = np.random.default_rng(6)
    A = rng.standard_normal((H, S, 1)).astype(np.float32)
    Bt = rng.standard_normal((1, S)).astype(np.float32)
    Bt[0, -3:] = -np.inf

    def ops(g, v, p, layer):
        v = g.node("Add", [v, g.init(p + "A", A)], name=p + "A/Add")
        v = _scaled(g, v, p, hd)
        v = g.node("Add", [v, g.init(p + "B", Bt)], name=p + "B/Add")
        v = g.node("Where", [g.init(p + "all", np.ones((S, S), np.bool_)), v,
                             g.const(np.array(np.finfo(np.float32).min, np.float32), "fill")], name=p + "where")
        return g.node("Mul", [v, g.const(np.array(0.5, np.float32), "half_scale")], name=p + "late_scale")

    path, _ = _variant(tmp_path, "stacked", "bert_relpos", ops)
    want = (A.astype(np.float64) / math.sqrt(hd) + Bt.astype(np.float64)) * 0.5  # [H, S, S]
    for o in _attention_ops(native, path, "fp32"):
        assert o["causal"] is False and o["bias_heads"] == H, o
        assert o["bias_masked"] == 3 * S * H
        assert o["bias_sum"] == pytest.approx(float(want[np.isfinite(want)].sum()), rel=1e-5)


def test_where_with_the_mask_selecting_the_fill(native, tmp_path):
    """Where(C, fill, scores): C marks the MASKED positions (the other operand order)."""
    from die_amd.models import generic as G

    spec = G.SPECS["gpt_causal"]
    S, hd = spec["seq"], spec["dim"] // spec["heads"]
    upper = np.triu(np.ones((1, 1, S, S), np.bool_), 1)

    def ops(g, v, p, layer):
        fill = g.const(np.array(-np.inf, np.float32), "fill")
        return g.node("Where", [g.init(p + "upper", upper), fill, _scaled(g, v, p, hd)], name=p + "causal")

    path, _ = _variant(tmp_path, "where_swapped", "gpt_causal", ops)
    for o in _attention_ops(native, path, "bf16"):
        assert o["causal"] is True and o["bias_heads"] == 0, o


def _rejected(native, tmp_path, name, ops, spec="bert_relpos"):
    path, _ = _variant(tmp_path, name, spec, ops)
    r = native.plan_report(path)
    assert not r["supported"]
    return r


def test_rejects_a_row_with_no_visible_key(native, tmp_path):
    from die_amd.models import generic as G

    spec = G.SPECS["bert_relpos"]
    S, hd = spec["seq"], spec["dim"] // spec["heads"]
    m = np.zeros((S, S), np.float32)
    m[7, :] = -np.inf  # softmax of this row is NaN in ONNX

    def ops(g, v, p, layer):
        return g.node("Add", [_scaled(g, v, p, hd), g.init(p + "m", m)], name=p + "dead_row")

    r = _rejected(native, tmp_path, "dead_row", ops)
    items = {i["node"]: i["error"] for i in r["unsupported"]}
    assert "layer0.dead_row" in items, r  # (layer 1 depends on layer 0's output: counted as blocked)
    assert "no visible key" in items["layer0.dead_row"] and "row 7" in items["layer0.dead_row"]


def test_rejects_a_finite_where_fill_that_is_not_a_mask(native, tmp_path):
    from die_amd.models import generic as G

    spec = G.SPECS["gpt_causal"]
    S, hd = spec["seq"], spec["dim"] // spec["heads"]

    def ops(g, v, p, layer):
        tril = g.init(p + "tril", np.tril(np.ones((S, S), np.bool_)))
        return g.node("Where", [tril, _scaled(g, v, p, hd), g.const(np.array(-5.0, np.float32), "fill")],
                      name=p + "soft_fill")

    r = _rejected(native, tmp_path, "soft_fill", ops, spec="gpt_causal")
    items = {i["node"]: i["error"] for i in r["unsupported"]}
    assert "layer0.soft_fill" in items, r
    assert "-1e4" in items["layer0.soft_fill"] or "-10000" in items["layer0.soft_fill"]


def test_rejects_a_table_that_does_not_broadcast(native, tmp_path):
    from die_amd.models import generic as G

    spec = G.SPECS["bert_relpos"]
    S, hd = spec["seq"], spec["dim"] // spec["heads"]

    def ops(g, v, p, layer):
        return g.node("Add", [_scaled(g, v, p, hd), g.init(p + "t", np.zeros((S + 1, S + 1), np.float32))],
                      name=p + "bad_table")

    r = _rejected(native, tmp_path, "bad_table", ops)
    items = {i["node"]: i["error"] for i in r["unsupported"]}
    assert "layer0.bad_table" in items and "broadcast" in items["layer0.bad_table"], r


def test_rejects_a_mask_that_is_not_an_initializer(native, tmp_path):
    """The exporter left the mask as a subgraph (here Cast(int64 initializer)): folding it is out of
    scope, and the Add says so."""
    from die_amd.models import generic as G

    spec = G.SPECS["bert_relpos"]
    S, hd = spec["seq"], spec["dim"] // spec["heads"]

    def ops(g, v, p, layer):
        m = g.node("Cast", [g.init(p + "m_int", np.zeros((S, S), np.int64))], name=p + "mask_cast", to=1)
        return g.node("Add", [_scaled(g, v, p, hd), m], name=p + "computed_mask")

    r = _rejected(native, tmp_path, "computed_mask", ops)
    items = {i["node"]: i["error"] for i in r["unsupported"]}
    assert "layer0.computed_mask" in items, r
    assert "initializer" in items["layer0.computed_mask"]


# ---- the oracle: the CPU executor on these graphs equals a plain torch implementation ------------

def _torch_forward(name, weights, x):
    import torch

    from die_amd.models import generic as G

    spec = G.SPECS[name]
    S, D, H = spec["seq"], spec["dim"], spec["heads"]
    hd = D // H
    w = {k: torch.from_numpy(np.asarray(v)) for k, v in weights.items()}
    pre_ln = name == "gpt_causal"

    def lin(a, n):
        return a @ w[n + ".weight"] + w[n + ".bias"]

    def ln(a, n):
        return torch.nn.functional.layer_norm(a, (D,), w[n + ".weight"], w[n + ".bias"], 1e-5)

    def scores(sc, p):
        if name == "gpt_causal":
            return torch.where(w[p + "causal_mask"], sc / math.sqrt(hd), torch.tensor(-1e4))
        if name == "bert_relpos":
            return sc / math.sqrt(hd) + w[p + "rel_bias"]
        if name == "bert_window":
            return (sc + w[p + "window_mask"]) / math.sqrt(hd)
        return sc / math.sqrt(hd) + w[p + "key_mask"]

    def attention(a, p):
        B = a.shape[0]
        q, k, v = (lin(a, p + n).view(B, S, H, hd).transpose(1, 2) for n in ("query", "key", "value"))
        pr = torch.softmax(scores(q @ k.transpose(-1, -2), p), -1)
        return lin((pr @ v).transpose(1, 2).reshape(B, S, D), p + "attn_out")

    def ffn(a, p):
        return lin(torch.nn.functional.gelu(lin(a, p + "intermediate")), p + "output")

    h = torch.from_numpy(x).view(-1, S, D)
    for i in range(spec["layers"]):
        p = "layer%d." % i
        if pre_ln:
            h = h + attention(ln(h, p + "ln1"), p)
            h = h + ffn(ln(h, p + "ln2"), p)
        else:
            h = ln(attention(h, p) + h, p + "ln1")
            h = ln(ffn(h, p) + h, p + "ln2")
    if pre_ln:
        h = ln(h, "ln_f")
    return (h.mean(1) @ w["classifier.weight"].T + w["classifier.bias"]).numpy()


@pytest.mark.parametrize("name", MASKED)
def test_cpu_executor_matches_torch_on_masked_models(native, masked_models, name):
    from die_amd.models import generic as G

    path, weights = masked_models[name]
    x = G.synthetic_input(name, 3, seed=11)
    got = native.cpu_run(path, x)
    ref = _torch_forward(name, weights, x)
    assert got.shape == ref.shape == (3, 3) and np.isfinite(got).all()
    err = float(np.linalg.norm(got - ref) / np.linalg.norm(ref))
    assert err <= 1e-5, (name, err)


def test_unmasked_plans_carry_no_mask(native, models, tmp_path):
    from die_amd.models import generic as G

    paths = []
    for name in ("bert", "bert_long"):
        p = str(tmp_path / (name + ".onnx"))
        open(p, "wb").write(G.build_onnx(name))
        paths.append(p)
    paths.append(models["get_vit"]("tiny")[0])
    for p in paths:
        for precision in ("fp32", "bf16"):
            att = [o for o in native.plan_summary(p, 8, precision=precision)["ops"] if o["kind"] == "attention"]
            assert att
            for o in att:
                assert o["causal"] is False and o["bias_heads"] == 0, o
                assert "bias_sum" not in o
