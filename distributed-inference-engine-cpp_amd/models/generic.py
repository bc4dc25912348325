"""Generated models for the HIP planner's general path ("model-agnostic device execution").

The reference serves whatever single-input ONNX model it is given (input 0 / output 0,
/root/reference/src/inference_engine.cpp:33-69).  These generators build small models with the op
mix a ResNet / ViT never exercises, random weights, written by the in-tree ONNX writer:

* `mlp`       2-D input [N, F], Gemm (transB) / MatMul layers with Relu / Tanh / Sigmoid / LeakyRelu,
              hidden and output widths that are NOT multiples of 8, Softmax head;
* `bert`      2-D input [N, S*D] reshaped to [N, S, D], post-LN encoder layers (attention in the
              torch export pattern, erf-GELU FFN), mean-pool over tokens, 3-class head;
* `se_cnn`    an image CNN with 12 input channels (> 8), odd channel counts, a squeeze-excitation
              gate (GAP -> FC -> ReLU -> FC -> Sigmoid -> broadcast Mul), channel Concat and
              Slice, and a Flatten of a 4x4 map (NCHW order) into the classifier.
* `ratio_mlp` a Div of two activations of width 10 (stored with 16 channels) feeding a Gemm: the
              pad columns of both operands are 0, so 0/0 must not reach the next GEMM.
* `ops_zoo`   the elementwise / data-movement ops of the wider ONNX op set on an image and on rows:
              Pad folded into a conv, Pad before a MaxPool (a pad pass), HardSwish, channel Split,
              Abs / Neg / Exp / Softplus / HardSigmoid / Max / Min / Pow / Reciprocal / Log / Sqrt /
              Erf, ReduceMax / ReduceSum over the spatial axes, GlobalMaxPool, a rows Split.
* `upsample_net` a decoder-style CNN: ConvTranspose (stride 2, output_padding, 12 output channels),
              Resize nearest (asymmetric / floor, the torch export), Resize linear down (half_pixel)
              and up (align_corners), comparisons of two activations and with constants, Where
              with activation and scalar branches, Not / And / Or, Cast of masks to float.  Every
              mask multiplies a value that is 0 where the mask flips, so bf16 rounding near a
              threshold cannot change the output discontinuously.
* `token_mixer` data-dependent token mixing: MatMul of two activations outside the attention
              pattern (softmax(h W) [S, S] x h [S, D], and x g [S, 20]: inner size 24 and an
              output width that are not multiples of 8).
* `ln_wide`    LayerNormalization over 20 features (stored with 24: pad columns out of the
              statistics) and over 2560 features (wider than the register-resident kernels hold).
* `ln_offset`  pre-norm rows whose LayerNorm input carries a large DC offset (~60 on every channel,
              |mean| / std ~ 60 per row) before the LayerNorm -> MatMul: the case where folding the
              LayerNorm into the GEMM (x.W' - mean * colsum) cancels.
* `bert_long`  the `bert` encoder at 320 tokens: attention past 256 keys (streaming kernel).
* `bert_hd32`, `bert_hd128`  the `bert` encoder with head dim 32 (4 heads of 128 features, 40 tokens)
              and 128 (2 heads of 256 features, 24 tokens).
* `gpt_causal`  pre-LN decoder blocks with the GPT-2 causal mask, Where(tril, scores / sqrt(d), -1e4).
* `bert_relpos` the `bert` encoder with a per-head relative-position table added to the scaled scores.
* `bert_window` a shared band mask (0 inside |i - j| <= 8, -inf outside) added BEFORE the scale, 72
              tokens: from row 41 on the first 32-key tile is entirely masked.
* `bert_keymask` the BERT extended attention mask: Add of [1, 1, 1, S] with -10000 on the last 9 keys.
* `bert_ids`   a token-id model: input [N, 48] of ids (vocab 1000, pad id 0), Gather from the embedding
              table + learned positions, LayerNorm, two `bert` layers whose attention masks the
              request's own padding, Where(Unsqueeze(Equal(ids, 0)), -inf, scores), CLS-token head.
* `bert_ids_hf` the same at 160 tokens (two query blocks, five key tiles) and 4 heads of 32, with a
              token-type row, a per-head relative-position table and the HF extended attention mask
              Add(scores, (1 - Cast(Greater(ids, 0))) * -10000): table and key mask together.
* `sbert_ids`  a sentence embedder: the `bert_ids` body, then the sentence-transformers export -- the
              visibility mask Unsqueeze(-1) -> Expand -> Cast, Mul with the last hidden states, ReduceSum
              over the tokens, divided by the clipped count of visible tokens -- and torch's
              F.normalize (ReduceL2 -> Clip(1e-12) -> Expand -> Div).  Output [N, 128], unit length.
* `sbert_ids_hf` the `bert_ids_hf` body with the mask left unexpanded ([N, S, 1] on the rows, an [N, 1]
              count) and LpNormalization.
* `sbert_cls`  the `bert_ids` body, the CLS token, LpNormalization (no mask in the pooling).
* `bert_hf3`   `bert_ids_hf` as HF exports it: graph inputs input_ids, attention_mask, token_type_ids
              (INT64), a [2, D] type table, mask[:, None, None, :] -> float -> (1 - m) * finfo.min added
              to the scores.  `bert_hf3_maskfirst`: the same at 48 tokens with the inputs declared
              attention_mask, token_type_ids, input_ids.
* `sbert_hf2`  `sbert_ids_hf`'s body with FLOAT inputs input_ids, attention_mask, fill -10000, and the
              sentence-transformers pooling (Unsqueeze(-1) -> Expand -> Cast of attention_mask) +
              F.normalize.  A request of these three is the concatenation of the inputs' [S] in
              declaration order (`synthetic_request`).
* `rope_bert`  the `bert` body (float embeddings in, post-LN, mean pool, 3-class head) with rotary position
              embeddings on Q and K in the HF layout: on [N, H, S, hd] after the head transpose,
              x * cos + Concat(Neg(Slice(x, hd/2:)), Slice(x, :hd/2)) * sin with [1, 1, S, hd] tables from
              theta = 10000.  2 heads of 64, 40 tokens (one full key tile and a partial one).
* `rope_bert_nshd` the same with the rotation on [N, S, H, hd] before the transposes, tables
              [1, S, 1, hd]; 2 heads of 128, 24 tokens.
* `llama_enc`  a token-id embedder shaped like the decoder-derived ones: ids [N, 160] (vocab 1000, pad 0),
              an embedding Gather with no position table, pre-norm blocks with torch's decomposed RMSNorm
              (Pow -> ReduceMean -> Add(eps) -> Sqrt -> Div(1, .) -> Mul -> Mul(weight)), bias-free Q / K / V / O
              projections, RoPE, 4 heads of 32, the ids-derived key mask of `bert_ids_hf`, a SwiGLU MLP
              (Mul(Mul(g, Sigmoid(g)), u) -> down projection), a final RMSNorm and the `sbert_ids_hf`
              masked-mean + LpNormalization tail.  Output [N, 128], unit length.
* `llama_enc_rmsnode` the same body and weights with every RMSNorm written as one RMSNormalization node
              (opset 23).
* `gqa_enc` / `mqa_causal` / `gqa_hd128`  grouped-query attention (K / V projected to fewer heads than Q
              and repeated per group by HF's repeat_kv: Unsqueeze -> Expand -> Reshape) on the `llama_enc`,
              `gpt_causal` and `rope_bert` bodies; see `build_gqa_model`.  expand_kv=True builds the
              multi-head twin from the same weights.
`synthetic_input(model, batch)` gives inputs of the right shape (token-id models: float32 ids in
[1, V), sample i padded with 0 past a length that cycles through 1, 32, S, 45, 33, every third sample
with one interior pad id).  The CPU executor is the fp32
oracle for all of them (tests/test_gpu_general.py).
"""
from __future__ import annotations

import math
from typing import Dict, Tuple

import numpy as np

from ..utils.onnx_writer import GraphBuilder

SPECS = {
    "mlp": dict(in_features=300, hidden=(100, 60, 36), classes=10),
    "bert": dict(seq=32, dim=128, heads=2, ffn=256, layers=2, classes=3),
    "se_cnn": dict(in_ch=12, image=16, classes=10),
    "ratio_mlp": dict(in_features=40, hidden=10, classes=5),
    "ops_zoo": dict(in_ch=8, image=16, classes=10),
    "upsample_net": dict(in_ch=8, image=12, classes=10),
    "token_mixer": dict(seq=24, dim=40, classes=10),
    "ln_wide": dict(seq=6, dim=20, wide=2560, classes=10),
    "ln_offset": dict(seq=64, dim=128, hidden=256, classes=10),
    "bert_long": dict(seq=320, dim=128, heads=2, ffn=256, layers=1, classes=3),
    "bert_hd32": dict(seq=40, dim=128, heads=4, ffn=256, layers=2, classes=3),
    "bert_hd128": dict(seq=24, dim=256, heads=2, ffn=512, layers=2, classes=3),
    "gpt_causal": dict(seq=40, dim=128, heads=2, ffn=256, layers=2, classes=3),
    "bert_relpos": dict(seq=40, dim=128, heads=4, ffn=256, layers=2, classes=3),
    "bert_window": dict(seq=72, dim=128, heads=2, ffn=256, layers=2, classes=3, window=8),
    "bert_keymask": dict(seq=40, dim=128, heads=2, ffn=256, layers=2, classes=3, masked_keys=9),
    "bert_ids": dict(seq=48, dim=128, heads=2, ffn=256, layers=2, classes=3, vocab=1000, pad=0),
    "bert_ids_hf": dict(seq=160, dim=128, heads=4, ffn=256, layers=2, classes=3, vocab=1000, pad=0),
    "sbert_ids": dict(seq=48, dim=128, heads=2, ffn=256, layers=2, vocab=1000, pad=0),
    "sbert_ids_hf": dict(seq=160, dim=128, heads=4, ffn=256, layers=2, vocab=1000, pad=0),
    "sbert_cls": dict(seq=48, dim=128, heads=2, ffn=256, layers=2, vocab=1000, pad=0),
    "bert_hf3": dict(seq=160, dim=128, heads=4, ffn=256, layers=2, classes=3, vocab=1000, pad=0, types=2,
                     inputs=("ids", "mask", "types"), int_input=True, mask_fill="finfo_min"),
    "sbert_hf2": dict(seq=160, dim=128, heads=4, ffn=256, layers=2, vocab=1000, pad=0,
                      inputs=("ids", "mask"), int_input=False, mask_fill=-10000.0),
    "bert_hf3_maskfirst": dict(seq=48, dim=128, heads=4, ffn=256, layers=2, classes=3, vocab=1000, pad=0, types=2,
                               inputs=("mask", "types", "ids"), int_input=True, mask_fill="finfo_min"),
    "rope_bert": dict(seq=40, dim=128, heads=2, ffn=256, layers=2, classes=3, theta=10000.0, layout="nhsd"),
    "rope_bert_nshd": dict(seq=24, dim=256, heads=2, ffn=512, layers=2, classes=3, theta=10000.0, layout="nshd"),
    "llama_enc": dict(seq=160, dim=128, heads=4, ffn=256, layers=2, vocab=1000, pad=0, theta=10000.0, eps=1e-6),
    "llama_enc_rmsnode": dict(seq=160, dim=128, heads=4, ffn=256, layers=2, vocab=1000, pad=0, theta=10000.0, eps=1e-6),
    "gqa_enc": dict(seq=160, dim=256, heads=4, kv_heads=2, ffn=512, layers=2, vocab=1000, pad=0, theta=10000.0, eps=1e-6,
                    body="llama"),
    "mqa_causal": dict(seq=72, dim=256, heads=4, kv_heads=1, ffn=512, layers=2, classes=3, body="gpt"),
    "gqa_hd128": dict(seq=40, dim=768, heads=6, kv_heads=2, ffn=512, layers=1, classes=3, theta=10000.0, body="rope_bert"),
}

MASKED = ("gpt_causal", "bert_relpos", "bert_window", "bert_keymask")
MULTI_INPUT = ("bert_hf3", "sbert_hf2", "bert_hf3_maskfirst")  # input_ids + attention_mask [+ token_type_ids]
ROPE_BERT = ("rope_bert", "rope_bert_nshd")
LLAMA = ("llama_enc", "llama_enc_rmsnode")
GQA = ("gqa_enc", "mqa_causal", "gqa_hd128")  # K / V with fewer heads than Q (build_gqa_model)
TOKEN_IDS = ("bert_ids", "bert_ids_hf", "sbert_ids", "sbert_ids_hf", "sbert_cls") + MULTI_INPUT + LLAMA + ("gqa_enc",)
INPUT_NAMES = {"ids": "input_ids", "mask": "attention_mask", "types": "token_type_ids"}


def _rng(seed):
    return np.random.default_rng(seed)


def _lin(rng, fan_in, shape):
    return (rng.standard_normal(shape) / math.sqrt(fan_in)).astype(np.float32)


def build_mlp(seed: int = 0, opset: int = 13) -> Tuple[bytes, Dict[str, np.ndarray]]:
    s = SPECS["mlp"]
    rng = _rng(seed)
    g = GraphBuilder(name="mlp")
    x = g.input("features", ["N", s["in_features"]])
    h, fan = x, s["in_features"]
    acts = ["Relu", "Tanh", "LeakyRelu"]
    for i, width in enumerate(s["hidden"]):
        if i % 2 == 0:  # Gemm with transB (torch nn.Linear export)
            w = g.init("fc%d.weight" % i, _lin(rng, fan, (width, fan)))
            b = g.init("fc%d.bias" % i, (0.1 * rng.standard_normal(width)).astype(np.float32))
            h = g.node("Gemm", [h, w, b], name="fc%d" % i, transB=1)
        else:  # MatMul + Add (the other common export)
            w = g.init("fc%d.weight" % i, _lin(rng, fan, (fan, width)))
            b = g.init("fc%d.bias" % i, (0.1 * rng.standard_normal(width)).astype(np.float32))
            h = g.node("Add", [g.node("MatMul", [h, w], name="fc%d/MatMul" % i), b], name="fc%d/Add" % i)
        a = acts[i % len(acts)]
        h = g.node(a, [h], name="act%d" % i, **({"alpha": 0.1} if a == "LeakyRelu" else {}))
        fan = width
    # a sigmoid gate on the last hidden layer, then the classifier
    gate = g.node("Sigmoid", [h], name="gate")
    h = g.node("Mul", [h, gate], name="gated")
    w = g.init("head.weight", _lin(rng, fan, (s["classes"], fan)))
    b = g.init("head.bias", (0.1 * rng.standard_normal(s["classes"])).astype(np.float32))
    y = g.node("Gemm", [h, w, b], name="head", transB=1)
    y = g.node("Softmax", [y], name="prob", axis=-1)
    g.output(y, ["N", s["classes"]])
    return g.model_proto(opset=opset), {}


def build_bert(seed: int = 0, opset: int = 17, spec: str = "bert") -> Tuple[bytes, Dict[str, np.ndarray]]:
    s = SPECS[spec]
    rng = _rng(seed)
    S, D, H, F = s["seq"], s["dim"], s["heads"], s["ffn"]
    hd = D // H
    g = GraphBuilder(name="bert_encoder")
    x = g.input("embeddings", ["N", S * D])  # token embeddings, flattened (2-D input)
    h = g.node("Reshape", [x, g.const(np.array([0, S, D], np.int64), "seq_shape")], name="to_tokens")
    heads_shape = g.const(np.array([0, 0, H, hd], np.int64), "heads_shape")
    merge_shape = g.const(np.array([0, 0, D], np.int64), "merge_shape")
    scale = g.const(np.array(math.sqrt(hd), np.float32), "sqrt_d")
    sqrt2 = g.const(np.array(1.4142135381698608, np.float32), "sqrt2")
    one = g.const(np.array(1.0, np.float32), "one")
    half = g.const(np.array(0.5, np.float32), "half")

    def linear(inp, name, fin, fout):
        w = g.init(name + ".weight", _lin(rng, fin, (fin, fout)))
        b = g.init(name + ".bias", (0.02 * rng.standard_normal(fout)).astype(np.float32))
        return g.node("Add", [g.node("MatMul", [inp, w], name=name + "/MatMul"), b], name=name + "/Add")

    def ln(inp, name):
        gw = g.init(name + ".weight", (1.0 + 0.1 * rng.standard_normal(D)).astype(np.float32))
        gb = g.init(name + ".bias", (0.1 * rng.standard_normal(D)).astype(np.float32))
        return g.node("LayerNormalization", [inp, gw, gb], name=name, axis=-1, epsilon=1e-12)

    for i in range(s["layers"]):
        p = "layer%d." % i
        q = linear(h, p + "query", D, D)
        k = linear(h, p + "key", D, D)
        v = linear(h, p + "value", D, D)
        q = g.node("Transpose", [g.node("Reshape", [q, heads_shape], name=p + "q_heads")], name=p + "q_perm",
                   perm=[0, 2, 1, 3])
        k = g.node("Transpose", [g.node("Reshape", [k, heads_shape], name=p + "k_heads")], name=p + "k_perm",
                   perm=[0, 2, 3, 1])
        v = g.node("Transpose", [g.node("Reshape", [v, heads_shape], name=p + "v_heads")], name=p + "v_perm",
                   perm=[0, 2, 1, 3])
        sc = g.node("Div", [g.node("MatMul", [q, k], name=p + "scores"), scale], name=p + "scale")
        sc = g.node("Softmax", [sc], name=p + "softmax", axis=-1)
        c = g.node("MatMul", [sc, v], name=p + "context")
        c = g.node("Reshape", [g.node("Transpose", [c], name=p + "ctx_perm", perm=[0, 2, 1, 3]), merge_shape],
                   name=p + "ctx_merge")
        o = linear(c, p + "attn_out", D, D)
        h = ln(g.node("Add", [o, h], name=p + "residual1"), p + "ln1")  # post-LN (BERT)
        m = linear(h, p + "intermediate", D, F)
        t = g.node("Div", [m, sqrt2], name=p + "gelu/div")
        t = g.node("Add", [g.node("Erf", [t], name=p + "gelu/erf"), one], name=p + "gelu/add")
        t = g.node("Mul", [g.node("Mul", [m, t], name=p + "gelu/mul"), half], name=p + "gelu/half")
        o = linear(t, p + "output", F, D)
        h = ln(g.node("Add", [o, h], name=p + "residual2"), p + "ln2")
    pooled = g.node("ReduceMean", [h], name="mean_pool", axes=[1], keepdims=0)
    w = g.init("classifier.weight", _lin(rng, D, (s["classes"], D)))
    b = g.init("classifier.bias", (0.1 * rng.standard_normal(s["classes"])).astype(np.float32))
    y = g.node("Gemm", [pooled, w, b], name="classifier", transB=1)
    g.output(y, ["N", s["classes"]])
    return g.model_proto(opset=opset), {}


def masked_score_ops(spec: str, seed: int = 0):
    """The nodes between Q K^T and the Softmax of the masked-attention models: a function
    (g, scores, prefix, layer) -> value.  All masks / tables are initializers."""
    s = SPECS[spec]
    S, H, hd = s["seq"], s["heads"], s["dim"] // s["heads"]
    rng = _rng(seed + 1000)

    def scale(g, v, p):
        return g.node("Div", [v, g.const(np.array(math.sqrt(hd), np.float32), "sqrt_d")], name=p + "scale")

    if spec == "gpt_causal":  # GPT-2 export: Where(tril, scores / sqrt(d), -1e4)
        def ops(g, v, p, layer):
            tril = g.init(p + "causal_mask", np.tril(np.ones((1, 1, S, S), np.bool_)))
            fill = g.const(np.array(-1e4, np.float32), "mask_fill")
            return g.node("Where", [tril, scale(g, v, p), fill], name=p + "causal")
    elif spec == "bert_relpos":  # learned relative-position bias per head, after the scale
        def ops(g, v, p, layer):
            table = g.init(p + "rel_bias", rng.standard_normal((1, H, S, S)).astype(np.float32))
            return g.node("Add", [scale(g, v, p), table], name=p + "rel_bias/Add")
    elif spec == "bert_window":  # shared band mask added BEFORE the scale
        def ops(g, v, p, layer):
            i = np.arange(S)
            band = np.where(np.abs(i[:, None] - i[None, :]) <= s["window"], 0.0, -np.inf).astype(np.float32)
            return scale(g, g.node("Add", [v, g.init(p + "window_mask", band)], name=p + "window"), p)
    elif spec == "bert_keymask":  # BERT extended attention mask: -10000 on the padded keys
        def ops(g, v, p, layer):
            m = np.zeros((1, 1, 1, S), np.float32)
            m[..., S - s["masked_keys"]:] = -10000.0
            return g.node("Add", [scale(g, v, p), g.init(p + "key_mask", m)], name=p + "key_mask/Add")
    else:
        raise KeyError(spec)
    return ops


def build_masked_encoder(seed: int = 0, opset: int = 17, spec: str = "bert_relpos", score_ops=None,
                         pre_ln=None) -> Tuple[bytes, Dict[str, np.ndarray]]:
    """Encoder / decoder stacks whose attention has a constant additive bias or mask between Q K^T and
    the Softmax (`gpt_causal`, `bert_relpos`, `bert_window`, `bert_keymask`).  score_ops overrides
    the nodes of that stretch (tests build further variants on the same stack); pre_ln: GPT-style
    pre-LayerNorm blocks (default: for `gpt_causal`), else the `bert` post-LN blocks."""
    s = SPECS[spec]
    rng = _rng(seed)
    S, D, H, F = s["seq"], s["dim"], s["heads"], s["ffn"]
    hd = D // H
    if score_ops is None:
        score_ops = masked_score_ops(spec, seed)
    if pre_ln is None:
        pre_ln = spec == "gpt_causal"
    g = GraphBuilder(name=spec)
    x = g.input("embeddings", ["N", S * D])
    h = g.node("Reshape", [x, g.const(np.array([0, S, D], np.int64), "seq_shape")], name="to_tokens")
    heads_shape = g.const(np.array([0, 0, H, hd], np.int64), "heads_shape")
    merge_shape = g.const(np.array([0, 0, D], np.int64), "merge_shape")
    sqrt2 = g.const(np.array(1.4142135381698608, np.float32), "sqrt2")
    one = g.const(np.array(1.0, np.float32), "one")
    half = g.const(np.array(0.5, np.float32), "half")

    def linear(inp, name, fin, fout):
        w = g.init(name + ".weight", _lin(rng, fin, (fin, fout)))
        b = g.init(name + ".bias", (0.02 * rng.standard_normal(fout)).astype(np.float32))
        return g.node("Add", [g.node("MatMul", [inp, w], name=name + "/MatMul"), b], name=name + "/Add")

    def ln(inp, name):
        gw = g.init(name + ".weight", (1.0 + 0.1 * rng.standard_normal(D)).astype(np.float32))
        gb = g.init(name + ".bias", (0.1 * rng.standard_normal(D)).astype(np.float32))
        return g.node("LayerNormalization", [inp, gw, gb], name=name, axis=-1, epsilon=1e-5)

    def attention(a, p, layer):
        q = linear(a, p + "query", D, D)
        k = linear(a, p + "key", D, D)
        v = linear(a, p + "value", D, D)
        q = g.node("Transpose", [g.node("Reshape", [q, heads_shape], name=p + "q_heads")], name=p + "q_perm",
                   perm=[0, 2, 1, 3])
        k = g.node("Transpose", [g.node("Reshape", [k, heads_shape], name=p + "k_heads")], name=p + "k_perm",
                   perm=[0, 2, 3, 1])
        v = g.node("Transpose", [g.node("Reshape", [v, heads_shape], name=p + "v_heads")], name=p + "v_perm",
                   perm=[0, 2, 1, 3])
        sc = score_ops(g, g.node("MatMul", [q, k], name=p + "scores"), p, layer)
        sc = g.node("Softmax", [sc], name=p + "softmax", axis=-1)
        c = g.node("MatMul", [sc, v], name=p + "context")
        c = g.node("Reshape", [g.node("Transpose", [c], name=p + "ctx_perm", perm=[0, 2, 1, 3]), merge_shape],
                   name=p + "ctx_merge")
        return linear(c, p + "attn_out", D, D)

    def ffn(a, p):
        m = linear(a, p + "intermediate", D, F)
        t = g.node("Div", [m, sqrt2], name=p + "gelu/div")
        t = g.node("Add", [g.node("Erf", [t], name=p + "gelu/erf"), one], name=p + "gelu/add")
        t = g.node("Mul", [g.node("Mul", [m, t], name=p + "gelu/mul"), half], name=p + "gelu/half")
        return linear(t, p + "output", F, D)

    for i in range(s["layers"]):
        p = "layer%d." % i
        if pre_ln:  # GPT: x + attn(ln(x)), x + ffn(ln(x))
            h = g.node("Add", [attention(ln(h, p + "ln1"), p, i), h], name=p + "residual1")
            h = g.node("Add", [ffn(ln(h, p + "ln2"), p), h], name=p + "residual2")
        else:
            h = ln(g.node("Add", [attention(h, p, i), h], name=p + "residual1"), p + "ln1")
            h = ln(g.node("Add", [ffn(h, p), h], name=p + "residual2"), p + "ln2")
    if pre_ln:
        h = ln(h, "ln_f")
    pooled = g.node("ReduceMean", [h], name="mean_pool", axes=[1], keepdims=0)
    w = g.init("classifier.weight", _lin(rng, D, (s["classes"], D)))
    b = g.init("classifier.bias", (0.1 * rng.standard_normal(s["classes"])).astype(np.float32))
    y = g.node("Gemm", [pooled, w, b], name="classifier", transB=1)
    g.output(y, ["N", s["classes"]])
    return g.model_proto(opset=opset), dict(g.initializers)


def build_token_encoder(seed: int = 0, opset: int = 17, spec: str = "bert_ids", int_input=None,
                        inputs=None) -> Tuple[bytes, Dict[str, np.ndarray]]:
    """Token-id encoders (`bert_ids`, `bert_ids_hf`): the graph input is [N, S] token ids carried as
    numbers (declared FLOAT, or INT64 with int_input), embedded by a Gather, and the attention mask
    is computed from the ids themselves (pad id 0).  The sentence embedders (`sbert_ids`,
    `sbert_ids_hf`, `sbert_cls`) end in a pooled, L2-normalised vector [N, D] instead of the CLS
    classifier.
    inputs: the graph inputs in declaration order, out of "ids", "mask", "types" (default: the spec's,
    ("ids",) for the single-input specs).  With "mask" the attention mask (and the pooling mask of an
    embedder) comes from an attention_mask input instead of the ids; with "types" the token-type
    embedding is a lookup of a token_type_ids input in a [T, D] table.  The HF-style specs build
    either way from the same weights (`bert_hf3` / `sbert_hf2` / `bert_hf3_maskfirst` with
    inputs=("ids",) are the single-input twins: row 0 of the type table is their type row), so a
    multi-input model fed mask = ids > 0, types = 0 computes what its twin computes.
    Returns (model bytes, initializers)."""
    from ..utils.onnx_writer import INT64

    s = SPECS[spec]
    rng = _rng(seed)
    S, D, H, F, V = s["seq"], s["dim"], s["heads"], s["ffn"], s["vocab"]
    hd = D // H
    hf = spec in ("bert_ids_hf", "sbert_ids_hf") + MULTI_INPUT
    inputs = tuple(inputs if inputs is not None else s.get("inputs", ("ids",)))
    if int_input is None:
        int_input = s.get("int_input", False)
    if "ids" not in inputs or (len(inputs) > 1 and not hf):
        raise ValueError("inputs %r: ids are required, mask / types inputs only on the HF-style specs" % (inputs,))
    g = GraphBuilder(name=spec)
    ins = {r: (g.input(INPUT_NAMES[r], ["N", S], elem_type=INT64) if int_input else g.input(INPUT_NAMES[r], ["N", S]))
           for r in inputs}
    x = ins["ids"]
    ids = x if int_input else g.node("Cast", [x], name="ids_int", to=INT64)
    table = g.init("embeddings.word", (0.5 * rng.standard_normal((V, D))).astype(np.float32))
    h = g.node("Gather", [table, ids], name="embeddings.lookup", axis=0)
    h = g.node("Add", [h, g.init("embeddings.position", (0.5 * rng.standard_normal((1, S, D))).astype(np.float32))],
               name="embeddings.add_position")
    if hf:
        type_row = (0.5 * rng.standard_normal(D)).astype(np.float32)
        if "types" in inputs:  # row 0 = the single-input twin's type row; the others from a stream of their own
            more = (0.5 * _rng(seed + 5000).standard_normal((s.get("types", 2) - 1, D))).astype(np.float32)
            ttab = g.init("embeddings.token_type", np.concatenate([type_row[None, :], more], axis=0))
            tids = ins["types"] if int_input else g.node("Cast", [ins["types"]], name="types_int", to=INT64)
            h = g.node("Add", [h, g.node("Gather", [ttab, tids], name="embeddings.type_lookup", axis=0)],
                       name="embeddings.add_type")
        else:
            h = g.node("Add", [h, g.init("embeddings.token_type", type_row)], name="embeddings.add_type")
    heads_shape = g.const(np.array([0, 0, H, hd], np.int64), "heads_shape")
    merge_shape = g.const(np.array([0, 0, D], np.int64), "merge_shape")
    sqrt2 = g.const(np.array(1.4142135381698608, np.float32), "sqrt2")
    one = g.const(np.array(1.0, np.float32), "one")
    half = g.const(np.array(0.5, np.float32), "half")
    axes12 = g.const(np.array([1, 2], np.int64), "mask_axes")
    fill = s.get("mask_fill", -10000.0)
    fill = float(np.finfo(np.float32).min) if fill == "finfo_min" else fill
    mask_in = ins.get("mask")
    if mask_in is not None and int_input:
        # current HF exports: mask[:, None, None, :] -> to float -> (1 - m) * finfo.min
        m = g.node("Unsqueeze", [g.node("Unsqueeze", [mask_in, g.const(np.array([1], np.int64), "mask_axis1")],
                                        name="mask_unsqueeze1"), g.const(np.array([2], np.int64), "mask_axis2")],
                   name="extended_mask")
        m = g.node("Cast", [m], name="extended_mask_f", to=1)
        key_term = g.node("Mul", [g.node("Sub", [one, m], name="inverted_mask"),
                                  g.const(np.array(fill, np.float32), "mask_value")], name="additive_mask")
    elif mask_in is not None:  # a float mask input: no Cast
        m = g.node("Unsqueeze", [mask_in, axes12], name="extended_mask")
        key_term = g.node("Mul", [g.node("Sub", [one, m], name="inverted_mask"),
                                  g.const(np.array(fill, np.float32), "mask_value")], name="additive_mask")
    elif hf:  # HF: extended = (1 - mask[:, None, None, :]) * -10000, mask = ids > 0, from the float input
        mask_f = g.node("Cast", [g.node("Greater", [x, g.const(np.array(0, np.int64 if int_input else np.float32), "pad_id")],
                                        name="attention_mask")], name="attention_mask_f", to=1)
        m = g.node("Unsqueeze", [mask_f, axes12], name="extended_mask")
        key_term = g.node("Mul", [g.node("Sub", [one, m], name="inverted_mask"),
                                  g.const(np.array(-10000.0, np.float32), "mask_value")], name="additive_mask")
    else:  # hidden = ids == pad on the integer ids
        is_pad = g.node("Equal", [ids, g.const(np.array(s["pad"], np.int64), "pad_id")], name="is_pad")
        hidden = g.node("Unsqueeze", [is_pad, axes12], name="pad_mask")
        fill = g.const(np.array(-np.inf, np.float32), "mask_fill")

    def linear(inp, name, fin, fout):
        w = g.init(name + ".weight", _lin(rng, fin, (fin, fout)))
        b = g.init(name + ".bias", (0.02 * rng.standard_normal(fout)).astype(np.float32))
        return g.node("Add", [g.node("MatMul", [inp, w], name=name + "/MatMul"), b], name=name + "/Add")

    def ln(inp, name):
        gw = g.init(name + ".weight", (1.0 + 0.1 * rng.standard_normal(D)).astype(np.float32))
        gb = g.init(name + ".bias", (0.1 * rng.standard_normal(D)).astype(np.float32))
        return g.node("LayerNormalization", [inp, gw, gb], name=name, axis=-1, epsilon=1e-5)

    h = ln(h, "embeddings.ln")
    for i in range(s["layers"]):
        p = "layer%d." % i
        q = linear(h, p + "query", D, D)
        k = linear(h, p + "key", D, D)
        v = linear(h, p + "value", D, D)
        q = g.node("Transpose", [g.node("Reshape", [q, heads_shape], name=p + "q_heads")], name=p + "q_perm",
                   perm=[0, 2, 1, 3])
        k = g.node("Transpose", [g.node("Reshape", [k, heads_shape], name=p + "k_heads")], name=p + "k_perm",
                   perm=[0, 2, 3, 1])
        v = g.node("Transpose", [g.node("Reshape", [v, heads_shape], name=p + "v_heads")], name=p + "v_perm",
                   perm=[0, 2, 1, 3])
        sc = g.node("Div", [g.node("MatMul", [q, k], name=p + "scores"),
                            g.const(np.array(math.sqrt(hd), np.float32), "sqrt_d")], name=p + "scale")
        if hf:
            rel = g.init(p + "rel_bias", rng.standard_normal((1, H, S, S)).astype(np.float32))
            sc = g.node("Add", [g.node("Add", [sc, rel], name=p + "rel_bias/Add"), key_term], name=p + "mask/Add")
        else:
            sc = g.node("Where", [hidden, fill, sc], name=p + "mask")
        sc = g.node("Softmax", [sc], name=p + "softmax", axis=-1)
        c = g.node("MatMul", [sc, v], name=p + "context")
        c = g.node("Reshape", [g.node("Transpose", [c], name=p + "ctx_perm", perm=[0, 2, 1, 3]), merge_shape],
                   name=p + "ctx_merge")
        h = ln(g.node("Add", [linear(c, p + "attn_out", D, D), h], name=p + "residual1"), p + "ln1")
        m1 = linear(h, p + "intermediate", D, F)
        t = g.node("Div", [m1, sqrt2], name=p + "gelu/div")
        t = g.node("Add", [g.node("Erf", [t], name=p + "gelu/erf"), one], name=p + "gelu/add")
        t = g.node("Mul", [g.node("Mul", [m1, t], name=p + "gelu/mul"), half], name=p + "gelu/half")
        h = ln(g.node("Add", [linear(t, p + "output", F, D), h], name=p + "residual2"), p + "ln2")
    if spec.startswith("sbert"):
        y = _sentence_head(g, spec, h, None if hf else is_pad, mask_f if hf and mask_in is None else None, mask_in)
        g.output(y, ["N", D])
        return g.model_proto(opset=opset), dict(g.initializers)
    cls = g.node("Gather", [h, g.const(np.array(0, np.int64), "cls_index")], name="cls_token", axis=1)
    w = g.init("classifier.weight", _lin(rng, D, (s["classes"], D)))
    b = g.init("classifier.bias", (0.1 * rng.standard_normal(s["classes"])).astype(np.float32))
    y = g.node("Gemm", [cls, w, b], name="classifier", transB=1)
    g.output(y, ["N", s["classes"]])
    return g.model_proto(opset=opset), dict(g.initializers)


def _sentence_head(g, spec, h, is_pad, mask_f, mask_in=None):
    """The pooling + normalisation tail of the sentence embedders on the last hidden states h [N, S, D].
    mask_in: the attention_mask graph input, which then is the visibility value of the
    sentence-transformers form."""
    last = g.const(np.array([-1], np.int64), "last_axis")
    tokens = g.const(np.array([1], np.int64), "token_axis")
    if spec == "sbert_cls":  # the CLS token, LpNormalization
        cls = g.node("Gather", [h, g.const(np.array(0, np.int64), "cls_index")], name="cls_token", axis=1)
        return g.node("LpNormalization", [cls], name="normalize", axis=-1, p=2)
    if mask_in is None and mask_f is not None:  # (`sbert_ids_hf`) the mask stays [N, S, 1] on the rows; an [N, 1] count; LpNormalization
        summed = g.node("ReduceSum", [g.node("Mul", [h, g.node("Unsqueeze", [mask_f, last], name="pool_mask")],
                                             name="masked_states"), tokens], name="masked_sum", keepdims=0)
        count = g.node("Clip", [g.node("ReduceSum", [mask_f, tokens], name="visible_count", keepdims=1),
                                g.const(np.array(1e-9, np.float32), "count_min")], name="count_clamp")
        return g.node("LpNormalization", [g.node("Div", [summed, count], name="mean_pool")], name="normalize", axis=1, p=2)
    # sentence-transformers: mask.unsqueeze(-1).expand(h.size()).float(); sum(h * m, 1) / clamp(m.sum(1), 1e-9);
    # then F.normalize(p=2, dim=1): x / clamp(norm(x), 1e-12).expand_as(x)
    vis = mask_in if mask_in is not None else g.node("Not", [is_pad], name="visible")
    m = g.node("Expand", [g.node("Unsqueeze", [vis, last], name="pool_mask"), g.node("Shape", [h], name="states_shape")],
               name="pool_mask_expanded")
    m = g.node("Cast", [m], name="pool_mask_f", to=1)
    summed = g.node("ReduceSum", [g.node("Mul", [h, m], name="masked_states"), tokens], name="masked_sum", keepdims=0)
    count = g.node("Clip", [g.node("ReduceSum", [m, tokens], name="visible_count", keepdims=0),
                            g.const(np.array(1e-9, np.float32), "count_min")], name="count_clamp")
    pooled = g.node("Div", [summed, count], name="mean_pool")
    norm = g.node("Clip", [g.node("ReduceL2", [pooled], name="norm", axes=[-1], keepdims=1),
                           g.const(np.array(1e-12, np.float32), "norm_eps")], name="norm_clamp")
    norm = g.node("Expand", [norm, g.node("Shape", [pooled], name="pooled_shape")], name="norm_expanded")
    return g.node("Div", [pooled, norm], name="normalize")


def rope_tables(S: int, hd: int, theta: float = 10000.0):
    """The rotary tables (cos, sin), float32 [S, hd]: angle[s, j] = s * theta^(-2 (j mod hd/2) / hd), both
    halves stored (the HF cache layout, emb = cat(freqs, freqs))."""
    inv = theta ** (-np.arange(0, hd, 2, dtype=np.float64) / hd)
    ang = np.arange(S, dtype=np.float64)[:, None] * inv[None, :]
    emb = np.concatenate([ang, ang], axis=1)
    return np.cos(emb).astype(np.float32), np.sin(emb).astype(np.float32)


def rope_nodes(g, x, cos, sin, hd, p, axis=-1, open_end=False, swap=False):
    """torch's apply_rotary_pos_emb export on the heads view x (last axis hd): x * cos + rotate_half(x) * sin.
    axis: the Slice / Concat axis as written (-1 or 3); open_end: the high half ends at INT64_MAX (the
    x[..., hd/2:] export); swap: the operand order of the commutative nodes reversed."""
    i64 = lambda v, n: g.const(np.array([v], np.int64), n)
    h2 = hd // 2
    ax, one = i64(axis, "rope_axis"), i64(1, "rope_step")
    lo = g.node("Slice", [x, i64(0, "rope_zero"), i64(h2, "rope_half"), ax, one], name=p + "rope/lo")
    hi = g.node("Slice", [x, i64(h2, "rope_half"), i64(np.iinfo(np.int64).max if open_end else hd, "rope_end"), ax, one],
                name=p + "rope/hi")
    rot = g.node("Concat", [g.node("Neg", [hi], name=p + "rope/neg"), lo], name=p + "rope/rotate_half", axis=axis)
    a = g.node("Mul", [cos, x] if swap else [x, cos], name=p + "rope/cos")
    b = g.node("Mul", [sin, rot] if swap else [rot, sin], name=p + "rope/sin")
    return g.node("Add", [b, a] if swap else [a, b], name=p + "rope/add")


def build_rope_encoder(seed: int = 0, opset: int = 17, spec: str = "rope_bert") -> Tuple[bytes, Dict[str, np.ndarray]]:
    """`rope_bert` / `rope_bert_nshd`: the `bert` post-LN encoder with rotary position embeddings on Q
    and K.  Returns (model bytes, initializers)."""
    s = SPECS[spec]
    rng = _rng(seed)
    S, D, H, F = s["seq"], s["dim"], s["heads"], s["ffn"]
    hd = D // H
    nshd = s["layout"] == "nshd"
    g = GraphBuilder(name=spec)
    x = g.input("embeddings", ["N", S * D])
    h = g.node("Reshape", [x, g.const(np.array([0, S, D], np.int64), "seq_shape")], name="to_tokens")
    heads_shape = g.const(np.array([0, 0, H, hd], np.int64), "heads_shape")
    merge_shape = g.const(np.array([0, 0, D], np.int64), "merge_shape")
    sqrt2 = g.const(np.array(1.4142135381698608, np.float32), "sqrt2")
    one = g.const(np.array(1.0, np.float32), "one")
    half = g.const(np.array(0.5, np.float32), "half")
    c, sn = rope_tables(S, hd, s["theta"])
    tshape = (1, S, 1, hd) if nshd else (1, 1, S, hd)
    cos, sin = g.init("rope.cos", c.reshape(tshape)), g.init("rope.sin", sn.reshape(tshape))

    def linear(inp, name, fin, fout):
        w = g.init(name + ".weight", _lin(rng, fin, (fin, fout)))
        b = g.init(name + ".bias", (0.02 * rng.standard_normal(fout)).astype(np.float32))
        return g.node("Add", [g.node("MatMul", [inp, w], name=name + "/MatMul"), b], name=name + "/Add")

    def ln(inp, name):
        gw = g.init(name + ".weight", (1.0 + 0.1 * rng.standard_normal(D)).astype(np.float32))
        gb = g.init(name + ".bias", (0.1 * rng.standard_normal(D)).astype(np.float32))
        return g.node("LayerNormalization", [inp, gw, gb], name=name, axis=-1, epsilon=1e-5)

    for i in range(s["layers"]):
        p = "layer%d." % i
        q = g.node("Reshape", [linear(h, p + "query", D, D), heads_shape], name=p + "q_heads")
        k = g.node("Reshape", [linear(h, p + "key", D, D), heads_shape], name=p + "k_heads")
        v = g.node("Reshape", [linear(h, p + "value", D, D), heads_shape], name=p + "v_heads")
        if nshd:  # rotate [N, S, H, hd], then transpose
            q = g.node("Transpose", [rope_nodes(g, q, cos, sin, hd, p + "q_", axis=3, open_end=True)], name=p + "q_perm",
                       perm=[0, 2, 1, 3])
            k = g.node("Transpose", [rope_nodes(g, k, cos, sin, hd, p + "k_", axis=3, swap=True)], name=p + "k_perm",
                       perm=[0, 2, 3, 1])
        else:  # HF: transpose to [N, H, S, hd], rotate, K transposed again for Q K^T
            q = rope_nodes(g, g.node("Transpose", [q], name=p + "q_perm", perm=[0, 2, 1, 3]), cos, sin, hd, p + "q_")
            k = rope_nodes(g, g.node("Transpose", [k], name=p + "k_perm", perm=[0, 2, 1, 3]), cos, sin, hd, p + "k_",
                           open_end=True, swap=True)
            k = g.node("Transpose", [k], name=p + "k_t", perm=[0, 1, 3, 2])
        v = g.node("Transpose", [v], name=p + "v_perm", perm=[0, 2, 1, 3])
        sc = g.node("Div", [g.node("MatMul", [q, k], name=p + "scores"),
                            g.const(np.array(math.sqrt(hd), np.float32), "sqrt_d")], name=p + "scale")
        sc = g.node("Softmax", [sc], name=p + "softmax", axis=-1)
        ctx = g.node("MatMul", [sc, v], name=p + "context")
        ctx = g.node("Reshape", [g.node("Transpose", [ctx], name=p + "ctx_perm", perm=[0, 2, 1, 3]), merge_shape],
                     name=p + "ctx_merge")
        h = ln(g.node("Add", [linear(ctx, p + "attn_out", D, D), h], name=p + "residual1"), p + "ln1")
        m = linear(h, p + "intermediate", D, F)
        t = g.node("Div", [m, sqrt2], name=p + "gelu/div")
        t = g.node("Add", [g.node("Erf", [t], name=p + "gelu/erf"), one], name=p + "gelu/add")
        t = g.node("Mul", [g.node("Mul", [m, t], name=p + "gelu/mul"), half], name=p + "gelu/half")
        h = ln(g.node("Add", [linear(t, p + "output", F, D), h], name=p + "residual2"), p + "ln2")
    pooled = g.node("ReduceMean", [h], name="mean_pool", axes=[1], keepdims=0)
    w = g.init("classifier.weight", _lin(rng, D, (s["classes"], D)))
    b = g.init("classifier.bias", (0.1 * rng.standard_normal(s["classes"])).astype(np.float32))
    y = g.node("Gemm", [pooled, w, b], name="classifier", transB=1)
    g.output(y, ["N", s["classes"]])
    return g.model_proto(opset=opset), dict(g.initializers)


def build_llama_encoder(seed: int = 0, opset: int = 17, spec: str = "llama_enc") -> Tuple[bytes, Dict[str, np.ndarray]]:
    """`llama_enc` / `llama_enc_rmsnode`: a decoder-derived token-id embedder (RMSNorm, RoPE, bias-free
    projections, SwiGLU, masked mean + L2 normalisation).  Both specs draw the same weights; the
    second writes each RMSNorm as one RMSNormalization node and needs opset 23.
    Returns (model bytes, initializers)."""
    from ..utils.onnx_writer import INT64

    s = SPECS[spec]
    rng = _rng(seed)
    S, D, H, F, V = s["seq"], s["dim"], s["heads"], s["ffn"], s["vocab"]
    hd = D // H
    node_form = spec == "llama_enc_rmsnode"
    if node_form:
        opset = max(opset, 23)
    g = GraphBuilder(name=spec)
    x = g.input("input_ids", ["N", S])
    ids = g.node("Cast", [x], name="ids_int", to=INT64)
    table = g.init("embed_tokens.weight", (0.5 * rng.standard_normal((V, D))).astype(np.float32))
    h = g.node("Gather", [table, ids], name="embed_tokens", axis=0)
    heads_shape = g.const(np.array([0, 0, H, hd], np.int64), "heads_shape")
    merge_shape = g.const(np.array([0, 0, D], np.int64), "merge_shape")
    one = g.const(np.array(1.0, np.float32), "one")
    two = g.const(np.array(2.0, np.float32), "two")
    eps = g.const(np.array(s["eps"], np.float32), "rms_eps")
    last = g.const(np.array([-1], np.int64), "rms_axis")
    c, sn = rope_tables(S, hd, s["theta"])
    cos, sin = g.init("rope.cos", c.reshape(1, 1, S, hd)), g.init("rope.sin", sn.reshape(1, 1, S, hd))
    # HF: extended = (1 - mask[:, None, None, :]) * -10000 with mask = ids > 0
    mask_f = g.node("Cast", [g.node("Greater", [x, g.const(np.array(0, np.float32), "pad_id")], name="attention_mask")],
                    name="attention_mask_f", to=1)
    m = g.node("Unsqueeze", [mask_f, g.const(np.array([1, 2], np.int64), "mask_axes")], name="extended_mask")
    key_term = g.node("Mul", [g.node("Sub", [one, m], name="inverted_mask"),
                              g.const(np.array(-10000.0, np.float32), "mask_value")], name="additive_mask")

    def proj(inp, name, fin, fout):
        return g.node("MatMul", [inp, g.init(name + ".weight", _lin(rng, fin, (fin, fout)))], name=name)

    def rms(inp, name):
        w = g.init(name + ".weight", (1.0 + 0.1 * rng.standard_normal(D)).astype(np.float32))
        if node_form:
            return g.node("RMSNormalization", [inp, w], name=name, axis=-1, epsilon=s["eps"])
        var = g.node("ReduceMean", [g.node("Pow", [inp, two], name=name + "/pow"), last], name=name + "/mean", keepdims=1) \
            if opset >= 18 else g.node("ReduceMean", [g.node("Pow", [inp, two], name=name + "/pow")], name=name + "/mean",
                                       axes=[-1], keepdims=1)
        inv = g.node("Div", [one, g.node("Sqrt", [g.node("Add", [var, eps], name=name + "/add_eps")], name=name + "/sqrt")],
                     name=name + "/rsqrt")
        return g.node("Mul", [w, g.node("Mul", [inp, inv], name=name + "/normalize")], name=name + "/scale")

    for i in range(s["layers"]):
        p = "layer%d." % i
        a = rms(h, p + "input_norm")
        q = g.node("Transpose", [g.node("Reshape", [proj(a, p + "q_proj", D, D), heads_shape], name=p + "q_heads")],
                   name=p + "q_perm", perm=[0, 2, 1, 3])
        k = g.node("Transpose", [g.node("Reshape", [proj(a, p + "k_proj", D, D), heads_shape], name=p + "k_heads")],
                   name=p + "k_perm", perm=[0, 2, 1, 3])
        v = g.node("Transpose", [g.node("Reshape", [proj(a, p + "v_proj", D, D), heads_shape], name=p + "v_heads")],
                   name=p + "v_perm", perm=[0, 2, 1, 3])
        q = rope_nodes(g, q, cos, sin, hd, p + "q_", open_end=True)
        k = g.node("Transpose", [rope_nodes(g, k, cos, sin, hd, p + "k_", open_end=True)], name=p + "k_t", perm=[0, 1, 3, 2])
        sc = g.node("Div", [g.node("MatMul", [q, k], name=p + "scores"),
                            g.const(np.array(math.sqrt(hd), np.float32), "sqrt_d")], name=p + "scale")
        sc = g.node("Softmax", [g.node("Add", [sc, key_term], name=p + "mask/Add")], name=p + "softmax", axis=-1)
        ctx = g.node("MatMul", [sc, v], name=p + "context")
        ctx = g.node("Reshape", [g.node("Transpose", [ctx], name=p + "ctx_perm", perm=[0, 2, 1, 3]), merge_shape],
                     name=p + "ctx_merge")
        h = g.node("Add", [h, proj(ctx, p + "o_proj", D, D)], name=p + "residual1")
        a = rms(h, p + "post_attention_norm")
        gate, up = proj(a, p + "gate_proj", D, F), proj(a, p + "up_proj", D, F)
        act = g.node("Mul", [g.node("Mul", [gate, g.node("Sigmoid", [gate], name=p + "silu/sigmoid")], name=p + "silu"), up],
                     name=p + "swiglu")
        h = g.node("Add", [h, proj(act, p + "down_proj", F, D)], name=p + "residual2")
    h = rms(h, "norm")
    y = _sentence_head(g, "sbert_ids_hf", h, None, mask_f)
    g.output(y, ["N", D])
    return g.model_proto(opset=opset), dict(g.initializers)


def build_se_cnn(seed: int = 0, opset: int = 13) -> Tuple[bytes, Dict[str, np.ndarray]]:
    s = SPECS["se_cnn"]
    rng = _rng(seed)
    g = GraphBuilder(name="se_cnn")
    x = g.input("image", ["N", s["in_ch"], s["image"], s["image"]])

    def conv(inp, name, cin, cout, k, stride=1, pad=None, bias=True):
        pad = k // 2 if pad is None else pad
        w = g.init(name + ".weight", _lin(rng, cin * k * k, (cout, cin, k, k)))
        ins = [inp, w]
        if bias:
            ins.append(g.init(name + ".bias", (0.1 * rng.standard_normal(cout)).astype(np.float32)))
        return g.node("Conv", ins, name=name, kernel_shape=[k, k], strides=[stride, stride], pads=[pad] * 4)

    def bn(inp, name, c):
        ps = [g.init(name + "." + k, v) for k, v in (
            ("gamma", (1 + 0.1 * rng.standard_normal(c)).astype(np.float32)),
            ("beta", (0.1 * rng.standard_normal(c)).astype(np.float32)),
            ("mean", (0.1 * rng.standard_normal(c)).astype(np.float32)),
            ("var", (0.5 + rng.random(c)).astype(np.float32)))]
        return g.node("BatchNormalization", [inp] + ps, name=name, epsilon=1e-5)

    h = g.node("Relu", [bn(conv(x, "conv1", s["in_ch"], 20, 3, bias=False), "bn1", 20)], name="relu1")  # 20 % 8 != 0
    h = g.node("Relu", [conv(h, "conv2", 20, 24, 3, stride=2)], name="relu2")  # 8x8
    # squeeze-excitation: GAP -> FC(24->6) -> ReLU -> FC(6->24) -> Sigmoid -> broadcast Mul
    z = g.node("Flatten", [g.node("GlobalAveragePool", [h], name="se_gap")], name="se_flat", axis=1)
    z = g.node("Relu", [g.node("Gemm", [z, g.init("se1.weight", _lin(rng, 24, (6, 24))),
                                         g.init("se1.bias", np.zeros(6, np.float32))], name="se1", transB=1)],
               name="se_relu")
    z = g.node("Sigmoid", [g.node("Gemm", [z, g.init("se2.weight", _lin(rng, 6, (24, 6))),
                                            g.init("se2.bias", np.zeros(24, np.float32))], name="se2", transB=1)],
               name="se_sigmoid")
    z = g.node("Reshape", [z, g.const(np.array([-1, 24, 1, 1], np.int64), "se_shape")], name="se_gate")
    h = g.node("Mul", [h, z], name="se_scale")
    # two branches joined on the channel axis, then a channel slice
    b1 = g.node("Relu", [conv(h, "branch1", 24, 16, 1)], name="b1_relu")
    b2 = g.node("Tanh", [conv(h, "branch2", 24, 12, 3)], name="b2_tanh")  # last input: 12 % 8 != 0
    h = g.node("Concat", [b1, b2], name="concat", axis=1)  # 28 channels
    h = g.node("Slice", [h, g.const(np.array([8], np.int64), "sl_start"), g.const(np.array([28], np.int64), "sl_end"),
                         g.const(np.array([1], np.int64), "sl_axes")], name="slice")  # 20 channels
    h = g.node("MaxPool", [h], name="pool", kernel_shape=[2, 2], strides=[2, 2])  # 4x4
    h = g.node("Flatten", [h], name="flatten", axis=1)  # NCHW order over a 4x4 map
    w = g.init("fc.weight", _lin(rng, 20 * 16, (s["classes"], 20 * 16)))
    y = g.node("Gemm", [h, w, g.init("fc.bias", (0.1 * rng.standard_normal(s["classes"])).astype(np.float32))],
               name="fc", transB=1)
    y = g.node("Softmax", [y], name="prob", axis=-1)
    g.output(y, ["N", s["classes"]])
    return g.model_proto(opset=opset), {}


def build_ratio_mlp(seed: int = 0, opset: int = 13) -> Tuple[bytes, Dict[str, np.ndarray]]:
    s = SPECS["ratio_mlp"]
    rng = _rng(seed)
    g = GraphBuilder(name="ratio_mlp")
    x = g.input("features", ["N", s["in_features"]])
    F, Hd = s["in_features"], s["hidden"]

    def fc(inp, name, fin, fout):
        w = g.init(name + ".weight", _lin(rng, fin, (fout, fin)))
        b = g.init(name + ".bias", (0.1 * rng.standard_normal(fout)).astype(np.float32))
        return g.node("Gemm", [inp, w, b], name=name, transB=1)

    num = g.node("Tanh", [fc(x, "num", F, Hd)], name="num_tanh")                       # pad columns 0
    den = g.node("Relu", [fc(x, "den", F, Hd)], name="den_relu")                       # pad columns 0
    den = g.node("Add", [den, g.const(np.array(1.0, np.float32), "one")], name="den_shift")  # >= 1, pads 0
    r = g.node("Div", [num, den], name="ratio")                                        # pads: 0 / 0
    y = fc(r, "head", Hd, s["classes"])
    g.output(y, ["N", s["classes"]])
    return g.model_proto(opset=opset), {}


def build_ops_zoo(seed: int = 0, opset: int = 13) -> Tuple[bytes, Dict[str, np.ndarray]]:
    s = SPECS["ops_zoo"]
    rng = _rng(seed)
    g = GraphBuilder(name="ops_zoo")
    x = g.input("image", ["N", s["in_ch"], s["image"], s["image"]])
    one = g.const(np.array(1.0, np.float32), "one")
    two = g.const(np.array(2.0, np.float32), "two")

    def conv(inp, name, cin, cout, k, pad):
        w = g.init(name + ".weight", _lin(rng, cin * k * k, (cout, cin, k, k)))
        b = g.init(name + ".bias", (0.1 * rng.standard_normal(cout)).astype(np.float32))
        return g.node("Conv", [inp, w, b], name=name, kernel_shape=[k, k], pads=[pad] * 4)

    # relu first so the graph input is materialised once; Pad(1) folded into the 3x3 conv (pads 0)
    h = g.node("Relu", [x], name="relu_in")
    h = g.node("Pad", [h, g.const(np.array([0, 0, 1, 1, 0, 0, 1, 1], np.int64), "pad1")], name="pad1", mode="constant")
    h = g.node("HardSwish", [conv(h, "conv1", s["in_ch"], 16, 3, 0)], name="hswish")
    # asymmetric Pad before a MaxPool: not foldable (zeros vs -inf) -> a pad pass; 17x17 -> 8x8
    h = g.node("Pad", [h, g.const(np.array([0, 0, 0, 1, 0, 0, 1, 0], np.int64), "pad2")], name="pad2", mode="constant")
    h = g.node("MaxPool", [h], name="pool", kernel_shape=[2, 2], strides=[2, 2])
    a, b = g.node("Split", [h, g.const(np.array([8, 8], np.int64), "split_sizes")], name="split", axis=1, n_out=2)
    a = g.node("Exp", [g.node("Neg", [g.node("Abs", [a], name="abs")], name="neg")], name="exp")  # (0, 1]
    sp = g.node("Softplus", [b], name="softplus")
    hs = g.node("HardSigmoid", [b], name="hsigmoid", alpha=0.25, beta=0.4)
    mx = g.node("Max", [a, sp], name="max")
    mn = g.node("Min", [a, hs], name="min")
    h = g.node("Concat", [mx, mn], name="cat", axis=1)  # 16 channels
    h = conv(h, "conv2", 16, 12, 1, 0)  # 12 % 8 != 0
    r = g.node("Reciprocal", [g.node("Add", [g.node("Pow", [h, two], name="pow"), one], name="pow1")], name="recip")
    h = g.node("Erf", [g.node("Log", [r], name="log")], name="erf")  # log of (0, 1]
    h = g.node("Sqrt", [g.node("Abs", [h], name="abs2")], name="sqrt")
    rmax = g.node("ReduceMax", [h], name="rmax", axes=[2, 3], keepdims=1)
    rsum = g.node("ReduceSum", [h, g.const(np.array([2, 3], np.int64), "rsum_axes")], name="rsum", keepdims=1)
    gmax = g.node("GlobalMaxPool", [h], name="gmax")
    z = g.node("Add", [g.node("Add", [rmax, rsum], name="pool_add"), gmax], name="pool_add2")
    z = g.node("Flatten", [z], name="flatten", axis=1)  # rows [N, 12]
    z = g.node("Gemm", [z, g.init("fc1.weight", _lin(rng, 12, (16, 12))),
                        g.init("fc1.bias", (0.1 * rng.standard_normal(16)).astype(np.float32))], name="fc1", transB=1)
    u, v = g.node("Split", [z], name="row_split", axis=1, n_out=2)  # equal parts of rows
    z = g.node("Concat", [g.node("HardSwish", [u], name="row_hswish"), g.node("Softplus", [v], name="row_softplus")],
               name="row_cat", axis=1)
    w = g.init("fc2.weight", _lin(rng, 16, (s["classes"], 16)))
    y = g.node("Gemm", [z, w, g.init("fc2.bias", np.zeros(s["classes"], np.float32))], name="fc2", transB=1)
    g.output(y, ["N", s["classes"]])
    return g.model_proto(opset=opset), {}


def build_upsample_net(seed: int = 0, opset: int = 13) -> Tuple[bytes, Dict[str, np.ndarray]]:
    s = SPECS["upsample_net"]
    rng = _rng(seed)
    g = GraphBuilder(name="upsample_net")
    x = g.input("image", ["N", s["in_ch"], s["image"], s["image"]])
    f32 = 1  # onnx FLOAT
    empty = g.const(np.zeros(0, np.float32), "no_roi")

    def c(v, name):
        return g.const(np.array(v, np.float32), name)

    w1 = g.init("conv1.weight", _lin(rng, 8 * 9, (16, 8, 3, 3)))
    h = g.node("Relu", [g.node("Conv", [x, w1, g.init("conv1.bias", (0.1 * rng.standard_normal(16)).astype(np.float32))],
                               name="conv1", kernel_shape=[3, 3], pads=[1, 1, 1, 1])], name="relu1")  # 12x12x16
    wt = g.init("up.weight", _lin(rng, 16 * 9 / 4, (16, 12, 3, 3)))  # ConvTranspose weight [Cin, Cout, kh, kw]
    d = g.node("ConvTranspose", [h, wt, g.init("up.bias", (0.1 * rng.standard_normal(12)).astype(np.float32))],
               name="up", kernel_shape=[3, 3], strides=[2, 2], pads=[1, 1, 1, 1], output_padding=[1, 1])  # 24x24x12
    u = g.node("Resize", [h, empty, g.const(np.array([1, 1, 2, 2], np.float32), "nn_scales")], name="nn_up",
               mode="nearest", coordinate_transformation_mode="asymmetric", nearest_mode="floor")  # 24x24x16
    u2 = g.node("Conv", [u, g.init("proj.weight", _lin(rng, 16, (12, 16, 1, 1)))], name="proj", kernel_shape=[1, 1])
    z = g.node("Where", [g.node("Greater", [d, u2], name="gt"), d, u2], name="pick_max")           # max(d, u2)
    z = g.node("Where", [g.node("Less", [z, c(0.0, "zero")], name="neg"), c(0.0, "zero_f"), z], name="relu_where")
    r = g.node("Resize", [z, empty, g.const(np.array([1, 1, 0.5, 0.5], np.float32), "down_scales")], name="down",
               mode="linear", coordinate_transformation_mode="half_pixel")                          # 12x12
    r2 = g.node("Resize", [r, empty, g.const(np.array([1, 1, 1.5, 1.5], np.float32), "up_scales")], name="up15",
                mode="linear", coordinate_transformation_mode="align_corners")                      # 18x18
    r2 = g.node("Sub", [r2, c(0.3, "shift")], name="center")
    m1 = g.node("And", [g.node("Greater", [r2, c(0.0, "zero2")], name="pos"),
                        g.node("Less", [c(50.0, "big"), r2], name="huge")], name="pos_and")  # r2 > 0 and 50 < r2: empty
    m1 = g.node("Or", [m1, g.node("Greater", [r2, c(0.0, "zero3")], name="pos2")], name="pos_or")  # = r2 > 0
    m2 = g.node("Not", [m1], name="nonpos")
    pos = g.node("Mul", [r2, g.node("Cast", [m1], name="m1f", to=f32)], name="pos_part")
    neg = g.node("Mul", [r2, g.node("Cast", [m2], name="m2f", to=f32)], name="neg_part")
    hsum = g.node("Sub", [pos, g.node("Mul", [neg, c(0.1, "slope")], name="leak")], name="leaky")  # leaky ReLU
    z = g.node("Flatten", [g.node("GlobalAveragePool", [hsum], name="gap")], name="flat", axis=1)
    w = g.init("fc.weight", _lin(rng, 12, (s["classes"], 12)))
    y = g.node("Gemm", [z, w, g.init("fc.bias", np.zeros(s["classes"], np.float32))], name="fc", transB=1)
    g.output(y, ["N", s["classes"]])
    return g.model_proto(opset=opset), {}


def build_token_mixer(seed: int = 0, opset: int = 13) -> Tuple[bytes, Dict[str, np.ndarray]]:
    s = SPECS["token_mixer"]
    rng = _rng(seed)
    S, D = s["seq"], s["dim"]
    g = GraphBuilder(name="token_mixer")
    x = g.input("tokens", ["N", S * D])
    h = g.node("Reshape", [x, g.const(np.array([0, S, D], np.int64), "seq_shape")], name="to_tokens")
    logits = g.node("MatMul", [h, g.init("mix.weight", _lin(rng, D, (D, S)))], name="mix_logits")  # [N, S, S]
    a = g.node("Softmax", [logits], name="mix_softmax", axis=-1)
    m = g.node("MatMul", [a, h], name="mix")                                                  # [S, S] x [S, D]
    h = g.node("Add", [m, h], name="mix_residual")
    gl = g.node("Add", [g.node("MatMul", [h, g.init("gate.weight", _lin(rng, D, (D, 20)))], name="gate/MatMul"),
                        g.init("gate.bias", (0.1 * rng.standard_normal(20)).astype(np.float32))], name="gate/Add")
    gl = g.node("Tanh", [gl], name="gate_tanh")                                               # [N, S, 20]
    m2 = g.node("MatMul", [a, gl], name="mix2")                                               # [S, S] x [S, 20]
    pooled = g.node("ReduceMean", [m2], name="pool", axes=[1], keepdims=0)                    # [N, 20]
    w = g.init("head.weight", _lin(rng, 20, (s["classes"], 20)))
    y = g.node("Gemm", [pooled, w, g.init("head.bias", np.zeros(s["classes"], np.float32))], name="head", transB=1)
    g.output(y, ["N", s["classes"]])
    return g.model_proto(opset=opset), {}


def build_ln_wide(seed: int = 0, opset: int = 17) -> Tuple[bytes, Dict[str, np.ndarray]]:
    s = SPECS["ln_wide"]
    rng = _rng(seed)
    S, D, Wd = s["seq"], s["dim"], s["wide"]
    g = GraphBuilder(name="ln_wide")
    x = g.input("tokens", ["N", S * D])
    h = g.node("Reshape", [x, g.const(np.array([0, S, D], np.int64), "seq_shape")], name="to_tokens")

    def ln(inp, name, c):
        gw = g.init(name + ".weight", (1.0 + 0.1 * rng.standard_normal(c)).astype(np.float32))
        gb = g.init(name + ".bias", (0.1 * rng.standard_normal(c)).astype(np.float32))
        return g.node("LayerNormalization", [inp, gw, gb], name=name, axis=-1, epsilon=1e-5)

    h = ln(h, "ln_in", D)  # 20 logical columns, 24 stored
    h = g.node("Add", [g.node("MatMul", [h, g.init("up.weight", _lin(rng, D, (D, Wd)))], name="up/MatMul"),
                       g.init("up.bias", (0.1 * rng.standard_normal(Wd)).astype(np.float32))], name="up/Add")
    h = g.node("Tanh", [ln(h, "ln_wide", Wd)], name="act")  # 2560 columns
    pooled = g.node("ReduceMean", [h], name="pool", axes=[1], keepdims=0)
    w = g.init("head.weight", _lin(rng, Wd, (s["classes"], Wd)))
    y = g.node("Gemm", [pooled, w, g.init("head.bias", np.zeros(s["classes"], np.float32))], name="head", transB=1)
    g.output(y, ["N", s["classes"]])
    return g.model_proto(opset=opset), {}


def build_ln_offset(seed: int = 0, opset: int = 17, offset: float = 60.0) -> Tuple[bytes, Dict[str, np.ndarray]]:
    """offset: the row-constant DC offset added before the LayerNorm, in units of the rows' own
    standard deviation (the tokens are N(0, 1))."""
    s = SPECS["ln_offset"]
    rng = _rng(seed)
    S, D, H = s["seq"], s["dim"], s["hidden"]
    g = GraphBuilder(name="ln_offset")
    x = g.input("tokens", ["N", S * D])
    h = g.node("Reshape", [x, g.const(np.array([0, S, D], np.int64), "seq_shape")], name="to_tokens")
    # a row-constant offset (the same for every channel): |mean| / std of each row ~ 60 -- the
    # cancellation case -- plus a small per-channel spread
    off = (offset + 0.5 * rng.standard_normal(D)).astype(np.float32)
    h = g.node("Add", [h, g.init("offset", off)], name="dc_offset")

    def ln(inp, name, c):
        gw = g.init(name + ".weight", (1.0 + 0.1 * rng.standard_normal(c)).astype(np.float32))
        gb = g.init(name + ".bias", (0.1 * rng.standard_normal(c)).astype(np.float32))
        return g.node("LayerNormalization", [inp, gw, gb], name=name, axis=-1, epsilon=1e-5)

    h = g.node("Add", [g.node("MatMul", [ln(h, "ln0", D), g.init("fc1.weight", _lin(rng, D, (D, H)))], name="fc1/MatMul"),
                       g.init("fc1.bias", (0.1 * rng.standard_normal(H)).astype(np.float32))], name="fc1/Add")
    h = g.node("Tanh", [h], name="act")
    pooled = g.node("ReduceMean", [h], name="pool", axes=[1], keepdims=0)
    w = g.init("head.weight", _lin(rng, H, (s["classes"], H)))
    y = g.node("Gemm", [pooled, w, g.init("head.bias", np.zeros(s["classes"], np.float32))], name="head", transB=1)
    g.output(y, ["N", s["classes"]])
    return g.model_proto(opset=opset), {}


def repeat_kv_nodes(g, x, Hkv, G, S, hd, p, full_shape=True, batch=0):
    """HF's repeat_kv export on the heads view x [N, Hkv, S, hd]: Unsqueeze(2) -> Expand -> Reshape to
    [N, Hkv * G, S, hd].  full_shape: the Expand target is [1, Hkv, G, S, hd], else [1, 1, G, 1, 1];
    batch: the Reshape's batch entry (0 or -1)."""
    u = g.node("Unsqueeze", [x, g.const(np.array([2], np.int64), "repeat_axis")], name=p + "repeat/unsqueeze")
    shape = [1, Hkv, G, S, hd] if full_shape else [1, 1, G, 1, 1]
    e = g.node("Expand", [u, g.const(np.array(shape, np.int64), "repeat_shape")], name=p + "repeat/expand")
    return g.node("Reshape", [e, g.const(np.array([batch, Hkv * G, S, hd], np.int64), "repeat_merge")],
                  name=p + "repeat/merge")


def build_gqa_model(seed: int = 0, opset: int = 17, spec: str = "gqa_enc",
                    expand_kv: bool = False) -> Tuple[bytes, Dict[str, np.ndarray]]:
    """The grouped-query attention models: K and V are projected to kv_heads < heads heads and every
    K/V head is repeated over its group of heads / kv_heads query heads by HF's repeat_kv
    (`repeat_kv_nodes`, after the head Transpose and after RoPE on K).
    * `gqa_enc`     the `llama_enc` body (token ids, RMSNorm, RoPE, bias-free projections, SwiGLU, ids-derived
                    key mask, masked mean + L2 normalisation): 4 heads of 64 over 2 K/V heads, 160 tokens.
    * `mqa_causal`  the `gpt_causal` body (float embeddings, pre-LN, projections with biases, the causal
                    Where, a classifier head): 4 heads of 64 over ONE K/V head, 72 tokens.
    * `gqa_hd128`   the `rope_bert` body (float embeddings, post-LN, RoPE, a classifier head): 6 heads of 128
                    over 2 K/V heads (groups of 3), 40 tokens.
    expand_kv: the multi-head twin -- the same weights with the K / V projection columns (and biases)
    repeated per group and no repeat nodes; it computes what the GQA model computes.
    Returns (model bytes, initializers)."""
    from ..utils.onnx_writer import INT64

    s = SPECS[spec]
    rng = _rng(seed)
    S, D, H, Hkv, F = s["seq"], s["dim"], s["heads"], s["kv_heads"], s["ffn"]
    hd, G = D // H, H // Hkv
    Dkv = Hkv * hd
    body = s["body"]  # "llama", "gpt" or "rope_bert"
    g = GraphBuilder(name=spec + ("_expanded" if expand_kv else ""))
    one = g.const(np.array(1.0, np.float32), "one")
    if body == "llama":
        x = g.input("input_ids", ["N", S])
        ids = g.node("Cast", [x], name="ids_int", to=INT64)
        table = g.init("embed_tokens.weight", (0.5 * rng.standard_normal((s["vocab"], D))).astype(np.float32))
        h = g.node("Gather", [table, ids], name="embed_tokens", axis=0)
        mask_f = g.node("Cast", [g.node("Greater", [x, g.const(np.array(0, np.float32), "pad_id")], name="attention_mask")],
                        name="attention_mask_f", to=1)
        m = g.node("Unsqueeze", [mask_f, g.const(np.array([1, 2], np.int64), "mask_axes")], name="extended_mask")
        key_term = g.node("Mul", [g.node("Sub", [one, m], name="inverted_mask"),
                                  g.const(np.array(-10000.0, np.float32), "mask_value")], name="additive_mask")
    else:
        x = g.input("embeddings", ["N", S * D])
        h = g.node("Reshape", [x, g.const(np.array([0, S, D], np.int64), "seq_shape")], name="to_tokens")
    q_shape = g.const(np.array([0, 0, H, hd], np.int64), "heads_shape")
    kv_shape = q_shape if expand_kv else g.const(np.array([0, 0, Hkv, hd], np.int64), "kv_heads_shape")
    merge_shape = g.const(np.array([0, 0, D], np.int64), "merge_shape")
    sqrt_d = g.const(np.array(math.sqrt(hd), np.float32), "sqrt_d")
    sqrt2 = g.const(np.array(1.4142135381698608, np.float32), "sqrt2")
    half = g.const(np.array(0.5, np.float32), "half")
    two = g.const(np.array(2.0, np.float32), "two")
    rope = body != "gpt"
    if rope:
        c, sn = rope_tables(S, hd, s["theta"])
        cos, sin = g.init("rope.cos", c.reshape(1, 1, S, hd)), g.init("rope.sin", sn.reshape(1, 1, S, hd))
    with_bias = body != "llama"

    def widen(a):  # [.., Hkv * hd] -> [.., H * hd]: every K/V head's columns repeated over its group
        return np.repeat(a.reshape(a.shape[:-1] + (Hkv, hd)), G, axis=-2).reshape(a.shape[:-1] + (D,))

    def linear(inp, name, fin, fout, kv=False):
        w = _lin(rng, fin, (fin, fout))
        b = (0.02 * rng.standard_normal(fout)).astype(np.float32) if with_bias else None
        if kv and expand_kv:
            w, b = widen(w), (widen(b) if b is not None else None)
        y = g.node("MatMul", [inp, g.init(name + ".weight", w)], name=name + ("/MatMul" if with_bias else ""))
        return g.node("Add", [y, g.init(name + ".bias", b)], name=name + "/Add") if with_bias else y

    def norm(inp, name):
        gw = g.init(name + ".weight", (1.0 + 0.1 * rng.standard_normal(D)).astype(np.float32))
        if body == "llama":  # torch's decomposed RMSNorm
            var = g.node("ReduceMean", [g.node("Pow", [inp, two], name=name + "/pow")], name=name + "/mean", axes=[-1],
                         keepdims=1)
            inv = g.node("Div", [one, g.node("Sqrt", [g.node("Add", [var, g.const(np.array(s["eps"], np.float32), "rms_eps")],
                                                             name=name + "/add_eps")], name=name + "/sqrt")],
                         name=name + "/rsqrt")
            return g.node("Mul", [gw, g.node("Mul", [inp, inv], name=name + "/normalize")], name=name + "/scale")
        gb = g.init(name + ".bias", (0.1 * rng.standard_normal(D)).astype(np.float32))
        return g.node("LayerNormalization", [inp, gw, gb], name=name, axis=-1, epsilon=1e-5)

    def attention(a, p, layer):
        bhsd = [0, 2, 1, 3]
        q = g.node("Transpose", [g.node("Reshape", [linear(a, p + "q_proj", D, D), q_shape], name=p + "q_heads")],
                   name=p + "q_perm", perm=bhsd)
        k = g.node("Transpose", [g.node("Reshape", [linear(a, p + "k_proj", D, Dkv, kv=True), kv_shape], name=p + "k_heads")],
                   name=p + "k_perm", perm=bhsd)
        v = g.node("Transpose", [g.node("Reshape", [linear(a, p + "v_proj", D, Dkv, kv=True), kv_shape], name=p + "v_heads")],
                   name=p + "v_perm", perm=bhsd)
        if rope:
            q = rope_nodes(g, q, cos, sin, hd, p + "q_", open_end=True)
            k = rope_nodes(g, k, cos, sin, hd, p + "k_", open_end=True)
        if not expand_kv:  # the two Expand shape forms and both Reshape batch entries, by layer
            k = repeat_kv_nodes(g, k, Hkv, G, S, hd, p + "k_", full_shape=layer % 2 == 0, batch=0)
            v = repeat_kv_nodes(g, v, Hkv, G, S, hd, p + "v_", full_shape=layer % 2 == 0, batch=-1 if layer % 2 else 0)
        k = g.node("Transpose", [k], name=p + "k_t", perm=[0, 1, 3, 2])
        sc = g.node("Div", [g.node("MatMul", [q, k], name=p + "scores"), sqrt_d], name=p + "scale")
        if body == "llama":
            sc = g.node("Add", [sc, key_term], name=p + "mask/Add")
        elif body == "gpt":
            tril = g.init(p + "causal_mask", np.tril(np.ones((1, 1, S, S), np.bool_)))
            sc = g.node("Where", [tril, sc, g.const(np.array(-1e4, np.float32), "mask_fill")], name=p + "causal")
        sc = g.node("Softmax", [sc], name=p + "softmax", axis=-1)
        ctx = g.node("MatMul", [sc, v], name=p + "context")
        ctx = g.node("Reshape", [g.node("Transpose", [ctx], name=p + "ctx_perm", perm=bhsd), merge_shape],
                     name=p + "ctx_merge")
        return linear(ctx, p + "o_proj", D, D)

    def ffn(a, p):
        if body == "llama":
            gate, up = linear(a, p + "gate_proj", D, F), linear(a, p + "up_proj", D, F)
            act = g.node("Mul", [g.node("Mul", [gate, g.node("Sigmoid", [gate], name=p + "silu/sigmoid")], name=p + "silu"),
                                 up], name=p + "swiglu")
            return linear(act, p + "down_proj", F, D)
        m1 = linear(a, p + "intermediate", D, F)
        t = g.node("Div", [m1, sqrt2], name=p + "gelu/div")
        t = g.node("Add", [g.node("Erf", [t], name=p + "gelu/erf"), one], name=p + "gelu/add")
        t = g.node("Mul", [g.node("Mul", [m1, t], name=p + "gelu/mul"), half], name=p + "gelu/half")
        return linear(t, p + "output", F, D)

    for i in range(s["layers"]):
        p = "layer%d." % i
        if body == "rope_bert":  # post-LN
            h = norm(g.node("Add", [attention(h, p, i), h], name=p + "residual1"), p + "ln1")
            h = norm(g.node("Add", [ffn(h, p), h], name=p + "residual2"), p + "ln2")
        else:  # pre-norm: x + attn(norm(x)), x + ffn(norm(x))
            h = g.node("Add", [h, attention(norm(h, p + "norm1"), p, i)], name=p + "residual1")
            h = g.node("Add", [h, ffn(norm(h, p + "norm2"), p)], name=p + "residual2")
    if body != "rope_bert":
        h = norm(h, "norm_f")
    if body == "llama":
        y = _sentence_head(g, "sbert_ids_hf", h, None, mask_f)
        g.output(y, ["N", D])
        return g.model_proto(opset=opset), dict(g.initializers)
    pooled = g.node("ReduceMean", [h], name="mean_pool", axes=[1], keepdims=0)
    w = g.init("classifier.weight", _lin(rng, D, (s["classes"], D)))
    b = g.init("classifier.bias", (0.1 * rng.standard_normal(s["classes"])).astype(np.float32))
    y = g.node("Gemm", [pooled, w, b], name="classifier", transB=1)
    g.output(y, ["N", s["classes"]])
    return g.model_proto(opset=opset), dict(g.initializers)


BUILDERS = {"mlp": build_mlp, "bert": build_bert, "se_cnn": build_se_cnn, "ratio_mlp": build_ratio_mlp,
            "ops_zoo": build_ops_zoo, "upsample_net": build_upsample_net, "token_mixer": build_token_mixer,
            "ln_wide": build_ln_wide, "ln_offset": build_ln_offset,
            "bert_long": lambda seed=0: build_bert(seed, spec="bert_long"),
            "bert_hd32": lambda seed=0: build_bert(seed, spec="bert_hd32"),
            "bert_hd128": lambda seed=0: build_bert(seed, spec="bert_hd128"),
            "gpt_causal": lambda seed=0: build_masked_encoder(seed, spec="gpt_causal"),
            "bert_relpos": lambda seed=0: build_masked_encoder(seed, spec="bert_relpos"),
            "bert_window": lambda seed=0: build_masked_encoder(seed, spec="bert_window"),
            "bert_keymask": lambda seed=0: build_masked_encoder(seed, spec="bert_keymask"),
            "bert_ids": lambda seed=0: build_token_encoder(seed, spec="bert_ids"),
            "bert_ids_hf": lambda seed=0: build_token_encoder(seed, spec="bert_ids_hf"),
            "sbert_ids": lambda seed=0: build_token_encoder(seed, spec="sbert_ids"),
            "sbert_ids_hf": lambda seed=0: build_token_encoder(seed, spec="sbert_ids_hf"),
            "sbert_cls": lambda seed=0: build_token_encoder(seed, spec="sbert_cls"),
            "bert_hf3": lambda seed=0: build_token_encoder(seed, spec="bert_hf3"),
            "sbert_hf2": lambda seed=0: build_token_encoder(seed, spec="sbert_hf2"),
            "bert_hf3_maskfirst": lambda seed=0: build_token_encoder(seed, spec="bert_hf3_maskfirst"),
            "rope_bert": lambda seed=0: build_rope_encoder(seed, spec="rope_bert"),
            "rope_bert_nshd": lambda seed=0: build_rope_encoder(seed, spec="rope_bert_nshd"),
            "llama_enc": lambda seed=0: build_llama_encoder(seed, spec="llama_enc"),
            "llama_enc_rmsnode": lambda seed=0: build_llama_encoder(seed, spec="llama_enc_rmsnode"),
            "gqa_enc": lambda seed=0, expand_kv=False: build_gqa_model(seed, spec="gqa_enc", expand_kv=expand_kv),
            "mqa_causal": lambda seed=0, expand_kv=False: build_gqa_model(seed, spec="mqa_causal", expand_kv=expand_kv),
            "gqa_hd128": lambda seed=0, expand_kv=False: build_gqa_model(seed, spec="gqa_hd128", expand_kv=expand_kv)}


def build_onnx(name: str, seed: int = 0) -> bytes:
    return BUILDERS[name](seed)[0]


def input_shape(name: str):
    s = SPECS[name]
    if name in ("mlp", "ratio_mlp"):
        return (s["in_features"],)
    if name in ("bert", "bert_long", "bert_hd32", "bert_hd128", "token_mixer", "ln_wide", "ln_offset") + MASKED + ROPE_BERT + \
            ("mqa_causal", "gqa_hd128"):
        return (s["seq"] * s["dim"],)
    if name in MULTI_INPUT:  # a request row: every input's [S] in declaration order
        return (len(s["inputs"]) * s["seq"],)
    if name in TOKEN_IDS:
        return (s["seq"],)
    return (s["in_ch"], s["image"], s["image"])


def synthetic_input(name: str, batch: int, seed: int = 1) -> np.ndarray:
    rng = np.random.default_rng(seed)
    if name in MULTI_INPUT:
        return synthetic_request(name, batch, rng)
    if name in TOKEN_IDS:
        return synthetic_ids(name, batch, rng)
    return rng.standard_normal((batch,) + input_shape(name)).astype(np.float32)


def synthetic_lengths(name: str, batch: int):
    """Sequence length of each sample of a token-id batch: a first-tile length, a tile edge, the full
    length and two mid-tile lengths, in turn."""
    S = SPECS[name]["seq"]
    return [min(S, (1, 32, S, 45, 33)[i % 5]) for i in range(batch)]


def synthetic_ids(name: str, batch: int, rng, full_length: bool = False) -> np.ndarray:
    """float32 ids in [1, V); past its length a row holds the pad id; every third sample has one
    pad id inside its length (a hole)."""
    s = SPECS[name]
    S, V, pad = s["seq"], s["vocab"], s["pad"]
    ids = rng.integers(1, V, size=(batch, S)).astype(np.float32)
    if full_length:
        return ids
    for i, n in enumerate(synthetic_lengths(name, batch)):
        ids[i, n:] = pad
        if i % 3 == 2 and n >= 3:
            ids[i, n // 2] = pad
    return ids


def synthetic_request(name: str, batch: int, rng, inputs=None) -> np.ndarray:
    """float32 request rows [batch, K * S] of a multi-input token model: the segments of `inputs`
    (default: the spec's declaration order) one after the other.  Built so that only a mask really
    read from the mask input gives the right answer: sample i is visible up to synthetic_lengths,
    every third sample has a hole (mask 0 inside its length), the ids in HIDDEN positions are random
    non-zero ids, every sample of length >= 3 has one VISIBLE token whose id is 0, and the types are 0
    up to half the length, then 1."""
    s = SPECS[name]
    S, V = s["seq"], s["vocab"]
    seg = dict(ids=rng.integers(1, V, size=(batch, S)).astype(np.float32), mask=np.zeros((batch, S), np.float32),
               types=np.zeros((batch, S), np.float32))
    for i, n in enumerate(synthetic_lengths(name, batch)):
        seg["mask"][i, :n] = 1
        seg["types"][i, n // 2:n] = 1
        if i % 3 == 2 and n >= 3:
            seg["mask"][i, n // 2] = 0
        if n >= 3:  # position 1 unless the hole sits there (n = 3)
            seg["ids"][i, 2 if seg["mask"][i, 1] == 0 else 1] = 0
    return np.concatenate([seg[r] for r in (inputs or s["inputs"])], axis=1)
