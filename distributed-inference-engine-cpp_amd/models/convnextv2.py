"""ConvNeXt-V2 ONNX generator + torch reference: ConvNeXt's channels-last blocks without the layer scale and
with Global Response Normalization (GRN) between the GELU and the second pointwise layer.

Graph layout follows the timm `convnextv2_*` and HuggingFace `ConvNextV2ForImageClassification` exports at
opset 17; the stem, downsample and head are the V1 generator's forms (models/convnext.py):
  block: Conv 7x7 pad 3 group=C (bias) -> Transpose(0,2,3,1) -> LayerNormalization
         -> MatMul [C,4C] + Add -> GELU(erf: Div, Erf, Add, Mul, Mul) = x
         -> GRN: G = ReduceL2(x, axes [1,2], keepdims 1); nx = Div(G, Add(ReduceMean(G, axes [-1], keepdims 1), eps))
                 spec "hf":   Add(Add(Mul(weight [1,1,1,4C], Mul(x, nx)), bias [1,1,1,4C]), x)
                 spec "timm": Add(x, Add(bias [4C], Mul(weight [4C], Mul(x, nx))))     (x + addcmul(bias, weight, x * nx))
         -> MatMul [4C,C] + Add -> Transpose(0,3,1,2) -> Add(shortcut)
Weights are random (no checkpoint offline); `torch_forward` rebuilds the network from the same arrays and is
the oracle.  The GRN weight is U(0.5, 1.5) and its bias N(0, 0.05): the checkpoints' init of zeros would hide
the op from every output check.
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Dict, Tuple

import numpy as np

from ..utils.onnx_writer import GraphBuilder
from .convnext import synthetic_input  # noqa: F401  (the same seeded images)


@dataclass
class ConvNeXtV2Config:
    image: int = 224
    in_ch: int = 3
    depths: Tuple[int, ...] = (3, 3, 9, 3)
    dims: Tuple[int, ...] = (96, 192, 384, 768)  # ConvNeXt-V2-T
    num_classes: int = 1000
    eps: float = 1e-6      # LayerNorm
    grn_eps: float = 1e-6
    seed: int = 0
    spec: str = "timm"     # the GRN export form: "timm" or "hf"


def tiny_convnextv2_config(seed: int = 0, **kw) -> ConvNeXtV2Config:
    # maps 8 / 4 / 2 / 1: GRN over 64, 16, 4 pixels and over one
    return ConvNeXtV2Config(image=32, depths=(1, 1, 2, 1), dims=(16, 32, 64, 128), num_classes=16, seed=seed, **kw)


def atto_config(seed: int = 0, **kw) -> ConvNeXtV2Config:
    return ConvNeXtV2Config(depths=(2, 2, 6, 2), dims=(40, 80, 160, 320), seed=seed, **kw)


# the export forms the tests run over
SPECS = {
    "timm": {"spec": "timm"},
    "hf": {"spec": "hf", "grn_eps": 1e-6},
}


def make_weights(cfg: ConvNeXtV2Config) -> Dict[str, np.ndarray]:
    rng = np.random.default_rng(cfg.seed)
    w: Dict[str, np.ndarray] = {}

    def conv(name, cout, cin_per_group, k):
        std = 1.0 / math.sqrt(cin_per_group * k * k)
        w[name + ".weight"] = rng.normal(0, std, (cout, cin_per_group, k, k)).astype(np.float32)
        w[name + ".bias"] = rng.normal(0, 0.02, cout).astype(np.float32)

    def ln(name, c):
        w[name + ".weight"] = rng.uniform(0.8, 1.2, c).astype(np.float32)
        w[name + ".bias"] = rng.normal(0, 0.05, c).astype(np.float32)

    def lin(name, k, n, std):
        w[name + ".weight"] = rng.normal(0, std, (k, n)).astype(np.float32)  # [in, out]
        w[name + ".bias"] = rng.normal(0, 0.02, n).astype(np.float32)

    conv("stem.conv", cfg.dims[0], cfg.in_ch, 4)
    ln("stem.norm", cfg.dims[0])
    for s, (depth, C) in enumerate(zip(cfg.depths, cfg.dims)):
        if s > 0:
            ln("stages.%d.downsample.norm" % s, cfg.dims[s - 1])
            conv("stages.%d.downsample.conv" % s, C, cfg.dims[s - 1], 2)
        for i in range(depth):
            p = "stages.%d.blocks.%d." % (s, i)
            conv(p + "dwconv", C, 1, 7)
            ln(p + "norm", C)
            lin(p + "pwconv1", C, 4 * C, 1.0 / math.sqrt(C))
            w[p + "grn.weight"] = rng.uniform(0.5, 1.5, 4 * C).astype(np.float32)
            w[p + "grn.bias"] = rng.normal(0, 0.05, 4 * C).astype(np.float32)
            lin(p + "pwconv2", 4 * C, C, 0.5 / math.sqrt(4 * C))
    ln("head.norm", cfg.dims[-1])
    w["head.fc.weight"] = rng.normal(0, 1.0 / math.sqrt(cfg.dims[-1]), (cfg.num_classes, cfg.dims[-1])).astype(np.float32)
    w["head.fc.bias"] = rng.normal(0, 0.01, cfg.num_classes).astype(np.float32)
    return w


def grn_nodes(g: GraphBuilder, x: str, weight: str, bias: str, eps: str, name: str, spec: str = "timm",
              spatial=(1, 2), channel: int = -1) -> str:
    """The exported GRN chain on `x`; weight / bias / eps are value names (None: that parameter is absent)."""
    G = g.node("ReduceL2", [x], name=name + "/norm", axes=list(spatial), keepdims=1)
    mu = g.node("ReduceMean", [G], name=name + "/mean", axes=[channel], keepdims=1)
    nx = g.node("Div", [G, g.node("Add", [mu, eps], name=name + "/add_eps")], name=name + "/div")
    y = g.node("Mul", [x, nx], name=name + "/mul_x")
    if spec == "hf":
        if weight is not None:
            y = g.node("Mul", [weight, y], name=name + "/scale")
        if bias is not None:
            y = g.node("Add", [y, bias], name=name + "/shift")
        return g.node("Add", [y, x], name=name + "/residual")
    if weight is not None:
        y = g.node("Mul", [weight, y], name=name + "/scale")
    if bias is not None:
        y = g.node("Add", [bias, y], name=name + "/shift")
    return g.node("Add", [x, y], name=name + "/residual")


def build_onnx(cfg: ConvNeXtV2Config = ConvNeXtV2Config(), opset: int = 17) -> Tuple[bytes, Dict[str, np.ndarray]]:
    assert cfg.spec in ("timm", "hf"), cfg.spec
    w = make_weights(cfg)
    g = GraphBuilder(name="convnextv2")
    for k, v in w.items():
        if cfg.spec == "hf" and (k.endswith("grn.weight") or k.endswith("grn.bias")):
            v = v.reshape(1, 1, 1, -1)
        g.init(k, v)
    x = g.input("pixel_values", ["batch", cfg.in_ch, cfg.image, cfg.image])
    sqrt2 = g.const(np.array(1.4142135381698608, np.float32), "sqrt2")
    one = g.const(np.array(1.0, np.float32), "one")
    half = g.const(np.array(0.5, np.float32), "half")
    grn_eps = g.const(np.array(cfg.grn_eps, np.float32), "grn_eps")

    def image_ln(inp, wname, name):
        t = g.node("Transpose", [inp], name=name + "/to_nhwc", perm=[0, 2, 3, 1])
        t = g.node("LayerNormalization", [t, wname + ".weight", wname + ".bias"], name=name, axis=-1, epsilon=cfg.eps)
        return g.node("Transpose", [t], name=name + "/to_nchw", perm=[0, 3, 1, 2])

    def conv(inp, name, k, stride, pad, group=1):
        return g.node("Conv", [inp, name + ".weight", name + ".bias"], name=name, kernel_shape=[k, k],
                      strides=[stride, stride], pads=[pad] * 4, group=group)

    def linear(inp, name):
        y = g.node("MatMul", [inp, name + ".weight"], name=name + "/MatMul")
        return g.node("Add", [y, name + ".bias"], name=name + "/Add")

    h = conv(x, "stem.conv", 4, 4, 0)
    h = image_ln(h, "stem.norm", "stem.norm")
    for s, (depth, C) in enumerate(zip(cfg.depths, cfg.dims)):
        if s > 0:
            h = image_ln(h, "stages.%d.downsample.norm" % s, "stages.%d.downsample.norm" % s)
            h = conv(h, "stages.%d.downsample.conv" % s, 2, 2, 0)
        for i in range(depth):
            p = "stages.%d.blocks.%d." % (s, i)
            y = conv(h, p + "dwconv", 7, 1, 3, group=C)
            y = g.node("Transpose", [y], name=p + "to_nhwc", perm=[0, 2, 3, 1])
            y = g.node("LayerNormalization", [y, p + "norm.weight", p + "norm.bias"], name=p + "norm", axis=-1,
                       epsilon=cfg.eps)
            m = linear(y, p + "pwconv1")
            t = g.node("Div", [m, sqrt2], name=p + "gelu/div")
            t = g.node("Erf", [t], name=p + "gelu/erf")
            t = g.node("Add", [t, one], name=p + "gelu/add")
            t = g.node("Mul", [m, t], name=p + "gelu/mul")
            t = g.node("Mul", [t, half], name=p + "gelu/half")
            t = grn_nodes(g, t, p + "grn.weight", p + "grn.bias", grn_eps, p + "grn", cfg.spec)
            y = linear(t, p + "pwconv2")
            y = g.node("Transpose", [y], name=p + "to_nchw", perm=[0, 3, 1, 2])
            h = g.node("Add", [y, h], name=p + "residual")
    h = g.node("GlobalAveragePool", [h], name="head.pool")
    h = image_ln(h, "head.norm", "head.norm")
    h = g.node("Flatten", [h], name="head.flatten", axis=1)
    y = g.node("Gemm", [h, "head.fc.weight", "head.fc.bias"], name="head.fc", transB=1)
    g.output(y, ["batch", cfg.num_classes])
    return g.model_proto(opset=opset, ir_version=8), w


def torch_grn(x, weight, bias, eps):
    """GRN on a channels-last tensor [N, H, W, C] (timm GlobalResponseNorm / HF ConvNextV2GRN)"""
    import torch

    G = torch.linalg.vector_norm(x, ord=2, dim=(1, 2), keepdim=True)
    nx = G / (G.mean(dim=-1, keepdim=True) + eps)
    return weight * (x * nx) + bias + x


def torch_forward(w: Dict[str, np.ndarray], x, cfg: ConvNeXtV2Config = ConvNeXtV2Config(), device="cpu", dtype=None):
    import torch
    import torch.nn.functional as F

    dtype = dtype or torch.float32
    t = {k: torch.from_numpy(v).to(device=device, dtype=dtype) for k, v in w.items()}
    if not torch.is_tensor(x):
        x = torch.from_numpy(np.asarray(x, np.float32))
    x = x.to(device=device, dtype=dtype)

    def image_ln(z, name):
        C = z.shape[1]
        z = F.layer_norm(z.permute(0, 2, 3, 1), (C,), t[name + ".weight"], t[name + ".bias"], cfg.eps)
        return z.permute(0, 3, 1, 2)

    h = F.conv2d(x, t["stem.conv.weight"], t["stem.conv.bias"], stride=4)
    h = image_ln(h, "stem.norm")
    for s, (depth, C) in enumerate(zip(cfg.depths, cfg.dims)):
        if s > 0:
            h = image_ln(h, "stages.%d.downsample.norm" % s)
            h = F.conv2d(h, t["stages.%d.downsample.conv.weight" % s], t["stages.%d.downsample.conv.bias" % s], stride=2)
        for i in range(depth):
            p = "stages.%d.blocks.%d." % (s, i)
            y = F.conv2d(h, t[p + "dwconv.weight"], t[p + "dwconv.bias"], padding=3, groups=C)
            y = F.layer_norm(y.permute(0, 2, 3, 1), (C,), t[p + "norm.weight"], t[p + "norm.bias"], cfg.eps)
            m = y @ t[p + "pwconv1.weight"] + t[p + "pwconv1.bias"]
            m = 0.5 * m * (1.0 + torch.erf(m / 1.4142135381698608))
            m = torch_grn(m, t[p + "grn.weight"], t[p + "grn.bias"], cfg.grn_eps)
            y = m @ t[p + "pwconv2.weight"] + t[p + "pwconv2.bias"]
            h = y.permute(0, 3, 1, 2) + h
    h = image_ln(h.mean(dim=(2, 3), keepdim=True), "head.norm")
    return F.linear(h.flatten(1), t["head.fc.weight"], t["head.fc.bias"])
