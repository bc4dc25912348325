"""ConvNeXt ONNX generator + torch reference (channels-last blocks, 7x7 depthwise convs).

Graph layout follows a timm / current HuggingFace `ConvNextForImageClassification` export at opset 17:
  stem:       Conv 4x4/4 (bias) -> Transpose(0,2,3,1) -> LayerNormalization(axis -1) -> Transpose(0,3,1,2)
  block:      Conv 7x7 pad 3 group=C (bias) -> Transpose(0,2,3,1) -> LayerNormalization
              -> MatMul [C,4C] + Add -> GELU(erf: Div, Erf, Add, Mul, Mul) -> MatMul [4C,C] + Add
              -> Mul(gamma [C]) -> Transpose(0,3,1,2) -> Add(shortcut)
  downsample: Transpose / LayerNormalization / Transpose -> Conv 2x2/2 (bias)
  head:       GlobalAveragePool -> Transpose / LayerNormalization / Transpose on [N,C,1,1] -> Flatten -> Gemm
Weights are random (no checkpoint offline); `torch_forward` rebuilds the network from the same
arrays and is the oracle.  The layer-scale init is 1.0 (timm's 1e-6 would hide the MLP branch from
every output check).

Export variants: `channels_first_ln` writes the stem, downsample and head LayerNorms the way older
HF exports do, decomposed over axis 1 of the NCHW map (ReduceMean(axes [1]), Sub, Pow, ReduceMean,
Add, Sqrt, Div, Mul(w [C,1,1]), Add(b [C,1,1])); `reduce_mean_head` pools with
ReduceMean(axes [2,3], keepdims 1) instead of GlobalAveragePool.
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Dict, Tuple

import numpy as np

from ..utils.onnx_writer import GraphBuilder


@dataclass
class ConvNeXtConfig:
    image: int = 224
    in_ch: int = 3
    depths: Tuple[int, ...] = (3, 3, 9, 3)
    dims: Tuple[int, ...] = (96, 192, 384, 768)
    num_classes: int = 1000
    eps: float = 1e-6
    layer_scale: float = 1.0
    seed: int = 0
    channels_first_ln: bool = False
    reduce_mean_head: bool = False


def tiny_convnext_config(seed: int = 0, **kw) -> ConvNeXtConfig:
    # maps 8 / 4 / 2 / 1: a partial tile, maps smaller than the 7x7 window and a 1x1 map
    return ConvNeXtConfig(image=32, depths=(1, 1, 2, 1), dims=(16, 32, 64, 128), num_classes=16, seed=seed, **kw)


# the export forms the planner tests run over
SPECS = {
    "timm": {},
    "channels_first_ln": {"channels_first_ln": True},
    "reduce_mean_head": {"reduce_mean_head": True},
}


def make_weights(cfg: ConvNeXtConfig) -> Dict[str, np.ndarray]:
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
            lin(p + "pwconv2", 4 * C, C, 0.5 / math.sqrt(4 * C))
            w[p + "gamma"] = (cfg.layer_scale * rng.uniform(0.5, 1.5, C)).astype(np.float32)
    ln("head.norm", cfg.dims[-1])
    w["head.fc.weight"] = rng.normal(0, 1.0 / math.sqrt(cfg.dims[-1]), (cfg.num_classes, cfg.dims[-1])).astype(np.float32)
    w["head.fc.bias"] = rng.normal(0, 0.01, cfg.num_classes).astype(np.float32)
    return w


def build_onnx(cfg: ConvNeXtConfig = ConvNeXtConfig(), opset: int = 17) -> Tuple[bytes, Dict[str, np.ndarray]]:
    w = make_weights(cfg)
    g = GraphBuilder(name="convnext")
    for k, v in w.items():
        g.init(k, v)
    x = g.input("pixel_values", ["batch", cfg.in_ch, cfg.image, cfg.image])
    sqrt2 = g.const(np.array(1.4142135381698608, np.float32), "sqrt2")
    one = g.const(np.array(1.0, np.float32), "one")
    half = g.const(np.array(0.5, np.float32), "half")
    two = g.const(np.array(2.0, np.float32), "two")
    eps_c = g.const(np.array(cfg.eps, np.float32), "ln_eps")

    def rows_ln(inp, wname, name):
        return g.node("LayerNormalization", [inp, wname + ".weight", wname + ".bias"], name=name, axis=-1,
                      epsilon=cfg.eps)

    def image_ln(inp, wname, name):
        """LayerNorm over the channels of an NCHW map"""
        if not cfg.channels_first_ln:
            t = g.node("Transpose", [inp], name=name + "/to_nhwc", perm=[0, 2, 3, 1])
            t = rows_ln(t, wname, name)
            return g.node("Transpose", [t], name=name + "/to_nchw", perm=[0, 3, 1, 2])
        C = w[wname + ".weight"].shape[0]
        wc = g.const(w[wname + ".weight"].reshape(C, 1, 1), name + "/w")
        bc = g.const(w[wname + ".bias"].reshape(C, 1, 1), name + "/b")
        mu = g.node("ReduceMean", [inp], name=name + "/mean", axes=[1], keepdims=1)
        d = g.node("Sub", [inp, mu], name=name + "/sub")
        var = g.node("ReduceMean", [g.node("Pow", [d, two], name=name + "/pow")], name=name + "/var", axes=[1],
                     keepdims=1)
        sd = g.node("Sqrt", [g.node("Add", [var, eps_c], name=name + "/add_eps")], name=name + "/sqrt")
        y = g.node("Div", [d, sd], name=name + "/div")
        y = g.node("Mul", [y, wc], name=name + "/scale")
        return g.node("Add", [y, bc], name=name + "/shift")

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
            y = rows_ln(y, p + "norm", p + "norm")
            m = linear(y, p + "pwconv1")
            t = g.node("Div", [m, sqrt2], name=p + "gelu/div")
            t = g.node("Erf", [t], name=p + "gelu/erf")
            t = g.node("Add", [t, one], name=p + "gelu/add")
            t = g.node("Mul", [m, t], name=p + "gelu/mul")
            t = g.node("Mul", [t, half], name=p + "gelu/half")
            y = linear(t, p + "pwconv2")
            y = g.node("Mul", [y, p + "gamma"], name=p + "layer_scale")
            y = g.node("Transpose", [y], name=p + "to_nchw", perm=[0, 3, 1, 2])
            h = g.node("Add", [y, h], name=p + "residual")
    if cfg.reduce_mean_head:
        h = g.node("ReduceMean", [h], name="head.pool", axes=[2, 3], keepdims=1)
    else:
        h = g.node("GlobalAveragePool", [h], name="head.pool")
    h = image_ln(h, "head.norm", "head.norm")
    h = g.node("Flatten", [h], name="head.flatten", axis=1)
    y = g.node("Gemm", [h, "head.fc.weight", "head.fc.bias"], name="head.fc", transB=1)
    g.output(y, ["batch", cfg.num_classes])
    return g.model_proto(opset=opset, ir_version=8), w


def torch_forward(w: Dict[str, np.ndarray], x, cfg: ConvNeXtConfig = ConvNeXtConfig(), device="cpu", dtype=None):
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
            y = (m @ t[p + "pwconv2.weight"] + t[p + "pwconv2.bias"]) * t[p + "gamma"]
            h = y.permute(0, 3, 1, 2) + h
    h = image_ln(h.mean(dim=(2, 3), keepdim=True), "head.norm")
    return F.linear(h.flatten(1), t["head.fc.weight"], t["head.fc.bias"])


def synthetic_input(batch: int, cfg: ConvNeXtConfig = ConvNeXtConfig(), seed: int = 1) -> np.ndarray:
    rng = np.random.default_rng(seed)
    x = rng.random((batch, cfg.in_ch, cfg.image, cfg.image), dtype=np.float32) * 2 - 1
    return np.round(x, 4).astype(np.float32)
