"""EfficientNet-Lite0 ONNX generator + torch fp32 reference: the ReLU6, no-squeeze-excitation member of the
EfficientNet family (MBConv stages with depthwise 3x3 / 5x5 convs at strides 1 and 2, Clip(0, 6), inverted-
residual Adds, GAP + FC; stem and head widths fixed as in the Lite models).  Stride-2 depthwise convs carry the
TF "SAME" pads of an even map ([0, 0, 1, 1] for 3x3, [1, 1, 2, 2] for 5x5).  On the HIP engine the 5x5 stride-1
convs run on the tiled kernel (kernels/dwconv.hip), every other depthwise conv on the polyphase kernel
(kernels/dwconv_poly.hip).  Weights are random (no checkpoint offline); `torch_forward` rebuilds the network
from the same arrays and is the oracle.
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Dict, List, Tuple

import numpy as np

from ..utils.onnx_writer import GraphBuilder
from .mobilenet import _div8

# (expansion t, window k, stride s, channels c, repeats n) of EfficientNet-B0 / Lite0
SETTINGS = [(1, 3, 1, 16, 1), (6, 3, 2, 24, 2), (6, 5, 2, 40, 2), (6, 3, 2, 80, 3), (6, 5, 1, 112, 3), (6, 5, 2, 192, 4),
            (6, 3, 1, 320, 1)]


@dataclass
class EfficientNetLiteConfig:
    width: float = 1.0
    image: int = 224
    in_ch: int = 3
    num_classes: int = 1000
    stem: int = 32
    last: int = 1280
    seed: int = 0


def tiny_efficientnet_lite_config(seed: int = 0) -> EfficientNetLiteConfig:
    return EfficientNetLiteConfig(width=0.5, image=64, num_classes=10, last=256, seed=seed)


def _blocks(cfg: EfficientNetLiteConfig) -> List[dict]:
    out, cin = [], cfg.stem
    for t, k, s, c, n in SETTINGS:
        cout = _div8(c * cfg.width)
        for i in range(n):
            stride = s if i == 0 else 1
            pads = [k // 2] * 4 if stride == 1 else [k // 2 - 1, k // 2 - 1, k // 2, k // 2]
            out.append({"t": t, "k": k, "cin": cin, "cout": cout, "stride": stride, "hidden": cin * t, "pads": pads})
            cin = cout
    return out


def make_weights(cfg: EfficientNetLiteConfig) -> Dict[str, np.ndarray]:
    rng = np.random.default_rng(cfg.seed)
    w: Dict[str, np.ndarray] = {}

    def conv_bn(name, cout, cin_per_group, k, gain=1.0):
        std = gain * math.sqrt(2.0 / (cin_per_group * k * k))
        w[name + ".weight"] = rng.normal(0, std, (cout, cin_per_group, k, k)).astype(np.float32)
        w[name + "_bn.gamma"] = rng.uniform(0.7, 1.3, cout).astype(np.float32)
        w[name + "_bn.beta"] = rng.normal(0, 0.1, cout).astype(np.float32)
        w[name + "_bn.mean"] = rng.normal(0, 0.1, cout).astype(np.float32)
        w[name + "_bn.var"] = rng.uniform(0.6, 1.4, cout).astype(np.float32)

    conv_bn("stem", cfg.stem, cfg.in_ch, 3)
    for i, b in enumerate(_blocks(cfg)):
        p = "block%d." % i
        if b["t"] != 1:
            conv_bn(p + "expand", b["hidden"], b["cin"], 1)
        conv_bn(p + "dw", b["hidden"], 1, b["k"])
        conv_bn(p + "project", b["cout"], b["hidden"], 1, gain=0.5)
    conv_bn("head", cfg.last, _blocks(cfg)[-1]["cout"], 1)
    w["fc.weight"] = rng.normal(0, 1.0 / math.sqrt(cfg.last), (cfg.num_classes, cfg.last)).astype(np.float32)
    w["fc.bias"] = rng.normal(0, 0.01, cfg.num_classes).astype(np.float32)
    return w


def build_onnx(cfg: EfficientNetLiteConfig = EfficientNetLiteConfig(), opset: int = 13) -> Tuple[bytes, Dict[str, np.ndarray]]:
    w = make_weights(cfg)
    g = GraphBuilder(name="efficientnet_lite0")
    for k, v in w.items():
        g.init(k, v)
    lo = g.const(np.array(0.0, np.float32), "clip_min")
    hi = g.const(np.array(6.0, np.float32), "clip_max")
    x = g.input("input", ["N", cfg.in_ch, cfg.image, cfg.image])

    def conv_bn(inp, name, k, stride, pads, group=1, relu6=True):
        y = g.node("Conv", [inp, name + ".weight"], name=name, kernel_shape=[k, k], strides=[stride, stride], pads=pads,
                   group=group)
        bn = name + "_bn"
        y = g.node("BatchNormalization", [y, bn + ".gamma", bn + ".beta", bn + ".mean", bn + ".var"], name=bn, epsilon=1e-5)
        return g.node("Clip", [y, lo, hi], name=name + "_relu6") if relu6 else y

    h = conv_bn(x, "stem", 3, 2, [1, 1, 1, 1])
    for i, b in enumerate(_blocks(cfg)):
        p = "block%d." % i
        y = h
        if b["t"] != 1:
            y = conv_bn(y, p + "expand", 1, 1, [0, 0, 0, 0])
        y = conv_bn(y, p + "dw", b["k"], b["stride"], b["pads"], group=b["hidden"])
        y = conv_bn(y, p + "project", 1, 1, [0, 0, 0, 0], relu6=False)
        if b["stride"] == 1 and b["cin"] == b["cout"]:
            y = g.node("Add", [y, h], name=p + "residual")
        h = y
    h = conv_bn(h, "head", 1, 1, [0, 0, 0, 0])
    h = g.node("GlobalAveragePool", [h], name="gap")
    h = g.node("Flatten", [h], name="flatten", axis=1)
    y = g.node("Gemm", [h, "fc.weight", "fc.bias"], name="fc", transB=1)
    g.output(y, ["N", cfg.num_classes])
    return g.model_proto(opset=opset, ir_version=7), w


def torch_forward(w: Dict[str, np.ndarray], x, cfg: EfficientNetLiteConfig = EfficientNetLiteConfig(), device="cpu",
                  dtype=None):
    import torch
    import torch.nn.functional as F

    dtype = dtype or torch.float32
    t = {k: torch.from_numpy(v).to(device=device, dtype=dtype) for k, v in w.items()}
    if not torch.is_tensor(x):
        x = torch.from_numpy(np.asarray(x, np.float32))
    x = x.to(device=device, dtype=dtype)

    def conv_bn(inp, name, stride, pads, group=1, relu6=True):
        inp = F.pad(inp, (pads[1], pads[3], pads[0], pads[2]))  # ONNX [top, left, bottom, right]
        y = F.conv2d(inp, t[name + ".weight"], stride=stride, groups=group)
        bn = name + "_bn"
        y = F.batch_norm(y, t[bn + ".mean"], t[bn + ".var"], t[bn + ".gamma"], t[bn + ".beta"], False, 0.0, 1e-5)
        return torch.clamp(y, 0, 6) if relu6 else y

    h = conv_bn(x, "stem", 2, [1, 1, 1, 1])
    for i, b in enumerate(_blocks(cfg)):
        p = "block%d." % i
        y = h
        if b["t"] != 1:
            y = conv_bn(y, p + "expand", 1, [0, 0, 0, 0])
        y = conv_bn(y, p + "dw", b["stride"], b["pads"], group=b["hidden"])
        y = conv_bn(y, p + "project", 1, [0, 0, 0, 0], relu6=False)
        if b["stride"] == 1 and b["cin"] == b["cout"]:
            y = y + h
        h = y
    h = conv_bn(h, "head", 1, [0, 0, 0, 0])
    return F.linear(h.mean(dim=(2, 3)), t["fc.weight"], t["fc.bias"])


def synthetic_input(batch: int, cfg: EfficientNetLiteConfig = EfficientNetLiteConfig(), seed: int = 1) -> np.ndarray:
    rng = np.random.default_rng(seed)
    return np.round(rng.random((batch, cfg.in_ch, cfg.image, cfg.image), dtype=np.float32), 4).astype(np.float32)
