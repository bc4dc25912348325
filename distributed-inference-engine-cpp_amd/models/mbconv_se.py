"""MBConv models with squeeze-excitation: one table-driven ONNX generator + torch fp32 oracle for
  * EfficientNet-B0 in the torchvision layout: SiLU (exported Mul(x, Sigmoid(x))) behind every conv but the
    projections, SE of a quarter of the BLOCK INPUT channels with SiLU inside and a Sigmoid gate;
  * MobileNetV3-Large in the torchvision layout: ReLU / HardSwish blocks, SE of a quarter of the expanded
    channels (rounded to 8) with ReLU inside and a HardSigmoid(1/6, 0.5) gate, Linear + HardSwish + Linear head.
Both pad symmetrically ((k - 1) / 2), as torchvision does.  The SE block is the exported
GlobalAveragePool -> Conv1x1 -> act -> Conv1x1 -> gate -> Mul chain, which the HIP planner lowers to one `se` op
(kernels/se.hip); the activations go into the conv epilogues.  Weights are random (no checkpoint offline);
`torch_forward` rebuilds the network from the same arrays and is the oracle.
"""
from __future__ import annotations

import math
from dataclasses import dataclass, field
from typing import Dict, List, Tuple

import numpy as np

from ..utils.onnx_writer import GraphBuilder
from .efficientnet_lite import SETTINGS as B0_SETTINGS

# MobileNetV3-Large: (window k, expanded channels, output channels, SE, activation, stride)
V3_LARGE = [(3, 16, 16, 0, "relu", 1), (3, 64, 24, 0, "relu", 2), (3, 72, 24, 0, "relu", 1), (5, 72, 40, 1, "relu", 2),
            (5, 120, 40, 1, "relu", 1), (5, 120, 40, 1, "relu", 1), (3, 240, 80, 0, "hardswish", 2),
            (3, 200, 80, 0, "hardswish", 1), (3, 184, 80, 0, "hardswish", 1), (3, 184, 80, 0, "hardswish", 1),
            (3, 480, 112, 1, "hardswish", 1), (3, 672, 112, 1, "hardswish", 1), (5, 672, 160, 1, "hardswish", 2),
            (5, 960, 160, 1, "hardswish", 1), (5, 960, 160, 1, "hardswish", 1)]


@dataclass
class MbconvSeConfig:
    arch: str = "efficientnet_b0"  # or "mobilenet_v3_large"
    image: int = 224
    in_ch: int = 3
    num_classes: int = 1000
    seed: int = 0
    # rows (k, expanded, out, squeeze channels or 0, act, stride); empty: the arch's full table
    rows: List[tuple] = field(default_factory=list)
    stem: int = 0     # 0: the arch's (32 / 16)
    last: int = 0     # channels of the last 1x1 conv (0: 1280 / 960)
    hidden: int = 0   # MobileNetV3: width of the classifier's first Linear (0: 1280)


def _is_b0(cfg: MbconvSeConfig) -> bool:
    if cfg.arch not in ("efficientnet_b0", "mobilenet_v3_large"):
        raise ValueError("unknown arch " + cfg.arch)
    return cfg.arch == "efficientnet_b0"


def _make_divisible(v: float, divisor: int = 8) -> int:
    """torchvision's rounding of channel counts: to the nearest multiple, never more than 10 % down"""
    new_v = max(divisor, int(v + divisor / 2) // divisor * divisor)
    return new_v + divisor if new_v < 0.9 * v else new_v


def _rows(cfg: MbconvSeConfig) -> List[tuple]:
    if cfg.rows:
        return list(cfg.rows)
    if not _is_b0(cfg):
        return [(k, e, c, _make_divisible(e // 4) if se else 0, act, s) for k, e, c, se, act, s in V3_LARGE]
    out, cin = [], 32
    for t, k, s, c, n in B0_SETTINGS:
        for i in range(n):
            out.append((k, cin * t, c, max(1, cin // 4), "silu", s if i == 0 else 1))
            cin = c
    return out


def tiny_config(arch: str, seed: int = 0) -> MbconvSeConfig:
    """32x32 input, a few blocks, every activation / SE variant of the arch at least once."""
    if arch == "efficientnet_b0":
        rows = [(3, 32, 16, 8, "silu", 1), (3, 96, 24, 4, "silu", 2), (5, 144, 24, 6, "silu", 1)]
        return MbconvSeConfig(arch, 32, 3, 10, seed, rows, 32, 128)
    rows = [(3, 16, 16, 0, "relu", 1), (3, 64, 24, 0, "relu", 2), (5, 72, 40, 24, "relu", 2), (3, 120, 40, 16, "hardswish", 1),
            (3, 240, 80, 0, "hardswish", 1)]
    return MbconvSeConfig(arch, 32, 3, 10, seed, rows, 16, 160, 128)


def _dims(cfg: MbconvSeConfig):
    b0 = _is_b0(cfg)
    return (cfg.stem or (32 if b0 else 16), cfg.last or (1280 if b0 else 960), cfg.hidden or 1280)


def se_shapes(cfg: MbconvSeConfig) -> List[Tuple[int, int, int]]:
    """(map side, C, Cr) of every SE block, in order."""
    side, out = cfg.image // 2, []
    for k, e, c, sq, act, s in _rows(cfg):
        side = (side + 2 * (k // 2) - k) // s + 1
        if sq:
            out.append((side, e, sq))
    return out


def make_weights(cfg: MbconvSeConfig) -> Dict[str, np.ndarray]:
    rng = np.random.default_rng(cfg.seed)
    w: Dict[str, np.ndarray] = {}
    stem, last, hidden = _dims(cfg)

    def conv_bn(name, cout, cin_per_group, k, gain=1.0):
        std = gain * math.sqrt(2.0 / (cin_per_group * k * k))
        w[name + ".weight"] = rng.normal(0, std, (cout, cin_per_group, k, k)).astype(np.float32)
        w[name + "_bn.gamma"] = rng.uniform(0.7, 1.3, cout).astype(np.float32)
        w[name + "_bn.beta"] = rng.normal(0, 0.1, cout).astype(np.float32)
        w[name + "_bn.mean"] = rng.normal(0, 0.1, cout).astype(np.float32)
        w[name + "_bn.var"] = rng.uniform(0.6, 1.4, cout).astype(np.float32)

    def fc(name, cout, cin, shape):
        w[name + ".weight"] = rng.normal(0, 1.0 / math.sqrt(cin), shape).astype(np.float32)
        w[name + ".bias"] = rng.normal(0, 0.2, cout).astype(np.float32)

    conv_bn("stem", stem, cfg.in_ch, 3)
    cin = stem
    for i, (k, e, c, sq, act, s) in enumerate(_rows(cfg)):
        p = "block%d." % i
        if e != cin:
            conv_bn(p + "expand", e, cin, 1)
        conv_bn(p + "dw", e, 1, k)
        if sq:
            fc(p + "se1", sq, e, (sq, e, 1, 1))
            fc(p + "se2", e, sq, (e, sq, 1, 1))
        conv_bn(p + "project", c, e, 1, gain=0.5)
        cin = c
    conv_bn("head", last, cin, 1)
    if not _is_b0(cfg):
        fc("fc0", hidden, last, (hidden, last))
        last = hidden
    fc("fc", cfg.num_classes, last, (cfg.num_classes, last))
    return w


def build_onnx(cfg: MbconvSeConfig = MbconvSeConfig(), opset: int = 14) -> Tuple[bytes, Dict[str, np.ndarray]]:
    w = make_weights(cfg)
    b0 = _is_b0(cfg)
    g = GraphBuilder(name=cfg.arch)
    for k, v in w.items():
        g.init(k, v)
    x = g.input("input", ["N", cfg.in_ch, cfg.image, cfg.image])

    def act_node(y, act, name):
        if act == "relu":
            return g.node("Relu", [y], name=name + "_relu")
        if act == "hardswish":
            return g.node("HardSwish", [y], name=name + "_hswish")
        if act == "silu":
            return g.node("Mul", [y, g.node("Sigmoid", [y], name=name + "_sigmoid")], name=name + "_silu")
        return y

    def conv_bn(inp, name, k, stride, act, group=1):
        y = g.node("Conv", [inp, name + ".weight"], name=name, kernel_shape=[k, k], strides=[stride, stride],
                   pads=[k // 2] * 4, group=group)
        bn = name + "_bn"
        y = g.node("BatchNormalization", [y, bn + ".gamma", bn + ".beta", bn + ".mean", bn + ".var"], name=bn, epsilon=1e-5)
        return act_node(y, act, name)

    h = conv_bn(x, "stem", 3, 2, "silu" if b0 else "hardswish")
    cin = _dims(cfg)[0]
    for i, (k, e, c, sq, act, s) in enumerate(_rows(cfg)):
        p = "block%d." % i
        y = h
        if e != cin:
            y = conv_bn(y, p + "expand", 1, 1, act)
        y = conv_bn(y, p + "dw", k, s, act, group=e)
        if sq:
            z = g.node("GlobalAveragePool", [y], name=p + "se_pool")
            z = g.node("Conv", [z, p + "se1.weight", p + "se1.bias"], name=p + "se1", kernel_shape=[1, 1])
            z = act_node(z, "silu" if b0 else "relu", p + "se1")
            z = g.node("Conv", [z, p + "se2.weight", p + "se2.bias"], name=p + "se2", kernel_shape=[1, 1])
            if b0:
                z = g.node("Sigmoid", [z], name=p + "se_gate")
            else:
                z = g.node("HardSigmoid", [z], name=p + "se_gate", alpha=1.0 / 6.0, beta=0.5)
            y = g.node("Mul", [z, y] if i % 2 else [y, z], name=p + "se_scale")  # both operand orders
        y = conv_bn(y, p + "project", 1, 1, None)
        if s == 1 and cin == c:
            y = g.node("Add", [y, h], name=p + "residual")
        h, cin = y, c
    h = conv_bn(h, "head", 1, 1, "silu" if b0 else "hardswish")
    h = g.node("GlobalAveragePool", [h], name="gap")
    h = g.node("Flatten", [h], name="flatten", axis=1)
    if not b0:
        h = g.node("Gemm", [h, "fc0.weight", "fc0.bias"], name="fc0", transB=1)
        h = g.node("HardSwish", [h], name="fc0_hswish")
    y = g.node("Gemm", [h, "fc.weight", "fc.bias"], name="fc", transB=1)
    g.output(y, ["N", cfg.num_classes])
    return g.model_proto(opset=opset, ir_version=7), w


def torch_forward(w: Dict[str, np.ndarray], x, cfg: MbconvSeConfig = MbconvSeConfig(), device="cpu", dtype=None):
    import torch
    import torch.nn.functional as F

    dtype = dtype or torch.float32
    t = {k: torch.from_numpy(v).to(device=device, dtype=dtype) for k, v in w.items()}
    if not torch.is_tensor(x):
        x = torch.from_numpy(np.asarray(x, np.float32))
    x = x.to(device=device, dtype=dtype)
    b0 = _is_b0(cfg)
    acts = {"relu": F.relu, "hardswish": F.hardswish, "silu": F.silu, None: lambda v: v}

    def conv_bn(inp, name, k, stride, act, group=1):
        y = F.conv2d(inp, t[name + ".weight"], stride=stride, padding=k // 2, groups=group)
        bn = name + "_bn"
        return acts[act](F.batch_norm(y, t[bn + ".mean"], t[bn + ".var"], t[bn + ".gamma"], t[bn + ".beta"], False, 0.0, 1e-5))

    h = conv_bn(x, "stem", 3, 2, "silu" if b0 else "hardswish")
    cin = _dims(cfg)[0]
    for i, (k, e, c, sq, act, s) in enumerate(_rows(cfg)):
        p = "block%d." % i
        y = h
        if e != cin:
            y = conv_bn(y, p + "expand", 1, 1, act)
        y = conv_bn(y, p + "dw", k, s, act, group=e)
        if sq:
            z = y.mean(dim=(2, 3), keepdim=True)
            z = acts["silu" if b0 else "relu"](F.conv2d(z, t[p + "se1.weight"], t[p + "se1.bias"]))
            z = F.conv2d(z, t[p + "se2.weight"], t[p + "se2.bias"])
            y = y * (torch.sigmoid(z) if b0 else F.hardsigmoid(z))
        y = conv_bn(y, p + "project", 1, 1, None)
        if s == 1 and cin == c:
            y = y + h
        h, cin = y, c
    h = conv_bn(h, "head", 1, 1, "silu" if b0 else "hardswish").mean(dim=(2, 3))
    if not b0:
        h = F.hardswish(F.linear(h, t["fc0.weight"], t["fc0.bias"]))
    return F.linear(h, t["fc.weight"], t["fc.bias"])


def synthetic_input(batch: int, cfg: MbconvSeConfig = MbconvSeConfig(), seed: int = 1) -> np.ndarray:
    rng = np.random.default_rng(seed)
    return np.round(rng.random((batch, cfg.in_ch, cfg.image, cfg.image), dtype=np.float32), 4).astype(np.float32)
