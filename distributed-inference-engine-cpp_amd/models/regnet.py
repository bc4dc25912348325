"""RegNet X / Y ONNX generator + torch fp32 reference (grouped 3x3 convs on the HIP engine's wide-group MFMA kernel).

torchvision-layout blocks: 1x1 -> BN -> ReLU -> grouped 3x3 (carries the stride) -> BN -> ReLU -> [Y only: SE, the
exported GlobalAveragePool -> Conv1x1 -> ReLU -> Conv1x1 -> Sigmoid -> Mul chain, squeezed to a quarter of the
BLOCK INPUT width] -> 1x1 -> BN, then the Add with an identity or projection (1x1 stride s + BN) shortcut and a
ReLU; stem 3x3 / 2 with 32 channels; every stage opens with a stride-2 block.  The bottleneck ratio is 1, so the
grouped conv has the stage's width in groups of `group_width` channels: 24 (X / Y-1.6GF), 48 (X-3.2GF), 56
(Y-8GF) -- and channel counts such as 72, 120, 168, 888 that are no multiple of 16.  Weights are random (no
checkpoint offline); `torch_forward` rebuilds the network from the same arrays and is the oracle.
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Dict, List, Tuple

import numpy as np

from ..utils.onnx_writer import GraphBuilder


@dataclass
class RegNetConfig:
    # per stage: (blocks, width, group width, stride of the first block)
    stages: Tuple[Tuple[int, int, int, int], ...] = ((2, 72, 24, 2), (4, 168, 24, 2), (10, 408, 24, 2), (2, 912, 24, 2))
    se: bool = False
    stem: int = 32
    image: int = 224
    in_ch: int = 3
    num_classes: int = 1000
    seed: int = 0


def _cfg(depths, widths, gw, se):
    return RegNetConfig(stages=tuple((d, w, gw, 2) for d, w in zip(depths, widths)), se=se)


def regnet_x_1_6gf() -> RegNetConfig:
    return _cfg((2, 4, 10, 2), (72, 168, 408, 912), 24, False)


def regnet_y_1_6gf() -> RegNetConfig:
    return _cfg((2, 6, 17, 2), (48, 120, 336, 888), 24, True)


def regnet_x_3_2gf() -> RegNetConfig:
    return _cfg((2, 6, 15, 2), (96, 192, 432, 1008), 48, False)


def regnet_y_8gf() -> RegNetConfig:
    return _cfg((2, 4, 10, 1), (224, 448, 896, 2016), 56, True)


CONFIGS = {"regnet_x_1_6gf": regnet_x_1_6gf, "regnet_y_1_6gf": regnet_y_1_6gf, "regnet_x_3_2gf": regnet_x_3_2gf,
           "regnet_y_8gf": regnet_y_8gf}


def tiny_regnet_config(se: bool = False, seed: int = 0) -> RegNetConfig:
    """One-block stages of width 72, 120, 96, 168, 128 in groups of 24, 40, 48, 56, 64 (five stages, so that every
    group width of the wide-group kernel occurs; 72, 120 and 168 are no multiple of 16) on input maps 16, 16, 8, 4,
    4: three stride-2 grouped convs."""
    return RegNetConfig(stages=((1, 72, 24, 1), (1, 120, 40, 2), (1, 96, 48, 2), (1, 168, 56, 1), (1, 128, 64, 2)),
                        se=se, image=32, num_classes=16, seed=seed)


def _blocks(cfg: RegNetConfig) -> List[dict]:
    out, cin = [], cfg.stem
    for n, width, gw, stride in cfg.stages:
        for i in range(n):
            s = stride if i == 0 else 1
            out.append({"cin": cin, "width": width, "groups": width // gw, "stride": s, "project": s != 1 or cin != width,
                        "se": int(round(0.25 * cin)) if cfg.se else 0})
            cin = width
    return out


def grouped_convs(cfg: RegNetConfig) -> List[dict]:
    """The grouped 3x3 convs in order: input map, channels, groups, stride (tools/gconv_wide_bench.py), and the
    squeezed width of the SE block behind each (0: none)."""
    hw, out = cfg.image // 2, []
    for b in _blocks(cfg):
        out.append({"hw": hw, "C": b["width"], "groups": b["groups"], "stride": b["stride"], "se": b["se"]})
        hw //= b["stride"]
    return out


def make_weights(cfg: RegNetConfig) -> Dict[str, np.ndarray]:
    rng = np.random.default_rng(cfg.seed)
    w: Dict[str, np.ndarray] = {}

    def conv(name, cout, cin_per_group, k, gain=1.0, bias=False):
        std = gain * math.sqrt(2.0 / (cin_per_group * k * k))
        w[name + ".weight"] = rng.normal(0, std, (cout, cin_per_group, k, k)).astype(np.float32)
        if bias:
            w[name + ".bias"] = rng.normal(0, 0.1, cout).astype(np.float32)

    def bn(name, c):
        w[name + ".gamma"] = rng.uniform(0.7, 1.3, c).astype(np.float32)
        w[name + ".beta"] = rng.normal(0, 0.1, c).astype(np.float32)
        w[name + ".mean"] = rng.normal(0, 0.1, c).astype(np.float32)
        w[name + ".var"] = rng.uniform(0.6, 1.4, c).astype(np.float32)

    conv("stem", cfg.stem, cfg.in_ch, 3)
    bn("stem_bn", cfg.stem)
    for i, b in enumerate(_blocks(cfg)):
        p = "block%d." % i
        conv(p + "conv1", b["width"], b["cin"], 1)
        bn(p + "bn1", b["width"])
        conv(p + "conv2", b["width"], b["width"] // b["groups"], 3)
        bn(p + "bn2", b["width"])
        if b["se"]:
            conv(p + "se1", b["se"], b["width"], 1, bias=True)
            conv(p + "se2", b["width"], b["se"], 1, gain=0.7, bias=True)
        conv(p + "conv3", b["width"], b["width"], 1, gain=0.5)
        bn(p + "bn3", b["width"])
        if b["project"]:
            conv(p + "down", b["width"], b["cin"], 1, gain=0.5)
            bn(p + "down_bn", b["width"])
    cl = _blocks(cfg)[-1]["width"]
    w["fc.weight"] = rng.normal(0, 1.0 / math.sqrt(cl), (cfg.num_classes, cl)).astype(np.float32)
    w["fc.bias"] = rng.normal(0, 0.01, cfg.num_classes).astype(np.float32)
    return w


def build_onnx(cfg: RegNetConfig, opset: int = 13) -> Tuple[bytes, Dict[str, np.ndarray]]:
    w = make_weights(cfg)
    g = GraphBuilder(name="regnet")
    for k, v in w.items():
        g.init(k, v)
    x = g.input("input", ["N", cfg.in_ch, cfg.image, cfg.image])

    def conv_bn(inp, name, bn_name, k, stride, group=1):
        y = g.node("Conv", [inp, name + ".weight"], name=name, kernel_shape=[k, k], strides=[stride, stride],
                   pads=[k // 2] * 4, group=group)
        return g.node("BatchNormalization", [y, bn_name + ".gamma", bn_name + ".beta", bn_name + ".mean",
                                             bn_name + ".var"], name=bn_name, epsilon=1e-5)

    h = g.node("Relu", [conv_bn(x, "stem", "stem_bn", 3, 2)], name="stem_relu")
    for i, b in enumerate(_blocks(cfg)):
        p = "block%d." % i
        y = g.node("Relu", [conv_bn(h, p + "conv1", p + "bn1", 1, 1)], name=p + "relu1")
        y = g.node("Relu", [conv_bn(y, p + "conv2", p + "bn2", 3, b["stride"], group=b["groups"])], name=p + "relu2")
        if b["se"]:
            z = g.node("GlobalAveragePool", [y], name=p + "se_pool")
            z = g.node("Conv", [z, p + "se1.weight", p + "se1.bias"], name=p + "se1", kernel_shape=[1, 1])
            z = g.node("Relu", [z], name=p + "se1_relu")
            z = g.node("Conv", [z, p + "se2.weight", p + "se2.bias"], name=p + "se2", kernel_shape=[1, 1])
            z = g.node("Sigmoid", [z], name=p + "se_gate")
            y = g.node("Mul", [z, y], name=p + "se_scale")
        y = conv_bn(y, p + "conv3", p + "bn3", 1, 1)
        sc = conv_bn(h, p + "down", p + "down_bn", 1, b["stride"]) if b["project"] else h
        h = g.node("Relu", [g.node("Add", [sc, y], name=p + "add")], name=p + "relu3")
    h = g.node("GlobalAveragePool", [h], name="gap")
    h = g.node("Flatten", [h], name="flatten", axis=1)
    y = g.node("Gemm", [h, "fc.weight", "fc.bias"], name="fc", transB=1)
    g.output(y, ["N", cfg.num_classes])
    return g.model_proto(opset=opset, ir_version=7), w


def torch_forward(w: Dict[str, np.ndarray], x, cfg: RegNetConfig, device="cpu", dtype=None):
    import torch
    import torch.nn.functional as F

    dtype = dtype or torch.float32
    t = {k: torch.from_numpy(v).to(device=device, dtype=dtype) for k, v in w.items()}
    if not torch.is_tensor(x):
        x = torch.from_numpy(np.asarray(x, np.float32))
    x = x.to(device=device, dtype=dtype)

    def conv_bn(inp, name, bn, k, stride, group=1):
        y = F.conv2d(inp, t[name + ".weight"], stride=stride, padding=k // 2, groups=group)
        return F.batch_norm(y, t[bn + ".mean"], t[bn + ".var"], t[bn + ".gamma"], t[bn + ".beta"], False, 0.0, 1e-5)

    h = torch.relu(conv_bn(x, "stem", "stem_bn", 3, 2))
    for i, b in enumerate(_blocks(cfg)):
        p = "block%d." % i
        y = torch.relu(conv_bn(h, p + "conv1", p + "bn1", 1, 1))
        y = torch.relu(conv_bn(y, p + "conv2", p + "bn2", 3, b["stride"], group=b["groups"]))
        if b["se"]:
            z = y.mean(dim=(2, 3), keepdim=True)
            z = torch.relu(F.conv2d(z, t[p + "se1.weight"], t[p + "se1.bias"]))
            y = y * torch.sigmoid(F.conv2d(z, t[p + "se2.weight"], t[p + "se2.bias"]))
        y = conv_bn(y, p + "conv3", p + "bn3", 1, 1)
        sc = conv_bn(h, p + "down", p + "down_bn", 1, b["stride"]) if b["project"] else h
        h = torch.relu(sc + y)
    return F.linear(h.mean(dim=(2, 3)), t["fc.weight"], t["fc.bias"])


def synthetic_input(batch: int, cfg: RegNetConfig, seed: int = 1) -> np.ndarray:
    rng = np.random.default_rng(seed)
    return np.round(rng.random((batch, cfg.in_ch, cfg.image, cfg.image), dtype=np.float32), 4).astype(np.float32)
