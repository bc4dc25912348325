"""ResNeXt ONNX generator + torch fp32 reference (grouped 3x3 convs on the HIP engine's MFMA kernel).

torchvision-layout bottlenecks: 1x1 -> BN -> ReLU -> grouped 3x3 (carries the stride) -> BN -> ReLU -> 1x1 -> BN,
then the Add with an identity or projection (1x1 + BN) shortcut and a ReLU.  The grouped conv has
width = planes * base_width / 64 * cardinality channels in `cardinality` groups: ResNeXt-50 32x4d has group
widths 4, 8, 16, 32 over its four stages and three stride-2 grouped convs.  Weights are random (no checkpoint
offline); `torch_forward` rebuilds the network from the same arrays and is the oracle.
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Dict, List, Tuple

import numpy as np

from ..utils.onnx_writer import GraphBuilder


@dataclass
class ResNeXtConfig:
    stages: Tuple[int, ...] = (3, 4, 6, 3)
    cardinality: int = 32
    base_width: int = 4
    stem: int = 64
    image: int = 224
    in_ch: int = 3
    num_classes: int = 1000
    seed: int = 0


def tiny_resnext_config(seed: int = 0) -> ResNeXtConfig:
    """Grouped widths 32, 64, 128, 256 in 8 groups: group widths 4, 8, 16, 32, on input maps 8, 8, 4, 2."""
    return ResNeXtConfig(stages=(1, 1, 1, 1), cardinality=8, base_width=4, image=32, num_classes=16, seed=seed)


def _blocks(cfg: ResNeXtConfig) -> List[dict]:
    out, cin = [], cfg.stem
    for s, n in enumerate(cfg.stages):
        planes = 64 << s
        width = planes * cfg.base_width // 64 * cfg.cardinality
        for i in range(n):
            stride = 2 if (i == 0 and s > 0) else 1
            out.append({"cin": cin, "width": width, "cout": planes * 4, "stride": stride,
                        "project": stride != 1 or cin != planes * 4})
            cin = planes * 4
    return out


def grouped_convs(cfg: ResNeXtConfig = ResNeXtConfig()) -> List[dict]:
    """The grouped 3x3 convs in order: input map, channels, groups, stride (tools/gconv_bench.py)."""
    hw, out = cfg.image // 4, []
    for b in _blocks(cfg):
        out.append({"hw": hw, "C": b["width"], "groups": cfg.cardinality, "stride": b["stride"]})
        hw //= b["stride"]
    return out


def make_weights(cfg: ResNeXtConfig) -> Dict[str, np.ndarray]:
    rng = np.random.default_rng(cfg.seed)
    w: Dict[str, np.ndarray] = {}

    def conv(name, cout, cin_per_group, k, gain=1.0):
        std = gain * math.sqrt(2.0 / (cin_per_group * k * k))
        w[name + ".weight"] = rng.normal(0, std, (cout, cin_per_group, k, k)).astype(np.float32)

    def bn(name, c):
        w[name + ".gamma"] = rng.uniform(0.7, 1.3, c).astype(np.float32)
        w[name + ".beta"] = rng.normal(0, 0.1, c).astype(np.float32)
        w[name + ".mean"] = rng.normal(0, 0.1, c).astype(np.float32)
        w[name + ".var"] = rng.uniform(0.6, 1.4, c).astype(np.float32)

    conv("stem", cfg.stem, cfg.in_ch, 7)
    bn("stem_bn", cfg.stem)
    for i, b in enumerate(_blocks(cfg)):
        p = "block%d." % i
        conv(p + "conv1", b["width"], b["cin"], 1)
        bn(p + "bn1", b["width"])
        conv(p + "conv2", b["width"], b["width"] // cfg.cardinality, 3)
        bn(p + "bn2", b["width"])
        conv(p + "conv3", b["cout"], b["width"], 1, gain=0.5)
        bn(p + "bn3", b["cout"])
        if b["project"]:
            conv(p + "down", b["cout"], b["cin"], 1, gain=0.5)
            bn(p + "down_bn", b["cout"])
    cl = _blocks(cfg)[-1]["cout"]
    w["fc.weight"] = rng.normal(0, 1.0 / math.sqrt(cl), (cfg.num_classes, cl)).astype(np.float32)
    w["fc.bias"] = rng.normal(0, 0.01, cfg.num_classes).astype(np.float32)
    return w


def build_onnx(cfg: ResNeXtConfig = ResNeXtConfig(), opset: int = 13) -> Tuple[bytes, Dict[str, np.ndarray]]:
    w = make_weights(cfg)
    g = GraphBuilder(name="resnext")
    for k, v in w.items():
        g.init(k, v)
    x = g.input("input", ["N", cfg.in_ch, cfg.image, cfg.image])

    def conv_bn(inp, name, bn_name, k, stride, group=1):
        y = g.node("Conv", [inp, name + ".weight"], name=name, kernel_shape=[k, k], strides=[stride, stride],
                   pads=[k // 2] * 4, group=group)
        return g.node("BatchNormalization", [y, bn_name + ".gamma", bn_name + ".beta", bn_name + ".mean",
                                             bn_name + ".var"], name=bn_name, epsilon=1e-5)

    h = g.node("Relu", [conv_bn(x, "stem", "stem_bn", 7, 2)], name="stem_relu")
    h = g.node("MaxPool", [h], name="stem_pool", kernel_shape=[3, 3], strides=[2, 2], pads=[1, 1, 1, 1])
    for i, b in enumerate(_blocks(cfg)):
        p = "block%d." % i
        y = g.node("Relu", [conv_bn(h, p + "conv1", p + "bn1", 1, 1)], name=p + "relu1")
        y = g.node("Relu", [conv_bn(y, p + "conv2", p + "bn2", 3, b["stride"], group=cfg.cardinality)], name=p + "relu2")
        y = conv_bn(y, p + "conv3", p + "bn3", 1, 1)
        sc = conv_bn(h, p + "down", p + "down_bn", 1, b["stride"]) if b["project"] else h
        h = g.node("Relu", [g.node("Add", [y, sc], name=p + "add")], name=p + "relu3")
    h = g.node("GlobalAveragePool", [h], name="gap")
    h = g.node("Flatten", [h], name="flatten", axis=1)
    y = g.node("Gemm", [h, "fc.weight", "fc.bias"], name="fc", transB=1)
    g.output(y, ["N", cfg.num_classes])
    return g.model_proto(opset=opset, ir_version=7), w


def torch_forward(w: Dict[str, np.ndarray], x, cfg: ResNeXtConfig = ResNeXtConfig(), device="cpu", dtype=None):
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

    h = F.max_pool2d(torch.relu(conv_bn(x, "stem", "stem_bn", 7, 2)), 3, 2, 1)
    for i, b in enumerate(_blocks(cfg)):
        p = "block%d." % i
        y = torch.relu(conv_bn(h, p + "conv1", p + "bn1", 1, 1))
        y = torch.relu(conv_bn(y, p + "conv2", p + "bn2", 3, b["stride"], group=cfg.cardinality))
        y = conv_bn(y, p + "conv3", p + "bn3", 1, 1)
        sc = conv_bn(h, p + "down", p + "down_bn", 1, b["stride"]) if b["project"] else h
        h = torch.relu(y + sc)
    return F.linear(h.mean(dim=(2, 3)), t["fc.weight"], t["fc.bias"])


def synthetic_input(batch: int, cfg: ResNeXtConfig = ResNeXtConfig(), seed: int = 1) -> np.ndarray:
    rng = np.random.default_rng(seed)
    return np.round(rng.random((batch, cfg.in_ch, cfg.image, cfg.image), dtype=np.float32), 4).astype(np.float32)
