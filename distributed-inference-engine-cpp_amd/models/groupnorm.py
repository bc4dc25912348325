"""GroupNorm / InstanceNorm models: ONNX generators + torch references (random weights).

  gn_resnet       BiT-style GN-ResNet on 32x32: stem conv -> GN -> ReLU, three bottleneck stages (conv 1x1 ->
                  GN -> ReLU -> conv 3x3 -> GN -> ReLU -> conv 1x1 -> GN, + projected shortcut -> GN, Add, ReLU) of
                  widths 32 / 64 / 96 with 8 or 32 groups (4, 8, 3 and 12 channels per group), GAP + FC.  Every
                  GroupNorm is written the way torch exports it below opset 18: Reshape(x, [0, G, -1]) ->
                  InstanceNormalization(ones [G], zeros [G]) -> Reshape(., [0, C, H, W]) -> Mul(w [C,1,1]) ->
                  Add(b [C,1,1]).
  gn_resnet_node  the same weights through GroupNormalization nodes: stage 0 and the stem with per-group
                  parameters (opset 18; the weights are then constant over a group), the rest per channel
                  (opset 21).  gn_resnet itself is built with those group-constant weights in the same places,
                  so the two graphs compute the same function.
  gn_decoder      autoencoder / UNet decoder piece on an 8x8 latent: conv -> two residual blocks
                  h + conv(SiLU(GN8(h))) at 80 channels (10 per group) -> nearest x2 Resize -> conv -> GN8 ->
                  SiLU -> conv to 3 channels; the image is the graph output.  SiLU is Mul(y, Sigmoid(y)), in both
                  operand orders; the back-shape of the GroupNorm export is folded from a Shape node in the
                  first block and a constant elsewhere.
  inorm_net       style-transfer piece: conv -> InstanceNormalization -> ReLU three times (16, 20 and 8
                  channels: the 20 are stored as 24), the image is the graph output.
"""
from __future__ import annotations

import math
from typing import Dict, Tuple

import numpy as np

from ..utils.onnx_writer import GraphBuilder

SPECS = {
    "gn_resnet": dict(in_ch=3, image=32, classes=10, eps=1e-5,
                      # (width, stride, groups of the three block norms, groups of the shortcut norm)
                      stages=((32, 1, (8, 8, 8), 8), (64, 2, (8, 8, 8), 8), (96, 2, (32, 32, 8), 32))),
    "gn_decoder": dict(in_ch=8, image=8, width=80, mid=32, out_ch=3, groups=8, eps=1e-6),
    "inorm_net": dict(in_ch=3, image=12, widths=(16, 20, 8), eps=1e-5),
}
SPECS["gn_resnet_node"] = SPECS["gn_resnet"]


def _rng(seed):
    return np.random.default_rng(seed)


def _conv_w(rng, cout, cin, k):
    return rng.normal(0, 1.0 / math.sqrt(cin * k * k), (cout, cin, k, k)).astype(np.float32)


def _norm_w(rng, w, name, C, G=None):
    """gamma / beta of a norm; G: constant over each of the G groups (expressible per group)"""
    n = C if G is None else G
    g, b = rng.uniform(0.7, 1.3, n).astype(np.float32), rng.normal(0, 0.1, n).astype(np.float32)
    if G is not None:
        g, b = np.repeat(g, C // G), np.repeat(b, C // G)
    w[name + ".weight"], w[name + ".bias"] = g, b


# ---- graph pieces -------------------------------------------------------------------------------------

def _gn_export(g, x, w, name, C, H, W, G, eps, shape_node=False):
    """torch's GroupNorm export below opset 18"""
    r = g.node("Reshape", [x, g.const(np.array([0, G, -1], np.int64), name + "/shape")], name=name + "/group")
    n = g.node("InstanceNormalization", [r, g.const(np.ones(G, np.float32), name + "/ones"),
                                         g.const(np.zeros(G, np.float32), name + "/zeros")], name=name, epsilon=eps)
    back = g.node("Shape", [x], name=name + "/shape_of") if shape_node else \
        g.const(np.array([0, C, H, W], np.int64), name + "/back_shape")
    y = g.node("Reshape", [n, back], name=name + "/ungroup")
    y = g.node("Mul", [y, g.const(w[name + ".weight"].reshape(C, 1, 1), name + "/w")], name=name + "/scale")
    return g.node("Add", [y, g.const(w[name + ".bias"].reshape(C, 1, 1), name + "/b")], name=name + "/shift")


def _gn_node(g, x, w, name, C, G, eps, per_group):
    gm, bt = w[name + ".weight"], w[name + ".bias"]
    if per_group:
        gm, bt = gm[::C // G], bt[::C // G]
    return g.node("GroupNormalization", [x, g.const(gm, name + "/w"), g.const(bt, name + "/b")], name=name,
                  num_groups=G, epsilon=eps)


def _conv(g, x, w, name, k, stride=1, bias=False):
    ins = [x, g.init(name + ".weight", w[name + ".weight"])]
    if bias:
        ins.append(g.init(name + ".bias", w[name + ".bias"]))
    return g.node("Conv", ins, name=name, kernel_shape=[k, k], strides=[stride, stride], pads=[k // 2] * 4)


# ---- gn_resnet / gn_resnet_node ---------------------------------------------------------------------------

def _resnet_weights(seed):
    s = SPECS["gn_resnet"]
    rng, w = _rng(seed), {}
    w["stem.conv.weight"] = _conv_w(rng, 32, s["in_ch"], 3)
    _norm_w(rng, w, "stem.norm", 32, 8)
    cin = 32
    for i, (C, stride, gs, gsc) in enumerate(s["stages"]):
        p = "stage%d." % i
        grouped = i == 0  # written per group in gn_resnet_node
        for j, (co, ci, k) in enumerate(((C, cin, 1), (C, C, 3), (C, C, 1))):
            w[p + "conv%d.weight" % j] = _conv_w(rng, co, ci, k)
            _norm_w(rng, w, p + "norm%d" % j, C, gs[j] if grouped else None)
        w[p + "short.conv.weight"] = _conv_w(rng, C, cin, 1)
        _norm_w(rng, w, p + "short.norm", C, gsc if grouped else None)
        cin = C
    w["fc.weight"] = rng.normal(0, 1.0 / math.sqrt(cin), (s["classes"], cin)).astype(np.float32)
    w["fc.bias"] = rng.normal(0, 0.01, s["classes"]).astype(np.float32)
    return w


def build_gn_resnet(seed: int = 0, node_form: bool = False) -> Tuple[bytes, Dict[str, np.ndarray]]:
    s = SPECS["gn_resnet"]
    w = _resnet_weights(seed)
    g = GraphBuilder(name="gn_resnet_node" if node_form else "gn_resnet")
    x = g.input("image", ["N", s["in_ch"], s["image"], s["image"]])
    eps = s["eps"]

    def norm(h, name, C, HW, G, per_group):
        if node_form:
            return _gn_node(g, h, w, name, C, G, eps, per_group)
        return _gn_export(g, h, w, name, C, HW, HW, G, eps)

    hw = s["image"]
    h = _conv(g, x, w, "stem.conv", 3)
    h = g.node("Relu", [norm(h, "stem.norm", 32, hw, 8, True)], name="stem.relu")
    for i, (C, stride, gs, gsc) in enumerate(s["stages"]):
        p = "stage%d." % i
        per_group = i == 0
        sc = _conv(g, h, w, p + "short.conv", 1, stride)
        y = _conv(g, h, w, p + "conv0", 1)
        y = g.node("Relu", [norm(y, p + "norm0", C, hw, gs[0], per_group)], name=p + "relu0")
        y = _conv(g, y, w, p + "conv1", 3, stride)
        hw //= stride
        sc = norm(sc, p + "short.norm", C, hw, gsc, per_group)
        y = g.node("Relu", [norm(y, p + "norm1", C, hw, gs[1], per_group)], name=p + "relu1")
        y = _conv(g, y, w, p + "conv2", 1)
        y = norm(y, p + "norm2", C, hw, gs[2], per_group)
        h = g.node("Relu", [g.node("Add", [y, sc], name=p + "add")], name=p + "relu2")
    h = g.node("Flatten", [g.node("GlobalAveragePool", [h], name="gap")], name="flatten", axis=1)
    y = g.node("Gemm", [h, g.init("fc.weight", w["fc.weight"]), g.init("fc.bias", w["fc.bias"])], name="fc", transB=1)
    g.output(y, ["N", s["classes"]])
    return g.model_proto(opset=21 if node_form else 17), w


def _resnet_forward(w, x, t, F):
    s = SPECS["gn_resnet"]

    def norm(h, name, G):
        return F.group_norm(h, G, t[name + ".weight"], t[name + ".bias"], s["eps"])

    h = F.relu(norm(F.conv2d(x, t["stem.conv.weight"], padding=1), "stem.norm", 8))
    for i, (C, stride, gs, gsc) in enumerate(s["stages"]):
        p = "stage%d." % i
        sc = norm(F.conv2d(h, t[p + "short.conv.weight"], stride=stride), p + "short.norm", gsc)
        y = F.relu(norm(F.conv2d(h, t[p + "conv0.weight"]), p + "norm0", gs[0]))
        y = F.relu(norm(F.conv2d(y, t[p + "conv1.weight"], stride=stride, padding=1), p + "norm1", gs[1]))
        y = norm(F.conv2d(y, t[p + "conv2.weight"]), p + "norm2", gs[2])
        h = F.relu(y + sc)
    return F.linear(h.mean(dim=(2, 3)), t["fc.weight"], t["fc.bias"])


# ---- gn_decoder ---------------------------------------------------------------------------------------------

def build_gn_decoder(seed: int = 0) -> Tuple[bytes, Dict[str, np.ndarray]]:
    s = SPECS["gn_decoder"]
    rng, w = _rng(seed), {}
    C, M, G, hw = s["width"], s["mid"], s["groups"], s["image"]
    for name, co, ci in (("conv_in", C, s["in_ch"]), ("block0.conv", C, C), ("block1.conv", C, C), ("conv_up", M, C),
                         ("conv_out", s["out_ch"], M)):
        w[name + ".weight"] = _conv_w(rng, co, ci, 3)
        w[name + ".bias"] = rng.normal(0, 0.02, co).astype(np.float32)
    for name, c in (("block0.norm", C), ("block1.norm", C), ("norm_out", M)):
        _norm_w(rng, w, name, c)
    g = GraphBuilder(name="gn_decoder")
    x = g.input("latent", ["N", s["in_ch"], hw, hw])

    def silu(y, name, swapped):
        sg = g.node("Sigmoid", [y], name=name + "/sigmoid")
        return g.node("Mul", [sg, y] if swapped else [y, sg], name=name + "/mul")

    h = _conv(g, x, w, "conv_in", 3, bias=True)
    for b in range(2):
        p = "block%d." % b
        y = _gn_export(g, h, w, p + "norm", C, hw, hw, G, s["eps"], shape_node=b == 0)
        y = _conv(g, silu(y, p + "silu", swapped=b == 1), w, p + "conv", 3, bias=True)
        h = g.node("Add", [h, y], name=p + "add")
    empty = g.const(np.zeros(0, np.float32), "no_roi")
    h = g.node("Resize", [h, empty, g.const(np.array([1, 1, 2, 2], np.float32), "up_scales")], name="upsample",
               mode="nearest", coordinate_transformation_mode="asymmetric", nearest_mode="floor")
    h = _conv(g, h, w, "conv_up", 3, bias=True)
    y = _gn_export(g, h, w, "norm_out", M, 2 * hw, 2 * hw, G, s["eps"])
    y = _conv(g, silu(y, "silu_out", swapped=False), w, "conv_out", 3, bias=True)
    g.output(y, ["N", s["out_ch"], 2 * hw, 2 * hw])
    return g.model_proto(opset=17), w


def _decoder_forward(w, x, t, F):
    s = SPECS["gn_decoder"]

    def conv(h, name):
        return F.conv2d(h, t[name + ".weight"], t[name + ".bias"], padding=1)

    def norm(h, name):
        return F.silu(F.group_norm(h, s["groups"], t[name + ".weight"], t[name + ".bias"], s["eps"]))

    h = conv(x, "conv_in")
    for b in range(2):
        h = h + conv(norm(h, "block%d.norm" % b), "block%d.conv" % b)
    h = conv(F.interpolate(h, scale_factor=2, mode="nearest"), "conv_up")
    return conv(norm(h, "norm_out"), "conv_out")


# ---- inorm_net ------------------------------------------------------------------------------------------------

def build_inorm_net(seed: int = 0) -> Tuple[bytes, Dict[str, np.ndarray]]:
    s = SPECS["inorm_net"]
    rng, w = _rng(seed), {}
    g = GraphBuilder(name="inorm_net")
    h = g.input("image", ["N", s["in_ch"], s["image"], s["image"]])
    cin = s["in_ch"]
    for i, C in enumerate(s["widths"]):
        p = "layer%d." % i
        w[p + "conv.weight"] = _conv_w(rng, C, cin, 3)
        w[p + "conv.bias"] = rng.normal(0, 0.02, C).astype(np.float32)
        _norm_w(rng, w, p + "norm", C)
        h = _conv(g, h, w, p + "conv", 3, bias=True)
        h = g.node("InstanceNormalization", [h, g.init(p + "norm.weight", w[p + "norm.weight"]),
                                             g.init(p + "norm.bias", w[p + "norm.bias"])], name=p + "norm", epsilon=s["eps"])
        h = g.node("Relu", [h], name=p + "relu")
        cin = C
    g.output(h, ["N", cin, s["image"], s["image"]])
    return g.model_proto(opset=13), w


def _inorm_forward(w, x, t, F):
    s = SPECS["inorm_net"]
    h = x
    for i in range(len(s["widths"])):
        p = "layer%d." % i
        h = F.conv2d(h, t[p + "conv.weight"], t[p + "conv.bias"], padding=1)
        h = F.relu(F.instance_norm(h, weight=t[p + "norm.weight"], bias=t[p + "norm.bias"], eps=s["eps"]))
    return h


# ---- the tables -------------------------------------------------------------------------------------------------

BUILDERS = {
    "gn_resnet": lambda seed=0: build_gn_resnet(seed),
    "gn_resnet_node": lambda seed=0: build_gn_resnet(seed, node_form=True),
    "gn_decoder": build_gn_decoder,
    "inorm_net": build_inorm_net,
}
_FORWARDS = {"gn_resnet": _resnet_forward, "gn_resnet_node": _resnet_forward, "gn_decoder": _decoder_forward,
             "inorm_net": _inorm_forward}
# GROUPNORM ops a model's plan holds: (groups, logical channels, act) in plan order; act 0 none, 1 ReLU, 2 SiLU
EXPECTED_NORMS = {
    "gn_resnet": [(8, 32, 1)] + [n for C, _, gs, gsc in SPECS["gn_resnet"]["stages"]
                                 for n in ((gs[0], C, 1), (gsc, C, 0), (gs[1], C, 1), (gs[2], C, 0))],
    "gn_decoder": [(8, 80, 2), (8, 80, 2), (8, 32, 2)],
    "inorm_net": [(16, 16, 1), (20, 20, 1), (8, 8, 1)],
}
EXPECTED_NORMS["gn_resnet_node"] = EXPECTED_NORMS["gn_resnet"]


def input_shape(name: str):
    s = SPECS[name]
    return (s["in_ch"], s["image"], s["image"])


def synthetic_input(name: str, batch: int, seed: int = 1) -> np.ndarray:
    x = _rng(seed).standard_normal((batch,) + input_shape(name)).astype(np.float32)
    return np.round(x, 4).astype(np.float32)


def torch_forward(name: str, w: Dict[str, np.ndarray], x, device="cpu", dtype=None):
    import torch
    import torch.nn.functional as F

    dtype = dtype or torch.float32
    t = {k: torch.from_numpy(v).to(device=device, dtype=dtype) for k, v in w.items()}
    if not torch.is_tensor(x):
        x = torch.from_numpy(np.asarray(x, np.float32))
    return _FORWARDS[name](w, x.to(device=device, dtype=dtype), t, F)
