#!/usr/bin/env python3
"""The polyphase tiled depthwise conv kernel (kernels/dwconv_poly.hip) against gconv_kernel<true>
(kernels/gconv.hip) on the device, in both precisions: every depthwise conv shape of MobileNetV2-224 and
EfficientNet-Lite0-224 in the kernel's three (window, stride) classes (3x3 stride 1 / 2, 5x5 stride 2; taken
from the model generators, with their pads, the asymmetric stride-2 form included), at batch 1, 8 and 32, with
the models' epilogue (bias + Clip(0, 6)).

Method of tools/dwconv_bench.py: each figure is a captured hipGraph of 20 launches on preallocated buffers, in
microseconds per launch: the median [min, max] of 9 replays, the two kernels' replays interleaved in one
process; both outputs are compared bit for bit first.  `spread` is the larger of the two (max - min) / median.
The rule per (window, stride) class: the class is marked in the planner (kern::dwconv_poly_class_on) only if
on every shape at batch 8 and 32, in both precisions, the new median beats gconv's by more than the spread.
`floor GB/s` is bytes moved (input once, output once, weights, bias) over the new kernel's median time.

--model: e.profile(32) totals of MobileNetV2-224 and EfficientNet-Lite0-224 with EngineOptions::poly_dwconv on
and off, both engines in one process, five alternating runs each.

  python tools/dwconv_poly_bench.py [--model] [--md out.md] [--json out.json]
"""
import argparse
import json
import os
import statistics
import sys
import tempfile

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from dwconv_bench import capture, replay_us  # noqa: E402

BATCHES = (1, 8, 32)
REPLAYS = 9
CLASSES = ((3, 1), (3, 2), (5, 2))


def model_shapes(mb, el):
    """[(k, stride, H = W of the input, C, pads)] of both models at 224, in the three classes, without repeats"""
    seen = []
    for blocks, first in ((mb._blocks(mb.MobileNetConfig()), 112), (el._blocks(el.EfficientNetLiteConfig()), 112)):
        hw = first
        for b in blocks:
            k, s = b.get("k", 3), b["stride"]
            pads = tuple(b["pads"]) if "pads" in b else ((0, 0, 1, 1) if s == 2 else (1, 1, 1, 1))
            shape = (k, s, hw, b["hidden"], pads)
            if (k, s) in CLASSES and shape not in seen:
                seen.append(shape)
            hw = (hw + pads[0] + pads[2] - k) // s + 1
    return sorted(seen, key=lambda t: (t[0], t[1], -t[2], t[3]))


def kernel_rows(torch, native, K, shapes):
    L = native.kernels()
    rows = []
    for split in (True, False):
        for k, stride, hw, C, pads in shapes:
            ho = (hw + pads[0] + pads[2] - k) // stride + 1
            for B in BATCHES:
                g = torch.Generator(device="cuda").manual_seed(hw + C)
                x = torch.randn(B, hw, hw, C, device="cuda", generator=g)
                w = torch.randn(C, 1, k, k, device="cuda", generator=g) * 0.2
                bias = torch.randn(C, device="cuda", generator=g)
                xin = K.split_planes(x) if split else x.to(torch.bfloat16).contiguous()
                ws = [w.reshape(C, k * k).t().contiguous(), w.permute(0, 2, 3, 1).contiguous()]  # [tap][C], [C][k][k][1]
                outs = [torch.zeros(((2,) if split else ()) + (B, ho, ho, C), dtype=torch.bfloat16, device="cuda") for _ in (0, 1)]
                geom = json.dumps(dict(B=B, H=hw, W=hw, Cin=C, Ho=ho, Wo=ho, Cout=C, groups=C, KH=k, KW=k, stride=stride,
                                       dil=1, pad_h=pads[0], pad_w=pads[1], act=3, clip_lo=0.0, clip_hi=6.0,
                                       split=int(split))).encode()

                def launch(i):  # on the current stream: the capture stream inside torch.cuda.graph
                    st = int(torch.cuda.current_stream().cuda_stream)
                    if i == 0:
                        rc = L.die_kern_dwconv_poly(geom, xin.data_ptr(), ws[0].data_ptr(), bias.data_ptr(), 0,
                                                    outs[0].data_ptr(), 0, 0, st)
                    else:
                        rc = L.die_kern_dwconv(geom, 0, xin.data_ptr(), ws[1].data_ptr(), bias.data_ptr(), 0,
                                               outs[1].data_ptr(), 0, 0, st)
                    assert rc == 0, rc

                graphs = [capture(torch, lambda: launch(0)), capture(torch, lambda: launch(1))]
                assert torch.equal(outs[0].view(torch.int16), outs[1].view(torch.int16)), (k, stride, hw, C, B, split)
                ts = [[], []]
                for _ in range(REPLAYS):
                    for i in (0, 1):
                        ts[i].append(replay_us(torch, graphs[i]))
                med = [statistics.median(t) for t in ts]
                spread = max((max(t) - min(t)) / statistics.median(t) for t in ts)
                nbytes = (2 + 2 * split) * B * C * (hw * hw + ho * ho) + 4 * C * (k * k + 1)
                r = {"precision": "fp32" if split else "bf16", "k": k, "stride": stride, "hw": hw, "C": C, "pads": list(pads),
                     "B": B, "poly_us": round(med[0], 2), "poly_min": round(min(ts[0]), 2), "poly_max": round(max(ts[0]), 2),
                     "gconv_us": round(med[1], 2), "gconv_min": round(min(ts[1]), 2), "gconv_max": round(max(ts[1]), 2),
                     "spread": round(spread, 3), "gconv_over_poly": round(med[1] / med[0], 3), "bytes": nbytes,
                     "poly_gbps": round(nbytes / med[0] / 1e3, 1), "poly_wins": bool(med[0] < med[1] * (1 - spread))}
                rows.append(r)
                print(json.dumps(r), flush=True)
    return rows


def model_rows(native, mb, el, runs=5):
    rows = []
    for name, mod, cfg in (("mobilenet_v2", mb, mb.MobileNetConfig()), ("efficientnet_lite0", el, el.EfficientNetLiteConfig())):
        path = os.path.join(tempfile.mkdtemp(), name + ".onnx")
        open(path, "wb").write(mod.build_onnx(cfg)[0])
        for precision in ("fp32", "bf16"):
            engines = {on: native.Engine(path, device="hip", max_batch=32, precision=precision, poly_dwconv=on) for on in (True, False)}
            us = {True: [], False: []}
            for _ in range(runs):
                for on, e in engines.items():
                    us[on].append(e.profile(32, iters=10)["total_us"])
            for e in engines.values():
                e.close()
            r = {"model": name, "precision": precision, "B": 32}
            for on, key in ((True, "on"), (False, "off")):
                r[key + "_us"] = round(statistics.median(us[on]), 1)
                r[key + "_min"], r[key + "_max"] = round(min(us[on]), 1), round(max(us[on]), 1)
            rows.append(r)
            print(json.dumps(r), flush=True)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--md", default="")
    ap.add_argument("--json", default="")
    ap.add_argument("--model", action="store_true")
    a = ap.parse_args()
    sys.path.insert(0, HERE)
    import torch

    import die_amd  # noqa: F401
    from die_amd import native
    from die_amd.models import efficientnet_lite as el
    from die_amd.models import mobilenet as mb
    from die_amd.ops import kernels as K

    rows = kernel_rows(torch, native, K, model_shapes(mb, el))
    lines = ["| precision | window / stride | map x C | pads | B | poly us [min, max] | gconv us [min, max] | spread | gconv / poly | poly GB/s | poly wins |",
             "|---|---|---|---|---:|---:|---:|---:|---:|---:|---|"]
    for r in rows:
        lines.append("| %s | %dx%d / %d | %dx%dx%d | %s | %d | %.1f [%.1f, %.1f] | %.1f [%.1f, %.1f] | %.1f%% | %.2f | %.0f | %s |" % (
            r["precision"], r["k"], r["k"], r["stride"], r["hw"], r["hw"], r["C"], ",".join(map(str, r["pads"])), r["B"],
            r["poly_us"], r["poly_min"], r["poly_max"], r["gconv_us"], r["gconv_min"], r["gconv_max"], 100 * r["spread"],
            r["gconv_over_poly"], r["poly_gbps"], "yes" if r["poly_wins"] else "no"))
    lines += ["", "| window / stride | shapes x precisions at B = 8, 32 | poly wins | least gconv / poly | class on |", "|---|---:|---:|---:|---|"]
    for k, s in CLASSES:
        dec = [r for r in rows if (r["k"], r["stride"]) == (k, s) and r["B"] >= 8]
        lines.append("| %dx%d / %d | %d | %d | %.2f | %s |" % (k, k, s, len(dec), sum(r["poly_wins"] for r in dec),
                                                             min(r["gconv_over_poly"] for r in dec),
                                                             "yes" if all(r["poly_wins"] for r in dec) else "no"))
    mrows = model_rows(native, mb, el) if a.model else []
    if mrows:
        lines += ["", "| model | precision | B | poly_dwconv on us [min, max] | off us [min, max] | off / on |", "|---|---|---:|---:|---:|---:|"]
        lines += ["| %s | %s | %d | %.1f [%.1f, %.1f] | %.1f [%.1f, %.1f] | %.3f |" % (
            r["model"], r["precision"], r["B"], r["on_us"], r["on_min"], r["on_max"], r["off_us"], r["off_min"], r["off_max"],
            r["off_us"] / r["on_us"]) for r in mrows]
    text = "\n".join(lines) + "\n"
    print(text)
    if a.md:
        open(a.md, "w").write(text)
    if a.json:
        json.dump({"kernels": rows, "model": mrows}, open(a.json, "w"), indent=1)


if __name__ == "__main__":
    main()
