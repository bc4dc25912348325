#!/usr/bin/env python3
"""The wide-group MFMA grouped 3x3 conv kernel (kernels/gconv_wide.hip) against gconv_kernel<false>
(kernels/gconv.hip, through die_kern_gconv) on the device, in both precisions: every distinct grouped-conv shape
of RegNetX-1.6GF, RegNetY-1.6GF, RegNetX-3.2GF, RegNetY-8GF and of the last stage of ResNeXt-101 32x8d at batch 1,
8 and 32, bias + ReLU epilogue, pads 1.

The method is tools/gconv_bench.py's: each figure is a captured hipGraph of LAUNCHES launches on preallocated
buffers, in microseconds per launch, the median [min, max] of REPLAYS replays, the two kernels' replays interleaved
in one process; `spread` is the larger of the two (max - min) / median, and the new kernel is "faster" for a shape
where its median times (1 + spread) is below gconv's.  The outputs are compared first.  `bytes` is what the layer
must move (input + output + packed weights, once), `mfma` the v_mfma_f32_16x16x32_bf16 the kernel issues (tiles x
bundles x 4 fragments x K-steps, x 3 in fp32 mode), both computed from the shape.  The summary per (w, stride)
class is the planner's mark rule (kern::gconv_wide_class_on): a class is on when every shape of it is faster.

--model adds the forward of RegNetX-1.6GF, RegNetY-1.6GF and RegNetY-8GF at batch 8 and 32 (autotune off): device
time per forward with EngineOptions::mfma_gconv on and off, alternating twice.

  python tools/gconv_wide_bench.py [--md out.md] [--json out.json] [--model]
"""
import argparse
import json
import os
import statistics
import sys
import tempfile

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(HERE, "tools"))

from gconv_bench import REPLAYS, capture, replay_us  # noqa: E402

BATCHES = (1, 8, 32)


def model_shapes(rn, rx):
    """(map, C, groups, stride) -> the models that have it"""
    shapes = {}
    for name, make in rn.CONFIGS.items():
        for c in rn.grouped_convs(make()):
            shapes.setdefault((c["hw"], c["C"], c["groups"], c["stride"]), []).append(name)
    for c in rx.grouped_convs(rx.ResNeXtConfig(stages=(3, 4, 23, 3), cardinality=32, base_width=8))[-3:]:
        shapes.setdefault((c["hw"], c["C"], c["groups"], c["stride"]), []).append("resnext101_32x8d")
    return shapes


def kernel_rows(torch, native, K, shapes):
    L = native.kernels()
    rows = []
    for split in (True, False):
        for hw, C, G, stride in sorted(shapes, key=lambda s: (s[1] // s[2], -s[0], s[1])):
            for B in BATCHES:
                cw, Ho = C // G, (hw - 1) // stride + 1
                g = torch.Generator(device="cuda").manual_seed(hw + C)
                x = torch.randn(B, hw, hw, C, device="cuda", generator=g)
                w = torch.randn(C, cw, 3, 3, device="cuda", generator=g) / (9 * cw) ** 0.5
                bias = torch.randn(C, device="cuda", generator=g)
                xin = K.split_planes(x) if split else x.to(torch.bfloat16).contiguous()
                wp, wplane = K.pack_gconv_wide_weight(w, split)
                w_old = w.permute(0, 2, 3, 1).contiguous()
                shape = ((2,) if split else ()) + (B, Ho, Ho, C)
                outs = [torch.zeros(shape, dtype=torch.bfloat16, device="cuda") for _ in (0, 1)]
                geom = json.dumps(dict(B=B, H=hw, W=hw, Cin=C, Ho=Ho, Wo=Ho, Cout=C, groups=G, KH=3, KW=3, stride=stride,
                                       dil=1, pad_h=1, pad_w=1, act=1, split=int(split))).encode()

                def launch(wide):  # on the current stream: the capture stream inside torch.cuda.graph
                    st = int(torch.cuda.current_stream().cuda_stream)
                    if wide:
                        rc = L.die_kern_gconv_wide(geom, xin.data_ptr(), wp.data_ptr(), wplane, bias.data_ptr(), 0,
                                                   outs[0].data_ptr(), 0, 0, st)
                    else:
                        rc = L.die_kern_gconv(geom, xin.data_ptr(), w_old.data_ptr(), bias.data_ptr(), outs[1].data_ptr(), st)
                    assert rc == 0, rc

                graphs = [capture(torch, lambda: launch(True)), capture(torch, lambda: launch(False))]
                va, vb = [(K.join_planes(o) if split else o.float()) for o in outs]
                diff = float((va - vb).abs().max() / vb.abs().max())
                # bf16: gconv_kernel keeps fp32 weights, the MFMA kernel rounds them to bf16 (2^-9 per product), and
                # both round the stored output (2^-9); fp32 mode: 2^-17 per operand and stored value
                assert diff < (2e-4 if split else 3e-2), (hw, C, B, split, diff)
                ts = [[], []]
                for _ in range(REPLAYS):
                    for i in (0, 1):
                        ts[i].append(replay_us(torch, graphs[i]))
                med = [statistics.median(t) for t in ts]
                spread = max((max(t) - min(t)) / statistics.median(t) for t in ts)
                nbytes = (x.numel() + B * Ho * Ho * C) * (4 if split else 2) + wp.numel() * 2
                tiles = B * ((Ho + 7) // 8) ** 2
                mfma = tiles * G * ((cw + 15) // 16) * 4 * ((9 * cw + 31) // 32) * (3 if split else 1)
                r = {"precision": "fp32" if split else "bf16", "hw": hw, "C": C, "w": cw, "stride": stride, "B": B,
                     "wide_us": round(med[0], 2), "wide_min": round(min(ts[0]), 2), "wide_max": round(max(ts[0]), 2),
                     "gconv_us": round(med[1], 2), "gconv_min": round(min(ts[1]), 2), "gconv_max": round(max(ts[1]), 2),
                     "spread": round(spread, 3), "gconv_over_wide": round(med[1] / med[0], 3), "bytes": nbytes, "mfma": mfma,
                     "max_rel_diff": diff, "wide_faster": bool(med[0] * (1 + spread) < med[1]),
                     "models": sorted(set(shapes[(hw, C, G, stride)]))}
                rows.append(r)
                print(json.dumps(r), flush=True)
    return rows


def model_rows(native, rn, iters=10):
    rows = []
    for name in ("regnet_x_1_6gf", "regnet_y_1_6gf", "regnet_y_8gf"):
        cfg = rn.CONFIGS[name]()
        path = os.path.join(tempfile.mkdtemp(), name + ".onnx")
        open(path, "wb").write(rn.build_onnx(cfg)[0])
        for precision in ("fp32", "bf16"):
            engines = {on: native.Engine(path, device="hip", max_batch=32, precision=precision, autotune=False,
                                         mfma_gconv=on) for on in (True, False)}
            for B in (8, 32):
                x = rn.synthetic_input(B, cfg, seed=3).reshape(B, -1)
                for rep in (0, 1):
                    for on, e in engines.items():
                        for _ in range(3):
                            e.run(x)
                        i0 = e.refresh_info()
                        for _ in range(iters):
                            e.run(x)
                        i1 = e.refresh_info()
                        us = 1e3 * (i1["device_busy_ms"] - i0["device_busy_ms"]) / (i1["batches"] - i0["batches"])
                        r = {"model": name, "precision": precision, "B": B, "mfma_gconv": on, "rep": rep,
                             "forward_us": round(us, 1)}
                        rows.append(r)
                        print(json.dumps(r), flush=True)
            for e in engines.values():
                e.close()
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
    from die_amd.models import regnet as rn
    from die_amd.models import resnext as rx
    from die_amd.ops import kernels as K

    rows = kernel_rows(torch, native, K, model_shapes(rn, rx))
    lines = ["| precision | map x C | w | stride | B | wide us [min, max] | gconv us [min, max] | spread | gconv / wide | MB | MFMA | wide faster |",
             "|---|---|---:|---:|---:|---:|---:|---:|---:|---:|---:|---|"]
    for r in rows:
        lines.append("| %s | %dx%dx%d | %d | %d | %d | %.1f [%.1f, %.1f] | %.1f [%.1f, %.1f] | %.1f%% | %.2f | %.2f | %d | %s |" % (
            r["precision"], r["hw"], r["hw"], r["C"], r["w"], r["stride"], r["B"], r["wide_us"], r["wide_min"], r["wide_max"],
            r["gconv_us"], r["gconv_min"], r["gconv_max"], 100 * r["spread"], r["gconv_over_wide"], r["bytes"] / 1e6, r["mfma"],
            "yes" if r["wide_faster"] else "no"))
    lines += ["", "| w | stride | shapes | faster | smallest gconv / wide | largest |", "|---:|---:|---:|---:|---:|---:|"]
    for cls in sorted({(r["w"], r["stride"]) for r in rows}):
        rs = [r for r in rows if (r["w"], r["stride"]) == cls]
        lines.append("| %d | %d | %d | %d | %.2f | %.2f |" % (cls + (len(rs), sum(r["wide_faster"] for r in rs),
                                                               min(r["gconv_over_wide"] for r in rs),
                                                               max(r["gconv_over_wide"] for r in rs))))
    mrows = model_rows(native, rn) if a.model else []
    if mrows:
        lines += ["", "| model | precision | B | mfma_gconv | run | forward us |", "|---|---|---:|---|---:|---:|"]
        lines += ["| %s | %s | %d | %s | %d | %.1f |" % (r["model"], r["precision"], r["B"], "on" if r["mfma_gconv"] else "off",
                                                       r["rep"], r["forward_us"]) for r in mrows]
    text = "\n".join(lines) + "\n"
    print(text)
    if a.md:
        open(a.md, "w").write(text)
    if a.json:
        json.dump({"kernels": rows, "model": mrows}, open(a.json, "w"), indent=1)


if __name__ == "__main__":
    main()
