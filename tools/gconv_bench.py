#!/usr/bin/env python3
"""The MFMA grouped 3x3 conv kernel (kernels/gconv_mfma.hip) against gconv_kernel<false> (kernels/gconv.hip,
through die_kern_gconv) on the device, in both precisions: every distinct grouped-conv shape of ResNeXt-50
32x4d at batch 1 and 32, bias + ReLU epilogue, pads 1.

Each figure is a captured hipGraph of LAUNCHES launches on preallocated buffers (warm: the same input every
launch), in microseconds per launch: the median [min, max] of REPLAYS replays, the two kernels' replays
interleaved in one process.  `spread` is the larger of the two (max - min) / median; the MFMA kernel is "no
slower" for a shape where its median is at most gconv's times (1 + spread).  The outputs are compared first
(max |a - b| over max |b|: the kernels round their weights differently, so not bit for bit).  `floor us` is
the bytes the layer must move (input + output + packed weights, once) over 8 TB/s: a lower bound from HBM
that a warm input in the last-level cache can beat, not a share of peak.

--model adds the ResNeXt-50 forward at batch 32: device time per forward (the engine's device_busy_ms over
`iters` runs after 3 warm-up runs) with EngineOptions::mfma_gconv on and off, alternating twice.

  python tools/gconv_bench.py [--md out.md] [--json out.json] [--model]
"""
import argparse
import json
import os
import statistics
import sys
import tempfile

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

BATCHES = (1, 32)
LAUNCHES, REPLAYS = 10, 7
HBM_BYTES_PER_US = 8e6  # 8 TB/s


def capture(torch, launch):
    launch()
    torch.cuda.synchronize()
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gr):
        for _ in range(LAUNCHES):
            launch()
    gr.replay()
    torch.cuda.synchronize()
    return gr


def replay_us(torch, gr):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    gr.replay()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1000 / LAUNCHES


def kernel_rows(torch, native, K, rx):
    L = native.kernels()
    shapes = sorted({(c["hw"], c["C"], c["groups"], c["stride"]) for c in rx.grouped_convs()}, key=lambda s: (-s[0], s[1]))
    rows = []
    for split in (True, False):
        for hw, C, G, stride in shapes:
            for B in BATCHES:
                cw, Ho = C // G, (hw - 1) // stride + 1
                g = torch.Generator(device="cuda").manual_seed(hw + C)
                x = torch.randn(B, hw, hw, C, device="cuda", generator=g)
                w = torch.randn(C, cw, 3, 3, device="cuda", generator=g) / (9 * cw) ** 0.5
                bias = torch.randn(C, device="cuda", generator=g)
                xin = K.split_planes(x) if split else x.to(torch.bfloat16).contiguous()
                wp, wplane = K.pack_gconv_mfma_weight(w, split)
                w_old = w.permute(0, 2, 3, 1).contiguous()
                shape = ((2,) if split else ()) + (B, Ho, Ho, C)
                outs = [torch.zeros(shape, dtype=torch.bfloat16, device="cuda") for _ in (0, 1)]
                geom = json.dumps(dict(B=B, H=hw, W=hw, Cin=C, Ho=Ho, Wo=Ho, Cout=C, groups=G, KH=3, KW=3, stride=stride,
                                       dil=1, pad_h=1, pad_w=1, act=1, split=int(split))).encode()

                def launch(mfma):  # on the current stream: the capture stream inside torch.cuda.graph
                    st = int(torch.cuda.current_stream().cuda_stream)
                    if mfma:
                        rc = L.die_kern_gconv_mfma(geom, xin.data_ptr(), wp.data_ptr(), wplane, bias.data_ptr(), 0,
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
                r = {"precision": "fp32" if split else "bf16", "hw": hw, "C": C, "w": cw, "stride": stride, "B": B,
                     "mfma_us": round(med[0], 2), "mfma_min": round(min(ts[0]), 2), "mfma_max": round(max(ts[0]), 2),
                     "gconv_us": round(med[1], 2), "gconv_min": round(min(ts[1]), 2), "gconv_max": round(max(ts[1]), 2),
                     "spread": round(spread, 3), "gconv_over_mfma": round(med[1] / med[0], 3), "bytes": nbytes,
                     "floor_us": round(nbytes / HBM_BYTES_PER_US, 2), "max_rel_diff": diff,
                     "mfma_no_slower": bool(med[0] <= med[1] * (1 + spread))}
                rows.append(r)
                print(json.dumps(r), flush=True)
    return rows


def model_rows(native, rx, iters=20):
    cfg = rx.ResNeXtConfig()
    path = os.path.join(tempfile.mkdtemp(), "resnext50_32x4d.onnx")
    open(path, "wb").write(rx.build_onnx(cfg)[0])
    x = rx.synthetic_input(32, cfg, seed=3).reshape(32, -1)
    rows = []
    for precision in ("fp32", "bf16"):
        engines = {on: native.Engine(path, device="hip", max_batch=32, precision=precision, mfma_gconv=on) for on in (True, False)}
        for rep in (0, 1):
            for on, e in engines.items():
                for _ in range(3):
                    e.run(x)
                i0 = e.refresh_info()
                for _ in range(iters):
                    e.run(x)
                i1 = e.refresh_info()
                us = 1e3 * (i1["device_busy_ms"] - i0["device_busy_ms"]) / (i1["batches"] - i0["batches"])
                r = {"model": "resnext50_32x4d", "precision": precision, "B": 32, "mfma_gconv": on, "rep": rep,
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
    from die_amd.models import resnext as rx
    from die_amd.ops import kernels as K

    rows = kernel_rows(torch, native, K, rx)
    lines = ["| precision | map x C | w | stride | B | mfma us [min, max] | gconv us [min, max] | spread | gconv / mfma | floor us | mfma no slower |",
             "|---|---|---:|---:|---:|---:|---:|---:|---:|---:|---|"]
    for r in rows:
        lines.append("| %s | %dx%dx%d | %d | %d | %d | %.1f [%.1f, %.1f] | %.1f [%.1f, %.1f] | %.1f%% | %.2f | %.2f | %s |" % (
            r["precision"], r["hw"], r["hw"], r["C"], r["w"], r["stride"], r["B"], r["mfma_us"], r["mfma_min"], r["mfma_max"],
            r["gconv_us"], r["gconv_min"], r["gconv_max"], 100 * r["spread"], r["gconv_over_mfma"], r["floor_us"],
            "yes" if r["mfma_no_slower"] else "no"))
    mrows = model_rows(native, rx) if a.model else []
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
