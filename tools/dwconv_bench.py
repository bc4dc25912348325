#!/usr/bin/env python3
"""The tiled depthwise conv kernel (kernels/dwconv.hip) against gconv_kernel<true> (kernels/gconv.hip) on
the device, in both precisions: the four depthwise shapes of ConvNeXt-T (7x7 on 56x56x96, 28x28x192,
14x14x384, 7x7x768) and a 5x5 on 28x28x240, at batch 1, 8 and 32, bias epilogue, pads k // 2.

Each figure is a captured hipGraph of 20 launches on preallocated buffers (warm: the same input every
launch), in microseconds per launch: the median [min, max] of 9 replays, the two kernels' replays
interleaved in one process.  `spread` is the larger of the two (max - min) / median; the tiled kernel is the
one to take for a shape only where its median beats gconv's by more than that.  Both outputs are compared bit
for bit first.

  python tools/dwconv_bench.py [--md out.md] [--json out.json]
"""
import argparse
import json
import os
import statistics
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (k, H = W, C)
SHAPES = ((7, 56, 96), (7, 28, 192), (7, 14, 384), (7, 7, 768), (5, 28, 240))
BATCHES = (1, 8, 32)
LAUNCHES, REPLAYS = 20, 9


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--md", default="")
    ap.add_argument("--json", default="")
    a = ap.parse_args()
    sys.path.insert(0, HERE)
    import torch

    import die_amd  # noqa: F401
    from die_amd import native
    from die_amd.ops import kernels as K

    L = native.kernels()
    rows = []
    for split in (True, False):
        for k, hw, C in SHAPES:
            for B in BATCHES:
                g = torch.Generator(device="cuda").manual_seed(hw + C)
                x = torch.randn(B, hw, hw, C, device="cuda", generator=g)
                w = torch.randn(C, 1, k, k, device="cuda", generator=g) * 0.2
                bias = torch.randn(C, device="cuda", generator=g)
                xin = K.split_planes(x) if split else x.to(torch.bfloat16).contiguous()
                w_tap = w.reshape(C, k * k).t().contiguous()
                w_old = w.permute(0, 2, 3, 1).contiguous()
                outs = [torch.zeros_like(xin), torch.zeros_like(xin)]
                geom = json.dumps(dict(B=B, H=hw, W=hw, Cin=C, Ho=hw, Wo=hw, Cout=C, groups=C, KH=k, KW=k, stride=1, dil=1,
                                       pad_h=k // 2, pad_w=k // 2, act=0, split=int(split))).encode()

                def launch(tiled):  # on the current stream: the capture stream inside torch.cuda.graph
                    rc = L.die_kern_dwconv(geom, int(tiled), xin.data_ptr(), (w_tap if tiled else w_old).data_ptr(),
                                           bias.data_ptr(), 0, outs[0 if tiled else 1].data_ptr(), 0, 0,
                                           int(torch.cuda.current_stream().cuda_stream))
                    assert rc == 0, rc

                graphs = [capture(torch, lambda: launch(True)), capture(torch, lambda: launch(False))]
                assert torch.equal(outs[0].view(torch.int16), outs[1].view(torch.int16)), (k, hw, C, B, split)
                ts = [[], []]
                for _ in range(REPLAYS):
                    for i in (0, 1):
                        ts[i].append(replay_us(torch, graphs[i]))
                med = [statistics.median(t) for t in ts]
                spread = max((max(t) - min(t)) / statistics.median(t) for t in ts)
                r = {"precision": "fp32" if split else "bf16", "k": k, "hw": hw, "C": C, "B": B,
                     "tiled_us": round(med[0], 2), "tiled_min": round(min(ts[0]), 2), "tiled_max": round(max(ts[0]), 2),
                     "gconv_us": round(med[1], 2), "gconv_min": round(min(ts[1]), 2), "gconv_max": round(max(ts[1]), 2),
                     "spread": round(spread, 3), "gconv_over_tiled": round(med[1] / med[0], 3),
                     "tiled_wins": bool(med[0] < med[1] * (1 - spread))}
                rows.append(r)
                print(json.dumps(r), flush=True)
    lines = ["| precision | window | map x C | B | tiled us [min, max] | gconv us [min, max] | spread | gconv / tiled | tiled wins |",
             "|---|---|---|---:|---:|---:|---:|---:|---|"]
    for r in rows:
        lines.append("| %s | %dx%d | %dx%dx%d | %d | %.1f [%.1f, %.1f] | %.1f [%.1f, %.1f] | %.1f%% | %.2f | %s |" % (
            r["precision"], r["k"], r["k"], r["hw"], r["hw"], r["C"], r["B"], r["tiled_us"], r["tiled_min"], r["tiled_max"],
            r["gconv_us"], r["gconv_min"], r["gconv_max"], 100 * r["spread"], r["gconv_over_tiled"],
            "yes" if r["tiled_wins"] else "no"))
    text = "\n".join(lines) + "\n"
    print(text)
    if a.md:
        open(a.md, "w").write(text)
    if a.json:
        json.dump(rows, open(a.json, "w"), indent=1)


if __name__ == "__main__":
    main()
