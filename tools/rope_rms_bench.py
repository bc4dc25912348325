#!/usr/bin/env python3
"""rope_rows and layernorm_rows in RMS mode (kernels/transformer.hip) device time, in both precisions:
the shapes of the generated models at batch 32 and serving-size ones whose rows do not fit the
Infinity Cache.  Each figure: a captured hipGraph of 50 launches on preallocated buffers, the median
of 7 replays; results are checked against float64 torch first.  Bytes = rows read + rows written +
tables (gamma), both planes in fp32 mode.

  python tools/rope_rms_bench.py [--md out.md]
"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

# (B, S, H, D, fused): fused = the K block of a [Q | K | V] buffer (ldx = 3 H D)
ROPE_SHAPES = ((32, 160, 4, 32, False), (32, 24, 2, 128, True), (32, 512, 12, 64, True), (32, 512, 32, 128, False))
RMS_SHAPES = ((32 * 160, 128), (32 * 512, 768), (32 * 512, 2048), (32 * 512, 4096))  # (rows, C); 4096: block per row
LAUNCHES, REPLAYS = 50, 7


def timed(torch, launch):
    launch()
    torch.cuda.synchronize()
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gr):
        for _ in range(LAUNCHES):
            launch()
    gr.replay()
    torch.cuda.synchronize()
    ts = []
    for _ in range(REPLAYS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        gr.replay()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1) * 1000 / LAUNCHES)
    return statistics.median(ts), min(ts), max(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--md", default="")
    a = ap.parse_args()
    import torch

    import die_amd  # noqa: F401
    from die_amd import native
    from die_amd.models import generic as G
    from die_amd.ops import kernels as K

    L = native.kernels()

    def st():  # the stream of the moment: torch captures on a side stream
        return int(torch.cuda.current_stream().cuda_stream)

    lines = ["# rope_rows / RMS layernorm_rows device time (MI355X; hipGraph of %d launches, median [min, max] of %d replays)"
             % (LAUNCHES, REPLAYS), "", "| op | shape | mode | us | MB moved | GB/s | rel err |", "|---|---|---|---:|---:|---:|---:|"]
    for B, S, H, D, fused in ROPE_SHAPES:
        W, rows = H * D, B * S
        ldx, col = (3 * W, W) if fused else (W, 0)
        x32 = torch.randn(rows, ldx, device="cuda")
        cos, sin = (torch.from_numpy(t).cuda() for t in G.rope_tables(S, D))
        for split in (True, False):
            xin = K.split_planes(x32) if split else x32.to(torch.bfloat16).contiguous()
            y = torch.empty(((2,) if split else ()) + (rows, W), dtype=torch.bfloat16, device="cuda")

            def rope():
                rc = L.die_kern_rope_rows(int(xin.data_ptr()) + 2 * col, int(y.data_ptr()), int(cos.data_ptr()),
                                          int(sin.data_ptr()), B, S, H, D, ldx, W, st(), int(split))
                assert rc == 0, rc

            rope()
            xs = (K.join_planes(xin) if split else xin.float()).double()[:, col:col + W].reshape(B, S, H, D)
            c, s = cos.double()[None, :, None, :], sin.double()[None, :, None, :]
            rot = torch.cat([-xs[..., D // 2:], xs[..., :D // 2]], dim=-1)
            ref = xs * c + rot * s
            got = (K.join_planes(y) if split else y.float()).double().reshape(B, S, H, D)
            err = float((got - ref).norm() / ref.norm())
            us, lo, hi = timed(torch, rope)
            mb = (2 * rows * W * 2 * (2 if split else 1) + 2 * S * D * 4) / 1e6
            lines.append("| rope_rows | B %d S %d H %d D %d ldx %d | %s | %.2f [%.2f, %.2f] | %.2f | %.0f | %.1e |" % (
                B, S, H, D, ldx, "fp32 split" if split else "bf16", us, lo, hi, mb, mb / us * 1e3, err))
            print(lines[-1], flush=True)
    for rows, C in RMS_SHAPES:
        x32 = torch.randn(rows, C, device="cuda") + 3.0
        g = (1.0 + 0.1 * torch.randn(C, device="cuda")).float().contiguous()
        for split in (True, False):
            xin = K.split_planes(x32) if split else x32.to(torch.bfloat16).contiguous()
            y = torch.empty(((2,) if split else ()) + (rows, C), dtype=torch.bfloat16, device="cuda")
            for rms in (1, 0):  # the LayerNorm mode of the same kernel at the same shape beside it
                def norm():
                    rc = L.die_kern_layernorm(int(xin.data_ptr()), int(y.data_ptr()), int(g.data_ptr()), int(g.data_ptr()), 1e-6,
                                              rows, C, st(), int(split), 0, 0, 0, rms)
                    assert rc == 0, rc

                norm()
                xs = (K.join_planes(xin) if split else xin.float()).double()
                if rms:
                    ref = xs / torch.sqrt((xs ** 2).mean(1, keepdim=True) + 1e-6) * g.double()
                else:
                    mu = xs.mean(1, keepdim=True)
                    ref = (xs - mu) / torch.sqrt(((xs - mu) ** 2).mean(1, keepdim=True) + 1e-6) * g.double() + g.double()
                got = (K.join_planes(y) if split else y.float()).double()
                err = float((got - ref).norm() / ref.norm())
                us, lo, hi = timed(torch, norm)
                mb = (2 * rows * C * 2 * (2 if split else 1) + C * 4) / 1e6
                lines.append("| layernorm_rows %s | rows %d C %d | %s | %.2f [%.2f, %.2f] | %.2f | %.0f | %.1e |" % (
                    "rms" if rms else "(LayerNorm mode)", rows, C, "fp32 split" if split else "bf16", us, lo, hi, mb,
                    mb / us * 1e3, err))
                print(lines[-1], flush=True)
    if a.md:
        os.makedirs(os.path.dirname(os.path.abspath(a.md)), exist_ok=True)
        open(a.md, "w").write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
