#!/usr/bin/env python3
"""pool_tokens (kernels/transformer.hip) device time: the masked mean over the visible tokens + L2
normalisation at sentence-embedder shapes, in both precisions, at several fills (the share of each
sequence that is visible), with the existing global_avgpool token mean (all S rows, no mask, no
normalisation) at the same shapes as the yardstick.  Each figure: a captured hipGraph of 50 launches
on preallocated buffers, the median of 7 replays; results are checked against float64 torch first.

  python tools/pool_bench.py [--md out.md]
"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = ((8, 128, 384), (32, 512, 768))
FILLS = (1.0, 0.5, 0.25)
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
    from die_amd.ops import kernels as K

    L = native.kernels()

    def st():  # the stream of the moment: torch captures on a side stream
        return int(torch.cuda.current_stream().cuda_stream)

    lines = ["# pool_tokens device time (MI355X; hipGraph of %d launches, median [min, max] of %d replays)" % (LAUNCHES, REPLAYS),
             "", "| B | S | D | mode | op | fill | us | rows read GB/s | rel err |", "|---:|---:|---:|---|---|---:|---:|---:|---:|"]
    for B, S, D in SHAPES:
        x32 = torch.randn(B, S, D, device="cuda") + 0.25
        for split in (True, False):
            xin = K.split_planes(x32) if split else x32.to(torch.bfloat16).contiguous()
            stored = (K.join_planes(xin) if split else xin.float()).double()
            out = torch.empty(((2,) if split else ()) + (B, D), dtype=torch.bfloat16, device="cuda")
            out32 = torch.empty((B, D), dtype=torch.float32, device="cuda")
            ws_bytes = int(L.die_kern_pool_tokens_ws_bytes(B, D))
            ws = torch.empty((ws_bytes // 4,), dtype=torch.float32, device="cuda")
            counters = torch.zeros((B,), dtype=torch.int32, device="cuda")
            mode = "fp32 split" if split else "bf16"
            plane_bytes = 2 * (2 if split else 1)

            def gap():
                rc = L.die_kern_gap(int(xin.data_ptr()), int(out.data_ptr()), int(out32.data_ptr()), 0, 0, 0, B, S, D, st(), int(split),
                                    0, 0)
                assert rc == 0, rc

            gap()
            ref = stored.mean(1)
            err = float((out32.double() - ref).norm() / ref.norm())
            us, lo, hi = timed(torch, gap)
            lines.append("| %d | %d | %d | %s | global_avgpool (token mean) | 1.00 | %.2f [%.2f, %.2f] | %.0f | %.1e |" % (
                B, S, D, mode, us, lo, hi, B * S * D * plane_bytes / us / 1e3, err))
            print(lines[-1], flush=True)
            for normalize in (0, 1):
                for fill in FILLS:
                    n = max(1, int(round(S * fill)))
                    vis = torch.zeros((B, S), dtype=torch.bool, device="cuda")
                    vis[:, :n] = True
                    kvis, kend = K.key_mask_data(vis)

                    geom = native.geometry(dict(x=int(xin.data_ptr()), out=int(out.data_ptr()), out_f32=int(out32.data_ptr()), B=B,
                                                S=S, C=D, D=D, kvis=int(kvis.data_ptr()), kend=int(kend.data_ptr()),
                                                Sp=int(kvis.shape[1]), clip_min=1e-9, normalize=normalize, eps=1e-12,
                                                split=int(split), ws=int(ws.data_ptr()), ws_bytes=ws_bytes,
                                                counters=int(counters.data_ptr()), counters_n=B))

                    def pool():
                        rc = L.die_kern_pool_tokens(geom, st())
                        assert rc == 0, rc

                    pool()
                    ref = stored[:, :n].mean(1)
                    if normalize:
                        ref = ref / ref.norm(dim=1, keepdim=True)
                    err = float((out32.double() - ref).norm() / ref.norm())
                    us, lo, hi = timed(torch, pool)
                    assert int(counters.abs().sum()) == 0
                    lines.append("| %d | %d | %d | %s | pool_tokens masked%s | %.2f | %.2f [%.2f, %.2f] | %.0f | %.1e |" % (
                        B, S, D, mode, " + normalize" if normalize else "", fill, us, lo, hi,
                        B * n * D * plane_bytes / us / 1e3, err))
                    print(lines[-1], flush=True)
    if a.md:
        open(a.md, "w").write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
