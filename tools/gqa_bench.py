#!/usr/bin/env python3
"""Grouped-query attention on the device, in both precisions.

Kernel section: the GQA mode of the streaming attention kernel (kernels/transformer.hip) against the
per-head kernel run on K / V physically repeated to H heads, at the shapes of `gqa_enc` and `gqa_hd128`
at batch 32 and one serving-size shape, unmasked and causal.  Each figure: a captured hipGraph of 20
launches on preallocated buffers, the median [min, max] of 7 replays; both results are checked against
float64 torch first.  Blocks launched and the K / V bytes a block stages (every key tile it walks, both
planes in fp32 mode) are listed for both.

Forward section: the in-graph device time of one forward at batch 32 of each GQA model and of its
`expand_kv` multi-head twin (Engine.run on a fixed batch, the engine's device_busy_ms counter over
`--runs` forwards after a warm-up).  --tree DIR imports the engine of another checkout of this
repository (to time the twins on an earlier commit); --models then names the ONNX files to time, which
--write-models DIR produces.

  python tools/gqa_bench.py [--md out.md] [--json out.json] [--section kernel|forward|all]
"""
import argparse
import json
import os
import statistics
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (B, S, H, Hkv, D)
KERNEL_SHAPES = ((32, 160, 4, 2, 64), (32, 40, 6, 2, 128), (4, 2048, 32, 8, 128))
LAUNCHES, REPLAYS = 20, 7
MODELS = ("gqa_enc", "mqa_causal", "gqa_hd128")


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


def kernel_section(lines, results):
    import math

    import torch

    from die_amd import native
    from die_amd.ops import kernels as K

    L = native.kernels()

    def st():  # the stream of the moment: torch captures on a side stream
        return int(torch.cuda.current_stream().cuda_stream)

    lines += ["## Kernel time (MI355X; hipGraph of %d launches, median [min, max] of %d replays)" % (LAUNCHES, REPLAYS), "",
              "| shape | mode | precision | mapping | blocks | K/V staged per block | us | rel err vs float64 |",
              "|---|---|---|---|---:|---:|---:|---:|"]
    for B, S, H, Hkv, D in KERNEL_SHAPES:
        G, C, Ckv = H // Hkv, H * D, Hkv * D
        nqt = (S + 31) // 32
        qkv = torch.randn(B, S, C + 2 * Ckv, device="cuda")
        k = qkv[..., C:C + Ckv].reshape(B, S, Hkv, D).repeat_interleave(G, dim=2).reshape(B, S, C)
        v = qkv[..., C + Ckv:].reshape(B, S, Hkv, D).repeat_interleave(G, dim=2).reshape(B, S, C)
        rep = torch.cat([qkv[..., :C], k, v], dim=-1).contiguous()
        scale = 1.0 / math.sqrt(D)
        q64, k64, v64 = (rep[..., i * C:(i + 1) * C].double().reshape(B, S, H, D).transpose(1, 2) for i in range(3))
        for causal in (0, 1):
            sc = q64 @ k64.transpose(-1, -2) * scale
            if causal:
                sc = sc.masked_fill(~torch.ones(S, S, dtype=torch.bool, device="cuda").tril(), -math.inf)
            ref = (torch.softmax(sc, -1) @ v64).transpose(1, 2).reshape(B, S, C)
            del sc
            for split in (1, 0):
                planes = 2 if split else 1
                for gqa in (1, 0):
                    src = qkv if gqa else rep
                    xin = K.split_planes(src) if split else src.to(torch.bfloat16).contiguous()
                    ld = src.shape[-1]
                    kw = Ckv if gqa else C
                    out = torch.empty(((2,) if split else ()) + (B, S, C), dtype=torch.bfloat16, device="cuda")
                    base = int(xin.data_ptr())

                    geom = native.geometry(dict(q=base, k=base + 2 * C, v=base + 2 * (C + kw), out=int(out.data_ptr()), B=B, S=S,
                                                H=H, D=D, ldq=ld, ldk=ld, ldv=ld, ldo=C, scale=scale, split=split,
                                                causal=causal, kv_heads=Hkv if gqa else H))

                    def attn():
                        rc = L.die_kern_attention(geom, st())
                        assert rc == 0, rc

                    attn()
                    got = (K.join_planes(out) if split else out.float()).double()
                    err = float((got - ref).norm() / ref.norm())
                    us, lo, hi = timed(torch, attn)
                    if gqa:
                        nb = (nqt * G + 3) // 4
                        blocks = nb * Hkv * B
                        # tiles walked by a block: causal = up to its last item's query tile, averaged over the blocks
                        tiles = sum(min(nqt - 1, (4 * b + 3) // G) + 1 for b in range(nb)) / nb if causal else nqt
                    else:
                        nb = (S + 127) // 128
                        blocks = nb * H * B
                        tiles = sum(min(nqt, 4 * b + 4) for b in range(nb)) / nb if causal else nqt
                    staged = tiles * 32 * D * 2 * 2 * planes  # K and V, bf16, per plane
                    row = dict(B=B, S=S, H=H, Hkv=Hkv, D=D, causal=bool(causal), precision="fp32" if split else "bf16",
                               mapping="gqa" if gqa else "per-head on repeated K/V", blocks=blocks, staged_bytes_per_block=staged,
                               us=us, us_min=lo, us_max=hi, rel_err=err)
                    results["kernel"].append(row)
                    lines.append("| B %d S %d H %d Hkv %d D %d | %s | %s | %s | %d | %.0f KiB | %.2f [%.2f, %.2f] | %.1e |" % (
                        B, S, H, Hkv, D, "causal" if causal else "unmasked", row["precision"], row["mapping"], blocks,
                        staged / 1024, us, lo, hi, err))
                    print(lines[-1], flush=True)
    lines.append("")


def forward_time(native, path, x, runs, precision):
    eng = native.Engine(path, device="hip", max_batch=len(x), precision=precision)
    try:
        for _ in range(5):
            eng.run(x)
        t0 = eng.refresh_info()["device_busy_ms"]
        for _ in range(runs):
            eng.run(x)
        t1 = eng.refresh_info()["device_busy_ms"]
        return (t1 - t0) / runs
    finally:
        eng.close()


def forward_section(lines, results, a):
    import numpy as np

    from die_amd import native

    files = []
    if a.models:
        for p in a.models:
            files.append((os.path.splitext(os.path.basename(p))[0], p, np.load(os.path.splitext(p)[0] + ".input.npy")))
    else:
        import tempfile

        from die_amd.models import generic as G

        d = a.write_models or tempfile.mkdtemp(prefix="gqa_bench_")
        os.makedirs(d, exist_ok=True)
        for name in MODELS:
            x = G.synthetic_input(name, 32, seed=7)
            x = x.reshape(32, -1)
            for twin in (False, True):
                tag = name + ("_mha" if twin else "")
                p = os.path.join(d, tag + ".onnx")
                open(p, "wb").write(G.BUILDERS[name](0, expand_kv=twin)[0])
                np.save(os.path.join(d, tag + ".input.npy"), x)
                files.append((tag, p, x))
        if a.write_models:
            return
    lines += ["## Forward device time at batch 32 (ms per forward, %d forwards per figure; tree: %s)" % (a.runs, a.label), "",
              "| model | precision | ms |", "|---|---|---:|"]
    for tag, p, x in files:
        for precision in ("fp32", "bf16"):
            ms = forward_time(native, p, x, a.runs, precision)
            results["forward"].append(dict(model=tag, precision=precision, ms=ms, tree=a.label))
            lines.append("| %s | %s | %.4f |" % (tag, precision, ms))
            print(lines[-1], flush=True)
    lines.append("")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--md", default="")
    ap.add_argument("--json", default="")
    ap.add_argument("--section", choices=["kernel", "forward", "all"], default="all")
    ap.add_argument("--tree", default=HERE, help="checkout whose engine is imported (default: this one)")
    ap.add_argument("--label", default="this tree")
    ap.add_argument("--models", nargs="*", default=[], help="ONNX files to time (with NAME.input.npy next to each)")
    ap.add_argument("--write-models", default="", metavar="DIR", help="write the models and inputs there and stop")
    ap.add_argument("--runs", type=int, default=200)
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.tree))
    import die_amd  # noqa: F401

    lines, results = ["# Grouped-query attention: device time", ""], dict(kernel=[], forward=[])
    if a.section in ("kernel", "all") and not a.write_models:
        kernel_section(lines, results)
    if a.section in ("forward", "all") or a.write_models:
        forward_section(lines, results, a)
    if a.md:
        os.makedirs(os.path.dirname(os.path.abspath(a.md)), exist_ok=True)
        open(a.md, "w").write("\n".join(lines) + "\n")
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        json.dump(results, open(a.json, "w"), indent=1)


if __name__ == "__main__":
    main()
