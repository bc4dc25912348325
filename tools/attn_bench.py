#!/usr/bin/env python3
"""Streaming-attention variants (kernels.h set_attention_variant: 0 default, 1 K/V two tiles ahead,
2 without the XCD-aware pair mapping) and masked modes on ViT-B/16's attention: packed
QKV rows [B * 197, 3 * 768] as the fused QKV GEMM writes them, 12 heads of 64, fp32 split mode and
bf16; each a captured hipGraph of 20 launches, median of 5 trials; outputs checked against the
default variant (bitwise) and against torch float64.

--mask takes a comma-separated list of
  none        the unmasked kernel (all three variants, as before)
  bias        one fp32 [S, S] table shared by the heads
  bias_heads  a per-head [H, S, S] table
  causal      the causal flag (no table); at long S compare its time to `none`: a block fetches
              only the key tiles up to its last query and a wave skips the tiles past its own
  keypad      the per-sample key (padding) mask: sample i sees the first ceil(fill_i * S) keys, its
              key data (kvis, kend) as embed_tokens writes it; a block walks only the key tiles
              below kend[i], so compare its time to `none` and to `keypad_table`
  keypad_table  the same mask through the BIAS mode, as a shared [1, S, S] table (the first fill
              value for every sample: one table serves the whole batch)
--fill (repeatable) gives the visible fraction per sample of the keypad modes, a comma-separated
list cycled over the batch; each --fill is one measured case (default: 1.0).
The masked modes run the default variant only (they have no two-tiles-ahead instantiation).

  python tools/attn_bench.py [--batch 32] [--seq 197] [--mask none,bias,bias_heads,causal,keypad,keypad_table]
                             [--fill 1.0 --fill 0.5 --fill 1.0,0.5,0.25] [--md out.md]
"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

MASKS = ("none", "bias", "bias_heads", "causal", "keypad", "keypad_table")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--seq", type=int, default=197)
    ap.add_argument("--heads", type=int, default=12)
    ap.add_argument("--mask", default="none", help="comma-separated: " + ", ".join(MASKS))
    ap.add_argument("--fill", action="append", default=None,
                    help="keypad modes: visible fraction per sample, comma-separated, cycled; repeatable")
    ap.add_argument("--md", default="")
    a = ap.parse_args()
    fills = [[float(f) for f in spec.split(",") if f] for spec in (a.fill or ["1.0"])]
    masks = [m for m in a.mask.split(",") if m]
    for m in masks:
        if m not in MASKS:
            ap.error("unknown mask mode %r" % m)
    import numpy as np
    import torch

    import die_amd  # noqa: F401
    from die_amd import native
    from die_amd.ops import kernels as K

    B, S, H, D = a.batch, a.seq, a.heads, 64
    C = H * D
    Sp = (S + 31) // 32 * 32
    LOG2E = 1.4426950408889634
    qkv = torch.randn(B, S, 3 * C, device="cuda")
    q, k, v = (qkv[..., i * C:(i + 1) * C].double().reshape(B, S, H, D).transpose(1, 2) for i in range(3))
    scores = q @ k.transpose(-1, -2) / np.sqrt(D)
    L = native.kernels()
    lines = ["# Streaming attention, B=%d S=%d H=%d D=64 (MI355X)" % (B, S, H), "",
             "| mode | mask | variant | us | rel err vs fp64 | bitwise = variant 0 |", "|---|---|---:|---:|---:|---|"]
    cases = []
    for m in masks:
        cases += [(m, f) for f in fills] if m.startswith("keypad") else [(m, None)]
    for mask, fill in cases:
        label = mask
        kvis = kend = None
        if fill is not None:
            if mask == "keypad_table":
                fill = fill[:1]
            label = "%s fill %s" % (mask, ",".join("%g" % f for f in fill))
            n_vis = torch.tensor([max(1, min(S, int(np.ceil(fill[i % len(fill)] * S)))) for i in range(B)], device="cuda")
            visible = torch.arange(S, device="cuda")[None, :] < n_vis[:, None]  # [B, S]
        # the additive term of the float64 reference and the kernel's table ([Hb][S][Sp], exp2 units)
        bias_nat = None
        if mask == "bias":
            bias_nat = torch.randn(1, S, S, device="cuda")
        elif mask == "bias_heads":
            bias_nat = torch.randn(H, S, S, device="cuda")
        term = bias_nat.double() if bias_nat is not None else 0.0
        if mask == "causal":
            i = torch.arange(S, device="cuda")
            term = torch.where(i[None, :] <= i[:, None], 0.0, -float("inf")).double()
        if mask == "keypad":
            kvis, kend = K.key_mask_data(visible)
            term = torch.where(visible, 0.0, -float("inf")).double()[:, None, None, :]
        if mask == "keypad_table":
            bias_nat = torch.where(visible[0], 0.0, -float("inf"))[None, None, :].expand(1, S, S).contiguous()
            term = bias_nat.double()
        ref = (torch.softmax(scores + term, -1) @ v).transpose(1, 2).reshape(B, S, C)
        table, hb = None, 0
        if bias_nat is not None:
            hb = bias_nat.shape[0]
            table = torch.zeros(hb, S, Sp, device="cuda")
            table[..., :S] = bias_nat * LOG2E
        for split in (True, False):
            if split:
                src = K.split_planes(qkv)  # [2, B, S, 3C] bf16
                out = torch.empty((2, B, S, C), dtype=torch.bfloat16, device="cuda")
            else:
                src = qkv.to(torch.bfloat16).contiguous()
                out = torch.empty((B, S, C), dtype=torch.bfloat16, device="cuda")
            base = src.data_ptr()

            geom = dict(q=base, k=base + 2 * C, v=base + 4 * C, out=out.data_ptr(), B=B, S=S, H=H, D=D, ldq=3 * C, ldk=3 * C,
                        ldv=3 * C, ldo=C, scale=float(1 / np.sqrt(D)), split=int(split))
            if mask == "keypad":
                geom.update(Sp=Sp, kvis=kvis.data_ptr(), kend=kend.data_ptr())
            elif mask != "none":
                geom.update(bias=table.data_ptr() if table is not None else 0, bias_heads=hb,
                            Sp=Sp if table is not None else 0, causal=int(mask == "causal"))
            geom = native.geometry(geom)

            def launch():
                rc = L.die_kern_attention(geom, torch.cuda.current_stream().cuda_stream)
                assert rc == 0, rc

            first = None
            for var in (0, 1, 2) if mask == "none" else (0,):
                K.set_attention_variant(var)
                launch()
                torch.cuda.synchronize()
                res = (K.join_planes(out) if split else out.float()).clone()
                err = float((res.double() - ref).norm() / ref.norm())
                same = "-" if first is None else str(bool(torch.equal(res, first)))
                if first is None:
                    first = res
                g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g):
                    for _ in range(20):
                        launch()
                g.replay()
                torch.cuda.synchronize()
                ts = []
                for _ in range(5):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    g.replay()
                    e1.record()
                    e1.synchronize()
                    ts.append(e0.elapsed_time(e1) * 1000 / 20)
                lines.append("| %s | %s | %d | %.2f | %.1e | %s |" % ("fp32 split" if split else "bf16", label, var,
                                                                       statistics.median(ts), err, same))
                print(lines[-1], flush=True)
            K.set_attention_variant(0)
    if a.md:
        open(a.md, "w").write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
