#!/usr/bin/env python3
"""The GroupNorm kernels (kernels/groupnorm.hip: statistics, merge and apply launches of one kern::group_norm
call) on the device, in both storage formats, at batch 1 and 8: 64x64x128, 32x32x320, 16x16x640, 8x8x1280
and 56x56x256, all with 32 groups, gamma + beta, SiLU.

Each figure is a captured hipGraph of 20 calls on preallocated buffers (warm: the same input every call), in
microseconds of device time per call: the median [min, max] of 9 replays, ours and the yardstick's replays
interleaved in one process.  Yardsticks, none of them the code under test:
  1. bytes: x read twice and y written once in the storage format used (bf16: 2 bytes per element; split
     fp32: two planes, 4 bytes), over the MI355X's achievable HBM streaming rate (6.3 TB/s) and the rate it reads
     from the Infinity Cache (8.6 TB/s);
  2. torch.nn.functional.group_norm + silu on a channels_last tensor of the same shape: bf16 for the bf16
     format, fp32 for the split format;
  3. (--models) the per-op profile of gn_resnet and gn_decoder at B = 8 on this tree (the parent cannot run
     them: see profiles/groupnorm.md).

  python tools/groupnorm_bench.py [--md out.md] [--json out.json] [--models]
"""
import argparse
import json
import os
import statistics
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (H = W, C, G)
SHAPES = ((64, 128, 32), (32, 320, 32), (16, 640, 32), (8, 1280, 32), (56, 256, 32))
BATCHES = (1, 8)
LAUNCHES, REPLAYS = 20, 9
HBM_TBS, MALL_TBS = 6.3, 8.6


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


def kernel_rows(torch, native, K):
    L = native.kernels()
    rows = []
    for split in (True, False):
        for hw, C, G in SHAPES:
            for B in BATCHES:
                g = torch.Generator(device="cuda").manual_seed(hw + C)
                x = torch.randn(B, hw, hw, C, device="cuda", generator=g)
                gamma = torch.rand(C, device="cuda", generator=g) + 0.5
                beta = torch.randn(C, device="cuda", generator=g)
                xin = K.split_planes(x) if split else x.to(torch.bfloat16).contiguous()
                out = torch.zeros_like(xin)
                nws = int(L.die_groupnorm_workspace_bytes(B, hw * hw, C, G))
                ws = torch.empty(nws // 4, dtype=torch.float32, device="cuda")
                geom = json.dumps(dict(B=B, HW=hw * hw, C=C, Cl=C, G=G, eps=1e-5, act=2, split=int(split),
                                       ws_bytes=nws)).encode()
                # the yardstick: torch on a channels_last tensor (NCHW logical shape, NHWC memory)
                xt = (x if split else x.to(torch.bfloat16)).permute(0, 3, 1, 2)
                gt, bt = (gamma, beta) if split else (gamma.to(torch.bfloat16), beta.to(torch.bfloat16))
                keep = [None]

                def ours():  # on the current stream: the capture stream inside torch.cuda.graph
                    rc = L.die_kern_groupnorm(geom, xin.data_ptr(), gamma.data_ptr(), beta.data_ptr(), out.data_ptr(),
                                              ws.data_ptr(), 0, int(torch.cuda.current_stream().cuda_stream))
                    assert rc == 0, rc

                def theirs():
                    keep[0] = torch.nn.functional.silu(torch.nn.functional.group_norm(xt, G, gt, bt, 1e-5))

                graphs = [capture(torch, ours), capture(torch, theirs)]
                got = (K.join_planes(out) if split else out.float()).permute(0, 3, 1, 2)
                err = float((got.double() - keep[0].double()).norm() / keep[0].double().norm())
                assert err < (1e-4 if split else 3e-2), (hw, C, B, split, err)  # the same function (torch's own rounding)
                ts = [[], []]
                for _ in range(REPLAYS):
                    for i in (0, 1):
                        ts[i].append(replay_us(torch, graphs[i]))
                med = [statistics.median(t) for t in ts]
                nbytes = 3 * B * hw * hw * C * (4 if split else 2)
                r = {"precision": "fp32" if split else "bf16", "hw": hw, "C": C, "G": G, "B": B, "mbytes": round(nbytes / 1e6, 2),
                     "ours_us": round(med[0], 2), "ours_min": round(min(ts[0]), 2), "ours_max": round(max(ts[0]), 2),
                     "torch_us": round(med[1], 2), "torch_min": round(min(ts[1]), 2), "torch_max": round(max(ts[1]), 2),
                     "hbm_us": round(nbytes / (HBM_TBS * 1e6), 2), "mall_us": round(nbytes / (MALL_TBS * 1e6), 2),
                     "torch_over_ours": round(med[1] / med[0], 2),
                     "share_of_mall_rate": round(nbytes / (MALL_TBS * 1e6) / med[0], 3)}
                rows.append(r)
                print(json.dumps(r), flush=True)
    return rows


def model_rows(native, M, tmp):
    rows = []
    for name in ("gn_resnet", "gn_decoder"):
        p = os.path.join(tmp, name + ".onnx")
        open(p, "wb").write(M.BUILDERS[name](0)[0])
        eng = native.Engine(p, device="hip", max_batch=8, precision="fp32")
        try:
            eng.run(M.synthetic_input(name, 8).reshape(8, -1))
            prof = eng.profile(8, iters=20)
            by_kind = {}
            for o in prof["ops"]:
                by_kind[o["kind"]] = by_kind.get(o["kind"], 0.0) + o["us"]
            top = max(prof["ops"], key=lambda o: o["us"])
            r = {"model": name, "batch": prof["batch"], "total_us": round(prof["total_us"], 1),
                 "us_by_kind": {k: round(v, 1) for k, v in sorted(by_kind.items(), key=lambda kv: -kv[1])},
                 "slowest_op": [top["kind"], top["name"], round(top["us"], 1)],
                 "groupnorm_ops": [[o["name"], o["groups"], o["channels"], o["pixels"], round(o["us"], 1)]
                                   for o in prof["ops"] if o["kind"] == "groupnorm"]}
            rows.append(r)
            print(json.dumps(r), flush=True)
        finally:
            eng.close()
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--md", default="")
    ap.add_argument("--json", default="")
    ap.add_argument("--models", action="store_true")
    a = ap.parse_args()
    sys.path.insert(0, HERE)
    import tempfile

    import torch

    import die_amd  # noqa: F401
    from die_amd import native
    from die_amd.models import groupnorm as M
    from die_amd.ops import kernels as K

    if not torch.cuda.is_available():
        sys.exit("groupnorm_bench needs a GPU: device times are not measured anywhere else")
    rows = kernel_rows(torch, native, K)
    lines = ["| format | map x C (G) | B | MB moved | ours us [min, max] | torch us [min, max] | HBM-rate us | cache-rate us | torch / ours |",
             "|---|---|---:|---:|---:|---:|---:|---:|---:|"]
    for r in rows:
        lines.append("| %s | %dx%dx%d (%d) | %d | %.2f | %.1f [%.1f, %.1f] | %.1f [%.1f, %.1f] | %.2f | %.2f | %.2f |" % (
            r["precision"], r["hw"], r["hw"], r["C"], r["G"], r["B"], r["mbytes"], r["ours_us"], r["ours_min"], r["ours_max"],
            r["torch_us"], r["torch_min"], r["torch_max"], r["hbm_us"], r["mall_us"], r["torch_over_ours"]))
    models = []
    if a.models:
        with tempfile.TemporaryDirectory() as tmp:
            models = model_rows(native, M, tmp)
        for r in models:
            lines += ["", "%s, B = %d, fp32: %.1f us over all ops; by kind %s; slowest op %s" % (
                r["model"], r["batch"], r["total_us"], json.dumps(r["us_by_kind"]), json.dumps(r["slowest_op"]))]
    text = "\n".join(lines) + "\n"
    print(text)
    if a.md:
        open(a.md, "w").write(text)
    if a.json:
        json.dump({"kernels": rows, "models": models}, open(a.json, "w"), indent=1)


if __name__ == "__main__":
    main()
