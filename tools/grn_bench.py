#!/usr/bin/env python3
"""The Global Response Normalization kernels (kernels/grn.hip, one kern::grn call) on the device, in both
storage formats, on every GRN map of ConvNeXt-V2-Atto (56x56x160 ... 7x7x1280) and ConvNeXt-V2-T (56x56x384
... 7x7x3072) at batch 1, 8 and 32, with gamma and beta.

Each figure is a captured hipGraph of 20 calls on preallocated buffers (warm: the same input every call), in
microseconds of device time per call: the median [min, max] of 9 replays, all candidates' replays interleaved
in one process.  Yardsticks, none of them the code under test:
  1. bytes: x read twice and y written once in the storage format used (bf16: 2 bytes per element; split
     fp32: two planes, 4 bytes), as achieved bytes/s and against the MI355X's achievable HBM streaming rate
     (6.3 TB/s);
  2. kern::group_norm with G = 1 and no activation on the same map where it can run (C <= 2048): the same
     bytes with more arithmetic;
  3. torch eager evaluating the exported expression on a contiguous [B,H,W,C] tensor: bf16 for the bf16 format,
     fp32 for the split format.
--forms: the one-launch form against the three launches (GrnArgs::form) on maps of 256 ... 8192 16-byte
         chunks per sample, the measurement behind the kernel's fused-form bound.
--models: the per-op profile of ConvNeXt-V2-T at B = 32 in both precisions and of Atto, GRN's share of the
          forward, and the forward of ConvNeXt-V2-T at B = 8 through Engine.run.

  python tools/grn_bench.py [--md out.md] [--json out.json] [--forms] [--models] [--quick]
"""
import argparse
import json
import os
import statistics
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (model, H = W, C): the hidden width 4 * dim of each stage
MAPS = (("atto", 56, 160), ("atto", 28, 320), ("atto", 14, 640), ("atto", 7, 1280),
        ("v2-t", 56, 384), ("v2-t", 28, 768), ("v2-t", 14, 1536), ("v2-t", 7, 3072))
BATCHES = (1, 8, 32)
# (H, W, C) for --forms: 32 and 128 chunks per pixel, 256 ... 8192 chunks per sample, and stage 4 of both models
FORM_MAPS = ((2, 4, 256), (4, 4, 256), (4, 8, 256), (8, 8, 256), (8, 16, 256), (16, 16, 256),
             (1, 2, 1024), (2, 2, 1024), (2, 4, 1024), (4, 4, 1024), (4, 8, 1024), (7, 7, 1280), (7, 7, 3072))
LAUNCHES, REPLAYS = 20, 9
HBM_TBS = 6.3


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


def interleaved(torch, graphs):
    ts = [[] for _ in graphs]
    for _ in range(REPLAYS):
        for i, gr in enumerate(graphs):
            ts[i].append(replay_us(torch, gr))
    return [(round(statistics.median(t), 2), round(min(t), 2), round(max(t), 2)) for t in ts]


def setup(torch, K, L, B, H, W, C, split):
    g = torch.Generator(device="cuda").manual_seed(H * W + C)
    x = torch.randn(B, H, W, C, device="cuda", generator=g)
    gamma = torch.rand(C, device="cuda", generator=g) + 0.5
    beta = torch.randn(C, device="cuda", generator=g) * 0.1
    xin = K.split_planes(x) if split else x.to(torch.bfloat16).contiguous()
    out = torch.zeros_like(xin)
    nws = int(L.die_grn_workspace_bytes(B, H * W, C))
    ws = torch.empty(nws // 4, dtype=torch.float32, device="cuda")

    def grn(form=0):
        geom = json.dumps(dict(B=B, HW=H * W, C=C, eps=1e-6, split=int(split), ws_bytes=nws, form=form)).encode()

        def launch():  # on the current stream: the capture stream inside torch.cuda.graph
            rc = L.die_kern_grn(geom, xin.data_ptr(), gamma.data_ptr(), beta.data_ptr(), out.data_ptr(), ws.data_ptr(), 0,
                                int(torch.cuda.current_stream().cuda_stream))
            assert rc == 0, rc
        return launch

    return x, gamma, beta, xin, out, grn


def kernel_rows(torch, native, K, maps, batches):
    L = native.kernels()
    rows = []
    for split in (True, False):
        for model, hw, C in maps:
            for B in batches:
                x, gamma, beta, xin, out, grn = setup(torch, K, L, B, hw, hw, C, split)
                # torch eager on the exported expression, in the format's own dtype
                xt = x if split else x.to(torch.bfloat16)
                gt, bt = (gamma, beta) if split else (gamma.to(torch.bfloat16), beta.to(torch.bfloat16))
                keep = [None]

                def theirs():
                    G = torch.linalg.vector_norm(xt, ord=2, dim=(1, 2), keepdim=True)
                    nx = G / (G.mean(dim=-1, keepdim=True) + 1e-6)
                    keep[0] = gt * (xt * nx) + bt + xt

                names, graphs = ["grn", "torch"], [capture(torch, grn()), capture(torch, theirs)]
                got = K.join_planes(out) if split else out.float()
                err = float((got.double() - keep[0].double()).norm() / keep[0].double().norm())
                assert err < (1e-4 if split else 3e-2), (hw, C, B, split, err)  # the same function (torch's own rounding)
                if C <= 2048:  # group_norm with one group: the same bytes, more arithmetic
                    gout = torch.zeros_like(xin)
                    gws_n = int(L.die_groupnorm_workspace_bytes(B, hw * hw, C, 1))
                    gws = torch.empty(max(gws_n, 8) // 4, dtype=torch.float32, device="cuda")
                    ggeom = json.dumps(dict(B=B, HW=hw * hw, C=C, Cl=C, G=1, eps=1e-5, act=0, split=int(split),
                                            ws_bytes=gws_n)).encode()

                    def gn():
                        rc = L.die_kern_groupnorm(ggeom, xin.data_ptr(), gamma.data_ptr(), beta.data_ptr(), gout.data_ptr(),
                                                  gws.data_ptr(), 0, int(torch.cuda.current_stream().cuda_stream))
                        assert rc == 0, rc

                    names.append("group_norm")
                    graphs.append(capture(torch, gn))
                t = dict(zip(names, interleaved(torch, graphs)))
                nbytes = 3 * B * hw * hw * C * (4 if split else 2)
                r = {"precision": "fp32" if split else "bf16", "model": model, "hw": hw, "C": C, "B": B,
                     "mbytes": round(nbytes / 1e6, 2), "grn_us": t["grn"], "torch_us": t["torch"],
                     "group_norm_us": t.get("group_norm"), "tbytes_per_s": round(nbytes / t["grn"][0] / 1e6, 3),
                     "hbm_us": round(nbytes / (HBM_TBS * 1e6), 2), "torch_over_grn": round(t["torch"][0] / t["grn"][0], 2),
                     "grn_over_group_norm": round(t["grn"][0] / t["group_norm"][0], 2) if "group_norm" in t else None}
                rows.append(r)
                print(json.dumps(r), flush=True)
                del graphs
    return rows


def form_rows(torch, native, K, batches):
    L = native.kernels()
    rows = []
    for split in (True, False):
        for H, W, C in FORM_MAPS:
            for B in batches:
                _, _, _, _, out, grn = setup(torch, K, L, B, H, W, C, split)
                graphs = [capture(torch, grn(1))]
                one = out.clone()
                graphs.append(capture(torch, grn(2)))
                # the two forms add in different orders: the same function to fp32 rounding
                a, b = (K.join_planes(t) if split else t.float() for t in (one, out))
                assert float((a.double() - b.double()).norm() / b.double().norm()) < (1e-5 if split else 1e-2)
                t1, t3 = interleaved(torch, graphs)
                r = {"precision": "fp32" if split else "bf16", "H": H, "W": W, "C": C, "B": B, "chunks": H * W * C // 8,
                     "one_launch_us": t1, "three_launches_us": t3, "three_over_one": round(t3[0] / t1[0], 2)}
                rows.append(r)
                print(json.dumps(r), flush=True)
    return rows


def model_rows(torch, native, v2, tmp, quick):
    rows = []
    jobs = [("v2-t", v2.ConvNeXtV2Config(), 32, "fp32"), ("v2-t", v2.ConvNeXtV2Config(), 32, "bf16"),
            ("atto", v2.atto_config(), 32, "fp32")]
    if quick:
        jobs = [("tiny", v2.tiny_convnextv2_config(), 8, "fp32")]
    for name, cfg, B, precision in jobs:
        p = os.path.join(tmp, name + ".onnx")
        if not os.path.exists(p):
            open(p, "wb").write(v2.build_onnx(cfg)[0])
        eng = native.Engine(p, device="hip", max_batch=B, precision=precision)
        try:
            x = v2.synthetic_input(B, cfg).reshape(B, -1)
            eng.run(x)
            prof = eng.profile(B, iters=20)
            by_kind = {}
            for o in prof["ops"]:
                by_kind[o["kind"]] = by_kind.get(o["kind"], 0.0) + o["us"]
            r = {"model": name, "precision": precision, "batch": prof["batch"], "total_us": round(prof["total_us"], 1),
                 "us_by_kind": {k: round(v, 1) for k, v in sorted(by_kind.items(), key=lambda kv: -kv[1])},
                 "grn_share": round(by_kind.get("grn", 0.0) / prof["total_us"], 4),
                 "grn_ops": [[o["name"], o["C"], o["rows"], round(o["us"], 1)] for o in prof["ops"] if o["kind"] == "grn"]}
            if name != "atto":  # the forward as a caller sees it (host wall around Engine.run, which ends in a synchronise)
                b8 = min(8, B)
                x8 = x[:b8].copy()
                for _ in range(3):
                    eng.run(x8)
                ts = []
                for _ in range(9):
                    t0 = time.perf_counter()
                    eng.run(x8)
                    ts.append((time.perf_counter() - t0) * 1e6)
                r["run_b8_us"] = [round(statistics.median(ts), 1), round(min(ts), 1), round(max(ts), 1)]
                r["engine"] = eng.refresh_info()["name"]
            rows.append(r)
            print(json.dumps(r), flush=True)
        finally:
            eng.close()
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--md", default="")
    ap.add_argument("--json", default="")
    ap.add_argument("--forms", action="store_true")
    ap.add_argument("--models", action="store_true")
    ap.add_argument("--quick", action="store_true", help="one small map and the tiny model: a rehearsal of the script")
    a = ap.parse_args()
    sys.path.insert(0, HERE)
    import tempfile

    import torch

    import die_amd  # noqa: F401
    from die_amd import native
    from die_amd.models import convnextv2 as v2
    from die_amd.ops import kernels as K

    if not torch.cuda.is_available():
        sys.exit("grn_bench needs a GPU: device times are not measured anywhere else")
    maps, batches = (MAPS[3:4], (1, 8)) if a.quick else (MAPS, BATCHES)
    rows = kernel_rows(torch, native, K, maps, batches)

    def cell(t):
        return "-" if t is None else "%.1f [%.1f, %.1f]" % tuple(t)

    lines = ["| format | model | map x C | B | MB moved | grn us [min, max] | TB/s | HBM-rate us | group_norm G=1 us | torch eager us | torch / grn |",
             "|---|---|---|---:|---:|---:|---:|---:|---:|---:|---:|"]
    for r in rows:
        lines.append("| %s | %s | %dx%dx%d | %d | %.2f | %s | %.2f | %.2f | %s | %s | %.1f |" % (
            r["precision"], r["model"], r["hw"], r["hw"], r["C"], r["B"], r["mbytes"], cell(r["grn_us"]), r["tbytes_per_s"],
            r["hbm_us"], cell(r["group_norm_us"]), cell(r["torch_us"]), r["torch_over_grn"]))
    forms = form_rows(torch, native, K, batches) if a.forms else []
    if forms:
        lines += ["", "| format | map x C | chunks per sample | B | one launch us [min, max] | three launches us [min, max] | three / one |",
                  "|---|---|---:|---:|---:|---:|---:|"]
        for r in forms:
            lines.append("| %s | %dx%dx%d | %d | %d | %s | %s | %.2f |" % (
                r["precision"], r["H"], r["W"], r["C"], r["chunks"], r["B"], cell(r["one_launch_us"]),
                cell(r["three_launches_us"]), r["three_over_one"]))
    models = []
    if a.models:
        with tempfile.TemporaryDirectory() as tmp:
            models = model_rows(torch, native, v2, tmp, a.quick)
        for r in models:
            lines += ["", "%s, B = %d, %s: %.1f us over all ops, grn %.1f %% of it; by kind %s%s" % (
                r["model"], r["batch"], r["precision"], r["total_us"], 100 * r["grn_share"], json.dumps(r["us_by_kind"]),
                "; Engine.run at B = 8: %.1f us [%.1f, %.1f] (%s)" % (tuple(r["run_b8_us"]) + (r["engine"],)) if "run_b8_us" in r else "")]
    text = "\n".join(lines) + "\n"
    print(text)
    if a.md:
        open(a.md, "w").write(text)
    if a.json:
        json.dump({"kernels": rows, "forms": forms, "models": models}, open(a.json, "w"), indent=1)


if __name__ == "__main__":
    main()
