#!/usr/bin/env python3
"""Squeeze-excitation on the device: the `se` op (kernels/se.hip, one kern::se_block call) against the unfused
chain the planner emits with EngineOptions::fuse_se = false (gap, two convs at M = batch rows, unary / binary
ops), on every SE block of EfficientNet-B0 and MobileNetV3-Large (models/mbconv_se.py) at 224 x 224, in both
precisions, at batch 8 and 32.  Both engines of a (model, precision) live in one process and are profiled in
turn (Engine.profile: per-op device time, ops launched eagerly and timed one after another with an event each,
so every op carries its launch and event overhead), REPEATS alternating runs each; a row gives the median and
the [min, max] of the runs.  Per block: the time of the se op against the sum of the ops of the same block's
chain; per model: the sum of all ops with the option on and off, and the forward as the serving path runs it
(Engine.run: a hipGraph replay, wall time per call over 50 back-to-back calls, copies included).  A block whose class the
planner's mark rule leaves unfused (plan_lower_se.cpp se_class_on) shows the chain in both columns.

  python tools/se_bench.py [--md out.md] [--json out.json] [--quick]
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BATCHES = (8, 32)
REPEATS = 5


def block_of(name):
    """'block3.se_pool' -> 'block3' for the ops of an SE chain, None for every other op"""
    head, _, tail = name.partition(".")
    return head if tail.startswith("se") else None


def spread(v):
    return [round(statistics.median(v), 1), round(min(v), 1), round(max(v), 1)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--md")
    ap.add_argument("--json")
    ap.add_argument("--quick", action="store_true", help="one precision, one batch, two repeats")
    a = ap.parse_args()
    sys.path.insert(0, HERE)
    import die_amd  # noqa: F401
    from die_amd import native
    from die_amd.models import mbconv_se as ms

    rows, totals = [], []
    for arch in ("efficientnet_b0", "mobilenet_v3_large"):
        cfg = ms.MbconvSeConfig(arch)
        shapes = ms.se_shapes(cfg)
        with tempfile.TemporaryDirectory() as d:
            path = os.path.join(d, arch + ".onnx")
            open(path, "wb").write(ms.build_onnx(cfg)[0])
            for precision in (("fp32",) if a.quick else ("fp32", "bf16")):
                eng = {on: native.Engine(path, device="hip", max_batch=32, precision=precision, fuse_se=on) for on in (True, False)}
                for B in (BATCHES[:1] if a.quick else BATCHES):
                    per = {True: {}, False: {}}   # fuse_se -> block -> [us per run]
                    tot = {True: [], False: []}
                    for _ in range(2 if a.quick else REPEATS):
                        for on, e in eng.items():
                            p = e.profile(B, iters=10)
                            tot[on].append(p["total_us"])
                            run = {}
                            for o in p["ops"]:
                                if block_of(o["name"]):
                                    run[block_of(o["name"])] = run.get(block_of(o["name"]), 0.0) + o["us"]
                            for blk, us in run.items():
                                per[on].setdefault(blk, []).append(us)
                    blocks = sorted(per[True], key=lambda s: int(s[5:]))
                    assert blocks == sorted(per[False], key=lambda s: int(s[5:])) and len(blocks) == len(shapes)
                    for blk, (side, C, Cr) in zip(blocks, shapes):
                        f, u = spread(per[True][blk]), spread(per[False][blk])
                        rows.append({"model": arch, "precision": precision, "B": B, "block": blk, "map": side, "C": C, "Cr": Cr,
                                     "se_us": f, "unfused_us": u, "unfused_over_se": round(u[0] / f[0], 2)})
                    # the same forward as the serving path runs it: Engine.run (hipGraph replay of bucket B), wall time
                    # of 50 back-to-back calls per run, input and output copies included on both sides
                    x = ms.synthetic_input(B, cfg).reshape(B, -1)
                    wall = {True: [], False: []}
                    for _ in range(2 if a.quick else REPEATS):
                        for on, e in eng.items():
                            e.run(x)
                            t0 = time.perf_counter()
                            for _ in range(50):
                                e.run(x)
                            wall[on].append((time.perf_counter() - t0) / 50 * 1e6)
                    f, u = spread(tot[True]), spread(tot[False])
                    gf, gu = spread(wall[True]), spread(wall[False])
                    totals.append({"model": arch, "precision": precision, "B": B, "fuse_se_us": f, "no_fuse_se_us": u,
                                   "off_over_on": round(u[0] / f[0], 3), "graph_fuse_se_us": gf, "graph_no_fuse_se_us": gu,
                                   "graph_off_over_on": round(gu[0] / gf[0], 3)})
                    print(totals[-1], flush=True)
                for e in eng.values():
                    e.close()
    lines = ["| model | precision | B | block | map | C | Cr | se us [min, max] | unfused us [min, max] | unfused / se |", "|---|---|---:|---|---:|---:|---:|---:|---:|---:|"]
    for r in rows:
        lines.append("| %s | %s | %d | %s | %dx%d | %d | %d | %.1f [%.1f, %.1f] | %.1f [%.1f, %.1f] | %.2f |" % (
            r["model"], r["precision"], r["B"], r["block"], r["map"], r["map"], r["C"], r["Cr"], *r["se_us"], *r["unfused_us"], r["unfused_over_se"]))
    lines += ["", "| model | precision | B | sum of the ops, fuse_se on us [min, max] | off us [min, max] | off / on | graph replay (Engine.run), on us [min, max] | off us [min, max] | off / on |",
              "|---|---|---:|---:|---:|---:|---:|---:|---:|"]
    for r in totals:
        lines.append("| %s | %s | %d | %.1f [%.1f, %.1f] | %.1f [%.1f, %.1f] | %.3f | %.1f [%.1f, %.1f] | %.1f [%.1f, %.1f] | %.3f |" % (
            r["model"], r["precision"], r["B"], *r["fuse_se_us"], *r["no_fuse_se_us"], r["off_over_on"], *r["graph_fuse_se_us"],
            *r["graph_no_fuse_se_us"], r["graph_off_over_on"]))
    text = "\n".join(lines) + "\n"
    print(text)
    if a.md:
        open(a.md, "w").write(text)
    if a.json:
        with open(a.json, "w") as f:  # one row per line
            f.write("{\n" + ",\n".join('"%s": [\n%s\n]' % (k, ",\n".join(json.dumps(r) for r in v))
                                       for k, v in (("blocks", rows), ("forward", totals))) + "\n}\n")


if __name__ == "__main__":
    main()
