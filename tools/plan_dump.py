#!/usr/bin/env python3
"""Every plan the repository's generated models lower to, as one text file.

For a planner change that must not change any plan: run this before and after and compare the two
files byte for byte.  A section per (model, precision, option set) holds native.plan_dump's text --
every PlanOp member, every buffer, the plan's scalars and a hash of the parameter blob -- or, for a
model the HIP planner rejects, the support report's text.  Runs on the CPU.

  python tools/plan_dump.py [--out plans.txt] [--tiny-only] [--tree DIR]

--tree DIR imports the package of another checkout of this repository (an earlier commit).
"""
import argparse
import hashlib
import os
import sys
import tempfile

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# option sets: name -> plan_dump keyword arguments
OPTION_SETS = (("defaults", {}),
               ("side_branches", {"side_branches": True}),
               ("fuse_gap_fc", {"fuse_gap_fc": True}),
               ("no_fold_layernorm", {"fold_layernorm": False}),
               ("no_ln_stats_epilogue", {"ln_stats_epilogue": False}),
               ("no_fuse_pairs_stem_pool", {"fuse_pairs": False, "fuse_stem_pool": False}))


def models(tiny_only=False):
    """(name, onnx bytes) of every model the repository can generate."""
    from die_amd.models import convnext, fuzz, generic, mobilenet, resnet_v2, vit

    for name in generic.BUILDERS:
        yield name, generic.build_onnx(name)
    yield "resnet_v2_tiny", resnet_v2.build_onnx(resnet_v2.tiny_config())[0]
    yield "vit_tiny", vit.build_onnx(vit.tiny_vit_config())[0]
    yield "mobilenet_tiny", mobilenet.build_onnx(mobilenet.tiny_mobilenet_config())[0]
    yield "convnext_tiny", convnext.build_onnx(convnext.tiny_convnext_config())[0]
    for seed in range(20):
        yield "fuzz_%d" % seed, fuzz.build_random(seed)[0]
        yield "fuzz_rows_%d" % seed, fuzz.build_random_rows(seed)[0]
    if not tiny_only:
        yield "resnet50_v2", resnet_v2.build_onnx(resnet_v2.ResNetConfig())[0]
        yield "vit_b16", vit.build_onnx(vit.ViTConfig())[0]
        yield "convnext_t", convnext.build_onnx(convnext.ConvNeXtConfig())[0]


def dump_all(native, tiny_only=False):
    """-> (text, plans, reports): the sections, and how many hold a plan / a support report."""
    parts, plans, reports = [], 0, 0
    with tempfile.TemporaryDirectory() as d:
        for name, blob in models(tiny_only):
            path = os.path.join(d, name + ".onnx")
            with open(path, "wb") as f:
                f.write(blob)
            for precision in ("bf16", "fp32"):
                for oname, kw in OPTION_SETS:
                    parts.append("== %s %s %s\n" % (name, precision, oname))
                    try:
                        parts.append(native.plan_dump(path, precision=precision, **kw))
                        plans += 1
                    except RuntimeError:
                        parts.append("unsupported\n" + native.plan_report(path, precision=precision)["text"] + "\n")
                        reports += 1
            os.remove(path)
    return "".join(parts), plans, reports


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default="plans.txt")
    ap.add_argument("--tiny-only", action="store_true", help="leave out ResNet50-v2, ViT-B/16 and ConvNeXt-T")
    ap.add_argument("--tree", default=HERE, help="the checkout whose package to import")
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.tree))
    import die_amd  # noqa: F401
    from die_amd import native

    text, plans, reports = dump_all(native, args.tiny_only)
    with open(args.out, "w") as f:
        f.write(text)
    print("%s: %d plans, %d support reports, sha1 %s" % (args.out, plans, reports,
                                                           hashlib.sha1(text.encode()).hexdigest()))


if __name__ == "__main__":
    main()
