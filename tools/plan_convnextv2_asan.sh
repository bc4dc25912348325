#!/bin/bash
# The GRN lowering of the planner under AddressSanitizer + UBSan, as a stand-alone host program
# (make plan-asan; no GPU, nothing loaded into python): the two tiny ConvNeXt-V2 models of
# models/convnextv2.py (timm and HF export forms) must lower, with grn ops, in both precisions.
set -euo pipefail
R=$(cd "$(dirname "$0")/.." && pwd)
cd "$R"
make plan-asan > /dev/null
T=$(mktemp -d)
trap 'rm -rf "$T"' EXIT
python3 - "$T" <<'PY'
import sys
sys.path.insert(0, ".")
import die_amd  # noqa: F401
from die_amd.models import convnextv2 as v2
for spec, kw in v2.SPECS.items():
    open("%s/v2_%s.onnx" % (sys.argv[1], spec), "wb").write(v2.build_onnx(v2.tiny_convnextv2_config(**kw))[0])
PY
distributed-inference-engine-cpp_amd/bin/die_plan_asan --supported "$T"/v2_timm.onnx "$T"/v2_hf.onnx
