#!/bin/bash
# The GroupNorm lowering of the planner under AddressSanitizer + UBSan, as a stand-alone host program
# (make plan-asan; no GPU, nothing loaded into python): the four models of models/groupnorm.py must
# lower, with groupnorm ops, in both precisions.
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
from die_amd.models import groupnorm as M
for name, build in M.BUILDERS.items():
    open("%s/%s.onnx" % (sys.argv[1], name), "wb").write(build(0)[0])
PY
distributed-inference-engine-cpp_amd/bin/die_plan_asan --supported "$T"/gn_resnet.onnx "$T"/gn_resnet_node.onnx \
  "$T"/gn_decoder.onnx "$T"/inorm_net.onnx
