// Stand-alone host program for the sanitizers (make plan-asan): the planner alone, no GPU code linked,
// on ONNX files given on the command line (tools/plan_groupnorm_asan.sh writes the four models of
// models/groupnorm.py and the rejected variants, tools/plan_convnextv2_asan.sh the two tiny ConvNeXt-V2 models).  For each file and both precisions: the support
// report, and for a supported graph the plan's ops by kind.  Exits 1 when a file given after --supported
// is not fully lowered or holds neither a groupnorm nor a grn op.
#include <cstdio>
#include <cstring>
#include <map>
#include <string>

#include "../engine/hip_plan.h"
#include "../onnx/onnx_model.h"

using namespace die;

// Stand-ins for the host helpers the planner asks the kernel library (HIP objects, not linked here):
// the heuristic tile, "no" for the optional fusions, and the upper bound of the GroupNorm workspace
// (256 statistics blocks per sample + the merged statistics, float2 per group) and of the GRN one (64
// blocks of partial sums per sample + the coefficients, a float per channel).
namespace die {
namespace kern {
bool attention_supported(int, int, bool) { return true; }
int choose_tile(int, int, int) { return TILE_64x64; }
bool conv_pair_supported(int, int, int) { return false; }
int gap_fc_slice(int, int, int, size_t) { return 0; }
bool stem_pool_supported(int, int, int, int, int, int, int) { return false; }
size_t group_norm_workspace_bytes(int B, int HW, int C, int G) {
  return C % 8 || C > 2048 ? 0 : static_cast<size_t>(B) * 257 * G * 8;
}
size_t grn_workspace_bytes(int B, int HW, int C) { return C % 8 ? 0 : static_cast<size_t>(B) * 65 * C * 4; }
}  // namespace kern
}  // namespace die

int main(int argc, char** argv) {
  bool must_lower = false;
  int bad = 0;
  for (int i = 1; i < argc; ++i) {
    if (!std::strcmp(argv[i], "--supported")) { must_lower = true; continue; }
    if (!std::strcmp(argv[i], "--rejected")) { must_lower = false; continue; }
    const onnx::Model m = onnx::load_onnx(argv[i]);
    for (int split = 0; split < 2; ++split) {
      const PlanReport r = plan_report(m, 8, split != 0);
      std::printf("%s %s: %s, %zu unsupported, %d blocked\n%s", argv[i], split ? "fp32" : "bf16",
                  r.supported ? "supported" : "rejected", r.unsupported.size(), r.blocked, r.text().c_str());
      if (r.supported != must_lower) ++bad;
      if (!r.supported) continue;
      PlanOptions opt;
      opt.split = split != 0;
      const Plan p = build_plan(m, 8, opt);
      std::map<std::string, int> kinds;
      for (const PlanOp& o : p.ops) kinds[plan_kind_name(o.kind)]++;
      std::string line;
      for (const auto& kv : kinds) line += " " + kv.first + "=" + std::to_string(kv.second);
      std::printf("  %s;%s\n", p.summary().c_str(), line.c_str());
      if (must_lower && !kinds.count("groupnorm") && !kinds.count("grn")) ++bad;
    }
  }
  return bad ? 1 : 0;
}
