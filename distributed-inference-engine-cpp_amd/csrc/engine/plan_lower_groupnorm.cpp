// GroupNorm / InstanceNorm of a dense NHWC image, all one GROUPNORM op (kern::group_norm):
//  * InstanceNormalization(x [N, C, H, W], scale [C], B [C]): a group per channel, G = C;
//  * GroupNormalization(x, scale, bias, num_groups), parameters per group [G] (opset 18) or per channel
//    [C] (opset 21), told apart by their length and expanded to per channel here;
//  * torch's export of GroupNorm below opset 18:
//      Reshape(x, [0 / N, G, -1]) -> InstanceNormalization(scale [G], B [G]) -> Reshape(., x's shape)
//      [-> Mul(w [C, 1, 1])] [-> Add(b [C, 1, 1])]
//    with the back-shape a constant or folded from Shape nodes.  The walk is one pass with lookahead,
//    so the chain is anchored at its first Reshape (groupnorm_anchor).  The inner node's per-group
//    scale s and bias t (torch writes ones and zeros) fold into the per-channel pair:
//    gamma[c] = s[g] w[c], beta[c] = t[g] w[c] + b[c].
//  * a trailing activation whose input has no other reader becomes the op's act: Relu (1), or SiLU (2)
//    written Mul(y, Sigmoid(y)) in either operand order.  A trailing Add of a residual image is not
//    fused: it stays the binary kernel.
// Rejected with a report line (the hybrid engine then takes the nodes): channels not divisible by the
// groups, a chain whose inner tensors have another reader, a back-Reshape to anything but x's shape,
// scale / bias that are not initializers, an input that is not a dense image (rows, an [N, H, W, C]
// view), InstanceNormalization of rank-3 rows outside the chain, more than 2048 stored channels.
#include "planner.h"

namespace die {

namespace {
// w / b of the chain's trailing Mul / Add: one value per channel, shaped [C, 1, 1] or [1, C, 1, 1]
bool per_channel_init(const onnx::Tensor& t, int C) {
  const auto& d = t.dims;
  if (static_cast<int>(t.f.size()) != C || (d.size() != 3 && d.size() != 4)) return false;
  return d[d.size() - 3] == C && d[d.size() - 2] == 1 && d[d.size() - 1] == 1;
}
}  // namespace

// A Reshape of an image (or of an [N, H, W, C] view of one, for the report line) that an
// InstanceNormalization reads: the head of torch's GroupNorm export, or an error.
bool Planner::groupnorm_anchor(const Node& n) const {
  auto xi = vid_.find(n.in(0));
  if (xi == vid_.end() || n.outputs.empty()) return false;
  const Val& x = vals_[xi->second];
  if (!(x.kind == Val::NHWC || x.kind == Val::GRAPH_IN || (x.kind == Val::ROWS_BF16 && x.rank == 4))) return false;
  for (int c : consumers(n.outputs[0]))
    if (m_.nodes[c].op_type == "InstanceNormalization") return true;
  return false;
}

void Planner::lower_groupnorm_chain(int idx) {
  const Node& n = m_.nodes[idx];
  auto fail = [&](const Node& at, const std::string& why) {
    reject(at, "a Reshape read by an InstanceNormalization is only supported as torch's GroupNorm export, Reshape(x, "
               "[N, G, -1]) -> InstanceNormalization -> Reshape(., x's shape) (" + why + ")");
  };
  if (val(n.in(0), n).kind == Val::ROWS_BF16) fail(n, "the input must be a dense image, not an [N, H, W, C] view");
  const Val x = materialize_in(n.in(0), n);
  if (x.kind != Val::NHWC || !dense(x)) fail(n, "the input must be a dense image");
  const int Cl = x.logical();
  std::vector<int64_t> shp;
  if (!ints_of(n.in(1), shp)) fail(n, "the target shape must be static");
  auto is_batch = [](int64_t d) { return d == 0 || d == -1 || d == kBatchDim; };
  const int64_t per_sample = static_cast<int64_t>(Cl) * x.H * x.W;
  if (shp.size() != 3 || !is_batch(shp[0]) || shp[1] < 1) fail(n, "the target shape must be [N, G, -1]");
  const int G = static_cast<int>(shp[1]);
  if (Cl % G) fail(n, std::to_string(Cl) + " channels are not divisible by " + std::to_string(G) + " groups");
  if (shp[2] != -1 && shp[2] != per_sample / G) fail(n, "the target shape must be [N, G, -1]");
  const std::string& grouped = n.outputs[0];
  const int in_idx = next_op(grouped, "InstanceNormalization");
  if (in_idx < 0) fail(n, "the grouped tensor " + grouped + " has another reader");
  const Node& inorm = m_.nodes[in_idx];
  if (inorm.inputs.size() < 3) fail(inorm, "needs scale and B");
  for (int k = 1; k <= 2; ++k)
    if (!is_init(inorm.in(k))) fail(inorm, "scale / B " + inorm.in(k) + " must be an initializer");
  const std::vector<float>& s = m_.initializers.at(inorm.in(1)).f;
  const std::vector<float>& t = m_.initializers.at(inorm.in(2)).f;
  if (static_cast<int>(s.size()) != G || static_cast<int>(t.size()) != G) fail(inorm, "scale / B must hold one value per group");
  const int back_idx = next_op(inorm.outputs[0], "Reshape");
  if (back_idx < 0) fail(inorm, "its output " + inorm.outputs[0] + " must be read by the back-Reshape alone");
  const Node& back = m_.nodes[back_idx];
  std::vector<int64_t> bshp;
  if (!ints_of(back.in(1), bshp)) {
    // torch writes Shape(x) after the InstanceNormalization: the walk has not reached it yet (it stays
    // in the walk, where it lowers to no op)
    auto pi = producer_.find(back.in(1));
    if (pi == producer_.end() || m_.nodes[pi->second].op_type != "Shape" || m_.nodes[pi->second].in(0) != n.in(0))
      fail(back, "the target shape must be static");
    bshp = {kBatchDim, Cl, x.H, x.W};
  }
  // Shape(x) of a padded image reports the stored channels (lower_shape_op)
  if (bshp.size() != 4 || !is_batch(bshp[0]) || (bshp[1] != Cl && bshp[1] != x.C) || bshp[2] != x.H || bshp[3] != x.W)
    fail(back, "it must restore x's shape [N, " + std::to_string(Cl) + ", " + std::to_string(x.H) + ", " +
                   std::to_string(x.W) + "]");
  const int Cg = Cl / G;
  std::vector<float> gamma(Cl), beta(Cl);
  for (int c = 0; c < Cl; ++c) {
    gamma[c] = s[c / Cg];
    beta[c] = t[c / Cg];
  }
  std::vector<int> used = {in_idx, back_idx};
  std::string cur = back.outputs[0];
  int c = next_op(cur, "Mul");
  if (c >= 0 && is_init(other_input(m_.nodes[c], cur)) && per_channel_init(m_.initializers.at(other_input(m_.nodes[c], cur)), Cl)) {
    const std::vector<float>& w = m_.initializers.at(other_input(m_.nodes[c], cur)).f;
    for (int k = 0; k < Cl; ++k) {
      gamma[k] *= w[k];
      beta[k] *= w[k];
    }
    used.push_back(c);
    cur = m_.nodes[c].outputs[0];
  }
  c = next_op(cur, "Add");
  if (c >= 0 && is_init(other_input(m_.nodes[c], cur)) && per_channel_init(m_.initializers.at(other_input(m_.nodes[c], cur)), Cl)) {
    const std::vector<float>& b = m_.initializers.at(other_input(m_.nodes[c], cur)).f;
    for (int k = 0; k < Cl; ++k) beta[k] += b[k];
    used.push_back(c);
    cur = m_.nodes[c].outputs[0];
  }
  for (int u : used) done_[u] = true;
  emit_groupnorm(inorm, inorm.name + "+groupnorm_export", x, G, std::move(gamma), std::move(beta),
                 inorm.get_float("epsilon", 1e-5f), cur);
}

// The single nodes InstanceNormalization (G = C) and GroupNormalization
void Planner::lower_groupnorm(int idx) {
  const Node& n = m_.nodes[idx];
  const bool inorm = n.op_type == "InstanceNormalization";
  {
    const Val& v = val(n.in(0), n);
    if (v.kind == Val::ROWS_BF16 && v.rank == 3 && inorm)
      reject(n, "InstanceNormalization of rank-3 rows is only supported inside torch's GroupNorm export (Reshape(image, "
                "[N, G, -1]) -> InstanceNormalization -> Reshape back)");
    if (v.kind != Val::NHWC && v.kind != Val::GRAPH_IN) reject(n, "the input must be a dense image [N, C, H, W]");
  }
  const Val x = materialize_in(n.in(0), n);
  if (x.kind != Val::NHWC || !dense(x)) reject(n, "the input must be a dense image [N, C, H, W]");
  const int Cl = x.logical();
  const int64_t groups = inorm ? Cl : n.get_int("num_groups", 0);
  if (groups < 1) reject(n, "needs num_groups >= 1");
  if (Cl % groups) reject(n, std::to_string(Cl) + " channels are not divisible by " + std::to_string(groups) + " groups");
  const int G = static_cast<int>(groups), Cg = Cl / G;
  if (n.inputs.size() < 3) reject(n, "needs scale and bias");
  const std::vector<float>& s = init(n.in(1), n).f;
  const std::vector<float>& t = init(n.in(2), n).f;
  auto fits = [&](const std::vector<float>& p) {
    return static_cast<int>(p.size()) == Cl || (!inorm && static_cast<int>(p.size()) == G);
  };
  if (!fits(s) || !fits(t)) reject(n, "scale / bias must hold one value per channel" + std::string(inorm ? "" : " or per group"));
  std::vector<float> gamma(Cl), beta(Cl);
  for (int c = 0; c < Cl; ++c) {
    gamma[c] = s[static_cast<int>(s.size()) == Cl ? c : c / Cg];
    beta[c] = t[static_cast<int>(t.size()) == Cl ? c : c / Cg];
  }
  emit_groupnorm(n, n.name, x, G, std::move(gamma), std::move(beta), n.get_float("epsilon", 1e-5f), n.outputs[0]);
}

// The one GROUPNORM op of the lowerings above on the dense image x: gamma / beta [Cl] go into the
// parameter blob, a trailing Relu / SiLU of `cur` is taken as the op's act, the workspace of the
// launch is a plan buffer (out2) of the arena.
void Planner::emit_groupnorm(const Node& n, const std::string& name, const Val& x, int G, std::vector<float> gamma,
                             std::vector<float> beta, float eps, std::string cur) {
  if (x.C % 8) reject(n, "the image must be stored with a multiple of 8 channels");
  const size_t ws = kern::group_norm_workspace_bytes(1, x.H * x.W, x.C, G);
  if (!ws) reject(n, "more than 2048 stored channels");
  int act = 0;
  if (const int r = next_op(cur, "Relu"); r >= 0) {
    act = 1;
    done_[r] = true;
    cur = m_.nodes[r].outputs[0];
  } else if (!graph_outputs_.count(cur)) {
    // SiLU: cur read by exactly Sigmoid(cur) and Mul(cur, that) / Mul(that, cur), the Sigmoid by the Mul alone
    const std::vector<int> cs = consumers(cur);
    int sg = -1, mu = -1;
    for (int c : cs) {
      if (done_[c]) continue;
      if (m_.nodes[c].op_type == "Sigmoid") sg = c;
      else if (m_.nodes[c].op_type == "Mul") mu = c;
    }
    if (cs.size() == 2 && sg >= 0 && mu >= 0 && next_op(m_.nodes[sg].outputs[0], "Mul") == mu &&
        m_.nodes[mu].inputs.size() == 2 && other_input(m_.nodes[mu], cur) == m_.nodes[sg].outputs[0]) {
      act = 2;
      done_[sg] = done_[mu] = true;
      cur = m_.nodes[mu].outputs[0];
    }
  }
  PlanOp p;
  p.kind = PlanOp::GROUPNORM;
  p.name = name;
  p.in = x.buf;
  p.scale_off = push_f32(gamma);
  p.shift_off = push_f32(beta);
  p.eps = eps;
  p.act = act;
  p.groups = G;
  p.C = x.C;
  p.Cp = x.logical();
  p.H = x.H;
  p.W = x.W;
  p.out = buf_like(x);
  p.out2 = new_buf(ws);
  plan_.bufs[p.out2].bytes_per_sample = ws;  // fp32 partials in both precisions
  same_shape(cur, x, p.out, /*clear_affine=*/true);
  add_op(std::move(p));
}

}  // namespace die
