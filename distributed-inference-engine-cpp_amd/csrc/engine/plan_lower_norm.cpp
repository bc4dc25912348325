// Row normalisations, all one LAYERNORM op:
//  * LayerNormalization over the last axis of rows, and torch's decomposed export of it;
//  * RMSNorm: Pow(x, 2) / Mul(x, x) -> ReduceMean(-1) -> Add(eps) -> Sqrt -> Div(x, .) /
//    Mul(x, Reciprocal(.)) / Mul(x, Div(1, .)) [-> Mul(weight [C])], and the single nodes
//    RMSNormalization / SimplifiedLayerNormalization, are a LAYERNORM op with rms = 1 (never folded
//    into its GEMM readers);
//  * the decomposed LayerNorm over axis 1 of an NCHW image (ConvNeXt) is the op over the image's rows.
#include "planner.h"

namespace die {

// The one LAYERNORM op of the three lowerings below: gamma then beta go into the parameter blob (beta
// also when it is all zeros), Cp = the logical columns (0: not set), the output has x's shape.
void Planner::emit_layernorm(const std::string& name, const Val& x, const std::vector<float>& gamma,
                             const std::vector<float>& beta, float eps, bool rms, int Cp, const std::string& out_name,
                             bool clear_affine) {
  PlanOp p;
  p.kind = PlanOp::LAYERNORM;
  p.name = name;
  p.in = x.buf;
  p.scale_off = push_f32(gamma);
  p.shift_off = push_f32(beta);
  p.eps = eps;
  p.rms = rms ? 1 : 0;
  p.C = x.C;
  p.Cp = Cp;
  p.rows_per_sample = static_cast<long long>(x.H) * x.W;
  p.out = buf_like(x);
  same_shape(out_name, x, p.out, clear_affine);
  add_op(std::move(p));
}

// LayerNormalization, and the single-node RMSNorms RMSNormalization (opset 23) /
// SimplifiedLayerNormalization (ONNX Runtime's optimiser): the same row kernel in its rms mode
void Planner::lower_layernorm(int idx) {
  const Node& n = m_.nodes[idx];
  const bool rms = n.op_type != "LayerNormalization";
  const Val x = val(n.in(0), n);
  if (x.kind != Val::ROWS_BF16 || !dense(x)) reject(n, "input must be dense rows");
  const int64_t axis = n.get_int("axis", -1);
  if (!(axis == -1 || axis == (x.rank ? x.rank : 2) - 1))
    throw std::runtime_error(rms ? n.op_type + " " + n.name + ": axis must be last" : "LayerNormalization: axis must be last");
  if (rms)
    for (size_t k = 1; k < n.outputs.size(); ++k)
      if (!n.outputs[k].empty() && (!consumers(n.outputs[k]).empty() || graph_outputs_.count(n.outputs[k])))
        reject(n, "the inv_std_var output must be unused");
  const int Cl = x.logical();
  std::vector<float> g = init(n.in(1), n).f, b(Cl, 0.f);
  if (!rms && n.inputs.size() > 2 && !n.in(2).empty()) b = init(n.in(2), n).f;
  if (static_cast<int>(g.size()) != Cl || static_cast<int>(b.size()) != Cl) reject(n, "scale/bias size mismatch");
  g.resize(x.C, 0.f);  // stored pad columns: written 0 by the kernel
  b.resize(x.C, 0.f);
  emit_layernorm(n.name, x, g, b, n.get_float("epsilon", 1e-5f), rms, Cl, n.outputs[0]);
}

// ---- RMSNorm as torch exports it ------------------------------------------------------------------
// Pow(x, 2) / Mul(x, x) -> ReduceMean(-1, keepdims) -> Add(eps) -> Sqrt -> Div(x, .) /
// Mul(x, Reciprocal(.)) / Mul(x, Div(1, .)) [-> Mul(weight [C])]  ==> one LAYERNORM op with rms = 1.
// The walk reaches the square first, so the chain is anchored there: a square of rows read only by
// a ReduceMean that is not the token-axis mean (lower_spatial_reduce) is this pattern or an error.
bool Planner::rmsnorm_anchor(const Node& n) const {
  auto xi = vid_.find(n.in(0));
  if (xi == vid_.end() || vals_[xi->second].kind != Val::ROWS_BF16) return false;
  const int rm = next_op(n.outputs[0], "ReduceMean");
  if (rm < 0) return false;
  std::vector<int64_t> ax;
  node_axes(m_.nodes[rm], ax);
  const Val& x = vals_[xi->second];
  return !(x.rank == 3 && (ax == std::vector<int64_t>{1} || ax == std::vector<int64_t>{-2}));
}

void Planner::lower_rmsnorm(int idx) {
  const Node& n = m_.nodes[idx];
  const Val x = val(n.in(0), n);
  const std::string& xn = n.in(0);
  auto fail = [&](const std::string& why) {
    reject(n, "a square under a ReduceMean is only supported as the head of "
           "the decomposed RMSNorm pattern (" + why + ")");
  };
  if (n.op_type == "Pow" && !scalar_is(n.in(1), 2.f)) fail("the exponent must be 2");
  const Node& rm = m_.nodes[sole_consumer(n.outputs[0])];
  bool ok;
  const int64_t axis = last_axis_of(rm, m_, ok);
  if (!ok || !(axis == -1 || axis == (x.rank ? x.rank : 2) - 1))
    fail("ReduceMean " + rm.name + " must reduce over the last axis with keepdims");
  if (!dense(x)) fail("input must be dense rows");
  const int add = next_op(rm.outputs[0], "Add");
  if (add < 0)
    fail("the mean of squares " + rm.outputs[0] + " must be read by the Add of eps alone");
  const std::string& eps_name = other_input(m_.nodes[add], rm.outputs[0]);
  auto ei = m_.initializers.find(eps_name);
  if (ei == m_.initializers.end() || ei->second.f.size() != 1)
    fail("eps of Add " + m_.nodes[add].name + " must be a scalar constant");
  const int sq_rt = next_op(m_.nodes[add].outputs[0], "Sqrt");
  if (sq_rt < 0) fail("no Sqrt of mean + eps");
  const std::string& rt = m_.nodes[sq_rt].outputs[0];
  std::vector<int> used = {sole_consumer(n.outputs[0]), add, sq_rt};
  int c = sole_consumer(rt), norm = -1;
  if (c >= 0 && m_.nodes[c].op_type == "Div" && m_.nodes[c].in(0) == xn && m_.nodes[c].in(1) == rt) {
    norm = c;
  } else if (c >= 0 && (m_.nodes[c].op_type == "Reciprocal" ||
                        (m_.nodes[c].op_type == "Div" && m_.nodes[c].in(1) == rt && scalar_is(m_.nodes[c].in(0), 1.f)))) {
    used.push_back(c);
    const std::string& inv = m_.nodes[c].outputs[0];
    const int mu = next_op(inv, "Mul");
    if (mu >= 0 && other_input(m_.nodes[mu], inv) == xn) norm = mu;
  }
  if (norm < 0) fail("no x / sqrt, x * Reciprocal(sqrt) or x * (1 / sqrt) after Sqrt " + m_.nodes[sq_rt].name);
  used.push_back(norm);
  std::vector<float> g(x.C, 1.f);
  std::string cur = m_.nodes[norm].outputs[0];
  c = next_op(cur, "Mul");
  if (c >= 0 && is_init(other_input(m_.nodes[c], cur)) &&
      static_cast<int>(m_.initializers.at(other_input(m_.nodes[c], cur)).f.size()) == x.logical()) {
    g = m_.initializers.at(other_input(m_.nodes[c], cur)).f;
    used.push_back(c);
    cur = m_.nodes[c].outputs[0];
  }
  if (x.padded()) fail("C % 8 == 0 (stored pad columns)");
  for (int u : used) done_[u] = true;
  emit_layernorm(n.name + "+decomposed_rmsnorm", x, g, std::vector<float>(x.C, 0.f), ei->second.f[0], true, x.C, cur,
                 /*clear_affine=*/true);
}

int64_t Planner::last_axis_of(const Node& n, const onnx::Model& m, bool& ok) {
  std::vector<int64_t> ax = n.get_ints("axes");
  if (ax.empty() && n.inputs.size() > 1 && !n.in(1).empty()) {
    auto it = m.initializers.find(n.in(1));
    if (it != m.initializers.end()) ax = it->second.i;
  }
  ok = ax.size() == 1 && n.get_int("keepdims", 1) == 1;
  return ok ? ax[0] : 0;
}

// torch's LayerNorm export below opset 17: ReduceMean -> Sub -> Pow(2) -> ReduceMean -> Add(eps)
// -> Sqrt -> Div [-> Mul(gamma)] [-> Add(beta)]  ==> one LAYERNORM op.
void Planner::lower_reduce_mean(int idx) {
  const Node& n = m_.nodes[idx];
  if (lower_spatial_reduce(idx, 0)) return;
  const Val x = val(n.in(0), n);
  auto fail = [&](const std::string& why) {
    throw std::runtime_error("ReduceMean " + n.name + ": only the decomposed LayerNormalization pattern is supported (" +
                             why + ")");
  };
  bool ok;
  const int64_t axis = last_axis_of(n, m_, ok);
  const int rank = x.rank ? x.rank : 2;
  // over axis 1 of an NCHW image (channels-first LayerNorm of older ConvNeXt exports): the channel
  // axis is the last one of the stored NHWC pixels, so it is the same op on the image's H * W rows
  const bool image = x.kind == Val::NHWC;
  if (image && !(ok && (axis == 1 || axis == -3))) fail("on an image, reduction over the channel axis with keepdims");
  if (!image && (!ok || !(axis == -1 || axis == rank - 1))) fail("reduction over the last axis with keepdims");
  if (!(x.kind == Val::ROWS_BF16 || image) || x.pitch() != x.C || x.col) fail("input must be dense rows");
  // gamma / beta: [C] on rows, [C, 1, 1] (broadcast over the pixels) on an image
  auto affine_init = [&](const std::string& nm) {
    auto it = m_.initializers.find(nm);
    if (it == m_.initializers.end() || static_cast<int>(it->second.f.size()) != x.C) return false;
    const auto& d = it->second.dims;
    if (!image) return true;
    return (d.size() == 3 || d.size() == 4) && d[d.size() - 3] == x.C;
  };
  const std::string& xn = n.in(0);
  const std::string& mu = n.outputs[0];
  int sub = -1;
  for (int c : consumers(mu))
    if (m_.nodes[c].op_type == "Sub" && m_.nodes[c].in(0) == xn && m_.nodes[c].in(1) == mu) sub = c;
  if (sub < 0) fail("no x - mean");
  const std::string& d = m_.nodes[sub].outputs[0];
  int sq = -1, div = -1;
  for (int c : consumers(d)) {
    const Node& q = m_.nodes[c];
    if ((q.op_type == "Pow" && q.in(0) == d && scalar_is(q.in(1), 2.f)) || (q.op_type == "Mul" && q.in(0) == d && q.in(1) == d))
      sq = c;
    else if (q.op_type == "Div" && q.in(0) == d)
      div = c;
  }
  if (sq < 0 || div < 0) fail("no variance / normalisation");
  const int rm2 = next_op(m_.nodes[sq].outputs[0], "ReduceMean");
  if (rm2 < 0) fail("no variance mean");
  const int add = next_op(m_.nodes[rm2].outputs[0], "Add");
  if (add < 0) fail("no variance + eps");
  const std::string eps_name = other_input(m_.nodes[add], m_.nodes[rm2].outputs[0]);
  auto ei = m_.initializers.find(eps_name);
  if (ei == m_.initializers.end() || ei->second.f.size() != 1) fail("eps must be a scalar constant");
  const int sq_rt = next_op(m_.nodes[add].outputs[0], "Sqrt");
  if (sq_rt < 0 || m_.nodes[div].in(1) != m_.nodes[sq_rt].outputs[0])
    fail("no sqrt feeding the division");
  std::vector<float> g(x.C, 1.f), b(x.C, 0.f);
  std::string cur = m_.nodes[div].outputs[0];
  std::vector<int> used = {sub, sq, rm2, add, sq_rt, div};
  int c = next_op(cur, "Mul");
  if (c >= 0 && affine_init(other_input(m_.nodes[c], cur))) {
    g = m_.initializers.at(other_input(m_.nodes[c], cur)).f;
    used.push_back(c);
    cur = m_.nodes[c].outputs[0];
  }
  c = next_op(cur, "Add");
  if (c >= 0 && affine_init(other_input(m_.nodes[c], cur))) {
    b = m_.initializers.at(other_input(m_.nodes[c], cur)).f;
    used.push_back(c);
    cur = m_.nodes[c].outputs[0];
  }
  if (x.padded()) fail("C % 8 == 0 (stored pad columns)");
  for (int u : used) done_[u] = true;
  emit_layernorm(n.name + "+decomposed_layernorm", x, g, b, ei->second.f[0], false, /*Cp=*/0, cur);
}

}  // namespace die
