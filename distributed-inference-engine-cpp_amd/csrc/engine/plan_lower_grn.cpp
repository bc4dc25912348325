// ConvNeXt-V2's Global Response Normalization, one GRN op (kern::grn) for the exported chain
//   G  = ReduceL2(x, the two spatial axes, keepdims 1)
//   nx = Div(G, Add(ReduceMean(G, the channel axis, keepdims 1), eps))
//   y  = Add(Add(Mul(weight, Mul(x, nx)), bias), x)
// on a map whose buffer is [H * W][C] per sample:
//  * channels-last (timm GlobalResponseNorm(channels_last=True), HF ConvNextV2GRN) on the [N, H, W, C] rows
//    view of an image: axes [1, 2], the mean over axis -1 / 3, parameters shaped [C] or [1, 1, 1, C];
//  * channels-first (timm channels_last=False) on a dense NHWC image value, logically [N, C, H, W]: axes
//    [2, 3], the mean over axis 1, parameters shaped [1, C, 1, 1] or [C, 1, 1].  The same buffer layout,
//    the same op.
// The axes are an attribute or an input; every commutative node is taken in either operand order, so both
// HF's Add(., bias) -> Add(., x) and timm's Add(bias, .) -> Add(x, .) match; weight and / or bias may be
// absent (gamma = 1 / beta = 0).  The walk is one pass with lookahead, so the chain is anchored at the
// ReduceL2 -- the first of x's three readers the walk reaches, the other two depend on it
// (lower_l2norm hands over a ReduceL2 of two axes over such a value).  The result is the same kind of value
// as x (the rows view keeps img_h / img_w, so pwconv2's Transpose -> Add(shortcut) epilogue matches as
// before) in a new buffer; the launch's workspace is a plan buffer (out2) of the arena.
// Rejected with a report line naming the node (the hybrid engine then takes the nodes): reduce axes other
// than the two spatial ones or keepdims 0, a mean over anything but the channel axis, an eps that is not a
// scalar constant, parameters that are not initializers with one value per channel, an inner tensor of the
// chain with another reader (or that is a graph output), trailing Adds that do not add back the very x
// the ReduceL2 read, an input with stored pad channels or one that is not dense.
// Out of scope: the decomposed norm (Mul(x, x) / Pow -> ReduceSum -> Sqrt), the sum of squares from
// pwconv1's epilogue, the scale folded into pwconv2's operand load.
#include "planner.h"

namespace die {

namespace {
// one value per channel, every other dimension 1, the channels at `axis` counted from the END of a
// rank-4 shape (1: [.., C], 3: [.., C, 1, 1]); a rank-1 [C] is taken for the last axis only
bool grn_param(const onnx::Tensor& t, int C, int from_end) {
  const auto& d = t.dims;
  if (static_cast<int>(t.f.size()) != C || d.empty() || d.size() > 4) return false;
  if (static_cast<int>(d.size()) < from_end) return false;
  for (size_t k = 0; k < d.size(); ++k)
    if (d[k] != (k + from_end == d.size() ? C : 1)) return false;
  return true;
}
}  // namespace

bool Planner::grn_anchor(const Node& n) const {
  if (n.op_type != "ReduceL2") return false;
  auto xi = vid_.find(n.in(0));
  if (xi == vid_.end()) return false;
  const Val& x = vals_[xi->second];
  if (!(x.kind == Val::NHWC || (x.kind == Val::ROWS_BF16 && x.rank == 4))) return false;
  std::vector<int64_t> ax;
  return node_axes(n, ax) && ax.size() == 2;
}

void Planner::lower_grn(int idx) {
  const Node& n = m_.nodes[idx];
  const std::string& xname = n.in(0);
  const bool view = val(xname, n).kind == Val::ROWS_BF16;  // channels-last: the [N, H, W, C] rows view
  const Val x = view ? val(xname, n) : materialize_in(xname, n);
  auto fail = [&](const Node& at, const std::string& why) {
    reject(at, "a ReduceL2 over two axes of a map is only supported as ConvNeXt-V2's GRN, ReduceL2(x, spatial axes) -> "
               "ReduceMean(channel axis) -> Add(eps) -> Div -> Mul(x, .) [-> Mul(weight)] [-> Add(bias)] -> Add(x) (" + why + ")");
  };
  const int64_t sp0 = view ? 1 : 2, ch = view ? 3 : 1;
  const int from_end = view ? 1 : 3;  // where a parameter's channels sit, counted from the end of its shape
  auto norm_axis = [](int64_t a) { return a < 0 ? a + 4 : a; };
  std::vector<int64_t> ax;
  node_axes(n, ax);
  for (auto& a : ax) a = norm_axis(a);
  std::sort(ax.begin(), ax.end());
  if (ax.size() != 2 || ax[0] != sp0 || ax[1] != sp0 + 1)
    fail(n, "the norm is taken over the two spatial axes, [" + std::to_string(sp0) + ", " + std::to_string(sp0 + 1) + "] here");
  if (n.get_int("keepdims", 1) != 1) fail(n, "the norm is taken over the two spatial axes with keepdims 1");
  if (!dense(x)) fail(n, "the input must be dense");
  if (x.padded() || x.C % 8) fail(n, "the input must hold a multiple of 8 channels, with no stored pad channels");
  const int C = x.C;

  // G's readers: the ReduceMean and the Div, nobody else
  const std::string& G = n.outputs[0];
  auto another_reader = [&](const Node& at, const std::string& v) {
    fail(at, "the inner tensor " + v + (graph_outputs_.count(v) ? " is a graph output" : " has another reader"));
  };
  if (graph_outputs_.count(G)) another_reader(n, G);
  int mean_idx = -1, div_idx = -1;
  for (int c : consumers(G)) {
    const Node& q = m_.nodes[c];
    if (!done_[c] && q.op_type == "ReduceMean" && mean_idx < 0) mean_idx = c;
    else if (!done_[c] && q.op_type == "Div" && div_idx < 0 && q.in(0) == G) div_idx = c;
    else another_reader(n, G);
  }
  if (mean_idx < 0 || div_idx < 0) fail(n, "the norm " + G + " must be read by ReduceMean(G) and Div(G, .)");
  const Node& mean = m_.nodes[mean_idx];
  std::vector<int64_t> mx;
  if (!node_axes(mean, mx) || mx.size() != 1 || norm_axis(mx[0]) != ch || mean.get_int("keepdims", 1) != 1)
    fail(mean, "the mean is taken over the channel axis, " + std::to_string(ch) + " here, with keepdims 1");
  const int eps_idx = sole_consumer(mean.outputs[0]);
  if (eps_idx < 0) another_reader(mean, mean.outputs[0]);
  const Node& addeps = m_.nodes[eps_idx];
  float eps = 0.f;
  if (addeps.op_type != "Add" || addeps.inputs.size() != 2 || !scalar_init(other_input(addeps, mean.outputs[0]), eps) || !(eps >= 0.f))
    fail(addeps, "the mean's reader must be Add(., eps) with eps a scalar constant >= 0");
  const Node& div = m_.nodes[div_idx];
  if (sole_consumer(addeps.outputs[0]) != div_idx) another_reader(addeps, addeps.outputs[0]);
  if (div.in(1) != addeps.outputs[0]) fail(div, "must be Div(G, mean + eps)");
  const int mul_idx = sole_consumer(div.outputs[0]);
  if (mul_idx < 0) another_reader(div, div.outputs[0]);
  const Node& mulx = m_.nodes[mul_idx];
  if (mulx.op_type != "Mul" || mulx.inputs.size() != 2 || other_input(mulx, div.outputs[0]) != xname)
    fail(mulx, "the normalised norm must be read by Mul(x, .) with the x the ReduceL2 read");
  std::vector<int> used = {mean_idx, eps_idx, div_idx, mul_idx};
  std::string cur = mulx.outputs[0];

  // [Mul(weight)], then the Adds of the bias and of x
  std::vector<float> gamma(C, 1.f), beta;
  int c = sole_consumer(cur);
  if (c < 0) another_reader(mulx, cur);
  if (m_.nodes[c].op_type == "Mul") {
    const Node& q = m_.nodes[c];
    const std::string& w = other_input(q, cur);
    if (q.inputs.size() != 2 || !is_init(w) || !grn_param(m_.initializers.at(w), C, from_end))
      fail(q, "the weight " + w + " must be an initializer with one value per channel");
    gamma = m_.initializers.at(w).f;
    used.push_back(c);
    cur = q.outputs[0];
    c = sole_consumer(cur);
    if (c < 0) another_reader(q, cur);
  }
  bool residual = false;
  for (int k = 0; k < 2 && !residual; ++k) {
    const Node& q = m_.nodes[c];
    const std::string why = "the chain must end in [Add(bias)] and an Add that adds back the x the ReduceL2 read";
    if (q.op_type != "Add" || q.inputs.size() != 2) fail(q, why);
    const std::string& o = other_input(q, cur);
    if (o == xname && q.in(0) != q.in(1)) {
      residual = true;
    } else if (is_init(o) && beta.empty()) {
      if (!grn_param(m_.initializers.at(o), C, from_end)) fail(q, "the bias " + o + " must hold one value per channel");
      beta = m_.initializers.at(o).f;
    } else {
      // an operand that is neither x nor a constant: a computed bias if the next Add adds x back
      const int nx = next_op(q.outputs[0], "Add");
      if (beta.empty() && nx >= 0 && other_input(m_.nodes[nx], q.outputs[0]) == xname)
        fail(q, "the bias " + o + " must be an initializer with one value per channel");
      fail(q, why);
    }
    used.push_back(c);
    cur = q.outputs[0];
    if (!residual) {
      c = sole_consumer(cur);
      if (c < 0) another_reader(q, cur);
    }
  }
  if (!residual) fail(m_.nodes[used.back()], "the chain must end in an Add that adds back the x the ReduceL2 read");

  for (int u : used) done_[u] = true;
  const size_t ws = kern::grn_workspace_bytes(1, x.H * x.W, C);
  PlanOp p;
  p.kind = PlanOp::GRN;
  p.name = n.name;
  p.in = x.buf;
  p.scale_off = push_f32(gamma);
  if (!beta.empty()) p.shift_off = push_f32(beta);
  p.eps = eps;
  p.C = p.Cp = C;
  p.H = x.H;
  p.W = x.W;
  p.flops_per_sample = 4.0 * x.H * x.W * C;
  p.out = buf_like(x);
  p.out2 = new_buf(ws);
  plan_.bufs[p.out2].bytes_per_sample = ws;  // fp32 partial sums in both precisions
  same_shape(cur, x, p.out, /*clear_affine=*/true);
  add_op(std::move(p));
}

}  // namespace die
