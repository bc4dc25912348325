// Squeeze-excitation blocks and the trailing activations of the MBConv families.
//
// trailing_act: "the activation behind a value" for the producers that take it into their epilogue (the
// project conv, the grouped / depthwise kernels, GroupNorm):
//  * SiLU written Mul(v, Sigmoid(v)) in either operand order, where v is read by exactly those two nodes
//    and the Sigmoid by the Mul alone (code 4);
//  * the HardSwish node, or HardSigmoid(alpha = 1/6, beta = 0.5)(v) + Mul(v, .) with the same reader rule
//    (code 5).
// It only looks; the caller marks `used` done when it takes the activation.
//
// lower_se: one SE op (kern::se_block, kernels/se.hip) for the torchvision / timm chain
//   s = GlobalAveragePool(x)   or   ReduceMean(x, axes [2, 3], keepdims 1)
//   g = Sigmoid | HardSigmoid (Conv1x1(act1(Conv1x1(s))))        act1 = Relu | SiLU | HardSwish
//   y = Mul(x, g)                                                 in either operand order
// on a dense NHWC image x with a multiple of 8 channels and no stored pad channels.  Both convs have
// [Cr, C, 1, 1] / [C, Cr, 1, 1] initializers, group 1, stride 1, no pads, an optional bias; every inner
// tensor has one reader and is not a graph output; x is read by the pool and the final Mul alone.  The
// second FC is transposed here so that consecutive lanes of the kernel read consecutive channels.  The f32
// gate and the slices' partial sums live in a plan buffer of the arena (out2); the per-sample counters are
// the engine's zeroed split-K counters.
// A chain that does not match is not an error: lower_se returns false with nothing marked, and the pool,
// the convs and the elementwise nodes lower as before (PlanOptions::fuse_se = false: always).  The
// Flatten -> Gemm -> ... -> Reshape form of SE is not matched.
#include "planner.h"

namespace die {

namespace {
// The mark rule: the classes of SE blocks, by the FC weights C * Cr and the precision, in which the se op beat
// the unfused chain by more than the spread on every block of EfficientNet-B0 and MobileNetV3-Large at batch
// 8 and 32 (profiles/se_mbconv.md).  One block per sample runs both FCs, so past ~10k weights the serial FC
// phase costs more than the launches it saves (672 x 28: 0.85x - 1.06x, 960 x 240: 0.13x); in bf16 storage
// the unfused chain is cheaper and the crossover comes earlier (120 x 32: 0.98x - 1.12x).  A class that is off
// keeps the pool + conv + elementwise lowering and stays reachable through kern::se_block itself.
bool se_class_on(int C, int Cr, bool split) { return static_cast<long long>(C) * Cr <= (split ? 9600 : 2400); }
}  // namespace

int Planner::trailing_act(const std::string& cur, std::vector<int>& used, std::string& out) const {
  if (graph_outputs_.count(cur)) return 0;
  const std::vector<int> cs = consumers(cur);
  if (cs.size() == 1 && !done_[cs[0]] && m_.nodes[cs[0]].op_type == "HardSwish") {
    used = {cs[0]};
    out = m_.nodes[cs[0]].outputs[0];
    return 5;
  }
  if (cs.size() != 2) return 0;
  int sg = -1, mu = -1;
  for (int c : cs) {
    if (done_[c]) return 0;
    const std::string& t = m_.nodes[c].op_type;
    if (t == "Sigmoid" || t == "HardSigmoid") sg = c;
    else if (t == "Mul") mu = c;
  }
  if (sg < 0 || mu < 0) return 0;
  const Node& s = m_.nodes[sg];
  const Node& m = m_.nodes[mu];
  if (next_op(s.outputs[0], "Mul") != mu || m.inputs.size() != 2 || m.in(0) == m.in(1) || other_input(m, cur) != s.outputs[0]) return 0;
  int act = 4;
  if (s.op_type == "HardSigmoid") {
    if (std::fabs(s.get_float("alpha", 0.2f) - 1.f / 6.f) > 1e-6f || s.get_float("beta", 0.5f) != 0.5f) return 0;
    act = 5;
  }
  used = {sg, mu};
  out = m.outputs[0];
  return act;
}

bool Planner::lower_se(int idx) {
  if (!opt_.fuse_se) return false;
  const Node& n = m_.nodes[idx];
  const std::string& xname = n.in(0);
  auto xi = vid_.find(xname);
  if (xi == vid_.end()) return false;
  const Val x = vals_[xi->second];
  if (x.kind != Val::NHWC || !dense(x) || x.padded() || x.C % 8 || x.C < 8 || x.C > 4096 || x.has_affine) return false;
  if (n.op_type == "ReduceMean") {
    std::vector<int64_t> ax;
    if (!node_axes(n, ax) || n.get_int("keepdims", 1) != 1) return false;
    std::sort(ax.begin(), ax.end());
    if (ax != std::vector<int64_t>{2, 3} && ax != std::vector<int64_t>{-2, -1}) return false;
  }
  const int C = x.C;
  // a 1x1 conv of the pooled vector: weights [N, K, 1, 1], plain geometry, optional bias
  auto fc = [&](int c, int N, int K) {
    if (c < 0) return false;
    const Node& q = m_.nodes[c];
    if (q.op_type != "Conv" || !is_init(q.in(1)) || q.get_int("group", 1) != 1) return false;
    const onnx::Tensor& w = m_.initializers.at(q.in(1));
    if (w.dims != std::vector<int64_t>{N, K, 1, 1} || w.f.size() != static_cast<size_t>(N) * K) return false;
    if (q.get_ints("strides", {1, 1}) != std::vector<int64_t>{1, 1} || q.get_ints("dilations", {1, 1}) != std::vector<int64_t>{1, 1} ||
        q.get_ints("pads", {0, 0, 0, 0}) != std::vector<int64_t>{0, 0, 0, 0})
      return false;
    const std::string ap = q.get_string("auto_pad", "NOTSET");
    if (ap != "NOTSET" && ap != "VALID") return false;
    if (q.in(2).empty()) return true;
    return is_init(q.in(2)) && m_.initializers.at(q.in(2)).f.size() == static_cast<size_t>(N);
  };
  const int c1 = sole_consumer(n.outputs[0]);
  if (c1 < 0 || m_.nodes[c1].op_type != "Conv" || !is_init(m_.nodes[c1].in(1))) return false;
  const onnx::Tensor& wt1 = m_.initializers.at(m_.nodes[c1].in(1));
  if (wt1.dims.size() != 4 || wt1.dims[0] < 1 || wt1.dims[0] > 1024) return false;
  const int Cr = static_cast<int>(wt1.dims[0]);
  if (!fc(c1, Cr, C) || !se_class_on(C, Cr, opt_.split)) return false;
  std::vector<int> used = {c1}, act_nodes;
  std::string cur = m_.nodes[c1].outputs[0];
  int act1 = 0;
  if (const int r = next_op(cur, "Relu"); r >= 0) {
    act1 = 1;
    act_nodes = {r};
    cur = m_.nodes[r].outputs[0];
  } else {
    std::string out;
    act1 = trailing_act(cur, act_nodes, out);
    cur = out;
  }
  if (!act1) return false;
  used.insert(used.end(), act_nodes.begin(), act_nodes.end());
  const int c2 = sole_consumer(cur);
  if (!fc(c2, C, Cr)) return false;
  used.push_back(c2);
  const int gi = sole_consumer(m_.nodes[c2].outputs[0]);
  if (gi < 0) return false;
  const Node& gn = m_.nodes[gi];
  int act2 = 0;
  float alpha = 0.f, beta = 0.f;
  if (gn.op_type == "HardSigmoid") {
    act2 = 1;
    alpha = gn.get_float("alpha", 0.2f);
    beta = gn.get_float("beta", 0.5f);
  } else if (gn.op_type != "Sigmoid") {
    return false;
  }
  used.push_back(gi);
  const int mi = next_op(gn.outputs[0], "Mul");
  if (mi < 0) return false;
  const Node& mul = m_.nodes[mi];
  if (mul.inputs.size() != 2 || mul.in(0) == mul.in(1) || other_input(mul, gn.outputs[0]) != xname) return false;
  const std::vector<int> xr = consumers(xname);  // the pool and the final Mul, nobody else
  if (xr.size() != 2 || std::find(xr.begin(), xr.end(), mi) == xr.end()) return false;
  used.push_back(mi);

  for (int u : used) done_[u] = true;
  const onnx::Tensor& wt2 = m_.initializers.at(m_.nodes[c2].in(1));
  std::vector<float> w2t(static_cast<size_t>(Cr) * C);
  for (int c = 0; c < C; ++c)
    for (int r = 0; r < Cr; ++r) w2t[static_cast<size_t>(r) * C + c] = wt2.f[static_cast<size_t>(c) * Cr + r];
  PlanOp p;
  p.kind = PlanOp::SE;
  p.name = n.name;
  p.in = x.buf;
  p.w_off = push_f32(wt1.f);
  if (!m_.nodes[c1].in(2).empty()) p.bias_off = push_f32(m_.initializers.at(m_.nodes[c1].in(2)).f);
  p.w2_off = push_f32(w2t);
  if (!m_.nodes[c2].in(2).empty()) p.bias2_off = push_f32(m_.initializers.at(m_.nodes[c2].in(2)).f);
  p.act = act1;
  p.gidx = act2;
  p.clip_lo = alpha;
  p.clip_hi = beta;
  p.C = C;
  p.Cp = Cr;
  p.H = x.H;
  p.W = x.W;
  p.flops_per_sample = 2.0 * x.H * x.W * C + 4.0 * C * Cr;
  p.out = buf_like(x);
  const size_t ws = static_cast<size_t>(1 + kern::se_slices(1, x.H * x.W)) * C * sizeof(float);
  p.out2 = new_buf(ws);
  plan_.bufs[p.out2].bytes_per_sample = ws;  // fp32 in both precisions
  same_shape(mul.outputs[0], x, p.out, /*clear_affine=*/true);
  add_op(std::move(p));
  return true;
}

}  // namespace die
