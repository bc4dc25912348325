// The general path (kernels/generic.hip) for what no fused lowering claims: any-activation unary ops,
// comparisons, Where, Cast, broadcast binary ops of two activations, channel Split / Slice / Concat
// as column copies.  An op outside even these is rejected with a clear error (the CPU executor
// still runs such models).
#include "planner.h"

namespace die {

bool Planner::scalar_init(const std::string& name, float& v) const {
  auto it = m_.initializers.find(name);
  if (it == m_.initializers.end() || it->second.numel() != 1) return false;
  v = it->second.f.empty() ? static_cast<float>(it->second.i.at(0)) : it->second.f[0];
  return true;
}

// Comparisons (bool results are stored as 1 / 0 activations): two activations -> a binary op,
// an activation and a scalar constant -> a unary code (the constant on the left mirrors the test).
void Planner::lower_compare(int idx) {
  const Node& n = m_.nodes[idx];
  static const std::map<std::string, int> codes = {
      {"Greater", 18}, {"Less", 19}, {"Equal", 20}, {"GreaterOrEqual", 21}, {"LessOrEqual", 22}};
  float c = 0.f;
  if (scalar_init(n.in(1), c)) return emit_unary(n, materialize_in(n.in(0), n), codes.at(n.op_type), c, 0.f, n.outputs[0]);
  if (scalar_init(n.in(0), c)) {
    int code = codes.at(n.op_type);
    code = code == 18 ? 19 : code == 19 ? 18 : code == 21 ? 22 : code == 22 ? 21 : code;
    return emit_unary(n, materialize_in(n.in(1), n), code, c, 0.f, n.outputs[0]);
  }
  if (lower_binary_acts(n)) return;
  reject(n, "only two activations of one shape or one and a scalar");
}

// Where(cond, a, b): cond an activation; a / b activations of cond's shape or scalar constants.
void Planner::lower_where(int idx) {
  const Node& n = m_.nodes[idx];
  // Where(C, scores, f) / Where(C, f, scores) on attention scores: a constant mask.  The fill f
  // (<= -1e4: GPT-2's -1e4, -1e9, finfo.min, -inf) is treated as -inf -- for scores of ordinary
  // size (|score - row max| far below 1e4) an fp32 softmax gives such positions exactly zero
  // weight either way.  A finite fill above -1e4 is a value, not a mask.
  for (int side = 1; side <= 2 && n.inputs.size() == 3; ++side) {
    auto it = vid_.find(n.in(side));
    if (it == vid_.end() || vals_[it->second].kind != Val::ATTN || vals_[it->second].stage != 0) continue;
    const Val x = vals_[it->second];
    check_score_fill(n, n.in(3 - side));
    return lower_attn_mask(n, x, n.in(0), side == 1 ? 1 : 2);
  }
  const Val c = materialize_in(n.in(0), n);
  if (!dense(c)) throw std::runtime_error("Where " + n.name + ": the condition must be a dense activation");
  PlanOp p;
  p.kind = PlanOp::WHERE;
  p.name = n.name;
  p.in = c.buf;
  float* sv[2] = {&p.clip_lo, &p.clip_hi};
  int* bufs[2] = {&p.in2, &p.in3};
  const Val* like = &c;
  Val vb[2];
  for (int k = 0; k < 2; ++k) {
    if (scalar_init(n.in(1 + k), *sv[k])) continue;
    vb[k] = materialize_in(n.in(1 + k), n);
    if (!dense(vb[k]) || vb[k].kind != c.kind || vb[k].H != c.H || vb[k].W != c.W || vb[k].C != c.C ||
        vb[k].logical() != c.logical())
      throw std::runtime_error("Where " + n.name + ": the branches must be scalars or activations of the condition's shape");
    *bufs[k] = vb[k].buf;
    like = &vb[k];
  }
  p.C = c.C;
  p.Cp = c.logical();
  p.rows_per_sample = rows_of(c);
  p.out = buf_like(c);
  same_shape(n.outputs[0], *like, p.out, /*clear_affine=*/true);
  add_op(std::move(p));
}

// Cast of an activation: to a float type -> the same values; to bool -> v != 0.  Integer targets
// would need rounding the stored representation cannot express exactly: rejected.
void Planner::lower_cast(int idx) {
  const Node& n = m_.nodes[idx];
  const int to = static_cast<int>(n.get_int("to", onnx::FLOAT));
  if (to == onnx::BOOL) return emit_unary(n, materialize_in(n.in(0), n), 24, 0.f, 0.f, n.outputs[0]);
  if (!onnx::is_float_type(to)) throw std::runtime_error("Cast " + n.name + ": only casts to float types or bool");
  define(n.outputs[0], val(n.in(0), n));
}

// Channel range [s0, e0) of a dense image / rows value -> a column copy (s0 % 8 == 0).
void Planner::emit_channel_slice(const Node& n, const Val& x, int64_t s0, int64_t e0, const std::string& out) {
  const int len = static_cast<int>(e0 - s0), Cs = round8(len);
  PlanOp p;
  p.kind = PlanOp::COPY_COLS;
  p.name = n.name;
  p.in = x.buf;
  p.col[0] = static_cast<int>(s0);
  p.ld[0] = x.C;
  p.col[1] = 0;
  p.ld[1] = Cs;
  p.C = std::min(Cs, x.C - static_cast<int>(s0));
  p.rows_per_sample = rows_of(x);
  p.out = new_buf(static_cast<size_t>(rows_of(x)) * Cs * 2);
  Val o = x;
  o.C = Cs;
  o.cl = Cs != len ? len : 0;
  o.buf = p.out;
  define(out, o);
  add_op(std::move(p));
}

// Split along the channel axis (sizes from the attribute, the input, or equal parts): one column
// copy per output; every boundary but the end must be a multiple of 8.
void Planner::lower_split(int idx) {
  const Node& n = m_.nodes[idx];
  const Val x = materialize_in(n.in(0), n);
  const int64_t axis = n.get_int("axis", 0);
  if (!dense(x) || !is_channel_axis(x, axis))
    throw std::runtime_error("Split " + n.name + ": only along the channel axis of an image or rows");
  std::vector<int64_t> sizes = n.get_ints("split");
  if (sizes.empty() && n.inputs.size() >= 2 && !n.in(1).empty()) ints_of(n.in(1), sizes);
  const int64_t Cl = x.logical(), parts = static_cast<int64_t>(n.outputs.size());
  if (sizes.empty()) {
    const int64_t each = (Cl + parts - 1) / parts;  // equal parts (opset 18: the last may be smaller)
    for (int64_t k = 0, s = 0; k < parts; ++k, s += each) sizes.push_back(std::min(each, Cl - s));
  }
  if (static_cast<int64_t>(sizes.size()) != parts) throw std::runtime_error("Split " + n.name + ": sizes/outputs mismatch");
  int64_t s0 = 0;
  for (int64_t k = 0; k < parts; ++k) {
    if (s0 % 8 || sizes[k] <= 0 || s0 + sizes[k] > Cl)
      throw std::runtime_error("Split " + n.name + ": parts must start at multiples of 8 channels");
    if (!n.outputs[k].empty()) emit_channel_slice(n, x, s0, s0 + sizes[k], n.outputs[k]);
    s0 += sizes[k];
  }
  if (s0 != Cl) throw std::runtime_error("Split " + n.name + ": sizes do not cover the axis");
}

// Slice of one token along axis 1 of [B, S, C] rows (e.g. the cls token) -> row gather; a channel
// range -> a column copy.
void Planner::lower_slice(int idx) {
  const Node& n = m_.nodes[idx];
  const Val x = val(n.in(0), n);
  std::vector<int64_t> starts = n.get_ints("starts"), ends = n.get_ints("ends"), axes = n.get_ints("axes"), steps;
  if (starts.empty() && n.inputs.size() >= 3) {  // opset >= 10: inputs
    ints_of(n.in(1), starts);
    ints_of(n.in(2), ends);
    if (n.inputs.size() > 3 && !n.in(3).empty()) ints_of(n.in(3), axes);
    if (n.inputs.size() > 4 && !n.in(4).empty()) ints_of(n.in(4), steps);
  }
  if (axes.empty())
    for (size_t i = 0; i < starts.size(); ++i) axes.push_back(static_cast<int64_t>(i));
  const int S = x.H * x.W;
  if (x.kind == Val::ROWS_BF16 && x.rank == 3 && x.pitch() == x.C && starts.size() == 1 && ends.size() == 1 &&
      axes.size() == 1 && axes[0] == 1 && (steps.empty() || steps[0] == 1)) {
    int64_t s0 = starts[0] < 0 ? starts[0] + S : starts[0];
    int64_t e0 = ends[0] < 0 ? ends[0] + S : std::min<int64_t>(ends[0], S);
    if (s0 >= 0 && e0 == s0 + 1) {
      PlanOp p;
      p.kind = PlanOp::GATHER_ROWS;
      p.name = n.name;
      p.in = x.buf;
      p.S = S;
      p.gidx = static_cast<int>(s0);
      p.C = x.C;
      p.out = new_buf(static_cast<size_t>(x.C) * 2);
      Val o;
      o.kind = Val::ROWS_BF16;
      o.C = x.C;
      o.H = 1;
      o.rank = 3;
      o.buf = p.out;
      define(n.outputs[0], o);
      add_op(std::move(p));
      return;
    }
  }
  // channel-axis slice [start, end) with start % 8 == 0: a column copy
  if (dense(x) && starts.size() == 1 && ends.size() == 1 && axes.size() == 1 && is_channel_axis(x, axes[0]) &&
      (steps.empty() || steps[0] == 1)) {
    const int64_t Cl = x.logical();
    int64_t s0 = starts[0] < 0 ? starts[0] + Cl : std::min<int64_t>(starts[0], Cl);
    int64_t e0 = ends[0] < 0 ? ends[0] + Cl : std::min<int64_t>(ends[0], Cl);
    if (s0 >= 0 && e0 > s0 && s0 % 8 == 0 && (e0 % 8 == 0 || e0 == Cl)) {
      emit_channel_slice(n, x, s0, e0, n.outputs[0]);
      return;
    }
  }
  throw std::runtime_error("Slice " + n.name + ": supported: one token along axis 1 of [B, S, C] rows, or a channel "
                           "range starting at a multiple of 8");
}

void Planner::lower_unary(int idx) {
  const Node& n = m_.nodes[idx];
  const Val x = materialize_in(n.in(0), n);
  const std::string& op = n.op_type;
  if (op == "Gelu" && n.get_string("approximate", "none") != "none")
    throw std::runtime_error("Gelu " + n.name + ": only the exact (erf) form is supported");
  static const std::map<std::string, int> codes = {
      {"Gelu", 2}, {"Sigmoid", 4}, {"Tanh", 5}, {"LeakyRelu", 6}, {"Exp", 7}, {"Abs", 8}, {"Sqrt", 9}, {"Neg", 10},
      {"Reciprocal", 11}, {"Log", 12}, {"Erf", 13}, {"Pow", 14}, {"HardSigmoid", 15}, {"HardSwish", 16}, {"Softplus", 17}};
  const int act = codes.at(op);
  float a = 0.f, b = 0.f;
  if (op == "LeakyRelu") a = n.get_float("alpha", 0.01f);
  if (op == "HardSigmoid") {
    a = n.get_float("alpha", 0.2f);
    b = n.get_float("beta", 0.5f);
  }
  if (op == "Pow") {  // activation ^ scalar constant
    auto it = m_.initializers.find(n.in(1));
    if (it == m_.initializers.end() || it->second.f.size() != 1)
      throw std::runtime_error("Pow " + n.name + ": the exponent must be a scalar constant");
    a = it->second.f[0];
  }
  emit_unary(n, x, act, a, b, n.outputs[0]);
}

void Planner::emit_unary(const Node& n, const Val& x, int act, float a, float b, const std::string& out_name) {
  if (!dense(x)) reject(n, "input must be a dense image or rows tensor");
  PlanOp p;
  p.kind = PlanOp::UNARY;
  p.name = n.name;
  p.in = x.buf;
  p.act = act;
  p.clip_lo = a;
  p.clip_hi = b;
  p.C = x.C;
  p.Cp = x.logical();  // pad columns are written 0 (exp(0) = 1, 1/0 = inf must not reach a GEMM)
  p.rows_per_sample = rows_of(x);
  p.out = buf_like(x);
  same_shape(out_name, x, p.out, /*clear_affine=*/true);
  add_op(std::move(p));
}

// Add / Sub / Mul / Div of two activations: same shape, or the second one broadcast per sample
// ([B, C, 1, 1] or [B, C] gates over an image's pixels / a sequence's rows: squeeze-excitation,
// GLU-style gating).  Returns false when the operands do not fit (the caller tries other forms).
bool Planner::lower_binary_acts(const Node& n) {
  if (n.inputs.size() != 2 || !vid_.count(n.in(0)) || !vid_.count(n.in(1))) return false;
  const std::string& t = n.op_type;
  static const std::map<std::string, int> ops = {
      {"Add", 0}, {"Sub", 1}, {"Mul", 2}, {"Div", 3}, {"Max", 4}, {"Min", 5}, {"Or", 4}, {"And", 5},
      {"Greater", 6}, {"Less", 7}, {"Equal", 8}, {"GreaterOrEqual", 9}, {"LessOrEqual", 10}};
  auto oi = ops.find(t);
  if (oi == ops.end()) return false;
  int op = oi->second;
  for (int side = 0; side < 2; ++side)
    if (vals_[vid_.at(n.in(side))].kind == Val::GRAPH_IN) materialize_in(n.in(side), n);
  Val a = vals_[vid_.at(n.in(0))], b = vals_[vid_.at(n.in(1))];
  if (!dense(a) || !dense(b) || a.C != b.C || a.logical() != b.logical()) return false;
  int ymode;
  if (a.kind == b.kind && a.H == b.H && a.W == b.W) {
    if (op == 0) return false;  // plain same-shape Add: the affine kernel's residual path
    ymode = 0;
  } else if (rows_of(b) == 1 && rows_of(a) > 1) {
    ymode = 1;
  } else if (rows_of(a) == 1 && rows_of(b) > 1 && op != 1 && op != 3) {
    std::swap(a, b);  // broadcast operand second: commutative ops, comparisons mirrored
    if (op >= 6) op = op == 6 ? 7 : op == 7 ? 6 : op == 9 ? 10 : op == 10 ? 9 : op;
    ymode = 1;
  } else {
    return false;
  }
  std::string cur = n.outputs[0];
  float lo = 0.f, hi = 0.f;
  PlanOp p;
  p.kind = PlanOp::BINARY;
  p.name = n.name;
  p.in = a.buf;
  p.in2 = b.buf;
  p.gidx = op;
  p.S = ymode;
  p.act = take_act(cur, lo, hi);
  p.clip_lo = lo;
  p.clip_hi = hi;
  p.C = a.C;
  p.Cp = a.logical();  // pad columns are written 0 (Div of two zero pads would be NaN)
  p.rows_per_sample = rows_of(a);
  p.out = buf_like(a);
  same_shape(cur, a, p.out, /*clear_affine=*/true);
  add_op(std::move(p));
  return true;
}

// The channel axis of a value (NHWC: NCHW axis 1; rows: the last axis) for Concat / Slice.
bool Planner::is_channel_axis(const Val& v, int64_t axis) {
  if (v.kind == Val::NHWC) return axis == 1 || axis == -3;
  const int r = v.rank ? v.rank : 2;
  return v.kind == Val::ROWS_BF16 && (axis == -1 || axis == r - 1);
}

void Planner::general_concat(const Node& n, int64_t axis) {
  std::vector<Val> xs;
  for (auto& in : n.inputs) xs.push_back(val(in, n));
  int Cs = 0, Cl = 0;
  for (size_t i = 0; i < xs.size(); ++i) {
    const Val& v = xs[i];
    if (!dense(v) || !is_channel_axis(v, axis) || v.kind != xs[0].kind || v.H != xs[0].H || v.W != xs[0].W)
      throw std::runtime_error("Concat " + n.name + ": inputs must be dense tensors of one shape, joined on the channel axis");
    if (i + 1 < xs.size() && v.padded())
      throw std::runtime_error("Concat " + n.name + ": only the last input may have a channel count that is not a multiple of 8");
    Cs += i + 1 < xs.size() ? v.logical() : v.C;
    Cl += v.logical();
  }
  const int out = new_buf(static_cast<size_t>(rows_of(xs[0])) * Cs * 2);
  int col = 0;
  for (size_t i = 0; i < xs.size(); ++i) {
    PlanOp p;
    p.kind = PlanOp::COPY_COLS;
    p.name = n.name + "#" + std::to_string(i);
    p.in = xs[i].buf;
    p.out = out;
    p.col[0] = 0;
    p.ld[0] = xs[i].C;
    p.col[1] = col;
    p.ld[1] = Cs;
    p.C = xs[i].C;
    p.rows_per_sample = rows_of(xs[0]);
    add_op(std::move(p));
    col += xs[i].logical();
  }
  Val o = xs[0];
  o.C = Cs;
  o.cl = Cl != Cs ? Cl : 0;
  o.buf = out;
  define(n.outputs[0], o);
}

}  // namespace die
