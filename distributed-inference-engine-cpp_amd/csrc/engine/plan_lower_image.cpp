// Image (NHWC) lowerings:
//  * BatchNormalization directly on the graph input -> folded into the input-prep kernel that also
//    converts NCHW fp32 -> NHWC bf16 (it cannot be folded into the stem weights exactly, because the
//    stem's zero padding is applied after the BN);
//  * Conv -> BatchNormalization -> Relu  -> one conv with folded weights/bias and ReLU epilogue;
//  * Conv -> Add(other) [-> Relu]        -> residual epilogue (other operand already computed);
//  * value -> BatchNormalization [-> Relu] consumed next to the value itself (pre-activation units)
//    -> the producing conv's second output (dual store), so ResNet-v2 has no standalone BN/ReLU/Add;
//  * GlobalAveragePool / MaxPool / AveragePool -> NHWC kernels; Flatten of 1x1 maps -> view.
//  * channels-last blocks (ConvNeXt): Transpose(0,2,3,1) of a dense NHWC image is the same buffer read
//    as an [N, H, W, C] rows view (no op, no copy; lower_transpose), on which LayerNormalization over
//    the last axis, MatMul with a [C, N] initializer + bias Add and the erf-GELU chain take the rows
//    lowerings; Transpose(0,3,1,2) of such a view is the image again, and behind a GEMM the Add of the
//    shortcut image after it is that GEMM's residual epilogue (gemm_tail).  Mul(GEMM output, gamma [C])
//    with no other reader of the GEMM (layer scale) is folded into its weights and bias.  The
//    decomposed LayerNorm over axis 1 of an NCHW image is the LAYERNORM op over the image's rows
//    (lower_reduce_mean).  Depthwise 5x5 / 7x7 stride-1 convs are marked for the tiled kernel
//    (PlanOp::tiled).  Rejected with a report line: other 4-D permutes of an image, the view as the
//    graph output, a LayerNorm over any other axis.
// Standalone BatchNormalization / Relu / Add that fold into nothing become affine / add / relu kernels.
#include "planner.h"

namespace die {

// BN parameters -> per-channel (scale, shift).
void Planner::bn_affine(const Node& bn, std::vector<float>& sc, std::vector<float>& sh) {
  const auto& g = init(bn.in(1), bn).f;
  const auto& b = init(bn.in(2), bn).f;
  const auto& mu = init(bn.in(3), bn).f;
  const auto& var = init(bn.in(4), bn).f;
  const float eps = bn.get_float("epsilon", 1e-5f);
  sc.resize(g.size());
  sh.resize(g.size());
  for (size_t c = 0; c < g.size(); ++c) {
    sc[c] = g[c] / std::sqrt(var[c] + eps);
    sh[c] = b[c] - mu[c] * sc[c];
  }
}

int Planner::ensure_nhwc_input(Val& x, const std::string& name) {
  // Graph input -> input-prep kernel (applies any pending BN affine), memoised per value.
  auto it = prepped_.find(name);
  if (it != prepped_.end()) return it->second;
  PlanOp p;
  p.kind = PlanOp::INPUT_PREP;
  p.name = "input_prep";
  p.in = kBufGraphIn;
  p.C = x.C;
  p.H = x.H;
  p.W = x.W;
  p.Cp = x.C <= 4 ? 4 : round8(x.C);  // > 8 channels: input_prep_wide
  if (x.has_affine) {
    p.scale_off = push_f32(x.asc);
    p.shift_off = push_f32(x.ash);
  }
  p.out = new_buf(static_cast<size_t>(p.Cp) * x.H * x.W * 2);
  const int buf = p.out;
  add_op(std::move(p));
  prepped_[name] = buf;
  return buf;
}

// An image graph input (lazy: f32 NCHW plus any pending BN affine) consumed by something other
// than a conv's input load -- a ReLU, a pool, the residual operand of an Add: the input-prep
// pass materialises it as an NHWC tensor once (per value: the raw input and its BN'd form are
// two values) and every later reader sees that.  Hybrid HIP + CPU segments start at such inputs
// (engine/hybrid_engine.cpp: a ResNet segment begins at a unit's raw sum x).
Val Planner::materialize_in(const std::string& name, const Node& n) {
  Val v = val(name, n);
  if (v.kind != Val::GRAPH_IN) return v;
  const int buf = ensure_nhwc_input(v, name);
  Val o = v;
  o.kind = Val::NHWC;
  o.C = v.C <= 4 ? 4 : round8(v.C);
  o.cl = o.C != v.C ? v.C : 0;
  o.buf = buf;
  o.has_affine = false;
  o.asc.clear();
  o.ash.clear();
  define(name, o);
  return o;
}

void Planner::lower_conv(int idx) {
  const Node& n = m_.nodes[idx];
  Val x = val(n.in(0), n);
  const auto& wt = init(n.in(1), n);
  if (wt.dims.size() != 4) throw std::runtime_error("Conv " + n.name + ": only 2-D convs are supported");
  if (n.get_int("group", 1) != 1) throw std::runtime_error("Conv " + n.name + ": grouped convs are not supported yet");
  const int Cout = static_cast<int>(wt.dims[0]), Cin = static_cast<int>(wt.dims[1]);
  const int KH = static_cast<int>(wt.dims[2]), KW = static_cast<int>(wt.dims[3]);
  auto st = n.get_ints("strides", {1, 1});
  auto dl = n.get_ints("dilations", {1, 1});
  auto pads = conv_pads(n);
  if (st[0] != st[1] || dl[0] != dl[1]) throw std::runtime_error("Conv " + n.name + ": anisotropic stride/dilation");
  const std::string ap = n.get_string("auto_pad", "NOTSET");
  int in_buf;
  int Cstore;
  // A ResNet-style stem on the graph input reads the fp32 NCHW input itself (input_prep fused into
  // its patch loader); the prep pass is only planned if this conv turns out not to be that stem.
  bool deferred_prep = false;
  if (x.kind == Val::GRAPH_IN) {
    deferred_prep = KH == 7 && KW == 7 && x.C <= 4;
    in_buf = deferred_prep ? -2 : ensure_nhwc_input(x, n.in(0));
    Cstore = x.C <= 4 ? 4 : round8(x.C);
  } else if (x.kind == Val::NHWC) {
    in_buf = x.buf;
    Cstore = x.C;  // stored channels (pad channels get zero weights)
  } else {
    throw std::runtime_error("Conv " + n.name + ": input must be an image tensor");
  }
  if (Cin != (x.kind == Val::GRAPH_IN ? x.C : x.logical())) throw std::runtime_error("Conv " + n.name + ": channel mismatch");
  if (ap == "SAME_UPPER" || ap == "SAME_LOWER") {
    for (int d = 0; d < 2; ++d) {
      const int in = d ? x.W : x.H, k = d ? KW : KH;
      const int out = (in + static_cast<int>(st[0]) - 1) / static_cast<int>(st[0]);
      const int total = std::max(0, (out - 1) * static_cast<int>(st[0]) + (k - 1) * static_cast<int>(dl[0]) + 1 - in);
      const int lo = ap == "SAME_UPPER" ? total / 2 : total - total / 2;
      pads[d] = lo;
      pads[d + 2] = total - lo;
    }
  } else if (ap == "VALID") {
    pads = {0, 0, 0, 0};
  }
  // pads = [top, left, bottom, right]: the kernels offset by top/left and bound-check the input,
  // so asymmetric padding (TF-style SAME exports) only changes the output size
  const int s = static_cast<int>(st[0]), d = static_cast<int>(dl[0]);
  const int Ho = (x.H + static_cast<int>(pads[0] + pads[2]) - d * (KH - 1) - 1) / s + 1;
  const int Wo = (x.W + static_cast<int>(pads[1] + pads[3]) - d * (KW - 1) - 1) / s + 1;
  // Cout % 8 != 0: computed and stored with Cp channels (zero weights and bias: pad channels are
  // act(0)), the Val remembers the logical count
  const int Cp = round8(Cout);

  // --- fusion lookahead ---
  std::vector<float> scale(Cp, 1.f), shift(Cp, 0.f);
  if (!n.in(2).empty()) {
    const auto& b = init(n.in(2), n).f;
    for (int c = 0; c < Cout; ++c) shift[c] = b[c];
  }
  std::string cur = n.outputs[0];
  int c1 = next_op(cur, "BatchNormalization");
  if (c1 >= 0) {
    std::vector<float> sc, sh;
    bn_affine(m_.nodes[c1], sc, sh);
    for (int c = 0; c < Cout; ++c) {
      scale[c] = sc[c];
      shift[c] = shift[c] * sc[c] + sh[c];
    }
    done_[c1] = true;
    cur = m_.nodes[c1].outputs[0];
  }
  int relu = 0, res_buf = -1;
  float clip_lo = 0.f, clip_hi = 0.f;
  std::string res_name;
  c1 = sole_consumer(cur);
  if (c1 >= 0 && m_.nodes[c1].op_type == "Relu") {
    relu = 1;
    done_[c1] = true;
    cur = m_.nodes[c1].outputs[0];
  } else if (c1 >= 0 && m_.nodes[c1].op_type == "Clip" && clip_bounds(m_.nodes[c1], clip_lo, clip_hi)) {
    relu = 3;  // Clip epilogue (ReLU6)
    done_[c1] = true;
    cur = m_.nodes[c1].outputs[0];
  } else if (c1 >= 0 && m_.nodes[c1].op_type == "Add") {
    const Node& add = m_.nodes[c1];
    const std::string other = add.in(0) == cur ? add.in(1) : add.in(0);
    if (vid_.count(other) && vals_[vid_.at(other)].kind == Val::GRAPH_IN) materialize_in(other, add);
    auto it = vid_.find(other);
    if (it != vid_.end() && vals_[it->second].kind == Val::NHWC && vals_[it->second].C == Cp &&
        vals_[it->second].logical() == Cout && vals_[it->second].H == Ho && vals_[it->second].W == Wo &&
        add.in(0) != add.in(1)) {
      res_buf = vals_[it->second].buf;
      res_name = other;
      done_[c1] = true;
      cur = add.outputs[0];
      const int c2 = next_op(cur, "Relu");
      if (c2 >= 0) {
        relu = 1;
        done_[c2] = true;
        cur = m_.nodes[c2].outputs[0];
      }
    }
  }
  // dual store: a BN (+ReLU) consumer of `cur`
  std::string out2_name;
  std::vector<float> s2, b2;
  int relu2 = 0;
  int bn2 = -1;
  for (int ci : consumers(cur)) {
    if (!done_[ci] && m_.nodes[ci].op_type == "BatchNormalization" && m_.nodes[ci].in(0) == cur) {
      bn2 = ci;
      break;
    }
  }
  if (bn2 >= 0) {
    bn_affine(m_.nodes[bn2], s2, b2);
    s2.resize(Cp, 1.f);
    b2.resize(Cp, 0.f);
    done_[bn2] = true;
    out2_name = m_.nodes[bn2].outputs[0];
    const int c3 = next_op(out2_name, "Relu");
    if (c3 >= 0) {
      relu2 = 1;
      done_[c3] = true;
      out2_name = m_.nodes[c3].outputs[0];
    }
  }
  bool need_out1 = graph_outputs_.count(cur) != 0 || bn2 < 0;
  for (int ci : consumers(cur))
    if (ci != bn2) need_out1 = true;

  // --- weights: [Npad][Kpad] bf16, k = (ky*KW + kx)*Cstore + ci ---
  const int K = KH * KW * Cstore;
  const int Kpad = static_cast<int>(round_up(K, 64));
  const int Npad = static_cast<int>(round_up(Cp, 128));
  std::vector<float> wp(static_cast<size_t>(Npad) * Kpad, 0.f);
  for (int co = 0; co < Cout; ++co)
    for (int ci = 0; ci < Cin; ++ci)
      for (int ky = 0; ky < KH; ++ky)
        for (int kx = 0; kx < KW; ++kx) {
          const float w = wt.f[((static_cast<size_t>(co) * Cin + ci) * KH + ky) * KW + kx] * scale[co];
          wp[static_cast<size_t>(co) * Kpad + (ky * KW + kx) * Cstore + ci] = w;
        }

  PlanOp p;
  p.kind = PlanOp::CONV;
  p.name = n.name;
  p.in = in_buf;
  p.in2 = res_buf;
  // ResNet stem (7x7/2, pad 3, 4 stored input channels, 64 outputs, plain epilogue): LDS-patch kernel
  const bool stem = KH == 7 && KW == 7 && s == 2 && d == 1 && pads[0] == 3 && pads[1] == 3 && pads[2] == 3 &&
                    pads[3] == 3 && Cstore == 4 && Cout == 64 && res_buf < 0 && bn2 < 0 && need_out1 &&
                    relu != 3 && !graph_outputs_.count(cur);
  if (deferred_prep && !stem) {
    in_buf = ensure_nhwc_input(x, n.in(0));
    p.in = in_buf;
  }
  if (stem) {
    p.kind = PlanOp::STEM;
    if (in_buf == -2) {  // fused input prep: channel count and the input's pending affine
      p.C = x.C;
      if (x.has_affine) {
        p.scale_off = push_f32(x.asc);
        p.shift_off = push_f32(x.ash);
      }
    }
    std::vector<float> ws(64 * 224, 0.f);
    for (int co = 0; co < Cout; ++co)
      for (int ci = 0; ci < Cin; ++ci)
        for (int ky = 0; ky < 7; ++ky)
          for (int kx = 0; kx < 7; ++kx)
            ws[co * 224 + ky * 32 + kx * 4 + ci] = wt.f[((static_cast<size_t>(co) * Cin + ci) * KH + ky) * KW + kx] * scale[co];
    wp.swap(ws);
  }
  p.w_off = push_weights(wp, p.conv.wplane);
  p.conv.split = opt_.split;
  p.bias_off = push_f32(shift);
  auto& a = p.conv;
  a.H = x.H;
  a.W = x.W;
  a.Cin = Cstore;
  a.Ho = Ho;
  a.Wo = Wo;
  a.N = Cp;
  a.KH = KH;
  a.KW = KW;
  a.stride = s;
  a.pad_h = static_cast<int>(pads[0]);
  a.pad_w = static_cast<int>(pads[1]);
  a.dil = d;
  a.K = K;
  a.Kpad = Kpad;
  a.relu = relu;
  a.relu2 = relu2;
  a.clip_lo = clip_lo;
  a.clip_hi = clip_hi;
  p.flops_per_sample = 2.0 * Ho * Wo * Cout * (KH * KW * Cin);
  p.tile_bmax = kern::choose_tile(max_batch_ * Ho * Wo, Cp, K);
  const size_t out_bytes = static_cast<size_t>(Ho) * Wo * Cp * 2;
  Val o;
  o.kind = Val::NHWC;
  o.C = Cp;
  o.cl = Cp != Cout ? Cout : 0;
  o.H = Ho;
  o.W = Wo;
  if (need_out1) {
    p.out = new_buf(out_bytes);
    o.buf = p.out;
    define(cur, o);
  }
  if (bn2 >= 0) {
    p.s2_off = push_f32(s2);
    p.b2_off = push_f32(b2);
    p.out2 = new_buf(out_bytes);
    Val o2 = o;
    o2.buf = p.out2;
    define(out2_name, o2);
  }
  add_op(std::move(p));
}

// ---- Clip / grouped conv / decomposed LayerNorm / row softmax / constant binary ops ------------
// Clip bounds from attributes (opset < 11) or the optional min/max initializer inputs.
bool Planner::clip_bounds(const Node& n, float& lo, float& hi) const {
  lo = -3.4e38f;
  hi = 3.4e38f;
  if (n.has("min") || n.has("max")) {
    lo = n.get_float("min", lo);
    hi = n.get_float("max", hi);
    return true;
  }
  for (int k = 1; k <= 2; ++k) {
    if (n.inputs.size() <= static_cast<size_t>(k) || n.in(k).empty()) continue;
    auto it = m_.initializers.find(n.in(k));
    if (it == m_.initializers.end() || it->second.f.size() != 1) return false;
    (k == 1 ? lo : hi) = it->second.f[0];
  }
  return true;
}

// Activation consumer of `cur` (Relu / Clip): folds it into the producing op.
int Planner::take_act(std::string& cur, float& lo, float& hi) {
  const int c = sole_consumer(cur);
  if (c < 0) return 0;
  const Node& a = m_.nodes[c];
  int act = 0;
  if (a.op_type == "Relu") act = 1;
  else if (a.op_type == "Clip" && clip_bounds(a, lo, hi)) act = 3;
  if (!act) return 0;
  done_[c] = true;
  cur = a.outputs[0];
  return act;
}

// Grouped / depthwise Conv (group > 1): direct NHWC kernel, BN folded, ReLU/Clip epilogue.
void Planner::lower_gconv(int idx) {
  const Node& n = m_.nodes[idx];
  const Val x = val(n.in(0), n);
  if (x.kind != Val::NHWC) throw std::runtime_error("Conv " + n.name + ": grouped conv input must be an image tensor");
  const auto& wt = init(n.in(1), n);
  const int G = static_cast<int>(n.get_int("group", 1));
  const int Cout = static_cast<int>(wt.dims[0]), cpg = static_cast<int>(wt.dims[1]);
  const int KH = static_cast<int>(wt.dims[2]), KW = static_cast<int>(wt.dims[3]);
  if (cpg * G != x.C || Cout % G || Cout % 8 || x.C % 8)
    throw std::runtime_error("Conv " + n.name + ": grouped conv needs Cin = group * Cin/group and channels % 8 == 0");
  auto st = n.get_ints("strides", {1, 1});
  auto dl = n.get_ints("dilations", {1, 1});
  auto pads = conv_pads(n);
  if (st[0] != st[1] || dl[0] != dl[1]) throw std::runtime_error("Conv " + n.name + ": anisotropic stride/dilation");
  const std::string ap = n.get_string("auto_pad", "NOTSET");
  if (ap == "SAME_UPPER" || ap == "SAME_LOWER") {
    for (int d = 0; d < 2; ++d) {
      const int in = d ? x.W : x.H, k = d ? KW : KH;
      const int out = (in + static_cast<int>(st[0]) - 1) / static_cast<int>(st[0]);
      const int total = std::max(0, (out - 1) * static_cast<int>(st[0]) + (k - 1) * static_cast<int>(dl[0]) + 1 - in);
      const int lo = ap == "SAME_UPPER" ? total / 2 : total - total / 2;
      pads[d] = lo;
      pads[d + 2] = total - lo;
    }
  } else if (ap == "VALID") {
    pads = {0, 0, 0, 0};
  }
  const int s = static_cast<int>(st[0]), d = static_cast<int>(dl[0]);
  const int Ho = (x.H + static_cast<int>(pads[0] + pads[2]) - d * (KH - 1) - 1) / s + 1;
  const int Wo = (x.W + static_cast<int>(pads[1] + pads[3]) - d * (KW - 1) - 1) / s + 1;
  std::vector<float> scale(Cout, 1.f), shift(Cout, 0.f);
  if (!n.in(2).empty()) shift = init(n.in(2), n).f;
  std::string cur = n.outputs[0];
  int c1 = next_op(cur, "BatchNormalization");
  if (c1 >= 0) {
    std::vector<float> sc, sh;
    bn_affine(m_.nodes[c1], sc, sh);
    for (int c = 0; c < Cout; ++c) {
      scale[c] = sc[c];
      shift[c] = shift[c] * sc[c] + sh[c];
    }
    done_[c1] = true;
    cur = m_.nodes[c1].outputs[0];
  }
  PlanOp p;
  p.kind = PlanOp::GCONV;
  p.name = n.name;
  p.in = x.buf;
  p.act = take_act(cur, p.clip_lo, p.clip_hi);
  // fp32 weights [Cout][KH][KW][cpg] with the BN scale folded
  std::vector<float> w(static_cast<size_t>(Cout) * KH * KW * cpg);
  for (int co = 0; co < Cout; ++co)
    for (int ci = 0; ci < cpg; ++ci)
      for (int ky = 0; ky < KH; ++ky)
        for (int kx = 0; kx < KW; ++kx)
          w[((static_cast<size_t>(co) * KH + ky) * KW + kx) * cpg + ci] =
              wt.f[((static_cast<size_t>(co) * cpg + ci) * KH + ky) * KW + kx] * scale[co];
  p.w_off = push_f32(w);
  p.bias_off = push_f32(shift);
  if (G == x.C && G == Cout && s == 1 && d == 1 && KH == KW && (KH == 5 || KH == 7)) {
    std::vector<float> wt_tap(static_cast<size_t>(KH) * KW * Cout);
    for (int co = 0; co < Cout; ++co)
      for (int tap = 0; tap < KH * KW; ++tap) wt_tap[static_cast<size_t>(tap) * Cout + co] = w[static_cast<size_t>(co) * KH * KW + tap];
    p.tiled = 1;
    p.tap_w_off = push_f32(wt_tap);
  }
  p.groups = G;
  p.C = x.C;
  p.H = x.H;
  p.W = x.W;
  p.Ho = Ho;
  p.Wo = Wo;
  p.Cp = Cout;
  p.kh = KH;
  p.kw = KW;
  p.sh = s;
  p.sw = d;  // dilation
  p.ph = static_cast<int>(pads[0]);
  p.pw = static_cast<int>(pads[1]);
  p.flops_per_sample = 2.0 * Ho * Wo * Cout * KH * KW * cpg;
  p.out = new_buf(static_cast<size_t>(Ho) * Wo * Cout * 2);
  Val o;
  o.kind = Val::NHWC;
  o.C = Cout;
  o.H = Ho;
  o.W = Wo;
  o.buf = p.out;
  define(cur, o);
  add_op(std::move(p));
}

void Planner::lower_clip(int idx) {
  const Node& n = m_.nodes[idx];
  const Val x = val(n.in(0), n);
  float lo, hi;
  if (!clip_bounds(n, lo, hi)) throw std::runtime_error("Clip " + n.name + ": bounds must be constants");
  standalone_affine(n, x, nullptr, nullptr, nullptr, 3, lo, hi);
}

// ReduceMean / ReduceSum / ReduceMax over the spatial axes of an image or the token axis of
// rows: the GAP kernel in mode 0 / 1 / 2.  False when the reduction is some other one.
bool Planner::lower_spatial_reduce(int idx, int mode) {
  const Node& n = m_.nodes[idx];
  const Val x = materialize_in(n.in(0), n);
  std::vector<int64_t> ax;
  node_axes(n, ax);
  std::sort(ax.begin(), ax.end());
  const bool keep = n.get_int("keepdims", 1) != 0;
  const bool spatial = x.kind == Val::NHWC && (ax == std::vector<int64_t>{2, 3} || ax == std::vector<int64_t>{-2, -1});
  const bool tokens = x.kind == Val::ROWS_BF16 && x.rank == 3 && (ax == std::vector<int64_t>{1} || ax == std::vector<int64_t>{-2});
  if (!(spatial || tokens) || !dense(x)) return false;
  PlanOp p;
  p.kind = PlanOp::GAP;
  p.gidx = mode;
  p.name = n.name;
  p.in = x.buf;
  p.C = x.C;
  p.H = x.H;
  p.W = x.W;
  p.out = new_buf(static_cast<size_t>(x.C) * 2);
  Val o;
  o.kind = spatial && keep ? Val::NHWC : Val::ROWS_BF16;
  o.C = x.C;
  o.cl = x.cl;
  o.rank = tokens && keep ? 3 : 2;
  o.buf = p.out;
  define(n.outputs[0], o);
  add_op(std::move(p));
  return true;
}

// Explicit pads of a conv plus those of a zero Pad folded into it (lower_pad).
std::vector<int64_t> Planner::conv_pads(const Node& n) const {
  auto pads = n.get_ints("pads", {0, 0, 0, 0});
  if (pads.size() != 4) throw std::runtime_error("Conv " + n.name + ": expected 4 pads");
  auto it = folded_pad_.find(n.in(0));
  if (it != folded_pad_.end())
    for (int k = 0; k < 4; ++k) pads[k] += it->second[k];
  return pads;
}

// Pad (constant mode, value 0, spatial axes of an NHWC image only; the reference engine has no Pad
// kernel -- ONNX Runtime's CPU EP runs it there).  A Pad whose only reader is a Conv with explicit
// pads folds into that conv (the conv kernels read out-of-range pixels as zero); otherwise one
// NHWC pad pass writes the padded image.
// ZeroInsert (domain "die", from rewrite_conv_transpose): the same pass with strides: zeros between
// the input's pixels and `pads` = [top, left, bottom, right] around them.
void Planner::lower_pad(int idx) {
  const Node& n = m_.nodes[idx];
  int sy = 1, sx = 1;
  std::array<int64_t, 4> tlbr{};
  if (n.op_type == "ZeroInsert") {
    const auto st = n.get_ints("strides", {1, 1}), pd = n.get_ints("pads", {0, 0, 0, 0});
    sy = static_cast<int>(st.at(0));
    sx = static_cast<int>(st.at(1));
    for (int k = 0; k < 4; ++k) tlbr[k] = pd.at(k);
    const Val x = materialize_in(n.in(0), n);
    if (x.kind != Val::NHWC || !dense(x)) throw std::runtime_error("ConvTranspose " + n.name + ": input must be an image");
    return emit_pad(n, x, tlbr, sy, sx);
  }
  if (n.get_string("mode", "constant") != "constant") throw std::runtime_error("Pad " + n.name + ": only constant mode");
  std::vector<int64_t> pads = n.get_ints("pads");
  float value = n.get_float("value", 0.f);
  if (pads.empty() && n.inputs.size() >= 2) ints_of(n.in(1), pads);
  if (n.inputs.size() >= 3 && !n.in(2).empty()) {
    const auto& cv = init(n.in(2), n);
    value = cv.f.empty() ? (cv.i.empty() ? 0.f : static_cast<float>(cv.i[0])) : cv.f[0];
  }
  if (n.inputs.size() >= 4 && !n.in(3).empty()) throw std::runtime_error("Pad " + n.name + ": the axes input is not supported");
  if (value != 0.f) throw std::runtime_error("Pad " + n.name + ": only zero padding");
  const Val x = materialize_in(n.in(0), n);
  if (x.kind != Val::NHWC || pads.size() != 8 || pads[0] || pads[1] || pads[4] || pads[5])
    throw std::runtime_error("Pad " + n.name + ": only the spatial axes of an [N, C, H, W] image");
  for (auto v : pads)
    if (v < 0) throw std::runtime_error("Pad " + n.name + ": negative pads (cropping) are not supported");
  tlbr = {{pads[2], pads[3], pads[6], pads[7]}};
  emit_pad(n, x, tlbr, 1, 1);
}

void Planner::emit_pad(const Node& n, const Val& x, const std::array<int64_t, 4>& tlbr, int sy, int sx) {
  const int c = next_op(n.outputs[0], "Conv");
  if (sy == 1 && sx == 1 && c >= 0 && m_.nodes[c].in(0) == n.outputs[0] &&
      m_.nodes[c].get_string("auto_pad", "NOTSET") == "NOTSET") {
    folded_pad_[n.outputs[0]] = tlbr;
    define(n.outputs[0], x);
    return;
  }
  PlanOp p;
  p.kind = PlanOp::PAD;
  p.name = n.name;
  p.in = x.buf;
  p.C = x.C;
  p.H = x.H;
  p.W = x.W;
  p.ph = static_cast<int>(tlbr[0]);
  p.pw = static_cast<int>(tlbr[1]);
  p.sh = sy;
  p.sw = sx;
  p.Ho = (x.H - 1) * sy + 1 + static_cast<int>(tlbr[0] + tlbr[2]);
  p.Wo = (x.W - 1) * sx + 1 + static_cast<int>(tlbr[1] + tlbr[3]);
  p.out = new_buf(static_cast<size_t>(p.Ho) * p.Wo * x.C * 2);
  Val o = x;
  o.H = p.Ho;
  o.W = p.Wo;
  o.buf = p.out;
  define(n.outputs[0], o);
  add_op(std::move(p));
}

// Resize (opset 10+: scales / sizes inputs) and Upsample (scales attribute or input) of an
// image: nearest or linear over H, W.
void Planner::lower_resize(int idx) {
  const Node& n = m_.nodes[idx];
  const Val x = materialize_in(n.in(0), n);
  if (x.kind != Val::NHWC || !dense(x)) reject(n, "only images");
  const std::string mode = n.get_string("mode", "nearest");
  if (mode != "nearest" && mode != "linear" && mode != "bilinear")
    reject(n, "mode " + mode + " is not supported (nearest, linear)");
  if (n.get_int("antialias", 0) != 0) reject(n, "antialias is not supported");
  if (n.has("axes")) reject(n, "the axes attribute is not supported");
  std::vector<float> scales = n.get_floats("scales");
  std::vector<int64_t> sizes;
  const bool upsample = n.op_type == "Upsample";
  auto floats_of = [&](const std::string& nm) {
    auto it = m_.initializers.find(nm);
    if (it == m_.initializers.end()) reject(n, "scales must be a constant");
    return it->second.f;
  };
  if (scales.empty()) {
    if (upsample && n.inputs.size() >= 2) scales = floats_of(n.in(1));
    if (!upsample && n.inputs.size() == 2 && !n.in(1).empty()) scales = floats_of(n.in(1));  // opset 10
    if (!upsample && n.inputs.size() >= 3 && !n.in(2).empty() && !floats_of(n.in(2)).empty()) scales = floats_of(n.in(2));
    if (!upsample && scales.empty() && n.inputs.size() >= 4 && !n.in(3).empty() && !ints_of(n.in(3), sizes))
      reject(n, "sizes must be known at load time");
  }
  float sh, sw;
  int Ho, Wo;
  if (!sizes.empty()) {
    if (sizes.size() != 4 || (sizes[1] != x.logical() && sizes[1] != kBatchDim))
      reject(n, "sizes must be [N, C, H, W] with C unchanged");
    Ho = static_cast<int>(sizes[2]);
    Wo = static_cast<int>(sizes[3]);
    sh = static_cast<float>(Ho) / x.H;
    sw = static_cast<float>(Wo) / x.W;
  } else {
    if (scales.size() != 4 || scales[0] != 1.f || scales[1] != 1.f) reject(n, "scales must be [1, 1, sh, sw]");
    sh = scales[2];
    sw = scales[3];
    Ho = static_cast<int>(std::floor(x.H * static_cast<double>(sh)));
    Wo = static_cast<int>(std::floor(x.W * static_cast<double>(sw)));
  }
  if (Ho < 1 || Wo < 1 || !(sh > 0.f) || !(sw > 0.f)) reject(n, "empty output");
  static const std::map<std::string, int> coords = {{"half_pixel", 0}, {"asymmetric", 1}, {"align_corners", 2},
                                                    {"pytorch_half_pixel", 3}, {"tf_half_pixel_for_nn", 4}};
  static const std::map<std::string, int> nearests = {
      {"round_prefer_floor", 0}, {"round_prefer_ceil", 1}, {"floor", 2}, {"ceil", 3}};
  // Upsample and opset-10 Resize: asymmetric coordinates, floor rounding for nearest
  const bool legacy = upsample || m_.opset() < 11;
  const std::string cm = legacy ? "asymmetric" : n.get_string("coordinate_transformation_mode", "half_pixel");
  const std::string nm = legacy ? "floor" : n.get_string("nearest_mode", "round_prefer_floor");
  if (!coords.count(cm) || !nearests.count(nm))
    reject(n, "coordinate mode " + cm + " / nearest mode " + nm + " is not supported");
  PlanOp p;
  p.kind = PlanOp::RESIZE;
  p.name = n.name;
  p.in = x.buf;
  p.C = x.C;
  p.H = x.H;
  p.W = x.W;
  p.Ho = Ho;
  p.Wo = Wo;
  p.clip_lo = sh;
  p.clip_hi = sw;
  p.gidx = coords.at(cm);
  p.act = mode == "nearest" ? 0 : 1;
  p.is_max = nearests.at(nm);
  p.out = new_buf(static_cast<size_t>(Ho) * Wo * x.C * 2);
  Val o = x;
  o.H = Ho;
  o.W = Wo;
  o.buf = p.out;
  define(n.outputs[0], o);
  add_op(std::move(p));
}

void Planner::lower_bn(int idx) {
  const Node& n = m_.nodes[idx];
  Val& x = val(n.in(0), n);
  std::vector<float> sc, sh;
  bn_affine(n, sc, sh);
  if (x.kind == Val::GRAPH_IN) {  // fold into input prep
    Val v = x;
    if (v.has_affine) {
      for (size_t c = 0; c < sc.size(); ++c) {
        v.ash[c] = v.ash[c] * sc[c] + sh[c];
        v.asc[c] *= sc[c];
      }
    } else {
      v.has_affine = true;
      v.asc = sc;
      v.ash = sh;
    }
    define(n.outputs[0], v);
    return;
  }
  sc.resize(x.C, 1.f);
  sh.resize(x.C, 0.f);
  standalone_affine(n, x, &sc, &sh, nullptr);
}

void Planner::lower_relu(int idx) {
  const Node& n = m_.nodes[idx];
  const Val x = materialize_in(n.in(0), n);
  standalone_affine(n, x, nullptr, nullptr, nullptr);
}

void Planner::lower_add(int idx) {
  const Node& n = m_.nodes[idx];
  // attention scores + constant bias / mask table -> folded into the attention op
  for (int side = 0; side < 2 && n.inputs.size() == 2; ++side) {
    auto it = vid_.find(n.in(side));
    if (it != vid_.end() && vals_[it->second].kind == Val::ATTN && vals_[it->second].stage == 0) {
      const Val x = vals_[it->second];
      return lower_attn_mask(n, x, n.in(1 - side), 0);
    }
  }
  // [cls, patches] + position embedding -> token assembly
  for (int side = 0; side < 2; ++side) {
    auto it = vid_.find(n.in(side));
    if (it != vid_.end() && vals_[it->second].kind == Val::TOKCAT && is_init(n.in(1 - side))) {
      const Val cat = vals_[it->second];
      return emit_tokens(n, cat, &n.in(1 - side), n.outputs[0]);
    }
  }
  for (int side = 0; side < 2; ++side) {  // activation + per-channel / scalar constant
    if (!vid_.count(n.in(side)) || !is_init(n.in(1 - side))) continue;
    const Val& x = vals_[vid_.at(n.in(side))];
    const auto& c = m_.initializers.at(n.in(1 - side)).f;
    if (c.size() != 1 && static_cast<int>(c.size()) != x.logical()) continue;
    std::vector<float> sc(x.C, 1.f), sh(x.C, 0.f);
    for (int k = 0; k < x.logical(); ++k) sh[k] = c[c.size() == 1 ? 0 : k];
    return standalone_affine(n, x, &sc, &sh, nullptr);
  }
  for (int side = 0; side < 2; ++side)
    if (vid_.count(n.in(side)) && vals_[vid_.at(n.in(side))].kind == Val::GRAPH_IN) materialize_in(n.in(side), n);
  if (lower_binary_acts(n)) return;
  const Val a = val(n.in(0), n);
  const Val b = val(n.in(1), n);
  if (a.pitch() != a.C || b.pitch() != b.C || a.col || b.col)
    throw std::runtime_error("Add " + n.name + ": strided operands are not supported");
  if (a.kind != b.kind || a.C != b.C || a.H != b.H || a.W != b.W)
    throw std::runtime_error("Add " + n.name + ": broadcasting adds are not supported by the HIP engine");
  standalone_affine(n, a, nullptr, nullptr, &b);
}

void Planner::standalone_affine(const Node& n, const Val& x, const std::vector<float>* sc, const std::vector<float>* sh,
                                const Val* z, int own_act, float own_lo, float own_hi) {
  if (x.kind != Val::NHWC && x.kind != Val::ROWS_BF16) reject(n, "unsupported input layout");
  if (x.C % 8) reject(n, "channels must be a multiple of 8");
  if (x.pitch() != x.C || x.col) reject(n, "strided operand");
  std::string cur = n.outputs[0];
  int act = n.op_type == "Relu" ? 1 : own_act;
  float lo = own_lo, hi = own_hi;
  if (!act) act = take_act(cur, lo, hi);
  PlanOp p;
  p.clip_lo = lo;
  p.clip_hi = hi;
  p.kind = PlanOp::AFFINE;
  p.name = n.name;
  p.in = x.buf;
  p.in2 = z ? z->buf : -1;
  if (sc) {
    p.scale_off = push_f32(*sc);
    p.shift_off = push_f32(*sh);
  }
  p.act = act;
  p.C = x.C;
  p.rows_per_sample = static_cast<long long>(x.H) * x.W;
  p.out = buf_like(x);
  same_shape(cur, x, p.out, /*clear_affine=*/true);
  add_op(std::move(p));
}

void Planner::lower_pool(int idx) {
  const Node& n = m_.nodes[idx];
  Val x = materialize_in(n.in(0), n);
  if (x.kind != Val::NHWC) reject(n, "input must be an image tensor");
  auto k = n.get_ints("kernel_shape");
  auto st = n.get_ints("strides", {1, 1});
  auto pads = n.get_ints("pads", {0, 0, 0, 0});
  const bool cip_avg = n.op_type == "AveragePool" && n.get_int("count_include_pad", 0);
  if ((pads[0] != pads[2] || pads[1] != pads[3]) && cip_avg)
    reject(n, "count_include_pad with asymmetric pads is not supported");
  const bool ceil_mode = n.get_int("ceil_mode", 0) != 0;
  auto od = [&](int in, int d) {
    double v = static_cast<double>(in + pads[d] + pads[d + 2] - k[d]) / st[d];
    return static_cast<int>(ceil_mode ? std::ceil(v) : std::floor(v)) + 1;
  };
  PlanOp p;
  p.kind = PlanOp::POOL;
  p.name = n.name;
  p.in = x.buf;
  p.C = x.C;
  p.H = x.H;
  p.W = x.W;
  p.Ho = od(x.H, 0);
  p.Wo = od(x.W, 1);
  p.kh = static_cast<int>(k[0]);
  p.kw = static_cast<int>(k[1]);
  p.sh = static_cast<int>(st[0]);
  p.sw = static_cast<int>(st[1]);
  p.ph = static_cast<int>(pads[0]);
  p.pw = static_cast<int>(pads[1]);
  p.is_max = n.op_type == "MaxPool";
  p.cip = static_cast<int>(n.get_int("count_include_pad", 0));
  p.out = new_buf(static_cast<size_t>(p.Ho) * p.Wo * x.C * 2);
  Val o = x;
  o.H = p.Ho;
  o.W = p.Wo;
  o.buf = p.out;
  define(n.outputs[0], o);
  add_op(std::move(p));
}

// GlobalAveragePool (mode 0) / GlobalMaxPool (mode 2)
void Planner::lower_gap(int idx, int mode) {
  const Node& n = m_.nodes[idx];
  Val x = materialize_in(n.in(0), n);
  if (x.kind != Val::NHWC) throw std::runtime_error(n.op_type + ": input must be an image tensor");
  PlanOp p;
  p.kind = PlanOp::GAP;
  p.gidx = mode;
  p.name = n.name;
  p.in = x.buf;
  p.C = x.C;
  p.H = x.H;
  p.W = x.W;
  p.out = new_buf(static_cast<size_t>(x.C) * 2);
  Val o;
  o.kind = Val::NHWC;  // [C,1,1]
  o.C = x.C;
  o.cl = x.cl;
  o.buf = p.out;
  define(n.outputs[0], o);
  add_op(std::move(p));
}

void Planner::lower_flatten(int idx) {
  const Node& n = m_.nodes[idx];
  Val x = val(n.in(0), n);
  if (n.op_type == "Flatten" && n.get_int("axis", 1) != 1) throw std::runtime_error("Flatten: axis must be 1");
  if (x.kind == Val::NHWC && x.H * x.W > 1 && n.op_type == "Flatten") {
    define(n.outputs[0], flatten_nhwc(x));
    return;
  }
  if (!((x.kind == Val::ROWS_BF16 || x.kind == Val::NHWC) && x.H == 1 && x.W == 1))
    reject(n, "only flattening of 1x1 feature maps is supported");
  Val o = x;
  o.kind = Val::ROWS_BF16;
  o.rank = 2;
  define(n.outputs[0], o);
}

// [B, C, H, W] -> [B, C*H*W] over an NHWC buffer: a lazy view in (h, w, c) order that only a
// Gemm/MatMul with an initializer can consume (it permutes its weight rows to match).
Val Planner::flatten_nhwc(const Val& x) const {
  Val o;
  o.kind = Val::ROWS_BF16;
  o.rank = 2;
  o.C = x.H * x.W * x.C;
  o.buf = x.buf;
  o.flat_hw = x.H * x.W;
  o.flat_c = x.logical();
  return o;
}

}  // namespace die
