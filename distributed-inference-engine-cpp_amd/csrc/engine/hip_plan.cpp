#include "planner.h"

namespace die {

Plan Planner::run() {
  if (m_.inputs.empty() || m_.outputs.empty()) throw std::runtime_error("model needs an input and an output");
  for (size_t i = 0; i < m_.nodes.size(); ++i)
    for (auto& in : m_.nodes[i].inputs) consumers_[in].push_back(static_cast<int>(i));
  for (auto& o : m_.outputs) graph_outputs_.insert(o.name);
  for (size_t i = 0; i < m_.nodes.size(); ++i)
    for (auto& o : m_.nodes[i].outputs) producer_[o] = static_cast<int>(i);
  plan_.split = opt_.split;
  define_graph_input();

  done_.assign(m_.nodes.size(), false);
  for (size_t i = 0; i < m_.nodes.size(); ++i) {
    if (done_[i]) continue;
    done_[i] = true;
    const Node& n = m_.nodes[i];
    bool blocked = false;
    for (const auto& in : n.inputs) {
      auto it = vid_.find(in);
      if (it != vid_.end() && vals_[it->second].kind == Val::UNKNOWN) blocked = true;
    }
    if (blocked && !reports_own_input(n)) {
      report_.blocked++;
      mark_unknown(n);
      continue;
    }
    try {
      lower(static_cast<int>(i));
      check_output_view(n);
    } catch (const std::exception& e) {
      report_.supported = false;
      report_.unsupported.push_back(PlanReport::Item{n.name, n.op_type, e.what()});
      mark_unknown(n);
    }
  }
  if (!report_.supported) throw PlanUnsupported("HIP engine cannot lower this graph:\n" + report_.text());
  finalize_output();
  passes::fuse_pool_affine(plan_);
  if (opt_.fuse_stem_pool) passes::fuse_stem_pool(plan_);
  if (opt_.fuse_pairs) passes::fuse_conv_pairs(plan_);
  if (opt_.fuse_gap_fc) passes::fuse_gap_fc(plan_, max_batch_);
  // fp32 (split) mode only: in bf16 the weights re-rounded with gamma folded in and the mean
  // subtracted after a bf16-input GEMM cost ViT-B/16 ~3 % of its rel-L2 budget
  if (opt_.fold_layernorm && opt_.split) passes::fold_layernorm(plan_);
  if (opt_.fold_layernorm && opt_.split && opt_.ln_stats_epilogue) passes::stats_from_producer(plan_);
  if (opt_.side_branches) passes::mark_side_branches(plan_);
  passes::assign_arena(plan_, max_batch_);
  return std::move(plan_);
}

void Planner::mark_unknown(const Node& n) {
  Val u;
  u.kind = Val::UNKNOWN;
  for (const auto& o : n.outputs)
    if (!vid_.count(o)) define(o, u);
}

// Graph input 0 (the reference binds input 0 of any model, src/inference_engine.cpp:35-52):
//  * rank 4 [N, C, H, W]: an image (lazy: folded into the stem or an input-prep pass);
//  * rank 2 [N, F] / rank 3 [N, S, F]: rows -> one ROWS_PREP pass (f32 -> bf16 / split, F padded
//    to a multiple of 8).
void Planner::define_graph_input() {
  if (m_.inputs.size() > 1) return define_token_inputs();
  const auto& vi = m_.inputs[0];
  const size_t r = vi.dims.size();
  for (size_t k = 1; k < r; ++k)
    if (vi.dims[k] <= 0) throw std::runtime_error("input dims must be static except the batch");
  plan_.inputs = onnx::input_segments(m_);
  if (r == 2 && token_input(vi.name)) {  // [N, S] token ids: read in place by EMBED_TOKENS, no ROWS_PREP
    Val in;
    in.kind = Val::TOKEN_IDS;
    in.H = static_cast<int>(vi.dims[1]);
    in.buf = kBufGraphIn;
    in.pad.truncated = vi.elem_type == onnx::INT64 || vi.elem_type == onnx::INT32;
    define(vi.name, in);
    plan_.input_shape = {1, in.H};
    plan_.input_numel = static_cast<size_t>(in.H);
    return;
  }
  plan_.inputs[0].role = "activations";
  if (r == 4) {
    Val in;
    in.kind = Val::GRAPH_IN;
    in.C = static_cast<int>(vi.dims[1]);
    in.H = static_cast<int>(vi.dims[2]);
    in.W = static_cast<int>(vi.dims[3]);
    in.buf = kBufGraphIn;
    define(vi.name, in);
    plan_.input_shape = {1, in.C, in.H, in.W};
    plan_.input_numel = static_cast<size_t>(in.C) * in.H * in.W;
    return;
  }
  if (r != 2 && r != 3)
    throw std::runtime_error("HIP engine takes a rank-2, -3 or -4 input, got rank " + std::to_string(r));
  const int S = r == 3 ? static_cast<int>(vi.dims[1]) : 1;
  const int F = static_cast<int>(vi.dims[r - 1]);
  PlanOp p;
  p.kind = PlanOp::ROWS_PREP;
  p.name = "rows_prep";
  p.in = kBufGraphIn;
  p.C = F;
  p.Cp = round8(F);
  p.rows_per_sample = S;
  p.out = new_buf(static_cast<size_t>(S) * p.Cp * 2);
  Val v;
  v.kind = Val::ROWS_BF16;
  v.C = p.Cp;
  v.cl = p.Cp != F ? F : 0;
  v.H = S;
  v.rank = static_cast<int>(r);
  v.buf = p.out;
  add_op(std::move(p));
  define(vi.name, v);
  plan_.input_shape = r == 3 ? std::vector<int64_t>{1, S, F} : std::vector<int64_t>{1, F};
  plan_.input_numel = static_cast<size_t>(S) * F;
}

Planner::InputUse Planner::input_use(const std::string& name) const {
  static const char* flows[] = {"Not", "Unsqueeze", "Reshape", "Sub", "Mul", "Where", "Expand", "ReduceSum", "Identity"};
  InputUse u;
  std::vector<std::string> work{name};
  for (size_t w = 0; w < work.size(); ++w) {
    if (graph_outputs_.count(work[w])) u.other = true, u.mask_like = false, u.other_node = "(graph output)";
    for (int ci : consumers(work[w])) {
      const Node& c = m_.nodes[ci];
      if (c.op_type == "Cast") {
        work.push_back(c.outputs[0]);
      } else if (c.op_type == "Gather" && c.inputs.size() == 2 && c.in(1) == work[w] && c.in(0) != work[w]) {
        u.gathered = true;
      } else {
        const bool flow = std::any_of(std::begin(flows), std::end(flows), [&](const char* f) { return c.op_type == f; });
        const bool compare = c.op_type == "Equal" || c.op_type == "Greater" || c.op_type == "Less";
        if (!u.other) u.other_node = c.op_type + " " + c.name;
        u.other = u.other || !compare;  // a pad test against a scalar is a use of ids as ids
        u.mask_like = u.mask_like && flow;
      }
    }
  }
  return u;
}

// Two or three graph inputs: a token model taking attention_mask and / or token_type_ids next to
// its ids.  All are [N, S] with one S, declared FLOAT, INT64 or INT32, in any order; the request
// row of a sample is their concatenation in declaration order (onnx::input_segments), read in
// place.  Roles come from use: the indices of an embedding Gather (TOKEN_IDS; which of two is the
// ids and which the types is decided by declaration order, the lookups are symmetric) or a
// visibility value (KEYVIS rooted in the input: visible = value != 0, truncated first for an
// integer declaration).  Anything else is rejected here, naming the input.
void Planner::define_token_inputs() {
  const size_t K = m_.inputs.size();
  auto shape_of = [](const onnx::ValueInfo& vi) {
    std::string s = "[";
    for (size_t k = 0; k < vi.dims.size(); ++k) s += (k ? ", " : "") + (k == 0 ? std::string("N") : std::to_string(vi.dims[k]));
    return s + "]";
  };
  if (K > 3)
    throw std::runtime_error("the model has " + std::to_string(K) + " graph inputs (the last one '" + m_.inputs[K - 1].name +
                             "'): the HIP engine takes at most 3 (token ids, attention mask, token types)");
  const auto& first = m_.inputs[0];
  for (const auto& vi : m_.inputs) {
    if (vi.dims.size() != 2 || vi.dims[1] <= 0)
      throw std::runtime_error("input '" + vi.name + "' has the shape " + shape_of(vi) + ": with several graph inputs every "
                               "one must be [N, S] (token ids, attention mask, token types of a token model)");
    if (first.dims.size() == 2 && vi.dims[1] != first.dims[1])
      throw std::runtime_error("input '" + vi.name + "' has the shape " + shape_of(vi) + " but input '" + first.name + "' " +
                               shape_of(first) + ": the inputs of a token model share one sequence length S");
    if (vi.elem_type != onnx::FLOAT && vi.elem_type != onnx::INT64 && vi.elem_type != onnx::INT32)
      throw std::runtime_error("input '" + vi.name + "' must be declared FLOAT, INT64 or INT32");
  }
  const int S = static_cast<int>(first.dims[1]);
  plan_.inputs = onnx::input_segments(m_);
  int n_ids = 0, n_mask = 0;
  std::vector<Val> vals;
  for (size_t k = 0; k < K; ++k) {
    const auto& vi = m_.inputs[k];
    const InputUse u = input_use(vi.name);
    Val in;
    in.H = S;
    in.buf = kBufGraphIn;
    in.seg = static_cast<int>(plan_.inputs[k].offset);
    in.in_idx = static_cast<int>(k);
    in.pad.truncated = vi.elem_type != onnx::FLOAT;
    if (u.gathered && u.other)
      throw std::runtime_error("input '" + vi.name + "' is used both as the indices of an embedding Gather and in " +
                               u.other_node + ": a graph input is token ids or a mask, not both");
    if (u.gathered) {
      in.kind = Val::TOKEN_IDS;
      ++n_ids;
    } else if (u.other && u.mask_like) {
      in.kind = Val::KEYVIS;  // visible where the value is non-zero: not (value == 0)
      in.pad.op = 0;
      in.pad.value = 0.f;
      in.pad.negated = true;
      in.pad.src = in.seg;
      plan_.inputs[k].role = "mask";
      ++n_mask;
    } else {
      throw std::runtime_error("input '" + vi.name + "' is neither the indices of an embedding Gather nor an attention mask" +
                               (u.other_node.empty() ? " (it has no reader)" : " (read by " + u.other_node + ")") +
                               ": the only further graph inputs the HIP engine takes");
    }
    vals.push_back(in);
  }
  if (n_ids == 0)
    throw std::runtime_error("input '" + m_.inputs[1].name + "': a second graph input is taken only by token models, and no "
                             "input of this one indexes an embedding Gather");
  if (n_ids > 2 || n_mask > 1)
    throw std::runtime_error("input '" + m_.inputs[K - 1].name + "': at most two inputs index embedding tables (ids, token "
                             "types) and at most one is a mask");
  for (size_t k = 0; k < K; ++k) define(m_.inputs[k].name, vals[k]);
  plan_.input_shape = {1, static_cast<int64_t>(K), S};
  plan_.input_numel = K * static_cast<size_t>(S);
}

// ---- lowering ---------------------------------------------------------------------------------
// A node with an input from an unsupported node is counted as blocked and not tried -- except these,
// which are tried all the same because their own report line says more:
bool Planner::reports_own_input(const Node& n) const {
  // an Add / Where on attention scores whose mask came from an unsupported node is still tried:
  // its own report line says that the mask must be an initializer
  if (attn_mask_node(n)) return true;
  // (likewise an embedding Gather on token ids whose table came from an unsupported node: it
  // says that the table must be an initializer)
  if (n.op_type == "Gather" && token_node(n)) return true;
  // (and the Mul of a heads view by a rotary table that came from one: the tables must be initializers)
  if (n.op_type == "Mul" && rope_anchor(n)) return true;
  // (and a GroupNormalization / InstanceNormalization of a known value whose scale or bias came from
  // one: they must be initializers)
  if (n.op_type != "GroupNormalization" && n.op_type != "InstanceNormalization") return false;
  auto it = vid_.find(n.in(0));
  return it != vid_.end() && vals_[it->second].kind != Val::UNKNOWN;
}

// The dispatch.  Its order is semantics, not style: the predicates on the operands' kinds come before
// the ones on the op type, because they claim nodes the later lines would lower differently -- a
// node with a token-id / key-mask operand (token_node) before a repeat_kv in progress
// (kv_repeat_node), then the shape subgraph (lower_shape_op), then the anchors of the multi-node
// RoPE and RMSNorm patterns (which take Mul / Slice / Pow nodes away from lower_scale, lower_slice
// and lower_unary) and of torch's GroupNorm export (a Reshape of an image read by an
// InstanceNormalization, taken away from lower_reshape), and only then one line per op type.
void Planner::lower(int idx) {
  const Node& n = m_.nodes[idx];
  const std::string& op = n.op_type;
  if (token_node(n)) return lower_token_node(idx);
  if (kv_repeat_node(n)) return lower_kv_repeat(idx);
  if (lower_shape_op(idx)) return;
  if ((op == "Mul" || op == "Slice") && rope_anchor(n)) return lower_rope(idx);
  if ((op == "Pow" || (op == "Mul" && n.inputs.size() == 2 && n.in(0) == n.in(1))) && rmsnorm_anchor(n)) return lower_rmsnorm(idx);
  if (op == "RMSNormalization" || op == "SimplifiedLayerNormalization") return lower_layernorm(idx);
  if (op == "Reshape" && groupnorm_anchor(n)) return lower_groupnorm_chain(idx);
  if (op == "InstanceNormalization" || op == "GroupNormalization") return lower_groupnorm(idx);
  if (op == "Conv") return n.get_int("group", 1) != 1 ? lower_gconv(idx) : lower_conv(idx);
  if (op == "Gemm" || (op == "MatMul" && is_init(n.in(1)))) return lower_gemm(idx);
  if (op == "MatMul") return lower_attn_matmul(idx);
  if (op == "BatchNormalization") return lower_bn(idx);
  if (op == "Relu") return lower_relu(idx);
  if (op == "Add") return lower_add(idx);
  if (op == "MaxPool" || op == "AveragePool") return lower_pool(idx);
  if (op == "GlobalAveragePool") return lower_gap(idx);
  if (op == "Reshape") return lower_reshape(idx);
  if (op == "Flatten" || op == "Squeeze") return lower_flatten(idx);
  if (op == "Transpose") return lower_transpose(idx);
  if (op == "Div" || op == "Mul" || op == "Sub") return lower_scale(idx);
  if (op == "Softmax") return lower_softmax(idx);
  if (op == "Clip") return lower_clip(idx);
  if (op == "ReduceMean") return lower_reduce_mean(idx);
  if (op == "ReduceL2" || op == "LpNormalization") return lower_l2norm(idx);
  if (op == "ReduceSum" || op == "ReduceMax") {
    if (lower_spatial_reduce(idx, op == "ReduceSum" ? 1 : 2)) return;
    reject(n, "only reductions over the spatial axes of an image or the token axis of rows");
  }
  if (op == "GlobalMaxPool") return lower_gap(idx, 2);
  if (op == "Max" || op == "Min") {
    if (n.inputs.size() == 2 && lower_binary_acts(n)) return;
    reject(n, "only two activations of one shape (or a per-sample broadcast)");
  }
  if (op == "Pad") return lower_pad(idx);
  if (op == "ZeroInsert" && n.domain == "die") return lower_pad(idx);  // ConvTranspose rewrite (rewrite_for_device)
  if (op == "Greater" || op == "Less" || op == "Equal" || op == "GreaterOrEqual" || op == "LessOrEqual")
    return lower_compare(idx);
  if (op == "And" || op == "Or") {
    if (lower_binary_acts(n)) return;
    reject(n, "only two boolean activations of one shape");
  }
  if (op == "Not") return emit_unary(n, materialize_in(n.in(0), n), 23, 0.f, 0.f, n.outputs[0]);
  if (op == "Where") return lower_where(idx);
  if (op == "Cast") return lower_cast(idx);
  if (op == "Resize" || op == "Upsample") return lower_resize(idx);
  if (op == "Split") return lower_split(idx);
  if (op == "Slice") return lower_slice(idx);
  if (op == "LayerNormalization") return lower_layernorm(idx);
  if (op == "Gather") return lower_gather(idx);
  if (op == "Concat") return lower_concat(idx);
  if (op == "Sigmoid" || op == "Tanh" || op == "LeakyRelu" || op == "Gelu" || op == "Exp" || op == "Abs" ||
      op == "Sqrt" || op == "Neg" || op == "Reciprocal" || op == "Log" || op == "Erf" || op == "Pow" ||
      op == "HardSigmoid" || op == "HardSwish" || op == "Softplus")
    return lower_unary(idx);
  if (op == "Identity" || op == "Dropout") {
    Val v = val(n.in(0), n);
    define(n.outputs[0], v);
    return;
  }
  throw std::runtime_error("HIP engine: unsupported op " + op + " (" + n.name + ")");
}

// The graph output cannot be an [N, H, W, C] rows view: the output ops write [N, C] / [N, S, C] rows
// or NCHW images.  Checked after each node so that the report names the node producing it.
void Planner::check_output_view(const Node& n) {
  auto it = vid_.find(m_.outputs[0].name);
  if (output_view_seen_ || it == vid_.end() || vals_[it->second].kind != Val::ROWS_BF16 || vals_[it->second].rank != 4) return;
  output_view_seen_ = true;
  reject(n, "an [N, H, W, C] view of an image cannot be the graph output "
         "(transpose it back to [N, C, H, W])");
}

void Planner::finalize_output() {
  const std::string& name = m_.outputs[0].name;
  auto it = vid_.find(name);
  if (it == vid_.end()) throw std::runtime_error("graph output " + name + " is not produced");
  Val v = vals_[it->second];
  if (v.kind == Val::TOKCAT) {  // never materialised by a consumer
    emit_tokens(m_.nodes[0], v, nullptr, name + "#tokens");
    v = vals_[vid_.at(name + "#tokens")];
  }
  if (v.kind == Val::ROWS_F32 && v.buf == kBufGraphOut) {
    plan_.output_shape = {1, v.logical()};
    if (v.rank == 3) plan_.output_shape = {1, v.H, v.logical()};
  } else if (v.kind == Val::ROWS_BF16 || (v.kind == Val::NHWC && v.H == 1 && v.W == 1 &&
                                         m_.outputs[0].dims.size() == 2)) {
    PlanOp p;
    p.kind = PlanOp::BF16_TO_F32;
    p.name = "output_cast";
    if (v.pitch() != v.C || v.col || v.flat_hw) throw std::runtime_error("graph output is a strided view");
    p.in = v.buf;
    // padded rows: [rows][logical] f32 from rows of pitch C
    p.C = v.padded() ? v.logical() : v.C * v.H * v.W;
    p.ld_store = v.padded() ? v.C : 0;
    p.rows_per_sample = v.padded() ? static_cast<long long>(v.H) * v.W : 1;
    p.out_f32 = kBufGraphOut;
    add_op(std::move(p));
    plan_.output_shape = {1, v.logical()};
    if (v.kind == Val::ROWS_BF16 && v.rank == 3) plan_.output_shape = {1, v.H * v.W, v.logical()};
  } else if (v.kind == Val::NHWC) {
    PlanOp p;
    p.kind = PlanOp::TO_NCHW_F32;
    p.name = "output_nchw";
    p.in = v.buf;
    p.C = v.logical();
    p.ld_store = v.padded() ? v.C : 0;
    p.H = v.H;
    p.W = v.W;
    p.out_f32 = kBufGraphOut;
    add_op(std::move(p));
    plan_.output_shape = {1, v.logical(), v.H, v.W};
  } else {
    throw std::runtime_error("unsupported graph output layout");
  }
  plan_.output_numel = 1;
  for (auto dim : plan_.output_shape) plan_.output_numel *= static_cast<size_t>(dim);
}

const char* plan_kind_name(PlanOp::Kind kind) {
  static const char* kinds[] = {"input_prep", "conv", "pool", "gap", "affine", "to_nchw_f32", "bf16_to_f32",
                                "layernorm", "tokens", "gather_rows", "attention", "stem", "gconv", "softmax",
                                "rows_prep", "copy_cols", "binary", "unary", "conv_pair", "pad", "where", "resize", "bmm", "gap_fc",
                                "embed_tokens", "pool_tokens", "rope", "groupnorm", "grn"};
  static_assert(sizeof(kinds) / sizeof(kinds[0]) == PlanOp::GRN + 1, "one name per PlanOp kind");
  return kinds[kind];
}

std::string Plan::summary() const {
  std::ostringstream os;
  size_t convs = 0;
  for (auto& o : ops) convs += o.kind == PlanOp::CONV || o.kind == PlanOp::STEM || o.kind == PlanOp::CONV_PAIR;
  os << ops.size() << " device ops (" << convs << " MFMA conv/gemm), arena " << arena_bytes / (1 << 20) << " MiB, params "
     << params.size() / (1 << 20) << " MiB, " << flops_per_sample / 1e9 << " GFLOP/sample";
  return os.str();
}

namespace {

onnx::Attribute ints_attr(const std::string& name, std::vector<int64_t> v) {
  onnx::Attribute a;
  a.name = name;
  a.type = onnx::Attribute::INTS;
  a.ints = std::move(v);
  return a;
}

bool has_conv_transpose(const onnx::Model& m) {
  for (const auto& n : m.nodes)
    if (n.op_type == "ConvTranspose" && n.domain.empty()) return true;
  return false;
}

// ConvTranspose (2-D, group 1, dilation 1, explicit pads, weights an initializer) -> ZeroInsert +
// Conv: the input with stride - 1 zeros between its pixels and k - 1 - p zero borders (+ the output
// padding at the end), convolved at stride 1 with the transposed, flipped kernel -- the MFMA conv
// path instead of a scatter kernel.  Other ConvTranspose forms are left for the planner to report.
onnx::Model rewrite_conv_transpose(const onnx::Model& src) {
  onnx::Model m = src;
  std::vector<onnx::Node> out;
  for (const auto& n : src.nodes) {
    auto wi = m.initializers.find(n.in(1));
    bool ok = n.op_type == "ConvTranspose" && n.domain.empty() && wi != m.initializers.end() && wi->second.dims.size() == 4 &&
              n.get_int("group", 1) == 1 && !n.has("output_shape") && n.get_string("auto_pad", "NOTSET") == "NOTSET";
    const auto dl = n.get_ints("dilations", {1, 1}), st = n.get_ints("strides", {1, 1});
    const auto pd = n.get_ints("pads", {0, 0, 0, 0}), op = n.get_ints("output_padding", {0, 0});
    ok = ok && dl.size() == 2 && dl[0] == 1 && dl[1] == 1 && st.size() == 2 && pd.size() == 4 && op.size() == 2;
    if (!ok) {
      out.push_back(n);
      continue;
    }
    const auto& w = wi->second;
    const int64_t Cin = w.dims[0], Cout = w.dims[1], kh = w.dims[2], kw = w.dims[3];
    const std::vector<int64_t> zp = {kh - 1 - pd[0], kw - 1 - pd[1], kh - 1 - pd[2] + op[0], kw - 1 - pd[3] + op[1]};
    if (*std::min_element(zp.begin(), zp.end()) < 0) {  // cropping transposed convs: not rewritten
      out.push_back(n);
      continue;
    }
    onnx::Node zi;
    zi.name = n.name + "/zero_insert";
    zi.op_type = "ZeroInsert";
    zi.domain = "die";
    zi.inputs = {n.in(0)};
    zi.outputs = {n.outputs.at(0) + "/zero_insert"};
    zi.attrs["strides"] = ints_attr("strides", st);
    zi.attrs["pads"] = ints_attr("pads", zp);
    onnx::Tensor cw;
    cw.name = n.in(1) + "/as_conv";
    cw.dims = {Cout, Cin, kh, kw};
    cw.f.resize(static_cast<size_t>(Cout * Cin * kh * kw));
    for (int64_t ci = 0; ci < Cin; ++ci)
      for (int64_t co = 0; co < Cout; ++co)
        for (int64_t y = 0; y < kh; ++y)
          for (int64_t x = 0; x < kw; ++x)
            cw.f[((co * Cin + ci) * kh + y) * kw + x] = w.f[((ci * Cout + co) * kh + (kh - 1 - y)) * kw + (kw - 1 - x)];
    m.initializers[cw.name] = cw;
    onnx::Node cv;
    cv.name = n.name;
    cv.op_type = "Conv";
    cv.inputs = {zi.outputs[0], cw.name};
    if (!n.in(2).empty()) cv.inputs.push_back(n.in(2));
    cv.outputs = n.outputs;
    cv.attrs["kernel_shape"] = ints_attr("kernel_shape", {kh, kw});
    cv.attrs["strides"] = ints_attr("strides", {1, 1});
    cv.attrs["pads"] = ints_attr("pads", {0, 0, 0, 0});
    cv.attrs["dilations"] = ints_attr("dilations", {1, 1});
    out.push_back(std::move(zi));
    out.push_back(std::move(cv));
  }
  m.nodes = std::move(out);
  return m;
}

}  // namespace

Plan build_plan(const onnx::Model& m, int max_batch, const PlanOptions& opt) {
  const bool rw = has_conv_transpose(m);
  const onnx::Model r = rw ? rewrite_conv_transpose(m) : onnx::Model();
  return Planner(rw ? r : m, max_batch, opt).run();
}

std::string PlanReport::text() const {
  std::ostringstream os;
  for (const Item& it : unsupported) os << "  " << it.op << " '" << it.node << "': " << it.error << "\n";
  if (blocked) os << "  (" << blocked << " further node(s) depend on these)\n";
  return os.str();
}

PlanReport plan_report(const onnx::Model& m, int max_batch, bool split) {
  const bool rw = has_conv_transpose(m);
  const onnx::Model r = rw ? rewrite_conv_transpose(m) : onnx::Model();
  PlanOptions opt;
  opt.split = split;
  Planner p(rw ? r : m, max_batch, opt);
  try {
    p.run();
  } catch (const std::exception& e) {
    if (p.report_.supported) {  // failed outside the per-node walk (input, output layout)
      p.report_.supported = false;
      p.report_.unsupported.push_back(PlanReport::Item{"(graph)", "", e.what()});
    }
  }
  std::unordered_set<std::string> ct;
  for (const auto& n : m.nodes)
    if (n.op_type == "ConvTranspose") ct.insert(n.name);
  for (auto& it : p.report_.unsupported) {  // report rewritten nodes under the model's own names
    if (ct.count(it.node)) it.op = "ConvTranspose";
    const std::string suf = "/zero_insert";
    if (it.node.size() > suf.size() && it.node.compare(it.node.size() - suf.size(), suf.size(), suf) == 0) {
      it.node.resize(it.node.size() - suf.size());
      it.op = "ConvTranspose";
    }
  }
  return p.report_;
}

}  // namespace die
