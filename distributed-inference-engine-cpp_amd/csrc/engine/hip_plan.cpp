#include "hip_plan.h"

#include "plan_passes.h"

#include <algorithm>
#include <array>
#include <climits>
#include <cmath>
#include <cstring>
#include <sstream>
#include <stdexcept>
#include <unordered_map>
#include <unordered_set>

namespace die {

using onnx::Node;

namespace {

using passes::from_bf16;
using passes::kBufGraphIn;
using passes::kBufGraphOut;
using passes::round_up;
using passes::to_bf16;

constexpr int64_t kBatchDim = INT64_MIN;  // symbolic batch size inside SHAPE values

// A planner value.  Besides materialised tensors (NHWC images, bf16/f32 rows) the planner keeps
// lazy views that only become kernels when consumed in a supported way.
struct Val {
  enum Kind {
    GRAPH_IN,    // f32 NCHW graph input
    NHWC,        // bf16 [B][H][W][C]
    ROWS_BF16,   // bf16 rows: logical [B, H*W, C] (rank 3) or [B, C] (rank 2, H*W == 1)
    ROWS_F32,    // f32 rows (graph output)
    NCHW_FLAT,   // Reshape(NHWC, [0, C, -1]) : logical [B, C, H*W] over an NHWC buffer
    HEADS,       // Reshape(rows, [0, 0, nh, hd]) (+ Transposes): base [B, S, nh, hd], logical = perm
    ATTN,        // attention chain: stage 0 = Q K^T, 1 = softmax, 2 = (P V) with logical perm
    SHAPE,       // int64 shape-computation value (ints known unless `known` is false)
    BCAST_INIT,  // Expand(initializer, shape) -> [B, 1, C]
    TOKCAT,      // Concat([cls, patch rows], axis=1)
    TOKEN_IDS,   // the rank-2 graph input [N, S] read as token ids (fp32 in the input buffer; H = S)
    KEYVIS,      // per-key boolean derived from the ids (padding): a pad test, a polarity, a shape
    KVREP,       // HF repeat_kv in progress on a heads view [N, Hkv, S, hd]: stage 1 = after Unsqueeze(2)
                 // [N, Hkv, 1, S, hd], 2 = after Expand [N, Hkv, G, S, hd] (kvg = G); the other fields = the view
    POOLV,       // masked mean pooling in progress (stage 0: rows x key mask [N, S, D], 1: their sum over the
                 // tokens [N, D], 2: the count of visible tokens [N, D] / [N, 1]); buf / C / cl / H = the rows
    UNKNOWN      // produced by a node the planner could not lower (support report)
  } kind = NHWC;
  int C = 0, H = 1, W = 1;
  // Stored vs logical channels: rows / NHWC pixels are stored with C channels (a multiple of 8:
  // 16-byte vectors, MFMA K/N steps); `cl` is the model's channel count when that is smaller (pad
  // channels hold finite values that every consumer ignores: zero weights, dropped on output).
  int cl = 0;
  // ROWS_BF16 from Flatten/Reshape of an NHWC map with H*W > 1: ONNX order is (c, h, w), the buffer
  // holds (h, w, c); a Gemm/MatMul consumer permutes its weight rows instead of the data.
  int flat_hw = 0, flat_c = 0;
  int buf = -1;
  int rank = 0;         // ROWS: 2 or 3; 4 = Transpose(0,2,3,1) of a dense NHWC image, the same buffer read as
                        // [N, H, W, C] rows (H * W rows of C per sample, kept in H; the image was img_h x img_w)
  int img_h = 0, img_w = 0;
  int ld = 0, col = 0;  // ROWS/HEADS: row pitch (0 -> C) and column offset, in elements
  bool has_affine = false;
  std::vector<float> asc, ash;
  // HEADS / ATTN
  int nh = 0, hd = 0;
  // HEADS behind a repeat_kv: nh counts the LOGICAL heads, the buffer stores nh / kvg of them and
  // logical head h is stored head h / kvg (no copy is made); 0 = no repeat
  int kvg = 0;
  std::array<int, 4> perm{{0, 1, 2, 3}};
  int q = -1, k = -1, v = -1, stage = 0;
  float scale = 1.f;
  int mask = -1;  // ATTN stage 0/1/2: index of the folded bias / mask table (Planner::masks_), -1 = none
  bool kmask = false;  // ATTN: the scores carry the request's key mask (PlanOp::key_mask)
  // TOKEN_IDS: pad.truncated = behind a Cast to an integer type.  KEYVIS: the value is true (additive
  // form, kv_add: masked, i.e. <= -1e4) where the test `pad` holds; kv_rank = 2 [N, S], 3 [N, 1, S],
  // 4 [N, 1, 1, S]
  PadTest pad;
  // TOKEN_IDS / KEYVIS of a model with several graph inputs: seg = the input's offset in a sample's
  // request row, in_idx = its place in the declaration order
  int seg = 0, in_idx = 0;
  int kv_rank = 2;
  bool kv_add = false;
  // KEYVIS for pooling: kv_last = unsqueezed at the LAST axis, [N, S, 1] (kv_rank 3), kv_D > 0 = then
  // expanded to [N, S, kv_D].  POOLV keeps the mask's fields; pool_c = stage 2: the count's lower bound
  bool kv_last = false;
  int kv_D = 0;
  float pool_c = 0.f;
  // SHAPE / BCAST_INIT / TOKCAT
  std::vector<int64_t> ints;
  bool known = true;
  std::string init_name;
  int patches = -1;
  int pitch() const { return ld ? ld : C; }
  int logical() const { return cl ? cl : C; }
  bool padded() const { return cl && cl != C; }
};

int round8(int c) { return (c + 7) / 8 * 8; }

class Planner {
 public:
  Planner(const onnx::Model& m, int max_batch, const PlanOptions& opt)
      : m_(m), max_batch_(max_batch), opt_(opt) {}

  // Every node is tried; a node that cannot be lowered is recorded (with its error) and its
  // outputs become UNKNOWN, so the walk goes on and the report lists every unsupported node.
  PlanReport report_;

  Plan run() {
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
      // an Add / Where on attention scores whose mask came from an unsupported node is still tried:
      // its own report line says that the mask must be an initializer
      // (likewise an embedding Gather on token ids whose table came from an unsupported node: it
      // says that the table must be an initializer)
      // (and the Mul of a heads view by a rotary table that came from one: the tables must be initializers)
      if (blocked && !attn_mask_node(n) && !(n.op_type == "Gather" && token_node(n)) && !(n.op_type == "Mul" && rope_anchor(n))) {
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

 private:
  // ---- helpers --------------------------------------------------------------------------------
  const onnx::Tensor& init(const std::string& name, const Node& n) const {
    auto it = m_.initializers.find(name);
    if (it == m_.initializers.end())
      throw std::runtime_error(n.op_type + " " + n.name + ": input " + name + " must be an initializer");
    return it->second;
  }
  bool is_init(const std::string& name) const { return m_.initializers.count(name) != 0; }
  Val& val(const std::string& name, const Node& n) {
    auto it = vid_.find(name);
    if (it == vid_.end()) throw std::runtime_error(n.op_type + " " + n.name + ": unknown input value " + name);
    return vals_[it->second];
  }
  void define(const std::string& name, const Val& v) {
    vid_[name] = static_cast<int>(vals_.size());
    vals_.push_back(v);
  }
  int sole_consumer(const std::string& name) const {
    if (graph_outputs_.count(name)) return -1;
    auto it = consumers_.find(name);
    if (it == consumers_.end() || it->second.size() != 1) return -1;
    return done_[it->second[0]] ? -1 : it->second[0];
  }
  std::vector<int> consumers(const std::string& name) const {
    auto it = consumers_.find(name);
    return it == consumers_.end() ? std::vector<int>{} : it->second;
  }
  int new_buf(size_t bytes_per_sample) { return passes::new_buf(plan_, bytes_per_sample); }
  size_t push_f32(const std::vector<float>& v) { return passes::push_f32(plan_, v); }
  size_t push_bf16(const std::vector<uint16_t>& v) { return passes::push_bf16(plan_, v); }
  // GEMM weights given in fp32: bf16, or (fp32 mode) the hi plane followed by the lo plane
  // (lo = bf16(w - hi)); `wplane` receives the plane distance in elements (0 when not split).
  size_t push_weights(const std::vector<float>& w, long long& wplane) {
    std::vector<uint16_t> q(w.size() * (opt_.split ? 2 : 1));
    for (size_t i = 0; i < w.size(); ++i) {
      q[i] = to_bf16(w[i]);
      if (opt_.split) {
        uint32_t u = static_cast<uint32_t>(q[i]) << 16;
        float hi;
        std::memcpy(&hi, &u, 4);
        q[w.size() + i] = to_bf16(w[i] - hi);
      }
    }
    wplane = opt_.split ? static_cast<long long>(w.size()) : 0;
    return push_bf16(q);
  }
  void add_op(PlanOp op) { plan_.ops.push_back(std::move(op)); }

  void mark_unknown(const Node& n) {
    Val u;
    u.kind = Val::UNKNOWN;
    for (const auto& o : n.outputs)
      if (!vid_.count(o)) define(o, u);
  }

  // Graph input 0 (the reference binds input 0 of any model, src/inference_engine.cpp:35-52):
  //  * rank 4 [N, C, H, W]: an image (lazy: folded into the stem or an input-prep pass);
  //  * rank 2 [N, F] / rank 3 [N, S, F]: rows -> one ROWS_PREP pass (f32 -> bf16 / split, F padded
  //    to a multiple of 8).
  void define_graph_input() {
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

  // How a graph input is used, through Casts: as the indices of a Gather, and / or in any other way
  // (`mask_like`: every such other use is one a key mask flows through or ends in).
  struct InputUse {
    bool gathered = false, other = false, mask_like = true;
    std::string other_node;
  };
  InputUse input_use(const std::string& name) const {
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
  void define_token_inputs() {
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

  // BN parameters -> per-channel (scale, shift).
  void bn_affine(const Node& bn, std::vector<float>& sc, std::vector<float>& sh) {
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

  // ---- lowering ---------------------------------------------------------------------------------
  void lower(int idx) {
    const Node& n = m_.nodes[idx];
    const std::string& op = n.op_type;
    if (token_node(n)) return lower_token_node(idx);
    if (kv_repeat_node(n)) return lower_kv_repeat(idx);
    if (lower_shape_op(idx)) return;
    if ((op == "Mul" || op == "Slice") && rope_anchor(n)) return lower_rope(idx);
    if ((op == "Pow" || (op == "Mul" && n.inputs.size() == 2 && n.in(0) == n.in(1))) && rmsnorm_anchor(n)) return lower_rmsnorm(idx);
    if (op == "RMSNormalization" || op == "SimplifiedLayerNormalization") return lower_layernorm(idx);
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
      throw std::runtime_error(op + " " + n.name + ": only reductions over the spatial axes of an image or the token axis of rows");
    }
    if (op == "GlobalMaxPool") return lower_gap(idx, 2);
    if (op == "Max" || op == "Min") {
      if (n.inputs.size() == 2 && lower_binary_acts(n)) return;
      throw std::runtime_error(op + " " + n.name + ": only two activations of one shape (or a per-sample broadcast)");
    }
    if (op == "Pad") return lower_pad(idx);
    if (op == "ZeroInsert" && n.domain == "die") return lower_pad(idx);  // ConvTranspose rewrite (rewrite_for_device)
    if (op == "Greater" || op == "Less" || op == "Equal" || op == "GreaterOrEqual" || op == "LessOrEqual")
      return lower_compare(idx);
    if (op == "And" || op == "Or") {
      if (lower_binary_acts(n)) return;
      throw std::runtime_error(op + " " + n.name + ": only two boolean activations of one shape");
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

  int ensure_nhwc_input(Val& x, const std::string& name) {
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
  Val materialize_in(const std::string& name, const Node& n) {
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

  void lower_conv(int idx) {
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
    int c1 = sole_consumer(cur);
    if (c1 >= 0 && m_.nodes[c1].op_type == "BatchNormalization") {
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
        const int c2 = sole_consumer(cur);
        if (c2 >= 0 && m_.nodes[c2].op_type == "Relu") {
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
      const int c3 = sole_consumer(out2_name);
      if (c3 >= 0 && m_.nodes[c3].op_type == "Relu") {
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

  // ---- GEMM over rows ---------------------------------------------------------------------------
  bool scalar_is(const std::string& name, float want) const {
    auto it = m_.initializers.find(name);
    if (it == m_.initializers.end() || it->second.f.size() != 1) return false;
    return std::fabs(it->second.f[0] - want) <= 1e-3f * std::fabs(want);
  }
  static const std::string& other_input(const Node& nd, const std::string& x) { return nd.in(0) == x ? nd.in(1) : nd.in(0); }

  // erf-GELU as exported by torch: x/sqrt2 -> Erf -> +1 -> (x * .) -> (* 0.5), or 0.5x * (1 + erf).
  bool match_gelu(const std::string& v, std::vector<int>& used, std::string& out) const {
    if (graph_outputs_.count(v)) return false;
    const auto cs = consumers(v);
    if (cs.size() != 2) return false;
    int dv = -1, mu = -1;
    for (int c : cs) {
      if (done_[c]) return false;
      const Node& nd = m_.nodes[c];
      if (nd.op_type == "Div" && nd.in(0) == v && scalar_is(nd.in(1), 1.41421356f)) dv = c;
      else if (nd.op_type == "Mul" && scalar_is(other_input(nd, v), 0.70710678f)) dv = c;
      else if (nd.op_type == "Mul") mu = c;
      else return false;
    }
    if (dv < 0 || mu < 0) return false;
    const int er = sole_consumer(m_.nodes[dv].outputs[0]);
    if (er < 0 || m_.nodes[er].op_type != "Erf") return false;
    const int ad = sole_consumer(m_.nodes[er].outputs[0]);
    if (ad < 0 || m_.nodes[ad].op_type != "Add" || !scalar_is(other_input(m_.nodes[ad], m_.nodes[er].outputs[0]), 1.f))
      return false;
    const std::string& a = m_.nodes[ad].outputs[0];
    const Node& M = m_.nodes[mu];
    const std::string& mo = other_input(M, v);
    if (mo == a) {
      const int hf = sole_consumer(M.outputs[0]);
      if (hf < 0 || m_.nodes[hf].op_type != "Mul" || !scalar_is(other_input(m_.nodes[hf], M.outputs[0]), 0.5f)) return false;
      used = {dv, er, ad, mu, hf};
      out = m_.nodes[hf].outputs[0];
      return true;
    }
    if (scalar_is(mo, 0.5f)) {
      const int fin = sole_consumer(a);
      if (fin < 0 || fin != sole_consumer(M.outputs[0]) || m_.nodes[fin].op_type != "Mul") return false;
      used = {dv, er, ad, mu, fin};
      out = m_.nodes[fin].outputs[0];
      return true;
    }
    return false;
  }

  struct GemmTail {
    std::vector<float> bias;  // from a following Add(initializer), empty if none
    int act = 0;              // 1 relu, 2 gelu
    std::string res;          // residual operand (rows; image = true: an NHWC image)
    std::vector<float> colscale;  // from a following Mul(initializer [N]) (layer scale), empty if none
    bool image = false;       // the tail went through Transpose(0,3,1,2): the output is the NHWC image of the view
    std::string out;
    std::vector<int> used;
  };
  // Epilogue fusion lookahead for a MatMul/Gemm producing `N` columns over `rows` rows per sample.
  GemmTail gemm_tail(const Node& n, int N, int rows, bool is_gemm, int N_logical, const Val& x) const {
    GemmTail t;
    t.out = n.outputs[0];
    int c1 = sole_consumer(t.out);
    if (!is_gemm && c1 >= 0 && m_.nodes[c1].op_type == "Add" && is_init(other_input(m_.nodes[c1], t.out))) {
      const auto& c = m_.initializers.at(other_input(m_.nodes[c1], t.out)).f;
      if (c.size() == static_cast<size_t>(N_logical) || c.size() == 1) {
        t.bias.assign(N, 0.f);
        for (int j = 0; j < N_logical; ++j) t.bias[j] = c[c.size() == 1 ? 0 : j];
        t.used.push_back(c1);
        t.out = m_.nodes[c1].outputs[0];
        c1 = sole_consumer(t.out);
      }
    }
    // Channels-last block tail on an [N, H, W, C] view (ConvNeXt): Mul(gamma [C]), the layer scale, is
    // folded into the GEMM's weights and bias by the caller; Transpose(0,3,1,2) -> Add(shortcut image)
    // is the residual epilogue and the output is the NHWC image
    if (x.kind == Val::ROWS_BF16 && x.rank == 4) {
      if (c1 >= 0 && m_.nodes[c1].op_type == "Mul" && N_logical > 1 && is_init(other_input(m_.nodes[c1], t.out))) {
        const auto& gm = m_.initializers.at(other_input(m_.nodes[c1], t.out));
        if (gm.f.size() == static_cast<size_t>(N_logical) && !gm.dims.empty() && gm.dims.back() == N_logical) {
          t.colscale = gm.f;
          t.used.push_back(c1);
          t.out = m_.nodes[c1].outputs[0];
          c1 = sole_consumer(t.out);
        }
      }
      if (c1 >= 0 && m_.nodes[c1].op_type == "Transpose" && m_.nodes[c1].get_ints("perm") == std::vector<int64_t>{0, 3, 1, 2}) {
        const int c2 = sole_consumer(m_.nodes[c1].outputs[0]);
        if (c2 >= 0 && m_.nodes[c2].op_type == "Add" && m_.nodes[c2].in(0) != m_.nodes[c2].in(1)) {
          const std::string& other = other_input(m_.nodes[c2], m_.nodes[c1].outputs[0]);
          auto it = vid_.find(other);
          if (it != vid_.end()) {
            const Val& r = vals_[it->second];
            if (r.kind == Val::NHWC && dense(r) && r.C == N && r.logical() == N_logical && r.H == x.img_h && r.W == x.img_w) {
              t.res = other;
              t.image = true;
              t.used.push_back(c1);
              t.used.push_back(c2);
              t.out = m_.nodes[c2].outputs[0];
              return t;
            }
          }
        }
      }
    }
    std::vector<int> gu;
    std::string g;
    if (c1 >= 0 && m_.nodes[c1].op_type == "Relu") {
      t.act = 1;
      t.used.push_back(c1);
      t.out = m_.nodes[c1].outputs[0];
    } else if (match_gelu(t.out, gu, g)) {
      t.act = 2;
      t.used.insert(t.used.end(), gu.begin(), gu.end());
      t.out = g;
    } else if (c1 >= 0 && m_.nodes[c1].op_type == "Add") {
      const Node& add = m_.nodes[c1];
      const std::string& other = other_input(add, t.out);
      auto it = vid_.find(other);
      if (it != vid_.end() && add.in(0) != add.in(1)) {
        const Val& r = vals_[it->second];
        if (r.kind == Val::ROWS_BF16 && r.C == N && r.logical() == N_logical && r.H * r.W == rows &&
            r.pitch() == r.C && r.col == 0) {
          t.res = other;
          t.used.push_back(c1);
          t.out = add.outputs[0];
          const int c2 = sole_consumer(t.out);
          if (c2 >= 0 && m_.nodes[c2].op_type == "Relu") {
            t.act = 1;
            t.used.push_back(c2);
            t.out = m_.nodes[c2].outputs[0];
          }
        }
      }
    }
    return t;
  }

  // Sibling MatMuls of one input that each only add a bias and feed a Reshape (Q/K/V projections)
  // -> one GEMM with concatenated weights.  Returns the group (just {idx} when not applicable).
  std::vector<int> qkv_group(int idx, const std::string& xname, int K) const {
    std::vector<int> g;
    bool self = false;
    for (int c : consumers(xname)) {
      if (c != idx && done_[c]) continue;
      const Node& nd = m_.nodes[c];
      if (nd.op_type != "MatMul" || nd.in(0) != xname || !is_init(nd.in(1))) continue;
      const auto& w = m_.initializers.at(nd.in(1));
      if (w.dims.size() != 2 || w.dims[0] != K || w.dims[1] % 8) continue;
      const int a = sole_consumer(nd.outputs[0]);
      if (a < 0 || m_.nodes[a].op_type != "Add" || !is_init(other_input(m_.nodes[a], nd.outputs[0]))) continue;
      if (m_.initializers.at(other_input(m_.nodes[a], nd.outputs[0])).f.size() != static_cast<size_t>(w.dims[1])) continue;
      const int r = sole_consumer(m_.nodes[a].outputs[0]);
      if (r < 0 || m_.nodes[r].op_type != "Reshape") continue;
      g.push_back(c);
      self |= c == idx;
    }
    if (!self || g.size() < 2) return {idx};
    return g;
  }

  void lower_gemm(int idx) {
    const Node& n = m_.nodes[idx];
    const Val x = val(n.in(0), n);
    const bool gemm = n.op_type == "Gemm";
    int rows = 1, rank = 2;
    if (x.kind == Val::ROWS_BF16) {
      rows = x.H * x.W;
      rank = x.rank ? x.rank : (rows == 1 ? 2 : 3);
    } else if (!(x.kind == Val::NHWC && x.H == 1 && x.W == 1)) {
      throw std::runtime_error(n.op_type + " " + n.name + ": input must be a [batch, (tokens,) features] matrix");
    }
    if (x.pitch() != x.C || x.col) throw std::runtime_error(n.op_type + " " + n.name + ": strided input rows");
    if (gemm && rank != 2) throw std::runtime_error("Gemm " + n.name + ": input must be 2-D");
    const auto& wt = init(n.in(1), n);
    if (wt.dims.size() != 2) throw std::runtime_error(n.op_type + " " + n.name + ": weight must be 2-D");
    if (gemm && n.get_int("transA", 0)) throw std::runtime_error("Gemm " + n.name + ": transA is not supported");
    const bool tb = gemm && n.get_int("transB", 0);
    const float alpha = gemm ? n.get_float("alpha", 1.f) : 1.f;
    const float beta = gemm ? n.get_float("beta", 1.f) : 1.f;
    // K: the model's inner dimension; Ks: the stored row length (pads / NHWC-flatten order)
    const int K = static_cast<int>(tb ? wt.dims[1] : wt.dims[0]);
    const int Ks = x.C;
    const int hw = x.flat_hw;  // Flatten of an NHWC map: logical k = c*hw + p sits at p*Cs + c
    const int Kl = hw ? x.flat_c * hw : x.logical();
    if (K != Kl) throw std::runtime_error(n.op_type + " " + n.name + ": inner dimension mismatch");
    auto kstore = [&](int k) { return hw ? (k % hw) * (Ks / hw) + k / hw : k; };

    const std::vector<int> group = gemm ? std::vector<int>{idx} : qkv_group(idx, n.in(0), K);
    // columns of each member
    std::vector<int> Ns, offs;
    int Ntot = 0;
    for (int gi : group) {
      const auto& w = init(m_.nodes[gi].in(1), m_.nodes[gi]);
      const int Nj = static_cast<int>(tb ? w.dims[0] : w.dims[1]);
      offs.push_back(Ntot);
      Ns.push_back(Nj);
      Ntot += Nj;
    }
    const int Np = group.size() > 1 ? Ntot : round8(Ntot);  // stored columns (QKV members are % 8 already)
    const int Kpad = static_cast<int>(round_up(Ks, 64));
    const int Npad = static_cast<int>(round_up(Np, 128));
    std::vector<float> wp(static_cast<size_t>(Npad) * Kpad, 0.f);
    std::vector<float> bias(Np, 0.f);
    for (size_t g = 0; g < group.size(); ++g) {
      const Node& nd = m_.nodes[group[g]];
      const auto& w = init(nd.in(1), nd);
      const int Nj = Ns[g];
      for (int j = 0; j < Nj; ++j)
        for (int k = 0; k < K; ++k) {
          const float v = tb ? w.f[static_cast<size_t>(j) * K + k] : w.f[static_cast<size_t>(k) * Nj + j];
          wp[static_cast<size_t>(offs[g] + j) * Kpad + kstore(k)] = alpha * v;
        }
      if (gemm && !nd.in(2).empty()) {
        const auto& c = init(nd.in(2), nd).f;
        for (int j = 0; j < Nj; ++j) bias[offs[g] + j] = beta * c[c.size() == 1 ? 0 : j % c.size()];
      }
    }
    // epilogue lookahead (a single GEMM only); a layer scale found there multiplies the weight columns
    const GemmTail t = group.size() > 1 ? GemmTail{} : gemm_tail(n, Np, rows, gemm, Ntot, x);
    for (size_t j = 0; j < t.colscale.size(); ++j)
      for (int k = 0; k < Kpad; ++k) wp[j * Kpad + k] *= t.colscale[j];
    PlanOp p;
    p.kind = PlanOp::CONV;
    p.name = group.size() > 1 ? n.name + "+qkv" : n.name;
    p.in = x.buf;
    p.w_off = push_weights(wp, p.conv.wplane);
    p.conv.split = opt_.split;
    auto& a = p.conv;
    a.H = a.Ho = rows;
    a.Cin = Ks;
    a.N = Np;
    a.K = Ks;
    a.Kpad = Kpad;
    p.flops_per_sample = 2.0 * rows * Ntot * K;
    p.tile_bmax = kern::choose_tile(max_batch_ * rows, Np, Ks);

    if (group.size() > 1) {
      // bias of each member's Add; outputs are column slices of one [rows][Ntot] buffer
      p.out = new_buf(static_cast<size_t>(rows) * Ntot * 2);
      for (size_t g = 0; g < group.size(); ++g) {
        done_[group[g]] = true;
        const Node& nd = m_.nodes[group[g]];
        const int ad = sole_consumer(nd.outputs[0]);
        const auto& c = m_.initializers.at(other_input(m_.nodes[ad], nd.outputs[0])).f;
        for (int j = 0; j < Ns[g]; ++j) bias[offs[g] + j] += c[j];
        done_[ad] = true;
        Val o;
        o.kind = Val::ROWS_BF16;
        o.C = Ns[g];
        o.H = rows;
        o.rank = rank;
        o.buf = p.out;
        o.ld = Ntot;
        o.col = offs[g];
        define(m_.nodes[ad].outputs[0], o);
      }
      p.bias_off = push_f32(bias);
      add_op(std::move(p));
      return;
    }

    for (int u : t.used) done_[u] = true;
    for (int j = 0; j < Np && !t.bias.empty(); ++j) bias[j] += t.bias[j];
    for (size_t j = 0; j < t.colscale.size(); ++j) bias[j] *= t.colscale[j];
    p.bias_off = push_f32(bias);
    a.relu = t.act;
    if (!t.res.empty()) p.in2 = vals_[vid_.at(t.res)].buf;
    Val o;
    o.C = Np;
    o.cl = Np != Ntot ? Ntot : 0;
    o.H = rows;
    o.rank = rank;
    o.img_h = x.img_h;
    o.img_w = x.img_w;
    if (t.image) {  // back in NCHW order: the NHWC image the view was taken of
      p.out = new_buf(static_cast<size_t>(rows) * Np * 2);
      o.kind = Val::NHWC;
      o.H = x.img_h;
      o.W = x.img_w;
      o.rank = o.img_h = o.img_w = 0;
      o.buf = p.out;
    } else if (graph_outputs_.count(t.out) && consumers(t.out).empty() && Np == Ntot && rank != 4) {
      p.out_f32 = kBufGraphOut;
      o.kind = Val::ROWS_F32;
      o.buf = kBufGraphOut;
    } else {
      p.out = new_buf(static_cast<size_t>(rows) * Np * 2);
      o.kind = Val::ROWS_BF16;
      o.buf = p.out;
    }
    define(t.out, o);
    add_op(std::move(p));
  }

  // ---- transformer views / ops --------------------------------------------------------------------
  // The axes of a Reduce* / Unsqueeze node: the attribute, or (opset 13+) input 1.  False when there
  // are none or they are not known.
  bool node_axes(const Node& n, std::vector<int64_t>& ax) const {
    ax = n.get_ints("axes");
    if (ax.empty() && n.inputs.size() > 1 && !n.in(1).empty()) return ints_of(n.in(1), ax) && !ax.empty();
    return !ax.empty();
  }
  bool ints_of(const std::string& nm, std::vector<int64_t>& out) const {
    auto it = vid_.find(nm);
    if (it != vid_.end() && vals_[it->second].kind == Val::SHAPE) {
      out = vals_[it->second].ints;
      return vals_[it->second].known;
    }
    auto ii = m_.initializers.find(nm);
    if (ii == m_.initializers.end()) return false;
    if (!ii->second.i.empty()) out = ii->second.i;
    else {
      out.clear();
      for (float f : ii->second.f) out.push_back(static_cast<int64_t>(f));
    }
    return true;
  }

  // Shape-computation subgraph (Shape/Gather/Concat/Unsqueeze/... on int64 shapes) and Expand.
  bool lower_shape_op(int idx) {
    const Node& n = m_.nodes[idx];
    const std::string& op = n.op_type;
    if (op == "Expand") {
      if (!is_init(n.in(0))) throw std::runtime_error("Expand " + n.name + ": only initializers can be expanded");
      const auto& t = m_.initializers.at(n.in(0));
      const int C = static_cast<int>(t.dims.empty() ? 1 : t.dims.back());
      if (static_cast<int64_t>(C) != t.numel()) throw std::runtime_error("Expand " + n.name + ": expects a [1, 1, C] token");
      Val v;
      v.kind = Val::BCAST_INIT;
      v.C = C;
      v.init_name = n.in(0);
      define(n.outputs[0], v);
      return true;
    }
    if (op == "Shape") {
      const Val x = val(n.in(0), n);
      Val s;
      s.kind = Val::SHAPE;
      if (x.kind == Val::GRAPH_IN || x.kind == Val::NHWC) s.ints = {kBatchDim, x.C, x.H, x.W};
      else if (x.kind == Val::ROWS_BF16 && x.rank == 3) s.ints = {kBatchDim, x.H * x.W, x.C};
      else if (x.kind == Val::ROWS_BF16) s.ints = {kBatchDim, x.C};
      else if (x.kind == Val::HEADS) {
        const int64_t base[4] = {kBatchDim, x.H, x.nh, x.hd};
        for (int i = 0; i < 4; ++i) s.ints.push_back(base[x.perm[i]]);
      } else s.known = false;
      define(n.outputs[0], s);
      return true;
    }
    bool any_shape = false;
    for (auto& in : n.inputs) {
      auto it = vid_.find(in);
      if (it != vid_.end() && vals_[it->second].kind == Val::SHAPE) any_shape = true;
    }
    if (!any_shape || op == "Reshape") return false;
    Val s;
    s.kind = Val::SHAPE;
    std::vector<int64_t> a, b;
    if (op == "Gather" && n.get_int("axis", 0) == 0) {
      s.known = ints_of(n.in(0), a) && ints_of(n.in(1), b);
      for (int64_t i : b) {
        if (!s.known) break;
        if (i < 0) i += static_cast<int64_t>(a.size());
        if (i < 0 || i >= static_cast<int64_t>(a.size())) s.known = false;
        else s.ints.push_back(a[i]);
      }
    } else if (op == "Concat") {
      for (auto& in : n.inputs) {
        if (!ints_of(in, a)) s.known = false;
        s.ints.insert(s.ints.end(), a.begin(), a.end());
      }
    } else if (op == "Unsqueeze" || op == "Squeeze" || op == "Cast" || op == "Identity") {
      s.known = ints_of(n.in(0), s.ints);
    } else {
      s.known = false;
    }
    for (auto& o : n.outputs) define(o, s);
    return true;
  }

  // ---- grouped-query attention: HF's repeat_kv on a K / V heads view -------------------------------
  // x [N, Hkv, S, hd] (the bhsd permutation, after the head Transpose and any rope op) ->
  // Unsqueeze(axes [2]) -> Expand to [., Hkv, G, S, hd] -> Reshape to [., Hkv * G, S, hd]: a heads view
  // of the SAME buffer with nh = Hkv * G and kvg = G.  No op, no copy; the attention op reads stored
  // head h / G for logical head h (PlanOp::kv_heads).
  bool kv_repeat_node(const Node& n) const {
    for (size_t i = 0; i < n.inputs.size(); ++i) {
      auto it = vid_.find(n.inputs[i]);
      if (it == vid_.end()) continue;
      const Val& x = vals_[it->second];
      if (x.kind == Val::KVREP) return true;
      if (i == 0 && x.kind == Val::HEADS && n.op_type == "Unsqueeze") return true;
    }
    return false;
  }

  void lower_kv_repeat(int idx) {
    const Node& n = m_.nodes[idx];
    const std::string where = n.op_type + " " + n.name + ": ";
    const Val x = val(n.in(0), n);
    const std::array<int, 4> bhsd{{0, 2, 1, 3}};
    if (n.op_type == "Unsqueeze" && x.kind == Val::HEADS) {
      std::vector<int64_t> ax;
      if (x.perm == std::array<int, 4>{{0, 1, 2, 3}})
        throw std::runtime_error(where + "a K/V repeat on the [N, S, H, hd] layout, before the head Transpose, is not "
                                 "supported (repeat_kv is matched on [N, Hkv, S, hd], after the Transpose and any rotary "
                                 "embedding)");
      if (x.perm != bhsd || !node_axes(n, ax) || ax != std::vector<int64_t>{2})
        throw std::runtime_error(where + "a heads view is unsqueezed only as the first node of repeat_kv: axes [2] on "
                                 "[N, Hkv, S, hd]");
      if (x.kvg) throw std::runtime_error(where + "the heads view already carries a K/V repeat");
      if (graph_outputs_.count(n.outputs[0])) throw std::runtime_error(where + "a heads view cannot be a graph output");
      Val o = x;
      o.kind = Val::KVREP;
      o.stage = 1;
      define(n.outputs[0], o);
      return;
    }
    if (x.kind != Val::KVREP)
      throw std::runtime_error(where + "reads a K/V repeat in progress: repeat_kv is Unsqueeze -> Expand -> Reshape on the "
                               "heads view alone");
    const int Hkv = x.nh, S = x.H, hd = x.hd;
    if (n.op_type == "Expand" && x.stage == 1) {
      std::vector<int64_t> e;
      if (n.inputs.size() < 2 || !ints_of(n.in(1), e))
        throw std::runtime_error(where + "the shape of a K/V repeat must be static (a constant, or folded from Shape nodes)");
      const bool ok = e.size() == 5 && (e[0] == 1 || e[0] == kBatchDim) && (e[1] == 1 || e[1] == Hkv) && e[2] >= 1 &&
                      (e[3] == 1 || e[3] == S) && (e[4] == 1 || e[4] == hd);
      if (!ok) {
        std::string shp;
        for (auto d : e) shp += (shp.empty() ? "" : ", ") + (d == kBatchDim ? std::string("N") : std::to_string(d));
        throw std::runtime_error(where + "a K/V repeat expands axis 2 alone, [N, " + std::to_string(Hkv) + ", 1, " +
                                 std::to_string(S) + ", " + std::to_string(hd) + "] -> [N, " + std::to_string(Hkv) + ", G, " +
                                 std::to_string(S) + ", " + std::to_string(hd) + "]; got the shape [" + shp + "]");
      }
      if (graph_outputs_.count(n.outputs[0])) throw std::runtime_error(where + "a heads view cannot be a graph output");
      Val o = x;
      o.stage = 2;
      o.kvg = static_cast<int>(e[2]);
      define(n.outputs[0], o);
      return;
    }
    if (n.op_type == "Reshape" && x.stage == 2) {
      std::vector<int64_t> shp;
      if (!ints_of(n.in(1), shp)) throw std::runtime_error(where + "target shape must be static");
      const int G = x.kvg;
      const bool ok = shp.size() == 4 && (shp[0] == 0 || shp[0] == -1 || shp[0] == kBatchDim) &&
                      shp[1] == static_cast<int64_t>(Hkv) * G && shp[2] == S && shp[3] == hd;
      if (!ok)
        throw std::runtime_error(where + "a K/V repeat ends in a Reshape to [N, Hkv * G, S, hd] = [N, " +
                                 std::to_string(Hkv * G) + ", " + std::to_string(S) + ", " + std::to_string(hd) +
                                 "] (batch entry 0, -1 or N)");
      // the repeated view exists for the attention MatMuls only (K through its Transpose)
      auto only_matmuls = [&](const std::string& v, bool through_transpose, auto&& self) -> std::string {
        if (graph_outputs_.count(v)) return "(graph output)";
        for (int c : consumers(v)) {
          const Node& r = m_.nodes[c];
          if (r.op_type == "MatMul") continue;
          if (r.op_type == "Transpose" && through_transpose) {
            const std::string bad = self(r.outputs[0], false, self);
            if (!bad.empty()) return bad;
            continue;
          }
          return r.op_type + " " + r.name;
        }
        return std::string();
      };
      const std::string bad = only_matmuls(n.outputs[0], true, only_matmuls);
      if (!bad.empty())
        throw std::runtime_error(where + "the repeated K/V view is read by " + bad + ": only the attention MatMuls (and the "
                                 "Transpose of K before Q K^T) may read it -- the repeat is never materialised");
      Val o = x;
      o.kind = Val::HEADS;
      o.stage = 0;
      o.nh = Hkv * G;
      define(n.outputs[0], o);
      return;
    }
    throw std::runtime_error(where + "reads a K/V repeat in progress: repeat_kv is Unsqueeze(axes [2]) -> Expand -> Reshape "
                             "on the heads view alone");
  }

  // ---- token-id models: embedding lookup and the request's own key (padding) mask ------------------
  // A rank-2 graph input [N, S] is a token input when every consumer treats it as ids: an optional
  // Cast to INT64 / INT32, the indices of a Gather, and the pad tests Equal / Greater / Less against
  // a scalar initializer -- and at least one Gather reads it (any other rank-2 input plans as rows).
  // Whether the Gather is one the engine lowers (axis 0, an initializer table) is lower_embed's
  // business: a token input with a Gather it rejects gives that report line.
  bool token_input(const std::string& name) const {
    bool gathered = false;
    std::vector<std::string> work{name};
    for (size_t w = 0; w < work.size(); ++w) {
      if (graph_outputs_.count(work[w])) return false;
      for (int ci : consumers(work[w])) {
        const Node& c = m_.nodes[ci];
        if (c.op_type == "Cast") {
          const int to = static_cast<int>(c.get_int("to", onnx::FLOAT));
          if (to != onnx::INT64 && to != onnx::INT32) return false;
          work.push_back(c.outputs[0]);
        } else if (c.op_type == "Gather" && c.inputs.size() == 2 && c.in(1) == work[w] && c.in(0) != work[w]) {
          gathered = true;
        } else if (c.op_type == "Equal" || c.op_type == "Greater" || c.op_type == "Less") {
          float f;
          if (c.inputs.size() != 2 || !scalar_init(c.in(0) == work[w] ? c.in(1) : c.in(0), f)) return false;
        } else {
          return false;
        }
      }
    }
    return gathered;
  }

  // A node with a token-id or key-visibility operand: lowered by lower_token_node or rejected there
  // (nothing else in the planner knows these values).
  bool token_node(const Node& n) const {
    for (const auto& in : n.inputs) {
      auto it = vid_.find(in);
      if (it != vid_.end() && (vals_[it->second].kind == Val::TOKEN_IDS || vals_[it->second].kind == Val::KEYVIS ||
                               vals_[it->second].kind == Val::POOLV))
        return true;
    }
    return false;
  }

  const Val* val_if(const std::string& name, Val::Kind kind) const {
    auto it = vid_.find(name);
    return it != vid_.end() && vals_[it->second].kind == kind ? &vals_[it->second] : nullptr;
  }

  // The token-id value `name` is, or is a Cast to INT64 / INT32 of (a Cast that need not be lowered yet)
  const Val* ids_behind(std::string name) const {
    for (int hops = 0; hops < 4; ++hops) {
      if (const Val* v = val_if(name, Val::TOKEN_IDS)) return v;
      auto pr = producer_.find(name);
      if (pr == producer_.end() || m_.nodes[pr->second].op_type != "Cast") return nullptr;
      const int to = static_cast<int>(m_.nodes[pr->second].get_int("to", onnx::FLOAT));
      if (to != onnx::INT64 && to != onnx::INT32) return nullptr;
      name = m_.nodes[pr->second].in(0);
    }
    return nullptr;
  }

  // The first EMBED_TOKENS op of the plan also writes the key data (kvis, kend) every key-masked
  // attention reads; one pad test per model.
  int key_op_ = -1;           // index of that op; its out2 / out3 = kvis / kend once a mask uses them
  bool key_test_set_ = false;

  void lower_token_node(int idx) {
    const Node& n = m_.nodes[idx];
    const std::string& op = n.op_type;
    const std::string who = op + " " + n.name + ": ";
    if (lower_pool_node(idx)) return;
    if (const Val* ids = n.inputs.empty() ? nullptr : val_if(n.in(0), Val::TOKEN_IDS)) {
      if (op == "Cast") {
        const int to = static_cast<int>(n.get_int("to", onnx::FLOAT));
        if (to != onnx::INT64 && to != onnx::INT32) throw std::runtime_error(who + "token ids cast only to INT64 / INT32");
        Val o = *ids;
        o.pad.truncated = true;
        define(n.outputs[0], o);
        return;
      }
    }
    if (op == "Gather" && n.inputs.size() == 2 && val_if(n.in(1), Val::TOKEN_IDS)) return lower_embed(idx);
    if (op == "Equal" || op == "Greater" || op == "Less") {  // pad test roots
      for (int side = 0; side < 2 && n.inputs.size() == 2; ++side) {
        const Val* ids = val_if(n.in(side), Val::TOKEN_IDS);
        float c = 0.f;
        if (!ids || !scalar_init(n.in(1 - side), c)) continue;
        Val o;
        o.kind = Val::KEYVIS;
        o.H = ids->H;
        o.pad.op = op == "Equal" ? 0 : (op == "Greater") == (side == 0) ? 1 : 2;  // c > ids = ids < c
        o.pad.value = c;
        o.pad.truncated = ids->pad.truncated;
        if (m_.inputs.size() > 1) o.pad.src = ids->seg;  // which of the inputs the test reads
        define(n.outputs[0], o);
        return;
      }
      throw std::runtime_error(who + "token ids compare only with a scalar initializer");
    }
    // consumers on attention scores: Where(vis, scores, f), Where(hidden, f, scores), Add(scores, additive)
    if (op == "Where" && n.inputs.size() == 3) {
      const Val* m = val_if(n.in(0), Val::KEYVIS);
      for (int side = 1; side <= 2 && m; ++side) {
        const Val* x = val_if(n.in(side), Val::ATTN);
        if (!x || x->stage != 0) continue;
        check_score_fill(n, n.in(3 - side));
        if (m->kv_add) throw std::runtime_error(who + "the condition must be a boolean key mask");
        return define_key_masked(n, *x, *m, side == 1);
      }
    }
    if (op == "Add" && n.inputs.size() == 2)
      for (int side = 0; side < 2; ++side) {
        const Val* m = val_if(n.in(side), Val::KEYVIS);
        const Val* x = val_if(n.in(1 - side), Val::ATTN);
        if (!m || !x || x->stage != 0) continue;
        if (!m->kv_add)
          throw std::runtime_error(who + "a key mask added to attention scores must be additive (mask * c with c <= -1e4)");
        return define_key_masked(n, *x, *m, false);  // masked where the value is true
      }
    // propagation
    const Val* m = n.inputs.empty() ? nullptr : val_if(n.in(0), Val::KEYVIS);
    if (m && !m->kv_add && (op == "Not" || op == "Cast" || op == "Identity")) {
      Val o = *m;
      if (op == "Not") o.pad.negated = !o.pad.negated;
      // a mask input cast to an integer type: the test reads the truncated value from there on
      const int to = op == "Cast" ? static_cast<int>(n.get_int("to", onnx::FLOAT)) : 0;
      if (o.pad.src >= 0 && (to == onnx::INT64 || to == onnx::INT32)) o.pad.truncated = true;
      define(n.outputs[0], o);
      return;
    }
    if (m && op == "Unsqueeze") {
      std::vector<int64_t> axes;
      node_axes(n, axes);
      Val o = *m;
      o.kv_rank = m->kv_rank + static_cast<int>(axes.size());
      bool ok = !axes.empty() && o.kv_rank <= 4;
      for (int64_t a : axes) {
        if (a < 0) a += o.kv_rank;
        ok = ok && a >= 1 && a <= o.kv_rank - 2;  // the batch stays first, the keys last
      }
      if (!ok) throw std::runtime_error(who + "a key mask is unsqueezed only towards [N, 1, 1, S]");
      define(n.outputs[0], o);
      return;
    }
    if (m && op == "Reshape") {
      std::vector<int64_t> shp;
      const bool ok = ints_of(n.in(1), shp) && shp.size() == 4 && (shp[0] == 0 || shp[0] == -1 || shp[0] == kBatchDim) &&
                      shp[1] == 1 && shp[2] == 1 && (shp[3] == m->H || (shp[3] == -1 && shp[0] != -1));
      if (!ok) throw std::runtime_error(who + "a key mask is reshaped only to [N, 1, 1, S]");
      Val o = *m;
      o.kv_rank = 4;
      define(n.outputs[0], o);
      return;
    }
    if (op == "Sub" && n.inputs.size() == 2 && scalar_is(n.in(0), 1.f)) {  // 1 - m
      if (const Val* s = val_if(n.in(1), Val::KEYVIS); s && !s->kv_add) {
        Val o = *s;
        o.pad.negated = !o.pad.negated;
        define(n.outputs[0], o);
        return;
      }
    }
    if (op == "Mul" && n.inputs.size() == 2)  // m * c, c <= -1e4: the additive form
      for (int side = 0; side < 2; ++side) {
        const Val* s = val_if(n.in(side), Val::KEYVIS);
        float c = 0.f;
        if (!s || s->kv_add || !scalar_init(n.in(1 - side), c)) continue;
        if (!(c <= -1e4f))
          throw std::runtime_error(who + "a key mask times " + std::to_string(c) + " is not a mask (only factors <= -1e4 "
                                   "fold into the attention kernel as -inf)");
        Val o = *s;
        o.kv_add = true;
        define(n.outputs[0], o);
        return;
      }
    throw std::runtime_error(who + "token ids feed only a Cast to INT64 / INT32, an embedding Gather (axis 0) and the pad "
                             "tests Equal / Greater / Less, and a key mask derived from them only Not, Cast, Unsqueeze / "
                             "Reshape to [N, 1, 1, S], Sub(1, m), Mul(m, c <= -1e4), the Where / Add on attention scores and "
                             "the masked mean over the tokens (Unsqueeze(-1), Expand to [N, S, D], Mul(rows, m), "
                             "ReduceSum(m, axis 1)); other uses are out of scope");
  }

  // Gather(table [V, D] float initializer, ids, axis 0) [+ Add(positions [S, D] / [1, S, D])]
  // [+ Add(token-type row [D] / [1, 1, D])] -> one EMBED_TOKENS op producing rows [N, S, D].
  void lower_embed(int idx) {
    const Node& n = m_.nodes[idx];
    const Val ids = val(n.in(1), n);
    if (n.get_int("axis", 0) != 0)
      throw std::runtime_error("Gather " + n.name + ": token ids index only axis 0 of an embedding table");
    auto it = m_.initializers.find(n.in(0));
    if (it == m_.initializers.end())
      throw std::runtime_error("Gather " + n.name + ": the embedding table " + n.in(0) + " must be an initializer");
    const onnx::Tensor& t = it->second;
    if (t.dims.size() != 2 || !onnx::is_float_type(t.dtype) || static_cast<int64_t>(t.f.size()) != t.numel() || t.numel() == 0)
      throw std::runtime_error("Gather " + n.name + ": the embedding table must be a float [V, D] initializer");
    const int V = static_cast<int>(t.dims[0]), D = static_cast<int>(t.dims[1]), S = ids.H, Dp = round8(D);
    auto padded = [&](const std::vector<float>& f, int rows) {  // [rows][D] -> [rows][Dp], pad columns 0
      std::vector<float> o(static_cast<size_t>(rows) * Dp, 0.f);
      for (int r = 0; r < rows; ++r)
        std::copy_n(f.begin() + static_cast<size_t>(r) * D, D, o.begin() + static_cast<size_t>(r) * Dp);
      return o;
    };
    PlanOp p;
    p.kind = PlanOp::EMBED_TOKENS;
    p.name = n.name;
    p.in = kBufGraphIn;
    p.S = S;
    p.gidx = V;
    p.C = Dp;
    p.Cp = D;
    p.w_off = push_f32(padded(t.f, V));
    const bool multi = m_.inputs.size() > 1;
    if (multi) {
      p.in_ld = static_cast<int>(plan_.input_numel);
      p.seg_ids = ids.seg;
    }
    // the position Add, then the token-type Add, each the value's only reader.  With several graph
    // inputs the Adds come in any order, and the type term is the lookup of another input in its own
    // table (a sibling Gather read by that Add alone), which joins this op.
    std::string out = n.outputs[0];
    for (int step = 0; step < 2; ++step) {
      const int ci = sole_consumer(out);
      if (ci < 0 || m_.nodes[ci].op_type != "Add" || m_.nodes[ci].inputs.size() != 2) break;
      const Node& a = m_.nodes[ci];
      const std::string& cn = a.in(0) == out ? a.in(1) : a.in(0);
      auto ct = m_.initializers.find(cn);
      if (ct == m_.initializers.end()) {
        auto pg = producer_.find(cn);
        if (!multi || pg == producer_.end() || done_[pg->second] || p.bias_off != SIZE_MAX || p.seg_types >= 0) break;
        const Node& g2 = m_.nodes[pg->second];
        const Val* ids2 = g2.op_type == "Gather" && g2.inputs.size() == 2 && g2.get_int("axis", 0) == 0 ? ids_behind(g2.in(1)) : nullptr;
        auto t2 = m_.initializers.find(g2.in(0));
        if (!ids2 || ids2->in_idx == ids.in_idx || t2 == m_.initializers.end() || consumers(cn).size() != 1 ||
            graph_outputs_.count(cn))
          break;
        const onnx::Tensor& tt = t2->second;
        if (tt.dims.size() != 2 || tt.dims[1] != D || !onnx::is_float_type(tt.dtype) ||
            static_cast<int64_t>(tt.f.size()) != tt.numel() || tt.numel() == 0)
          break;
        p.seg_types = ids2->seg;
        p.type_rows = static_cast<int>(tt.dims[0]);
        p.type_off = push_f32(padded(tt.f, p.type_rows));
        if (ids2->in_idx < ids.in_idx) {  // the earlier-declared input is the ids: swap the two lookups
          std::swap(p.seg_ids, p.seg_types);
          std::swap(p.w_off, p.type_off);
          std::swap(p.gidx, p.type_rows);
        }
        done_[pg->second] = true;
        done_[ci] = true;
        out = a.outputs[0];
        continue;
      }
      if (!onnx::is_float_type(ct->second.dtype)) break;
      const auto& d = ct->second.dims;
      const bool is_pos = (d.size() == 2 && d[0] == S && d[1] == D) || (d.size() == 3 && d[0] == 1 && d[1] == S && d[2] == D);
      const bool is_type = (d.size() == 1 && d[0] == D) || (d.size() == 3 && d[0] == 1 && d[1] == 1 && d[2] == D);
      if ((step == 0 || multi) && is_pos && p.shift_off == SIZE_MAX) p.shift_off = push_f32(padded(ct->second.f, S));
      else if (is_type && p.bias_off == SIZE_MAX && p.seg_types < 0) p.bias_off = push_f32(padded(ct->second.f, 1));
      else break;
      done_[ci] = true;
      out = a.outputs[0];
    }
    p.out = new_buf(static_cast<size_t>(S) * Dp * 2);
    Val o;
    o.kind = Val::ROWS_BF16;
    o.C = Dp;
    o.cl = Dp != D ? D : 0;
    o.H = S;
    o.rank = 3;
    o.buf = p.out;
    define(out, o);
    if (key_op_ < 0) key_op_ = static_cast<int>(plan_.ops.size());
    add_op(std::move(p));
  }

  // scores x with the key mask m: visible where m's value is true (vis_when_true) or false.
  void define_key_masked(const Node& n, const Val& x, const Val& m, bool vis_when_true) {
    const std::string who = n.op_type + " " + n.name + ": ";
    if (m.kv_rank != 4)
      throw std::runtime_error(who + "a key mask on attention scores must have the shape [N, 1, 1, S] (rank " +
                               std::to_string(m.kv_rank) + " here)");
    if (m.H != vals_[x.q].H) throw std::runtime_error(who + "the key mask's length is not the attention's");
    bind_key_test(who, m, vis_when_true);
    Val o = x;
    o.kmask = true;
    define(n.outputs[0], o);
  }

  // The model's one pad test, on the EMBED_TOKENS op that writes the key data (kvis, kend) for it:
  // set by the first user (an attention or the token pooling), compared by every later one.
  void bind_key_test(const std::string& who, const Val& m, bool vis_when_true) {
    if (key_op_ < 0)
      throw std::runtime_error(who + "a key mask needs the token embedding (EMBED_TOKENS writes the key data) lowered first");
    PadTest visible = m.pad;  // m's value is true where m.pad holds
    visible.negated = m.pad.negated != !vis_when_true;
    PlanOp& e = plan_.ops[key_op_];
    if (!key_test_set_) {
      key_test_set_ = true;
      e.pad = visible;
      const int Sp = kern::key_pitch(m.H);
      e.out2 = new_buf(static_cast<size_t>(Sp) * 4);  // kvis: fp32 [Sp] per sample
      e.out3 = new_buf(16);                           // kend: one int per sample
      plan_.bufs[e.out2].bytes_per_sample = static_cast<size_t>(Sp) * 4;  // (fp32 in both precisions)
      plan_.bufs[e.out3].bytes_per_sample = 4;
    } else if (!(e.pad == visible)) {
      throw std::runtime_error(who + "a second, different pad test (one key mask per model: every attention shares the key data)");
    }
  }

  // ---- sentence embedders: masked mean over the tokens and L2 normalisation -------------------------
  // vis [N, S] -> Unsqueeze(-1) [-> Expand to [N, S, D]] -> Cast = m;  Mul(rows, m) -> ReduceSum(axis 1)
  // = the masked sum;  ReduceSum(m, axis 1) (or of the unexpanded [N, S] mask, keepdims 1)
  // [-> Clip(min = c) / Max(., c)] = the count;  Div(sum, count) closes the pattern: one POOL_TOKENS op
  // reading the key data of the plan's EMBED_TOKENS op.  An L2 normalisation that is the pooled
  // vector's only reader sets the op's normalize flag; on any other rank-2 rows it is a POOL_TOKENS op
  // with S = 1.

  // `name` is written by ReduceSum(Mul(., .)): the shape of a masked sum (whether the Mul has a key
  // mask operand is that Mul's business)
  bool masked_sum_shape(const std::string& name) const {
    auto r = producer_.find(name);
    if (r == producer_.end() || m_.nodes[r->second].op_type != "ReduceSum" || m_.nodes[r->second].inputs.empty()) return false;
    auto q = producer_.find(m_.nodes[r->second].in(0));
    return q != producer_.end() && m_.nodes[q->second].op_type == "Mul";
  }

  bool lower_pool_node(int idx) {
    const Node& n = m_.nodes[idx];
    const std::string& op = n.op_type;
    const std::string who = op + " " + n.name + ": ";
    auto fail = [&](const std::string& why) { throw std::runtime_error(who + why); };
    const Val* m = n.inputs.empty() ? nullptr : val_if(n.in(0), Val::KEYVIS);
    if (m && op == "Unsqueeze" && m->kv_rank == 2 && !m->kv_add) {  // [N, S] -> [N, S, 1]
      std::vector<int64_t> axes;
      node_axes(n, axes);
      if (axes.size() != 1 || !(axes[0] == -1 || axes[0] == 2)) return false;  // towards [N, 1, 1, S]: lower_token_node
      Val o = *m;
      o.kv_rank = 3;
      o.kv_last = true;
      define(n.outputs[0], o);
      return true;
    }
    if (m && m->kv_last && (op == "Unsqueeze" || op == "Reshape" || op == "Sub"))
      fail("a key mask [N, S, 1] goes only through Expand to [N, S, D], Cast and Not (masked mean pooling)");
    if (m && m->kv_last && op == "Expand") {
      std::vector<int64_t> shp;
      const bool ok = n.inputs.size() == 2 && ints_of(n.in(1), shp) && shp.size() == 3 && (shp[0] == 1 || shp[0] == kBatchDim) &&
                      (shp[1] == 1 || shp[1] == m->H) && shp[2] >= 1 && !m->kv_D;
      if (!ok) fail("a key mask [N, S, 1] expands only to [N, S, D]");
      Val o = *m;
      o.kv_D = static_cast<int>(shp[2]);
      define(n.outputs[0], o);
      return true;
    }
    if (op == "Mul" && n.inputs.size() == 2)  // rows x mask
      for (int side = 0; side < 2; ++side) {
        const Val* s = val_if(n.in(side), Val::KEYVIS);
        const Val* x = val_if(n.in(1 - side), Val::ROWS_BF16);
        if (!s || !x) continue;
        if (s->kv_add || !s->kv_last || x->rank != 3)
          fail("rows [N, S, D] are multiplied only by a key mask of the shape [N, S, 1] or [N, S, D] (masked mean pooling)");
        if (!dense(*x)) fail("the masked rows must be dense");
        const int S = x->H * x->W;
        if (s->H != S)
          fail("the key mask's length " + std::to_string(s->H) + " is not the rows' " + std::to_string(S));
        if (s->kv_D && s->kv_D != x->logical() && s->kv_D != x->C) fail("the expanded key mask's width is not the rows'");
        const int r = sole_consumer(n.outputs[0]);
        std::vector<int64_t> ax;
        if (r < 0 || m_.nodes[r].op_type != "ReduceSum" || !node_axes(m_.nodes[r], ax) || ax.size() != 1 ||
            !(ax[0] == 1 || ax[0] == -2) || m_.nodes[r].get_int("keepdims", 1) != 0)
          fail("rows times a key mask feed only ReduceSum(axis 1, keepdims 0), the masked sum over the tokens");
        Val o = *s;
        o.kind = Val::POOLV;
        o.stage = 0;
        o.buf = x->buf;
        o.C = x->C;
        o.cl = x->cl;
        o.H = S;
        define(n.outputs[0], o);
        return true;
      }
    if (op == "ReduceSum" && !n.inputs.empty()) {
      std::vector<int64_t> ax;
      node_axes(n, ax);
      const bool keep = n.get_int("keepdims", 1) != 0;
      if (const Val* r = val_if(n.in(0), Val::POOLV)) {  // the masked sum (axes checked by the Mul)
        if (r->stage != 0) fail("only rows times a key mask are summed over the tokens");
        const int d = sole_consumer(n.outputs[0]);
        if (d < 0 || m_.nodes[d].op_type != "Div" || m_.nodes[d].inputs.size() != 2 || m_.nodes[d].in(0) != n.outputs[0] ||
            m_.nodes[d].in(1) == n.outputs[0])
          fail("a masked sum over the tokens must be divided by the count of visible tokens (masked mean pooling; sum "
               "pooling is out of scope)");
        Val o = *r;
        o.stage = 1;
        define(n.outputs[0], o);
        return true;
      }
      if (m) {  // the count of visible tokens
        const bool form = !m->kv_add && ax.size() == 1 &&
                          (m->kv_last ? (ax[0] == 1 || ax[0] == -2) && !keep : m->kv_rank == 2 && (ax[0] == 1 || ax[0] == -1) && keep);
        if (!form)
          fail("a key mask is summed only over the token axis, to the count of visible tokens [N, D] or [N, 1] (masked "
               "mean pooling)");
        std::string cur = n.outputs[0];
        for (bool closed = false; !closed;) {
          const int c = sole_consumer(cur);
          const Node* q = c >= 0 ? &m_.nodes[c] : nullptr;
          if (q && q->inputs.size() >= 1 && (q->op_type == "Clip" || q->op_type == "Max") &&
              (q->in(0) == cur || (q->op_type == "Max" && q->inputs.size() == 2 && q->in(1) == cur)))
            cur = q->outputs[0];  // its bounds are that node's business
          else if (q && q->op_type == "Div" && q->inputs.size() == 2 && q->in(1) == cur && masked_sum_shape(q->in(0)))
            closed = true;
          else
            fail("the count of a key mask's visible tokens must end, through Clip(min) / Max, as the divisor of the masked "
                 "sum Mul(rows, mask) -> ReduceSum(axis 1) (masked mean pooling); other uses of a key mask are out of scope");
        }
        Val o = *m;
        o.kind = Val::POOLV;
        o.stage = 2;
        o.pool_c = 0.f;
        define(n.outputs[0], o);
        return true;
      }
    }
    if (op == "Clip" || op == "Max") {  // lower bound of the count
      const Val* c = n.inputs.empty() ? nullptr : val_if(n.in(0), Val::POOLV);
      int side = 0;
      if (!c && op == "Max" && n.inputs.size() == 2 && (c = val_if(n.in(1), Val::POOLV))) side = 1;
      if (c) {
        if (c->stage != 2) fail("only the count of visible tokens is clipped (masked mean pooling)");
        float lo = 0.f, hi = 3.4e38f;
        if (op == "Clip") {
          if (!clip_bounds(n, lo, hi)) fail("bounds must be constants");
          if (hi < 3.4e38f) fail("a Clip with a max on the count of visible tokens is not supported (only a lower bound)");
          if (lo == -3.4e38f) lo = 0.f;
        } else if (n.inputs.size() != 2 || !scalar_init(n.in(1 - side), lo)) {
          fail("the count of visible tokens is bounded only by a scalar initializer");
        }
        if (!(lo >= 0.f)) fail("the lower bound of the count of visible tokens must be >= 0");
        Val o = *c;
        o.pool_c = std::max(c->pool_c, lo);
        define(n.outputs[0], o);
        return true;
      }
    }
    if (op == "Div" && n.inputs.size() == 2) {
      const Val* a = val_if(n.in(0), Val::POOLV);
      const Val* b = val_if(n.in(1), Val::POOLV);
      if (a || b) {
        if (!a || !b || a->stage != 1 || b->stage != 2)
          fail("masked mean pooling divides the masked sum over the tokens by the count of visible tokens, nothing else");
        if (!(a->pad == b->pad))
          fail("the count is not over the visibility value of the masked sum (different pad tests)");
        if (b->kv_D && b->kv_D != a->logical() && b->kv_D != a->C) fail("the count's width is not the masked sum's");
        const Val rows = *a, vis = *a;
        emit_pool_tokens(n, rows, rows.H, &vis, b->pool_c, n.outputs[0], true, false, 0.f);
        return true;
      }
    }
    for (const auto& in : n.inputs)
      if (val_if(in, Val::POOLV))
        fail("a masked sum / count of visible tokens feeds only Clip(min) / Max and the Div that closes the masked mean");
    return false;
  }

  // ReduceL2(x, last axis, keepdims 1) [-> Clip(min = eps) | Max(., eps)] [-> Expand] -> Div(x, .), from
  // the ReduceL2 node: torch's export of F.normalize.  False with a reason when it is something else.
  // The Expand's shape is constant or Shape(x); used lists the chain's nodes, the Div last, and
  // shape_node that Shape (-1: none).
  bool l2_chain(int ridx, int rank, float& eps, std::string& out, std::vector<int>& used, std::string& why,
                int& shape_node) const {
    const Node& r = m_.nodes[ridx];
    const std::string& x = r.in(0);
    std::vector<int64_t> ax;
    if (!node_axes(r, ax) || ax.size() != 1 || !(ax[0] == -1 || ax[0] == rank - 1) || r.get_int("keepdims", 1) != 1) {
      why = "the norm is taken over the last axis with keepdims 1";
      return false;
    }
    used = {ridx};
    eps = 0.f;
    shape_node = -1;
    std::string cur = r.outputs[0];
    int c = sole_consumer(cur);
    if (c >= 0 && (m_.nodes[c].op_type == "Clip" || m_.nodes[c].op_type == "Max")) {
      const Node& q = m_.nodes[c];
      float lo = 0.f, hi = 3.4e38f;
      if (q.op_type == "Clip") {
        if (q.in(0) != cur || !clip_bounds(q, lo, hi) || hi < 3.4e38f) {
          why = "Clip " + q.name + ": only a constant min (a Clip with a max is not supported)";
          return false;
        }
        if (lo == -3.4e38f) lo = 0.f;
      } else if (q.inputs.size() != 2 || !scalar_init(other_input(q, cur), lo)) {
        why = "Max " + q.name + ": only with a scalar initializer";
        return false;
      }
      if (!(lo >= 0.f)) {
        why = q.op_type + " " + q.name + ": the lower bound of a norm must be >= 0";
        return false;
      }
      eps = lo;
      used.push_back(c);
      cur = q.outputs[0];
      c = sole_consumer(cur);
    }
    if (c >= 0 && m_.nodes[c].op_type == "Expand" && m_.nodes[c].in(0) == cur) {
      std::vector<int64_t> shp;
      const auto sp = m_.nodes[c].inputs.size() == 2 ? producer_.find(m_.nodes[c].in(1)) : producer_.end();
      if (sp != producer_.end() && m_.nodes[sp->second].op_type == "Shape" && m_.nodes[sp->second].in(0) == x &&
          consumers(m_.nodes[sp->second].outputs[0]).size() == 1) {
        shape_node = sp->second;
      } else if (m_.nodes[c].inputs.size() != 2 || !ints_of(m_.nodes[c].in(1), shp) || static_cast<int>(shp.size()) != rank) {
        why = "Expand " + m_.nodes[c].name + ": the norm expands only to the rows' shape";
        return false;
      }
      used.push_back(c);
      cur = m_.nodes[c].outputs[0];
      c = sole_consumer(cur);
    }
    if (c < 0 || m_.nodes[c].op_type != "Div" || m_.nodes[c].inputs.size() != 2 || m_.nodes[c].in(0) != x ||
        m_.nodes[c].in(1) != cur) {
      why = "the norm's only reader must be Div(x, norm)";
      return false;
    }
    used.push_back(c);
    out = m_.nodes[c].outputs[0];
    return true;
  }

  // Every reader of the rank-2 value `x` belongs to one L2 normalisation over its last axis.
  bool only_l2_normalized(const std::string& x, float& eps, std::string& out, std::vector<int>& used) const {
    if (graph_outputs_.count(x)) return false;
    const std::vector<int> cs = consumers(x);
    if (cs.size() == 1 && m_.nodes[cs[0]].op_type == "LpNormalization" && !done_[cs[0]]) {
      const Node& l = m_.nodes[cs[0]];
      const int64_t axis = l.get_int("axis", -1);
      if (l.get_int("p", 2) != 2 || !(axis == -1 || axis == 1)) return false;  // rejected at that node
      eps = 0.f;
      out = l.outputs[0];
      used = {cs[0]};
      return true;
    }
    for (int r : cs) {
      std::string why;
      int shape_node = -1;
      if (m_.nodes[r].op_type != "ReduceL2" || done_[r] || !l2_chain(r, 2, eps, out, used, why, shape_node)) continue;
      for (int c : cs)  // x's readers: the ReduceL2, the Div and the Shape for the Expand
        if (c != r && c != used.back() && c != shape_node) return false;
      if (shape_node >= 0 && !done_[shape_node]) used.push_back(shape_node);
      return true;
    }
    return false;
  }

  // LpNormalization / ReduceL2 on rows that are not a pooled vector's only use: POOL_TOKENS with S = 1.
  void lower_l2norm(int idx) {
    const Node& n = m_.nodes[idx];
    const std::string who = n.op_type + " " + n.name + ": ";
    const Val x = val(n.in(0), n);
    const int rank = x.rank ? x.rank : 2;
    float eps = 0.f;
    std::string out = n.outputs[0];
    std::vector<int> used;
    if (n.op_type == "LpNormalization") {
      const int64_t axis = n.get_int("axis", -1);
      if (n.get_int("p", 2) != 2) throw std::runtime_error(who + "only p = 2 (L2 normalisation) is supported");
      if (!(axis == -1 || axis == rank - 1)) throw std::runtime_error(who + "only the last axis is normalised");
    } else {
      std::string why;
      int shape_node = -1;
      if (!l2_chain(idx, rank, eps, out, used, why, shape_node))
        throw std::runtime_error(who + "only torch's export of F.normalize, ReduceL2(last axis, keepdims 1) -> Clip(min = eps) "
                                 "-> [Expand] -> Div(x, .), is supported (" + why + ")");
    }
    if (x.kind != Val::ROWS_BF16 || rank != 2 || x.H * x.W != 1 || !dense(x))
      throw std::runtime_error(who + "only dense rank-2 rows [N, D] are L2-normalised");
    for (int u : used) done_[u] = true;
    emit_pool_tokens(n, x, 1, nullptr, 0.f, out, false, true, eps);
  }

  // One POOL_TOKENS op over the rows x ([S][C] per sample); vis: the key mask of a masked mean (nullptr:
  // all S rows).  try_norm: an L2 normalisation that is the result's only reader joins the op.
  void emit_pool_tokens(const Node& n, const Val& x, int S, const Val* vis, float clip_min, std::string out_name,
                        bool try_norm, bool normalize, float eps) {
    PlanOp p;
    p.kind = PlanOp::POOL_TOKENS;
    p.name = n.name;
    p.in = x.buf;
    p.S = S;
    p.C = x.C;
    p.Cp = x.logical();
    p.count_min = clip_min;
    if (vis) {
      bind_key_test(n.op_type + " " + n.name + ": ", *vis, true);  // the mask multiplies: true = visible
      p.key_mask = 1;
      p.in4 = plan_.ops[key_op_].out2;
      p.in5 = plan_.ops[key_op_].out3;
    }
    std::vector<int> used;
    std::string nout;
    if (try_norm && only_l2_normalized(out_name, eps, nout, used)) {
      normalize = true;
      for (int u : used) done_[u] = true;
      p.name += "+" + m_.nodes[used[0]].name;
      out_name = nout;
    }
    p.normalize = normalize;
    p.eps = normalize ? eps : 0.f;
    p.flops_per_sample = static_cast<double>(S) * p.Cp;
    Val o;
    o.kind = Val::ROWS_BF16;
    o.C = x.C;
    o.cl = x.cl;
    o.rank = 2;
    if (graph_outputs_.count(out_name) && consumers(out_name).empty()) {  // fp32 straight to the output
      p.out_f32 = kBufGraphOut;
      o.kind = Val::ROWS_F32;
      o.buf = kBufGraphOut;
    } else {
      p.out = new_buf(static_cast<size_t>(x.C) * 2);
      o.buf = p.out;
    }
    define(out_name, o);
    add_op(std::move(p));
  }

  // ---- attention bias / mask folding --------------------------------------------------------------
  // Between Q K^T and the Softmax a chain may hold, besides the scalar Div / Mul, any number of
  // Add(scores, B) and Where(C, scores, f) nodes with B / C initializers broadcastable to
  // [1, nh, S, S].  They fold at plan time into one dense additive table per attention, in the
  // softmax's natural units: scores' = scale * (Q K^T) + table.  A later scale multiplies the table
  // too, several Adds sum, a Where puts -inf at its masked positions.  emit_attention classifies
  // the table (causal flag, shared / per-head, nothing left) and stores it.
  struct AttnTable {
    int heads = 1;         // 1 (shared) or nh
    std::vector<float> t;  // [heads][S][S]
  };
  std::vector<AttnTable> masks_;  // indexed by Val::mask (a Val is copied by value everywhere)

  // Add / Where with an attention-scores operand (stage 0)
  bool attn_mask_node(const Node& n) const {
    if (n.op_type != "Add" && n.op_type != "Where") return false;
    for (const auto& in : n.inputs) {
      auto it = vid_.find(in);
      if (it != vid_.end() && vals_[it->second].kind == Val::ATTN && vals_[it->second].stage == 0) return true;
    }
    return false;
  }

  // The table of scores value x with room for `heads` slices (zeros when x has none yet).
  AttnTable attn_table(const Val& x, int heads) const {
    const size_t SS = static_cast<size_t>(vals_[x.q].H) * vals_[x.q].H;
    AttnTable t;
    if (x.mask >= 0) t = masks_[x.mask];
    else t.t.assign(SS, 0.f);
    if (t.heads < heads) {
      t.t.resize(SS * heads);
      for (int h = 1; h < heads; ++h) std::copy(t.t.begin(), t.t.begin() + SS, t.t.begin() + h * SS);
      t.heads = heads;
    }
    return t;
  }

  // Checks a folded table and defines `out` = x with it.  +inf / NaN entries (a -inf entry scaled
  // by a non-positive constant, inf - inf) have no meaning as a mask; a query row without any
  // finite entry has an all-zero softmax denominator (NaN in ONNX, undefined on the device).
  void define_masked(const Node& n, const Val& x, AttnTable t) {
    const int S = vals_[x.q].H;
    for (int h = 0; h < t.heads; ++h)
      for (int i = 0; i < S; ++i) {
        const float* row = t.t.data() + (static_cast<size_t>(h) * S + i) * S;
        bool visible = false;
        for (int j = 0; j < S; ++j) {
          if (std::isnan(row[j]) || row[j] == INFINITY)
            throw std::runtime_error(n.op_type + " " + n.name + ": the folded attention bias has a NaN / +inf entry (a mask "
                                     "scaled by a constant that is not positive?)");
          visible = visible || std::isfinite(row[j]);
        }
        if (!visible)
          throw std::runtime_error(n.op_type + " " + n.name + ": attention mask leaves query row " + std::to_string(i) +
                                   (t.heads > 1 ? " of head " + std::to_string(h) : std::string()) +
                                   " with no visible key (its softmax is NaN in ONNX; the device kernel does not define it)");
      }
    Val o = x;
    o.mask = static_cast<int>(masks_.size());
    masks_.push_back(std::move(t));
    define(n.outputs[0], o);
  }

  // Add(scores, B) / Where(C, scores, f) / Where(C, f, scores) on attention scores x.
  // mode 0: add the float tensor; 1: -inf where the bool tensor is false; 2: -inf where it is true.
  void lower_attn_mask(const Node& n, const Val& x, const std::string& tname, int mode) {
    const char* what = mode == 0 ? "bias" : "mask";
    auto it = m_.initializers.find(tname);
    if (it == m_.initializers.end())
      throw std::runtime_error(n.op_type + " " + n.name + ": the attention " + what + " " + tname +
                               " must be an initializer, or a key mask derived from the token ids (see the report line of "
                               "the node producing it); other masks that depend on the input, and folding a mask the "
                               "exporter left as a Slice / Cast / ... subgraph of constants, are out of scope");
    const onnx::Tensor& c = it->second;
    const int S = vals_[x.q].H, nh = vals_[x.q].nh;
    const size_t r = c.dims.size();
    const bool typed = mode == 0 ? onnx::is_float_type(c.dtype) && static_cast<int64_t>(c.f.size()) == c.numel()
                                 : c.dtype == onnx::BOOL && static_cast<int64_t>(c.i.size()) == c.numel();
    if (!typed)
      throw std::runtime_error(n.op_type + " " + n.name + ": the attention " + what + " " + tname + " must be a " +
                               (mode == 0 ? "float" : "bool") + " tensor");
    // right-aligned against [1, nh, S, S]: rank 2..4, leading dims 1 or nh, last two (S, S), (1, S) or (S, 1)
    const int64_t dc = r >= 1 ? c.dims[r - 1] : 0, dr = r >= 2 ? c.dims[r - 2] : 0, dh = r >= 3 ? c.dims[r - 3] : 1,
                  db = r >= 4 ? c.dims[0] : 1;
    const bool rows_ok = (dr == S && dc == S) || (dr == 1 && dc == S) || (dr == S && dc == 1);
    if (r < 2 || r > 4 || db != 1 || (dh != 1 && dh != nh) || !rows_ok) {
      std::string shape;
      for (auto d : c.dims) shape += (shape.empty() ? "" : ", ") + std::to_string(d);
      throw std::runtime_error(n.op_type + " " + n.name + ": attention " + what + " " + tname + " [" + shape +
                               "] does not broadcast to [1, " + std::to_string(nh) + ", " + std::to_string(S) + ", " +
                               std::to_string(S) + "] (rank 2 to 4, leading dims 1 or the head count, last two dims (S, S), (1, S) or (S, 1))");
    }
    AttnTable t = attn_table(x, static_cast<int>(dh));
    for (int h = 0; h < t.heads; ++h)
      for (int i = 0; i < S; ++i)
        for (int j = 0; j < S; ++j) {
          const size_t src = ((dh == 1 ? 0 : static_cast<size_t>(h)) * dr + (dr == 1 ? 0 : i)) * dc + (dc == 1 ? 0 : j);
          float& e = t.t[(static_cast<size_t>(h) * S + i) * S + j];
          if (mode == 0) e += c.f[src];
          else if ((c.i[src] != 0) == (mode == 2)) e = -INFINITY;
        }
    define_masked(n, x, std::move(t));
  }

  // Materialise an attention context (logical [B, S, nh, hd]) as rows [B, S, nh*hd].
  int emit_attention(const Val& ctx, const std::string& name) {
    const Val& q = vals_[ctx.q];
    const Val& k = vals_[ctx.k];
    const Val& v = vals_[ctx.v];
    const int S = q.H, C = q.nh * q.hd;
    if (!kern::attention_supported(q.hd, S) || k.H != S || v.H != S)
      throw std::runtime_error("attention " + name + ": needs head dim 32, 64, 80, 96 or 128 (64 and <= 256 tokens " +
                               "without the streaming kernel)");
    if ((ctx.mask >= 0 || ctx.kmask) && !kern::attention_supported(q.hd, S, true))
      throw std::runtime_error("attention " + name + ": a bias / mask on the scores needs the streaming attention kernel, "
                               "which this build leaves out");
    PlanOp p;
    p.kind = PlanOp::ATTENTION;
    p.name = name;
    p.in = q.buf;
    p.in2 = k.buf;
    p.in3 = v.buf;
    p.col[0] = q.col;
    p.col[1] = k.col;
    p.col[2] = v.col;
    p.ld[0] = q.pitch();
    p.ld[1] = k.pitch();
    p.ld[2] = v.pitch();
    p.S = S;
    p.nh = q.nh;
    p.hd = q.hd;
    p.fscale = ctx.scale;
    p.C = C;
    p.flops_per_sample = 4.0 * S * S * q.hd * q.nh;
    if (ctx.mask >= 0) {
      AttnTable t = masks_[ctx.mask];
      const size_t SS = static_cast<size_t>(S) * S;
      // a strict upper triangle of -inf in every head is the causal flag (the kernel masks from
      // indices and skips the tiles); what remains of the table is its lower triangle
      bool causal = S > 1;
      for (int h = 0; h < t.heads && causal; ++h)
        for (int i = 0; i < S && causal; ++i)
          for (int j = i + 1; j < S; ++j)
            if (t.t[h * SS + static_cast<size_t>(i) * S + j] != -INFINITY) {
              causal = false;
              break;
            }
      if (causal)
        for (int h = 0; h < t.heads; ++h)
          for (int i = 0; i < S; ++i)
            for (int j = i + 1; j < S; ++j) t.t[h * SS + static_cast<size_t>(i) * S + j] = 0.f;
      bool same = true;  // all heads equal: one shared slice
      for (int h = 1; h < t.heads && same; ++h) same = std::equal(t.t.begin(), t.t.begin() + SS, t.t.begin() + h * SS);
      if (same) {
        t.heads = 1;
        t.t.resize(SS);
      }
      const bool zero = std::all_of(t.t.begin(), t.t.end(), [](float e) { return e == 0.f; });
      if (!zero) {  // [heads][S][Sp], rows padded to a multiple of 32, in the kernel's exp2 units
        const int Sp = kern::key_pitch(S);
        std::vector<float> tab(static_cast<size_t>(t.heads) * S * Sp, 0.f);
        for (size_t row = 0; row < static_cast<size_t>(t.heads) * S; ++row)
          for (int j = 0; j < S; ++j) tab[row * Sp + j] = t.t[row * S + j] * 1.4426950408889634f;
        p.bias_off = push_f32(tab);
        p.bias_heads = t.heads;
      }
      p.causal = causal ? 1 : 0;
      if (causal) p.flops_per_sample = 4.0 * q.hd * q.nh * (static_cast<double>(S) * (S + 1) / 2);
    }
    if (ctx.kmask) {  // the request's key mask: the key data the first EMBED_TOKENS op writes
      if (p.causal)
        throw std::runtime_error("attention " + name + ": a key (padding) mask together with a causal mask is not "
                                 "supported (a left-padded causal row has no visible key)");
      p.key_mask = 1;
      p.in4 = plan_.ops[key_op_].out2;
      p.in5 = plan_.ops[key_op_].out3;
    }
    // grouped-query attention: K / V store nh / G heads (their views carry the group size)
    const int kg = std::max(1, k.kvg);
    p.kv_heads = q.nh / kg;
    if (kg > 1) {
      if (q.hd != 64 && q.hd != 128)
        throw std::runtime_error("attention " + name + ": grouped-query attention (" + std::to_string(q.nh) + " heads over " +
                                 std::to_string(p.kv_heads) + " K/V heads) needs head dim 64 or 128, not " + std::to_string(q.hd));
      if (p.bias_heads)
        throw std::runtime_error("attention " + name + ": grouped-query attention with a bias table on the scores is not "
                                 "supported (unmasked, causal or the request's key mask only)");
      if (q.col % 8 || k.col % 8 || v.col % 8 || (p.kv_heads * q.hd) % 8)
        throw std::runtime_error("attention " + name + ": grouped-query attention needs Q / K / V column offsets and the "
                                 "K/V width in multiples of 8");
    }
    p.out = new_buf(static_cast<size_t>(S) * C * 2);
    const int buf = p.out;
    add_op(std::move(p));
    return buf;
  }

  void lower_reshape(int idx) {
    const Node& n = m_.nodes[idx];
    const Val x = val(n.in(0), n);
    std::vector<int64_t> shp;
    if (!ints_of(n.in(1), shp)) throw std::runtime_error("Reshape " + n.name + ": target shape must be static");
    for (auto& d : shp)
      if (d == kBatchDim) d = 0;
    auto is_batch = [](int64_t d) { return d == 0 || d == -1; };
    // NHWC map -> [B, C, H*W]
    if (x.kind == Val::NHWC && shp.size() == 3 && is_batch(shp[0]) && shp[1] == x.C &&
        (shp[2] == -1 || shp[2] == static_cast<int64_t>(x.H) * x.W) && x.H * x.W > 1) {
      Val o = x;
      o.kind = Val::NCHW_FLAT;
      define(n.outputs[0], o);
      return;
    }
    // rows [B, S, C] -> heads [B, S, nh, hd]
    if (x.kind == Val::ROWS_BF16 && shp.size() == 4 && is_batch(shp[0]) &&
        (shp[1] == 0 || shp[1] == -1 || shp[1] == x.H * x.W)) {
      const int64_t nh = shp[2], hd = shp[3];
      if (nh > 0 && hd > 0 && nh * hd == x.C) {
        Val o = x;
        o.kind = Val::HEADS;
        o.H = x.H * x.W;
        o.W = 1;
        o.nh = static_cast<int>(nh);
        o.hd = static_cast<int>(hd);
        o.perm = {{0, 1, 2, 3}};
        define(n.outputs[0], o);
        return;
      }
    }
    // attention context [B, S, nh, hd] -> rows [B, S, nh*hd]
    if (x.kind == Val::ATTN && x.stage == 2 && x.perm == std::array<int, 4>{{0, 1, 2, 3}} && shp.size() == 3 &&
        is_batch(shp[0])) {
      const Val& q = vals_[x.q];
      Val o;
      o.kind = Val::ROWS_BF16;
      o.C = q.nh * q.hd;
      o.H = q.H;
      o.rank = 3;
      o.buf = emit_attention(x, n.name);
      define(n.outputs[0], o);
      return;
    }
    // NHWC map -> [B, C*H*W] (NCHW order): the flatten view
    if (x.kind == Val::NHWC && x.H * x.W > 1 && shp.size() == 2 && is_batch(shp[0]) &&
        (shp[1] == -1 || shp[1] == static_cast<int64_t>(x.logical()) * x.H * x.W)) {
      define(n.outputs[0], flatten_nhwc(x));
      return;
    }
    // dense rows [B, S*D] <-> [B, S, D] (same memory): rank-2 <-> rank-3 views
    if (x.kind == Val::ROWS_BF16 && !x.padded() && !x.flat_hw && x.pitch() == x.C && !x.col) {
      const int64_t total = static_cast<int64_t>(x.H) * x.W * x.C;
      if (shp.size() == 3 && is_batch(shp[0])) {
        int64_t S = shp[1], D = shp[2];
        if (S == -1 && D > 0) S = total / D;
        if (D == -1 && S > 0) D = total / S;
        if (S > 0 && D > 0 && S * D == total && D % 8 == 0) {
          Val o = x;
          o.H = static_cast<int>(S);
          o.W = 1;
          o.C = static_cast<int>(D);
          o.cl = 0;
          o.rank = 3;
          define(n.outputs[0], o);
          return;
        }
      }
      if (shp.size() == 2 && is_batch(shp[0]) && (shp[1] == -1 || shp[1] == total) && total % 8 == 0) {
        Val o = x;
        o.H = o.W = 1;
        o.C = static_cast<int>(total);
        o.cl = 0;
        o.rank = 2;
        define(n.outputs[0], o);
        return;
      }
    }
    // the graph input's rows [B, S*D] -> [B, S, D] with D % 8 != 0: the input-prep pass itself writes
    // S rows of D (stored round8(D)) per sample -- the f32 input is [B*S][D] in memory already
    if (x.kind == Val::ROWS_BF16 && x.rank == 2 && consumers(n.in(0)).size() == 1 && shp.size() == 3 &&
        is_batch(shp[0]) && !graph_outputs_.count(n.in(0))) {
      for (PlanOp& q : plan_.ops)
        if (q.kind == PlanOp::ROWS_PREP && q.out == x.buf && q.rows_per_sample == 1) {
          const int64_t F = q.C;
          int64_t S = shp[1], D = shp[2];
          if (S == -1 && D > 0) S = F / D;
          if (D == -1 && S > 0) D = F / S;
          if (S <= 0 || D <= 0 || S * D != F) break;
          q.C = static_cast<int>(D);
          q.Cp = round8(static_cast<int>(D));
          q.rows_per_sample = S;
          plan_.bufs[q.out].bytes_per_sample = static_cast<size_t>(S) * q.Cp * 2 * (opt_.split ? 2 : 1);
          Val o = x;
          o.H = static_cast<int>(S);
          o.W = 1;
          o.C = q.Cp;
          o.cl = q.Cp != D ? static_cast<int>(D) : 0;
          o.rank = 3;
          define(n.outputs[0], o);
          return;
        }
    }
    // one row per sample [B, C] -> [B, C, 1, 1] (gates broadcast over an image: squeeze-excitation)
    if ((x.kind == Val::ROWS_BF16 || x.kind == Val::NHWC) && x.H * x.W == 1 && shp.size() == 4 && is_batch(shp[0]) &&
        shp[1] == x.logical() && shp[2] == 1 && shp[3] == 1 && !x.flat_hw) {
      Val o = x;
      o.kind = Val::NHWC;
      o.rank = 0;
      define(n.outputs[0], o);
      return;
    }
    // rows with a single row per sample -> [B, C]
    if ((x.kind == Val::ROWS_BF16 || x.kind == Val::NHWC) && x.H * x.W == 1 && shp.size() == 2) {
      Val o = x;
      o.kind = Val::ROWS_BF16;
      o.rank = 2;
      define(n.outputs[0], o);
      return;
    }
    throw std::runtime_error("Reshape " + n.name + ": unsupported reshape for the HIP engine");
  }

  void lower_transpose(int idx) {
    const Node& n = m_.nodes[idx];
    const Val x = val(n.in(0), n);
    const auto perm = n.get_ints("perm");
    if (x.kind == Val::NCHW_FLAT && perm == std::vector<int64_t>{0, 2, 1}) {
      Val o = x;  // [B, C, HW]^T = the NHWC buffer read as rows
      o.kind = Val::ROWS_BF16;
      o.H = x.H * x.W;
      o.W = 1;
      o.rank = 3;
      define(n.outputs[0], o);
      return;
    }
    if ((x.kind == Val::HEADS || (x.kind == Val::ATTN && x.stage == 2)) && perm.size() == 4) {
      Val o = x;
      for (int i = 0; i < 4; ++i) o.perm[i] = x.perm[static_cast<int>(perm[i])];
      define(n.outputs[0], o);
      return;
    }
    // Channels-last blocks (ConvNeXt): activations are NHWC already, so NCHW -> NHWC is the same
    // buffer read as H * W rows of C per sample, and NHWC -> NCHW of such a view is the image again
    if (x.kind == Val::NHWC && dense(x) && perm == std::vector<int64_t>{0, 2, 3, 1}) {
      Val o = x;
      o.kind = Val::ROWS_BF16;
      o.img_h = x.H;
      o.img_w = x.W;
      o.H = x.H * x.W;
      o.W = 1;
      o.rank = 4;
      define(n.outputs[0], o);
      return;
    }
    if (x.kind == Val::ROWS_BF16 && x.rank == 4 && dense(x) && perm == std::vector<int64_t>{0, 3, 1, 2}) {
      Val o = x;
      o.kind = Val::NHWC;
      o.H = x.img_h;
      o.W = x.img_w;
      o.rank = o.img_h = o.img_w = 0;
      define(n.outputs[0], o);
      return;
    }
    throw std::runtime_error("Transpose " + n.name + ": unsupported transpose for the HIP engine");
  }

  // The graph output cannot be an [N, H, W, C] rows view: the output ops write [N, C] / [N, S, C] rows
  // or NCHW images.  Checked after each node so that the report names the node producing it.
  void check_output_view(const Node& n) {
    auto it = vid_.find(m_.outputs[0].name);
    if (output_view_seen_ || it == vid_.end() || vals_[it->second].kind != Val::ROWS_BF16 || vals_[it->second].rank != 4) return;
    output_view_seen_ = true;
    throw std::runtime_error(n.op_type + " " + n.name + ": an [N, H, W, C] view of an image cannot be the graph output "
                             "(transpose it back to [N, C, H, W])");
  }

  void lower_attn_matmul(int idx) {
    const Node& n = m_.nodes[idx];
    const Val a = val(n.in(0), n);
    const Val b = val(n.in(1), n);
    const std::array<int, 4> bhsd{{0, 2, 1, 3}}, bhds{{0, 2, 3, 1}};
    if (a.kind == Val::HEADS && a.kvg > 1)
      throw std::runtime_error("MatMul " + n.name + ": the first operand (Q, or the probabilities' place) carries a K/V "
                               "repeat; only K and V of an attention are repeated per group");
    if (a.kind == Val::HEADS && b.kind == Val::HEADS && a.perm == bhsd && b.perm == bhds && a.hd == b.hd && a.nh != b.nh)
      throw std::runtime_error("MatMul " + n.name + ": Q has " + std::to_string(a.nh) + " heads and K " + std::to_string(b.nh) +
                               (b.kvg ? " (" + std::to_string(b.nh / b.kvg) + " stored x groups of " + std::to_string(b.kvg) + ")"
                                      : std::string()) +
                               ": grouped-query attention needs K and V repeated to the query heads (repeat_kv with "
                               "G = heads / kv_heads)");
    if (a.kind == Val::HEADS && b.kind == Val::HEADS && a.perm == bhsd && b.perm == bhds && a.nh == b.nh &&
        a.hd == b.hd) {
      Val s;
      s.kind = Val::ATTN;
      s.stage = 0;
      s.q = vid_.at(n.in(0));
      s.k = vid_.at(n.in(1));
      define(n.outputs[0], s);
      return;
    }
    if (a.kind == Val::ATTN && a.stage == 1 && b.kind == Val::HEADS && b.perm == bhsd) {
      const int kg = std::max(1, vals_[a.k].kvg), vg = std::max(1, b.kvg);
      if (kg != vg || b.nh != vals_[a.k].nh)
        throw std::runtime_error("MatMul " + n.name + ": K is repeated over groups of " + std::to_string(kg) + " heads (" +
                                 std::to_string(vals_[a.k].nh) + " in all) and V over groups of " + std::to_string(vg) + " (" +
                                 std::to_string(b.nh) + "): grouped-query attention needs one group size for both");
      Val c = a;
      c.stage = 2;
      c.v = vid_.at(n.in(1));
      c.perm = bhsd;
      define(n.outputs[0], c);
      return;
    }
    // general batched MatMul of two dense rank-3 row activations: [S, K] x [K, N] per sample
    if (a.kind == Val::ROWS_BF16 && b.kind == Val::ROWS_BF16 && a.rank == 3 && b.rank == 3 && dense(a) && dense(b) &&
        a.logical() == b.H * b.W) {
      PlanOp p;
      p.kind = PlanOp::BMM;
      p.name = n.name;
      p.in = a.buf;
      p.in2 = b.buf;
      p.S = static_cast<int>(rows_of(a));
      p.gidx = a.logical();
      p.ld[0] = a.C;
      p.ld[1] = b.C;
      p.C = b.C;
      p.Cp = b.logical();
      p.rows_per_sample = rows_of(a);
      p.flops_per_sample = 2.0 * p.S * p.gidx * p.Cp;
      p.out = new_buf(static_cast<size_t>(p.S) * p.C * 2);
      Val o = a;
      o.C = b.C;
      o.cl = b.cl;
      o.buf = p.out;
      o.has_affine = false;
      define(n.outputs[0], o);
      add_op(std::move(p));
      return;
    }
    throw std::runtime_error("MatMul " + n.name + ": activation x activation MatMul outside the attention pattern and the "
                             "[S, K] x [K, N] row form");
  }

  void lower_scale(int idx) {
    const Node& n = m_.nodes[idx];
    {  // standalone erf-GELU (x / sqrt2 -> Erf -> + 1 -> * x -> * 0.5) on any activation
      std::vector<int> used;
      std::string gout;
      auto xi = vid_.find(n.in(0));
      if ((n.op_type == "Div" || n.op_type == "Mul") && xi != vid_.end() &&
          (vals_[xi->second].kind == Val::NHWC || vals_[xi->second].kind == Val::ROWS_BF16) &&
          match_gelu(n.in(0), used, gout)) {
        const Val x = vals_[xi->second];
        for (int u : used) done_[u] = true;
        return emit_unary(n, x, 2, 0.f, 0.f, gout);
      }
    }
    if (lower_binary_acts(n)) return;
    auto it = m_.initializers.find(n.in(1));
    if (n.op_type != "Sub" && vid_.count(n.in(0))) {
      const Val& x = vals_[vid_.at(n.in(0))];
      if (x.kind == Val::ATTN && x.stage == 0 && it != m_.initializers.end() && it->second.f.size() == 1) {
        Val o = x;
        if (x.kmask && !(it->second.f[0] > 0.f))
          throw std::runtime_error(n.op_type + " " + n.name + ": a scale after a key mask must be positive");
        o.scale = n.op_type == "Div" ? x.scale / it->second.f[0] : x.scale * it->second.f[0];
        if (x.mask >= 0) {  // a scale after an Add / Where reaches the accumulated bias as well
          AttnTable t = masks_[x.mask];
          for (float& e : t.t) e = n.op_type == "Div" ? e / it->second.f[0] : e * it->second.f[0];
          return define_masked(n, o, std::move(t));
        }
        define(n.outputs[0], o);
        return;
      }
    }
    // activation (op) per-channel / scalar constant  ->  affine
    for (int side = 0; side < 2; ++side) {
      const std::string& an = n.in(side);
      const std::string& cn = n.in(1 - side);
      if (!vid_.count(an) || !is_init(cn)) continue;
      const Val& x = vals_[vid_.at(an)];
      const auto& c = m_.initializers.at(cn).f;
      if (c.size() != 1 && static_cast<int>(c.size()) != x.logical()) continue;
      std::vector<float> sc(x.C, 1.f), sh(x.C, 0.f);
      for (int k = 0; k < x.logical(); ++k) {
        const float v = c[c.size() == 1 ? 0 : k];
        if (n.op_type == "Mul") sc[k] = v;
        else if (n.op_type == "Div" && side == 0) sc[k] = 1.f / v;
        else if (n.op_type == "Sub" && side == 0) sh[k] = -v;          // x - c
        else if (n.op_type == "Sub") { sc[k] = -1.f; sh[k] = v; }      // c - x
        else throw std::runtime_error(n.op_type + " " + n.name + ": constant / activation is not supported");
      }
      return standalone_affine(n, x, &sc, &sh, nullptr);
    }
    // Sub of two activations: a - b = (-1) * b + a
    if (n.op_type == "Sub" && vid_.count(n.in(0)) && vid_.count(n.in(1))) {
      const Val a = vals_[vid_.at(n.in(0))];
      const Val b = vals_[vid_.at(n.in(1))];
      if (a.kind == b.kind && a.C == b.C && a.H == b.H && a.W == b.W && a.pitch() == a.C && b.pitch() == b.C && !a.col && !b.col) {
        std::vector<float> sc(b.C, -1.f), sh(b.C, 0.f);
        return standalone_affine(n, b, &sc, &sh, &a);
      }
    }
    throw std::runtime_error(n.op_type + " " + n.name + ": unsupported elementwise op for the HIP engine");
  }

  void lower_softmax(int idx) {
    const Node& n = m_.nodes[idx];
    const Val x = val(n.in(0), n);
    const int64_t axis = n.get_int("axis", -1);
    if (x.kind == Val::ATTN && x.stage == 0 && (axis == -1 || axis == 3)) {
      Val o = x;
      o.stage = 1;
      define(n.outputs[0], o);
      return;
    }
    const int rank = x.rank ? x.rank : 2;
    if ((x.kind == Val::ROWS_BF16 || (x.kind == Val::NHWC && x.H * x.W == 1)) && dense(x) &&
        (axis == -1 || axis == rank - 1)) {
      PlanOp p;
      p.kind = PlanOp::SOFTMAX;
      p.name = n.name;
      p.in = x.buf;
      p.C = x.logical();  // pad columns: skipped by the reduction, written 0
      p.ld_store = x.padded() ? x.C : 0;
      p.rows_per_sample = static_cast<long long>(x.H) * x.W;
      Val o = x;
      o.kind = Val::ROWS_BF16;
      o.rank = rank;
      if (graph_outputs_.count(n.outputs[0]) && consumers(n.outputs[0]).empty()) {
        p.out_f32 = kBufGraphOut;  // probabilities straight to the f32 output
        o.kind = Val::ROWS_F32;
        o.buf = kBufGraphOut;
      } else {
        p.out = new_buf(static_cast<size_t>(p.rows_per_sample) * x.C * 2);
        o.buf = p.out;
      }
      define(n.outputs[0], o);
      add_op(std::move(p));
      return;
    }
    throw std::runtime_error("Softmax " + n.name + ": only attention scores or the last axis of rows are supported");
  }

  // LayerNormalization, and the single-node RMSNorms RMSNormalization (opset 23) /
  // SimplifiedLayerNormalization (ONNX Runtime's optimiser): the same row kernel in its rms mode
  void lower_layernorm(int idx) {
    const Node& n = m_.nodes[idx];
    const bool rms = n.op_type != "LayerNormalization";
    const Val x = val(n.in(0), n);
    if (x.kind != Val::ROWS_BF16 || !dense(x))
      throw std::runtime_error(n.op_type + " " + n.name + ": input must be dense rows");
    const int64_t axis = n.get_int("axis", -1);
    if (!(axis == -1 || axis == (x.rank ? x.rank : 2) - 1))
      throw std::runtime_error(rms ? n.op_type + " " + n.name + ": axis must be last" : "LayerNormalization: axis must be last");
    if (rms)
      for (size_t k = 1; k < n.outputs.size(); ++k)
        if (!n.outputs[k].empty() && (!consumers(n.outputs[k]).empty() || graph_outputs_.count(n.outputs[k])))
          throw std::runtime_error(n.op_type + " " + n.name + ": the inv_std_var output must be unused");
    const int Cl = x.logical();
    std::vector<float> g = init(n.in(1), n).f, b(Cl, 0.f);
    if (!rms && n.inputs.size() > 2 && !n.in(2).empty()) b = init(n.in(2), n).f;
    if (static_cast<int>(g.size()) != Cl || static_cast<int>(b.size()) != Cl)
      throw std::runtime_error(n.op_type + " " + n.name + ": scale/bias size mismatch");
    g.resize(x.C, 0.f);  // stored pad columns: written 0 by the kernel
    b.resize(x.C, 0.f);
    PlanOp p;
    p.kind = PlanOp::LAYERNORM;
    p.name = n.name;
    p.in = x.buf;
    p.scale_off = push_f32(g);
    p.shift_off = push_f32(b);
    p.eps = n.get_float("epsilon", 1e-5f);
    p.rms = rms ? 1 : 0;
    p.C = x.C;
    p.Cp = Cl;
    p.rows_per_sample = static_cast<long long>(x.H) * x.W;
    p.out = new_buf(static_cast<size_t>(x.H) * x.W * x.C * 2);
    Val o = x;
    o.buf = p.out;
    define(n.outputs[0], o);
    add_op(std::move(p));
  }

  // ---- RMSNorm as torch exports it ------------------------------------------------------------------
  // Pow(x, 2) / Mul(x, x) -> ReduceMean(-1, keepdims) -> Add(eps) -> Sqrt -> Div(x, .) /
  // Mul(x, Reciprocal(.)) / Mul(x, Div(1, .)) [-> Mul(weight [C])]  ==> one LAYERNORM op with rms = 1.
  // The walk reaches the square first, so the chain is anchored there: a square of rows read only by
  // a ReduceMean that is not the token-axis mean (lower_spatial_reduce) is this pattern or an error.
  bool rmsnorm_anchor(const Node& n) const {
    auto xi = vid_.find(n.in(0));
    if (xi == vid_.end() || vals_[xi->second].kind != Val::ROWS_BF16) return false;
    const int rm = sole_consumer(n.outputs[0]);
    if (rm < 0 || m_.nodes[rm].op_type != "ReduceMean") return false;
    std::vector<int64_t> ax;
    node_axes(m_.nodes[rm], ax);
    const Val& x = vals_[xi->second];
    return !(x.rank == 3 && (ax == std::vector<int64_t>{1} || ax == std::vector<int64_t>{-2}));
  }

  void lower_rmsnorm(int idx) {
    const Node& n = m_.nodes[idx];
    const Val x = val(n.in(0), n);
    const std::string& xn = n.in(0);
    auto fail = [&](const std::string& why) {
      throw std::runtime_error(n.op_type + " " + n.name + ": a square under a ReduceMean is only supported as the head of "
                               "the decomposed RMSNorm pattern (" + why + ")");
    };
    if (n.op_type == "Pow" && !scalar_is(n.in(1), 2.f)) fail("the exponent must be 2");
    const Node& rm = m_.nodes[sole_consumer(n.outputs[0])];
    bool ok;
    const int64_t axis = last_axis_of(rm, m_, ok);
    if (!ok || !(axis == -1 || axis == (x.rank ? x.rank : 2) - 1))
      fail("ReduceMean " + rm.name + " must reduce over the last axis with keepdims");
    if (!dense(x)) fail("input must be dense rows");
    const int add = sole_consumer(rm.outputs[0]);
    if (add < 0 || m_.nodes[add].op_type != "Add")
      fail("the mean of squares " + rm.outputs[0] + " must be read by the Add of eps alone");
    const std::string& eps_name = other_input(m_.nodes[add], rm.outputs[0]);
    auto ei = m_.initializers.find(eps_name);
    if (ei == m_.initializers.end() || ei->second.f.size() != 1)
      fail("eps of Add " + m_.nodes[add].name + " must be a scalar constant");
    const int sq_rt = sole_consumer(m_.nodes[add].outputs[0]);
    if (sq_rt < 0 || m_.nodes[sq_rt].op_type != "Sqrt") fail("no Sqrt of mean + eps");
    const std::string& rt = m_.nodes[sq_rt].outputs[0];
    std::vector<int> used = {sole_consumer(n.outputs[0]), add, sq_rt};
    int c = sole_consumer(rt), norm = -1;
    if (c >= 0 && m_.nodes[c].op_type == "Div" && m_.nodes[c].in(0) == xn && m_.nodes[c].in(1) == rt) {
      norm = c;
    } else if (c >= 0 && (m_.nodes[c].op_type == "Reciprocal" ||
                          (m_.nodes[c].op_type == "Div" && m_.nodes[c].in(1) == rt && scalar_is(m_.nodes[c].in(0), 1.f)))) {
      used.push_back(c);
      const std::string& inv = m_.nodes[c].outputs[0];
      const int mu = sole_consumer(inv);
      if (mu >= 0 && m_.nodes[mu].op_type == "Mul" && other_input(m_.nodes[mu], inv) == xn) norm = mu;
    }
    if (norm < 0) fail("no x / sqrt, x * Reciprocal(sqrt) or x * (1 / sqrt) after Sqrt " + m_.nodes[sq_rt].name);
    used.push_back(norm);
    std::vector<float> g(x.C, 1.f);
    std::string cur = m_.nodes[norm].outputs[0];
    c = sole_consumer(cur);
    if (c >= 0 && m_.nodes[c].op_type == "Mul" && is_init(other_input(m_.nodes[c], cur)) &&
        static_cast<int>(m_.initializers.at(other_input(m_.nodes[c], cur)).f.size()) == x.logical()) {
      g = m_.initializers.at(other_input(m_.nodes[c], cur)).f;
      used.push_back(c);
      cur = m_.nodes[c].outputs[0];
    }
    if (x.padded()) fail("C % 8 == 0 (stored pad columns)");
    for (int u : used) done_[u] = true;
    PlanOp p;
    p.kind = PlanOp::LAYERNORM;
    p.name = n.name + "+decomposed_rmsnorm";
    p.in = x.buf;
    p.scale_off = push_f32(g);
    p.shift_off = push_f32(std::vector<float>(x.C, 0.f));
    p.eps = ei->second.f[0];
    p.rms = 1;
    p.C = x.C;
    p.Cp = x.C;
    p.rows_per_sample = static_cast<long long>(x.H) * x.W;
    p.out = new_buf(static_cast<size_t>(x.H) * x.W * x.C * 2);
    Val o = x;
    o.buf = p.out;
    o.has_affine = false;
    define(cur, o);
    add_op(std::move(p));
  }

  // ---- rotary position embeddings ---------------------------------------------------------------------
  // On a heads view x, [N, H, S, hd] (perm {0,2,1,3}) or [N, S, H, hd] (identity), torch's
  // x * cos + rotate_half(x) * sin exports as Mul(x, COS), Slice(x, 0:hd/2), Slice(x, hd/2:hd), Neg(hi),
  // Concat([-hi, lo], -1), Mul(., SIN), Add.  A Mul or a last-axis Slice reading such a view is one of
  // x's three readers in that pattern or an error; the whole pattern is one ROPE op.
  static int rope_layout(const Val& v) {
    if (v.kind != Val::HEADS) return -1;
    if (v.perm == std::array<int, 4>{{0, 2, 1, 3}}) return 0;
    if (v.perm == std::array<int, 4>{{0, 1, 2, 3}}) return 1;
    return -1;
  }
  // the heads-view operand of a Mul / Slice (-1: none)
  int rope_operand(const Node& n) const {
    const int k = n.op_type == "Slice" ? 1 : 2;
    for (int side = 0; side < k && side < static_cast<int>(n.inputs.size()); ++side) {
      auto it = vid_.find(n.in(side));
      if (it != vid_.end() && rope_layout(vals_[it->second]) >= 0) return side;
    }
    return -1;
  }
  // a Slice of a heads view, or a Mul of one that a Slice reads too (a Mul alone keeps its other lowerings)
  bool rope_anchor(const Node& n) const {
    const int side = rope_operand(n);
    if (side < 0 || n.op_type == "Slice") return side >= 0;
    for (int c : consumers(n.in(side)))
      if (m_.nodes[c].op_type == "Slice" && m_.nodes[c].in(0) == n.in(side)) return true;
    return false;
  }

  // starts / ends / axes / steps of a one-axis Slice (attributes or inputs); false when not static
  bool slice_range(const Node& n, int64_t& s0, int64_t& e0, int64_t& axis, int64_t& step) const {
    std::vector<int64_t> starts = n.get_ints("starts"), ends = n.get_ints("ends"), axes = n.get_ints("axes"), steps;
    if (starts.empty() && n.inputs.size() >= 3) {
      if (!ints_of(n.in(1), starts) || !ints_of(n.in(2), ends)) return false;
      if (n.inputs.size() > 3 && !n.in(3).empty() && !ints_of(n.in(3), axes)) return false;
      if (n.inputs.size() > 4 && !n.in(4).empty() && !ints_of(n.in(4), steps)) return false;
    }
    if (starts.size() != 1 || ends.size() != 1 || axes.size() > 1 || steps.size() > 1) return false;
    s0 = starts[0];
    e0 = ends[0];
    axis = axes.empty() ? 0 : axes[0];
    step = steps.empty() ? 1 : steps[0];
    return true;
  }

  // A rotary table: a float initializer that broadcasts over the view's logical shape as [S][hd]
  std::vector<float> rope_table(const Node& at, const std::string& name, const Val& x, int layout) const {
    auto it = m_.initializers.find(name);
    if (it == m_.initializers.end())
      throw std::runtime_error("Mul " + at.name + ": the rotary table " + name + " must be an initializer (tables computed "
                               "in the graph or gathered by a position_ids input are not supported)");
    const auto& t = it->second;
    const int64_t S = x.H, hd = x.hd;
    using V = std::vector<int64_t>;
    const bool ok = layout == 0 ? (t.dims == V{S, hd} || t.dims == V{1, S, hd} || t.dims == V{1, 1, S, hd})
                                : t.dims == V{1, S, 1, hd};
    if (!ok || t.f.size() != static_cast<size_t>(S * hd)) {
      std::string shp;
      for (auto d : t.dims) shp += (shp.empty() ? "" : ", ") + std::to_string(d);
      throw std::runtime_error("Mul " + at.name + ": the rotary table " + name + " [" + shp + "] does not broadcast over the "
                               "heads as [S, hd] = [" + std::to_string(S) + ", " + std::to_string(hd) + "] (accepted: " +
                               (layout == 0 ? "[S, hd], [1, S, hd], [1, 1, S, hd]" : "[1, S, 1, hd]") + ")");
    }
    return t.f;
  }

  void lower_rope(int idx) {
    const Node& n = m_.nodes[idx];
    const std::string& xn = n.in(rope_operand(n));
    const Val x = val(xn, n);
    const int layout = rope_layout(x), hd = x.hd, h2 = x.hd / 2;
    const std::string where = n.op_type + " " + n.name + ": ";
    if (graph_outputs_.count(xn)) throw std::runtime_error(where + "a heads view cannot be a graph output");
    // x's readers in the pattern: the Mul by COS and the two half Slices
    int mul_cos = -1, lo = -1, hi = -1;
    for (int c : consumers(xn)) {
      const Node& q = m_.nodes[c];
      if (done_[c] && c != idx) continue;
      if (q.op_type == "Mul" && q.inputs.size() == 2 && q.in(0) != q.in(1)) {
        if (mul_cos >= 0) throw std::runtime_error(where + "two Muls (" + m_.nodes[mul_cos].name + ", " + q.name + ") read the heads view " + xn + ": not a rotary embedding");
        mul_cos = c;
      } else if (q.op_type == "Slice" && q.in(0) == xn) {
        int64_t s0, e0, axis, step;
        if (!slice_range(q, s0, e0, axis, step)) throw std::runtime_error("Slice " + q.name + ": the range of a slice of a heads view must be static");
        if (!(axis == -1 || axis == 3)) throw std::runtime_error("Slice " + q.name + ": a heads view is sliced only along its last axis (rotary embedding)");
        if (step != 1)
          throw std::runtime_error("Slice " + q.name + ": step " + std::to_string(step) + " on a heads view: only the rotate-half "
                                   "rotary embedding (two contiguous halves) is supported, not the interleaved form");
        if (s0 < 0) s0 += hd;
        if (e0 < 0) e0 += hd;
        e0 = std::min<int64_t>(e0, hd);
        if (s0 == 0 && e0 == h2 && lo < 0) lo = c;
        else if (s0 == h2 && e0 == hd && hi < 0) hi = c;
        else
          throw std::runtime_error("Slice " + q.name + ": [" + std::to_string(s0) + ", " + std::to_string(e0) + ") of a heads view with hd = " +
                                   std::to_string(hd) + ": the halves of a rotary embedding must be [0, hd/2) and [hd/2, hd) "
                                   "(partial and interleaved rotary are not supported)");
      }
    }
    if (mul_cos < 0 || lo < 0 || hi < 0)
      throw std::runtime_error(where + "a Mul / Slice of a heads view is supported only as part of a rotary embedding over all hd "
                               "columns: Mul(x, COS), Slice(x, 0:hd/2), Slice(x, hd/2:hd) (partial rotary is not supported)");
    const Node& mc = m_.nodes[mul_cos];
    const int neg = sole_consumer(m_.nodes[hi].outputs[0]);
    if (neg < 0 || m_.nodes[neg].op_type != "Neg")
      throw std::runtime_error("Slice " + m_.nodes[hi].name + ": the high half of a rotary embedding must be read by a Neg alone "
                               "(partial rotary with a pass-through half is not supported)");
    const int cat = sole_consumer(m_.nodes[neg].outputs[0]);
    const int cat2 = sole_consumer(m_.nodes[lo].outputs[0]);
    if (cat < 0 || cat != cat2 || m_.nodes[cat].op_type != "Concat" || m_.nodes[cat].inputs.size() != 2 ||
        m_.nodes[cat].in(0) != m_.nodes[neg].outputs[0] || m_.nodes[cat].in(1) != m_.nodes[lo].outputs[0] ||
        !(m_.nodes[cat].get_int("axis", 0) == -1 || m_.nodes[cat].get_int("axis", 0) == 3))
      throw std::runtime_error("Slice " + m_.nodes[lo].name + ": the halves of a rotary embedding must meet in Concat([-hi, lo], "
                               "axis -1)");
    const int mul_sin = sole_consumer(m_.nodes[cat].outputs[0]);
    if (mul_sin < 0 || m_.nodes[mul_sin].op_type != "Mul")
      throw std::runtime_error("Concat " + m_.nodes[cat].name + ": the rotated halves must be multiplied by the SIN table");
    const Node& ms = m_.nodes[mul_sin];
    const int add = sole_consumer(ms.outputs[0]);
    if (add < 0 || add != sole_consumer(mc.outputs[0]) || m_.nodes[add].op_type != "Add" || m_.nodes[add].inputs.size() != 2)
      throw std::runtime_error("Mul " + ms.name + ": x * COS and rotate_half(x) * SIN must meet in one Add");
    if (!kern::attention_supported(hd, x.H))
      throw std::runtime_error(where + "rotary embedding on head dim " + std::to_string(hd) + ": needs a head dim the attention "
                               "kernel takes (32, 64, 80, 96 or 128)");
    const std::vector<float> cs = rope_table(mc, other_input(mc, xn), x, layout);
    const std::vector<float> sn = rope_table(ms, other_input(ms, m_.nodes[cat].outputs[0]), x, layout);
    for (int u : {mul_cos, lo, hi, neg, cat, mul_sin, add}) done_[u] = true;
    PlanOp p;
    p.kind = PlanOp::ROPE;
    p.name = m_.nodes[add].name + "+rope";
    p.in = x.buf;
    p.col[0] = x.col;
    p.ld[0] = x.pitch();
    p.S = x.H;
    p.nh = x.nh;
    p.hd = hd;
    p.gidx = layout;
    p.scale_off = push_f32(cs);
    p.shift_off = push_f32(sn);
    p.C = x.nh * hd;
    p.rows_per_sample = x.H;
    p.out = new_buf(static_cast<size_t>(x.H) * p.C * 2);
    Val o = x;  // the same heads view over the new dense rows
    o.buf = p.out;
    o.C = p.C;
    o.cl = 0;
    o.ld = 0;
    o.col = 0;
    define(m_.nodes[add].outputs[0], o);
    add_op(std::move(p));
  }

  void lower_gather(int idx) {
    const Node& n = m_.nodes[idx];
    const Val x = val(n.in(0), n);
    std::vector<int64_t> ix;
    const auto it = m_.initializers.find(n.in(1));
    if (x.kind == Val::ROWS_BF16 && x.rank == 3 && n.get_int("axis", 0) == 1 && it != m_.initializers.end() &&
        it->second.dims.empty() && ints_of(n.in(1), ix) && ix.size() == 1 && x.pitch() == x.C) {
      const int S = x.H * x.W;
      int64_t i = ix[0] < 0 ? ix[0] + S : ix[0];
      if (i < 0 || i >= S) throw std::runtime_error("Gather " + n.name + ": index out of range");
      PlanOp p;
      p.kind = PlanOp::GATHER_ROWS;
      p.name = n.name;
      p.in = x.buf;
      p.S = S;
      p.gidx = static_cast<int>(i);
      p.C = x.C;
      p.out = new_buf(static_cast<size_t>(x.C) * 2);
      Val o;
      o.kind = Val::ROWS_BF16;
      o.C = x.C;
      o.rank = 2;
      o.buf = p.out;
      define(n.outputs[0], o);
      add_op(std::move(p));
      return;
    }
    throw std::runtime_error("Gather " + n.name + ": only selecting one token (axis 1, scalar index) is supported");
  }

  void lower_concat(int idx) {
    const Node& n = m_.nodes[idx];
    if (n.inputs.size() == 2 && n.get_int("axis", 0) == 1) {
      const Val a = val(n.in(0), n);
      const Val b = val(n.in(1), n);
      if (a.kind == Val::BCAST_INIT && b.kind == Val::ROWS_BF16 && b.rank == 3 && a.C == b.C && b.pitch() == b.C) {
        Val o;
        o.kind = Val::TOKCAT;
        o.C = b.C;
        o.H = b.H * b.W + 1;
        o.rank = 3;
        o.init_name = a.init_name;
        o.patches = vid_.at(n.in(1));
        define(n.outputs[0], o);
        return;
      }
    }
    return general_concat(n, n.get_int("axis", 0));
  }

  // TOKCAT (+ optional position embedding initializer) -> token assembly kernel.
  void emit_tokens(const Node& n, const Val& cat, const std::string* pos_name, const std::string& out_name) {
    const Val& pt = vals_[cat.patches];
    const int S = cat.H, C = cat.C;
    PlanOp p;
    p.kind = PlanOp::TOKENS;
    p.name = n.name;
    p.in = pt.buf;
    p.S = S - 1;
    p.C = C;
    p.scale_off = push_f32(m_.initializers.at(cat.init_name).f);
    if (pos_name) {
      const auto& pos = m_.initializers.at(*pos_name);
      if (pos.numel() != static_cast<int64_t>(S) * C)
        throw std::runtime_error("Add " + n.name + ": position embedding must be [1, S, C]");
      p.shift_off = push_f32(pos.f);
    }
    p.out = new_buf(static_cast<size_t>(S) * C * 2);
    Val o;
    o.kind = Val::ROWS_BF16;
    o.C = C;
    o.H = S;
    o.rank = 3;
    o.buf = p.out;
    define(out_name, o);
    add_op(std::move(p));
  }

  // ---- Clip / grouped conv / decomposed LayerNorm / row softmax / constant binary ops ------------
  // Clip bounds from attributes (opset < 11) or the optional min/max initializer inputs.
  bool clip_bounds(const Node& n, float& lo, float& hi) const {
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
  int take_act(std::string& cur, float& lo, float& hi) {
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
  void lower_gconv(int idx) {
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
    int c1 = sole_consumer(cur);
    if (c1 >= 0 && m_.nodes[c1].op_type == "BatchNormalization") {
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

  void lower_clip(int idx) {
    const Node& n = m_.nodes[idx];
    const Val x = val(n.in(0), n);
    float lo, hi;
    if (!clip_bounds(n, lo, hi)) throw std::runtime_error("Clip " + n.name + ": bounds must be constants");
    standalone_affine(n, x, nullptr, nullptr, nullptr, 3, lo, hi);
  }

  static int64_t last_axis_of(const Node& n, const onnx::Model& m, bool& ok) {
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
  // ReduceMean / ReduceSum / ReduceMax over the spatial axes of an image or the token axis of
  // rows: the GAP kernel in mode 0 / 1 / 2.  False when the reduction is some other one.
  bool lower_spatial_reduce(int idx, int mode) {
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

  void lower_reduce_mean(int idx) {
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
    const int rm2 = sole_consumer(m_.nodes[sq].outputs[0]);
    if (rm2 < 0 || m_.nodes[rm2].op_type != "ReduceMean") fail("no variance mean");
    const int add = sole_consumer(m_.nodes[rm2].outputs[0]);
    if (add < 0 || m_.nodes[add].op_type != "Add") fail("no variance + eps");
    const std::string eps_name = other_input(m_.nodes[add], m_.nodes[rm2].outputs[0]);
    auto ei = m_.initializers.find(eps_name);
    if (ei == m_.initializers.end() || ei->second.f.size() != 1) fail("eps must be a scalar constant");
    const int sq_rt = sole_consumer(m_.nodes[add].outputs[0]);
    if (sq_rt < 0 || m_.nodes[sq_rt].op_type != "Sqrt" || m_.nodes[div].in(1) != m_.nodes[sq_rt].outputs[0])
      fail("no sqrt feeding the division");
    std::vector<float> g(x.C, 1.f), b(x.C, 0.f);
    std::string cur = m_.nodes[div].outputs[0];
    std::vector<int> used = {sub, sq, rm2, add, sq_rt, div};
    int c = sole_consumer(cur);
    if (c >= 0 && m_.nodes[c].op_type == "Mul" && affine_init(other_input(m_.nodes[c], cur))) {
      g = m_.initializers.at(other_input(m_.nodes[c], cur)).f;
      used.push_back(c);
      cur = m_.nodes[c].outputs[0];
      c = sole_consumer(cur);
    }
    if (c >= 0 && m_.nodes[c].op_type == "Add" && affine_init(other_input(m_.nodes[c], cur))) {
      b = m_.initializers.at(other_input(m_.nodes[c], cur)).f;
      used.push_back(c);
      cur = m_.nodes[c].outputs[0];
    }
    if (x.padded()) fail("C % 8 == 0 (stored pad columns)");
    for (int u : used) done_[u] = true;
    PlanOp p;
    p.kind = PlanOp::LAYERNORM;
    p.name = n.name + "+decomposed_layernorm";
    p.in = x.buf;
    p.scale_off = push_f32(g);
    p.shift_off = push_f32(b);
    p.eps = ei->second.f[0];
    p.C = x.C;
    p.rows_per_sample = static_cast<long long>(x.H) * x.W;
    p.out = new_buf(static_cast<size_t>(x.H) * x.W * x.C * 2);
    Val o = x;
    o.buf = p.out;
    define(cur, o);
    add_op(std::move(p));
  }

  // Explicit pads of a conv plus those of a zero Pad folded into it (lower_pad).
  std::vector<int64_t> conv_pads(const Node& n) const {
    auto pads = n.get_ints("pads", {0, 0, 0, 0});
    if (pads.size() != 4) throw std::runtime_error("Conv " + n.name + ": expected 4 pads");
    auto it = folded_pad_.find(n.in(0));
    if (it != folded_pad_.end())
      for (int k = 0; k < 4; ++k) pads[k] += it->second[k];
    return pads;
  }

  // Pad (constant mode, value 0, spatial axes of an NHWC image only, /root/reference has no Pad
  // kernel -- ONNX Runtime's CPU EP runs it there).  A Pad whose only reader is a Conv with explicit
  // pads folds into that conv (the conv kernels read out-of-range pixels as zero); otherwise one
  // NHWC pad pass writes the padded image.
  // ZeroInsert (domain "die", from rewrite_conv_transpose): the same pass with strides: zeros between
  // the input's pixels and `pads` = [top, left, bottom, right] around them.
  void lower_pad(int idx) {
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

  void emit_pad(const Node& n, const Val& x, const std::array<int64_t, 4>& tlbr, int sy, int sx) {
    const int c = sole_consumer(n.outputs[0]);
    if (sy == 1 && sx == 1 && c >= 0 && m_.nodes[c].op_type == "Conv" && m_.nodes[c].in(0) == n.outputs[0] &&
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

  bool scalar_init(const std::string& name, float& v) const {
    auto it = m_.initializers.find(name);
    if (it == m_.initializers.end() || it->second.numel() != 1) return false;
    v = it->second.f.empty() ? static_cast<float>(it->second.i.at(0)) : it->second.f[0];
    return true;
  }
  // The other branch `fill` of the Where `n` on attention scores: a scalar initializer <= -1e4.
  void check_score_fill(const Node& n, const std::string& fill) const {
    float f = 0.f;
    if (!scalar_init(fill, f))
      throw std::runtime_error("Where " + n.name + ": on attention scores the other branch must be a scalar initializer");
    if (!(f <= -1e4f))
      throw std::runtime_error("Where " + n.name + ": fill " + std::to_string(f) + " is not a mask (only fills <= -1e4 or "
                               "-inf fold into the attention kernel as -inf); a finite fill above -1e4 is not supported");
  }

  // Comparisons (bool results are stored as 1 / 0 activations): two activations -> a binary op,
  // an activation and a scalar constant -> a unary code (the constant on the left mirrors the test).
  void lower_compare(int idx) {
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
    throw std::runtime_error(n.op_type + " " + n.name + ": only two activations of one shape or one and a scalar");
  }

  // Where(cond, a, b): cond an activation; a / b activations of cond's shape or scalar constants.
  void lower_where(int idx) {
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
    p.out = new_buf(static_cast<size_t>(rows_of(c)) * c.C * 2);
    Val o = *like;
    o.buf = p.out;
    o.has_affine = false;
    define(n.outputs[0], o);
    add_op(std::move(p));
  }

  // Cast of an activation: to a float type -> the same values; to bool -> v != 0.  Integer targets
  // would need rounding the stored representation cannot express exactly: rejected.
  void lower_cast(int idx) {
    const Node& n = m_.nodes[idx];
    const int to = static_cast<int>(n.get_int("to", onnx::FLOAT));
    if (to == onnx::BOOL) return emit_unary(n, materialize_in(n.in(0), n), 24, 0.f, 0.f, n.outputs[0]);
    if (!onnx::is_float_type(to)) throw std::runtime_error("Cast " + n.name + ": only casts to float types or bool");
    define(n.outputs[0], val(n.in(0), n));
  }

  // Resize (opset 10+: scales / sizes inputs) and Upsample (scales attribute or input) of an
  // image: nearest or linear over H, W.
  void lower_resize(int idx) {
    const Node& n = m_.nodes[idx];
    const Val x = materialize_in(n.in(0), n);
    if (x.kind != Val::NHWC || !dense(x)) throw std::runtime_error(n.op_type + " " + n.name + ": only images");
    const std::string mode = n.get_string("mode", "nearest");
    if (mode != "nearest" && mode != "linear" && mode != "bilinear")
      throw std::runtime_error(n.op_type + " " + n.name + ": mode " + mode + " is not supported (nearest, linear)");
    if (n.get_int("antialias", 0) != 0) throw std::runtime_error(n.op_type + " " + n.name + ": antialias is not supported");
    if (n.has("axes")) throw std::runtime_error(n.op_type + " " + n.name + ": the axes attribute is not supported");
    std::vector<float> scales = n.get_floats("scales");
    std::vector<int64_t> sizes;
    const bool upsample = n.op_type == "Upsample";
    auto floats_of = [&](const std::string& nm) {
      auto it = m_.initializers.find(nm);
      if (it == m_.initializers.end()) throw std::runtime_error(n.op_type + " " + n.name + ": scales must be a constant");
      return it->second.f;
    };
    if (scales.empty()) {
      if (upsample && n.inputs.size() >= 2) scales = floats_of(n.in(1));
      if (!upsample && n.inputs.size() == 2 && !n.in(1).empty()) scales = floats_of(n.in(1));  // opset 10
      if (!upsample && n.inputs.size() >= 3 && !n.in(2).empty() && !floats_of(n.in(2)).empty()) scales = floats_of(n.in(2));
      if (!upsample && scales.empty() && n.inputs.size() >= 4 && !n.in(3).empty() && !ints_of(n.in(3), sizes))
        throw std::runtime_error(n.op_type + " " + n.name + ": sizes must be known at load time");
    }
    float sh, sw;
    int Ho, Wo;
    if (!sizes.empty()) {
      if (sizes.size() != 4 || (sizes[1] != x.logical() && sizes[1] != kBatchDim))
        throw std::runtime_error(n.op_type + " " + n.name + ": sizes must be [N, C, H, W] with C unchanged");
      Ho = static_cast<int>(sizes[2]);
      Wo = static_cast<int>(sizes[3]);
      sh = static_cast<float>(Ho) / x.H;
      sw = static_cast<float>(Wo) / x.W;
    } else {
      if (scales.size() != 4 || scales[0] != 1.f || scales[1] != 1.f)
        throw std::runtime_error(n.op_type + " " + n.name + ": scales must be [1, 1, sh, sw]");
      sh = scales[2];
      sw = scales[3];
      Ho = static_cast<int>(std::floor(x.H * static_cast<double>(sh)));
      Wo = static_cast<int>(std::floor(x.W * static_cast<double>(sw)));
    }
    if (Ho < 1 || Wo < 1 || !(sh > 0.f) || !(sw > 0.f)) throw std::runtime_error(n.op_type + " " + n.name + ": empty output");
    static const std::map<std::string, int> coords = {{"half_pixel", 0}, {"asymmetric", 1}, {"align_corners", 2},
                                                      {"pytorch_half_pixel", 3}, {"tf_half_pixel_for_nn", 4}};
    static const std::map<std::string, int> nearests = {
        {"round_prefer_floor", 0}, {"round_prefer_ceil", 1}, {"floor", 2}, {"ceil", 3}};
    // Upsample and opset-10 Resize: asymmetric coordinates, floor rounding for nearest
    const bool legacy = upsample || m_.opset() < 11;
    const std::string cm = legacy ? "asymmetric" : n.get_string("coordinate_transformation_mode", "half_pixel");
    const std::string nm = legacy ? "floor" : n.get_string("nearest_mode", "round_prefer_floor");
    if (!coords.count(cm) || !nearests.count(nm))
      throw std::runtime_error(n.op_type + " " + n.name + ": coordinate mode " + cm + " / nearest mode " + nm + " is not supported");
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

  // Channel range [s0, e0) of a dense image / rows value -> a column copy (s0 % 8 == 0).
  void emit_channel_slice(const Node& n, const Val& x, int64_t s0, int64_t e0, const std::string& out) {
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
  void lower_split(int idx) {
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
  void lower_slice(int idx) {
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

  void lower_bn(int idx) {
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

  void lower_relu(int idx) {
    const Node& n = m_.nodes[idx];
    const Val x = materialize_in(n.in(0), n);
    standalone_affine(n, x, nullptr, nullptr, nullptr);
  }

  void lower_add(int idx) {
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

  // ---- general path: any-activation unary, broadcast binary, concat / slice -----------------------
  static bool dense(const Val& v) { return (v.kind == Val::NHWC || v.kind == Val::ROWS_BF16) && v.pitch() == v.C && !v.col && !v.flat_hw; }
  static long long rows_of(const Val& v) { return static_cast<long long>(v.H) * v.W; }

  void lower_unary(int idx) {
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

  void emit_unary(const Node& n, const Val& x, int act, float a, float b, const std::string& out_name) {
    if (!dense(x)) throw std::runtime_error(n.op_type + " " + n.name + ": input must be a dense image or rows tensor");
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
    p.out = new_buf(static_cast<size_t>(rows_of(x)) * x.C * 2);
    Val o = x;
    o.buf = p.out;
    o.has_affine = false;
    define(out_name, o);
    add_op(std::move(p));
  }

  // Add / Sub / Mul / Div of two activations: same shape, or the second one broadcast per sample
  // ([B, C, 1, 1] or [B, C] gates over an image's pixels / a sequence's rows: squeeze-excitation,
  // GLU-style gating).  Returns false when the operands do not fit (the caller tries other forms).
  bool lower_binary_acts(const Node& n) {
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
    p.out = new_buf(static_cast<size_t>(rows_of(a)) * a.C * 2);
    Val o = a;
    o.buf = p.out;
    o.has_affine = false;
    define(cur, o);
    add_op(std::move(p));
    return true;
  }

  // The channel axis of a value (NHWC: NCHW axis 1; rows: the last axis) for Concat / Slice.
  static bool is_channel_axis(const Val& v, int64_t axis) {
    if (v.kind == Val::NHWC) return axis == 1 || axis == -3;
    const int r = v.rank ? v.rank : 2;
    return v.kind == Val::ROWS_BF16 && (axis == -1 || axis == r - 1);
  }

  void general_concat(const Node& n, int64_t axis) {
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

  void standalone_affine(const Node& n, const Val& x, const std::vector<float>* sc, const std::vector<float>* sh,
                         const Val* z, int own_act = 0, float own_lo = 0.f, float own_hi = 0.f) {
    if (x.kind != Val::NHWC && x.kind != Val::ROWS_BF16)
      throw std::runtime_error(n.op_type + " " + n.name + ": unsupported input layout");
    if (x.C % 8) throw std::runtime_error(n.op_type + " " + n.name + ": channels must be a multiple of 8");
    if (x.pitch() != x.C || x.col) throw std::runtime_error(n.op_type + " " + n.name + ": strided operand");
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
    p.out = new_buf(static_cast<size_t>(x.H) * x.W * x.C * 2);
    Val o = x;
    o.buf = p.out;
    o.has_affine = false;
    define(cur, o);
    add_op(std::move(p));
  }

  void lower_pool(int idx) {
    const Node& n = m_.nodes[idx];
    Val x = materialize_in(n.in(0), n);
    if (x.kind != Val::NHWC) throw std::runtime_error(n.op_type + " " + n.name + ": input must be an image tensor");
    auto k = n.get_ints("kernel_shape");
    auto st = n.get_ints("strides", {1, 1});
    auto pads = n.get_ints("pads", {0, 0, 0, 0});
    const bool cip_avg = n.op_type == "AveragePool" && n.get_int("count_include_pad", 0);
    if ((pads[0] != pads[2] || pads[1] != pads[3]) && cip_avg)
      throw std::runtime_error(n.op_type + " " + n.name + ": count_include_pad with asymmetric pads is not supported");
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
  void lower_gap(int idx, int mode = 0) {
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

  void lower_flatten(int idx) {
    const Node& n = m_.nodes[idx];
    Val x = val(n.in(0), n);
    if (n.op_type == "Flatten" && n.get_int("axis", 1) != 1) throw std::runtime_error("Flatten: axis must be 1");
    if (x.kind == Val::NHWC && x.H * x.W > 1 && n.op_type == "Flatten") {
      define(n.outputs[0], flatten_nhwc(x));
      return;
    }
    if (!((x.kind == Val::ROWS_BF16 || x.kind == Val::NHWC) && x.H == 1 && x.W == 1))
      throw std::runtime_error(n.op_type + " " + n.name + ": only flattening of 1x1 feature maps is supported");
    Val o = x;
    o.kind = Val::ROWS_BF16;
    o.rank = 2;
    define(n.outputs[0], o);
  }

  // [B, C, H, W] -> [B, C*H*W] over an NHWC buffer: a lazy view in (h, w, c) order that only a
  // Gemm/MatMul with an initializer can consume (it permutes its weight rows to match).
  Val flatten_nhwc(const Val& x) const {
    Val o;
    o.kind = Val::ROWS_BF16;
    o.rank = 2;
    o.C = x.H * x.W * x.C;
    o.buf = x.buf;
    o.flat_hw = x.H * x.W;
    o.flat_c = x.logical();
    return o;
  }

  void finalize_output() {
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

  const onnx::Model& m_;
  int max_batch_;
  PlanOptions opt_;
  Plan plan_;
  std::vector<Val> vals_;
  std::unordered_map<std::string, int> vid_;
  std::unordered_map<std::string, std::vector<int>> consumers_;
  std::unordered_set<std::string> graph_outputs_;
  std::unordered_map<std::string, int> producer_;  // value name -> the node writing it
  std::unordered_map<std::string, int> prepped_;
  std::unordered_map<std::string, std::array<int64_t, 4>> folded_pad_;  // Pad output -> (t, l, b, r) for its conv
  std::vector<bool> done_;
  bool output_view_seen_ = false;
};

}  // namespace

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
