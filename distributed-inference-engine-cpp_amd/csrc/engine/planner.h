// The lowering walk's state and the table of contents of its methods.  Internal to the planner's
// translation units (hip_plan.cpp and plan_lower_*.cpp), like plan_passes.h; the contract with the
// rest of the engine is hip_plan.h.
#pragma once

#include "hip_plan.h"

#include "plan_passes.h"

#include <algorithm>
#include <array>
#include <climits>
#include <cmath>
#include <cstring>
#include <map>
#include <sstream>
#include <stdexcept>
#include <unordered_map>
#include <unordered_set>

namespace die {

using onnx::Node;
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

inline int round8(int c) { return (c + 7) / 8 * 8; }

class Planner {
 public:
  Planner(const onnx::Model& m, int max_batch, const PlanOptions& opt)
      : m_(m), max_batch_(max_batch), opt_(opt) {}

  // Every node is tried; a node that cannot be lowered is recorded (with its error) and its
  // outputs become UNKNOWN, so the walk goes on and the report lists every unsupported node.
  PlanReport report_;
  Plan run();

 private:
  // How a graph input is used, through Casts: as the indices of a Gather, and / or in any other way
  // (`mask_like`: every such other use is one a key mask flows through or ends in).
  struct InputUse {
    bool gathered = false, other = false, mask_like = true;
    std::string other_node;
  };
  // What gemm_tail found behind a MatMul / Gemm to fold into its epilogue
  struct GemmTail {
    std::vector<float> bias;  // from a following Add(initializer), empty if none
    int act = 0;              // 1 relu, 2 gelu
    std::string res;          // residual operand (rows; image = true: an NHWC image)
    std::vector<float> colscale;  // from a following Mul(initializer [N]) (layer scale), empty if none
    bool image = false;       // the tail went through Transpose(0,3,1,2): the output is the NHWC image of the view
    std::string out;
    std::vector<int> used;
  };
  // The folded bias / mask table of an attention (plan_lower_attention.cpp)
  struct AttnTable {
    int heads = 1;         // 1 (shared) or nh
    std::vector<float> t;  // [heads][S][S]
  };

  // ---- helpers (inline) -----------------------------------------------------------------------
  const onnx::Tensor& init(const std::string& name, const Node& n) const {
    auto it = m_.initializers.find(name);
    if (it == m_.initializers.end()) reject(n, "input " + name + " must be an initializer");
    return it->second;
  }
  bool is_init(const std::string& name) const { return m_.initializers.count(name) != 0; }
  Val& val(const std::string& name, const Node& n) {
    auto it = vid_.find(name);
    if (it == vid_.end()) reject(n, "unknown input value " + name);
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
  // The sole not-yet-consumed consumer of `value` if it is an `op_type` node, else -1 (chain walking)
  int next_op(const std::string& value, const char* op_type) const {
    const int c = sole_consumer(value);
    return c >= 0 && m_.nodes[c].op_type == op_type ? c : -1;
  }
  // The report line of a node that cannot be lowered: "<op_type> <name>: <why>"
  [[noreturn]] void reject(const Node& n, const std::string& why) const {
    throw std::runtime_error(n.op_type + " " + n.name + ": " + why);
  }
  // A new bf16 buffer for an activation of x's shape, and the value `name` = x in the buffer `buf`
  // (clear_affine: without x's pending affine flag)
  int buf_like(const Val& x) { return new_buf(static_cast<size_t>(x.H) * x.W * x.C * 2); }
  void same_shape(const std::string& name, const Val& x, int buf, bool clear_affine = false) {
    define(name, x);
    vals_.back().buf = buf;
    if (clear_affine) vals_.back().has_affine = false;
  }
  static const std::string& other_input(const Node& nd, const std::string& x) { return nd.in(0) == x ? nd.in(1) : nd.in(0); }
  static bool dense(const Val& v) { return (v.kind == Val::NHWC || v.kind == Val::ROWS_BF16) && v.pitch() == v.C && !v.col && !v.flat_hw; }
  static long long rows_of(const Val& v) { return static_cast<long long>(v.H) * v.W; }

  // ---- the lowering methods, by the file that defines them ---------------------------------------
  // ---- hip_plan.cpp ----
  void mark_unknown(const Node& n);
  void define_graph_input();
  InputUse input_use(const std::string& name) const;
  void define_token_inputs();
  bool reports_own_input(const Node& n) const;
  void lower(int idx);
  void check_output_view(const Node& n);
  void finalize_output();

  // ---- plan_lower_image.cpp ----
  void bn_affine(const Node& bn, std::vector<float>& sc, std::vector<float>& sh);
  int ensure_nhwc_input(Val& x, const std::string& name);
  Val materialize_in(const std::string& name, const Node& n);
  void lower_conv(int idx);
  bool clip_bounds(const Node& n, float& lo, float& hi) const;
  int take_act(std::string& cur, float& lo, float& hi);
  void lower_gconv(int idx);
  void lower_clip(int idx);
  bool lower_spatial_reduce(int idx, int mode);
  std::vector<int64_t> conv_pads(const Node& n) const;
  void lower_pad(int idx);
  void emit_pad(const Node& n, const Val& x, const std::array<int64_t, 4>& tlbr, int sy, int sx);
  void lower_resize(int idx);
  void lower_bn(int idx);
  void lower_relu(int idx);
  void lower_add(int idx);
  void standalone_affine(const Node& n, const Val& x, const std::vector<float>* sc, const std::vector<float>* sh,
                         const Val* z, int own_act = 0, float own_lo = 0.f, float own_hi = 0.f);
  void lower_pool(int idx);
  void lower_gap(int idx, int mode = 0);
  void lower_flatten(int idx);
  Val flatten_nhwc(const Val& x) const;

  // ---- plan_lower_gemm.cpp ----
  bool scalar_is(const std::string& name, float want) const;
  bool match_gelu(const std::string& v, std::vector<int>& used, std::string& out) const;
  GemmTail gemm_tail(const Node& n, int N, int rows, bool is_gemm, int N_logical, const Val& x) const;
  std::vector<int> qkv_group(int idx, const std::string& xname, int K) const;
  void lower_gemm(int idx);

  // ---- plan_lower_attention.cpp ----
  bool node_axes(const Node& n, std::vector<int64_t>& ax) const;
  bool ints_of(const std::string& nm, std::vector<int64_t>& out) const;
  bool lower_shape_op(int idx);
  bool kv_repeat_node(const Node& n) const;
  void lower_kv_repeat(int idx);
  bool attn_mask_node(const Node& n) const;
  AttnTable attn_table(const Val& x, int heads) const;
  void define_masked(const Node& n, const Val& x, AttnTable t);
  void lower_attn_mask(const Node& n, const Val& x, const std::string& tname, int mode);
  int emit_attention(const Val& ctx, const std::string& name);
  void lower_reshape(int idx);
  void lower_transpose(int idx);
  void lower_attn_matmul(int idx);
  void lower_scale(int idx);
  void lower_softmax(int idx);
  static int rope_layout(const Val& v);
  int rope_operand(const Node& n) const;
  bool rope_anchor(const Node& n) const;
  bool slice_range(const Node& n, int64_t& s0, int64_t& e0, int64_t& axis, int64_t& step) const;
  std::vector<float> rope_table(const Node& at, const std::string& name, const Val& x, int layout) const;
  void lower_rope(int idx);
  void check_score_fill(const Node& n, const std::string& fill) const;

  // ---- plan_lower_tokens.cpp ----
  bool token_input(const std::string& name) const;
  bool token_node(const Node& n) const;
  const Val* val_if(const std::string& name, Val::Kind kind) const;
  const Val* ids_behind(std::string name) const;
  void lower_token_node(int idx);
  void lower_embed(int idx);
  void define_key_masked(const Node& n, const Val& x, const Val& m, bool vis_when_true);
  void bind_key_test(const std::string& who, const Val& m, bool vis_when_true);
  bool masked_sum_shape(const std::string& name) const;
  bool lower_pool_node(int idx);
  bool l2_chain(int ridx, int rank, float& eps, std::string& out, std::vector<int>& used, std::string& why,
                int& shape_node) const;
  bool only_l2_normalized(const std::string& x, float& eps, std::string& out, std::vector<int>& used) const;
  void lower_l2norm(int idx);
  void emit_pool_tokens(const Node& n, const Val& x, int S, const Val* vis, float clip_min, std::string out_name,
                        bool try_norm, bool normalize, float eps);
  void lower_gather(int idx);
  void lower_concat(int idx);
  void emit_tokens(const Node& n, const Val& cat, const std::string* pos_name, const std::string& out_name);

  // ---- plan_lower_norm.cpp ----
  void emit_layernorm(const std::string& name, const Val& x, const std::vector<float>& gamma,
                      const std::vector<float>& beta, float eps, bool rms, int Cp, const std::string& out_name,
                      bool clear_affine = false);
  void lower_layernorm(int idx);
  bool rmsnorm_anchor(const Node& n) const;
  void lower_rmsnorm(int idx);
  static int64_t last_axis_of(const Node& n, const onnx::Model& m, bool& ok);
  void lower_reduce_mean(int idx);

  // ---- plan_lower_groupnorm.cpp ----
  bool groupnorm_anchor(const Node& n) const;
  void lower_groupnorm_chain(int idx);
  void lower_groupnorm(int idx);
  void emit_groupnorm(const Node& n, const std::string& name, const Val& x, int G, std::vector<float> gamma,
                      std::vector<float> beta, float eps, std::string cur);

  // ---- plan_lower_grn.cpp ----
  bool grn_anchor(const Node& n) const;
  void lower_grn(int idx);

  // ---- plan_lower_general.cpp ----
  bool scalar_init(const std::string& name, float& v) const;
  void lower_compare(int idx);
  void lower_where(int idx);
  void lower_cast(int idx);
  void emit_channel_slice(const Node& n, const Val& x, int64_t s0, int64_t e0, const std::string& out);
  void lower_split(int idx);
  void lower_slice(int idx);
  void lower_unary(int idx);
  void emit_unary(const Node& n, const Val& x, int act, float a, float b, const std::string& out_name);
  bool lower_binary_acts(const Node& n);
  static bool is_channel_axis(const Val& v, int64_t axis);
  void general_concat(const Node& n, int64_t axis);

  // ---- state ----
  // The first EMBED_TOKENS op of the plan also writes the key data (kvis, kend) every key-masked
  // attention reads; one pad test per model.
  int key_op_ = -1;           // index of that op; its out2 / out3 = kvis / kend once a mask uses them
  bool key_test_set_ = false;
  std::vector<AttnTable> masks_;  // indexed by Val::mask (a Val is copied by value everywhere)
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

}  // namespace die
