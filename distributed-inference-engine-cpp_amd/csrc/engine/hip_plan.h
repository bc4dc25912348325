// Lowering of an ONNX graph to a fused, NHWC/bf16 device program for gfx950: one walk over the
// topologically sorted nodes, with lookahead (Planner, engine/planner.h), then the post-lowering
// passes (engine/plan_passes.h).  What each family of nodes lowers to, and what is rejected with a
// report line, is described at the head of the file that implements it:
//  * hip_plan.cpp             the walk, the dispatch by operand kind and op type, graph inputs / output
//  * plan_lower_image.cpp     convs with their BN / ReLU / residual / dual-store epilogues, pools, pads,
//                             Resize, channels-last blocks (ConvNeXt)
//  * plan_lower_gemm.cpp      Gemm / MatMul(initializer) with bias, GELU and residual epilogues, Q/K/V merge
//  * plan_lower_attention.cpp head views, the attention chain with folded biases / masks, repeat_kv
//                             (grouped-query attention), rotary position embeddings
//  * plan_lower_tokens.cpp    token-id models, attention_mask / token_type_ids inputs, sentence pooling,
//                             ViT token assembly
//  * plan_lower_norm.cpp      LayerNormalization, RMSNorm and their decomposed exports
//  * plan_lower_groupnorm.cpp InstanceNormalization, GroupNormalization and torch's Reshape / InstanceNorm /
//                             Reshape export of GroupNorm, with a trailing ReLU / SiLU
//  * plan_lower_grn.cpp       ConvNeXt-V2's Global Response Normalization: the ReduceL2(two spatial axes) /
//                             ReduceMean / Add / Div / Mul / Mul / Add / Add chain, channels-last or -first
//  * plan_lower_general.cpp   everything else: standalone unary / binary / compare / Where / concat / slice
// Anything the planner cannot lower is rejected with a clear error (the CPU executor still runs such
// models).
#pragma once

#include <cstdint>
#include <stdexcept>
#include <string>
#include <vector>

#include "../kernels/kernels.h"
#include "../onnx/onnx_model.h"

namespace die {

struct PlanBuf {
  size_t bytes_per_sample = 0;  // scaled by the batch size at allocation time
  size_t offset = 0;            // arena offset (max batch), assigned by the planner
  int first_use = -1, last_use = -1;
};

// The pad test of a token-id model: a key is visible iff ((truncated ? trunc(id) : id) OP value) !=
// negated, OP = op (0 Equal, 1 Greater, 2 Less) -- the pad_* arguments of kern::embed_tokens.
// src: what the test reads -- -1 the ids of a single-input model, else the offset in a sample's
// request row of the input it reads (models with several graph inputs): the attention-mask input
// (the test is then "value != 0") or, for a test still derived from ids, that ids input.
struct PadTest {
  int op = 0;
  float value = 0.f;
  bool negated = false, truncated = false;
  int src = -1;
  bool operator==(const PadTest& o) const {
    return op == o.op && value == o.value && negated == o.negated && truncated == o.truncated && src == o.src;
  }
};

struct PlanOp {
  enum Kind {
    INPUT_PREP, CONV, POOL, GAP, AFFINE, TO_NCHW_F32, BF16_TO_F32,
    LAYERNORM, TOKENS, GATHER_ROWS, ATTENTION, STEM, GCONV, SOFTMAX,
    // general path (kernels/generic.hip)
    ROWS_PREP,  // rank-2/3 graph input: f32 [rows][C] -> bf16 rows [rows][Cp]
    COPY_COLS,  // out[:, col[1] + j] = in[:, col[0] + j], j < C (concat / slice); pitches ld[0], ld[1]
    BINARY,     // out = act(in (op gidx) in2); S = 0: same shape, 1: in2 = one row per sample
    UNARY,      // out = act(in * scale + shift) with any activation code
    // ResNet-v2 bottleneck boundary in one launch (kernels/conv_pair.hip): a dual-store 1x1 expand
    // conv fused with the 1x1 reduce conv that is the sole reader of its pre-activation output
    CONV_PAIR,
    PAD,     // NHWC zero padding (ONNX Pad not folded into a conv): out [Ho][Wo] = in [H][W] at (ph, pw),
             // stride sh, sw (zero insertion: ConvTranspose lowered to a stride-1 conv)
    WHERE,   // out = in != 0 ? in2 : in3 (in2 / in3 = -1: the scalars clip_lo / clip_hi)
    RESIZE,  // NHWC Resize: in [H][W] -> out [Ho][Wo]; act = mode, gidx = coord, is_max = nearest mode,
             // clip_lo / clip_hi = scales (output / input)
    BMM,     // batched MatMul of two row activations: out [S][Cp pitch C] = in [S][gidx of ld[0]] x
             // in2 [gidx][ld[1]]; Cp = logical N
    GAP_FC,  // global pool (gidx = mode) of in [H*W][C] + the 1x1 GEMM that is its only reader, in one
             // launch: out_f32 [Cp] = act(pool . w + bias); conv describes the GEMM (Kpad, wplane)
    EMBED_TOKENS,  // token ids (the fp32 graph input [S], in = -2) -> rows: out [S][C] = table[idx(id)] + pos + type
                  // with w_off = table [gidx = V][C] f32, shift_off = pos [S][C], bias_off = type [C] (C = stored
                  // width, Cp = the model's); key data for key-masked attention when out2 >= 0: out2 = kvis
                  // f32 [kern::key_pitch(S)], out3 = kend (one int), from the pad test `pad`.
                  // Several graph inputs (in_ld > 0, kern::EmbedArgs::ld_in): a sample's request row has in_ld
                  // floats, the ids at seg_ids, the type ids at seg_types (>= 0: type_off = their table
                  // [type_rows][C] f32, instead of the constant row bias_off), the mask at pad.src
    POOL_TOKENS,  // rows in [S][C] (Cp logical columns) -> one vector: out [C] (bf16 / split) or out_f32 [Cp] (the
                 // graph output).  key_mask = 1: the mean over the visible tokens, sum / max(count, count_min),
                 // with in4 / in5 = the EMBED_TOKENS op's kvis / kend; else the mean of all S rows.
                 // normalize: then v / max(||v||_2, eps).  S = 1, normalize: a row L2 normalisation
    ROPE,  // rotary position embedding (rotate-half) of the nh heads of hd columns at in [S][ld[0]] + col[0] ->
           // dense rows out [S][nh*hd]; scale_off / shift_off = the cos / sin tables [S][hd] f32
           // (kern::rope_rows); gidx = the layout the graph rotated in (0: [N, H, S, hd], 1: [N, S, H, hd])
    GROUPNORM,  // GroupNorm / InstanceNorm of the image in [H][W][C] (Cp logical channels) over `groups` groups
                // (groups = Cp: InstanceNorm): out = act((in - mean) * rstd * gamma + beta), scale_off /
                // shift_off = gamma / beta [Cp] f32 (SIZE_MAX: none), act 0 none, 1 ReLU, 2 SiLU, eps;
                // out2 = the launch's workspace (kern::group_norm_workspace_bytes per sample)
    GRN  // Global Response Normalization of the map in [H * W][C] (dense, no pad channels; an image or an
         // [N, H, W, C] rows view of one): out = gamma * (in * nx) + beta + in with nx = G / (mean_c G + eps),
         // G[c] = the L2 norm of channel c over the map; scale_off / shift_off = gamma / beta [C] f32
         // (SIZE_MAX: none); out2 = the launch's workspace (kern::grn_workspace_bytes per sample)
  } kind;
  std::string name;
  // buffers (-1 = none).  -2 = the graph input (f32 NCHW), -3 = the graph output (f32).
  int in = -1, in2 = -1, in3 = -1, out = -1, out2 = -1, out_f32 = -1;
  int out3 = -1;  // CONV_PAIR: the pre-activation `a` when ops other than the fused reduce conv read it
  // parameter offsets (bytes) into the device parameter blob
  size_t w_off = 0, bias_off = SIZE_MAX, s2_off = SIZE_MAX, b2_off = SIZE_MAX, scale_off = SIZE_MAX,
         shift_off = SIZE_MAX;
  // conv geometry (per sample; ConvArgs B/M are set at launch)
  kern::ConvArgs conv;
  int tile_bmax = 0;
  // generic geometry
  int C = 0, H = 0, W = 0, Ho = 0, Wo = 0, Cp = 0;
  int kh = 0, kw = 0, sh = 1, sw = 1, ph = 0, pw = 0, is_max = 0, cip = 0, act = 0;
  // stored row pitch when it differs from the logical channel count C (padded channels; 0 = C):
  // BF16_TO_F32 / TO_NCHW_F32 drop the pad columns, SOFTMAX reads and writes rows of this pitch
  int ld_store = 0;
  int groups = 1;                      // GCONV
  // GCONV in the scope of the tiled depthwise kernel (kern::dwconv_tiled: depthwise, stride 1,
  // dilation 1, 5x5 / 7x7): tiled = 1 and tap_w_off = the same weights as fp32 [tap][C]; the engine
  // picks the kernel (EngineOptions::tiled_dwconv), w_off stays valid for kern::grouped_conv
  int tiled = 0;
  size_t tap_w_off = SIZE_MAX;
  float clip_lo = 0.f, clip_hi = 0.f;  // act == 3 (Clip) of AFFINE / GCONV
  long long rows_per_sample = 0;  // AFFINE / LAYERNORM: rows of C per sample
  // transformer ops: sequence length, heads, head dim, column offsets / pitches of in/in2/in3
  int S = 0, nh = 0, hd = 0, gidx = 0;
  int col[3] = {0, 0, 0}, ld[3] = {0, 0, 0};
  float fscale = 1.f, eps = 0.f;
  // ATTENTION with a folded bias / mask: bias_off = fp32 table [bias_heads][S][kern::key_pitch(S)] in
  // the kernel's exp2 units (kern::attention), bias_heads = 0 (none), 1 (shared) or nh; causal = 1:
  // key j visible to query i iff j <= i
  int bias_heads = 0, causal = 0;
  // ATTENTION with the request's key (padding) mask: in4 / in5 = the kvis / kend buffers of the plan's
  // EMBED_TOKENS op (kern::attention); combines with a bias table, never with causal
  int key_mask = 0, in4 = -1, in5 = -1;
  // ATTENTION: heads stored in in2 / in3 (K / V).  nh: every query head its own; a divisor of nh:
  // grouped-query attention, query head h reads stored head h / (nh / kv_heads) (kern::attention)
  int kv_heads = 0;
  PadTest pad;            // EMBED_TOKENS writing key data (out2 >= 0)
  int in_ld = 0, seg_ids = 0, seg_types = -1, type_rows = 0;  // EMBED_TOKENS of a model with several graph inputs
  size_t type_off = SIZE_MAX;
  bool normalize = false;  // POOL_TOKENS
  float count_min = 0.f;   // POOL_TOKENS with key_mask: lower bound of the count of visible tokens
  double flops_per_sample = 0;
  // Side branch: this op may run on a second stream, concurrently with the ops after it, until
  // op `join` (its first consumer) waits for it.  The arena keeps its inputs live until `join`.
  int join = -1;
  // CONV_PAIR: in = expand input [M][K1], in2 = residual, out = raw sum x (-1: not stored), out2 =
  // reduce output [M][n2]; conv/w_off/bias_off/s2_off/b2_off describe the expand conv and the BN of
  // the pre-activation, w2_off/bias2_off/w2plane/pair_relu the reduce conv.  Both weight matrices
  // have their rows permuted by kern::pair_permute_row.
  size_t w2_off = 0, bias2_off = SIZE_MAX;
  long long w2plane = 0;
  int n2 = 0, pair_relu = 0;
  // LayerNorm folded into its GEMM readers (EngineOptions::fold_layernorm): the LAYERNORM op has
  // stats_only = 1 and out = a [rows][2] f32 (mean, rstd) buffer; each reading CONV has in = the
  // LayerNorm's input, in3 = that statistics buffer, gamma folded into its weights, beta into its
  // bias and colsum_off = the per-column sums of its weights (ConvArgs::row_stats / col_sum).
  int stats_only = 0;
  int rms = 0;  // LAYERNORM: RMSNorm (no mean, no beta); never folded into its readers
  size_t colsum_off = SIZE_MAX;
  // LayerNorm statistics from the producer's epilogue (stats_from_producer): the CONV that writes a
  // statistics-only LayerNorm's input also writes out_stats = the [M][N/64] (mean, M2) column-group
  // partials (ConvArgs::stats_out), the LayerNorm op is gone, and its folded readers have
  // in3 = out_stats, in3_parts = 1 (ConvArgs::row_parts) and eps = the LayerNorm's epsilon.
  int out_stats = -1;
  int in3_parts = 0;
};

// An EMBED_TOKENS op whose key data comes from an attention-mask input (not from an ids input)
inline bool pad_reads_mask(const PlanOp& o) {
  return o.out2 >= 0 && o.pad.src >= 0 && o.pad.src != o.seg_ids && o.pad.src != o.seg_types;
}

struct Plan {
  std::vector<PlanOp> ops;
  std::vector<PlanBuf> bufs;
  std::vector<uint8_t> params;  // host copy of the packed device parameters
  size_t arena_bytes_per_sample = 0;  // sum of per-sample sizes at the chosen offsets (scaled by Bmax)
  size_t arena_bytes = 0;             // for max_batch
  std::vector<int64_t> input_shape;   // [1, C, H, W]; K token inputs [N, S]: [1, K, S]
  // the graph inputs as segments of a request row, roles as the planner bound them
  std::vector<onnx::InputSegment> inputs;
  std::vector<int64_t> output_shape;  // [1, ...]
  size_t input_numel = 0, output_numel = 0;
  double flops_per_sample = 0;
  // fp32 mode: every activation buffer holds split (hi, lo) bf16 planes (kernels/common.h), GEMM
  // weights are packed as hi + lo planes, and every kernel runs its split variant.
  bool split = false;
  std::string summary() const;
};

// "conv", "layernorm", ...: the name of an op kind in summaries and profiles
const char* plan_kind_name(PlanOp::Kind kind);

// Thrown by build_plan for a graph with nodes the HIP planner cannot lower (what() lists them all):
// the engine factory's cue for the hybrid HIP + CPU partition (engine.cpp create_engine).
struct PlanUnsupported : std::runtime_error {
  using std::runtime_error::runtime_error;
};

struct PlanOptions {
  bool side_branches = false;  // mark independent convs to run on a second stream (PlanOp::join; extends
                               // their inputs' lifetimes)
  bool split = false;          // fp32 mode (Plan::split)
  // the post-lowering passes, each named after its EngineOptions member
  bool fuse_pairs = true;         // expand -> reduce 1x1 conv pairs become CONV_PAIR ops
  bool fuse_stem_pool = true;     // stem conv + max pool in one STEM op
  bool fuse_gap_fc = false;       // global pool + the FC head reading it in one GAP_FC op
  bool fold_layernorm = true;     // LayerNorms read only by GEMMs become statistics ops (fp32 mode only)
  bool ln_stats_epilogue = true;  // ... and those statistics come from the epilogue of the GEMM
                                  // producing the LayerNorm's input where one does
};

// Build the plan for batches up to max_batch.  Throws PlanUnsupported on unsupported graphs, listing EVERY node
// the engine cannot lower (not only the first).
Plan build_plan(const onnx::Model& m, int max_batch, const PlanOptions& opt = {});

// Load-time support report: which nodes the HIP planner cannot lower, and why.  `blocked` counts
// nodes not tried because an input came from an unsupported node.
struct PlanReport {
  bool supported = true;
  struct Item {
    std::string node, op, error;
  };
  std::vector<Item> unsupported;
  int blocked = 0;
  std::string text() const;  // one line per unsupported node
};
PlanReport plan_report(const onnx::Model& m, int max_batch = 8, bool split = false);

}  // namespace die
