#include "plan_passes.h"

#include <algorithm>

namespace die {
namespace passes {

int new_buf(Plan& plan, size_t bytes_per_sample) {
  PlanBuf b;
  b.bytes_per_sample = bytes_per_sample * (plan.split ? 2 : 1);
  plan.bufs.push_back(b);
  return static_cast<int>(plan.bufs.size()) - 1;
}
size_t push_f32(Plan& plan, const std::vector<float>& v) {
  size_t off = round_up(plan.params.size(), 256);
  plan.params.resize(off + round_up(v.size(), 128) * 4, 0);
  std::memcpy(plan.params.data() + off, v.data(), v.size() * 4);
  return off;
}
size_t push_bf16(Plan& plan, const std::vector<uint16_t>& v) {
  size_t off = round_up(plan.params.size(), 256);
  plan.params.resize(off + v.size() * 2);
  std::memcpy(plan.params.data() + off, v.data(), v.size() * 2);
  return off;
}

namespace {

// GEMM weights in the parameter blob: [n][kpad] bf16, in fp32 mode the lo plane `plane` elements on.
double weight_at(const Plan& plan, size_t w_off, long long plane, int kpad, int n, int k) {
  const uint16_t* w = reinterpret_cast<const uint16_t*>(plan.params.data() + w_off);
  const size_t i = static_cast<size_t>(n) * kpad + k;
  double v = from_bf16(w[i]);
  if (plane > 0) v += from_bf16(w[i + plane]);
  return v;
}
void set_weight(Plan& plan, size_t w_off, long long plane, int kpad, int n, int k, float v) {
  uint16_t* w = reinterpret_cast<uint16_t*>(plan.params.data() + w_off);
  const size_t i = static_cast<size_t>(n) * kpad + k;
  const uint16_t hi = to_bf16(v);
  w[i] = hi;
  if (plane > 0) w[i + plane] = to_bf16(v - static_cast<float>(from_bf16(hi)));
}
// Rows of a weight matrix permuted in place by kern::pair_permute_row.
void permute_weight_rows(Plan& plan, size_t off, int rows, int kpad, long long plane) {
  const int planes = plane > 0 ? 2 : 1;
  std::vector<uint16_t> tmp(static_cast<size_t>(rows) * kpad);
  for (int pl = 0; pl < planes; ++pl) {
    uint16_t* w = reinterpret_cast<uint16_t*>(plan.params.data() + off) + static_cast<size_t>(pl) * plane;
    std::memcpy(tmp.data(), w, tmp.size() * 2);
    for (int n = 0; n < rows; ++n)
      std::memcpy(w + static_cast<size_t>(kern::pair_permute_row(n)) * kpad, tmp.data() + static_cast<size_t>(n) * kpad,
                  static_cast<size_t>(kpad) * 2);
  }
}
bool plain_1x1(const kern::ConvArgs& c) {
  return c.KH == 1 && c.KW == 1 && c.stride == 1 && c.pad_h == 0 && c.pad_w == 0 && c.dil == 1 && c.H == c.Ho &&
         c.W == c.Wo && c.K == c.Cin && c.Kpad == c.K;
}

}  // namespace

// Pool -> BN(+ReLU) where the pooled value has no other reader (ResNet-v2: the stem's max pool
// feeds only stage 1's pre-activation BN, the first unit having a projection shortcut): the pool
// kernel applies the per-channel affine and activation before its single store.
void fuse_pool_affine(Plan& plan) {
  std::vector<int> readers(plan.bufs.size(), 0);
  for (const PlanOp& p : plan.ops)
    for (int b : {p.in, p.in2, p.in3})
      if (b >= 0) readers[b]++;
  std::vector<PlanOp> out;
  out.reserve(plan.ops.size());
  for (size_t i = 0; i < plan.ops.size(); ++i) {
    PlanOp& p = plan.ops[i];
    if (p.kind == PlanOp::AFFINE && p.in2 < 0 && p.in >= 0 && readers[p.in] == 1 && !out.empty() &&
        out.back().kind == PlanOp::POOL && out.back().out == p.in && out.back().scale_off == SIZE_MAX &&
        out.back().act == 0 && p.rows_per_sample == static_cast<long long>(out.back().Ho) * out.back().Wo) {
      PlanOp& pool = out.back();
      pool.scale_off = p.scale_off;
      pool.shift_off = p.shift_off;
      pool.act = p.act;
      pool.out = p.out;
      pool.name += "+" + p.name;
      continue;
    }
    out.push_back(std::move(p));
  }
  plan.ops = std::move(out);
}

// Stem -> 3x3/2 max pool (pad 1) [-> the pooled value's BN/ReLU, fuse_pool_affine] where the stem
// map has no other reader: one STEM op with is_max = 1 (kernels/stem.hip stem_pool_nchw_kernel);
// the stem map is never stored.  Ho/Wo become the pooled size, s2_off/b2_off/act the pool's affine.
void fuse_stem_pool(Plan& plan) {
  std::vector<int> readers(plan.bufs.size(), 0);
  for (const PlanOp& p : plan.ops)
    for (int b : {p.in, p.in2, p.in3})
      if (b >= 0) readers[b]++;
  std::vector<PlanOp> out;
  out.reserve(plan.ops.size());
  for (size_t i = 0; i < plan.ops.size(); ++i) {
    PlanOp& p = plan.ops[i];
    if (p.kind == PlanOp::POOL && p.is_max && p.kh == 3 && p.kw == 3 && p.sh == 2 && p.sw == 2 && p.ph == 1 &&
        p.pw == 1 && p.act <= 1 && p.C == 64 && p.in >= 0 && readers[p.in] == 1 && !out.empty()) {
      PlanOp& s = out.back();
      const auto& c = s.conv;
      if (s.kind == PlanOp::STEM && s.in == kBufGraphIn && !s.is_max && s.out == p.in && c.Ho == p.H && c.Wo == p.W &&
          kern::stem_pool_supported(c.H, c.W, c.Ho, c.Wo, p.Ho, p.Wo, plan.split)) {
        permute_weight_rows(plan, s.w_off, 64, 224, c.wplane);
        s.is_max = 1;
        s.Ho = p.Ho;
        s.Wo = p.Wo;
        s.s2_off = p.scale_off;
        s.b2_off = p.shift_off;
        s.act = p.act;
        s.out = p.out;
        s.name += "+" + p.name;
        continue;
      }
    }
    out.push_back(std::move(p));
  }
  plan.ops = std::move(out);
}

// Global pool -> the FC head (Gemm / 1x1 conv over the pooled [C] vector) that is its ONLY reader,
// with an fp32 output (a buffer or the graph output, directly or through a BF16_TO_F32 op) and no
// residual / second output: one GAP_FC op at the pool's position
// (kernels/misc.hip gap_fc_kernel); the pooled vector is never stored.
void fuse_gap_fc(Plan& plan, int max_batch) {
  std::vector<int> readers(plan.bufs.size(), 0), reader_op(plan.bufs.size(), -1);
  const int nops = static_cast<int>(plan.ops.size());
  for (int i = 0; i < nops; ++i)
    for (int b : {plan.ops[i].in, plan.ops[i].in2, plan.ops[i].in3})
      if (b >= 0) {
        readers[b]++;
        reader_op[b] = i;
      }
  std::vector<bool> drop(nops, false);
  for (int i = 0; i < nops; ++i) {
    PlanOp& p = plan.ops[i];
    if (p.kind != PlanOp::GAP || p.out < 0 || p.out2 >= 0 || p.out_f32 != -1 || p.join >= 0 || p.in < 0 ||
        readers[p.out] != 1)
      continue;
    const int j = reader_op[p.out];
    if (j <= i || drop[j]) continue;
    const PlanOp& q = plan.ops[j];
    const kern::ConvArgs& c = q.conv;
    if (q.kind != PlanOp::CONV || q.in != p.out || q.in2 >= 0 || q.in3 >= 0 || q.out2 >= 0 || q.join >= 0 ||
        c.relu > 1 || c.KH != 1 || c.KW != 1 || c.H != 1 || c.W != 1 || c.Cin != p.C || c.K != p.C)
      continue;
    // the f32 logits come from the conv itself, or (N % 8 != 0) from the BF16_TO_F32 op that is
    // the only reader of its bf16 output -- the fused op writes them directly, in fp32
    int conv_out = -1, nout = c.N, k = -1;
    if (q.out_f32 != -1 && q.out < 0) {
      conv_out = q.out_f32;
    } else if (q.out_f32 == -1 && q.out >= 0 && readers[q.out] == 1) {
      k = reader_op[q.out];
      const PlanOp& r = plan.ops[k];
      if (k <= j || drop[k] || r.kind != PlanOp::BF16_TO_F32 || r.in != q.out || r.out_f32 == -1 || r.join >= 0 ||
          (r.ld_store > 0 && r.rows_per_sample != 1) || r.C > c.N)
        continue;
      conv_out = r.out_f32;
      nout = r.C;
    } else {
      continue;
    }
    if (!kern::gap_fc_slice(p.C, max_batch, nout, kern::kSplitKWorkspaceBytes)) continue;
    p.kind = PlanOp::GAP_FC;
    p.name += "+" + q.name;
    p.conv = c;
    p.Cp = nout;  // logits per sample (= the f32 row pitch)
    p.w_off = q.w_off;
    p.bias_off = q.bias_off;
    p.act = c.relu;
    p.out = -1;  // the pooled buffer is dropped (no op references it any more)
    p.out_f32 = conv_out;
    p.flops_per_sample += q.flops_per_sample;
    drop[j] = true;
    if (k >= 0) drop[k] = true;
  }
  std::vector<PlanOp> out;
  out.reserve(plan.ops.size());
  for (int i = 0; i < nops; ++i)
    if (!drop[i]) out.push_back(std::move(plan.ops[i]));
  plan.ops = std::move(out);
}

// LayerNorm -> GEMMs (ViT / BERT pre-norm blocks: the norm feeds the QKV or the first MLP GEMM
// only).  LN(x) W + b = rstd (x (gamma W) - mean colsum(gamma W)) + (beta W + b) per row, so the
// GEMMs read x itself with gamma folded into their weights, beta into their bias, and apply the
// per-row (mean, rstd) in the epilogue (ConvArgs::row_stats); the LayerNorm only computes the
// statistics -- the normalised rows are never written or read.  Exact in real arithmetic; in
// fp32 the error grows with |mean| / std of a row (ViT residual rows: mean ~ 0).
void fold_layernorm(Plan& plan) {
  const int nops = static_cast<int>(plan.ops.size());
  std::vector<std::vector<int>> readers(plan.bufs.size());
  for (int i = 0; i < nops; ++i)
    for (int b : {plan.ops[i].in, plan.ops[i].in2, plan.ops[i].in3})
      if (b >= 0) readers[b].push_back(i);
  for (int i = 0; i < nops; ++i) {
    PlanOp& p = plan.ops[i];
    if (p.kind != PlanOp::LAYERNORM || p.rms || p.stats_only || p.out < 0 || p.in < 0 || p.C != p.Cp || p.join >= 0 ||
        readers[p.out].empty())
      continue;
    bool ok = true;
    for (int j : readers[p.out]) {
      const PlanOp& q = plan.ops[j];
      const kern::ConvArgs& c = q.conv;
      ok = ok && j > i && q.kind == PlanOp::CONV && q.in == p.out && q.in2 != p.out && q.in3 < 0 && q.join < 0 &&
           c.KH == 1 && c.KW == 1 && c.stride == 1 && c.pad_h == 0 && c.pad_w == 0 && c.K == p.C && c.Cin == p.C &&
           c.Kpad == c.K && c.Ho * c.Wo == p.rows_per_sample;
    }
    if (!ok) continue;
    const float* gamma = reinterpret_cast<const float*>(plan.params.data() + p.scale_off);
    const float* beta = reinterpret_cast<const float*>(plan.params.data() + p.shift_off);
    const std::vector<float> g(gamma, gamma + p.C), be(beta, beta + p.C);
    const int stats = new_buf(plan, static_cast<size_t>(p.rows_per_sample) * 2 * 4);
    for (int j : readers[p.out]) {
      PlanOp& q = plan.ops[j];
      const kern::ConvArgs& c = q.conv;
      const int Npad = static_cast<int>(round_up(c.N, 128));
      std::vector<float> bias(Npad, 0.f), colsum(round_up(c.N, 8), 0.f);
      if (q.bias_off != SIZE_MAX) {
        const float* b0 = reinterpret_cast<const float*>(plan.params.data() + q.bias_off);
        std::copy(b0, b0 + c.N, bias.begin());
      }
      for (int n = 0; n < c.N; ++n) {
        double bsum = bias[n], csum = 0.0;
        for (int k = 0; k < c.K; ++k) {
          const double w = weight_at(plan, q.w_off, c.wplane, c.Kpad, n, k);
          bsum += static_cast<double>(be[k]) * w;
          set_weight(plan, q.w_off, c.wplane, c.Kpad, n, k, static_cast<float>(w * g[k]));
          csum += weight_at(plan, q.w_off, c.wplane, c.Kpad, n, k);  // what the GEMM multiplies by
        }
        bias[n] = static_cast<float>(bsum);
        colsum[n] = static_cast<float>(csum);
      }
      bias.resize(round_up(c.N, 8));
      q.bias_off = push_f32(plan, bias);
      q.colsum_off = push_f32(plan, colsum);
      q.conv.bias = nullptr;
      q.in = p.in;
      q.in3 = stats;
      q.name = p.name + "+" + q.name;
    }
    p.stats_only = 1;
    p.out = stats;
  }
}

// Statistics-only LayerNorm whose input is the stored output of a rows GEMM (ViT pre-norm
// blocks: the attention-out and MLP2 GEMMs, residual add in their epilogue) -> deleted.  That GEMM
// also writes per-(row, 64-column group) (mean, M2) partials from the values it holds in registers
// (ConvArgs::stats_out), and every block of a folded reader merges its rows' groups in a fixed
// order while its first operand tiles load (ConvArgs::row_parts): no launch, no re-read of the rows.
// The block-0 LayerNorm's input comes from the token assembly, which emits the same partials.
void stats_from_producer(Plan& plan) {
  const int nops = static_cast<int>(plan.ops.size());
  std::vector<std::vector<int>> readers(plan.bufs.size());
  for (int i = 0; i < nops; ++i)
    for (int b : {plan.ops[i].in, plan.ops[i].in2, plan.ops[i].in3})
      if (b >= 0) readers[b].push_back(i);
  std::vector<int> writer(plan.bufs.size(), -1);  // latest op writing each buffer
  std::vector<bool> drop(nops, false);
  for (int i = 0; i < nops; ++i) {
    PlanOp& p = plan.ops[i];
    const int w = p.kind == PlanOp::LAYERNORM && !p.rms && p.stats_only && p.in >= 0 ? writer[p.in] : -1;
    if (w >= 0 && p.C == p.Cp && p.C % 64 == 0 && p.C <= 2048 && p.join < 0) {
      PlanOp& q = plan.ops[w];
      const kern::ConvArgs& c = q.conv;
      // rows GEMM (attention-out / MLP2), or the token assembly (block 0)
      const bool gemm = q.kind == PlanOp::CONV && c.N == p.C && c.Ho * c.Wo == p.rows_per_sample && q.out2 < 0;
      const bool tokens = q.kind == PlanOp::TOKENS && q.C == p.C && q.S + 1 == p.rows_per_sample;
      bool ok = (gemm || tokens) && q.out == p.in && q.out_stats < 0 && q.join < 0;
      for (int j : readers[p.out]) {
        const PlanOp& r = plan.ops[j];
        ok = ok && j > i && r.kind == PlanOp::CONV && r.in3 == p.out && r.colsum_off != SIZE_MAX &&
             r.conv.N % 8 == 0 && r.conv.K == p.C && r.join < 0;
      }
      if (ok && !readers[p.out].empty()) {
        const int st = new_buf(plan, static_cast<size_t>(p.rows_per_sample) * (p.C / 64) * 2 * 4);
        q.out_stats = st;
        q.name += "+stats";
        for (int j : readers[p.out]) {
          PlanOp& r = plan.ops[j];
          r.in3 = st;
          r.in3_parts = 1;
          r.eps = p.eps;
        }
        drop[i] = true;
      }
    }
    for (int b : {p.out, p.out2, p.out3, p.out_f32})
      if (b >= 0) writer[b] = i;
  }
  std::vector<PlanOp> out;
  out.reserve(plan.ops.size());
  for (int i = 0; i < nops; ++i)
    if (!drop[i]) out.push_back(std::move(plan.ops[i]));
  plan.ops = std::move(out);
}

// Back-to-back 1x1 pair (ResNet-v2 bottleneck boundary).  A dual-store expand conv P writes the
// raw sum x (next residual) and a = act(bn(x)); when a's ONLY reader is a plain 1x1/s1 reduce conv
// Q, both become one CONV_PAIR op at P's position (Q has no other input, so computing it early is
// safe) and `a` is never stored: kernels/conv_pair.hip consumes it from LDS.  Rows of both weight
// matrices are permuted in place (kern::pair_permute_row) -- P and Q exist only inside the pair.
// With other readers of `a` (a stage boundary: the next stage's projection shortcut reads it
// too) the pair also stores a (PlanOp::out3) and those readers keep reading it.
// Reduce widths up to 128: the kernel takes 256 (stage 2 -> 3) but at one block per CU it is
// faster than the two convs only at small batches (B=20: 43.3 vs 51.1 us; B=32: 76.4 vs 69.1).
constexpr int kMaxPairN2 = 128;
void fuse_conv_pairs(Plan& plan) {
  const int nops = static_cast<int>(plan.ops.size());
  std::vector<std::vector<int>> readers(plan.bufs.size());
  for (int i = 0; i < nops; ++i)
    for (int b : {plan.ops[i].in, plan.ops[i].in2, plan.ops[i].in3})
      if (b >= 0) readers[b].push_back(i);
  std::vector<bool> drop(nops, false);
  auto reduce_ok = [&](const PlanOp& p, const PlanOp& q) {
    return q.kind == PlanOp::CONV && q.in == p.out2 && q.in2 < 0 && q.in3 < 0 && q.out >= 0 && q.out2 < 0 &&
           q.out_f32 < 0 && q.conv.relu <= 1 && plain_1x1(q.conv) && q.conv.Cin == p.conv.N &&
           q.conv.H == p.conv.Ho && q.conv.W == p.conv.Wo && q.join < 0 && q.conv.N <= kMaxPairN2 &&
           kern::conv_pair_supported(p.conv.K, p.conv.N, q.conv.N);
  };
  for (int i = 0; i < nops; ++i) {
    PlanOp& p = plan.ops[i];
    if (p.kind != PlanOp::CONV || p.in2 < 0 || p.out2 < 0 || p.s2_off == SIZE_MAX || p.out_f32 >= 0 ||
        p.conv.relu != 0 || !plain_1x1(p.conv) || p.join >= 0)
      continue;
    const std::vector<int>& rd = readers[p.out2];
    int j = -1;
    for (int r : rd)
      if (r > i && !drop[r] && reduce_ok(p, plan.ops[r])) {
        j = r;
        break;
      }
    if (j < 0) continue;
    bool others_ok = true;  // every other reader runs after the pair (at P's position) and reads a as an input
    for (int r : rd)
      if (r != j && (r <= i || plan.ops[r].join >= 0)) others_ok = false;
    if (!others_ok) continue;
    const PlanOp& q = plan.ops[j];
    permute_weight_rows(plan, p.w_off, static_cast<int>(round_up(p.conv.N, 128)), p.conv.Kpad, p.conv.wplane);
    permute_weight_rows(plan, q.w_off, static_cast<int>(round_up(q.conv.N, 128)), q.conv.Kpad, q.conv.wplane);
    p.kind = PlanOp::CONV_PAIR;
    p.name += "+" + q.name;
    p.w2_off = q.w_off;
    p.bias2_off = q.bias_off;
    p.w2plane = q.conv.wplane;
    p.n2 = q.conv.N;
    p.pair_relu = q.conv.relu;
    p.out3 = rd.size() > 1 ? p.out2 : -1;  // a stored for its other readers, else dropped
    p.out2 = q.out;
    p.flops_per_sample += q.flops_per_sample;
    drop[j] = true;
  }
  std::vector<PlanOp> out;
  out.reserve(plan.ops.size());
  for (int i = 0; i < nops; ++i)
    if (!drop[i]) out.push_back(std::move(plan.ops[i]));
  plan.ops = std::move(out);
}

// Branch concurrency: a conv whose output is first consumed two or more ops later (ResNet's
// projection shortcut: consumed as the residual of the unit's expand conv, after the reduce and
// 3x3 convs) is independent of the ops in between.  At serving batch sizes every one of those
// convs is latency-bound and leaves CUs idle, so the engine runs the branch on a second stream
// and joins it at its consumer.  One branch open at a time.
void mark_side_branches(Plan& plan) {
  const int nops = static_cast<int>(plan.ops.size());
  int open_until = -1;
  for (int i = 0; i < nops; ++i) {
    PlanOp& p = plan.ops[i];
    if (i <= open_until || p.kind != PlanOp::CONV || p.out < 0 || p.out_f32 >= 0 || p.out_stats >= 0) continue;
    int j = -1;
    for (int k = i + 1; k < nops && j < 0; ++k) {
      const PlanOp& q = plan.ops[k];
      for (int b : {q.in, q.in2, q.in3})
        if (b >= 0 && (b == p.out || b == p.out2)) j = k;
    }
    if (j < i + 2) continue;
    p.join = j;
    open_until = j;
  }
}

void assign_arena(Plan& plan, int max_batch) {
  const int nops = static_cast<int>(plan.ops.size());
  for (int i = 0; i < nops; ++i) {
    const PlanOp& p = plan.ops[i];
    for (int b : {p.out, p.out2, p.out3, p.out_stats})
      if (b >= 0 && plan.bufs[b].first_use < 0) plan.bufs[b].first_use = i;
    for (int b : {p.in, p.in2, p.in3, p.in4, p.in5, p.out, p.out2, p.out3, p.out_stats})
      if (b >= 0) plan.bufs[b].last_use = std::max(plan.bufs[b].last_use, i);
    // a side branch may still be reading its inputs until its join
    if (p.join >= 0)
      for (int b : {p.in, p.in2, p.in3, p.in4, p.in5})
        if (b >= 0) plan.bufs[b].last_use = std::max(plan.bufs[b].last_use, p.join);
  }
  // Offsets: greedy by size (largest first, each at the lowest offset that does not overlap an
  // already placed buffer whose lifetime intersects its own) -- for ResNet50 this packs the
  // arena ~1.5x tighter than first-fit in program order, which keeps activations + weights inside
  // the 256 MiB Infinity Cache.
  std::vector<int> order;
  for (size_t i = 0; i < plan.bufs.size(); ++i)
    if (plan.bufs[i].first_use >= 0 || plan.bufs[i].last_use >= 0) order.push_back(static_cast<int>(i));
  auto bytes_of = [&](int bi) { return round_up(plan.bufs[bi].bytes_per_sample * max_batch, 256); };
  std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return bytes_of(a) > bytes_of(b); });
  struct Placed {
    size_t off, size;
    int first, last;
  };
  std::vector<Placed> placed;
  size_t top = 0;
  for (int bi : order) {
    PlanBuf& b = plan.bufs[bi];
    const size_t size = bytes_of(bi);
    const int first = b.first_use < 0 ? 0 : b.first_use;
    const int last = std::max(b.last_use, first);
    std::vector<std::pair<size_t, size_t>> busy;  // ranges of lifetime-overlapping buffers
    for (const Placed& q : placed)
      if (q.first <= last && first <= q.last) busy.emplace_back(q.off, q.off + q.size);
    std::sort(busy.begin(), busy.end());
    size_t cand = 0;
    for (const auto& r : busy) {
      if (r.first >= cand + size) break;
      cand = std::max(cand, r.second);
    }
    b.offset = cand;
    placed.push_back(Placed{cand, size, first, last});
    top = std::max(top, cand + size);
  }
  plan.arena_bytes = top;
  double fl = 0;
  for (auto& p : plan.ops) fl += p.flops_per_sample;
  plan.flops_per_sample = fl;
}

}  // namespace passes
}  // namespace die
