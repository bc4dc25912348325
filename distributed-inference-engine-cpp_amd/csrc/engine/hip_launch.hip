// HIP engine: encoding a forward pass -- the frame (table fetch, device decode, the side-branch
// fork / join, per-op events) and launch_op, the switch with one case per PlanOp kind.  A new op
// family adds its case there and nowhere else in the engine.
#include "hip_engine.h"

namespace die {
namespace hip {

void* HipEngine::buf_ptr(int id, int s) {
  Slot& sl = slots_[s];
  if (id == -2) return sl.d_in;
  if (id == -3) return sl.d_out;
  if (id < 0) return nullptr;
  for (size_t k = 0; k < prep_out_ids_.size(); ++k)
    if (prep_out_ids_[k] == id) return sl.d_prep[k];
  return arenas_[s % n_exec_] + plan_.bufs[id].offset;
}
const float* HipEngine::prm_ptr(size_t off) const {
  return off == SIZE_MAX ? nullptr : reinterpret_cast<const float*>(params_ + off);
}

kern::ConvArgs HipEngine::conv_args(const PlanOp& op, int B, int s) {
  kern::ConvArgs a = op.conv;
  a.B = B;
  a.M = B * a.Ho * a.Wo;
  a.x = static_cast<const uint16_t*>(buf_ptr(op.in, s));
  a.w = reinterpret_cast<const uint16_t*>(params_ + op.w_off);
  a.bias = prm_ptr(op.bias_off);
  a.res = static_cast<const uint16_t*>(buf_ptr(op.in2, s));
  a.out = static_cast<uint16_t*>(buf_ptr(op.out, s));
  a.out_f32 = static_cast<float*>(buf_ptr(op.out_f32, s));
  a.scale2 = prm_ptr(op.s2_off);
  a.shift2 = prm_ptr(op.b2_off);
  a.out2 = static_cast<uint16_t*>(buf_ptr(op.out2, s));
  a.zeros = zeros_;
  a.counters = counterss_[s % n_exec_];
  a.counters_n = kCounters;
  a.live = slots_[s].d_lens + live_index();
  const float* in3 = op.in3 >= 0 ? static_cast<const float*>(buf_ptr(op.in3, s)) : nullptr;
  a.row_stats = op.in3_parts ? nullptr : in3;
  a.row_parts = op.in3_parts ? in3 : nullptr;
  a.ln_eps = op.eps;
  a.stats_out = op.out_stats >= 0 ? static_cast<float*>(buf_ptr(op.out_stats, s)) : nullptr;
  a.col_sum = prm_ptr(op.colsum_off);
  return a;
}

void HipEngine::encode_forward(int B, int s, hipStream_t st, const Event* op_events, Part part, size_t range_begin,
                               size_t range_end) {
  const bool ranged = range_begin != SIZE_MAX;
  if (ranged) part = MAIN;
  const size_t op_begin = ranged ? range_begin : part == MAIN ? n_prep_ops_ : 0;
  const size_t op_end = ranged ? range_end : part == PREP ? n_prep_ops_ : plan_.ops.size();
  if (part != MAIN) {  // the slot's table (live batch; decode lens/offsets) from host-coherent memory
    const hipError_t ec = kern::copy_i64(slots_[s].h_lens_dev, slots_[s].d_lens, static_cast<int>(table_len()), st);
    if (ec != hipSuccess) throw std::runtime_error("launch of table fetch failed: " + std::string(hipGetErrorString(ec)));
  }
  if (text_cap_ && part != MAIN) {
    Slot& sl = slots_[s];
    // packed samples (d_lens row 2 >= 0) are expanded in registers by the decode kernels
    const hipError_t e = kern::decode_json_numbers(d_text_, sl.d_lens + max_batch_, text_cap_, sl.d_lens, B, sl.d_in,
                                                   static_cast<long long>(in_numel_), sl.d_status,
                                                   sl.d_status + max_batch_, sl.d_scratch, st, d_packed_,
                                                   d_packed_ ? sl.d_lens + 2 * max_batch_ : nullptr);
    if (e != hipSuccess) throw std::runtime_error("launch of device decode failed: " + std::string(hipGetErrorString(e)));
  }
  if (op_events) HIP_CHECK(hipEventRecord(op_events[0], st));
  const hipStream_t main_st = st;
  const long long* live = use_live_ ? slots_[s].d_lens + live_index() : nullptr;
  int pending_join = -1;  // open side branch: the op that waits for it
  for (size_t op_index = op_begin; op_index < op_end; ++op_index) {
    const PlanOp& op = plan_.ops[op_index];
    if (static_cast<int>(op_index) == pending_join) {
      HIP_CHECK(hipStreamWaitEvent(main_st, ev_join_, 0));
      pending_join = -1;
    }
    // per-op profiling times ops one after another: no branches then
    const bool side = branches_ && !op_events && op.join >= 0 && pending_join < 0;
    st = main_st;
    if (side) {
      HIP_CHECK(hipEventRecord(ev_fork_, main_st));
      HIP_CHECK(hipStreamWaitEvent(s_side_, ev_fork_, 0));
      st = s_side_;
    }
    const hipError_t e = launch_op(op, op_index, B, s, st, side, live);
    if (e != hipSuccess)
      throw std::runtime_error("launch of " + op.name + " failed: " + std::string(hipGetErrorString(e)));
    if (side) {
      HIP_CHECK(hipEventRecord(ev_join_, s_side_));
      pending_join = op.join;
    }
    if (op_events) HIP_CHECK(hipEventRecord(op_events[op_index + 1], st));
  }
  if (pending_join >= 0) HIP_CHECK(hipStreamWaitEvent(main_st, ev_join_, 0));  // part ended before the join
}

hipError_t HipEngine::launch_op(const PlanOp& op, size_t op_index, int B, int s, hipStream_t st, bool side,
                                const long long* live) {
  // plan buffer `id` of slot s as bf16 / fp32 (null for an absent id)
  auto buf = [&](int id) -> void* { return buf_ptr(id, s); };
  auto bf = [&](int id) { return static_cast<uint16_t*>(buf_ptr(id, s)); };
  auto cbf = [&](int id) { return static_cast<const uint16_t*>(buf_ptr(id, s)); };
  auto f32 = [&](int id) { return static_cast<float*>(buf_ptr(id, s)); };
  auto cf32 = [&](int id) { return static_cast<const float*>(buf_ptr(id, s)); };
  auto prm = [&](size_t off) -> const float* { return prm_ptr(off); };
  // split-K scratch of the stream in use: a side branch has its own, beside the executor's
  float* const ws = side ? ws_side_ : wss_[s % n_exec_];
  int* const counters = side ? counters_side_ : counterss_[s % n_exec_];
  hipError_t e = hipSuccess;
  switch (op.kind) {
    case PlanOp::INPUT_PREP:
      if (op.Cp > 8)
        e = kern::input_prep_wide(cf32(op.in), prm(op.scale_off), prm(op.shift_off), bf(op.out), B, op.C, op.H, op.W,
                                  op.Cp, st, sp_);
      else
        e = kern::input_prep(cf32(op.in), prm(op.scale_off), prm(op.shift_off), bf(op.out), B, op.C, op.H, op.W, op.Cp,
                             st, sp_);
      break;
    case PlanOp::ROWS_PREP:
      e = kern::rows_prep(cf32(op.in), bf(op.out), op.rows_per_sample * B, op.C, op.Cp, st, sp_);
      break;
    case PlanOp::COPY_COLS: {
      const long long R = op.rows_per_sample * B;
      e = kern::copy_cols(cbf(op.in), R * op.ld[0], op.ld[0], op.col[0], bf(op.out), R * op.ld[1], op.ld[1], op.col[1], R,
                          op.C, st, sp_);
      break;
    }
    case PlanOp::BINARY:
      e = kern::binary_rows(cbf(op.in), cbf(op.in2), bf(op.out), op.rows_per_sample * B, op.C, op.rows_per_sample, op.S,
                            op.gidx, op.act, op.clip_lo, op.clip_hi, st, live, sp_, op.Cp);
      break;
    case PlanOp::UNARY:
      e = kern::unary_rows(cbf(op.in), prm(op.scale_off), prm(op.shift_off), bf(op.out), op.rows_per_sample * B, op.C,
                           op.act, op.clip_lo, op.clip_hi, st, live, op.rows_per_sample, sp_, op.Cp);
      break;
    case PlanOp::CONV: {
      kern::ConvArgs a = conv_args(op, B, s);
      if (!use_live_) a.live = nullptr;
      const Tune t = tune_for(B, op_index);
      a.splits = t.splits;
      a.tail = t.tail;
      a.sk = t.sk;
      a.order = opt_.conv_order > 0 ? opt_.conv_order : t.order;
      a.ws = ws;
      a.counters = t.fused ? counters : nullptr;
      e = kern::conv_igemm(a, t.tile, st);
      break;
    }
    case PlanOp::CONV_PAIR: {
      kern::PairArgs a;
      a.x = cbf(op.in);
      a.w1 = reinterpret_cast<const uint16_t*>(params_ + op.w_off);
      a.bias1 = prm(op.bias_off);
      a.res = cbf(op.in2);
      a.xout = bf(op.out);
      a.aout = bf(op.out3);
      a.scale2 = prm(op.s2_off);
      a.shift2 = prm(op.b2_off);
      a.relu2 = op.conv.relu2;
      a.w2 = reinterpret_cast<const uint16_t*>(params_ + op.w2_off);
      a.bias2 = prm(op.bias2_off);
      a.relu = op.pair_relu;
      a.out = bf(op.out2);
      a.M = B * op.conv.Ho * op.conv.Wo;
      a.K1 = op.conv.K;
      a.N1 = op.conv.N;
      a.N2 = op.n2;
      a.rows_per_sample = op.conv.Ho * op.conv.Wo;
      a.live = live;
      a.zeros = zeros_;
      a.split = sp_;
      a.wplane1 = op.conv.wplane;
      a.wplane2 = op.w2plane;
      e = kern::conv_pair(a, st);
      break;
    }
    case PlanOp::PAD:
      e = kern::pad_nhwc(cbf(op.in), bf(op.out), B, op.H, op.W, op.C, op.Ho, op.Wo, op.ph, op.pw, st, sp_, op.sh, op.sw);
      break;
    case PlanOp::WHERE:
      e = kern::where_rows(cbf(op.in), op.in2 >= 0 ? cbf(op.in2) : nullptr, op.in3 >= 0 ? cbf(op.in3) : nullptr,
                           op.clip_lo, op.clip_hi, bf(op.out), op.rows_per_sample * B, op.C, st, live,
                           op.rows_per_sample, sp_, op.Cp);
      break;
    case PlanOp::BMM:
      e = kern::bmm_rows(cbf(op.in), cbf(op.in2), bf(op.out), B, op.S, op.Cp, op.gidx, op.ld[0], op.ld[1], op.C, st, live,
                         sp_);
      break;
    case PlanOp::RESIZE:
      e = kern::resize_nhwc(cbf(op.in), bf(op.out), B, op.H, op.W, op.C, op.Ho, op.Wo, op.clip_lo, op.clip_hi, op.gidx,
                            op.act, op.is_max, st, live, sp_);
      break;
    case PlanOp::POOL:
      e = kern::pool2d(cbf(op.in), bf(op.out), B, op.H, op.W, op.C, op.Ho, op.Wo, op.kh, op.kw, op.sh, op.sw, op.ph,
                       op.pw, op.is_max, op.cip, st, live, prm(op.scale_off), prm(op.shift_off), op.act, sp_);
      break;
    case PlanOp::GAP:
      e = kern::global_avgpool(cbf(op.in), bf(op.out), nullptr, nullptr, nullptr, 0, B, op.H * op.W, op.C, st, live, sp_,
                               op.gidx);
      break;
    case PlanOp::GAP_FC:
      e = kern::gap_fc(cbf(op.in), B, op.H * op.W, op.C, op.gidx, reinterpret_cast<const uint16_t*>(params_ + op.w_off),
                       op.conv.wplane, op.conv.Kpad, prm(op.bias_off), op.Cp, op.act, f32(op.out_f32), ws, ws_bytes_,
                       counters, kCounters, st, live, sp_);
      break;
    case PlanOp::AFFINE:
      e = kern::affine_act(cbf(op.in), cbf(op.in2), prm(op.scale_off), prm(op.shift_off), op.act, bf(op.out),
                           op.rows_per_sample * B, op.C, st, live, op.rows_per_sample, sp_, op.clip_lo, op.clip_hi);
      break;
    case PlanOp::TO_NCHW_F32:
      if (op.ld_store > 0)
        e = kern::nhwc_to_nchw_f32_strided(cbf(op.in), f32(op.out_f32), B, op.H, op.W, op.C, op.ld_store, st, sp_);
      else
        e = kern::nhwc_to_nchw_f32(cbf(op.in), f32(op.out_f32), B, op.H, op.W, op.C, st, sp_);
      break;
    case PlanOp::STEM:
      if (op.is_max) {  // + max pool (+ the pooled value's affine), input prep fused
        e = kern::conv_stem_pool_nchw(cf32(op.in), op.C, prm(op.scale_off), prm(op.shift_off),
                                      reinterpret_cast<const uint16_t*>(params_ + op.w_off), prm(op.bias_off),
                                      op.conv.relu, prm(op.s2_off), prm(op.b2_off), op.act, bf(op.out), B, op.conv.H,
                                      op.conv.W, op.conv.Ho, op.conv.Wo, op.Ho, op.Wo, st, live, sp_);
        break;
      }
      if (op.in == -2) {  // graph input, input prep fused
        e = kern::conv_stem7x7_nchw(cf32(op.in), op.C, prm(op.scale_off), prm(op.shift_off),
                                    reinterpret_cast<const uint16_t*>(params_ + op.w_off), prm(op.bias_off), bf(op.out),
                                    B, op.conv.H, op.conv.W, op.conv.Ho, op.conv.Wo, op.conv.relu, st, live, sp_);
        break;
      }
      e = kern::conv_stem7x7(cbf(op.in), reinterpret_cast<const uint16_t*>(params_ + op.w_off), prm(op.bias_off),
                             bf(op.out), B, op.conv.H, op.conv.W, op.conv.Ho, op.conv.Wo, op.conv.relu, st, live, sp_);
      break;
    case PlanOp::LAYERNORM:
      if (op.stats_only)
        e = kern::layernorm_rows(cbf(op.in), nullptr, prm(op.scale_off), prm(op.shift_off), op.eps,
                                 op.rows_per_sample * B, op.C, st, sp_, op.Cp, 0, f32(op.out));
      else
        e = kern::layernorm_rows(cbf(op.in), bf(op.out), prm(op.scale_off), prm(op.shift_off), op.eps,
                                 op.rows_per_sample * B, op.C, st, sp_, op.Cp, 0, nullptr, op.rms);
      break;
    case PlanOp::TOKENS:
      e = kern::tokens_assemble(cbf(op.in), prm(op.scale_off), prm(op.shift_off), bf(op.out), B, op.S, op.C, st, sp_,
                                op.out_stats >= 0 ? f32(op.out_stats) : nullptr);
      break;
    case PlanOp::GATHER_ROWS:
      e = kern::gather_rows(cbf(op.in), bf(op.out), B, op.S, op.gidx, op.C, st, sp_);
      break;
    case PlanOp::ATTENTION: {
      kern::AttentionArgs a;
      a.q = cbf(op.in) + op.col[0];
      a.k = cbf(op.in2) + op.col[1];
      a.v = cbf(op.in3) + op.col[2];
      a.out = bf(op.out);
      a.B = B;
      a.S = op.S;
      a.H = op.nh;
      a.D = op.hd;
      a.ldq = op.ld[0];
      a.ldk = op.ld[1];
      a.ldv = op.ld[2];
      a.ldo = op.C;
      a.scale = op.fscale;
      a.split = sp_;
      a.bias = op.bias_heads ? prm(op.bias_off) : nullptr;
      a.bias_heads = op.bias_heads;
      a.Sp = op.bias_heads || op.key_mask ? kern::key_pitch(op.S) : 0;
      a.causal = op.causal;
      a.kvis = op.key_mask ? cf32(op.in4) : nullptr;
      a.kend = op.key_mask ? static_cast<const int*>(buf(op.in5)) : nullptr;
      a.kv_heads = op.kv_heads;
      e = kern::attention(a, st);
      break;
    }
    case PlanOp::EMBED_TOKENS: {
      kern::EmbedArgs a;
      a.ids = cf32(op.in);
      a.ttab = prm(op.bias_off);
      if (op.in_ld > 0) {  // several graph inputs: segments of the packed request rows
        const float* row = cf32(op.in);
        a.ids = row + op.seg_ids;
        a.mask = op.pad.src >= 0 && op.out2 >= 0 ? row + op.pad.src : nullptr;
        a.ld_in = op.in_ld;
        if (op.seg_types >= 0) {
          a.types = row + op.seg_types;
          a.ttab = prm(op.type_off);
        }
        a.ldtt = op.C;
        a.T = op.type_rows;
      }
      a.table = prm(op.w_off);
      a.ldt = op.C;
      a.pos = prm(op.shift_off);
      a.out = bf(op.out);
      a.B = B;
      a.S = op.S;
      a.V = op.gidx;
      a.C = op.C;
      a.split = sp_;
      a.kvis = f32(op.out2);
      a.kend = static_cast<int*>(buf(op.out3));
      a.Sp = op.out2 >= 0 ? kern::key_pitch(op.S) : 0;
      a.pad_op = op.pad.op;
      a.pad_c = op.pad.value;
      a.pad_neg = op.pad.negated;
      a.pad_trunc = op.pad.truncated;
      e = kern::embed_tokens(a, st);
      break;
    }
    case PlanOp::POOL_TOKENS: {
      kern::PoolTokensArgs a;
      a.x = cbf(op.in);
      a.out = op.out >= 0 ? bf(op.out) : nullptr;
      a.out_f32 = op.out_f32 != -1 ? f32(op.out_f32) : nullptr;
      a.B = B;
      a.S = op.S;
      a.C = op.C;
      a.D = op.Cp;
      a.kvis = op.key_mask ? cf32(op.in4) : nullptr;
      a.kend = op.key_mask ? static_cast<const int*>(buf(op.in5)) : nullptr;
      a.Sp = op.key_mask ? kern::key_pitch(op.S) : 0;
      a.clip_min = op.count_min;
      a.normalize = op.normalize;
      a.eps = op.eps;
      a.live = live;
      a.split = sp_;
      a.ws = ws;
      a.ws_bytes = ws_bytes_;
      a.counters = counters;
      a.counters_n = kCounters;
      e = kern::pool_tokens(a, st);
      break;
    }
    case PlanOp::ROPE:
      e = kern::rope_rows(cbf(op.in) + op.col[0], bf(op.out), prm(op.scale_off), prm(op.shift_off), B, op.S, op.nh,
                          op.hd, op.ld[0], op.C, st, sp_);
      break;
    case PlanOp::GROUPNORM: {
      kern::GroupNormArgs g;
      g.x = cbf(op.in);
      g.out = bf(op.out);
      g.gamma = prm(op.scale_off);
      g.beta = prm(op.shift_off);
      g.B = B;
      g.HW = op.H * op.W;
      g.C = op.C;
      g.Cl = op.Cp;
      g.G = op.groups;
      g.eps = op.eps;
      g.act = op.act;
      g.split = sp_;
      g.live = live;
      g.ws = f32(op.out2);  // a plan buffer of the arena: kern::group_norm_workspace_bytes per sample
      g.ws_bytes = kern::group_norm_workspace_bytes(B, g.HW, g.C, g.G);
      e = kern::group_norm(g, st);
      break;
    }
    case PlanOp::GRN: {
      kern::GrnArgs g;
      g.x = cbf(op.in);
      g.out = bf(op.out);
      g.gamma = prm(op.scale_off);
      g.beta = prm(op.shift_off);
      g.B = B;
      g.HW = op.H * op.W;
      g.C = op.C;
      g.eps = op.eps;
      g.split = sp_;
      g.live = live;
      g.ws = f32(op.out2);  // a plan buffer of the arena: kern::grn_workspace_bytes per sample
      g.ws_bytes = kern::grn_workspace_bytes(B, g.HW, g.C);
      e = kern::grn(g, st);
      break;
    }
    case PlanOp::GCONV: {
      kern::GConvArgs g;
      g.x = cbf(op.in);
      g.w = prm(op.w_off);
      g.bias = prm(op.bias_off);
      g.res = cbf(op.in2);
      g.out = bf(op.out);
      g.B = B;
      g.H = op.H;
      g.W = op.W;
      g.Cin = op.C;
      g.Ho = op.Ho;
      g.Wo = op.Wo;
      g.Cout = op.Cp;
      g.groups = op.groups;
      g.KH = op.kh;
      g.KW = op.kw;
      g.stride = op.sh;
      g.dil = op.sw;
      g.pad_h = op.ph;
      g.pad_w = op.pw;
      g.act = op.act;
      g.clip_lo = op.clip_lo;
      g.clip_hi = op.clip_hi;
      g.split = sp_;
      g.live = live;
      if (op.tiled && opt_.tiled_dwconv) {
        g.w = prm(op.tap_w_off);
        e = kern::dwconv_tiled(g, st);
      } else {
        e = kern::grouped_conv(g, st);
      }
      break;
    }
    case PlanOp::SOFTMAX:
      e = kern::softmax_rows(cbf(op.in), bf(op.out), f32(op.out_f32), op.rows_per_sample * B, op.C, st, sp_, op.ld_store);
      break;
    case PlanOp::BF16_TO_F32:
      if (op.ld_store > 0)
        e = kern::rows_to_f32(cbf(op.in), f32(op.out_f32), op.rows_per_sample * B, op.C, op.ld_store, st, sp_);
      else
        e = kern::bf16_to_f32(cbf(op.in), f32(op.out_f32), static_cast<long long>(B) * op.C, st, sp_);
      break;
  }
  return e;
}

Json HipEngine::profile_ops(int B, int iters) {
  std::lock_guard<std::mutex> submit_guard(submit_mu_);
  synchronize();
  B = std::max(1, std::min(B, max_batch_));
  const size_t n = plan_.ops.size();
  std::vector<Event> ev(n + 1);
  for (auto& e : ev) HIP_CHECK(e.create());
  std::vector<double> us(n, 0.0);
  const int Bk = buckets_[bucket_index(B)];
  slots_[0].h_lens[live_index()] = Bk;  // profile the whole bucket
  encode_forward(Bk, 0, s_compute_);  // warm
  for (int it = 0; it < iters; ++it) {
    encode_forward(Bk, 0, s_compute_, ev.data());
    HIP_CHECK(hipStreamSynchronize(s_compute_));
    for (size_t i = 0; i < n; ++i) {
      float ms = 0;
      HIP_CHECK(hipEventElapsedTime(&ms, ev[i], ev[i + 1]));
      us[i] += ms * 1000.0 / iters;
    }
  }
  Json out = Json::object();
  Json ops = Json::array();
  double total = 0;
  for (size_t i = 0; i < n; ++i) {
    const PlanOp& op = plan_.ops[i];
    Json o = Json::object();
    o["name"] = op.name;
    o["kind"] = plan_kind_name(op.kind);
    o["us"] = us[i];
    o["gflop"] = op.flops_per_sample * Bk / 1e9;
    o["tflops"] = us[i] > 0 ? op.flops_per_sample * Bk / (us[i] * 1e6) : 0.0;
    if (op.kind == PlanOp::CONV) {
      const Tune t = tune_for(Bk, i);
      o["tile"] = t.tile;
      o["splits"] = t.splits;
      o["fused_splitk"] = t.fused;
      o["tile_order"] = t.order;
      o["tail_splitk"] = t.tail > 0;
      o["streamk_blocks"] = t.sk;
    }
    if (op.kind == PlanOp::ATTENTION) {
      o["bias_heads"] = op.bias_heads;
      o["causal"] = op.causal != 0;
      o["key_mask"] = op.key_mask != 0;
      o["kv_heads"] = op.kv_heads;
    }
    if (op.kind == PlanOp::POOL_TOKENS) {
      o["masked"] = op.key_mask != 0;
      o["normalize"] = op.normalize;
    }
    if (op.kind == PlanOp::LAYERNORM) o["rms"] = op.rms != 0;
    if (op.kind == PlanOp::GROUPNORM) {
      o["groups"] = op.groups;
      o["channels"] = op.Cp;
      o["pixels"] = op.H * op.W;
      o["act"] = op.act;
    }
    if (op.kind == PlanOp::GRN) {
      o["C"] = op.C;
      o["rows"] = op.H * op.W;
      o["eps"] = static_cast<double>(op.eps);
    }
    total += us[i];
    ops.push_back(o);
  }
  out["batch"] = Bk;
  out["total_us"] = total;
  out["tflops"] = total > 0 ? plan_.flops_per_sample * Bk / (total * 1e6) : 0.0;
  out["ops"] = ops;
  return out;
}

}  // namespace hip
}  // namespace die
