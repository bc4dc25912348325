// C ABI for launching individual HIP kernels on caller-provided device pointers (numerics tests
// compare them with torch on the GPU box).  Pointers/streams travel as uint64 (torch data_ptr()
// and torch.cuda.current_stream().cuda_stream).
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include "../core/json.h"
#include "../engine/engine.h"
#include "../engine/hip_plan.h"
#include "../kernels/kernels.h"
#include "../onnx/onnx_model.h"

using namespace die;

namespace {
template <typename T>
T* P(uint64_t v) {
  return reinterpret_cast<T*>(static_cast<uintptr_t>(v));
}
hipStream_t S(uint64_t v) { return reinterpret_cast<hipStream_t>(static_cast<uintptr_t>(v)); }
int geti(const Json& j, const char* k, int d) {
  auto* v = j.find(k);
  return v ? static_cast<int>(v->as_int()) : d;
}
// Reader of a launcher's geometry JSON whose keys are exactly the members of its argument struct
// (device addresses as integers).  A key that is missing leaves the member at its default; a key
// that no member took makes done() throw, so a misspelt key never silently becomes a default.
class Geom {
 public:
  explicit Geom(const char* text) : j_(Json::parse(text)) {}
  void operator()(const char* k, int& m) { if (auto* v = take(k)) m = static_cast<int>(v->as_int()); }
  void operator()(const char* k, size_t& m) { if (auto* v = take(k)) m = static_cast<size_t>(v->as_int()); }
  void operator()(const char* k, float& m) { if (auto* v = take(k)) m = static_cast<float>(v->as_double()); }
  template <typename T>
  void operator()(const char* k, T*& m) { if (auto* v = take(k)) m = P<T>(static_cast<uint64_t>(v->as_int())); }
  void done() const { if (taken_ != j_.as_object().size()) throw JsonError("unknown key in geometry"); }

 private:
  const Json* take(const char* k) {
    const Json* v = j_.find(k);
    taken_ += v != nullptr;
    return v;
  }
  Json j_;
  size_t taken_ = 0;
};
char* dup(const std::string& s) {
  char* p = static_cast<char*>(std::malloc(s.size() + 1));
  std::memcpy(p, s.data(), s.size() + 1);
  return p;
}

// The whole of a plan as text, for "same plan" checks (tools/plan_dump.py): one line per op with every
// PlanOp member (for `conv` every non-pointer ConvArgs member), one per buffer, the plan's scalars and
// a 64-bit FNV-1a of the parameter blob.  Floats print with 9 significant digits (exact for fp32),
// doubles with 17; an offset of SIZE_MAX prints as -1.
struct DumpLine {
  std::string s;
  char tmp[64];
  DumpLine& str(const char* k, const std::string& v) { return s += std::string(" ") + k + "=" + v, *this; }
  DumpLine& i(const char* k, long long v) { return str(k, std::to_string(v)); }
  DumpLine& off(const char* k, size_t v) { return i(k, v == SIZE_MAX ? -1 : static_cast<long long>(v)); }
  DumpLine& f(const char* k, float v) { return std::snprintf(tmp, sizeof tmp, "%.9g", static_cast<double>(v)), str(k, tmp); }
  DumpLine& d(const char* k, double v) { return std::snprintf(tmp, sizeof tmp, "%.17g", v), str(k, tmp); }
};

std::string plan_dump(const Plan& p) {
  std::string out;
  for (const PlanOp& o : p.ops) {
    DumpLine l;
    l.s = "op";
    l.i("kind", o.kind).str("name", o.name);
    l.i("in", o.in).i("in2", o.in2).i("in3", o.in3).i("in4", o.in4).i("in5", o.in5);
    l.i("out", o.out).i("out2", o.out2).i("out3", o.out3).i("out_f32", o.out_f32).i("out_stats", o.out_stats);
    l.off("w_off", o.w_off).off("bias_off", o.bias_off).off("s2_off", o.s2_off).off("b2_off", o.b2_off);
    l.off("scale_off", o.scale_off).off("shift_off", o.shift_off).off("tap_w_off", o.tap_w_off);
    l.off("type_off", o.type_off).off("w2_off", o.w2_off).off("bias2_off", o.bias2_off).off("colsum_off", o.colsum_off);
    const kern::ConvArgs& a = o.conv;
    l.i("conv.B", a.B).i("conv.H", a.H).i("conv.W", a.W).i("conv.Cin", a.Cin).i("conv.Ho", a.Ho).i("conv.Wo", a.Wo);
    l.i("conv.N", a.N).i("conv.KH", a.KH).i("conv.KW", a.KW).i("conv.stride", a.stride).i("conv.pad_h", a.pad_h);
    l.i("conv.pad_w", a.pad_w).i("conv.dil", a.dil).i("conv.K", a.K).i("conv.Kpad", a.Kpad).i("conv.M", a.M);
    l.i("conv.relu", a.relu).i("conv.relu2", a.relu2).i("conv.splits", a.splits).i("conv.counters_n", a.counters_n);
    l.f("conv.clip_lo", a.clip_lo).f("conv.clip_hi", a.clip_hi).f("conv.ln_eps", a.ln_eps).i("conv.split", a.split);
    l.i("conv.wplane", a.wplane).i("conv.xplane", a.xplane).i("conv.oplane", a.oplane).i("conv.order", a.order);
    l.i("conv.probe", a.probe).i("conv.tail", a.tail).i("conv.sk", a.sk);
    l.i("tile_bmax", o.tile_bmax).i("C", o.C).i("H", o.H).i("W", o.W).i("Ho", o.Ho).i("Wo", o.Wo).i("Cp", o.Cp);
    l.i("kh", o.kh).i("kw", o.kw).i("sh", o.sh).i("sw", o.sw).i("ph", o.ph).i("pw", o.pw).i("is_max", o.is_max);
    l.i("cip", o.cip).i("act", o.act).i("ld_store", o.ld_store).i("groups", o.groups).i("tiled", o.tiled);
    l.f("clip_lo", o.clip_lo).f("clip_hi", o.clip_hi).i("rows_per_sample", o.rows_per_sample);
    l.i("S", o.S).i("nh", o.nh).i("hd", o.hd).i("gidx", o.gidx);
    for (int r = 0; r < 3; ++r) l.i(("col" + std::to_string(r)).c_str(), o.col[r]).i(("ld" + std::to_string(r)).c_str(), o.ld[r]);
    l.f("fscale", o.fscale).f("eps", o.eps).i("bias_heads", o.bias_heads).i("causal", o.causal);
    l.i("key_mask", o.key_mask).i("kv_heads", o.kv_heads);
    l.i("pad.op", o.pad.op).f("pad.value", o.pad.value).i("pad.negated", o.pad.negated);
    l.i("pad.truncated", o.pad.truncated).i("pad.src", o.pad.src);
    l.i("in_ld", o.in_ld).i("seg_ids", o.seg_ids).i("seg_types", o.seg_types).i("type_rows", o.type_rows);
    l.i("normalize", o.normalize).f("count_min", o.count_min).d("flops", o.flops_per_sample).i("join", o.join);
    l.i("w2plane", o.w2plane).i("n2", o.n2).i("pair_relu", o.pair_relu).i("stats_only", o.stats_only).i("rms", o.rms);
    l.i("in3_parts", o.in3_parts);
    out += l.s + "\n";
  }
  for (const PlanBuf& b : p.bufs) {
    DumpLine l;
    l.s = "buf";
    l.i("bytes_per_sample", static_cast<long long>(b.bytes_per_sample)).i("offset", static_cast<long long>(b.offset));
    l.i("first_use", b.first_use).i("last_use", b.last_use);
    out += l.s + "\n";
  }
  DumpLine l;
  l.s = "plan";
  l.i("arena_bytes_per_sample", static_cast<long long>(p.arena_bytes_per_sample));
  l.i("arena_bytes", static_cast<long long>(p.arena_bytes));
  l.i("input_numel", static_cast<long long>(p.input_numel)).i("output_numel", static_cast<long long>(p.output_numel));
  l.d("flops", p.flops_per_sample).i("split", p.split);
  std::string shape;
  for (auto v : p.input_shape) shape += (shape.empty() ? "" : ",") + std::to_string(v);
  l.str("input_shape", shape);
  shape.clear();
  for (auto v : p.output_shape) shape += (shape.empty() ? "" : ",") + std::to_string(v);
  l.str("output_shape", shape);
  for (const auto& s : p.inputs)
    l.str("input", s.name + ":" + s.role + ":" + std::to_string(s.offset) + ":" + std::to_string(s.numel));
  uint64_t h = 14695981039346656037ull;
  for (uint8_t b : p.params) h = (h ^ b) * 1099511628211ull;
  std::snprintf(l.tmp, sizeof l.tmp, "%016llx", static_cast<unsigned long long>(h));
  l.i("param_bytes", static_cast<long long>(p.params.size())).str("params_fnv1a", l.tmp);
  return out + l.s + "\n";
}

// fuse: bit 0 conv pairs, bit 1 stem + pool, bit 2 global pool + FC head, bit 3 LayerNorm folding,
// bit 4 LayerNorm statistics from the producing GEMM's epilogue
PlanOptions plan_options(int side_branches, int split, int fuse) {
  PlanOptions po;
  po.side_branches = side_branches != 0;
  po.split = split != 0;
  po.fuse_pairs = (fuse & 1) != 0;
  po.fuse_stem_pool = (fuse & 2) != 0;
  po.fuse_gap_fc = (fuse & 4) != 0;
  po.fold_layernorm = (fuse & 8) != 0;
  po.ln_stats_epilogue = (fuse & 16) != 0;
  return po;
}
}  // namespace

extern "C" {

// geometry JSON: B,H,W,Cin,Ho,Wo,N,KH,KW,stride,pad_h,pad_w,dil,K,Kpad,relu,relu2
int die_kern_conv(const char* geom, uint64_t x, uint64_t w, uint64_t bias, uint64_t res, uint64_t out,
                  uint64_t out_f32, uint64_t scale2, uint64_t shift2, uint64_t out2, int tile, uint64_t stream) {
  try {
    Json j = Json::parse(geom);
    kern::ConvArgs a;
    a.B = geti(j, "B", 1);
    a.H = geti(j, "H", 1);
    a.W = geti(j, "W", 1);
    a.Cin = geti(j, "Cin", 1);
    a.Ho = geti(j, "Ho", 1);
    a.Wo = geti(j, "Wo", 1);
    a.N = geti(j, "N", 1);
    a.KH = geti(j, "KH", 1);
    a.KW = geti(j, "KW", 1);
    a.stride = geti(j, "stride", 1);
    a.pad_h = geti(j, "pad_h", 0);
    a.pad_w = geti(j, "pad_w", 0);
    a.dil = geti(j, "dil", 1);
    a.K = geti(j, "K", a.KH * a.KW * a.Cin);
    a.Kpad = geti(j, "Kpad", (a.K + 63) / 64 * 64);
    a.M = a.B * a.Ho * a.Wo;
    a.relu = geti(j, "relu", 0);
    a.relu2 = geti(j, "relu2", 0);
    a.x = P<const uint16_t>(x);
    a.w = P<const uint16_t>(w);
    a.bias = P<const float>(bias);
    a.res = P<const uint16_t>(res);
    a.out = P<uint16_t>(out);
    a.out_f32 = P<float>(out_f32);
    a.scale2 = P<const float>(scale2);
    a.shift2 = P<const float>(shift2);
    a.out2 = P<uint16_t>(out2);
    a.splits = geti(j, "splits", 1);
    a.order = geti(j, "order", 0);
    a.probe = geti(j, "probe", 0);
    a.tail = geti(j, "tail", 0);
    a.sk = geti(j, "sk", 0);
    if (auto* v = j.find("live")) a.live = P<const long long>(static_cast<uint64_t>(v->as_int()));  // live batch (int64 on the device)
    if (auto* v = j.find("ws")) a.ws = P<float>(static_cast<uint64_t>(v->as_int()));
    if (auto* v = j.find("zeros")) a.zeros = P<const uint16_t>(static_cast<uint64_t>(v->as_int()));
    if (auto* v = j.find("counters")) a.counters = P<int>(static_cast<uint64_t>(v->as_int()));
    a.counters_n = geti(j, "counters_n", 0);
    a.split = geti(j, "split", 0);
    if (auto* v = j.find("wplane")) a.wplane = v->as_int();
    // LayerNorm folding / statistics (ConvArgs::row_stats, col_sum, row_parts, stats_out, ln_eps)
    if (auto* v = j.find("row_stats")) a.row_stats = P<const float>(static_cast<uint64_t>(v->as_int()));
    if (auto* v = j.find("col_sum")) a.col_sum = P<const float>(static_cast<uint64_t>(v->as_int()));
    if (auto* v = j.find("row_parts")) a.row_parts = P<const float>(static_cast<uint64_t>(v->as_int()));
    if (auto* v = j.find("stats_out")) a.stats_out = P<float>(static_cast<uint64_t>(v->as_int()));
    if (auto* v = j.find("ln_eps")) a.ln_eps = static_cast<float>(v->as_double());
    if (tile < 0) tile = kern::choose_tile(a.M, a.N, a.K);
    return static_cast<int>(kern::conv_igemm(a, tile, S(stream)));
  } catch (...) {
    return -1;
  }
}

// geometry JSON: M, K1, N1, N2, relu, relu2, split, wplane1, wplane2, zeros
int die_kern_conv_pair(const char* geom, uint64_t x, uint64_t w1, uint64_t bias1, uint64_t res, uint64_t xout,
                       uint64_t scale2, uint64_t shift2, uint64_t w2, uint64_t bias2, uint64_t out, uint64_t stream) {
  try {
    Json j = Json::parse(geom);
    kern::PairArgs a;
    a.M = geti(j, "M", 0);
    a.K1 = geti(j, "K1", 64);
    a.N1 = geti(j, "N1", 256);
    a.N2 = geti(j, "N2", 64);
    a.relu = geti(j, "relu", 1);
    a.relu2 = geti(j, "relu2", 1);
    a.split = geti(j, "split", 0);
    a.shared_w = geti(j, "shared_w", -1);
    if (auto* v = j.find("wplane1")) a.wplane1 = v->as_int();
    if (auto* v = j.find("wplane2")) a.wplane2 = v->as_int();
    if (auto* v = j.find("zeros")) a.zeros = P<const uint16_t>(static_cast<uint64_t>(v->as_int()));
    if (auto* v = j.find("aout")) a.aout = P<uint16_t>(static_cast<uint64_t>(v->as_int()));
    a.x = P<const uint16_t>(x);
    a.w1 = P<const uint16_t>(w1);
    a.bias1 = P<const float>(bias1);
    a.res = P<const uint16_t>(res);
    a.xout = P<uint16_t>(xout);
    a.scale2 = P<const float>(scale2);
    a.shift2 = P<const float>(shift2);
    a.w2 = P<const uint16_t>(w2);
    a.bias2 = P<const float>(bias2);
    a.out = P<uint16_t>(out);
    return static_cast<int>(kern::conv_pair(a, S(stream)));
  } catch (...) {
    return -1;
  }
}

int die_pair_permute_row(int n) { return kern::pair_permute_row(n); }

int die_kern_input_prep(uint64_t x, uint64_t scale, uint64_t shift, uint64_t out, int B, int C, int H, int W, int Cp,
                        uint64_t stream, int split) {
  return static_cast<int>(kern::input_prep(P<const float>(x), P<const float>(scale), P<const float>(shift),
                                           P<uint16_t>(out), B, C, H, W, Cp, S(stream), split));
}

// live 0 = the whole batch; scale / shift (0 = none): per-channel affine on the pooled value, then act (0 = none)
int die_kern_pool2d(uint64_t x, uint64_t y, int B, int H, int W, int C, int Ho, int Wo, int kh, int kw, int sh,
                    int sw, int ph, int pw, int is_max, int cip, uint64_t stream, int split, uint64_t live,
                    uint64_t scale, uint64_t shift, int act) {
  return static_cast<int>(kern::pool2d(P<const uint16_t>(x), P<uint16_t>(y), B, H, W, C, Ho, Wo, kh, kw, sh, sw, ph,
                                       pw, is_max, cip, S(stream), P<const long long>(live), P<const float>(scale),
                                       P<const float>(shift), act, split));
}

// live 0 = the whole batch; mode 0 mean, 1 sum, 2 max
int die_kern_gap(uint64_t x, uint64_t out, uint64_t out_f32, uint64_t scale, uint64_t shift, int relu, int B, int HW,
                 int C, uint64_t stream, int split, uint64_t live, int mode) {
  return static_cast<int>(kern::global_avgpool(P<const uint16_t>(x), P<uint16_t>(out), P<float>(out_f32),
                                               P<const float>(scale), P<const float>(shift), relu, B, HW, C, S(stream),
                                               P<const long long>(live), split, mode));
}

// ---- generic kernels (kernels/generic.hip) and batched MatMul (kernels/bmm.hip); live 0 = none ----
int die_kern_rows_prep(uint64_t x, uint64_t y, long long R, int F, int Fp, uint64_t stream, int split) {
  return static_cast<int>(kern::rows_prep(P<const float>(x), P<uint16_t>(y), R, F, Fp, S(stream), split));
}

int die_kern_input_prep_wide(uint64_t x, uint64_t scale, uint64_t shift, uint64_t out, int B, int C, int H, int W,
                             int Cp, uint64_t stream, int split) {
  return static_cast<int>(kern::input_prep_wide(P<const float>(x), P<const float>(scale), P<const float>(shift),
                                                P<uint16_t>(out), B, C, H, W, Cp, S(stream), split));
}

int die_kern_copy_cols(uint64_t x, long long xplane, int ldx, int colx, uint64_t y, long long yplane, int ldy, int coly,
                       long long R, int ncols, uint64_t stream, int split) {
  return static_cast<int>(kern::copy_cols(P<const uint16_t>(x), xplane, ldx, colx, P<uint16_t>(y), yplane, ldy, coly, R,
                                          ncols, S(stream), split));
}

int die_kern_binary_rows(uint64_t x, uint64_t y, uint64_t out, long long R, int C, long long rows_per_sample, int ymode,
                         int op, int act, float a, float b, uint64_t stream, uint64_t live, int split, int Cl) {
  return static_cast<int>(kern::binary_rows(P<const uint16_t>(x), P<const uint16_t>(y), P<uint16_t>(out), R, C,
                                            rows_per_sample, ymode, op, act, a, b, S(stream), P<const long long>(live),
                                            split, Cl));
}

int die_kern_unary_rows(uint64_t x, uint64_t scale, uint64_t shift, uint64_t y, long long R, int C, int act, float a,
                        float b, uint64_t stream, uint64_t live, long long rows_per_sample, int split, int Cl) {
  return static_cast<int>(kern::unary_rows(P<const uint16_t>(x), P<const float>(scale), P<const float>(shift),
                                           P<uint16_t>(y), R, C, act, a, b, S(stream), P<const long long>(live),
                                           rows_per_sample, split, Cl));
}

int die_kern_where_rows(uint64_t c, uint64_t a, uint64_t b, float av, float bv, uint64_t out, long long R, int C,
                        uint64_t stream, uint64_t live, long long rows_per_sample, int split, int Cl) {
  return static_cast<int>(kern::where_rows(P<const uint16_t>(c), P<const uint16_t>(a), P<const uint16_t>(b), av, bv,
                                           P<uint16_t>(out), R, C, S(stream), P<const long long>(live), rows_per_sample,
                                           split, Cl));
}

int die_kern_resize_nhwc(uint64_t x, uint64_t y, int B, int H, int W, int C, int Ho, int Wo, float scale_h,
                         float scale_w, int coord, int mode, int nearest, uint64_t stream, uint64_t live, int split) {
  return static_cast<int>(kern::resize_nhwc(P<const uint16_t>(x), P<uint16_t>(y), B, H, W, C, Ho, Wo, scale_h, scale_w,
                                            coord, mode, nearest, S(stream), P<const long long>(live), split));
}

int die_kern_pad_nhwc(uint64_t x, uint64_t y, int B, int H, int W, int C, int Ho, int Wo, int t, int l, uint64_t stream,
                      int split, int sy, int sx) {
  return static_cast<int>(kern::pad_nhwc(P<const uint16_t>(x), P<uint16_t>(y), B, H, W, C, Ho, Wo, t, l, S(stream),
                                         split, sy, sx));
}

int die_kern_rows_to_f32(uint64_t x, uint64_t y, long long R, int C, int ld, uint64_t stream, int split) {
  return static_cast<int>(kern::rows_to_f32(P<const uint16_t>(x), P<float>(y), R, C, ld, S(stream), split));
}

int die_kern_nhwc_to_nchw_strided(uint64_t x, uint64_t y, int B, int H, int W, int C, int Cs, uint64_t stream,
                                  int split) {
  return static_cast<int>(kern::nhwc_to_nchw_f32_strided(P<const uint16_t>(x), P<float>(y), B, H, W, C, Cs, S(stream),
                                                         split));
}

int die_kern_bmm_rows(uint64_t A, uint64_t Bm, uint64_t C, int batch, int M, int N, int K, int lda, int ldb, int ldc,
                      uint64_t stream, uint64_t live, int split) {
  return static_cast<int>(kern::bmm_rows(P<const uint16_t>(A), P<const uint16_t>(Bm), P<uint16_t>(C), batch, M, N, K,
                                         lda, ldb, ldc, S(stream), P<const long long>(live), split));
}

int die_kern_affine(uint64_t x, uint64_t z, uint64_t scale, uint64_t shift, int act, uint64_t y, long long M, int C,
                    uint64_t stream, int split) {
  return static_cast<int>(kern::affine_act(P<const uint16_t>(x), P<const uint16_t>(z), P<const float>(scale),
                                           P<const float>(shift), act, P<uint16_t>(y), M, C, S(stream), nullptr, 0,
                                           split));
}

int die_kern_nhwc_to_nchw(uint64_t x, uint64_t y, int B, int H, int W, int C, uint64_t stream, int split) {
  return static_cast<int>(kern::nhwc_to_nchw_f32(P<const uint16_t>(x), P<float>(y), B, H, W, C, S(stream), split));
}

// kernels.h layernorm_rows: Cl logical columns (0 = C), stats 0 = none, rms != 0 = RMSNorm (beta unused)
int die_kern_layernorm(uint64_t x, uint64_t y, uint64_t gamma, uint64_t beta, float eps, long long rows, int C,
                       uint64_t stream, int split, int Cl, int variant, uint64_t stats, int rms) {
  return static_cast<int>(kern::layernorm_rows(P<const uint16_t>(x), P<uint16_t>(y), P<const float>(gamma),
                                               P<const float>(beta), eps, rows, C, S(stream), split, Cl, variant,
                                               P<float>(stats), rms));
}

// Rotary position embedding of head rows (kernels.h rope_rows)
int die_kern_rope_rows(uint64_t x, uint64_t y, uint64_t cos, uint64_t sin, int B, int Sq, int H, int D, int ldx, int ldy,
                       uint64_t stream, int split) {
  return static_cast<int>(kern::rope_rows(P<const uint16_t>(x), P<uint16_t>(y), P<const float>(cos), P<const float>(sin),
                                          B, Sq, H, D, ldx, ldy, S(stream), split));
}

int die_kern_tokens(uint64_t patches, uint64_t cls, uint64_t pos, uint64_t out, int B, int S0, int C, uint64_t stream,
                    int split) {
  return static_cast<int>(kern::tokens_assemble(P<const uint16_t>(patches), P<const float>(cls), P<const float>(pos),
                                                P<uint16_t>(out), B, S0, C, S(stream), split));
}

int die_kern_gather_rows(uint64_t x, uint64_t y, int B, int Sq, int idx, int C, uint64_t stream, int split) {
  return static_cast<int>(kern::gather_rows(P<const uint16_t>(x), P<uint16_t>(y), B, Sq, idx, C, S(stream), split));
}

void die_kern_set_gap_fc_stop(int v) { kern::set_gap_fc_stop(v); }

int die_kern_gap_fc(uint64_t x, int B, int HW, int C, int mode, uint64_t w, long long wplane, int Kpad, uint64_t bias,
                    int N, int act, uint64_t out, uint64_t ws, long long ws_bytes, uint64_t counters, int counters_n,
                    uint64_t stream, int split) {
  return static_cast<int>(kern::gap_fc(P<const uint16_t>(x), B, HW, C, mode, P<const uint16_t>(w), wplane, Kpad,
                                       P<const float>(bias), N, act, P<float>(out), P<float>(ws),
                                       static_cast<size_t>(ws_bytes), P<int>(counters), counters_n, S(stream), nullptr,
                                       split));
}

void die_kern_set_attention_variant(int v) { kern::set_attention_variant(v); }
void die_kern_set_decode_variant(int v) { kern::set_decode_variant(v); }
void die_kern_set_layernorm_xcd(int v) { kern::set_layernorm_xcd(v); }
void die_kern_set_pair_shared_w(int v) { kern::set_pair_shared_w(v); }

// The token-model launchers take a geometry JSON whose keys are exactly the members of their argument
// struct (kernels.h; device addresses as integers, a missing key = the member's default) and the
// stream.  An unknown key returns -1 and launches nothing.  Floats (scale, pad_c, clip_min, eps)
// arrive bit-exact: the caller prints the double with all its digits (Python's repr), Json parses
// it back to that double (from_chars / strtod) and it is cast to float once, here -- the same single
// rounding a c_float argument gets.
int die_kern_attention(const char* geom, uint64_t stream) {
  try {
    Geom g(geom);
    kern::AttentionArgs a;
    g("q", a.q), g("k", a.k), g("v", a.v), g("out", a.out);
    g("B", a.B), g("S", a.S), g("H", a.H), g("D", a.D);
    g("ldq", a.ldq), g("ldk", a.ldk), g("ldv", a.ldv), g("ldo", a.ldo);
    g("scale", a.scale), g("split", a.split);
    g("bias", a.bias), g("bias_heads", a.bias_heads), g("Sp", a.Sp), g("causal", a.causal);
    g("kvis", a.kvis), g("kend", a.kend), g("kv_heads", a.kv_heads);
    g.done();
    return static_cast<int>(kern::attention(a, S(stream)));
  } catch (...) {
    return -1;
  }
}

int die_kern_embed_tokens(const char* geom, uint64_t stream) {
  try {
    Geom g(geom);
    kern::EmbedArgs a;
    g("ids", a.ids), g("types", a.types), g("mask", a.mask), g("ld_in", a.ld_in);
    g("table", a.table), g("ldt", a.ldt), g("pos", a.pos), g("ttab", a.ttab), g("ldtt", a.ldtt), g("T", a.T);
    g("out", a.out), g("B", a.B), g("S", a.S), g("V", a.V), g("C", a.C), g("split", a.split);
    g("kvis", a.kvis), g("kend", a.kend), g("Sp", a.Sp);
    g("pad_op", a.pad_op), g("pad_c", a.pad_c), g("pad_neg", a.pad_neg), g("pad_trunc", a.pad_trunc);
    g.done();
    return static_cast<int>(kern::embed_tokens(a, S(stream)));
  } catch (...) {
    return -1;
  }
}

int die_kern_pool_tokens(const char* geom, uint64_t stream) {
  try {
    Geom g(geom);
    kern::PoolTokensArgs a;
    g("x", a.x), g("out", a.out), g("out_f32", a.out_f32);
    g("B", a.B), g("S", a.S), g("C", a.C), g("D", a.D);
    g("kvis", a.kvis), g("kend", a.kend), g("Sp", a.Sp);
    g("clip_min", a.clip_min), g("normalize", a.normalize), g("eps", a.eps);
    g("live", a.live), g("split", a.split);
    g("ws", a.ws), g("ws_bytes", a.ws_bytes), g("counters", a.counters), g("counters_n", a.counters_n);
    g.done();
    return static_cast<int>(kern::pool_tokens(a, S(stream)));
  } catch (...) {
    return -1;
  }
}
uint64_t die_kern_pool_tokens_ws_bytes(int B, int C) { return kern::pool_tokens_ws_bytes(B, C); }

// the kernels' id -> table row rule on the host (k::token_index)
int die_token_index(float x, int V) { return kern::token_index_host(x, V); }

// geometry JSON: B,H,W,Cin,Ho,Wo,Cout,groups,KH,KW,stride,pad_h,pad_w,dil,act,clip_lo,clip_hi,split
static kern::GConvArgs gconv_geometry(const char* geom) {
  Json j = Json::parse(geom);
  kern::GConvArgs a;
  a.B = geti(j, "B", 1);
  a.H = geti(j, "H", 1);
  a.W = geti(j, "W", 1);
  a.Cin = geti(j, "Cin", 8);
  a.Ho = geti(j, "Ho", 1);
  a.Wo = geti(j, "Wo", 1);
  a.Cout = geti(j, "Cout", 8);
  a.groups = geti(j, "groups", 1);
  a.KH = geti(j, "KH", 1);
  a.KW = geti(j, "KW", 1);
  a.stride = geti(j, "stride", 1);
  a.pad_h = geti(j, "pad_h", 0);
  a.pad_w = geti(j, "pad_w", 0);
  a.dil = geti(j, "dil", 1);
  a.act = geti(j, "act", 0);
  if (auto* v = j.find("clip_lo")) a.clip_lo = static_cast<float>(v->as_double());
  if (auto* v = j.find("clip_hi")) a.clip_hi = static_cast<float>(v->as_double());
  a.split = geti(j, "split", 0);
  return a;
}

int die_kern_gconv(const char* geom, uint64_t x, uint64_t w, uint64_t bias, uint64_t out, uint64_t stream) {
  try {
    kern::GConvArgs a = gconv_geometry(geom);
    a.x = P<const uint16_t>(x);
    a.w = P<const float>(w);
    a.bias = P<const float>(bias);
    a.out = P<uint16_t>(out);
    return static_cast<int>(kern::grouped_conv(a, S(stream)));
  } catch (...) {
    return -1;
  }
}

// Depthwise conv with the whole GConvArgs epilogue (residual, f32 output, device-side live batch
// count) on either kernel: tiled = 1 the tiled kernel (w = fp32 [KH*KW][C]), 0 grouped_conv
// (w = fp32 [C][KH][KW][1]).  Returns the hipError_t (1 = hipErrorInvalidValue: outside the scope).
int die_kern_dwconv(const char* geom, int tiled, uint64_t x, uint64_t w, uint64_t bias, uint64_t res, uint64_t out,
                    uint64_t out_f32, uint64_t live, uint64_t stream) {
  try {
    kern::GConvArgs a = gconv_geometry(geom);
    a.x = P<const uint16_t>(x);
    a.w = P<const float>(w);
    a.bias = P<const float>(bias);
    a.res = P<const uint16_t>(res);
    a.out = P<uint16_t>(out);
    a.out_f32 = P<float>(out_f32);
    a.live = P<const long long>(live);
    return static_cast<int>(tiled ? kern::dwconv_tiled(a, S(stream)) : kern::grouped_conv(a, S(stream)));
  } catch (...) {
    return -1;
  }
}

// GroupNorm / InstanceNorm (kern::group_norm): geom's keys are the scalar members of GroupNormArgs.
// Returns the hipError_t (1 = hipErrorInvalidValue: bad arguments, nothing launched).
long long die_groupnorm_workspace_bytes(int B, int HW, int C, int G) {
  return static_cast<long long>(kern::group_norm_workspace_bytes(B, HW, C, G));
}
int die_kern_groupnorm(const char* geom, uint64_t x, uint64_t gamma, uint64_t beta, uint64_t out, uint64_t ws,
                       uint64_t live, uint64_t stream) {
  try {
    kern::GroupNormArgs a;
    Geom g(geom);
    g("B", a.B), g("HW", a.HW), g("C", a.C), g("Cl", a.Cl), g("G", a.G), g("eps", a.eps), g("act", a.act);
    g("split", a.split), g("ws_bytes", a.ws_bytes);
    g.done();
    a.x = P<const uint16_t>(x);
    a.gamma = P<const float>(gamma);
    a.beta = P<const float>(beta);
    a.out = P<uint16_t>(out);
    a.ws = P<float>(ws);
    a.live = P<const long long>(live);
    return static_cast<int>(kern::group_norm(a, S(stream)));
  } catch (...) {
    return -1;
  }
}

// Global Response Normalization (kern::grn): geom's keys are the scalar members of GrnArgs.
// Returns the hipError_t (1 = hipErrorInvalidValue: bad arguments, nothing launched).
long long die_grn_workspace_bytes(int B, int HW, int C) {
  return static_cast<long long>(kern::grn_workspace_bytes(B, HW, C));
}
int die_kern_grn(const char* geom, uint64_t x, uint64_t gamma, uint64_t beta, uint64_t out, uint64_t ws, uint64_t live,
                 uint64_t stream) {
  try {
    kern::GrnArgs a;
    Geom g(geom);
    g("B", a.B), g("HW", a.HW), g("C", a.C), g("eps", a.eps), g("split", a.split), g("ws_bytes", a.ws_bytes), g("form", a.form);
    g.done();
    a.x = P<const uint16_t>(x);
    a.gamma = P<const float>(gamma);
    a.beta = P<const float>(beta);
    a.out = P<uint16_t>(out);
    a.ws = P<float>(ws);
    a.live = P<const long long>(live);
    return static_cast<int>(kern::grn(a, S(stream)));
  } catch (...) {
    return -1;
  }
}

int die_kern_softmax(uint64_t x, uint64_t y, uint64_t yf, long long rows, int C, uint64_t stream, int split) {
  return static_cast<int>(kern::softmax_rows(P<const uint16_t>(x), P<uint16_t>(y), P<float>(yf), rows, C, S(stream), split));
}

long long die_decode_scratch_bytes(int max_batch, long long text_cap) {
  return static_cast<long long>(kern::decode_scratch_bytes(max_batch, static_cast<size_t>(text_cap)));
}

// packed / poffs (0 = raw text only): 4-bit packed samples at packed + poffs[b] (poffs[b] < 0: raw text at text + offs[b])
int die_kern_decode(uint64_t text, uint64_t offs, uint64_t packed, uint64_t poffs, long long text_cap,
                    uint64_t lens, int B, uint64_t out, long long numel, uint64_t status, uint64_t ntok,
                    uint64_t scratch, uint64_t stream) {
  return static_cast<int>(kern::decode_json_numbers(P<const unsigned char>(text), P<const long long>(offs),
                                                    static_cast<size_t>(text_cap), P<const long long>(lens), B,
                                                    P<float>(out), numel, P<int>(status), P<int>(ntok), P<void>(scratch),
                                                    S(stream), P<const unsigned char>(packed), P<const long long>(poffs)));
}

int die_kern_stem(uint64_t x, uint64_t w, uint64_t bias, uint64_t out, int B, int H, int W, int Ho, int Wo, int relu,
                  uint64_t stream, int split) {
  return static_cast<int>(kern::conv_stem7x7(P<const uint16_t>(x), P<const uint16_t>(w), P<const float>(bias),
                                             P<uint16_t>(out), B, H, W, Ho, Wo, relu, S(stream), nullptr, split));
}

int die_kern_stem_nchw(uint64_t x, int C, uint64_t scale, uint64_t shift, uint64_t w, uint64_t bias, uint64_t out, int B,
                       int H, int W, int Ho, int Wo, int relu, uint64_t stream, int split, int max_blocks) {
  return static_cast<int>(kern::conv_stem7x7_nchw(P<const float>(x), C, P<const float>(scale), P<const float>(shift),
                                                  P<const uint16_t>(w), P<const float>(bias), P<uint16_t>(out), B, H, W,
                                                  Ho, Wo, relu, S(stream), nullptr, split, max_blocks));
}

// Load-time support report: every node the HIP planner cannot lower, with the reason.
char* die_plan_report(const char* model_path, int split, char** err) {
  try {
    const PlanReport r = plan_report(onnx::load_onnx(model_path), 8, split != 0);
    Json j = Json::object();
    j["supported"] = r.supported;
    Json items = Json::array();
    for (const auto& it : r.unsupported) {
      Json e = Json::object();
      e["node"] = it.node;
      e["op"] = it.op;
      e["error"] = it.error;
      items.push_back(e);
    }
    j["unsupported"] = items;
    j["blocked"] = r.blocked;
    j["text"] = r.text();
    return dup(j.dump());
  } catch (const std::exception& e) {
    if (err) *err = dup(e.what());
    return nullptr;
  }
}

// Plan summary of a model (op list with fused epilogues), for tests and docs.
// Hybrid HIP + CPU partition of a model (engine/hybrid_engine.cpp), computed on the host.
char* die_hybrid_partition(const char* model_path, int max_batch, int split, char** err) {
  try {
    const onnx::Model m = onnx::load_onnx(model_path);
    Json out = Json::array();
    for (const HybridSegment& s : hybrid_partition(m, max_batch, split != 0)) {
      Json e = Json::object();
      e["device"] = s.hip ? "hip" : "cpu";
      e["first"] = s.first;
      e["last"] = s.last;
      e["input"] = s.input;
      e["output"] = s.output;
      e["gemm_nodes"] = s.convs;
      Json ops = Json::array();
      for (int k = s.first; k <= s.last; ++k) ops.push_back(m.nodes[static_cast<size_t>(k)].op_type);
      e["ops"] = ops;
      out.push_back(e);
    }
    return dup(out.dump());
  } catch (const std::exception& ex) {
    if (err) *err = dup(ex.what());
    return nullptr;
  }
}

// Every member of a model's plan as text (plan_dump above); the arguments of die_plan_summary.
char* die_plan_dump(const char* model_path, int max_batch, int side_branches, int split, int fuse, char** err) {
  try {
    return dup(plan_dump(build_plan(onnx::load_onnx(model_path), max_batch, plan_options(side_branches, split, fuse))));
  } catch (const std::exception& e) {
    if (err) *err = dup(e.what());
    return nullptr;
  }
}

// fuse: the bits of plan_options
char* die_plan_summary(const char* model_path, int max_batch, int side_branches, int split, int fuse, char** err) {
  try {
    Plan p = build_plan(onnx::load_onnx(model_path), max_batch, plan_options(side_branches, split, fuse));
    Json j = Json::object();
    j["summary"] = p.summary();
    j["arena_bytes"] = static_cast<long long>(p.arena_bytes);
    j["param_bytes"] = static_cast<long long>(p.params.size());
    j["gflop_per_sample"] = p.flops_per_sample / 1e9;
    j["precision"] = p.split ? "fp32" : "bf16";
    Json ops = Json::array();
    for (auto& o : p.ops) {
      Json e = Json::object();
      e["kind"] = plan_kind_name(o.kind);
      e["name"] = o.name;
      e["gflop"] = o.flops_per_sample / 1e9;
      e["join"] = o.join;
      // arena ranges [offset, offset + bytes) at max_batch of the op's buffers, by role
      Json bufs = Json::object();
      const char* roles[] = {"in", "in2", "in3", "out", "out2", "out3", "out_stats", "in4", "in5"};
      const int ids[] = {o.in, o.in2, o.in3, o.out, o.out2, o.out3, o.out_stats, o.in4, o.in5};
      for (int r = 0; r < 9; ++r)
        if (ids[r] >= 0) {
          Json range = Json::array();
          range.push_back(static_cast<long long>(p.bufs[ids[r]].offset));
          range.push_back(static_cast<long long>(p.bufs[ids[r]].offset + p.bufs[ids[r]].bytes_per_sample * max_batch));
          bufs[roles[r]] = range;
        }
      e["bufs"] = bufs;
      if (o.kind == PlanOp::CONV) {
        e["N"] = o.conv.N;
        e["K"] = o.conv.K;
        e["KH"] = o.conv.KH;
        e["stride"] = o.conv.stride;
        e["relu"] = o.conv.relu;
        e["residual"] = o.in2 >= 0;
        e["dual_store"] = o.out2 >= 0;
        e["store_main"] = o.out >= 0 || o.out_f32 != -1;
        e["relu2"] = o.conv.relu2;
        e["act"] = o.conv.relu;
        e["rows"] = o.conv.Ho * o.conv.Wo;
        e["layernorm_folded"] = o.colsum_off != SIZE_MAX;
        e["stats_from_producer"] = o.in3_parts != 0;  // reads (merges) LayerNorm statistics partials
      }
      if (o.kind == PlanOp::ATTENTION) {
        e["bias_heads"] = o.bias_heads;  // 0: no table, 1: one slice shared by the heads, nh: per head
        e["causal"] = o.causal != 0;
        e["key_mask"] = o.key_mask != 0;  // the request's padding mask (key data from the embed_tokens op)
        e["kv_heads"] = o.kv_heads;  // K / V heads stored (< nh: grouped-query attention)
        e["heads"] = o.nh;
        e["head_dim"] = o.hd;
        Json cols = Json::array(), lds = Json::array();  // column offset / row pitch of Q, K, V in their buffers
        for (int r = 0; r < 3; ++r) {
          cols.push_back(o.col[r]);
          lds.push_back(o.ld[r]);
        }
        e["cols"] = cols;
        e["lds"] = lds;
        if (o.bias_heads) {  // the folded table, back in natural units: sum of its finite entries, count of -inf
          const int Sp = kern::key_pitch(o.S);
          const float* t = reinterpret_cast<const float*>(p.params.data() + o.bias_off);
          double sum = 0;
          long long masked = 0;
          for (long long row = 0; row < static_cast<long long>(o.bias_heads) * o.S; ++row)
            for (int c = 0; c < o.S; ++c) {
              const float v = t[row * Sp + c];
              if (std::isfinite(v)) sum += v;
              else ++masked;
            }
          e["bias_sum"] = sum / 1.4426950408889634;
          e["bias_masked"] = masked;
        }
      }
      if (o.kind == PlanOp::EMBED_TOKENS) {
        e["vocab"] = o.gidx;
        e["seq"] = o.S;
        e["dim"] = o.Cp;
        e["positions"] = o.shift_off != SIZE_MAX;
        e["token_type"] = o.bias_off != SIZE_MAX;
        e["key_data"] = o.out2 >= 0;
        if (o.in_ld > 0) {  // several graph inputs: where each segment sits in a request row
          e["row_pitch"] = o.in_ld;
          e["ids_offset"] = o.seg_ids;
          e["types_offset"] = o.seg_types;  // -1: no type input
          e["type_rows"] = o.type_rows;
          e["token_type"] = o.bias_off != SIZE_MAX || o.seg_types >= 0;
          e["mask_offset"] = pad_reads_mask(o) ? o.pad.src : -1;  // -1: the pad test reads the ids
        }
        if (o.out2 >= 0) {
          static const char* cmp[] = {"equal", "greater", "less"};
          e["pad_op"] = cmp[o.pad.op];
          e["pad_value"] = static_cast<double>(o.pad.value);
          e["pad_negated"] = o.pad.negated;
          e["pad_truncated"] = o.pad.truncated;
        }
      }
      if (o.kind == PlanOp::POOL_TOKENS) {
        e["masked"] = o.key_mask != 0;  // mean over the visible tokens (key data from the embed_tokens op)
        e["normalize"] = o.normalize;
        e["clip_min"] = static_cast<double>(o.count_min);
        e["eps"] = static_cast<double>(o.eps);
        e["seq"] = o.S;
        e["dim"] = o.Cp;
      }
      if (o.kind == PlanOp::LAYERNORM) {
        e["stats_only"] = o.stats_only != 0;
        e["rms"] = o.rms != 0;
        e["rows"] = o.rows_per_sample;
      }
      if (o.kind == PlanOp::GCONV) {
        e["tiled"] = o.tiled != 0;  // in the scope of the tiled depthwise kernel (kernels/dwconv.hip)
        e["KH"] = o.kh;
        e["stride"] = o.sh;
        e["groups"] = o.groups;
        e["residual"] = o.in2 >= 0;
      }
      if (o.kind == PlanOp::ROPE) {
        e["heads"] = o.nh;
        e["head_dim"] = o.hd;
        e["seq"] = o.S;
        e["ld_in"] = o.ld[0];
        e["col"] = o.col[0];
        e["layout"] = o.gidx ? "nshd" : "nhsd";  // the logical head view the rotation was written on
      }
      if (o.kind == PlanOp::GROUPNORM) {
        e["groups"] = o.groups;  // == channels: InstanceNorm
        e["channels"] = o.Cp;
        e["stored_channels"] = o.C;
        e["pixels"] = o.H * o.W;
        e["act"] = o.act;  // 0 none, 1 ReLU, 2 SiLU
        e["eps"] = static_cast<double>(o.eps);
      }
      if (o.kind == PlanOp::GRN) {
        e["C"] = o.C;
        e["rows"] = o.H * o.W;  // pixels of the map
        e["eps"] = static_cast<double>(o.eps);
        e["gamma"] = o.scale_off != SIZE_MAX;
        e["beta"] = o.shift_off != SIZE_MAX;
      }
      if (o.kind == PlanOp::CONV || o.kind == PlanOp::TOKENS) e["stats_out"] = o.out_stats >= 0;  // writes the partials
      if (o.kind == PlanOp::STEM) {
        e["pool_fused"] = o.is_max != 0;
        e["rows"] = o.is_max ? o.Ho * o.Wo : o.conv.Ho * o.conv.Wo;
      }
      if (o.kind == PlanOp::CONV_PAIR) {
        e["K1"] = o.conv.K;
        e["N1"] = o.conv.N;
        e["N2"] = o.n2;
        e["residual"] = o.in2 >= 0;
        e["store_main"] = o.out >= 0;
        e["store_preact"] = o.out3 >= 0;
        e["relu"] = o.pair_relu;
        e["rows"] = o.conv.Ho * o.conv.Wo;
      }
      ops.push_back(e);
    }
    j["ops"] = ops;
    Json in = Json::array(), out = Json::array();
    for (auto d : p.input_shape) in.push_back(static_cast<long long>(d));
    for (auto d : p.output_shape) out.push_back(static_cast<long long>(d));
    j["input_shape"] = in;
    j["output_shape"] = out;
    j["inputs"] = input_segments_json(p.inputs);
    return dup(j.dump());
  } catch (const std::exception& e) {
    if (err) *err = dup(e.what());
    return nullptr;
  }
}

}  // extern "C"
