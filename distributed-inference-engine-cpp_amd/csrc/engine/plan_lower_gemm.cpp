// Gemm / MatMul(2-D initializer) -> the same MFMA kernel as a 1x1 conv over rows.  Sibling Q/K/V
// MatMuls become one GEMM (N = 3*D); MatMul -> Add(bias) -> erf-GELU and MatMul -> Add(bias) ->
// Add(residual) fold into the GEMM epilogue; on a channels-last view (ConvNeXt) the layer-scale Mul
// folds into the weights and the Add of the shortcut image is the residual epilogue.
#include "planner.h"

namespace die {

// ---- GEMM over rows ---------------------------------------------------------------------------
bool Planner::scalar_is(const std::string& name, float want) const {
  auto it = m_.initializers.find(name);
  if (it == m_.initializers.end() || it->second.f.size() != 1) return false;
  return std::fabs(it->second.f[0] - want) <= 1e-3f * std::fabs(want);
}

// erf-GELU as exported by torch: x/sqrt2 -> Erf -> +1 -> (x * .) -> (* 0.5), or 0.5x * (1 + erf).
bool Planner::match_gelu(const std::string& v, std::vector<int>& used, std::string& out) const {
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
  const int er = next_op(m_.nodes[dv].outputs[0], "Erf");
  if (er < 0) return false;
  const int ad = next_op(m_.nodes[er].outputs[0], "Add");
  if (ad < 0 || !scalar_is(other_input(m_.nodes[ad], m_.nodes[er].outputs[0]), 1.f))
    return false;
  const std::string& a = m_.nodes[ad].outputs[0];
  const Node& M = m_.nodes[mu];
  const std::string& mo = other_input(M, v);
  if (mo == a) {
    const int hf = next_op(M.outputs[0], "Mul");
    if (hf < 0 || !scalar_is(other_input(m_.nodes[hf], M.outputs[0]), 0.5f)) return false;
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

// Epilogue fusion lookahead for a MatMul/Gemm producing `N` columns over `rows` rows per sample.
Planner::GemmTail Planner::gemm_tail(const Node& n, int N, int rows, bool is_gemm, int N_logical, const Val& x) const {
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
      const int c2 = next_op(m_.nodes[c1].outputs[0], "Add");
      if (c2 >= 0 && m_.nodes[c2].in(0) != m_.nodes[c2].in(1)) {
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
        const int c2 = next_op(t.out, "Relu");
        if (c2 >= 0) {
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
std::vector<int> Planner::qkv_group(int idx, const std::string& xname, int K) const {
  std::vector<int> g;
  bool self = false;
  for (int c : consumers(xname)) {
    if (c != idx && done_[c]) continue;
    const Node& nd = m_.nodes[c];
    if (nd.op_type != "MatMul" || nd.in(0) != xname || !is_init(nd.in(1))) continue;
    const auto& w = m_.initializers.at(nd.in(1));
    if (w.dims.size() != 2 || w.dims[0] != K || w.dims[1] % 8) continue;
    const int a = next_op(nd.outputs[0], "Add");
    if (a < 0 || !is_init(other_input(m_.nodes[a], nd.outputs[0]))) continue;
    if (m_.initializers.at(other_input(m_.nodes[a], nd.outputs[0])).f.size() != static_cast<size_t>(w.dims[1])) continue;
    const int r = next_op(m_.nodes[a].outputs[0], "Reshape");
    if (r < 0) continue;
    g.push_back(c);
    self |= c == idx;
  }
  if (!self || g.size() < 2) return {idx};
  return g;
}

void Planner::lower_gemm(int idx) {
  const Node& n = m_.nodes[idx];
  const Val x = val(n.in(0), n);
  const bool gemm = n.op_type == "Gemm";
  int rows = 1, rank = 2;
  if (x.kind == Val::ROWS_BF16) {
    rows = x.H * x.W;
    rank = x.rank ? x.rank : (rows == 1 ? 2 : 3);
  } else if (!(x.kind == Val::NHWC && x.H == 1 && x.W == 1)) {
    reject(n, "input must be a [batch, (tokens,) features] matrix");
  }
  if (x.pitch() != x.C || x.col) reject(n, "strided input rows");
  if (gemm && rank != 2) throw std::runtime_error("Gemm " + n.name + ": input must be 2-D");
  const auto& wt = init(n.in(1), n);
  if (wt.dims.size() != 2) reject(n, "weight must be 2-D");
  if (gemm && n.get_int("transA", 0)) throw std::runtime_error("Gemm " + n.name + ": transA is not supported");
  const bool tb = gemm && n.get_int("transB", 0);
  const float alpha = gemm ? n.get_float("alpha", 1.f) : 1.f;
  const float beta = gemm ? n.get_float("beta", 1.f) : 1.f;
  // K: the model's inner dimension; Ks: the stored row length (pads / NHWC-flatten order)
  const int K = static_cast<int>(tb ? wt.dims[1] : wt.dims[0]);
  const int Ks = x.C;
  const int hw = x.flat_hw;  // Flatten of an NHWC map: logical k = c*hw + p sits at p*Cs + c
  const int Kl = hw ? x.flat_c * hw : x.logical();
  if (K != Kl) reject(n, "inner dimension mismatch");
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

}  // namespace die
