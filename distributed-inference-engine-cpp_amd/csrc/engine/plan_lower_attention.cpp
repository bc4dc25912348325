// Transformer views and the attention chain:
//  * transformers (ViT): the patch Conv's Reshape/Transpose, the heads Reshape/Transpose, the
//    MatMul -> Div -> Softmax -> MatMul chain and the shape-computation subgraph are all lazy views;
//    the chain materialises as one fused attention kernel when the context is merged back into rows.
//    Between Q K^T and the Softmax the chain also takes, in any number and order, Add(scores, B)
//    with a float initializer B and Where(C, scores, f) / Where(C, f, scores) with a bool
//    initializer C and a scalar fill f <= -1e4 (taken as -inf), B / C broadcastable to
//    [1, nh, S, S] (rank 2 to 4, leading dims 1 or nh, last two (S, S), (1, S) or (S, 1)).  They
//    fold into one additive table per attention (a later scale multiplies it, Adds sum), which is
//    classified: a -inf strict upper triangle becomes the kernel's causal flag, equal heads one
//    shared slice, an all-zero remainder no table at all (causal masks, relative-position / ALiBi
//    tables, BERT key masks, sliding windows).  Rejected with a report line: shapes that do not
//    broadcast, a finite fill above -1e4, a query row with no visible key, and a mask that is not an
//    initializer -- folding of mask-building Slice / Cast subgraphs, cross-attention and KV caches
//    are out of scope.
//  * grouped-query attention: HF's repeat_kv on a K / V heads view is a view of the same buffer.
//  * rotary position embeddings: on a heads view x ([N, H, S, hd] after the head transpose, or
//    [N, S, H, hd] before it) the seven nodes Mul(x, COS), Slice(x, 0:hd/2), Slice(x, hd/2:hd), Neg,
//    Concat([-hi, lo]), Mul(., SIN), Add are one ROPE op with the two float initializers as [S][hd]
//    tables; its output is a heads view on a new dense rows buffer, so the attention lowering is
//    unchanged (one launch each for Q and K).  Rejected with a report line: halves that do not meet
//    at hd/2 or a step != 1 (interleaved), rotation of fewer than hd columns (partial), tables that
//    are not initializers or do not broadcast over [S, hd], a head dim attention does not take.
#include "planner.h"

namespace die {

// ---- transformer views / ops --------------------------------------------------------------------
// The axes of a Reduce* / Unsqueeze node: the attribute, or (opset 13+) input 1.  False when there
// are none or they are not known.
bool Planner::node_axes(const Node& n, std::vector<int64_t>& ax) const {
  ax = n.get_ints("axes");
  if (ax.empty() && n.inputs.size() > 1 && !n.in(1).empty()) return ints_of(n.in(1), ax) && !ax.empty();
  return !ax.empty();
}

bool Planner::ints_of(const std::string& nm, std::vector<int64_t>& out) const {
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
bool Planner::lower_shape_op(int idx) {
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
bool Planner::kv_repeat_node(const Node& n) const {
  for (size_t i = 0; i < n.inputs.size(); ++i) {
    auto it = vid_.find(n.inputs[i]);
    if (it == vid_.end()) continue;
    const Val& x = vals_[it->second];
    if (x.kind == Val::KVREP) return true;
    if (i == 0 && x.kind == Val::HEADS && n.op_type == "Unsqueeze") return true;
  }
  return false;
}

void Planner::lower_kv_repeat(int idx) {
  const Node& n = m_.nodes[idx];
  const Val x = val(n.in(0), n);
  const std::array<int, 4> bhsd{{0, 2, 1, 3}};
  if (n.op_type == "Unsqueeze" && x.kind == Val::HEADS) {
    std::vector<int64_t> ax;
    if (x.perm == std::array<int, 4>{{0, 1, 2, 3}})
      reject(n, "a K/V repeat on the [N, S, H, hd] layout, before the head Transpose, is not "
             "supported (repeat_kv is matched on [N, Hkv, S, hd], after the Transpose and any rotary "
             "embedding)");
    if (x.perm != bhsd || !node_axes(n, ax) || ax != std::vector<int64_t>{2})
      reject(n, "a heads view is unsqueezed only as the first node of repeat_kv: axes [2] on "
             "[N, Hkv, S, hd]");
    if (x.kvg) reject(n, "the heads view already carries a K/V repeat");
    if (graph_outputs_.count(n.outputs[0])) reject(n, "a heads view cannot be a graph output");
    Val o = x;
    o.kind = Val::KVREP;
    o.stage = 1;
    define(n.outputs[0], o);
    return;
  }
  if (x.kind != Val::KVREP)
    reject(n, "reads a K/V repeat in progress: repeat_kv is Unsqueeze -> Expand -> Reshape on the "
           "heads view alone");
  const int Hkv = x.nh, S = x.H, hd = x.hd;
  if (n.op_type == "Expand" && x.stage == 1) {
    std::vector<int64_t> e;
    if (n.inputs.size() < 2 || !ints_of(n.in(1), e))
      reject(n, "the shape of a K/V repeat must be static (a constant, or folded from Shape nodes)");
    const bool ok = e.size() == 5 && (e[0] == 1 || e[0] == kBatchDim) && (e[1] == 1 || e[1] == Hkv) && e[2] >= 1 &&
                    (e[3] == 1 || e[3] == S) && (e[4] == 1 || e[4] == hd);
    if (!ok) {
      std::string shp;
      for (auto d : e) shp += (shp.empty() ? "" : ", ") + (d == kBatchDim ? std::string("N") : std::to_string(d));
      reject(n, "a K/V repeat expands axis 2 alone, [N, " + std::to_string(Hkv) + ", 1, " +
             std::to_string(S) + ", " + std::to_string(hd) + "] -> [N, " + std::to_string(Hkv) + ", G, " +
             std::to_string(S) + ", " + std::to_string(hd) + "]; got the shape [" + shp + "]");
    }
    if (graph_outputs_.count(n.outputs[0])) reject(n, "a heads view cannot be a graph output");
    Val o = x;
    o.stage = 2;
    o.kvg = static_cast<int>(e[2]);
    define(n.outputs[0], o);
    return;
  }
  if (n.op_type == "Reshape" && x.stage == 2) {
    std::vector<int64_t> shp;
    if (!ints_of(n.in(1), shp)) reject(n, "target shape must be static");
    const int G = x.kvg;
    const bool ok = shp.size() == 4 && (shp[0] == 0 || shp[0] == -1 || shp[0] == kBatchDim) &&
                    shp[1] == static_cast<int64_t>(Hkv) * G && shp[2] == S && shp[3] == hd;
    if (!ok)
      reject(n, "a K/V repeat ends in a Reshape to [N, Hkv * G, S, hd] = [N, " +
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
      reject(n, "the repeated K/V view is read by " + bad + ": only the attention MatMuls (and the "
             "Transpose of K before Q K^T) may read it -- the repeat is never materialised");
    Val o = x;
    o.kind = Val::HEADS;
    o.stage = 0;
    o.nh = Hkv * G;
    define(n.outputs[0], o);
    return;
  }
  reject(n, "reads a K/V repeat in progress: repeat_kv is Unsqueeze(axes [2]) -> Expand -> Reshape "
         "on the heads view alone");
}

// ---- attention bias / mask folding --------------------------------------------------------------
// Between Q K^T and the Softmax a chain may hold, besides the scalar Div / Mul, any number of
// Add(scores, B) and Where(C, scores, f) nodes with B / C initializers broadcastable to
// [1, nh, S, S].  They fold at plan time into one dense additive table per attention, in the
// softmax's natural units: scores' = scale * (Q K^T) + table.  A later scale multiplies the table
// too, several Adds sum, a Where puts -inf at its masked positions.  emit_attention classifies
// the table (causal flag, shared / per-head, nothing left) and stores it.

// Add / Where with an attention-scores operand (stage 0)
bool Planner::attn_mask_node(const Node& n) const {
  if (n.op_type != "Add" && n.op_type != "Where") return false;
  for (const auto& in : n.inputs) {
    auto it = vid_.find(in);
    if (it != vid_.end() && vals_[it->second].kind == Val::ATTN && vals_[it->second].stage == 0) return true;
  }
  return false;
}

// The table of scores value x with room for `heads` slices (zeros when x has none yet).
Planner::AttnTable Planner::attn_table(const Val& x, int heads) const {
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
void Planner::define_masked(const Node& n, const Val& x, AttnTable t) {
  const int S = vals_[x.q].H;
  for (int h = 0; h < t.heads; ++h)
    for (int i = 0; i < S; ++i) {
      const float* row = t.t.data() + (static_cast<size_t>(h) * S + i) * S;
      bool visible = false;
      for (int j = 0; j < S; ++j) {
        if (std::isnan(row[j]) || row[j] == INFINITY)
          reject(n, "the folded attention bias has a NaN / +inf entry (a mask "
                 "scaled by a constant that is not positive?)");
        visible = visible || std::isfinite(row[j]);
      }
      if (!visible)
        reject(n, "attention mask leaves query row " + std::to_string(i) +
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
void Planner::lower_attn_mask(const Node& n, const Val& x, const std::string& tname, int mode) {
  const std::string what = mode == 0 ? "bias" : "mask";
  auto it = m_.initializers.find(tname);
  if (it == m_.initializers.end())
    reject(n, "the attention " + what + " " + tname +
           " must be an initializer, or a key mask derived from the token ids (see the report line of "
           "the node producing it); other masks that depend on the input, and folding a mask the "
           "exporter left as a Slice / Cast / ... subgraph of constants, are out of scope");
  const onnx::Tensor& c = it->second;
  const int S = vals_[x.q].H, nh = vals_[x.q].nh;
  const size_t r = c.dims.size();
  const bool typed = mode == 0 ? onnx::is_float_type(c.dtype) && static_cast<int64_t>(c.f.size()) == c.numel()
                               : c.dtype == onnx::BOOL && static_cast<int64_t>(c.i.size()) == c.numel();
  if (!typed)
    reject(n, "the attention " + what + " " + tname + " must be a " +
           (mode == 0 ? "float" : "bool") + " tensor");
  // right-aligned against [1, nh, S, S]: rank 2..4, leading dims 1 or nh, last two (S, S), (1, S) or (S, 1)
  const int64_t dc = r >= 1 ? c.dims[r - 1] : 0, dr = r >= 2 ? c.dims[r - 2] : 0, dh = r >= 3 ? c.dims[r - 3] : 1,
                db = r >= 4 ? c.dims[0] : 1;
  const bool rows_ok = (dr == S && dc == S) || (dr == 1 && dc == S) || (dr == S && dc == 1);
  if (r < 2 || r > 4 || db != 1 || (dh != 1 && dh != nh) || !rows_ok) {
    std::string shape;
    for (auto d : c.dims) shape += (shape.empty() ? "" : ", ") + std::to_string(d);
    reject(n, "attention " + what + " " + tname + " [" + shape +
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
int Planner::emit_attention(const Val& ctx, const std::string& name) {
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

void Planner::lower_reshape(int idx) {
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

void Planner::lower_transpose(int idx) {
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

void Planner::lower_attn_matmul(int idx) {
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

void Planner::lower_scale(int idx) {
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
      if (x.kmask && !(it->second.f[0] > 0.f)) reject(n, "a scale after a key mask must be positive");
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
      else reject(n, "constant / activation is not supported");
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
  reject(n, "unsupported elementwise op for the HIP engine");
}

void Planner::lower_softmax(int idx) {
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

// ---- rotary position embeddings ---------------------------------------------------------------------
// On a heads view x, [N, H, S, hd] (perm {0,2,1,3}) or [N, S, H, hd] (identity), torch's
// x * cos + rotate_half(x) * sin exports as Mul(x, COS), Slice(x, 0:hd/2), Slice(x, hd/2:hd), Neg(hi),
// Concat([-hi, lo], -1), Mul(., SIN), Add.  A Mul or a last-axis Slice reading such a view is one of
// x's three readers in that pattern or an error; the whole pattern is one ROPE op.
int Planner::rope_layout(const Val& v) {
  if (v.kind != Val::HEADS) return -1;
  if (v.perm == std::array<int, 4>{{0, 2, 1, 3}}) return 0;
  if (v.perm == std::array<int, 4>{{0, 1, 2, 3}}) return 1;
  return -1;
}

// the heads-view operand of a Mul / Slice (-1: none)
int Planner::rope_operand(const Node& n) const {
  const int k = n.op_type == "Slice" ? 1 : 2;
  for (int side = 0; side < k && side < static_cast<int>(n.inputs.size()); ++side) {
    auto it = vid_.find(n.in(side));
    if (it != vid_.end() && rope_layout(vals_[it->second]) >= 0) return side;
  }
  return -1;
}

// a Slice of a heads view, or a Mul of one that a Slice reads too (a Mul alone keeps its other lowerings)
bool Planner::rope_anchor(const Node& n) const {
  const int side = rope_operand(n);
  if (side < 0 || n.op_type == "Slice") return side >= 0;
  for (int c : consumers(n.in(side)))
    if (m_.nodes[c].op_type == "Slice" && m_.nodes[c].in(0) == n.in(side)) return true;
  return false;
}

// starts / ends / axes / steps of a one-axis Slice (attributes or inputs); false when not static
bool Planner::slice_range(const Node& n, int64_t& s0, int64_t& e0, int64_t& axis, int64_t& step) const {
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
std::vector<float> Planner::rope_table(const Node& at, const std::string& name, const Val& x, int layout) const {
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

void Planner::lower_rope(int idx) {
  const Node& n = m_.nodes[idx];
  const std::string& xn = n.in(rope_operand(n));
  const Val x = val(xn, n);
  const int layout = rope_layout(x), hd = x.hd, h2 = x.hd / 2;
  if (graph_outputs_.count(xn)) reject(n, "a heads view cannot be a graph output");
  // x's readers in the pattern: the Mul by COS and the two half Slices
  int mul_cos = -1, lo = -1, hi = -1;
  for (int c : consumers(xn)) {
    const Node& q = m_.nodes[c];
    if (done_[c] && c != idx) continue;
    if (q.op_type == "Mul" && q.inputs.size() == 2 && q.in(0) != q.in(1)) {
      if (mul_cos >= 0) reject(n, "two Muls (" + m_.nodes[mul_cos].name + ", " + q.name + ") read the heads view " + xn + ": not a rotary embedding");
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
    reject(n, "a Mul / Slice of a heads view is supported only as part of a rotary embedding over all hd "
           "columns: Mul(x, COS), Slice(x, 0:hd/2), Slice(x, hd/2:hd) (partial rotary is not supported)");
  const Node& mc = m_.nodes[mul_cos];
  const int neg = next_op(m_.nodes[hi].outputs[0], "Neg");
  if (neg < 0)
    throw std::runtime_error("Slice " + m_.nodes[hi].name + ": the high half of a rotary embedding must be read by a Neg alone "
                             "(partial rotary with a pass-through half is not supported)");
  const int cat = sole_consumer(m_.nodes[neg].outputs[0]);
  const int cat2 = sole_consumer(m_.nodes[lo].outputs[0]);
  if (cat < 0 || cat != cat2 || m_.nodes[cat].op_type != "Concat" || m_.nodes[cat].inputs.size() != 2 ||
      m_.nodes[cat].in(0) != m_.nodes[neg].outputs[0] || m_.nodes[cat].in(1) != m_.nodes[lo].outputs[0] ||
      !(m_.nodes[cat].get_int("axis", 0) == -1 || m_.nodes[cat].get_int("axis", 0) == 3))
    throw std::runtime_error("Slice " + m_.nodes[lo].name + ": the halves of a rotary embedding must meet in Concat([-hi, lo], "
                             "axis -1)");
  const int mul_sin = next_op(m_.nodes[cat].outputs[0], "Mul");
  if (mul_sin < 0)
    throw std::runtime_error("Concat " + m_.nodes[cat].name + ": the rotated halves must be multiplied by the SIN table");
  const Node& ms = m_.nodes[mul_sin];
  const int add = sole_consumer(ms.outputs[0]);
  if (add < 0 || add != sole_consumer(mc.outputs[0]) || m_.nodes[add].op_type != "Add" || m_.nodes[add].inputs.size() != 2)
    throw std::runtime_error("Mul " + ms.name + ": x * COS and rotate_half(x) * SIN must meet in one Add");
  if (!kern::attention_supported(hd, x.H))
    reject(n, "rotary embedding on head dim " + std::to_string(hd) + ": needs a head dim the attention "
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

// The other branch `fill` of the Where `n` on attention scores: a scalar initializer <= -1e4.
void Planner::check_score_fill(const Node& n, const std::string& fill) const {
  float f = 0.f;
  if (!scalar_init(fill, f))
    throw std::runtime_error("Where " + n.name + ": on attention scores the other branch must be a scalar initializer");
  if (!(f <= -1e4f))
    throw std::runtime_error("Where " + n.name + ": fill " + std::to_string(f) + " is not a mask (only fills <= -1e4 or "
                             "-inf fold into the attention kernel as -inf); a finite fill above -1e4 is not supported");
}

}  // namespace die
