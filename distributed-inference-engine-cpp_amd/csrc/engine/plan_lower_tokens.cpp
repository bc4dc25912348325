// Token models:
//  * ViT token assembly: cls Expand/Concat + position Add -> one token-assembly kernel;
//    Gather(token) -> a row kernel.
//  * token-id models: a rank-2 input [N, S] whose consumers all treat it as ids (Cast to an integer
//    type, Gather indices, Equal / Greater / Less against a scalar) gets no ROWS_PREP;
//    Gather(table, ids, axis 0) [+ Add(positions)] [+ Add(token-type row)] is one EMBED_TOKENS op
//    reading the fp32 input in place, and a padding mask derived from the ids (a pad test through
//    Not / Cast / Unsqueeze / Reshape / Sub(1, m) / Mul(m, c <= -1e4)) consumed on attention scores
//    as Where(vis, scores, f), Where(hidden, f, scores) or Add(scores, additive) becomes the
//    attention op's key_mask flag: EMBED_TOKENS writes the per-sample key data once per forward.
//    Rejected with a report line: key mask + causal, a visibility value used in any other way,
//    Gather on another axis or from a non-initializer table, mask shapes other than
//    [N, 1, 1, S].
//  * attention_mask / token_type_ids graph inputs: 2 or 3 rank-2 inputs [N, S] with one S, declared
//    FLOAT / INT64 / INT32 in any order; a request row is their concatenation in declaration order
//    and is read in place.  Roles come from use: an input that only indexes Gather(initializer
//    [V, D], ., axis 0) is ids or types (the earlier-declared of two is the ids), and the two lookups,
//    summed by Add with each other and the position Add in any order, are one EMBED_TOKENS op (a
//    constant type row and a type input exclude each other); an input that is a visibility value
//    roots the key-mask machinery above as the pad test "value != 0" read from the mask segment
//    (values other than 0 / 1 are outside the contract: non-zero is visible).  Rejected with a
//    report line naming the input (define_token_inputs in hip_plan.cpp): different S or rank, more
//    than 3 inputs, an input that is neither, one used both ways, a second input on a model without
//    token ids; a mask input plus a different ids-derived pad test is two pad tests.  Such a model
//    is never partitioned.
//  * sentence embedders: the masked mean over the tokens, Mul(rows, m) -> ReduceSum(axis 1) divided by
//    ReduceSum(m, axis 1) [-> Clip(min) / Max] with m = the same visibility value unsqueezed at the
//    last axis [-> Expand to [N, S, D]] -> Cast, is one POOL_TOKENS op reading the key data; an L2
//    normalisation of rank-2 rows over the last axis (LpNormalization p = 2, or torch's F.normalize
//    export ReduceL2 -> Clip(min = eps) -> [Expand] -> Div) joins that op when the pooled vector has
//    no other reader and is a POOL_TOKENS op with S = 1 anywhere else.  As the graph output the op
//    writes fp32 straight into the output buffer.  Sum / max / last-token pooling: out of scope.
#include "planner.h"

namespace die {

// ---- token-id models: embedding lookup and the request's own key (padding) mask ------------------
// A rank-2 graph input [N, S] is a token input when every consumer treats it as ids: an optional
// Cast to INT64 / INT32, the indices of a Gather, and the pad tests Equal / Greater / Less against
// a scalar initializer -- and at least one Gather reads it (any other rank-2 input plans as rows).
// Whether the Gather is one the engine lowers (axis 0, an initializer table) is lower_embed's
// business: a token input with a Gather it rejects gives that report line.
bool Planner::token_input(const std::string& name) const {
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
bool Planner::token_node(const Node& n) const {
  for (const auto& in : n.inputs) {
    auto it = vid_.find(in);
    if (it != vid_.end() && (vals_[it->second].kind == Val::TOKEN_IDS || vals_[it->second].kind == Val::KEYVIS ||
                             vals_[it->second].kind == Val::POOLV))
      return true;
  }
  return false;
}

const Val* Planner::val_if(const std::string& name, Val::Kind kind) const {
  auto it = vid_.find(name);
  return it != vid_.end() && vals_[it->second].kind == kind ? &vals_[it->second] : nullptr;
}

// The token-id value `name` is, or is a Cast to INT64 / INT32 of (a Cast that need not be lowered yet)
const Val* Planner::ids_behind(std::string name) const {
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

void Planner::lower_token_node(int idx) {
  const Node& n = m_.nodes[idx];
  const std::string& op = n.op_type;
  if (lower_pool_node(idx)) return;
  if (const Val* ids = n.inputs.empty() ? nullptr : val_if(n.in(0), Val::TOKEN_IDS)) {
    if (op == "Cast") {
      const int to = static_cast<int>(n.get_int("to", onnx::FLOAT));
      if (to != onnx::INT64 && to != onnx::INT32) reject(n, "token ids cast only to INT64 / INT32");
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
    reject(n, "token ids compare only with a scalar initializer");
  }
  // consumers on attention scores: Where(vis, scores, f), Where(hidden, f, scores), Add(scores, additive)
  if (op == "Where" && n.inputs.size() == 3) {
    const Val* m = val_if(n.in(0), Val::KEYVIS);
    for (int side = 1; side <= 2 && m; ++side) {
      const Val* x = val_if(n.in(side), Val::ATTN);
      if (!x || x->stage != 0) continue;
      check_score_fill(n, n.in(3 - side));
      if (m->kv_add) reject(n, "the condition must be a boolean key mask");
      return define_key_masked(n, *x, *m, side == 1);
    }
  }
  if (op == "Add" && n.inputs.size() == 2)
    for (int side = 0; side < 2; ++side) {
      const Val* m = val_if(n.in(side), Val::KEYVIS);
      const Val* x = val_if(n.in(1 - side), Val::ATTN);
      if (!m || !x || x->stage != 0) continue;
      if (!m->kv_add) reject(n, "a key mask added to attention scores must be additive (mask * c with c <= -1e4)");
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
    if (!ok) reject(n, "a key mask is unsqueezed only towards [N, 1, 1, S]");
    define(n.outputs[0], o);
    return;
  }
  if (m && op == "Reshape") {
    std::vector<int64_t> shp;
    const bool ok = ints_of(n.in(1), shp) && shp.size() == 4 && (shp[0] == 0 || shp[0] == -1 || shp[0] == kBatchDim) &&
                    shp[1] == 1 && shp[2] == 1 && (shp[3] == m->H || (shp[3] == -1 && shp[0] != -1));
    if (!ok) reject(n, "a key mask is reshaped only to [N, 1, 1, S]");
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
        reject(n, "a key mask times " + std::to_string(c) + " is not a mask (only factors <= -1e4 "
               "fold into the attention kernel as -inf)");
      Val o = *s;
      o.kv_add = true;
      define(n.outputs[0], o);
      return;
    }
  reject(n, "token ids feed only a Cast to INT64 / INT32, an embedding Gather (axis 0) and the pad "
         "tests Equal / Greater / Less, and a key mask derived from them only Not, Cast, Unsqueeze / "
         "Reshape to [N, 1, 1, S], Sub(1, m), Mul(m, c <= -1e4), the Where / Add on attention scores and "
         "the masked mean over the tokens (Unsqueeze(-1), Expand to [N, S, D], Mul(rows, m), "
         "ReduceSum(m, axis 1)); other uses are out of scope");
}

// Gather(table [V, D] float initializer, ids, axis 0) [+ Add(positions [S, D] / [1, S, D])]
// [+ Add(token-type row [D] / [1, 1, D])] -> one EMBED_TOKENS op producing rows [N, S, D].
void Planner::lower_embed(int idx) {
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
    const int ci = next_op(out, "Add");
    if (ci < 0 || m_.nodes[ci].inputs.size() != 2) break;
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
void Planner::define_key_masked(const Node& n, const Val& x, const Val& m, bool vis_when_true) {
  const std::string who = n.op_type + " " + n.name + ": ";
  if (m.kv_rank != 4)
    reject(n, "a key mask on attention scores must have the shape [N, 1, 1, S] (rank " +
           std::to_string(m.kv_rank) + " here)");
  if (m.H != vals_[x.q].H) reject(n, "the key mask's length is not the attention's");
  bind_key_test(who, m, vis_when_true);
  Val o = x;
  o.kmask = true;
  define(n.outputs[0], o);
}

// The model's one pad test, on the EMBED_TOKENS op that writes the key data (kvis, kend) for it:
// set by the first user (an attention or the token pooling), compared by every later one.
void Planner::bind_key_test(const std::string& who, const Val& m, bool vis_when_true) {
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
bool Planner::masked_sum_shape(const std::string& name) const {
  auto r = producer_.find(name);
  if (r == producer_.end() || m_.nodes[r->second].op_type != "ReduceSum" || m_.nodes[r->second].inputs.empty()) return false;
  auto q = producer_.find(m_.nodes[r->second].in(0));
  return q != producer_.end() && m_.nodes[q->second].op_type == "Mul";
}

bool Planner::lower_pool_node(int idx) {
  const Node& n = m_.nodes[idx];
  const std::string& op = n.op_type;
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
    reject(n, "a key mask [N, S, 1] goes only through Expand to [N, S, D], Cast and Not (masked mean pooling)");
  if (m && m->kv_last && op == "Expand") {
    std::vector<int64_t> shp;
    const bool ok = n.inputs.size() == 2 && ints_of(n.in(1), shp) && shp.size() == 3 && (shp[0] == 1 || shp[0] == kBatchDim) &&
                    (shp[1] == 1 || shp[1] == m->H) && shp[2] >= 1 && !m->kv_D;
    if (!ok) reject(n, "a key mask [N, S, 1] expands only to [N, S, D]");
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
        reject(n, "rows [N, S, D] are multiplied only by a key mask of the shape [N, S, 1] or [N, S, D] (masked mean pooling)");
      if (!dense(*x)) reject(n, "the masked rows must be dense");
      const int S = x->H * x->W;
      if (s->H != S)
        reject(n, "the key mask's length " + std::to_string(s->H) + " is not the rows' " + std::to_string(S));
      if (s->kv_D && s->kv_D != x->logical() && s->kv_D != x->C) reject(n, "the expanded key mask's width is not the rows'");
      const int r = sole_consumer(n.outputs[0]);
      std::vector<int64_t> ax;
      if (r < 0 || m_.nodes[r].op_type != "ReduceSum" || !node_axes(m_.nodes[r], ax) || ax.size() != 1 ||
          !(ax[0] == 1 || ax[0] == -2) || m_.nodes[r].get_int("keepdims", 1) != 0)
        reject(n, "rows times a key mask feed only ReduceSum(axis 1, keepdims 0), the masked sum over the tokens");
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
      if (r->stage != 0) reject(n, "only rows times a key mask are summed over the tokens");
      const int d = next_op(n.outputs[0], "Div");
      if (d < 0 || m_.nodes[d].inputs.size() != 2 || m_.nodes[d].in(0) != n.outputs[0] ||
          m_.nodes[d].in(1) == n.outputs[0])
        reject(n, "a masked sum over the tokens must be divided by the count of visible tokens (masked mean pooling; sum "
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
        reject(n, "a key mask is summed only over the token axis, to the count of visible tokens [N, D] or [N, 1] (masked "
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
          reject(n, "the count of a key mask's visible tokens must end, through Clip(min) / Max, as the divisor of the masked "
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
      if (c->stage != 2) reject(n, "only the count of visible tokens is clipped (masked mean pooling)");
      float lo = 0.f, hi = 3.4e38f;
      if (op == "Clip") {
        if (!clip_bounds(n, lo, hi)) reject(n, "bounds must be constants");
        if (hi < 3.4e38f) reject(n, "a Clip with a max on the count of visible tokens is not supported (only a lower bound)");
        if (lo == -3.4e38f) lo = 0.f;
      } else if (n.inputs.size() != 2 || !scalar_init(n.in(1 - side), lo)) {
        reject(n, "the count of visible tokens is bounded only by a scalar initializer");
      }
      if (!(lo >= 0.f)) reject(n, "the lower bound of the count of visible tokens must be >= 0");
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
        reject(n, "masked mean pooling divides the masked sum over the tokens by the count of visible tokens, nothing else");
      if (!(a->pad == b->pad))
        reject(n, "the count is not over the visibility value of the masked sum (different pad tests)");
      if (b->kv_D && b->kv_D != a->logical() && b->kv_D != a->C) reject(n, "the count's width is not the masked sum's");
      const Val rows = *a, vis = *a;
      emit_pool_tokens(n, rows, rows.H, &vis, b->pool_c, n.outputs[0], true, false, 0.f);
      return true;
    }
  }
  for (const auto& in : n.inputs)
    if (val_if(in, Val::POOLV))
      reject(n, "a masked sum / count of visible tokens feeds only Clip(min) / Max and the Div that closes the masked mean");
  return false;
}

// ReduceL2(x, last axis, keepdims 1) [-> Clip(min = eps) | Max(., eps)] [-> Expand] -> Div(x, .), from
// the ReduceL2 node: torch's export of F.normalize.  False with a reason when it is something else.
// The Expand's shape is constant or Shape(x); used lists the chain's nodes, the Div last, and
// shape_node that Shape (-1: none).
bool Planner::l2_chain(int ridx, int rank, float& eps, std::string& out, std::vector<int>& used, std::string& why,
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
bool Planner::only_l2_normalized(const std::string& x, float& eps, std::string& out, std::vector<int>& used) const {
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
void Planner::lower_l2norm(int idx) {
  const Node& n = m_.nodes[idx];
  if (grn_anchor(n)) return lower_grn(idx);  // two axes of an image / an [N, H, W, C] view: ConvNeXt-V2's GRN
  const Val x = val(n.in(0), n);
  const int rank = x.rank ? x.rank : 2;
  float eps = 0.f;
  std::string out = n.outputs[0];
  std::vector<int> used;
  if (n.op_type == "LpNormalization") {
    const int64_t axis = n.get_int("axis", -1);
    if (n.get_int("p", 2) != 2) reject(n, "only p = 2 (L2 normalisation) is supported");
    if (!(axis == -1 || axis == rank - 1)) reject(n, "only the last axis is normalised");
  } else {
    std::string why;
    int shape_node = -1;
    if (!l2_chain(idx, rank, eps, out, used, why, shape_node))
      reject(n, "only torch's export of F.normalize, ReduceL2(last axis, keepdims 1) -> Clip(min = eps) "
             "-> [Expand] -> Div(x, .), is supported (" + why + ")");
  }
  if (x.kind != Val::ROWS_BF16 || rank != 2 || x.H * x.W != 1 || !dense(x))
    reject(n, "only dense rank-2 rows [N, D] are L2-normalised");
  for (int u : used) done_[u] = true;
  emit_pool_tokens(n, x, 1, nullptr, 0.f, out, false, true, eps);
}

// One POOL_TOKENS op over the rows x ([S][C] per sample); vis: the key mask of a masked mean (nullptr:
// all S rows).  try_norm: an L2 normalisation that is the result's only reader joins the op.
void Planner::emit_pool_tokens(const Node& n, const Val& x, int S, const Val* vis, float clip_min, std::string out_name,
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

void Planner::lower_gather(int idx) {
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

void Planner::lower_concat(int idx) {
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
void Planner::emit_tokens(const Node& n, const Val& cat, const std::string* pos_name, const std::string& out_name) {
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

}  // namespace die
