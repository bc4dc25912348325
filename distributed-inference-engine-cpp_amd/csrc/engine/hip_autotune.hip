// HIP engine: start-up measurements -- the per-conv autotune, the in-graph retune and the
// per-batch-size curve of the captured forward.
//
// Autotune: time every (tile, split-K) candidate of every conv/GEMM at every bucket and keep the
// fastest.  Runs once at start-up on the real buffers (a full forward first, so inputs hold real
// data).  Candidates are timed one launch at a time behind an L2 scrub (EngineOptions::tune_cold =
// false: back-to-back launches instead): inside a forward a layer reads its input just written by
// the previous layer and its weights from the Infinity Cache, never a warm L2 -- warm back-to-back
// timing favoured shallow LDS rings whose load latency is exposed once the operands come from
// further away (stage-3 3x3 convs: 17.5 us tuned, 27 us in the graph).
#include "hip_engine.h"

namespace die {
namespace hip {

Tune HipEngine::tune_for(int B, size_t op_index) const {
  const size_t bi = bucket_index(B);
  if (bi < tune_.size() && op_index < tune_[bi].size() && tune_[bi][op_index].tile >= 0) return tune_[bi][op_index];
  const PlanOp& op = plan_.ops[op_index];
  const int M = B * op.conv.Ho * op.conv.Wo;
  Tune t;
  t.tile = kern::choose_tile(M, op.conv.N, op.conv.K);
  t.splits = kern::choose_splits(M, op.conv.N, op.conv.K, t.tile);
  t.fused = t.splits > 1 && !opt_.splitk_two_kernel;
  return t;
}

// Tune-cache / memo key of a conv problem: the shape, its epilogue, and the tuning regime.
std::string HipEngine::shape_key(const kern::ConvArgs& base, bool warm_input) const {
  char key[256];
  std::snprintf(key, sizeof(key), "o%s%s%s%s%s%s%s%d,%d,%d,%d,%d,%d,%d,%d,%d,%d,%d,%d,%d,%d,%d", opt_.tune_streamk ? "k:" : "",
                opt_.tune_tail ? "t:" : "",
                opt_.tune_cold ? "c:" : "",
                warm_input ? "w:" : "", sp_ ? "f32:" : "", base.stats_out || base.row_parts ? "ls:" : "",
                opt_.splitk_two_kernel ? (opt_.splitk_fused_margin > 0.f ? "fm:" : "sk2:") : (opt_.tune_orders ? "" : "o0:"),
                base.M, base.N, base.K, base.Cin, base.H, base.W, base.KH, base.KW, base.stride, base.pad_h, base.relu,
                base.res != nullptr, base.out2 != nullptr, base.out_f32 != nullptr, base.out != nullptr);
  return key;
}

void HipEngine::autotune() {
  Event e0, e1;
  HIP_CHECK(e0.create());
  HIP_CHECK(e1.create());
  const bool cold = opt_.tune_cold;
  constexpr size_t kScrubBytes = 96u << 20;
  DeviceMem<void> scrub;
  DeviceMem<float> sink;
  if (cold) {
    HIP_CHECK(scrub.alloc(kScrubBytes));
    HIP_CHECK(hipMemset(scrub, 0, kScrubBytes));
    HIP_CHECK(sink.alloc(sizeof(float)));
  }
  // One candidate's time in ms on the three-launch scale of the stored times, after its warm-up
  // launch.  producer >= 0 (EngineOptions::tune_warm_input): that op runs before every cold launch.
  auto time_candidate = [&](const kern::ConvArgs& a, int tile, int B, int producer) {
    float ms = 0;
    if (cold) {
      // median of 3 (x3, to keep the 3-launch scale of the stored times): one slow
      // repetition (a clock or queue hiccup) no longer decides the winner -- the mean
      // did, and repeated tunings of one model picked different tiles run to run
      float rep[3];
      for (int r = 0; r < 3; ++r) {
        HIP_CHECK(kern::l2_scrub(scrub, kScrubBytes, sink, s_compute_));
        if (producer >= 0)
          encode_forward(B, 0, s_compute_, nullptr, ALL, static_cast<size_t>(producer),
                         static_cast<size_t>(producer) + 1);
        HIP_CHECK(hipEventRecord(e0, s_compute_));
        HIP_CHECK(kern::conv_igemm(a, tile, s_compute_));
        HIP_CHECK(hipEventRecord(e1, s_compute_));
        HIP_CHECK(hipEventSynchronize(e1));
        HIP_CHECK(hipEventElapsedTime(&rep[r], e0, e1));
      }
      std::sort(rep, rep + 3);
      ms = 3.f * rep[1];
    } else {
      HIP_CHECK(hipEventRecord(e0, s_compute_));
      for (int r = 0; r < 3; ++r) HIP_CHECK(kern::conv_igemm(a, tile, s_compute_));
      HIP_CHECK(hipEventRecord(e1, s_compute_));
      HIP_CHECK(hipEventSynchronize(e1));
      HIP_CHECK(hipEventElapsedTime(&ms, e0, e1));
    }
    return ms;
  };
  tune_.assign(buckets_.size(), std::vector<Tune>(plan_.ops.size(), Tune{-1, 1}));
  double total_best_us = 0;
  TuneMap tuned_shapes;
  const std::string cache_path = tune_cache_path(opt_);
  const size_t loaded = load_tune_cache(cache_path, arch_, tuned_shapes);
  for (size_t bi = 0; bi < buckets_.size(); ++bi) {
    const int B = buckets_[bi];
    encode_forward(B, 0, s_compute_);
    HIP_CHECK(hipStreamSynchronize(s_compute_));
    for (size_t oi = 0; oi < plan_.ops.size(); ++oi) {
      const PlanOp& op = plan_.ops[oi];
      if (op.kind != PlanOp::CONV) continue;
      kern::ConvArgs base = conv_args(op, B, 0);
      base.ws = ws_;
      base.live = nullptr;  // tune the whole bucket
      // EngineOptions::tune_warm_input: the op that produced this conv's input runs right before
      // every timed launch (after the L2 scrub), so the candidate reads its input warm from the
      // producer and its weights cold -- as inside a forward
      int producer = -1;
      if (opt_.tune_warm_input)
        for (int j = static_cast<int>(oi) - 1; j >= 0 && producer < 0; --j) {
          const PlanOp& q = plan_.ops[static_cast<size_t>(j)];
          if ((q.out >= 0 && q.out == op.in) || (q.out2 >= 0 && q.out2 == op.in) || (q.out3 >= 0 && q.out3 == op.in))
            producer = j;
        }
      // identical problems (repeated blocks) share one measurement
      const std::string key = shape_key(base, producer >= 0);
      auto memo = tuned_shapes.find(key);
      // (a cached result without this run's candidate list is re-measured when the in-graph pass
      // needs the front runners -- unless that pass's own results are cached too)
      if (memo != tuned_shapes.end() && (!opt_.tune_in_graph || cands_.count(key) || in_graph_cached(tuned_shapes, B))) {
        tune_[bi][oi] = memo->second.first;
        if (B == max_batch_) total_best_us += memo->second.second;
        continue;
      }
      const int nk = base.Kpad / 64;
      float best = 1e30f, best_fused = 1e30f;
      Tune bt{kern::choose_tile(base.M, base.N, base.K), 1}, bt_fused = bt;
      std::vector<std::pair<float, Tune>> measured;  // every valid candidate (in-graph retune)
      for (int tile = 0; tile < kern::NUM_CFGS; ++tile) {
        for (int sp = 1; sp <= 16; sp *= 2) {
          if (sp > 1 && (base.N % 8 || sp > nk || kern::splitk_workspace_bytes(base.M, base.N, sp) > ws_bytes_)) break;
          // split-K candidates reduce in-kernel unless the two-kernel form is allowed
          for (int fused = sp > 1 && !opt_.splitk_two_kernel ? 1 : 0; fused < (sp > 1 ? 2 : 1); ++fused)
          // Tile order: the heuristic (ConvArgs::order 0; tuning N- vs M-fastest per shape picked
          // M-fastest for ~30 % of shapes behind a cold L2 but made the in-graph forwards 1-2 %
          // slower, profiles/r3_gemm_feed.md section 6), plus -- where the heuristic replicates the
          // weights on every XCD, there are >= 4 N-tiles and the activations are at most 3x the
          // weights (a panel order reads every activation row once per panel: ViT's MLP2, 8x,
          // won in isolation and lost 16 % in the graph) -- the 2- and 4-panel orders, whose
          // XCDs each read one panel of the weights (profiles/r5_xcd_panels.md)
          for (int order : {0, 3, 4})
          // Tail split-K (ConvArgs::tail = 256, one tile per CU per round): next to each fused
          // split-K candidate of an LDS-DMA config, heuristic order, when the tile grid spills a
          // few tiles (at most 160) past a whole number of 256-tile rounds -- the steps of the
          // per-batch-size forward time (profiles/r5_batch_curve.md)
          for (int tail : {0, 256}) {
            if (tail > 0) {
              int bm, bn;
              kern::tile_dims(tile, bm, bn);
              const int T = ((base.M + bm - 1) / bm) * ((base.N + bn - 1) / bn);
              const int v = tile / kern::NUM_TILES;
              if (!opt_.tune_tail || !fused || order != 0 || v == 0 || v >= 6 || T <= tail || T % tail == 0 ||
                  T % tail > 160)
                continue;
            }
            if (order > 0 && !opt_.tune_orders) continue;
            if (order > 0) {
              int bm, bn;
              kern::tile_dims(tile, bm, bn);
              const long long wts = static_cast<long long>(base.N) * base.K;
              const long long acts = static_cast<long long>(base.B) * base.H * base.W * base.Cin;
              if (tile / kern::NUM_TILES >= 6 || wts > acts || acts > 3 * wts ||
                  (base.N + bn - 1) / bn < 4 * (order == 4 ? 2 : 1))
                continue;
            }
            kern::ConvArgs a = base;
            a.splits = sp;
            a.order = order;
            a.tail = tail;
            if (!fused) a.counters = nullptr;
            if (kern::conv_igemm(a, tile, s_compute_) != hipSuccess) continue;  // warm-up / validity
            const float ms = time_candidate(a, tile, B, producer);
            measured.push_back({ms, Tune{tile, sp, fused != 0, order, tail}});
            if (ms < best) {
              best = ms;
              bt = Tune{tile, sp, fused != 0, order, tail};
            }
            if (fused && ms < best_fused) {
              best_fused = ms;
              bt_fused = Tune{tile, sp, true, order, tail};
            }
          }
        }
      }
      // Stream-K candidates (EngineOptions::tune_streamk): the LDS-DMA loops with P = 256 / 512 /
      // 1024 blocks splitting the tiles x K-steps evenly (ConvArgs::sk) -- for grids whose tile
      // count lands just past a multiple of the CU count (ResNet50 stage-3 reduce at B = 24: 296
      // tiles = two tiles on 40 CUs, one on the rest)
      if (opt_.tune_streamk && base.N % 8 == 0 && !base.row_parts && !base.stats_out)
        for (int tile = 0; tile < kern::NUM_CFGS; ++tile) {
          const int v = tile / kern::NUM_TILES;
          if (v != 1 && v != 5) continue;  // 2-stage ring and 1-stage loop
          int bm, bn;
          kern::tile_dims(tile, bm, bn);
          const long long T = static_cast<long long>((base.M + bm - 1) / bm) * ((base.N + bn - 1) / bn);
          for (int P : {256, 512, 1024}) {
            if (T * nk < P || T > kCounters || kern::streamk_workspace_bytes(P, bm, bn) > ws_bytes_) continue;
            kern::ConvArgs a = base;
            a.splits = 1;
            a.sk = P;
            if (kern::conv_igemm(a, tile, s_compute_) != hipSuccess) continue;
            const float ms = time_candidate(a, tile, B, producer);
            Tune tk{tile, 1, true, 0, 0, P};
            measured.push_back({ms, tk});
            if (ms < best) {
              best = ms;
              bt = tk;
            }
          }
        }
      if (bt.splits > 1 && !bt.fused && best_fused <= best * (1.f + opt_.splitk_fused_margin)) {
        bt = bt_fused;  // EngineOptions::splitk_fused_margin: one graph node instead of two
        best = best_fused;
      }
      tune_[bi][oi] = bt;
      tuned_shapes[key] = {bt, best / 3 * 1000.0};
      if (opt_.tune_in_graph) {  // the isolated-launch front runners, for the in-graph pass
        std::sort(measured.begin(), measured.end(), [](const auto& a, const auto& b) { return a.first < b.first; });
        auto& c = cands_[key];
        for (const auto& m : measured)
          if (c.size() < kInGraphCands && m.first <= best * kInGraphSlack) c.push_back(m.second);
      }
      if (B == max_batch_) total_best_us += best / 3 * 1000.0;
    }
  }
  tuned_conv_us_ = total_best_us;
  tune_cache_hits_ = static_cast<long long>(loaded);
  if (opt_.tune_in_graph) tune_in_graph(tuned_shapes);
  if (tuned_shapes.size() > loaded) save_tune_cache(cache_path, arch_, tuned_shapes);
}

// the in-graph pass's results for bucket B are in the tune cache already
bool HipEngine::in_graph_cached(const TuneMap& shapes, int B) const {
  const std::string pre = "g" + std::to_string(plan_.ops.size()) + ":b" + std::to_string(B) + ":";
  for (const auto& kv : shapes)
    if (kv.first.compare(0, pre.size(), pre) == 0) return true;
  return false;
}

// In-graph retune (EngineOptions::tune_in_graph): the isolated launches above time each conv
// behind an L2 scrub; inside a forward the conv reads its input just written by the previous op
// and its weights from wherever the last forward left them.  For every conv with more than one
// front runner (within kInGraphSlack of the isolated best, at most kInGraphCands), each candidate
// is timed IN PLACE -- eager forwards with events around every op, the conv's own interval, median
// of kInGraphReps -- and the fastest kept.  Ops are visited in order, so later ops are timed
// behind the earlier ops' final choices.  Results go to the tune cache under the op's position.
void HipEngine::tune_in_graph(TuneMap& tuned_shapes) {
  const size_t n = plan_.ops.size();
  std::vector<Event> ev(n + 1);
  for (auto& e : ev) HIP_CHECK(e.create());
  long long changed = 0, timed = 0;
  for (size_t bi = 0; bi < buckets_.size(); ++bi) {
    const int B = buckets_[bi];
    slots_[0].h_lens[live_index()] = B;  // the whole bucket is live
    encode_forward(B, 0, s_compute_);   // warm
    for (size_t oi = 0; oi < n; ++oi) {
      const PlanOp& op = plan_.ops[oi];
      if (op.kind != PlanOp::CONV) continue;
      kern::ConvArgs base = conv_args(op, B, 0);
      // keyed by position AND by the op's shape + tuning regime: another model with
      // the same op count and names, or another tuning regime, never loads this choice
      const std::string gkey = "g" + std::to_string(n) + ":b" + std::to_string(B) + ":o" + std::to_string(oi) + ":" +
                               op.name.substr(0, 64) + ":" + std::to_string(sp_) + ":" + shape_key(base, false);
      auto memo = tuned_shapes.find(gkey);
      if (memo != tuned_shapes.end()) {
        tune_[bi][oi] = memo->second.first;
        continue;
      }
      const auto c = cands_.find(shape_key(base, false));  // the isolated-launch front runners
      if (c == cands_.end() || c->second.size() < 2) continue;
      float best = 1e30f;
      Tune bt = tune_[bi][oi];
      for (const Tune& t : c->second) {
        tune_[bi][oi] = t;
        std::vector<float> v;
        for (int r = 0; r < kInGraphReps; ++r) {
          encode_forward(B, 0, s_compute_, ev.data());
          HIP_CHECK(hipStreamSynchronize(s_compute_));
          float ms = 0;
          HIP_CHECK(hipEventElapsedTime(&ms, ev[oi], ev[oi + 1]));
          v.push_back(ms);
        }
        std::nth_element(v.begin(), v.begin() + v.size() / 2, v.end());
        ++timed;
        if (v[v.size() / 2] < best) {
          best = v[v.size() / 2];
          bt = t;
        }
      }
      const Tune& first = c->second.front();
      if (bt.tile != first.tile || bt.splits != first.splits || bt.fused != first.fused) ++changed;
      tune_[bi][oi] = bt;
      tuned_shapes[gkey] = {bt, best * 1000.0};
    }
  }
  in_graph_timed_ = timed;
  in_graph_changed_ = changed;
}

// Device time of the captured forward at every batch size 1..max_batch (EngineOptions::
// efficient_batch): slot 0's MAIN graph of the batch's bucket with the live count set to B, one
// warm-up and three timed back-to-back replays (the serving loop runs graphs back to back), or
// (EngineOptions::batch_curve_median) the median of three such groups.
void HipEngine::measure_batch_curve() {
  Event e0, e1;
  HIP_CHECK(e0.create());
  HIP_CHECK(e1.create());
  auto time_three_replays = [&](hipGraphExec_t g) {
    float ms = 0.f;
    HIP_CHECK(hipEventRecord(e0, s_compute_));
    for (int r = 0; r < 3; ++r) HIP_CHECK(hipGraphLaunch(g, s_compute_));
    HIP_CHECK(hipEventRecord(e1, s_compute_));
    HIP_CHECK(hipEventSynchronize(e1));
    HIP_CHECK(hipEventElapsedTime(&ms, e0, e1));
    return ms;
  };
  Slot& sl = slots_[0];
  long long* lv = sl.h_lens + live_index();
  batch_ms_.assign(static_cast<size_t>(max_batch_) + 1, 0.0);
  for (int b = 1; b <= max_batch_; ++b) {
    hipGraphExec_t g = graphs_[bucket_index(b) * static_cast<size_t>(depth_)];
    *lv = use_live_ ? b : max_batch_;
    HIP_CHECK(hipMemcpyAsync(sl.d_lens + live_index(), lv, sizeof(long long), hipMemcpyHostToDevice, s_compute_));
    HIP_CHECK(hipGraphLaunch(g, s_compute_));
    if (opt_.batch_curve_median) {  // median of three groups of three replays
      float grp[3];
      for (float& ms : grp) ms = time_three_replays(g);
      std::sort(grp, grp + 3);
      batch_ms_[static_cast<size_t>(b)] = grp[1] / 3.0;
    } else {  // the mean of three replays right behind the warm-up (round 5)
      batch_ms_[static_cast<size_t>(b)] = time_three_replays(g) / 3.0;
    }
  }
  *lv = max_batch_;
  HIP_CHECK(hipMemcpyAsync(sl.d_lens + live_index(), lv, sizeof(long long), hipMemcpyHostToDevice, s_compute_));
  HIP_CHECK(hipStreamSynchronize(s_compute_));
}

}  // namespace hip
}  // namespace die
