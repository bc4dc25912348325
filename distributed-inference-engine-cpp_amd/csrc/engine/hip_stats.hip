// HIP engine: stats(), the engine's part of the worker's info / metrics JSON.
#include "hip_engine.h"

namespace die {
namespace hip {

Json HipEngine::stats() const {
  Json j = Json::object();
  j["device"] = name();
  j["batches"] = static_cast<long long>(batches_.load());
  j["images"] = static_cast<long long>(images_.load());
  const long long nb = batches_.load();
  j["avg_device_ms"] = nb ? device_ms_total_.load() / nb : 0.0;
  // per-GPU I/O and activity counters
  j["device_id"] = dev_;
  j["h2d_bytes"] = h2d_bytes_.load();
  j["d2h_bytes"] = d2h_bytes_.load();
  j["graph_replays"] = graph_replays_.load();
  j["device_busy_ms"] = device_ms_total_.load();
  // per batch: compute stream waiting for the batch's PREP (copies + decode) / idle before it was submitted
  j["avg_copy_wait_ms"] = nb ? copy_wait_ms_total_.load() / nb : 0.0;
  j["avg_gpu_gap_ms"] = nb ? gpu_gap_ms_total_.load() / nb : 0.0;
  j["avg_prep_ms"] = nb ? prep_ms_total_.load() / nb : 0.0;  // decode + input prep, on the copy stream
  j["options"] = engine_options_json(opt_);
  j["pace"] = opt_.pace && n_exec_ == 1 && !comm_ && !graphs_.empty();
  j["pack_text"] = d_packed_ != nullptr;
  j["branch_streams"] = branches_;
  j["prep_on_compute"] = prep_on_compute_;
  j["completion_poll_us"] = completion_poll_us_;
  j["live_batch"] = use_live_;
  j["paced_batches"] = static_cast<long long>(paced_batches_.load());
  {
    std::lock_guard<std::mutex> g(pace_mu_);
    j["avg_pace_lead_ms"] = nb ? lead_ms_total_ / nb : 0.0;
    j["pace_input_ms"] = input_ms_;
    j["pace_margin_ms"] = margin_ms_;
  }
  j["hip_graphs"] = !graphs_.empty();
  j["efficient_batch"] = !batch_ms_.empty();
  if (!batch_ms_.empty()) {
    Json c = Json::array();  // device ms of the captured forward at batch 1, 2, ..., max_batch
    for (size_t b = 1; b < batch_ms_.size(); ++b) c.push_back(batch_ms_[b]);
    j["batch_curve_ms"] = c;
  }
  j["pipeline_depth"] = depth_;
  j["executors"] = n_exec_;
  j["copy_streams"] = n_copy_streams_;
  j["plan"] = plan_.summary();
  {  // what a request's numbers are: activations, or token ids looked up in an embedding table
    const PlanOp* emb = nullptr;
    for (const PlanOp& op : plan_.ops)
      if (op.kind == PlanOp::EMBED_TOKENS && !emb) emb = &op;
    j["input_kind"] = emb ? "token_ids" : "activations";
    if (emb) {
      j["vocab"] = emb->gidx;
      static const char* cmp[] = {"==", ">", "<"};
      if (pad_reads_mask(*emb))  // ... read from the attention-mask input, not the ids
        j["pad_compare"] = std::string(emb->pad.truncated ? "trunc(mask input)" : "mask input") +
                           (emb->pad.negated ? " != 0" : " == 0");
      else if (emb->out2 >= 0)  // a key is visible where this holds
        j["pad_compare"] = std::string(emb->pad.negated ? "not " : "") + (emb->pad.truncated ? "trunc(id) " : "id ") +
                           cmp[emb->pad.op] + " " + std::to_string(emb->pad.value);
      else j["pad_compare"] = "none";
    }
  }
  {  // the attention ops' shape: heads over stored K / V heads (kv_heads < heads: grouped-query attention) and masks
    Json at = Json::array();
    for (const PlanOp& op : plan_.ops)
      if (op.kind == PlanOp::ATTENTION) {
        Json o = Json::object();
        o["heads"] = op.nh;
        o["kv_heads"] = op.kv_heads;
        o["head_dim"] = op.hd;
        o["causal"] = op.causal != 0;
        o["key_mask"] = op.key_mask != 0;
        at.push_back(o);
      }
    j["attention"] = at;
  }
  {  // the GroupNorm / InstanceNorm ops' geometry (groups == channels: InstanceNorm); act 0 none, 1 ReLU, 2 SiLU
    Json gn = Json::array();
    for (const PlanOp& op : plan_.ops)
      if (op.kind == PlanOp::GROUPNORM) {
        Json o = Json::object();
        o["name"] = op.name;
        o["groups"] = op.groups;
        o["channels"] = op.Cp;
        o["stored_channels"] = op.C;
        o["pixels"] = op.H * op.W;
        o["act"] = op.act;
        gn.push_back(o);
      }
    if (gn.size()) j["groupnorm"] = gn;
  }
  {  // the Global Response Normalization ops' geometry (rows = the pixels of the map)
    Json gr = Json::array();
    for (const PlanOp& op : plan_.ops)
      if (op.kind == PlanOp::GRN) {
        Json o = Json::object();
        o["name"] = op.name;
        o["C"] = op.C;
        o["rows"] = op.H * op.W;
        o["eps"] = static_cast<double>(op.eps);
        gr.push_back(o);
      }
    if (gr.size()) j["grn"] = gr;
  }
  j["inputs"] = input_segments_json(plan_.inputs);  // the graph inputs as segments of a request
  j["precision"] = sp_ ? "fp32" : "bf16";
  j["gflop_per_image"] = plan_.flops_per_sample / 1e9;
  j["arena_mib"] = static_cast<double>(plan_.arena_bytes) / (1 << 20);
  j["pinned_samples"] = static_cast<long long>(pool_->allocated());
  j["device_decode"] = text_cap_ > 0;
  j["dp_rank"] = comm_ ? comm_->rank() : 0;
  j["dp_weight_broadcast_ms"] = weight_bcast_ms_;
  j["dp_collective_ops"] = dp_collective_ops_.load();
  j["text_capacity"] = static_cast<long long>(text_cap_);
  j["stage_slots"] = n_stage_;
  j["staged_uploads"] = staged_total_.load();
  j["batches_with_staged"] = staged_used_.load();
  {
    const long long st = std::max<long long>(1, staged_total_.load());
    Json d = Json::object();
    d["stager_issue_us_avg"] = diag_issue_ns_.load() / 1e3 / st;
    d["submit_wait_us_avg"] = diag_submit_wait_ns_.load() / 1e3 / st;
    d["staged_not_ready_at_submit"] = diag_not_ready_.load();
    d["submit_us_avg"] = diag_submit_ns_.load() / 1e3 / std::max<long long>(1, batches_.load());
    j["staging_diag"] = d;
  }
  j["autotuned"] = !tune_.empty();
  j["tuned_conv_us_at_max_batch"] = tuned_conv_us_;
  j["tune_in_graph_timed"] = in_graph_timed_;      // candidates timed in place (EngineOptions::tune_in_graph)
  j["tune_in_graph_changed"] = in_graph_changed_;  // convs whose in-place winner differs from the isolated one
  j["tune_cache_entries_loaded"] = tune_cache_hits_;
  if (!tune_.empty()) {
    Json t = Json::array();
    for (size_t oi = 0; oi < plan_.ops.size(); ++oi)
      if (plan_.ops[oi].kind == PlanOp::CONV) {
        const Tune& x = tune_.back()[oi];
        t.push_back(std::to_string(x.tile) + "/" + std::to_string(x.splits) + (x.fused ? "f" : "") +
                    (x.order == 2 ? "m" : x.order == 1 ? "n" : "") + (x.tail ? "t" : "") +
                    (x.sk ? "k" + std::to_string(x.sk) : ""));
      }
    j["tile_split_at_max_batch"] = t;
  }
  return j;
}

}  // namespace hip
}  // namespace die
