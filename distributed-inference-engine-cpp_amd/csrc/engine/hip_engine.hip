// HIP execution engine for MI355X (gfx950): construction, teardown and the factories.
//
// Replaces the reference's ONNX Runtime session (src/inference_engine.cpp:16-87 construction,
// :134-209 batchPredict).  One engine owns one GPU:
//  * the ONNX graph is lowered once (hip_plan.cpp) to ~60 fused device ops; all packed weights
//    live in one device blob and all activations in one planned arena, both resident in HBM;
//  * request inputs are parsed by the HTTP layer straight into pinned host buffers handed out by
//    this engine (SamplePool backed by hipHostMalloc), so H2D is a DMA from the parse target;
//  * a batch runs on three streams: H2D copies, the forward (a hipGraph captured per batch
//    bucket and pipeline slot), D2H of the logits; `pipeline_depth` slots let batch k+1's copies
//    overlap batch k's forward;
//  * a completion thread waits for each slot's D2H event in FIFO order and runs the callback.
//
// Executors: n_exec_ compute streams, each with its own activation arena, split-K workspace and
// tile counters, so n_exec_ batches run on the GPU at once (slot s -> executor s % n_exec_).  At
// serving batch sizes (~16) every conv is latency-bound and leaves most CUs idle; a second
// batch in flight fills them.  Data-parallel ranks keep one (RCCL collectives in one order).
//
// Streams = hardware queues: the executor streams (graphs + the small result D2H) and copy
// streams (early uploads, submit-time copies, PREP).  HIP gives a process GPU_MAX_HW_QUEUES
// queues; more streams than that share queues (serialising copies behind kernels).  The engine
// stays within four (1 executor + 2 copy streams [+ prep/side], or 2 + 1), and the serving
// processes raise the limit to 8 (configure_hip_runtime_env) so that an RCCL communicator's
// internal streams do not push the engine's onto shared queues (profiles/r3_rccl_hw_queues.md).
// Two executors time-slice the compute queues instead of overlapping (forwards 1.8x longer).
//
// Batch buckets ~sqrt(2) apart up to 16 (1, 2, 4, 6, 8, 12, 16), eighth steps above
// (18, 20, ..., 32, 36, ...): a batch runs the graph of the smallest bucket >= B, and the
// serving loop's batches (17-24 at the headline load) get kernels tuned within 2 of their size
// (fp32 headline A/B: sqrt(2) steps 13.1-13.2k, quarter steps 13.6-13.7k, eighth steps
// 13.9-14.1k req/s; profiles/r2_state.md).  EngineOptions::bucket_div = steps per octave above
// 16; coarse_buckets: sqrt(2) steps throughout.
#include "hip_engine.h"

namespace die {
namespace hip {

HipEngine::HipEngine(const std::string& path, onnx::Model model, const EngineOptions& opt) : path_(path), opt_(opt) {
  shard_id_ = opt.shard_id;
  dev_ = opt.device_id;
  HIP_CHECK(hipSetDevice(dev_));
  hipDeviceProp_t prop;
  HIP_CHECK(hipGetDeviceProperties(&prop, dev_));
  arch_ = prop.gcnArchName;
  if (arch_.find("gfx950") == std::string::npos)
    throw std::runtime_error("HIP engine is built for gfx950 (MI355X); device reports " + arch_);
  max_batch_ = std::max(1, opt.max_batch);
  depth_ = std::max(1, std::min(opt.pipeline_depth, 4));
  // fp32 (the reference's ORT numerics): split hi/lo bf16 operands on the matrix cores
  PlanOptions po;
  po.side_branches = opt.branch_streams && opt.exec_streams <= 1;
  po.split = opt.precision == "fp32";
  po.fuse_pairs = opt.fuse_pairs;
  po.fuse_stem_pool = opt.fuse_stem_pool;
  po.fuse_gap_fc = opt.fuse_gap_fc;
  po.fold_layernorm = opt.fold_layernorm;
  po.ln_stats_epilogue = opt.ln_stats_epilogue;
  plan_ = build_plan(model, max_batch_, po);
  sp_ = plan_.split ? 1 : 0;
  while (n_prep_ops_ < plan_.ops.size() && plan_.ops[n_prep_ops_].kind == PlanOp::INPUT_PREP) {
    prep_out_ids_.push_back(plan_.ops[n_prep_ops_].out);
    ++n_prep_ops_;
  }
  in_numel_ = plan_.input_numel;
  out_numel_ = plan_.output_numel;

  comm_ = opt.dp_comm;
  dp_world_ = comm_ ? comm_->world() : 1;
  HIP_CHECK(params_.alloc(std::max<size_t>(plan_.params.size(), 256)));
  // executors (see the head of this file)
  n_exec_ = comm_ ? 1 : std::max(1, std::min({opt.exec_streams, depth_, kMaxExec}));
  arena_bytes_ = std::max<size_t>(plan_.arena_bytes, 256);
  for (int e = 0; e < n_exec_; ++e) {
    HIP_CHECK(arenas_[e].alloc(arena_bytes_));
    HIP_CHECK(s_exec_[e].create());
  }
  s_compute_ = s_exec_[0];
  // copy streams: the engine stays within four hardware queues (see the head of this file)
  n_copy_streams_ = n_exec_ > 1 ? 1 : kStageStreams;
  if (opt.copy_streams > 0) n_copy_streams_ = std::min(kStageStreams, opt.copy_streams);
  for (int i = 0; i < n_copy_streams_; ++i) HIP_CHECK(s_stage_[i].create());
  // side-branch stream (plan ops with join >= 0): the fourth and last queue; only with one executor
  branches_ = opt.branch_streams && n_exec_ == 1;
  // the fourth queue: side branches, or a dedicated PREP stream when texts are uploaded early
  if (!branches_ && n_exec_ == 1 && opt.device_decode && opt.stage_slots != 0 && !comm_) HIP_CHECK(s_prep_.create());
  // Result stream: each batch's logits / status D2H (and, data parallel, its collectives) wait on
  // an event after MAIN instead of queueing on the compute stream, so the next batch's MAIN starts
  // right behind this one's (the copies are blit kernels that otherwise sit between two graphs).
  if (opt.result_stream) HIP_CHECK(s_out_.create());
  prep_on_compute_ = opt.prep_on_compute;
  use_live_ = opt.live_batch;
  lead_scale_ = std::max(0.0, opt.pace_lead_scale);
  completion_poll_us_ = std::max(0, opt.completion_poll_us);
  if (branches_) {
    HIP_CHECK(s_side_.create());
    HIP_CHECK(ev_fork_.create(hipEventDisableTiming));
    HIP_CHECK(ev_join_.create(hipEventDisableTiming));
  }
  if (!comm_ || comm_->rank() == 0)
    HIP_CHECK(hipMemcpy(params_, plan_.params.data(), plan_.params.size(), hipMemcpyHostToDevice));
  if (comm_) {  // data parallel: every rank gets the packed weights from rank 0 over xGMI
    const auto tb = std::chrono::steady_clock::now();
    comm_->broadcast(params_, plan_.params.size(), 0, s_compute_);
    HIP_CHECK(hipStreamSynchronize(s_compute_));
    weight_bcast_ms_ = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - tb).count();
    DIE_LOG(INFO, "dp rank " << comm_->rank() << ": weight broadcast " << plan_.params.size() / 1048576.0
                                   << " MiB in " << weight_bcast_ms_ << " ms (" << comm_->backend() << ")");
  }
  if (opt.device_decode) text_cap_ = (in_numel_ * 24 + 4095) / 4096 * 4096;  // up to 23 chars + separator per value
  if (text_cap_) {
    // One device text arena: n_stage_ early-upload slots (stage_text) followed by max_batch
    // fallback slots per pipeline slot (texts copied at submit).  Decode finds sample i at
    // offs[i].  Data-parallel ranks get their shards through the DP arena instead.
    n_stage_ = opt.stage_slots >= 0 ? opt.stage_slots : std::min(1024, std::max(256, 8 * max_batch_));
    if (comm_) n_stage_ = 0;
    HIP_CHECK(d_text_.alloc(text_cap_ * (static_cast<size_t>(n_stage_) + static_cast<size_t>(depth_) * max_batch_)));
    // 4-bit packed texts (BatchItem::packed; early-uploaded or copied at submit) land here, slot
    // for slot like d_text_; the decode kernels expand them in registers (no character copy in HBM).
    // Data-parallel ranks take packed texts too: the ingesting rank packs into the DP arena.
    if (opt.pack_text)
      HIP_CHECK(d_packed_.alloc(text_cap_ / 2 * (static_cast<size_t>(n_stage_) + static_cast<size_t>(depth_) * max_batch_)));
    stage_ev_.resize(n_stage_);
    stage_seq_.assign(n_stage_, 0);
    stage_packed_.assign(n_stage_, 0);
    stage_stream_.assign(n_stage_, 0);
    stage_state_.assign(n_stage_, kIssued);
    for (int t = 0; t < n_stage_; ++t) {
      HIP_CHECK(stage_ev_[t].create(hipEventDisableTiming));
      stage_free_.push_back(n_stage_ - 1 - t);
    }
  }
  slots_.resize(depth_);
  for (auto& sl : slots_) {
    if (text_cap_) HIP_CHECK(sl.d_scratch.alloc(kern::decode_scratch_bytes(max_batch_, text_cap_)));
    // [lens x max_batch][text offsets x max_batch][packed-text offsets x max_batch (-1 = raw)]
    HIP_CHECK(sl.d_lens.alloc(sizeof(long long) * table_len()));
    HIP_CHECK(hipMemset(sl.d_lens, 0xFF, sizeof(long long) * max_batch_));  // all -1: no text samples
    HIP_CHECK(hipMemset(sl.d_lens + max_batch_, 0, sizeof(long long) * max_batch_));
    HIP_CHECK(hipMemset(sl.d_lens + 2 * max_batch_, 0xFF, sizeof(long long) * max_batch_));
    HIP_CHECK(sl.d_status.alloc(sizeof(int) * status_len()));
    HIP_CHECK(hipMemset(sl.d_status, 0, sizeof(int) * status_len()));
    if (comm_) {
      HIP_CHECK(sl.d_gather.alloc(sizeof(float) * out_numel_ * max_batch_ * dp_world_));
      HIP_CHECK(sl.d_gstatus.alloc(sizeof(int) * status_len() * dp_world_));
      HIP_CHECK(sl.h_gather.alloc(sizeof(float) * out_numel_ * max_batch_ * dp_world_));
      HIP_CHECK(sl.h_gstatus.alloc(sizeof(int) * status_len() * dp_world_));
      HIP_CHECK(sl.ev_gather.create(hipEventDisableTiming));
    }
    // host-coherent: the graph's first kernel reads it directly (see encode_forward)
    HIP_CHECK(sl.h_lens.alloc(sizeof(long long) * table_len(), hipHostMallocCoherent | hipHostMallocMapped));
    HIP_CHECK(hipHostGetDevicePointer(reinterpret_cast<void**>(&sl.h_lens_dev), sl.h_lens, 0));
    for (int i = 0; i < max_batch_; ++i) {  // no text samples until a submit says otherwise
      sl.h_lens[i] = -1;
      sl.h_lens[max_batch_ + i] = 0;
      sl.h_lens[2 * max_batch_ + i] = -1;
    }
    sl.h_lens[live_index()] = max_batch_;  // live batch: every sample of the bucket until a submit
    HIP_CHECK(hipMemcpy(sl.d_lens + live_index(), sl.h_lens + live_index(), sizeof(long long), hipMemcpyHostToDevice));
    HIP_CHECK(sl.h_status.alloc(sizeof(int) * 2 * max_batch_));
    HIP_CHECK(sl.d_in.alloc(sizeof(float) * in_numel_ * max_batch_));
    HIP_CHECK(sl.d_out.alloc(sizeof(float) * out_numel_ * max_batch_));
    HIP_CHECK(hipMemset(sl.d_in, 0, sizeof(float) * in_numel_ * max_batch_));
    fill_token_input(sl.d_in);
    HIP_CHECK(sl.h_out.alloc(sizeof(float) * out_numel_ * max_batch_));
    for (auto& ev : sl.ev_h2d) HIP_CHECK(ev.create(hipEventDisableTiming));
    HIP_CHECK(sl.ev_d2h.create(hipEventDisableTiming | hipEventBlockingSync));
    HIP_CHECK(sl.ev_main.create(hipEventDisableTiming));
    HIP_CHECK(sl.ev_prep.create(hipEventDisableTiming));
    for (int id : prep_out_ids_) {
      DeviceMem<void> pbuf;
      HIP_CHECK(pbuf.alloc(std::max<size_t>(plan_.bufs[id].bytes_per_sample * max_batch_, 256)));
      sl.d_prep.push_back(std::move(pbuf));
    }
  }
  // batch buckets (see the head of this file)
  const bool coarse = opt.coarse_buckets;
  const int fine = std::max(1, opt.bucket_div);
  for (int b = 1; b < max_batch_; b *= 2) {
    buckets_.push_back(b);
    if (b >= 16 && !coarse) {
      for (int q = 1; q < fine; ++q)
        if (b + q * b / fine < max_batch_) buckets_.push_back(b + q * b / fine);
    } else if (b >= 4 && b + b / 2 < max_batch_) {
      buckets_.push_back(b + b / 2);
    }
  }
  buckets_.push_back(max_batch_);
  est_ms_.assign(buckets_.size(), 0.0);

  // (the pool owns what this allocator hands it, and frees it through the second callback)
  pool_ = std::make_unique<SamplePool>(
      std::max(in_numel_, text_cap_ / sizeof(float)),
      [](size_t bytes) -> void* {
        void* p = nullptr;
        if (hipHostMalloc(&p, bytes, hipHostMallocDefault) != hipSuccess) return nullptr;
        return p;
      },
      [](void* p) { (void)hipHostFree(p); }, 32);

  ws_bytes_ = kern::kSplitKWorkspaceBytes;  // split-K / GAP_FC partials (choose_splits / autotune stay within it)
  // zero page for the LDS-DMA conv loads: padding pixels and M-tail rows (a whole K row)
  size_t zeros_bytes = 4096;
  for (const PlanOp& op : plan_.ops)
    if (op.kind == PlanOp::CONV) zeros_bytes = std::max<size_t>(zeros_bytes, (static_cast<size_t>(op.conv.Kpad) + 64) * 2);
  HIP_CHECK(zeros_.alloc(zeros_bytes));
  HIP_CHECK(hipMemset(zeros_, 0, zeros_bytes));
  for (int e = 0; e < n_exec_; ++e) {
    HIP_CHECK(wss_[e].alloc(ws_bytes_));
    HIP_CHECK(counterss_[e].alloc(sizeof(int) * kCounters));  // fused split-K tile counters
    HIP_CHECK(hipMemset(counterss_[e], 0, sizeof(int) * kCounters));
  }
  if (branches_) {  // a branch running beside the main chain needs its own split-K scratch
    HIP_CHECK(ws_side_.alloc(ws_bytes_));
    HIP_CHECK(counters_side_.alloc(sizeof(int) * kCounters));
    HIP_CHECK(hipMemset(counters_side_, 0, sizeof(int) * kCounters));
  }
  ws_ = wss_[0];
  // Validate every op eagerly at the largest bucket, tune, then capture one graph per
  // (bucket, slot).
  for (int s = 0; s < depth_; ++s) encode_forward(max_batch_, s, s_compute_);
  HIP_CHECK(hipStreamSynchronize(s_compute_));
  if (opt.autotune) autotune();
  if (opt.use_graphs) {
    graphs_.resize(buckets_.size() * depth_);
    prep_graphs_.resize(buckets_.size() * depth_);
    auto capture = [&](int B, int s, Part part) {
      hipGraph_t g;
      HIP_CHECK(hipStreamBeginCapture(s_compute_, hipStreamCaptureModeThreadLocal));
      encode_forward(B, s, s_compute_, nullptr, part);
      HIP_CHECK(hipStreamEndCapture(s_compute_, &g));
      GraphExec ge;
      HIP_CHECK(ge.instantiate(g));
      HIP_CHECK(hipGraphDestroy(g));
      return ge;
    };
    for (size_t bi = 0; bi < buckets_.size(); ++bi)
      for (int s = 0; s < depth_; ++s) {
        prep_graphs_[bi * depth_ + s] = capture(buckets_[bi], s, PREP);
        graphs_[bi * depth_ + s] = capture(buckets_[bi], s, MAIN);
      }
    HIP_CHECK(hipGraphLaunch(prep_graphs_.back(), s_compute_));
    // warm the graph path once
    HIP_CHECK(hipGraphLaunch(graphs_.back(), s_compute_));
    HIP_CHECK(hipStreamSynchronize(s_compute_));
    // (data parallel too: the leader's merge takes the local curve's sizes -- the MAIN graphs hold
    // no collectives, so each rank times its own forward)
    if (opt.efficient_batch && n_exec_ == 1) measure_batch_curve();
  }
  for (auto& e : tev_) HIP_CHECK(e.create());
  completion_ = std::thread([this] {
    pthread_setname_np(pthread_self(), "die-complete");
    completion_loop();
  });
  if (n_stage_)
    stager_ = std::thread([this] {
      pthread_setname_np(pthread_self(), "die-stager");
      stager_loop();
    });
}

// The handles release streams, events, graphs and memory after this body (hip_engine.h).
HipEngine::~HipEngine() {
  {
    std::lock_guard<std::mutex> g(mu_);
    stop_ = true;
  }
  cv_.notify_all();
  if (completion_.joinable()) completion_.join();
  {
    std::lock_guard<std::mutex> g(stage_mu_);
    stage_stop_ = true;  // the stager drains its queue first (queued tickets still get issued)
  }
  stage_cv_.notify_all();
  if (stager_.joinable()) stager_.join();
  (void)hipSetDevice(dev_);
  (void)hipDeviceSynchronize();
  for (void* p : registered_) (void)hipHostUnregister(p);
  pool_.reset();
}

size_t HipEngine::register_host_memory(void* p, size_t bytes) {
  HIP_CHECK(hipSetDevice(dev_));
  HIP_CHECK(hipHostRegister(p, bytes, hipHostRegisterDefault));
  registered_.push_back(p);
  return bytes;
}

// Token-id plans: an all-zero start-up input is all padding under the usual pad id 0, and the
// eager validation pass, autotune and the batch curve would time attention with no visible key.
// Fill the slot with an in-range id the pad test keeps visible, so they see full-length
// sequences; serving inputs overwrite it as before.
void HipEngine::fill_token_input(float* d_in) {
  for (const PlanOp& op : plan_.ops) {
    if (op.kind != PlanOp::EMBED_TOKENS) continue;
    float id = 0.f;
    if (op.out2 >= 0) {
      bool found = false;
      for (int c = 0; c < op.gidx && !found; ++c) {  // ids near the compare constant first, then 0, 1, ...
        for (float t : {op.pad.value + 1.f + c, op.pad.value - 1.f - c, static_cast<float>(c)}) {
          if (t < 0.f || t > static_cast<float>(op.gidx - 1) || t != std::floor(t)) continue;
          if (kern::token_visible_host(t, op.pad.op, op.pad.value, op.pad.negated, op.pad.truncated)) {
            id = t;
            found = true;
            break;
          }
        }
      }
    }
    std::vector<float> h(in_numel_ * max_batch_, id);
    if (op.in_ld > 0) {  // several graph inputs: a visible in-range id, mask 1, types 0 in their segments
      const bool masked = pad_reads_mask(op);
      if (masked) id = static_cast<float>(std::min(1, op.gidx - 1));  // the test reads the mask, not the ids
      for (size_t b = 0; b < static_cast<size_t>(max_batch_); ++b) {
        float* row = h.data() + b * in_numel_;
        std::fill_n(row, in_numel_, 0.f);
        std::fill_n(row + op.seg_ids, op.S, id);
        if (masked) std::fill_n(row + op.pad.src, op.S, 1.f);
      }
    }
    HIP_CHECK(hipMemcpy(d_in, h.data(), h.size() * sizeof(float), hipMemcpyHostToDevice));
    return;
  }
}

}  // namespace hip

std::unique_ptr<Engine> create_hip_engine(const std::string& model_path, const EngineOptions& opt, std::string* why) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || n == 0) {
    if (why) *why = "no HIP device visible";
    return nullptr;
  }
  if (opt.device_id >= n) {
    if (why) *why = "device " + std::to_string(opt.device_id) + " not present (" + std::to_string(n) + " visible)";
    return nullptr;
  }
  return std::make_unique<hip::HipEngine>(model_path, opt);
}

std::unique_ptr<Engine> create_hip_engine_model(const std::string& label, onnx::Model model, const EngineOptions& opt,
                                                std::string* why) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || n == 0 || opt.device_id >= n) {
    if (why) *why = "no HIP device visible";
    return nullptr;
  }
  return std::make_unique<hip::HipEngine>(label, std::move(model), opt);
}

}  // namespace die
