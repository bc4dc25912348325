// HIP execution engine for MI355X (gfx950): the class, shared by the files that implement it.
//
//   hip_engine.hip    construction and teardown, batch buckets, the factories
//   hip_launch.hip    encode_forward / launch_op (one case per op kind), profile_ops
//   hip_pipeline.hip  submit, the stager and completion threads, pacing, data-parallel collectives
//   hip_autotune.hip  conv autotune, the in-graph retune, the batch curve
//   hip_stats.hip     stats()
//
// Internal to csrc/engine: everything else sees engine.h's Engine and the create_hip_engine factories.
#pragma once

#include <pthread.h>
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <chrono>
#include <condition_variable>
#include <unistd.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <iostream>
#include <map>
#include <mutex>
#include <stdexcept>
#include <thread>

#include "../kernels/kernels.h"
#include "engine.h"
#include "hip_handles.h"
#include "hip_plan.h"
#include "tune_cache.h"
#include "../core/log.h"
#include "../core/trace.h"
#include "../parallel/comm.h"

#define HIP_CHECK(expr)                                                                                     \
  do {                                                                                                      \
    hipError_t e_ = (expr);                                                                                 \
    if (e_ != hipSuccess) throw std::runtime_error(std::string(#expr) + " failed: " + hipGetErrorString(e_)); \
  } while (0)

namespace die {
namespace hip {

class HipEngine : public Engine {
 public:
  HipEngine(const std::string& path, const EngineOptions& opt) : HipEngine(path, onnx::load_onnx(path), opt) {}
  // `model` given in memory (a segment of a hybrid HIP + CPU partition); `path` labels it
  HipEngine(const std::string& path, onnx::Model model, const EngineOptions& opt);
  ~HipEngine() override;

  std::string name() const override { return "hip:" + arch_ + ":" + std::to_string(dev_); }
  const std::string& getModelPath() const override { return path_; }
  std::vector<int64_t> getInputShape() const override { return plan_.input_shape; }
  std::vector<int64_t> getOutputShape() const override { return plan_.output_shape; }
  int max_batch() const override { return max_batch_; }
  SamplePool& sample_pool() override { return *pool_; }
  size_t text_capacity() const override { return text_cap_; }
  bool text_packing() const override { return d_packed_ != nullptr; }
  bool device_gather() const override { return comm_ != nullptr; }
  size_t register_host_memory(void* p, size_t bytes) override;

  long stage_text(const char* text, size_t len, bool packed) override;
  void release_staged(long t, bool ran) override;
  void wait_for_slot() override;
  void submit(std::vector<BatchItem> items, BatchDone done) override;
  std::chrono::steady_clock::time_point dispatch_not_before() override;
  int preferred_batch(int queued) const override;
  void synchronize() override;
  Json stats() const override;
  // Per-op device time (eager launches bracketed by events), averaged over `iters` forwards.
  Json profile_ops(int B, int iters) override;

 private:
  static constexpr int kStageStreams = 2;
  struct Slot {
    DeviceMem<float> d_gather;  // data parallel: [world][max_batch][out_numel]
    DeviceMem<int> d_gstatus;
    PinnedMem<float> h_gather;
    PinnedMem<int> h_gstatus;
    DeviceMem<float> d_in;
    DeviceMem<float> d_out;
    PinnedMem<float> h_out;
    DeviceMem<void> d_scratch;
    DeviceMem<long long> d_lens;      // [lens][text offsets into d_text_][packed offsets into d_packed_] x max_batch
    PinnedMem<long long> h_lens;      // pinned host-coherent, same layout
    long long* h_lens_dev = nullptr;  // its device-side address
    DeviceMem<int> d_status;          // [status x max_batch][ntok x max_batch]
    PinnedMem<int> h_status;          // pinned
    std::vector<DeviceMem<void>> d_prep;  // per-slot outputs of the PREP part's input-prep ops
    Event ev_gather;
    Event ev_h2d[kStageStreams];
    Event ev_d2h;
    Event ev_main;  // MAIN done on the compute stream: the result copies (s_out_) wait on it
    Event ev_prep;
  };
  struct Job {
    int slot = 0;
    int B = 0;
    BatchDone done;
    std::chrono::steady_clock::time_point t0;
    std::string error;
    bool has_text = false;
    bool dp_gathered = false;  // failed, but the collectives ran with this rank's shard flag cleared
    int ev = 0;  // first of its kEvPerJob timing events in tev_
    int bi = 0;  // batch bucket
  };

  struct StageReq {
    int t;
    const char* text;
    size_t len;
    bool packed;  // 4-bit packed: (len + 1) / 2 bytes to d_packed_
  };
  static constexpr int kQueued = 0, kIssued = 1, kFailed = 2;

  // PREP = decode-table fetch + device decode + the leading input-prep ops (per-slot buffers only);
  // MAIN = the rest.  submit() runs PREP on the copy stream so it overlaps the previous batch's
  // MAIN on the compute stream.
  enum Part { ALL = 0, PREP = 1, MAIN = 2 };

  static constexpr int kTableRows = 3;  // per-slot decode table: lens, text offsets, packed offsets
  // ... followed by one element: the live batch (samples of the bucket that are real)
  size_t table_len() const { return static_cast<size_t>(kTableRows) * max_batch_ + 1; }
  // per-slot status table: [status x max_batch][ntok x max_batch][shard ok flag, 3 x pad]; a
  // data-parallel rank all-gathers the whole table, so the flag rides with the rows
  size_t status_len() const { return 2 * static_cast<size_t>(max_batch_) + 4; }
  size_t rank_ok_index() const { return 2 * static_cast<size_t>(max_batch_); }
  size_t live_index() const { return static_cast<size_t>(kTableRows) * max_batch_; }
  size_t bucket_index(int B) const {
    size_t bi = 0;
    while (bi + 1 < buckets_.size() && buckets_[bi] < B) ++bi;
    return bi;
  }

  // hip_engine.hip
  void fill_token_input(float* d_in);

  // hip_launch.hip
  void* buf_ptr(int id, int s);
  const float* prm_ptr(size_t off) const;
  kern::ConvArgs conv_args(const PlanOp& op, int B, int s);
  // Encode one forward pass for `B` samples using slot `s`'s input/output buffers.
  // op_events (profiling): if given, events[0] is recorded before the first op and events[i + 1]
  // after op i.
  // range_begin/range_end (autotune): encode only ops [range_begin, range_end), nothing else.
  void encode_forward(int B, int s, hipStream_t st, const Event* op_events = nullptr, Part part = ALL,
                      size_t range_begin = SIZE_MAX, size_t range_end = 0);
  // The launch of one op on `st`; `side`: on the side-branch stream, with its split-K scratch.
  hipError_t launch_op(const PlanOp& op, size_t op_index, int B, int s, hipStream_t st, bool side,
                       const long long* live);

  // hip_pipeline.hip
  int wait_staged(int t);
  void stager_loop();
  void completion_loop();
  void fill_gathered(BatchResult& r, Slot& sl, const Job& job);
  hipStream_t result_stream(Slot& sl, hipStream_t cs);
  void dp_collectives(Slot& sl, int B, hipStream_t cs);

  // hip_autotune.hip
  Tune tune_for(int B, size_t op_index) const;
  std::string shape_key(const kern::ConvArgs& base, bool warm_input) const;
  void autotune();
  bool in_graph_cached(const TuneMap& shapes, int B) const;
  static constexpr size_t kInGraphCands = 4;
  static constexpr float kInGraphSlack = 1.25f;
  static constexpr int kInGraphReps = 5;
  void tune_in_graph(TuneMap& tuned_shapes);
  void measure_batch_curve();

  std::string path_;
  EngineOptions opt_;
  int dev_ = 0;
  std::string arch_;
  int max_batch_ = 32;
  int depth_ = 2;
  Plan plan_;
  int sp_ = 0;  // fp32 mode (split kernels)
  size_t in_numel_ = 0, out_numel_ = 0;
  size_t text_cap_ = 0;  // bytes of input text per sample for device decode (0 = off)
  int n_stage_ = 0;                  // early-upload slots (stage_text)
  int n_copy_streams_ = kStageStreams;  // copy streams in use (EngineOptions::copy_streams, 1..kStageStreams)
  unsigned long long stage_counter_[kStageStreams] = {};
  std::vector<unsigned long long> stage_seq_;  // guarded by stage_mu_ (like the three below)
  std::vector<int> stage_stream_;
  std::vector<char> stage_packed_;  // the ticket's text is 4-bit packed
  std::vector<int> stage_state_;
  std::vector<int> stage_free_;
  std::deque<StageReq> stage_q_;
  bool stage_stop_ = false;
  std::mutex stage_mu_;
  std::condition_variable stage_cv_, stage_done_cv_;
  std::thread stager_;
  std::atomic<long long> staged_total_{0}, staged_used_{0};
  std::atomic<long long> diag_issue_ns_{0}, diag_submit_wait_ns_{0}, diag_not_ready_{0}, diag_submit_ns_{0};
  long long tune_cache_hits_ = 0;
  static constexpr int kCounters = 1 << 16;
  std::map<std::string, std::vector<Tune>> cands_;  // isolated-launch front runners per shape (tune_in_graph)
  long long in_graph_timed_ = 0, in_graph_changed_ = 0;
  static constexpr int kMaxExec = 2;
  int n_exec_ = 1;
  bool branches_ = false;  // side-branch stream in use (PlanOp::join)
  int completion_poll_us_ = 0;     // EngineOptions::completion_poll_us: > 0 = sleep-poll the D2H event (0 = hipEventSynchronize)
  bool prep_on_compute_ = false;  // PREP runs on the compute stream before MAIN (EngineOptions)
  bool use_live_ = true;          // skip the bucket's padding samples (EngineOptions::live_batch)
  double lead_scale_ = 1.0;       // EngineOptions::pace_lead_scale (< 1: dispatch later, trading GPU idle for batch size)
  size_t arena_bytes_ = 0;
  Communicator* comm_ = nullptr;  // data parallel (not owned)
  int dp_world_ = 1;
  double weight_bcast_ms_ = 0;                 // RCCL weight broadcast at start-up (stats)
  std::atomic<long long> dp_collective_ops_{0};  // grouped per-batch gathers issued
  std::vector<void*> registered_;
  float* ws_ = nullptr;  // executor 0's (autotune)
  size_t ws_bytes_ = 0;
  std::vector<std::vector<Tune>> tune_;  // [bucket][op]
  double tuned_conv_us_ = 0;
  hipStream_t s_compute_{};  // executor 0's
  std::vector<int> buckets_;
  size_t n_prep_ops_ = 0;                    // leading INPUT_PREP ops (PREP part)
  std::vector<int> prep_out_ids_;            // their outputs live in per-slot buffers
  std::unique_ptr<SamplePool> pool_;
  std::thread completion_;
  std::mutex mu_, submit_mu_;
  std::condition_variable cv_, slot_cv_;
  std::deque<Job> jobs_;
  int inflight_ = 0;
  // per job: [0] compute stream reaches the job, [1] MAIN start, [2] MAIN end, [3] PREP start,
  // [4] PREP end, [5] first input copy issued, [6] input copies done
  static constexpr int kTimingJobs = 16, kEvPerJob = 7;
  unsigned long long job_seq_ = 0;  // guarded by submit_mu_
  int prev_ev_ = -1;                // completion thread
  std::atomic<double> copy_wait_ms_total_{0.0}, gpu_gap_ms_total_{0.0}, prep_ms_total_{0.0};
  int callbacks_running_ = 0;           // submitted batches whose callback has not returned yet
  std::vector<float> out_copy_;         // completion thread: results of the batch being called back
  std::vector<int> status_copy_;
  std::vector<int> rank_ok_copy_;       // data parallel: gathered shard flags of the batch being called back
  bool dp_issued_ = false;              // submit(): this batch's collectives are issued (guarded by submit_mu_)
  long long nth_batch_ = 0;             // submit(): batches seen (fault injection; guarded by submit_mu_)
  int next_slot_ = 0;
  int last_ev_ = -1, last_bi_ = 0;  // most recent submitted job (guarded by mu_)
  mutable std::mutex pace_mu_;
  std::vector<double> est_ms_;      // EMA device ms per bucket (pace_mu_)
  std::vector<double> batch_ms_;    // start-up device ms per batch size (efficient_batch; empty = off)
  double lead_ms_ = 0.3, lead_ms_total_ = 0.0, input_ms_ = 0.0, margin_ms_ = 0.08;
  std::chrono::steady_clock::time_point pace_drain_{};  // predicted drain of the batch in flight
  bool pace_armed_ = false;
  std::atomic<long long> paced_batches_{0};
  bool stop_ = false;
  std::atomic<long long> batches_{0}, images_{0};
  std::atomic<long long> h2d_bytes_{0}, d2h_bytes_{0}, graph_replays_{0};
  std::atomic<double> device_ms_total_{0.0};

  // The GPU resources, owned by handles and released by member destruction once ~HipEngine's body
  // has synchronized the device -- in reverse order of declaration, so keep memory first, then
  // streams and events, then the graph execs: graphs go before the streams they ran on, streams and
  // events before the memory their work touched.  (Slot keeps the same order inside.)
  DeviceMem<uint8_t> params_;
  DeviceMem<uint16_t> zeros_;
  DeviceMem<uint8_t> arenas_[kMaxExec];
  DeviceMem<float> wss_[kMaxExec];
  DeviceMem<int> counterss_[kMaxExec];
  DeviceMem<float> ws_side_;
  DeviceMem<int> counters_side_;
  DeviceMem<unsigned char> d_text_;  // (n_stage_ + depth_ * max_batch_) x text_cap_
  DeviceMem<unsigned char> d_packed_;  // depth_ * max_batch_ x text_cap_ / 2 (packed texts, copied at submit)
  std::vector<Slot> slots_;
  Stream s_exec_[kMaxExec];
  Stream s_stage_[kStageStreams];
  Stream s_out_;      // result copies / data-parallel collectives (behind Slot::ev_main)
  Stream s_side_;
  Stream s_prep_;  // PREP stream (early upload), else PREP shares copy stream 0
  Event ev_fork_, ev_join_;
  std::vector<Event> stage_ev_;
  Event tev_[kEvPerJob * kTimingJobs];
  std::vector<GraphExec> graphs_;       // MAIN part per (bucket, slot)
  std::vector<GraphExec> prep_graphs_;  // PREP part per (bucket, slot)
};

}  // namespace hip
}  // namespace die
