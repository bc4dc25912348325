// HIP engine: the serving pipeline -- early text uploads (the stager thread), submit, just-in-time
// dispatch, the completion thread and the data-parallel collectives.
//
// A batch runs on three streams: H2D copies, the forward (a hipGraph captured per batch bucket and
// pipeline slot), D2H of the logits; `pipeline_depth` slots let batch k+1's copies overlap batch
// k's forward.  The completion thread waits for each slot's D2H event in FIFO order and runs the
// callback.
#include "hip_engine.h"

namespace die {
namespace hip {

// Early upload: reactor threads only queue the request; ONE stager thread issues every staged
// copy (no HIP API traffic from the HTTP threads competing with the batcher's graph launches and
// the completion thread's waits -- measured: issuing from 16 reactors cost ~15% throughput).
long HipEngine::stage_text(const char* text, size_t len, bool packed) {
  if (!text_cap_ || n_stage_ == 0 || len == 0 || len > text_cap_ || (packed && !d_packed_)) return -1;
  int t;
  {
    std::lock_guard<std::mutex> g(stage_mu_);
    if (stage_free_.empty() || stage_stop_) return -1;
    t = stage_free_.back();
    stage_free_.pop_back();
    stage_state_[t] = kQueued;
    stage_packed_[t] = packed;
    stage_q_.push_back(StageReq{t, text, len, packed});
  }
  stage_cv_.notify_one();
  staged_total_.fetch_add(1, std::memory_order_relaxed);
  return t;
}

void HipEngine::release_staged(long t, bool ran) {
  if (t < 0 || t >= n_stage_) return;
  if (!ran) {  // the pinned source may be reused after this: wait for an unconsumed copy
    if (wait_staged(static_cast<int>(t)) == kIssued) {
      (void)hipSetDevice(dev_);
      (void)hipEventSynchronize(stage_ev_[t]);
    }
  }
  std::lock_guard<std::mutex> g(stage_mu_);
  stage_free_.push_back(static_cast<int>(t));
}

void HipEngine::wait_for_slot() {
  std::unique_lock<std::mutex> lk(mu_);
  slot_cv_.wait(lk, [&] { return inflight_ < depth_ || stop_; });
}

void HipEngine::submit(std::vector<BatchItem> items, BatchDone done) {
  const int B = static_cast<int>(items.size());
  if (B == 0) {
    BatchResult r;
    done(r);
    return;
  }
  if (B > max_batch_) {
    BatchResult r;
    r.ok = false;
    r.error = "batch of " + std::to_string(B) + " exceeds max_batch " + std::to_string(max_batch_);
    done(r);
    return;
  }
  std::lock_guard<std::mutex> submit_guard(submit_mu_);
  int slot;
  {
    std::unique_lock<std::mutex> lk(mu_);
    slot_cv_.wait(lk, [&] { return inflight_ < depth_ || stop_; });
    if (stop_) {
      BatchResult r;
      r.ok = false;
      r.error = "engine stopped";
      done(r);
      return;
    }
    ++inflight_;
    slot = next_slot_;
    next_slot_ = (next_slot_ + 1) % depth_;
  }
  TraceRange tr_submit("engine.submit(h2d+graph)");
  {
    // paced dispatch that arrives after the predicted drain of the batch in flight: the GPU idled
    std::lock_guard<std::mutex> g(pace_mu_);
    if (pace_armed_) {
      pace_armed_ = false;
      const double late = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - pace_drain_).count();
      if (late > 0.03) margin_ms_ = std::min(margin_ms_ + 0.5 * late, 1.0);
    }
  }
  Job job;
  job.slot = slot;
  job.B = B;
  job.done = std::move(done);
  job.t0 = std::chrono::steady_clock::now();
  try {
    HIP_CHECK(hipSetDevice(dev_));
    if (opt_.fail_batch_every > 0 && ++nth_batch_ % opt_.fail_batch_every == 0)
      throw std::runtime_error("injected batch failure (fail_batch_every)");
    Slot& sl = slots_[slot];
    job.ev = static_cast<int>((job_seq_++ % kTimingJobs) * kEvPerJob);
    job.bi = static_cast<int>(bucket_index(B));
    HIP_CHECK(hipEventRecord(tev_[job.ev + 5], s_prep_ ? s_prep_ : s_stage_[0]));  // input path starts (pacing model)
    bool any_text = false;
    long long* h_offs = sl.h_lens + max_batch_;
    long long* h_poffs = sl.h_lens + 2 * max_batch_;
    int wait_ticket[kStageStreams];  // per copy stream, the staged copy issued last covers the earlier ones
    bool copied[kStageStreams] = {};  // submit-time copies issued on that stream
    for (auto& w : wait_ticket) w = -1;
    int rr = 0;
    for (int i = 0; i < B; ++i) {
      h_offs[i] = 0;
      h_poffs[i] = -1;
      if (items[i].text) {
        if (!text_cap_ || items[i].text_len > text_cap_) throw std::runtime_error("input text exceeds device decode capacity");
        if (items[i].packed && !d_packed_) throw std::runtime_error("engine does not take packed text");
        const long t = items[i].staged;
        const auto tw0 = std::chrono::steady_clock::now();
        const bool issued = t >= 0 && t < n_stage_ && wait_staged(static_cast<int>(t)) == kIssued;
        if (t >= 0) {
          diag_submit_wait_ns_ += std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now() - tw0).count();
          if (issued && hipEventQuery(stage_ev_[t]) != hipSuccess) diag_not_ready_++;
        }
        if (issued) {  // already uploaded (raw, or packed: decoded straight from its packed slot)
          h_offs[i] = static_cast<long long>(t) * static_cast<long long>(text_cap_);
          if (stage_packed_[t]) h_poffs[i] = static_cast<long long>(t) * static_cast<long long>(text_cap_ / 2);
          int& w = wait_ticket[stage_stream_[t]];
          if (w < 0 || stage_seq_[t] > stage_seq_[w]) w = static_cast<int>(t);
        } else if (items[i].packed) {
          const size_t idx = static_cast<size_t>(n_stage_) + static_cast<size_t>(slot) * max_batch_ + i;
          h_offs[i] = static_cast<long long>(idx * text_cap_);
          h_poffs[i] = static_cast<long long>(idx * (text_cap_ / 2));
          const int si = rr++ % n_copy_streams_;
          HIP_CHECK(hipMemcpyAsync(d_packed_ + idx * (text_cap_ / 2), items[i].text, (items[i].text_len + 1) / 2,
                                   hipMemcpyHostToDevice, s_stage_[si]));
          h2d_bytes_.fetch_add(static_cast<long long>((items[i].text_len + 1) / 2), std::memory_order_relaxed);
          copied[si] = true;
        } else {
          const size_t idx = static_cast<size_t>(n_stage_) + static_cast<size_t>(slot) * max_batch_ + i;
          h_offs[i] = static_cast<long long>(idx * text_cap_);
          const int si = rr++ % n_copy_streams_;
          HIP_CHECK(hipMemcpyAsync(d_text_ + idx * text_cap_, items[i].text, items[i].text_len, hipMemcpyHostToDevice,
                                   s_stage_[si]));
          h2d_bytes_.fetch_add(static_cast<long long>(items[i].text_len), std::memory_order_relaxed);
          copied[si] = true;
        }
        sl.h_lens[i] = static_cast<long long>(items[i].text_len);
        any_text = true;
        continue;
      }
      sl.h_lens[i] = -1;
      const size_t n = std::min(items[i].len, in_numel_);
      float* dst = sl.d_in + static_cast<size_t>(i) * in_numel_;
      const int si = rr++ % n_copy_streams_;
      if (n) HIP_CHECK(hipMemcpyAsync(dst, items[i].input, n * sizeof(float), hipMemcpyHostToDevice, s_stage_[si]));
      h2d_bytes_.fetch_add(static_cast<long long>(n * sizeof(float)), std::memory_order_relaxed);
      if (n < in_numel_) HIP_CHECK(hipMemsetAsync(dst + n, 0, (in_numel_ - n) * sizeof(float), s_stage_[si]));
      copied[si] = true;
    }
    sl.h_lens[live_index()] = use_live_ ? B : max_batch_;
    for (int i = B; i < max_batch_; ++i) {
      sl.h_lens[i] = -1;
      h_offs[i] = 0;
      h_poffs[i] = -1;
    }
    job.has_text = any_text;
    const size_t bi = static_cast<size_t>(job.bi);
    // PREP (decode-table fetch from host-coherent memory, device decode, input prep) runs on copy
    // stream 0 behind this batch's copies, overlapping the previous batch's MAIN on the compute
    // stream; MAIN waits for it.  Timing events come from a ring (a job's events outlive its slot's
    // reuse): pre = compute stream done with earlier work, fwd0/fwd1 around MAIN, p0/p1 around PREP.
    // PREP runs on its own stream when there is one (early upload: the stager's copies for later
    // batches must not queue behind this batch's decode on a copy stream), else on copy stream 0
    hipStream_t ps = s_prep_ ? s_prep_ : s_stage_[0];
    hipStream_t cs = s_exec_[slot % n_exec_];
    for (int si = s_prep_ ? 0 : 1; si < kStageStreams; ++si)
      if (copied[si]) {
        HIP_CHECK(hipEventRecord(sl.ev_h2d[si], s_stage_[si]));
        HIP_CHECK(hipStreamWaitEvent(ps, sl.ev_h2d[si], 0));
      }
    bool used_staged = false;
    for (int w : wait_ticket)
      if (w >= 0) {
        HIP_CHECK(hipStreamWaitEvent(ps, stage_ev_[w], 0));
        used_staged = true;
      }
    if (used_staged) staged_used_.fetch_add(1, std::memory_order_relaxed);
    HIP_CHECK(hipEventRecord(tev_[job.ev + 6], ps));  // all input copies landed
    if (prep_on_compute_) {
      // PREP in line on the compute stream, after the previous MAIN: only the copies need lead
      HIP_CHECK(hipEventRecord(sl.ev_prep, ps));
      HIP_CHECK(hipEventRecord(tev_[job.ev], cs));
      HIP_CHECK(hipStreamWaitEvent(cs, sl.ev_prep, 0));
      ps = cs;
    }
    HIP_CHECK(hipEventRecord(tev_[job.ev + 3], ps));
    if (!prep_graphs_.empty()) {
      HIP_CHECK(hipGraphLaunch(prep_graphs_[bi * depth_ + slot], ps));
      graph_replays_.fetch_add(1, std::memory_order_relaxed);
    } else {
      encode_forward(buckets_[bi], slot, ps, nullptr, PREP);
    }
    HIP_CHECK(hipEventRecord(tev_[job.ev + 4], ps));
    if (!prep_on_compute_) {
      HIP_CHECK(hipEventRecord(sl.ev_prep, ps));
      HIP_CHECK(hipEventRecord(tev_[job.ev], cs));
      HIP_CHECK(hipStreamWaitEvent(cs, sl.ev_prep, 0));
    }
    HIP_CHECK(hipEventRecord(tev_[job.ev + 1], cs));
    if (!graphs_.empty()) {
      HIP_CHECK(hipGraphLaunch(graphs_[bi * depth_ + slot], cs));
      graph_replays_.fetch_add(1, std::memory_order_relaxed);
    } else {
      encode_forward(buckets_[bi], slot, cs, nullptr, MAIN);
    }
    HIP_CHECK(hipEventRecord(tev_[job.ev + 2], cs));
    if (comm_) {
      // this rank's shard ran: its flag travels with the status rows, so the other ranks answer
      // this shard's items from the gathered rows (flag 0: they fail them; see the catch below)
      HIP_CHECK(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(sl.d_status + rank_ok_index()), 1, 1, cs));
      dp_collectives(sl, B, result_stream(sl, cs));
      job.has_text = text_cap_ > 0;
    } else {
      hipStream_t os = result_stream(sl, cs);
      HIP_CHECK(hipMemcpyAsync(sl.h_out, sl.d_out, sizeof(float) * out_numel_ * B, hipMemcpyDeviceToHost, os));
      d2h_bytes_.fetch_add(static_cast<long long>(sizeof(float) * out_numel_ * B), std::memory_order_relaxed);
      if (any_text) {
        HIP_CHECK(hipMemcpyAsync(sl.h_status, sl.d_status, sizeof(int) * 2 * max_batch_, hipMemcpyDeviceToHost, os));
        d2h_bytes_.fetch_add(static_cast<long long>(sizeof(int) * 2 * max_batch_), std::memory_order_relaxed);
      }
      HIP_CHECK(hipEventRecord(sl.ev_d2h, os));
    }
  } catch (const std::exception& e) {
    job.error = e.what();
    if (comm_ && !dp_issued_) {
      // The other ranks' collectives are waiting for this rank's: issue them anyway with the
      // shard flag cleared (a rank that skipped them would hang the whole group), so they fail
      // this shard's items and answer the rest.
      try {
        Slot& sl = slots_[slot];
        hipStream_t cs = s_exec_[slot % n_exec_];
        HIP_CHECK(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(sl.d_status + rank_ok_index()), 0, 1, cs));
        dp_collectives(sl, B, result_stream(sl, cs));
        job.dp_gathered = true;
        job.has_text = text_cap_ > 0;
      } catch (const std::exception&) {
      }
    }
  }
  dp_issued_ = false;
  diag_submit_ns_ += std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now() - job.t0).count();
  {
    std::lock_guard<std::mutex> g(mu_);
    if (job.error.empty()) {
      last_ev_ = job.ev;
      last_bi_ = job.bi;
    }
    jobs_.push_back(std::move(job));
    ++callbacks_running_;
  }
  cv_.notify_all();
}

// Just-in-time dispatch.  With the GPU busy on batch k, dispatching batch k+1 as soon as a slot
// frees makes it carry only what queued during k's submit; holding it until k is about to drain
// lets it absorb the requests that arrive meanwhile (bigger batches, better MFMA occupancy).
// Estimate: k's MAIN start (observed through its event) + the EMA device time of k's bucket - lead,
// where lead (next batch's copies + prep) adapts to the GPU idle time measured before each MAIN.
std::chrono::steady_clock::time_point HipEngine::dispatch_not_before() {
  using clk = std::chrono::steady_clock;
  const auto now = clk::now();
  if (!opt_.pace || n_exec_ > 1 || graphs_.empty()) return now;
  int ev, bi;
  {
    std::lock_guard<std::mutex> g(mu_);
    if (inflight_ == 0 || last_ev_ < 0) return now;
    ev = last_ev_;
    bi = last_bi_;
  }
  double est, lead, in_ms;
  {
    std::lock_guard<std::mutex> g(pace_mu_);
    est = est_ms_[bi];
    lead = lead_ms_;
    in_ms = input_ms_;
  }
  if (est <= 0.0 || est <= lead) return now;
  (void)hipSetDevice(dev_);
  const auto give_up = now + std::chrono::milliseconds(20);
  hipError_t q;
  while ((q = hipEventQuery(tev_[ev + 1])) == hipErrorNotReady) {  // k's MAIN has not started yet
    if (clk::now() > give_up) return clk::now();
    std::this_thread::sleep_for(std::chrono::microseconds(15));
  }
  if (q != hipSuccess || hipEventQuery(tev_[ev + 2]) != hipErrorNotReady) return clk::now();  // k drained
  const auto t0 = clk::now();
  const auto drain = t0 + std::chrono::duration_cast<clk::duration>(std::chrono::duration<double, std::milli>(est));
  const auto t = t0 + std::chrono::duration_cast<clk::duration>(std::chrono::duration<double, std::milli>(est - (lead_scale_ == 1.0 ? lead : in_ms * lead_scale_)));
  {
    std::lock_guard<std::mutex> g(pace_mu_);
    pace_drain_ = drain;
    pace_armed_ = true;
  }
  paced_batches_++;
  return t;
}

// EngineOptions::efficient_batch: the largest B <= queued whose per-image device time (the
// start-up curve) is within efficient_batch_tol of the best B' <= queued.  Per-image time falls
// with B except where a layer's tile grid spills into one more round of blocks (ResNet50 fp32:
// 61.6 us per image at B = 20, 69.6 at 21, profiles/r5_batch_curve.md), so this only ever cuts a
// batch back to just below such a step; the requests left over lead the next batch.
// A cut needs a smaller size cheaper per image by more than efficient_batch_margin (inside a
// bucket the curve is flat to within replay noise).
int HipEngine::preferred_batch(int queued) const {
  return pick_efficient_batch(batch_ms_.empty() ? nullptr : batch_ms_.data(), max_batch_, queued,
                              opt_.efficient_batch_tol, opt_.efficient_batch_margin,
                              opt_.efficient_batch_ends ? buckets_.data() : nullptr, static_cast<int>(buckets_.size()));
}

void HipEngine::synchronize() {
  std::unique_lock<std::mutex> lk(mu_);
  slot_cv_.wait(lk, [&] { return inflight_ == 0 && callbacks_running_ == 0; });
}

// Block until the stager has issued (or failed) ticket t's copy; returns its state.
int HipEngine::wait_staged(int t) {
  std::unique_lock<std::mutex> lk(stage_mu_);
  stage_done_cv_.wait(lk, [&] { return stage_state_[t] != kQueued; });
  return stage_state_[t];
}

void HipEngine::stager_loop() {
  (void)hipSetDevice(dev_);
  unsigned long long rr = 0;
  while (true) {
    StageReq rq;
    {
      std::unique_lock<std::mutex> lk(stage_mu_);
      stage_cv_.wait(lk, [&] { return stage_stop_ || !stage_q_.empty(); });
      if (stage_q_.empty()) return;
      rq = stage_q_.front();
      stage_q_.pop_front();
    }
    // round-robin over kStageStreams copy streams (one reaches ~36 GB/s for 1 MiB pinned copies,
    // two ~47 GB/s); per stream copies complete in issue order, which the sequence number records
    const int si = static_cast<int>(rr++ % n_copy_streams_);
    const auto ti0 = std::chrono::steady_clock::now();
    const bool ok = (rq.packed ? hipMemcpyAsync(d_packed_ + static_cast<size_t>(rq.t) * (text_cap_ / 2), rq.text,
                                                (rq.len + 1) / 2, hipMemcpyHostToDevice, s_stage_[si])
                               : hipMemcpyAsync(d_text_ + static_cast<size_t>(rq.t) * text_cap_, rq.text, rq.len,
                                                hipMemcpyHostToDevice, s_stage_[si])) == hipSuccess &&
                    hipEventRecord(stage_ev_[rq.t], s_stage_[si]) == hipSuccess;
    diag_issue_ns_ += std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now() - ti0).count();
    if (ok) h2d_bytes_.fetch_add(static_cast<long long>(rq.packed ? (rq.len + 1) / 2 : rq.len), std::memory_order_relaxed);
    {
      std::lock_guard<std::mutex> g(stage_mu_);
      stage_stream_[rq.t] = si;
      stage_seq_[rq.t] = ++stage_counter_[si];
      stage_state_[rq.t] = ok ? kIssued : kFailed;
    }
    stage_done_cv_.notify_all();
  }
}

// A data-parallel batch's result: every rank's rows and status tables, with the shard flags.
void HipEngine::fill_gathered(BatchResult& r, Slot& sl, const Job& job) {
  r.gathered = dp_world_;
  r.outputs = sl.h_gather;
  r.status = job.has_text ? sl.h_gstatus.get() : nullptr;
  r.ntok = r.status ? sl.h_gstatus + max_batch_ : nullptr;
  r.status_stride = static_cast<int>(status_len());
  rank_ok_copy_.resize(static_cast<size_t>(dp_world_));
  for (int k = 0; k < dp_world_; ++k)
    rank_ok_copy_[static_cast<size_t>(k)] = sl.h_gstatus[static_cast<size_t>(k) * status_len() + rank_ok_index()];
  r.rank_ok = rank_ok_copy_.data();
}

void HipEngine::completion_loop() {
  (void)hipSetDevice(dev_);
  while (true) {
    Job job;
    {
      std::unique_lock<std::mutex> lk(mu_);
      cv_.wait(lk, [&] { return stop_ || !jobs_.empty(); });
      if (jobs_.empty()) return;
      job = std::move(jobs_.front());
      jobs_.pop_front();
    }
    Slot& sl = slots_[job.slot];
    TraceRange tr_done("engine.completion(d2h wait+callback)");
    BatchResult r;
    if (job.error.empty()) {
      hipError_t e;
      if (completion_poll_us_ > 0) {
        // sleep-poll instead of the runtime wait, which was seen spinning a whole CPU even with a
        // blocking-sync event (gpurun_out/r2_46 threads_*.txt): that CPU serves HTTP/JSON instead
        while ((e = hipEventQuery(sl.ev_d2h)) == hipErrorNotReady)
          std::this_thread::sleep_for(std::chrono::microseconds(completion_poll_us_));
      } else {
        e = hipEventSynchronize(sl.ev_d2h);
      }
      if (e != hipSuccess) {
        r.ok = false;
        r.error = std::string("device error: ") + hipGetErrorString(e);
      } else {
        float ms = 0;
        if (hipEventElapsedTime(&ms, tev_[job.ev + 1], tev_[job.ev + 2]) == hipSuccess) r.device_us = ms * 1000.0;
        float wait_ms = 0, gap_ms = 0;
        if (hipEventElapsedTime(&wait_ms, tev_[job.ev], tev_[job.ev + (prep_on_compute_ ? 3 : 1)]) == hipSuccess) copy_wait_ms_total_ = copy_wait_ms_total_.load() + wait_ms;
        if (prev_ev_ >= 0 && hipEventElapsedTime(&gap_ms, tev_[prev_ev_ + 2], tev_[job.ev]) == hipSuccess && gap_ms > 0)
          gpu_gap_ms_total_ = gpu_gap_ms_total_.load() + gap_ms;
        prev_ev_ = job.ev;
        {
          // pacing model: device-time EMA per bucket, and lead = EMA of this batch's input path
          // (first copy issued -> PREP done, on the device) + a margin for the dispatch itself
          // that grows when MAIN had to wait for its input anyway (wait_ms: compute stream idle
          // behind the copies/prep) and shrinks slowly otherwise
          float in_ms = 0;
          // (PREP in line on the compute stream: the lead covers the copies only)
          const bool have_in =
              hipEventElapsedTime(&in_ms, tev_[job.ev + 5], tev_[job.ev + (prep_on_compute_ ? 6 : 4)]) == hipSuccess;
          std::lock_guard<std::mutex> g(pace_mu_);
          double& e = est_ms_[job.bi];
          e = e > 0.0 ? 0.8 * e + 0.2 * ms : ms;
          if (have_in) input_ms_ = input_ms_ > 0.0 ? 0.8 * input_ms_ + 0.2 * in_ms : in_ms;
          if (wait_ms > 0.02) margin_ms_ = std::min(margin_ms_ + 0.02, 1.0);
          else margin_ms_ = std::max(margin_ms_ - 0.004, 0.03);
          lead_ms_ = input_ms_ + margin_ms_;
          lead_ms_total_ += lead_ms_;
        }
        float prep_ms = 0;
        if (hipEventElapsedTime(&prep_ms, tev_[job.ev + 3], tev_[job.ev + 4]) == hipSuccess)
          prep_ms_total_ = prep_ms_total_.load() + prep_ms;
        r.outputs = sl.h_out;
        r.output_numel = out_numel_;
        if (job.has_text) {
          r.status = sl.h_status;
          r.ntok = sl.h_status + max_batch_;
        }
        if (comm_) fill_gathered(r, sl, job);
        batches_++;
        images_ += job.B;
        device_ms_total_ = device_ms_total_.load() + ms;
      }
    } else {
      r.ok = false;
      r.error = job.error;
      if (job.dp_gathered && comm_ && hipEventSynchronize(sl.ev_d2h) == hipSuccess) {
        // this rank's shard failed, the others' rows arrived: hand them over with the flags, so the
        // DP engine fails exactly this shard's items (the host backend's semantics, dp_layout.h)
        r.output_numel = out_numel_;
        fill_gathered(r, sl, job);
      }
    }
    r.wall_us = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - job.t0).count();
    // Take the results out of the slot's pinned buffers and free the slot BEFORE the callbacks
    // (cache inserts, response hand-off for B requests): the batcher can dispatch the next batch
    // into this slot while they run, so the GPU does not idle behind host bookkeeping.
    if (r.ok || r.rank_ok) {
      const size_t rows = static_cast<size_t>(job.B) * (comm_ ? dp_world_ : 1);
      if (r.outputs) {
        out_copy_.assign(r.outputs, r.outputs + rows * out_numel_);
        r.outputs = out_copy_.data();
      }
      if (r.status) {
        const size_t n = comm_ ? status_len() * dp_world_ : 2 * static_cast<size_t>(max_batch_);
        const int* base = r.status;
        status_copy_.assign(base, base + n);
        r.status = status_copy_.data();
        r.ntok = status_copy_.data() + max_batch_;
      }
    }
    {
      std::lock_guard<std::mutex> g(mu_);
      --inflight_;
    }
    slot_cv_.notify_all();
    try {
      job.done(r);
    } catch (...) {
    }
    {
      std::lock_guard<std::mutex> g(mu_);
      --callbacks_running_;
    }
    slot_cv_.notify_all();
  }
}

// The stream a batch's result copies / collectives go on: s_out_ behind an event after the work
// queued on cs so far (EngineOptions::result_stream), else cs itself.
hipStream_t HipEngine::result_stream(Slot& sl, hipStream_t cs) {
  if (!s_out_) return cs;
  HIP_CHECK(hipEventRecord(sl.ev_main, cs));
  HIP_CHECK(hipStreamWaitEvent(s_out_, sl.ev_main, 0));
  return s_out_;
}

// Data parallel: every rank contributes its B rows and its status table to every other rank over
// xGMI (the same collectives in the same order on every rank, whatever its shard holds), then
// copies all rows and tables to its host; a group of one copies straight from d_out.
void HipEngine::dp_collectives(Slot& sl, int B, hipStream_t cs) {
  dp_issued_ = true;
  if (dp_world_ > 1) {  // one grouped operation: logits + status table (shard flag included)
    comm_->group_begin();
    comm_->all_gather(sl.d_out, sl.d_gather, sizeof(float) * out_numel_ * B, cs);
    comm_->all_gather(sl.d_status, sl.d_gstatus, sizeof(int) * status_len(), cs);
    comm_->group_end();
    dp_collective_ops_.fetch_add(1, std::memory_order_relaxed);
  }
  HIP_CHECK(hipEventRecord(sl.ev_gather, cs));
  HIP_CHECK(hipMemcpyAsync(sl.h_gather, dp_world_ > 1 ? sl.d_gather : sl.d_out, sizeof(float) * out_numel_ * B * dp_world_,
                           hipMemcpyDeviceToHost, cs));
  HIP_CHECK(hipMemcpyAsync(sl.h_gstatus, dp_world_ > 1 ? sl.d_gstatus : sl.d_status, sizeof(int) * status_len() * dp_world_,
                           hipMemcpyDeviceToHost, cs));
  d2h_bytes_.fetch_add(static_cast<long long>((sizeof(float) * out_numel_ * B + sizeof(int) * status_len()) * dp_world_),
                       std::memory_order_relaxed);
  HIP_CHECK(hipEventRecord(sl.ev_d2h, cs));
}

}  // namespace hip
}  // namespace die
