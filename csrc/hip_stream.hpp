// What every user of a HIP stream here shares: the bounded, abort-aware wait
// (wait_stream) and GpuTransport, the part of a Transport that is the same on
// every GPU data plane (RcclTransport, IpcTransport): the device, the main
// stream with its marks and graphs, the device checks, the stream gate and
// the background load.  GPU translation units only.
#pragma once

#include <hip/hip_runtime.h>

#include <functional>
#include <memory>
#include <string>
#include <vector>

#include "device_checks.hpp"
#include "hip_check.hpp"
#include "load.hpp"
#include "provenance.hpp"
#include "stream_gate.hpp"
#include "transport.hpp"

namespace p2p {

// What differs between the users of wait_stream.  Both callables may be empty.
struct WaitPolicy {
  const char* noun = "stream";        // "<noun> did not finish within N s<tail>"
  const char* tail = "";
  const char* error_noun = "stream";  // "<error_noun> error: <HIP's text>"
  // A transport's wait answers the run's abort request (note_abort_done, its
  // own text); the load's wait only ends, with its timeout text.
  bool answers_abort = true;
  std::function<std::string()> poll_error;  // non-empty: fatal with it; asked every 256th poll only
  std::function<void()> before_failure;     // runs before any fatal path
};

// Bounded poll instead of hipStreamSynchronize: spins for the first 20 ms (so
// per-message syncs in wallclock mode are not inflated by sleeps), then backs
// off in 20 us sleeps.  Every 256th poll looks at the run's abort request,
// policy.poll_error and the deadline.  rank < 0: no "rank N: " in the texts.
void wait_stream(hipStream_t stream, double timeout_s, int rank, const WaitPolicy& policy);

class GpuTransport : public Transport {
 public:
  int rank() const override { return rank_; }
  int nranks() const override { return n_; }
  std::string device_desc() const override { return desc_; }
  std::string device_key() const override { return gpu_memory_key(device_); }
  void set_timeout(double seconds) override { timeout_ = seconds; }

  // On the main stream; the checks wait behind the bounded, abort-aware
  // sync() (device_checks.hpp).
  void fill(void* p, size_t bytes, uint64_t seed) override {
    before_buffer_work();
    dev::launch_fill(p, bytes, seed, stream_);
  }
  void zero(void* p, size_t bytes) override {
    before_buffer_work();
    HIPCHECK(hipMemsetAsync(p, 0, bytes, stream_));
  }
  VerifyResult verify(const void* p, size_t bytes, uint64_t seed) override {
    before_buffer_work();
    return checks_.verify(p, bytes, seed, stream_, [this] { sync(); });
  }
  std::vector<VerifyResult> verify_many(const std::vector<VerifyJob>& jobs) override {
    if (jobs.empty()) return {};
    before_buffer_work();
    return checks_.verify_many(jobs, stream_, [this] { sync(); });
  }
  std::vector<DiagExtent> diagnose(const void* p, size_t bytes, uint64_t seed,
                                   const std::vector<DiagCandidate>& candidates) override {
    before_buffer_work();
    return checks_.diagnose(p, bytes, seed, candidates, stream_, [this] { sync(); });
  }

  int mark() override;  // one event per mark on the main stream
  double elapsed_ms(int from, int to) override;
  void clear_marks() override { next_event_ = 0; }

  void capture_begin() override;
  int capture_end() override;
  void graph_launch(int handle) override;
  void graph_release(int handle) override;

  bool gate_arm(double timeout_s) override {
    gate_.arm(stream_, timeout_s);
    return true;
  }
  void gate_release() override { gate_.release(); }
  bool gate_timed_out() override { return gate_.timed_out(); }
  bool stream_idle() override;
  std::unique_ptr<BackgroundLoad> make_load(const std::string& kind, int wgs) override {
    HIPCHECK(hipSetDevice(device_));
    return make_background_load(kind, wgs, timeout_, stream_);
  }

 protected:
  // Picks opt.device (0 if unset), checks that it is visible, makes it
  // current and creates the main stream.  keep_graphs: a captured hipGraph_t
  // lives until graph_release() (RCCL: it holds the communicator's resources
  // next to the executable); otherwise it goes once it is instantiated.  The
  // two errors of opening the device come in the transport's own words, as
  // printf formats: none_visible(rank, HIP's text or "0 devices") and
  // out_of_range(rank, device wanted, devices visible).
  GpuTransport(Bootstrap& boot, const TransportOptions& opt, bool keep_graphs, const char* none_visible,
               const char* out_of_range);
  // No destructor of its own: the derived destructor decides whether and when
  // the stream's objects go (RCCL leaks them under kernels that never ended).
  void destroy_graphs();
  void destroy_stream_objects();  // graphs (if still there), mark events, the main stream

  // The main stream is about to touch payload buffers (fill, zero, verify,
  // diagnose).  RCCL joins its side streams here.
  virtual void before_buffer_work() {}
  hipEvent_t mark_event(int id) const { return events_.at(static_cast<size_t>(id)); }

  const int rank_, n_;
  double timeout_;
  int device_ = 0;
  hipStream_t stream_ = nullptr;
  std::string desc_;
  DeviceChecks checks_;  // verify, verify_many, diagnose; the inline-check records
  StreamGate gate_;
  bool capturing_ = false;

 private:
  const bool keep_graphs_;
  std::vector<hipEvent_t> events_;  // per mark, on the main stream
  int next_event_ = 0;
  std::vector<hipGraphExec_t> execs_;
  std::vector<hipGraph_t> graphs_;  // parallel to execs_; null unless keep_graphs_
};

}  // namespace p2p
