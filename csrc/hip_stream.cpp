// wait_stream and GpuTransport (hip_stream.hpp).
#include "hip_stream.hpp"

#include <chrono>
#include <thread>

#include "bootstrap.hpp"
#include "common.hpp"
#include "hip_check.hpp"

namespace p2p {

void wait_stream(hipStream_t stream, double timeout_s, int rank, const WaitPolicy& policy) {
  const double t0 = now_seconds();
  const double deadline = t0 + timeout_s;
  const auto who = [&] { return rank < 0 ? std::string() : strfmt("rank %d: ", rank); };
  for (long it = 0;; ++it) {
    const hipError_t e = hipStreamQuery(stream);
    if (e == hipSuccess) return;
    if (e != hipErrorNotReady) P2P_FATAL(strfmt("%s error: %s", policy.error_noun, hipGetErrorString(e)));
    if ((it & 255) == 0) {
      const bool abort = abort_requested(), answer = abort && policy.answers_abort;
      std::string why;
      if (answer) why = who() + "aborted while waiting (the run's deadline passed)";
      if (why.empty() && policy.poll_error) why = policy.poll_error();
      const double now = now_seconds();
      if (why.empty() && (abort || now > deadline))
        why = who() + strfmt("%s did not finish within %.0f s%s", policy.noun, timeout_s, policy.tail);
      if (!why.empty()) {
        if (policy.before_failure) policy.before_failure();
        if (answer) note_abort_done();
        P2P_FATAL(why);
      }
      if (now - t0 > 20e-3) std::this_thread::sleep_for(std::chrono::microseconds(20));
    }
  }
}

GpuTransport::GpuTransport(Bootstrap& boot, const TransportOptions& opt, bool keep_graphs, const char* none_visible,
                           const char* out_of_range)
    : rank_(boot.rank()), n_(boot.size()), timeout_(opt.timeout_s), checks_(static_cast<dev::VerifyImpl>(opt.verify_impl)),
      keep_graphs_(keep_graphs) {
  int ndev = 0;
  const hipError_t e = hipGetDeviceCount(&ndev);
  if (e != hipSuccess || ndev == 0)
    P2P_FATAL(strfmt(none_visible, rank_, e == hipSuccess ? "0 devices" : hipGetErrorString(e)));
  device_ = opt.device >= 0 ? opt.device : 0;
  if (device_ >= ndev) P2P_FATAL(strfmt(out_of_range, rank_, device_, ndev));
  HIPCHECK(hipSetDevice(device_));
  HIPCHECK(hipStreamCreateWithFlags(&stream_, hipStreamNonBlocking));
}

void GpuTransport::destroy_graphs() {
  for (auto ex : execs_)
    if (ex) (void)hipGraphExecDestroy(ex);
  for (auto g : graphs_)
    if (g) (void)hipGraphDestroy(g);
  execs_.clear();
  graphs_.clear();
}

void GpuTransport::destroy_stream_objects() {
  destroy_graphs();
  for (auto ev : events_) (void)hipEventDestroy(ev);
  events_.clear();
  if (stream_) (void)hipStreamDestroy(stream_);
  stream_ = nullptr;
}

int GpuTransport::mark() {
  if (next_event_ == static_cast<int>(events_.size())) {
    hipEvent_t ev;
    HIPCHECK(hipEventCreateWithFlags(&ev, timing_event_flags()));
    events_.push_back(ev);
  }
  HIPCHECK(hipEventRecord(events_[static_cast<size_t>(next_event_)], stream_));
  return next_event_++;
}
double GpuTransport::elapsed_ms(int from, int to) {
  float ms = 0;
  HIPCHECK(hipEventElapsedTime(&ms, mark_event(from), mark_event(to)));
  return ms;
}

void GpuTransport::capture_begin() {
  HIPCHECK(hipStreamBeginCapture(stream_, hipStreamCaptureModeThreadLocal));
  capturing_ = true;
}
int GpuTransport::capture_end() {
  capturing_ = false;
  hipGraph_t g = nullptr;
  HIPCHECK(hipStreamEndCapture(stream_, &g));
  hipGraphExec_t ex = nullptr;
  HIPCHECK(hipGraphInstantiate(&ex, g, nullptr, nullptr, 0));
  if (!keep_graphs_) {
    HIPCHECK(hipGraphDestroy(g));
    g = nullptr;
  }
  graphs_.push_back(g);
  execs_.push_back(ex);
  return static_cast<int>(execs_.size()) - 1;
}
void GpuTransport::graph_launch(int handle) {
  hipGraphExec_t ex = execs_.at(static_cast<size_t>(handle));
  P2P_CHECK(ex != nullptr, "graph_launch: the graph was released");
  HIPCHECK(hipGraphLaunch(ex, stream_));
}
void GpuTransport::graph_release(int handle) {
  hipGraphExec_t& ex = execs_.at(static_cast<size_t>(handle));
  hipGraph_t& g = graphs_.at(static_cast<size_t>(handle));
  if (ex) HIPCHECK(hipGraphExecDestroy(ex));
  if (g) HIPCHECK(hipGraphDestroy(g));
  ex = nullptr;
  g = nullptr;
}

bool GpuTransport::stream_idle() {
  const hipError_t e = hipStreamQuery(stream_);
  if (e != hipSuccess && e != hipErrorNotReady) P2P_FATAL(strfmt("stream error: %s", hipGetErrorString(e)));
  return e == hipSuccess;
}

}  // namespace p2p
