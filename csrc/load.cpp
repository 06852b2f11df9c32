// BackgroundLoad on a HIP device (background_load.hpp, load.hpp): a train of
// short launches of the load kernels on a non-blocking stream of its own.
#include "load.hpp"

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <thread>
#include <vector>

#include "common.hpp"
#include "hip_check.hpp"
#include "hip_stream.hpp"
#include "kernels.hpp"

namespace p2p {
namespace {

constexpr double kLaunchTargetS = 250e-6;  // one launch alone
constexpr double kAloneTrainS = 20e-3;     // the train alone_rate is measured over
constexpr double kCalibrateTrainS = 5e-3;  // the trains calibrate() sizes a launch by
constexpr size_t kHbmScratch = size_t{256} << 20;
constexpr uint64_t kLoadSeed = 0x10ADull;

class HipBackgroundLoad final : public BackgroundLoad {
 public:
  HipBackgroundLoad(const std::string& kind, int wgs, double timeout_s, hipStream_t beside)
      : kind_(kind), mfma_(kind == "mfma"), wgs_(wgs > 0 ? wgs : dev::cu_count()), timeout_(timeout_s), beside_(beside) {
    P2P_CHECK(mfma_ || kind == "hbm", "load kind must be 'mfma' or 'hbm'");
    P2P_CHECK(wgs >= 0, "load: workgroups must be >= 1 (0: one per CU)");
    try {
      allocate();
    } catch (...) {  // a destructor does not run for a constructor that threw
      release();
      throw;
    }
  }

  ~HipBackgroundLoad() override {
    if (cancel_) __atomic_store_n(cancel_, 1u, __ATOMIC_RELEASE);
    release();
  }

 private:
  void allocate() {
    // Fine-grained (coherent) host memory, as the stream gate's flag: the
    // kernels' system-scope accesses and the host's see each other's writes.
    HIPCHECK(hipHostMalloc(reinterpret_cast<void**>(&words_), 128, hipHostMallocCoherent));
    cancel_ = reinterpret_cast<unsigned int*>(words_);
    done_ = reinterpret_cast<unsigned long long*>(words_ + 64);
    __atomic_store_n(cancel_, 0u, __ATOMIC_RELEASE);
    __atomic_store_n(done_, 0ull, __ATOMIC_RELEASE);
    HIPCHECK(hipMalloc(reinterpret_cast<void**>(&tickets_), sizeof(unsigned long long)));
    HIPCHECK(hipMemset(tickets_, 0, sizeof(unsigned long long)));
    const size_t tile_bytes = dev::kLoadWaves * dev::kLoadTileFloats * sizeof(float);  // also what the probe writes
    const size_t out_bytes = mfma_ ? static_cast<size_t>(wgs_) * tile_bytes
                                   : std::max(static_cast<size_t>(wgs_) * sizeof(unsigned long long), tile_bytes);
    HIPCHECK(hipMalloc(&out_, out_bytes));
    pick_stream();
    if (!mfma_) {
      HIPCHECK(hipMalloc(&scratch_, kHbmScratch));
      dev::launch_fill(scratch_, kHbmScratch, kLoadSeed, stream_);
    }
    HIPCHECK(hipEventCreate(&ev_[0]));
    HIPCHECK(hipEventCreate(&ev_[1]));
    drain();
  }

  // A process has a few hardware queues (4 by default) and the runtime puts
  // a new stream on the least used one.  A load stream that lands on the
  // queue of the stream the transfers run on does not run beside them: the
  // queue takes the whole train first and the cell after it, on a quiet GPU.
  // So up to kProbeStreams candidates are made and held, and the first one on
  // which a ~200 us one-workgroup kernel overlaps the same kernel on `beside_`
  // (both take about the time of one, not of two) is kept.
  void pick_stream() {
    constexpr int kProbeStreams = 6;
    std::vector<hipStream_t> made;
    auto drop_others = [&] {
      for (hipStream_t c : made)
        if (c != stream_) (void)hipStreamDestroy(c);
    };
    try {
      for (int i = 0; i < kProbeStreams && !stream_; ++i) {
        hipStream_t c = nullptr;
        HIPCHECK(hipStreamCreateWithFlags(&c, hipStreamNonBlocking));
        made.push_back(c);
        if (!beside_ || runs_beside(c)) stream_ = c;
      }
      if (!stream_) {
        stream_ = made.front();
        std::fprintf(stderr,
                     "[p2p] load: no stream of %d ran beside the transfers' stream (hardware queues shared): a loaded "
                     "cell may run after the load's train, not beside it (\"covered\": false)\n", kProbeStreams);
      }
    } catch (...) {
      drop_others();
      throw;
    }
    drop_others();
  }

  bool runs_beside(hipStream_t c) {
    constexpr uint32_t kProbeReps = 4096;  // 8193 dependent MFMAs of one wave per SIMD: about 200 us
    float* out = static_cast<float*>(out_);
    auto both = [&](bool with_beside) {
      const double t0 = now_seconds();
      if (with_beside) dev::launch_load_mfma(1, kProbeReps, kLoadSeed, out, dev::LoadCtl{}, beside_);
      dev::launch_load_mfma(1, kProbeReps, kLoadSeed, out, dev::LoadCtl{}, c);
      drain(c);
      if (with_beside) drain(beside_);
      return now_seconds() - t0;
    };
    both(true);  // first use: code object, queues
    const double one = std::min(both(false), both(false));
    const double two = std::min(both(true), both(true));
    return two < 1.5 * one;
  }

  // Frees whatever allocate() got as far as making (every handle starts
  // null).  Memory under kernels that never finished is leaked, not freed.
  void release() {
    if (!drain_quietly()) return;
    for (hipEvent_t e : ev_)
      if (e) (void)hipEventDestroy(e);
    if (scratch_) (void)hipFree(scratch_);
    if (out_) (void)hipFree(out_);
    if (tickets_) (void)hipFree(tickets_);
    if (words_) (void)hipHostFree(words_);
    if (stream_) (void)hipStreamDestroy(stream_);
  }

 public:
  std::string kind() const override { return kind_; }
  int wgs() const override { return wgs_; }
  const char* unit() const override { return mfma_ ? "TFLOP/s" : "TB/s"; }
  double launch_s() const override { return launch_s_; }
  double alone_rate() const override { return alone_rate_; }

  void calibrate() override {
    __atomic_store_n(cancel_, 0u, __ATOMIC_RELEASE);
    amount_ = mfma_ ? 256 : 1;
    time_train(2);  // first use: code object load
    // Three rounds, each timing a train of about kCalibrateTrainS at the
    // current size, so the clocks have settled under this very load before a
    // launch is measured (4-launch trains, timed while the clocks still
    // ramped, left the launches 25-38% short of the target).
    for (int round = 0; round < 3; ++round) {
      const double per = launch_time(kCalibrateTrainS);
      const double want = static_cast<double>(amount_) * kLaunchTargetS / per;
      amount_ = static_cast<uint32_t>(std::clamp(want + 0.5, 1.0, 1e9));
    }
    launch_s_ = launch_time(kCalibrateTrainS);
    const long n = std::max<long>(1, static_cast<long>(kAloneTrainS / launch_s_ + 0.5));
    alone_rate_ = static_cast<double>(n) * work_per_launch() / time_train(n) / 1e12;
  }

  void start(double expected_s) override {
    P2P_CHECK(launch_s_ > 0, "load: start() before calibrate()");
    if (running_) {  // a phase that threw between start() and stop()
      __atomic_store_n(cancel_, 1u, __ATOMIC_RELEASE);
      drain();
      running_ = false;
    }
    __atomic_store_n(cancel_, 0u, __ATOMIC_RELEASE);
    base_ = ordinal_;
    const LoadPlan plan = load_plan(expected_s, launch_s_);
    enqueue(plan.launches);
    enqueued_ = plan.launches;
    win_[0] = win_[1] = Stamp{};
    running_ = true;
  }

  void window_begin() override { win_[0] = stamp(); }
  void window_end() override { win_[1] = stamp(); }

  LoadStats stop() override {
    P2P_CHECK(running_, "load: stop() without start()");
    __atomic_store_n(cancel_, 1u, __ATOMIC_RELEASE);
    drain();
    running_ = false;
    LoadStats s;
    s.launches = enqueued_;
    s.launches_done = static_cast<long>(stamp().done - base_);
    if (win_[0].set && win_[1].set) {
      s.window_launches = static_cast<long>(win_[1].done - win_[0].done);
      s.window_s = win_[1].t - win_[0].t;
      if (s.window_s > 0) s.during_rate = static_cast<double>(s.window_launches) * work_per_launch() / s.window_s / 1e12;
      s.covered = static_cast<long>(win_[1].done - base_) < enqueued_;
    }
    return s;
  }

 private:
  struct Stamp {
    unsigned long long done = 0;
    double t = 0;
    bool set = false;
  };
  // Plain host reads: no sync, no HIP call.
  // done_ counts launches since the object was made; a train whose first
  // launch has not finished yet still shows the previous train's count.
  Stamp stamp() const { return Stamp{std::max(__atomic_load_n(done_, __ATOMIC_ACQUIRE), base_), now_seconds(), true}; }

  double work_per_launch() const {
    return mfma_ ? static_cast<double>(wgs_) * dev::kLoadWaves * (2.0 * amount_ + 1.0) * dev::kLoadMfmaFlop
                 : static_cast<double>(kHbmScratch) * amount_;
  }

  void enqueue(long n) {
    dev::LoadCtl ctl;
    ctl.cancel = cancel_;
    ctl.done = done_;
    ctl.tickets = tickets_;
    for (long i = 0; i < n; ++i) {
      ctl.ordinal = ordinal_++;
      if (mfma_)
        dev::launch_load_mfma(wgs_, amount_, kLoadSeed, static_cast<float*>(out_), ctl, stream_);
      else
        dev::launch_load_hbm(scratch_, kHbmScratch, amount_, wgs_, static_cast<unsigned long long*>(out_), ctl, stream_);
    }
  }

  // Seconds `n` launches take alone, by hipEvents around them.
  double time_train(long n) {
    HIPCHECK(hipEventRecord(ev_[0], stream_));
    enqueue(n);
    HIPCHECK(hipEventRecord(ev_[1], stream_));
    drain();
    float ms = 0;
    HIPCHECK(hipEventElapsedTime(&ms, ev_[0], ev_[1]));
    return std::max(static_cast<double>(ms) * 1e-3, 1e-7);
  }

  // Seconds per launch over a train of about `train_s`: its length comes
  // from a short probe at the current size.
  double launch_time(double train_s) {
    const double probe = time_train(2) / 2;
    const long n = std::clamp<long>(static_cast<long>(train_s / probe + 0.5), 4, 4096);
    return time_train(n) / static_cast<double>(n);
  }

  // The transports' bounded wait (hip_stream.hpp): a stream error, an abort
  // request or the timeout cancels the train and ends it with an error.
  void drain() { drain(stream_); }
  void drain(hipStream_t st) { wait_stream(st, timeout_, -1, wait_policy_); }
  bool drain_quietly() {
    if (!stream_) return true;
    const double deadline = now_seconds() + std::min(timeout_, 10.0);
    while (hipStreamQuery(stream_) == hipErrorNotReady) {
      if (now_seconds() > deadline) return false;
      std::this_thread::sleep_for(std::chrono::microseconds(100));
    }
    return true;
  }

  std::string kind_;
  bool mfma_;
  int wgs_;
  double timeout_;
  const WaitPolicy wait_policy_{"background load", "", "load stream", /*answers_abort=*/false, nullptr, [this] {
                                  if (cancel_) __atomic_store_n(cancel_, 1u, __ATOMIC_RELEASE);
                                }};
  hipStream_t beside_;  // the stream the transfers run on (null: any stream will do)
  hipStream_t stream_ = nullptr;
  unsigned char* words_ = nullptr;  // pinned: cancel at +0, done at +64
  unsigned int* cancel_ = nullptr;
  unsigned long long* done_ = nullptr;
  unsigned long long* tickets_ = nullptr;
  void* out_ = nullptr;
  void* scratch_ = nullptr;
  hipEvent_t ev_[2] = {nullptr, nullptr};
  uint32_t amount_ = 0;  // reps (mfma) or passes (hbm) per launch
  double launch_s_ = 0;
  double alone_rate_ = 0;
  unsigned long long ordinal_ = 0;  // launches ever enqueued: done_ counts in it
  unsigned long long base_ = 0;     // ordinal_ at start()
  long enqueued_ = 0;
  bool running_ = false;
  Stamp win_[2];
};

}  // namespace

std::unique_ptr<BackgroundLoad> make_background_load(const std::string& kind, int wgs, double timeout_s,
                                                     hipStream_t beside) {
  return std::make_unique<HipBackgroundLoad>(kind, wgs, timeout_s, beside);
}

}  // namespace p2p
