// Background GPU load: what a cell delivers while the GPU is busy, and what
// the transfer costs the compute (--load).
//
// A load is a train of short, fixed-work kernel launches on a stream of its
// own: every launch ends by itself, nothing spins and nothing waits on the
// host.  The train is enqueued up front (load_plan), a `done` word in pinned
// host memory counts the launches that finished, and a `cancel` word makes the
// queued remainder return at once.  The engine brackets a phase's warm-up and
// timed loop with window_begin() / window_end(), two plain host reads, so the
// load's rate inside the window comes from the same counter.
//
// This header is the engine's side (no HIP): the GPU transports hand out the
// implementation (csrc/load.cpp) through Transport::make_load; the CPU
// transports return null.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <string>

namespace p2p {

// --load KIND[:WGS]
struct LoadSpec {
  std::string kind;  // "mfma" | "hbm"; empty: no load
  int wgs = 0;       // workgroups per launch; 0: one per CU
  bool on() const { return !kind.empty(); }
};
// False (with the reason in *err) for an unknown kind or WGS < 1.
bool parse_load_spec(const std::string& text, LoadSpec* spec, std::string* err);

// The train start() enqueues for a phase expected to take `expected_s` when
// one launch alone takes `launch_s`: twice the expected time (the cell slows
// down under the load, and so does the load), at most kMaxLoadLaunches.
constexpr long kMaxLoadLaunches = 16384;
struct LoadPlan {
  long launches = 0;
  double covers_s = 0;  // launches x launch_s
};
inline LoadPlan load_plan(double expected_s, double launch_s) {
  LoadPlan p;
  if (!(launch_s > 0)) return p;
  const double want = std::ceil(2.0 * std::max(expected_s, 0.0) / launch_s);
  p.launches = static_cast<long>(std::clamp(want, 1.0, static_cast<double>(kMaxLoadLaunches)));
  p.covers_s = static_cast<double>(p.launches) * launch_s;
  return p;
}

struct LoadStats {
  long launches = 0;         // enqueued by start()
  long launches_done = 0;    // finished before the cancel cut the train
  long window_launches = 0;  // finished between window_begin() and window_end()
  double window_s = 0;       // host seconds between the two
  double during_rate = 0;    // window_launches x work per launch / window_s, in `unit`
  bool covered = true;       // false: the train ran out before window_end()
};

class BackgroundLoad {
 public:
  virtual ~BackgroundLoad() = default;
  virtual std::string kind() const = 0;
  virtual int wgs() const = 0;
  virtual const char* unit() const = 0;  // "TFLOP/s" | "TB/s"
  // Blocking: sizes one launch to about 250 us and measures the load alone.
  virtual void calibrate() = 0;
  virtual double launch_s() const = 0;    // one launch alone, seconds
  virtual double alone_rate() const = 0;  // a ~20 ms train alone, in unit()
  // Enqueues the train for a phase expected to take `expected_s`; returns at
  // once (the launches run behind it).
  virtual void start(double expected_s) = 0;
  virtual void window_begin() = 0;
  virtual void window_end() = 0;
  // Cancels the queued remainder, waits for the load's stream (bounded by the
  // transport's timeout) and reports.
  virtual LoadStats stop() = 0;
};

}  // namespace p2p
