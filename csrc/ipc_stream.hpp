// DeviceStream: the IPC transport's device-initiated stream
// (Transport::stream_setup, device_stream; kernel in stream.hip).  Every rank
// owns one page of rings and flags (stream_layout.hpp), exported over hipIpc
// so peers write into it directly; uncached device memory when the runtime
// allows it.  Like DevicePingPong it shares the transport's stream, bounded
// wait, timeout and exporting allocator, and nothing else.  Which role of a
// call writes where, with which sequence base, and what the stamps it leaves
// mean is stream_plan.hpp (plain host code, under the CPU tests); this class
// turns its (rank, offset) pairs into pointers, launches and copies back.
// GPU translation units only.
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <functional>
#include <string>
#include <vector>

#include "common.hpp"
#include "hip_check.hpp"
#include "ipc_peer_map.hpp"
#include "kernels.hpp"
#include "stream_layout.hpp"
#include "stream_plan.hpp"
#include "transport.hpp"

namespace p2p {

class DeviceStream {
 public:
  using PageFn = std::function<void*(size_t bytes, IpcHandle* handle)>;

  DeviceStream(Bootstrap& boot, hipStream_t stream, std::function<void()> wait, const double& timeout_s, double tick_hz,
               PageFn page)
      : boot_(boot), rank_(boot.rank()), n_(boot.size()), stream_(stream), wait_(std::move(wait)), timeout_(timeout_s),
        tick_hz_(tick_hz), alloc_page_(std::move(page)) {}

  // Collective, every rank with the same arguments.  A second setup with
  // other arguments replaces the first; a failed one releases what it made.
  void setup(int channels, int depth, size_t max_bytes) {
    const StreamLayout want = stream_layout(n_, channels, depth, max_bytes);
    if (ready_ && want.channels == lay_.channels && want.depth == lay_.depth && want.bytes == lay_.bytes) return;
    if (ready_) {
      wait_();
      boot_.barrier();  // nobody writes into a page its owner is about to free
      release();
      boot_.barrier();
    }
    try {
      lay_ = want;
      setup_once();
    } catch (...) {
      release();
      throw;
    }
    ready_ = true;
  }

  void release() {
    close_peers(&peers_, rank_);
    if (page_) (void)hipFree(page_);
    if (scratch_) (void)hipFree(scratch_);
    if (host_) (void)hipHostFree(host_);
    page_ = scratch_ = host_ = nullptr;
    planner_.clear();
    ready_ = false;
  }

  Transport::DeviceStreamTimes stream(int send_to, int recv_from, size_t bytes, int iters, bool check_all) {
    P2P_CHECK(ready_, "stream_setup() first");
    // Who writes where, with which sequence base: stream_plan.hpp.
    const std::vector<StreamRolePlan> plan = planner_.plan(send_to, recv_from, bytes, iters, check_all);
    auto* scratch = static_cast<unsigned char*>(scratch_);
    HIPCHECK(hipMemsetAsync(scratch, 0, StreamScratch::kStatusBytes, stream_));
    auto page_of = [&](int r) {
      return static_cast<unsigned char*>(r == rank_ ? page_ : peers_.ptr[static_cast<size_t>(r)]);
    };
    std::vector<dev::StreamRole> roles;
    for (const StreamRolePlan& p : plan) {
      dev::StreamRole r{};
      r.bytes = p.bytes;
      r.depth = p.depth;
      r.iters = p.iters;
      r.sender = p.sender ? 1 : 0;
      r.check_all = p.check_all ? 1 : 0;
      r.base = p.base;
      r.out_flag = reinterpret_cast<unsigned long long*>(page_of(p.out_rank) + p.out_flag);
      r.in_flag = reinterpret_cast<const unsigned long long*>(static_cast<unsigned char*>(page_) + p.in_flag);
      r.ring = page_of(p.ring_rank) + p.ring;
      r.stamps = reinterpret_cast<unsigned long long*>(scratch + p.stamps);
      r.status = reinterpret_cast<unsigned int*>(scratch + p.status);
      r.timeout_ticks = static_cast<unsigned long long>(std::min(timeout_, 30.0) * tick_hz_);
      roles.push_back(r);
    }
    dev::launch_stream(roles.data(), static_cast<int>(roles.size()), stream_);
    return finish(plan, iters);
  }

 private:
  static_assert(StreamScratch::kMaxRoles == dev::kMaxStreamRoles, "a rank's senders and receivers fit one launch");
  static_assert(StreamLayout::kMaxBytes == dev::kMaxStreamBytes && StreamLayout::kMaxRingBytes == dev::kMaxStreamRingBytes &&
                    StreamLayout::kMaxDepth == dev::kMaxStreamDepth && StreamLayout::kMaxIters == dev::kMaxStreamIters,
                "the layout's limits are the kernel's");

  void setup_once() {
    IpcHandle handle;
    page_ = alloc_page_(lay_.total, &handle);
    // Stream-ordered and waited for with the bounded wait (see DevicePingPong).
    HIPCHECK(hipMemsetAsync(page_, 0, lay_.total, stream_));
    wait_();
    map_peers(boot_, handle, page_, kPeerMapUnchecked, "", 0, "device stream", &peers_);
    planner_.reset(lay_);
    HIPCHECK(hipMalloc(&scratch_, StreamScratch::kBytes));
    HIPCHECK(hipHostMalloc(&host_, StreamScratch::kBytes, hipHostMallocDefault));
    boot_.barrier();
  }

  // Waits for the kernel, reads status and stamps back in one copy; the fold
  // (stream_plan.hpp) checks every role's status words and turns the stamps
  // into the call's times.
  Transport::DeviceStreamTimes finish(const std::vector<StreamRolePlan>& plan, int iters) {
    HIPCHECK(hipGetLastError());
    const size_t used = StreamScratch::used(plan.size(), iters);
    HIPCHECK(hipMemcpyAsync(host_, scratch_, used, hipMemcpyDeviceToHost, stream_));
    wait_();
    const StreamFold f = fold_stream_stamps(plan, host_, used, tick_hz_);
    if (!f.ok()) {
      const StreamRolePlan& r = plan[static_cast<size_t>(f.role)];
      const std::string what = strfmt("device stream %s rank %d", r.sender ? "to" : "from", r.peer);
      if (f.deadline)
        P2P_FATAL(strfmt("rank %d: %s timed out (%s)", rank_, what.c_str(),
                         r.sender ? "the receiver's credit never came" : "the sender's message never came"));
      P2P_FATAL(strfmt("rank %d: %s: %u wrong 16-byte vectors in the messages it checked", rank_, what.c_str(), f.wrong));
    }
    return f.times;
  }

  Bootstrap& boot_;
  const int rank_, n_;
  const hipStream_t stream_;
  const std::function<void()> wait_;
  const double& timeout_;
  const double tick_hz_;
  const PageFn alloc_page_;
  bool ready_ = false;  // setup() completed
  StreamLayout lay_;
  void* page_ = nullptr;
  PeerMap peers_;  // every rank's page
  StreamPlanner planner_{rank_, n_};  // the roles of a call and their sequence bases
  void* scratch_ = nullptr;  // device: a status block per role, then a stamp region per role (StreamScratch)
  void* host_ = nullptr;     // pinned copy of it
};

}  // namespace p2p
