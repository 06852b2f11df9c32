// DevicePingPong: the IPC transport's device-initiated ping-pong and ring
// token (Transport::pingpong_setup, device_pingpong, device_ring_token;
// kernels in pingpong.hip).  Every rank owns one page of n + 1 inbox slots
// (slot r = messages from rank r, slot n = replies of the self path),
// exported over hipIpc so peers write into it directly.  Uncached device
// memory when the runtime allows it, so the spinning wave reads HBM, not a
// stale line.  It shares the transport's stream, bounded wait, timeout and
// exporting allocator, and nothing else.  GPU translation units only.
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

namespace p2p {

class DevicePingPong {
 public:
  // An exportable, uncached page of `bytes` with its handle (IpcBlocks::exportable).
  using PageFn = std::function<void*(size_t bytes, IpcHandle* handle)>;

  // `wait`: the transport's bounded sync(); `timeout_s`: its live timeout.
  DevicePingPong(Bootstrap& boot, hipStream_t stream, std::function<void()> wait, const double& timeout_s,
                 double tick_hz, PageFn page)
      : boot_(boot), rank_(boot.rank()), n_(boot.size()), stream_(stream), wait_(std::move(wait)), timeout_(timeout_s),
        tick_hz_(tick_hz), alloc_page_(std::move(page)) {}

  // Collective.  A setup that failed half way (the bounded wait timed out or
  // was aborted) releases what it made: no page_ is left behind that a later
  // call would take for a finished setup.
  void setup() {
    if (ready_) return;  // same state on every rank: they all set up together
    try {
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
    sent_.clear();
    recvd_.clear();
    ready_ = false;
  }

  std::vector<double> pingpong(int peer, size_t bytes, int iters) {
    P2P_CHECK(peer >= 0 && peer < n_, "bad peer");
    const bool self = peer == rank_;
    dev::PingRole a = role(bytes, iters);
    a.leader = (self || rank_ < peer) ? 1 : 0;
    if (self) {
      // Both waves on this GPU: a writes slot `rank`, the reply wave slot n.
      a.base = a.in_base = sent_[static_cast<size_t>(rank_)];
      a.out_flag = reinterpret_cast<unsigned long long*>(slot(page_, rank_));
      a.out_payload = slot(page_, rank_) + kHeader;
      a.in_flag = reinterpret_cast<const unsigned long long*>(slot(page_, n_));
      a.in_payload = slot(page_, n_) + kHeader;
      dev::PingRole b = a;  // the reply wave: mirror image through slot n
      b.leader = 0;
      b.out_flag = const_cast<unsigned long long*>(a.in_flag);
      b.out_payload = const_cast<unsigned char*>(a.in_payload);
      b.in_flag = a.out_flag;
      b.in_payload = a.out_payload;
      dev::launch_pingpong(a, &b, stream_);
      sent_[static_cast<size_t>(rank_)] += static_cast<unsigned long long>(iters);
    } else {
      set_links(&a, peer, peer);
      dev::launch_pingpong(a, nullptr, stream_);
      sent_[static_cast<size_t>(peer)] += static_cast<unsigned long long>(iters);
      recvd_[static_cast<size_t>(peer)] += static_cast<unsigned long long>(iters);
    }
    return finish(a.leader != 0, iters, 2.0, strfmt("device ping-pong with rank %d", peer));
  }

  std::vector<double> ring_token(int pred, int succ, bool leader, size_t bytes, int laps) {
    P2P_CHECK(pred >= 0 && pred < n_ && succ >= 0 && succ < n_ && pred != rank_ && succ != rank_,
              "ring token: predecessor and successor must be other ranks");
    dev::PingRole a = role(bytes, laps);
    a.leader = leader ? 1 : 0;
    set_links(&a, pred, succ);
    dev::launch_pingpong(a, nullptr, stream_);
    sent_[static_cast<size_t>(succ)] += static_cast<unsigned long long>(laps);
    recvd_[static_cast<size_t>(pred)] += static_cast<unsigned long long>(laps);
    return finish(leader, laps, 1.0, strfmt("ring token (from %d, to %d)", pred, succ));
  }

 private:
  static constexpr size_t kHeader = 256;  // flag + padding (own cache lines)
  static constexpr size_t kMaxBytes = 64u << 10;
  static constexpr size_t kSlot = kHeader + kMaxBytes;
  static constexpr int kMaxIters = 100000;
  static constexpr size_t kScratch = sizeof(unsigned long long) * (kMaxIters + 1) + 64;

  void setup_once() {
    const size_t bytes = kSlot * static_cast<size_t>(n_ + 1);
    IpcHandle handle;
    page_ = alloc_page_(bytes, &handle);
    // Stream-ordered and waited for with the bounded wait: a device-wide
    // synchronize would also wait, unbounded, for any other session's work.
    HIPCHECK(hipMemsetAsync(page_, 0, bytes, stream_));
    wait_();
    map_peers(boot_, handle, page_, kPeerMapUnchecked, "", 0, "device ping-pong", &peers_);
    sent_.assign(static_cast<size_t>(n_), 0);
    recvd_.assign(static_cast<size_t>(n_), 0);
    HIPCHECK(hipMalloc(&scratch_, kScratch));
    HIPCHECK(hipHostMalloc(&host_, kScratch, hipHostMallocDefault));
    boot_.barrier();
  }

  unsigned char* slot(void* page, int k) const { return static_cast<unsigned char*>(page) + kSlot * static_cast<size_t>(k); }
  // A role with its timing buffers and bounds set; links and bases follow.
  dev::PingRole role(size_t bytes, int iters) {
    P2P_CHECK(ready_, "pingpong_setup() first");
    P2P_CHECK(iters >= 1 && iters <= kMaxIters, strfmt("device ping-pong: 1..%d iterations", kMaxIters));
    P2P_CHECK(bytes <= kMaxBytes, strfmt("device ping-pong payload is at most %zu bytes", kMaxBytes));
    auto* stamps = static_cast<unsigned long long*>(scratch_);
    auto* status = reinterpret_cast<unsigned int*>(stamps + kMaxIters + 1);
    HIPCHECK(hipMemsetAsync(status, 0, 2 * sizeof(unsigned int), stream_));
    dev::PingRole a{};
    a.bytes = std::max<size_t>(16, (bytes + 15) / 16 * 16);
    a.iters = iters;
    a.stamps = stamps;
    a.status = status;
    a.timeout_ticks = static_cast<unsigned long long>(std::min(timeout_, 30.0) * tick_hz_);
    return a;
  }
  // Writes go to `to`'s inbox slot for this rank; waits read the slot `from`
  // writes here.  Sequence bases: what this rank has written to `to` and
  // read from `from` so far (flags are monotonic, never reset).
  void set_links(dev::PingRole* a, int from, int to) {
    unsigned char* out = slot(peers_.ptr[static_cast<size_t>(to)], rank_);
    unsigned char* in = slot(page_, from);
    a->base = sent_[static_cast<size_t>(to)];
    a->in_base = recvd_[static_cast<size_t>(from)];
    a->out_flag = reinterpret_cast<unsigned long long*>(out);
    a->out_payload = out + kHeader;
    a->in_flag = reinterpret_cast<const unsigned long long*>(in);
    a->in_payload = in + kHeader;
  }
  // Waits for the kernel, checks its status words, and returns the leader's
  // per-iteration times in microseconds divided by `div` (empty elsewhere).
  std::vector<double> finish(bool leader, int iters, double div, const std::string& what) {
    HIPCHECK(hipGetLastError());
    HIPCHECK(hipMemcpyAsync(host_, scratch_, kScratch, hipMemcpyDeviceToHost, stream_));
    wait_();
    const auto* host = static_cast<const unsigned long long*>(host_);
    const auto* st = reinterpret_cast<const unsigned int*>(host + kMaxIters + 1);
    if (st[0] & 1u) P2P_FATAL(strfmt("rank %d: %s timed out (partner kernel never answered)", rank_, what.c_str()));
    if (st[1]) P2P_FATAL(strfmt("rank %d: %s: %u payloads arrived before their data", rank_, what.c_str(), st[1]));
    std::vector<double> us;
    if (leader)
      for (int i = 0; i < iters; ++i)
        us.push_back(static_cast<double>(host[static_cast<size_t>(i) + 1] - host[static_cast<size_t>(i)]) / tick_hz_ * 1e6 /
                     div);
    return us;
  }

  Bootstrap& boot_;
  const int rank_, n_;
  const hipStream_t stream_;
  const std::function<void()> wait_;
  const double& timeout_;
  const double tick_hz_;
  const PageFn alloc_page_;
  bool ready_ = false;  // setup() completed
  void* page_ = nullptr;
  PeerMap peers_;  // every rank's page
  std::vector<unsigned long long> sent_, recvd_;  // ping messages written to / read from each rank
  void* scratch_ = nullptr;  // device: stamps[kMaxIters + 1], status[2]
  void* host_ = nullptr;     // pinned copy of it
};

}  // namespace p2p
