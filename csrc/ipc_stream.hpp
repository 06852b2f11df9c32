// DeviceStream: the IPC transport's device-initiated stream
// (Transport::stream_setup, device_stream; kernel in stream.hip).  Every rank
// owns one page of rings and flags (stream_layout.hpp), exported over hipIpc
// so peers write into it directly; uncached device memory when the runtime
// allows it.  Like DevicePingPong it shares the transport's stream, bounded
// wait, timeout and exporting allocator, and nothing else.  GPU translation
// units only.
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
    sent_.clear();
    recvd_.clear();
    ready_ = false;
  }

  Transport::DeviceStreamTimes stream(int send_to, int recv_from, size_t bytes, int iters, bool check_all) {
    P2P_CHECK(ready_, "stream_setup() first");
    P2P_CHECK(send_to >= -1 && send_to < n_ && recv_from >= -1 && recv_from < n_, "device stream: bad peer");
    P2P_CHECK(send_to >= 0 || recv_from >= 0, "device stream: nothing to send or receive");
    P2P_CHECK((send_to == rank_) == (recv_from == rank_),
              "device stream: the self path sends to and receives from the own rank in one call");
    P2P_CHECK(iters >= 1 && iters <= dev::kMaxStreamIters, strfmt("device stream: 1..%d messages", dev::kMaxStreamIters));
    const size_t b = std::max<size_t>(16, (bytes + 15) / 16 * 16);
    P2P_CHECK(b <= lay_.bytes, strfmt("device stream: messages of at most %zu bytes were set up", lay_.bytes));
    const int ch = lay_.channels;
    const size_t stride = stamp_stride(iters);
    auto* status = static_cast<unsigned int*>(scratch_);
    auto* stamps = reinterpret_cast<unsigned long long*>(static_cast<unsigned char*>(scratch_) + kStatusBytes);
    HIPCHECK(hipMemsetAsync(status, 0, kStatusBytes, stream_));

    std::vector<dev::StreamRole> roles;
    auto add = [&](bool sender, int c) {
      dev::StreamRole r{};
      r.bytes = b;
      r.depth = lay_.depth;
      r.iters = iters;
      r.sender = sender ? 1 : 0;
      r.check_all = check_all ? 1 : 0;
      r.stamps = stamps + roles.size() * stride;
      r.status = status + kStatusStride * roles.size();
      r.timeout_ticks = static_cast<unsigned long long>(std::min(timeout_, 30.0) * tick_hz_);
      if (sender) {
        // The ring and tail this rank writes live in the peer's page, in the
        // inbox slot of this rank (slot n on the self path); the credit comes
        // back into this rank's own page, on the line of that destination.
        const bool self = send_to == rank_;
        auto* peer = static_cast<unsigned char*>(self ? page_ : peers_.ptr[static_cast<size_t>(send_to)]);
        const int slot = self ? n_ : rank_, line = self ? n_ : send_to;
        r.out_flag = reinterpret_cast<unsigned long long*>(peer + lay_.tail(slot, c));
        r.ring = peer + lay_.ring(slot, c);
        r.in_flag = reinterpret_cast<const unsigned long long*>(static_cast<unsigned char*>(page_) + lay_.head(line, c));
        r.base = sent_[static_cast<size_t>(line) * ch + c];
      } else {
        const bool self = recv_from == rank_;
        auto* peer = static_cast<unsigned char*>(self ? page_ : peers_.ptr[static_cast<size_t>(recv_from)]);
        const int slot = self ? n_ : recv_from, line = self ? n_ : rank_;
        r.in_flag = reinterpret_cast<const unsigned long long*>(static_cast<unsigned char*>(page_) + lay_.tail(slot, c));
        r.ring = static_cast<unsigned char*>(page_) + lay_.ring(slot, c);
        r.out_flag = reinterpret_cast<unsigned long long*>(peer + lay_.head(line, c));
        r.base = recvd_[static_cast<size_t>(slot) * ch + c];
      }
      roles.push_back(r);
    };
    // Receivers first: a workgroup that waits for data is resident before the
    // one that produces it is dispatched.
    if (recv_from >= 0)
      for (int c = 0; c < ch; ++c) add(false, c);
    if (send_to >= 0)
      for (int c = 0; c < ch; ++c) add(true, c);
    dev::launch_stream(roles.data(), static_cast<int>(roles.size()), stream_);
    for (int c = 0; c < ch; ++c) {
      if (send_to >= 0) sent_[static_cast<size_t>(send_to == rank_ ? n_ : send_to) * ch + c] += static_cast<unsigned long long>(iters);
      if (recv_from >= 0)
        recvd_[static_cast<size_t>(recv_from == rank_ ? n_ : recv_from) * ch + c] += static_cast<unsigned long long>(iters);
    }
    return finish(roles, send_to, recv_from, iters, check_all);
  }

 private:
  // Every role is a workgroup of its own and may run on another XCD, whose
  // L2 is not coherent with the others': two roles never share a 256-byte
  // block, neither for their status words nor for their stamps.  (With the
  // stamp regions packed, a role's first stamp shared a line with its
  // neighbour's last ones and now and then came back as the stamp of an
  // earlier launch.)
  static constexpr size_t kRoleAlign = 256;
  static constexpr size_t kStatusStride = kRoleAlign / sizeof(unsigned int);  // in status words
  static constexpr size_t kStatusBytes = kRoleAlign * dev::kMaxStreamRoles;
  // Stamps per role, in entries: iters + 2 rounded up to whole blocks.
  static constexpr size_t kStampsPerBlock = kRoleAlign / sizeof(unsigned long long);
  static size_t stamp_stride(int iters) {
    return (static_cast<size_t>(iters) + 2 + kStampsPerBlock - 1) / kStampsPerBlock * kStampsPerBlock;
  }
  static constexpr size_t kScratch =
      kStatusBytes + sizeof(unsigned long long) * dev::kMaxStreamRoles *
                         ((static_cast<size_t>(dev::kMaxStreamIters) + 2 + kStampsPerBlock - 1) / kStampsPerBlock * kStampsPerBlock);
  static_assert(2 * StreamLayout::kMaxChannels <= dev::kMaxStreamRoles, "a rank's senders and receivers fit one launch");
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
    const size_t cells = static_cast<size_t>(n_ + 1) * static_cast<size_t>(lay_.channels);
    sent_.assign(cells, 0);
    recvd_.assign(cells, 0);
    HIPCHECK(hipMalloc(&scratch_, kScratch));
    HIPCHECK(hipHostMalloc(&host_, kScratch, hipHostMallocDefault));
    boot_.barrier();
  }

  // Waits for the kernel, reads status and stamps back in one copy, checks
  // every role's status words and folds the stamps into the call's times.
  Transport::DeviceStreamTimes finish(const std::vector<dev::StreamRole>& roles, int send_to, int recv_from, int iters,
                                      bool check_all) {
    HIPCHECK(hipGetLastError());
    const size_t stride = stamp_stride(iters);
    const size_t used = kStatusBytes + sizeof(unsigned long long) * stride * roles.size();
    HIPCHECK(hipMemcpyAsync(host_, scratch_, used, hipMemcpyDeviceToHost, stream_));
    wait_();
    const auto* st = static_cast<const unsigned int*>(host_);
    const auto* stamps = reinterpret_cast<const unsigned long long*>(static_cast<const unsigned char*>(host_) + kStatusBytes);
    Transport::DeviceStreamTimes out;
    unsigned long long s_first = ~0ull, s_last = 0, r_first = ~0ull, r_last = 0;
    for (size_t k = 0; k < roles.size(); ++k) {
      const dev::StreamRole& r = roles[k];
      const int peer = r.sender ? send_to : recv_from;
      const std::string what = strfmt("device stream %s rank %d", r.sender ? "to" : "from", peer);
      const unsigned int* rs = st + kStatusStride * k;
      if (rs[0] & 1u)
        P2P_FATAL(strfmt("rank %d: %s timed out (%s)", rank_, what.c_str(),
                         r.sender ? "the receiver's credit never came" : "the sender's message never came"));
      if (rs[1])
        P2P_FATAL(strfmt("rank %d: %s: %u wrong 16-byte vectors in the messages it checked", rank_, what.c_str(), rs[1]));
      const unsigned long long* s = stamps + k * stride;
      if (r.sender) {
        if (!out.sent)  // the first sender role is channel 0
          for (int i = 0; i < iters; ++i)
            out.gap_us.push_back(static_cast<double>(s[static_cast<size_t>(i) + 1] - s[static_cast<size_t>(i)]) / tick_hz_ * 1e6);
        out.sent = true;
        s_first = std::min(s_first, s[0]);
        s_last = std::max(s_last, s[static_cast<size_t>(iters) + 1]);
      } else {
        out.received = true;
        r_first = std::min(r_first, s[0]);
        r_last = std::max(r_last, s[static_cast<size_t>(iters) - 1]);
        const unsigned long long nvec = r.bytes / 16;
        out.checked_vectors += static_cast<uint64_t>(iters) * (check_all ? nvec : std::min<unsigned long long>(2, nvec));
      }
    }
    if (out.sent) out.send_span_s = static_cast<double>(s_last - s_first) / tick_hz_;
    if (out.received) out.recv_span_s = static_cast<double>(r_last - r_first) / tick_hz_;
    return out;
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
  // Sequence bases per (peer slot, channel): messages published to / consumed from each rank (slot n: the self path).
  std::vector<unsigned long long> sent_, recvd_;
  void* scratch_ = nullptr;  // device: a status block per role, then a stamp region per role (stamp_stride)
  void* host_ = nullptr;     // pinned copy of it
};

}  // namespace p2p
