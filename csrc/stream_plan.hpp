// StreamPlanner and fold_stream_stamps: what one rank of the device-initiated
// stream (ipc_stream.hpp, kernel in stream.hip) launches in a call and what
// the launch's raw stamps mean, as pure functions of the calls the runner
// makes (plain host code, no HIP).
//
// A call carries, per channel, a receiver role and / or a sender role.  The
// planner decides for each of them, over the page layout of
// stream_layout.hpp:
//   * sender to d:      ring and tail in d's page, in the inbox slot of this
//                       rank; the credit comes back into this rank's own
//                       page, on the head line of d;
//   * receiver from s:  ring and tail in this rank's own page, in the inbox
//                       slot of s; the credit goes into s's page, on the head
//                       line of this rank;
//   * the self path:    slot n and line n of the own page, for both roles.
// Flags are 64-bit sequence numbers that only grow: the planner keeps, per
// (slot or line, channel), how many messages this rank published and
// consumed, and a role's `base` is the value its two flag words hold when the
// launch starts, so nothing is ever reset.
//
// Roles are described by (rank, offset) pairs, not pointers; DeviceStream
// turns them into pointers, launches, and copies the scratch (a status block
// per role, then a stamp region per role) back for fold_stream_stamps.  The
// host unit tests run the planned roles of all ranks through a model of the
// kernel's protocol over fake pages and feed the fold scripted stamps
// (tests/host/test_main.cpp).
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <vector>

#include "common.hpp"
#include "stream_layout.hpp"
#include "transport.hpp"

namespace p2p {

// The scratch of one launch.  Every role is a workgroup of its own and may
// run on another XCD, whose L2 is not coherent with the others': two roles
// never share a 256-byte block, neither for their status words nor for their
// stamps.  (With the stamp regions packed, a role's first stamp shared a line
// with its neighbour's last ones and now and then came back as the stamp of
// an earlier launch.)
struct StreamScratch {
  static constexpr int kMaxRoles = 2 * StreamLayout::kMaxChannels;  // one launch (dev::kMaxStreamRoles)
  static constexpr size_t kRoleAlign = 256;
  static constexpr size_t kStatusStride = kRoleAlign / sizeof(unsigned int);  // in status words
  static constexpr size_t kStatusBytes = kRoleAlign * kMaxRoles;
  // Stamps per role, in entries: iters + 2 rounded up to whole blocks.
  static constexpr size_t kStampsPerBlock = kRoleAlign / sizeof(unsigned long long);
  static constexpr size_t stamp_stride(int iters) {
    return (static_cast<size_t>(iters) + 2 + kStampsPerBlock - 1) / kStampsPerBlock * kStampsPerBlock;
  }
  // What a launch of `roles` roles of `iters` messages uses, and the most any launch does.
  static constexpr size_t used(size_t roles, int iters) {
    return kStatusBytes + sizeof(unsigned long long) * stamp_stride(iters) * roles;
  }
  static constexpr size_t kBytes =
      kStatusBytes + sizeof(unsigned long long) * kMaxRoles *
                         ((static_cast<size_t>(StreamLayout::kMaxIters) + 2 + kStampsPerBlock - 1) / kStampsPerBlock * kStampsPerBlock);
};
static_assert(StreamScratch::kBytes == StreamScratch::used(StreamScratch::kMaxRoles, StreamLayout::kMaxIters),
              "the scratch holds the largest launch");

// One role of a launch.  Offsets are in bytes: of a rank's page for the
// flags and the ring, of the scratch for status and stamps.
struct StreamRolePlan {
  int out_rank = -1;    // whose page holds out_flag (sender: the peer's tail; receiver: the peer's head)
  size_t out_flag = 0;
  size_t in_flag = 0;   // in the own page (sender: own head; receiver: own tail)
  int ring_rank = -1;   // whose page holds the ring (sender: the peer's; receiver: the own)
  size_t ring = 0;
  size_t bytes = 0;     // per message, rounded up to 16
  int depth = 0;
  int iters = 0;
  bool sender = false;
  bool check_all = false;
  unsigned long long base = 0;  // messages of this flow before this launch
  size_t status = 0;    // this role's status block in the scratch
  size_t stamps = 0;    // this role's stamp region in the scratch
  int peer = -1;        // send_to / recv_from of the call
  int channel = 0;
};

class StreamPlanner {
 public:
  StreamPlanner(int rank, int nranks) : rank_(rank), n_(nranks) {}

  // What a new setup does: another geometry, pages zeroed, every count at 0.
  void reset(const StreamLayout& layout) {
    P2P_CHECK(layout.n == n_ && layout.channels >= 1, "device stream: the layout is for another rank count");
    lay_ = layout;
    const size_t cells = static_cast<size_t>(n_ + 1) * static_cast<size_t>(lay_.channels);
    sent_.assign(cells, 0);
    recvd_.assign(cells, 0);
  }
  void clear() {
    lay_ = StreamLayout();
    sent_.clear();
    recvd_.clear();
  }
  const StreamLayout& layout() const { return lay_; }

  // The roles of one call in launch order: receivers first (a workgroup that
  // waits for data is resident before the one that produces it is
  // dispatched), then senders, channel-ascending.  Counts the call's messages.
  std::vector<StreamRolePlan> plan(int send_to, int recv_from, size_t bytes, int iters, bool check_all) {
    P2P_CHECK(!sent_.empty(), "stream_setup() first");
    P2P_CHECK(send_to >= -1 && send_to < n_ && recv_from >= -1 && recv_from < n_, "device stream: bad peer");
    P2P_CHECK(send_to >= 0 || recv_from >= 0, "device stream: nothing to send or receive");
    P2P_CHECK((send_to == rank_) == (recv_from == rank_),
              "device stream: the self path sends to and receives from the own rank in one call");
    P2P_CHECK(iters >= 1 && iters <= StreamLayout::kMaxIters, strfmt("device stream: 1..%d messages", StreamLayout::kMaxIters));
    const size_t b = std::max<size_t>(16, (bytes + 15) / 16 * 16);
    P2P_CHECK(b <= lay_.bytes, strfmt("device stream: messages of at most %zu bytes were set up", lay_.bytes));
    const int ch = lay_.channels;
    const size_t stride = StreamScratch::stamp_stride(iters);

    std::vector<StreamRolePlan> roles;
    auto add = [&](bool sender, int c) {
      StreamRolePlan r;
      r.bytes = b;
      r.depth = lay_.depth;
      r.iters = iters;
      r.sender = sender;
      r.check_all = check_all;
      r.channel = c;
      r.status = StreamScratch::kRoleAlign * roles.size();
      r.stamps = StreamScratch::kStatusBytes + sizeof(unsigned long long) * stride * roles.size();
      if (sender) {
        // The ring and tail this rank writes live in the peer's page, in the
        // inbox slot of this rank (slot n on the self path); the credit comes
        // back into this rank's own page, on the line of that destination.
        const bool self = send_to == rank_;
        const int slot = self ? n_ : rank_, line = self ? n_ : send_to;
        r.peer = send_to;
        r.out_rank = r.ring_rank = send_to;
        r.out_flag = lay_.tail(slot, c);
        r.ring = lay_.ring(slot, c);
        r.in_flag = lay_.head(line, c);
        r.base = sent_[static_cast<size_t>(line) * ch + c];
      } else {
        const bool self = recv_from == rank_;
        const int slot = self ? n_ : recv_from, line = self ? n_ : rank_;
        r.peer = recv_from;
        r.out_rank = recv_from;
        r.ring_rank = rank_;
        r.in_flag = lay_.tail(slot, c);
        r.ring = lay_.ring(slot, c);
        r.out_flag = lay_.head(line, c);
        r.base = recvd_[static_cast<size_t>(slot) * ch + c];
      }
      roles.push_back(r);
    };
    if (recv_from >= 0)
      for (int c = 0; c < ch; ++c) add(false, c);
    if (send_to >= 0)
      for (int c = 0; c < ch; ++c) add(true, c);
    for (int c = 0; c < ch; ++c) {
      if (send_to >= 0) sent_[static_cast<size_t>(send_to == rank_ ? n_ : send_to) * ch + c] += static_cast<unsigned long long>(iters);
      if (recv_from >= 0)
        recvd_[static_cast<size_t>(recv_from == rank_ ? n_ : recv_from) * ch + c] += static_cast<unsigned long long>(iters);
    }
    return roles;
  }

  // Messages published to / consumed from each (peer slot, channel); slot n: the self path.
  const std::vector<unsigned long long>& sent() const { return sent_; }
  const std::vector<unsigned long long>& recvd() const { return recvd_; }

 private:
  int rank_, n_;
  StreamLayout lay_;
  std::vector<unsigned long long> sent_, recvd_;
};

// What fold_stream_stamps made of a launch's scratch.  `role` >= 0 names the
// first role (in launch order) whose status block reports a failure: a spin
// that hit its deadline, or `wrong` 16-byte vectors among those it checked.
// The times are then those of the roles before it.
struct StreamFold {
  Transport::DeviceStreamTimes times;
  int role = -1;
  bool deadline = false;
  unsigned int wrong = 0;
  bool ok() const { return role < 0; }
};

// `scratch` is the host copy of the launch's status blocks and stamp regions
// (StreamScratch::used(roles.size(), iters) bytes of it are read, no more).
//   send_span_s      earliest senders' stamps[0] to the latest stamps[iters + 1];
//   gap_us           channel 0's sender (the first sender role): stamps[i + 1] - stamps[i], iters values;
//   recv_span_s      earliest receivers' stamps[0] to the latest stamps[iters - 1];
//   checked_vectors  per receiver role iters x (every vector | first and last).
inline StreamFold fold_stream_stamps(const std::vector<StreamRolePlan>& roles, const void* scratch, size_t scratch_bytes,
                                     double tick_hz) {
  StreamFold f;
  Transport::DeviceStreamTimes& out = f.times;
  const auto* bytes = static_cast<const unsigned char*>(scratch);
  unsigned long long s_first = ~0ull, s_last = 0, r_first = ~0ull, r_last = 0;
  for (size_t k = 0; k < roles.size(); ++k) {
    const StreamRolePlan& r = roles[k];
    const size_t iters = static_cast<size_t>(r.iters);
    P2P_CHECK(r.iters >= 1 && r.status + 2 * sizeof(unsigned int) <= scratch_bytes &&
                  r.stamps + sizeof(unsigned long long) * (iters + 2) <= scratch_bytes,
              "device stream: a role's status or stamps lie outside the scratch");
    unsigned int rs[2];
    std::memcpy(rs, bytes + r.status, sizeof(rs));
    if ((rs[0] & 1u) || rs[1]) {
      f.role = static_cast<int>(k);
      f.deadline = (rs[0] & 1u) != 0;
      f.wrong = rs[1];
      out.wrong_vectors = rs[1];
      return f;
    }
    auto s = [&](size_t i) {
      unsigned long long v;
      std::memcpy(&v, bytes + r.stamps + sizeof(v) * i, sizeof(v));
      return v;
    };
    if (r.sender) {
      if (!out.sent)  // the first sender role is channel 0
        for (size_t i = 0; i < iters; ++i) out.gap_us.push_back(static_cast<double>(s(i + 1) - s(i)) / tick_hz * 1e6);
      out.sent = true;
      s_first = std::min(s_first, s(0));
      s_last = std::max(s_last, s(iters + 1));
    } else {
      out.received = true;
      r_first = std::min(r_first, s(0));
      r_last = std::max(r_last, s(iters - 1));
      const unsigned long long nvec = r.bytes / 16;
      out.checked_vectors += static_cast<uint64_t>(iters) * (r.check_all ? nvec : std::min<unsigned long long>(2, nvec));
    }
  }
  if (out.sent) out.send_span_s = static_cast<double>(s_last - s_first) / tick_hz;
  if (out.received) out.recv_span_s = static_cast<double>(r_last - r_first) / tick_hz;
  return f;
}

}  // namespace p2p
