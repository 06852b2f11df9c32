// PushPlanner: what one rank of the IPC push / relay engines does in a group,
// as a pure function of the calls the runner makes (plain host code, no HIP).
//
// The rendezvous (transport_ipc.cpp has the data plane):
//   * every rank owns one flag per peer and kind: `ready` (kPushReady), which
//     a receiver raises at a writer, and `done` (kPushDone), which a writer
//     raises at a receiver.  Flags only grow: the k-th group in which rank a
//     posts a kind to rank b carries the value k, and b's k-th wait for it
//     names k, so nothing is ever reset;
//   * a group is, on the stream: the pre-signal (ready out to every writer,
//     then ready in from every receiver), this rank's copies, the post-signal
//     (a release fence, done out to every receiver, then done in from every
//     writer);
//   * a writer is the sender of a message (push, and the direct stripe of
//     relay) or the relay rank of a two-hop stripe (routing.hpp).
//
// The planner holds the four per-peer counters, the peers of the group so
// far and the flows group_flows() already posted for the endpoints.  It
// decides which stripes this rank writes and which flags it posts and waits
// for, with which values, in which pieces; IpcTransport turns (peer, kind)
// into flag addresses, stripes into pointers, and launches.  The host unit
// tests drive the same class under the real runner and check the programs it
// yields against a model of the contract (tests/host/test_main.cpp).
#pragma once

#include <algorithm>
#include <array>
#include <cstddef>
#include <utility>
#include <vector>

#include "routing.hpp"
#include "transport.hpp"

namespace p2p {

// Flags one signal launch can carry per direction (dev::kMaxSignals).
constexpr int kPushMaxSignals = 16;

constexpr int kPushReady = 0, kPushDone = 1;

// A post writes `value` into the line (kind, this rank) of `peer`'s signal
// page; a wait reads the line (kind, peer) of this rank's own page.
struct PushFlag {
  int peer = -1;
  int kind = kPushReady;
  unsigned long long value = 0;
};

// One signal launch: every post is issued before the launch waits.
struct PushPiece {
  std::vector<PushFlag> posts, waits;
  bool release_first = false;
};

// A stripe this rank writes: `bytes` from `src_offset + offset` of rank
// src's send buffer to `offset` of receive slot `slot` on rank dst.
struct PushCopy {
  int src = -1;
  size_t src_offset = 0;
  int dst = -1;
  int slot = 0;
  size_t offset = 0;
  size_t bytes = 0;
};

struct PushFlush {
  // One entry per message, in posting order.
  std::vector<PushFlag> pre_posts, pre_waits, post_posts, post_waits;
  // The same, one entry per flag (the highest value), cut into launches.
  std::vector<PushPiece> pre, post;
};

class PushPlanner {
 public:
  PushPlanner(int rank, int nranks, bool relay, const RouteOptions& route = RouteOptions(),
              int max_signals = kPushMaxSignals)
      : rank_(rank), n_(nranks), relay_(relay), route_(route), max_signals_(std::max(1, max_signals)) {
    for (auto* v : {&ready_posted_, &ready_seen_, &done_posted_, &done_seen_}) v->assign(static_cast<size_t>(n_), 0);
  }

  bool relay() const { return relay_; }

  void group_begin() { covered_.clear(); }
  // False when group_flows named a flow of this rank that it never posted.
  bool group_complete() const { return covered_.empty(); }

  // Relay: every flow of the group, identical on every rank.  Returns the
  // stripes this rank writes (none while discarding: the rendezvous runs, the
  // payload stays behind) and notes its part of the rendezvous: the direct
  // stripe as the sender, the stripes routed through it as a relay, the
  // flags as the receiver.  The endpoints' own send / recv calls for these
  // flows are then checks only (take_covered).  Self flows are left to them.
  std::vector<PushCopy> group_flows(const std::vector<Transport::GroupFlow>& flows, size_t bytes, bool discarding) {
    std::vector<PushCopy> out;
    if (!relay_) return out;
    std::vector<std::pair<int, int>> pairs;
    pairs.reserve(flows.size());
    for (const auto& f : flows) pairs.emplace_back(f.src, f.dst);
    const auto plan = plan_routes(n_, pairs, bytes, route_);
    for (size_t i = 0; i < flows.size(); ++i) {
      const Transport::GroupFlow& f = flows[i];
      if (f.src == f.dst) continue;
      for (const Stripe& st : plan[i]) {
        const int writer = st.via < 0 ? f.src : st.via;
        if (rank_ == writer) {
          if (!discarding) out.push_back({f.src, f.src_offset, f.dst, f.slot, st.offset, st.bytes});
          sends_.push_back(f.dst);  // wait for its ready, raise its done
        }
        if (rank_ == f.dst) recvs_.push_back(writer);  // post ready, wait for done
      }
      if (rank_ == f.src || rank_ == f.dst) covered_.push_back({f.src, f.dst, f.slot});
    }
    return out;
  }

  // A send of this rank from `src_offset` of its send buffer.  True when it
  // has a copy to make (*copy); an injected skip fault and a flow that
  // group_flows posted have none.
  bool send(size_t src_offset, size_t bytes, int peer, int slot, bool discarding, PushCopy* copy) {
    if (take_covered(rank_, peer, slot)) return false;
    if (peer != rank_) sends_.push_back(peer);
    if (discarding) return false;
    *copy = {rank_, src_offset, peer, slot, 0, bytes};
    return true;
  }

  // A receive of this rank into its slot `slot`; a self receive is the self
  // send's copy.
  void recv(int peer, int slot) {
    if (take_covered(peer, rank_, slot)) return;
    if (peer != rank_) recvs_.push_back(peer);
  }

  // The group's signals; the copies noted so far go between `pre` and `post`.
  PushFlush flush() {
    PushFlush f;
    for (int p : recvs_) f.pre_posts.push_back({p, kPushReady, ++ready_posted_[static_cast<size_t>(p)]});
    for (int q : sends_) f.pre_waits.push_back({q, kPushReady, ++ready_seen_[static_cast<size_t>(q)]});
    for (int q : sends_) f.post_posts.push_back({q, kPushDone, ++done_posted_[static_cast<size_t>(q)]});
    for (int p : recvs_) f.post_waits.push_back({p, kPushDone, ++done_seen_[static_cast<size_t>(p)]});
    f.pre = pieces(f.pre_posts, f.pre_waits, max_signals_, false);
    f.post = pieces(f.post_posts, f.post_waits, max_signals_, true);
    sends_.clear();
    recvs_.clear();
    return f;
  }

  // Several messages to one peer in a group share its flag: one entry per
  // flag with the highest value (lanes storing to one address at once would
  // leave an arbitrary one of the values), in first-use order.
  static std::vector<PushFlag> dedupe(const std::vector<PushFlag>& in) {
    std::vector<PushFlag> out;
    for (const PushFlag& f : in) {
      auto it = std::find_if(out.begin(), out.end(), [&](const PushFlag& o) { return o.peer == f.peer && o.kind == f.kind; });
      if (it == out.end())
        out.push_back(f);
      else
        it->value = std::max(it->value, f.value);
    }
    return out;
  }

  // Launches of at most `max_signals` posts and `max_signals` waits: the
  // posts fill pieces first, so none of them is held back by a wait.  After
  // the copies (`after_copies`) every piece with a done post releases first,
  // and so does the last one (the group's usual single launch).
  static std::vector<PushPiece> pieces(const std::vector<PushFlag>& posts, const std::vector<PushFlag>& waits,
                                       int max_signals, bool after_copies) {
    const size_t cap = static_cast<size_t>(std::max(1, max_signals));
    std::vector<PushPiece> out;
    PushPiece cur;
    for (const PushFlag& f : dedupe(posts)) {
      if (cur.posts.size() == cap) out.push_back(std::move(cur)), cur = PushPiece();
      cur.posts.push_back(f);
    }
    for (const PushFlag& f : dedupe(waits)) {
      if (cur.waits.size() == cap) out.push_back(std::move(cur)), cur = PushPiece();
      cur.waits.push_back(f);
    }
    if (!cur.posts.empty() || !cur.waits.empty()) out.push_back(std::move(cur));
    for (size_t i = 0; i < out.size(); ++i) {
      const bool done_post = std::any_of(out[i].posts.begin(), out[i].posts.end(),
                                         [](const PushFlag& f) { return f.kind == kPushDone; });
      out[i].release_first = after_copies && (done_post || i + 1 == out.size());
    }
    return out;
  }

  // Peers of the group so far and the counters (debug output, tests).
  const std::vector<int>& sends() const { return sends_; }
  const std::vector<int>& recvs() const { return recvs_; }
  const std::vector<unsigned long long>& ready_posted() const { return ready_posted_; }
  const std::vector<unsigned long long>& ready_seen() const { return ready_seen_; }
  const std::vector<unsigned long long>& done_posted() const { return done_posted_; }
  const std::vector<unsigned long long>& done_seen() const { return done_seen_; }

 private:
  // A flow (src, dst, slot) that group_flows already posted for this rank;
  // consumed by the endpoint's matching send / recv call.
  bool take_covered(int src, int dst, int slot) {
    const std::array<int, 3> key{src, dst, slot};
    auto it = std::find(covered_.begin(), covered_.end(), key);
    if (it == covered_.end()) return false;
    covered_.erase(it);
    return true;
  }

  int rank_, n_;
  bool relay_;
  RouteOptions route_;
  int max_signals_;
  std::vector<unsigned long long> ready_posted_, ready_seen_, done_posted_, done_seen_;
  std::vector<int> sends_, recvs_;           // peers this rank writes to / receives from in the group
  std::vector<std::array<int, 3>> covered_;  // relay: (src, dst, slot) posted by group_flows
};

}  // namespace p2p
