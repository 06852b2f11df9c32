// IpcTransport: one-sided point-to-point over xGMI without RCCL.
//
// Every rank exports its send buffer with hipIpcGetMemHandle when the
// buffers are created (register_buffers, collective); every peer maps it
// with hipIpcOpenMemHandle.  A receive is then a *pull*: the receiver's GPU
// reads the sender's send buffer directly over the xGMI link into its own
// receive buffer.  A send moves nothing (the receiver does the work), which
// is valid for this benchmark because a phase's payload is written once
// (fill + sync + barrier) before any timed receive reads it.
//
// Data movers (TransportOptions::ipc_engine):
//   kernel — one launch of the gfx950 multi-source copy kernel per group
//            (kernels.hip: all receives of the group in one grid, workgroups
//            split by size, 4 x 16 B remote loads in flight per lane);
//   sdma   — hipMemcpyAsync per receive, forked onto one stream per receive
//            slot so the copies of an all-pairs group run concurrently.
//   push   — two-sided rendezvous with remote writes: a receive posts a
//            "ready" flag into the sender's signal page, the sender's stream
//            waits for it (one-wave signal kernel), the multi-copy kernel
//            writes the payload straight into the receiver's slot over xGMI,
//            and a second signal kernel releases it and raises "done" on the
//            receiver, whose stream waits for that.  Real send/recv semantics
//            (a send never overwrites a slot the receiver has not posted) on
//            the direction xGMI handles best (remote stores).  Which flags,
//            values and launches: PushPlanner (push_plan.hpp), for push and
//            relay alike; this file maps them to addresses and launches.
//   relay  — push, multi-path: each message is split into stripes
//            (routing.hpp plan_routes), one over the direct link, written by
//            the sender, and one per two-hop path s -> k -> d through a GPU k
//            whose links s->k and k->d carry no direct flow of the group.
//            k's copy kernel loads its stripe from s's hipIpc-mapped send
//            buffer and stores it into d's mapped receive slot, so the bytes
//            cross s->k and k->d and never touch k's HBM.  Every writer
//            (sender or relay) waits for the receiver's ready flag and raises
//            its done flag, exactly as in push.  The runner posts every group
//            on every rank and passes the group's global flows
//            (Transport::group_flows), so a relay knows what to move.  A
//            single pair of an 8-GPU node can then use up to 7 links; RCCL's
//            ncclSend/ncclRecv (and the reference's NCCL p2p) only ever use
//            the direct one.
//
// Why it exists: it is the hand-written CDNA4 data plane to compare RCCL's
// ncclSend/ncclRecv against on the same links, and, because IPC mappings
// also work between processes on ONE GPU, it lets the complete multi-rank GPU
// engine (events, kernels, verification, every schedule) run on a single
// MI355X, where RCCL refuses duplicate-GPU ranks.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "bootstrap.hpp"
#include "common.hpp"
#include "hip_check.hpp"
#include "hip_stream.hpp"
#include "ipc_blocks.hpp"
#include "ipc_peer_map.hpp"
#include "ipc_pingpong.hpp"
#include "ipc_stream.hpp"
#include "kernels.hpp"
#include "push_plan.hpp"
#include "routing.hpp"
#include "transport.hpp"
#include "units.hpp"

namespace p2p {
namespace {

constexpr const char* kWho = "ipc transport";  // map_peers: "<who> is intra-node only: ..."

class IpcTransport final : public GpuTransport {
 public:
  IpcTransport(Bootstrap& boot, const TransportOptions& opt)
      : GpuTransport(boot, opt, /*keep_graphs=*/false,
                     "ipc transport: no HIP device visible",
                     "check failed: device_ < ndev: rank %d wants GPU %d but only %d are visible"),
        boot_(boot), engine_(opt.ipc_engine), relay_(engine_ == "relay"), push_(engine_ == "push" || relay_),
        tick_hz_(dev::wall_clock_hz(device_)),
        blocks_(
            pool_cap_from_env(), size_fix_from_env(),
            [](void** q, size_t size) { return error_text(hipMalloc(q, size)); }, [](void* p) { (void)hipFree(p); },
            [this](void* p, IpcHandle* handle) {
              hipError_t e = hipIpcGetMemHandle(reinterpret_cast<hipIpcMemHandle_t*>(handle), p);
              if (e == hipSuccess && inject_refusals_ > 0) {  // test hook: P2P_INJECT_EXPORT_REFUSALS=<n>
                --inject_refusals_;
                e = hipErrorInvalidValue;
              }
              return error_text(e);
            },
            [this](size_t blocks, size_t size) {
              std::fprintf(stderr, "p2p_matrix: rank %d: hipIpcGetMemHandle refused %zu fresh %zu-byte block(s); reallocated\n",
                           rank_, blocks, size);
            }),
        ping_(boot, stream_, [this] { sync(); }, timeout_, tick_hz_,
              [this](size_t bytes, IpcHandle* handle) { return signal_page(bytes, handle); }),
        dstream_(boot, stream_, [this] { sync(); }, timeout_, tick_hz_,
                 [this](size_t bytes, IpcHandle* handle) { return signal_page(bytes, handle); }) {
    P2P_CHECK(engine_ == "kernel" || engine_ == "sdma" || engine_ == "push" || relay_,
              "ipc engine must be 'kernel', 'sdma', 'push' or 'relay'");
    static_assert(kPushMaxSignals == dev::kMaxSignals, "the planner cuts signals to what one launch carries");
    hipDeviceProp_t prop;
    HIPCHECK(hipGetDeviceProperties(&prop, device_));
    desc_ = strfmt("hip:%d %s (%s, %d CUs) ipc-%s", device_, prop.name, prop.gcnArchName, prop.multiProcessorCount,
                   engine_.c_str());
    P2P_CHECK(tick_hz_ > 0, "device reports no wall clock rate");
    wait_policy_.noun = "ipc stream";
    if (const char* ir = std::getenv("P2P_INJECT_EXPORT_REFUSALS")) inject_refusals_ = std::atoi(ir);
    if (push_) {
      plan_ = std::make_unique<PushPlanner>(rank_, n_, relay_, relay_ ? route_options_from_env() : RouteOptions());
      setup_sync_pages();
    }
  }

  ~IpcTransport() override {
    (void)hipStreamSynchronize(stream_);
    if (relay_ && std::getenv("P2P_RELAY_STATS"))
      std::fprintf(stderr, "p2p_matrix: rank %d relayed %llu bytes in %llu stripes\n", rank_, relayed_bytes_,
                   relayed_stripes_);
    for (auto& r : regs_) close_registration(r);
    regs_.clear();
    ping_.release();
    dstream_.release();
    release_sync_pages();
    blocks_.drain();
    destroy_graphs();
    for (auto s : side_) (void)hipStreamDestroy(s);
    for (auto e : side_done_) (void)hipEventDestroy(e);
    if (fork_) (void)hipEventDestroy(fork_);
    destroy_stream_objects();
  }

  std::string name() const override { return "ipc"; }

  // ---- memory: exported blocks and their pool (ipc_blocks.hpp) ----
  bool mem_info(size_t* free_b, size_t* total_b) override {
    if (hipMemGetInfo(free_b, total_b) != hipSuccess) return false;
    *free_b += blocks_.pooled_bytes();  // pooled blocks are handed back on demand
    return true;
  }
  void* alloc(size_t bytes) override { return blocks_.alloc(bytes); }
  void release(void* p) override { blocks_.release(p); }

  // Buffer sets are registered collectively in the same order on every rank,
  // so "the same set" on a peer is the one with the same position.  A receive
  // into one of a set's receive slots pulls from that set's send buffer on the
  // peer (at the message's offset).  Push / relay also map every peer's
  // receive arena: one export per set, slot i at base + i * stride.
  void register_buffers(const BufferSet& set) override {
    if (debug_)
      std::fprintf(stderr, "ipc rank %d: register send %zu B, arena %d x %zu B\n", rank_, set.send_bytes, set.nslots,
                   set.stride);
    Registration reg;
    reg.send = set.send;
    reg.send_bytes = set.send_bytes;
    reg.recv = set.recv;
    reg.stride = set.stride;
    reg.slot_bytes = set.slot_bytes;
    reg.nslots = set.nslots;
    map_peers(boot_, blocks_.handle_of(set.send), set.send, set.send_bytes,
              "ipc transport: send buffers differ in size across ranks", 0, kWho, &reg.peer_send);
    for (int r = 0; debug_ && r < n_; ++r)
      if (r != rank_) std::fprintf(stderr, "ipc rank %d: mapped send buffer of rank %d\n", rank_, r);
    if (push_) {
      // The sender (or a relay) writes into the receiver's slot: map every
      // peer's receive arena.  Slot counts may differ between ranks.
      map_peers(boot_, blocks_.handle_of(set.recv), set.recv, set.stride, "ipc transport: receive slots differ in size",
                static_cast<uint32_t>(set.nslots), kWho, &reg.peer_recv);
      for (int r = 0; debug_ && r < n_; ++r)
        std::fprintf(stderr, "ipc rank %d: mapped receive arena of rank %d\n", rank_, r);
    }
    regs_.push_back(std::move(reg));
    boot_.barrier();
  }

  void unregister_buffers(void* send) override {
    auto it = std::find_if(regs_.begin(), regs_.end(), [&](const Registration& r) { return r.send == send; });
    if (it == regs_.end()) return;
    sync();
    // Every rank stops moving data before any mapping goes, and every rank
    // has closed its mappings of a buffer before its owner releases it.
    boot_.barrier();
    close_registration(*it);
    regs_.erase(it);
    boot_.barrier();
  }

  // ---- data plane ----
  void group_begin() override {
    P2P_CHECK(!in_group_, "nested group");
    in_group_ = true;
    ops_.clear();
    checked_ops_.clear();
    if (plan_) plan_->group_begin();
  }

  bool wants_group_flows() const override { return relay_; }

  // Relay engine: plans every flow of the group (identically on every rank)
  // and posts this rank's part of each: the direct stripe as its sender, the
  // stripes routed through it as a relay, the flags as the receiver.  The
  // endpoints' own send / recv calls for these flows are then checks only.
  void group_flows(const void* set_send, const std::vector<GroupFlow>& flows, size_t bytes) override {
    if (!relay_) return;
    P2P_CHECK(in_group_, "group_flows outside a group");
    const Registration* reg = nullptr;
    for (const auto& r : regs_)
      if (r.send == set_send) reg = &r;
    P2P_CHECK(reg && bytes <= reg->slot_bytes, "ipc relay: flows of an unregistered buffer set");
    for (const auto& f : flows)
      P2P_CHECK(f.src == f.dst || f.src_offset + bytes <= reg->send_bytes, "ipc relay: message outside the send buffer");
    for (const PushCopy& c : plan_->group_flows(flows, bytes, discarding())) {
      push_copy(*reg, c);
      if (c.src != rank_) {
        relayed_bytes_ += c.bytes;
        ++relayed_stripes_;
      }
    }
  }

  void send(const void* p, size_t bytes, int peer) override { send_to_slot(p, bytes, peer, 0); }
  void send_to_slot(const void* p, size_t bytes, int peer, int slot) override {
    P2P_CHECK(peer >= 0 && peer < n_, "bad peer");
    const Registration* reg = nullptr;
    for (const auto& r : regs_)
      if (p >= r.send && static_cast<const char*>(p) + bytes <= static_cast<const char*>(r.send) + r.send_bytes &&
          bytes <= r.slot_bytes)
        reg = &r;
    P2P_CHECK(reg, "ipc transport sends only from a registered send buffer");
    if (!push_) return;  // nothing to move: the receiver pulls
    // Injected skip fault: the rendezvous runs, the payload stays behind.
    PushCopy c;
    const size_t src_offset = static_cast<size_t>(static_cast<const char*>(p) - static_cast<const char*>(reg->send));
    if (plan_->send(src_offset, bytes, peer, slot, discarding(), &c)) push_copy(*reg, c);
    if (!in_group_) flush();
  }
  void recv(void* p, size_t bytes, int peer) override { recv_from(p, bytes, peer, 0); }
  void recv_from(void* p, size_t bytes, int peer, size_t src_offset) override {
    post_recv(p, bytes, peer, src_offset, nullptr, 0);
  }

  // ---- inline check (transport.hpp): the pull engine's own kernel compares
  // each word it loads with the stream the sender filled (kernels.hpp
  // multi_copy_checked_kernel); one device record per delivery.
  bool supports_inline_check() const override { return engine_ == "kernel"; }
  void inline_check_begin(size_t nrecords) override {
    P2P_CHECK(supports_inline_check(), "ipc transport: the inline check needs --ipc-engine kernel");
    checks_.records_begin(nrecords, stream_, [this] { sync(); });
  }
  void recv_checked(void* p, size_t bytes, int peer, size_t src_offset, uint64_t seed, size_t record_index) override {
    P2P_CHECK(supports_inline_check(), "ipc transport: the inline check needs --ipc-engine kernel");
    // A replayed graph would write the record it captured, whatever it delivers.
    P2P_CHECK(!capturing_, "ipc transport: no inline check inside a graph capture");
    P2P_CHECK(record_index < checks_.records(), "ipc transport: inline_check_begin() first, with enough records");
    post_recv(p, bytes, peer, src_offset, &seed, record_index);
  }
  std::vector<InlineCheck> inline_check_results() override {
    return checks_.records_read(stream_, [this] { sync(); });
  }

  void group_end() override {
    P2P_CHECK(in_group_, "group_end without group_begin");
    in_group_ = false;
    P2P_CHECK(!plan_ || plan_->group_complete(), "ipc relay: group_flows named a flow this rank did not post");
    flush();
  }

  // Push / relay: the flag values are baked into each launch, so a replay
  // would wait for flags that were already consumed; no graphs there.
  bool supports_graphs() const override { return engine_ == "kernel"; }

  bool supports_device_pingpong() const override { return true; }
  void pingpong_setup() override { ping_.setup(); }
  std::vector<double> device_pingpong(int peer, size_t bytes, int iters) override {
    return ping_.pingpong(peer, bytes, iters);
  }
  std::vector<double> device_ring_token(int pred, int succ, bool leader, size_t bytes, int laps) override {
    return ping_.ring_token(pred, succ, leader, bytes, laps);
  }

  bool supports_device_stream() const override { return true; }
  void stream_setup(int channels, int depth, size_t max_bytes) override { dstream_.setup(channels, depth, max_bytes); }
  DeviceStreamTimes device_stream(int send_to, int recv_from, size_t bytes, int iters, bool check_all) override {
    return dstream_.stream(send_to, recv_from, bytes, iters, check_all);
  }

  // A finished stream still has to pass the rendezvous status word.
  void sync() override {
    wait_stream(stream_, timeout_, rank_, wait_policy_);
    if (sig_status_ && (*sig_status_ & 1u))
      P2P_FATAL(strfmt("rank %d: ipc push rendezvous timed out (a peer never posted its side)", rank_));
  }

 private:
  struct Registration {
    void* send = nullptr;
    size_t send_bytes = 0;
    void* recv = nullptr;  // receive arena: slot i at recv + i * stride
    size_t stride = 0;
    size_t slot_bytes = 0;
    int nslots = 0;
    PeerMap peer_send;  // mapped send buffer of every rank (own one for self)
    PeerMap peer_recv;  // push / relay: mapped receive arena of every rank, and its slot count
  };

  static const char* error_text(hipError_t e) {
    if (e == hipSuccess) return nullptr;
    (void)hipGetLastError();
    return hipGetErrorString(e);
  }
  // P2P_IPC_POOL: 32 GiB by default -- lower it when many ranks share one GPU.
  static size_t pool_cap_from_env() {
    const char* pc = std::getenv("P2P_IPC_POOL");
    if (!pc) return size_t{32} << 30;
    return std::strcmp(pc, "0") ? parse_size(pc) : 0;
  }
  // HIP 7.0's hipIpcOpenMemHandle never returns for a block whose size mod
  // 4 GiB is 2 GiB or more (scripts/ipc_open_probe.hip: 2 and 3.75 and 7 GiB
  // hang, 2 GiB - 2 MiB, 4, 4 GiB + 2 MiB and 5 GiB open in 0.1 s; HIP 7.2
  // opens them all).  Exported blocks are sized around it on such runtimes.
  static bool size_fix_from_env() {
    if (const char* sf = std::getenv("P2P_IPC_SIZE_FIX")) return std::atoi(sf) != 0;
    int hip_rt = 0;
    if (hipRuntimeGetVersion(&hip_rt) != hipSuccess) hip_rt = 0;
    return hip_rt < 70200000;
  }
  // A page for flags a wave spins on, exportable (the blocks' refusal retry).
  void* signal_page(size_t bytes, IpcHandle* handle) {
    return blocks_.exportable(bytes, handle, [](void** q, size_t size) { return error_text(dev::alloc_signal_page(q, size)); });
  }

  void close_registration(Registration& reg) {
    close_peers(&reg.peer_send, rank_);
    close_peers(&reg.peer_recv, rank_);
  }

  // Slot index of receive pointer p in reg's arena, -1 if it is not one.
  static int slot_of(const Registration& reg, const void* p) {
    const char* base = static_cast<const char*>(reg.recv);
    const char* q = static_cast<const char*>(p);
    if (q < base || reg.stride == 0) return -1;
    const size_t off = static_cast<size_t>(q - base);
    if (off % reg.stride || off / reg.stride >= static_cast<size_t>(reg.nslots)) return -1;
    return static_cast<int>(off / reg.stride);
  }
  char* remote_slot_ptr(const Registration& reg, int peer, int slot) const {
    P2P_CHECK(static_cast<size_t>(peer) < reg.peer_recv.ptr.size(), "ipc push: receive arenas are not mapped");
    const int nslots = static_cast<int>(reg.peer_recv.value[static_cast<size_t>(peer)]);
    P2P_CHECK(slot >= 0 && slot < nslots, strfmt("bad remote slot %d (rank %d has %d)", slot, peer, nslots));
    return static_cast<char*>(reg.peer_recv.ptr[static_cast<size_t>(peer)]) + reg.stride * static_cast<size_t>(slot);
  }

  // A receive; with `seed`, one the kernel checks against that stream into
  // record `record_index`.
  void post_recv(void* p, size_t bytes, int peer, size_t src_offset, const uint64_t* seed, size_t record_index) {
    P2P_CHECK(peer >= 0 && peer < n_, "bad peer");
    const Registration* reg = nullptr;
    int slot = -1;
    for (const auto& r : regs_) {
      const int s = slot_of(r, p);
      if (s >= 0 && bytes <= r.slot_bytes) {
        reg = &r;
        slot = s;
      }
    }
    P2P_CHECK(reg, "ipc transport receives only into a registered receive slot");
    if (push_) {
      plan_->recv(peer, slot);
      if (!in_group_) flush();
      return;
    }
    P2P_CHECK(src_offset + bytes <= reg->send_bytes, "ipc transport: receive beyond the peer's send buffer");
    // Injected skip fault: the pull is not issued (and a checked one leaves
    // its record at 0 wrong words: the check after timing catches it).
    if (!discarding()) {
      const dev::CopyOp op{static_cast<const char*>(reg->peer_send.ptr[static_cast<size_t>(peer)]) + src_offset, p, bytes,
                           peer != rank_};
      if (seed) {
        dev::CheckedCopyOp c;
        static_cast<dev::CopyOp&>(c) = op;
        c.seed = *seed;
        c.record = checks_.record(record_index);
        checked_ops_.push_back(c);
      } else {
        ops_.push_back(op);
      }
    }
    if (!in_group_) flush();
  }

  void flush() {
    if (push_) {
      flush_push();
      return;
    }
    // Kernel engine: the checked kernel when the group has checked receives
    // (the runner posts a group either all checked or all plain; plain ones
    // next to them go in the plain kernel), the plain kernel otherwise.
    if (!checked_ops_.empty()) {
      dev::launch_multi_copy_checked(checked_ops_.data(), static_cast<int>(checked_ops_.size()), stream_);
      checked_ops_.clear();
    }
    if (ops_.empty()) return;
    if (engine_ == "kernel") {
      dev::launch_multi_copy(ops_.data(), static_cast<int>(ops_.size()), stream_);
    } else if (ops_.size() == 1) {
      HIPCHECK(hipMemcpyAsync(ops_[0].dst, ops_[0].src, ops_[0].bytes, hipMemcpyDeviceToDevice, stream_));
    } else {
      // Fork: the receives round-robin over a few side streams so the copy
      // engines overlap, then join back into the main stream.  A small pool
      // (P2P_SDMA_STREAMS, default 4) rather than a stream per receive: more
      // streams than the process's hardware queues only share queues, and
      // every extra queue is one more for the GPU's scheduler to map.
      const size_t k = std::min(ops_.size(), sdma_streams());
      ensure_side_streams(k);
      HIPCHECK(hipEventRecord(fork_, stream_));
      for (size_t j = 0; j < k; ++j) HIPCHECK(hipStreamWaitEvent(side_[j], fork_, 0));
      for (size_t i = 0; i < ops_.size(); ++i)
        HIPCHECK(hipMemcpyAsync(ops_[i].dst, ops_[i].src, ops_[i].bytes, hipMemcpyDeviceToDevice, side_[i % k]));
      for (size_t j = 0; j < k; ++j) {
        HIPCHECK(hipEventRecord(side_done_[j], side_[j]));
        HIPCHECK(hipStreamWaitEvent(stream_, side_done_[j], 0));
      }
    }
    ops_.clear();
  }

  static size_t sdma_streams() {
    static const size_t k = [] {
      const char* e = std::getenv("P2P_SDMA_STREAMS");
      const int v = e ? std::atoi(e) : 4;
      return static_cast<size_t>(std::max(1, std::min(64, v)));
    }();
    return k;
  }

  void ensure_side_streams(size_t n) {
    if (!fork_) HIPCHECK(hipEventCreateWithFlags(&fork_, hipEventDisableTiming));
    while (side_.size() < n) {
      hipStream_t s;
      HIPCHECK(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
      side_.push_back(s);
      hipEvent_t e;
      HIPCHECK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
      side_done_.push_back(e);
    }
  }

  // A stripe the planner gave this rank, as a copy between mapped buffers.
  void push_copy(const Registration& reg, const PushCopy& c) {
    const char* src = static_cast<const char*>(reg.peer_send.ptr[static_cast<size_t>(c.src)]) + c.src_offset + c.offset;
    char* dst = remote_slot_ptr(reg, c.dst, c.slot) + c.offset;
    ops_.push_back({src, dst, c.bytes, c.src != rank_ || c.dst != rank_});
  }

  // Push group (push_plan.hpp): readies out / readies in, the copies, then
  // done out / done in.
  void flush_push() {
    const PushFlush f = plan_->flush();
    if (debug_) {
      std::string msg = strfmt("[ipc %d] group %ld sends-to:", rank_, groups_);
      for (const auto& q : f.pre_waits) msg += strfmt(" %d", q.peer);
      msg += " recvs-from:";
      for (const auto& p : f.pre_posts) msg += strfmt(" %d", p.peer);
      msg += " ready_posted:";
      for (auto v : plan_->ready_posted()) msg += strfmt(" %llu", v);
      msg += " ready_seen:";
      for (auto v : plan_->ready_seen()) msg += strfmt(" %llu", v);
      std::fprintf(stderr, "%s ops %zu\n", msg.c_str(), ops_.size());
    }
    ++groups_;
    for (const PushPiece& piece : f.pre) launch_signals(piece);
    if (!ops_.empty()) dev::launch_multi_copy(ops_.data(), static_cast<int>(ops_.size()), stream_);
    for (const PushPiece& piece : f.post) launch_signals(piece);
    ops_.clear();
  }

  // Signal page line of kind k (ready / done) that rank `from` writes.
  unsigned long long* sync_line(void* page, int kind, int from) const {
    return reinterpret_cast<unsigned long long*>(static_cast<unsigned char*>(page) +
                                                 kSyncLine * (static_cast<size_t>(kind) * n_ + static_cast<size_t>(from)));
  }
  // A post goes to this rank's line in the peer's page, a wait reads the
  // peer's line in this rank's page.
  void launch_signals(const PushPiece& piece) {
    if (piece.posts.empty() && piece.waits.empty()) return;
    P2P_CHECK(piece.posts.size() <= static_cast<size_t>(dev::kMaxSignals) &&
                  piece.waits.size() <= static_cast<size_t>(dev::kMaxSignals),
              "ipc push: a signal piece larger than one launch");
    dev::SignalArgs a{};
    for (const PushFlag& f : piece.posts) {
      a.post_flag[a.nposts] = sync_line(sync_peer_.ptr[static_cast<size_t>(f.peer)], f.kind, rank_);
      a.post_value[a.nposts++] = f.value;
    }
    for (const PushFlag& f : piece.waits) {
      a.wait_flag[a.nwaits] = sync_line(sync_page_, f.kind, f.peer);
      a.wait_value[a.nwaits++] = f.value;
    }
    a.release_first = piece.release_first ? 1 : 0;
    a.status = sig_status_;
    a.timeout_ticks = static_cast<unsigned long long>(timeout_ * tick_hz_);
    dev::launch_signal(a, stream_);
  }

  // Collective (constructor): one signal page per rank, 2 x n flag lines
  // (ready / done from every peer), exported to every peer.  A setup that
  // fails half way releases what it made (the constructor throws, so the
  // destructor does not run).
  void setup_sync_pages() {
    try {
      const size_t bytes = kSyncLine * 2 * static_cast<size_t>(n_);
      IpcHandle handle;
      sync_page_ = signal_page(bytes, &handle);
      HIPCHECK(hipMemsetAsync(sync_page_, 0, bytes, stream_));
      sync();  // bounded (see DevicePingPong::setup_once)
      HIPCHECK(hipHostMalloc(&sig_status_, 64, hipHostMallocMapped));
      *sig_status_ = 0;
      map_peers(boot_, handle, sync_page_, kPeerMapUnchecked, "", 0, kWho, &sync_peer_);
      boot_.barrier();
    } catch (...) {
      release_sync_pages();
      throw;
    }
  }

  void release_sync_pages() {
    close_peers(&sync_peer_, rank_);
    if (sync_page_) (void)hipFree(sync_page_);
    if (sig_status_) (void)hipHostFree(sig_status_);
    sync_page_ = nullptr;
    sig_status_ = nullptr;
  }

  Bootstrap& boot_;
  const std::string engine_;
  const bool relay_;  // multi-path push (engine "relay")
  const bool push_;   // rendezvous + remote writes (engines "push" and "relay")
  const double tick_hz_;
  WaitPolicy wait_policy_;  // sync(): "ipc stream did not finish ..."
  bool debug_ = std::getenv("P2P_IPC_DEBUG") != nullptr;  // per-group flag bookkeeping on stderr

  // Exported memory and what is mapped of the peers'.
  int inject_refusals_ = 0;
  IpcBlocks blocks_;
  std::vector<Registration> regs_;
  DevicePingPong ping_;
  DeviceStream dstream_;

  // The open group, for every data mover.
  bool in_group_ = false;
  std::vector<dev::CopyOp> ops_;
  long groups_ = 0;

  // Pull kernel: receives checked as they are copied.
  std::vector<dev::CheckedCopyOp> checked_ops_;

  // SDMA: the fork / join pool.
  std::vector<hipStream_t> side_;
  std::vector<hipEvent_t> side_done_;
  hipEvent_t fork_ = nullptr;

  // Push / relay: signal pages, the planner, and what this rank moved as a relay (P2P_RELAY_STATS).
  static constexpr size_t kSyncLine = 128;
  void* sync_page_ = nullptr;
  PeerMap sync_peer_;
  unsigned int* sig_status_ = nullptr;  // host-mapped; bit 0 = a signal wait timed out
  std::unique_ptr<PushPlanner> plan_;   // flag counters and every post / wait decision (push_plan.hpp)
  unsigned long long relayed_bytes_ = 0, relayed_stripes_ = 0;
};

}  // namespace

std::unique_ptr<Transport> make_ipc_transport(Bootstrap& boot, const TransportOptions& opt) {
  return std::make_unique<IpcTransport>(boot, opt);
}

}  // namespace p2p
