// HostTransport: the CPU data plane (host memory + a full TCP mesh).
//
// Exists so the complete engine (schedules, grouped send/recv semantics,
// timing, verification, reports) runs and is tested without a GPU, and as the
// native counterpart of the gloo plumbing config in BASELINE.json
// ("2-rank CPU/gloo send/recv of a 4 KiB buffer").  A group is executed at
// group_end() by a non-blocking progress loop over all of its ops, so the
// symmetric send+recv groups of bi-directional / ring / all-pairs phases
// cannot deadlock on socket buffers — the same guarantee ncclGroupEnd gives.
#include <arpa/inet.h>
#include <netdb.h>
#include <netinet/in.h>
#include <netinet/tcp.h>
#include <poll.h>
#include <sys/socket.h>
#include <unistd.h>

#include <algorithm>
#include <cerrno>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <thread>
#include <vector>

#include "bootstrap.hpp"
#include "common.hpp"
#include "transport.hpp"

namespace p2p {

void host_fill(void* p, size_t bytes, uint64_t seed) {
  auto* b = static_cast<uint8_t*>(p);
  size_t nw = bytes / 4;
  for (size_t i = 0; i < nw; ++i) {
    const uint32_t w = prng_word(seed, i);
    std::memcpy(b + 4 * i, &w, 4);  // any alignment
  }
  for (size_t i = nw * 4; i < bytes; ++i) b[i] = prng_byte(seed, i);
}

VerifyResult host_verify(const void* p, size_t bytes, uint64_t seed) {
  VerifyResult r;
  const auto* b = static_cast<const uint8_t*>(p);
  size_t nw = bytes / 4;
  for (size_t i = 0; i < nw; ++i) {
    uint32_t got;
    std::memcpy(&got, b + 4 * i, 4);
    r.checksum += got;
    if (got != prng_word(seed, i)) {
      if (!r.mismatches) r.first_bad = 4 * i;
      ++r.mismatches;
    }
  }
  size_t tail = bytes - nw * 4;
  if (tail) {
    uint32_t got = 0, want = prng_word(seed, nw);
    std::memcpy(&got, b + 4 * nw, tail);
    uint32_t mask = (1u << (8 * tail)) - 1u;
    r.checksum += got;
    if ((got & mask) != (want & mask)) {
      if (!r.mismatches) r.first_bad = 4 * nw;
      ++r.mismatches;
    }
  }
  return r;
}

void host_reduce(void* out, const void* const* operands, int k, size_t bytes, ReduceType t) {
  P2P_CHECK(k >= 1 && bytes % 4 == 0, "host_reduce: at least one operand, bytes a multiple of 4");
  std::vector<uint32_t> w(static_cast<size_t>(k));
  for (size_t i = 0; i < bytes; i += 4) {
    for (int j = 0; j < k; ++j) std::memcpy(&w[static_cast<size_t>(j)], static_cast<const char*>(operands[j]) + i, 4);
    const uint32_t r = reduce_word(w.data(), k, t);
    std::memcpy(static_cast<char*>(out) + i, &r, 4);
  }
}

void host_fill_operand(void* p, size_t bytes, uint64_t seed, ReduceType t) {
  P2P_CHECK(bytes % 4 == 0, "host_fill_operand: bytes must be a multiple of 4");
  for (size_t i = 0; i < bytes / 4; ++i) {
    const uint32_t w = operand_word(prng_word(seed, i), t);
    std::memcpy(static_cast<char*>(p) + 4 * i, &w, 4);
  }
}

VerifyResult host_verify_reduced(const void* p, size_t bytes, const uint64_t* seeds, int nseeds, ReduceType t) {
  P2P_CHECK(nseeds >= 1 && bytes % 4 == 0, "host_verify_reduced: at least one seed, bytes a multiple of 4");
  VerifyResult r;
  std::vector<uint32_t> w(static_cast<size_t>(nseeds));
  for (size_t i = 0; i < bytes / 4; ++i) {
    for (int j = 0; j < nseeds; ++j) w[static_cast<size_t>(j)] = operand_word(prng_word(seeds[j], i), t);
    uint32_t got;
    std::memcpy(&got, static_cast<const char*>(p) + 4 * i, 4);
    r.checksum += got;
    if (got != reduce_word(w.data(), nseeds, t)) {
      if (!r.mismatches) r.first_bad = 4 * i;
      ++r.mismatches;
    }
  }
  return r;
}

// ---- gated sum over rows (reduce_gate_op.hpp) ----
void host_gated_reduce(void* out, const void* const* operands, int k, size_t bytes, const void* gate, size_t row_elems) {
  P2P_CHECK(k >= 1 && k <= kGateSlots, "host_gated_reduce: 1..8 operands");
  P2P_CHECK(gate_rows(bytes, row_elems) > 0, "host_gated_reduce: whole rows of row_elems bf16, row_elems a multiple of 512");
  const size_t row_bytes = 2 * row_elems;
  uint32_t w[kGateSlots];
  float g[kGateSlots];
  for (size_t i = 0; i < bytes; i += 4) {
    if (i % row_bytes == 0) {
      uint32_t entry[4];
      std::memcpy(entry, static_cast<const char*>(gate) + i / row_bytes * kGateEntryBytes, sizeof(entry));
      for (int j = 0; j < k; ++j) g[j] = gate_value(entry, j);
    }
    for (int j = 0; j < k; ++j) std::memcpy(&w[j], static_cast<const char*>(operands[j]) + i, 4);
    const uint32_t r = gated_reduce_word(w, g, k);
    std::memcpy(static_cast<char*>(out) + i, &r, 4);
  }
}

void host_fill_gate(void* p, size_t rows, uint64_t seed) {
  for (size_t i = 0; i < 4 * rows; ++i) {
    const uint32_t w = gate_word(prng_word(seed, i));
    std::memcpy(static_cast<char*>(p) + 4 * i, &w, 4);
  }
}

VerifyResult host_verify_gated_reduced(const void* p, size_t bytes, const uint64_t* seeds, int nseeds, uint64_t gate_seed,
                                       size_t row_elems) {
  P2P_CHECK(nseeds >= 1 && nseeds <= kGateSlots, "host_verify_gated_reduced: 1..8 operand seeds");
  P2P_CHECK(gate_rows(bytes, row_elems) > 0, "host_verify_gated_reduced: whole rows of row_elems bf16, row_elems a multiple of 512");
  const size_t row_words = row_elems / 2;
  VerifyResult r;
  uint32_t w[kGateSlots];
  float g[kGateSlots];
  for (size_t i = 0; i < bytes / 4; ++i) {
    if (i % row_words == 0) {
      uint32_t entry[4];
      for (size_t j = 0; j < 4; ++j) entry[j] = gate_word(prng_word(gate_seed, i / row_words * 4 + j));
      for (int j = 0; j < nseeds; ++j) g[j] = gate_value(entry, j);
    }
    for (int j = 0; j < nseeds; ++j) w[j] = operand_word(prng_word(seeds[j], i), ReduceType::Bf16);
    uint32_t got;
    std::memcpy(&got, static_cast<const char*>(p) + 4 * i, 4);
    r.checksum += got;
    if (got != gated_reduce_word(w, g, nseeds)) {
      if (!r.mismatches) r.first_bad = 4 * i;
      ++r.mismatches;
    }
  }
  return r;
}

// ---- block-scaled wire formats (wire_op.hpp): tile by tile, block by block ----
namespace {

// Calls fn(block's payload offset, block's element bytes offset, scale byte offset) for every block.
template <typename Fn>
void for_each_wire_block(size_t n, WireFormat f, Fn fn) {
  const uint32_t eb = wire_block_elem_bytes(f);
  size_t wire_at = 0;
  for (size_t tile = 0; tile * kWireTilePayload < n; ++tile) {
    const uint32_t nb = static_cast<uint32_t>(std::min<size_t>(kWireTileBlocks, (n - tile * kWireTilePayload) / kWireBlockBytes));
    for (uint32_t b = 0; b < nb; ++b)
      fn(tile * kWireTilePayload + b * kWireBlockBytes, wire_at + b * eb, wire_at + wire_tile_scale_offset(nb, f) + b);
    wire_at += wire_tile_bytes(nb, f);
  }
}

void check_wire(size_t n, WireFormat f, const char* who) {
  P2P_CHECK(wire_format_valid(f), std::string(who) + ": the format is " + kWireFormatList);
  P2P_CHECK(n % kWireBlockBytes == 0, std::string(who) + ": the payload is a multiple of 64 bytes (blocks of 32 bf16)");
}

// Block `block` (counted from the payload's start) of operand stream `seed`.
void wire_operand_block(uint64_t seed, uint64_t block, uint16_t* x) {
  for (uint32_t j = 0; j < 16; ++j) {
    const uint64_t i = block * 16 + j;
    const uint32_t w = wire_operand_word(prng_word(seed, i), i);
    x[2 * j] = static_cast<uint16_t>(w);
    x[2 * j + 1] = static_cast<uint16_t>(w >> 16);
  }
}

}  // namespace

void host_wire_pack(void* wire, const void* payload, size_t n, WireFormat f) {
  check_wire(n, f, "host_wire_pack");
  std::memset(wire, 0, wire_bytes(n, f));  // the padding
  auto* out = static_cast<uint8_t*>(wire);
  for_each_wire_block(n, f, [&](size_t at, size_t elems, size_t scale) {
    uint16_t x[kWireBlockElems];
    std::memcpy(x, static_cast<const char*>(payload) + at, sizeof(x));
    wire_pack_block(x, out + elems, out + scale, f);
  });
}

void host_wire_unpack(void* payload, const void* wire, size_t n, WireFormat f) {
  check_wire(n, f, "host_wire_unpack");
  const auto* in = static_cast<const uint8_t*>(wire);
  for_each_wire_block(n, f, [&](size_t at, size_t elems, size_t scale) {
    uint16_t x[kWireBlockElems];
    wire_unpack_block(in + elems, in[scale], x, f);
    std::memcpy(static_cast<char*>(payload) + at, x, sizeof(x));
  });
}

void host_fill_packed(void* wire, size_t n, uint64_t seed, WireFormat f) {
  check_wire(n, f, "host_fill_packed");
  std::memset(wire, 0, wire_bytes(n, f));
  auto* out = static_cast<uint8_t*>(wire);
  for_each_wire_block(n, f, [&](size_t at, size_t elems, size_t scale) {
    uint16_t x[kWireBlockElems];
    wire_operand_block(seed, at / kWireBlockBytes, x);
    wire_pack_block(x, out + elems, out + scale, f);
  });
}

VerifyResult host_verify_unpacked(const void* p, size_t n, uint64_t seed, WireFormat f) {
  check_wire(n, f, "host_verify_unpacked");
  VerifyResult r;
  for (size_t at = 0; at < n; at += kWireBlockBytes) {
    uint16_t x[kWireBlockElems], want[kWireBlockElems];
    uint8_t elems[32], scale;
    wire_operand_block(seed, at / kWireBlockBytes, x);
    wire_pack_block(x, elems, &scale, f);
    wire_unpack_block(elems, scale, want, f);
    for (uint32_t j = 0; j < 16; ++j) {
      uint32_t got;
      std::memcpy(&got, static_cast<const char*>(p) + at + 4 * j, 4);
      r.checksum += got;
      if (got != (want[2 * j] | static_cast<uint32_t>(want[2 * j + 1]) << 16)) {
        if (!r.mismatches) r.first_bad = at + 4 * j;
        ++r.mismatches;
      }
    }
  }
  return r;
}

// ---- sum of wire images (wire_reduce_op.hpp) ----
void host_wire_reduce(void* out, const void* const* images, int k, size_t n, WireFormat f, bool own_bf16) {
  check_wire(n, f, "host_wire_reduce");
  P2P_CHECK(k >= 1 && k <= kMaxWireReduceSrcs, "host_wire_reduce: 1..8 images");
  for_each_wire_block(n, f, [&](size_t at, size_t elems, size_t scale) {
    uint32_t w[kMaxWireReduceSrcs][16];
    for (int j = 0; j < k; ++j) {
      const auto* in = static_cast<const uint8_t*>(images[j]);
      uint16_t x[kWireBlockElems];
      if (own_bf16 && j == 0) std::memcpy(x, in + at, sizeof(x));  // the own shard: bf16 as it is
      else wire_unpack_block(in + elems, in[scale], x, f);
      for (uint32_t i = 0; i < 16; ++i) w[j][i] = x[2 * i] | static_cast<uint32_t>(x[2 * i + 1]) << 16;
    }
    for (uint32_t i = 0; i < 16; ++i) {
      uint32_t col[kMaxWireReduceSrcs];
      for (int j = 0; j < k; ++j) col[j] = w[j][i];
      const uint32_t r = reduce_word(col, k, ReduceType::Bf16);
      std::memcpy(static_cast<char*>(out) + at + 4 * i, &r, 4);
    }
  });
}

void host_fill_wire_operand(void* p, size_t n, uint64_t seed) {
  P2P_CHECK(n % kWireBlockBytes == 0, "host_fill_wire_operand: the payload is a multiple of 64 bytes (blocks of 32 bf16)");
  for (size_t at = 0; at < n; at += kWireBlockBytes) {
    uint16_t x[kWireBlockElems];
    wire_operand_block(seed, at / kWireBlockBytes, x);
    std::memcpy(static_cast<char*>(p) + at, x, sizeof(x));
  }
}

VerifyResult host_verify_wire_reduced(const void* p, size_t n, const uint64_t* seeds, int nseeds, WireFormat f, bool own_bf16,
                                      bool roundtrip) {
  check_wire(n, f, "host_verify_wire_reduced");
  P2P_CHECK(nseeds >= 1 && nseeds <= kMaxWireReduceSrcs, "host_verify_wire_reduced: 1..8 operand seeds");
  VerifyResult r;
  for (size_t at = 0; at < n; at += kWireBlockBytes) {
    uint16_t x[kMaxWireReduceSrcs][kWireBlockElems];
    uint32_t sb[kMaxWireReduceSrcs];
    for (int j = 0; j < nseeds; ++j) {
      wire_operand_block(seeds[j], at / kWireBlockBytes, x[j]);
      uint32_t amax = 0;
      for (uint32_t i = 0; i < kWireBlockElems; ++i) amax = std::max<uint32_t>(amax, x[j][i] & 0x7FFFu);
      sb[j] = wire_scale_byte(amax, f);
    }
    uint32_t want[16], amax = 0;
    for (uint32_t i = 0; i < 16; ++i) {
      uint32_t w[kMaxWireReduceSrcs];
      for (int j = 0; j < nseeds; ++j) w[j] = x[j][2 * i] | static_cast<uint32_t>(x[j][2 * i + 1]) << 16;
      want[i] = wire_reduce_word(w, sb, nseeds, f, own_bf16);
      amax = std::max(amax, wire_word_amax(want[i]));
    }
    // --reduce-out both: what the block's image widens to.
    for (uint32_t i = 0; roundtrip && i < 16; ++i) want[i] = wire_roundtrip_word(want[i], wire_scale_byte(amax, f), f);
    for (uint32_t i = 0; i < 16; ++i) {
      uint32_t got;
      std::memcpy(&got, static_cast<const char*>(p) + at + 4 * i, 4);
      r.checksum += got;
      if (got != want[i]) {
        if (!r.mismatches) r.first_bad = at + 4 * i;
        ++r.mismatches;
      }
    }
  }
  return r;
}

// ---- the same sum, requantised (wire_reduce_op.hpp) ----
void host_wire_reduce_packed(void* out_image, const void* const* images, int k, size_t n, WireFormat f, bool own_bf16) {
  check_wire(n, f, "host_wire_reduce_packed");
  std::vector<char> sum(n);
  host_wire_reduce(sum.data(), images, k, n, f, own_bf16);
  host_wire_pack(out_image, sum.data(), n, f);
}

VerifyResult host_verify_wire_reduced_packed(const void* image, size_t n, const uint64_t* seeds, int nseeds, WireFormat f,
                                             bool own_bf16) {
  check_wire(n, f, "host_verify_wire_reduced_packed");
  P2P_CHECK(nseeds >= 1 && nseeds <= kMaxWireReduceSrcs, "host_verify_wire_reduced_packed: 1..8 operand seeds");
  const auto* in = static_cast<const uint8_t*>(image);
  const uint32_t code_words = wire_block_elem_bytes(f) / 4, per = 16 / code_words;  // sum words per word of codes
  VerifyResult r;
  auto wrong = [&](size_t at) {
    r.first_bad = std::min<uint64_t>(r.first_bad, at);
    ++r.mismatches;
  };
  for_each_wire_block(n, f, [&](size_t at, size_t elems, size_t scale) {
    uint16_t x[kMaxWireReduceSrcs][kWireBlockElems];
    uint32_t sb[kMaxWireReduceSrcs], sum[16], amax = 0;
    for (int j = 0; j < nseeds; ++j) {
      wire_operand_block(seeds[j], at / kWireBlockBytes, x[j]);
      uint32_t a = 0;
      for (uint32_t i = 0; i < kWireBlockElems; ++i) a = std::max<uint32_t>(a, x[j][i] & 0x7FFFu);
      sb[j] = wire_scale_byte(a, f);
    }
    for (uint32_t i = 0; i < 16; ++i) {
      uint32_t w[kMaxWireReduceSrcs];
      for (int j = 0; j < nseeds; ++j) w[j] = x[j][2 * i] | static_cast<uint32_t>(x[j][2 * i + 1]) << 16;
      sum[i] = wire_reduce_word(w, sb, nseeds, f, own_bf16);
      amax = std::max(amax, wire_word_amax(sum[i]));
    }
    const uint32_t out_sb = wire_scale_byte(amax, f);
    for (uint32_t c = 0; f == WireFormat::Mxfp6 && c < 4; ++c) {  // 6-byte groups of 8 codes, not whole words
      uint64_t got = 0;
      std::memcpy(&got, in + elems + 6 * c, 6);
      r.checksum += got;
      if (got != wire_code_bits6(sum + 4 * c, out_sb)) wrong(elems + 6 * c);
    }
    for (uint32_t c = 0; f != WireFormat::Mxfp6 && c < code_words; ++c) {
      uint32_t got;
      std::memcpy(&got, in + elems + 4 * c, 4);
      r.checksum += got;
      if (got != wire_code_word(sum + per * c, out_sb, f)) wrong(elems + 4 * c);
    }
    r.checksum += in[scale];
    if (in[scale] != out_sb) wrong(scale);
  });
  return r;
}

namespace {

void sockopts(int fd) {
  int one = 1;
  setsockopt(fd, IPPROTO_TCP, TCP_NODELAY, &one, sizeof(one));
}

void blocking_io(int fd, void* buf, size_t n, bool is_send, double timeout_s) {
  char* p = static_cast<char*>(buf);
  double deadline = now_seconds() + timeout_s;
  while (n) {
    ssize_t k = is_send ? ::send(fd, p, n, MSG_NOSIGNAL) : ::recv(fd, p, n, 0);
    if (k > 0) {
      p += k;
      n -= static_cast<size_t>(k);
    } else if (k == 0) {
      P2P_FATAL("host transport: peer closed connection");
    } else if (errno != EINTR && errno != EAGAIN) {
      P2P_FATAL(strfmt("host transport io: %s", std::strerror(errno)));
    }
    if (now_seconds() > deadline) P2P_FATAL("host transport: handshake timeout");
  }
}

struct Endpoint {
  char host[64];
  int32_t port;
  uint64_t host_hash;
};

class HostTransport final : public Transport {
 public:
  HostTransport(Bootstrap& boot, const TransportOptions& opt) : rank_(boot.rank()), n_(boot.size()), timeout_(opt.timeout_s) {
    fds_.assign(static_cast<size_t>(n_), -1);
    TcpListener listener(0);
    Endpoint me{};
    std::string hn = real_hostname();  // routable name, not the P2P_HOSTNAME test override
    std::snprintf(me.host, sizeof(me.host), "%s", hn.c_str());
    me.port = listener.port();
    me.host_hash = host_hash(hn);
    auto eps = boot.allgather_value(me);
    int lfd = listener.release();
    // Rank i connects to every j < i; j accepts.
    for (int j = 0; j < rank_; ++j) {
      std::string host = eps[j].host_hash == me.host_hash ? "127.0.0.1" : std::string(eps[j].host);
      fds_[j] = connect_to(host, eps[j].port);
      int32_t id = rank_;
      blocking_io(fds_[j], &id, sizeof(id), true, timeout_);
    }
    for (int got = 0; got < n_ - 1 - rank_; ++got) {
      pollfd p{lfd, POLLIN, 0};
      int rc = ::poll(&p, 1, static_cast<int>(timeout_ * 1000));
      P2P_CHECK(rc > 0, "host transport: timed out waiting for mesh connections");
      int fd = ::accept(lfd, nullptr, nullptr);
      P2P_CHECK(fd >= 0, "accept failed");
      sockopts(fd);
      int32_t id = -1;
      blocking_io(fd, &id, sizeof(id), false, timeout_);
      P2P_CHECK(id > rank_ && id < n_ && fds_[id] < 0, strfmt("bad mesh peer id %d", id));
      fds_[id] = fd;
    }
    ::close(lfd);
    boot.barrier();
  }

  ~HostTransport() override {
    release_discard_sink();
    for (int fd : fds_)
      if (fd >= 0) ::close(fd);
  }

  void set_timeout(double seconds) override { timeout_ = seconds; }
  // A CPU transport moves data inside group_end(), so there is no stream to
  // hold.  P2P_TEST_FAKE_GATE=1 (host unit tests) accepts the gate anyway, so
  // run_latency's batched pre-posted path runs on the CPU.
  bool gate_arm(double) override {
    const char* f = std::getenv("P2P_TEST_FAKE_GATE");
    return f && std::atoi(f) != 0;
  }
  std::string name() const override { return "host"; }
  int rank() const override { return rank_; }
  int nranks() const override { return n_; }
  std::string device_desc() const override { return "cpu:" + short_hostname(); }

  void* alloc(size_t bytes) override {
    void* p = nullptr;
    P2P_CHECK(posix_memalign(&p, 256, std::max<size_t>(bytes, 1)) == 0, "host alloc failed");
    return p;
  }
  void release(void* p) override { std::free(p); }
  void fill(void* p, size_t bytes, uint64_t seed) override { host_fill(p, bytes, seed); }
  void zero(void* p, size_t bytes) override { std::memset(p, 0, bytes); }
  VerifyResult verify(const void* p, size_t bytes, uint64_t seed) override { return host_verify(p, bytes, seed); }
  std::vector<DiagExtent> diagnose(const void* p, size_t bytes, uint64_t seed,
                                   const std::vector<DiagCandidate>& candidates) override {
    return host_diagnose_extents(p, bytes, seed, candidates);
  }

  // ---- receive-and-reduce: each message into scratch, then the CPU sum ----
  bool supports_reduce() const override { return true; }
  void fill_operand(void* p, size_t bytes, uint64_t seed, ReduceType dtype) override {
    host_fill_operand(p, bytes, seed, dtype);
  }
  VerifyResult verify_reduced(const void* p, size_t bytes, const std::vector<uint64_t>& seeds, ReduceType dtype) override {
    return host_verify_reduced(p, bytes, seeds.data(), static_cast<int>(seeds.size()), dtype);
  }
  void reduce_from(void* dst, size_t bytes, const void* local_src, const std::vector<int>& peers, size_t,
                   ReduceType dtype) override {
    P2P_CHECK(in_group_ && !reduce_.dst, "host transport: one reduce_from per group, inside the group");
    P2P_CHECK(bytes % 4 == 0, "host transport: a reduced message is a multiple of 4 bytes");
    reduce_ = {dst, bytes, local_src, dtype, peers.size()};
    if (scratch_.size() < bytes * peers.size()) scratch_.resize(bytes * peers.size());
    for (size_t i = 0; i < peers.size(); ++i) {
      P2P_CHECK(peers[i] >= 0 && peers[i] < n_, "bad peer");
      ops_.push_back({false, peers[i], scratch_.data() + i * bytes, bytes});
    }
  }

  // ---- gated sum: the same receives into scratch, then the CPU's gated sum ----
  bool supports_reduce_gate() const override { return true; }
  void fill_gate(void* p, size_t rows, uint64_t seed) override { host_fill_gate(p, rows, seed); }
  VerifyResult verify_reduced_gated(const void* p, size_t bytes, const std::vector<uint64_t>& seeds, uint64_t gate_seed,
                                    size_t row_elems) override {
    return host_verify_gated_reduced(p, bytes, seeds.data(), static_cast<int>(seeds.size()), gate_seed, row_elems);
  }
  void reduce_gated_from(void* dst, size_t bytes, const void* local_src, const std::vector<int>& peers, size_t src_offset,
                         const void* gate, size_t row_elems) override {
    P2P_CHECK(peers.size() < static_cast<size_t>(kGateSlots), "host transport: a gated sum has at most 8 operands (the own one and 7 incoming)");
    P2P_CHECK(gate && gate_rows(bytes, row_elems) > 0, "host transport: a gated sum is whole rows of row_elems bf16 under a gate table");
    reduce_from(dst, bytes, local_src, peers, src_offset, ReduceType::Bf16);
    reduce_.gate = gate;
    reduce_.row_elems = row_elems;
  }

  // ---- wire formats: the packed image travels, the CPU widens it ----
  bool supports_wire() const override { return true; }
  void fill_packed(void* p, size_t payload_bytes, uint64_t seed, WireFormat fmt) override {
    host_fill_packed(p, payload_bytes, seed, fmt);
  }
  VerifyResult verify_unpacked(const void* p, size_t payload_bytes, uint64_t seed, WireFormat fmt) override {
    return host_verify_unpacked(p, payload_bytes, seed, fmt);
  }
  void recv_unpacked(void* dst, size_t payload_bytes, int peer, size_t, WireFormat fmt) override {
    P2P_CHECK(in_group_, "host transport: recv_unpacked inside a group");
    P2P_CHECK(peer >= 0 && peer < n_, "bad peer");
    // Moving a vector keeps its storage: the op's pointer stays good as unpacks_ grows.
    unpacks_.push_back({dst, payload_bytes, fmt, std::vector<char>(wire_bytes(payload_bytes, fmt))});
    ops_.push_back({false, peer, unpacks_.back().wire.data(), unpacks_.back().wire.size()});
  }

  // ---- sum of wire images: each image into scratch, then the CPU sum ----
  bool supports_reduce_wire() const override { return true; }
  void fill_wire_operand(void* p, size_t payload_bytes, uint64_t seed) override { host_fill_wire_operand(p, payload_bytes, seed); }
  VerifyResult verify_reduced_unpacked(const void* p, size_t payload_bytes, const std::vector<uint64_t>& seeds,
                                       WireFormat fmt, bool own_bf16, bool roundtrip) override {
    return host_verify_wire_reduced(p, payload_bytes, seeds.data(), static_cast<int>(seeds.size()), fmt, own_bf16, roundtrip);
  }
  void reduce_unpacked_from(void* dst, size_t payload_bytes, const void* local_image, const std::vector<int>& peers, size_t,
                            WireFormat fmt, bool own_bf16) override {
    P2P_CHECK(in_group_ && !wire_reduce_.dst, "host transport: one reduce_unpacked_from per group, inside the group");
    P2P_CHECK(peers.size() < static_cast<size_t>(kMaxWireReduceSrcs),
              "host transport: a sum of wire images has at most 8 operands (the own one and 7 incoming)");
    const size_t image = wire_bytes(payload_bytes, fmt);
    wire_reduce_ = {dst, payload_bytes, local_image, fmt, peers.size(), false, own_bf16};
    if (scratch_.size() < image * peers.size()) scratch_.resize(image * peers.size());
    for (size_t i = 0; i < peers.size(); ++i) {
      P2P_CHECK(peers[i] >= 0 && peers[i] < n_, "bad peer");
      ops_.push_back({false, peers[i], scratch_.data() + i * image, image});
    }
  }
  // --reduce-out wire: the same receives, the sum packed again in group_end().
  VerifyResult verify_reduced_packed(const void* p, size_t payload_bytes, const std::vector<uint64_t>& seeds,
                                     WireFormat fmt, bool own_bf16) override {
    return host_verify_wire_reduced_packed(p, payload_bytes, seeds.data(), static_cast<int>(seeds.size()), fmt, own_bf16);
  }
  void reduce_packed_from(void* dst, size_t payload_bytes, const void* local_image, const std::vector<int>& peers,
                          size_t src_offset, WireFormat fmt, bool own_bf16, void* image_dst) override {
    reduce_unpacked_from(dst, payload_bytes, local_image, peers, src_offset, fmt, own_bf16);
    wire_reduce_.packed = true;
    wire_reduce_.image_dst = image_dst;
  }

  void group_begin() override {
    P2P_CHECK(!in_group_, "nested group");
    in_group_ = true;
    ops_.clear();
    reduce_ = {};
    wire_reduce_ = {};
    unpacks_.clear();
  }
  void send(const void* p, size_t bytes, int peer) override {
    P2P_CHECK(peer >= 0 && peer < n_, "bad peer");
    ops_.push_back({true, peer, const_cast<char*>(static_cast<const char*>(p)), bytes});
    if (!in_group_) run_ops();
  }
  void recv(void* p, size_t bytes, int peer) override {
    P2P_CHECK(peer >= 0 && peer < n_, "bad peer");
    // Injected skip fault: the bytes are read off the wire into a sink.
    ops_.push_back({false, peer, static_cast<char*>(discarding() ? discard_sink(bytes) : p), bytes});
    if (!in_group_) run_ops();
  }
  void group_end() override {
    P2P_CHECK(in_group_, "group_end without group_begin");
    in_group_ = false;
    std::vector<size_t> sent(static_cast<size_t>(n_), 0);
    for (const auto& op : ops_)
      if (op.is_send) sent[static_cast<size_t>(op.peer)] += op.bytes;
    emulate_link_delay(sent, rank_);
    run_ops();
    // Injected skip fault: the messages were read off the wire, the sum is not made.
    if (reduce_.dst && !discarding()) {
      std::vector<const void*> operands{reduce_.local_src};
      for (size_t i = 0; i < reduce_.npeers; ++i) operands.push_back(scratch_.data() + i * reduce_.bytes);
      if (reduce_.gate)
        host_gated_reduce(reduce_.dst, operands.data(), static_cast<int>(operands.size()), reduce_.bytes, reduce_.gate, reduce_.row_elems);
      else
        host_reduce(reduce_.dst, operands.data(), static_cast<int>(operands.size()), reduce_.bytes, reduce_.dtype);
    }
    reduce_ = {};
    if (wire_reduce_.dst && !discarding()) {
      const size_t image = wire_bytes(wire_reduce_.bytes, wire_reduce_.fmt);
      std::vector<const void*> images{wire_reduce_.local_image};
      for (size_t i = 0; i < wire_reduce_.npeers; ++i) images.push_back(scratch_.data() + i * image);
      void* out = wire_reduce_.image_dst ? wire_reduce_.image_dst : wire_reduce_.dst;
      (wire_reduce_.packed ? host_wire_reduce_packed : host_wire_reduce)(out, images.data(), static_cast<int>(images.size()),
                                                                         wire_reduce_.bytes, wire_reduce_.fmt, wire_reduce_.own_bf16);
      // --reduce-out both: the slot keeps what the image widens to.
      if (wire_reduce_.image_dst) host_wire_unpack(wire_reduce_.dst, wire_reduce_.image_dst, wire_reduce_.bytes, wire_reduce_.fmt);
    }
    wire_reduce_ = {};
    // Injected skip fault: the images were read off the wire and are dropped.
    for (const PendingUnpack& u : unpacks_)
      if (!discarding()) host_wire_unpack(u.dst, u.wire.data(), u.bytes, u.fmt);
    unpacks_.clear();
  }

  int mark() override {
    marks_.push_back(now_seconds());
    return static_cast<int>(marks_.size()) - 1;
  }
  double elapsed_ms(int a, int b) override { return (marks_.at(b) - marks_.at(a)) * 1e3; }
  void clear_marks() override { marks_.clear(); }
  void sync() override {}

 private:
  struct PendingReduce {
    void* dst = nullptr;
    size_t bytes = 0;
    const void* local_src = nullptr;
    ReduceType dtype = ReduceType::Off;
    size_t npeers = 0;
    const void* gate = nullptr;  // reduce_gated_from: the gate table, rows of row_elems bf16
    size_t row_elems = 0;
  };
  struct PendingWireReduce {
    void* dst = nullptr;
    size_t bytes = 0;  // payload
    const void* local_image = nullptr;
    WireFormat fmt = WireFormat::Off;
    size_t npeers = 0;
    bool packed = false;  // reduce_packed_from: dst receives the sum's wire image
    bool own_bf16 = false;  // local_image is the own shard in bf16
    void* image_dst = nullptr;  // --reduce-out both: the image goes here, dst takes its unpack
  };
  struct PendingUnpack {
    void* dst;
    size_t bytes;  // payload
    WireFormat fmt;
    std::vector<char> wire;
  };
  struct Op {
    bool is_send;
    int peer;
    char* buf;
    size_t bytes;
    size_t done = 0;
  };

  int connect_to(const std::string& host, int port) {
    double deadline = now_seconds() + timeout_;
    while (now_seconds() < deadline) {
      addrinfo hints{};
      hints.ai_family = AF_INET;
      hints.ai_socktype = SOCK_STREAM;
      addrinfo* res = nullptr;
      if (getaddrinfo(host.c_str(), std::to_string(port).c_str(), &hints, &res) == 0) {
        for (addrinfo* ai = res; ai; ai = ai->ai_next) {
          int fd = ::socket(ai->ai_family, ai->ai_socktype, ai->ai_protocol);
          if (fd < 0) continue;
          if (::connect(fd, ai->ai_addr, ai->ai_addrlen) == 0) {
            freeaddrinfo(res);
            sockopts(fd);
            return fd;
          }
          ::close(fd);
        }
        freeaddrinfo(res);
      }
      std::this_thread::sleep_for(std::chrono::milliseconds(20));
    }
    P2P_FATAL(strfmt("host transport: cannot connect to %s:%d", host.c_str(), port));
  }

  // Progress every op of the group; per peer, sends complete in posting order
  // and receives complete in posting order (NCCL's matching rule).
  void run_ops() {
    std::vector<std::deque<Op*>> sendq(static_cast<size_t>(n_)), recvq(static_cast<size_t>(n_));
    for (auto& op : ops_) (op.is_send ? sendq : recvq)[static_cast<size_t>(op.peer)].push_back(&op);
    // Self transfers: the k-th send to self matches the k-th recv from self.
    auto& ss = sendq[static_cast<size_t>(rank_)];
    auto& rs = recvq[static_cast<size_t>(rank_)];
    P2P_CHECK(ss.size() == rs.size() || !in_group_, "unmatched self send/recv in group");
    while (!ss.empty() && !rs.empty()) {
      P2P_CHECK(ss.front()->bytes == rs.front()->bytes, "self send/recv size mismatch");
      std::memcpy(rs.front()->buf, ss.front()->buf, ss.front()->bytes);
      ss.pop_front();
      rs.pop_front();
    }
    P2P_CHECK(ss.empty() && rs.empty(), "self send without matching recv");
    double deadline = now_seconds() + timeout_;
    for (;;) {
      std::vector<pollfd> pfds;
      for (int p = 0; p < n_; ++p) {
        if (p == rank_) continue;
        short ev = 0;
        if (!sendq[p].empty()) ev |= POLLOUT;
        if (!recvq[p].empty()) ev |= POLLIN;
        if (ev) pfds.push_back({fds_[p], ev, 0});
      }
      if (pfds.empty()) break;
      int rc = ::poll(pfds.data(), pfds.size(), 100);
      if (rc < 0 && errno == EINTR) continue;
      P2P_CHECK(rc >= 0, "poll failed");
      if (rc == 0) {
        if (now_seconds() > deadline) P2P_FATAL("host transport: group timed out (peer hung or dead)");
        if (abort_requested()) abort_wait("host transport");
        continue;
      }
      for (auto& pf : pfds) {
        int peer = static_cast<int>(std::find(fds_.begin(), fds_.end(), pf.fd) - fds_.begin());
        if (pf.revents & (POLLERR | POLLNVAL)) P2P_FATAL(strfmt("host transport: socket error with peer %d", peer));
        if ((pf.revents & POLLOUT) && !sendq[peer].empty()) {
          Op* op = sendq[peer].front();
          ssize_t k = ::send(pf.fd, op->buf + op->done, op->bytes - op->done, MSG_NOSIGNAL | MSG_DONTWAIT);
          if (k > 0) op->done += static_cast<size_t>(k);
          else if (k < 0 && errno != EAGAIN && errno != EINTR)
            P2P_FATAL(strfmt("host transport send to %d: %s", peer, std::strerror(errno)));
          if (op->done == op->bytes) sendq[peer].pop_front();
        }
        if ((pf.revents & (POLLIN | POLLHUP)) && !recvq[peer].empty()) {
          Op* op = recvq[peer].front();
          ssize_t k = ::recv(pf.fd, op->buf + op->done, op->bytes - op->done, MSG_DONTWAIT);
          // Re-arm quick ACKs: a delayed ACK stalls a sender whose message is
          // larger than its current send window.
          int one = 1;
          setsockopt(pf.fd, IPPROTO_TCP, TCP_QUICKACK, &one, sizeof(one));
          if (k > 0) op->done += static_cast<size_t>(k);
          else if (k == 0) P2P_FATAL(strfmt("host transport: peer %d closed the connection", peer));
          else if (errno != EAGAIN && errno != EINTR)
            P2P_FATAL(strfmt("host transport recv from %d: %s", peer, std::strerror(errno)));
          if (op->done == op->bytes) recvq[peer].pop_front();
        }
      }
    }
    ops_.clear();
  }

  int rank_, n_;
  double timeout_;
  std::vector<int> fds_;
  bool in_group_ = false;
  std::vector<Op> ops_;
  PendingWireReduce wire_reduce_;  // the open group's reduce_unpacked_from, summed in group_end()
  PendingReduce reduce_;       // the open group's reduce_from, summed in group_end()
  std::vector<char> scratch_;  // its incoming messages, one after the other
  std::vector<PendingUnpack> unpacks_;  // the open group's recv_unpacked, widened in group_end()
  std::vector<double> marks_;
};

}  // namespace

std::unique_ptr<Transport> make_host_transport(Bootstrap& boot, const TransportOptions& opt) {
  return std::make_unique<HostTransport>(boot, opt);
}

}  // namespace p2p
