// Where the device-initiated stream (stream.hip, ipc_stream.hpp) keeps its
// rings and flags: plain host code, no HIP, so the CPU tests drive it.
//
// Every rank owns one exported page with two areas:
//   inbox   for every source r in 0..n (n: the self path's slot) and channel
//           c, a 256-byte header whose first word is `tail` (written by the
//           sender), then the ring of depth x bytes the sender writes into;
//   credit  for every destination d in 0..n and channel c, one 128-byte line
//           whose first word is `head` (written by the receiver d).
// Every inbox region and the credit area start on a 256-byte boundary and
// nothing overlaps.  The limits are the kernel's (kernels.hpp StreamRole).
#pragma once

#include <cstddef>

#include "common.hpp"

namespace p2p {

struct StreamLayout {
  static constexpr size_t kHeader = 256;      // tail + padding: the ring starts on its own lines
  static constexpr size_t kCreditLine = 128;  // one head per line
  static constexpr int kMaxChannels = 8;
  static constexpr int kMaxDepth = 64;
  static constexpr size_t kMaxBytes = size_t{1} << 20;      // per message
  static constexpr size_t kMaxRingBytes = size_t{4} << 20;  // depth x bytes
  static constexpr size_t kPageCap = size_t{1} << 30;       // the whole page
  static constexpr int kMaxIters = 100000;                  // messages per channel and launch

  int n = 0, channels = 0, depth = 0;
  size_t bytes = 0;        // per message, as laid out (a multiple of 16)
  size_t ring_bytes = 0;   // depth x bytes, rounded up to 256
  size_t inbox_bytes = 0;  // (n + 1) x channels x (kHeader + ring_bytes)
  size_t credit_offset = 0;
  size_t credit_bytes = 0;  // (n + 1) x channels lines, rounded up to 256
  size_t total = 0;         // inbox_bytes + credit_bytes

  // Offsets in the owner's page.  src / dst in 0..n, c in 0..channels-1.
  size_t tail(int src, int c) const { return (static_cast<size_t>(src) * channels + c) * (kHeader + ring_bytes); }
  size_t ring(int src, int c) const { return tail(src, c) + kHeader; }
  size_t head(int dst, int c) const { return credit_offset + (static_cast<size_t>(dst) * channels + c) * kCreditLine; }
};

// "" when (channels, depth, bytes) are within the limits, otherwise the
// message that names the one they break.  `bytes` counts as rounded up to 16.
inline std::string stream_limits_error(long long channels, long long depth, unsigned long long bytes) {
  if (channels < 1 || channels > StreamLayout::kMaxChannels)
    return strfmt("device stream: 1..%d channels, got %lld", StreamLayout::kMaxChannels, channels);
  if (depth < 1 || depth > StreamLayout::kMaxDepth)
    return strfmt("device stream: depth 1..%d, got %lld", StreamLayout::kMaxDepth, depth);
  const unsigned long long b = (bytes + 15) / 16 * 16;
  if (b < 16 || b > StreamLayout::kMaxBytes)
    return strfmt("device stream: messages of 16 bytes to 1 MiB (%zu bytes), got %llu", StreamLayout::kMaxBytes, bytes);
  if (static_cast<unsigned long long>(depth) * b > StreamLayout::kMaxRingBytes)
    return strfmt("device stream: depth x bytes is at most 4 MiB (%zu bytes), got %lld x %llu", StreamLayout::kMaxRingBytes,
                  depth, b);
  return "";
}

inline StreamLayout stream_layout(int n, int channels, int depth, size_t bytes) {
  P2P_CHECK(n >= 1 && n <= 4096, "device stream: bad rank count");
  const std::string bad = stream_limits_error(channels, depth, bytes);
  P2P_CHECK(bad.empty(), bad);
  StreamLayout l;
  l.n = n;
  l.channels = channels;
  l.depth = depth;
  l.bytes = (bytes + 15) / 16 * 16;
  l.ring_bytes = (static_cast<size_t>(depth) * l.bytes + 255) / 256 * 256;
  const size_t cells = static_cast<size_t>(n + 1) * static_cast<size_t>(channels);
  l.inbox_bytes = cells * (StreamLayout::kHeader + l.ring_bytes);
  l.credit_offset = l.inbox_bytes;
  l.credit_bytes = (cells * StreamLayout::kCreditLine + 255) / 256 * 256;
  l.total = l.inbox_bytes + l.credit_bytes;
  P2P_CHECK(l.total <= StreamLayout::kPageCap,
            strfmt("device stream: %d ranks x %d channels x %d x %zu bytes need a page of %zu bytes, above the cap of %zu",
                   n, channels, depth, l.bytes, l.total, StreamLayout::kPageCap));
  return l;
}

}  // namespace p2p
