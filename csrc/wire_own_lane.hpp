// The load side of a bf16 own shard (WireReduceOp::own_bf16, --reduce-own
// bf16) that wire_reduce.hip and wire_reduce_pack.hip share for mxfp8 and
// mxfp4: a lane's own operand is the 16 elements it accumulates.  mxfp6, a
// block per lane, has wire6_lane.hpp load_block instead.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace p2p {
namespace dev {
namespace wire_own {

typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

// Unit 0 and unit 1 as 16 B each, at payload byte offsets 2 e0 and 2 e1 of the
// tile at ps (local memory), non-temporal.  Split mapping: two loads 4 KiB
// apart, each coalesced over the wave, the mirror of the bf16 sum's stores;
// contiguous: the lane's 32 B.  A unit past the tile's end re-reads the tile's
// first 16 B (every tile has a block); its lane stores nothing.
__device__ __forceinline__ void load_own(const char* ps, uint32_t e0, uint32_t e1, bool in0, bool in1, u32x4& h0, u32x4& h1) {
  h0 = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(ps + (in0 ? 2u * e0 : 0u)));
  h1 = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(ps + (in1 ? 2u * e1 : 0u)));
}
// 4 words of bf16 -> 8 f32, exact: shifts and masks, as reduce.hip widens.
__device__ __forceinline__ void widen_own(const u32x4& h, float (&x)[8]) {
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    x[2 * j] = __builtin_bit_cast(float, h[j] << 16);
    x[2 * j + 1] = __builtin_bit_cast(float, h[j] & 0xFFFF0000u);
  }
}

}  // namespace wire_own
}  // namespace dev
}  // namespace p2p
