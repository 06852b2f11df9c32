// Device side of the 6-bit wire format (mxfp6, OCP e2m3; wire_op.hpp): what
// the unpack and pack kernels (wire.hip) and the wire-reduce kernel
// (wire_reduce.hip) share.  Design:
//   * The 6-bit conversions are block instructions: v_cvt_scalef32_pk32_bf16_fp6
//     and _pk32_f32_fp6 widen 6 VGPRs of codes to 32 elements under one scale
//     operand, v_cvt_scalef32_pk32_fp6_bf16 narrows 16 VGPRs of bf16 to 6.  So
//     a lane owns a block: 24 B of codes and one scale byte in, 64 B of bf16
//     out; a wave owns 64 consecutive blocks (1536 B of codes, 4 KiB of
//     payload), two waves a tile.  No shuffle anywhere: a block's amax and its
//     scale never leave the lane.
//   * Loads.  A block's codes start 8 B aligned (24 B blocks in a 16 B aligned
//     tile), never more in general, so a lane issues three 8 B loads; the
//     wave's codes are contiguous, so the three instructions together fetch
//     whole cache lines.  The scale byte is one byte load, 64 consecutive
//     bytes per wave.  All loads of a tile precede its first conversion; in
//     the sum the compiler then waits with a counted vmcnt per operand, so
//     operand k is widened and added as soon as it has arrived while k + 1 ..
//     K - 1 are still in flight.
//   * Stores decide the rate (a lane writes 64 B for 25 B read), and a lane's
//     own 64 B would leave as four 16 B stores with a 64 B lane stride: every
//     instruction touches 64 cache lines for 1 KiB.  Two paths, selected by
//     the existing `lanes` argument:
//       contiguous: exactly that, no LDS;
//       split: the wave's 4 KiB goes through a wave-private 4 KiB LDS slot and
//         leaves as four fully coalesced 16 B stores, 1 KiB of consecutive
//         bytes per instruction.  Row r of the slot (64 B, lane r's block)
//         keeps its 16 B chunk c at position c ^ ((r >> 2) & 3): the 16 lanes
//         a ds_write_b128 serves at once then hit 16 different 4-bank groups,
//         and the read-back (lane l: row 16i + l / 4, chunk l % 4) walks 256
//         consecutive bytes per 16 lanes.  Conflict-free both ways in exactly
//         4 KiB, which padded rows are not (80 B rows make a quarter of the
//         reads two-way).  Only the wave touches its slot and the LDS executes
//         one wave's instructions in order, so there is no workgroup barrier:
//         wavefront-scope fences keep the compiler from reordering the slot's
//         writes and reads, the hardware needs nothing but the wait for the
//         read data.
//   * A lane past a ragged tile's end loads harmlessly (the tile's first block,
//     or offset = range end of the descriptor, which returns 0) and stores
//     nothing (a predicate, or the descriptor drops it).
#pragma once

#include <hip/hip_runtime.h>

#include "wire_op.hpp"

namespace p2p {
namespace dev {
namespace wire6 {

typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned int u32x6 __attribute__((ext_vector_type(6)));
typedef unsigned int u32x16 __attribute__((ext_vector_type(16)));
typedef __bf16 bf16x32 __attribute__((ext_vector_type(32)));
typedef float f32x32 __attribute__((ext_vector_type(32)));

constexpr WireFormat kF = WireFormat::Mxfp6;
constexpr uint32_t kEB = wire_block_elem_bytes(kF);                    // 24
constexpr uint32_t kFullTile = wire_tile_bytes(kWireTileBlocks, kF);   // 3200
constexpr uint32_t kTileLanes = kWireTileBlocks;                       // a lane per block
// Workgroup of the unpack and wire-reduce kernels: 4 waves, two tiles per pass.
// Measured against 128 lanes (one tile) with the two builds taking turns in
// one window (docs/DESIGN.md, profiles/wire6/workgroup_size.txt): level for
// the local unpack, 256 ahead by 2% in the cross-GPU form and by 1-3% for the
// sum at 1 GiB; 128 is ahead only for the sum at 32 MiB, K = 8 (3%).
constexpr int kLanes = 256;
constexpr uint32_t kTilesPerGroup = kLanes / kTileLanes;
constexpr uint32_t kSlotBytes = 64 * kWireBlockBytes;  // a wave's 4 KiB
static_assert(kLanes == 128 || kLanes == 256, "one or two tiles per workgroup");
// Cache-policy bits and descriptor word of the cross-GPU accesses (kernels.hip)
// and the conversions' scale operand: wire.hip and wire_reduce.hip use these
// definitions for all their formats.
constexpr int kSystemCoherent = 1 | 16;  // sc0 sc1
constexpr int kNonTemporal = 2;           // nt
constexpr int kRsrcFlags = 0x00020000;

__device__ __forceinline__ float scale_operand(uint32_t sb) { return __builtin_bit_cast(float, sb << 23); }

// A block's 24 B of codes at byte offset `at` of a tile's descriptor.
template <int AUX>
__device__ __forceinline__ u32x6 load_codes(__amdgpu_buffer_rsrc_t rs, int at) {
  const u32x2 a = __builtin_amdgcn_raw_buffer_load_b64(rs, at, 0, AUX);
  const u32x2 b = __builtin_amdgcn_raw_buffer_load_b64(rs, at + 8, 0, AUX);
  const u32x2 c = __builtin_amdgcn_raw_buffer_load_b64(rs, at + 16, 0, AUX);
  return u32x6{a[0], a[1], b[0], b[1], c[0], c[1]};
}
// The same from local memory, non-temporal.
__device__ __forceinline__ u32x6 load_codes(const char* p) {
  const auto* q = reinterpret_cast<const u32x2*>(p);
  const u32x2 a = __builtin_nontemporal_load(q), b = __builtin_nontemporal_load(q + 1), c = __builtin_nontemporal_load(q + 2);
  return u32x6{a[0], a[1], b[0], b[1], c[0], c[1]};
}

// Orders the wave's LDS accesses for the compiler; the hardware keeps one
// wave's LDS instructions in order by itself.
__device__ __forceinline__ void wave_lds_fence() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// Stores the lane's widened block v (64 B as four 16 B chunks) of a tile of nb
// blocks whose payload begins at pd.  lane: 0..63; wave_block: the tile block
// of the wave's lane 0 (0 or 64); slot: the wave's kSlotBytes of LDS (SPLIT).
// dst_coherent: pd is a peer's buffer, written at system scope through a
// descriptor over the tile's nb blocks, which drops what lies past them.
template <bool SPLIT>
__device__ __forceinline__ void store_block(const u32x4 (&v)[4], char* pd, uint32_t nb, uint32_t wave_block, uint32_t lane,
                                            bool dst_coherent, char* slot) {
  u32x4 o[4];
  uint32_t off[4];  // byte offsets in the tile's payload
  if constexpr (SPLIT) {
    const uint32_t wsw = (lane >> 2) & 3u;
#pragma unroll
    for (uint32_t c = 0; c < 4; ++c) *reinterpret_cast<u32x4*>(slot + 64u * lane + 16u * (c ^ wsw)) = v[c];
    wave_lds_fence();
#pragma unroll
    for (uint32_t i = 0; i < 4; ++i) {
      const uint32_t row = 16u * i + (lane >> 2), chunk = lane & 3u;
      o[i] = *reinterpret_cast<const u32x4*>(slot + 64u * row + 16u * (chunk ^ ((row >> 2) & 3u)));
      off[i] = kWireBlockBytes * wave_block + 1024u * i + 16u * lane;
    }
    wave_lds_fence();  // the next tile's writes stay behind these reads
  } else {
#pragma unroll
    for (uint32_t c = 0; c < 4; ++c) o[c] = v[c], off[c] = kWireBlockBytes * (wave_block + lane) + 16u * c;
  }
  if (dst_coherent) {
    auto rd = __builtin_amdgcn_make_buffer_rsrc(pd, 0, static_cast<int>(nb * kWireBlockBytes), kRsrcFlags);
#pragma unroll
    for (int i = 0; i < 4; ++i) __builtin_amdgcn_raw_buffer_store_b128(o[i], rd, static_cast<int>(off[i]), 0, kSystemCoherent);
  } else {
#pragma unroll
    for (int i = 0; i < 4; ++i)
      if (off[i] / kWireBlockBytes < nb) __builtin_nontemporal_store(o[i], reinterpret_cast<u32x4*>(pd + off[i]));
  }
}

// store_block's mirror, the load of a lane's own 64 B of bf16 (the sum's own
// shard, wire_reduce_op.hpp own_bf16): block wave_block + lane of a tile of nb
// blocks whose payload begins at ps, local memory.  Split in two so that the
// global loads can be issued with the tile's other loads and the LDS exchange
// waits for them alone.  SPLIT: the wave reads its 4 KiB as four fully
// coalesced 16 B loads (load_block: instruction i covers bytes 1024 i ..
// 1024 i + 1023 of the wave's payload, lane l the chunk l % 4 of row
// 16 i + l / 4), writes them into its slot under the store path's swizzle and
// reads its own row back as four ds_read_b128 (load_block_rows), conflict-free
// both ways for the reason given above.  The slot is the one store_block uses
// later in the tile; the fences here and there order the two uses for the
// compiler.  Contiguous: four 16 B loads straight from the lane's block, a
// 64 B lane stride.  A chunk past the tile's end is read from the tile's first
// 16 B instead (every tile has a block): its lane stores nothing.
template <bool SPLIT>
__device__ __forceinline__ void load_block(u32x4 (&g)[4], const char* ps, uint32_t nb, uint32_t wave_block, uint32_t lane) {
#pragma unroll
  for (uint32_t i = 0; i < 4; ++i) {
    const uint32_t off = SPLIT ? kWireBlockBytes * wave_block + 1024u * i + 16u * lane
                               : kWireBlockBytes * (wave_block + lane) + 16u * i;
    g[i] = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(ps + (off / kWireBlockBytes < nb ? off : 0u)));
  }
}
template <bool SPLIT>
__device__ __forceinline__ void load_block_rows(u32x4 (&g)[4], uint32_t lane, char* slot) {
  if constexpr (SPLIT) {
#pragma unroll
    for (uint32_t i = 0; i < 4; ++i) {
      const uint32_t row = 16u * i + (lane >> 2), chunk = lane & 3u;
      *reinterpret_cast<u32x4*>(slot + 64u * row + 16u * (chunk ^ ((row >> 2) & 3u))) = g[i];
    }
    wave_lds_fence();
    const uint32_t wsw = (lane >> 2) & 3u;
#pragma unroll
    for (uint32_t c = 0; c < 4; ++c) g[c] = *reinterpret_cast<const u32x4*>(slot + 64u * lane + 16u * (c ^ wsw));
    wave_lds_fence();  // the store stage's writes stay behind these reads
  }
}

}  // namespace wire6
}  // namespace dev
}  // namespace p2p
