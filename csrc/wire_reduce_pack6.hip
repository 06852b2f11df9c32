// gfx950 kernel of the requantising sum for mxfp6 (e2m3): K 6-bit wire images
// (or the bf16 own shard and K - 1 images) come in, the image of their bf16 sum
// leaves, and with BOTH the bf16 that image widens to beside it (--reduce-out
// both, the turn-around hop of a two-shot quantised all-reduce).  kernels.hpp
// has the contract, wire_reduce_op.hpp the arithmetic, wire6_lane.hpp the
// geometry this kernel shares with the unpack and the bf16 sum.  Design:
//   * A lane owns a block, a wave 64 consecutive blocks, two waves a tile, a
//     256-lane workgroup two tiles.  The 6-bit conversions are block
//     instructions, so nothing of the epilogue crosses a lane: that is what
//     separates this kernel from the mxfp8 / mxfp4 one (2 or 4 lanes a block,
//     DPP amax, a workgroup barrier per tile).  The waves of a tile never
//     meet: no barrier anywhere.
//   * Load side and f32 chains are wire_reduce6_kernel's (wire_reduce.hip):
//     all K x (three 8 B code loads + a scale byte) of a block before the first
//     conversion, v_cvt_scalef32_pk32_f32_fp6 per operand, 32 plain f32 adds;
//     OWN reads the wave's 4 KiB of bf16 coalesced and turns it into rows
//     through the wave's LDS slot.
//   * Epilogue, all inside the lane: 16 v_cvt_pk_bf16_f32 (the accumulators are
//     dead from here), an integer max over the 16 words' magnitudes,
//     wire_scale_byte, one v_cvt_scalef32_pk32_fp6_bf16 to 6 VGPRs of codes.
//   * Image stores, two paths on `lanes`:
//       contiguous: three 8 B stores at a 24 B lane stride (pack6_kernel's
//         way); the lane of an odd tile's last block writes the zero 8 B.
//       split: the wave's 1536 B of codes go through its slot and leave as
//         16 B stores of consecutive bytes, one by all 64 lanes and one by
//         lanes 0..31.  Rows stay linear, row r at byte 24 r, written as three
//         ds_write_b64: lane r's two dwords go to banks 6 r and 6 r + 1, and
//         6 r = 6 r' modulo the bank count B (32 or 64 dword banks) needs
//         r = r' modulo B / 2, so the 16 (or 32) lanes one LDS pass serves
//         hit that many distinct even banks and their odd neighbours: no
//         conflict, no padding, and no swizzle, because 24 B rows already have
//         the odd dword-pair stride a swizzle would create.  The read-back is
//         16 consecutive bytes per lane.  A lane past a ragged tile's end
//         writes a zero row, so the chunk that straddles an odd tile's last
//         block carries the zero 8 B with it; chunks at or past the scale
//         section are not stored.
//   * Scale bytes: a lane writes its byte (0 past the tile's end: the padding)
//     behind the code stage of the slot, lanes 0..3 read 16 B each and store
//     the chunks that begin inside the tile.  The wave that holds a ragged
//     tile's last block so writes the padding behind it.
//   * BOTH: one v_cvt_scalef32_pk32_bf16_fp6 widens the lane's codes back under
//     the same scale operand, store_block<SPLIT> writes them (wire6_lane.hpp).
//   * The slot is used three times per tile under SPLIT (own load_block_rows,
//     the image stage, the bf16 store_block), each use closed by a
//     wavefront-scope fence; the hardware keeps a wave's LDS accesses in order.
//   * Registers: every instantiation asks for 4 waves per SIMD (128 VGPRs), as
//     the OWN instantiations of the bf16 sum do; docs/DESIGN.md has the counts.
//   * No packed f32 instructions in this object (Makefile).
#include <hip/hip_runtime.h>

#include <algorithm>

#include "common.hpp"
#include "hip_check.hpp"
#include "kernels.hpp"
#include "wire6_lane.hpp"

namespace p2p {
namespace dev {

namespace {

using wire6::kNonTemporal;
using wire6::kRsrcFlags;
using wire6::kSystemCoherent;
using wire6::scale_operand;
using wire6::u32x2;
using wire6::u32x4;

constexpr uint64_t kMaxGrid = 1ull << 20;  // tiles per grid pass (8 GiB of payload)
constexpr uint32_t kCodeStage = 64 * wire6::kEB;  // a wave's codes: 1536 B

// By value in the kernarg segment.
struct ReducePack6Args {
  const char* src[kMaxWireReduceSrcs];
  char* dst;
  char* dst_bf16;  // BOTH
  uint64_t ntiles;
  uint32_t last_blocks;  // blocks of the last tile, 1..128
  uint32_t coherent;     // WireReduceOp::coherent_mask
};

template <int K, bool SPLIT, bool OWN, bool BOTH>
__global__ __launch_bounds__(wire6::kLanes) __attribute__((amdgpu_waves_per_eu(4))) void wire_reduce_pack6_kernel(
    const ReducePack6Args a) {
  using wire6::kF, wire6::kEB, wire6::kFullTile, wire6::kLanes, wire6::kTilesPerGroup, wire6::kSlotBytes, wire6::kTileLanes;
  using wire6::u32x6, wire6::u32x16, wire6::bf16x32, wire6::f32x32, wire6::load_codes, wire6::store_block, wire6::wave_lds_fence;
  // SPLIT: the 4 KiB the bf16 paths need, the image stage in its first 1600 B.
  constexpr uint32_t kSlot = SPLIT ? kSlotBytes : 64u, kScaleAt = SPLIT ? kCodeStage : 0u;
  __shared__ __attribute__((aligned(16))) char slots[(kLanes / 64) * kSlot];
  // The wave index as a scalar: the tile, its descriptors and the loop are uniform per wave.
  const uint32_t lane = threadIdx.x & 63u, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const uint32_t wave_block = 64u * (wave % (kTileLanes / 64u));  // 0 or 64
  const uint32_t blk = wave_block + lane;                         // the lane's block of its tile
  char* slot = slots + wave * kSlot;

  for (uint64_t t = static_cast<uint64_t>(blockIdx.x) * kTilesPerGroup + wave / (kTileLanes / 64u); t < a.ntiles;
       t += static_cast<uint64_t>(gridDim.x) * kTilesPerGroup) {
    const uint32_t nb = t + 1 == a.ntiles ? a.last_blocks : kWireTileBlocks;
    const uint32_t soff = wire_tile_scale_offset(nb, kF);
    const bool in = blk < nb;
    u32x6 codes[K];
    uint32_t sb[K];
    constexpr int K0 = OWN ? 1 : 0;  // the first source that is an image
    u32x4 own[4];
    if constexpr (OWN) wire6::load_block<SPLIT>(own, a.src[0] + t * kWireTilePayload, nb, wave_block, lane);
    if ((a.coherent & ((1u << K) - 1u)) == 0) {
      // Every image is local: a lane past the tile's end re-reads its first block.
      const uint32_t at = in ? kEB * blk : 0, sat = soff + (in ? blk : 0);
#pragma unroll
      for (int k = K0; k < K; ++k) {
        const char* ws = a.src[k] + t * kFullTile;
        codes[k] = load_codes(ws + at);
        sb[k] = reinterpret_cast<const uint8_t*>(ws)[sat];
      }
    } else {
      // One range-checked descriptor per source and tile; a lane past the end
      // aims at its end and loads 0.  The uniform branch picks the cache policy.
      const int at = static_cast<int>(in ? kEB * blk : soff + nb), sat = static_cast<int>(soff + blk);
#pragma unroll
      for (int k = K0; k < K; ++k) {
        auto rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<char*>(a.src[k] + t * kFullTile), 0,
                                                    static_cast<int>(soff + nb), kRsrcFlags);
        if ((a.coherent >> k) & 1u) {
          codes[k] = load_codes<kSystemCoherent>(rs, at);
          sb[k] = __builtin_amdgcn_raw_buffer_load_b8(rs, sat, 0, kSystemCoherent);
        } else {
          codes[k] = load_codes<kNonTemporal>(rs, at);
          sb[k] = __builtin_amdgcn_raw_buffer_load_b8(rs, sat, 0, kNonTemporal);
        }
      }
    }
    f32x32 acc;
    if constexpr (OWN) {
      wire6::load_block_rows<SPLIT>(own, lane, slot);
#pragma unroll
      for (int j = 0; j < 16; ++j) {
        acc[2 * j] = __builtin_bit_cast(float, own[j / 4][j % 4] << 16);
        acc[2 * j + 1] = __builtin_bit_cast(float, own[j / 4][j % 4] & 0xFFFF0000u);
      }
    } else {
      acc = __builtin_amdgcn_cvt_scalef32_pk32_f32_fp6(codes[0], scale_operand(sb[0]));
    }
#pragma unroll
    for (int k = 1; k < K; ++k) {
      const f32x32 x = __builtin_amdgcn_cvt_scalef32_pk32_f32_fp6(codes[k], scale_operand(sb[k]));
#pragma unroll
      for (int j = 0; j < 32; ++j) acc[j] = acc[j] + x[j];
    }
    // One rounding to bf16, the block's amax of the rounded values, its codes: all in the lane.
    u32x16 h;
    uint32_t amax = 0;
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      h[j] = reduce_pack_bf16(acc[2 * j], acc[2 * j + 1]);
      amax = max(amax, wire_word_amax(h[j]));
    }
    const uint32_t osb = wire_scale_byte(amax, kF);
    // The epilogue's lane index, opaque to the compiler: the LDS and store
    // addresses below are then formed here, where the accumulators are dead,
    // and not hoisted above the tile loop, where they cost the K = 7, 8
    // instantiations their 128-VGPR budget.
    uint32_t el = lane;
    asm volatile("" : "+v"(el));
    u32x6 c = __builtin_amdgcn_cvt_scalef32_pk32_fp6_bf16(__builtin_bit_cast(bf16x32, h), scale_operand(osb));
    char* wt = a.dst + t * kFullTile;
    if constexpr (SPLIT) {
      if (!in) c = u32x6{0, 0, 0, 0, 0, 0};  // a zero row: the padding behind an odd tile's last block
      auto* row = reinterpret_cast<u32x2*>(slot + kEB * el);
      row[0] = u32x2{c[0], c[1]}, row[1] = u32x2{c[2], c[3]}, row[2] = u32x2{c[4], c[5]};
    } else {
      if (in) {
        auto* out = reinterpret_cast<u32x2*>(wt + kEB * (wave_block + el));
        __builtin_nontemporal_store(u32x2{c[0], c[1]}, out);
        __builtin_nontemporal_store(u32x2{c[2], c[3]}, out + 1);
        __builtin_nontemporal_store(u32x2{c[4], c[5]}, out + 2);
        if (blk + 1 == nb && (nb & 1u)) __builtin_nontemporal_store(u32x2{0, 0}, out + 3);
      }
    }
    reinterpret_cast<uint8_t*>(slot)[kScaleAt + el] = in ? static_cast<uint8_t>(osb) : 0;
    wave_lds_fence();
    const u32x4 sv = *reinterpret_cast<const u32x4*>(slot + kScaleAt + 16u * (el & 3u));
    if constexpr (SPLIT) {
      // Chunk i of the wave's codes: bytes 16 i .. 16 i + 15 behind block wave_block.
      const u32x4 o0 = *reinterpret_cast<const u32x4*>(slot + 16u * el);
      const u32x4 o1 = *reinterpret_cast<const u32x4*>(slot + 1024u + 16u * (el & 31u));
      wave_lds_fence();  // the bf16 stage's writes stay behind these reads
      const uint32_t off0 = kEB * wave_block + 16u * el, off1 = off0 + 1024u;
      if (off0 < soff) __builtin_nontemporal_store(o0, reinterpret_cast<u32x4*>(wt + off0));
      if (el < 32u && off1 < soff) __builtin_nontemporal_store(o1, reinterpret_cast<u32x4*>(wt + off1));
    } else {
      wave_lds_fence();  // the next tile's byte stays behind this read
    }
    if (el < 4u && wave_block + 16u * el < nb)
      __builtin_nontemporal_store(sv, reinterpret_cast<u32x4*>(wt + soff + wave_block + 16u * el));
    if constexpr (BOTH) {
      const u32x16 r = __builtin_bit_cast(u32x16, __builtin_amdgcn_cvt_scalef32_pk32_bf16_fp6(c, scale_operand(osb)));
      const u32x4 v[4] = {{r[0], r[1], r[2], r[3]}, {r[4], r[5], r[6], r[7]}, {r[8], r[9], r[10], r[11]}, {r[12], r[13], r[14], r[15]}};
      store_block<SPLIT>(v, a.dst_bf16 + t * kWireTilePayload, nb, wave_block, el, false, slot);
    }
  }
}

template <bool SPLIT, bool OWN, bool BOTH, int K = kMaxWireReduceSrcs>
void launch_k(int nsrc, uint32_t groups, const ReducePack6Args& a, hipStream_t stream) {
  if constexpr (K < 1) {
    P2P_FATAL("wire_reduce_packed: an op needs 1..8 sources");
  } else {
    if (nsrc == K)
      wire_reduce_pack6_kernel<K, SPLIT, OWN, BOTH><<<groups, wire6::kLanes, 0, stream>>>(a);
    else
      launch_k<SPLIT, OWN, BOTH, K - 1>(nsrc, groups, a, stream);
  }
}
template <bool BOTH>
void launch_o(bool split, bool own, int nsrc, uint32_t groups, const ReducePack6Args& a, hipStream_t stream) {
  if (own) {
    if (split) launch_k<true, true, BOTH>(nsrc, groups, a, stream);
    else launch_k<false, true, BOTH>(nsrc, groups, a, stream);
  } else {
    if (split) launch_k<true, false, BOTH>(nsrc, groups, a, stream);
    else launch_k<false, false, BOTH>(nsrc, groups, a, stream);
  }
}

}  // namespace

// op has passed launch_wire_reduce_packed's checks and has a payload.
void launch_wire_reduce_packed6(const WireReduceOp& op, hipStream_t stream, int max_blocks, WireLanes lanes) {
  ReducePack6Args a{};
  for (int k = 0; k < op.nsrc; ++k) a.src[k] = static_cast<const char*>(op.src[k]);
  a.dst = static_cast<char*>(op.dst);
  a.dst_bf16 = static_cast<char*>(op.dst_bf16);
  a.ntiles = (op.payload_bytes + kWireTilePayload - 1) / kWireTilePayload;
  const size_t rest = op.payload_bytes % kWireTilePayload;
  a.last_blocks = static_cast<uint32_t>(rest ? rest / kWireBlockBytes : kWireTileBlocks);
  a.coherent = op.coherent_mask;
  const uint64_t cap = max_blocks > 0 ? static_cast<uint64_t>(max_blocks) : kMaxGrid;
  const uint32_t grid = static_cast<uint32_t>(std::min(a.ntiles, cap));
  const uint32_t groups = (grid + wire6::kTilesPerGroup - 1) / wire6::kTilesPerGroup;
  // Auto: split, measured 18-71% faster than contiguous with both outputs in every cell (docs/DESIGN.md).  The image
  // alone was not measured on its own and takes the same mapping.
  const bool split = lanes == WireLanes::Auto ? true : lanes == WireLanes::Split;
  if (op.dst_bf16) launch_o<true>(split, op.own_bf16, op.nsrc, groups, a, stream);
  else launch_o<false>(split, op.own_bf16, op.nsrc, groups, a, stream);
  HIPCHECK(hipGetLastError());
}

}  // namespace dev
}  // namespace p2p
