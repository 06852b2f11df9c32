// gfx950 kernels of the block-scaled wire formats (--wire): the pull engine's
// receive that widens MXFP8 / MXFP6 / MXFP4 to bf16, the sender's pack (from bf16 or
// straight from the operand stream) and the check of an unpacked buffer.
// kernels.hpp has the contract, wire_op.hpp the format and the arithmetic.
// Design:
//   * The unit of work is a tile: 128 blocks, 8 KiB of bf16, 4224 B (mxfp8) or
//     2176 B (mxfp4) on the wire.  A workgroup takes whole tiles, 16 elements
//     per lane, so every lane ends in two 16 B stores whatever the format.
//   * Unpack reads 1/2 or 1/4 of what it writes: the stores decide its rate,
//     so the lane mapping is chosen for them.  SPLIT: a lane takes 8 elements
//     at 8L and 8 at 8L + 2048 (two 8 B / 4 B loads) and its two stores are
//     fully coalesced, 1 KiB per wave and instruction.  Contiguous: a lane
//     takes 16 elements at 16L (one 16 B / 8 B load) and each of its stores
//     has a 32 B lane stride.  Both are built; docs/DESIGN.md has the numbers.
//   * Scale bytes: one byte load per lane and unit, from the tile's own
//     descriptor.  The 2 or 4 lanes of a block read the same byte and the 128
//     bytes of a tile are one or two cache lines, so the load unit merges
//     them; the loads are issued with the element loads and the wave waits
//     once.  Spreading one 16 B load of 8 lanes through LDS would add a
//     barrier between the loads and the conversions of every tile.
//   * byte << 23 is the f32 scale operand of v_cvt_scalef32_pk_bf16_fp8 / _fp4
//     (unpack) and of v_cvt_scalef32_pk_fp8_bf16 / _fp4_bf16 (pack).
//   * Pack: amax is an integer max of magnitudes in the lane, one xor shuffle
//     across the 2 lanes of an mxfp8 block; the scale bytes of a tile are
//     staged in LDS and leave as 16 B stores of 8 lanes.
//   * mxfp6 converts a whole block per lane and instruction, so it has
//     kernels of its own below (multi_unpack6_kernel, pack6_kernel) behind the
//     same launchers; wire6_lane.hpp has their design.
//   * No packed f32 instructions in this object (Makefile).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <vector>

#include "block_split.hpp"
#include "common.hpp"
#include "hip_check.hpp"
#include "kernels.hpp"
#include "wire6_lane.hpp"

namespace p2p {
namespace dev {

namespace {

typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef short i16x2 __attribute__((ext_vector_type(2)));

constexpr int kBlock = 256;
constexpr int kWaves = kBlock / 64;
constexpr uint64_t kMaxGrid = 1ull << 20;  // tiles per grid pass (8 GiB of payload)
constexpr int kVerifyPerCu = 16;           // verify_unpacked: workgroups per CU, grid-stride beyond
constexpr int kPackPerCu = 16;
// Cache-policy bits, descriptor word and scale operand: one definition for this file and wire_reduce.hip.
using wire6::kRsrcFlags;
using wire6::kSystemCoherent;

// The narrowing instructions divide by their scale operand and round to
// nearest even, the target's subnormals included: compared on a GPU, they
// agree with wire_quantize on every bf16 under every scale byte for which
// the quotient is inside the format (docs/DESIGN.md), so no step of the pack
// needs the integer arithmetic.
using wire6::scale_operand;

// ------------------------------------------------------------------ unpack ----

// By value in the kernarg segment, like the copy's CopyArgs (about 1 KiB).
struct UnpackArgs {
  const char* src[kMaxUnpackOps];
  char* dst[kMaxUnpackOps];
  uint64_t ntiles[kMaxUnpackOps];
  uint32_t last_blocks[kMaxUnpackOps];  // blocks of the last tile, 1..128
  uint32_t block_begin[kMaxUnpackOps + 1];
  uint32_t src_coherent, dst_coherent;  // one bit per op
  int nops;
  int32_t uniform;  // > 0: every op has this many workgroups (one division); 0: binary search
};

// 8 codes -> 8 bf16 (one 16 B vector).  mxfp8: w[0] and w[1]; mxfp4: w[0].
template <WireFormat F>
__device__ __forceinline__ u32x4 widen8(const uint32_t (&w)[2], float scale) {
  bf16x2 r[4];
  if constexpr (F == WireFormat::Mxfp8) {
    r[0] = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(w[0], scale, false);
    r[1] = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(w[0], scale, true);
    r[2] = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(w[1], scale, false);
    r[3] = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(w[1], scale, true);
  } else {
    r[0] = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(w[0], scale, 0);
    r[1] = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(w[0], scale, 1);
    r[2] = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(w[0], scale, 2);
    r[3] = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(w[0], scale, 3);
  }
  return u32x4{__builtin_bit_cast(uint32_t, r[0]), __builtin_bit_cast(uint32_t, r[1]), __builtin_bit_cast(uint32_t, r[2]),
               __builtin_bit_cast(uint32_t, r[3])};
}

template <WireFormat F, bool SPLIT>
__global__ __launch_bounds__(kBlock) void multi_unpack_kernel(const UnpackArgs a) {
  constexpr uint32_t EB = wire_block_elem_bytes(F);
  constexpr uint32_t kFullTile = wire_tile_bytes(kWireTileBlocks, F);
  constexpr bool FP8 = F == WireFormat::Mxfp8;
  int op = 0;
  if (a.uniform > 0) {
    op = min(static_cast<int>(blockIdx.x / static_cast<uint32_t>(a.uniform)), a.nops - 1);
  } else {
    int lo = 0, hi = a.nops - 1;  // largest op with block_begin[op] <= blockIdx.x
    while (lo < hi) {
      const int mid = (lo + hi + 1) >> 1;
      if (blockIdx.x >= a.block_begin[mid]) lo = mid; else hi = mid - 1;
    }
    op = lo;
  }
  const uint32_t b = blockIdx.x - a.block_begin[op];
  const uint32_t nwg = a.block_begin[op + 1] - a.block_begin[op];
  const uint64_t ntiles = a.ntiles[op];
  const bool src_coh = (a.src_coherent >> op) & 1u, dst_coh = (a.dst_coherent >> op) & 1u;
  const uint32_t L = threadIdx.x;
  // The lane's two units of 8 elements: element offsets inside the tile.
  const uint32_t e0 = SPLIT ? 8u * L : 16u * L;
  const uint32_t e1 = SPLIT ? 8u * L + 2048u : 16u * L + 8u;

  for (uint64_t t = b; t < ntiles; t += nwg) {
    // Block-uniform: the tile's blocks and the ranges of its descriptors.
    const uint32_t nb = t + 1 == ntiles ? a.last_blocks[op] : kWireTileBlocks;
    const char* ws = a.src[op] + t * kFullTile;
    char* pd = a.dst[op] + t * kWireTilePayload;
    const uint32_t ebytes = nb * EB;
    const bool in0 = (e0 >> 5) < nb, in1 = (e1 >> 5) < nb;
    // All loads are issued before the first conversion: the wave waits once.
    uint32_t w0[2] = {0, 0}, w1[2] = {0, 0}, s0, s1;
    if (src_coh) {
      // A peer's mapped buffer: system-scope loads through a range-checked
      // descriptor over the tile (elements and scale bytes); a lane past the
      // tile's end loads 0 and stores nothing.
      auto rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<char*>(ws), 0, static_cast<int>(ebytes + nb), kRsrcFlags);
      const int o0 = static_cast<int>(in0 ? (FP8 ? e0 : e0 / 2) : ebytes + nb);
      const int o1 = static_cast<int>(in1 ? (FP8 ? e1 : e1 / 2) : ebytes + nb);
      if constexpr (!SPLIT && FP8) {
        const u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(rs, o0, 0, kSystemCoherent);
        w0[0] = v[0], w0[1] = v[1], w1[0] = v[2], w1[1] = v[3];
      } else if constexpr (SPLIT && FP8) {
        const u32x2 u = __builtin_amdgcn_raw_buffer_load_b64(rs, o0, 0, kSystemCoherent);
        const u32x2 v = __builtin_amdgcn_raw_buffer_load_b64(rs, o1, 0, kSystemCoherent);
        w0[0] = u[0], w0[1] = u[1], w1[0] = v[0], w1[1] = v[1];
      } else if constexpr (!SPLIT) {
        const u32x2 v = __builtin_amdgcn_raw_buffer_load_b64(rs, o0, 0, kSystemCoherent);
        w0[0] = v[0], w1[0] = v[1];
      } else {
        w0[0] = __builtin_amdgcn_raw_buffer_load_b32(rs, o0, 0, kSystemCoherent);
        w1[0] = __builtin_amdgcn_raw_buffer_load_b32(rs, o1, 0, kSystemCoherent);
      }
      s0 = __builtin_amdgcn_raw_buffer_load_b8(rs, static_cast<int>(ebytes + (e0 >> 5)), 0, kSystemCoherent);
      s1 = SPLIT ? __builtin_amdgcn_raw_buffer_load_b8(rs, static_cast<int>(ebytes + (e1 >> 5)), 0, kSystemCoherent) : s0;
    } else {
      // Local memory: non-temporal loads; a lane past the end re-reads the
      // tile's first unit and stores nothing.
      const uint32_t o0 = in0 ? (FP8 ? e0 : e0 / 2) : 0, o1 = in1 ? (FP8 ? e1 : e1 / 2) : 0;
      if constexpr (!SPLIT && FP8) {
        const u32x4 v = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(ws + o0));
        w0[0] = v[0], w0[1] = v[1], w1[0] = v[2], w1[1] = v[3];
      } else if constexpr (SPLIT && FP8) {
        const u32x2 u = __builtin_nontemporal_load(reinterpret_cast<const u32x2*>(ws + o0));
        const u32x2 v = __builtin_nontemporal_load(reinterpret_cast<const u32x2*>(ws + o1));
        w0[0] = u[0], w0[1] = u[1], w1[0] = v[0], w1[1] = v[1];
      } else if constexpr (!SPLIT) {
        const u32x2 v = __builtin_nontemporal_load(reinterpret_cast<const u32x2*>(ws + o0));
        w0[0] = v[0], w1[0] = v[1];
      } else {
        w0[0] = __builtin_nontemporal_load(reinterpret_cast<const uint32_t*>(ws + o0));
        w1[0] = __builtin_nontemporal_load(reinterpret_cast<const uint32_t*>(ws + o1));
      }
      const auto* sc = reinterpret_cast<const uint8_t*>(ws + ebytes);
      s0 = sc[in0 ? e0 >> 5 : 0];
      s1 = SPLIT ? sc[in1 ? e1 >> 5 : 0] : s0;
    }
    const u32x4 r0 = widen8<F>(w0, scale_operand(s0));
    const u32x4 r1 = widen8<F>(w1, scale_operand(s1));
    if (dst_coh) {
      auto rd = __builtin_amdgcn_make_buffer_rsrc(pd, 0, static_cast<int>(nb * kWireBlockBytes), kRsrcFlags);
      __builtin_amdgcn_raw_buffer_store_b128(r0, rd, static_cast<int>(2 * e0), 0, kSystemCoherent);  // past the end: dropped
      __builtin_amdgcn_raw_buffer_store_b128(r1, rd, static_cast<int>(2 * e1), 0, kSystemCoherent);
    } else {
      if (in0) __builtin_nontemporal_store(r0, reinterpret_cast<u32x4*>(pd + 2 * e0));
      if (in1) __builtin_nontemporal_store(r1, reinterpret_cast<u32x4*>(pd + 2 * e1));
    }
  }
}

// mxfp6: a lane owns a block (wire6_lane.hpp has the geometry and the store
// paths).  The same op table, lookup and grid-stride passes; a workgroup's
// pass is kTilesPerGroup tiles, and its waves never meet: no barrier.
template <bool SPLIT>
__global__ __launch_bounds__(wire6::kLanes) void multi_unpack6_kernel(const UnpackArgs a) {
  using wire6::kF, wire6::kEB, wire6::kFullTile, wire6::kLanes, wire6::kTilesPerGroup, wire6::kSlotBytes, wire6::kTileLanes;
  using wire6::u32x6, wire6::u32x16, wire6::load_codes, wire6::store_block;
  __shared__ __attribute__((aligned(16))) char slots[SPLIT ? (kLanes / 64) * kSlotBytes : 16];
  int op = 0;
  if (a.uniform > 0) {
    op = min(static_cast<int>(blockIdx.x / static_cast<uint32_t>(a.uniform)), a.nops - 1);
  } else {
    int lo = 0, hi = a.nops - 1;  // largest op with block_begin[op] <= blockIdx.x
    while (lo < hi) {
      const int mid = (lo + hi + 1) >> 1;
      if (blockIdx.x >= a.block_begin[mid]) lo = mid; else hi = mid - 1;
    }
    op = lo;
  }
  const uint32_t b = blockIdx.x - a.block_begin[op];
  const uint32_t nwg = a.block_begin[op + 1] - a.block_begin[op];
  const uint64_t ntiles = a.ntiles[op];
  const bool src_coh = (a.src_coherent >> op) & 1u, dst_coh = (a.dst_coherent >> op) & 1u;
  // The wave index as a scalar: the tile, its descriptors and the loop are uniform per wave.
  const uint32_t lane = threadIdx.x & 63u, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const uint32_t wave_block = 64u * (wave % (kTileLanes / 64u));  // 0 or 64
  const uint32_t blk = wave_block + lane;                         // the lane's block of its tile
  char* slot = slots + (SPLIT ? wave * kSlotBytes : 0);

  for (uint64_t t = static_cast<uint64_t>(b) * kTilesPerGroup + wave / (kTileLanes / 64u); t < ntiles;
       t += static_cast<uint64_t>(nwg) * kTilesPerGroup) {
    // Uniform per wave: the tile's blocks and the ranges of its descriptors.
    const uint32_t nb = t + 1 == ntiles ? a.last_blocks[op] : kWireTileBlocks;
    const uint32_t soff = wire_tile_scale_offset(nb, kF);
    const char* ws = a.src[op] + t * kFullTile;
    const bool in = blk < nb;
    u32x6 codes;
    uint32_t sb;
    if (src_coh) {
      auto rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<char*>(ws), 0, static_cast<int>(soff + nb), kRsrcFlags);
      codes = load_codes<kSystemCoherent>(rs, static_cast<int>(in ? kEB * blk : soff + nb));
      sb = __builtin_amdgcn_raw_buffer_load_b8(rs, static_cast<int>(soff + blk), 0, kSystemCoherent);
    } else {
      codes = load_codes(ws + (in ? kEB * blk : 0));
      sb = reinterpret_cast<const uint8_t*>(ws + soff)[in ? blk : 0];
    }
    const u32x16 r = __builtin_bit_cast(u32x16, __builtin_amdgcn_cvt_scalef32_pk32_bf16_fp6(codes, scale_operand(sb)));
    const u32x4 v[4] = {{r[0], r[1], r[2], r[3]}, {r[4], r[5], r[6], r[7]}, {r[8], r[9], r[10], r[11]}, {r[12], r[13], r[14], r[15]}};
    store_block<SPLIT>(v, a.dst[op] + t * kWireTilePayload, nb, wave_block, lane, dst_coh, slot);
  }
}

// -------------------------------------------------------------------- pack ----

// Two bf16 words (4 elements, mxfp8) or four (8 elements, mxfp4) -> one word of codes.
template <WireFormat F>
__device__ __forceinline__ uint32_t narrow_word(const uint32_t* w, uint32_t sb) {
  if constexpr (F == WireFormat::Mxfp8) {
    const float scale = scale_operand(sb);
    i16x2 o = {0, 0};
    o = __builtin_amdgcn_cvt_scalef32_pk_fp8_bf16(o, __builtin_bit_cast(bf16x2, w[0]), scale, false);
    o = __builtin_amdgcn_cvt_scalef32_pk_fp8_bf16(o, __builtin_bit_cast(bf16x2, w[1]), scale, true);
    return __builtin_bit_cast(uint32_t, o);
  } else {
    const float scale = scale_operand(sb);
    uint32_t o = 0;
    o = __builtin_amdgcn_cvt_scalef32_pk_fp4_bf16(o, __builtin_bit_cast(bf16x2, w[0]), scale, 0);
    o = __builtin_amdgcn_cvt_scalef32_pk_fp4_bf16(o, __builtin_bit_cast(bf16x2, w[1]), scale, 1);
    o = __builtin_amdgcn_cvt_scalef32_pk_fp4_bf16(o, __builtin_bit_cast(bf16x2, w[2]), scale, 2);
    o = __builtin_amdgcn_cvt_scalef32_pk_fp4_bf16(o, __builtin_bit_cast(bf16x2, w[3]), scale, 3);
    return o;
  }
}

// Lanes of a tile: a lane loads the bf16 vectors that yield one 16 B element
// store, 2 (half a block) for mxfp8 and 4 (a block) for mxfp4.
template <WireFormat F>
constexpr int pack_lanes() { return F == WireFormat::Mxfp8 ? 256 : 128; }

template <WireFormat F, bool FROM_PRNG>
__global__ __launch_bounds__(pack_lanes<F>()) void pack_kernel(const u32x4* __restrict__ payload, char* __restrict__ wire,
                                                               uint64_t ntiles, uint32_t last_blocks, uint64_t seed) {
  constexpr uint32_t EB = wire_block_elem_bytes(F);
  constexpr uint32_t kFullTile = wire_tile_bytes(kWireTileBlocks, F);
  constexpr bool FP8 = F == WireFormat::Mxfp8;
  constexpr int NV = FP8 ? 2 : 4;  // 16 B payload vectors per lane
  __shared__ __attribute__((aligned(16))) uint8_t scales[kWireTileBlocks];
  const uint32_t L = threadIdx.x;
  const uint32_t block = FP8 ? L / 2 : L;
  for (uint64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
    const uint32_t nb = t + 1 == ntiles ? last_blocks : kWireTileBlocks;
    const bool mine = block < nb;
    uint32_t w[4 * NV];
    if constexpr (FROM_PRNG) {
      const uint64_t word0 = t * (kWireTilePayload / 4);  // a tile never straddles a 2^32-word key span
      const uint32_t key = prng_key(seed, word0);         // block-uniform: scalar ALU
#pragma unroll
      for (int i = 0; i < 4 * NV; ++i) {
        const uint64_t at = word0 + 4 * NV * L + i;
        w[i] = wire_operand_word(prng_word_k(key, static_cast<uint32_t>(at)), at);
      }
    } else {
      u32x4 v[NV];
#pragma unroll
      for (int i = 0; i < NV; ++i)  // a lane past the end re-reads the tile's first vector
        v[i] = __builtin_nontemporal_load(payload + t * (kWireTilePayload / 16) + (mine ? NV * L + i : 0));
#pragma unroll
      for (int i = 0; i < 4 * NV; ++i) w[i] = v[i / 4][i % 4];
    }
    uint32_t amax = 0;
#pragma unroll
    for (int i = 0; i < 4 * NV; ++i) amax = max(amax, max(w[i] & 0x7FFFu, (w[i] >> 16) & 0x7FFFu));
    if constexpr (FP8) amax = max(amax, static_cast<uint32_t>(__shfl_xor(static_cast<int>(amax), 1, 64)));
    const uint32_t sb = wire_scale_byte(amax, F);
    u32x4 out;
#pragma unroll
    for (int j = 0; j < 4; ++j) out[j] = narrow_word<F>(w + (FP8 ? 2 : 4) * j, sb);
    char* wt = wire + t * kFullTile;
    if (mine) *reinterpret_cast<u32x4*>(wt + 16 * L) = out;
    // The tile's scale bytes and the zero padding behind them, through LDS.
    if (!FP8 || (L & 1u) == 0) scales[block] = mine ? static_cast<uint8_t>(sb) : 0;
    __syncthreads();
    if (L < 8 && 16 * L < nb) *reinterpret_cast<u32x4*>(wt + nb * EB + 16 * L) = *reinterpret_cast<const u32x4*>(scales + 16 * L);
    __syncthreads();
  }
}

// mxfp6: a lane owns a block and a 128-lane workgroup a tile.  16 payload
// words per lane, the amax entirely in the lane, one
// v_cvt_scalef32_pk32_fp6_bf16, 24 B of codes at a 24 B lane stride (three
// 8 B stores; a wave's codes are contiguous).  The 8 B of zeros behind an odd
// tile's element section come from lane 0, the scale bytes and the zeros
// behind them through LDS as 16 B stores.  Not tuned: it is the sender's step.
template <bool FROM_PRNG>
__global__ __launch_bounds__(wire6::kTileLanes) void pack6_kernel(const u32x4* __restrict__ payload, char* __restrict__ wire,
                                                                  uint64_t ntiles, uint32_t last_blocks, uint64_t seed) {
  using wire6::kF, wire6::kEB, wire6::kFullTile, wire6::u32x6, wire6::u32x16, wire6::bf16x32;
  __shared__ __attribute__((aligned(16))) uint8_t scales[kWireTileBlocks];
  const uint32_t L = threadIdx.x;
  for (uint64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
    const uint32_t nb = t + 1 == ntiles ? last_blocks : kWireTileBlocks;
    const bool mine = L < nb;
    u32x16 w;
    if constexpr (FROM_PRNG) {
      const uint64_t word0 = t * (kWireTilePayload / 4);  // a tile never straddles a 2^32-word key span
      const uint32_t key = prng_key(seed, word0);         // block-uniform: scalar ALU
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const uint64_t at = word0 + 16 * L + i;
        w[i] = wire_operand_word(prng_word_k(key, static_cast<uint32_t>(at)), at);
      }
    } else {
#pragma unroll
      for (int i = 0; i < 4; ++i) {  // a lane past the end re-reads the tile's first block
        const u32x4 v = __builtin_nontemporal_load(payload + t * (kWireTilePayload / 16) + (mine ? 4 * L + i : i));
        w[4 * i] = v[0], w[4 * i + 1] = v[1], w[4 * i + 2] = v[2], w[4 * i + 3] = v[3];
      }
    }
    uint32_t amax = 0;
#pragma unroll
    for (int i = 0; i < 16; ++i) amax = max(amax, max(w[i] & 0x7FFFu, (w[i] >> 16) & 0x7FFFu));
    const uint32_t sb = wire_scale_byte(amax, kF);
    const u32x6 c = __builtin_amdgcn_cvt_scalef32_pk32_fp6_bf16(__builtin_bit_cast(bf16x32, w), scale_operand(sb));
    char* wt = wire + t * kFullTile;
    if (mine) {
      auto* out = reinterpret_cast<u32x2*>(wt + kEB * L);
      out[0] = u32x2{c[0], c[1]}, out[1] = u32x2{c[2], c[3]}, out[2] = u32x2{c[4], c[5]};
    }
    if (L == 0 && (nb & 1u)) *reinterpret_cast<u32x2*>(wt + kEB * nb) = u32x2{0, 0};
    scales[L] = mine ? static_cast<uint8_t>(sb) : 0;
    __syncthreads();
    if (L < 8 && 16 * L < nb)
      *reinterpret_cast<u32x4*>(wt + wire_tile_scale_offset(nb, kF) + 16 * L) = *reinterpret_cast<const u32x4*>(scales + 16 * L);
    __syncthreads();
  }
}

// --------------------------------------------------------- verify unpacked ----

struct Partial {
  unsigned long long mism, sum, first;
};

// The verify kernels' geometry: one 16 B vector per lane, so 4 lanes cover a block.
template <WireFormat F>
__global__ __launch_bounds__(kBlock) void verify_unpacked_kernel(const uint4* __restrict__ p, uint64_t nvec, uint64_t seed,
                                                                 VerifyAccum* __restrict__ out) {
  Partial acc{0, 0, ~0ull};
  for (uint64_t base = static_cast<uint64_t>(blockIdx.x) * kBlock; base < nvec; base += static_cast<uint64_t>(gridDim.x) * kBlock) {
    const uint64_t i = base + threadIdx.x;
    const bool in = i < nvec;  // nvec is a multiple of 4: a block's lanes are all in or all out
    const u32x4 v = in ? __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(p) + i) : u32x4{0, 0, 0, 0};
    const uint32_t key = prng_key(seed, base * 4);  // block-uniform: scalar ALU
    uint32_t w[4], amax = 0;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      w[c] = wire_operand_word(prng_word_k(key, static_cast<uint32_t>(i * 4 + c)), i * 4 + c);
      amax = max(amax, max(w[c] & 0x7FFFu, (w[c] >> 16) & 0x7FFFu));
    }
    amax = max(amax, static_cast<uint32_t>(__shfl_xor(static_cast<int>(amax), 1, 64)));
    amax = max(amax, static_cast<uint32_t>(__shfl_xor(static_cast<int>(amax), 2, 64)));
    const uint32_t sb = wire_scale_byte(amax, F);
    if (in) {
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        acc.sum += v[c];
        if (v[c] != wire_roundtrip_word(w[c], sb, F)) {
          acc.mism += 1;
          acc.first = min(acc.first, static_cast<unsigned long long>(i * 16 + 4 * c));
        }
      }
    }
  }
  // kernels.hip block_commit: wave butterfly, the 4 waves through LDS, one
  // atomic per non-zero field into this block's shard.
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    acc.mism += __shfl_xor(acc.mism, off, 64);
    acc.sum += __shfl_xor(acc.sum, off, 64);
    acc.first = min(acc.first, __shfl_xor(acc.first, off, 64));
  }
  __shared__ Partial red[kWaves];
  if ((threadIdx.x & 63) == 0) red[threadIdx.x / 64] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    Partial t = red[0];
#pragma unroll
    for (int w = 1; w < kWaves; ++w) {
      t.mism += red[w].mism;
      t.sum += red[w].sum;
      t.first = min(t.first, red[w].first);
    }
    VerifyAccum* sh = out + (blockIdx.x % kVerifyShards);
    if (t.sum) atomicAdd(&sh->checksum, t.sum);
    if (t.mism) {
      atomicAdd(&sh->mismatches, t.mism);
      atomicMin(&sh->first_bad, t.first);
    }
  }
}

// ------------------------------------------------------------------ launch ----

void check_format(WireFormat f, size_t n, const char* who) {
  P2P_CHECK(wire_format_valid(f), std::string(who) + ": the format is " + kWireFormatList);
  P2P_CHECK(n % kWireBlockBytes == 0, std::string(who) + ": the payload must be a multiple of 64 bytes (blocks of 32 bf16)");
}

uint64_t tiles_of(size_t n) { return (n + kWireTilePayload - 1) / kWireTilePayload; }
uint32_t last_blocks_of(size_t n) {
  const size_t rest = n % kWireTilePayload;
  return static_cast<uint32_t>(rest ? rest / kWireBlockBytes : kWireTileBlocks);
}

// One launch: cnt <= kMaxUnpackOps ops.
void launch_unpack_group(const UnpackOp* ops, int cnt, WireFormat fmt, hipStream_t stream, int max_blocks, WireLanes lanes) {
  UnpackArgs a{};
  a.nops = cnt;
  for (int i = 0; i < cnt; ++i) {
    const UnpackOp& o = ops[i];
    check_format(fmt, o.payload_bytes, "multi_unpack");
    P2P_CHECK(reinterpret_cast<uintptr_t>(o.dst) % 16 == 0 && reinterpret_cast<uintptr_t>(o.src) % 16 == 0,
              "multi_unpack: 16-byte aligned buffers required");
    a.src[i] = static_cast<const char*>(o.src);
    a.dst[i] = static_cast<char*>(o.dst);
    a.ntiles[i] = tiles_of(o.payload_bytes);
    a.last_blocks[i] = last_blocks_of(o.payload_bytes);
    if (o.coherent) a.src_coherent |= 1u << i;
    if (o.dst_coherent) a.dst_coherent |= 1u << i;
  }
  const uint64_t cap = max_blocks > 0 ? static_cast<uint64_t>(max_blocks) : kMaxGrid;
  const uint32_t grid = split_blocks(a.ntiles, cnt, fmt == WireFormat::Mxfp6 ? wire6::kTilesPerGroup : 1, cap, a.block_begin);
  a.uniform = static_cast<int32_t>(a.block_begin[1] - a.block_begin[0]);
  for (int i = 1; i < cnt; ++i)
    if (a.block_begin[i + 1] - a.block_begin[i] != static_cast<uint32_t>(a.uniform)) a.uniform = 0;
  // Auto: the mapping measured faster per format (docs/DESIGN.md).
  const bool split = lanes == WireLanes::Auto ? true : lanes == WireLanes::Split;
  if (fmt == WireFormat::Mxfp6) {
    if (split) multi_unpack6_kernel<true><<<grid, wire6::kLanes, 0, stream>>>(a);
    else multi_unpack6_kernel<false><<<grid, wire6::kLanes, 0, stream>>>(a);
  } else if (fmt == WireFormat::Mxfp8) {
    if (split) multi_unpack_kernel<WireFormat::Mxfp8, true><<<grid, kBlock, 0, stream>>>(a);
    else multi_unpack_kernel<WireFormat::Mxfp8, false><<<grid, kBlock, 0, stream>>>(a);
  } else {
    if (split) multi_unpack_kernel<WireFormat::Mxfp4, true><<<grid, kBlock, 0, stream>>>(a);
    else multi_unpack_kernel<WireFormat::Mxfp4, false><<<grid, kBlock, 0, stream>>>(a);
  }
  HIPCHECK(hipGetLastError());
}

template <bool FROM_PRNG>
void launch_pack_impl(void* wire, const void* payload, size_t n, uint64_t seed, WireFormat fmt, hipStream_t stream, const char* who) {
  check_format(fmt, n, who);
  if (!n) return;
  P2P_CHECK(reinterpret_cast<uintptr_t>(wire) % 16 == 0 && reinterpret_cast<uintptr_t>(payload) % 16 == 0,
            std::string(who) + ": 16-byte aligned buffers required");
  const uint64_t ntiles = tiles_of(n);
  const unsigned grid = static_cast<unsigned>(std::min<uint64_t>(ntiles, static_cast<uint64_t>(cu_count()) * kPackPerCu));
  const auto* src = static_cast<const u32x4*>(payload);
  auto* dst = static_cast<char*>(wire);
  if (fmt == WireFormat::Mxfp6)
    pack6_kernel<FROM_PRNG><<<grid, wire6::kTileLanes, 0, stream>>>(src, dst, ntiles, last_blocks_of(n), seed);
  else if (fmt == WireFormat::Mxfp8)
    pack_kernel<WireFormat::Mxfp8, FROM_PRNG><<<grid, pack_lanes<WireFormat::Mxfp8>(), 0, stream>>>(src, dst, ntiles, last_blocks_of(n), seed);
  else
    pack_kernel<WireFormat::Mxfp4, FROM_PRNG><<<grid, pack_lanes<WireFormat::Mxfp4>(), 0, stream>>>(src, dst, ntiles, last_blocks_of(n), seed);
  HIPCHECK(hipGetLastError());
}

}  // namespace

void launch_multi_unpack(const UnpackOp* ops, int nops, WireFormat fmt, hipStream_t stream, int max_blocks, WireLanes lanes) {
  for (int i = 0; i < nops; i += kMaxUnpackOps)
    launch_unpack_group(ops + i, std::min(kMaxUnpackOps, nops - i), fmt, stream, max_blocks, lanes);
}

void launch_pack(void* wire, const void* payload, size_t payload_bytes, WireFormat fmt, hipStream_t stream) {
  launch_pack_impl<false>(wire, payload, payload_bytes, 0, fmt, stream, "wire_pack");
}

void launch_fill_packed(void* wire, size_t payload_bytes, uint64_t seed, WireFormat fmt, hipStream_t stream) {
  launch_pack_impl<true>(wire, wire, payload_bytes, seed, fmt, stream, "fill_packed");
}

void launch_verify_unpacked(const void* p, size_t payload_bytes, uint64_t seed, WireFormat fmt, VerifyAccum* acc,
                            hipStream_t stream) {
  check_format(fmt, payload_bytes, "verify_unpacked");
  if (payload_bytes) {
    P2P_CHECK(reinterpret_cast<uintptr_t>(p) % 16 == 0, "verify_unpacked: buffer must be 16-byte aligned");
    const uint64_t nvec = payload_bytes / 16;
    const uint64_t cap = static_cast<uint64_t>(cu_count()) * kVerifyPerCu;
    const unsigned grid = static_cast<unsigned>(std::max<uint64_t>(1, std::min((nvec + kBlock - 1) / kBlock, cap)));
    const auto* vp = static_cast<const uint4*>(p);
    if (fmt == WireFormat::Mxfp8)
      verify_unpacked_kernel<WireFormat::Mxfp8><<<grid, kBlock, 0, stream>>>(vp, nvec, seed, acc);
    else if (fmt == WireFormat::Mxfp6)
      verify_unpacked_kernel<WireFormat::Mxfp6><<<grid, kBlock, 0, stream>>>(vp, nvec, seed, acc);
    else
      verify_unpacked_kernel<WireFormat::Mxfp4><<<grid, kBlock, 0, stream>>>(vp, nvec, seed, acc);
    HIPCHECK(hipGetLastError());
  }
  // The finalize of launch_verify (zero bytes: nothing else runs): shards -> acc[0].
  launch_verify(nullptr, 0, 0, acc, VerifyImpl::Auto, false, stream);
}

}  // namespace dev
}  // namespace p2p
