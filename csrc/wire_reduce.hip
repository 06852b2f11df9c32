// gfx950 kernels of --reduce-wire: the pull engine's receive that sums K
// MXFP8 / MXFP4 wire images into bf16 in one launch, and the check of such a
// sum.  kernels.hpp has the contract, wire_reduce_op.hpp the arithmetic and
// its range argument, wire_op.hpp the format.  Design:
//   * The unit of work is the wire tile: 128 blocks, 8 KiB of bf16 out, K x
//     4224 B (mxfp8) or K x 2176 B (mxfp4) in.  A 256-thread workgroup takes
//     whole tiles, 16 elements per lane, and every lane ends in two 16 B
//     non-temporal stores.  One op per launch: no workgroup -> op lookup.
//   * The loads decide (K = 8 reads 4.1x / 2.1x what it writes).  Fan-in K and
//     format are template parameters: a lane issues the K element loads and
//     the K scale-byte loads of a tile back to back into registers nothing
//     else writes (no zero-fill, see reduce.hip), and only then converts, so
//     the wave waits once per tile.  K = 8, mxfp8: 32 + 16 VGPRs of operands.
//   * A peer's image is read with system-scope (sc0 sc1) raw-buffer loads
//     through one range-checked descriptor per source and tile that covers the
//     elements and the scale bytes; a local image with non-temporal loads.
//     All images local: straight-line global loads.  Otherwise every source
//     goes through its descriptor and a block-uniform branch per source picks
//     the cache policy only, so both sides load from the same address
//     registers (a branch between a global and a buffer load made the
//     compiler wait for the previous source before the next address).
//   * 16 f32 accumulators per lane: v_cvt_scalef32_pk_f32_fp8 / _fp4 widen two
//     codes under byte << 23 as the scale operand, plain v_add_f32 chains in
//     operand order, one v_cvt_pk_bf16_f32 per output word.
//   * Two lane mappings, as the unpack has.  SPLIT: units of 8 elements at 8L
//     and 8L + 2048 (8 B / 4 B loads, two scale bytes), both stores fully
//     coalesced.  Contiguous: 16 elements at 16L (one 16 B / 8 B load, one
//     scale byte per source), stores with a 32 B lane stride.
//   * Scale bytes: one byte load per lane, unit and source.  No LDS: every
//     byte is used once.
//   * mxfp6 widens a whole block per lane and instruction: wire_reduce6_kernel
//     below, a lane per block and 32 accumulators, behind the same launcher;
//     wire6_lane.hpp has its geometry and its two store paths.
//   * A bf16 own shard (WireReduceOp::own_bf16, --reduce-own bf16): OWN is a
//     template parameter beside K and the format, so the all-image kernels
//     are what they were.  Source 0 is then payload bytes of bf16 in local
//     memory: a lane loads the 16 elements it accumulates as two 16 B
//     non-temporal loads ahead of the images' loads (split: 4 KiB apart, both
//     coalesced, the mirror of the stores; contiguous: its 32 B) and widens
//     them with shifts and masks into the accumulators.  mxfp6, a block per
//     lane: wire6_lane.hpp load_block.
//   * No packed f32 instructions in this object (Makefile): the add chains
//     stay scalar f32 adds.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "common.hpp"
#include "hip_check.hpp"
#include "kernels.hpp"
#include "wire6_lane.hpp"
#include "wire_own_lane.hpp"

namespace p2p {
namespace dev {

namespace {

typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));
typedef float f32x2 __attribute__((ext_vector_type(2)));

constexpr int kBlock = 256;
constexpr int kWaves = kBlock / 64;
constexpr uint64_t kMaxGrid = 1ull << 20;  // tiles per grid pass (8 GiB of payload)
constexpr int kVerifyPerCu = 16;           // verify_wire_reduced: workgroups per CU, grid-stride beyond
// Cache-policy bits, descriptor word and scale operand: one definition for this file and wire.hip.
using wire6::kNonTemporal;
using wire6::kRsrcFlags;
using wire6::kSystemCoherent;

// By value in the kernarg segment.
struct WireReduceArgs {
  const char* src[kMaxWireReduceSrcs];
  char* dst;
  uint64_t ntiles;
  uint32_t last_blocks;  // blocks of the last tile, 1..128
  uint32_t coherent;     // WireReduceOp::coherent_mask
};

using wire6::scale_operand;

// 8 codes (mxfp8: w[0] and w[1]; mxfp4: w[0]) under one scale -> 8 f32.
template <WireFormat F>
__device__ __forceinline__ void widen8(const uint32_t* w, float scale, float (&x)[8]) {
  f32x2 r[4];
  if constexpr (F == WireFormat::Mxfp8) {
    r[0] = __builtin_amdgcn_cvt_scalef32_pk_f32_fp8(w[0], scale, false);
    r[1] = __builtin_amdgcn_cvt_scalef32_pk_f32_fp8(w[0], scale, true);
    r[2] = __builtin_amdgcn_cvt_scalef32_pk_f32_fp8(w[1], scale, false);
    r[3] = __builtin_amdgcn_cvt_scalef32_pk_f32_fp8(w[1], scale, true);
  } else {
    r[0] = __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(w[0], scale, 0);
    r[1] = __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(w[0], scale, 1);
    r[2] = __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(w[0], scale, 2);
    r[3] = __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(w[0], scale, 3);
  }
#pragma unroll
  for (int j = 0; j < 4; ++j) x[2 * j] = r[j][0], x[2 * j + 1] = r[j][1];
}

// A lane's loads from one source's tile through its descriptor: the codes of
// both units and their scale bytes.  AUX: the cache policy of all of them.
template <bool FP8, bool SPLIT, int AUX>
__device__ __forceinline__ void load_desc(__amdgpu_buffer_rsrc_t rs, int r0, int r1, int q0, int q1, uint32_t* w0,
                                          uint32_t* w1, uint32_t& s0, uint32_t& s1) {
  if constexpr (!SPLIT && FP8) {
    const u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(rs, r0, 0, AUX);
    w0[0] = v[0], w0[1] = v[1], w1[0] = v[2], w1[1] = v[3];
  } else if constexpr (SPLIT && FP8) {
    const u32x2 u = __builtin_amdgcn_raw_buffer_load_b64(rs, r0, 0, AUX);
    const u32x2 v = __builtin_amdgcn_raw_buffer_load_b64(rs, r1, 0, AUX);
    w0[0] = u[0], w0[1] = u[1], w1[0] = v[0], w1[1] = v[1];
  } else if constexpr (!SPLIT) {
    const u32x2 v = __builtin_amdgcn_raw_buffer_load_b64(rs, r0, 0, AUX);
    w0[0] = v[0], w1[0] = v[1];
  } else {
    w0[0] = __builtin_amdgcn_raw_buffer_load_b32(rs, r0, 0, AUX);
    w1[0] = __builtin_amdgcn_raw_buffer_load_b32(rs, r1, 0, AUX);
  }
  s0 = __builtin_amdgcn_raw_buffer_load_b8(rs, q0, 0, AUX);
  s1 = SPLIT ? __builtin_amdgcn_raw_buffer_load_b8(rs, q1, 0, AUX) : s0;
}

using wire_own::load_own;  // the own shard's load side: wire_own_lane.hpp
using wire_own::widen_own;

// OWN: source 0 is the receiver's own shard in bf16 (local memory), not an
// image; it begins the chains as it is and sources 1..K-1 follow as before.
template <WireFormat F, int K, bool SPLIT, bool OWN>
__global__ __launch_bounds__(kBlock) void wire_reduce_kernel(const WireReduceArgs a) {
  constexpr uint32_t EB = wire_block_elem_bytes(F);
  constexpr uint32_t kFullTile = wire_tile_bytes(kWireTileBlocks, F);
  constexpr bool FP8 = F == WireFormat::Mxfp8;
  constexpr int EW = FP8 ? 2 : 1;  // 32-bit words of codes per unit of 8 elements
  const uint32_t L = threadIdx.x;
  // The lane's two units of 8 elements: element offsets inside the tile.
  const uint32_t e0 = SPLIT ? 8u * L : 16u * L;
  const uint32_t e1 = SPLIT ? 8u * L + 2048u : 16u * L + 8u;
  const uint32_t c0 = FP8 ? e0 : e0 / 2, c1 = FP8 ? e1 : e1 / 2;  // byte offsets of their codes

  for (uint64_t t = blockIdx.x; t < a.ntiles; t += gridDim.x) {
    // Block-uniform: the tile's blocks and the range of its descriptors.
    const uint32_t nb = t + 1 == a.ntiles ? a.last_blocks : kWireTileBlocks;
    const uint32_t ebytes = nb * EB;
    const bool in0 = (e0 >> 5) < nb, in1 = (e1 >> 5) < nb;
    // All K element loads and all K scale loads are issued before the first
    // conversion, and nothing else writes these registers in between (no
    // zero-fill of the lanes past the end): the wave waits once per tile.
    uint32_t w0[K][EW], w1[K][EW], s0[K], s1[K];
    constexpr int K0 = OWN ? 1 : 0;  // the first source that is an image
    u32x4 h0, h1;                    // OWN: the own shard's 16 elements, issued first
    if constexpr (OWN) load_own(a.src[0] + t * kWireTilePayload, e0, e1, in0, in1, h0, h1);
    if ((a.coherent & ((1u << K) - 1u)) == 0) {
      // Every image is local: straight-line non-temporal loads; a lane past
      // the tile's end re-reads the tile's first unit and stores nothing.
      const uint32_t l0 = in0 ? c0 : 0, l1 = in1 ? c1 : 0;
      const uint32_t b0 = in0 ? e0 >> 5 : 0, b1 = in1 ? e1 >> 5 : 0;
#pragma unroll
      for (int k = K0; k < K; ++k) {
        const char* ws = a.src[k] + t * kFullTile;
        if constexpr (!SPLIT && FP8) {
          const u32x4 v = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(ws + l0));
          w0[k][0] = v[0], w0[k][1] = v[1], w1[k][0] = v[2], w1[k][1] = v[3];
        } else if constexpr (SPLIT && FP8) {
          const u32x2 u = __builtin_nontemporal_load(reinterpret_cast<const u32x2*>(ws + l0));
          const u32x2 v = __builtin_nontemporal_load(reinterpret_cast<const u32x2*>(ws + l1));
          w0[k][0] = u[0], w0[k][1] = u[1], w1[k][0] = v[0], w1[k][1] = v[1];
        } else if constexpr (!SPLIT) {
          const u32x2 v = __builtin_nontemporal_load(reinterpret_cast<const u32x2*>(ws + l0));
          w0[k][0] = v[0], w1[k][0] = v[1];
        } else {
          w0[k][0] = __builtin_nontemporal_load(reinterpret_cast<const uint32_t*>(ws + l0));
          w1[k][0] = __builtin_nontemporal_load(reinterpret_cast<const uint32_t*>(ws + l1));
        }
        const auto* sc = reinterpret_cast<const uint8_t*>(ws + ebytes);
        s0[k] = sc[b0];
        s1[k] = SPLIT ? sc[b1] : s0[k];
      }
    } else {
      // One range-checked descriptor per source over the tile's elements and
      // scale bytes: a lane past the tile's end aims at the descriptor's end,
      // loads 0 and stores nothing.  The block-uniform branch picks the form:
      // system scope for a peer's image, non-temporal for a local one.
      const int r0 = static_cast<int>(in0 ? c0 : ebytes + nb), r1 = static_cast<int>(in1 ? c1 : ebytes + nb);
      const int q0 = static_cast<int>(ebytes + (e0 >> 5)), q1 = static_cast<int>(ebytes + (e1 >> 5));
#pragma unroll
      for (int k = K0; k < K; ++k) {
        auto rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<char*>(a.src[k] + t * kFullTile), 0,
                                                    static_cast<int>(ebytes + nb), kRsrcFlags);
        if ((a.coherent >> k) & 1u)
          load_desc<FP8, SPLIT, kSystemCoherent>(rs, r0, r1, q0, q1, w0[k], w1[k], s0[k], s1[k]);
        else
          load_desc<FP8, SPLIT, kNonTemporal>(rs, r0, r1, q0, q1, w0[k], w1[k], s0[k], s1[k]);
      }
    }
    // 16 accumulators: operand 0 begins the chains, the others add in order.
    float acc0[8], acc1[8];
    if constexpr (OWN) {
      widen_own(h0, acc0);
      widen_own(h1, acc1);
    } else {
      widen8<F>(w0[0], scale_operand(s0[0]), acc0);
      widen8<F>(w1[0], scale_operand(s1[0]), acc1);
    }
#pragma unroll
    for (int k = 1; k < K; ++k) {
      float x0[8], x1[8];
      widen8<F>(w0[k], scale_operand(s0[k]), x0);
      widen8<F>(w1[k], scale_operand(s1[k]), x1);
#pragma unroll
      for (int j = 0; j < 8; ++j) acc0[j] = acc0[j] + x0[j], acc1[j] = acc1[j] + x1[j];
    }
    u32x4 o0, o1;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      o0[j] = reduce_pack_bf16(acc0[2 * j], acc0[2 * j + 1]);
      o1[j] = reduce_pack_bf16(acc1[2 * j], acc1[2 * j + 1]);
    }
    char* pd = a.dst + t * kWireTilePayload;
    if (in0) __builtin_nontemporal_store(o0, reinterpret_cast<u32x4*>(pd + 2 * e0));
    if (in1) __builtin_nontemporal_store(o1, reinterpret_cast<u32x4*>(pd + 2 * e1));
  }
}

// mxfp6: a lane owns a block (wire6_lane.hpp has the geometry and the store
// paths).  The K x (three 8 B code loads + one scale byte load) of a block are
// issued before the first conversion; v_cvt_scalef32_pk32_f32_fp6 widens an
// operand's 32 codes at once, 32 plain v_add_f32 per further operand in
// operand order, 16 v_cvt_pk_bf16_f32.  Registers at K = 8: 48 of codes, 8
// scale bytes, 32 accumulators and 32 of the operand being widened.
// OWN: source 0 is the own shard in bf16, the lane's block 64 B of it.  Its
// four 16 B loads are issued first (load_block: coalesced over the wave under
// SPLIT), then the K - 1 images' loads; the wave then waits for the own data
// alone, turns it into rows through its LDS slot (load_block_rows: the slot
// the store stage uses at the end of the tile) and widens it with shifts and
// masks into the 32 accumulators while the images are still in flight.
// Registers: left to itself the K = 8 split OWN instantiation takes 130 VGPRs,
// two above the 128 that still fit 4 waves per SIMD (the all-image one takes
// 127).  OWN therefore asks for those 4 waves, and the compiler schedules it
// into 128 without a spill (docs/DESIGN.md); the all-image instantiations keep
// the default bound (at least one wave) and their code.
template <int K, bool SPLIT, bool OWN>
__global__ __launch_bounds__(wire6::kLanes) __attribute__((amdgpu_waves_per_eu(OWN ? 4 : 1))) void wire_reduce6_kernel(
    const WireReduceArgs a) {
  using wire6::kF, wire6::kEB, wire6::kFullTile, wire6::kLanes, wire6::kTilesPerGroup, wire6::kSlotBytes, wire6::kTileLanes;
  using wire6::u32x6, wire6::f32x32, wire6::load_codes, wire6::store_block;
  __shared__ __attribute__((aligned(16))) char slots[SPLIT ? (kLanes / 64) * kSlotBytes : 16];
  // The wave index as a scalar: the tile, its descriptors and the loop are uniform per wave.
  const uint32_t lane = threadIdx.x & 63u, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const uint32_t wave_block = 64u * (wave % (kTileLanes / 64u));  // 0 or 64
  const uint32_t blk = wave_block + lane;                         // the lane's block of its tile
  char* slot = slots + (SPLIT ? wave * kSlotBytes : 0);

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
    u32x4 v[4];
#pragma unroll
    for (int j = 0; j < 16; ++j) v[j / 4][j % 4] = reduce_pack_bf16(acc[2 * j], acc[2 * j + 1]);
    store_block<SPLIT>(v, a.dst + t * kWireTilePayload, nb, wave_block, lane, false, slot);
  }
}

// ------------------------------------------------------------------ verify ----

struct SeedArgs {
  uint64_t seed[kMaxWireReduceSrcs];
  int n;
  bool own_bf16;  // operand 0 is the raw stream, not its image
};

struct Partial {
  unsigned long long mism, sum, first;
};

// verify_unpacked_kernel's geometry: one 16 B vector per lane, 4 lanes per block.
// RT: the expected word is the sum's round trip under its block's scale byte (--reduce-out both).
template <WireFormat F, bool RT>
__global__ __launch_bounds__(kBlock) void verify_wire_reduced_kernel(const uint4* __restrict__ p, uint64_t nvec,
                                                                     const SeedArgs s, VerifyAccum* __restrict__ out) {
  Partial acc{0, 0, ~0ull};
  for (uint64_t base = static_cast<uint64_t>(blockIdx.x) * kBlock; base < nvec; base += static_cast<uint64_t>(gridDim.x) * kBlock) {
    const uint64_t i = base + threadIdx.x;
    const bool in = i < nvec;  // nvec is a multiple of 4: a block's lanes are all in or all out
    const u32x4 v = in ? __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(p) + i) : u32x4{0, 0, 0, 0};
    ReduceAcc sum[4] = {};
    for (int k = 0; k < s.n; ++k) {
      const uint32_t key = prng_key(s.seed[k], base * 4);  // block-uniform: scalar ALU
      uint32_t w[4], amax = 0;
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        w[c] = wire_operand_word(prng_word_k(key, static_cast<uint32_t>(i * 4 + c)), i * 4 + c);
        amax = max(amax, max(w[c] & 0x7FFFu, (w[c] >> 16) & 0x7FFFu));
      }
      amax = max(amax, static_cast<uint32_t>(__shfl_xor(static_cast<int>(amax), 1, 64)));
      amax = max(amax, static_cast<uint32_t>(__shfl_xor(static_cast<int>(amax), 2, 64)));
      const uint32_t sb = wire_scale_byte(amax, F);
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const uint32_t x = k == 0 && s.own_bf16 ? w[c] : wire_roundtrip_word(w[c], sb, F);
        if (k == 0) sum[c] = reduce_begin(x, ReduceType::Bf16);
        else reduce_add(sum[c], x, ReduceType::Bf16);
      }
    }
    uint32_t want[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) want[c] = reduce_finish(sum[c], ReduceType::Bf16);
    if constexpr (RT) {  // every lane takes part in the shuffles
      uint32_t amax = 0;
#pragma unroll
      for (int c = 0; c < 4; ++c) amax = max(amax, wire_word_amax(want[c]));
      amax = max(amax, static_cast<uint32_t>(__shfl_xor(static_cast<int>(amax), 1, 64)));
      amax = max(amax, static_cast<uint32_t>(__shfl_xor(static_cast<int>(amax), 2, 64)));
      const uint32_t sb = wire_scale_byte(amax, F);
#pragma unroll
      for (int c = 0; c < 4; ++c) want[c] = wire_roundtrip_word(want[c], sb, F);
    }
    if (in) {
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        acc.sum += v[c];
        if (v[c] != want[c]) {
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

// ------------------------------------------------------------ own-shard fill ----

// bf16 of operand stream `seed` (wire_operand_word), what fill_packed_kernel
// quantises: a 16 B vector per lane, the fill kernels' grid-stride geometry.
__global__ __launch_bounds__(kBlock) void fill_wire_operand_kernel(uint4* __restrict__ p, uint64_t nvec, uint64_t seed) {
  for (uint64_t base = static_cast<uint64_t>(blockIdx.x) * kBlock; base < nvec; base += static_cast<uint64_t>(gridDim.x) * kBlock) {
    const uint32_t key = prng_key(seed, base * 4);  // block-uniform: scalar ALU
    const uint64_t i = base + threadIdx.x;
    if (i < nvec) {
      uint32_t w[4];
#pragma unroll
      for (int c = 0; c < 4; ++c) w[c] = wire_operand_word(prng_word_k(key, static_cast<uint32_t>(i * 4 + c)), i * 4 + c);
      p[i] = make_uint4(w[0], w[1], w[2], w[3]);
    }
  }
}

// ------------------------------------------------------------------ launch ----

void check_format(WireFormat f, size_t n, const char* who) {
  P2P_CHECK(wire_format_valid(f), std::string(who) + ": the format is " + kWireFormatList);
  P2P_CHECK(n % kWireBlockBytes == 0, std::string(who) + ": the payload must be a multiple of 64 bytes (blocks of 32 bf16)");
}

template <WireFormat F, bool SPLIT, bool OWN, int K = kMaxWireReduceSrcs>
void launch_wire_reduce_k(int nsrc, uint32_t grid, const WireReduceArgs& a, hipStream_t stream) {
  if constexpr (K < 1) {
    P2P_FATAL("wire_reduce: an op needs 1..8 sources");
  } else {
    if (nsrc != K)
      launch_wire_reduce_k<F, SPLIT, OWN, K - 1>(nsrc, grid, a, stream);
    else if constexpr (F == WireFormat::Mxfp6)
      wire_reduce6_kernel<K, SPLIT, OWN><<<(grid + wire6::kTilesPerGroup - 1) / wire6::kTilesPerGroup, wire6::kLanes, 0, stream>>>(a);
    else
      wire_reduce_kernel<F, K, SPLIT, OWN><<<grid, kBlock, 0, stream>>>(a);
  }
}
template <WireFormat F>
void launch_wire_reduce_f(bool split, bool own, int nsrc, uint32_t grid, const WireReduceArgs& a, hipStream_t stream) {
  if (own) {
    if (split) launch_wire_reduce_k<F, true, true>(nsrc, grid, a, stream);
    else launch_wire_reduce_k<F, false, true>(nsrc, grid, a, stream);
  } else {
    if (split) launch_wire_reduce_k<F, true, false>(nsrc, grid, a, stream);
    else launch_wire_reduce_k<F, false, false>(nsrc, grid, a, stream);
  }
}

}  // namespace

void launch_wire_reduce(const WireReduceOp& op, WireFormat fmt, hipStream_t stream, int max_blocks, WireLanes lanes) {
  check_format(fmt, op.payload_bytes, "wire_reduce");
  P2P_CHECK(op.nsrc >= 1 && op.nsrc <= kMaxWireReduceSrcs, "wire_reduce: an op needs 1..8 sources");
  P2P_CHECK(!op.dst_bf16, "wire_reduce: dst_bf16 belongs to wire_reduce_packed (the bf16 sum is dst here)");
  P2P_CHECK(!op.own_bf16 || !(op.coherent_mask & 1u), "wire_reduce: a bf16 own shard (source 0) is local memory, not a peer's buffer");
  if (!op.payload_bytes) return;
  P2P_CHECK(op.dst && reinterpret_cast<uintptr_t>(op.dst) % 16 == 0, "wire_reduce: 16-byte aligned buffers required");
  WireReduceArgs a{};
  for (int k = 0; k < op.nsrc; ++k) {
    P2P_CHECK(op.src[k] && reinterpret_cast<uintptr_t>(op.src[k]) % 16 == 0, "wire_reduce: 16-byte aligned buffers required");
    a.src[k] = static_cast<const char*>(op.src[k]);
  }
  a.dst = static_cast<char*>(op.dst);
  a.ntiles = (op.payload_bytes + kWireTilePayload - 1) / kWireTilePayload;
  const size_t rest = op.payload_bytes % kWireTilePayload;
  a.last_blocks = static_cast<uint32_t>(rest ? rest / kWireBlockBytes : kWireTileBlocks);
  a.coherent = op.coherent_mask;
  const uint64_t cap = max_blocks > 0 ? static_cast<uint64_t>(max_blocks) : kMaxGrid;
  const uint32_t grid = static_cast<uint32_t>(std::min(a.ntiles, cap));
  // Auto: split was measured faster, or level, for every format at every fan-in (docs/DESIGN.md).
  const bool split = lanes == WireLanes::Auto ? true : lanes == WireLanes::Split;
  if (fmt == WireFormat::Mxfp6) launch_wire_reduce_f<WireFormat::Mxfp6>(split, op.own_bf16, op.nsrc, grid, a, stream);
  else if (fmt == WireFormat::Mxfp8) launch_wire_reduce_f<WireFormat::Mxfp8>(split, op.own_bf16, op.nsrc, grid, a, stream);
  else launch_wire_reduce_f<WireFormat::Mxfp4>(split, op.own_bf16, op.nsrc, grid, a, stream);
  HIPCHECK(hipGetLastError());
}

void launch_fill_wire_operand(void* p, size_t payload_bytes, uint64_t seed, hipStream_t stream) {
  P2P_CHECK(payload_bytes % kWireBlockBytes == 0, "fill_wire_operand: the payload must be a multiple of 64 bytes (blocks of 32 bf16)");
  if (!payload_bytes) return;
  P2P_CHECK(reinterpret_cast<uintptr_t>(p) % 16 == 0, "fill_wire_operand: buffer must be 16-byte aligned");
  const uint64_t nvec = payload_bytes / 16;
  const unsigned grid = static_cast<unsigned>(std::min((nvec + kBlock - 1) / kBlock, kMaxGrid));
  fill_wire_operand_kernel<<<grid, kBlock, 0, stream>>>(static_cast<uint4*>(p), nvec, seed);
  HIPCHECK(hipGetLastError());
}

void launch_verify_wire_reduced(const void* p, size_t payload_bytes, const uint64_t* seeds, int nseeds, WireFormat fmt,
                                VerifyAccum* acc, hipStream_t stream, bool own_bf16, bool roundtrip) {
  check_format(fmt, payload_bytes, "verify_wire_reduced");
  P2P_CHECK(nseeds >= 1 && nseeds <= kMaxWireReduceSrcs, "verify_wire_reduced: 1..8 operand seeds");
  if (payload_bytes) {
    P2P_CHECK(reinterpret_cast<uintptr_t>(p) % 16 == 0, "verify_wire_reduced: buffer must be 16-byte aligned");
    SeedArgs s{};
    s.n = nseeds;
    s.own_bf16 = own_bf16;
    for (int k = 0; k < nseeds; ++k) s.seed[k] = seeds[k];
    const uint64_t nvec = payload_bytes / 16;
    const uint64_t cap = static_cast<uint64_t>(cu_count()) * kVerifyPerCu;
    const unsigned grid = static_cast<unsigned>(std::max<uint64_t>(1, std::min((nvec + kBlock - 1) / kBlock, cap)));
    const auto* vp = static_cast<const uint4*>(p);
    auto launch = [&](auto kernel) { kernel<<<grid, kBlock, 0, stream>>>(vp, nvec, s, acc); };
    if (fmt == WireFormat::Mxfp8)
      roundtrip ? launch(verify_wire_reduced_kernel<WireFormat::Mxfp8, true>) : launch(verify_wire_reduced_kernel<WireFormat::Mxfp8, false>);
    else if (fmt == WireFormat::Mxfp6)
      roundtrip ? launch(verify_wire_reduced_kernel<WireFormat::Mxfp6, true>) : launch(verify_wire_reduced_kernel<WireFormat::Mxfp6, false>);
    else
      roundtrip ? launch(verify_wire_reduced_kernel<WireFormat::Mxfp4, true>) : launch(verify_wire_reduced_kernel<WireFormat::Mxfp4, false>);
    HIPCHECK(hipGetLastError());
  }
  // The finalize of launch_verify (zero bytes: nothing else runs): shards -> acc[0].
  launch_verify(nullptr, 0, 0, acc, VerifyImpl::Auto, false, stream);
}

}  // namespace dev
}  // namespace p2p
