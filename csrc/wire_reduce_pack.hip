// gfx950 kernels of --reduce-out wire: the middle hop of a quantised ring or
// combine.  K MXFP8 / MXFP4 wire images come in, their sum leaves as a wire
// image of the same format, in one launch; the bf16 sum never reaches memory.
// kernels.hpp has the contract, wire_reduce_op.hpp the arithmetic (the image
// is wire_pack_block of the bf16 sum, so this kernel equals launch_wire_reduce
// into scratch followed by launch_pack bit for bit), wire_op.hpp the format.
// Design:
//   * Load side as wire_reduce.hip: a 256-thread workgroup per 8 KiB-payload
//     tile, 16 elements per lane, fan-in K and format as template parameters,
//     the K element loads and K scale-byte loads of a tile issued before the
//     first conversion; all images local: straight non-temporal loads,
//     otherwise one range-checked descriptor per source and tile, system
//     scope for a peer's image.  16 f32 accumulators, widened with
//     v_cvt_scalef32_pk_f32_fp8 / _fp4, plain f32 adds in operand order.
//   * Epilogue, all in registers: v_cvt_pk_bf16_f32 rounds the sums to 8 words
//     of bf16; the amax of a unit is an integer max over its 8 magnitudes.  A
//     block's amax is completed across its lanes by xor shuffles (DPP
//     quad_perm on the v_max: a block's lanes share a quad), which never leave
//     the block.  SPLIT (units of 8 elements at 8L and 8L + 2048) has 4 lanes
//     per block and two blocks per lane, so xor 1 and xor 2 for each of the
//     two units; contiguous (16 elements at 16L) has 2 lanes per block, so the
//     two units' maxima are merged and one xor 1 finishes.
//     wire_scale_byte, then v_cvt_scalef32_pk_fp8_bf16 / _fp4_bf16 narrow the
//     bf16 words under byte << 23.
//   * Stores.  The image is 0.52x / 0.27x of the bf16 the other kernel writes,
//     so the lanes' stores are smaller: contiguous ends in one 16 B (mxfp8) or
//     8 B (mxfp4) store per lane, consecutive lanes adjacent; split in two
//     stores of half that size, each coalesced over the wave.  Vector stores
//     only, non-temporal: the next reader is another GPU or a later launch.
//   * Scale bytes: the first lane of a block writes the byte (0 for a block
//     past a ragged tile's end: that is the padding) into a 128 B LDS stage,
//     and lanes 0..7 store the stage as 16 B vectors behind the elements.  The
//     stage is double-buffered by tile parity, so a tile costs one barrier:
//     before any wave writes the stage of tile i + 2 it has passed the
//     barrier of tile i + 1, which wave 0 reaches only after its reads of
//     tile i's stage have returned.
//   * Lanes past a ragged tile's end take part in every shuffle and barrier
//     and store nothing; a block's lanes are all in or all out.
//   * BOTH (WireReduceOp::dst_bf16, --reduce-out both): the turn-around hop of
//     a two-shot all-reduce keeps what its peers will reconstruct from the
//     image.  A further template parameter, so the image-only kernels are
//     what they were: after narrow8 the lane widens its own codes back with
//     v_cvt_scalef32_pk_bf16_fp8 / _fp4 under the same byte << 23 (the unpack's
//     conversion) and stores its 16 bf16 as two 16 B non-temporal stores
//     (split: 4 KiB apart, both coalesced; contiguous: the lane's 32 B).
//   * mxfp6 has a kernel of its own, a lane per block and no barrier:
//     wire_reduce_pack6.hip.  Its check is here with the others'.
//   * No packed f32 instructions in this object (Makefile).
#include <hip/hip_runtime.h>

#include <algorithm>

#include "common.hpp"
#include "hip_check.hpp"
#include "kernels.hpp"
#include "wire_own_lane.hpp"

namespace p2p {
namespace dev {

namespace {

typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef short i16x2 __attribute__((ext_vector_type(2)));

constexpr int kBlock = 256;
constexpr int kWaves = kBlock / 64;
constexpr uint64_t kMaxGrid = 1ull << 20;  // tiles per grid pass (8 GiB of payload)
constexpr int kVerifyPerCu = 16;           // the check: workgroups per CU, grid-stride beyond
// Cache-policy bits and descriptor word of the cross-GPU accesses (kernels.hip).
constexpr int kSystemCoherent = 1 | 16;  // sc0 sc1
constexpr int kNonTemporal = 2;           // nt
constexpr int kRsrcFlags = 0x00020000;

// By value in the kernarg segment.
struct ReducePackArgs {
  const char* src[kMaxWireReduceSrcs];
  char* dst;
  uint64_t ntiles;
  uint32_t last_blocks;  // blocks of the last tile, 1..128
  uint32_t coherent;     // WireReduceOp::coherent_mask
  char* dst_bf16;        // BOTH: the round trip of the image, payload bytes of bf16
};

__device__ __forceinline__ float scale_operand(uint32_t sb) { return __builtin_bit_cast(float, sb << 23); }

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

// 8 f32 sums -> 4 words of bf16 (one rounding each) and the largest magnitude among them.
__device__ __forceinline__ uint32_t round8(const float (&acc)[8], uint32_t (&h)[4]) {
  uint32_t amax = 0;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    h[j] = reduce_pack_bf16(acc[2 * j], acc[2 * j + 1]);
    amax = max(amax, wire_word_amax(h[j]));
  }
  return amax;
}

// 4 words of bf16 under scale byte sb -> their codes: c[0] and c[1] (mxfp8) or c[0] (mxfp4).
template <WireFormat F>
__device__ __forceinline__ void narrow8(const uint32_t (&h)[4], uint32_t sb, uint32_t* c) {
  const float scale = scale_operand(sb);
  if constexpr (F == WireFormat::Mxfp8) {
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      i16x2 o = {0, 0};
      o = __builtin_amdgcn_cvt_scalef32_pk_fp8_bf16(o, __builtin_bit_cast(bf16x2, h[2 * j]), scale, false);
      o = __builtin_amdgcn_cvt_scalef32_pk_fp8_bf16(o, __builtin_bit_cast(bf16x2, h[2 * j + 1]), scale, true);
      c[j] = __builtin_bit_cast(uint32_t, o);
    }
  } else {
    uint32_t o = 0;
    o = __builtin_amdgcn_cvt_scalef32_pk_fp4_bf16(o, __builtin_bit_cast(bf16x2, h[0]), scale, 0);
    o = __builtin_amdgcn_cvt_scalef32_pk_fp4_bf16(o, __builtin_bit_cast(bf16x2, h[1]), scale, 1);
    o = __builtin_amdgcn_cvt_scalef32_pk_fp4_bf16(o, __builtin_bit_cast(bf16x2, h[2]), scale, 2);
    o = __builtin_amdgcn_cvt_scalef32_pk_fp4_bf16(o, __builtin_bit_cast(bf16x2, h[3]), scale, 3);
    c[0] = o;
  }
}

// BOTH: the codes narrow8 gave, widened again under the same scale byte: 8 bf16.
template <WireFormat F>
__device__ __forceinline__ u32x4 widen_back8(const uint32_t* c, uint32_t sb) {
  const float scale = scale_operand(sb);
  bf16x2 r[4];
  if constexpr (F == WireFormat::Mxfp8) {
    r[0] = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(c[0], scale, false);
    r[1] = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(c[0], scale, true);
    r[2] = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(c[1], scale, false);
    r[3] = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(c[1], scale, true);
  } else {
    r[0] = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(c[0], scale, 0);
    r[1] = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(c[0], scale, 1);
    r[2] = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(c[0], scale, 2);
    r[3] = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(c[0], scale, 3);
  }
  return u32x4{__builtin_bit_cast(uint32_t, r[0]), __builtin_bit_cast(uint32_t, r[1]), __builtin_bit_cast(uint32_t, r[2]),
               __builtin_bit_cast(uint32_t, r[3])};
}

// max with the lane at (lane ^ MASK), MASK 1 or 2: both stay inside a quad, so
// a DPP quad_perm ([1,0,3,2] / [2,3,0,1]) on the v_max does it without the
// LDS crossbar a general shuffle goes through.  Every lane is active here.
template <int MASK>
__device__ __forceinline__ uint32_t xor_max(uint32_t v) {
  static_assert(MASK == 1 || MASK == 2, "inside a quad");
  constexpr int kQuadPerm = MASK == 1 ? 0xB1 : 0x4E;
  return max(v, static_cast<uint32_t>(__builtin_amdgcn_update_dpp(0, static_cast<int>(v), kQuadPerm, 0xF, 0xF, false)));
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

// OWN: source 0 is the receiver's own shard in bf16 (local memory), not an image.
// BOTH: dst_bf16 receives the image's round trip beside it.
template <WireFormat F, int K, bool SPLIT, bool OWN, bool BOTH>
__global__ __launch_bounds__(kBlock) void wire_reduce_pack_kernel(const ReducePackArgs a) {
  constexpr uint32_t EB = wire_block_elem_bytes(F);
  constexpr uint32_t kFullTile = wire_tile_bytes(kWireTileBlocks, F);
  constexpr bool FP8 = F == WireFormat::Mxfp8;
  constexpr int EW = FP8 ? 2 : 1;  // 32-bit words of codes per unit of 8 elements
  __shared__ __attribute__((aligned(16))) uint8_t stage[2][kWireTileBlocks];
  const uint32_t L = threadIdx.x;
  // The lane's two units of 8 elements: element offsets inside the tile.
  const uint32_t e0 = SPLIT ? 8u * L : 16u * L;
  const uint32_t e1 = SPLIT ? 8u * L + 2048u : 16u * L + 8u;
  const uint32_t c0 = FP8 ? e0 : e0 / 2, c1 = FP8 ? e1 : e1 / 2;  // byte offsets of their codes, in and out
  const uint32_t blk0 = e0 >> 5, blk1 = e1 >> 5;                   // their blocks (contiguous: the same one)
  const bool first_of_block = SPLIT ? (L & 3u) == 0 : (L & 1u) == 0;
  uint32_t parity = 0;

  for (uint64_t t = blockIdx.x; t < a.ntiles; t += gridDim.x, parity ^= 1u) {
    // Block-uniform: the tile's blocks and the range of its descriptors.
    const uint32_t nb = t + 1 == a.ntiles ? a.last_blocks : kWireTileBlocks;
    const uint32_t ebytes = nb * EB;
    const bool in0 = blk0 < nb, in1 = blk1 < nb;
    // All K element loads and all K scale loads before the first conversion.
    uint32_t w0[K][EW], w1[K][EW], s0[K], s1[K];
    constexpr int K0 = OWN ? 1 : 0;  // the first source that is an image
    u32x4 own0, own1;                // OWN: the own shard's 16 elements, issued first
    if constexpr (OWN) load_own(a.src[0] + t * kWireTilePayload, e0, e1, in0, in1, own0, own1);
    if ((a.coherent & ((1u << K) - 1u)) == 0) {
      // Every image is local: straight-line non-temporal loads; a lane past
      // the tile's end re-reads the tile's first unit and stores nothing.
      const uint32_t l0 = in0 ? c0 : 0, l1 = in1 ? c1 : 0;
      const uint32_t b0 = in0 ? blk0 : 0, b1 = in1 ? blk1 : 0;
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
      // scale bytes: a lane past the tile's end aims at the descriptor's end
      // and loads 0.  The block-uniform branch picks the cache policy only.
      const int r0 = static_cast<int>(in0 ? c0 : ebytes + nb), r1 = static_cast<int>(in1 ? c1 : ebytes + nb);
      const int q0 = static_cast<int>(ebytes + blk0), q1 = static_cast<int>(ebytes + blk1);
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
      widen_own(own0, acc0);
      widen_own(own1, acc1);
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
    // One rounding to bf16, then the block's amax of the rounded values.
    uint32_t h0[4], h1[4];
    uint32_t amax0 = round8(acc0, h0), amax1 = round8(acc1, h1);
    if constexpr (SPLIT) {
      amax0 = xor_max<2>(xor_max<1>(amax0));
      amax1 = xor_max<2>(xor_max<1>(amax1));
    } else {
      amax0 = amax1 = xor_max<1>(max(amax0, amax1));
    }
    const uint32_t sb0 = wire_scale_byte(amax0, F), sb1 = SPLIT ? wire_scale_byte(amax1, F) : sb0;
    uint32_t n0[EW], n1[EW];
    narrow8<F>(h0, sb0, n0);
    narrow8<F>(h1, sb1, n1);
    char* wt = a.dst + t * kFullTile;
    if constexpr (!SPLIT && FP8) {
      if (in0) __builtin_nontemporal_store(u32x4{n0[0], n0[1], n1[0], n1[1]}, reinterpret_cast<u32x4*>(wt + c0));
    } else if constexpr (SPLIT && FP8) {
      if (in0) __builtin_nontemporal_store(u32x2{n0[0], n0[1]}, reinterpret_cast<u32x2*>(wt + c0));
      if (in1) __builtin_nontemporal_store(u32x2{n1[0], n1[1]}, reinterpret_cast<u32x2*>(wt + c1));
    } else if constexpr (!SPLIT) {
      if (in0) __builtin_nontemporal_store(u32x2{n0[0], n1[0]}, reinterpret_cast<u32x2*>(wt + c0));
    } else {
      if (in0) __builtin_nontemporal_store(n0[0], reinterpret_cast<uint32_t*>(wt + c0));
      if (in1) __builtin_nontemporal_store(n1[0], reinterpret_cast<uint32_t*>(wt + c1));
    }
    if constexpr (BOTH) {
      char* pd = a.dst_bf16 + t * kWireTilePayload;
      if (in0) __builtin_nontemporal_store(widen_back8<F>(n0, sb0), reinterpret_cast<u32x4*>(pd + 2 * e0));
      if (in1) __builtin_nontemporal_store(widen_back8<F>(n1, sb1), reinterpret_cast<u32x4*>(pd + 2 * e1));
    }
    // The tile's scale bytes and the zero padding behind them, through this
    // tile's half of the LDS stage (blk0, blk1 < 128 for every lane).
    if (first_of_block) {
      stage[parity][blk0] = in0 ? static_cast<uint8_t>(sb0) : 0;
      if constexpr (SPLIT) stage[parity][blk1] = in1 ? static_cast<uint8_t>(sb1) : 0;
    }
    __syncthreads();
    if (L < 8 && 16 * L < nb)
      __builtin_nontemporal_store(*reinterpret_cast<const u32x4*>(&stage[parity][16 * L]), reinterpret_cast<u32x4*>(wt + ebytes + 16 * L));
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

// verify_wire_reduced_kernel's geometry: lane i owns payload vector i (8
// elements), 4 lanes a block; what it reads is the image: its 8 codes, and the
// block's first lane the scale byte.
template <WireFormat F>
__global__ __launch_bounds__(kBlock) void verify_wire_reduced_packed_kernel(const char* __restrict__ image, uint64_t nvec,
                                                                            uint64_t ntiles, uint32_t last_blocks,
                                                                            const SeedArgs s, VerifyAccum* __restrict__ out) {
  constexpr uint32_t EB = wire_block_elem_bytes(F);
  constexpr uint32_t kFullTile = wire_tile_bytes(kWireTileBlocks, F);
  constexpr int CW = F == WireFormat::Mxfp8 ? 2 : 1;  // words of codes per lane
  constexpr uint32_t kTileVecs = kWireTilePayload / 16;
  Partial acc{0, 0, ~0ull};
  for (uint64_t base = static_cast<uint64_t>(blockIdx.x) * kBlock; base < nvec; base += static_cast<uint64_t>(gridDim.x) * kBlock) {
    const uint64_t i = base + threadIdx.x;
    const bool in = i < nvec;  // nvec is a multiple of 4: a block's lanes are all in or all out
    ReduceAcc sum[4] = {};
    for (int k = 0; k < s.n; ++k) {
      const uint32_t key = prng_key(s.seed[k], base * 4);  // block-uniform: scalar ALU
      uint32_t w[4], amax = 0;
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        w[c] = wire_operand_word(prng_word_k(key, static_cast<uint32_t>(i * 4 + c)), i * 4 + c);
        amax = max(amax, wire_word_amax(w[c]));
      }
      amax = xor_max<2>(xor_max<1>(amax));
      const uint32_t sb = wire_scale_byte(amax, F);
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const uint32_t x = k == 0 && s.own_bf16 ? w[c] : wire_roundtrip_word(w[c], sb, F);
        if (k == 0) sum[c] = reduce_begin(x, ReduceType::Bf16);
        else reduce_add(sum[c], x, ReduceType::Bf16);
      }
    }
    uint32_t h[4], amax = 0;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      h[c] = reduce_finish(sum[c], ReduceType::Bf16);
      amax = max(amax, wire_word_amax(h[c]));
    }
    amax = xor_max<2>(xor_max<1>(amax));
    const uint32_t sb = wire_scale_byte(amax, F);
    if (in) {
      const uint64_t t = i / kTileVecs;
      const uint32_t iv = static_cast<uint32_t>(i % kTileVecs);
      const uint32_t nb = t + 1 == ntiles ? last_blocks : kWireTileBlocks;
      const uint64_t at = t * kFullTile + iv * (EB / 4);
      if constexpr (F == WireFormat::Mxfp6) {
        // The lane's 8 codes are 6 bytes at a 6-byte stride, 2 B aligned: one unit of the count.
        const auto* q = reinterpret_cast<const uint16_t*>(image + at);
        const unsigned long long got = q[0] | static_cast<unsigned long long>(q[1]) << 16 | static_cast<unsigned long long>(q[2]) << 32;
        acc.sum += got;
        if (got != wire_code_bits6(h, sb)) {
          acc.mism += 1;
          acc.first = min(acc.first, static_cast<unsigned long long>(at));
        }
      } else {
#pragma unroll
        for (int c = 0; c < CW; ++c) {
          const uint32_t got = *reinterpret_cast<const uint32_t*>(image + at + 4 * c);
          acc.sum += got;
          if (got != wire_code_word(h + (4 / CW) * c, sb, F)) {
            acc.mism += 1;
            acc.first = min(acc.first, static_cast<unsigned long long>(at + 4 * c));
          }
        }
      }
      if ((iv & 3u) == 0) {
        const uint64_t sat = t * kFullTile + wire_tile_scale_offset(nb, F) + (iv >> 2);
        const uint32_t got = static_cast<uint8_t>(image[sat]);
        acc.sum += got;
        if (got != sb) {
          acc.mism += 1;
          acc.first = min(acc.first, static_cast<unsigned long long>(sat));
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

template <WireFormat F, bool SPLIT, bool OWN, bool BOTH, int K = kMaxWireReduceSrcs>
void launch_k(int nsrc, uint32_t grid, const ReducePackArgs& a, hipStream_t stream) {
  if constexpr (K < 1) {
    P2P_FATAL("wire_reduce_packed: an op needs 1..8 sources");
  } else {
    if (nsrc == K)
      wire_reduce_pack_kernel<F, K, SPLIT, OWN, BOTH><<<grid, kBlock, 0, stream>>>(a);
    else
      launch_k<F, SPLIT, OWN, BOTH, K - 1>(nsrc, grid, a, stream);
  }
}
template <WireFormat F, bool BOTH>
void launch_o(bool split, bool own, int nsrc, uint32_t grid, const ReducePackArgs& a, hipStream_t stream) {
  if (own) {
    if (split) launch_k<F, true, true, BOTH>(nsrc, grid, a, stream);
    else launch_k<F, false, true, BOTH>(nsrc, grid, a, stream);
  } else {
    if (split) launch_k<F, true, false, BOTH>(nsrc, grid, a, stream);
    else launch_k<F, false, false, BOTH>(nsrc, grid, a, stream);
  }
}
template <WireFormat F>
void launch_f(bool split, bool own, bool both, int nsrc, uint32_t grid, const ReducePackArgs& a, hipStream_t stream) {
  if (both) launch_o<F, true>(split, own, nsrc, grid, a, stream);
  else launch_o<F, false>(split, own, nsrc, grid, a, stream);
}

}  // namespace

void launch_wire_reduce_packed(const WireReduceOp& op, WireFormat fmt, hipStream_t stream, int max_blocks, WireLanes lanes) {
  check_format(fmt, op.payload_bytes, "wire_reduce_packed");
  P2P_CHECK(op.nsrc >= 1 && op.nsrc <= kMaxWireReduceSrcs, "wire_reduce_packed: an op needs 1..8 sources");
  P2P_CHECK(!op.own_bf16 || !(op.coherent_mask & 1u), "wire_reduce_packed: a bf16 own shard (source 0) is local memory, not a peer's buffer");
  if (!op.payload_bytes) return;
  P2P_CHECK(op.dst && reinterpret_cast<uintptr_t>(op.dst) % 16 == 0, "wire_reduce_packed: 16-byte aligned buffers required");
  P2P_CHECK(reinterpret_cast<uintptr_t>(op.dst_bf16) % 16 == 0, "wire_reduce_packed: 16-byte aligned buffers required");
  for (int k = 0; k < op.nsrc; ++k)
    P2P_CHECK(op.src[k] && reinterpret_cast<uintptr_t>(op.src[k]) % 16 == 0, "wire_reduce_packed: 16-byte aligned buffers required");
  if (fmt == WireFormat::Mxfp6) {  // a lane per block, no barrier: wire_reduce_pack6.hip
    launch_wire_reduce_packed6(op, stream, max_blocks, lanes);
    return;
  }
  ReducePackArgs a{};
  for (int k = 0; k < op.nsrc; ++k) a.src[k] = static_cast<const char*>(op.src[k]);
  a.dst = static_cast<char*>(op.dst);
  a.dst_bf16 = static_cast<char*>(op.dst_bf16);
  a.ntiles = tiles_of(op.payload_bytes);
  a.last_blocks = last_blocks_of(op.payload_bytes);
  a.coherent = op.coherent_mask;
  const uint64_t cap = max_blocks > 0 ? static_cast<uint64_t>(max_blocks) : kMaxGrid;
  const uint32_t grid = static_cast<uint32_t>(std::min(a.ntiles, cap));
  // Auto: contiguous was measured faster in every cell, by 1-8% against a spread under 1% (docs/DESIGN.md): unlike
  // wire_reduce.hip, where split's two coalesced 16 B stores win.
  // With both outputs the 8 KiB of bf16 a tile stores dominate, and split (both 16 B stores coalesced) was measured
  // 5-86% faster in every cell against a spread under 4.4% (docs/DESIGN.md): Auto follows the output.
  const bool both = op.dst_bf16 != nullptr;
  const bool split = lanes == WireLanes::Auto ? both : lanes == WireLanes::Split;
  if (fmt == WireFormat::Mxfp8) launch_f<WireFormat::Mxfp8>(split, op.own_bf16, both, op.nsrc, grid, a, stream);
  else launch_f<WireFormat::Mxfp4>(split, op.own_bf16, both, op.nsrc, grid, a, stream);
  HIPCHECK(hipGetLastError());
}

void launch_verify_wire_reduced_packed(const void* image, size_t payload_bytes, const uint64_t* seeds, int nseeds,
                                       WireFormat fmt, VerifyAccum* acc, hipStream_t stream, bool own_bf16) {
  check_format(fmt, payload_bytes, "verify_wire_reduced_packed");
  P2P_CHECK(nseeds >= 1 && nseeds <= kMaxWireReduceSrcs, "verify_wire_reduced_packed: 1..8 operand seeds");
  if (payload_bytes) {
    P2P_CHECK(reinterpret_cast<uintptr_t>(image) % 16 == 0, "verify_wire_reduced_packed: buffer must be 16-byte aligned");
    SeedArgs s{};
    s.n = nseeds;
    s.own_bf16 = own_bf16;
    for (int k = 0; k < nseeds; ++k) s.seed[k] = seeds[k];
    const uint64_t nvec = payload_bytes / 16;
    const uint64_t cap = static_cast<uint64_t>(cu_count()) * kVerifyPerCu;
    const unsigned grid = static_cast<unsigned>(std::max<uint64_t>(1, std::min((nvec + kBlock - 1) / kBlock, cap)));
    const auto* p = static_cast<const char*>(image);
    if (fmt == WireFormat::Mxfp8)
      verify_wire_reduced_packed_kernel<WireFormat::Mxfp8><<<grid, kBlock, 0, stream>>>(p, nvec, tiles_of(payload_bytes), last_blocks_of(payload_bytes), s, acc);
    else if (fmt == WireFormat::Mxfp6)
      verify_wire_reduced_packed_kernel<WireFormat::Mxfp6><<<grid, kBlock, 0, stream>>>(p, nvec, tiles_of(payload_bytes), last_blocks_of(payload_bytes), s, acc);
    else
      verify_wire_reduced_packed_kernel<WireFormat::Mxfp4><<<grid, kBlock, 0, stream>>>(p, nvec, tiles_of(payload_bytes), last_blocks_of(payload_bytes), s, acc);
    HIPCHECK(hipGetLastError());
  }
  // The finalize of launch_verify (zero bytes: nothing else runs): shards -> acc[0].
  launch_verify(nullptr, 0, 0, acc, VerifyImpl::Auto, false, stream);
}

}  // namespace dev
}  // namespace p2p
